# tests/emu/quantize.mk -- TEST INFRASTRUCTURE: the unique-position quantiser and the source partition compiled for
# the CPU wavefront emulator (make -f quantize.mk, in this directory; the flags of Makefile, and -ffp-contract=off so
# that the float expressions keep one rounding per operation on any host).
ROOT := ../..
CXX ?= g++
FLAGS := -O1 -g -std=c++17 -fPIC -Wall -Wno-unused-variable -Wno-unused-but-set-variable \
         -Wno-attributes -Wno-unknown-pragmas -Wno-unused-function -Wno-sign-compare -DGPCC_EXPERIMENTS=1 \
         -ffp-contract=off -I. -I$(ROOT)/include -I$(ROOT)/mpeg-pcc-tmc13_amd/csrc
SRCS := $(ROOT)/mpeg-pcc-tmc13_amd/csrc/quantize_positions.hpp $(ROOT)/mpeg-pcc-tmc13_amd/csrc/morton_sort.hpp \
        $(ROOT)/mpeg-pcc-tmc13_amd/csrc/recolour_kdtree.hpp $(ROOT)/mpeg-pcc-tmc13_amd/csrc/raht_common.hpp \
        $(ROOT)/mpeg-pcc-tmc13_amd/csrc/gpcc_primitives.hpp $(ROOT)/include/gpcc_attr_mi355.h emu_core.cpp \
        hip/hip_runtime.h

libquantize_emu.so: quantize_emu_harness.cpp $(SRCS)
	$(CXX) $(FLAGS) -shared quantize_emu_harness.cpp emu_core.cpp -o $@
