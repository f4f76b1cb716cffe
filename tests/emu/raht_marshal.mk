# tests/emu/raht_marshal.mk -- TEST INFRASTRUCTURE: the marshalling kernels of the device tier's RAHT slice coder
# (gather with the region offsets, clip and scatter) compiled for the CPU wavefront emulator (make -f raht_marshal.mk,
# in this directory; the flags of Makefile).
ROOT := ../..
CXX ?= g++
FLAGS := -O1 -g -std=c++17 -fPIC -Wall -Wno-unused-variable -Wno-unused-but-set-variable \
         -Wno-attributes -Wno-unknown-pragmas -Wno-unused-function -Wno-sign-compare -DGPCC_EXPERIMENTS=1 \
         -I. -I$(ROOT)/include -I$(ROOT)/mpeg-pcc-tmc13_amd/csrc
SRCS := $(ROOT)/mpeg-pcc-tmc13_amd/csrc/raht_marshal.hpp $(ROOT)/mpeg-pcc-tmc13_amd/csrc/raht_common.hpp \
        $(ROOT)/include/gpcc_attr_mi355.h emu_core.cpp hip/hip_runtime.h

libraht_marshal_emu.so: raht_marshal_emu_harness.cpp $(SRCS)
	$(CXX) $(FLAGS) -shared raht_marshal_emu_harness.cpp emu_core.cpp -o $@
