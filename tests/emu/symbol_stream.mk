# tests/emu/symbol_stream.mk -- TEST INFRASTRUCTURE: the entropy front end of the device tier (coefficients to
# symbols and bins, symbols to coefficients) compiled for the CPU wavefront emulator (make -f symbol_stream.mk, in
# this directory; the flags of Makefile).
ROOT := ../..
CXX ?= g++
FLAGS := -O1 -g -std=c++17 -fPIC -Wall -Wno-unused-variable -Wno-unused-but-set-variable \
         -Wno-attributes -Wno-unknown-pragmas -Wno-unused-function -Wno-sign-compare -DGPCC_EXPERIMENTS=1 \
         -I. -I$(ROOT)/include -I$(ROOT)/mpeg-pcc-tmc13_amd/csrc
SRCS := $(ROOT)/mpeg-pcc-tmc13_amd/csrc/symbol_stream.hpp $(ROOT)/mpeg-pcc-tmc13_amd/csrc/residual_bins.hpp \
        $(ROOT)/mpeg-pcc-tmc13_amd/csrc/spherical.hpp $(ROOT)/mpeg-pcc-tmc13_amd/csrc/gpcc_primitives.hpp \
        $(ROOT)/include/gpcc_attr_mi355.h emu_core.cpp hip/hip_runtime.h

libsymbol_stream_emu.so: symbol_stream_emu_harness.cpp $(SRCS)
	$(CXX) $(FLAGS) -shared symbol_stream_emu_harness.cpp emu_core.cpp -o $@
