# tests/emu/pred_repair.mk -- TEST INFRASTRUCTURE: the predicting encoder's passes and ordered walk
# compiled for the CPU wavefront emulator (make -f pred_repair.mk, in this directory; the flags of Makefile).
ROOT := ../..
CXX ?= g++
FLAGS := -O1 -g -std=c++17 -fPIC -Wall -Wno-unused-variable -Wno-unused-but-set-variable \
         -Wno-attributes -Wno-unknown-pragmas -Wno-unused-function -Wno-sign-compare -DGPCC_EXPERIMENTS=1 \
         -I. -I$(ROOT)/include -I$(ROOT)/mpeg-pcc-tmc13_amd/csrc
SRCS := $(wildcard $(ROOT)/mpeg-pcc-tmc13_amd/csrc/lod_*.hpp) $(ROOT)/mpeg-pcc-tmc13_amd/csrc/lift_kernels.hpp \
        $(ROOT)/mpeg-pcc-tmc13_amd/csrc/pred_kernels.hpp $(ROOT)/mpeg-pcc-tmc13_amd/csrc/pred_repair.hpp \
        $(ROOT)/mpeg-pcc-tmc13_amd/csrc/gpcc_primitives.hpp $(ROOT)/mpeg-pcc-tmc13_amd/csrc/raht_common.hpp \
        $(ROOT)/include/gpcc_attr_mi355.h emu_core.cpp hip/hip_runtime.h

libpred_repair_emu.so: pred_repair_emu_harness.cpp $(SRCS)
	$(CXX) $(FLAGS) -shared pred_repair_emu_harness.cpp emu_core.cpp -o $@
