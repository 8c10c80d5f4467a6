# TEST-ONLY: GcFileSource of csrc/engine/upload_pipeline.hpp, alone (make -f gc_file_source.mk), against the stand-ins of
# tests/hip_standin/hip_standin.hpp for the HIP calls the header's other classes make.  No HIP runtime is linked.  `asan` builds the same
# stand-alone program under the address + undefined-behaviour sanitizers, run by hand (its output is kept in profiles/b3_receiver/); the
# test suite builds the plain target.
CXX ?= g++
CXXFLAGS ?= -O1 -g -std=c++17 -Wall -Wextra -maes -msse2 -pthread
ROCM_PATH ?= /opt/rocm
SRC := ../../garbled_snark_verifier_amd/csrc
DEPS := gc_file_source_test.cpp ../hip_standin/hip_standin.hpp $(SRC)/engine/upload_pipeline.hpp $(SRC)/engine/hip_owned.hpp $(SRC)/engine/host_crypto.hpp
BUILD = $(CXX) $(CXXFLAGS) -D__HIP_PLATFORM_AMD__ -I$(ROCM_PATH)/include -o $@ gc_file_source_test.cpp
all: gc_file_source_test
gc_file_source_test: $(DEPS)
	$(BUILD)
gc_file_source_test_asan: $(DEPS)
	$(BUILD) -fsanitize=address,undefined -fno-sanitize-recover=undefined
asan: gc_file_source_test_asan
.PHONY: all asan
