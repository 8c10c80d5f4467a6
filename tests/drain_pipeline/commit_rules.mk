# TEST-ONLY: what a garbling pass may combine — DrainSink::commit / refusal and commit_slice_conflict of csrc/engine/drain_pipeline.hpp,
# alone (make -f commit_rules.mk), against the stand-ins for the HIP calls the header names.  No HIP runtime is linked.  `asan` builds the
# same stand-alone program under the address + undefined-behaviour sanitizers, run by hand; the test suite builds the plain target.
CXX ?= g++
CXXFLAGS ?= -O1 -g -std=c++17 -Wall -Wextra -maes -msse2 -pthread
ROCM_PATH ?= /opt/rocm
SRC := ../../garbled_snark_verifier_amd/csrc
DEPS := commit_rules_test.cpp ../hip_standin/hip_standin.hpp $(SRC)/engine/drain_pipeline.hpp $(SRC)/engine/hip_owned.hpp $(SRC)/engine/host_crypto.hpp $(SRC)/engine/outboard.hpp $(SRC)/engine/mac_checkpoints.hpp
BUILD = $(CXX) $(CXXFLAGS) -D__HIP_PLATFORM_AMD__ -I$(ROCM_PATH)/include -o $@ commit_rules_test.cpp
all: commit_rules_test
commit_rules_test: $(DEPS)
	$(BUILD)
commit_rules_test_asan: $(DEPS)
	$(BUILD) -fsanitize=address,undefined -fno-sanitize-recover=undefined
asan: commit_rules_test_asan
.PHONY: all asan
