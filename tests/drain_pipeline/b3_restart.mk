# TEST-ONLY: the host half of a restart point — B3Check's position and the Blake3Host hashers of csrc/engine/outboard.hpp and
# host_crypto.hpp — saved, advanced, restored and advanced again (make -f b3_restart.mk).  Host code only: no HIP header, no HIP runtime.
# `asan` builds the same stand-alone program under the address + undefined-behaviour sanitizers, run by hand; the test suite builds the
# plain target.
CXX ?= g++
CXXFLAGS ?= -O1 -g -std=c++17 -Wall -Wextra -maes -msse2 -pthread
SRC := ../../garbled_snark_verifier_amd/csrc
DEPS := b3_restart_test.cpp $(SRC)/engine/outboard.hpp $(SRC)/engine/host_crypto.hpp
BUILD = $(CXX) $(CXXFLAGS) -o $@ b3_restart_test.cpp
all: b3_restart_test
b3_restart_test: $(DEPS)
	$(BUILD)
b3_restart_test_asan: $(DEPS)
	$(BUILD) -fsanitize=address,undefined -fno-sanitize-recover=undefined
asan: b3_restart_test_asan
.PHONY: all asan
