# TEST-ONLY: B3Check and the outboard loaders of csrc/engine/outboard.hpp, alone (make -f b3_check.mk).  Host code only: no HIP header,
# no HIP runtime.  `asan` builds the same stand-alone program under the address + undefined-behaviour sanitizers, run by hand (its output
# is kept in profiles/b3_receiver/); the test suite builds the plain target.
CXX ?= g++
CXXFLAGS ?= -O1 -g -std=c++17 -Wall -Wextra -maes -msse2 -pthread
SRC := ../../garbled_snark_verifier_amd/csrc
DEPS := b3_check_test.cpp $(SRC)/engine/outboard.hpp $(SRC)/engine/host_crypto.hpp
BUILD = $(CXX) $(CXXFLAGS) -o $@ b3_check_test.cpp
all: b3_check_test
b3_check_test: $(DEPS)
	$(BUILD)
b3_check_test_asan: $(DEPS)
	$(BUILD) -fsanitize=address,undefined -fno-sanitize-recover=undefined
asan: b3_check_test_asan
.PHONY: all asan
