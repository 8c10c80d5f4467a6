# TEST-ONLY: the two back ends (files, host callback) of the outboard writer of csrc/engine/drain_pipeline.hpp (OutboardWriter) against
# the stand-ins of tests/hip_standin/hip_standin.hpp (make -f outboard_sink.mk).  No HIP runtime is linked.  `asan` / `tsan` build the same
# stand-alone program under the address + undefined-behaviour / thread sanitizers, run by hand; the test suite builds the plain target.
CXX ?= g++
CXXFLAGS ?= -O1 -g -std=c++17 -Wall -Wextra -maes -msse2 -pthread
ROCM_PATH ?= /opt/rocm
SRC := ../../garbled_snark_verifier_amd/csrc
DEPS := outboard_sink_test.cpp ../hip_standin/hip_standin.hpp $(SRC)/engine/drain_pipeline.hpp $(SRC)/engine/outboard.hpp $(SRC)/engine/hip_owned.hpp $(SRC)/engine/host_crypto.hpp
BUILD = $(CXX) $(CXXFLAGS) -D__HIP_PLATFORM_AMD__ -I$(ROCM_PATH)/include -o $@ outboard_sink_test.cpp
all: outboard_sink_test
outboard_sink_test: $(DEPS)
	$(BUILD)
outboard_sink_test_tsan: $(DEPS)
	$(BUILD) -fsanitize=thread
outboard_sink_test_asan: $(DEPS)
	$(BUILD) -fsanitize=address,undefined -fno-sanitize-recover=undefined
tsan: outboard_sink_test_tsan
asan: outboard_sink_test_asan
.PHONY: all tsan asan
