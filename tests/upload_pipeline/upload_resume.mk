# TEST-ONLY: CtUploader of csrc/engine/upload_pipeline.hpp started at a record other than 0 (make -f upload_resume.mk), against the stand-ins
# of tests/hip_standin/hip_standin.hpp for the HIP calls it makes.  No HIP runtime is linked.  `tsan` / `asan` build the same stand-alone
# program under the thread / address + undefined-behaviour sanitizers, run by hand; the test suite builds and runs the plain target only.
CXX ?= g++
CXXFLAGS ?= -O1 -g -std=c++17 -Wall -Wextra -maes -msse2 -pthread
ROCM_PATH ?= /opt/rocm
SRC := ../../garbled_snark_verifier_amd/csrc
DEPS := upload_resume_test.cpp ../hip_standin/hip_standin.hpp $(SRC)/engine/upload_pipeline.hpp $(SRC)/engine/hip_owned.hpp $(SRC)/engine/host_crypto.hpp
BUILD = $(CXX) $(CXXFLAGS) -D__HIP_PLATFORM_AMD__ -I$(ROCM_PATH)/include -o $@ upload_resume_test.cpp
all: upload_resume_test
upload_resume_test: $(DEPS)
	$(BUILD)
upload_resume_test_tsan: $(DEPS)
	$(BUILD) -fsanitize=thread
upload_resume_test_asan: $(DEPS)
	$(BUILD) -fsanitize=address,undefined -fno-sanitize-recover=undefined
tsan: upload_resume_test_tsan
asan: upload_resume_test_asan
.PHONY: all tsan asan
