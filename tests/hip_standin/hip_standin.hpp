// TEST-ONLY: stand-ins for the few hip* functions that hip_owned.hpp, drain_pipeline.hpp and upload_pipeline.hpp call, for stand-alone
// CPU programs (tests/drain_pipeline, tests/upload_pipeline) that include it ONCE, after the header under test.  The stand-ins model
// ASYNCHRONY: hipMemcpyAsync only records the copy against its stream; the bytes move when that stream, or an event recorded on it
// behind the copy, is synchronised — a pipeline that read or refilled a buffer before waiting for its copy would see, or land, the
// wrong bytes.  "Device" buffers are host arrays, the copy kind is ignored.  No HIP runtime is linked, no device is needed.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>

namespace {
struct PendingCopy { void* dst; const void* src; size_t n; uint64_t seq; };
struct FakeStream { std::deque<PendingCopy> pending; };
struct FakeEvent { FakeStream* on = nullptr; uint64_t seq = 0; };
std::mutex hip_mu;            // the stand-ins are called from every worker
uint64_t copy_seq = 0;        // hipMemcpyAsync calls so far
uint64_t fail_copy_at = 0;    // the copy with this number (1-based) fails; 0: none
// the copies recorded on `st` up to number `upto` happen now, in order
void flush(FakeStream* st, uint64_t upto) {
  while (!st->pending.empty() && st->pending.front().seq <= upto) {
    std::memcpy(st->pending.front().dst, st->pending.front().src, st->pending.front().n);
    st->pending.pop_front();
  }
}
int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)
}  // namespace

extern "C" {
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipMalloc(void** p, size_t n) { *p = std::malloc(n); return hipSuccess; }
hipError_t hipFree(void* p) { std::free(p); return hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t n, unsigned int) { *p = std::calloc(n ? n : 1, 1); return hipSuccess; }
hipError_t hipHostGetDevicePointer(void** dev, void* host, unsigned int) { *dev = host; return hipSuccess; }
hipError_t hipHostFree(void* p) { std::free(p); return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int) { *s = reinterpret_cast<hipStream_t>(new FakeStream()); return hipSuccess; }
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned int, int) { return hipStreamCreateWithFlags(s, 0); }
hipError_t hipStreamDestroy(hipStream_t s) { delete reinterpret_cast<FakeStream*>(s); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { *e = reinterpret_cast<hipEvent_t>(new FakeEvent()); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { delete reinterpret_cast<FakeEvent*>(e); return hipSuccess; }
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, hipMemcpyKind, hipStream_t s) {
  std::lock_guard<std::mutex> lk(hip_mu);
  if (++copy_seq == fail_copy_at) return hipErrorUnknown;
  reinterpret_cast<FakeStream*>(s)->pending.push_back(PendingCopy{dst, src, n, copy_seq});
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s) { std::lock_guard<std::mutex> lk(hip_mu); flush(reinterpret_cast<FakeStream*>(s), ~0ull); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
  std::lock_guard<std::mutex> lk(hip_mu);
  FakeEvent* ev = reinterpret_cast<FakeEvent*>(e);
  ev->on = reinterpret_cast<FakeStream*>(s); ev->seq = copy_seq;
  return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e) {
  std::lock_guard<std::mutex> lk(hip_mu);
  FakeEvent* ev = reinterpret_cast<FakeEvent*>(e);
  if (ev->on) flush(ev->on, ev->seq);
  return hipSuccess;
}
}
