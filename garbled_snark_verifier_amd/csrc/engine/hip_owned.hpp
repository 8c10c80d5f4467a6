// Move-only owners of the HIP resources the host runtime holds: device buffers, page-locked host buffers, streams, events.  An owner
// releases what it holds exactly once (destructor, reset(), or when something else is moved or allocated over it) and is empty
// afterwards; a failed create leaves it empty and clears the error HIP keeps for hipGetLastError() — the kernel launchers report that
// one, so the stale error of e.g. an out-of-memory hipMalloc would make every later launch of the process look failed.  The release
// calls synchronise the device: WHEN an owner may go away is the business of whoever holds it (engine_internal.hpp, deferred release).
// Nothing but the HIP runtime API and the standard library: this header compiles alone (tests/hip_owned).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <utility>

namespace gsv {
namespace detail {
template <class H, hipError_t (*Release)(H)>
class HipHandle {
 public:
  HipHandle() = default;
  HipHandle(HipHandle&& o) noexcept : h_(std::exchange(o.h_, H())) {}
  HipHandle& operator=(HipHandle&& o) noexcept { if (this != &o) { reset(); h_ = std::exchange(o.h_, H()); } return *this; }
  HipHandle(const HipHandle&) = delete;
  HipHandle& operator=(const HipHandle&) = delete;
  ~HipHandle() { reset(); }
  void reset() { if (h_) (void)Release(std::exchange(h_, H())); }
  explicit operator bool() const { return h_ != H(); }
 protected:
  hipError_t created(hipError_t e) { if (e != hipSuccess) { h_ = H(); (void)hipGetLastError(); } return e; }  // e: the result of the create call that wrote h_
  H h_ = H();
};
}  // namespace detail

// hipMalloc / hipFree
class DevBuf : public detail::HipHandle<void*, hipFree> {
 public:
  hipError_t alloc(size_t bytes) { reset(); bytes_ = bytes; return created(hipMalloc(&h_, bytes)); }  // releases what it held first
  void* get() const { return h_; }
  template <class T> T* as() const { return static_cast<T*>(h_); }
  size_t bytes() const { return h_ ? bytes_ : 0; }
 private:
  size_t bytes_ = 0;
};

// hipHostMalloc / hipHostFree: a page-locked chunk buffer (hipHostMallocDefault) or, with hipHostMallocMapped among the flags, host
// memory the device reads and writes through dev()
template <class T>
class MappedHost : public detail::HipHandle<void*, hipHostFree> {
 public:
  hipError_t alloc(size_t bytes, unsigned flags) {
    reset(); dev_ = nullptr;
    hipError_t e = created(hipHostMalloc(&h_, bytes, flags));
    if (e == hipSuccess && (flags & hipHostMallocMapped) && (e = hipHostGetDevicePointer(&dev_, h_, 0)) != hipSuccess) { reset(); (void)hipGetLastError(); }
    return e;
  }
  T* get() const { return static_cast<T*>(h_); }
  T* dev() const { return h_ ? static_cast<T*>(dev_) : nullptr; }  // the device's address of get() (mapped allocations)
 private:
  void* dev_ = nullptr;
};

// hipStreamCreateWithFlags / ...WithPriority, or adopts a stream created otherwise (CU mask) / hipStreamDestroy
class Stream : public detail::HipHandle<hipStream_t, hipStreamDestroy> {
 public:
  Stream() = default;
  explicit Stream(hipStream_t adopted) { h_ = adopted; }
  hipError_t create(unsigned flags) { reset(); return created(hipStreamCreateWithFlags(&h_, flags)); }
  hipError_t create(unsigned flags, int priority) { reset(); return created(hipStreamCreateWithPriority(&h_, flags, priority)); }
  hipStream_t get() const { return h_; }
};

// hipEventCreateWithFlags / hipEventDestroy
class Event : public detail::HipHandle<hipEvent_t, hipEventDestroy> {
 public:
  hipError_t create(unsigned flags = hipEventDefault) { reset(); return created(hipEventCreateWithFlags(&h_, flags)); }
  hipEvent_t get() const { return h_; }
};
}  // namespace gsv
