// TEST-ONLY (tests/test_hip_owned.py): the move-only owners of csrc/engine/hip_owned.hpp, alone.  This program defines the few hip*
// functions the header calls; the definitions keep the set of live handles and ABORT when a handle is released twice or was never
// created.  main() returns non-zero when a check fails or a handle is still live at the end.  No HIP runtime is linked, no device is needed.
#include "../../garbled_snark_verifier_amd/csrc/engine/hip_owned.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <vector>

using namespace gsv;

namespace {
std::set<std::pair<char, void*>> live;  // (kind: 'd' device, 'h' host, 's' stream, 'e' event; handle)
uintptr_t next_handle = 0;
size_t n_created = 0, n_released = 0;
int fail_creates = 0;                   // the next this-many create calls fail ...
bool fail_device_pointer = false;       // hipHostGetDevicePointer fails ...
hipError_t sticky = hipSuccess;         // ... and leave their error behind for hipGetLastError, as the runtime does
void* const POISON = reinterpret_cast<void*>(uintptr_t(0xDEAD0));  // what a failed create leaves in its out-parameter: never a live handle

hipError_t create(char kind, void** out) {
  if (fail_creates > 0) { --fail_creates; *out = POISON; return sticky = hipErrorOutOfMemory; }
  *out = reinterpret_cast<void*>(0x1000 * ++next_handle);
  live.insert({kind, *out});
  ++n_created;
  return hipSuccess;
}
hipError_t release(char kind, void* h) {
  if (!live.erase({kind, h})) { std::fprintf(stderr, "FATAL: handle %p of kind '%c' released twice, or never created\n", h, kind); std::abort(); }
  ++n_released;
  return hipSuccess;
}
int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)
}  // namespace

extern "C" {
hipError_t hipGetLastError(void) { hipError_t e = sticky; sticky = hipSuccess; return e; }
hipError_t hipMalloc(void** p, size_t) { return create('d', p); }
hipError_t hipFree(void* p) { return release('d', p); }
hipError_t hipHostMalloc(void** p, size_t, unsigned int) { return create('h', p); }
hipError_t hipHostGetDevicePointer(void** dev, void* host, unsigned int) {
  if (fail_device_pointer) return sticky = hipErrorInvalidValue;
  if (!live.count({'h', host})) { std::fprintf(stderr, "FATAL: device pointer of a host buffer that is not live\n"); std::abort(); }
  *dev = static_cast<char*>(host) + 1;  // (any address that is not the host's)
  return hipSuccess;
}
hipError_t hipHostFree(void* p) { return release('h', p); }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int) { return create('s', reinterpret_cast<void**>(s)); }
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned int, int) { return create('s', reinterpret_cast<void**>(s)); }
hipError_t hipStreamDestroy(hipStream_t s) { return release('s', s); }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return create('e', reinterpret_cast<void**>(e)); }
hipError_t hipEventDestroy(hipEvent_t e) { return release('e', e); }
}

// the shape of the engine's DevProgram: an aggregate of owners, held through shared_ptr and filed under several keys
struct Image { DevBuf steps, ands, xors; size_t bytes = 0; };

int main() {
  {  // construct and destroy: an empty owner releases nothing, a full one exactly once
    DevBuf none;
    CHECK(!none && none.get() == nullptr && none.bytes() == 0);
    DevBuf d; MappedHost<uint32_t> pinned, mapped; Stream s, prio; Event e;
    CHECK(d.alloc(100) == hipSuccess && d && d.bytes() == 100 && d.as<char>() == d.get());
    CHECK(pinned.alloc(64, hipHostMallocDefault) == hipSuccess && pinned && pinned.get());
    CHECK(mapped.alloc(64, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess && mapped.dev() && (void*)mapped.dev() != (void*)mapped.get());
    CHECK(s.create(hipStreamNonBlocking) == hipSuccess && s && prio.create(hipStreamNonBlocking, -1) == hipSuccess && prio.get() != s.get());
    CHECK(e.create(hipEventDisableTiming) == hipSuccess && e && e.get());
    CHECK(live.size() == 6);
  }
  CHECK(live.empty() && n_created == 6 && n_released == 6);
  {  // an adopted stream is released like a created one
    hipStream_t raw = nullptr;
    CHECK(hipStreamCreateWithFlags(&raw, 0) == hipSuccess);
    Stream s(raw);
    CHECK(s.get() == raw && live.size() == 1);
  }
  CHECK(live.empty());
  {  // move-construct; move-assign onto a live handle (released at once); self-move-assign
    DevBuf a, b;
    CHECK(a.alloc(10) == hipSuccess && b.alloc(20) == hipSuccess);
    void* const pa = a.get();
    DevBuf c(std::move(a));
    CHECK(!a && a.bytes() == 0 && c.get() == pa && c.bytes() == 10 && live.size() == 2);
    b = std::move(c);
    CHECK(!c && b.get() == pa && b.bytes() == 10 && live.size() == 1);
    DevBuf& self = b;
    b = std::move(self);
    CHECK(b.get() == pa && live.size() == 1);
    Event e1, e2;
    CHECK(e1.create() == hipSuccess && e2.create() == hipSuccess);
    e1 = std::move(e2);
    CHECK(e1 && !e2 && live.size() == 2);
    MappedHost<uint64_t> m1, m2;
    CHECK(m1.alloc(8, hipHostMallocMapped) == hipSuccess);
    uint64_t* const dev = m1.dev();
    m2 = std::move(m1);
    CHECK(m2.dev() == dev && m1.dev() == nullptr && m1.get() == nullptr);
  }
  CHECK(live.empty());
  {  // reset twice; alloc over a live buffer
    DevBuf d; Stream s;
    CHECK(d.alloc(1) == hipSuccess && s.create(0) == hipSuccess);
    d.reset(); d.reset(); s.reset(); s.reset();
    CHECK(!d && !s && live.empty());
    CHECK(d.alloc(5) == hipSuccess);
    void* const first = d.get();
    CHECK(d.alloc(7) == hipSuccess && d.bytes() == 7 && live.size() == 1 && !live.count({'d', first}));
    Event e;
    CHECK(e.create() == hipSuccess && e.create() == hipSuccess && live.size() == 2);
  }
  CHECK(live.empty());
  {  // a failed create leaves the owner empty — whatever the call wrote into its out-parameter — and the runtime's error cleared
    DevBuf d; MappedHost<char> h; Stream s; Event e;
    fail_creates = 1; CHECK(d.alloc(1 << 20) == hipErrorOutOfMemory && !d && d.get() == nullptr && d.bytes() == 0 && sticky == hipSuccess);
    fail_creates = 1; CHECK(h.alloc(64, hipHostMallocDefault) == hipErrorOutOfMemory && !h && sticky == hipSuccess);
    fail_creates = 1; CHECK(s.create(0) == hipErrorOutOfMemory && !s && sticky == hipSuccess);
    fail_creates = 1; CHECK(s.create(0, -1) == hipErrorOutOfMemory && !s && sticky == hipSuccess);
    fail_creates = 1; CHECK(e.create() == hipErrorOutOfMemory && !e && sticky == hipSuccess);
    CHECK(live.empty());
    // a failed alloc over a live buffer has released the old one; a mapped buffer whose device address cannot be had is released
    CHECK(d.alloc(4) == hipSuccess);
    fail_creates = 1; CHECK(d.alloc(8) != hipSuccess && !d && live.empty() && sticky == hipSuccess);
    MappedHost<char> m;
    CHECK(m.alloc(64, hipHostMallocDefault) == hipSuccess && m.get() && m.dev() == nullptr);  // not mapped: no device address
    fail_device_pointer = true;
    CHECK(m.alloc(64, hipHostMallocMapped) == hipErrorInvalidValue && !m && m.get() == nullptr && m.dev() == nullptr && live.empty() && sticky == hipSuccess);
    fail_device_pointer = false;
    CHECK(m.alloc(64, hipHostMallocMapped) == hipSuccess && m.dev() && m.alloc(64, hipHostMallocDefault) == hipSuccess && m.dev() == nullptr);  // no stale device address
  }
  CHECK(live.empty());
  {  // std::vector<DevBuf> growth: elements move, none is released on the way; clear() releases all
    std::vector<DevBuf> v;
    std::set<void*> handles;
    for (int i = 0; i < 100; ++i) { DevBuf q; CHECK(q.alloc(size_t(i) + 1) == hipSuccess); handles.insert(q.get()); v.push_back(std::move(q)); }
    CHECK(live.size() == 100 && handles.size() == 100);
    for (size_t i = 0; i < v.size(); ++i) CHECK(handles.count(v[i].get()) && v[i].bytes() == i + 1);
    v.erase(v.begin() + 10);
    CHECK(live.size() == 99);
    v.clear();
    CHECK(live.empty());
    std::vector<Stream> streams(3);  // default-constructed, then filled
    for (Stream& s : streams) CHECK(s.create(0) == hipSuccess);
    streams.resize(50);
    CHECK(live.size() == 3);
  }
  CHECK(live.empty());
  {  // an image filed under two keys is released once, when the last key goes — and not while a key still holds it
    std::map<int, std::shared_ptr<Image>> dev;
    auto img = std::make_shared<Image>();
    CHECK(img->steps.alloc(32) == hipSuccess && img->ands.alloc(32) == hipSuccess && img->xors.alloc(32) == hipSuccess);
    const Image* view = img.get();  // what a session keeps: it does not hold the image alive
    dev[1] = img; dev[4] = std::move(img);
    CHECK(live.size() == 3 && dev[1].get() == view && dev[4].get() == view);
    dev.erase(1);
    CHECK(live.size() == 3);
    dev.clear();
    CHECK(live.empty());
    auto half = std::make_shared<Image>();  // a failed upload: the local image goes with what it had allocated so far
    CHECK(half->steps.alloc(32) == hipSuccess);
    fail_creates = 1; CHECK(half->ands.alloc(32) != hipSuccess);
    half.reset();
    CHECK(live.empty());
  }
  CHECK(n_created == n_released);
  if (!live.empty()) { std::fprintf(stderr, "%zu handles still live at exit\n", live.size()); return 2; }
  if (failures) return 1;
  std::printf("hip_owned: ok, %zu handles created and released\n", n_created);
  return 0;
}
