// TEST-ONLY (tests/test_upload_pipeline.py): the host side of the streaming evaluator, csrc/engine/upload_pipeline.hpp, alone.  The few
// hip* functions the header (and hip_owned.hpp) calls are the stand-ins of tests/hip_standin/hip_standin.hpp, which model ASYNCHRONY:
// a copy's bytes move when its stream, or an event recorded on it behind the copy, is synchronised — an uploader that refilled a staging
// buffer before waiting for its copy would land the wrong bytes in the "device" buffer.  main() returns non-zero when a check fails; a
// deadlock is the caller's time limit.  No HIP runtime is linked, no device is needed; the same program is what the Makefile's tsan /
// asan targets build.
#include "../../garbled_snark_verifier_amd/csrc/engine/upload_pipeline.hpp"
#include "../hip_standin/hip_standin.hpp"

#include <dirent.h>

using namespace gsv;

namespace {
// record r of instance i: sixteen bytes that name both
void record_bytes(size_t inst, uint64_t r, uint8_t* out) {
  uint64_t x = (uint64_t(inst) + 1) * 0x9E3779B97F4A7C15ull ^ (r + 1) * 0xC2B2AE3D27D4EB4Full;
  for (int k = 0; k < 16; ++k) { x ^= x >> 29; x *= 0xBF58476D1CE4E5B9ull; out[k] = uint8_t(x >> 56); }
}
using Streams = std::vector<std::vector<uint8_t>>;
Streams make_streams(size_t n_inst, uint64_t n_records) {
  Streams s(n_inst, std::vector<uint8_t>(size_t(n_records) * 16));
  for (size_t i = 0; i < n_inst; ++i) for (uint64_t r = 0; r < n_records; ++r) record_bytes(i, r, s[i].data() + 16 * r);
  return s;
}
std::vector<uint8_t> serial_macs(const Streams& streams) {
  std::vector<uint8_t> d(16 * streams.size());
  for (size_t i = 0; i < streams.size(); ++i) { CbcMacHost m; m.update(streams[i].data(), streams[i].size() / 16); m.digest(d.data() + 16 * i); }
  return d;
}
size_t threads_of_this_process() {
  size_t n = 0;
  DIR* d = opendir("/proc/self/task");
  if (!d) return 0;
  while (dirent* e = readdir(d)) if (e->d_name[0] != '.') ++n;
  closedir(d);
  return n;
}
size_t pending_on(const Stream& st) { std::lock_guard<std::mutex> lk(hip_mu); return reinterpret_cast<FakeStream*>(st.get())->pending.size(); }

// A CiphertextSource over `streams` that records every read; a read past the end of an instance's stream reports "dry"
struct ReadCall { size_t inst; uint64_t first, n; bool operator==(const ReadCall& o) const { return inst == o.inst && first == o.first && n == o.n; } };
struct Source {
  const Streams& streams;
  std::vector<ReadCall> calls;
  CtUploader::Read fn() {
    return [this](size_t i, uint64_t first, uint8_t* dst, uint64_t n) -> int {
      calls.push_back(ReadCall{i, first, n});
      if ((first + n) * 16 > streams[i].size()) return 1;
      std::memcpy(dst, streams[i].data() + first * 16, n * 16);
      return 0;
    };
  }
};
// what a chunk-major uploader reads for segments of `lengths` records: offset outer, instance inner, n = min(chunk, left)
std::vector<ReadCall> chunk_major(const std::vector<uint64_t>& lengths, size_t n_inst, uint64_t chunk) {
  std::vector<ReadCall> v;
  uint64_t base = 0;
  for (uint64_t n : lengths) {
    for (uint64_t off = 0; off < n; off += chunk) for (size_t i = 0; i < n_inst; ++i) v.push_back(ReadCall{i, base + off, std::min(chunk, n - off)});
    base += n;
  }
  return v;
}

// One pass as evaluate_streaming_pass drives it: segment after segment into the ONE gate-order buffer, the stream synchronised after
// each (the engine's scatter and launch stand there).  Returns every segment's gate-order bytes, in order, then the MACs.
struct PassResult { std::vector<uint8_t> gate_bytes, macs; };
PassResult run_pass(const Streams& streams, const std::vector<uint64_t>& lengths, uint64_t seg_records, uint64_t chunk, size_t T) {
  const size_t n_inst = streams.size();
  PassResult out;
  Source src{streams, {}};
  Stream st;
  CHECK(st.create(hipStreamNonBlocking) == hipSuccess);
  std::vector<uint8_t> gate(n_inst * size_t(seg_records) * 16 + 16, 0xEE);
  const size_t threads_before = threads_of_this_process();
  CtUploader up(n_inst, seg_records, chunk, T, src.fn());
  // T = 0: no worker thread exists.  (T > 0: at least T more — a sanitizer's runtime may start a thread of its own beside the first)
  CHECK(T ? threads_of_this_process() >= threads_before + T : threads_of_this_process() == threads_before);
  CHECK(up.alloc() == hipSuccess);
  uint64_t base = 0;
  for (uint64_t n : lengths) {
    CHECK(up.upload(base, n, gate.data(), st.get()) == UploadError::None);
    CHECK(hipStreamSynchronize(st.get()) == hipSuccess);
    for (size_t i = 0; i < n_inst; ++i) {
      const uint8_t* got = gate.data() + (i * seg_records) * 16;
      CHECK(std::memcmp(got, streams[i].data() + base * 16, n * 16) == 0);
      out.gate_bytes.insert(out.gate_bytes.end(), got, got + n * 16);
    }
    base += n;
  }
  CHECK(src.calls == chunk_major(lengths, n_inst, chunk));
  up.finish();
  out.macs.assign(16 * n_inst, 0);
  up.digests(out.macs.data());
  return out;
}

// 1. placement, order, MACs: segments that are no multiple of the chunk / empty / shorter than a chunk / several chunks.  T = 0 has two
// staging buffers for the 15 reads of the first segment: every buffer is refilled with its copy still queued unless the uploader waits.
// 5. a second pass: a fresh uploader over the same source (the safe-schedule repeat) yields the same MACs and bytes
void case_placement(size_t T) {
  const Streams streams = make_streams(5, 18);
  const std::vector<uint64_t> lengths = {7, 0, 1, 10};
  const PassResult a = run_pass(streams, lengths, 10, 3, T);
  CHECK(a.macs == (T ? serial_macs(streams) : std::vector<uint8_t>(16 * 5, 0)));  // (no workers: no MAC is computed, the states stay zero)
  const PassResult b = run_pass(streams, lengths, 10, 3, T);
  CHECK(a.macs == b.macs && a.gate_bytes == b.gate_bytes);
}
// 2. degenerate and one-chunk shapes
void case_degenerate() {
  const Streams none = make_streams(3, 0);
  for (size_t T : {size_t(0), size_t(2)}) {
    const PassResult r = run_pass(none, {}, 0, 1, T);  // seg_records 0 (chunk = max(seg_records, 1)), no segments, with finish()
    CHECK(r.gate_bytes.empty() && r.macs == std::vector<uint8_t>(16 * 3, 0));
    Source src{none, {}};
    { CtUploader up(3, 0, 1, T, src.fn()); CHECK(up.alloc() == hipSuccess); }  // ... and destroyed without finish()
    { CtUploader never_allocated(3, 0, 1, T, src.fn()); }
    CHECK(src.calls.empty());
  }
  const Streams one = make_streams(1, 3);
  const PassResult r = run_pass(one, {3}, 3, 3, 1);  // one instance, one chunk
  CHECK(r.macs == serial_macs(one) && r.gate_bytes == one[0]);
}
// 3. the source runs dry: instance 2's stream is one record short.  Reported with the instance and the first record of the chunk whose
// read failed; nothing blocks (finish() or the destructor alone); the caller, who writes the hashes only after success, has not touched them
void case_dry(bool call_finish) {
  Streams streams = make_streams(5, 18);
  streams[2].resize(17 * 16);
  Source src{streams, {}};
  Stream st;
  CHECK(st.create(hipStreamNonBlocking) == hipSuccess);
  std::vector<uint8_t> gate(5 * 10 * 16), hashes(16 * 5, 0xAB);
  {
    CtUploader up(5, 10, 3, 2, src.fn());
    CHECK(up.alloc() == hipSuccess);
    UploadError e = UploadError::None;
    uint64_t base = 0;
    for (uint64_t n : {7, 0, 1, 10}) { if (e == UploadError::None) e = up.upload(base, n, gate.data(), st.get()); base += n; }
    CHECK(e == UploadError::Dry && up.dry_instance() == 2 && up.dry_record() == 17);  // segment [8, 18): chunks at 8, 11, 14, 17
    CHECK((src.calls.back() == ReadCall{2, 17, 1}));
    if (e == UploadError::None) up.digests(hashes.data());
    if (call_finish) up.finish();
  }
  CHECK(hashes == std::vector<uint8_t>(16 * 5, 0xAB));
}
// 4. the fourth hipMemcpyAsync fails: reported, nothing blocks, and the uploader goes away with copies still queued on a stream nobody
// synchronises — its destructor waits for them before the staging buffers they read are released
void case_copy_fails() {
  const Streams streams = make_streams(5, 18);
  Source src{streams, {}};
  Stream st;
  CHECK(st.create(hipStreamNonBlocking) == hipSuccess);
  std::vector<uint8_t> gate(5 * 10 * 16, 0xEE);
  { std::lock_guard<std::mutex> lk(hip_mu); fail_copy_at = copy_seq + 4; }
  {
    CtUploader up(5, 10, 3, 2, src.fn());
    CHECK(up.alloc() == hipSuccess);
    CHECK(up.upload(0, 7, gate.data(), st.get()) == UploadError::Copy);
    CHECK(src.calls.size() == 4 && pending_on(st) == 3);
    CHECK(gate[0] == 0xEE);  // nothing has moved yet
  }
  { std::lock_guard<std::mutex> lk(hip_mu); fail_copy_at = 0; }
  CHECK(pending_on(st) == 0);
  for (size_t i = 0; i < 3; ++i) CHECK(std::memcmp(gate.data() + i * 10 * 16, streams[i].data(), 3 * 16) == 0);
  CHECK(gate[3 * 10 * 16] == 0xEE);
}
}  // namespace

int main() {
  for (size_t T : {size_t(0), size_t(1), size_t(2), size_t(5)}) case_placement(T);
  case_degenerate();
  case_dry(true);
  case_dry(false);
  case_copy_fails();
  if (failures) return 1;
  std::printf("upload_pipeline: ok, %llu copies\n", (unsigned long long)copy_seq);
  return 0;
}
