// TEST-ONLY (tests/test_drain_pipeline.py): the host side of the streaming drain, csrc/engine/drain_pipeline.hpp, alone.  The few
// hip* functions the header (and hip_owned.hpp) calls are the stand-ins of tests/hip_standin/hip_standin.hpp, which model ASYNCHRONY:
// a copy's bytes move when its stream, or an event recorded on it behind the copy, is synchronised — a pipeline that hashed a chunk
// before waiting for its copy would see the bytes the chunk buffer held before.  main() returns non-zero when a check fails; a deadlock
// is the caller's time limit.  No HIP runtime is linked, no device is needed; the same program is what the Makefile's tsan / asan
// targets build.
#include "../../garbled_snark_verifier_amd/csrc/engine/drain_pipeline.hpp"
#include "../hip_standin/hip_standin.hpp"

#include <sys/stat.h>
#include <unistd.h>

#include <fstream>
#include <iterator>

using namespace gsv;

namespace {
// record r of instance i: sixteen bytes that name both
void record_bytes(size_t inst, uint64_t r, uint8_t* out) {
  uint64_t x = (uint64_t(inst) + 1) * 0x9E3779B97F4A7C15ull ^ (r + 1) * 0xC2B2AE3D27D4EB4Full;
  for (int k = 0; k < 16; ++k) { x ^= x >> 29; x *= 0xBF58476D1CE4E5B9ull; out[k] = uint8_t(x >> 56); }
}
std::vector<std::vector<uint8_t>> make_streams(size_t n_inst, uint64_t n_records) {
  std::vector<std::vector<uint8_t>> s(n_inst, std::vector<uint8_t>(size_t(n_records) * 16));
  for (size_t i = 0; i < n_inst; ++i) for (uint64_t r = 0; r < n_records; ++r) record_bytes(i, r, s[i].data() + 16 * r);
  return s;
}
std::vector<uint8_t> serial_mac(const std::vector<uint8_t>& stream) {
  CbcMacHost m; m.update(stream.data(), stream.size() / 16);
  std::vector<uint8_t> d(16); m.digest(d.data()); return d;
}
std::vector<uint8_t> digest_of(const CbcMacHost& m) { std::vector<uint8_t> d(16); m.digest(d.data()); return d; }
std::vector<uint8_t> read_file(const std::string& p) { std::ifstream f(p, std::ios::binary); return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>()); }
bool exists(const std::string& p) { struct stat sb; return ::stat(p.c_str(), &sb) == 0; }
std::string gc_path(const std::string& dir, size_t index) { return dir + "/gc_" + std::to_string(index) + ".bin"; }

// what ensure_drain sets up in the session: copy streams, pinned chunk sets, one event per worker
void setup_drain(gsv_drain& d, size_t T, size_t group, uint64_t chunk, int n_copy_streams = 2) {
  d.chunk = chunk; d.group = int(group);
  for (int k = 0; k < n_copy_streams; ++k) { Stream st; CHECK(st.create(hipStreamNonBlocking) == hipSuccess); d.copy_gate.idle.push_back(st.get()); d.copy_streams.push_back(std::move(st)); }
  d.workers.resize(T);
  for (gsv_drain::Worker& w : d.workers) {
    for (auto& set : w.pinned) for (size_t g = 0; g < group; ++g) CHECK(set[g].alloc(chunk * 16, hipHostMallocDefault) == hipSuccess);
    CHECK(w.done.create(hipEventBlockingSync | hipEventDisableTiming) == hipSuccess);
  }
}
struct Seg { uint64_t n, base; };
std::vector<Seg> segs_of(const std::vector<uint64_t>& lengths, uint64_t base = 0) {
  std::vector<Seg> v;
  for (uint64_t n : lengths) { v.push_back(Seg{n, base}); base += n; }
  return v;
}
// the callback's view: per instance (one worker's alone), the records in the order they arrived
struct Seen {
  std::vector<std::vector<uint8_t>> bytes;
  std::vector<uint64_t> next;    // the first_record the next run of an instance must carry
  std::atomic<int> calls{0}, out_of_order{0};
  int fail_at_call = 0;          // this call (1-based) returns non-zero
  std::function<bool(size_t inst, uint64_t first, const uint8_t* rec, uint64_t n)> also;  // a further check per run
  std::atomic<int> also_failed{0};
  Seen(size_t n_inst, uint64_t first) : bytes(n_inst), next(n_inst, first) {}
  static int fn(void* user, size_t inst, uint64_t first, const uint8_t* rec, uint64_t n) {
    Seen& s = *static_cast<Seen*>(user);
    if (++s.calls == s.fail_at_call) return 1;
    if (first != s.next[inst]) ++s.out_of_order;
    s.next[inst] = first + n;
    s.bytes[inst].insert(s.bytes[inst].end(), rec, rec + 16 * n);
    if (s.also && !s.also(inst, first, rec, n)) ++s.also_failed;
    return 0;
  }
};
// One pipeline over `segs`, as garble_streaming_pass drives it: wait for the buffer, "gather" the segment into it, push.  `fill`
// writes the segment into the gate-order buffer (default: the instances' streams).
struct Run {
  size_t n_inst, group, T, depth; uint64_t chunk, seg_records; bool blocking = false;
  DrainError error = DrainError::None;
  using Fill = std::function<void(size_t seg_index, const Seg&, uint8_t* buf)>;
  void go(const std::vector<std::vector<uint8_t>>& streams, const std::vector<Seg>& segs, const DrainSink& sink, std::vector<CbcMacHost>& macs, GcFiles& files, Fill fill = nullptr) {
    gsv_drain d;
    setup_drain(d, T, group, chunk);
    std::vector<std::vector<uint8_t>> gate(depth, std::vector<uint8_t>(n_inst * size_t(seg_records) * 16 + 16));
    DrainShape shape;
    shape.n_inst = n_inst; shape.group = group; shape.n_workers = T; shape.chunk = chunk; shape.seg_records = seg_records; shape.blocking_wait = blocking;
    for (auto& g : gate) shape.gate_bufs.push_back(g.data());
    std::atomic<DrainError> err{DrainError::None};
    DrainWorkers workers(&d, shape, sink, macs, files, err);
    CHECK(workers.depth() == depth);
    for (size_t k = 0; k < segs.size(); ++k) {
      CHECK(workers.next_buffer() == k % depth);
      (void)workers.wait_buffer();
      uint8_t* buf = gate[workers.next_buffer()].data();
      if (fill) fill(k, segs[k], buf);
      else for (size_t i = 0; i < n_inst; ++i) std::memcpy(buf + i * seg_records * 16, streams[i].data() + segs[k].base * 16, segs[k].n * 16);
      workers.push(segs[k].n, segs[k].base);
    }
    workers.finish();
    error = workers.error();
  }
};

// 1. ragged group, several segments (not a multiple of the chunk, empty, shorter than a chunk, several chunks), depth 2; MAC + files + callback
void case_ragged(const std::string& dir, size_t n_inst, size_t group, bool blocking) {
  const std::vector<Seg> segs = segs_of({7, 0, 1, 10});
  const auto streams = make_streams(n_inst, 18);
  std::vector<CbcMacHost> macs(n_inst);
  std::vector<uint8_t> hashes(16 * n_inst);
  Seen seen(n_inst, 0);
  DrainSink sink; sink.hashes = hashes.data(); sink.dir = dir.c_str(); sink.first_index = 100; sink.fn = Seen::fn; sink.user = &seen;
  {
    GcFiles files; std::string failed;
    CHECK(files.open(dir.c_str(), 100, n_inst, "wb", &failed));
    Run r{n_inst, group, 2, 2, 3, 10, blocking};
    r.go(streams, segs, sink, macs, files);
    CHECK(r.error == DrainError::None);
    files.keep();
  }
  CHECK(seen.out_of_order == 0);
  for (size_t i = 0; i < n_inst; ++i) {
    CHECK(digest_of(macs[i]) == serial_mac(streams[i]));
    CHECK(read_file(gc_path(dir, 100 + i)) == streams[i]);
    CHECK(seen.bytes[i] == streams[i]);  // every record exactly once, in stream order (first_record = base + off: out_of_order)
    std::remove(gc_path(dir, 100 + i).c_str());
  }
}
// 2. buffer recycling: after each wait_buffer() the producer overwrites the buffer with a pattern of the NEXT segment only; no run the
// callback sees may hold another segment's pattern
void case_recycling(size_t depth, size_t n_segs) {
  const size_t n_inst = 3;
  const uint64_t len = 8;
  std::vector<uint64_t> lengths(n_segs, len);
  std::vector<CbcMacHost> macs(n_inst);
  GcFiles files;
  Seen seen(n_inst, 0);
  seen.also = [&](size_t, uint64_t first, const uint8_t* rec, uint64_t n) {
    const uint8_t want = uint8_t(0xA0 + first / len);  // the pattern of the segment this run belongs to
    for (uint64_t k = 0; k < 16 * n; ++k) if (rec[k] != want) return false;
    return true;
  };
  DrainSink sink; sink.fn = Seen::fn; sink.user = &seen;
  Run r{n_inst, 1, 2, depth, 3, len};
  r.go({}, segs_of(lengths), sink, macs, files, [&](size_t k, const Seg&, uint8_t* buf) { std::memset(buf, 0xA0 + int(k), n_inst * len * 16); });
  CHECK(r.error == DrainError::None && seen.also_failed == 0 && seen.out_of_order == 0);
  for (size_t i = 0; i < n_inst; ++i) CHECK(seen.bytes[i].size() == n_segs * len * 16);
}
// 3. slices chain: two pipelines, one after the other, over the same MAC states and "ab" files = one pipeline over the concatenation
void case_slices(const std::string& dir) {
  const size_t n_inst = 5;
  const auto streams = make_streams(n_inst, 20);
  std::vector<CbcMacHost> macs(n_inst);
  std::vector<uint8_t> hashes(16 * n_inst);
  DrainSink sink; sink.hashes = hashes.data(); sink.dir = dir.c_str();
  const std::vector<std::vector<uint64_t>> slices = {{7, 2}, {4, 7}};
  uint64_t base = 0;
  for (size_t k = 0; k < 2; ++k) {
    GcFiles files; std::string failed;
    CHECK(files.open(dir.c_str(), 0, n_inst, k == 0 ? "wb" : "ab", &failed));
    Run r{n_inst, 4, 2, 2, 3, 7};
    r.go(streams, segs_of(slices[k], base), sink, macs, files);
    CHECK(r.error == DrainError::None);
    files.keep();
    base += 9;
  }
  for (size_t i = 0; i < n_inst; ++i) {
    CHECK(digest_of(macs[i]) == serial_mac(streams[i]));
    CHECK(read_file(gc_path(dir, i)) == streams[i]);
    std::remove(gc_path(dir, i).c_str());
  }
}
// 4. / 5. a failing sink (third call) or copy (fourth hipMemcpyAsync): the error is reported, nothing blocks — not finish(), not the
// wait_buffer() / push() calls behind the failure (the loop in Run::go carries on through all segments) — and no file is left behind
void case_failure(const std::string& dir, bool copy_fails) {
  const size_t n_inst = 5;
  const auto streams = make_streams(n_inst, 40);
  std::vector<CbcMacHost> macs(n_inst);
  Seen seen(n_inst, 0);
  DrainSink sink; sink.dir = dir.c_str(); sink.fn = Seen::fn; sink.user = &seen;
  if (copy_fails) { std::lock_guard<std::mutex> lk(hip_mu); fail_copy_at = copy_seq + 4; } else seen.fail_at_call = 3;
  {
    GcFiles files; std::string failed;
    CHECK(files.open(dir.c_str(), 7, n_inst, "wb", &failed));
    CHECK(exists(gc_path(dir, 7)) && exists(gc_path(dir, 11)));
    Run r{n_inst, 4, 2, 1, 3, 10};
    r.go(streams, segs_of({10, 10, 10, 10}), sink, macs, files);
    CHECK(r.error == (copy_fails ? DrainError::Copy : DrainError::Sink));
  }
  { std::lock_guard<std::mutex> lk(hip_mu); fail_copy_at = 0; }
  for (size_t i = 0; i < n_inst; ++i) CHECK(!exists(gc_path(dir, 7 + i)));
}
// 6. no segments at all: construct + finish(); construct + destroy
void case_empty() {
  std::vector<CbcMacHost> macs(4);
  GcFiles files;
  Run r{4, 4, 2, 2, 3, 10};
  r.go({}, {}, DrainSink(), macs, files);
  CHECK(r.error == DrainError::None);
  gsv_drain d;
  setup_drain(d, 2, 4, 3);
  std::vector<uint8_t> gate(4 * 10 * 16);
  DrainShape shape;
  shape.n_inst = 4; shape.group = 4; shape.n_workers = 2; shape.chunk = 3; shape.seg_records = 10; shape.gate_bufs = {gate.data()};
  std::atomic<DrainError> err{DrainError::None};
  { DrainWorkers workers(&d, shape, DrainSink(), macs, files, err); }
  { DrainShape none = shape; none.n_workers = 0; DrainWorkers idle(nullptr, none, DrainSink(), macs, files, err); CHECK(idle.wait_buffer() == 0); idle.push(5, 0); idle.push(5, 5); CHECK(idle.wait_buffer() == 0 && idle.next_buffer() == 0); }
  CHECK(err == DrainError::None);
}
// 7. the BLAKE3 absorbers: values are copied at submit time; every thread sees the tasks in submission order; false -> B3Order
void case_b3() {
  const size_t T = 3, n_tasks = 4, bytes = 96;
  std::mutex mu;
  std::vector<std::vector<uint8_t>> order(T);  // per thread: the first byte of every task it saw
  int bad_bytes = 0, bad_args = 0;
  auto absorb = [&](const uint8_t* vals, uint32_t groups, size_t t, size_t n) {
    std::lock_guard<std::mutex> lk(mu);
    if (n != T || t >= T || groups != uint32_t(vals[0]) + 1) { ++bad_args; return true; }
    for (size_t k = 0; k < bytes; ++k) if (vals[k] != vals[0]) ++bad_bytes;
    order[t].push_back(vals[0]);
    return true;
  };
  std::atomic<DrainError> err{DrainError::None};
  {
    B3Absorbers b3(T, absorb, err);
    std::vector<uint8_t> pinned(bytes);
    for (size_t k = 0; k < n_tasks; ++k) {
      std::memset(pinned.data(), int(k), bytes);
      b3.submit(pinned.data(), bytes, uint32_t(k) + 1);
      std::memset(pinned.data(), 0xEE, bytes);  // the next segment's copy lands there
    }
    b3.submit(pinned.data(), bytes, 0);  // no group values: nothing to absorb
    b3.finish();
    CHECK(b3.error() == DrainError::None);
  }
  CHECK(bad_bytes == 0 && bad_args == 0);
  for (size_t t = 0; t < T; ++t) CHECK(order[t] == (std::vector<uint8_t>{0, 1, 2, 3}));
  {
    std::atomic<DrainError> e2{DrainError::None};
    B3Absorbers b3(T, [](const uint8_t* vals, uint32_t, size_t t, size_t) { return !(vals[0] == 1 && t == 2); }, e2);
    const uint8_t v[2][4] = {{0, 0, 0, 0}, {1, 1, 1, 1}};
    b3.submit(v[0], 4, 1); b3.submit(v[1], 4, 1);
    b3.finish();
    CHECK(b3.error() == DrainError::B3Order);
  }
  { std::atomic<DrainError> e3{DrainError::None}; B3Absorbers b3(T, absorb, e3); b3.finish(); CHECK(b3.error() == DrainError::None); }  // an empty queue
  { std::atomic<DrainError> e4{DrainError::None}; B3Absorbers b3(T, absorb, e4); B3Absorbers none(0, absorb, e4); none.submit(nullptr, 0, 0); }  // destroyed without finish()
}
}  // namespace

int main() {
  char tmpl[] = "/tmp/gsv_drain_pipeline_XXXXXX";
  const char* made = mkdtemp(tmpl);
  if (!made) { std::perror("mkdtemp"); return 3; }
  const std::string dir = made;
  for (bool blocking : {false, true}) {
    case_ragged(dir, 5, 4, blocking);
    case_ragged(dir, 5, 1, blocking);
  }
  if (CbcMacHost::have_vaes()) { case_ragged(dir, 5, 16, false); case_ragged(dir, 18, 16, true); }
  case_recycling(1, 3);
  case_recycling(2, 5);
  case_slices(dir);
  case_failure(dir, false);
  case_failure(dir, true);
  case_empty();
  case_b3();
  CHECK(::rmdir(dir.c_str()) == 0);  // nothing was left behind
  if (failures) return 1;
  std::printf("drain_pipeline: ok, %llu copies%s\n", (unsigned long long)copy_seq, CbcMacHost::have_vaes() ? ", sixteen chains per step included" : "");
  return 0;
}
