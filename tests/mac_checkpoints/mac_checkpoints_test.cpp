// TEST-ONLY (tests/test_mac_checkpoints_standalone.py): CBC-MAC checkpoints without a device.
//   * CheckpointWriter of csrc/engine/drain_pipeline.hpp behind the MAC workers (DrainWorkers), as garble_streaming_pass drives them:
//     segments that are no multiple of the chunk, empty segments, segments shorter than a group, groups of 4 and 1 chains, two slices
//     appending to the same files — the files must be byte-identical to the host writer's (mac_checkpoints_of_file) over the gc files
//     the same workers wrote;
//   * the format code of csrc/engine/mac_checkpoints.hpp: files of one call that disagree, the host checker;
//   * the chain bookkeeping the device kernel runs (csrc/engine/cbcmac_device.hpp: mac_chain, mac_chain_run), here with PlainTables,
//     over the segmentations of the GPU tests: which state a chain starts from, where it ends, what it compares, the carry.
// The hip* functions the headers call are stand-ins defined here, which model ASYNCHRONY: a copy's bytes move when its stream, or an
// event recorded on it behind the copy, is synchronised.  No HIP runtime is linked.  main() returns non-zero when a check fails; a
// deadlock is the caller's time limit.
#include "../../garbled_snark_verifier_amd/csrc/engine/drain_pipeline.hpp"
#include "../../garbled_snark_verifier_amd/csrc/engine/cbcmac_device.hpp"

#include <deque>
#include <fstream>
#include <iterator>

using namespace gsv;

namespace {
int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)
struct PendingCopy { void* dst; const void* src; size_t n; uint64_t seq; };
struct FakeStream { std::deque<PendingCopy> pending; };
struct FakeEvent { FakeStream* on = nullptr; uint64_t seq = 0; };
std::mutex hip_mu;
uint64_t copy_seq = 0;
void flush(FakeStream* st, uint64_t upto) {
  while (!st->pending.empty() && st->pending.front().seq <= upto) {
    std::memcpy(st->pending.front().dst, st->pending.front().src, st->pending.front().n);
    st->pending.pop_front();
  }
}
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
  reinterpret_cast<FakeStream*>(s)->pending.push_back(PendingCopy{dst, src, n, ++copy_seq});
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

namespace {
void record_bytes(size_t inst, uint64_t r, uint8_t* out) {
  uint64_t x = (uint64_t(inst) + 1) * 0x9E3779B97F4A7C15ull ^ (r + 1) * 0xC2B2AE3D27D4EB4Full;
  for (int k = 0; k < 16; ++k) { x ^= x >> 29; x *= 0xBF58476D1CE4E5B9ull; out[k] = uint8_t(x >> 56); }
}
std::vector<std::vector<uint8_t>> make_streams(size_t n_inst, uint64_t n_records) {
  std::vector<std::vector<uint8_t>> s(n_inst, std::vector<uint8_t>(size_t(n_records) * 16));
  for (size_t i = 0; i < n_inst; ++i) for (uint64_t r = 0; r < n_records; ++r) record_bytes(i, r, s[i].data() + 16 * r);
  return s;
}
std::vector<uint8_t> read_file(const std::string& p) { std::ifstream f(p, std::ios::binary); return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>()); }
void write_file(const std::string& p, const std::vector<uint8_t>& b) { std::ofstream f(p, std::ios::binary); f.write(reinterpret_cast<const char*>(b.data()), std::streamsize(b.size())); }
bool exists(const std::string& p) { struct stat sb; return ::stat(p.c_str(), &sb) == 0; }
std::string gc_path(const std::string& dir, size_t index) { return dir + "/gc_" + std::to_string(index) + ".bin"; }

void setup_drain(gsv_drain& d, size_t T, size_t group, uint64_t chunk) {
  d.chunk = chunk; d.group = int(group);
  for (int k = 0; k < 2; ++k) { Stream st; CHECK(st.create(hipStreamNonBlocking) == hipSuccess); d.copy_gate.idle.push_back(st.get()); d.copy_streams.push_back(std::move(st)); }
  d.workers.resize(T);
  for (gsv_drain::Worker& w : d.workers) {
    for (auto& set : w.pinned) for (size_t g = 0; g < group; ++g) CHECK(set[g].alloc(chunk * 16, hipHostMallocDefault) == hipSuccess);
    CHECK(w.done.create(hipEventBlockingSync | hipEventDisableTiming) == hipSuccess);
  }
}
// One slice: records [base, base + sum(lengths)) of `streams` in segments of the given lengths, MAC + gc files + checkpoint files
void run_slice(const std::string& dir, const std::vector<std::vector<uint8_t>>& streams, uint64_t total, uint64_t base, const std::vector<uint64_t>& lengths, bool new_pass, uint32_t k,
               size_t group, size_t T, uint64_t chunk, std::vector<CbcMacHost>& macs, bool keep = true) {
  const size_t n_inst = streams.size();
  const uint64_t seg_records = 12, depth = 2;
  std::vector<uint8_t> hashes(16 * n_inst);
  DrainSink sink; sink.hashes = hashes.data(); sink.dir = dir.c_str(); sink.first_index = 40; sink.checkpoint_dir = dir.c_str();
  GcFiles files; CheckpointWriter ckw; std::string failed;
  CHECK(files.open(dir.c_str(), 40, n_inst, new_pass ? "wb" : "ab", &failed));
  CHECK(ckw.open(dir.c_str(), 40, n_inst, new_pass, k, total, &failed) && ckw.on());
  {
    gsv_drain d;
    setup_drain(d, T, group, chunk);
    std::vector<std::vector<uint8_t>> gate(depth, std::vector<uint8_t>(n_inst * size_t(seg_records) * 16 + 16));
    DrainShape shape;
    shape.n_inst = n_inst; shape.group = group; shape.n_workers = T; shape.chunk = chunk; shape.seg_records = seg_records;
    for (auto& g : gate) shape.gate_bufs.push_back(g.data());
    std::atomic<DrainError> err{DrainError::None};
    DrainWorkers workers(&d, shape, sink, macs, files, err, &ckw);
    for (uint64_t n : lengths) {
      CHECK(n <= seg_records);
      (void)workers.wait_buffer();
      uint8_t* buf = gate[workers.next_buffer()].data();
      for (size_t i = 0; i < n_inst; ++i) std::memcpy(buf + i * seg_records * 16, streams[i].data() + base * 16, n * 16);
      workers.push(n, base);
      base += n;
    }
    workers.finish();
    CHECK(workers.error() == DrainError::None);
  }
  CHECK(ckw.flush());
  if (keep) { files.keep(); ckw.keep(); }
}
// the files the workers wrote against the host writer over the gc files they wrote beside them
void compare_with_file_writer(const std::string& dir, const std::vector<std::vector<uint8_t>>& streams, uint32_t k, const std::vector<CbcMacHost>& macs) {
  for (size_t i = 0; i < streams.size(); ++i) {
    const std::string gc = gc_path(dir, 40 + i), ck = CheckpointWriter::path(dir.c_str(), 40 + i), ref = dir + "/ref.mck";
    CHECK(read_file(gc) == streams[i]);
    uint8_t hash[16], got[16]; std::string why;
    CHECK(mac_checkpoints_of_file(gc.c_str(), k, ref.c_str(), hash, &why));
    macs[i].digest(got);
    CHECK(std::memcmp(hash, got, 16) == 0);
    CHECK(read_file(ck) == read_file(ref));
    CHECK(read_file(ck).size() == MacCheckpoints::file_bytes(streams[i].size() / 16, k));
    std::remove(gc.c_str()); std::remove(ck.c_str()); std::remove(ref.c_str());
  }
}
void case_writer(const std::string& dir) {
  // 30 records: segments no multiple of the chunk (3), an empty one, some shorter than a group; groups of 4 chains and of 1; 5 instances: a ragged last group
  for (uint32_t k : {0u, 1u, 2u, 3u, 5u})
    for (size_t group : {size_t(4), size_t(1)}) {
      const auto streams = make_streams(5, 30);
      std::vector<CbcMacHost> macs(5);
      run_slice(dir, streams, 30, 0, {7, 0, 1, 10, 12}, true, k, group, 2, 3, macs);
      compare_with_file_writer(dir, streams, k, macs);
    }
  // two slices over the same MAC states and files, cut inside a group; then a pass that starts again truncates
  for (uint32_t k : {0u, 2u, 4u}) {
    const auto streams = make_streams(3, 29);
    std::vector<CbcMacHost> macs(3);
    run_slice(dir, streams, 29, 0, {5, 6}, true, k, 4, 1, 4, macs);
    run_slice(dir, streams, 29, 11, {12, 0, 6}, false, k, 4, 1, 4, macs);
    compare_with_file_writer(dir, streams, k, macs);
  }
  {  // a failed slice removes its files
    const auto streams = make_streams(2, 10);
    std::vector<CbcMacHost> macs(2);
    run_slice(dir, streams, 10, 0, {10}, true, 1, 1, 1, 4, macs, false);
    CHECK(!exists(CheckpointWriter::path(dir.c_str(), 40)) && !exists(CheckpointWriter::path(dir.c_str(), 41)) && !exists(gc_path(dir, 40)));
    CheckpointWriter w; std::string failed;
    CHECK(!w.open((dir + "/none").c_str(), 3, 2, true, 3, 1000, &failed) && failed == dir + "/none/gc_3.mck");
  }
  {  // the empty stream: a header and nothing else
    CheckpointWriter w; std::string failed;
    CHECK(w.open(dir.c_str(), 7, 1, true, 4, 0, &failed) && w.flush());
    w.keep();
  }
  CHECK(read_file(CheckpointWriter::path(dir.c_str(), 7)).size() == MacCheckpoints::HEADER_BYTES);
  std::remove(CheckpointWriter::path(dir.c_str(), 7).c_str());
}
void case_format(const std::string& dir) {
  const auto streams = make_streams(2, 21);
  const std::string a = dir + "/a.bin", b = dir + "/b.bin", a2 = dir + "/a.k2", b2 = dir + "/b.k2", b3 = dir + "/b.k3", c = dir + "/c.bin", c2 = dir + "/c.k2";
  write_file(a, streams[0]); write_file(b, streams[1]);
  write_file(c, std::vector<uint8_t>(streams[1].begin(), streams[1].begin() + 20 * 16));
  uint8_t h[16]; std::string why;
  CHECK(mac_checkpoints_of_file(a.c_str(), 2, a2.c_str(), h, &why) && mac_checkpoints_of_file(b.c_str(), 2, b2.c_str(), h, &why));
  CHECK(mac_checkpoints_of_file(b.c_str(), 3, b3.c_str(), h, &why) && mac_checkpoints_of_file(c.c_str(), 2, c2.c_str(), h, &why));
  CHECK(!mac_checkpoints_of_file(a.c_str(), 31, nullptr, h, &why));
  std::vector<MacCheckpointFile> files;
  const uint64_t n21 = 21;
  { const char* p[2] = {a2.c_str(), b2.c_str()}; CHECK(open_mac_checkpoints(p, 2, &n21, &files, &why) && files[0].head.k == 2 && files[1].head.states() == 6); }
  { const char* p[2] = {a2.c_str(), b3.c_str()}; why.clear(); CHECK(!open_mac_checkpoints(p, 2, &n21, &files, &why) && why.find("must agree") != std::string::npos && why.find("k = 3") != std::string::npos); }
  { const char* p[2] = {a2.c_str(), c2.c_str()}; why.clear(); CHECK(!open_mac_checkpoints(p, 2, nullptr, &files, &why) && why.find("must agree") != std::string::npos); }
  { const char* p[1] = {c2.c_str()}; why.clear(); CHECK(!open_mac_checkpoints(p, 1, &n21, &files, &why) && why.find("20 records") != std::string::npos); }
  // the host checker, 1 and 3 threads: intact, a flipped record, a flipped state
  for (size_t T : {size_t(1), size_t(3)}) {
    MacCheckpointFile ck; uint64_t bad = 0;
    CHECK(ck.open(a2, &why) && mac_check_file(a.c_str(), ck, T, &bad, &why) && bad == ~0ull);
    std::vector<uint8_t> bytes = streams[0];
    bytes[16 * 9 + 3] ^= 1;
    write_file(a, bytes);
    CHECK(mac_check_file(a.c_str(), ck, T, &bad, &why) && bad == 2);
    write_file(a, streams[0]);
    uint8_t st[16 * 2];
    CHECK(ck.read_states(-1, 2, st) && std::all_of(st, st + 16, [](uint8_t x) { return x == 0; }));
    CHECK(!ck.read_states(5, 2, st));  // past the last state
  }
  for (const std::string& q : {a, b, c, a2, b2, b3, c2}) std::remove(q.c_str());
}

// ---- the kernel's bookkeeping on the host: one "launch" per segment, every chain of every instance, the carries ping-pong ----
struct HostCheck {
  dev::PlainTables T;
  HostCheck() {
    const AesTables& t = AesTables::fixed_key();
    for (int i = 0; i < 4; ++i) T.te[i] = t.te[i];
    T.rkp = t.rk;
  }
  // lowest failing group per stream (~0: none) of `streams` against `states` (per stream: the claimed states, without a header)
  std::vector<uint64_t> run(const std::vector<std::vector<uint8_t>>& streams, const std::vector<std::vector<uint8_t>>& states, uint32_t k, const std::vector<uint64_t>& segments) const {
    const uint64_t total = streams[0].size() / 16;
    std::vector<uint64_t> bad(streams.size(), ~0ull);
    std::vector<dev::Label> carry[2] = {std::vector<dev::Label>(streams.size()), std::vector<dev::Label>(streams.size())};
    int cpar = 0;
    uint64_t first = 0;
    for (uint64_t n : segments) {
      if (n == 0) continue;  // (nothing is launched)
      const uint64_t chains = dev::mac_chain_count(first, n, k);
      for (size_t i = 0; i < streams.size(); ++i) {
        // the slice the host uploads: states (first >> k) - 1 .. (first + n - 1) >> k, the one in front of the stream as zeros
        std::vector<dev::Label> slice(chains + 1, dev::Label{{0, 0, 0, 0}});
        for (uint64_t j = 0; j <= chains; ++j) {
          const int64_t s = int64_t(first >> k) - 1 + int64_t(j);
          if (s >= 0) { CHECK(uint64_t(s) * 16 + 16 <= states[i].size()); std::memcpy(&slice[j], states[i].data() + s * 16, 16); }
        }
        uint64_t covered = 0;
        int carries_written = 0;
        for (uint64_t c = 0; c < chains; ++c) {
          const dev::MacChain m = dev::mac_chain(first, n, k, total, c);
          CHECK(m.lo < m.hi && m.hi <= n && m.lo == covered);  // the chains tile the segment
          CHECK((m.start == dev::MAC_FROM_CARRY) == (c == 0 && (first & ((1ull << k) - 1)) != 0));
          CHECK((m.start == dev::MAC_FROM_ZERO) == (m.group == 0 && first == 0));
          CHECK(m.ends_group || c + 1 == chains);  // only the last chain may leave a carry
          covered = m.hi;
          carries_written += m.ends_group ? 0 : 1;
          const uint8_t* seg = streams[i].data() + first * 16;
          const bool differs = dev::mac_chain_run(T, m, first, k, [seg](uint64_t q) { dev::Label l; std::memcpy(&l, seg + q * 16, 16); return l; }, slice.data(), &carry[cpar][i], &carry[cpar ^ 1][i]);
          if (differs && m.group < bad[i]) bad[i] = m.group;
        }
        CHECK(covered == n && carries_written <= 1);
      }
      cpar ^= 1;
      first += n;
    }
    CHECK(first == total);
    return bad;
  }
};
std::vector<std::vector<uint64_t>> segmentations(uint64_t n, uint32_t k) {
  const uint64_t G = 1ull << k;
  std::vector<std::vector<uint64_t>> v;
  v.push_back({n});
  v.push_back(std::vector<uint64_t>(size_t(n), 1));
  { std::vector<uint64_t> s; for (uint64_t r = n; r;) { const uint64_t m = std::min<uint64_t>(37, r); s.push_back(m); r -= m; } v.push_back(s); }
  if (n >= 2 * G && G > 1) v.push_back({G - 1, G + 1, n - 2 * G});
  return v;
}
void case_bookkeeping() {
  const HostCheck hc;
  for (uint32_t k : {0u, 2u, 6u}) {
    const uint64_t G = 1ull << k;
    for (uint64_t n : {uint64_t(0), uint64_t(1), G - 1, G, G + 1, uint64_t(259), uint64_t(1500)}) {
      const size_t n_streams = 3;
      const auto streams = make_streams(n_streams, n);
      std::vector<std::vector<uint8_t>> states(n_streams);
      for (size_t i = 0; i < n_streams; ++i) {  // the chain states by the serial host MAC
        CbcMacHost mac;
        for (uint64_t r = 0; r < n; ++r) {
          mac.update(streams[i].data() + 16 * r, 1);
          if (((r + 1) & (G - 1)) == 0 || r + 1 == n) { states[i].resize(states[i].size() + 16); mac.digest(states[i].data() + states[i].size() - 16); }
        }
        CHECK(states[i].size() == 16 * MacCheckpoints::state_count(n, k));
      }
      const uint64_t last_group = n ? (n - 1) >> k : 0;
      for (const auto& segs : segmentations(n, k)) {
        const std::vector<uint64_t> none(n_streams, ~0ull);
        CHECK(hc.run(streams, states, k, segs) == none);
        if (n == 0) continue;
        // one corruption at a time, in stream 1: records, then states
        std::vector<uint64_t> recs = {0, G - 1, G, n - 1};
        for (uint64_t r : recs) {
          if (r >= n) continue;
          auto bad_streams = streams;
          bad_streams[1][16 * r + 7] ^= 0x20;
          std::vector<uint64_t> want = none; want[1] = r >> k;
          CHECK(hc.run(bad_streams, states, k, segs) == want);
        }
        for (uint64_t g : {last_group / 2, last_group}) {
          auto bad_states = states;
          bad_states[1][16 * g + 2] ^= 0x04;
          std::vector<uint64_t> want = none; want[1] = g;
          CHECK(hc.run(streams, bad_states, k, segs) == want);
        }
      }
    }
  }
}
}  // namespace

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  case_writer(dir);
  case_format(dir);
  case_bookkeeping();
  if (failures) { std::fprintf(stderr, "mac_checkpoints: %d checks failed\n", failures); return 1; }
  std::printf("mac_checkpoints: ok\n");
  return 0;
}
