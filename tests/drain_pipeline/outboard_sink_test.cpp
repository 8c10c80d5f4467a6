// TEST-ONLY (tests/test_outboard_sink.py): the two back ends of the drain-side outboard writer, OutboardWriter of
// csrc/engine/drain_pipeline.hpp — gc_<i>.b3o files and the host callback (gsv_outboard_sink_fn) — driven side by side as
// garble_streaming_pass drives them: the header when the writer is opened, group values through the B3Absorbers' threads, the pending
// chunk values from the pass's own thread.  The values are real ones, computed with the host code of csrc/engine/outboard.hpp from
// streams made here, so that what both back ends deliver can also be compared with the host writer's outboard of the same stream.
// The hip* functions the header calls are the stand-ins of tests/hip_standin/hip_standin.hpp; no HIP runtime is linked, no device is
// needed.  main() returns non-zero when a check fails.
#include "../../garbled_snark_verifier_amd/csrc/engine/drain_pipeline.hpp"
#include "../hip_standin/hip_standin.hpp"

#include <sys/stat.h>
#include <unistd.h>

#include <fstream>
#include <iterator>

using namespace gsv;

namespace {
std::vector<uint8_t> read_file(const std::string& p) { std::ifstream f(p, std::ios::binary); return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>()); }
bool exists(const std::string& p) { struct stat sb; return ::stat(p.c_str(), &sb) == 0; }

// the stream of instance `inst`: n_records x 16 bytes
std::vector<uint8_t> stream_of(size_t inst, uint64_t n_records) {
  std::vector<uint8_t> a(size_t(n_records) * 16);
  uint32_t x = 0x9e3779b9u * uint32_t(inst + 1) + uint32_t(n_records);
  for (uint8_t& b : a) { x = x * 1664525u + 1013904223u; b = uint8_t(x >> 24); }
  return a;
}
// The values the host receives for one stream, in order: the group values, then the pending chunk values
struct Values { std::vector<uint8_t> groups, pending; uint64_t n_groups = 0, n_pending = 0; };
Values values_of(const std::vector<uint8_t>& stream, uint32_t k) {
  Values v;
  const uint64_t n_records = stream.size() / 16, dev_chunks = Outboard::chunks(n_records) - 1, G = 1ull << k;
  v.n_groups = dev_chunks >> k; v.n_pending = dev_chunks & (G - 1);
  std::vector<uint8_t> group;
  for (uint64_t c = 0; c < dev_chunks; ++c) {
    uint8_t cv[32];
    outboard_chunk_value(stream.data() + 1024 * c, c, cv);
    group.insert(group.end(), cv, cv + 32);
    if (group.size() == G * 32) { outboard_reduce_group(group.data(), k); v.groups.insert(v.groups.end(), group.begin(), group.begin() + 32); group.clear(); }
  }
  v.pending = group;
  return v;
}
// values [first, first + count) of every instance's `which` list, [instance][value] dense: what a segment leaves in the page-locked buffer
std::vector<uint8_t> dense(const std::vector<Values>& vals, bool pending, uint64_t first, uint32_t count) {
  std::vector<uint8_t> a;
  for (const Values& v : vals) { const std::vector<uint8_t>& src = pending ? v.pending : v.groups; a.insert(a.end(), src.begin() + 32 * first, src.begin() + 32 * (first + count)); }
  return a;
}

// The host's side of the callback: appends, and notes everything the contract forbids
struct Collector {
  std::vector<std::vector<uint8_t>> got;
  std::vector<std::atomic<int>> busy;
  std::atomic<int> calls{0}, bad_offset{0}, overlapped{0}, bad_instance{0};
  int fail_at_call = -1;         // the call (counted over all instances) that returns non-zero
  explicit Collector(size_t n) : got(n), busy(n) { for (auto& b : busy) b = 0; }
  static int fn(void* user, size_t inst, uint64_t off, const uint8_t* bytes, uint64_t n) {
    Collector& c = *static_cast<Collector*>(user);
    const int call = c.calls++;
    if (inst >= c.got.size()) { ++c.bad_instance; return 1; }
    if (c.busy[inst].exchange(1) != 0) ++c.overlapped;
    int rc = 0;
    if (call == c.fail_at_call) rc = 1;
    else {
      if (off != c.got[inst].size()) ++c.bad_offset;
      c.got[inst].insert(c.got[inst].end(), bytes, bytes + n);
    }
    c.busy[inst] = 0;
    return rc;
  }
  bool clean() const { return !bad_offset && !overlapped && !bad_instance; }
};

// One call of the drain over `vals`: group values [g0, g1) in submissions of `step` through T absorber threads, then (ends_pass) the
// pending chunk values from this thread, flush and keep — or, after an error, neither.
struct Pass {
  OutboardWriter w;
  std::atomic<DrainError> err{DrainError::None};
  bool run(const std::vector<Values>& vals, size_t T, uint64_t g0, uint64_t g1, uint32_t step, bool ends_pass) {
    {
      B3Absorbers absorbers(T, [this](const uint8_t* v, uint32_t groups, size_t t, size_t n) {
        if (!w.append(v, groups, t, n)) drain_set_error(err, w.to_callback() ? DrainError::OutboardSink : DrainError::FileWrite);
        return true;
      }, err);
      for (uint64_t g = g0; g < g1; g += step) {
        const uint32_t m = uint32_t(std::min<uint64_t>(step, g1 - g));
        std::vector<uint8_t> pinned = dense(vals, false, g, m);
        absorbers.submit(pinned.data(), pinned.size(), m);
        std::fill(pinned.begin(), pinned.end(), 0xEE);  // the next segment's copy lands there
      }
      absorbers.finish();
    }
    if (err != DrainError::None) return false;
    if (ends_pass) {
      const uint32_t pend = uint32_t(vals[0].n_pending);
      const std::vector<uint8_t> p = dense(vals, true, 0, pend);
      if (pend && !w.append(p.data(), pend, 0, 1)) return false;
    }
    if (!w.flush()) return false;
    w.keep();
    return true;
  }
};

// 1. callback bytes == file bytes == the host writer's outboard, for every length and k
void case_lengths(const std::string& dir) {
  const size_t n_inst = 3;
  for (uint32_t k : {0u, 2u})
    for (uint64_t n_records : {0ull, 1ull, 64ull, 65ull, 256ull, 257ull, 320ull, 1665ull}) {
      std::vector<Values> vals;
      for (size_t i = 0; i < n_inst; ++i) vals.push_back(values_of(stream_of(i, n_records), k));
      const uint64_t G = vals[0].n_groups;
      { Pass p; std::string failed; CHECK(p.w.open(dir.c_str(), 0, n_inst, true, k, n_records, &failed) && !p.w.to_callback()); CHECK(p.run(vals, 2, 0, G, 2, true)); }
      Collector c(n_inst);
      { Pass p; CHECK(p.w.open(&Collector::fn, &c, n_inst, true, k, n_records, 0) && p.w.to_callback() && p.w.size() == n_inst); CHECK(p.run(vals, 2, 0, G, 2, true)); CHECK(!p.w.callback_failed()); }
      CHECK(c.clean());
      for (size_t i = 0; i < n_inst; ++i) {
        const std::vector<uint8_t> file = read_file(OutboardWriter::path(dir.c_str(), i));
        CHECK(c.got[i] == file);
        CHECK(file.size() == Outboard::file_bytes(n_records, k));
        const std::string gc = dir + "/gc_" + std::to_string(i) + ".bin";
        const std::vector<uint8_t> s = stream_of(i, n_records);
        { std::ofstream f(gc, std::ios::binary); f.write(reinterpret_cast<const char*>(s.data()), std::streamsize(s.size())); }
        std::vector<uint8_t> ob, last; std::string why;
        CHECK(outboard_of_file(gc.c_str(), k, &ob, &last, &why) && ob == c.got[i]);
        Outboard o; uint8_t root[32], want[32];
        CHECK(Outboard::parse(c.got[i].data(), c.got[i].size(), &o, &why) && o.root(last.data(), last.size(), root, &why));
        Blake3Host h; h.update(s.data(), s.size()); CHECK(h.finalize(want) && std::memcmp(root, want, 32) == 0);
        std::remove(gc.c_str());
        std::remove(OutboardWriter::path(dir.c_str(), i).c_str());
      }
    }
}
// 2. two slices: the header once, the second slice's offsets go on where the first one's ended; files append likewise
void case_slices(const std::string& dir) {
  const size_t n_inst = 3;
  const uint32_t k = 2;
  const uint64_t n_records = 1665;  // six groups, two pending chunk values
  std::vector<Values> vals;
  for (size_t i = 0; i < n_inst; ++i) vals.push_back(values_of(stream_of(i, n_records), k));
  { Pass p; std::string failed; CHECK(p.w.open(dir.c_str(), 0, n_inst, true, k, n_records, &failed)); CHECK(p.run(vals, 3, 0, 4, 3, false)); }
  { Pass p; std::string failed; CHECK(p.w.open(dir.c_str(), 0, n_inst, false, k, n_records, &failed)); CHECK(p.run(vals, 3, 4, 6, 1, true)); }
  Collector c(n_inst);
  { Pass p; CHECK(p.w.open(&Collector::fn, &c, n_inst, true, k, n_records, 0)); CHECK(p.run(vals, 3, 0, 4, 3, false)); }
  for (size_t i = 0; i < n_inst; ++i) CHECK(c.got[i].size() == Outboard::HEADER_BYTES + 32 * 4);
  const int calls_before = c.calls;
  { Pass p; CHECK(p.w.open(&Collector::fn, &c, n_inst, false, k, n_records, 4)); CHECK(c.calls == calls_before); CHECK(p.run(vals, 3, 4, 6, 1, true)); }  // (no second header)
  CHECK(c.clean());
  for (size_t i = 0; i < n_inst; ++i) {
    CHECK(c.got[i] == read_file(OutboardWriter::path(dir.c_str(), i)) && c.got[i].size() == Outboard::file_bytes(n_records, k));
    CHECK(std::memcmp(c.got[i].data(), Outboard::MAGIC, 8) == 0 && std::memcmp(c.got[i].data() + Outboard::HEADER_BYTES, vals[i].groups.data(), 32 * 6) == 0);
  }
  // a slice that starts the pass again starts every outboard at offset 0 again: a host that keeps the old bytes sees the wrong offset
  { Pass p; CHECK(p.w.open(&Collector::fn, &c, n_inst, true, k, n_records, 0)); }
  CHECK(c.bad_offset == int(n_inst));
  for (size_t i = 0; i < n_inst; ++i) std::remove(OutboardWriter::path(dir.c_str(), i).c_str());
}
// 3. a sample drain: two of three instances leave the device, the third is never mentioned
void case_subset(const std::string& dir) {
  const uint32_t k = 0;
  const uint64_t n_records = 320;  // four values, no pending ones at k = 0
  std::vector<Values> vals;
  for (size_t i = 0; i < 2; ++i) vals.push_back(values_of(stream_of(i, n_records), k));
  { Pass p; std::string failed; CHECK(p.w.open(dir.c_str(), 5, 2, true, k, n_records, &failed)); CHECK(p.run(vals, 4, 0, 4, 4, true)); }
  Collector c(3);
  { Pass p; CHECK(p.w.open(&Collector::fn, &c, 2, true, k, n_records, 0)); CHECK(p.run(vals, 4, 0, 4, 4, true)); }
  CHECK(c.clean() && c.got[2].empty() && !exists(OutboardWriter::path(dir.c_str(), 7)));
  for (size_t i = 0; i < 2; ++i) { CHECK(c.got[i] == read_file(OutboardWriter::path(dir.c_str(), 5 + i))); std::remove(OutboardWriter::path(dir.c_str(), 5 + i).c_str()); }
}
// 4. a callback that fails: the pass fails with the outboard sink's error and nothing further is delivered, to any instance; a refused
// header fails the open
void case_callback_failure() {
  const size_t n_inst = 3;
  const uint32_t k = 2;
  const uint64_t n_records = 1665;
  std::vector<Values> vals;
  for (size_t i = 0; i < n_inst; ++i) vals.push_back(values_of(stream_of(i, n_records), k));
  Collector c(n_inst);
  c.fail_at_call = 4;  // three headers, one delivery, then the refusal
  {
    Pass p;
    CHECK(p.w.open(&Collector::fn, &c, n_inst, true, k, n_records, 0));
    CHECK(!p.run(vals, 1, 0, 6, 1, true));  // (one absorber thread: the order of the calls is the order of the instances)
    CHECK(p.err == DrainError::OutboardSink && p.w.callback_failed());
    CHECK(c.calls == 5);
    const std::vector<uint8_t> more = dense(vals, true, 0, 2);
    CHECK(!p.w.append(more.data(), 2, 0, 1) && c.calls == 5);  // the pending values of a failed pass go nowhere
  }
  CHECK(c.clean() && c.got[0].size() == Outboard::HEADER_BYTES + 32 && c.got[1].size() == Outboard::HEADER_BYTES && c.got[2].size() == Outboard::HEADER_BYTES);
  Collector d(n_inst);
  d.fail_at_call = 1;
  { OutboardWriter w; CHECK(!w.open(&Collector::fn, &d, n_inst, true, k, n_records, 0) && w.callback_failed() && d.calls == 2); }
}
// 5. file mode: a failed call — the object goes away without keep() — still removes its files
void case_file_failure(const std::string& dir) {
  const size_t n_inst = 2;
  std::vector<Values> vals;
  for (size_t i = 0; i < n_inst; ++i) vals.push_back(values_of(stream_of(i, 1665), 2));
  {
    Pass p; std::string failed;
    CHECK(p.w.open(dir.c_str(), 20, n_inst, true, 2, 1665, &failed));
    drain_set_error(p.err, DrainError::Copy);  // (what a failing copy of the same pass leaves in the shared slot)
    CHECK(!p.run(vals, 2, 0, 6, 2, true));
    CHECK(exists(OutboardWriter::path(dir.c_str(), 20)) && exists(OutboardWriter::path(dir.c_str(), 21)));
  }
  CHECK(!exists(OutboardWriter::path(dir.c_str(), 20)) && !exists(OutboardWriter::path(dir.c_str(), 21)));
  { OutboardWriter w; std::string failed; CHECK(!w.open((dir + "/none").c_str(), 3, 2, true, 2, 1665, &failed) && failed == dir + "/none/gc_3.b3o"); }
}
}  // namespace

int main() {
  char tmpl[] = "/tmp/gsv_outboard_sink_XXXXXX";
  const char* made = mkdtemp(tmpl);
  if (!made) { std::perror("mkdtemp"); return 3; }
  const std::string dir = made;
  case_lengths(dir);
  case_slices(dir);
  case_subset(dir);
  case_callback_failure();
  case_file_failure(dir);
  CHECK(::rmdir(dir.c_str()) == 0);  // nothing was left behind
  if (failures) return 1;
  std::printf("outboard_sink: ok\n");
  return 0;
}
