// TEST-ONLY (tests/test_b3_restart.py): the host half of a restart point of a sliced, verified evaluation — B3Check's position
// (position / rewind) and the per-instance hashers (Blake3Host, kept by value) — saved in the middle of a stream, advanced, restored and
// advanced again.  The device half is modelled on the host as B3Stream keeps it (engine_blake3.ipp): the records of the chunk that is
// still open (the carry), the chunk values of the group that is still open (pending), the count of chunks done; the last chunk is never
// reduced, it is hashed as bytes at the end.  Real outboards (outboard_of_file over temporary files), three streams, uneven segments.
// Every save point is tried, among them ones taken while a group is open and while chunk values are pending; the advance behind a save
// runs over a tampered stream until the comparison stops it, as the evaluation a restart point exists for does.  No HIP, no device.
// main() returns non-zero when a check fails.
#include "../../garbled_snark_verifier_amd/csrc/engine/outboard.hpp"

#include <unistd.h>

#include <fstream>

using namespace gsv;

namespace {
int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

constexpr size_t N_INST = 3;
using Streams = std::vector<std::vector<uint8_t>>;

// what a restart point holds for the streams of one pass
struct Receiver {
  uint32_t k = 0;
  uint64_t total = 0, dev_chunks = 0, chunks_done = 0, records_done = 0;
  std::vector<uint8_t> carry[N_INST], pending[N_INST];  // open chunk (bytes), open group (chunk values)
  Blake3Host hashers[N_INST];
  uint64_t position = 0;  // B3Check::position()
  void begin(uint32_t k_, uint64_t total_) { *this = Receiver(); k = k_; total = total_; dev_chunks = Outboard::chunks(total_) - 1; }
  bool group_open() const { return !pending[0].empty(); }
  // records [records_done, records_done + n) of every stream; false: the comparison stopped the pass (check holds the place)
  bool feed(const Streams& s, uint64_t n, B3Check& check) {
    check.rewind(position);
    std::vector<uint8_t> groups[N_INST];
    for (size_t i = 0; i < N_INST; ++i) {
      carry[i].insert(carry[i].end(), s[i].begin() + records_done * 16, s[i].begin() + (records_done + n) * 16);
      uint64_t done = chunks_done;
      size_t used = 0;
      while (carry[i].size() - used >= 1024 && done < dev_chunks) {
        uint8_t cv[32];
        outboard_chunk_value(carry[i].data() + used, done++, cv);
        used += 1024;
        pending[i].insert(pending[i].end(), cv, cv + 32);
        if (pending[i].size() == (size_t(32) << k)) { outboard_reduce_group(pending[i].data(), k); groups[i].insert(groups[i].end(), pending[i].begin(), pending[i].begin() + 32); pending[i].clear(); }
      }
      carry[i].erase(carry[i].begin(), carry[i].begin() + used);
      if (i + 1 == N_INST) chunks_done = done;
    }
    records_done += n;
    const uint32_t g = uint32_t(groups[0].size() / 32);
    std::vector<uint8_t> dense(N_INST * size_t(g) * 32 + 1);
    for (size_t i = 0; i < N_INST; ++i) { CHECK(groups[i].size() == size_t(g) * 32); if (g) std::memcpy(dense.data() + i * g * 32, groups[i].data(), size_t(g) * 32); }
    if (!check.groups_match(dense.data(), g)) return false;
    position = check.position();
    for (size_t i = 0; i < N_INST; ++i) for (uint32_t q = 0; q < g; ++q) CHECK(hashers[i].absorb_subtree(groups[i].data() + 32 * q, k));
    return true;
  }
  // the end of the streams: pending chunk values compared and absorbed, the last chunk hashed; false: mismatch
  bool finish(B3Check& check, uint8_t digests[N_INST][32]) {
    check.rewind(position);
    CHECK(records_done == total);
    const uint32_t pend = uint32_t(pending[0].size() / 32);
    std::vector<uint8_t> dense(N_INST * size_t(pend) * 32 + 1);
    for (size_t i = 0; pend && i < N_INST; ++i) std::memcpy(dense.data() + i * pend * 32, pending[i].data(), size_t(pend) * 32);
    if (!check.pending_match(dense.data(), pend)) return false;
    for (size_t i = 0; i < N_INST; ++i) {
      for (uint32_t q = 0; q < pend; ++q) CHECK(hashers[i].absorb_subtree(pending[i].data() + 32 * q, 0));
      if (!carry[i].empty()) hashers[i].update(carry[i].data(), carry[i].size());
      CHECK(hashers[i].finalize(digests[i]));
    }
    return true;
  }
};

void case_stream(const std::string& dir, uint32_t k, uint64_t total, const std::vector<uint64_t>& segments, bool want_open_group, bool want_pending_at_end) {
  Streams clean(N_INST, std::vector<uint8_t>(size_t(total) * 16));
  B3Check check;
  check.shape(N_INST, k, total);
  uint8_t want[N_INST][32];
  for (size_t i = 0; i < N_INST; ++i) {
    for (size_t j = 0; j < clean[i].size(); ++j) clean[i][j] = uint8_t(j * 131 + (j >> 8) * 7 + i * 29);
    const std::string gc = dir + "/gc.bin";
    { std::ofstream f(gc, std::ios::binary); f.write(reinterpret_cast<const char*>(clean[i].data()), std::streamsize(clean[i].size())); }
    std::vector<uint8_t> last;
    std::string why;
    CHECK(outboard_of_file(gc.c_str(), k, &check.bytes[i], &last, &why));
    std::remove(gc.c_str());
    Blake3Host h;
    h.update(clean[i].data(), clean[i].size());
    CHECK(h.finalize(want[i]));  // the digest of the bytes themselves
  }
  CHECK(check.holds(N_INST, k, total) && !check.holds(N_INST, k + 1, total) && !check.holds(N_INST + 1, k, total));
  uint64_t sum = 0;
  for (uint64_t n : segments) sum += n;
  CHECK(sum == total);
  // the straight run: the position behind every segment, the digests
  std::vector<uint64_t> straight;
  uint8_t got[N_INST][32];
  Receiver r;
  r.begin(k, total);
  for (uint64_t n : segments) { CHECK(r.feed(clean, n, check)); straight.push_back(r.position); }
  CHECK(r.group_open() == want_pending_at_end);
  CHECK(r.finish(check, got) && std::memcmp(got, want, sizeof got) == 0);
  // a save behind every segment j (j = 0: in front of the first), the advance behind it over a stream with one flipped bit
  bool saw_open_group = false, saw_open_chunk = false;
  for (size_t j = 0; j <= segments.size(); ++j) {
    Receiver a;
    a.begin(k, total);
    for (size_t q = 0; q < j; ++q) CHECK(a.feed(clean, segments[q], check) && a.position == straight[q]);
    const Receiver saved = a;  // the restart point
    saw_open_group = saw_open_group || (saved.group_open() && j < segments.size());
    saw_open_chunk = saw_open_chunk || !saved.carry[0].empty();
    // tampered: one bit of instance 1, in the first record behind the save (behind the last segment nothing is left to tamper with)
    Streams bad = clean;
    const uint64_t record = std::min(saved.records_done, total - 1);
    if (j < segments.size()) bad[1][record * 16 + 5] ^= 0x08;
    bool stopped = false;
    for (size_t q = j; q < segments.size() && !stopped; ++q) stopped = !a.feed(bad, segments[q], check);
    uint8_t other[N_INST][32];
    if (!stopped) stopped = !a.finish(check, other);
    if (j == segments.size()) CHECK(!stopped && std::memcmp(other, want, sizeof other) == 0);
    else if (stopped) {
      CHECK(check.bad_instance == 1 && check.bad_record <= record && record < check.bad_record + (uint64_t(64) << k));
      // a group that began in front of the save: the restart point of the slice before is the one to go back to
      if (check.bad_record < saved.records_done) CHECK(saved.group_open() || !saved.carry[0].empty());
    } else {
      // nothing the outboard covers was touched: the flipped bit lies in the last chunk, and only the digest tells
      CHECK(record >= (Outboard::chunks(total) - 1) * 64 && std::memcmp(other[1], want[1], 32) != 0 && std::memcmp(other[0], want[0], 32) == 0);
    }
    // restored, advanced again over the clean stream: the straight run's positions and digests
    Receiver b = saved;
    CHECK(b.position == (j ? straight[j - 1] : 0));
    for (size_t q = j; q < segments.size(); ++q) CHECK(b.feed(clean, segments[q], check) && b.position == straight[q]);
    uint8_t again[N_INST][32];
    CHECK(b.finish(check, again) && std::memcmp(again, want, sizeof again) == 0);
    // ... and once more from the same restart point (a repeat that fails again leaves it usable)
    Receiver c = saved;
    for (size_t q = j; q < segments.size(); ++q) CHECK(c.feed(clean, segments[q], check));
    CHECK(c.finish(check, again) && std::memcmp(again, want, sizeof again) == 0);
  }
  CHECK(saw_open_group == want_open_group && saw_open_chunk);
}
}  // namespace

int main() {
  char tmpl[] = "/tmp/gsv_b3_restart_XXXXXX";
  const char* made = mkdtemp(tmpl);
  if (!made) { std::perror("mkdtemp"); return 3; }
  const std::string dir = made;
  // 1 665 records: 27 chunks, at k = 2 six groups, two pending chunk values and a last chunk of one record
  case_stream(dir, 2, 1665, {100, 37, 259, 64, 1, 700, 504}, true, true);
  case_stream(dir, 2, 1665, {256, 256, 512, 641}, false, true);   // saves on group boundaries only; the pending values at the end
  case_stream(dir, 0, 1665, {100, 37, 259, 64, 1, 700, 504}, false, false);  // k = 0: a group is a chunk, none is ever open behind a segment
  case_stream(dir, 1, 775, {214, 208, 187, 166}, true, false);    // the small plan's windows: 12 chunks in six groups of two
  case_stream(dir, 2, 64, {64}, false, false);                    // one chunk: nothing but the last chunk
  CHECK(::rmdir(dir.c_str()) == 0);
  if (failures) return 1;
  std::printf("b3_restart: ok\n");
  return 0;
}
