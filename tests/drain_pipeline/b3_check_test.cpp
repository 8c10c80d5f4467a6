// TEST-ONLY (tests/test_b3_check.py): the receiver's side of the BLAKE3 outboards, B3Check and check_outboard / load_outboard of
// csrc/engine/outboard.hpp, alone: which (instance, group) a stream that differs from its outboard is blamed on, and which outboards
// are refused before a pass.  The outboards are real ones (outboard_of_file over temporary files); the "device's" values are the
// outboards' own, fed dense [instance][group] as a segment leaves them.  No HIP, no device.  main() returns non-zero when a check fails.
#include "../../garbled_snark_verifier_amd/csrc/engine/outboard.hpp"

#include <unistd.h>

#include <fstream>

using namespace gsv;

namespace {
int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

constexpr size_t N_INST = 3;
struct Streams {
  uint32_t k; uint64_t n_records;
  std::vector<uint8_t> ob[N_INST];
  std::string ob_path[N_INST];
  B3Check check;
  // values [first, first + count) of every instance, dense, as they sit in the page-locked buffer
  std::vector<uint8_t> dense(uint64_t first, uint32_t count) const {
    std::vector<uint8_t> a(N_INST * size_t(count) * 32 + 1);  // (+1: never empty)
    for (size_t i = 0; i < N_INST; ++i) std::memcpy(a.data() + i * count * 32, ob[i].data() + Outboard::HEADER_BYTES + 32 * first, size_t(count) * 32);
    return a;
  }
  static void flip(std::vector<uint8_t>& a, uint32_t count, size_t inst, uint32_t v) { a[(inst * count + v) * 32 + 5] ^= 0x40; }
};
// three streams of distinct content, their outboards written by the host writer and loaded back as a receiver loads them
void make(const std::string& dir, uint32_t k, uint64_t n_records, Streams* s) {
  s->k = k; s->n_records = n_records;
  s->check = B3Check();
  s->check.shape(N_INST, k, n_records);
  for (size_t i = 0; i < N_INST; ++i) {
    const std::string gc = dir + "/gc_" + std::to_string(i) + ".bin";
    std::vector<uint8_t> stream(size_t(n_records) * 16), last;
    for (size_t j = 0; j < stream.size(); ++j) stream[j] = uint8_t(j * 131 + (j >> 8) * 7 + i * 29);
    { std::ofstream f(gc, std::ios::binary); f.write(reinterpret_cast<const char*>(stream.data()), std::streamsize(stream.size())); }
    std::string why;
    CHECK(outboard_of_file(gc.c_str(), k, &s->ob[i], &last, &why));
    s->ob_path[i] = dir + "/gc_" + std::to_string(i) + ".b3o";
    { std::ofstream f(s->ob_path[i], std::ios::binary); f.write(reinterpret_cast<const char*>(s->ob[i].data()), std::streamsize(s->ob[i].size())); }
    CHECK(load_outboard(s->ob_path[i], k, n_records, &s->check.bytes[i], &why) && s->check.bytes[i] == s->ob[i]);
    std::remove(gc.c_str());
  }
}
void cleanup(const Streams& s) { for (const std::string& p : s.ob_path) std::remove(p.c_str()); }

void case_stream(const std::string& dir, uint32_t k, uint64_t n_records, uint64_t want_chunks, uint64_t want_groups, uint64_t want_pending) {
  Streams s;
  make(dir, k, n_records, &s);
  B3Check& c = s.check;
  const uint64_t G = want_groups;
  CHECK(Outboard::chunks(n_records) == want_chunks && c.n_groups == G && c.n_pending == want_pending && c.k == k && c.n_records == n_records);
  // 1. uneven batches, then the pending chunk values: everything matches
  {
    const uint32_t sizes[] = {1, 3, 2};
    uint64_t g = 0;
    for (size_t b = 0; g < G; ++b) {
      const uint32_t n = uint32_t(std::min<uint64_t>(sizes[b % 3], G - g));
      CHECK(c.groups_match(s.dense(g, n).data(), n));
      g += n;
      CHECK(c.next == g);
    }
    CHECK(c.groups_match(s.dense(0, 0).data(), 0));  // (a segment without a complete group)
    CHECK(c.pending_match(s.dense(G, uint32_t(want_pending)).data(), uint32_t(want_pending)));
    // 2. one group more than the outboard holds: instance 0 at group n_groups
    c.bad_instance = 9;
    const std::vector<uint8_t> extra(N_INST * 32, 0);
    CHECK(!c.groups_match(extra.data(), 1) && c.bad_instance == 0 && c.bad_group == G && c.bad_record == (G << k) * 64);
    // 3. a wrong count of pending chunk values is refused
    c.bad_instance = 9;
    CHECK(!c.pending_match(s.dense(G, uint32_t(want_pending)).data(), uint32_t(want_pending) + 1) && c.bad_instance == 0 && c.bad_group == G && c.bad_record == (G << k) * 64);
    // 4. reset(): the streams start again from group 0
    c.reset();
    CHECK(c.next == 0);
    if (G) CHECK(c.groups_match(s.dense(0, uint32_t(G)).data(), uint32_t(G)) && c.next == G);
  }
  // 5. the pending values before all groups have arrived: blamed on group `next`
  if (G >= 2) {
    c.reset();
    CHECK(c.groups_match(s.dense(0, 1).data(), 1));
    c.bad_instance = 9;
    CHECK(!c.pending_match(s.dense(G, uint32_t(want_pending)).data(), uint32_t(want_pending)) && c.bad_instance == 0 && c.bad_group == 1 && c.bad_record == (1ull << k) * 64);
  }
  // 6. flips at (instance 1, group 3) and (instance 0, group 4) in one batch: the lowest group wins
  if (G >= 5) {
    c.reset();
    std::vector<uint8_t> v = s.dense(0, uint32_t(G));
    Streams::flip(v, uint32_t(G), 1, 3); Streams::flip(v, uint32_t(G), 0, 4);
    CHECK(!c.groups_match(v.data(), uint32_t(G)) && c.bad_instance == 1 && c.bad_group == 3 && c.bad_record == (3ull << k) * 64);
    CHECK(c.where("file") == "file 1 does not match its outboard in group 3 (from record " + std::to_string((3ull << k) * 64) + ")");
    CHECK(c.where("the ciphertext stream of instance") == "the ciphertext stream of instance 1 does not match its outboard in group 3 (from record " + std::to_string((3ull << k) * 64) + ")");
    CHECK(c.next == 0);  // (nothing of a batch that differs counts as compared)
    // ... and in batches: groups 0 .. 1 pass, the batch of groups 2 .. 4 is blamed on (1, 3)
    CHECK(c.groups_match(s.dense(0, 2).data(), 2));
    std::vector<uint8_t> w = s.dense(2, 3);
    Streams::flip(w, 3, 1, 1); Streams::flip(w, 3, 0, 2);
    CHECK(!c.groups_match(w.data(), 3) && c.bad_instance == 1 && c.bad_group == 3 && c.bad_record == (3ull << k) * 64);
  }
  // 7. two instances flipped in the same group: the lower instance
  if (G >= 3) {
    c.reset();
    std::vector<uint8_t> v = s.dense(0, uint32_t(G));
    Streams::flip(v, uint32_t(G), 2, 2); Streams::flip(v, uint32_t(G), 1, 2);
    CHECK(!c.groups_match(v.data(), uint32_t(G)) && c.bad_instance == 1 && c.bad_group == 2 && c.bad_record == (2ull << k) * 64);
  }
  // 8. a flipped pending value c: group n_groups, the record the chunk starts at
  if (want_pending >= 2) {
    c.reset();
    if (G) CHECK(c.groups_match(s.dense(0, uint32_t(G)).data(), uint32_t(G)));
    std::vector<uint8_t> v = s.dense(G, uint32_t(want_pending));
    Streams::flip(v, uint32_t(want_pending), 2, 1);
    CHECK(!c.pending_match(v.data(), uint32_t(want_pending)) && c.bad_instance == 2 && c.bad_group == G && c.bad_record == ((G << k) + 1) * 64);
    CHECK(c.where("file") == "file 2 does not match its outboard in group " + std::to_string(G) + " (from record " + std::to_string(((G << k) + 1) * 64) + ")");
  }
  cleanup(s);
}

// check_outboard: what is refused, which refusal comes first, and that the message names both sides
void case_refusals(const std::string& dir) {
  Streams s;
  make(dir, 2, 1665, &s);
  const std::vector<uint8_t>& ob = s.ob[1];
  std::string why;
  CHECK(check_outboard("outboards[1]", ob.data(), ob.size(), 2, 1665, &why));
  // 1. another n_records — in front of another k and a length that is off
  CHECK(!check_outboard("outboards[1]", ob.data(), ob.size() - 1, 3, 1664, &why));
  CHECK(why == "outboards[1] is the outboard of a stream of 1665 records, the stream here holds 1664");
  // 2. another k — in front of a length that is off
  CHECK(!check_outboard("outboards[1]", ob.data(), ob.size() - 1, 3, 1665, &why));
  CHECK(why == "outboards[1] was written for groups of 2^2 chunks, this pass reduces groups of 2^3 (GSV_B3_SUBTREE_LOG2)");
  // 3. a length off by one byte, either way
  const uint64_t want = Outboard::file_bytes(1665, 2);
  CHECK(ob.size() == want && want == 24 + 32 * 8);
  CHECK(!check_outboard("outboards[1]", ob.data(), ob.size() - 1, 2, 1665, &why));
  CHECK(why == "outboards[1]: the outboard holds " + std::to_string(want - 1) + " bytes, but k = 2 and n_records = 1665 make " + std::to_string(want));
  std::vector<uint8_t> longer(ob); longer.push_back(0);
  CHECK(!check_outboard("outboards[1]", longer.data(), longer.size(), 2, 1665, &why));
  CHECK(why == "outboards[1]: the outboard holds " + std::to_string(want + 1) + " bytes, but k = 2 and n_records = 1665 make " + std::to_string(want));
  // 4. a buffer shorter than the header
  CHECK(!check_outboard("outboards[1]", ob.data(), 23, 2, 1665, &why));
  CHECK(why == "outboards[1]: the outboard is shorter than its 24-byte header");
  // load_outboard: the same refusals under the file's path; a file longer than the stream's outboard is not read to its end
  CHECK(!load_outboard(s.ob_path[1], 2, 1664, &s.check.bytes[1], &why) && why == s.ob_path[1] + " is the outboard of a stream of 1665 records, the stream here holds 1664");
  CHECK(!load_outboard(dir + "/none.b3o", 2, 1665, &s.check.bytes[1], &why) && why == "cannot open " + dir + "/none.b3o");
  { std::ofstream f(s.ob_path[2], std::ios::binary | std::ios::app); f.write("\0\0\0", 3); }
  CHECK(!load_outboard(s.ob_path[2], 2, 1665, &s.check.bytes[2], &why));
  CHECK(why == s.ob_path[2] + ": the outboard holds " + std::to_string(want + 1) + " bytes, but k = 2 and n_records = 1665 make " + std::to_string(want));
  cleanup(s);
}
}  // namespace

int main() {
  char tmpl[] = "/tmp/gsv_b3_check_XXXXXX";
  const char* made = mkdtemp(tmpl);
  if (!made) { std::perror("mkdtemp"); return 3; }
  const std::string dir = made;
  //                     records chunks groups pending
  case_stream(dir, 2, 1665, 27, 6, 2);  // the layered fixture's shape
  case_stream(dir, 2, 775, 13, 3, 0);
  case_stream(dir, 2, 64, 1, 0, 0);     // no values at all
  case_stream(dir, 2, 0, 1, 0, 0);
  case_stream(dir, 0, 1665, 27, 26, 0);  // k = 0: every chunk value is a group value
  case_stream(dir, 0, 775, 13, 12, 0);
  case_stream(dir, 0, 64, 1, 0, 0);
  case_stream(dir, 0, 0, 1, 0, 0);
  case_refusals(dir);
  CHECK(::rmdir(dir.c_str()) == 0);  // nothing was left behind
  if (failures) return 1;
  std::printf("b3_check: ok\n");
  return 0;
}
