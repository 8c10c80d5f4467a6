// TEST-ONLY (tests/test_commit_rules.py): what a garbling pass may combine, csrc/engine/drain_pipeline.hpp alone — DrainSink::commit(),
// DrainSink::refusal() over every combination of the nine destinations, a ring and a pair; commit_slice_conflict over every pair of
// flag sets.  The expected answers are worked out here on bit masks from the rules as DrainSink's field comments state them ("needs
// b3", "needs hashes", "nothing leaves the device and no MAC worker starts"), the texts are the engine's of before the rules had one
// home, as literals.  No thread starts, no HIP call is made.
#include "../../garbled_snark_verifier_amd/csrc/engine/drain_pipeline.hpp"
#include "../hip_standin/hip_standin.hpp"

using namespace gsv;

namespace {
// (hip_standin.hpp counts in `failures`; this form names the case)
#define EXPECT(cond, ...) do { if (!(cond)) { if (++failures <= 20) { std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

const char* const NEEDS_B3_OUTBOARD = "an outboard holds the values of the BLAKE3 commitment: blake3_digests must be given";
const char* const NEEDS_B3_LAST = "the last chunks come with the BLAKE3 commitment: blake3_digests must be given";
const char* const NEEDS_HASHES = "checkpoint files hold the states of the CBC-MAC: hashes must be given";
const char* const NOT_OVER_A_RING = "CBC-MAC checkpoints are not written or checked over a ciphertext ring (retain_stream = GSV_STREAM_RING): create the session with launch windows";
const char* const RUNS_ALONE = "internal: the CBC-MAC check runs alone";
const char* const SAME_B3 = "every slice of a pass with a BLAKE3 commitment must ask for the same commitments as its first slice";
const char* const SAME_MCK = "every slice of a pass that writes or checks CBC-MAC checkpoints must ask for the same as its first slice";

enum : unsigned { HASHES = 1, DIR = 2, FN = 4, B3 = 8, OB_DIR = 16, OB_FN = 32, LAST = 64, CKPT = 128, CHECK = 256, ALL = 512 };
int a_sink(void*, size_t, uint64_t, const uint8_t*, uint64_t) { return 0; }
bool same(const char* got, const char* want) { return got == nullptr ? want == nullptr : want != nullptr && std::strcmp(got, want) == 0; }
const char* show(const char* s) { return s ? s : "(null)"; }

DrainSink sink_of(unsigned m) {
  static uint8_t buf[1024];
  DrainSink k;
  if (m & HASHES) k.hashes = buf;
  if (m & DIR) k.dir = "/nowhere";
  if (m & FN) k.fn = a_sink;
  if (m & B3) k.b3 = buf;
  if (m & OB_DIR) k.outboard_dir = "/nowhere";
  if (m & OB_FN) k.ob_fn = a_sink;
  if (m & LAST) k.last_chunks = buf;
  if (m & CKPT) k.checkpoint_dir = "/nowhere";
  if (m & CHECK) k.mac_check_dir = "/nowhere";
  return k;
}
// the rules in the order the engine has always reported them
const char* want_refusal(unsigned m, bool ring, bool paired) {
  if ((m & (OB_DIR | OB_FN)) && !(m & B3)) return NEEDS_B3_OUTBOARD;            // outboard_dir, ob_fn: "needs b3"
  if ((m & LAST) && !(m & B3)) return NEEDS_B3_LAST;                            // last_chunks: "needs b3"
  if ((m & CKPT) && !(m & HASHES)) return NEEDS_HASHES;                         // checkpoint_dir: "needs hashes"
  if ((m & (CKPT | CHECK)) && ring) return NOT_OVER_A_RING;
  if ((m & CHECK) && ((m & (HASHES | DIR | FN | B3)) || paired)) return RUNS_ALONE;  // "nothing leaves the device and no MAC worker starts"
  return nullptr;
}

void sink_rules() {
  unsigned refused = 0;
  for (unsigned m = 0; m < ALL; ++m) {
    const DrainSink k = sink_of(m);
    const unsigned flags = ((m & HASHES) ? 1 : 0) | ((m & B3) ? 2 : 0) | ((m & (OB_DIR | OB_FN)) ? 4 : 0) | ((m & CHECK) ? 8 : 0) | ((m & CKPT) ? 16 : 0);
    EXPECT(unsigned(k.commit()) == flags, "destinations %#x: commit() = %u, expected %u", m, unsigned(k.commit()), flags);
    EXPECT(has(k.commit(), PassCommit::Mac) == ((m & HASHES) != 0) && has(k.commit(), PassCommit::B3) == ((m & B3) != 0) && has(k.commit(), PassCommit::Outboard) == ((m & (OB_DIR | OB_FN)) != 0) &&
              has(k.commit(), PassCommit::MacCheck) == ((m & CHECK) != 0) && has(k.commit(), PassCommit::Checkpoints) == ((m & CKPT) != 0), "destinations %#x: the named flags", m);
    for (int ring = 0; ring < 2; ++ring)
      for (int paired = 0; paired < 2; ++paired) {
        const char* const want = want_refusal(m, ring != 0, paired != 0);
        const char* const got = k.refusal(ring != 0, paired != 0);
        EXPECT(same(got, want), "destinations %#x, ring %d, paired %d: \"%s\", expected \"%s\"", m, ring, paired, show(got), show(want));
        refused += want != nullptr;
      }
    // the two rules an entry point checks on its own arguments are the first two of the whole list
    const char* const first = want_refusal(m, false, false);
    const char* const want_b3 = first == NEEDS_B3_OUTBOARD || first == NEEDS_B3_LAST ? first : nullptr;
    EXPECT(same(k.b3_refusal(), want_b3), "destinations %#x: b3_refusal() = \"%s\", expected \"%s\"", m, show(k.b3_refusal()), show(want_b3));
  }
  EXPECT(refused > 1000 && refused < 4 * ALL, "%u of %u cases refused", refused, 4 * ALL);  // (both outcomes occur)
}

void slice_rules() {
  const unsigned B3_BIT = 2, MCK_BITS = 8 | 16;
  for (unsigned a = 0; a < 32; ++a)
    for (unsigned b = 0; b < 32; ++b) {
      const char* want = nullptr;
      if (a != b && ((a | b) & B3_BIT)) want = SAME_B3;
      else if (a != b && ((a | b) & MCK_BITS)) want = SAME_MCK;
      const char* const got = commit_slice_conflict(PassCommit(a), PassCommit(b));
      EXPECT(same(got, want), "first slice %u, this slice %u: \"%s\", expected \"%s\"", a, b, show(got), show(want));
    }
  // the numbering the table above uses is the named one
  EXPECT(unsigned(PassCommit::Mac) == 1 && unsigned(PassCommit::B3) == 2 && unsigned(PassCommit::Outboard) == 4 && unsigned(PassCommit::MacCheck) == 8 && unsigned(PassCommit::Checkpoints) == 16, "flag values");
  EXPECT(commit_slice_conflict(PassCommit::Mac, PassCommit::None) == nullptr, "a pass of MACs alone may drop them");
}
}  // namespace

int main() {
  sink_rules();
  slice_rules();
  if (failures) { std::printf("commit_rules: %d check(s) failed\n", failures); return 1; }
  std::printf("commit_rules: ok (2048 sink cases, 1024 slice pairs)\n");
  return 0;
}
