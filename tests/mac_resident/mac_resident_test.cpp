// TEST-ONLY (tests/test_mac_resident_standalone.py): the CBC-MAC check of a stream that lies in PROGRAM order, and of a stream that is
// evaluated in slices, without a device.
//   * the indexed accessor (csrc/engine/cbcmac_device.hpp: MacIndexedPos) against the gathered stream: random n_ct, position tables,
//     replay counts, range sizes and k; per range every chain runs twice through mac_chain_run with PlainTables — once over the
//     gate-order copy with the plain accessor, once over the program-order block through the position table — and must give the same
//     verdict and the same carry.  Clean streams, then one corrupted record, then one corrupted state.
//   * save and restore of the check's host-side state (csrc/engine/mac_checkpoints.hpp: MacCheckPosition) with the carries, in the
//     middle of a stream: going on after a restore equals never having stopped — also after a detour over corrupted records.
//   * which sets of commitments a streaming evaluation may ask for, and which slice may follow which (csrc/engine/drain_pipeline.hpp:
//     EvalCommit, eval_commit_refusal), as plain values: all 128 x 128 pairs against the rule written out on bit masks.
// No thread starts, no HIP call is made.
#include "../../garbled_snark_verifier_amd/csrc/engine/drain_pipeline.hpp"
#include "../../garbled_snark_verifier_amd/csrc/engine/cbcmac_device.hpp"
#include "../hip_standin/hip_standin.hpp"

#include <random>

using namespace gsv;

namespace {
using Label = dev::Label;
struct Tables {
  dev::PlainTables T;
  Tables() {
    const AesTables& t = AesTables::fixed_key();
    for (int i = 0; i < 4; ++i) T.te[i] = t.te[i];
    T.rkp = t.rk;
  }
};
Label label_of(std::mt19937_64& rng) { Label l; for (auto& w : l.w) w = uint32_t(rng()); return l; }
bool same(const Label& a, const Label& b) { return std::memcmp(&a, &b, 16) == 0; }

// the claimed states of a gate-order stream, by the serial host MAC
std::vector<Label> states_of(const std::vector<Label>& gate, uint32_t k) {
  const uint64_t G = 1ull << k, n = gate.size();
  std::vector<Label> st;
  CbcMacHost mac;
  for (uint64_t r = 0; r < n; ++r) {
    mac.update(reinterpret_cast<const uint8_t*>(&gate[r]), 1);
    if (((r + 1) & (G - 1)) == 0 || r + 1 == n) { st.emplace_back(); mac.digest(reinterpret_cast<uint8_t*>(&st.back())); }
  }
  CHECK(st.size() == MacCheckpoints::state_count(n, k));
  return st;
}
// the slice of a segment as the host uploads it: states (first >> k) - 1 .. (first + n - 1) >> k, the one in front of the stream as zeros
std::vector<Label> slice_of(const std::vector<Label>& states, uint64_t first, uint64_t n, uint32_t k) {
  const uint64_t chains = dev::mac_chain_count(first, n, k);
  std::vector<Label> slice(chains + 1, Label{{0, 0, 0, 0}});
  for (uint64_t j = 0; j <= chains; ++j) {
    const int64_t s = int64_t(first >> k) - 1 + int64_t(j);
    if (s >= 0) { CHECK(uint64_t(s) < states.size()); slice[j] = states[size_t(s)]; }
  }
  return slice;
}

// One stream of `replays` x n_ct records: `block` in program order, `gate` the same records in gate order.
struct Resident {
  uint64_t n_ct, replays;
  std::vector<uint32_t> ct_pos;
  std::vector<Label> block, gate;
  Resident(std::mt19937_64& rng, uint64_t n_ct_, uint64_t replays_) : n_ct(n_ct_), replays(replays_), ct_pos(n_ct_), block(n_ct_ * replays_), gate(n_ct_ * replays_) {
    for (uint64_t g = 0; g < n_ct; ++g) ct_pos[g] = uint32_t(g);
    std::shuffle(ct_pos.begin(), ct_pos.end(), rng);
    for (auto& l : block) l = label_of(rng);
    gather();
  }
  void gather() { for (uint64_t r = 0; r < replays; ++r) for (uint64_t g = 0; g < n_ct; ++g) gate[r * n_ct + g] = block[r * n_ct + ct_pos[g]]; }
};
// The stream range by range (`cap` records at most), both accessors side by side.  Returns the lowest failing group (~0: none).
uint64_t run_both(const Tables& tb, const Resident& s, const std::vector<Label>& states, uint32_t k, uint64_t cap) {
  const uint64_t total = s.gate.size();
  uint64_t bad = ~0ull;
  Label carry_a[2] = {}, carry_b[2] = {};
  MacCheckPosition pos;
  for (uint64_t first = 0; first < total; first += cap) {
    const uint64_t n = std::min(cap, total - first);
    const std::vector<Label> slice = slice_of(states, first, n, k);
    for (uint64_t c = 0; c < dev::mac_chain_count(first, n, k); ++c) {
      const dev::MacChain m = dev::mac_chain(first, n, k, total, c);
      const Label* seg = s.gate.data() + first;
      const bool da = dev::mac_chain_run(tb.T, m, first, k, [seg](uint64_t q) { return seg[q]; }, slice.data(), &carry_a[pos.cpar], &carry_a[pos.cpar ^ 1]);
      dev::MacIndexedPos at(s.ct_pos.data(), s.n_ct);
      const Label* block = s.block.data();
      const bool db = dev::mac_chain_run(tb.T, m, first, k, [block, first, at](uint64_t q) mutable { return block[at.at(first + q)]; }, slice.data(), &carry_b[pos.cpar], &carry_b[pos.cpar ^ 1]);
      CHECK(da == db);
      if (!m.ends_group) CHECK(same(carry_a[pos.cpar ^ 1], carry_b[pos.cpar ^ 1]));
      if (da && m.group < bad) bad = m.group;
    }
    pos.advance(n);
  }
  CHECK(pos.records_done == total);
  return bad;
}
void case_indexed() {
  const Tables tb;
  std::mt19937_64 rng(20261021);
  for (int round = 0; round < 60; ++round) {
    const uint64_t n_ct = 1 + rng() % 97, replays = 1 + rng() % 9, total = n_ct * replays;
    const uint32_t k = uint32_t(rng() % 8);
    const uint64_t cap = round % 5 == 0 ? total : 1 + rng() % (total + 3);
    Resident s(rng, n_ct, replays);
    // the position: any order of requests gives the mapping the header documents
    dev::MacIndexedPos at(s.ct_pos.data(), n_ct);
    for (int j = 0; j < 50; ++j) { const uint64_t q = rng() % total; CHECK(at.at(q) == (q / n_ct) * n_ct + s.ct_pos[q % n_ct]); }
    for (uint64_t q = 0; q < total; ++q) CHECK(s.block[at.at(q)].w[0] == s.gate[q].w[0]);
    const std::vector<Label> states = states_of(s.gate, k);
    CHECK(run_both(tb, s, states, k, cap) == ~0ull);
    // one record of the BLOCK changed: the group of its gate position
    const uint64_t q = rng() % total;
    Resident t = s;
    t.block[(q / n_ct) * n_ct + s.ct_pos[q % n_ct]].w[1] ^= 0x400u;
    t.gather();
    CHECK(run_both(tb, t, states, k, cap) == q >> k);
    // one claimed state changed: that group (and the next one starts from it, so the lowest is reported)
    std::vector<Label> wrong = states;
    const uint64_t g = rng() % states.size();
    wrong[g].w[3] ^= 1u;
    CHECK(run_both(tb, s, wrong, k, cap) == g);
  }
}

// ---- the check in segments with its state saved and restored, as a sliced evaluation does it at a restart point ----
struct HostStream {
  MacCheckPosition pos;
  Label carry[2] = {};
  uint64_t bad = ~0ull;
  void feed(const Tables& tb, const std::vector<Label>& gate, const std::vector<Label>& states, uint32_t k, uint64_t n) {
    const uint64_t first = pos.records_done, total = gate.size();
    const std::vector<Label> slice = slice_of(states, first, n, k);
    const Label* seg = gate.data() + first;
    for (uint64_t c = 0; c < dev::mac_chain_count(first, n, k); ++c) {
      const dev::MacChain m = dev::mac_chain(first, n, k, total, c);
      if (dev::mac_chain_run(tb.T, m, first, k, [seg](uint64_t q) { return seg[q]; }, slice.data(), &carry[pos.cpar], &carry[pos.cpar ^ 1]) && m.group < bad) bad = m.group;
    }
    pos.advance(n);
  }
};
void case_restore() {
  const Tables tb;
  std::mt19937_64 rng(7);
  for (int round = 0; round < 40; ++round) {
    const uint64_t total = 40 + rng() % 400;
    const uint32_t k = uint32_t(rng() % 7);
    std::vector<Label> gate(total);
    for (auto& l : gate) l = label_of(rng);
    const std::vector<Label> states = states_of(gate, k);
    std::vector<uint64_t> segs;
    for (uint64_t left = total; left;) { const uint64_t n = 1 + rng() % std::min<uint64_t>(left, 61); segs.push_back(n); left -= n; }
    HostStream straight;
    for (uint64_t n : segs) straight.feed(tb, gate, states, k, n);
    CHECK(straight.bad == ~0ull && straight.pos.records_done == total && straight.pos.fed == segs.size());
    // stop in front of segment `cut`, go on over corrupted records (a failing slice), restore, go on over the repaired ones
    const size_t cut = rng() % segs.size();
    HostStream h;
    for (size_t j = 0; j < cut; ++j) h.feed(tb, gate, states, k, segs[j]);
    const MacCheckPosition saved_pos = h.pos;
    const Label saved_carry[2] = {h.carry[0], h.carry[1]};
    CHECK(h.bad == ~0ull);  // (a restart point is taken between slices: no group has failed)
    std::vector<Label> damaged = gate;
    const uint64_t r = saved_pos.records_done + rng() % (total - saved_pos.records_done);
    damaged[r].w[2] ^= 0x10000u;
    for (size_t j = cut; j < segs.size(); ++j) h.feed(tb, damaged, states, k, segs[j]);
    CHECK(h.bad == r >> k);
    h.pos = saved_pos; h.carry[0] = saved_carry[0]; h.carry[1] = saved_carry[1]; h.bad = ~0ull;  // roll_back: the carries, the position, the words all ones
    for (size_t j = cut; j < segs.size(); ++j) h.feed(tb, gate, states, k, segs[j]);
    CHECK(h.bad == ~0ull);
    CHECK(h.pos.cpar == straight.pos.cpar && h.pos.records_done == straight.pos.records_done && h.pos.fed == straight.pos.fed);
    CHECK(same(h.carry[0], straight.carry[0]) && same(h.carry[1], straight.carry[1]));
  }
}

// ---- what a streaming evaluation may ask for ----
const char* const CHECKPOINTS_ALONE = "a streaming evaluation verified against CBC-MAC checkpoints computes no other commitment and takes no other kind of verification";
const char* const SAME_AS_FIRST = "every slice of a streaming evaluation must ask for the same commitments and the same kind of verification as its first slice";
bool same_text(const char* got, const char* want) { return got == nullptr ? want == nullptr : want != nullptr && std::strcmp(got, want) == 0; }
void case_commit_rules() {
  CHECK(unsigned(EvalCommit::Mac) == 1 && unsigned(EvalCommit::B3) == 2 && unsigned(EvalCommit::VerifiedFiles) == 4 && unsigned(EvalCommit::VerifiedUpFront) == 8 &&
        unsigned(EvalCommit::VerifiedDeferred) == 16 && unsigned(EvalCommit::CheckpointFiles) == 32 && unsigned(EvalCommit::CheckpointMemory) == 64);
  for (unsigned first = 0; first < 128; ++first)
    for (unsigned now = 0; now < 128; ++now)
      for (int first_slice = 0; first_slice < 2; ++first_slice) {
        const char* want = nullptr;
        if ((now & 96u) && now != 32u && now != 64u) want = CHECKPOINTS_ALONE;  // with a MAC, a digest, a BLAKE3 kind, or both checkpoint kinds at once
        else if (!first_slice && first != now) want = SAME_AS_FIRST;
        CHECK(same_text(eval_commit_refusal(EvalCommit(first), EvalCommit(now), first_slice != 0), want));
      }
  // the cases by name: files then memory, verified then not, a BLAKE3 pass then checkpoints
  CHECK(same_text(eval_commit_refusal(EvalCommit::CheckpointFiles, EvalCommit::CheckpointMemory, false), SAME_AS_FIRST));
  CHECK(same_text(eval_commit_refusal(EvalCommit::CheckpointFiles, EvalCommit::Mac, false), SAME_AS_FIRST));
  CHECK(same_text(eval_commit_refusal(EvalCommit::B3 | EvalCommit::VerifiedFiles, EvalCommit::CheckpointFiles, false), SAME_AS_FIRST));
  CHECK(same_text(eval_commit_refusal(EvalCommit::None, EvalCommit::CheckpointFiles | EvalCommit::Mac, true), CHECKPOINTS_ALONE));
  CHECK(eval_commit_refusal(EvalCommit::CheckpointFiles, EvalCommit::CheckpointFiles, false) == nullptr);
  CHECK(eval_commit_refusal(EvalCommit::Mac, EvalCommit::CheckpointMemory, true) == nullptr);  // (a new pass asks what it likes)
}
}  // namespace

int main() {
  case_indexed();
  case_restore();
  case_commit_rules();
  if (failures) { std::fprintf(stderr, "mac_resident: %d checks failed\n", failures); return 1; }
  std::printf("mac_resident: ok\n");
  return 0;
}
