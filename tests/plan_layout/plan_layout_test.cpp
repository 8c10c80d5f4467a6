// TEST-ONLY: csrc/engine/plan_layout.hpp alone — the tables a window launch reads (build_plan_layout) on a hand-built plan under the
// retained, windowed, ring and safe layouts, its three error returns, and the parameter policy (plan_sched_params) with one case per
// clamp.  Built with g++ against tests/hip_standin: no HIP runtime, no engine library, no device.
#include "../../garbled_snark_verifier_amd/csrc/engine/plan_layout.hpp"
#include "../hip_standin/hip_standin.hpp"

#include <algorithm>

using namespace gsv;

// ---- (a) the hand-built plan ---------------------------------------------------------------------------------------------------------
// Three unit shapes (only what the tables read of a program: slots, ciphertexts, steps, record form, where its inputs and outputs sit):
//   A  2 inputs -> 1 output, 5 ciphertexts          B  1 -> 1, NO ciphertexts          C  3 -> 2, 9 ciphertexts, and_terms = 4
// Four plan inputs (globals 0..3) feed two chains that never meet: calls 0,2,4,.. over inputs 0,1 and calls 1,3,5,.. over inputs 2,3,
// with constant operands in the C calls.  Plan outputs: the end of each chain, input wire 1, and the constant TRUE.
struct TestPlan {
  Program A, B, C;
  std::vector<std::vector<uint32_t>> ins, outs;
  std::vector<PlanCallView> views;
  uint32_t n_globals = 0, n_inputs = 4;
  std::vector<uint32_t> outputs;
  uint64_t n_gates = 0, n_ct = 0;
  TestPlan() {
    A.n_slots = 10; A.n_ct = 5; A.n_steps = 3; A.n_gates = 7; A.and_terms = 2; A.input_slots = {3, 4}; A.output_slots = {7};
    B.n_slots = 6; B.n_ct = 0; B.n_steps = 1; B.n_gates = 2; B.and_terms = 2; B.input_slots = {3}; B.output_slots = {5};
    C.n_slots = 20; C.n_ct = 9; C.n_steps = 4; C.n_gates = 12; C.and_terms = 4; C.input_slots = {3, 4, 5}; C.output_slots = {10, 11};
    uint32_t next = n_inputs;
    std::vector<const Program*> progs;
    auto call = [&](const Program& p, std::vector<uint32_t> in, size_t n_out) {
      std::vector<uint32_t> out;
      for (size_t i = 0; i < n_out; ++i) out.push_back(next++);
      progs.push_back(&p); ins.push_back(in); outs.push_back(out);
      return out;
    };
    uint32_t a = 0, a2 = 1, b = 2, b2 = 3;  // the live wires of the two chains
    for (int round = 0; round < 2; ++round) {
      a = call(A, {a, a2}, 1)[0];                                   b = call(A, {b, b2}, 1)[0];
      a2 = call(B, {a}, 1)[0];                                      { auto o = call(C, {b, PLAN_WIRE_FALSE, b2}, 2); b = o[0]; b2 = o[1]; }
      { auto o = call(C, {a2, PLAN_WIRE_TRUE, a}, 2); a = o[0]; a2 = o[1]; }  b2 = call(B, {b2}, 1)[0];
    }
    n_globals = next;
    outputs = {a, b, 1, PLAN_WIRE_TRUE};
    views.resize(progs.size());
    for (size_t k = 0; k < progs.size(); ++k) {
      views[k].prog = progs[k];
      views[k].in_globals = PlanCallView::ids(ins[k]); views[k].out_globals = PlanCallView::ids(outs[k]);
      views[k].gid_off = n_gates; views[k].ct_off = n_ct;
      n_gates += progs[k]->n_gates; n_ct += progs[k]->n_ct;
    }
  }
  PlanLayout layout(const SchedParams& sp, bool retain, bool safe, bool withhold) const {
    const std::vector<SchedCall> calls = sched_calls(views);
    Schedule sc = schedule_calls(calls, n_globals, outputs, sp);
    CHECK(verify_schedule(calls, n_globals, outputs, sc).empty());
    PlanLayout L;
    const std::string err = build_plan_layout(views, n_globals, n_inputs, outputs, n_gates, n_ct, std::move(sc), retain, safe, withhold, &L);
    CHECK(err.empty());
    return L;
  }
};

enum Form { RETAINED, WINDOWED, RING };
struct Seen { bool base0 = false, base_other = false, later_window_ct = false, wrapped = false; size_t n_windows = 0, n_deps = 0; };

// every property of the tables that does not depend on which layout it is, and the ct_off form of this one
static Seen check_tables(const TestPlan& tp, const PlanLayout& L, Form form, bool safe, bool withheld) {
  Seen seen;
  const Schedule& sc = L.sched;
  const size_t n = tp.views.size();
  CHECK(L.calls.size() == n && L.copy_src.size() == L.copy_dst.size());
  CHECK(L.global_base % 8 == 0 && L.global_base >= SLOT_FIRST_INPUT && L.global_base >= sc.scratch_slots);
  CHECK(L.retain == (form == RETAINED) && L.ring == (form == RING) && L.safe == safe);
  CHECK(L.max_block == (form == RING ? sc.ring_ct : sc.max_window_ct) && L.max_segment == sc.max_segment_ct);
  // the facade: the wire file's stride, the plan's inputs at the head of the global region, outputs where their wires live (constants at slots 0 / 1)
  CHECK(L.facade.n_slots == L.global_base + tp.n_globals && L.facade.n_gates == tp.n_gates && L.facade.n_ct == tp.n_ct);
  CHECK(L.facade.input_slots.size() == tp.n_inputs);
  for (uint32_t i = 0; i < tp.n_inputs; ++i) CHECK(L.facade.input_slots[i] == L.global_base + i);
  CHECK(L.facade.output_slots.size() == 4 && L.facade.output_slots[0] == L.global_base + tp.outputs[0] && L.facade.output_slots[1] == L.global_base + tp.outputs[1]);
  CHECK(L.facade.output_slots[2] == L.global_base + 1);  // a plan output that is an input wire
  CHECK(L.facade.output_slots[3] == SLOT_TRUE);          // ... that is a constant
  uint32_t widest = 0;
  for (const Schedule::Window& w : sc.windows) widest = std::max(widest, w.call1 - w.call0);
  CHECK(L.flag_stride == widest + 2);
  seen.n_windows = sc.windows.size();
  size_t n_withheld = 0, list_pos = 0, dep_pos = 0;
  for (const Schedule::Window& w : sc.windows) {
    for (uint32_t k = w.call0; k < w.call1; ++k) {
      const dev::CallDesc& d = L.calls[k];
      const PlanCallView& c = tp.views[k];
      const Program& g = *c.prog;
      CHECK(d.ct_pos == nullptr && d.done_host == nullptr && d.steps == nullptr && d.ands == nullptr && d.xors == nullptr);  // the device half's
      CHECK(d.gid_off == c.gid_off && d.w_base == sc.scratch_base[k] && d.n_steps == g.n_steps && d.and_terms == g.and_terms);
      CHECK(d.w_base + g.n_slots <= L.global_base);
      (d.w_base ? seen.base_other : seen.base0) = true;
      // pre: the three constant copies exactly when the region is not the one at slot 0, then one entry per input
      CHECK(d.pre_off == list_pos && d.n_pre == (d.w_base ? SLOT_FIRST_INPUT : 0) + c.in_globals.size());
      uint32_t q = d.pre_off;
      if (d.w_base) for (uint32_t t = 0; t < SLOT_FIRST_INPUT; ++t, ++q) CHECK(L.copy_src[q] == t && L.copy_dst[q] == d.w_base + t);
      for (size_t i = 0; i < c.in_globals.size(); ++i, ++q) {
        const uint32_t w_id = c.in_globals[i];
        CHECK(L.copy_src[q] == (w_id == PLAN_WIRE_FALSE ? SLOT_FALSE : w_id == PLAN_WIRE_TRUE ? SLOT_TRUE : L.global_base + w_id));
        CHECK(L.copy_dst[q] == d.w_base + g.input_slots[i]);
      }
      // post: w_base + output_slots[i] -> global_base + out_globals[i]
      CHECK(d.post_off == q && d.n_post == c.out_globals.size());
      for (size_t i = 0; i < c.out_globals.size(); ++i, ++q) CHECK(L.copy_src[q] == d.w_base + g.output_slots[i] && L.copy_dst[q] == L.global_base + c.out_globals[i]);
      list_pos = q;
      // dependencies: window-relative, every one an EARLIER call of the window (or the one withheld entry)
      CHECK(d.dep_off == dep_pos && d.n_deps == sc.dep_off[k + 1] - sc.dep_off[k]);
      for (uint32_t t = 0; t < d.n_deps; ++t) {
        const uint32_t dep = L.deps[d.dep_off + t];
        if (dep == L.flag_stride - 2) { ++n_withheld; continue; }
        CHECK(dep < k - w.call0 && dep == sc.deps[sc.dep_off[k] + t] - w.call0);
      }
      dep_pos += d.n_deps;
      // the three forms of ct_off
      if (form == RETAINED) CHECK(d.ct_off == c.ct_off && d.ct_need == 0 && d.ct_ready == 0);
      if (form == WINDOWED) { CHECK(d.ct_off == c.ct_off - w.ct0 && d.ct_off + g.n_ct <= L.max_block && d.ct_need == 0 && d.ct_ready == 0); if (w.ct0 && g.n_ct) seen.later_window_ct = true; }
      if (form == RING) { CHECK(d.ct_off == sc.ring_off[k] && d.ct_off + g.n_ct <= L.max_block && d.ct_need == sc.ring_need[k] && d.ct_ready == sc.seg_end[k]); if (d.ct_off < c.ct_off && g.n_ct) seen.wrapped = true; }
    }
  }
  CHECK(list_pos == L.copy_src.size() && dep_pos == L.deps.size());
  CHECK(n_withheld == (withheld ? 1u : 0u));
  seen.n_deps = L.deps.size();
  return seen;
}

static void test_tables() {
  const TestPlan tp;
  CHECK(tp.views.size() == 12 && tp.n_ct == 56);
  for (int withhold = 0; withhold < 2; ++withhold) {
    {  // retained: one window, the stream itself
      SchedParams sp; sp.max_calls_in_flight = 4;
      const Seen s = check_tables(tp, tp.layout(sp, true, false, withhold), RETAINED, false, withhold);
      CHECK(s.n_windows == 1 && s.base0 && s.base_other && s.n_deps > 0);
    }
    {  // windows of at most 15 records: ct_off relative to the window's first record
      SchedParams sp; sp.max_calls_in_flight = 4; sp.max_window_ct = 15;
      const Seen s = check_tables(tp, tp.layout(sp, false, false, withhold), WINDOWED, false, withhold);
      CHECK(s.n_windows > 1 && s.later_window_ct && s.n_deps > 0);
    }
    {  // a ring of 2 segments of 10 + the largest call (9) = 29 records under a stream of 56: ct_off = the block's place in the ring
      SchedParams sp; sp.max_calls_in_flight = 4; sp.segment_ct = 10; sp.ring_ct = 29;
      const Seen s = check_tables(tp, tp.layout(sp, false, false, withhold), RING, false, withhold);
      CHECK(s.n_windows == 1 && s.wrapped && s.n_deps > 0);
    }
    {  // the safe layout: one call per window, no dependency at all — and never a withheld one
      SchedParams sp; sp.max_calls_in_flight = 1; sp.max_window_calls = 1; sp.max_window_ct = 9;
      const PlanLayout L = tp.layout(sp, false, true, withhold);
      const Seen s = check_tables(tp, L, WINDOWED, true, false);
      CHECK(s.n_windows == 12 && s.n_deps == 0 && L.flag_stride == 3 && s.base0 && !s.base_other);
    }
  }
}

// ---- (b) an error leaves the output as it was ------------------------------------------------------------------------------------------
static bool same_program(const Program& a, const Program& b) {
  return a.n_slots == b.n_slots && a.n_gates == b.n_gates && a.n_ct == b.n_ct && a.input_slots == b.input_slots && a.output_slots == b.output_slots && a.n_steps == b.n_steps;
}
static bool same_layout(const PlanLayout& a, const PlanLayout& b) {
  const Schedule &x = a.sched, &y = b.sched;
  return x.windows.size() == y.windows.size() && x.segments.size() == y.segments.size() && x.scratch_base == y.scratch_base && x.dep_off == y.dep_off && x.deps == y.deps && x.ring_ct == y.ring_ct &&
         x.ring_off == y.ring_off && x.scratch_slots == y.scratch_slots && same_program(a.facade, b.facade) && a.global_base == b.global_base && a.retain == b.retain && a.ring == b.ring &&
         a.safe == b.safe && a.max_block == b.max_block && a.max_segment == b.max_segment && a.calls.size() == b.calls.size() &&
         (a.calls.empty() || std::memcmp(a.calls.data(), b.calls.data(), a.calls.size() * sizeof(dev::CallDesc)) == 0) && a.copy_src == b.copy_src && a.copy_dst == b.copy_dst && a.deps == b.deps &&
         a.flag_stride == b.flag_stride;
}
static void test_errors() {
  const TestPlan tp;
  SchedParams sp; sp.max_calls_in_flight = 4; sp.max_window_ct = 15;
  PlanLayout out = tp.layout(sp, false, false, false);  // what a session would hold when a second build fails
  const PlanLayout before = out;
  const dev::CallDesc* const calls_at = out.calls.data();
  const uint32_t* const src_at = out.copy_src.data();
  const std::vector<SchedCall> calls = sched_calls(tp.views);
  SchedParams safe; safe.max_calls_in_flight = 1; safe.max_window_calls = 1;
  auto untouched = [&] { return same_layout(out, before) && out.calls.data() == calls_at && out.copy_src.data() == src_at; };
  // the wire file: scratch + globals must stay below 2^32 - 16 slots
  CHECK(build_plan_layout(tp.views, 0xFFFFFFF0u, tp.n_inputs, tp.outputs, tp.n_gates, tp.n_ct, schedule_calls(calls, tp.n_globals, tp.outputs, safe), false, true, false, &out) == "plan wire file too large");
  CHECK(untouched());
  // a program whose output was left in the LDS window (the compiler pins outputs to the wire file: an internal error)
  {
    TestPlan bad;
    bad.C.output_slots[1] = SLOT_LDS_FLAG | 5;
    const std::vector<SchedCall> bc = sched_calls(bad.views);
    CHECK(build_plan_layout(bad.views, bad.n_globals, bad.n_inputs, bad.outputs, bad.n_gates, bad.n_ct, schedule_calls(bc, bad.n_globals, bad.outputs, safe), false, true, false, &out) ==
          "internal: a program output lives in the LDS window");
    CHECK(untouched());
  }
  // hand-over lists longer than their 32-bit offsets reach (here: than 20 entries — the real limit needs 17 GB of lists)
  CHECK(build_plan_layout(tp.views, tp.n_globals, tp.n_inputs, tp.outputs, tp.n_gates, tp.n_ct, schedule_calls(calls, tp.n_globals, tp.outputs, safe), false, true, false, &out, 20) == "plan hand-over lists too large");
  CHECK(untouched());
  // ... and the same arguments without the small limit succeed and replace it
  CHECK(build_plan_layout(tp.views, tp.n_globals, tp.n_inputs, tp.outputs, tp.n_gates, tp.n_ct, schedule_calls(calls, tp.n_globals, tp.outputs, safe), false, true, false, &out).empty());
  CHECK(out.safe && out.sched.windows.size() == 12 && !same_layout(out, before));
}

// ---- (c) the parameter policy ------------------------------------------------------------------------------------------------------------
static knobs::Sched no_knobs() {  // (the struct reads the environment when constructed: the cases set what they mean)
  knobs::Sched kn;
  kn.plan_concurrency = 0; kn.drain_segment_records = 0; kn.ct_ring_records = 0; kn.ct_ring = false; kn.fault_withhold_dep = false; kn.verify = false;
  return kn;
}
static void test_params() {
  const knobs::Sched kn = no_knobs();
  const int CUS = 256;
  const size_t GB250 = 250000000000ull, GB50 = 50000000000ull;
  const uint64_t STREAM = 3000000000ull, MAX_BLOCK = 1000000;  // records of the whole stream / of the largest call
  const uint32_t MAX_SLOTS = 50000;
  gsv_plan_session_opts o{};
  // 1 instance, retained.  Concurrency = CUs / workgroups = 256 / 1; a retained stream is not drained, so nothing is reserved.  Scratch:
  // 1/16 of the free memory in 16-byte slots = 250e9 / 16 / 16 = 976 562 500 (< 2^30).  Window: the whole stream.  Segment: a tenth of
  // the memory for three buffers = 250e9 * 0.1 / 48 = 520 833 333 records, capped at 2^26.
  o.retain_stream = 1;
  SchedParams p = plan_sched_params(o, 1, 1, CUS, GB250, kn, STREAM, MAX_BLOCK, MAX_SLOTS);
  CHECK(p.max_calls_in_flight == 256 && p.max_scratch_slots == 976562500ull && p.max_window_ct == ~0ull && p.segment_ct == (1ull << 26) && p.ring_ct == 0 && p.max_window_calls == 32768);
  // 1 instance, drained.  256 calls x 1 workgroup + 16 > 256 CUs: 16 CUs are left to the gathers, (256 - 16) / 1 = 240.  Window: 40 % of
  // 250 GB is 100 GB, capped at 48 GB = 3e9 records; segment still 2^26.
  o.retain_stream = 0;
  p = plan_sched_params(o, 1, 1, CUS, GB250, kn, STREAM, MAX_BLOCK, MAX_SLOTS);
  CHECK(p.max_calls_in_flight == 240 && p.max_window_ct == 3000000000ull && p.segment_ct == (1ull << 26) && p.ring_ct == 0);
  // ... with 50 GB free the 40 % rule binds: 20 GB = 1.25e9 records; a tenth of 50 GB / 48 = 104 166 666 is still above 2^26.  Scratch: 50e9 / 256 = 195 312 500.
  p = plan_sched_params(o, 1, 1, CUS, GB50, kn, STREAM, MAX_BLOCK, MAX_SLOTS);
  CHECK(p.max_calls_in_flight == 240 && p.max_window_ct == 1250000000ull && p.segment_ct == (1ull << 26) && p.max_scratch_slots == 195312500ull);
  // 16 instances at 1 per workgroup, drained.  256 / 16 = 16 calls; 16 x 16 + 16 > 256: (256 - 16) / 16 = 15.  Window: 48 GB over 16
  // instances = 187 500 000 records.  Segment: the one-tenth rule binds, 250e9 * 0.1 / 48 / 16 = 32 552 083.  Scratch: 250e9 / 256 / 16 = 61 035 156.
  p = plan_sched_params(o, 16, 1, CUS, GB250, kn, STREAM, MAX_BLOCK, MAX_SLOTS);
  CHECK(p.max_calls_in_flight == 15 && p.max_window_ct == 187500000ull && p.segment_ct == 32552083ull && p.max_scratch_slots == 61035156ull && p.ring_ct == 0);
  // ... retained, the reserve does not apply: 16.
  o.retain_stream = 1;
  p = plan_sched_params(o, 16, 1, CUS, GB250, kn, STREAM, MAX_BLOCK, MAX_SLOTS);
  CHECK(p.max_calls_in_flight == 16 && p.max_window_ct == ~0ull);
  // 1024 instances at 4 per workgroup: 256 workgroups fill the device, ONE call at a time.  A sequential session keeps the one-call
  // block (window = the largest call), a scratch ring of one region, and a segment no larger than its window.
  o.retain_stream = 0;
  p = plan_sched_params(o, 1024, 4, CUS, GB250, kn, STREAM, MAX_BLOCK, MAX_SLOTS);
  CHECK(p.max_calls_in_flight == 1 && p.max_window_ct == MAX_BLOCK && p.max_scratch_slots == MAX_SLOTS && p.segment_ct == MAX_BLOCK && p.ring_ct == 0);
  // ... and so does any session told to run one call at a time (the safe schedule's options), with one call per window
  o.max_concurrent_calls = 1; o.max_window_calls = 1;
  p = plan_sched_params(o, 16, 1, CUS, GB250, kn, STREAM, MAX_BLOCK, MAX_SLOTS);
  CHECK(p.max_calls_in_flight == 1 && p.max_window_ct == MAX_BLOCK && p.max_scratch_slots == MAX_SLOTS && p.max_window_calls == 1);
  // options win over knobs, knobs over the defaults
  {
    knobs::Sched k2 = no_knobs();
    k2.plan_concurrency = 7; k2.drain_segment_records = 2000000;
    gsv_plan_session_opts o2{};
    p = plan_sched_params(o2, 16, 1, CUS, GB250, k2, STREAM, MAX_BLOCK, MAX_SLOTS);
    CHECK(p.max_calls_in_flight == 7 && p.segment_ct == 2000000);  // (7 x 16 + 16 <= 256: no reserve to take)
    o2.max_concurrent_calls = 5; o2.drain_segment_records = 3000000; o2.max_scratch_slots = 123456; o2.window_ct_records = 5000000;
    p = plan_sched_params(o2, 16, 1, CUS, GB250, k2, STREAM, MAX_BLOCK, MAX_SLOTS);
    CHECK(p.max_calls_in_flight == 5 && p.segment_ct == 3000000 && p.max_scratch_slots == 123456 && p.max_window_ct == 5000000);
  }
  // The ring: three segments (3 x 32 552 083 = 97 656 249 records, more than 2 segments + the largest call), taken only when it is
  // asked for, no window_ct_records was given, calls run side by side, and the ring is shorter than the stream (and fits the window)
  gsv_plan_session_opts r{};
  r.retain_stream = GSV_STREAM_RING;
  p = plan_sched_params(r, 16, 1, CUS, GB250, kn, STREAM, MAX_BLOCK, MAX_SLOTS);
  CHECK(p.ring_ct == 97656249ull && p.max_window_ct == ~0ull && p.segment_ct == 32552083ull && p.max_calls_in_flight == 15);
  {
    knobs::Sched k2 = no_knobs();
    k2.ct_ring = true;  // GSV_CT_RING=1 asks for it on behalf of a retain_stream = 0 session ...
    gsv_plan_session_opts o2{};
    CHECK(plan_sched_params(o2, 16, 1, CUS, GB250, k2, STREAM, MAX_BLOCK, MAX_SLOTS).ring_ct == 97656249ull);
    o2.retain_stream = 1;  // ... never of one that retains its stream
    CHECK(plan_sched_params(o2, 16, 1, CUS, GB250, k2, STREAM, MAX_BLOCK, MAX_SLOTS).ring_ct == 0);
    k2.ct_ring_records = 70000000;  // GSV_CT_RING_RECORDS: the ring's size, never below 2 segments + the largest call = 66 104 166
    CHECK(plan_sched_params(r, 16, 1, CUS, GB250, k2, STREAM, MAX_BLOCK, MAX_SLOTS).ring_ct == 70000000ull);
    k2.ct_ring_records = 1000;
    CHECK(plan_sched_params(r, 16, 1, CUS, GB250, k2, STREAM, MAX_BLOCK, MAX_SLOTS).ring_ct == 66104166ull);
  }
  gsv_plan_session_opts none{};  // not asked for
  CHECK(plan_sched_params(none, 16, 1, CUS, GB250, kn, STREAM, MAX_BLOCK, MAX_SLOTS).ring_ct == 0);
  gsv_plan_session_opts sized = r;  // the caller sizes the launches
  sized.window_ct_records = 100000000;
  p = plan_sched_params(sized, 16, 1, CUS, GB250, kn, STREAM, MAX_BLOCK, MAX_SLOTS);
  CHECK(p.ring_ct == 0 && p.max_window_ct == 100000000);
  gsv_plan_session_opts seq = r;  // one call at a time
  seq.max_concurrent_calls = 1;
  CHECK(plan_sched_params(seq, 16, 1, CUS, GB250, kn, STREAM, MAX_BLOCK, MAX_SLOTS).ring_ct == 0);
  p = plan_sched_params(r, 16, 1, CUS, GB250, kn, 97656249ull, MAX_BLOCK, MAX_SLOTS);  // the whole stream fits the ring
  CHECK(p.ring_ct == 0 && p.max_window_ct == 187500000ull);
  CHECK(plan_sched_params(r, 16, 1, CUS, GB250, kn, 97656250ull, MAX_BLOCK, MAX_SLOTS).ring_ct == 97656249ull);  // ... one record more does not
}

int main() {
  test_tables();
  test_errors();
  test_params();
  if (failures) { std::fprintf(stderr, "plan_layout: %d check(s) failed\n", failures); return 1; }
  std::printf("plan_layout: ok (4 layouts with and without a withheld dependency, 3 errors, the parameter policy)\n");
  return 0;
}
