// Everything of a plan session that depends on its SCHEDULE, as host values with no device in sight: the parameter policy that turns the
// session's options, the device's size and the schedule knobs into SchedParams (plan_sched_params), and the tables a window launch reads —
// the wire-file layout (scratch regions in front of the global wires), the facade program, one dev::CallDesc per call, the wire hand-over
// lists, the window-relative dependency lists (build_plan_layout).  Pure arithmetic: no HIP function is called, so the host interpreter
// (tests/hostsim) executes these very tables on the CPU and tests/plan_layout checks them alone.  The device half — allocation, upload,
// the mapped counters — is gsv_session::PlanState (engine_internal.hpp, make_plan_state).
#pragma once
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/gsv_engine.h"
#include "kernel_api.h"
#include "knobs.hpp"
#include "plan_builder.hpp"
#include "program.hpp"
#include "schedule.hpp"

namespace gsv {

// What the tables need from one call of the plan.
struct PlanCallView {
  struct Ids {  // global wire ids (PLAN_WIRE_FALSE / PLAN_WIRE_TRUE: the constants)
    const uint32_t* p = nullptr; size_t n = 0;
    size_t size() const { return n; }
    const uint32_t* data() const { return p; }
    uint32_t operator[](size_t i) const { return p[i]; }
  };
  static Ids ids(const std::vector<uint32_t>& v) { return Ids{v.data(), v.size()}; }
  const Program* prog = nullptr;  // the program that runs: the variant for the session's instances per workgroup
  Ids in_globals, out_globals;
  uint64_t gid_off = 0, ct_off = 0;  // gate ids / ciphertext records consumed by the calls before this one
  const void *steps = nullptr, *ands = nullptr, *xors = nullptr;  // the program's image on the device (opaque here; null in host tests)
};
// the scheduler's view of the same calls (schedule.hpp)
inline std::vector<SchedCall> sched_calls(const std::vector<PlanCallView>& views) {
  std::vector<SchedCall> calls(views.size());
  for (size_t k = 0; k < views.size(); ++k) {
    const PlanCallView& c = views[k];
    const Program& g = *c.prog;
    calls[k].in = c.in_globals.data(); calls[k].n_in = c.in_globals.size();
    calls[k].out = c.out_globals.data(); calls[k].n_out = c.out_globals.size();
    calls[k].n_slots = g.n_slots; calls[k].n_ct = g.n_ct; calls[k].n_steps = g.n_steps;
  }
  return calls;
}

// The schedule-dependent host state of a plan session, one value: built whole by build_plan_layout, never edited afterwards.
struct PlanLayout {
  Schedule sched;
  Program facade;            // stands in for the program: slots = wire-file stride, inputs / outputs in the global region
  uint32_t global_base = 0;  // first slot of the plan's global region
  bool retain = true;        // whole ciphertext stream kept on the device (else one block: streaming only)
  bool ring = false;         // the device block is a ring of max_block records (schedule.hpp, SchedParams::ring_ct)
  bool safe = false;         // the safe schedule: ONE call per launch, no dependency waits on the device
  uint64_t max_block = 0;    // ciphertext records per instance of the device block: the largest WINDOW of the schedule, or the ring
  uint64_t max_segment = 0;  // ... of a gate-order buffer: the largest drain SEGMENT (schedule.hpp)
  // the tables of the window launches, in stream order: call descriptors (ct_pos / done_host null: the device half patches them in), the
  // concatenated wire hand-over lists (globals -> the call's scratch region -> globals), the dependency lists (window-relative call indices)
  std::vector<dev::CallDesc> calls;
  std::vector<uint32_t> copy_src, copy_dst, deps;
  uint32_t flag_stride = 0;  // completion flags per instance group: the widest window + a slot nobody writes + the group's progress counter
};

// The tables of `sc` over the calls of a plan.  Returns an empty string and assigns *out, or the error; *out is then untouched.
// withhold_first_dep (GSV_FAULT_WITHHOLD_DEP=1, tests): see below; never for the safe schedule.  max_list: entries a hand-over list may
// hold (offsets into it are 32 bits; tests/plan_layout passes a small one to meet the error).
inline std::string build_plan_layout(const std::vector<PlanCallView>& calls, uint32_t n_globals, uint32_t n_inputs, const std::vector<uint32_t>& outputs, uint64_t n_gates, uint64_t n_ct,
                                     Schedule schedule, bool retain, bool safe, bool withhold_first_dep, PlanLayout* out, uint64_t max_list = 0xFFFFFF00ull) {
  PlanLayout L;
  L.sched = std::move(schedule);
  const Schedule& sc = L.sched;
  const uint32_t scratch = uint32_t((std::max<uint64_t>(sc.scratch_slots, SLOT_FIRST_INPUT) + 7) / 8 * 8);
  L.global_base = scratch;
  L.retain = retain;
  L.safe = safe;
  L.ring = sc.ring_ct != 0;
  L.max_block = L.ring ? sc.ring_ct : sc.max_window_ct;
  L.max_segment = sc.max_segment_ct;
  if (uint64_t(scratch) + n_globals > 0xFFFFFFF0ull) return "plan wire file too large";
  Program& f = L.facade;
  f.n_slots = scratch + n_globals;
  f.n_gates = n_gates; f.n_ct = n_ct;
  for (uint32_t i = 0; i < n_inputs; ++i) f.input_slots.push_back(scratch + i);
  auto global_slot = [&](uint32_t w) -> uint32_t { return w == PLAN_WIRE_FALSE ? SLOT_FALSE : w == PLAN_WIRE_TRUE ? SLOT_TRUE : scratch + w; };
  for (uint32_t w : outputs) f.output_slots.push_back(global_slot(w));
  // descriptors, wire hand-over lists and dependency lists, all in stream order
  {
    const size_t n = calls.size();
    std::vector<dev::CallDesc>& cds = L.calls;
    cds.resize(n);
    std::vector<uint32_t>&csrc = L.copy_src, &cdst = L.copy_dst, &deps = L.deps;
    for (const Schedule::Window& w : sc.windows) {
      for (uint32_t k = w.call0; k < w.call1; ++k) {
        const PlanCallView& c = calls[k];
        const Program& g = *c.prog;
        const uint32_t base = sc.scratch_base[k];
        dev::CallDesc& d = cds[k];
        std::memset(&d, 0, sizeof d);
        d.steps = c.steps; d.ands = c.ands; d.xors = c.xors;
        d.gid_off = c.gid_off; d.ct_off = L.retain ? c.ct_off : L.ring ? sc.ring_off[k] : c.ct_off - w.ct0;
        if (L.ring) { d.ct_need = sc.ring_need[k]; d.ct_ready = sc.seg_end[k]; }
        d.w_base = base; d.n_steps = g.n_steps; d.and_terms = g.and_terms;
        d.pre_off = uint32_t(csrc.size());
        if (base != 0)  // the call's own copies of the constant labels (FALSE, TRUE, the all-zero label) in front of its scratch region
          for (uint32_t q = 0; q < SLOT_FIRST_INPUT; ++q) { csrc.push_back(q); cdst.push_back(base + q); }
        for (size_t i = 0; i < c.in_globals.size(); ++i) { csrc.push_back(global_slot(c.in_globals[i])); cdst.push_back(base + g.input_slots[i]); }
        d.n_pre = uint32_t(csrc.size()) - d.pre_off;
        d.post_off = uint32_t(csrc.size());
        for (size_t i = 0; i < c.out_globals.size(); ++i) {
          if (g.output_slots[i] & SLOT_LDS_FLAG) return "internal: a program output lives in the LDS window";
          csrc.push_back(base + g.output_slots[i]); cdst.push_back(scratch + c.out_globals[i]);
        }
        d.n_post = uint32_t(csrc.size()) - d.post_off;
        d.dep_off = uint32_t(deps.size());
        for (uint32_t q = sc.dep_off[k]; q < sc.dep_off[k + 1]; ++q) deps.push_back(sc.deps[q] - w.call0);
        d.n_deps = uint32_t(deps.size()) - d.dep_off;
        if (csrc.size() > max_list) return "plan hand-over lists too large";
      }
      L.flag_stride = std::max<uint32_t>(L.flag_stride, w.call1 - w.call0 + 2);  // + a slot nobody writes (fault injection below) + the group's progress counter (kernels.hip, watchdog)
    }
    // GSV_FAULT_WITHHOLD_DEP=1 (tests): the first dependency of the first call that has one is pointed at the slot nobody writes — on
    // the device exactly what a violated dispatch-order assumption looks like (a dependency that never completes).  Never for the safe schedule.
    if (!L.safe && withhold_first_dep)
      for (size_t k = 0; k < n; ++k) if (cds[k].n_deps) { deps[cds[k].dep_off] = L.flag_stride - 2; break; }
  }
  *out = std::move(L);
  return std::string();
}

// The parameter policy of a plan session's schedule: the options it was created with (a non-zero field wins over its knob), the shape of
// the launch (`n_instances` at `ni` per workgroup on `n_cus` CUs), the device's free memory, the schedule knobs, and of the plan the
// records of its whole stream and its largest call's ciphertext records and scratch slots.
inline SchedParams plan_sched_params(const gsv_plan_session_opts& o, size_t n_instances, uint32_t ni, int n_cus, size_t free_bytes, const knobs::Sched& kn, uint64_t stream_ct, uint64_t max_block,
                                     uint32_t max_slots) {
  SchedParams sp;
  const size_t n_wg = (n_instances + ni - 1) / ni;
  // calls side by side: as many as it takes to give every CU a workgroup (GSV_PLAN_CONCURRENCY / opts override)
  uint32_t conc = o.max_concurrent_calls ? o.max_concurrent_calls : uint32_t(std::max<size_t>(1, size_t(n_cus) / std::max<size_t>(1, n_wg)));
  if (!o.max_concurrent_calls && kn.plan_concurrency) conc = kn.plan_concurrency;
  // a session that drains its stream leaves a few CUs to the gather kernels that bring finished segments into gate order beside the
  // running window (a workgroup of the garbling kernel takes a whole CU, also while it waits for a dependency)
  if (!o.max_concurrent_calls && o.retain_stream != 1 && conc > 1 && n_wg * size_t(conc) + 16 > size_t(n_cus)) conc = uint32_t(std::max<size_t>(1, (size_t(n_cus) - std::min<size_t>(16, size_t(n_cus) / 2)) / n_wg));
  sp.max_calls_in_flight = std::min<uint32_t>(conc, 65535u);
  // the scratch ring: at most ~1/16 of the free device memory over all instances, and 2^30 slots (slot offsets are 32 bits)
  uint64_t slots = o.max_scratch_slots ? o.max_scratch_slots : uint64_t(free_bytes / 16 / 16 / std::max<size_t>(1, n_instances));
  sp.max_scratch_slots = std::min<uint64_t>(std::max<uint64_t>(slots, max_slots), 1ull << 30);
  if (conc == 1) sp.max_scratch_slots = max_slots;
  // ciphertext window: the whole stream when it is retained, else about a quarter of the free memory for the two window buffers
  if (o.retain_stream == 1) sp.max_window_ct = ~0ull;
  else {
    // Default for sessions that do not retain the stream: the device block (= one window, the scope inside which independent call chains
    // overlap: schedule.hpp) takes up to 40 % of the free memory, at most 48 GB over all instances (one instance of the verifier, 47.7 GB
    // of ciphertexts, is ONE window: 26.7 s instead of the 27.6 s of two — profiles/r04_e2e/verifier_mixed_units.log).  The stream leaves the
    // device in SEGMENTS of a window (below), so a large window costs the drain nothing.  Round 3's default cut one instance's pass into
    // 2 windows and drained whole windows (48.2 s with the commitment: half of the 27-s CBC-MAC chain uncovered); 46 windows of 1 GB hid
    // the chain but cost the garbling 4.7 s — the verifier's line-coefficient chain precedes the Miller loop in stream order and only
    // runs beside it inside one window (29.6 s with 2 windows, 33.4 s with 18, 34.3 s with 46: profiles/r04_e2e/one_instance_windows.log).
    // (... and at most 48 GB over all instances: device memory that has been freed is scrubbed before it is handed out again, ~25 GB/s,
    // so a session of 16 instances with a 96-GB block took 6 s to create; its garbling is 3 % faster with 6-GB windows than with 2-GB ones)
    const double block_bytes = std::min(double(free_bytes) * 0.4, 48e9);
    uint64_t w = o.window_ct_records ? o.window_ct_records : uint64_t(block_bytes / 16.0 / double(std::max<size_t>(1, n_instances)));
    if (!o.window_ct_records && conc == 1) w = 0;  // sequential sessions keep the one-call block of rounds 1-2 (smallest footprint)
    sp.max_window_ct = std::max<uint64_t>(w, max_block);
  }
  // Drain segments: at most 64 M records (1 GB) per instance — the serial CBC-MAC chain of a segment takes 0.6 s —, less when three
  // gate-order buffers of that size would take more than a tenth of the free memory; never smaller than the largest call.
  {
    uint64_t sg = o.drain_segment_records ? o.drain_segment_records : std::min<uint64_t>(uint64_t(double(free_bytes) * 0.1 / (3.0 * 16.0) / double(std::max<size_t>(1, n_instances))), 1ull << 26);
    if (kn.drain_segment_records && !o.drain_segment_records) sg = kn.drain_segment_records;
    sp.segment_ct = std::min<uint64_t>(std::max<uint64_t>(sg, max_block), sp.max_window_ct);
  }
  // Ciphertext ring (schedule.hpp), retain_stream = GSV_STREAM_RING or GSV_CT_RING=1 in the environment: a session that does not
  // retain the stream and runs calls side by side keeps THREE
  // segments' worth of ciphertexts on the device instead of a window's, and the window becomes the whole pass (one instance: 48 GB of
  // device block -> 3.2 GB, 2 windows -> 1; sixteen: 17 windows -> 1 over a 27-GB ring).  Opt-in: with large windows + segments the
  // pass is already bounded by the dependent depth and the host's MAC chain (tools/ring_ab.py: 30.7 s either way for one instance,
  // 32.9 s vs 32.5-33.4 s for sixteen), and a ring makes the running launch WAIT for the host — it must never share a hardware queue
  // with the side streams (create_side_stream).  Not with an explicit window_ct_records (the caller sizes the launches: garble ||
  // evaluate pairs, tests), not for sequential sessions, and not when the whole stream fits the ring anyway.
  const bool ring_wanted = o.retain_stream == GSV_STREAM_RING || (o.retain_stream == 0 && kn.ct_ring);
  if (ring_wanted && !o.window_ct_records && conc > 1) {
    uint64_t ring = std::max<uint64_t>(3 * sp.segment_ct, 2 * sp.segment_ct + max_block);
    if (kn.ct_ring_records) ring = std::max<uint64_t>(kn.ct_ring_records, 2 * sp.segment_ct + max_block);  // tests: small rings on small circuits
    if (ring < stream_ct && ring <= sp.max_window_ct) { sp.ring_ct = ring; sp.max_window_ct = ~0ull; }
  }
  sp.max_window_calls = std::min<uint32_t>(o.max_window_calls ? o.max_window_calls : 32768u, 65535u);
  return sp;
}

}  // namespace gsv
