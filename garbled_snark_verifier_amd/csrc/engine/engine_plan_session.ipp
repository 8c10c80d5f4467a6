// Part of engine.cpp: plan sessions — schedule, wire-file layout and device tables (make_plan_state), inputs, window launches, the non-streaming garble.
int gsv_session_create_plan(gsv_engine* e, const gsv_plan* plan, size_t n_instances, gsv_session** out) { return gsv_session_create_plan_ex(e, plan, n_instances, 1, out); }
int gsv_session_create_plan_ex(gsv_engine* e, const gsv_plan* plan, size_t n_instances, int retain_stream, gsv_session** out) {
  gsv_plan_session_opts o{};
  o.retain_stream = retain_stream;
  return gsv_session_create_plan_opts(e, plan, n_instances, &o, out);
}
static int make_plan_state(gsv_session* s, const gsv_plan_session_opts& o, bool safe, int n_cus, size_t free_b, gsv_session::PlanState* out);
// The call-level schedule of a plan session (schedule.hpp) under the parameters plan_sched_params chose (plan_layout.hpp).
static Schedule make_schedule(const std::vector<PlanCallView>& views, const gsv_plan* plan, const SchedParams& sp, const knobs::Sched& kn) {
  const std::vector<SchedCall> calls = sched_calls(views);
  Schedule sc = schedule_calls(calls, plan->n_globals, plan->outputs, sp);
  {  // always: the O(calls) ring checks (a violation would otherwise show up as a 60 s device stall and status 2)
    const std::string err = verify_ring_bounds(calls, sc);
    if (!err.empty()) gsv_panic("plan schedule: " + err);
  }
  if (kn.verify) {
    const std::string err = verify_schedule(calls, plan->n_globals, plan->outputs, sc);
    if (!err.empty()) gsv_panic("internal: plan schedule violates a hazard: " + err);
    std::fprintf(stderr, "plan schedule: %zu calls, %zu windows, <= %u calls in flight (width %u), scratch ring %llu slots, depth %llu of %llu steps, %zu dependencies\n", calls.size(),
                 sc.windows.size(), sp.max_calls_in_flight, sc.max_width, (unsigned long long)sc.scratch_slots, (unsigned long long)sc.critical_steps, (unsigned long long)sc.total_steps, sc.deps.size());
  }
  return sc;
}
int gsv_session_create_plan_opts(gsv_engine* e, const gsv_plan* plan, size_t n_instances, const gsv_plan_session_opts* opts, gsv_session** out) {
  if (!e || !plan || !out || n_instances == 0 || !plan->finished || plan->calls.empty()) return fail(GSV_ERR_INVALID, "bad argument / plan not finished");
  gsv_plan_session_opts o{};
  o.retain_stream = 1;
  if (opts) o = *opts;
  HIPCHK(hipSetDevice(e->device));
  if (plan->device >= 0 && plan->device != e->device) return fail(GSV_ERR_INVALID, "this plan was loaded into device " + std::to_string(plan->device) + " (gsv_plan_load with an engine): it serves sessions on that device only");
  SessionPtr s(new gsv_session());
  s->e = e; s->p = plan->calls[0].prog; s->plan = plan; s->n_inst = n_instances; s->replays = 1; s->ct_cap = 1;
  s->ct_uploaded.assign(n_instances, 0);
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, e->device));
  {
    uint32_t servable = 4;
    for (const auto& c : plan->calls) if (!c.prog->src) servable = std::min(servable, c.prog->window_div);
    s->ni = choose_instances_per_wg(n_instances, prop.multiProcessorCount, servable, s->kn.instances_per_wg);
  }
  s->call_dev.resize(plan->calls.size());
  if (s->ni > 1) {  // the plan's programs are independent: compile their missing window variants in parallel
    GSV_TRY
    std::vector<gsv_program*> todo;
    for (const auto& c : plan->calls) if (std::find(todo.begin(), todo.end(), c.prog) == todo.end()) todo.push_back(c.prog);
    const uint32_t ni = s->ni;
    parallel_for_programs(todo.size(), knobs::compile_threads(), [&](size_t i) { std::lock_guard<std::mutex> lk(todo[i]->mu); compile_window_variant(todo[i], ni); });
    GSV_CATCH
  }
  for (size_t k = 0; k < plan->calls.size(); ++k) {
    int rc = upload_program(e, plan->calls[k].prog, s->ni, &s->call_dev[k]);
    if (rc) return rc;
  }
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  s->opts = o;
  {
    int rc = make_plan_state(s.get(), o, false, prop.multiProcessorCount, free_b, &s->ps);
    if (rc || (rc = alloc_session_buffers(s.get(), s->prog()))) return rc;
  }
  *out = s.release();
  return GSV_OK;
}
// Everything of a plan session that depends on its SCHEDULE, built whole: the layout (plan_layout.hpp: the schedule under `o`, the wire-file
// layout, the tables of the window launches) and its device half — the tables uploaded, the completion flags, the ring's position counter
// and the completion counters in mapped host memory.  Built into a local; *out is assigned only on success, so a failure leaves the
// session as it was.  Called by gsv_session_create_plan_opts and again, with the safe options, by fall_back_to_safe_schedule.
static int make_plan_state(gsv_session* s, const gsv_plan_session_opts& o, bool safe, int n_cus, size_t free_b, gsv_session::PlanState* out) {
  const gsv_plan* plan = s->plan;
  const size_t n = plan->calls.size();
  const knobs::Sched kn;
  gsv_session::PlanState st;
  GSV_TRY
  std::vector<PlanCallView> views(n);
  uint64_t max_block = 0;
  uint32_t max_slots = 0;
  for (size_t k = 0; k < n; ++k) {
    const PlanCall& c = plan->calls[k];
    PlanCallView& v = views[k];
    v.prog = &s->call_prog(k);
    v.in_globals = PlanCallView::ids(c.in_globals); v.out_globals = PlanCallView::ids(c.out_globals);
    v.gid_off = c.gid_off; v.ct_off = c.ct_off;
    v.steps = s->call_dev[k]->steps.get(); v.ands = s->call_dev[k]->ands.get(); v.xors = s->call_dev[k]->xors.get();
    max_block = std::max<uint64_t>(max_block, v.prog->n_ct);
    max_slots = std::max(max_slots, v.prog->n_slots);
  }
  const SchedParams sp = plan_sched_params(o, s->n_inst, s->ni, n_cus, free_b, kn, plan->n_ct, max_block, max_slots);
  const std::string err = build_plan_layout(views, plan->n_globals, plan->n_inputs, plan->outputs, plan->n_gates, plan->n_ct, make_schedule(views, plan, sp, kn), o.retain_stream == 1, safe,
                                            kn.fault_withhold_dep, &st.L);
  if (!err.empty()) return fail(GSV_ERR_CIRCUIT, err);
  GSV_CATCH
  PlanLayout& L = st.L;
  if (L.ring) {
    HIPCHK(st.ct_pos.alloc(64, hipHostMallocMapped | hipHostMallocCoherent));
    *st.ct_pos.get() = 0;
  }
  // the device-written completion counters (one per call of the PLAN: windows enqueued back to back never share a counter), in mapped host memory
  HIPCHK(st.done.alloc(n * 4 + 64, hipHostMallocMapped | hipHostMallocCoherent));
  std::memset(st.done.get(), 0, n * 4 + 64);
  for (size_t k = 0; k < n; ++k) { L.calls[k].ct_pos = st.ct_pos.dev(); L.calls[k].done_host = st.done.dev() + k; }
  auto up = [&](DevBuf& dst, const void* src, size_t bytes) -> int { return upload_padded(dst, src, bytes, 64, false); };
  // one flag row per instance: the rows are indexed by blockIdx.x, and a session switched to BLAKE3 after its creation launches one
  // workgroup per instance whatever s->ni says (gsv_session::launch_ni) — flag_stride * 4 bytes per instance
  const size_t n_rows = s->n_inst;
  int rc;
  if ((rc = up(st.d_calls, L.calls.data(), L.calls.size() * sizeof(dev::CallDesc))) || (rc = up(st.d_copy_src, L.copy_src.data(), L.copy_src.size() * 4)) ||
      (rc = up(st.d_copy_dst, L.copy_dst.data(), L.copy_dst.size() * 4)) || (rc = up(st.d_deps, L.deps.data(), L.deps.size() * 4)))
    return rc;
  HIPCHK(st.d_flags.alloc(n_rows * size_t(L.flag_stride) * 4 + 64));
  HIPCHK(hipMemset(st.d_flags.get(), 0, st.d_flags.bytes()));
  HIPCHK(st.d_error.alloc(64));
  HIPCHK(hipMemset(st.d_error.get(), 0, 64));
  if ((rc = up(st.plan_out_slots, L.facade.output_slots.data(), L.facade.output_slots.size() * 4))) return rc;
  *out = std::move(st);
  return GSV_OK;
}
int gsv_session_plan_schedule_info(const gsv_session* s, gsv_plan_schedule_info* info) {
  if (!s || !s->plan || !info) return fail(GSV_ERR_INVALID, "null argument / not a plan session");
  const Schedule& sc = s->sched();
  info->n_calls = s->plan->calls.size(); info->n_windows = sc.windows.size(); info->n_dependencies = sc.deps.size();
  info->max_width = sc.max_width;
  info->scratch_slots = s->ps.L.global_base; info->wire_file_slots = s->prog().n_slots; info->window_ct_records = sc.max_window_ct;
  info->critical_steps = sc.critical_steps; info->total_steps = sc.total_steps;
  info->n_segments = sc.segments.size(); info->segment_ct_records = sc.max_segment_ct;
  info->ct_ring_records = sc.ring_ct;
  return GSV_OK;
}
int gsv_session_plan_window(const gsv_session* s, uint64_t window, uint64_t* first_call, uint64_t* n_calls, uint64_t* max_width) {
  if (!s || !s->plan || window >= s->sched().windows.size()) return fail(GSV_ERR_INVALID, "null argument / window index out of range");
  const Schedule::Window& w = s->sched().windows[size_t(window)];
  if (first_call) *first_call = w.call0;
  if (n_calls) *n_calls = w.call1 - w.call0;
  if (max_width) *max_width = w.max_width;
  return GSV_OK;
}
int gsv_session_set_drain_instances(gsv_session* s, size_t n) {
  if (!s || n > s->n_inst) return fail(GSV_ERR_INVALID, "null session / more instances than the session holds");
  s->drain_instances = n;  // (the gate-order buffers are re-allocated by the next streaming call if they were sized for fewer: ensure_ct_gate)
  return GSV_OK;
}
int gsv_session_set_unchecked_slices(gsv_session* s, int on) {
  if (!s) return fail(GSV_ERR_INVALID, "null session");
  s->unchecked_slices = on != 0;
  return GSV_OK;
}

static int stage_labels(gsv_session* s, const uint8_t* consts, const uint8_t* inputs) {
  // Per instance the wire file starts [FALSE, TRUE, ZERO, input0, input1, ...]: one strided copy.
  if (int rc = plan_session_usable(s)) return rc;
  const Program& g = s->prog();
  const size_t n_in = g.input_slots.size();
  if (s->plan) {  // constants at slots 0..2, inputs at the head of the global region: two strided copies
    std::vector<uint8_t> host(s->n_inst * 48, 0);
    for (size_t i = 0; i < s->n_inst; ++i) std::memcpy(&host[i * 48], consts + 32 * i, 32);
    HIPCHK(hipMemcpy2D(s->W.get(), size_t(g.n_slots) * 16, host.data(), 48, 48, s->n_inst, hipMemcpyHostToDevice));
    if (n_in) HIPCHK(hipMemcpy2D(static_cast<uint8_t*>(s->W.get()) + size_t(s->ps.L.global_base) * 16, size_t(g.n_slots) * 16, inputs, n_in * 16, n_in * 16, s->n_inst, hipMemcpyHostToDevice));
    return GSV_OK;
  }
  const size_t row = (SLOT_FIRST_INPUT + n_in) * 16;
  std::vector<uint8_t> host(s->n_inst * row, 0);
  for (size_t i = 0; i < s->n_inst; ++i) {
    std::memcpy(&host[i * row], consts + 32 * i, 32);
    if (n_in) std::memcpy(&host[i * row + SLOT_FIRST_INPUT * 16], inputs + i * n_in * 16, n_in * 16);
  }
  HIPCHK(hipMemcpy2D(s->W.get(), size_t(g.n_slots) * 16, host.data(), row, row, s->n_inst, hipMemcpyHostToDevice));
  return GSV_OK;
}

// Plan sessions keep the host's last inputs: a pass that is repeated on the safe schedule (fall_back_to_safe_schedule) starts from them —
// the wire file's input region is recycled by the plan's later calls, and the safe schedule lays the wire file out differently.
static void stash_inputs(gsv_session* s, int kind, const uint8_t* delta, const uint8_t* consts, const uint8_t* inputs, const uint8_t* bits) {
  if (!s->plan) return;
  const size_t n_in = s->prog().input_slots.size();
  s->stash_kind = kind;
  if (delta) s->stash_delta.assign(delta, delta + s->n_inst * 16); else s->stash_delta.clear();
  s->stash_consts.assign(consts, consts + s->n_inst * 32);
  if (n_in) s->stash_inputs.assign(inputs, inputs + s->n_inst * n_in * 16); else s->stash_inputs.clear();
  if (bits && n_in) s->stash_bits.assign(bits, bits + s->n_inst * n_in); else s->stash_bits.clear();
}
static int set_garble_inputs_impl(gsv_session* s, const uint8_t* delta, const uint8_t* const_label0, const uint8_t* input_label0) {
  HIPCHK(hipSetDevice(s->e->device));
  HIPCHK(hipMemcpy(s->delta.get(), delta, s->n_inst * 16, hipMemcpyHostToDevice));
  return stage_labels(s, const_label0, input_label0);
}
int gsv_session_set_garble_inputs(gsv_session* s, const uint8_t* delta, const uint8_t* const_label0, const uint8_t* input_label0) {
  if (!s || !delta || !const_label0 || (!input_label0 && !s->prog().input_slots.empty())) return fail(GSV_ERR_INVALID, "null argument");
  stash_inputs(s, 1, delta, const_label0, input_label0, nullptr);
  return set_garble_inputs_impl(s, delta, const_label0, input_label0);
}
static int set_evaluate_inputs_impl(gsv_session* s, const uint8_t* const_active, const uint8_t* input_active, const uint8_t* input_bits);
int gsv_session_set_evaluate_inputs(gsv_session* s, const uint8_t* const_active, const uint8_t* input_active, const uint8_t* input_bits) {
  if (!s || !const_active || ((!input_active || !input_bits) && !s->prog().input_slots.empty())) return fail(GSV_ERR_INVALID, "null argument");
  stash_inputs(s, 2, nullptr, const_active, input_active, input_bits);
  return set_evaluate_inputs_impl(s, const_active, input_active, input_bits);
}
static int set_evaluate_inputs_impl(gsv_session* s, const uint8_t* const_active, const uint8_t* input_active, const uint8_t* input_bits) {
  HIPCHK(hipSetDevice(s->e->device));
  int rc = stage_labels(s, const_active, input_active);
  if (rc) return rc;
  const Program& g = s->prog();
  const size_t n_in = g.input_slots.size();
  // plaintext bits: constants FALSE=0 / TRUE=1 (evaluate_mode.rs:104-121), then the input bits
  HIPCHK(hipMemset(s->VB.get(), 0, s->n_inst * size_t(g.n_slots)));
  std::vector<uint8_t> two(s->n_inst * 2);
  for (size_t i = 0; i < s->n_inst; ++i) { two[2 * i] = 0; two[2 * i + 1] = 1; }
  HIPCHK(hipMemcpy2D(s->VB.get(), g.n_slots, two.data(), 2, 2, s->n_inst, hipMemcpyHostToDevice));
  if (n_in) {
    std::vector<uint8_t> nb(s->n_inst * n_in);
    for (size_t i = 0; i < nb.size(); ++i) nb[i] = input_bits[i] ? 1 : 0;
    HIPCHK(hipMemcpy(s->in_bits.get(), nb.data(), nb.size(), hipMemcpyHostToDevice));
    if (gsvk_scatter_bits(s->VB.get(), g.n_slots, s->first_input_slot(), s->in_bits.get(), uint32_t(n_in), uint32_t(s->n_inst), nullptr) != 0) return fail(GSV_ERR_DEVICE, "scatter_bits launch failed");
    HIPCHK(hipDeviceSynchronize());
  }
  return GSV_OK;
}
// The device stream of an instance holds each replay's ciphertexts in PROGRAM order (coalesced stores, program.hpp);
// every host-facing call speaks GATE order (the reference's stream / gc_{i}.bin order) through a staging buffer
// and a gather / scatter kernel.
static const uint64_t CT_STAGE_RECORDS = 1ull << 20;  // 16 MiB
static int ensure_ct_stage(gsv_session* s) {
  if (!s->ct_stage) HIPCHK(s->ct_stage.alloc(CT_STAGE_RECORDS * 16));
  return GSV_OK;
}
// stage[0..n) <-> gate-order records [first, first+n) of one instance's stream.  Program sessions: one permutation per replay
// block; plan sessions: one per call block.
static int permute_range(gsv_session* s, size_t instance, uint64_t first, uint64_t n, int scatter) {
  uint8_t* stream = static_cast<uint8_t*>(s->CT.get()) + instance * s->ct_stride() * 16;
  if (!s->plan) return gsvk_permute_ciphertexts(stream, s->dp->ct_pos.as<const uint32_t>(), s->prog().n_ct, first, n, s->ct_stage.get(), scatter, s->e->stream.get());
  for (size_t k = 0; k < s->plan->calls.size(); ++k) {
    const uint64_t b0 = s->plan->calls[k].ct_off, b1 = b0 + s->call_prog(k).n_ct;
    const uint64_t lo = std::max(first, b0), hi = std::min(first + n, b1);
    if (lo >= hi) continue;
    int rc = gsvk_permute_ciphertexts(stream + b0 * 16, s->call_dev[k]->ct_pos.as<const uint32_t>(), b1 - b0, lo - b0, hi - lo, static_cast<uint8_t*>(s->ct_stage.get()) + (lo - first) * 16, scatter, s->e->stream.get());
    if (rc) return rc;
  }
  return 0;
}
// copies stream records [first, first+n) of one instance, in gate order, to host memory
static int fetch_ciphertexts(gsv_session* s, size_t instance, uint64_t first, uint64_t n, uint8_t* out) {
  int rc = ensure_ct_stage(s);
  if (rc) return rc;
  if (permute_range(s, instance, first, n, 0) != 0) return fail(GSV_ERR_DEVICE, "ciphertext gather launch failed");
  HIPCHK(hipMemcpyAsync(out, s->ct_stage.get(), n * 16, hipMemcpyDeviceToHost, s->e->stream.get()));
  HIPCHK(hipStreamSynchronize(s->e->stream.get()));
  return GSV_OK;
}

int gsv_session_upload_ciphertexts(gsv_session* s, size_t instance, const uint8_t* cts, uint64_t n_records) {
  if (!s || instance >= s->n_inst || (!cts && n_records)) return fail(GSV_ERR_INVALID, "bad argument");
  if (n_records > s->ct_stride()) return fail(GSV_ERR_INVALID, "more ciphertexts than the session's stream capacity");
  HIPCHK(hipSetDevice(s->e->device));
  // gate-order records from the host -> program-order positions of the device stream (staged in chunks)
  int rc = ensure_ct_stage(s);
  if (rc) return rc;
  for (uint64_t off = 0; off < n_records; off += CT_STAGE_RECORDS) {
    const uint64_t n = std::min<uint64_t>(CT_STAGE_RECORDS, n_records - off);
    HIPCHK(hipMemcpyAsync(s->ct_stage.get(), cts + off * 16, n * 16, hipMemcpyHostToDevice, s->e->stream.get()));
    if (permute_range(s, instance, off, n, 1) != 0) return fail(GSV_ERR_DEVICE, "ciphertext scatter launch failed");
    HIPCHK(hipStreamSynchronize(s->e->stream.get()));
  }
  s->ct_uploaded[instance] = n_records;
  return GSV_OK;
}

static int launch_plan(gsv_session* s, uint64_t gate_id_base, bool eval);
// What every launch of a session passes to the kernels, whatever it runs: the per-instance buffers (ciphertexts into / from `ct_block`), the layout, the hasher.
static dev::KernelArgs session_kernel_args(const gsv_session* s, void* ct_block, uint64_t gate_id_base) {
  dev::KernelArgs ka{};
  ka.W = s->W.as<uint4>(); ka.VB = s->VB.as<uint8_t>(); ka.CT = static_cast<uint4*>(ct_block);
  ka.delta = s->delta.as<const uint4>(); ka.te = s->e->te.as<const uint32_t>();
  ka.ct_stride = s->ct_stride(); ka.gid_base = gate_id_base; ka.n_slots = s->prog().n_slots;
  ka.n_instances = uint32_t(s->n_inst); ka.hasher = uint32_t(s->hasher); ka.instances_per_wg = s->launch_ni();
  ka.diag = s->pass.diag;
  return ka;
}
static int launch(gsv_session* s, uint64_t gate_id_base, bool eval, uint64_t rep_base = 0, uint64_t n_replays = 0) {
  if (int rc = plan_session_usable(s)) return rc;
  if (s->plan) return launch_plan(s, gate_id_base, eval);
  const Program& g = s->prog();
  HIPCHK(hipSetDevice(s->e->device));
  dev::KernelArgs ka = session_kernel_args(s, s->CT.get(), gate_id_base);
  ka.steps = s->dp->steps.get(); ka.ands = s->dp->ands.get(); ka.xors = s->dp->xors.get();
  ka.fb_src = s->dp->fb_src.as<const uint32_t>(); ka.fb_dst = s->dp->fb_dst.as<const uint32_t>();
  ka.n_gates = g.n_gates; ka.n_ct = g.n_ct;
  ka.n_steps = g.n_steps; ka.replays = uint32_t(n_replays ? n_replays : s->replays); ka.rep_base = uint32_t(rep_base); ka.ct_cap_replays = uint32_t(s->ct_cap);
  ka.n_fb = uint32_t(g.fb_src_slot.size()); ka.fb_stage_base = g.fb_stage_base;
  ka.and_terms = g.and_terms; ka.any_four_wire = g.and_terms == 4;
  ka.step_clock = s->step_clock.as<unsigned long long>();
  HIPCHK(hipEventRecord(s->ev0.get(), s->e->stream.get()));
  if (ka.n_steps) {
    int lrc = gsvk_launch_program(&ka, uint32_t(s->n_inst), eval ? 1 : 0, s->e->stream.get());
    if (lrc != 0) return fail(GSV_ERR_DEVICE, std::string("kernel launch failed: ") + hipGetErrorString(hipError_t(lrc)));
  }
  HIPCHK(hipEventRecord(s->ev1.get(), s->e->stream.get()));
  if (!g.output_slots.empty()) {
    if (gsvk_gather_outputs(s->W.get(), s->VB.get(), g.n_slots, s->dp->out_slots.as<const uint32_t>(), uint32_t(g.output_slots.size()),
                            uint32_t(s->n_inst), s->out.get(), eval ? s->out_bits.get() : nullptr, s->e->stream.get()) != 0)
      return fail(GSV_ERR_DEVICE, "gather launch failed");
  }
  s->ran = true; s->last_eval = eval;
  return GSV_OK;
}
// One WINDOW of a plan session = one launch: grid = (instance groups, calls of the window); every workgroup waits for the
// completion flags of the calls it depends on, fetches its inputs from the global wires, runs its program in its own scratch region
// and publishes its outputs (kernels.hip).  A sequential schedule (one call in flight) is the same launch with each call depending on
// its predecessor: the instance groups still drift apart instead of meeting at a launch boundary after every call.
static int launch_plan_window(gsv_session* s, size_t w, uint64_t gate_id_base, bool eval, void* ct_block = nullptr, hipStream_t stream = nullptr) {
  const gsv_session::PlanState& sd = s->ps;
  if (!ct_block) ct_block = s->CT.get();       // (garble -> evaluate: the garbler's current block, for both sessions)
  if (!stream) stream = s->e->stream.get();
  const Schedule::Window& win = s->sched().windows[w];
  dev::KernelArgs ka = session_kernel_args(s, ct_block, gate_id_base);
  ka.calls = sd.d_calls.as<const dev::CallDesc>() + win.call0;
  ka.copy_src = sd.d_copy_src.as<const uint32_t>(); ka.copy_dst = sd.d_copy_dst.as<const uint32_t>();
  ka.deps = sd.d_deps.as<const uint32_t>(); ka.flags = sd.d_flags.as<uint32_t>(); ka.error = sd.d_error.as<uint32_t>();
  if (sd.done) {  // (the counters of THIS window's calls: its launch of the previous pass has long finished — every pass ends synchronised)
    std::memset(sd.done.get() + win.call0, 0, size_t(win.call1 - win.call0) * 4);
    __atomic_thread_fence(__ATOMIC_RELEASE);
  }
  ka.flag_stride = sd.L.flag_stride; ka.epoch = ++s->epoch;
  ka.wait_ticks = (unsigned long long)(s->pass.dep_wait_seconds * 1e8);  // dependency watchdog (kernels.hip): seconds without ANY completed call of the instance group before a wait gives up
  ka.replays = 1; ka.ct_cap_replays = 1;  // (n_gates, n_ct, n_steps, rep_base: 0 — the calls' descriptors carry their own)
  for (uint32_t k = win.call0; k < win.call1 && !ka.any_four_wire; ++k) ka.any_four_wire = s->call_prog(k).and_terms == 4;
  int lrc = gsvk_launch_batch(&ka, uint32_t(s->n_inst), win.call1 - win.call0, eval ? 1 : 0, stream);
  if (lrc != 0) return fail(GSV_ERR_DEVICE, std::string("kernel launch failed: ") + hipGetErrorString(hipError_t(lrc)));
  ++s->windows_launched;
  return GSV_OK;
}
int gsv_session_windows_launched(const gsv_session* s, uint64_t* n) {
  if (!s || !s->plan || !n) return fail(GSV_ERR_INVALID, "null argument / not a plan session");
  *n = s->windows_launched;
  return GSV_OK;
}
// after a synchronisation: did a dependency wait give up?
static int check_plan_error(gsv_session* s) {
  uint32_t ew[16] = {0};
  HIPCHK(hipMemcpy(ew, s->ps.d_error.get(), 64, hipMemcpyDeviceToHost));
  const uint32_t err = ew[0];
  s->dep_fault = err == 1;
  if (err == 2) {
    // which calls of the last window have not finished everywhere, and where the host's position stood (diagnostics)
    std::string open_calls;
    if (s->ps.done.get() && !s->sched().windows.empty()) {
      const uint32_t n_wg = uint32_t(s->launch_groups());
      const Schedule::Window& win = s->sched().windows.back();
      int shown = 0;
      for (uint32_t k = win.call0; k < win.call1 && shown < 12; ++k)
        if (s->ps.done.get()[k] != n_wg) { open_calls += " " + std::to_string(k) + "(" + std::to_string(s->ps.done.get()[k]) + "/" + std::to_string(n_wg) + ", need " + std::to_string(s->sched().ring_need[k]) + ")"; ++shown; }
    }
    return fail(GSV_ERR_DEVICE, "a call waited for the host's stream position (ciphertext ring) and saw it stand still at " + std::to_string(s->ps.ct_pos.get() ? *s->ps.ct_pos.get() : 0) +
                                    "; unfinished calls:" + open_calls + "; the call that gave up: " + std::to_string(ew[8]) + " of the window (instance group " + std::to_string(ew[9]) + "), it wanted position " +
                                    std::to_string((uint64_t(ew[11]) << 32) | ew[10]) + ", saw " + std::to_string((uint64_t(ew[13]) << 32) | ew[12]) + " unchanged for " +
                                    std::to_string(double((uint64_t(ew[15]) << 32) | ew[14]) * 1e-8) + " s" + (s->ring_diag.empty() ? "" : "; host: " + s->ring_diag) + "; results are invalid");
  }
  if (err) return fail(GSV_ERR_DEVICE, "a call of the plan waited for a dependency that never completed (dispatch-order assumption of schedule.hpp violated); results are invalid");
  return GSV_OK;
}
// Gate order <-> program order for calls [k0, k1) of window w (a drain segment, or the whole window): gate-order buffer, records
// relative to `gate_ct0` (the stream index of the buffer's first record) <-> the window's device block.
static int permute_plan_calls(gsv_session* s, size_t w, uint32_t k0, uint32_t k1, uint64_t gate_ct0, uint64_t gate_stride, int scatter, void* ct_block, void* gate_buf, hipStream_t stream) {
  const Schedule::Window& win = s->sched().windows[w];
  if (!ct_block) ct_block = s->CT.get();
  if (!gate_buf) gate_buf = s->ct_gate.get();
  if (!stream) stream = s->e->stream.get();
  for (uint32_t k = k0; k < k1; ++k) {
    const Program& cp = s->call_prog(k);
    if (!cp.n_ct) continue;
    const uint64_t rel = s->plan->calls[k].ct_off - win.ct0;
    uint8_t* block = static_cast<uint8_t*>(ct_block) + (s->retain() ? s->plan->calls[k].ct_off : s->ring() ? s->sched().ring_off[k] : rel) * 16;
    const size_t n_gather = (!scatter && s->drain_instances) ? std::min(s->drain_instances, s->n_inst) : s->n_inst;  // gsv_session_set_drain_instances
    if (gsvk_gather_segment(block, s->ct_stride(), s->call_dev[k]->ct_pos.as<const uint32_t>(), cp.n_ct, 1, uint32_t(n_gather), static_cast<uint8_t*>(gate_buf) + (s->plan->calls[k].ct_off - gate_ct0) * 16, gate_stride, scatter, stream) != 0)
      return fail(GSV_ERR_DEVICE, scatter ? "ciphertext scatter launch failed" : "ciphertext gather launch failed");
  }
  return GSV_OK;
}
// windows [w0, w1) that cover exactly the calls [c0, c1), or an error: a slice of a plan starts and ends on window boundaries
static int window_range(const gsv_session* s, size_t c0, size_t c1, size_t* w0, size_t* w1) {
  const auto& ws = s->sched().windows;
  size_t a = 0;
  while (a < ws.size() && ws[a].call0 < c0) ++a;
  size_t b = a;
  while (b < ws.size() && ws[b].call1 <= c1) ++b;
  if (c0 == c1) { *w0 = *w1 = a; return GSV_OK; }
  if (a >= ws.size() || ws[a].call0 != c0 || b == a || ws[b - 1].call1 != c1)
    return fail(GSV_ERR_INVALID, "a slice of a plan session must start and end on window boundaries of its schedule (gsv_session_plan_window)");
  *w0 = a; *w1 = b;
  return GSV_OK;
}
static int gather_plan_outputs(gsv_session* s, bool eval) {
  const Program& f = s->prog();
  if (!f.output_slots.empty()) {
    if (gsvk_gather_outputs(s->W.get(), s->VB.get(), f.n_slots, s->ps.plan_out_slots.as<const uint32_t>(), uint32_t(f.output_slots.size()), uint32_t(s->n_inst), s->out.get(),
                            eval ? s->out_bits.get() : nullptr, s->e->stream.get()) != 0) return fail(GSV_ERR_DEVICE, "gather launch failed");
  }
  s->ran = true; s->last_eval = eval;
  return GSV_OK;
}
static int launch_plan(gsv_session* s, uint64_t gate_id_base, bool eval) {
  if (!s->retain()) return fail(GSV_ERR_INVALID, "this plan session keeps one window of ciphertexts only: use gsv_session_garble_streaming");
  HIPCHK(hipSetDevice(s->e->device));
  HIPCHK(hipMemsetAsync(s->ps.d_error.get(), 0, 4, s->e->stream.get()));  // every pass starts with a clean dependency-wait flag
  HIPCHK(hipEventRecord(s->ev0.get(), s->e->stream.get()));
  s->windows_launched = 0;
  for (size_t w = 0; w < s->sched().windows.size(); ++w) {
    int rc = launch_plan_window(s, w, gate_id_base, eval);
    if (rc) return rc;
  }
  HIPCHK(hipEventRecord(s->ev1.get(), s->e->stream.get()));
  return gather_plan_outputs(s, eval);
}

int gsv_session_garble(gsv_session* s, uint64_t gate_id_base) {
  if (!s) return fail(GSV_ERR_INVALID, "null session");
  s->pass = knobs::Pass();  // this pass's knobs
  int rc = launch(s, gate_id_base, false);
  if (rc == GSV_OK) s->garbled = true;
  return rc;
}
