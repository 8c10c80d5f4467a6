// Part of engine.cpp: program sessions — window variants, program upload, create / destroy.
// ---------------------------------------------------------------- sessions
// The variant of a program for `ni` instances per workgroup (1/ni of the LDS window each), compiled on first use.  Throws on failure; p->mu held by the caller.
static void compile_window_variant(gsv_program* p, uint32_t ni) {
  if (ni <= p->window_div || p->variants.count(ni)) return;
  if (!p->src) gsv_panic("this program was compiled for 1/" + std::to_string(p->window_div) + " of the LDS window and its trace was not kept: it cannot serve " + std::to_string(ni) +
                         " instances per workgroup (build the plan with GSV_PLAN_WINDOW_DIV=" + std::to_string(ni) + ")");
  CompileOptions opt = p->src->opt;
  opt.lds_slots = std::min<uint32_t>(opt.lds_slots, LDS_WINDOW_SLOTS / ni);
  std::unique_ptr<Program> q(new Program(compile_program(p->src->trace, p->src->inputs, p->src->outputs, p->src->feedback, opt)));
  for (size_t i = 0; i < q->input_slots.size(); ++i)
    if (q->input_slots[i] != SLOT_FIRST_INPUT + i) gsv_panic("internal: inputs are not slot-contiguous");
  p->variants[ni] = std::move(q);
}
// Instances per workgroup of a session: as many (1, 2, 4) as keep every CU busy — the latency-bound narrow steps then cost their fixed
// time once for all of them (kernels.hip) — limited to what the programs can serve; `forced` (GSV_INSTANCES_PER_WG=1|2|4, 0 = not set) overrides.
static uint32_t choose_instances_per_wg(size_t n_instances, int n_cus, uint32_t max_servable, uint32_t forced) {
  uint32_t ni = forced ? forced : n_instances > 2 * size_t(n_cus) ? 4u : n_instances > size_t(n_cus) ? 2u : 1u;
  while (ni > 1 && (ni > max_servable || ni > n_instances)) ni /= 2;
  return ni;
}
// One device buffer of `bytes` + `pad` bytes holding `src` — `zeroed`: the padding too (without, it is never read).
static int upload_padded(DevBuf& dst, const void* src, size_t bytes, size_t pad, bool zeroed) {
  HIPCHK(dst.alloc(bytes + pad));
  if (zeroed) HIPCHK(hipMemset(dst.get(), 0, bytes + pad));
  if (bytes) HIPCHK(hipMemcpy(dst.get(), src, bytes, hipMemcpyHostToDevice));
  return GSV_OK;
}
static int upload_program(gsv_engine* e, gsv_program* p, uint32_t ni, const DevProgram** out) {
  std::lock_guard<std::mutex> lk(p->mu);
  // one image per compiled variant: a program compiled for a share of the window serves every layout up to it from ONE copy in HBM
  // (the verifier plan's images are 41 GB)
  const int key = int(p->image_key(ni));
  auto it = p->dev.find({e->device, key});
  if (it != p->dev.end()) { *out = it->second.get(); return GSV_OK; }
  // a program loaded by gsv_plan_load(path, engine) has no host copy of its records: there is nothing to upload to another device
  if (p->prog.spilled) return fail(GSV_ERR_INVALID, "this program's records were written to a plan file and dropped (gsv_plan_build_file / a plan recorder with a plan file): load the file with gsv_plan_load");
  if (p->device_only) return fail(GSV_ERR_INVALID, "this program was loaded straight into another device's memory (gsv_plan_load with an engine): it has no image for device " + std::to_string(e->device));
  if (ni > p->window_div) {  // first session with this many instances per workgroup: compile for that share of the LDS window
    GSV_TRY
    compile_window_variant(p, ni);
    GSV_CATCH
  }
  auto d = std::make_shared<DevProgram>();  // filed in p->dev when it is complete: a failed upload releases what it allocated
  const Program& g = p->variant(ni);
  auto up = [&](DevBuf& dst, const void* src, size_t bytes) -> int {
    d->bytes += bytes;
    return upload_padded(dst, src, bytes, 32, true);  // 32 bytes of zero padding: the kernel's record prefetch reads 24 bytes wherever a lane's record starts
  };
  int rc;
  if ((rc = up(d->steps, g.steps.data(), g.steps.size() * sizeof(StepDesc))) || (rc = up(d->ands, g.ands.data(), g.ands.size() * sizeof(AndRec))) ||
      (rc = up(d->xors, g.xors.data(), g.xors.size() * sizeof(XorRec))) || (rc = up(d->fb_src, g.fb_src_slot.data(), g.fb_src_slot.size() * 4)) ||
      (rc = up(d->fb_dst, g.fb_dst_slot.data(), g.fb_dst_slot.size() * 4)) || (rc = up(d->out_slots, g.output_slots.data(), g.output_slots.size() * 4)) ||
      (rc = up(d->ct_pos, g.ct_pos.data(), g.ct_pos.size() * 4)))
    return rc;
  *out = d.get();
  p->dev[{e->device, key}] = std::move(d);
  return GSV_OK;
}
// The per-instance buffers and the two timing events of a session whose wire file and outputs are those of `g` (the program, or a plan
// session's facade).  Called again after a second schedule was installed (fall_back_to_safe_schedule): the wire files and the
// ciphertext block are then re-allocated only where the new schedule needs more (released first: the peak does not double), the rest
// exists.  VB is cleared either way.
static int alloc_session_buffers(gsv_session* s, const Program& g) {
  const size_t n = s->n_inst;
  if (!s->W || !s->VB || s->W.bytes() < n * size_t(g.n_slots) * 16) {
    s->W.reset(); s->VB.reset();
    DEVALLOC(s->W, n * size_t(g.n_slots) * 16, "the wire files");
    HIPCHK(s->VB.alloc(n * size_t(g.n_slots)));
  }
  HIPCHK(hipMemset(s->VB.get(), 0, n * size_t(g.n_slots)));
  if (!s->CT || s->CT.bytes() < n * size_t(s->ct_stride()) * 16) {
    s->CT.reset(); s->ct_alt.reset();
    DEVALLOC(s->CT, n * size_t(s->ct_stride()) * 16, "the ciphertext blocks");
  }
  if (s->delta) return GSV_OK;
  HIPCHK(s->delta.alloc(n * 16));
  HIPCHK(s->out.alloc(n * g.output_slots.size() * 16 + 16));
  HIPCHK(s->out_bits.alloc(n * g.output_slots.size() + 16));
  HIPCHK(s->in_bits.alloc(n * g.input_slots.size() + 16));
  HIPCHK(s->ev0.create());
  HIPCHK(s->ev1.create());
  return GSV_OK;
}

int gsv_session_create(gsv_engine* e, const gsv_program* cp, size_t n_instances, uint64_t replays, uint64_t ct_capacity_replays, gsv_session** out) {
  if (!e || !cp || !out || n_instances == 0 || replays == 0) return fail(GSV_ERR_INVALID, "bad argument");
  gsv_program* p = const_cast<gsv_program*>(cp);
  { int rc = program_ready(p); if (rc) return rc; }
  if (ct_capacity_replays == 0 || ct_capacity_replays > replays) ct_capacity_replays = replays;
  if (replays > 0xFFFFFFFFull) return fail(GSV_ERR_INVALID, "too many replays");
  HIPCHK(hipSetDevice(e->device));
  SessionPtr s(new gsv_session());
  s->e = e; s->p = p; s->n_inst = n_instances; s->replays = replays; s->ct_cap = ct_capacity_replays;
  s->ct_uploaded.assign(n_instances, 0);
  // Two instances per workgroup once there are more instances than CUs (each then works with half of the LDS label
  // window, see kernels.hip); GSV_INSTANCES_PER_WG=1|2 overrides.
  {
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, e->device));
    s->ni = choose_instances_per_wg(n_instances, prop.multiProcessorCount, p->src ? 4u : p->window_div, s->kn.instances_per_wg);
  }
  int rc = upload_program(e, p, s->ni, &s->dp);
  if (rc || (rc = alloc_session_buffers(s.get(), s->prog()))) return rc;
  *out = s.release();
  return GSV_OK;
}
void gsv_session_destroy(gsv_session* s) {
  if (!s) return;
  release_or_defer([s] { delete s; });  // ~gsv_session (engine_drain.ipp)
}
