// Part of engine.cpp: evaluation, of the resident stream and from streaming sources (host side: upload_pipeline.hpp).
// A resident stream the host uploaded holds `need` records per instance before anything reads it: EvaluateMode panics with "Ciphertext
// source exhausted at gate .." when the source runs dry (evaluate_mode.rs:139-142).
static int check_resident_stream(const gsv_session* s, uint64_t need) {
  if (!s->garbled)
    for (size_t i = 0; i < s->n_inst; ++i)
      if (s->ct_uploaded[i] < need)
        return fail(GSV_ERR_EXHAUSTED, "Ciphertext source exhausted: instance " + std::to_string(i) + " holds " + std::to_string(s->ct_uploaded[i]) + " of " + std::to_string(need) + " ciphertexts");
  return GSV_OK;
}
int gsv_session_evaluate(gsv_session* s, uint64_t gate_id_base) {
  if (!s) return fail(GSV_ERR_INVALID, "null session");
  s->pass = knobs::Pass();  // this pass's knobs
  if (s->ct_cap != s->replays || (s->plan && !s->retain())) return fail(GSV_ERR_INVALID, "evaluate needs the whole ciphertext stream resident (ct_capacity_replays == replays)");
  if (int rc = check_resident_stream(s, s->prog().n_ct * s->replays)) return rc;
  return launch(s, gate_id_base, true);
}

// The part of a pass one streaming evaluation runs (plan sessions: a slice of whole windows; program sessions: always the whole pass)
struct EvalRange {
  size_t c0 = 0, c1 = 0;          // calls of the plan
  size_t w0 = 0, w1 = 0;          // ... which are these windows of the session's schedule
  uint64_t ct0 = 0, ct1 = 0;      // ... and these records of every instance's stream
  bool first = true, last = true; // the slice starts / ends the pass
  bool restartable = false;       // a restart point is taken in front of the slice, and a failure rolls the session back to one
};
// the range of calls [c0, c1) on the session's present schedule (c0 = c1 = 0 for a program session: the whole pass)
static int eval_range(const gsv_session* s, size_t c0, size_t c1, bool restartable, EvalRange* rg) {
  *rg = EvalRange();
  rg->restartable = restartable;
  rg->ct1 = stream_records(s);
  if (!s->plan) return GSV_OK;
  rg->c0 = c0; rg->c1 = c1;
  if (int rc = window_range(s, c0, c1, &rg->w0, &rg->w1)) return rc;
  const auto& ws = s->sched().windows;
  rg->ct0 = rg->w0 < ws.size() ? ws[rg->w0].ct0 : s->plan->n_ct;
  rg->ct1 = rg->w1 < ws.size() ? ws[rg->w1].ct0 : s->plan->n_ct;
  rg->first = c0 == 0; rg->last = c1 == s->plan->calls.size();
  return GSV_OK;
}
// What the three drivers of one evaluate_streaming_pass share
struct EvalPass {
  gsv_session* s;
  uint64_t gate_id_base;
  CtUploader& up;
  uint64_t seg_records;  // per instance: stride of the gate-order buffer
  B3Receiver& b3;        // BLAKE3 of the uploaded segments, when digests were asked for; verified mode: with the instances' outboards
  MacCheckReceiver& mac; // the CBC-MAC check of the uploaded segments against checkpoints, when the pass verifies that way
  const EvalRange& rg;
  // `n` records per instance starting at stream index `base` -> the gate-order buffer through `st` (bounded page-locked chunks, hashed as read)
  int upload(uint64_t base, uint64_t n, hipStream_t st) {
    switch (up.upload(base, n, s->ct_gate.get(), st)) {
      case UploadError::None: return GSV_OK;
      case UploadError::EventWait: return fail(GSV_ERR_DEVICE, "event wait failed");
      case UploadError::Dry: return fail(GSV_ERR_EXHAUSTED, "Ciphertext source exhausted: instance " + std::to_string(up.dry_instance()) + " ran dry at record " + std::to_string(up.dry_record()));
      case UploadError::Order: return fail(GSV_ERR_INVALID, "internal: a segment at record " + std::to_string(base) + " does not follow the stream, which stands at record " + std::to_string(up.next_record()));
      default: return fail(GSV_ERR_DEVICE, "ciphertext upload failed");
    }
  }
  // the `n` records per instance just uploaded to the gate-order buffer through `st`: hashed in front of their scatter
  int hash(uint64_t n, hipStream_t st) {
    if (int rc = b3.feed(s->ct_gate.get(), seg_records, n, st)) return rc;
    return mac.feed(s->ct_gate.get(), seg_records, n, st);
  }
  // verified modes, in front of a launch: every group value (BLAKE3) and every failing-group word (CBC-MAC) the segments uploaded so far
  // have produced is waited for and looked at
  int verified() {
    if (b3.check) if (int rc = b3.flush()) return rc;
    return mac.finish(false);
  }
};
// Plan session over a ciphertext ring: the window (the whole pass) is launched FIRST; its calls wait on the device until the host's
// position counter says their segment has been uploaded.  Segment after segment: wait until the calls whose blocks this segment's
// blocks overwrite have completed (their flags), upload and scatter on the side stream, publish the segment's end.
static int evaluate_plan_ring(EvalPass& p) {
  gsv_session* const s = p.s;
  int rc = ensure_aux(s);
  for (size_t w = p.rg.w0; w < p.rg.w1 && rc == GSV_OK; ++w) {  // (a ring's schedule is one window: the slice is the pass)
    const Schedule::Window& win = s->sched().windows[w];
    __atomic_store_n(s->ps.ct_pos.get(), (unsigned long long)win.ct0, __ATOMIC_RELEASE);
    rc = launch_plan_window(s, w, p.gate_id_base, true);
    bool window_done = false;
    for (uint32_t q = win.seg0; q < win.seg1 && rc == GSV_OK; ++q) {
      const Schedule::Segment& sg = s->sched().segments[q];
      uint32_t o0 = ~0u, o1 = 0;
      for (uint32_t k = sg.call0; k < sg.call1; ++k) if (s->sched().ovl1[k] > s->sched().ovl0[k]) { o0 = std::min(o0, s->sched().ovl0[k]); o1 = std::max(o1, s->sched().ovl1[k]); }
      // [ovl0, ovl1) is a RANGE around the overwritten calls: the calls it spans beside them are earlier calls too, but those of this
      // very segment cannot run before this upload — and are never among the overwritten ones (the ring holds two segments and a call)
      o1 = std::min(o1, sg.call0);
      if (o1 > o0) rc = wait_calls_done(s, w, o0, o1, &window_done);
      if (rc != GSV_OK) break;
      if (window_done) { rc = fail(GSV_ERR_DEVICE, "internal: the window finished before its ciphertexts were uploaded"); break; }
      // uploads and the scatter go through the side stream (the main stream holds the running window)
      rc = p.upload(sg.ct0, sg.n_ct, s->aux_stream.get());
      if (rc == GSV_OK) rc = p.hash(sg.n_ct, s->aux_stream.get());
      if (rc == GSV_OK) rc = permute_plan_calls(s, w, sg.call0, sg.call1, sg.ct0, p.seg_records, 1, nullptr, nullptr, s->aux_stream.get());
      if (rc == GSV_OK && hipStreamSynchronize(s->aux_stream.get()) != hipSuccess) rc = fail(GSV_ERR_DEVICE, "ciphertext scatter failed");
      if (rc == GSV_OK) __atomic_store_n(s->ps.ct_pos.get(), (unsigned long long)(sg.ct0 + sg.n_ct), __ATOMIC_RELEASE);
    }
    if (rc != GSV_OK) {
      // let the calls that still wait for ciphertexts run out (their results are discarded with the error) instead of hanging the stream
      __atomic_store_n(s->ps.ct_pos.get(), ~0ull, __ATOMIC_RELEASE);
      (void)hipStreamSynchronize(s->e->stream.get());
      break;
    }
    if (hipStreamSynchronize(s->e->stream.get()) != hipSuccess) rc = fail(GSV_ERR_DEVICE, "kernel failed");
  }
  return rc;
}
// Plan session, one window of the schedule per launch: its ciphertexts uploaded and scattered segment by segment, then the window.
static int evaluate_plan_windows(EvalPass& p) {
  gsv_session* const s = p.s;
  int rc = GSV_OK;
  for (size_t w = p.rg.w0; w < p.rg.w1 && rc == GSV_OK; ++w) {
    const Schedule::Window& win = s->sched().windows[w];
    for (uint32_t q = win.seg0; q < win.seg1 && rc == GSV_OK; ++q) {
      const Schedule::Segment& sg = s->sched().segments[q];
      // (the stream orders this segment's uploads behind the scatter of the previous one, which read the same buffer)
      rc = p.upload(sg.ct0, sg.n_ct, s->e->stream.get());
      if (rc == GSV_OK) rc = p.hash(sg.n_ct, s->e->stream.get());
      if (rc == GSV_OK) rc = permute_plan_calls(s, w, sg.call0, sg.call1, sg.ct0, p.seg_records, 1, nullptr, nullptr, nullptr);
    }
    // verified modes: what the segments uploaded so far have produced is compared before the window that reads them is launched
    if (rc == GSV_OK) rc = p.verified();
    if (rc == GSV_OK) rc = launch_plan_window(s, w, p.gate_id_base, true);
  }
  return rc;
}
// Program session, one ring (ct_cap replays) per launch
static int evaluate_program_rings(EvalPass& p) {
  gsv_session* const s = p.s;
  const uint64_t n_ct = s->prog().n_ct, total = s->replays, seg = s->ct_cap;
  int rc = GSV_OK;
  for (uint64_t r0 = 0; r0 < total && rc == GSV_OK; r0 += seg) {
    const uint64_t r1 = std::min(total, r0 + seg);
    rc = p.upload(r0 * n_ct, (r1 - r0) * n_ct, s->e->stream.get());
    if (rc == GSV_OK) rc = p.hash((r1 - r0) * n_ct, s->e->stream.get());
    if (rc == GSV_OK) rc = p.verified();  // verified modes: compared before the ring is scattered and launched
    if (rc != GSV_OK) break;
    if (gsvk_gather_segment(s->CT.get(), s->ct_stride(), s->dp->ct_pos.as<const uint32_t>(), n_ct, uint32_t(r1 - r0), uint32_t(s->n_inst), s->ct_gate.get(), p.seg_records, 1, s->e->stream.get()) != 0) { rc = fail(GSV_ERR_DEVICE, "ciphertext scatter launch failed"); break; }
    rc = launch(s, p.gate_id_base, true, r0, r1 - r0);
  }
  return rc;
}
// Evaluate with the ciphertexts coming from a CiphertextSource (ciphertext_source.rs:14-107), segment by segment: program sessions one
// ring at a time, plan sessions one window of the schedule at a time.  The records arrive in gate order in bounded chunks (a
// page-locked 16 MiB staging buffer: a window may be gigabytes), are folded into the per-instance CBC-MAC as FileSource does while
// reading (ciphertext_source.rs:36-107), uploaded, scattered to the program-order positions the kernel reads, and evaluated.
//   read(instance, first_record, dst, n) -> 0, or non-zero when the source runs dry ("Ciphertext source exhausted", evaluate_mode.rs:139-142)
// With `digests` the uploaded gate-order segments are also fed to the BLAKE3 kernels of the garbler's drain (engine_blake3.ipp), on the
// stream that scatters them: what the evaluator compares with commit_i = BLAKE3(gc_<i>.bin) costs the host 32 bytes per group of chunks.
// Verified mode (gsv_session_evaluate_streaming_verified): the instances' outboards, already checked against `expected`, and the
// commitments themselves (n_inst x expected_len bytes) for the last look at the computed digests.
// A pass in slices (EvalRange): the wire file stays where the previous slice left it, the uploader starts at the slice's first record
// with the MAC states of the slice before, the B3Stream and the outboard comparison go on where they stood (s->evs); a slice that does
// not end the pass leaves no group value in flight, gathers no outputs and writes no digests.
// Verified against CBC-MAC checkpoints (EvalVerify::mac): where the claimed states come from — files or memory, opened and checked by
// every slice —, their k, the commitments they claim (n_inst x 16) and where the slice that ends the pass writes them (or null)
struct EvalMacVerify { MacStateSource states; uint32_t k = 0; std::vector<uint8_t> claimed; uint8_t* hashes_out = nullptr; };
// kind: the verification's member of EvalCommit; no_place: the mismatch was the digest's, at the end of the pass; bad_*: where a stream
// differs (what gsv_session_mismatch_info reports, and what decides which restart point a failed slice rolls back to)
struct EvalVerify { B3Check& check; const uint8_t* expected; uint64_t expected_len; EvalCommit kind; bool no_place = false; EvalMacVerify* mac = nullptr; uint64_t bad_instance = 0, bad_group = 0, bad_record = 0; };
static EvalCarry& eval_carry(gsv_session* s) { if (!s->evs) s->evs.reset(new EvalCarry()); return *s->evs; }
static int evaluate_streaming_pass_inner(gsv_session* s, uint64_t gate_id_base, const CtUploader::Read& read, uint8_t* hashes, uint8_t* digests, EvalVerify* vf, const EvalRange& rg) {
  if (int urc = plan_session_usable(s)) return urc;
  const Program& g = s->prog();
  EvalCarry& cy = eval_carry(s);
  if (s->plan && rg.first) s->windows_launched = 0;
  // plan sessions: one window of the schedule per launch, its ciphertexts uploaded SEGMENT by segment (schedule.hpp: a gate-order buffer
  // holds the largest segment, the program-order device block the largest window); program sessions: one ring per launch
  const size_t n_inst = s->n_inst;
  HIPCHK(hipSetDevice(s->e->device));
  const uint64_t seg_records = s->plan ? s->max_segment() : s->ct_cap * g.n_ct;  // per instance: stride of the gate-order buffer
  if (seg_records) { int grc = ensure_ct_gate(s, n_inst * size_t(seg_records) * 16); if (grc) return grc; }  // (a sample drain before may have sized it for fewer instances)
  // With hashes asked for, T workers fold the chunks into the per-instance CBC-MACs beside the uploads (upload_pipeline.hpp; the
  // reference folds while reading, ciphertext_source.rs:36-107, and runs its finalized cases under into_par_iter: cut_and_choose/evaluator.rs:118-181)
  const size_t T = hashes ? std::max<size_t>(1, std::min<size_t>(std::min<size_t>(n_inst, 16), gsv_drain::usable_cores() > 1 ? gsv_drain::usable_cores() - 1 : 1)) : 0;
  CtUploader up(n_inst, seg_records, std::min<uint64_t>(std::max<uint64_t>(seg_records, 1), CT_STAGE_RECORDS), T, read);
  if (!rg.first) {
    if (hashes && cy.macs.size() != n_inst) return fail(GSV_ERR_INVALID, "this slice continues a pass whose earlier slices computed no CBC-MAC for these instances");
    up.start_at(rg.ct0, hashes ? cy.macs : std::vector<CbcMacHost>());
  }
  if (up.alloc() != hipSuccess) return fail(GSV_ERR_DEVICE, "cannot allocate the ciphertext staging buffers");
  B3Receiver b3(s->b3_eval, "the ciphertext stream of instance", vf && !vf->mac ? &vf->check : nullptr);
  MacCheckReceiver mac(s->mac_eval, "the ciphertext stream of instance", s->e->te.get(), vf && vf->mac ? vf->mac->states : MacStateSource());
  EvalPass p{s, gate_id_base, up, seg_records, b3, mac, rg};
  // where the check found a stream that differs, for the caller
  auto placed = [&](int rc) { if (rc == GSV_ERR_MISMATCH && mac.on) { vf->bad_instance = mac.bad_instance; vf->bad_group = mac.bad_group; vf->bad_record = mac.bad_record; } return rc; };
  // a pass starts the hash afresh, and verifies from group 0 (the pass the safe-schedule fallback repeats too); its later slices go on
  if (digests) {
    const int brc = rg.first ? b3.begin(n_inst, stream_records(s), seg_records, s->pass.b3_subtree_log2) : b3.resume(n_inst, stream_records(s), seg_records, s->pass.b3_subtree_log2);
    if (brc) return brc;
  }
  // ... and so does the check against checkpoints: its carries and its position live in the session (s->mac_eval)
  if (vf && vf->mac) {
    const int mrc = rg.first ? mac.begin(n_inst, stream_records(s), seg_records, vf->mac->k, s->e->stream.get()) : mac.resume(n_inst, stream_records(s), seg_records, vf->mac->k);
    if (mrc) return mrc;
  }
  if (s->plan && rg.first) HIPCHK(hipMemsetAsync(s->ps.d_error.get(), 0, 4, s->e->stream.get()));
  HIPCHK(hipEventRecord(s->ev0.get(), s->e->stream.get()));
  int rc = s->plan ? (s->ring() ? evaluate_plan_ring(p) : evaluate_plan_windows(p)) : evaluate_program_rings(p);
  if (hipStreamSynchronize(s->e->stream.get()) != hipSuccess && rc == GSV_OK) rc = fail(GSV_ERR_DEVICE, "kernel failed");
  if (rc != GSV_OK) return placed(rc);
  if (s->plan) {
    HIPCHK(hipEventRecord(s->ev1.get(), s->e->stream.get()));
    if (rg.last) { rc = gather_plan_outputs(s, true); if (rc) return rc; }
    HIPCHK(hipStreamSynchronize(s->e->stream.get()));
    rc = check_plan_error(s);
    if (rc) return rc;
    if (!rg.last) s->ran = false;  // no outputs before the slice that ends the pass: gsv_session_read_outputs fails as after a pass that never ran
  }
  up.finish();
  // (before the MACs are written: a failure leaves both arrays untouched.)  The end of a verified pass compares the computed digests with
  // the commitments: the last chunk was read before the pass, what was uploaded is what counts
  if (digests && rg.last) {
    rc = b3.finish(s->e->stream.get(), digests, vf ? vf->expected : nullptr, vf ? vf->expected_len : 0);
    if (rc) { if (vf) vf->no_place = b3.at_end; return rc; }
  } else if (digests) { rc = b3.flush(); if (rc) return rc; }  // the next slice's receiver finds nothing in flight
  // the check against checkpoints: nothing is in flight between two slices; the slice that ends the pass has seen every group hold, so
  // the last claimed states are the streams' true CBC-MACs
  if (mac.on) {
    rc = mac.finish(rg.last);
    if (rc) return placed(rc);
    if (rg.last && vf->mac->hashes_out) std::memcpy(vf->mac->hashes_out, vf->mac->claimed.data(), vf->mac->claimed.size());
  }
  if (hashes) { cy.macs = up.mac_states(); up.digests(hashes); } else cy.macs.clear();
  return GSV_OK;
}
static int evaluate_streaming_pass(gsv_session* s, uint64_t gate_id_base, const CtUploader::Read& read, uint8_t* hashes, uint8_t* digests, EvalVerify* vf, const EvalRange& rg) {
  if (vf) clear_mismatch(s);
  const int rc = evaluate_streaming_pass_inner(s, gate_id_base, read, hashes, digests, vf, rg);
  if (rc == GSV_ERR_MISMATCH) {  // the stream differs from its outboard, or from its checkpoints, at the place the check holds
    if (!vf->mac) { vf->bad_instance = vf->check.bad_instance; vf->bad_group = vf->check.bad_group; vf->bad_record = vf->check.bad_record; }
    set_mismatch(s, vf->bad_instance, vf->bad_group, vf->bad_record);
    s->ran = false;  // no outputs for a stream that did not verify: gsv_session_read_outputs fails as after a pass that never ran
  }
  return rc;
}
// ---- restart points (include/gsv_engine.h "Sliced evaluation") ----
// The session as it stands -> r, in front of the slice `rg`: stream-ordered copies on the engine's stream, which the slice's uploads,
// scatters and launches follow.  (The slice at call 0 begins the B3Stream afresh: there is no B3 half to keep.)
static int take_restart_point(gsv_session* s, EvalRestart& r, const EvalRange& rg, bool want_b3, bool want_mac) {
  EvalCarry& cy = *s->evs;
  const size_t n = s->n_inst, slots = s->prog().n_slots;
  const hipStream_t st = s->e->stream.get();
  HIPCHK(hipSetDevice(s->e->device));
  r.held = false;
  if (int rc = ensure_dev(r.W, n * slots * 16, "a restart point's wire files")) return rc;
  if (int rc = ensure_dev(r.VB, n * slots, "a restart point's plaintext bits")) return rc;
  HIPCHK(hipMemcpyAsync(r.W.get(), s->W.get(), n * slots * 16, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(r.VB.get(), s->VB.get(), n * slots, hipMemcpyDeviceToDevice, st));
  r.n_slots = uint32_t(slots); r.global_base = s->ps.L.global_base;
  r.b3 = false;
  if (want_b3 && !rg.first) {
    if (!s->b3_eval) return fail(GSV_ERR_INVALID, "this slice continues a pass whose earlier slices computed no BLAKE3 commitment");
    if (int rc = b3_save(*s->b3_eval, r, st)) return rc;
  }
  r.mac = false;  // (likewise: the slice at call 0 begins the check afresh)
  if (want_mac && !rg.first) {
    if (!s->mac_eval) return fail(GSV_ERR_INVALID, "this slice continues a pass whose earlier slices ran no CBC-MAC check");
    if (int rc = mac_save(*s->mac_eval, r, st)) return rc;
  }
  r.macs = rg.first ? std::vector<CbcMacHost>() : cy.macs;
  r.check_position = rg.first ? 0 : cy.check.position();
  r.windows_launched = rg.first ? 0 : s->windows_launched;
  r.call = rg.c0; r.record = rg.ct0;
  r.held = true;
  return GSV_OK;
}
// r -> the session.  The wire-file layout may have changed since r was taken (the safe schedule has a scratch area of its own): what
// one window hands to the next are the constants and the plan's global wires, which then move to where the present layout has them.
static int roll_back(gsv_session* s, const EvalRestart& r) {
  EvalCarry& cy = *s->evs;
  const size_t n = s->n_inst, slots = s->prog().n_slots;
  const hipStream_t st = s->e->stream.get();
  HIPCHK(hipSetDevice(s->e->device));
  HIPCHK(hipStreamSynchronize(st));  // whatever the failed slice left queued
  if (r.n_slots == slots && r.global_base == s->ps.L.global_base) {
    HIPCHK(hipMemcpyAsync(s->W.get(), r.W.get(), n * slots * 16, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(s->VB.get(), r.VB.get(), n * slots, hipMemcpyDeviceToDevice, st));
  } else {
    const size_t n_glob = s->plan ? s->plan->n_globals : 0;
    if (!s->plan || r.n_slots - r.global_base != n_glob || slots - s->ps.L.global_base != n_glob) return fail(GSV_ERR_INVALID, "internal: a restart point of another wire file");
    for (int part = 0; part < 2; ++part) {
      const size_t from = part ? r.global_base : 0, to = part ? s->ps.L.global_base : 0, count = part ? n_glob : SLOT_FIRST_INPUT;
      if (!count) continue;
      HIPCHK(hipMemcpy2DAsync(s->W.as<uint8_t>() + to * 16, slots * 16, r.W.as<uint8_t>() + from * 16, size_t(r.n_slots) * 16, count * 16, n, hipMemcpyDeviceToDevice, st));
      HIPCHK(hipMemcpy2DAsync(s->VB.as<uint8_t>() + to, slots, r.VB.as<uint8_t>() + from, size_t(r.n_slots), count, n, hipMemcpyDeviceToDevice, st));
    }
  }
  if (r.b3) { if (!s->b3_eval) return fail(GSV_ERR_INVALID, "internal: a restart point without its BLAKE3 stream"); if (int rc = b3_restore(*s->b3_eval, r, st)) return rc; }
  if (r.mac) { if (!s->mac_eval) return fail(GSV_ERR_INVALID, "internal: a restart point without its CBC-MAC check"); if (int rc = mac_restore(*s->mac_eval, r, st)) return rc; }
  HIPCHK(hipStreamSynchronize(st));
  cy.macs = r.macs; cy.check.rewind(r.check_position);
  s->windows_launched = r.windows_launched;
  cy.next_call = r.call;
  cy.resumable = true; cy.resume_call = r.call; cy.resume_record = r.record;
  s->ran = false;
  return GSV_OK;
}
// One slice — the whole pass is the slice [0, n_calls) without a restart point — with what surrounds it: the commitments every slice of
// a pass must share, the restart point, the evaluator's side of the safe-schedule fallback (engine_drain.ipp, fall_back_to_safe_schedule)
// and the rollback of a restartable slice that failed.
// Fallback: a slice that ended with a dependency wait giving up switches the session to one call per launch.  A whole pass over a source
// that can be read again from the start (gc files) is then evaluated again at once; a restartable slice over such a source is repeated
// alone, from its restart point (any call range is a range of the safe schedule's windows); any other source gets the error with the
// remedy — its records have been consumed — and the host's repeat, of the pass or of the rolled-back slice, succeeds.
// The commitments and the kind of verification every slice of a pass shares (kind: the verification's member of EvalCommit, None for
// none).  The verified entry points ask in front of their up-front checks; evaluate_streaming_impl asks again where the slice runs.
static int check_slice_commit(gsv_session* s, const uint8_t* hashes, const uint8_t* digests, EvalCommit kind, const EvalRange& rg) {
  EvalCarry& cy = eval_carry(s);
  const EvalCommit commit = (hashes ? EvalCommit::Mac : EvalCommit::None) | (digests ? EvalCommit::B3 : EvalCommit::None) | kind;
  if (const char* why = eval_commit_refusal(cy.commit, commit, rg.first)) return fail(GSV_ERR_INVALID, why);
  cy.commit = commit;
  return GSV_OK;
}
static int evaluate_streaming_impl(gsv_session* s, uint64_t gate_id_base, const std::function<int(size_t, uint64_t, uint8_t*, uint64_t)>& read, uint8_t* hashes, uint8_t* digests, EvalRange rg, bool rereadable = false, EvalVerify* vf = nullptr) {
  EvalCarry& cy = eval_carry(s);
  if (int crc = check_slice_commit(s, hashes, digests, vf ? vf->kind : EvalCommit::None, rg)) return crc;  // (records cy.commit in front of the refusal below, not behind it: a verified slice's entry point has recorded the same value already)
  if (vf && vf->mac && rg.restartable && rg.ct1 - rg.ct0 < (1ull << vf->mac->k))
    return fail(GSV_ERR_INVALID, "a verified restartable slice must hold at least one whole group of 2^k records per instance (k = " + std::to_string(vf->mac->k) + " in the checkpoints: " + std::to_string(1ull << vf->mac->k) +
                                     " records): this one holds " + std::to_string(rg.ct1 - rg.ct0));
  if (vf && !vf->mac && rg.restartable && rg.ct1 - rg.ct0 < (64ull << s->pass.b3_subtree_log2))
    return fail(GSV_ERR_INVALID, "a verified restartable slice must hold at least one whole group of 2^k chunks per instance (" + std::to_string(64ull << s->pass.b3_subtree_log2) + " records): this one holds " + std::to_string(rg.ct1 - rg.ct0));
  // the restart points: [0] is this slice's, [1] stays the one of the restartable slice before it — unless this is the repeat of a slice
  // the session was rolled back to, whose predecessor's is still the one in [1]
  const bool repeat = cy.resumable && cy.resume_call == rg.c0 && cy.rp[0].held && cy.rp[0].call == rg.c0;
  cy.resumable = false;
  if (rg.first) cy.rp[0].held = cy.rp[1].held = false;
  if (rg.restartable) {
    if (!repeat) std::swap(cy.rp[0], cy.rp[1]);
    if (int rc = take_restart_point(s, cy.rp[0], rg, digests != nullptr, vf && vf->mac)) { cy.rp[0].held = cy.rp[1].held = false; cy.next_call = 0; return rc; }
  } else cy.rp[0].held = cy.rp[1].held = false;
  int rc = evaluate_streaming_pass(s, gate_id_base, read, hashes, digests, vf, rg);
  if (rc == GSV_ERR_DEVICE && s->plan && s->dep_fault && !s->safe()) {
    const std::string first_error = g_err;
    const bool whole = rg.first && rg.last;
    if (fall_back_to_safe_schedule(s)) { cy.next_call = 0; return fail(GSV_ERR_DEVICE, first_error + "; the fall-back to the safe schedule failed too: " + g_err); }
    if (rg.restartable) {
      if (roll_back(s, cy.rp[0])) { cy.resumable = false; cy.next_call = 0; return fail(GSV_ERR_DEVICE, first_error + "; the session now runs the safe schedule, but its restart point could not be restored: " + g_err); }
      if (!rereadable) return fail(GSV_ERR_DEVICE, first_error + "; the session now runs the safe schedule (one call per launch) and stands where this slice began: repeat the slice (gsv_session_evaluate_resume_info)");
    } else if (!whole || !rereadable) {
      cy.next_call = 0;
      return fail(GSV_ERR_DEVICE, first_error + "; the session now runs the safe schedule (one call per launch): repeat the pass from gsv_session_set_evaluate_inputs");
    }
    if (s->pass.drain_debug || s->pass.plan_debug) std::fprintf(stderr, "plan session: %s -- repeating the %s on the safe schedule (one call per launch)\n", first_error.c_str(), whole ? "evaluation" : "slice");
    if (int rrc = eval_range(s, rg.c0, rg.c1, rg.restartable, &rg)) { cy.resumable = false; cy.next_call = 0; return rrc; }
    cy.resumable = false;
    rc = evaluate_streaming_pass(s, gate_id_base, read, hashes, digests, vf, rg);
  }
  if (rc == GSV_OK) { cy.next_call = rg.c1; return GSV_OK; }
  // a failed slice: rolled back to a restart point when it took one and the failure has a place in the stream, else the pass is over
  const std::string error = g_err;
  const EvalRestart* to = nullptr;
  bool from_call_0 = false;
  if (rg.restartable && rc == GSV_ERR_EXHAUSTED) to = &cy.rp[0];
  else if (rg.restartable && rc == GSV_ERR_MISMATCH && vf && !vf->no_place) {
    // the group that differs may have begun in the slice before (THE GUARANTEE: one open group per instance is evaluated before it is
    // verified): that slice's wire file cannot be trusted either
    const int which = vf->bad_record < rg.ct0 ? 1 : 0;
    if (cy.rp[which].held) to = &cy.rp[which]; else from_call_0 = true;
    if (to && which == 1) { std::swap(cy.rp[0], cy.rp[1]); cy.rp[1].held = false; to = &cy.rp[0]; }
  }
  cy.next_call = 0;
  if (to && roll_back(s, *to) != GSV_OK) { to = nullptr; cy.resumable = false; }
  if (!to) cy.rp[0].held = cy.rp[1].held = false;
  if (from_call_0) { cy.resumable = true; cy.resume_call = cy.resume_record = 0; }  // no restart point reaches back that far: the pass starts again
  return fail(rc, error);
}
int gsv_session_evaluate_resume_info(const gsv_session* s, uint64_t* next_call, uint64_t* next_record) {
  if (!s) return fail(GSV_ERR_INVALID, "null session");
  if (!s->evs || !s->evs->resumable) return fail(GSV_ERR_INVALID, "the session's last streaming evaluation left nothing to resume");
  if (next_call) *next_call = s->evs->resume_call;
  if (next_record) *next_record = s->evs->resume_record;
  return GSV_OK;
}
// The call range of a sliced entry point (first_call = n_calls = 0: the whole pass), checked as garble_slice checks the garbler's
static int eval_slice_range(gsv_session* s, uint64_t first_call, uint64_t n_calls, int restartable, EvalRange* rg) {
  if (!s->plan) return fail(GSV_ERR_INVALID, "not a plan session: program sessions are evaluated in one pass");
  const uint64_t n = s->plan->calls.size();
  if (first_call == 0 && n_calls == 0) n_calls = n;
  if (first_call > n || n_calls > n - first_call) return fail(GSV_ERR_INVALID, "call range outside the plan");
  if (n_calls == 0) return fail(GSV_ERR_INVALID, "an empty slice: n_calls == 0 is the whole pass with first_call == 0 and nothing anywhere else");
  const EvalCarry& cy = eval_carry(s);
  if (first_call != 0 && first_call != cy.next_call && !s->unchecked_slices)
    return fail(GSV_ERR_INVALID, "slice starts at call " + std::to_string(first_call) + " but the previous evaluate slice ended at call " + std::to_string(cy.next_call) +
                                     " (gsv_session_set_unchecked_slices for timing runs)");
  if (restartable && s->ring()) return fail(GSV_ERR_INVALID, "restart points are not available over a ciphertext ring (retain_stream = GSV_STREAM_RING): its pass is one launch; use launch windows (retain_stream = 0)");
  return eval_range(s, size_t(first_call), size_t(first_call + n_calls), restartable != 0, rg);
}
static int eval_whole_range(gsv_session* s, EvalRange* rg) { return eval_range(s, 0, s->plan ? s->plan->calls.size() : 0, false, rg); }
// In front of a verified pass, before anything is uploaded: every instance's outboard is loaded and bounds-checked against the SESSION's
// stream length and this pass's k — all of them before any is folded — and then, with `last_chunk`, its root — folded with the
// instance's last chunk — must be the commitment.  A difference there has no place in the stream: the mismatch names the instance
// alone.  No kernel has run when this fails.  All of this in the slice at call 0; a later slice finds the parsed outboards in the
// session, or (`reload`: the in-memory form, whose host hands them in again) loads and bounds-checks them once more.
//   load(i, k, n_records, out, why) -> the outboard of instance i, well-formed (load_outboard, check_outboard), or false
//   last_chunk(i, dst, n_records) -> 0 with the last n_records records of instance i's stream in dst; null: the roots are left to the end of the pass
using LoadOutboard = std::function<bool(size_t, uint32_t, uint64_t, std::vector<uint8_t>*, std::string*)>;
using LastChunk = std::function<int(size_t, uint8_t*, uint64_t)>;
static int prepare_verified_pass(gsv_session* s, EvalVerify& vf, const LoadOutboard& load, const LastChunk& last_chunk, const EvalRange& rg, bool reload) {
  const uint32_t k = s->pass.b3_subtree_log2;
  if (int krc = check_b3_k(k)) return krc;
  const uint64_t total = stream_records(s), first_of_last = (Outboard::chunks(total) - 1) * 64;
  B3Check& c = vf.check;
  std::string why;
  if (!rg.first) {
    if (c.bytes.size() != s->n_inst || c.k != k || c.n_records != total) return fail(GSV_ERR_INVALID, "this slice continues a verified pass whose slice at call 0 took no outboards of this shape (instances, GSV_B3_SUBTREE_LOG2)");
    for (size_t i = 0; reload && i < s->n_inst; ++i) if (!load(i, k, total, &c.bytes[i], &why)) return fail(GSV_ERR_INVALID, why);
    if (!c.holds(s->n_inst, k, total)) return fail(GSV_ERR_INVALID, "this slice continues a verified pass whose slice at call 0 took no outboards of this shape (instances, GSV_B3_SUBTREE_LOG2)");
    return GSV_OK;
  }
  c.shape(s->n_inst, k, total);
  clear_mismatch(s);
  eval_carry(s).resumable = false;
  for (size_t i = 0; i < s->n_inst; ++i) if (!load(i, k, total, &c.bytes[i], &why)) return fail(GSV_ERR_INVALID, why);
  std::vector<uint8_t> last(size_t(total - first_of_last) * 16);
  for (size_t i = 0; last_chunk && i < s->n_inst; ++i) {
    if (last_chunk(i, last.data(), total - first_of_last) != 0)
      return fail(GSV_ERR_EXHAUSTED, "Ciphertext source exhausted: instance " + std::to_string(i) + " holds fewer than " + std::to_string(total) + " ciphertexts");
    Outboard o;
    uint8_t root[32];
    if (!Outboard::parse(c.bytes[i].data(), c.bytes[i].size(), &o, &why) || !o.root(last.data(), last.size(), root, &why)) return fail(GSV_ERR_INVALID, why);
    if (std::memcmp(root, vf.expected + vf.expected_len * i, size_t(vf.expected_len)) != 0) {
      set_mismatch(s, i, ~0ull, ~0ull);
      s->ran = false;
      return fail(GSV_ERR_MISMATCH, "outboard or last chunk of instance " + std::to_string(i) + " does not match the commitment");
    }
  }
  return GSV_OK;
}
// FileSource: instance i reads <dir>/gc_<indexes[i]>.bin (indexes == NULL: first_index + i).  Verified mode (outboard_dir): the
// outboards lie in files too, and a file's last chunk lies where the session's stream length puts it.  The files are opened per slice.
static int evaluate_from_files(gsv_session* s, uint64_t gate_id_base, const char* dir, const uint64_t* indexes, uint64_t first_index, uint8_t* hashes, uint8_t* digests, const EvalRange& rg,
                               const char* outboard_dir = nullptr, const uint8_t* expected = nullptr, uint64_t expected_len = 0) {
  auto index = [&](size_t i) { return indexes ? indexes[i] : first_index + i; };
  GcFileSource files;
  std::string why;
  for (size_t i = 0; i < s->n_inst; ++i)
    if (!files.add(std::string(dir) + "/gc_" + std::to_string(index(i)) + ".bin", &why)) return fail(GSV_ERR_INVALID, why);
  EvalVerify vf{eval_carry(s).check, expected, expected_len, EvalCommit::VerifiedFiles};
  if (int crc = check_slice_commit(s, hashes, digests, outboard_dir ? vf.kind : EvalCommit::None, rg)) return crc;
  if (outboard_dir) {
    const int vrc = prepare_verified_pass(s, vf,
        [&](size_t i, uint32_t k, uint64_t n_records, std::vector<uint8_t>* out, std::string* w) { return load_outboard(OutboardWriter::path(outboard_dir, index(i)), k, n_records, out, w); },
        [&](size_t i, uint8_t* dst, uint64_t n) { return files.read(i, stream_records(s) - n, dst, n); }, rg, /*reload=*/false);
    if (vrc) return vrc;
  }
  return evaluate_streaming_impl(s, gate_id_base, [&](size_t i, uint64_t first, uint8_t* dst, uint64_t n) { return files.read(i, first, dst, n); }, hashes, digests, rg, /*rereadable=*/true, outboard_dir ? &vf : nullptr);
}
// The whole pass over files: what the entry points below share (the range [0, n_calls), no restart point)
static int evaluate_pass_from_files(gsv_session* s, uint64_t gate_id_base, const char* dir, const uint64_t* indexes, uint64_t first_index, uint8_t* hashes, uint8_t* digests,
                                    const char* outboard_dir = nullptr, const uint8_t* expected = nullptr, uint64_t expected_len = 0) {
  if (!s || !dir) return fail(GSV_ERR_INVALID, "null argument");
  EvalRange rg;
  if (int rc = eval_whole_range(s, &rg)) return rc;
  return evaluate_from_files(s, gate_id_base, dir, indexes, first_index, hashes, digests, rg, outboard_dir, expected, expected_len);
}
int gsv_session_evaluate_streaming(gsv_session* s, uint64_t gate_id_base, const char* dir, uint64_t first_index, uint8_t* hashes) {
  PassGuard pass_guard(s);  // destroys requested while this pass runs wait for its end (deferred release)
  return evaluate_pass_from_files(s, gate_id_base, dir, nullptr, first_index, hashes, nullptr);
}
int gsv_session_evaluate_streaming_indexed(gsv_session* s, uint64_t gate_id_base, const char* dir, const uint64_t* indexes, uint8_t* hashes) {
  PassGuard pass_guard(s);  // destroys requested while this pass runs wait for its end (deferred release)
  if (!indexes) return fail(GSV_ERR_INVALID, "null index list");
  return evaluate_pass_from_files(s, gate_id_base, dir, indexes, 0, hashes, nullptr);
}
// the generic source as CtUploader reads it
static CtUploader::Read source_reader(gsv_ct_source_fn source, void* user) { return [source, user](size_t i, uint64_t first, uint8_t* dst, uint64_t n) -> int { return source(user, i, first, dst, n); }; }
int gsv_session_evaluate_streaming_source(gsv_session* s, uint64_t gate_id_base, gsv_ct_source_fn source, void* user, uint8_t* hashes) {
  return gsv_session_evaluate_streaming_source_commit(s, gate_id_base, source, user, hashes, nullptr);
}
// The three above with either commitment or both (blake3_digests == NULL is what they do)
int gsv_session_evaluate_streaming_commit(gsv_session* s, uint64_t gate_id_base, const char* dir, const uint64_t* indexes, uint64_t first_index, uint8_t* cbcmac_hashes, uint8_t* blake3_digests) {
  PassGuard pass_guard(s);  // destroys requested while this pass runs wait for its end (deferred release)
  return evaluate_pass_from_files(s, gate_id_base, dir, indexes, first_index, cbcmac_hashes, blake3_digests);
}
// ... and verified against outboards and commitments the caller trusts (include/gsv_engine.h, "BLAKE3 outboards")
static const char* const VERIFIED_OVER_A_RING =
    "verified streaming is not available for plan sessions over a ciphertext ring (retain_stream = GSV_STREAM_RING): their pass is one launch that waits on the device for the host's "
    "stream position, and a host that stops feeding it would leave that launch to the watchdog; use launch windows (retain_stream = 0)";
static int check_verified_args(const gsv_session* s, const uint8_t* expected, uint64_t expected_len, const uint8_t* blake3_digests) {
  if (!expected || !blake3_digests) return fail(GSV_ERR_INVALID, "null argument");
  if (expected_len != 16 && expected_len != 32) return fail(GSV_ERR_INVALID, "expected_len must be 16 (a truncated digest) or 32");
  if (s->plan && s->ring()) return fail(GSV_ERR_INVALID, VERIFIED_OVER_A_RING);
  return GSV_OK;
}
int gsv_session_evaluate_streaming_verified(gsv_session* s, uint64_t gate_id_base, const char* dir, const uint64_t* indexes, uint64_t first_index, const char* outboard_dir, const uint8_t* expected,
                                            uint64_t expected_len, uint8_t* cbcmac_hashes, uint8_t* blake3_digests) {
  PassGuard pass_guard(s);  // destroys requested while this pass runs wait for its end (deferred release)
  if (!s || !dir || !outboard_dir) return fail(GSV_ERR_INVALID, "null argument");
  if (int rc = check_verified_args(s, expected, expected_len, blake3_digests)) return rc;
  return evaluate_pass_from_files(s, gate_id_base, dir, indexes, first_index, cbcmac_hashes, blake3_digests, outboard_dir, expected, expected_len);
}
int gsv_session_mismatch_info(const gsv_session* s, uint64_t* instance, uint64_t* group, uint64_t* first_record) {
  if (!s) return fail(GSV_ERR_INVALID, "null session");
  if (!s->mismatch) return fail(GSV_ERR_INVALID, "the session's last verified pass found no mismatch");
  if (instance) *instance = s->mismatch_instance;
  if (group) *group = s->mismatch_group;
  if (first_record) *first_record = s->mismatch_record;
  return GSV_OK;
}
// The generic source, verified (include/gsv_engine.h, "Commitments on the callback paths"): the outboards come in memory.  With the last
// chunks (up-front mode) they are authenticated against `expected` before the source is called at all; without (deferred mode) they are
// checked for form only, and the computed digests meet `expected` at the end of the pass.  `outboards` == NULL: unverified.
static int evaluate_from_source(gsv_session* s, uint64_t gate_id_base, gsv_ct_source_fn source, void* user, const uint8_t* const* outboards, const uint64_t* outboard_bytes,
                                const uint8_t* last_chunks, const uint8_t* expected, uint64_t expected_len, uint8_t* cbcmac_hashes, uint8_t* blake3_digests, const EvalRange& rg) {
  if (!outboards) return evaluate_streaming_impl(s, gate_id_base, source_reader(source, user), cbcmac_hashes, blake3_digests, rg);
  EvalVerify vf{eval_carry(s).check, expected, expected_len, last_chunks ? EvalCommit::VerifiedUpFront : EvalCommit::VerifiedDeferred};
  if (int crc = check_slice_commit(s, cbcmac_hashes, blake3_digests, vf.kind, rg)) return crc;
  const int vrc = prepare_verified_pass(s, vf,
      [&](size_t i, uint32_t k, uint64_t n_records, std::vector<uint8_t>* out, std::string* why) {
        if (!outboards[i]) { *why = "null outboard"; return false; }
        if (!check_outboard("outboards[" + std::to_string(i) + "]", outboards[i], outboard_bytes[i], k, n_records, why)) return false;
        out->assign(outboards[i], outboards[i] + outboard_bytes[i]);
        return true;
      },
      last_chunks ? LastChunk([&](size_t i, uint8_t* dst, uint64_t n) { if (n) std::memcpy(dst, last_chunks + 1024 * i, size_t(n) * 16); return 0; }) : LastChunk(), rg, /*reload=*/true);
  if (vrc) return vrc;
  return evaluate_streaming_impl(s, gate_id_base, source_reader(source, user), cbcmac_hashes, blake3_digests, rg, /*rereadable=*/false, &vf);
}
int gsv_session_evaluate_streaming_source_commit(gsv_session* s, uint64_t gate_id_base, gsv_ct_source_fn source, void* user, uint8_t* cbcmac_hashes, uint8_t* blake3_digests) {
  PassGuard pass_guard(s);  // destroys requested while this pass runs wait for its end (deferred release)
  if (!s || !source) return fail(GSV_ERR_INVALID, "null argument");
  EvalRange rg;
  if (int rc = eval_whole_range(s, &rg)) return rc;
  return evaluate_from_source(s, gate_id_base, source, user, nullptr, nullptr, nullptr, nullptr, 0, cbcmac_hashes, blake3_digests, rg);
}
int gsv_session_evaluate_streaming_source_verified(gsv_session* s, uint64_t gate_id_base, gsv_ct_source_fn source, void* user, const uint8_t* const* outboards, const uint64_t* outboard_bytes,
                                                   const uint8_t* last_chunks, const uint8_t* expected, uint64_t expected_len, uint8_t* cbcmac_hashes, uint8_t* blake3_digests) {
  PassGuard pass_guard(s);  // destroys requested while this pass runs wait for its end (deferred release)
  if (!s || !source || !outboards || !outboard_bytes) return fail(GSV_ERR_INVALID, "null argument");
  if (int rc = check_verified_args(s, expected, expected_len, blake3_digests)) return rc;
  EvalRange rg;
  if (int rc = eval_whole_range(s, &rg)) return rc;
  return evaluate_from_source(s, gate_id_base, source, user, outboards, outboard_bytes, last_chunks, expected, expected_len, cbcmac_hashes, blake3_digests, rg);
}
// ---- slices (include/gsv_engine.h "Sliced evaluation"): the entry points above with a call range and, on request, a restart point ----
int gsv_session_evaluate_streaming_calls(gsv_session* s, uint64_t gate_id_base, uint64_t first_call, uint64_t n_calls, int restartable, const char* dir, const uint64_t* indexes, uint64_t first_index,
                                         const char* outboard_dir, const uint8_t* expected, uint64_t expected_len, uint8_t* cbcmac_hashes, uint8_t* blake3_digests) {
  PassGuard pass_guard(s);  // destroys requested while this pass runs wait for its end (deferred release)
  if (!s || !dir) return fail(GSV_ERR_INVALID, "null argument");
  EvalRange rg;
  if (int rc = eval_slice_range(s, first_call, n_calls, restartable, &rg)) return rc;
  if (outboard_dir) { if (int rc = check_verified_args(s, expected, expected_len, blake3_digests)) return rc; }
  return evaluate_from_files(s, gate_id_base, dir, indexes, first_index, cbcmac_hashes, blake3_digests, rg, outboard_dir, expected, expected_len);
}
int gsv_session_evaluate_streaming_source_calls(gsv_session* s, uint64_t gate_id_base, uint64_t first_call, uint64_t n_calls, int restartable, gsv_ct_source_fn source, void* user,
                                                const uint8_t* const* outboards, const uint64_t* outboard_bytes, const uint8_t* last_chunks, const uint8_t* expected, uint64_t expected_len,
                                                uint8_t* cbcmac_hashes, uint8_t* blake3_digests) {
  PassGuard pass_guard(s);  // destroys requested while this pass runs wait for its end (deferred release)
  if (!s || !source || (outboards && !outboard_bytes)) return fail(GSV_ERR_INVALID, "null argument");
  EvalRange rg;
  if (int rc = eval_slice_range(s, first_call, n_calls, restartable, &rg)) return rc;
  if (outboards) { if (int rc = check_verified_args(s, expected, expected_len, blake3_digests)) return rc; }
  return evaluate_from_source(s, gate_id_base, source, user, outboards, outboard_bytes, last_chunks, expected, expected_len, cbcmac_hashes, blake3_digests, rg);
}
// ---- verified against CBC-MAC checkpoints (include/gsv_engine.h "CBC-MAC checkpoints while evaluating") ----
// What the two entry points below share once the checkpoints of the slice have been opened (files) or bounds-checked (memory) — both
// before anything is uploaded and before a source is called: the commitments the checkpoints claim meet the ones the caller trusts (a
// difference there has no place in the stream) — in EVERY slice, since every slice opens the files or takes the checkpoints anew and
// the slice that ends the pass returns what IT read —; then the slice runs with the receiver in place of the MAC workers.
static int evaluate_against_checkpoints(gsv_session* s, uint64_t gate_id_base, const CtUploader::Read& read, EvalMacVerify& mv, EvalCommit kind, const uint8_t* expected, const EvalRange& rg, bool rereadable) {
  if (rg.first) {
    clear_mismatch(s);
    eval_carry(s).resumable = false;
  }
  for (size_t i = 0; expected && i < s->n_inst; ++i)
    if (std::memcmp(mv.claimed.data() + 16 * i, expected + 16 * i, 16) != 0) {
      set_mismatch(s, i, ~0ull, ~0ull);
      s->ran = false;
      eval_carry(s).resumable = false;
      return fail(GSV_ERR_MISMATCH, "the last checkpoint of instance " + std::to_string(i) + " does not match the commitment");
    }
  EvalVerify vf{eval_carry(s).check, nullptr, 0, kind};
  vf.mac = &mv;
  return evaluate_streaming_impl(s, gate_id_base, read, nullptr, nullptr, rg, rereadable, &vf);
}
// the call range of the two: a program session takes the whole pass only, as gsv_session_garble_streaming_check does
static int eval_checkpoint_range(gsv_session* s, uint64_t first_call, uint64_t n_calls, int restartable, EvalRange* rg) {
  if (!s->plan) {
    if (first_call || n_calls || restartable) return fail(GSV_ERR_INVALID, "program sessions are evaluated in one pass (first_call = n_calls = 0, no restart point)");
    return eval_whole_range(s, rg);
  }
  if (int rc = eval_slice_range(s, first_call, n_calls, restartable, rg)) return rc;
  return s->ring() ? fail(GSV_ERR_INVALID, VERIFIED_OVER_A_RING) : GSV_OK;
}
int gsv_session_evaluate_streaming_mac_calls(gsv_session* s, uint64_t gate_id_base, uint64_t first_call, uint64_t n_calls, int restartable, const char* dir, const uint64_t* indexes, uint64_t first_index,
                                             const char* checkpoint_dir, const uint8_t* expected, uint8_t* cbcmac_hashes) {
  PassGuard pass_guard(s);  // destroys requested while this pass runs wait for its end (deferred release)
  if (!s || !dir || !checkpoint_dir || !cbcmac_hashes) return fail(GSV_ERR_INVALID, "null argument");
  EvalRange rg;
  if (int rc = eval_checkpoint_range(s, first_call, n_calls, restartable, &rg)) return rc;
  if (int rc = check_slice_commit(s, nullptr, nullptr, EvalCommit::CheckpointFiles, rg)) return rc;
  auto index = [&](size_t i) { return indexes ? indexes[i] : first_index + i; };
  GcFileSource files;
  std::string why;
  std::vector<std::string> names(s->n_inst);
  std::vector<const char*> ptrs(s->n_inst);
  for (size_t i = 0; i < s->n_inst; ++i) {
    if (!files.add(std::string(dir) + "/gc_" + std::to_string(index(i)) + ".bin", &why)) return fail(GSV_ERR_INVALID, why);
    names[i] = CheckpointWriter::path(checkpoint_dir, index(i)); ptrs[i] = names[i].c_str();
  }
  // the checkpoint files are opened and validated by every slice (headers, lengths, the session's stream length); they are never held whole
  const uint64_t records = stream_records(s);
  std::vector<MacCheckpointFile> cks;
  if (!open_mac_checkpoints(ptrs.data(), s->n_inst, &records, &cks, &why)) return fail(GSV_ERR_INVALID, why);
  EvalMacVerify mv;
  mv.k = cks[0].head.k; mv.hashes_out = cbcmac_hashes;
  mv.claimed.resize(s->n_inst * 16);
  for (size_t i = 0; i < s->n_inst; ++i) if (!cks[i].commitment(mv.claimed.data() + 16 * i)) return fail(GSV_ERR_INVALID, "read error on " + cks[i].path());
  mv.states = [&cks](size_t i, int64_t s0, uint64_t count, uint8_t* dst) { return cks[i].read_states(s0, count, dst); };
  return evaluate_against_checkpoints(s, gate_id_base, [&](size_t i, uint64_t first, uint8_t* dst, uint64_t n) { return files.read(i, first, dst, n); }, mv, EvalCommit::CheckpointFiles, expected, rg, /*rereadable=*/true);
}
int gsv_session_evaluate_streaming_source_mac_calls(gsv_session* s, uint64_t gate_id_base, uint64_t first_call, uint64_t n_calls, int restartable, gsv_ct_source_fn source, void* user,
                                                    const uint8_t* const* checkpoints, const uint64_t* checkpoint_bytes, const uint8_t* expected, uint8_t* cbcmac_hashes) {
  PassGuard pass_guard(s);  // destroys requested while this pass runs wait for its end (deferred release)
  if (!s || !source || !checkpoints || !checkpoint_bytes || !cbcmac_hashes) return fail(GSV_ERR_INVALID, "null argument");
  EvalRange rg;
  if (int rc = eval_checkpoint_range(s, first_call, n_calls, restartable, &rg)) return rc;
  if (int rc = check_slice_commit(s, nullptr, nullptr, EvalCommit::CheckpointMemory, rg)) return rc;
  // the host hands the checkpoints in with every slice, and every slice bounds-checks them again (as the in-memory outboards)
  const uint64_t records = stream_records(s);
  EvalMacVerify mv;
  mv.hashes_out = cbcmac_hashes;
  mv.claimed.assign(s->n_inst * 16, 0);
  std::string why;
  for (size_t i = 0; i < s->n_inst; ++i) {
    const std::string who = "checkpoints[" + std::to_string(i) + "]: ";
    MacCheckpoints h;
    if (!checkpoints[i]) return fail(GSV_ERR_INVALID, who + "null");
    if (!MacCheckpoints::parse_header(checkpoints[i], checkpoint_bytes[i], &h, &why)) return fail(GSV_ERR_INVALID, who + why);
    if (h.n_records != records) return fail(GSV_ERR_INVALID, who + "for a stream of " + std::to_string(h.n_records) + " records, the stream here holds " + std::to_string(records));
    if (i && h.k != mv.k) return fail(GSV_ERR_INVALID, "the checkpoints of one call must agree on k: checkpoints[0] has " + std::to_string(mv.k) + ", checkpoints[" + std::to_string(i) + "] has " + std::to_string(h.k));
    if (!h.length_ok(checkpoint_bytes[i], &why)) return fail(GSV_ERR_INVALID, who + why);
    mv.k = h.k;
    if (h.states()) std::memcpy(mv.claimed.data() + 16 * i, checkpoints[i] + MacCheckpoints::HEADER_BYTES + (h.states() - 1) * 16, 16);
  }
  const uint64_t n_states = MacCheckpoints::state_count(records, mv.k);
  mv.states = [checkpoints, n_states](size_t i, int64_t s0, uint64_t count, uint8_t* dst) {
    if (count && s0 < 0) { std::memset(dst, 0, 16); dst += 16; ++s0; --count; }
    if (uint64_t(s0) + count > n_states) return false;
    std::memcpy(dst, checkpoints[i] + MacCheckpoints::HEADER_BYTES + uint64_t(s0) * 16, size_t(count) * 16);
    return true;
  };
  return evaluate_against_checkpoints(s, gate_id_base, source_reader(source, user), mv, EvalCommit::CheckpointMemory, expected, rg, /*rereadable=*/false);
}
