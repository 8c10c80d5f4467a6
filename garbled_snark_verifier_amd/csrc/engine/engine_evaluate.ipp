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
  if (s->ct_cap != s->replays || (s->plan && !s->plan_retain)) return fail(GSV_ERR_INVALID, "evaluate needs the whole ciphertext stream resident (ct_capacity_replays == replays)");
  if (int rc = check_resident_stream(s, s->prog().n_ct * s->replays)) return rc;
  return launch(s, gate_id_base, true);
}

// What the three drivers of one evaluate_streaming_pass share
struct EvalPass {
  gsv_session* s;
  uint64_t gate_id_base;
  CtUploader& up;
  uint64_t seg_records;  // per instance: stride of the gate-order buffer
  B3Receiver& b3;        // BLAKE3 of the uploaded segments, when digests were asked for; verified mode: with the instances' outboards
  // `n` records per instance starting at stream index `base` -> the gate-order buffer through `st` (bounded page-locked chunks, hashed as read)
  int upload(uint64_t base, uint64_t n, hipStream_t st) {
    switch (up.upload(base, n, s->ct_gate.get(), st)) {
      case UploadError::None: return GSV_OK;
      case UploadError::EventWait: return fail(GSV_ERR_DEVICE, "event wait failed");
      case UploadError::Dry: return fail(GSV_ERR_EXHAUSTED, "Ciphertext source exhausted: instance " + std::to_string(up.dry_instance()) + " ran dry at record " + std::to_string(up.dry_record()));
      default: return fail(GSV_ERR_DEVICE, "ciphertext upload failed");
    }
  }
  // the `n` records per instance just uploaded to the gate-order buffer through `st`: hashed in front of their scatter
  int hash(uint64_t n, hipStream_t st) { return b3.feed(s->ct_gate.get(), seg_records, n, st); }
};
// Plan session over a ciphertext ring: the window (the whole pass) is launched FIRST; its calls wait on the device until the host's
// position counter says their segment has been uploaded.  Segment after segment: wait until the calls whose blocks this segment's
// blocks overwrite have completed (their flags), upload and scatter on the side stream, publish the segment's end.
static int evaluate_plan_ring(EvalPass& p) {
  gsv_session* const s = p.s;
  int rc = ensure_aux(s);
  for (size_t w = 0; w < s->sched.windows.size() && rc == GSV_OK; ++w) {
    const Schedule::Window& win = s->sched.windows[w];
    __atomic_store_n(s->sd.ct_pos.get(), (unsigned long long)win.ct0, __ATOMIC_RELEASE);
    rc = launch_plan_window(s, w, p.gate_id_base, true);
    bool window_done = false;
    for (uint32_t q = win.seg0; q < win.seg1 && rc == GSV_OK; ++q) {
      const Schedule::Segment& sg = s->sched.segments[q];
      uint32_t o0 = ~0u, o1 = 0;
      for (uint32_t k = sg.call0; k < sg.call1; ++k) if (s->sched.ovl1[k] > s->sched.ovl0[k]) { o0 = std::min(o0, s->sched.ovl0[k]); o1 = std::max(o1, s->sched.ovl1[k]); }
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
      if (rc == GSV_OK) __atomic_store_n(s->sd.ct_pos.get(), (unsigned long long)(sg.ct0 + sg.n_ct), __ATOMIC_RELEASE);
    }
    if (rc != GSV_OK) {
      // let the calls that still wait for ciphertexts run out (their results are discarded with the error) instead of hanging the stream
      __atomic_store_n(s->sd.ct_pos.get(), ~0ull, __ATOMIC_RELEASE);
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
  for (size_t w = 0; w < s->sched.windows.size() && rc == GSV_OK; ++w) {
    const Schedule::Window& win = s->sched.windows[w];
    for (uint32_t q = win.seg0; q < win.seg1 && rc == GSV_OK; ++q) {
      const Schedule::Segment& sg = s->sched.segments[q];
      // (the stream orders this segment's uploads behind the scatter of the previous one, which read the same buffer)
      rc = p.upload(sg.ct0, sg.n_ct, s->e->stream.get());
      if (rc == GSV_OK) rc = p.hash(sg.n_ct, s->e->stream.get());
      if (rc == GSV_OK) rc = permute_plan_calls(s, w, sg.call0, sg.call1, sg.ct0, p.seg_records, 1, nullptr, nullptr, nullptr);
    }
    // verified mode: every group value the segments uploaded so far have produced is compared before the window that reads them is launched
    if (rc == GSV_OK && p.b3.check) rc = p.b3.flush();
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
    if (rc == GSV_OK && p.b3.check) rc = p.b3.flush();  // verified mode: compared before the ring is scattered and launched
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
struct EvalVerify { B3Check check; const uint8_t* expected; uint64_t expected_len; };
static int evaluate_streaming_pass_inner(gsv_session* s, uint64_t gate_id_base, const CtUploader::Read& read, uint8_t* hashes, uint8_t* digests, EvalVerify* vf) {
  const Program& g = s->prog();
  if (s->plan) s->windows_launched = 0;
  // plan sessions: one window of the schedule per launch, its ciphertexts uploaded SEGMENT by segment (schedule.hpp: a gate-order buffer
  // holds the largest segment, the program-order device block the largest window); program sessions: one ring per launch
  const size_t n_inst = s->n_inst;
  HIPCHK(hipSetDevice(s->e->device));
  const uint64_t seg_records = s->plan ? s->plan_max_segment : s->ct_cap * g.n_ct;  // per instance: stride of the gate-order buffer
  if (seg_records) { int grc = ensure_ct_gate(s, n_inst * size_t(seg_records) * 16); if (grc) return grc; }  // (a sample drain before may have sized it for fewer instances)
  // With hashes asked for, T workers fold the chunks into the per-instance CBC-MACs beside the uploads (upload_pipeline.hpp; the
  // reference folds while reading, ciphertext_source.rs:36-107, and runs its finalized cases under into_par_iter: cut_and_choose/evaluator.rs:118-181)
  const size_t T = hashes ? std::max<size_t>(1, std::min<size_t>(std::min<size_t>(n_inst, 16), gsv_drain::usable_cores() > 1 ? gsv_drain::usable_cores() - 1 : 1)) : 0;
  CtUploader up(n_inst, seg_records, std::min<uint64_t>(std::max<uint64_t>(seg_records, 1), CT_STAGE_RECORDS), T, read);
  if (up.alloc() != hipSuccess) return fail(GSV_ERR_DEVICE, "cannot allocate the ciphertext staging buffers");
  B3Receiver b3(s->b3_eval, "the ciphertext stream of instance", vf ? &vf->check : nullptr);
  EvalPass p{s, gate_id_base, up, seg_records, b3};
  // every pass starts the hash afresh, and verifies from group 0 (the pass the safe-schedule fallback repeats too)
  if (digests) { int brc = b3.begin(n_inst, stream_records(s), seg_records, s->pass.b3_subtree_log2); if (brc) return brc; }
  if (s->plan) HIPCHK(hipMemsetAsync(s->sd.d_error.get(), 0, 4, s->e->stream.get()));
  HIPCHK(hipEventRecord(s->ev0.get(), s->e->stream.get()));
  int rc = s->plan ? (s->ct_ring ? evaluate_plan_ring(p) : evaluate_plan_windows(p)) : evaluate_program_rings(p);
  if (hipStreamSynchronize(s->e->stream.get()) != hipSuccess && rc == GSV_OK) rc = fail(GSV_ERR_DEVICE, "kernel failed");
  if (rc != GSV_OK) return rc;
  if (s->plan) { HIPCHK(hipEventRecord(s->ev1.get(), s->e->stream.get())); rc = gather_plan_outputs(s, true); if (rc) return rc; HIPCHK(hipStreamSynchronize(s->e->stream.get())); rc = check_plan_error(s); if (rc) return rc; }
  up.finish();
  // (before the MACs are written: a failure leaves both arrays untouched.)  The end of a verified pass compares the computed digests with
  // the commitments: the last chunk was read before the pass, what was uploaded is what counts
  if (digests) { rc = b3.finish(s->e->stream.get(), digests, vf ? vf->expected : nullptr, vf ? vf->expected_len : 0); if (rc) return rc; }
  if (hashes) up.digests(hashes);
  return GSV_OK;
}
static int evaluate_streaming_pass(gsv_session* s, uint64_t gate_id_base, const CtUploader::Read& read, uint8_t* hashes, uint8_t* digests, EvalVerify* vf = nullptr) {
  if (vf) s->mismatch = false;
  const int rc = evaluate_streaming_pass_inner(s, gate_id_base, read, hashes, digests, vf);
  if (rc == GSV_ERR_MISMATCH) {  // the stream differs from its outboard at the place the check holds
    s->mismatch = true; s->mismatch_instance = vf->check.bad_instance; s->mismatch_group = vf->check.bad_group; s->mismatch_record = vf->check.bad_record;
    s->ran = false;  // no outputs for a stream that did not verify: gsv_session_read_outputs fails as after a pass that never ran
  }
  return rc;
}
// The evaluator's side of the safe-schedule fallback (engine_drain.ipp, fall_back_to_safe_schedule): a pass that ended with a dependency wait
// giving up switches the session to one call per launch; a source that can be read again from the start (gc files) is then evaluated
// again at once, any other source gets the error with the remedy (its records have been consumed) and the host's repeat succeeds.
static int evaluate_streaming_impl(gsv_session* s, uint64_t gate_id_base, const std::function<int(size_t, uint64_t, uint8_t*, uint64_t)>& read, uint8_t* hashes, uint8_t* digests, bool rereadable = false, EvalVerify* vf = nullptr) {
  int rc = evaluate_streaming_pass(s, gate_id_base, read, hashes, digests, vf);
  if (rc != GSV_ERR_DEVICE || !s->plan || !s->dep_fault || s->safe_mode) return rc;
  const std::string first_error = g_err;
  if (fall_back_to_safe_schedule(s)) return fail(GSV_ERR_DEVICE, first_error + "; the fall-back to the safe schedule failed too: " + g_err);
  if (!rereadable) return fail(GSV_ERR_DEVICE, first_error + "; the session now runs the safe schedule (one call per launch): repeat the pass from gsv_session_set_evaluate_inputs");
  if (s->pass.drain_debug || s->pass.plan_debug) std::fprintf(stderr, "plan session: %s -- repeating the evaluation on the safe schedule (one call per launch)\n", first_error.c_str());
  return evaluate_streaming_pass(s, gate_id_base, read, hashes, digests, vf);
}
// In front of a verified pass, before anything is uploaded: every instance's outboard is loaded and bounds-checked against the SESSION's
// stream length and this pass's k — all of them before any is folded — and then, with `last_chunk`, its root — folded with the
// instance's last chunk — must be the commitment.  A difference there has no place in the stream: the mismatch names the instance
// alone.  No kernel has run when this fails.
//   load(i, k, n_records, out, why) -> the outboard of instance i, well-formed (load_outboard, check_outboard), or false
//   last_chunk(i, dst, n_records) -> 0 with the last n_records records of instance i's stream in dst; null: the roots are left to the end of the pass
using LoadOutboard = std::function<bool(size_t, uint32_t, uint64_t, std::vector<uint8_t>*, std::string*)>;
using LastChunk = std::function<int(size_t, uint8_t*, uint64_t)>;
static int prepare_verified_pass(gsv_session* s, EvalVerify& vf, const LoadOutboard& load, const LastChunk& last_chunk) {
  const uint32_t k = s->pass.b3_subtree_log2;
  if (int krc = check_b3_k(k)) return krc;
  const uint64_t total = stream_records(s), first_of_last = (Outboard::chunks(total) - 1) * 64;
  B3Check& c = vf.check;
  c.shape(s->n_inst, k, total);
  s->mismatch = false;
  std::string why;
  for (size_t i = 0; i < s->n_inst; ++i) if (!load(i, k, total, &c.bytes[i], &why)) return fail(GSV_ERR_INVALID, why);
  std::vector<uint8_t> last(size_t(total - first_of_last) * 16);
  for (size_t i = 0; last_chunk && i < s->n_inst; ++i) {
    if (last_chunk(i, last.data(), total - first_of_last) != 0)
      return fail(GSV_ERR_EXHAUSTED, "Ciphertext source exhausted: instance " + std::to_string(i) + " holds fewer than " + std::to_string(total) + " ciphertexts");
    Outboard o;
    uint8_t root[32];
    if (!Outboard::parse(c.bytes[i].data(), c.bytes[i].size(), &o, &why) || !o.root(last.data(), last.size(), root, &why)) return fail(GSV_ERR_INVALID, why);
    if (std::memcmp(root, vf.expected + vf.expected_len * i, size_t(vf.expected_len)) != 0) {
      s->mismatch = true; s->mismatch_instance = i; s->mismatch_group = s->mismatch_record = ~0ull;
      s->ran = false;
      return fail(GSV_ERR_MISMATCH, "outboard or last chunk of instance " + std::to_string(i) + " does not match the commitment");
    }
  }
  return GSV_OK;
}
// FileSource: instance i reads <dir>/gc_<indexes[i]>.bin (indexes == NULL: first_index + i).  Verified mode (outboard_dir): the
// outboards lie in files too, and a file's last chunk lies where the session's stream length puts it.
static int evaluate_from_files(gsv_session* s, uint64_t gate_id_base, const char* dir, const uint64_t* indexes, uint64_t first_index, uint8_t* hashes, uint8_t* digests,
                               const char* outboard_dir = nullptr, const uint8_t* expected = nullptr, uint64_t expected_len = 0) {
  if (!s || !dir) return fail(GSV_ERR_INVALID, "null argument");
  auto index = [&](size_t i) { return indexes ? indexes[i] : first_index + i; };
  GcFileSource files;
  std::string why;
  for (size_t i = 0; i < s->n_inst; ++i)
    if (!files.add(std::string(dir) + "/gc_" + std::to_string(index(i)) + ".bin", &why)) return fail(GSV_ERR_INVALID, why);
  EvalVerify vf{B3Check(), expected, expected_len};
  if (outboard_dir) {
    const int vrc = prepare_verified_pass(s, vf,
        [&](size_t i, uint32_t k, uint64_t n_records, std::vector<uint8_t>* out, std::string* w) { return load_outboard(OutboardWriter::path(outboard_dir, index(i)), k, n_records, out, w); },
        [&](size_t i, uint8_t* dst, uint64_t n) { return files.read(i, stream_records(s) - n, dst, n); });
    if (vrc) return vrc;
  }
  return evaluate_streaming_impl(s, gate_id_base, [&](size_t i, uint64_t first, uint8_t* dst, uint64_t n) { return files.read(i, first, dst, n); }, hashes, digests, /*rereadable=*/true, outboard_dir ? &vf : nullptr);
}
int gsv_session_evaluate_streaming(gsv_session* s, uint64_t gate_id_base, const char* dir, uint64_t first_index, uint8_t* hashes) {
  PassGuard pass_guard(s);  // destroys requested while this pass runs wait for its end (deferred release)
  return evaluate_from_files(s, gate_id_base, dir, nullptr, first_index, hashes, nullptr);
}
int gsv_session_evaluate_streaming_indexed(gsv_session* s, uint64_t gate_id_base, const char* dir, const uint64_t* indexes, uint8_t* hashes) {
  PassGuard pass_guard(s);  // destroys requested while this pass runs wait for its end (deferred release)
  if (!indexes) return fail(GSV_ERR_INVALID, "null index list");
  return evaluate_from_files(s, gate_id_base, dir, indexes, 0, hashes, nullptr);
}
int gsv_session_evaluate_streaming_source(gsv_session* s, uint64_t gate_id_base, gsv_ct_source_fn source, void* user, uint8_t* hashes) {
  PassGuard pass_guard(s);  // destroys requested while this pass runs wait for its end (deferred release)
  if (!s || !source) return fail(GSV_ERR_INVALID, "null argument");
  return evaluate_streaming_impl(s, gate_id_base, [&](size_t i, uint64_t first, uint8_t* dst, uint64_t n) -> int { return source(user, i, first, dst, n); }, hashes, nullptr);
}
// The three above with either commitment or both (blake3_digests == NULL is what they do)
int gsv_session_evaluate_streaming_commit(gsv_session* s, uint64_t gate_id_base, const char* dir, const uint64_t* indexes, uint64_t first_index, uint8_t* cbcmac_hashes, uint8_t* blake3_digests) {
  PassGuard pass_guard(s);  // destroys requested while this pass runs wait for its end (deferred release)
  return evaluate_from_files(s, gate_id_base, dir, indexes, first_index, cbcmac_hashes, blake3_digests);
}
// ... and verified against outboards and commitments the caller trusts (include/gsv_engine.h, "BLAKE3 outboards")
static const char* const VERIFIED_OVER_A_RING =
    "verified streaming is not available for plan sessions over a ciphertext ring (retain_stream = GSV_STREAM_RING): their pass is one launch that waits on the device for the host's "
    "stream position, and a host that stops feeding it would leave that launch to the watchdog; use launch windows (retain_stream = 0)";
int gsv_session_evaluate_streaming_verified(gsv_session* s, uint64_t gate_id_base, const char* dir, const uint64_t* indexes, uint64_t first_index, const char* outboard_dir, const uint8_t* expected,
                                            uint64_t expected_len, uint8_t* cbcmac_hashes, uint8_t* blake3_digests) {
  PassGuard pass_guard(s);  // destroys requested while this pass runs wait for its end (deferred release)
  if (!s || !dir || !outboard_dir || !expected || !blake3_digests) return fail(GSV_ERR_INVALID, "null argument");
  if (expected_len != 16 && expected_len != 32) return fail(GSV_ERR_INVALID, "expected_len must be 16 (a truncated digest) or 32");
  if (s->plan && s->ct_ring) return fail(GSV_ERR_INVALID, VERIFIED_OVER_A_RING);
  return evaluate_from_files(s, gate_id_base, dir, indexes, first_index, cbcmac_hashes, blake3_digests, outboard_dir, expected, expected_len);
}
int gsv_session_mismatch_info(const gsv_session* s, uint64_t* instance, uint64_t* group, uint64_t* first_record) {
  if (!s) return fail(GSV_ERR_INVALID, "null session");
  if (!s->mismatch) return fail(GSV_ERR_INVALID, "the session's last verified pass found no mismatch");
  if (instance) *instance = s->mismatch_instance;
  if (group) *group = s->mismatch_group;
  if (first_record) *first_record = s->mismatch_record;
  return GSV_OK;
}
int gsv_session_evaluate_streaming_source_commit(gsv_session* s, uint64_t gate_id_base, gsv_ct_source_fn source, void* user, uint8_t* cbcmac_hashes, uint8_t* blake3_digests) {
  PassGuard pass_guard(s);  // destroys requested while this pass runs wait for its end (deferred release)
  if (!s || !source) return fail(GSV_ERR_INVALID, "null argument");
  return evaluate_streaming_impl(s, gate_id_base, [&](size_t i, uint64_t first, uint8_t* dst, uint64_t n) -> int { return source(user, i, first, dst, n); }, cbcmac_hashes, blake3_digests);
}
// The generic source, verified (include/gsv_engine.h, "Commitments on the callback paths"): the outboards come in memory.  With the last
// chunks (up-front mode) they are authenticated against `expected` before the source is called at all; without (deferred mode) they are
// checked for form only, and the computed digests meet `expected` at the end of the pass.
int gsv_session_evaluate_streaming_source_verified(gsv_session* s, uint64_t gate_id_base, gsv_ct_source_fn source, void* user, const uint8_t* const* outboards, const uint64_t* outboard_bytes,
                                                   const uint8_t* last_chunks, const uint8_t* expected, uint64_t expected_len, uint8_t* cbcmac_hashes, uint8_t* blake3_digests) {
  PassGuard pass_guard(s);  // destroys requested while this pass runs wait for its end (deferred release)
  if (!s || !source || !outboards || !outboard_bytes || !expected || !blake3_digests) return fail(GSV_ERR_INVALID, "null argument");
  if (expected_len != 16 && expected_len != 32) return fail(GSV_ERR_INVALID, "expected_len must be 16 (a truncated digest) or 32");
  if (s->plan && s->ct_ring) return fail(GSV_ERR_INVALID, VERIFIED_OVER_A_RING);
  EvalVerify vf{B3Check(), expected, expected_len};
  const int vrc = prepare_verified_pass(s, vf,
      [&](size_t i, uint32_t k, uint64_t n_records, std::vector<uint8_t>* out, std::string* why) {
        if (!outboards[i]) { *why = "null outboard"; return false; }
        if (!check_outboard("outboards[" + std::to_string(i) + "]", outboards[i], outboard_bytes[i], k, n_records, why)) return false;
        out->assign(outboards[i], outboards[i] + outboard_bytes[i]);
        return true;
      },
      last_chunks ? LastChunk([&](size_t i, uint8_t* dst, uint64_t n) { if (n) std::memcpy(dst, last_chunks + 1024 * i, size_t(n) * 16); return 0; }) : LastChunk());
  if (vrc) return vrc;
  return evaluate_streaming_impl(s, gate_id_base, [&](size_t i, uint64_t first, uint8_t* dst, uint64_t n) -> int { return source(user, i, first, dst, n); }, cbcmac_hashes, blake3_digests, /*rereadable=*/false, &vf);
}
