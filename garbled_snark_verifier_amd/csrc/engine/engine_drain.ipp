// Part of engine.cpp: the streaming garbler — drain pipeline (gather, D2H, CBC-MAC / files / sink), garble || evaluate pairs, the safe-schedule fallback.
// Garble + drain.  The launch is cut into segments of one device ring (ct_cap replays).  After a segment the ring
// (program order) is gathered into a second device buffer in GATE order (a ~ms kernel between two garbling launches,
// which own every CU while they run); while the next segment is garbled, host threads copy that buffer out with plain
// sequential D2H copies (the copy engines work beside the kernel), fold each instance's bytes into its CBC-MAC (strictly
// serial per instance, hence the host: ciphertext_hasher.rs:23-29) and optionally append them to gc_<index>.bin
// (ciphertext_repository.rs:94-127).
static int ensure_drain(gsv_session* s, size_t T, uint64_t seg_records, int group) {
  // records per chunk: 16 MiB by default — measured on the MI355X box (tools/d2h_bw.py) a D2H copy stream moves 39-48 GB/s in 4 MiB
  // pieces and 54-57 GB/s from 16 MiB up; the buffers are page-locked once per session, not per call as in round 1
  const uint64_t chunk = std::min<uint64_t>(std::max<uint64_t>(seg_records, 1), (s->pass.drain_chunk_mb << 20) / 16);
  if (s->drain && s->drain->workers.size() >= T && s->drain->chunk == chunk && s->drain->group == group) return GSV_OK;
  std::vector<CbcMacHost> keep;
  if (s->drain) keep = s->drain->macs;
  s->drain.reset();
  s->drain.reset(new gsv_drain());
  gsv_drain& d = *s->drain;
  d.macs = keep;
  d.chunk = chunk;
  d.group = group;
  // Copy sets in flight at once.  Round 3, whole Miller-loop pass at 64 instances (tools/e2e_plan_drain.py, profiles/r03_e2e/): 1 set
  // 48 GB/s, 2-4 sets 50 GB/s, 6 sets 40 GB/s, 12 sets 41 GB/s — the link is full with two or three 16 MiB copies queued.
  const int n_copy_streams = s->pass.drain_copies;
  bool ok = true;
  for (int k = 0; k < n_copy_streams && ok; ++k) {
    Stream st;
    ok = create_side_stream(st, s->kn.side_stream_priority) == hipSuccess;
    if (ok) { d.copy_gate.idle.push_back(st.get()); d.copy_streams.push_back(std::move(st)); }
  }
  d.workers.resize(T);
  for (gsv_drain::Worker& w : d.workers) {
    for (auto& set : w.pinned) for (int g = 0; g < group; ++g) ok = ok && set[g].alloc(chunk * 16, hipHostMallocDefault) == hipSuccess;
    ok = ok && w.done.create(hipEventBlockingSync | hipEventDisableTiming) == hipSuccess;
  }
  if (!ok) { s->drain.reset(); return fail(GSV_ERR_DEVICE, "cannot allocate the drain buffers"); }
  return GSV_OK;
}

// Discarding form: calls [c0, c1) of a plan (or the whole program launch), ciphertexts stay in / are overwritten on the device.
static int garble_discard(gsv_session* s, uint64_t gate_id_base, size_t c0, size_t c1) {
  HIPCHK(hipSetDevice(s->e->device));
  HIPCHK(hipEventRecord(s->ev0.get(), s->e->stream.get()));
  int rc = GSV_OK;
  if (s->plan) {
    size_t w0 = 0, w1 = 0;
    if (c0 == 0) HIPCHK(hipMemsetAsync(s->ps.d_error.get(), 0, 4, s->e->stream.get()));
    if (c0 == 0) s->windows_launched = 0;
    if (s->ring()) __atomic_store_n(s->ps.ct_pos.get(), ~0ull, __ATOMIC_RELEASE);  // nothing reads the ciphertexts: every block of the ring is free at once
    rc = window_range(s, c0, c1, &w0, &w1);
    for (size_t w = w0; w < w1 && rc == GSV_OK; ++w) rc = launch_plan_window(s, w, gate_id_base, false);
    if (rc == GSV_OK) {
      HIPCHK(hipEventRecord(s->ev1.get(), s->e->stream.get()));
      if (c1 == s->plan->calls.size()) rc = gather_plan_outputs(s, false); else { s->ran = true; s->last_eval = false; }
    }
  } else {
    rc = launch(s, gate_id_base, false);
  }
  if (rc == GSV_OK) { HIPCHK(hipStreamSynchronize(s->e->stream.get())); s->garbled = !s->plan || s->retain(); }
  if (rc == GSV_OK && s->plan) rc = check_plan_error(s);
  return rc;
}

// Garble -> evaluate on the device (gsv_session_garble_evaluate): the evaluator session consumes window k from the garbler's
// program-order block while the garbler writes window k+1 into the other one of two blocks.
struct PairState {
  Stream stream;                           // the evaluator's launches
  Stream gstream;                          // CU-masked pairs: the garbler's launches (else they go to the engine's stream)
  Event ready;                             // engine stream -> gstream hand-over at the start of a pass
  Event garbled[2], evaluated[2];
};
gsv_session::gsv_session() = default;
gsv_session::~gsv_session() { (void)hipSetDevice(e->device); (void)hipStreamSynchronize(e->stream.get()); }  // ... then the members release, in reverse order
static int ensure_pair(gsv_session* s) {
  if (!s->ct_alt) DEVALLOC(s->ct_alt, s->n_inst * size_t(s->ct_stride()) * 16, "the second ciphertext block (garble -> evaluate)");
  if (!s->pair) {
    std::unique_ptr<PairState> ps(new PairState());
    // The evaluator's stream: same priority as the engine's, on ANOTHER hardware queue.  Which queue a new stream lands on is the
    // runtime's business (round-robin over a few), so every candidate is probed — a one-thread kernel on the engine's stream waits up to
    // 5 ms for a one-thread kernel on the candidate — and the ones that queue up behind the engine's stream are kept alive until a
    // good one is found (the round-robin moves on), then destroyed.  No overlapping stream among eight: the last one serves (the pair
    // is still correct, window k is then evaluated after window k+1 has been garbled instead of beside it).
    // Round 5: the two long launches get DISJOINT sets of CUs through CU-masked streams (hipExtStreamCreateWithCUMask): a masked stream
    // owns a hardware queue of its own (the mask is a queue property), so the overlap no longer depends on which queue the runtime's
    // round-robin picks, and neither launch's waiting workgroups — a window holds more calls than run at once, the rest spin on their
    // dependency flags with a whole CU's LDS each — can sit on the CUs the other one needs (the 40 - 65 s run-to-run spread of round 4).
    // Three quarters of the CUs garble (two AES blocks per AND), a quarter evaluates (one).  The mask bits alternate in blocks of eight,
    // 3 : 1: whichever way the runtime maps bits to XCDs / shader engines, every XCD keeps CUs of both launches.  GSV_PAIR_CU_MASK=0, or a
    // runtime that refuses the masks, falls back to the probed unmasked stream below.
    if (s->pass.pair_cu_mask) {
      hipDeviceProp_t prop;
      if (hipGetDeviceProperties(&prop, s->e->device) == hipSuccess && prop.multiProcessorCount >= 32) {
        const uint32_t n_cu = uint32_t(prop.multiProcessorCount), words = (n_cu + 31) / 32;
        std::vector<uint32_t> gm(words, 0), em(words, 0);
        for (uint32_t i = 0; i < n_cu; ++i) (((i / 8) % 4 == 3) ? em : gm)[i / 32] |= 1u << (i % 32);
        hipStream_t g = nullptr, e2 = nullptr;
        const bool made = hipExtStreamCreateWithCUMask(&g, words, gm.data()) == hipSuccess && hipExtStreamCreateWithCUMask(&e2, words, em.data()) == hipSuccess;
        Stream g_owner(g), e2_owner(e2);  // (released here when anything failed)
        if (made && ps->ready.create(hipEventDisableTiming) == hipSuccess) {
          ps->gstream = std::move(g_owner); ps->stream = std::move(e2_owner);
          if (s->pass.drain_debug) std::fprintf(stderr, "garble -> evaluate: CU-masked streams, %u CUs garble, %u evaluate\n", n_cu - n_cu / 4, n_cu / 4);
        } else (void)hipGetLastError();
      }
    }
    if (!ps->stream) {
      std::vector<Stream> rejected;  // (destroyed when the search ends)
      uint32_t* const word = s->ps.d_error.as<uint32_t>() + 4;
      for (int attempt = 0; attempt < 8 && !ps->stream; ++attempt) {
        Stream cand_owner;
        if (cand_owner.create(hipStreamNonBlocking) != hipSuccess) break;
        const hipStream_t cand = cand_owner.get();
        uint32_t result[2] = {0, 0};
        const bool probed = hipMemsetAsync(word, 0, 8, s->e->stream.get()) == hipSuccess && hipStreamSynchronize(s->e->stream.get()) == hipSuccess &&
                            gsvk_probe_overlap(word, 500000ull, s->e->stream.get(), cand) == 0 && hipStreamSynchronize(cand) == hipSuccess &&
                            hipStreamSynchronize(s->e->stream.get()) == hipSuccess && hipMemcpy(result, word, 8, hipMemcpyDeviceToHost) == hipSuccess;
        if (!probed || result[1] == 1u || attempt == 7) ps->stream = std::move(cand_owner);
        else rejected.push_back(std::move(cand_owner));
        if (s->pass.drain_debug) std::fprintf(stderr, "garble -> evaluate: candidate stream %d %s\n", attempt, !probed ? "could not be probed" : result[1] == 1u ? "overlaps the engine's stream" : "queues behind the engine's stream");
      }
      rejected.clear();
      if (!ps->stream) return fail(GSV_ERR_DEVICE, "cannot create the evaluator's stream");
    }
    for (int b = 0; b < 2; ++b) {
      HIPCHK(ps->garbled[b].create(hipEventDisableTiming));
      HIPCHK(ps->evaluated[b].create(hipEventDisableTiming));
    }
    s->pair = std::move(ps);
  }
  return GSV_OK;
}

// Follows the RUNNING window w through the completion counters its workgroups write into mapped host memory (kernels.hip, epilogue)
// until calls [k0, k1) of the plan have completed for every instance group, or the window's launch itself has finished (*window_done).
static int wait_calls_done(gsv_session* s, size_t w, uint32_t k0, uint32_t k1, bool* window_done, hipStream_t launch_stream = nullptr) {
  if (!launch_stream) launch_stream = s->e->stream.get();  // the stream the running window was launched on
  const Schedule::Window& win = s->sched().windows[w];
  const uint32_t n_wg = uint32_t(s->launch_groups());  // workgroups that count a call done (one per instance under BLAKE3)
  const auto t0 = std::chrono::steady_clock::now();
  bool reported = false;
  // Host-side deadline, progress based like the device's watchdog (kernels.hip) and longer than it: the device gives up after
  // GSV_DEP_WAIT_SECONDS (default 60) without a completed call of an instance group and then ENDS its launch, which the stream query below
  // sees; this deadline covers the device that never comes back at all (no counter of the window has moved for twice that time + 30 s).
  const double deadline = 2.0 * s->pass.dep_wait_seconds + 30.0;
  uint64_t last_sum = ~0ull;
  auto last_move = t0;
  uint32_t polls = 0;
  while (!*window_done && k0 < k1) {
    bool all = true;
    for (uint32_t k = k0; k < k1 && all; ++k) all = __atomic_load_n(s->ps.done.get() + k, __ATOMIC_ACQUIRE) == n_wg;
    if (all) break;
    const hipError_t q = hipStreamQuery(launch_stream);
    if (q == hipSuccess) { *window_done = true; break; }
    if (q != hipErrorNotReady) {  // a failed launch / a lost device is neither "done" nor "running": the caller's error path must run
      (void)hipGetLastError();
      return fail(GSV_ERR_DEVICE, std::string("the window's launch failed while its stream was being drained: ") + hipGetErrorString(q));
    }
    std::this_thread::sleep_for(std::chrono::microseconds(100));
    if ((++polls & 1023u) == 0) {  // every ~0.1 s: has any call of the window completed for another workgroup?
      uint64_t sum = 0;
      for (uint32_t k = win.call0; k < win.call1; ++k) sum += __atomic_load_n(s->ps.done.get() + k, __ATOMIC_RELAXED);
      const auto now = std::chrono::steady_clock::now();
      if (sum != last_sum) { last_sum = sum; last_move = now; }
      else if (std::chrono::duration<double>(now - last_move).count() > deadline)
        return fail(GSV_ERR_DEVICE, "no call of the running window has completed for " + std::to_string(int(deadline)) + " s and its launch has not ended: giving up on the device");
    }
    if (!reported && s->pass.drain_debug && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 3.0) {
      reported = true;
      std::string msg;
      for (uint32_t k = win.call0; k < win.call1; ++k)
        if (s->ps.done.get()[k] != n_wg) msg += " " + std::to_string(k) + "(" + std::to_string(s->ps.done.get()[k]) + "/" + std::to_string(n_wg) + (s->ring() ? ",need " + std::to_string(s->sched().ring_need[k]) + ",ready " + std::to_string(s->sched().seg_end[k]) : "") + ")";
      std::fprintf(stderr, "drain debug: waiting > 3 s for calls [%u, %u) of window %zu; host position %llu; unfinished:%s\n", k0, k1, w, s->ps.ct_pos.get() ? (unsigned long long)*s->ps.ct_pos.get() : 0ull, msg.substr(0, 1500).c_str());
    }
  }
  return GSV_OK;
}
// the side stream and the device-written completion counters of a session whose stream leaves the device while a window runs
// The gate-order buffers (ct_gate + the drain pipeline's further ones) hold `bytes` each — or are released and ct_gate re-allocated.  A
// sample drain (gsv_session_set_drain_instances) sizes them for the sample; a later call over more instances (a full drain, or any
// evaluate_streaming: the evaluator uploads EVERY instance's stream) must not write past them.
static int ensure_ct_gate(gsv_session* s, size_t bytes) {
  if (s->ct_gate && s->ct_gate.bytes() >= bytes) return GSV_OK;
  if (s->ct_gate || !s->ct_gate_more.empty()) {
    HIPCHK(hipStreamSynchronize(s->e->stream.get()));
    if (s->aux_stream) HIPCHK(hipStreamSynchronize(s->aux_stream.get()));
    s->ct_gate_more.clear(); s->ct_gate.reset();
  }
  DEVALLOC(s->ct_gate, bytes, "the gate-order ciphertext buffer");
  return GSV_OK;
}
static int ensure_aux(gsv_session* s) {
  if (!s->aux_stream) HIPCHK(create_side_stream(s->aux_stream, s->kn.side_stream_priority));
  if (!s->ps.done) return fail(GSV_ERR_INVALID, "internal: a plan session without completion counters");  // (allocated with its call descriptors)
  return GSV_OK;
}

// The gate-order buffers a call's pipeline runs over (drain_pipeline.hpp, DrainWorkers): ct_gate and as many further ones as `n_units`
// drain units (segments of plans, rings of programs) can use.
static std::vector<void*> drain_gate_buffers(gsv_session* s, size_t n_units, size_t n_inst, uint64_t seg_records, bool want_host) {
  std::vector<void*> gate_bufs(1, s->ct_gate.get());
  size_t want = 1;
  if (seg_records && n_units > 1 && want_host) {  // (BLAKE3 alone: a buffer is free again when the hash kernels of its segment have finished, one serves)
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    const size_t buf_bytes = n_inst * size_t(seg_records) * 16;
    // up to eight buffers, within half of the free memory and 32 GB (allocating device memory takes time too: ~25 GB/s)
    want = std::min<size_t>(std::min<size_t>(8, 1 + size_t(double(free_b) * 0.5 / double(buf_bytes))), std::max<size_t>(2, size_t(32e9 / double(buf_bytes))));
    if (s->pass.drain_depth) want = s->pass.drain_depth;
  }
  while (1 + s->ct_gate_more.size() < want) {
    DevBuf q;
    if (q.alloc(s->ct_gate.bytes()) != hipSuccess) break;  // (every buffer of the pipeline has ct_gate's capacity)
    s->ct_gate_more.push_back(std::move(q));
  }
  for (const DevBuf& q : s->ct_gate_more) if (gate_bufs.size() < want) gate_bufs.push_back(q.get());
  return gate_bufs;
}
// What the device loops of one garble_streaming_pass share
struct DrainPass {
  gsv_session *s, *ev;             // ev: the evaluator of a garble || evaluate pair, or null
  uint64_t gate_id_base;
  size_t pw0, n_inst;              // plans: the first window of this call; instances whose streams leave the device
  uint64_t seg_records;            // records between two instances in a gate-order buffer
  bool want_drain;                 // finished segments are brought into gate order
  std::vector<void*> gate_bufs;
  DrainWorkers& workers; GarbleCommit& commit; DrainStats& stats;  // commit: what is hashed or checked in the gate-order buffers
  hipStream_t gs;                  // the stream the garbler's windows are launched on
  hipEvent_t device_done;          // not null: the host thread sleeps on this blocking-sync event instead of spinning in hipStreamSynchronize
  std::chrono::steady_clock::time_point t_last_pub;  // ring diagnostics: the last publication of the host's position ...
  double worst_gap;                                  // ... and the longest interval between two
  void* gate() const { return gate_bufs[workers.next_buffer()]; }  // the gate-order buffer the next segment goes to
  bool wait_device(hipStream_t st) const { return device_done ? hipEventRecord(device_done, st) == hipSuccess && hipEventSynchronize(device_done) == hipSuccess : hipStreamSynchronize(st) == hipSuccess; }
};
// One window of a plan: launched (in a pair: handed to the evaluator as well), then drained segment by segment while it runs.
static int drain_plan_window(DrainPass& p, size_t w) {
  gsv_session *const s = p.s, *const ev = p.ev;
  const hipStream_t gs = p.gs;
  DrainStats& st = p.stats;
  void* block = s->CT.get();
  const int b = int(w & 1);
  if (ev) {
    // window w goes to block w & 1; the evaluator must be done with what that block held (window w - 2)
    block = b ? s->ct_alt.get() : s->CT.get();
    if (w >= p.pw0 + 2 && hipStreamWaitEvent(gs, s->pair->evaluated[b].get(), 0) != hipSuccess) return fail(GSV_ERR_DEVICE, "hipStreamWaitEvent failed");
  }
  int rc = launch_plan_window(s, w, p.gate_id_base, false, block, gs);
  if (rc != GSV_OK) return rc;
  if (ev) {
    if (hipEventRecord(s->pair->garbled[b].get(), gs) != hipSuccess || hipStreamWaitEvent(s->pair->stream.get(), s->pair->garbled[b].get(), 0) != hipSuccess) return fail(GSV_ERR_DEVICE, "event hand-over failed");
    rc = launch_plan_window(ev, w, p.gate_id_base, true, block, s->pair->stream.get());
    if (rc != GSV_OK) return rc;
    if (hipEventRecord(s->pair->evaluated[b].get(), s->pair->stream.get()) != hipSuccess) return fail(GSV_ERR_DEVICE, "hipEventRecord failed");
  }
  // The window is running.  Its segments leave the device one after the other, in stream order, each as soon as every call of it
  // has completed for every instance group: the host follows the completion flags of the running launch (a page-locked copy,
  // refreshed through a side stream), brings the finished segment into gate order with a gather kernel on that side stream — the
  // session's schedule leaves it a few CUs — and hands it to the workers, while the window goes on garbling.
  const Schedule::Window& win = s->sched().windows[w];
  bool window_done = false;
  for (uint32_t q = win.seg0; p.want_drain && q < win.seg1; ++q) {
    const Schedule::Segment& sg = s->sched().segments[q];
    const bool last = q + 1 == win.seg1;
    const auto t0 = std::chrono::steady_clock::now();
    if (!last && (rc = wait_calls_done(s, w, sg.call0, sg.call1, &window_done, gs)) != GSV_OK) return rc;
    if (last && !window_done) {
      // the last segment ends with the window: sleep on the stream (on a blocking-sync event when the workers own the cores)
      if (!p.wait_device(gs)) return fail(GSV_ERR_DEVICE, "kernel failed");
      window_done = true;
    }
    st.t_wait_device += drain_secs(t0);
    const double waited = p.workers.wait_buffer();  // the gate-order buffer this segment goes to is free again
    st.t_wait_drain += waited;
    const auto tg = std::chrono::steady_clock::now();
    rc = permute_plan_calls(s, w, sg.call0, sg.call1, sg.ct0, p.seg_records, 0, block, p.gate(), s->aux_stream.get());
    if (rc != GSV_OK) return rc;
    if ((rc = p.commit.feed(p.gate(), p.seg_records, sg.n_ct, s->aux_stream.get())) != GSV_OK) return rc;  // (behind the gather, on the side stream)
    if (hipStreamSynchronize(s->aux_stream.get()) != hipSuccess) return fail(GSV_ERR_DEVICE, "ciphertext gather failed");
    p.commit.submit();
    st.t_gather += drain_secs(tg);
    if (s->ring()) {
      __atomic_store_n(s->ps.ct_pos.get(), (unsigned long long)(sg.ct0 + sg.n_ct), __ATOMIC_RELEASE);  // the calls whose blocks overlap this segment's may write now
      const double gap = drain_secs(p.t_last_pub);
      if (gap > p.worst_gap) {
        p.worst_gap = gap;
        char buf[256];
        std::snprintf(buf, sizeof buf, "longest interval between two positions %.2f s, before segment %u (calls [%u, %u)): %.2f s waiting for its calls, %.2f s for a free gate-order buffer, %.2f s gathering", gap, q,
                      sg.call0, sg.call1, std::chrono::duration<double>(tg - t0).count() - waited, waited, drain_secs(tg));
        s->ring_diag = buf;
      }
      p.t_last_pub = std::chrono::steady_clock::now();
    }
    st.drained_records += sg.n_ct;
    p.workers.push(sg.n_ct, sg.ct0);
  }
  if (hipStreamSynchronize(gs) != hipSuccess) return fail(GSV_ERR_DEVICE, "kernel failed");
  return GSV_OK;
}
// One ring of a program session, replays [r0, r1): garbled, gathered into gate order on the engine's stream, handed to the workers.
static int drain_program_ring(DrainPass& p, uint64_t r0, uint64_t r1) {
  gsv_session* const s = p.s;
  const uint64_t n_ct = s->prog().n_ct, n_records = (r1 - r0) * n_ct, base = r0 * n_ct;  // per instance, in this ring; stream index of its first record
  // ring slots are (replay % ct_cap): a segment starts at a multiple of ct_cap, so its replays sit in slots 0..n_rep-1
  int rc = launch(s, p.gate_id_base, false, r0, r1 - r0);
  if (rc != GSV_OK) return rc;
  p.stats.t_wait_drain += p.workers.wait_buffer();
  if (gsvk_gather_segment(s->CT.get(), s->ct_stride(), s->dp->ct_pos.as<const uint32_t>(), n_ct, uint32_t(r1 - r0), uint32_t(p.n_inst), p.gate(), p.seg_records, 0, s->e->stream.get()) != 0)
    return fail(GSV_ERR_DEVICE, "ciphertext gather launch failed");
  if ((rc = p.commit.feed(p.gate(), p.seg_records, n_records, s->e->stream.get())) != GSV_OK) return rc;
  // the workers own the cores when there is one chain per core: this thread then sleeps on a blocking-sync event instead of
  // spinning in hipStreamSynchronize
  const auto t0 = std::chrono::steady_clock::now();
  if (!p.wait_device(s->e->stream.get())) return fail(GSV_ERR_DEVICE, "kernel failed");
  p.stats.t_wait_device += drain_secs(t0);
  p.stats.drained_records += n_records;
  p.commit.submit();
  p.workers.push(n_records, base);
  return GSV_OK;
}

// `ev`: an evaluator session over the same plan / schedule (plan sessions that do not retain the stream): every window is evaluated
// straight from the garbler's device block while the next window is garbled.
static int garble_streaming_pass(gsv_session* s, uint64_t gate_id_base, size_t c0, size_t c1, const DrainSink& sink, int n_threads, gsv_session* ev) {
  if (int urc = plan_session_usable(s)) return urc;
  if (ev) if (int urc = plan_session_usable(ev)) return urc;
  if (!sink.any() && !ev) return garble_discard(s, gate_id_base, c0, c1);  // garble only (output labels, device-rate measurements of long plans / chains)
  const Program& g = s->prog();
  // program sessions: segments of one ring (ct_cap replays of n_ct records); plan sessions: one WINDOW of the schedule per segment
  size_t pw0 = 0, pw1 = 0;
  if (s->plan) { int wrc = window_range(s, c0, c1, &pw0, &pw1); if (wrc) return wrc; }
  // (plan sessions: the stream leaves the device in SEGMENTS of a window, a gate-order buffer holds the largest segment)
  const uint64_t n_ct = s->plan ? s->max_segment() : g.n_ct, seg = s->plan ? 1 : s->ct_cap;
  const uint64_t first = s->plan ? pw0 : 0, total = s->plan ? pw1 : s->replays;
  const bool new_pass = s->plan ? c0 == 0 : true;
  // the instances whose streams leave the device: all of them, or the first drain_instances (every instance is garbled either way)
  const size_t n_inst = s->drain_instances ? std::min(s->drain_instances, s->n_inst) : s->n_inst;
  const bool want_drain = sink.any();    // finished segments are brought into gate order ...
  const bool want_host = sink.host();    // ... and copied out by the workers
  if (const char* why = sink.refusal(s->ring(), ev != nullptr)) return fail(GSV_ERR_INVALID, why);
  if (sink.mac_check_dir) clear_mismatch(s);
  if (s->plan && new_pass) s->windows_launched = 0;
  const size_t GROUP = size_t(gsv_drain::group_for(n_inst, s->pass.drain_group));
  const size_t n_groups = (n_inst + GROUP - 1) / GROUP;
  // a worker MACs GROUP streams side by side at ~3e8 blocks/s (four chains, AES-NI) or ~1e9 (sixteen, VAES): a dozen / four of them keep
  // up with the PCIe link, 32 leave room for slow cores without page-locking more than 4 GB (16 GB) of chunk buffers
  size_t T = n_threads > 0 ? size_t(n_threads) : std::max<size_t>(1, std::min<size_t>(std::min<size_t>(n_groups, GROUP == 16 ? 8 : 32), std::thread::hardware_concurrency()));
  T = std::min(T, n_groups);
  HIPCHK(hipSetDevice(s->e->device));
  const uint64_t seg_records = seg * n_ct;  // per instance
  if (want_drain) {
    if (seg_records) { int grc = ensure_ct_gate(s, n_inst * size_t(seg_records) * 16); if (grc) return grc; }
    int rc = want_host ? ensure_drain(s, T, seg_records, int(GROUP)) : GSV_OK;
    if (rc) return rc;
  }
  // Declared before the pools and the gc files: its own threads are joined, and its files removed, after theirs (engine_garble_commit.ipp)
  GarbleCommit commit(s, sink);
  if (int rc = commit.begin(new_pass, n_inst, seg_records)) return rc;
  if (ev && (s->ring() || ev->ring())) return fail(GSV_ERR_INVALID, "garble || evaluate pairs need sessions with explicit launch windows (window_ct_records, e.g. 1 << 28): the default is one whole-pass window over a ciphertext ring");
  if (ev) { int rc = ensure_pair(s); if (rc) return rc; }
  if (s->ring()) __atomic_store_n(s->ps.ct_pos.get(), (unsigned long long)(s->plan && pw0 < s->sched().windows.size() ? s->sched().windows[pw0].ct0 : 0), __ATOMIC_RELEASE);
  if (s->plan && want_drain) { int rc = ensure_aux(s); if (rc) return rc; }
  if (s->plan && new_pass) HIPCHK(hipMemsetAsync(s->ps.d_error.get(), 0, 4, s->e->stream.get()));  // a new pass starts with a clean dependency-wait flag
  if (ev && new_pass) HIPCHK(hipMemsetAsync(ev->ps.d_error.get(), 0, 4, s->e->stream.get()));
  std::vector<CbcMacHost> no_macs;
  if (want_host && (new_pass || s->drain->macs.size() != n_inst)) s->drain->macs.assign(n_inst, CbcMacHost());  // a new pass starts from h = 0; later slices chain
  std::vector<CbcMacHost>& macs = want_host ? s->drain->macs : no_macs;
  GcFiles files;  // (removed again on every return but the last)
  if (std::string failed; sink.dir && !files.open(sink.dir, sink.first_index, n_inst, new_pass ? "wb" : "ab", &failed)) return fail(GSV_ERR_INVALID, "cannot create " + failed);
  if (int rc = commit.open(s->plan ? s->aux_stream.get() : s->e->stream.get())) return rc;  // (the stream the segments are gathered on)
  DrainShape shape;
  shape.device = s->e->device; shape.n_inst = n_inst; shape.group = GROUP; shape.n_workers = want_host ? T : 0;
  shape.chunk = want_host ? s->drain->chunk : 0; shape.seg_records = seg_records; shape.blocking_wait = T > 8;
  if (want_drain) {
    size_t n_units = size_t((total - first + seg - 1) / seg);  // drain units of this call: segments (plans) or rings
    if (s->plan) { n_units = 0; for (size_t w = pw0; w < pw1; ++w) n_units += s->sched().windows[w].seg1 - s->sched().windows[w].seg0; }
    shape.gate_bufs = drain_gate_buffers(s, n_units, n_inst, seg_records, want_host);
  }
  // The pool is declared after everything its threads use — the gate-order buffers, `macs`, `files`, the checkpoint files of `commit`:
  // it is joined first, however this function returns.  Its threads run members of the pool (drain_pipeline.hpp), never a lambda over the locals here.
  DrainWorkers workers(s->drain.get(), shape, sink, macs, files, commit.err, commit.checkpoints());
  DrainStats stats;
  s->ring_diag.clear();
  Event device_done;
  if (want_host && T + 1 > gsv_drain::usable_cores()) (void)device_done.create(hipEventBlockingSync | hipEventDisableTiming);
  // The stream the garbler's windows are launched on: the engine's, or — a garble || evaluate pair with CU-masked streams (ensure_pair) —
  // the pair's masked garbler stream, which first waits for whatever the engine's stream still holds (input staging, the memsets above).
  hipStream_t gs = s->e->stream.get();
  if (ev && s->pair->gstream) {
    gs = s->pair->gstream.get();
    if (hipEventRecord(s->pair->ready.get(), s->e->stream.get()) != hipSuccess || hipStreamWaitEvent(gs, s->pair->ready.get(), 0) != hipSuccess) return fail(GSV_ERR_DEVICE, "stream hand-over failed");
  }
  if (hipEventRecord(s->ev0.get(), gs) != hipSuccess) return fail(GSV_ERR_DEVICE, "hipEventRecord failed");
  DrainPass p{s, ev, gate_id_base, pw0, n_inst, seg_records, want_drain, shape.gate_bufs, workers, commit, stats, gs, device_done.get(), std::chrono::steady_clock::now(), 0.0};
  int rc = GSV_OK;
  for (uint64_t r0 = first; r0 < total && rc == GSV_OK; r0 += seg) rc = s->plan ? drain_plan_window(p, size_t(r0)) : drain_program_ring(p, r0, std::min(total, r0 + seg));
  if (s->ring() && rc != GSV_OK) {
    // a failed pass: calls of the running window may still wait for room in the ring — let them run out (the results are discarded)
    __atomic_store_n(s->ps.ct_pos.get(), ~0ull, __ATOMIC_RELEASE);
    (void)hipStreamSynchronize(gs);
  }
  const auto t_finish = std::chrono::steady_clock::now();
  workers.finish(); commit.join();
  stats.t_wait_drain += drain_secs(t_finish);
  if (ev && hipStreamSynchronize(s->pair->stream.get()) != hipSuccess && rc == GSV_OK) rc = fail(GSV_ERR_DEVICE, "evaluation kernel failed");
  if (s->pass.drain_stats) stats.print(n_inst, T, GROUP, workers.depth());
  if (rc == GSV_OK && s->plan) {
    (void)hipEventRecord(s->ev1.get(), gs);  // (every window on gs has been synchronised: the output gather on the engine's stream follows safely)
    if (c1 == s->plan->calls.size()) {
      rc = gather_plan_outputs(s, false);
      if (rc == GSV_OK && ev) rc = gather_plan_outputs(ev, true);
    } else { s->ran = true; s->last_eval = false; }
  }
  if (rc == GSV_OK && s->plan) rc = check_plan_error(s);
  if (rc == GSV_OK && ev) rc = check_plan_error(ev);
  rc = commit.close(rc, !s->plan || c1 == s->plan->calls.size());
  if (rc != GSV_OK) return rc;
  files.keep();
  s->garbled = true;
  return GSV_OK;
}
// A dependency wait gave up (status 1): the schedule's one assumption — a workgroup only waits for workgroups with a smaller linear index,
// which the hardware dispatches first (include/gsv_engine.h, max_concurrent_calls) — did not hold on this device / driver.  The session
// is switched, in place, to the SAFE schedule: one call per launch, in stream order, no dependency wait on the device at all (the stream
// orders the launches) and no ciphertext ring.  Same plan images, same wire-file and ciphertext allocations (the safe schedule needs
// less of both; re-allocated if not), the host's last inputs re-staged.  Slower (every call ends with a launch boundary), never wrong.
// The safe PlanState is built whole beside the installed one (tables of KBs to MBs: no memory peak) and then swapped in: a failure up
// to there leaves the session exactly as it was, on its old schedule.  A failure while W / VB / CT grow afterwards leaves the session
// without a schedule and with the reason in `unusable`: it refuses to stage inputs or to run from then on (plan_session_usable).
static int fall_back_to_safe_schedule(gsv_session* s) {
  if (int rc = plan_session_usable(s)) return rc;
  if (!s->plan || s->safe()) return fail(GSV_ERR_DEVICE, "internal: no safe schedule to fall back to");
  HIPCHK(hipSetDevice(s->e->device));
  HIPCHK(hipDeviceSynchronize());
  gsv_plan_session_opts o = s->opts;
  o.max_concurrent_calls = 1;
  o.max_window_calls = 1;
  if (o.retain_stream == GSV_STREAM_RING) o.retain_stream = 0;
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, s->e->device));
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  gsv_session::PlanState safe;
  int rc = make_plan_state(s, o, true, prop.multiProcessorCount, free_b, &safe);
  if (rc) return rc;
  s->ps = std::move(safe);  // (the device is idle: the old tables go here)
  s->next_call = 0;
  if ((rc = alloc_session_buffers(s, s->prog()))) {  // (W / VB / CT grow where the safe schedule needs more; VB cleared)
    s->unusable = "the fall-back to the safe schedule failed while the session's buffers were growing (" + g_err + "): the session has no schedule left and cannot run; destroy it";
    s->ps = gsv_session::PlanState();
    s->garbled = s->ran = false;
    return rc;
  }
  ++s->n_fallbacks;
  s->dep_fault = false;
  s->garbled = false;
  std::fill(s->ct_uploaded.begin(), s->ct_uploaded.end(), 0);
  if (s->stash_kind == 1) return set_garble_inputs_impl(s, s->stash_delta.data(), s->stash_consts.data(), s->stash_inputs.data());
  if (s->stash_kind == 2) return set_evaluate_inputs_impl(s, s->stash_consts.data(), s->stash_inputs.data(), s->stash_bits.data());
  return GSV_OK;
}
int gsv_session_fallback_count(const gsv_session* s, uint64_t* n) {
  if (!s || !n) return fail(GSV_ERR_INVALID, "null argument");
  *n = s->n_fallbacks;
  return GSV_OK;
}
// A whole pass whose results the engine alone has seen (discarded, MAC'ed, written to gc files) is repeated on the safe schedule by
// itself; a pass that fed a host callback (ciphertexts or outboard values) or an evaluator session, or a slice of a pass, fails as
// before — the host has consumed a prefix of a stream that is invalid, and a slice's call range follows the old schedule's windows —
// but leaves the session on the safe schedule, so that the host's own repeat of the pass (from gsv_session_set_garble_inputs on) succeeds.
static int garble_streaming_range(gsv_session* s, uint64_t gate_id_base, size_t c0, size_t c1, const DrainSink& sink, int n_threads, gsv_session* ev = nullptr) {
  int rc = garble_streaming_pass(s, gate_id_base, c0, c1, sink, n_threads, ev);
  if (rc != GSV_ERR_DEVICE || !s->plan || !(s->dep_fault || (ev && ev->dep_fault)) || s->safe()) return rc;
  const std::string first_error = g_err;
  const bool whole = c0 == 0 && c1 == s->plan->calls.size();
  int frc = fall_back_to_safe_schedule(s);
  if (frc) return fail(GSV_ERR_DEVICE, first_error + "; the fall-back to the safe schedule failed too: " + g_err);
  if (ev) { frc = fall_back_to_safe_schedule(ev); if (frc) return fail(GSV_ERR_DEVICE, first_error + "; the evaluator's fall-back to the safe schedule failed: " + g_err); }
  if (!whole || sink.fn || sink.ob_fn || ev)
    return fail(GSV_ERR_DEVICE, first_error + "; the session now runs the safe schedule (one call per launch): repeat the pass from gsv_session_set_garble_inputs");
  if (s->pass.drain_debug || s->pass.plan_debug) std::fprintf(stderr, "plan session: %s -- repeating the pass on the safe schedule (one call per launch)\n", first_error.c_str());
  return garble_streaming_pass(s, gate_id_base, 0, s->plan->calls.size(), sink, n_threads, nullptr);
}
static DrainSink mac_file_sink(uint8_t* hashes, const char* dir, uint64_t first_index) { DrainSink k; k.hashes = hashes; k.dir = dir; k.first_index = first_index; return k; }
int gsv_session_garble_streaming(gsv_session* s, uint64_t gate_id_base, const char* dir, uint64_t first_index, int n_threads, uint8_t* hashes) {
  PassGuard pass_guard(s);  // destroys requested while this pass runs wait for its end (deferred release)
  if (!s) return fail(GSV_ERR_INVALID, "null argument");
  if (dir && !hashes) return fail(GSV_ERR_INVALID, "null hash buffer");
  return garble_streaming_range(s, gate_id_base, 0, s->plan ? s->plan->calls.size() : 1, mac_file_sink(hashes, dir, first_index), n_threads);
}
// One slice of a plan session's pass, calls [first_call, first_call + n_calls).  Wires, gate ids and the MAC states continue from slice
// to slice: a slice either starts a new pass or continues where the previous one ended.  `arg_error`: what the entry point found wrong
// with its own arguments (reported behind a bad call range, as ever).
static int garble_slice(gsv_session* s, uint64_t gate_id_base, uint64_t first_call, uint64_t n_calls, const DrainSink& k, int n_threads, const char* arg_error = nullptr) {
  if (!s || !s->plan) return fail(GSV_ERR_INVALID, "null session / not a plan session");
  if (first_call > s->plan->calls.size() || n_calls > s->plan->calls.size() - first_call) return fail(GSV_ERR_INVALID, "call range outside the plan");
  if (first_call != 0 && first_call != s->next_call && !s->unchecked_slices)
    return fail(GSV_ERR_INVALID, "slice starts at call " + std::to_string(first_call) + " but the previous slice ended at call " + std::to_string(s->next_call) +
                                     " (gsv_session_set_unchecked_slices for timing runs)");
  if (arg_error) return fail(GSV_ERR_INVALID, arg_error);
  const int rc = garble_streaming_range(s, gate_id_base, size_t(first_call), size_t(first_call + n_calls), k, n_threads);
  if (rc == GSV_OK) { s->next_call = first_call + n_calls; s->garbled = s->retain() && s->next_call == s->plan->calls.size(); }
  return rc;
}
// What the entry points that take a call range end in: a program session is garbled in one pass, (0, 0) on a plan session is the whole
// plan.  `any_program_range`: gsv_session_garble_streaming_sink has always ignored a call range on a program session; it still does.
static int garble_call_range(gsv_session* s, uint64_t gate_id_base, uint64_t first_call, uint64_t n_calls, const DrainSink& k, int n_threads, bool any_program_range = false) {
  if (!s->plan) {
    if (!any_program_range && (first_call || n_calls)) return fail(GSV_ERR_INVALID, "program sessions are garbled in one pass (first_call = n_calls = 0)");
    return garble_streaming_range(s, gate_id_base, 0, 1, k, n_threads);
  }
  if (first_call == 0 && n_calls == 0) n_calls = s->plan->calls.size();
  return garble_slice(s, gate_id_base, first_call, n_calls, k, n_threads);
}
int gsv_session_garble_streaming_calls(gsv_session* s, uint64_t gate_id_base, uint64_t first_call, uint64_t n_calls, const char* dir, uint64_t first_index, int n_threads, uint8_t* hashes) {
  PassGuard pass_guard(s);  // destroys requested while this pass runs wait for its end (deferred release)
  return garble_slice(s, gate_id_base, first_call, n_calls, mac_file_sink(hashes, dir, first_index), n_threads, dir && !hashes ? "null hash buffer" : nullptr);
}
// Either commitment or both (include/gsv_engine.h, "BLAKE3 commitments"): the CBC-MAC on the host's cores, BLAKE3 where the ciphertexts are.
int gsv_session_garble_streaming_commit(gsv_session* s, uint64_t gate_id_base, uint64_t first_call, uint64_t n_calls, const char* dir, uint64_t first_index, int n_threads,
                                        uint8_t* cbcmac_hashes, uint8_t* blake3_digests) {
  return gsv_session_garble_streaming_commit_outboard(s, gate_id_base, first_call, n_calls, dir, first_index, n_threads, cbcmac_hashes, blake3_digests, nullptr);
}
// ... and with the values the absorbers receive kept as gc_<index>.b3o (include/gsv_engine.h, "BLAKE3 outboards")
int gsv_session_garble_streaming_commit_outboard(gsv_session* s, uint64_t gate_id_base, uint64_t first_call, uint64_t n_calls, const char* dir, uint64_t first_index, int n_threads,
                                                 uint8_t* cbcmac_hashes, uint8_t* blake3_digests, const char* outboard_dir) {
  PassGuard pass_guard(s);  // destroys requested while this pass runs wait for its end (deferred release)
  if (!s) return fail(GSV_ERR_INVALID, "null argument");
  DrainSink k = mac_file_sink(cbcmac_hashes, dir, first_index);
  k.b3 = blake3_digests;
  k.outboard_dir = outboard_dir;
  if (const char* why = k.b3_refusal()) return fail(GSV_ERR_INVALID, why);
  return garble_call_range(s, gate_id_base, first_call, n_calls, k, n_threads);
}
// gsv_session_garble_streaming_calls that also writes <checkpoint_dir>/gc_<first_index + i>.mck (include/gsv_engine.h, "CBC-MAC checkpoints"):
// the chain states the MAC workers pass through anyway, k = GSV_MAC_GROUP_LOG2 of the pass
int gsv_session_garble_streaming_checkpoints(gsv_session* s, uint64_t gate_id_base, uint64_t first_call, uint64_t n_calls, const char* dir, uint64_t first_index, int n_threads,
                                             uint8_t* hashes, const char* checkpoint_dir) {
  PassGuard pass_guard(s);  // destroys requested while this pass runs wait for its end (deferred release)
  if (!s) return fail(GSV_ERR_INVALID, "null argument");
  if ((dir || checkpoint_dir) && !hashes) return fail(GSV_ERR_INVALID, "null hash buffer");
  DrainSink k = mac_file_sink(hashes, dir, first_index);
  k.checkpoint_dir = checkpoint_dir;
  return garble_call_range(s, gate_id_base, first_call, n_calls, k, n_threads);
}
// Garbles and verifies against checkpoint files where the ciphertexts are: nothing is drained, no MAC worker starts
int gsv_session_garble_streaming_check(gsv_session* s, uint64_t gate_id_base, uint64_t first_call, uint64_t n_calls, const char* checkpoint_dir, const uint64_t* indexes, uint64_t first_index,
                                       const uint8_t* expected, uint8_t* hashes) {
  PassGuard pass_guard(s);  // destroys requested while this pass runs wait for its end (deferred release)
  if (!s || !checkpoint_dir) return fail(GSV_ERR_INVALID, "null argument");
  DrainSink k;
  k.first_index = first_index;
  k.mac_check_dir = checkpoint_dir; k.mac_check_indexes = indexes; k.mac_check_expected = expected; k.mac_check_hashes = hashes;
  return garble_call_range(s, gate_id_base, first_call, n_calls, k, 0);
}
// The generic CiphertextHandler: every drained run of records is handed to `sink` (gate order, per instance in stream order).
int gsv_session_garble_streaming_sink(gsv_session* s, uint64_t gate_id_base, uint64_t first_call, uint64_t n_calls, gsv_ct_sink_fn sink, void* user, int n_threads, uint8_t* hashes) {
  PassGuard pass_guard(s);  // destroys requested while this pass runs wait for its end (deferred release)
  if (!s || !sink) return fail(GSV_ERR_INVALID, "null argument");
  DrainSink k;
  k.hashes = hashes; k.fn = sink; k.user = user;
  return garble_call_range(s, gate_id_base, first_call, n_calls, k, n_threads, /*any_program_range=*/true);
}
// ... with either commitment or both, the outboards handed to a second callback and the last chunks returned (include/gsv_engine.h,
// "Commitments on the callback paths"): gsv_session_garble_streaming_commit_outboard with the handler in place of `dir`, the callback in place of `outboard_dir`.
int gsv_session_garble_streaming_sink_commit(gsv_session* s, uint64_t gate_id_base, uint64_t first_call, uint64_t n_calls, gsv_ct_sink_fn sink, void* user, int n_threads,
                                             uint8_t* cbcmac_hashes, uint8_t* blake3_digests, gsv_outboard_sink_fn outboard_sink, void* outboard_user, uint8_t* last_chunks) {
  PassGuard pass_guard(s);  // destroys requested while this pass runs wait for its end (deferred release)
  if (!s) return fail(GSV_ERR_INVALID, "null argument");
  DrainSink k;
  k.hashes = cbcmac_hashes; k.fn = sink; k.user = user;
  k.b3 = blake3_digests; k.ob_fn = outboard_sink; k.ob_user = outboard_user; k.last_chunks = last_chunks;
  if (const char* why = k.b3_refusal()) return fail(GSV_ERR_INVALID, why);
  return garble_call_range(s, gate_id_base, first_call, n_calls, k, n_threads);
}
// Garble and evaluate side by side on the device (examples/groth16_garble.rs:171-230: the garbler thread feeds the evaluator thread
// through a channel; here window k of the garbler's device block is evaluated while window k+1 is garbled).
int gsv_session_garble_evaluate(gsv_session* gs, gsv_session* es, uint64_t gate_id_base, int n_threads, uint8_t* hashes) {
  PassGuard pass_guard(gs);  // destroys requested while this pass runs wait for its end (deferred release)
  if (!gs || !es || gs == es) return fail(GSV_ERR_INVALID, "null / identical sessions");
  es->pass = gs->pass;
  if (!gs->plan || gs->plan != es->plan || gs->e != es->e || gs->n_inst != es->n_inst || gs->ni != es->ni || gs->hasher != es->hasher)
    return fail(GSV_ERR_INVALID, "garbler and evaluator must be plan sessions of the same plan, engine, instance count and hasher");
  if (gs->retain() || es->retain()) return fail(GSV_ERR_INVALID, "gsv_session_garble_evaluate is for sessions that do not retain the stream (retain_stream = 0)");
  const auto &wa = gs->sched().windows, &wb = es->sched().windows;
  if (wa.size() != wb.size() || gs->max_block() != es->max_block()) return fail(GSV_ERR_INVALID, "garbler and evaluator sessions have different schedules (create both with the same options)");
  for (size_t i = 0; i < wa.size(); ++i) if (wa[i].call0 != wb[i].call0 || wa[i].call1 != wb[i].call1) return fail(GSV_ERR_INVALID, "garbler and evaluator sessions have different schedules (create both with the same options)");
  DrainSink k;
  k.hashes = hashes;
  int rc = garble_streaming_range(gs, gate_id_base, 0, gs->plan->calls.size(), k, n_threads, es);
  if (rc == GSV_OK) { gs->next_call = gs->plan->calls.size(); gs->garbled = false; }
  return rc;
}
