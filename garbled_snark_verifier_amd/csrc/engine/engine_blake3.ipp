// Part of engine.cpp: BLAKE3 commitments — the host hasher behind gsv_blake3_*, and the device tree hash of n equally long streams
// that arrive in segments of a gate-order buffer (blake3_device.hpp: B3Stream, b3_begin / b3_segment / b3_absorb / b3_finish).  The
// streaming drain (engine_drain.ipp) absorbs the values on threads of its own; everyone else — the streaming evaluators
// (engine_evaluate.ipp), gsv_session_ciphertext_blake3 (engine_readback.ipp: it feeds ranges of the resident program-order stream),
// gsv_engine_blake3_streams and gsv_engine_blake3_files — goes through one B3Receiver, which also compares what the streams hash to
// with their outboards (outboard.hpp: the values the host absorbs, kept by the drain; B3Check) and with the commitments.
//
// Split (DESIGN.md §3 "Commitment stage"): a stream of L records has N = max(1, ceil(L / 64)) chunks.  The device hashes chunks
// 0 .. N-2 and reduces aligned groups of G = 2^k of them to one value each; the host absorbs floor((N-1) / G) group values, then the
// (N-1) mod G chunk values behind them, then hashes the last chunk (the carry: at most 64 records) and folds the stack.
struct B3Stream {
  size_t n_inst = 0;
  uint32_t k = 10;                 // log2 of the group size (GSV_B3_SUBTREE_LOG2)
  uint64_t total = 0;              // records per stream
  uint64_t dev_chunks = 0;         // N - 1
  uint64_t seg_cap = 0;            // most records per instance a segment may hold
  uint64_t cv_stride = 0, red_cap = 0;  // 32-byte values per instance: chunk values of a segment behind the pending ones; group values of a segment
  DevBuf carry[2], cv[2], red;     // ping-pong: a launch reads carry[cpar] / cv[vpar] and leaves what stays behind in the other one
  MappedHost<uint8_t> pinned;      // group values of the segment in flight; at the end the pending chunk values, then the carries
  int cpar = 0, vpar = 0;
  uint32_t carry_n = 0, pend = 0;  // records in carry[cpar], chunk values in cv[vpar], per instance
  uint64_t chunks_done = 0, records_done = 0;
  std::vector<Blake3Host> hashers;
};
static int check_b3_k(uint32_t k) { return k > 20 ? fail(GSV_ERR_INVALID, "GSV_B3_SUBTREE_LOG2 must be an integer in [0, 20]") : GSV_OK; }
// a new stream set: buffers are kept when the shape is the one they were allocated for
static int b3_begin(std::unique_ptr<B3Stream>& p, size_t n_inst, uint64_t total, uint64_t seg_cap, uint32_t k) {
  if (n_inst == 0 || n_inst > 65535) return fail(GSV_ERR_INVALID, "BLAKE3 commitments take 1 .. 65535 streams at a time");
  if (int rc = check_b3_k(k)) return rc;
  const uint64_t cv_stride = ((1ull << k) - 1) + (seg_cap + 64) / 64 + 1, red_cap = (cv_stride >> k) + 1;
  if (cv_stride >= (1ull << 32)) return fail(GSV_ERR_INVALID, "segment too long for the BLAKE3 value buffers");
  if (!p || p->n_inst != n_inst || p->k != k || p->cv_stride != cv_stride) {
    p.reset(new B3Stream());
    bool ok = true;
    for (int i = 0; i < 2; ++i) ok = ok && p->carry[i].alloc(n_inst * 1024) == hipSuccess && p->cv[i].alloc(n_inst * size_t(cv_stride) * 32) == hipSuccess;
    ok = ok && p->red.alloc(n_inst * size_t(red_cap) * 32) == hipSuccess;
    ok = ok && p->pinned.alloc(n_inst * size_t(std::max<uint64_t>(std::max<uint64_t>(red_cap, 1ull << k) * 32, 1024)), hipHostMallocDefault) == hipSuccess;
    if (!ok) { p.reset(); return fail(GSV_ERR_DEVICE, "cannot allocate the BLAKE3 commitment buffers"); }
  }
  B3Stream& b = *p;
  b.n_inst = n_inst; b.k = k; b.total = total; b.seg_cap = seg_cap; b.cv_stride = cv_stride; b.red_cap = red_cap;
  b.dev_chunks = std::max<uint64_t>(1, (total + 63) / 64) - 1;
  b.cpar = b.vpar = 0; b.carry_n = b.pend = 0; b.chunks_done = b.records_done = 0;
  b.hashers.assign(n_inst, Blake3Host());
  return GSV_OK;
}
// The next n records of every stream: buf[inst * stride + r], r < n.  Launches on st; when st has been synchronised *n_groups group values
// per instance sit in b.pinned ([inst][group], dense) and buf is free again.
// ... or, with `ix`, records [ix->first, ix->first + n) of the gate-order stream of a block that lies in program order (a resident
// ring, a plan call's block): block[inst * stride + (q / n_ct) * n_ct + ct_pos[q % n_ct]].  The block is only read.
struct B3Indexed { const void* ct_pos; uint64_t n_ct, first; };
static int b3_segment(B3Stream& b, const void* buf, uint64_t stride, uint64_t n, hipStream_t st, uint32_t* n_groups, const B3Indexed* ix = nullptr) {
  *n_groups = 0;
  if (n > b.seg_cap || b.records_done + n > b.total) return fail(GSV_ERR_INVALID, "internal: BLAKE3 segment outside the stream");
  if (n == 0) return GSV_OK;
  const uint64_t avail = b.carry_n + n;
  const uint32_t n_chunks = uint32_t(std::min<uint64_t>(avail / 64, b.dev_chunks - b.chunks_done));
  const uint64_t tail = avail - 64ull * n_chunks;
  if (tail > 64 || uint64_t(b.pend) + n_chunks > b.cv_stride) return fail(GSV_ERR_INVALID, "internal: BLAKE3 carry / value buffer overflow");
  const int krc = ix ? gsvk_b3_chunks_indexed(buf, stride, ix->ct_pos, ix->n_ct, ix->first, b.carry[b.cpar].get(), b.carry_n, b.carry[b.cpar ^ 1].get(), uint32_t(tail), b.chunks_done, n_chunks, b.cv[b.vpar].get(), b.cv_stride, b.pend, uint32_t(b.n_inst), st)
                     : gsvk_b3_chunks(buf, stride, b.carry[b.cpar].get(), b.carry_n, b.carry[b.cpar ^ 1].get(), uint32_t(tail), b.chunks_done, n_chunks, b.cv[b.vpar].get(), b.cv_stride, b.pend, uint32_t(b.n_inst), st);
  if (krc != 0) return fail(GSV_ERR_DEVICE, "BLAKE3 chunk kernel launch failed");
  b.cpar ^= 1; b.carry_n = uint32_t(tail); b.chunks_done += n_chunks; b.records_done += n;
  if (n_chunks) {
    const uint32_t n_have = b.pend + n_chunks, groups = n_have >> b.k;
    if (groups > b.red_cap) return fail(GSV_ERR_INVALID, "internal: BLAKE3 group buffer overflow");
    if (gsvk_b3_reduce(b.cv[b.vpar].get(), b.cv_stride, n_have, b.k, b.red.get(), b.cv[b.vpar ^ 1].get(), uint32_t(b.n_inst), st) != 0) return fail(GSV_ERR_DEVICE, "BLAKE3 reduce kernel launch failed");
    b.vpar ^= 1; b.pend = n_have - (groups << b.k);
    if (groups) HIPCHK(hipMemcpyAsync(b.pinned.get(), b.red.get(), b.n_inst * size_t(groups) * 32, hipMemcpyDeviceToHost, st));
    *n_groups = groups;
  }
  return GSV_OK;
}
// group values ([inst][group], dense, for all instances) into the hashers of instances i0, i0 + step, ...
static bool b3_absorb(B3Stream& b, const uint8_t* vals, uint32_t groups, unsigned k, size_t i0, size_t step) {
  bool ok = true;
  for (size_t i = i0; i < b.n_inst; i += step)
    for (uint32_t g = 0; g < groups; ++g) ok = b.hashers[i].absorb_subtree(vals + (i * groups + g) * 32, k) && ok;
  return ok;
}

// every record has been fed and every group value absorbed: the pending chunk values and the last chunks come to the host.
// `pending` (optional) sees the pending chunk values ([instance][value], dense) before they are absorbed and before anything is
// written to `digests`; a non-zero return ends the call with it.  `last_chunks` (optional, n_inst x 1024) receives the last chunks
// themselves — the carries the host hashes — each padded with zeros.
static int b3_finish(B3Stream& b, hipStream_t st, uint8_t* digests, const std::function<int(const uint8_t* vals, uint32_t pend)>& pending = nullptr, uint8_t* last_chunks = nullptr) {
  if (b.records_done != b.total) return fail(GSV_ERR_INVALID, "internal: BLAKE3 stream ended early");
  // the folding (up to 2^k - 1 parents, the last chunk and the stack per instance) runs on a few threads, not on the caller's
  const size_t T = std::min<size_t>(4, b.n_inst);
  auto on_pool = [&](auto&& per_instance) {
    std::atomic<bool> ok{true};
    std::vector<std::thread> pool;
    for (size_t t = 0; t < T; ++t) pool.emplace_back([&, t] { for (size_t i = t; i < b.n_inst; i += T) if (!per_instance(i)) ok = false; });
    for (auto& th : pool) th.join();
    return ok.load();
  };
  if (b.pend) {
    HIPCHK(hipMemcpy2DAsync(b.pinned.get(), size_t(b.pend) * 32, b.cv[b.vpar].get(), size_t(b.cv_stride) * 32, size_t(b.pend) * 32, b.n_inst, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (pending) { const int prc = pending(b.pinned.get(), b.pend); if (prc) return prc; }
    const bool ok = on_pool([&](size_t i) { bool r = true; for (uint32_t g = 0; g < b.pend; ++g) r = b.hashers[i].absorb_subtree(b.pinned.get() + (i * b.pend + g) * 32, 0) && r; return r; });
    if (!ok) return fail(GSV_ERR_INVALID, "internal: BLAKE3 chunk values out of order");
  } else if (pending) { const int prc = pending(nullptr, 0); if (prc) return prc; }
  if (b.carry_n) {
    HIPCHK(hipMemcpyAsync(b.pinned.get(), b.carry[b.cpar].get(), b.n_inst * 1024, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  if (!on_pool([&](size_t i) { b.hashers[i].update(b.pinned.get() + i * 1024, uint64_t(b.carry_n) * 16); return b.hashers[i].finalize(digests + 32 * i); }))
    return fail(GSV_ERR_INVALID, "internal: BLAKE3 stream without a last chunk");
  if (last_chunks) {
    const size_t have = size_t(b.carry_n) * 16;
    std::memset(last_chunks, 0, b.n_inst * 1024);
    for (size_t i = 0; i < b.n_inst && have; ++i) std::memcpy(last_chunks + i * 1024, b.pinned.get() + i * 1024, have);
  }
  return GSV_OK;
}
// The single-threaded consumer of a B3Stream, for whoever receives streams and hashes them on one thread: the streaming evaluators, the
// two commitments to streams that lie in device memory and gsv_engine_blake3_files (the drain absorbs on threads of its own:
// B3Absorbers).  The group values of a segment sit in the page-locked buffer once `ev` — recorded behind the segment's hash kernels —
// has passed; they are looked at when the next segment is fed, or at flush().  With a `check` (verified mode) every value is compared
// with the outboard of its instance before it is absorbed, and a difference ends the pass with GSV_ERR_MISMATCH: `check` holds the place.
struct B3Receiver {
  std::unique_ptr<B3Stream>& slot;  // the caller's: a session keeps its buffers from pass to pass
  const char* noun;                 // what a mismatch calls a stream: "file", "the ciphertext stream of instance"
  B3Check* check;                   // the streams' outboards, or null
  Event ev;
  uint32_t groups = 0;              // group values per instance in flight
  bool on = false;                  // begin() has succeeded: feed() hashes (else it does nothing)
  bool at_end = false;              // finish() ended with a digest that differs from its commitment: a mismatch without a group of its own
  explicit B3Receiver(std::unique_ptr<B3Stream>& slot_, const char* noun_ = "stream", B3Check* check_ = nullptr) : slot(slot_), noun(noun_), check(check_) {}
  int begin(size_t n_inst, uint64_t total, uint64_t seg_cap, uint32_t k) {
    if (int rc = b3_begin(slot, n_inst, total, seg_cap, k)) return rc;
    HIPCHK(ev.create(hipEventDisableTiming));
    if (check) check->reset();
    groups = 0; on = true;
    return GSV_OK;
  }
  // ... or goes on with streams an earlier receiver began (a later slice of a sliced evaluation): nothing is reset, no value is in
  // flight — every slice ends with a flush() — and the comparison stands where it stood
  int resume(size_t n_inst, uint64_t total, uint64_t seg_cap, uint32_t k) {
    if (!slot || slot->n_inst != n_inst || slot->total != total || slot->k != k)
      return fail(GSV_ERR_INVALID, "this slice continues a pass whose earlier slices computed no BLAKE3 commitment of this shape (instances, GSV_B3_SUBTREE_LOG2)");
    // The value buffers were sized for the largest segment of the schedule the pass began on.  A schedule installed in the middle of a
    // pass is the safe one (fall_back_to_safe_schedule): its windows, and so its segments, are single calls, and a segment of any
    // schedule holds at least one whole call — its largest segment cannot be larger.  Should that ever change, say so:
    if (slot->seg_cap < seg_cap)
      return fail(GSV_ERR_INVALID, "internal: the schedule's largest segment grew in the middle of a pass (" + std::to_string(slot->seg_cap) + " -> " + std::to_string(seg_cap) + " records): the BLAKE3 value buffers of the pass cannot hold it");
    HIPCHK(ev.create(hipEventDisableTiming));
    groups = 0; on = true;
    return GSV_OK;
  }
  int mismatch() const { return fail(GSV_ERR_MISMATCH, check->where(noun)); }
  // the values in flight: waited for, compared, absorbed
  int flush() {
    if (!groups) return GSV_OK;
    if (hipEventSynchronize(ev.get()) != hipSuccess) return fail(GSV_ERR_DEVICE, "event wait failed");
    const uint32_t g = groups;
    groups = 0;
    if (check && !check->groups_match(slot->pinned.get(), g)) return mismatch();
    return b3_absorb(*slot, slot->pinned.get(), g, slot->k, 0, 1) ? GSV_OK : fail(GSV_ERR_INVALID, "internal: BLAKE3 group values out of order");
  }
  // the next n records of every stream (b3_segment), enqueued on st behind a flush(): the page-locked buffer is free for their values
  int feed(const void* buf, uint64_t stride, uint64_t n, hipStream_t st, const B3Indexed* ix = nullptr) {
    if (!on) return GSV_OK;
    int rc = flush();
    if (rc == GSV_OK) rc = b3_segment(*slot, buf, stride, n, st, &groups, ix);
    if (rc == GSV_OK && groups && hipEventRecord(ev.get(), st) != hipSuccess) rc = fail(GSV_ERR_DEVICE, "event record failed");
    return rc;
  }
  // The end of the streams: the chunk values behind the last complete group against the outboards, then — with `expected`, n_inst x
  // expected_len bytes, which needs a `check` — the computed digests against the commitments: a difference there has no group of its
  // own and is blamed on the last chunk.  `digests` (n_inst x 32) is written only when everything succeeded.
  int finish(hipStream_t st, uint8_t* digests, const uint8_t* expected = nullptr, uint64_t expected_len = 0) {
    int rc = flush();
    if (rc) return rc;
    std::vector<uint8_t> got(slot->n_inst * 32);
    rc = b3_finish(*slot, st, got.data(), check ? std::function<int(const uint8_t*, uint32_t)>([this](const uint8_t* vals, uint32_t pend) { return check->pending_match(vals, pend) ? GSV_OK : mismatch(); }) : nullptr);
    for (size_t i = 0; expected && i < slot->n_inst && rc == GSV_OK; ++i)
      if (std::memcmp(got.data() + 32 * i, expected + expected_len * i, size_t(expected_len)) != 0) {
        check->bad_instance = i; check->bad_group = check->n_groups; check->bad_record = (Outboard::chunks(check->n_records) - 1) * 64;
        at_end = true;
        rc = mismatch();
      }
    if (rc == GSV_OK) std::memcpy(digests, got.data(), got.size());
    return rc;
  }
};

// ---- what a sliced streaming evaluation carries from slice to slice (engine_evaluate.ipp; include/gsv_engine.h "Sliced evaluation") ----
// A restart point: the session as it stood when a restartable slice began, before anything of the slice was uploaded.  The wire files
// (labels and plaintext bits) and the device half of the evaluator's B3Stream are stream-ordered device-to-device copies into buffers
// allocated at the first restartable slice; the host half is plain values.
struct EvalRestart {
  bool held = false;
  uint64_t call = 0, record = 0;                  // the slice's first call, and its first record
  DevBuf W, VB, carry[2], cv[2];
  uint32_t n_slots = 0, global_base = 0;          // the wire-file layout W / VB were copied in (the safe schedule lays it out anew)
  bool b3 = false;                                // the B3 half below was taken (the pass computes BLAKE3 commitments)
  int cpar = 0, vpar = 0;
  uint32_t carry_n = 0, pend = 0;
  uint64_t chunks_done = 0, records_done = 0;
  std::vector<Blake3Host> hashers;
  std::vector<CbcMacHost> macs;
  uint64_t check_position = 0, windows_launched = 0;
  bool mac = false;                               // the CBC-MAC check's half below was taken (the pass verifies against checkpoints; engine_cbcmac.ipp, mac_save)
  DevBuf mac_carry[2];                            // the per-instance carries, 16 bytes each; the failing-group words are all ones at a restart point
  MacCheckPosition mac_position;                  // ... and the host half (mac_checkpoints.hpp)
};
struct EvalCarry {
  uint64_t next_call = 0;            // the call the next slice must start with (garbling has a counter of its own: gsv_session::next_call)
  EvalCommit commit = EvalCommit::None;  // what the pass in progress asked for
  std::vector<CbcMacHost> macs;      // the per-instance MAC states after the last slice
  B3Check check;                     // verified passes: the parsed outboards (the slice at call 0 loaded them) and the comparison's position
  EvalRestart rp[2];                 // [0]: where the last restartable slice began, [1]: the restartable slice before it
  bool resumable = false;            // the last slice failed and the session was rolled back: to `resume_call` / `resume_record`
  uint64_t resume_call = 0, resume_record = 0;
};
static int ensure_dev(DevBuf& d, size_t bytes, const char* what) {
  if (d && d.bytes() >= bytes) return GSV_OK;
  return dev_alloc(d, bytes, what);
}
// the device half of a B3Stream and its counts <-> a restart point, through st
static int b3_save(const B3Stream& b, EvalRestart& r, hipStream_t st) {
  for (int i = 0; i < 2; ++i) {
    if (int rc = ensure_dev(r.carry[i], b.carry[i].bytes(), "a restart point's BLAKE3 carries")) return rc;
    if (int rc = ensure_dev(r.cv[i], b.cv[i].bytes(), "a restart point's BLAKE3 values")) return rc;
    HIPCHK(hipMemcpyAsync(r.carry[i].get(), b.carry[i].get(), b.carry[i].bytes(), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(r.cv[i].get(), b.cv[i].get(), b.cv[i].bytes(), hipMemcpyDeviceToDevice, st));
  }
  r.cpar = b.cpar; r.vpar = b.vpar; r.carry_n = b.carry_n; r.pend = b.pend; r.chunks_done = b.chunks_done; r.records_done = b.records_done;
  r.hashers = b.hashers;
  r.b3 = true;
  return GSV_OK;
}
static int b3_restore(B3Stream& b, const EvalRestart& r, hipStream_t st) {
  for (int i = 0; i < 2; ++i) {
    if (r.carry[i].bytes() < b.carry[i].bytes() || r.cv[i].bytes() < b.cv[i].bytes()) return fail(GSV_ERR_INVALID, "internal: a restart point of another BLAKE3 stream shape");
    HIPCHK(hipMemcpyAsync(b.carry[i].get(), r.carry[i].get(), b.carry[i].bytes(), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(b.cv[i].get(), r.cv[i].get(), b.cv[i].bytes(), hipMemcpyDeviceToDevice, st));
  }
  b.cpar = r.cpar; b.vpar = r.vpar; b.carry_n = r.carry_n; b.pend = r.pend; b.chunks_done = r.chunks_done; b.records_done = r.records_done;
  b.hashers = r.hashers;
  return GSV_OK;
}

struct gsv_blake3 { Blake3Host h; };
int gsv_blake3_create(gsv_blake3** out) {
  if (!out) return fail(GSV_ERR_INVALID, "null argument");
  *out = new gsv_blake3();
  return GSV_OK;
}
void gsv_blake3_destroy(gsv_blake3* h) { delete h; }
int gsv_blake3_update(gsv_blake3* h, const uint8_t* data, uint64_t n_bytes) {
  if (!h || (!data && n_bytes)) return fail(GSV_ERR_INVALID, "null argument");
  h->h.update(data, n_bytes);
  return GSV_OK;
}
int gsv_blake3_absorb_subtree(gsv_blake3* h, const uint8_t* chaining_value, uint32_t log2_chunks) {
  if (!h || !chaining_value) return fail(GSV_ERR_INVALID, "null argument");
  if (!h->h.absorb_subtree(chaining_value, log2_chunks)) return fail(GSV_ERR_INVALID, "a subtree of 2^k chunks can only be absorbed between chunks, at a chunk count that is a multiple of 2^k");
  return GSV_OK;
}
int gsv_blake3_finalize(const gsv_blake3* h, uint8_t* out) {
  if (!h || !out) return fail(GSV_ERR_INVALID, "null argument");
  if (!h->h.finalize(out)) return fail(GSV_ERR_INVALID, "the input ends with an absorbed subtree: the last chunk must be given as bytes");
  return GSV_OK;
}
int gsv_blake3_file(const char* path, uint8_t* out) {
  if (!path || !out) return fail(GSV_ERR_INVALID, "null argument");
  FILE* f = std::fopen(path, "rb");
  if (!f) return fail(GSV_ERR_INVALID, std::string("cannot open ") + path);
  Blake3Host h;
  std::vector<uint8_t> buf(1 << 20);
  size_t n;
  while ((n = std::fread(buf.data(), 1, buf.size(), f)) > 0) h.update(buf.data(), n);
  const bool bad = std::ferror(f) != 0;
  std::fclose(f);
  if (bad) return fail(GSV_ERR_INVALID, std::string("read error on ") + path);
  h.finalize(out);
  return GSV_OK;
}
// ---- outboards (include/gsv_engine.h "BLAKE3 outboards", outboard.hpp) ----
int gsv_blake3_outboard_root(const uint8_t* outboard, uint64_t n_bytes, const uint8_t* last_chunk, uint64_t last_chunk_bytes, uint8_t* out) {
  if (!outboard || !out || (!last_chunk && last_chunk_bytes)) return fail(GSV_ERR_INVALID, "null argument");
  if (last_chunk_bytes > 1024 || (last_chunk_bytes & 15)) return fail(GSV_ERR_INVALID, "the last chunk holds 16 .. 1024 bytes in whole records (0 only for the empty stream)");
  Outboard o;
  std::string why;
  if (!Outboard::parse(outboard, n_bytes, &o, &why) || !o.root(last_chunk, last_chunk_bytes, out, &why)) return fail(GSV_ERR_INVALID, why);
  return GSV_OK;
}
int gsv_blake3_outboard_size(uint64_t n_records, uint32_t k, uint64_t* outboard_bytes, uint64_t* last_chunk_bytes) {
  if (k > Outboard::MAX_K) return fail(GSV_ERR_INVALID, "the group size must be 2^k chunks with k in [0, 20]");
  if (n_records > Outboard::MAX_RECORDS) return fail(GSV_ERR_INVALID, "n_records " + std::to_string(n_records) + " is out of range");
  if (outboard_bytes) *outboard_bytes = Outboard::file_bytes(n_records, k);
  if (last_chunk_bytes) *last_chunk_bytes = Outboard::last_chunk_bytes(n_records);
  return GSV_OK;
}
int gsv_blake3_file_outboard(const char* path, uint32_t k, const char* outboard_path, uint8_t* out) {
  if (!path || !out) return fail(GSV_ERR_INVALID, "null argument");
  std::vector<uint8_t> ob, last;
  std::string why;
  if (!outboard_of_file(path, k, &ob, &last, &why)) return fail(GSV_ERR_INVALID, why);
  Outboard o;
  if (!Outboard::parse(ob.data(), ob.size(), &o, &why) || !o.root(last.data(), last.size(), out, &why)) return fail(GSV_ERR_INVALID, why);
  if (outboard_path) {
    FILE* f = std::fopen(outboard_path, "wb");
    if (!f) return fail(GSV_ERR_INVALID, std::string("cannot create ") + outboard_path);
    const bool ok = std::fwrite(ob.data(), 1, ob.size(), f) == ob.size();
    if (std::fclose(f) != 0 || !ok) { std::remove(outboard_path); return fail(GSV_ERR_INVALID, std::string("short write to ") + outboard_path); }
  }
  return GSV_OK;
}
// ---- n equally long streams brought to the device: received files, and streams in memory (here and in engine_cbcmac.ipp) ----
// Received files where the kernels are: n equally long files are read in segments through two page-locked staging buffers (CtUploader
// without MAC workers: the read of a piece overlaps the upload of the one before) and uploaded to a gate-order buffer of one segment,
// which is handed to `feed` as n streams — the whole input is never resident.
static void report_bad(uint64_t* stream_out, uint64_t* group_out, uint64_t stream, uint64_t group) { if (stream_out) *stream_out = stream; if (group_out) *group_out = group; }  // where a mismatch sits
using SegmentFeed = std::function<int(const void* buf, uint64_t stride, uint64_t n_records, hipStream_t st)>;  // buf[stream * stride + r], r < n_records
struct FilesOnDevice {
  GcFileSource files; const char* const* paths = nullptr; size_t n = 0;
  uint64_t total = 0, seg = 0;  // records per file; per file and segment
  // records(i, file, why) -> the record count of paths[i], or false with the caller's own message; `also` (optional): a second list
  // of paths that must not hold a null either.  seg_knob: GSV_DRAIN_SEGMENT_RECORDS, else 16 MiB per file within 256 MiB for all of them.
  int open(const char* const* paths_, const char* const* also, size_t n_files, uint64_t seg_knob, const std::function<bool(size_t, FILE*, uint64_t*, std::string*)>& records) {
    paths = paths_; n = n_files;
    std::string why;
    for (size_t i = 0; i < n; ++i) {
      if (!paths[i] || (also && !also[i])) return fail(GSV_ERR_INVALID, "null path");
      if (!files.add(paths[i], &why)) return fail(GSV_ERR_INVALID, why);
      uint64_t r = 0;
      if (!records(i, files.file(i), &r, &why)) return fail(GSV_ERR_INVALID, why);
      if (i == 0) total = r;
      else if (r != total) return fail(GSV_ERR_INVALID, "the files must be equally long: " + std::string(paths[0]) + " holds " + std::to_string(total) + " records, " + paths[i] + " " + std::to_string(r));
    }
    seg = std::max<uint64_t>(1, std::min<uint64_t>(total, seg_knob ? seg_knob : std::max<uint64_t>(4096, std::min<uint64_t>(1ull << 20, (1ull << 24) / n))));
    return GSV_OK;
  }
  // begin() -> status, once the device is selected and the buffers stand; then feed -> status per segment.  Whatever the outcome, the
  // stream is synchronised before the buffers are released: the caller finishes behind it.
  int run(gsv_engine* e, const char* what, const std::function<int()>& begin, const SegmentFeed& feed) {
    HIPCHK(hipSetDevice(e->device));
    const hipStream_t st = e->stream.get();
    DevBuf gate;
    DEVALLOC(gate, n * size_t(seg) * 16, what);
    CtUploader up(n, seg, std::min<uint64_t>(seg, CT_STAGE_RECORDS), 0, [&](size_t i, uint64_t first, uint8_t* dst, uint64_t m) { return files.read(i, first, dst, m); });
    if (up.alloc() != hipSuccess) return fail(GSV_ERR_DEVICE, "cannot allocate the staging buffers");
    int rc = begin();
    for (uint64_t off = 0; off < total && rc == GSV_OK; off += seg) {
      const uint64_t m = std::min(seg, total - off);
      switch (up.upload(off, m, gate.get(), st)) {
        case UploadError::None: break;
        case UploadError::Dry: rc = fail(GSV_ERR_INVALID, std::string("read error on ") + paths[up.dry_instance()]); break;
        default: rc = fail(GSV_ERR_DEVICE, "upload of a file segment failed");
      }
      if (rc == GSV_OK) rc = feed(gate.get(), seg, m, st);  // (a receiver looks at what the segment before left behind)
    }
    (void)hipStreamSynchronize(st);  // (nothing of `gate` or the staging buffers is in flight when they are released)
    return rc;
  }
};
// The kernels alone: n_streams streams of records_per_stream records each (data: [stream][record]) are uploaded and fed in the given
// segmentation, between two timing events on the engine's stream; what the time covers is the caller's business (stop()).
struct StreamsOnDevice {
  DevBuf d; Event t0, t1; hipStream_t st = nullptr;
  static int segments(const uint64_t* segment_records, uint64_t n_segments, uint64_t records_per_stream, uint64_t* seg_cap) {  // the largest one; they must add up
    uint64_t sum = 0;
    for (uint64_t i = 0; i < n_segments; ++i) { sum += segment_records[i]; *seg_cap = std::max(*seg_cap, segment_records[i]); }
    return sum == records_per_stream ? GSV_OK : fail(GSV_ERR_INVALID, "the segments do not add up to records_per_stream");
  }
  static int count(uint64_t n_streams, uint64_t records_per_stream, const char* who) {
    if (n_streams == 0 || n_streams > 65535) return fail(GSV_ERR_INVALID, std::string(who) + " take 1 .. 65535 streams at a time");
    return records_per_stream > (~0ull >> 4) / n_streams ? fail(GSV_ERR_INVALID, "n_streams x records_per_stream x 16 bytes does not fit 64 bits") : GSV_OK;
  }
  // upload, begin(stream) -> status, t0, then feed -> status per segment (a receiver that could not begin is fed nothing)
  int run(gsv_engine* e, const uint8_t* data, uint64_t n_streams, uint64_t records_per_stream, const uint64_t* segment_records, uint64_t n_segments, const char* what, const std::function<int(hipStream_t)>& begin, const SegmentFeed& feed) {
    HIPCHK(hipSetDevice(e->device));
    DEVALLOC(d, size_t(n_streams) * size_t(records_per_stream) * 16, what);
    st = e->stream.get();
    if (records_per_stream) HIPCHK(hipMemcpyAsync(d.get(), data, size_t(n_streams) * size_t(records_per_stream) * 16, hipMemcpyHostToDevice, st));
    int rc = begin(st);
    HIPCHK(t0.create()); HIPCHK(t1.create());
    HIPCHK(hipEventRecord(t0.get(), st));
    for (uint64_t i = 0, off = 0; i < n_segments && rc == GSV_OK; off += segment_records[i++]) rc = feed(d.as<uint8_t>() + off * 16, records_per_stream, segment_records[i], st);
    return rc;
  }
  hipError_t stop(double* seconds) {  // t1 behind whatever the stream holds: the seconds since t0
    float ms = 0;
    hipError_t q = hipEventRecord(t1.get(), st);
    if (q == hipSuccess && (q = hipEventSynchronize(t1.get())) == hipSuccess && (q = hipEventElapsedTime(&ms, t0.get(), t1.get())) == hipSuccess) *seconds = double(ms) * 1e-3;
    return q;
  }
  ~StreamsOnDevice() { if (st) (void)hipStreamSynchronize(st); }  // (nothing of d is in flight when it is released: declare the receiver first)
};
// Received files hashed: fed to b3_begin / b3_segment / b3_finish as n streams.  With outboards every value the host receives is
// compared before it is absorbed; the values of a segment are looked at when the next segment has been enqueued.
int gsv_engine_blake3_files(gsv_engine* e, const char* const* paths, uint64_t n_files, const char* const* outboard_paths, uint8_t* digests, uint64_t* bad_file_out, uint64_t* bad_group_out) {
  if (!e || !paths || !digests) return fail(GSV_ERR_INVALID, "null argument");
  const uint32_t k = knobs::b3_subtree_log2();
  const uint64_t seg_knob = knobs::at_least_1("GSV_DRAIN_SEGMENT_RECORDS");
  if (int krc = check_b3_k(k)) return krc;
  if (n_files == 0 || n_files > 65535) return fail(GSV_ERR_INVALID, "BLAKE3 commitments take 1 .. 65535 streams at a time");
  FilesOnDevice f;
  if (int rc = f.open(paths, outboard_paths, size_t(n_files), seg_knob, [&](size_t i, FILE* file, uint64_t* records, std::string* why) { return mac_file_records(fileno(file), paths[i], records, why, Outboard::MAX_RECORDS); })) return rc;
  B3Check check;
  std::string why;
  if (outboard_paths) {
    check.shape(f.n, k, f.total);
    for (size_t i = 0; i < f.n; ++i) if (!load_outboard(outboard_paths[i], k, f.total, &check.bytes[i], &why)) return fail(GSV_ERR_INVALID, why);
  }
  std::unique_ptr<B3Stream> b;
  B3Receiver rx(b, "file", outboard_paths ? &check : nullptr);
  int rc = f.run(e, "the segment of the files to hash", [&] { return rx.begin(f.n, f.total, f.seg, k); }, [&](const void* gate, uint64_t stride, uint64_t m, hipStream_t st) { return rx.feed(gate, stride, m, st); });
  if (rc == GSV_OK) rc = rx.finish(e->stream.get(), digests);
  if (rc == GSV_ERR_MISMATCH) report_bad(bad_file_out, bad_group_out, check.bad_instance, check.bad_group);
  return rc;
}
// The kernels alone: the streams are fed to the chunk, reduce and carry code of the drain; the host finishes them.
int gsv_engine_blake3_streams(gsv_engine* e, const uint8_t* data, uint64_t n_streams, uint64_t records_per_stream, const uint64_t* segment_records, uint64_t n_segments, uint8_t* digests) {
  if (!e || !digests || (!data && records_per_stream) || (!segment_records && n_segments)) return fail(GSV_ERR_INVALID, "null argument");
  const uint32_t k = knobs::b3_subtree_log2();
  uint64_t seg_cap = 0;
  if (int rc = StreamsOnDevice::segments(segment_records, n_segments, records_per_stream, &seg_cap)) return rc;
  if (int krc = check_b3_k(k)) return krc;
  if (int rc = StreamsOnDevice::count(n_streams, records_per_stream, "BLAKE3 commitments")) return rc;
  std::unique_ptr<B3Stream> b;
  B3Receiver rx(b);
  StreamsOnDevice up;  // (a segment's group values are absorbed before the next one is enqueued)
  int rc = up.run(e, data, n_streams, records_per_stream, segment_records, n_segments, "the streams to hash", [&](hipStream_t) { return rx.begin(size_t(n_streams), records_per_stream, seg_cap, k); },
                  [&](const void* buf, uint64_t stride, uint64_t m, hipStream_t st) { return rx.feed(buf, stride, m, st); });
  if (rc == GSV_OK) rc = rx.flush();  // (in front of t1: the time covers the host's folding between the segments)
  if (rc == GSV_OK) {
    HIPCHK(up.stop(&e->b3_streams_seconds));
    rc = rx.finish(e->stream.get(), digests);
  }
  return rc;
}
int gsv_engine_blake3_streams_seconds(const gsv_engine* e, double* seconds) {
  if (!e || !seconds) return fail(GSV_ERR_INVALID, "null argument");
  *seconds = e->b3_streams_seconds;
  return GSV_OK;
}
