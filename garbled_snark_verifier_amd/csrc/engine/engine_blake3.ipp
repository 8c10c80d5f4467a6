// Part of engine.cpp: BLAKE3 commitments — the host hasher behind gsv_blake3_*, and the device tree hash of n equally long streams
// that arrive in segments of a gate-order buffer (blake3_device.hpp), shared by the streaming drain (engine_drain.ipp), the streaming
// evaluators (engine_evaluate.ipp), gsv_session_ciphertext_blake3 (engine_readback.ipp: it feeds ranges of the resident program-order stream) and
// gsv_engine_blake3_streams.
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
// a new stream set: buffers are kept when the shape is the one they were allocated for
static int b3_begin(std::unique_ptr<B3Stream>& p, size_t n_inst, uint64_t total, uint64_t seg_cap, uint32_t k) {
  if (n_inst == 0 || n_inst > 65535) return fail(GSV_ERR_INVALID, "BLAKE3 commitments take 1 .. 65535 streams at a time");
  if (k > 20) return fail(GSV_ERR_INVALID, "GSV_B3_SUBTREE_LOG2 must be an integer in [0, 20]");
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
// every record has been fed and every group value absorbed: the pending chunk values and the last chunks come to the host
static int b3_finish(B3Stream& b, hipStream_t st, uint8_t* digests) {
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
    const bool ok = on_pool([&](size_t i) { bool r = true; for (uint32_t g = 0; g < b.pend; ++g) r = b.hashers[i].absorb_subtree(b.pinned.get() + (i * b.pend + g) * 32, 0) && r; return r; });
    if (!ok) return fail(GSV_ERR_INVALID, "internal: BLAKE3 chunk values out of order");
  }
  if (b.carry_n) {
    HIPCHK(hipMemcpyAsync(b.pinned.get(), b.carry[b.cpar].get(), b.n_inst * 1024, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  if (!on_pool([&](size_t i) { b.hashers[i].update(b.pinned.get() + i * 1024, uint64_t(b.carry_n) * 16); return b.hashers[i].finalize(digests + 32 * i); }))
    return fail(GSV_ERR_INVALID, "internal: BLAKE3 stream without a last chunk");
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
// The kernels alone: n_streams streams of records_per_stream records each (data: [stream][record]) are uploaded and fed to the chunk,
// reduce and carry code of the drain in the given segmentation; the host finishes them.
int gsv_engine_blake3_streams(gsv_engine* e, const uint8_t* data, uint64_t n_streams, uint64_t records_per_stream, const uint64_t* segment_records, uint64_t n_segments, uint8_t* digests) {
  if (!e || !digests || (!data && records_per_stream) || (!segment_records && n_segments)) return fail(GSV_ERR_INVALID, "null argument");
  const uint32_t k = knobs::b3_subtree_log2();
  uint64_t sum = 0, seg_cap = 0;
  for (uint64_t i = 0; i < n_segments; ++i) { sum += segment_records[i]; seg_cap = std::max(seg_cap, segment_records[i]); }
  if (sum != records_per_stream) return fail(GSV_ERR_INVALID, "the segments do not add up to records_per_stream");
  if (k > 20) return fail(GSV_ERR_INVALID, "GSV_B3_SUBTREE_LOG2 must be an integer in [0, 20]");
  if (n_streams == 0 || n_streams > 65535) return fail(GSV_ERR_INVALID, "BLAKE3 commitments take 1 .. 65535 streams at a time");
  if (records_per_stream > (~0ull >> 4) / n_streams) return fail(GSV_ERR_INVALID, "n_streams x records_per_stream x 16 bytes does not fit 64 bits");
  HIPCHK(hipSetDevice(e->device));
  DevBuf d;
  DEVALLOC(d, size_t(n_streams) * size_t(records_per_stream) * 16, "the streams to hash");
  if (records_per_stream) HIPCHK(hipMemcpyAsync(d.get(), data, size_t(n_streams) * size_t(records_per_stream) * 16, hipMemcpyHostToDevice, e->stream.get()));
  std::unique_ptr<B3Stream> b;
  int rc = b3_begin(b, size_t(n_streams), records_per_stream, seg_cap, k);
  Event t0, t1;
  HIPCHK(t0.create()); HIPCHK(t1.create());
  HIPCHK(hipEventRecord(t0.get(), e->stream.get()));
  uint64_t off = 0;
  for (uint64_t i = 0; i < n_segments && rc == GSV_OK; ++i) {
    uint32_t groups = 0;
    rc = b3_segment(*b, d.as<uint8_t>() + off * 16, records_per_stream, segment_records[i], e->stream.get(), &groups);
    off += segment_records[i];
    if (rc == GSV_OK && groups) {
      HIPCHK(hipStreamSynchronize(e->stream.get()));
      if (!b3_absorb(*b, b->pinned.get(), groups, k, 0, 1)) rc = fail(GSV_ERR_INVALID, "internal: BLAKE3 group values out of order");
    }
  }
  if (rc == GSV_OK) {
    float ms = 0;
    HIPCHK(hipEventRecord(t1.get(), e->stream.get()));
    HIPCHK(hipEventSynchronize(t1.get()));
    HIPCHK(hipEventElapsedTime(&ms, t0.get(), t1.get()));
    e->b3_streams_seconds = double(ms) * 1e-3;
    rc = b3_finish(*b, e->stream.get(), digests);
  }
  (void)hipStreamSynchronize(e->stream.get());  // (nothing of d is in flight when it is released)
  return rc;
}
int gsv_engine_blake3_streams_seconds(const gsv_engine* e, double* seconds) {
  if (!e || !seconds) return fail(GSV_ERR_INVALID, "null argument");
  *seconds = e->b3_streams_seconds;
  return GSV_OK;
}
