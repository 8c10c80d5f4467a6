// Part of engine.cpp: read-back of outputs and ciphertexts, step-clock diagnostics, program step statistics, commitments to the resident stream, CBC-MAC helpers.
int gsv_session_set_hasher(gsv_session* s, int kind) {
  if (!s || (kind != GSV_HASHER_AES && kind != GSV_HASHER_BLAKE3)) return fail(GSV_ERR_INVALID, "unknown hasher");
  s->hasher = kind;
  return GSV_OK;
}

int gsv_session_sync(gsv_session* s) {
  if (!s) return fail(GSV_ERR_INVALID, "null session");
  HIPCHK(hipSetDevice(s->e->device));
  HIPCHK(hipStreamSynchronize(s->e->stream.get()));
  if (s->plan) return check_plan_error(s);
  return GSV_OK;
}
// Diagnostics: per-step wall-clock stamps (100 MHz) of instance 0's workgroup during the last replay of a launch.
int gsv_session_enable_step_clock(gsv_session* s) {
  if (!s) return fail(GSV_ERR_INVALID, "null session");
  HIPCHK(hipSetDevice(s->e->device));
  if (!s->step_clock) {
    const size_t bytes = (size_t(s->prog().n_steps) + 1) * sizeof(uint64_t);
    HIPCHK(s->step_clock.alloc(bytes));
    HIPCHK(hipMemset(s->step_clock.get(), 0, bytes));
  }
  return GSV_OK;
}
int gsv_session_read_step_clock(gsv_session* s, uint64_t* out) {
  if (!s || !out || !s->step_clock || !s->ran) return fail(GSV_ERR_INVALID, "step clock not enabled / nothing ran");
  HIPCHK(hipSetDevice(s->e->device));
  HIPCHK(hipStreamSynchronize(s->e->stream.get()));
  HIPCHK(hipMemcpy(out, s->step_clock.get(), (size_t(s->prog().n_steps) + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return GSV_OK;
}
// Diagnostics: per step {and_cnt, xor_cnt, lds_reads, hbm_reads, lds_writes, hbm_writes} decoded from the compiled records.
int gsv_program_step_stats(const gsv_program* p, uint32_t* out6) {
  if (!p || !out6) return fail(GSV_ERR_INVALID, "null argument");
  { int rc = program_ready(p); if (rc) return rc; }
  const Program& g = p->prog;
  for (size_t s = 0; s < g.steps.size(); ++s) {
    const StepDesc& d = g.steps[s];
    uint32_t* o = out6 + 6 * s;
    o[0] = d.and_cnt; o[1] = d.xor_cnt; o[2] = o[3] = o[4] = o[5] = 0;
    auto rd = [&](uint32_t sl) { if (sl != SLOT_LDS_ZERO) o[(sl & SLOT_LDS_FLAG) ? 2 : 3]++; };
    auto wr = [&](uint32_t sl) { o[(sl & SLOT_LDS_FLAG) ? 4 : 5]++; };
    for (uint32_t k = 0; k < d.and_cnt; ++k) {
      const AndRec& r = g.ands[d.and_off + k];
      rd(uint32_t(r.w0) & SLOT_MASK); rd(uint32_t(r.w0 >> 21) & SLOT_MASK); rd(uint32_t(r.w0 >> 42) & SLOT_MASK);
      rd(uint32_t(r.w1) & SLOT_MASK); rd(uint32_t(r.w1 >> 21) & SLOT_MASK);
      if (g.and_terms == 4) { rd(uint32_t(r.w1 >> 42) & SLOT_MASK); rd(uint32_t(r.w2) & SLOT_MASK); rd(uint32_t(r.w2 >> 21) & SLOT_MASK); rd(uint32_t(r.w2 >> 42) & SLOT_MASK); wr(uint32_t(r.w3) & SLOT_MASK); }
      else wr(uint32_t(r.w1 >> 42) & SLOT_MASK);
    }
    for (uint32_t k = 0; k < d.xor_cnt; ++k) {
      const XorRec& r = g.xors[d.xor_off + k];
      rd(uint32_t(r.w0) & SLOT_MASK); rd(uint32_t(r.w0 >> 21) & SLOT_MASK); rd(uint32_t(r.w0 >> 42) & SLOT_MASK);
      rd(uint32_t(r.w1) & SLOT_MASK); wr(uint32_t(r.w1 >> 21) & SLOT_MASK);
    }
  }
  return GSV_OK;
}
int gsv_session_instances_per_workgroup(const gsv_session* s, int* n) {
  if (!s || !n) return fail(GSV_ERR_INVALID, "null argument");
  *n = int(s->launch_ni());
  return GSV_OK;
}
int gsv_session_last_kernel_ms(gsv_session* s, double* ms) {
  if (!s || !ms || !s->ran) return fail(GSV_ERR_INVALID, "no launch recorded");
  HIPCHK(hipEventSynchronize(s->ev1.get()));
  float f = 0;
  HIPCHK(hipEventElapsedTime(&f, s->ev0.get(), s->ev1.get()));
  *ms = f;
  return GSV_OK;
}
int gsv_session_read_outputs(gsv_session* s, uint8_t* labels, uint8_t* bits) {
  if (!s || !labels || !s->ran) return fail(GSV_ERR_INVALID, "bad argument / nothing ran");
  HIPCHK(hipSetDevice(s->e->device));
  HIPCHK(hipStreamSynchronize(s->e->stream.get()));
  if (s->plan) { int rc = check_plan_error(s); if (rc) return rc; }
  const size_t n = s->n_inst * s->prog().output_slots.size();
  if (n) HIPCHK(hipMemcpy(labels, s->out.get(), n * 16, hipMemcpyDeviceToHost));
  if (bits) {
    if (!s->last_eval) return fail(GSV_ERR_INVALID, "plaintext bits exist only after evaluate");
    if (n) HIPCHK(hipMemcpy(bits, s->out_bits.get(), n, hipMemcpyDeviceToHost));
  }
  return GSV_OK;
}
int gsv_session_read_ciphertexts(gsv_session* s, size_t instance, uint64_t first, uint64_t n_records, uint8_t* out) {
  if (!s || instance >= s->n_inst || (!out && n_records)) return fail(GSV_ERR_INVALID, "bad argument");
  if (s->plan && !s->retain()) return fail(GSV_ERR_INVALID, "this plan session does not retain the ciphertext stream");
  if (first + n_records > s->ct_stride()) return fail(GSV_ERR_INVALID, "range exceeds the retained ciphertext stream");
  HIPCHK(hipSetDevice(s->e->device));
  HIPCHK(hipStreamSynchronize(s->e->stream.get()));
  for (uint64_t off = 0; off < n_records; off += CT_STAGE_RECORDS) {
    const uint64_t n = std::min<uint64_t>(CT_STAGE_RECORDS, n_records - off);
    int rc = fetch_ciphertexts(s, instance, first + off, n, out + off * 16);
    if (rc) return rc;
  }
  return GSV_OK;
}
int gsv_session_ciphertext_hash(gsv_session* s, size_t instance, uint8_t hash[16]) {
  if (!s || instance >= s->n_inst || !hash) return fail(GSV_ERR_INVALID, "bad argument");
  if (s->ct_cap != s->replays || (s->plan && !s->retain())) return fail(GSV_ERR_INVALID, "the session retains only part of the stream (ct_capacity_replays < replays)");
  HIPCHK(hipSetDevice(s->e->device));
  HIPCHK(hipStreamSynchronize(s->e->stream.get()));
  const uint64_t total = s->ct_stride();
  const uint64_t chunk = CT_STAGE_RECORDS;
  std::vector<uint8_t> buf(size_t(std::min<uint64_t>(chunk, total ? total : 1)) * 16);
  CbcMacHost mac;
  for (uint64_t off = 0; off < total; off += chunk) {
    uint64_t n = std::min(chunk, total - off);
    int rc = fetch_ciphertexts(s, instance, off, n, buf.data());
    if (rc) return rc;
    mac.update(buf.data(), n);
  }
  mac.digest(hash);
  return GSV_OK;
}
// BLAKE3 of every instance's retained stream, hashed where it lies (blake3_device.hpp, b3_chunk_indexed_kernel): ranges of at most
// GSV_B3_RESIDENT_RECORDS records per instance — of the one ring (program sessions), of one call block after the other (plan sessions;
// chunks straddle ranges and blocks through the carry) — go through the chunk, reduce and carry code of the drain on the engine's stream.
int gsv_session_ciphertext_blake3(gsv_session* s, uint8_t* digests) {
  if (!s || !digests) return fail(GSV_ERR_INVALID, "null argument");
  const knobs::ResidentB3 kn;
  if (s->ct_cap != s->replays || (s->plan && !s->retain())) return fail(GSV_ERR_INVALID, "the session retains only part of the stream (ct_capacity_replays < replays)");
  const uint64_t total = s->ct_stride();
  if (int rc = check_resident_stream(s, total)) return rc;
  HIPCHK(hipSetDevice(s->e->device));
  uint64_t cap = kn.resident_records;
  if (!cap) {
    // two value buffers of (2^k - 1 pending + cap / 64 + 2) x 32 bytes per instance (b3_begin) in a tenth of what is free
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const uint64_t values = uint64_t(free_b) / 10 / (2 * 32 * s->n_inst), fixed = (1ull << std::min<uint32_t>(kn.b3_subtree_log2, 20)) + 2;
    cap = std::min<uint64_t>(64ull << 20, values > fixed ? (values - fixed) * 64 : 64);
  }
  cap = std::min(cap, std::max<uint64_t>(total, 1));
  const hipStream_t st = s->e->stream.get();
  std::unique_ptr<B3Stream> b;
  B3Receiver rx(b);
  struct Quiesce { hipStream_t st; ~Quiesce() { (void)hipStreamSynchronize(st); } } quiesce{st};  // declared after `b`: nothing of its buffers is in flight when they go
  int rc = rx.begin(s->n_inst, total, cap, kn.b3_subtree_log2);
  if (rc) return rc;
  Event t0, t1;
  HIPCHK(t0.create()); HIPCHK(t1.create());
  HIPCHK(hipEventRecord(t0.get(), st));
  // records [first, first + n) of the gate-order stream of one block (block_off records into every instance's stream, n_ct records per replay);
  // the group values of a range are out of the page-locked buffer before the next range is enqueued
  auto feed = [&](uint64_t block_off, const DevBuf& ct_pos, uint64_t n_ct, uint64_t block_records) -> int {
    for (uint64_t first = 0; first < block_records; first += cap) {
      const B3Indexed ix{ct_pos.get(), n_ct, first};
      if (int frc = rx.feed(static_cast<const uint8_t*>(s->CT.get()) + block_off * 16, s->ct_stride(), std::min(cap, block_records - first), st, &ix)) return frc;
    }
    return GSV_OK;
  };
  if (!s->plan) rc = total ? feed(0, s->dp->ct_pos, s->prog().n_ct, total) : GSV_OK;
  else
    for (size_t k = 0; k < s->plan->calls.size() && rc == GSV_OK; ++k) {
      const uint64_t n_ct = s->call_prog(k).n_ct;
      if (n_ct) rc = feed(s->plan->calls[k].ct_off, s->call_dev[k]->ct_pos, n_ct, n_ct);
    }
  if (rc == GSV_OK) rc = rx.flush();  // (in front of t1: the time covers the host's folding between the ranges)
  if (rc) return rc;
  float ms = 0;
  HIPCHK(hipEventRecord(t1.get(), st));
  HIPCHK(hipEventSynchronize(t1.get()));
  HIPCHK(hipEventElapsedTime(&ms, t0.get(), t1.get()));
  s->e->b3_streams_seconds = double(ms) * 1e-3;
  rc = rx.finish(st, digests);
  if (rc) return rc;
  return s->plan ? check_plan_error(s) : GSV_OK;  // (behind an asynchronous garble: a pass whose dependency wait gave up left no stream to commit to)
}
// The retained stream of every instance verified against checkpoint files where it lies (cbcmac_device.hpp, cbcmac_check_indexed_kernel):
// gsv_session_ciphertext_blake3's ranges — at most GSV_MAC_RESIDENT_RECORDS records per instance, of the one ring or of one call block
// after the other; groups straddle ranges and blocks through the carry — fed to the receiver of gsv_session_garble_streaming_check.
int gsv_session_ciphertext_cbcmac_check(gsv_session* s, const char* checkpoint_dir, const uint64_t* indexes, uint64_t first_index, const uint8_t* expected, uint8_t* hashes) {
  if (!s || !checkpoint_dir || !hashes) return fail(GSV_ERR_INVALID, "null argument");
  const knobs::ResidentMac kn;
  if (s->ct_cap != s->replays || (s->plan && !s->retain())) return fail(GSV_ERR_INVALID, "the session retains only part of the stream (ct_capacity_replays < replays)");
  const uint64_t total = s->ct_stride();
  if (int rc = check_resident_stream(s, total)) return rc;
  const size_t n = s->n_inst;
  std::vector<std::string> names(n);
  std::vector<const char*> ptrs(n);
  for (size_t i = 0; i < n; ++i) { names[i] = CheckpointWriter::path(checkpoint_dir, indexes ? indexes[i] : first_index + i); ptrs[i] = names[i].c_str(); }
  std::string why;
  std::vector<MacCheckpointFile> cks;
  if (!open_mac_checkpoints(ptrs.data(), n, &total, &cks, &why)) return fail(GSV_ERR_INVALID, why);
  clear_mismatch(s);
  // the commitments the files claim: compared with the ones the caller trusts before anything is launched
  std::vector<uint8_t> claimed(n * 16);
  for (size_t i = 0; i < n; ++i) {
    if (!cks[i].commitment(claimed.data() + 16 * i)) return fail(GSV_ERR_INVALID, "read error on " + cks[i].path());
    if (expected && std::memcmp(claimed.data() + 16 * i, expected + 16 * i, 16) != 0) {
      set_mismatch(s, i, ~0ull, ~0ull);
      return fail(GSV_ERR_MISMATCH, "the last checkpoint of instance " + std::to_string(i) + " does not match the commitment");
    }
  }
  HIPCHK(hipSetDevice(s->e->device));
  const uint32_t k = cks[0].head.k;
  uint64_t cap = kn.resident_records;
  if (!cap) {
    // only the slice of claimed states has to fit: (cap >> k) + 3 states of 16 bytes per instance, once on the device and twice
    // page-locked on the host (MacCheckReceiver::begin) — the three together in a tenth of what is free on the device
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const uint64_t states = uint64_t(free_b) / 10 / (3 * 16 * n);
    cap = std::min<uint64_t>(64ull << 20, states > 3 ? std::min<uint64_t>(states - 3, 64ull << 20) << k : 1);
  }
  cap = std::min(cap, std::max<uint64_t>(total, 1));
  const hipStream_t st = s->e->stream.get();
  std::unique_ptr<MacCheckStream> slot;
  MacCheckReceiver rx(slot, "the ciphertext stream of instance", s->e->te.get(), [&cks](size_t i, int64_t s0, uint64_t count, uint8_t* dst) { return cks[i].read_states(s0, count, dst); });
  struct Quiesce { hipStream_t st; ~Quiesce() { (void)hipStreamSynchronize(st); } } quiesce{st};  // declared after `slot`: nothing of its buffers is in flight when they go
  int rc = rx.begin(n, total, cap, k, st);
  if (rc) return rc;
  // records [first, first + m) of the gate-order stream of one block (block_off records into every instance's stream, whole replays of n_ct records)
  auto feed = [&](uint64_t block_off, const DevBuf& ct_pos, uint64_t n_ct, uint64_t block_records) -> int {
    for (uint64_t first = 0; first < block_records; first += cap) {
      const MacIndexed ix{ct_pos.get(), n_ct, block_records, first};
      if (int frc = rx.feed(static_cast<const uint8_t*>(s->CT.get()) + block_off * 16, s->ct_stride(), std::min(cap, block_records - first), st, &ix)) return frc;
    }
    return GSV_OK;
  };
  if (!s->plan) rc = total ? feed(0, s->dp->ct_pos, s->prog().n_ct, total) : GSV_OK;
  else
    for (size_t c = 0; c < s->plan->calls.size() && rc == GSV_OK; ++c) {
      const uint64_t n_ct = s->call_prog(c).n_ct;
      if (n_ct) rc = feed(s->plan->calls[c].ct_off, s->call_dev[c]->ct_pos, n_ct, n_ct);
    }
  if (rc == GSV_OK) rc = rx.finish();
  // behind an asynchronous garble: a pass whose dependency wait gave up left no stream to verify — that is the error to report, not
  // the mismatch the check finds in what the pass left behind (finish() has waited for the stream up to the last failing-group word)
  if (s->plan && (rc == GSV_OK || rc == GSV_ERR_MISMATCH)) {
    const std::string found = g_err;
    HIPCHK(hipStreamSynchronize(st));
    if (int prc = check_plan_error(s)) return prc;
    if (rc) g_err = found;
  }
  if (rc == GSV_ERR_MISMATCH) set_mismatch(s, rx.bad_instance, rx.bad_group, rx.bad_record);
  if (rc) return rc;
  std::memcpy(hashes, claimed.data(), claimed.size());
  return GSV_OK;
}
int gsv_cbcmac_chains_per_step(void) { return CbcMacHost::have_vaes() ? 16 : GSV_HOST_AESNI ? 4 : 1; }
int gsv_cbcmac_update_many(uint8_t* states, const uint8_t* const* cts, size_t n_chains, uint64_t n_records) {
  if ((!states || !cts) && n_chains) return fail(GSV_ERR_INVALID, "null argument");
  for (size_t i = 0; i < n_chains; ++i) if (!cts[i] && n_records) return fail(GSV_ERR_INVALID, "null stream");
  // CbcMacHost starts from zero: chain by XOR-ing the state into a copy of the first block (h ^ ct)
  if (n_records == 0) return GSV_OK;
  std::vector<CbcMacHost> macs(n_chains);
  for (size_t i = 0; i < n_chains; ++i) {
    uint8_t first[16];
    for (int k = 0; k < 16; ++k) first[k] = cts[i][k] ^ states[16 * i + k];
    macs[i].update(first, 1);
  }
  std::vector<CbcMacHost*> mp(n_chains);
  std::vector<const uint8_t*> cp(n_chains);
  for (size_t i = 0; i < n_chains; ++i) { mp[i] = &macs[i]; cp[i] = cts[i] + 16; }
  CbcMacHost::update_many(mp.data(), cp.data(), n_chains, n_records - 1);  // sixteen chains per step with VAES, else four
  for (size_t k = 0; k < n_chains; ++k) macs[k].digest(states + 16 * k);
  return GSV_OK;
}
int gsv_cbcmac_update(uint8_t state[16], const uint8_t* cts, uint64_t n_records) {  // one chain
  if (!state || (!cts && n_records)) return fail(GSV_ERR_INVALID, "null argument");
  return gsv_cbcmac_update_many(state, &cts, 1, n_records);
}
int gsv_commit_labels(const uint8_t* labels, uint64_t n, uint8_t* out) {
  if ((!labels || !out) && n) return fail(GSV_ERR_INVALID, "null argument");
  for (uint64_t i = 0; i < n; ++i) {  // AES_K(label): one-block CBC-MAC from zero state
    CbcMacHost mac;
    mac.update(labels + 16 * i, 1);
    mac.digest(out + 16 * i);
  }
  return GSV_OK;
}
