// Part of engine.cpp: CBC-MAC commitments verified against chain checkpoints (mac_checkpoints.hpp: the format, the host writer and the
// host checker; cbcmac_device.hpp: the kernel).  n equally long streams arrive in segments of a gate-order buffer, as for the BLAKE3
// commitments (engine_blake3.ipp); per segment the MacCheckReceiver uploads the slice of claimed states the segment touches, launches
// the check, and looks at the failing-group words of the segment BEFORE — after this one has been enqueued.
//
// Soundness: every group starts from the CLAIMED state in front of it, so the groups are independent chains; if all of
// them arrive at their claimed states, and state -1 is zero, the stream's true CBC-MAC is the last claimed state.  The checkpoint
// files are untrusted input: a wrong one can only make the check fail.
struct MacCheckStream : MacCheckPosition {  // (cpar; records_done, fed: records per stream, and segments, enqueued so far)
  size_t n_inst = 0;
  uint32_t k = 0;
  uint64_t total = 0, seg_cap = 0, slice_cap = 0;  // slice_cap: most claimed states per instance a segment touches
  DevBuf slice, carry[2], bad;
  MappedHost<uint8_t> stage[2];                    // the slice of a segment on its way up, [instance][state] dense: ping-pong
  MappedHost<unsigned long long> bad_host[2];      // the failing-group words behind a segment
};
static int check_mac_k(uint32_t k) { return k > MacCheckpoints::MAX_K ? fail(GSV_ERR_INVALID, "GSV_MAC_GROUP_LOG2 must be an integer in [0, 30]") : GSV_OK; }
// states [s0, s0 + count) of instance i -> dst; s0 = -1: the zero state in front of the stream.  False: they cannot be read.
using MacStateSource = std::function<bool(size_t i, int64_t s0, uint64_t count, uint8_t* dst)>;
// A segment that lies in program order (gsv_session_ciphertext_cbcmac_check): records [first, first + n) of the gate-order stream of a
// block of block_records records, read through the position table (cbcmac_check_indexed_kernel); `buf` is then the block, `stride` its stride
struct MacIndexed { const void* ct_pos; uint64_t n_ct, block_records, first; };

struct MacCheckReceiver {
  std::unique_ptr<MacCheckStream>& slot;  // the caller's
  const char* noun;                       // what a mismatch calls a stream: "file", "stream"
  const void* te;                         // the engine's device T-tables
  MacStateSource states;
  Event ev[2];
  bool in_flight[2] = {false, false};
  bool on = false;
  size_t bad_instance = 0;
  uint64_t bad_group = 0, bad_record = 0;
  MacCheckReceiver(std::unique_ptr<MacCheckStream>& slot_, const char* noun_, const void* te_, MacStateSource states_) : slot(slot_), noun(noun_), te(te_), states(std::move(states_)) {}
  int begin(size_t n_inst, uint64_t total, uint64_t seg_cap, uint32_t k, hipStream_t st) {
    if (n_inst == 0 || n_inst > 65535) return fail(GSV_ERR_INVALID, "CBC-MAC checks take 1 .. 65535 streams at a time");
    if (int rc = check_mac_k(k)) return rc;
    if (total > MacCheckpoints::MAX_RECORDS) return fail(GSV_ERR_INVALID, "n_records " + std::to_string(total) + " is out of range");
    seg_cap = std::max<uint64_t>(1, std::min(seg_cap, std::max<uint64_t>(total, 1)));
    const uint64_t slice_cap = (seg_cap >> k) + 3;  // a segment of n records touches at most ((n - 1) >> k) + 2 groups, and one state more
    if (!slot || slot->n_inst != n_inst || slot->slice_cap < slice_cap) {
      slot.reset(new MacCheckStream());
      MacCheckStream& m = *slot;
      bool ok = slice_cap <= (~size_t(0) >> 5) / n_inst;
      ok = ok && m.slice.alloc(n_inst * size_t(slice_cap) * 16) == hipSuccess && m.bad.alloc(n_inst * 8) == hipSuccess;
      for (int i = 0; i < 2; ++i)
        ok = ok && m.carry[i].alloc(n_inst * 16) == hipSuccess && m.stage[i].alloc(n_inst * size_t(slice_cap) * 16, hipHostMallocDefault) == hipSuccess && m.bad_host[i].alloc(n_inst * 8, hipHostMallocDefault) == hipSuccess;
      if (!ok) { slot.reset(); (void)hipGetLastError(); return fail(GSV_ERR_DEVICE, "cannot allocate the buffers of the CBC-MAC check (" + std::to_string(slice_cap) + " states per stream and segment)"); }
      m.slice_cap = slice_cap;
    }
    MacCheckStream& m = *slot;
    m.n_inst = n_inst; m.k = k; m.total = total; m.seg_cap = seg_cap;
    static_cast<MacCheckPosition&>(m) = MacCheckPosition();
    for (int i = 0; i < 2; ++i) { HIPCHK(ev[i].create(hipEventDisableTiming)); in_flight[i] = false; }
    HIPCHK(hipMemsetAsync(m.bad.get(), 0xff, n_inst * 8, st));
    on = true;
    return GSV_OK;
  }
  // ... or goes on with streams an earlier receiver began (a later slice of a sliced garbling pass): nothing is reset, nothing is in
  // flight — every slice ends with a finish() — and the carries, the failing-group words and the position stand where they stood
  int resume(size_t n_inst, uint64_t total, uint64_t seg_cap, uint32_t k) {
    if (!slot || slot->n_inst != n_inst || slot->total != total || slot->k != k)
      return fail(GSV_ERR_INVALID, "this slice continues a pass whose earlier slices ran no CBC-MAC check of this shape (instances, checkpoint files)");
    if (slot->slice_cap < (std::max<uint64_t>(1, std::min(seg_cap, std::max<uint64_t>(total, 1))) >> k) + 3 || slot->seg_cap < std::min(seg_cap, std::max<uint64_t>(total, 1)))
      return fail(GSV_ERR_INVALID, "internal: the schedule's largest segment grew in the middle of a pass: the buffers of the CBC-MAC check cannot hold it");
    for (int i = 0; i < 2; ++i) { HIPCHK(ev[i].create(hipEventDisableTiming)); in_flight[i] = false; }
    on = true;
    return GSV_OK;
  }
  int mismatch() const {
    return fail(GSV_ERR_MISMATCH, std::string(noun) + " " + std::to_string(bad_instance) + " does not match its checkpoints in group " + std::to_string(bad_group) + " (from record " + std::to_string(bad_record) + ")");
  }
  // the failing-group words behind the segment in buffer b: waited for and looked at.  The lowest group first, then the lowest instance.
  int look(int b) {
    if (!in_flight[b]) return GSV_OK;
    in_flight[b] = false;
    if (hipEventSynchronize(ev[b].get()) != hipSuccess) return fail(GSV_ERR_DEVICE, "event wait failed");
    const unsigned long long* w = slot->bad_host[b].get();
    unsigned long long lowest = ~0ull;
    for (size_t i = 0; i < slot->n_inst; ++i) if (w[i] < lowest) { lowest = w[i]; bad_instance = i; }
    if (lowest == ~0ull) return GSV_OK;
    bad_group = lowest; bad_record = lowest << slot->k;
    return mismatch();
  }
  // the next n records of every stream: buf[inst * stride + r], r < n.  The words of the segment before are looked at once this one is enqueued.
  int feed(const void* buf, uint64_t stride, uint64_t n, hipStream_t st, const MacIndexed* ix = nullptr) {
    if (!on || n == 0) return GSV_OK;
    MacCheckStream& m = *slot;
    if (n > m.seg_cap || m.records_done + n > m.total || (!ix && n > stride)) return fail(GSV_ERR_INVALID, "internal: CBC-MAC check segment outside the stream");
    const int b = int(m.fed & 1);  // (its last upload is two segments old, and the segment before this one was waited for behind it)
    const uint64_t first = m.records_done, n_states = ((first + n - 1) >> m.k) - (first >> m.k) + 2;  // one chain per group the segment touches (cbcmac_device.hpp, mac_chain_count), and one state more
    if (n_states > m.slice_cap) return fail(GSV_ERR_INVALID, "internal: CBC-MAC check slice overflow");
    for (size_t i = 0; i < m.n_inst; ++i)
      if (!states(i, int64_t(first >> m.k) - 1, n_states, m.stage[b].get() + i * size_t(n_states) * 16)) return fail(GSV_ERR_INVALID, std::string("cannot read the checkpoints of ") + noun + " " + std::to_string(i));
    HIPCHK(hipMemcpyAsync(m.slice.get(), m.stage[b].get(), m.n_inst * size_t(n_states) * 16, hipMemcpyHostToDevice, st));
    const int krc = ix ? gsvk_cbcmac_check_indexed(te, buf, stride, ix->ct_pos, ix->n_ct, ix->block_records, ix->first, first, n, m.k, m.total, m.slice.get(), n_states, m.carry[m.cpar].get(), m.carry[m.cpar ^ 1].get(), m.bad.get(), uint32_t(m.n_inst), st)
                       : gsvk_cbcmac_check(te, buf, stride, first, n, m.k, m.total, m.slice.get(), n_states, m.carry[m.cpar].get(), m.carry[m.cpar ^ 1].get(), m.bad.get(), uint32_t(m.n_inst), st);
    if (krc != 0) {
      (void)hipGetLastError();
      return fail(GSV_ERR_DEVICE, "CBC-MAC check kernel launch failed");
    }
    m.advance(n);
    HIPCHK(hipMemcpyAsync(m.bad_host[b].get(), m.bad.get(), m.n_inst * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(ev[b].get(), st));
    in_flight[b] = true;
    return look(b ^ 1);
  }
  // the end of the streams: whatever is still in flight is looked at, the older segment first
  int finish(bool end_of_streams = true) {
    if (!on) return GSV_OK;
    const int older = int(slot->fed & 1);
    if (int rc = look(older)) return rc;
    if (int rc = look(older ^ 1)) return rc;
    if (end_of_streams && slot->records_done != slot->total) return fail(GSV_ERR_INVALID, "internal: CBC-MAC check ended early");
    return GSV_OK;
  }
};

// The check's state <-> a restart point of a sliced evaluation (EvalRestart, engine_blake3.ipp), through st.  Between two slices nothing
// is in flight and no group has failed: the device half is the carries (the failing-group words are all ones), the host half the position.
static int mac_save(const MacCheckStream& m, EvalRestart& r, hipStream_t st) {
  for (int i = 0; i < 2; ++i) {
    if (int rc = ensure_dev(r.mac_carry[i], m.n_inst * 16, "a restart point's CBC-MAC carries")) return rc;
    HIPCHK(hipMemcpyAsync(r.mac_carry[i].get(), m.carry[i].get(), m.n_inst * 16, hipMemcpyDeviceToDevice, st));
  }
  r.mac_position = m;
  r.mac = true;
  return GSV_OK;
}
static int mac_restore(MacCheckStream& m, const EvalRestart& r, hipStream_t st) {
  for (int i = 0; i < 2; ++i) {
    if (r.mac_carry[i].bytes() < m.n_inst * 16) return fail(GSV_ERR_INVALID, "internal: a restart point of another CBC-MAC check shape");
    HIPCHK(hipMemcpyAsync(m.carry[i].get(), r.mac_carry[i].get(), m.n_inst * 16, hipMemcpyDeviceToDevice, st));
  }
  HIPCHK(hipMemsetAsync(m.bad.get(), 0xff, m.n_inst * 8, st));  // (the failed slice may have lowered them)
  static_cast<MacCheckPosition&>(m) = r.mac_position;
  return GSV_OK;
}

static uint32_t mac_group_log2_or(uint32_t k) { return k == GSV_MAC_GROUP_DEFAULT ? knobs::mac_group_log2() : k; }

// ---- the host side (include/gsv_engine.h "CBC-MAC checkpoints") ----
int gsv_cbcmac_checkpoints_size(uint64_t n_records, uint32_t k, uint64_t* bytes) {
  k = mac_group_log2_or(k);
  if (int rc = check_mac_k(k)) return rc;
  if (n_records > MacCheckpoints::MAX_RECORDS) return fail(GSV_ERR_INVALID, "n_records " + std::to_string(n_records) + " is out of range");
  if (bytes) *bytes = MacCheckpoints::file_bytes(n_records, k);
  return GSV_OK;
}
int gsv_cbcmac_file_checkpoints(const char* path, uint32_t k, const char* out_path, uint8_t* hash) {
  if (!path || !hash) return fail(GSV_ERR_INVALID, "null argument");
  k = mac_group_log2_or(k);
  if (int rc = check_mac_k(k)) return rc;
  std::string why;
  if (!mac_checkpoints_of_file(path, k, out_path, hash, &why)) return fail(GSV_ERR_INVALID, why);
  return GSV_OK;
}
int gsv_cbcmac_file_check(const char* path, const char* checkpoints_path, int n_threads, uint8_t* hash, uint64_t* bad_group) {
  if (!path || !checkpoints_path || !hash) return fail(GSV_ERR_INVALID, "null argument");
  std::string why;
  MacCheckpointFile ck;
  uint64_t bad = ~0ull;
  if (!ck.open(checkpoints_path, &why)) return fail(GSV_ERR_INVALID, why);
  const size_t T = n_threads > 0 ? size_t(n_threads) : std::max<size_t>(1, std::min<size_t>(16, std::thread::hardware_concurrency()));
  if (!mac_check_file(path, ck, T, &bad, &why)) return fail(GSV_ERR_INVALID, why);
  if (bad != ~0ull) {
    if (bad_group) *bad_group = bad;
    return fail(GSV_ERR_MISMATCH, std::string(path) + " does not match its checkpoints in group " + std::to_string(bad) + " (from record " + std::to_string(bad << ck.head.k) + ")");
  }
  if (!ck.commitment(hash)) return fail(GSV_ERR_INVALID, "read error on " + ck.path());
  return GSV_OK;
}

// ---- the device side ----
// The kernel alone: n_streams streams of records_per_stream records (data: [stream][record]) are uploaded and checked in the given
// segmentation against n_streams checkpoint files in memory (checkpoints: [stream][checkpoint_bytes]).
int gsv_engine_cbcmac_streams_check(gsv_engine* e, const uint8_t* data, uint64_t n_streams, uint64_t records_per_stream, const uint64_t* segment_records, uint64_t n_segments,
                                    const uint8_t* checkpoints, uint64_t checkpoint_bytes, uint64_t* bad_stream, uint64_t* bad_group) {
  if (!e || !checkpoints || (!data && records_per_stream) || (!segment_records && n_segments)) return fail(GSV_ERR_INVALID, "null argument");
  uint64_t seg_cap = 0;
  if (int rc = StreamsOnDevice::segments(segment_records, n_segments, records_per_stream, &seg_cap)) return rc;
  if (int rc = StreamsOnDevice::count(n_streams, records_per_stream, "CBC-MAC checks")) return rc;
  MacCheckpoints head;
  std::string why;
  for (uint64_t i = 0; i < n_streams; ++i) {
    MacCheckpoints h;
    if (!MacCheckpoints::parse_header(checkpoints + i * checkpoint_bytes, checkpoint_bytes, &h, &why)) return fail(GSV_ERR_INVALID, "checkpoints of stream " + std::to_string(i) + ": " + why);
    if (h.n_records != records_per_stream) return fail(GSV_ERR_INVALID, "checkpoints of stream " + std::to_string(i) + ": for a stream of " + std::to_string(h.n_records) + " records, the stream here holds " + std::to_string(records_per_stream));
    if (i && h.k != head.k) return fail(GSV_ERR_INVALID, "the checkpoints of one call must agree on k: stream 0 has " + std::to_string(head.k) + ", stream " + std::to_string(i) + " has " + std::to_string(h.k));
    if (!h.length_ok(checkpoint_bytes, &why)) return fail(GSV_ERR_INVALID, "checkpoints of stream " + std::to_string(i) + ": " + why);
    head = h;
  }
  const uint64_t n_states = head.states();
  std::unique_ptr<MacCheckStream> slot;
  MacCheckReceiver rx(slot, "stream", e->te.get(), [&](size_t i, int64_t s0, uint64_t count, uint8_t* dst) {
    if (count && s0 < 0) { std::memset(dst, 0, 16); dst += 16; ++s0; --count; }
    if (uint64_t(s0) + count > n_states) return false;
    std::memcpy(dst, checkpoints + i * checkpoint_bytes + MacCheckpoints::HEADER_BYTES + uint64_t(s0) * 16, size_t(count) * 16);
    return true;
  });
  StreamsOnDevice up;
  int rc = up.run(e, data, n_streams, records_per_stream, segment_records, n_segments, "the streams to check", [&](hipStream_t st) { return rx.begin(size_t(n_streams), records_per_stream, seg_cap, head.k, st); },
                  [&](const void* buf, uint64_t stride, uint64_t m, hipStream_t st) { return rx.feed(buf, stride, m, st); });
  if (rc == GSV_OK) rc = rx.finish();
  if (rc == GSV_OK || rc == GSV_ERR_MISMATCH) (void)up.stop(&e->mac_check_seconds);  // (behind finish(), and on a mismatch too: the time runs to the last failing-group word)
  if (rc == GSV_ERR_MISMATCH) report_bad(bad_stream, bad_group, rx.bad_instance, rx.bad_group);
  return rc;
}
int gsv_engine_cbcmac_streams_check_seconds(const gsv_engine* e, double* seconds) {
  if (!e || !seconds) return fail(GSV_ERR_INVALID, "null argument");
  *seconds = e->mac_check_seconds;
  return GSV_OK;
}
// Received files verified where the kernels are, without evaluating them: gsv_engine_blake3_files with the CBC-MAC check in the place of
// the hash (FilesOnDevice + the receiver).  The checkpoint files are never held whole.
int gsv_engine_cbcmac_files(gsv_engine* e, const char* const* paths, uint64_t n_files, const char* const* checkpoint_paths, const uint8_t* expected, uint8_t* hashes,
                            uint64_t* bad_file_out, uint64_t* bad_group_out) {
  if (!e || !paths || !checkpoint_paths || !hashes) return fail(GSV_ERR_INVALID, "null argument");
  const uint64_t seg_knob = knobs::at_least_1("GSV_DRAIN_SEGMENT_RECORDS");
  if (n_files == 0 || n_files > 65535) return fail(GSV_ERR_INVALID, "CBC-MAC checks take 1 .. 65535 streams at a time");
  FilesOnDevice f;
  if (int rc = f.open(paths, checkpoint_paths, size_t(n_files), seg_knob, [&](size_t i, FILE* file, uint64_t* records, std::string* why) { return mac_file_records(fileno(file), paths[i], records, why); })) return rc;
  const size_t n = f.n;
  std::string why;
  std::vector<MacCheckpointFile> cks;
  if (!open_mac_checkpoints(checkpoint_paths, n, &f.total, &cks, &why)) return fail(GSV_ERR_INVALID, why);
  // the commitments the files claim: compared with the ones the caller trusts before anything is uploaded
  std::vector<uint8_t> claimed(n * 16);
  for (size_t i = 0; i < n; ++i) {
    if (!cks[i].commitment(claimed.data() + 16 * i)) return fail(GSV_ERR_INVALID, "read error on " + cks[i].path());
    if (expected && std::memcmp(claimed.data() + 16 * i, expected + 16 * i, 16) != 0) {
      report_bad(bad_file_out, bad_group_out, i, ~0ull);
      return fail(GSV_ERR_MISMATCH, "the last checkpoint of file " + std::to_string(i) + " does not match the commitment");
    }
  }
  if (f.total == 0) { std::memcpy(hashes, claimed.data(), claimed.size()); return GSV_OK; }
  std::unique_ptr<MacCheckStream> slot;
  MacCheckReceiver rx(slot, "file", e->te.get(), [&](size_t i, int64_t s0, uint64_t count, uint8_t* dst) { return cks[i].read_states(s0, count, dst); });
  int rc = f.run(e, "the segment of the files to check", [&] { return rx.begin(n, f.total, f.seg, cks[0].head.k, e->stream.get()); }, [&](const void* gate, uint64_t stride, uint64_t m, hipStream_t st) { return rx.feed(gate, stride, m, st); });
  if (rc == GSV_OK) rc = rx.finish();
  if (rc == GSV_ERR_MISMATCH) report_bad(bad_file_out, bad_group_out, rx.bad_instance, rx.bad_group);
  if (rc == GSV_OK) std::memcpy(hashes, claimed.data(), claimed.size());
  return rc;
}
