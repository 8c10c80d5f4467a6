// Part of engine.cpp: GarbleCommit, the commitments of one slice of a streaming garbling pass — what the drain (engine_drain.ipp) carries
// beside launching windows and draining them: the BLAKE3 state and its absorbers, the outboards, the CBC-MAC checkpoint files and the check
// against such files on the device.  What may be combined is DrainSink's business (drain_pipeline.hpp); the session keeps what chains from slice to slice.
static int fail_drain(DrainError e) {
  switch (e) {
    case DrainError::FileWrite: return fail(GSV_ERR_INVALID, "short write to a gc or outboard file");
    case DrainError::Sink: return fail(GSV_ERR_INVALID, "the ciphertext sink reported an error");
    case DrainError::OutboardSink: return fail(GSV_ERR_INVALID, "the outboard sink reported an error");
    case DrainError::B3Order: return fail(GSV_ERR_INVALID, "internal: BLAKE3 group values out of order");
    default: return fail(GSV_ERR_DEVICE, "device copy failed while draining ciphertexts");
  }
}
// begin() — what the session carries — then open() — what this slice writes and reads —; per segment feed() on the stream the segment
// was gathered on and, once that stream has been synchronised, submit(); join() when the last segment is in; close() ends the slice.
// Lifetime: the absorbers' threads write the outboards and fold into the session's BLAKE3 state, the drain's MAC workers write the
// checkpoint files.  The absorbers are the LAST member — joined first, however the caller returns — and the caller declares its
// DrainWorkers after this object; only then do the writers go, and they REMOVE their files unless close() succeeded.
struct GarbleCommit {
  std::atomic<DrainError> err{DrainError::None};  // the one error slot of the slice's pools: the drain's workers share it
  GarbleCommit(gsv_session* s, const DrainSink& sink)
      : s_(s), sink_(sink), flags_(sink.commit()),
        mac_rx_(s->mac_check, "the ciphertext stream of instance", s->e->te.get(), [this](size_t i, int64_t s0, uint64_t count, uint8_t* dst) { return mcks_[i].read_states(s0, count, dst); }) {}
  // A plan's later slices repeat the commitments of the first; the checkpoint files' group size is the one the pass began with; the
  // BLAKE3 state lives in the session like the MAC states — a new pass starts it afresh, later slices chain.
  int begin(bool new_pass, size_t n_inst, uint64_t seg_records) {
    new_pass_ = new_pass; n_inst_ = n_inst; seg_records_ = seg_records;
    if (new_pass || !s_->plan) s_->pass_commit = flags_;
    else if (const char* why = commit_slice_conflict(s_->pass_commit, flags_)) return fail(GSV_ERR_INVALID, why);
    if (want(PassCommit::Checkpoints) && new_pass) { if (int rc = check_mac_k(s_->pass.mac_group_log2)) return rc; s_->mck_k = s_->pass.mac_group_log2; }
    if (want(PassCommit::B3)) {
      if (new_pass) { if (int rc = b3_begin(s_->b3, n_inst, stream_records(s_), seg_records, s_->pass.b3_subtree_log2)) return rc; }
      else if (!s_->b3 || s_->b3->n_inst != n_inst || s_->b3->seg_cap < seg_records) return fail(GSV_ERR_INVALID, "this slice continues a pass whose earlier slices computed no BLAKE3 commitment for these instances");
    }
    return GSV_OK;
  }
  // mac_stream: where the segments are gathered (a new check clears its failing-group words there)
  int open(hipStream_t mac_stream) {
    const uint64_t records = stream_records(s_);
    if (std::string failed; want(PassCommit::Checkpoints) && !checkpoints_.open(sink_.checkpoint_dir, sink_.first_index, n_inst_, new_pass_, s_->mck_k, records, &failed)) return fail(GSV_ERR_INVALID, "cannot create " + failed);
    // The CBC-MAC check: the checkpoint files are opened and validated by every slice (headers and lengths; they are never held whole);
    // the receiver's device state lives in the session and restarts with a pass that starts at call 0
    if (want(PassCommit::MacCheck)) {
      std::vector<std::string> names(n_inst_);
      std::vector<const char*> ptrs(n_inst_);
      for (size_t i = 0; i < n_inst_; ++i) { names[i] = CheckpointWriter::path(sink_.mac_check_dir, sink_.mac_check_indexes ? sink_.mac_check_indexes[i] : sink_.first_index + i); ptrs[i] = names[i].c_str(); }
      std::string why;
      if (!open_mac_checkpoints(ptrs.data(), n_inst_, &records, &mcks_, &why)) return fail(GSV_ERR_INVALID, why);
      claimed_.resize(n_inst_ * 16);
      for (size_t i = 0; i < n_inst_; ++i) {
        if (!mcks_[i].commitment(claimed_.data() + 16 * i)) return fail(GSV_ERR_INVALID, "read error on " + mcks_[i].path());
        if (new_pass_ && sink_.mac_check_expected && std::memcmp(claimed_.data() + 16 * i, sink_.mac_check_expected + 16 * i, 16) != 0) {
          set_mismatch(s_, i, ~0ull, ~0ull);
          return fail(GSV_ERR_MISMATCH, "the last checkpoint of instance " + std::to_string(i) + " does not match the commitment");
        }
      }
      if (int rc = new_pass_ ? mac_rx_.begin(n_inst_, records, seg_records_, mcks_[0].head.k, mac_stream) : mac_rx_.resume(n_inst_, records, seg_records_, mcks_[0].head.k)) return rc;
    }
    const B3Stream* const b = s_->b3.get();
    if (std::string failed; sink_.outboard_dir && !outboards_.open(sink_.outboard_dir, sink_.first_index, n_inst_, new_pass_, b->k, b->total, &failed)) return fail(GSV_ERR_INVALID, "cannot create " + failed);
    // (a later slice goes on behind the group values of the earlier ones: every chunk hashed so far but the pending ones is in a group)
    if (sink_.ob_fn && !sink_.outboard_dir && !outboards_.open(sink_.ob_fn, sink_.ob_user, n_inst_, new_pass_, b->k, b->total, (b->chunks_done - b->pend) >> b->k)) return fail_drain(DrainError::OutboardSink);
    if (want(PassCommit::B3))
      absorbers_.emplace(std::min<size_t>(4, n_inst_), [b3s = s_->b3.get(), obf = outboards(), err = &err](const uint8_t* vals, uint32_t groups, size_t t, size_t n) {
        if (obf && !obf->append(vals, groups, t, n)) drain_set_error(*err, obf->to_callback() ? DrainError::OutboardSink : DrainError::FileWrite);  // thread t keeps the values of ITS instances as it receives them
        return b3_absorb(*b3s, vals, groups, b3s->k, t, n);
      }, err);
    return GSV_OK;
  }
  CheckpointWriter* checkpoints() { return want(PassCommit::Checkpoints) ? &checkpoints_ : nullptr; }  // for the MAC workers
  // The next n records of every instance lie in gate[inst * stride + r]: the hash kernels and the check follow the gather on st (the
  // words of the segment before are looked at here); the buffer is free again when they have finished.
  int feed(const void* gate, uint64_t stride, uint64_t n, hipStream_t st) {
    groups_ = 0;
    if (want(PassCommit::B3)) if (int rc = b3_segment(*s_->b3, gate, stride, n, st, &groups_)) return rc;
    return want(PassCommit::MacCheck) ? mac_rx_.feed(gate, stride, n, st) : GSV_OK;
  }
  // ... and st has been synchronised: the segment's group values leave the page-locked buffer for the absorbers
  void submit() { if (absorbers_) absorbers_->submit(s_->b3->pinned.get(), n_inst_ * size_t(groups_) * 32, groups_); }
  void join() { if (absorbers_) absorbers_->finish(); }  // every submitted value absorbed, the threads gone
  // The end of the slice, after join() and the drain's own finish: `rc` is what the device side ended with, the status comes back.  In
  // this order: a host-side error first; every slice looks at what its last segments left behind (nothing of the check is in flight
  // between two slices); files are flushed before anything is reported; outputs are written, and files kept, on success only.
  int close(int rc, bool end_of_pass) {
    OutboardWriter* const obf = outboards();
    if (rc == GSV_OK && err != DrainError::None) rc = fail_drain(err);
    if (rc == GSV_OK && want(PassCommit::MacCheck)) rc = mac_rx_.finish(end_of_pass);
    if (want(PassCommit::MacCheck) && rc == GSV_ERR_MISMATCH) set_mismatch(s_, mac_rx_.bad_instance, mac_rx_.bad_group, mac_rx_.bad_record);
    if (rc == GSV_OK && want(PassCommit::Checkpoints) && !checkpoints_.flush()) rc = fail(GSV_ERR_INVALID, "short write to a checkpoint file");
    // the call that ends the pass finishes the BLAKE3 streams: pending chunk values and the last chunks come to the host (<= 1 KiB + 32 B x 2^k per instance)
    if (rc == GSV_OK && want(PassCommit::B3) && end_of_pass)
      rc = b3_finish(*s_->b3, s_->e->stream.get(), sink_.b3, obf ? std::function<int(const uint8_t*, uint32_t)>([obf](const uint8_t* vals, uint32_t pend) {
        return !pend || obf->append(vals, pend, 0, 1) ? GSV_OK : obf->to_callback() ? fail_drain(DrainError::OutboardSink) : fail(GSV_ERR_INVALID, "short write to an outboard file");
      }) : nullptr, sink_.last_chunks);
    if (rc == GSV_OK && obf && !obf->flush()) rc = fail(GSV_ERR_INVALID, "short write to an outboard file");
    if (rc != GSV_OK) return rc;
    if (want(PassCommit::Mac)) for (size_t i = 0; i < n_inst_; ++i) s_->drain->macs[i].digest(sink_.hashes + 16 * i);
    // the commitments a checked pass returns are the ones its checkpoint files claim — proven once the last slice has passed
    if (want(PassCommit::MacCheck) && sink_.mac_check_hashes && end_of_pass) std::memcpy(sink_.mac_check_hashes, claimed_.data(), claimed_.size());
    outboards_.keep(); checkpoints_.keep();
    return GSV_OK;
  }
 private:
  bool want(PassCommit c) const { return has(flags_, c); }
  OutboardWriter* outboards() { return sink_.outboard() ? &outboards_ : nullptr; }
  gsv_session* const s_; const DrainSink& sink_; const PassCommit flags_;
  bool new_pass_ = true; size_t n_inst_ = 0; uint64_t seg_records_ = 0;
  uint32_t groups_ = 0;                  // group values per instance of the segment fed last, not yet submitted
  CheckpointWriter checkpoints_;         // written by the MAC workers
  std::vector<MacCheckpointFile> mcks_;  // the check: the files, the commitments they claim, the receiver that reads their states
  std::vector<uint8_t> claimed_;
  MacCheckReceiver mac_rx_;
  OutboardWriter outboards_;             // written by the absorbers' threads, and by the caller's when the pass ends
  std::optional<B3Absorbers> absorbers_;  // last: see above
};
