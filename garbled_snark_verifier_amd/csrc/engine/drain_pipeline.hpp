// The host side of the streaming drain (engine_drain.ipp): the session's copy streams, pinned chunk buffers and MAC states; where a drained stream goes, what that
// makes a pass carry (PassCommit) and which combinations are refused (DrainSink::refusal, commit_slice_conflict: the policy, as plain values); the gc_<i>.bin files of
// a pass and its outboards (gc_<i>.b3o files, or a host callback); the pool of MAC / copy workers behind a queue of segments; the BLAKE3 absorbers; the CBC-MAC
// checkpoint files (gc_<i>.mck: the chain states the MAC workers pass through anyway, kept).
// Each pool owns its threads and joins them in its destructor.  Nothing here knows sessions, schedules, plans or knobs — plain values
// in — and nothing but the HIP runtime API, hip_owned.hpp, host_crypto.hpp and the standard library is needed: this header compiles
// alone (tests/drain_pipeline runs it against stand-ins for the HIP calls, also under the thread and address sanitizers).
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "hip_owned.hpp"
#include "host_crypto.hpp"
#include "mac_checkpoints.hpp"
#include "outboard.hpp"

namespace gsv {
// The drain machinery (copy streams, pinned chunk buffers, the per-instance MAC states) lives in the session, so that a plan can
// be garbled in SLICES of consecutive calls (gsv_session_garble_streaming_calls): the MACs chain from slice to slice and the
// page-locked buffers are set up once.
struct gsv_drain {
  // Many host threads are wanted for the MACs (one serial chain per instance) but only a few D2H copies should be in
  // flight at once: measured on the MI355X box, 128 concurrent copy streams move 9 GB/s where a handful move 22 GB/s
  // (and the number of STREAMS matters as much as the number of copies: the copies share a small pool of streams).
  struct CopyGate {
    std::mutex mu; std::condition_variable cv; std::vector<hipStream_t> idle;
    hipStream_t acquire() { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return !idle.empty(); }); hipStream_t st = idle.back(); idle.pop_back(); return st; }
    void release(hipStream_t st) { { std::lock_guard<std::mutex> lk(mu); idle.push_back(st); } cv.notify_one(); }
  } copy_gate;
  std::vector<Stream> copy_streams;  // (copy_gate hands them out)
  // Instances whose MAC chains one worker advances side by side: four (AES-NI, CbcMacHost::update_interleaved) or, on hosts with
  // VAES + AVX-512 and sessions with at least 128 instances (eight workers' worth), sixteen (update_interleaved16_vaes: one core
  // then MACs ~3 x as many blocks per second, so a node's GPUs need a third of the host cores for their commitments).
  static constexpr int GROUP_MAX = 16;
  // CPUs this process may actually use: the visible ones, capped by the container's CPU bandwidth quota (cgroup cpu.max)
  static size_t usable_cores() {
    size_t n = std::max<size_t>(1, std::thread::hardware_concurrency());
    if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
      char q[64] = {0}; double per = 0;
      if (std::fscanf(f, "%63s %lf", q, &per) == 2 && std::strcmp(q, "max") != 0 && per > 0) n = std::min<size_t>(n, std::max<size_t>(1, size_t(std::atof(q) / per)));
      std::fclose(f);
    }
    return n;
  }
  // One chain per worker while there is a core per instance: a chain alone advances at ~1.1e8 blocks/s, one of four interleaved at
  // ~0.75e8 — sixteen instances (BASELINE config 5 on one GPU) hashed four to a worker took 40 s for 34.8 s of garbling, their
  // sixteen chains one per core take 27 s.  More instances than cores: four (AES-NI) or sixteen (VAES, >= 128 instances) per worker.
  static int group_for(size_t n_inst, int forced) {  // forced: GSV_DRAIN_GROUP, 0 = not set
    if (forced) return forced;
    if (n_inst <= usable_cores()) return 1;
    return CbcMacHost::have_vaes() && n_inst >= 128 ? 16 : 4;
  }
  int group = 4;
  struct Worker {
    MappedHost<uint8_t> pinned[2][GROUP_MAX];  // two sets of pinned chunk buffers: copy set j+1 while set j is hashed
    Event done;                   // blocking-sync event: a worker waiting for its copies sleeps instead of spinning on a core
  };
  std::vector<Worker> workers;
  uint64_t chunk = 0;  // records per chunk buffer
  std::vector<CbcMacHost> macs;
};

// What a garbling pass carries from slice to slice, as a set: gsv_session::pass_commit holds the first slice's.  (An outboard, to files
// or to a callback, is part of what a BLAKE3 pass carries.)
enum class PassCommit : uint8_t { None = 0, Mac = 1, B3 = 2, Outboard = 4, MacCheck = 8, Checkpoints = 16 };
constexpr PassCommit operator|(PassCommit a, PassCommit b) { return PassCommit(uint8_t(a) | uint8_t(b)); }
constexpr bool has(PassCommit set, PassCommit any_of) { return (uint8_t(set) & uint8_t(any_of)) != 0; }
// A pass that commits with BLAKE3 carries the same commitments in every slice: a slice without MAC workers leaves the MAC states
// behind, one without the hash kernels the BLAKE3 state (likewise the checkpoint files and the check).  Null: `now` may follow `first`.
inline const char* commit_slice_conflict(PassCommit first, PassCommit now) {
  if (first == now) return nullptr;
  if (has(first | now, PassCommit::B3)) return "every slice of a pass with a BLAKE3 commitment must ask for the same commitments as its first slice";
  if (has(first | now, PassCommit::MacCheck | PassCommit::Checkpoints)) return "every slice of a pass that writes or checks CBC-MAC checkpoints must ask for the same as its first slice";
  return nullptr;
}
// What a streaming EVALUATION asks for, as a set: every slice of a pass asks for the same (EvalCarry::commit holds the first slice's).
// At most one kind of verification: BLAKE3 outboards from files; outboards in memory, authenticated up front with the last chunks, or
// at the end of the pass; CBC-MAC checkpoints from files, or in memory (engine_cbcmac.ipp).  A checkpoint pass computes no commitment
// beside the one it proves: no MAC worker starts and no BLAKE3 digest is taken.
enum class EvalCommit : uint8_t { None = 0, Mac = 1, B3 = 2, VerifiedFiles = 4, VerifiedUpFront = 8, VerifiedDeferred = 16, CheckpointFiles = 32, CheckpointMemory = 64 };
constexpr EvalCommit operator|(EvalCommit a, EvalCommit b) { return EvalCommit(uint8_t(a) | uint8_t(b)); }
constexpr bool has(EvalCommit set, EvalCommit any_of) { return (uint8_t(set) & uint8_t(any_of)) != 0; }
// The first rule the set `now` breaks behind a pass whose slice at call 0 asked for `first` (first_slice: `now` is that slice), or null
inline const char* eval_commit_refusal(EvalCommit first, EvalCommit now, bool first_slice) {
  const EvalCommit checkpoints = EvalCommit::CheckpointFiles | EvalCommit::CheckpointMemory;
  if (has(now, checkpoints) && (now != EvalCommit::CheckpointFiles && now != EvalCommit::CheckpointMemory))
    return "a streaming evaluation verified against CBC-MAC checkpoints computes no other commitment and takes no other kind of verification";
  if (!first_slice && first != now) return "every slice of a streaming evaluation must ask for the same commitments and the same kind of verification as its first slice";
  return nullptr;
}
// Where a drained stream goes (any combination): the per-instance CBC-MAC (AESAccumulatingHash), gc_<index>.bin files, a host callback,
// the per-instance BLAKE3 tree hash on the device (engine_blake3.ipp) — the one destination for which no ciphertext leaves the device.
using DrainSinkFn = int (*)(void* user, size_t instance, uint64_t first_record, const uint8_t* records, uint64_t n_records);  // (gsv_ct_sink_fn of include/gsv_engine.h)
using OutboardSinkFn = int (*)(void* user, size_t instance, uint64_t byte_offset, const uint8_t* bytes, uint64_t n_bytes);  // (gsv_outboard_sink_fn)
struct DrainSink {
  uint8_t* hashes = nullptr;           // n_inst x 16: the MAC states after this call
  const char* dir = nullptr;           // gc_<index>.bin, index = indexes ? indexes[i] : first_index + i
  uint64_t first_index = 0;
  DrainSinkFn fn = nullptr;            // CiphertextHandler::handle over a run of records of one instance
  void* user = nullptr;
  uint8_t* b3 = nullptr;               // n_inst x 32: the BLAKE3 digests, written by the call that ends the pass
  const char* outboard_dir = nullptr;  // gc_<index>.b3o: the values the BLAKE3 absorbers receive, kept (needs b3)
  OutboardSinkFn ob_fn = nullptr;      // ... or handed to the host as they are produced (needs b3)
  void* ob_user = nullptr;
  uint8_t* last_chunks = nullptr;      // n_inst x 1024: the streams' last chunks, zero-padded, written with b3 (needs b3)
  const char* checkpoint_dir = nullptr;  // gc_<index>.mck: the MAC states after every 2^k records, kept (needs hashes)
  // the CBC-MAC check on the device (engine_cbcmac.ipp): the streams are verified against the checkpoint files gc_<index>.mck of
  // mac_check_dir, index = mac_check_indexes ? mac_check_indexes[i] : first_index + i; nothing leaves the device and no MAC worker starts
  const char* mac_check_dir = nullptr;
  const uint64_t* mac_check_indexes = nullptr;
  const uint8_t* mac_check_expected = nullptr;  // n_inst x 16 or null: the commitments the caller trusts
  uint8_t* mac_check_hashes = nullptr;          // n_inst x 16 or null: the verified commitments, written by the call that ends the pass
  bool outboard() const { return outboard_dir || ob_fn; }
  bool host() const { return hashes || dir || fn; }  // the stream is copied to the host
  bool any() const { return host() || b3 || mac_check_dir; }
  PassCommit commit() const {
    const auto on = [](bool q, PassCommit c) { return q ? c : PassCommit::None; };
    return on(hashes, PassCommit::Mac) | on(b3, PassCommit::B3) | on(outboard(), PassCommit::Outboard) | on(mac_check_dir, PassCommit::MacCheck) | on(checkpoint_dir, PassCommit::Checkpoints);
  }
  // The first rule this combination breaks, or null.  b3_refusal: the two an entry point can tell from its own arguments.
  const char* b3_refusal() const {
    if (outboard() && !b3) return "an outboard holds the values of the BLAKE3 commitment: blake3_digests must be given";
    if (last_chunks && !b3) return "the last chunks come with the BLAKE3 commitment: blake3_digests must be given";
    return nullptr;
  }
  // ring: the session's device block is a ciphertext ring; paired: an evaluator session consumes the windows (garble || evaluate)
  const char* refusal(bool ring, bool paired) const {
    if (const char* why = b3_refusal()) return why;
    if (checkpoint_dir && !hashes) return "checkpoint files hold the states of the CBC-MAC: hashes must be given";  // (no entry point of the C ABI gets here: the one that takes a checkpoint directory answers "null hash buffer" first)
    if ((mac_check_dir || checkpoint_dir) && ring) return "CBC-MAC checkpoints are not written or checked over a ciphertext ring (retain_stream = GSV_STREAM_RING): create the session with launch windows";
    if (mac_check_dir && (host() || b3 || paired)) return "internal: the CBC-MAC check runs alone";
    return nullptr;
  }
};

// The files one call writes, one per instance.  Closed when the object goes away and REMOVED unless keep() was called: a failed pass
// must not leave a plausible-looking prefix of a ciphertext file (or of its outboard, or of its checkpoints) behind, whichever way it returns.
class KeptFiles {
 public:
  KeptFiles() = default;
  KeptFiles(const KeptFiles&) = delete;
  KeptFiles& operator=(const KeptFiles&) = delete;
  ~KeptFiles() {
    for (FILE* f : files_) std::fclose(f);
    if (!keep_) for (const std::string& q : paths_) std::remove(q.c_str());
  }
  bool flush() { bool ok = true; for (FILE* f : files_) ok = std::fflush(f) == 0 && ok; return ok; }
  void keep() { keep_ = true; }
 protected:
  bool add(const std::string& path, const char* mode, const uint8_t* header, size_t header_bytes, std::string* failed) {
    FILE* f = std::fopen(path.c_str(), mode);
    if (f) { files_.push_back(f); paths_.push_back(path); }
    if (f && (!header || std::fwrite(header, 1, header_bytes, f) == header_bytes)) return true;
    *failed = path;  // the path that could not be created, or its header not written
    return false;
  }
  std::vector<FILE*> files_;
 private:
  std::vector<std::string> paths_;
  bool keep_ = false;
};
class GcFiles : public KeptFiles {  // the gc_<first_index + i>.bin files of one call
 public:
  // mode "wb" (a new pass) or "ab" (a later slice).  False: `*failed` is the path that could not be created.
  bool open(const char* dir, uint64_t first_index, size_t n_inst, const char* mode, std::string* failed) {
    for (size_t i = 0; i < n_inst; ++i) if (!add(std::string(dir) + "/gc_" + std::to_string(first_index + i) + ".bin", mode, nullptr, 0, failed)) return false;
    return true;
  }
  FILE* operator[](size_t i) const { return files_[i]; }
};

// The outboards of one call (outboard.hpp): a header, then the 32-byte values in the order the host absorbs them.  One writer, two
// back ends.  FILES: gc_<first_index + i>.b3o — a new pass writes the header, a later slice appends; closed when the object goes away
// and REMOVED unless keep() was called, like the gc files beside them.  CALLBACK (gsv_outboard_sink_fn of include/gsv_engine.h): the
// same bytes handed to the host as they are produced, per instance at increasing byte offsets — the header at offset 0 by the slice
// that starts a pass, a later slice goes on behind the values the earlier ones delivered; once a call has returned non-zero no
// further call is started.  Instances may be written from different threads, one instance from one thread at a time.
class OutboardWriter : public KeptFiles {
 public:
  static std::string path(const char* dir, uint64_t index) { return std::string(dir) + "/gc_" + std::to_string(index) + ".b3o"; }
  // new_pass: truncate and write the header for a stream of n_records records in groups of 2^k chunks; else append.  False: `*failed`.
  bool open(const char* dir, uint64_t first_index, size_t n_inst, bool new_pass, uint32_t k, uint64_t n_records, std::string* failed) {
    uint8_t header[Outboard::HEADER_BYTES];
    Outboard::put_header(header, k, n_records);
    n_ = n_inst;
    for (size_t i = 0; i < n_inst; ++i) if (!add(path(dir, first_index + i), new_pass ? "wb" : "ab", new_pass ? header : nullptr, sizeof header, failed)) return false;
    return true;
  }
  // The callback back end.  new_pass: every instance receives the header at offset 0, here, on the calling thread; else the slice goes
  // on behind the `values_before` values per instance that the pass's earlier slices delivered.  False: the callback refused a header.
  bool open(OutboardSinkFn fn, void* user, size_t n_inst, bool new_pass, uint32_t k, uint64_t n_records, uint64_t values_before) {
    fn_ = fn; user_ = user; n_ = n_inst;
    offset_.assign(n_inst, new_pass ? 0 : Outboard::HEADER_BYTES + 32 * values_before);
    if (!new_pass) return true;
    uint8_t header[Outboard::HEADER_BYTES];
    Outboard::put_header(header, k, n_records);
    for (size_t i = 0; i < n_inst; ++i) if (!deliver(i, header, sizeof header)) return false;
    return true;
  }
  size_t size() const { return n_; }
  bool to_callback() const { return fn_ != nullptr; }
  bool callback_failed() const { return refused_.load(); }
  // `count` values per instance ([instance][value], dense, for all instances) go to instances i0, i0 + step, ...
  bool append(const uint8_t* vals, uint32_t count, size_t i0, size_t step) {
    bool ok = true;
    for (size_t i = i0; i < n_; i += step) {
      const uint8_t* const v = vals + i * size_t(count) * 32;
      if (fn_) { if (count) ok = deliver(i, v, uint64_t(count) * 32) && ok; }
      else ok = std::fwrite(v, 32, count, files_[i]) == count && ok;
    }
    return ok;
  }
 private:
  bool deliver(size_t i, const uint8_t* bytes, uint64_t n) {
    if (refused_.load()) return false;
    if (fn_(user_, i, offset_[i], bytes, n) != 0) { refused_.store(true); return false; }
    offset_[i] += n;
    return true;
  }
  OutboardSinkFn fn_ = nullptr;
  void* user_ = nullptr;
  std::vector<uint64_t> offset_;     // callback: the next byte of every instance's outboard
  std::atomic<bool> refused_{false};
  size_t n_ = 0;
};
using OutboardFiles = OutboardWriter;  // (the name from before the callback back end)

// The CBC-MAC checkpoint files of one call (mac_checkpoints.hpp): gc_<first_index + i>.mck — a header, then the chain state after every
// 2^k records and at the end of the stream, in stream order.  A new pass writes the header, a later slice appends; closed when the
// object goes away and REMOVED unless keep() was called, like the gc files beside them.  The MAC workers write them: instances may be
// written from different threads, one instance from one thread at a time.
class CheckpointWriter : public KeptFiles {
 public:
  static std::string path(const char* dir, uint64_t index) { return std::string(dir) + "/gc_" + std::to_string(index) + ".mck"; }
  // new_pass: truncate and write the header for a stream of n_records records in groups of 2^k records; else append.  False: `*failed`.
  bool open(const char* dir, uint64_t first_index, size_t n_inst, bool new_pass, uint32_t k, uint64_t n_records, std::string* failed) {
    uint8_t header[MacCheckpoints::HEADER_BYTES];
    MacCheckpoints::put_header(header, k, n_records);
    k_ = k; total_ = n_records;
    for (size_t i = 0; i < n_inst; ++i) if (!add(path(dir, first_index + i), new_pass ? "wb" : "ab", new_pass ? header : nullptr, sizeof header, failed)) return false;
    return true;
  }
  bool on() const { return !files_.empty(); }
  // records a chain at stream position `pos` may advance before its state has to be kept: up to the next multiple of 2^k, at least 1
  uint64_t run(uint64_t pos, uint64_t most) const { return std::min<uint64_t>(most, (1ull << k_) - (pos & ((1ull << k_) - 1))); }
  // is the state of a chain that has absorbed `pos` records a checkpoint?  (a multiple of 2^k, or the end of the stream)
  bool due(uint64_t pos) const { return pos && ((pos & ((1ull << k_) - 1)) == 0 || pos == total_); }
  bool append(size_t i, const CbcMacHost& mac) {
    uint8_t st[16];
    mac.digest(st);
    return std::fwrite(st, 1, 16, files_[i]) == 16;
  }
 private:
  uint32_t k_ = 0;
  uint64_t total_ = 0;
};

// What went wrong on the host side of a drain.  The pools of one pass share one slot, the first error stays: a worker that sees one
// set stops copying and hashing.
enum class DrainError { None, Copy, FileWrite, Sink, B3Order, OutboardSink };
inline void drain_set_error(std::atomic<DrainError>& slot, DrainError e) { DrainError none = DrainError::None; slot.compare_exchange_strong(none, e); }

inline double drain_secs(std::chrono::steady_clock::time_point a) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - a).count(); }
// GSV_DRAIN_STATS=1: where the host thread of the pipeline waits (for a free gate-order buffer = the host side is the slower stage;
// for the kernel + gather = the device is), printed once per call
struct DrainStats {
  double t_wait_drain = 0, t_wait_device = 0, t_gather = 0;
  uint64_t drained_records = 0;  // per instance
  std::chrono::steady_clock::time_point t_begin = std::chrono::steady_clock::now();
  void print(size_t n_inst, size_t n_workers, size_t group, size_t depth) const {
    const double tot = drain_secs(t_begin);
    std::fprintf(stderr, "drain: %.2f s for %zu instances x %llu records (%.1f GB/s), %zu MAC workers x %zu chains, %zu gate-order buffers; host thread waited %.2f s for drains, %.2f s for the device and %.2f s for the gathers of running windows\n", tot, n_inst,
                 (unsigned long long)drained_records, double(drained_records) * double(n_inst) * 16e-9 / tot, n_workers, group, depth, t_wait_drain, t_wait_device, t_gather);
  }
};

// The drain is a PIPELINE of segments: the device side (garble a window, bring it into gate order in one of `depth` gate-order
// buffers) runs ahead of the host side (copy out, CBC-MAC, files, sink) by up to `depth` segments.  A window's ciphertext count is
// fixed but its garbling time is not (the ladders and inversions produce a gigabyte of ciphertexts in seconds, the Miller loop in
// half a second), while the serial CBC-MAC chain takes the same 0.58 s for every gigabyte: with ONE buffer a pass costs
// sum(max(garble_w, mac_w)) — 37.0 s for one instance whose garbling takes 31 s and whose chain takes 27 s — with a few buffers
// max(sum garble, sum mac).  Workers are persistent for the call and take the segments strictly in order (an instance's chain must
// see its stream in order); a buffer is reused once every worker is done with the segment that held it.
struct DrainShape {
  int device = 0;                  // the workers select it before their first copy
  size_t n_inst = 0, group = 1;    // instances whose streams leave the device; chains a worker advances side by side
  size_t n_workers = 0;            // 0: nothing is copied to the host (no threads, wait_buffer / push only count)
  uint64_t chunk = 0;              // records per pinned chunk buffer (gsv_drain::chunk)
  uint64_t seg_records = 0;        // records between two instances in a gate-order buffer
  std::vector<void*> gate_bufs;    // the gate-order buffers (device memory), used round robin
  bool blocking_wait = false;      // workers sleep on their blocking-sync event instead of spinning on the copy stream
};
class DrainWorkers {
 public:
  // `d` (n_workers > 0: its workers, chunk buffers and copy streams), `macs` and `files` must outlive this object
  // `checkpoints` (optional; needs sink.hashes): the MAC states after every 2^k records go there as the workers pass through them
  DrainWorkers(gsv_drain* d, const DrainShape& shape, const DrainSink& sink, std::vector<CbcMacHost>& macs, const GcFiles& files, std::atomic<DrainError>& err, CheckpointWriter* checkpoints = nullptr)
      : d_(d), c_(shape), sink_(sink), macs_(macs), files_(files), err_(err), ckw_(checkpoints && checkpoints->on() ? checkpoints : nullptr), depth_(std::max<size_t>(1, shape.gate_bufs.size())), n_groups_((shape.n_inst + shape.group - 1) / shape.group) {
    for (size_t t = 0; t < c_.n_workers; ++t) threads_.emplace_back([this, t] { work(t); });
  }
  ~DrainWorkers() { finish(); }
  size_t depth() const { return depth_; }
  size_t next_buffer() const { return n_pushed_ % depth_; }  // index of the gate-order buffer the next segment goes to
  // blocks until the segment that last used that buffer has been consumed by every worker; returns the seconds waited
  double wait_buffer() {
    if (threads_.empty() || n_pushed_ < depth_) return 0;
    const auto t0 = std::chrono::steady_clock::now();
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return seg_done_[n_pushed_ - depth_] == c_.n_workers; });
    return drain_secs(t0);
  }
  // the next segment: `n` records per instance in buffer next_buffer(), the first of them record `base` of the stream
  void push(uint64_t n, uint64_t base) {
    if (!threads_.empty()) {
      { std::lock_guard<std::mutex> lk(mu_); segments_.push_back(Segment{n, base, next_buffer()}); seg_done_.push_back(0); }
      cv_.notify_all();
    }
    ++n_pushed_;
  }
  void finish() {  // every pushed segment consumed (or skipped, after an error), workers gone
    { std::lock_guard<std::mutex> lk(mu_); closed_ = true; }
    cv_.notify_all();
    for (std::thread& th : threads_) th.join();
    threads_.clear();
  }
  DrainError error() const { return err_.load(); }
 private:
  struct Segment { uint64_t n, base; size_t buf; };
  void work(size_t t) {
    const size_t T = c_.n_workers, GROUP = c_.group;
    const uint64_t chunk = c_.chunk;
    if (hipSetDevice(c_.device) != hipSuccess) drain_set_error(err_, DrainError::Copy);
    gsv_drain& dr = *d_;
    gsv_drain::Worker& w = dr.workers[t];
    for (size_t j = 0;; ++j) {
      Segment sg;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return j < segments_.size() || closed_; });
        if (j >= segments_.size()) return;
        sg = segments_[j];
      }
      const uint64_t n = sg.n, base = sg.base;
      const uint8_t* const gate = static_cast<const uint8_t*>(c_.gate_bufs[sg.buf]);
      // (after an error the loop below does nothing, but the worker still walks every remaining segment and counts it done: that is
      // what keeps wait_buffer, which waits for ALL workers to be done with a segment, from blocking forever)
      for (size_t grp = t; grp < n_groups_ && err_.load() == DrainError::None && n; grp += T) {
        const size_t i0 = grp * GROUP, ng = std::min(GROUP, c_.n_inst - i0);  // instances i0 .. i0+ng-1 advance together
        // the copies of one chunk set share a stream of the pool (a set holds a slot of the gate from issue to completion)
        auto copy = [&](uint64_t off, int b) {
          hipStream_t st = dr.copy_gate.acquire();
          bool ok = true;
          for (size_t g = 0; g < ng && ok; ++g)
            ok = hipMemcpyAsync(w.pinned[b][g].get(), gate + ((i0 + g) * c_.seg_records + off) * 16, std::min(chunk, n - off) * 16, hipMemcpyDeviceToHost, st) == hipSuccess;
          // many workers: sleep on the blocking-sync event (spinning workers eat the cores the MACs need); a handful of
          // workers (one instance: the whole-stream check) spin instead, a blocking wait's wake-up latency would be paid per chunk
          ok = ok && (c_.blocking_wait ? hipEventRecord(w.done.get(), st) == hipSuccess && hipEventSynchronize(w.done.get()) == hipSuccess : hipStreamSynchronize(st) == hipSuccess);
          dr.copy_gate.release(st);
          return ok;
        };
        int b = 0;
        if (!copy(0, 0)) { drain_set_error(err_, DrainError::Copy); break; }
        for (uint64_t off = 0; off < n; off += chunk, b ^= 1) {
          const uint64_t m = std::min(chunk, n - off);
          if (sink_.hashes) {
            CbcMacHost* mp[gsv_drain::GROUP_MAX];
            const uint8_t* cp[gsv_drain::GROUP_MAX];
            for (size_t g = 0; g < ng; ++g) { mp[g] = &macs_[i0 + g]; cp[g] = w.pinned[b][g].get(); }
            if (!ckw_) CbcMacHost::update_many(mp, cp, ng, m);  // sixteen / four chains per step, a ragged last group chain by chain
            else {
              // checkpoints: the call is split at the multiples of 2^k of the stream position base + off — all chains of the group are
              // at the same position, so the split is common to them — and the states behind each split are kept
              for (uint64_t q = 0; q < m;) {
                const uint64_t step = ckw_->run(base + off + q, m - q);
                const uint8_t* cq[gsv_drain::GROUP_MAX];
                for (size_t g = 0; g < ng; ++g) cq[g] = cp[g] + q * 16;
                CbcMacHost::update_many(mp, cq, ng, step);
                q += step;
                if (ckw_->due(base + off + q))
                  for (size_t g = 0; g < ng; ++g) if (!ckw_->append(i0 + g, macs_[i0 + g])) { drain_set_error(err_, DrainError::FileWrite); break; }
              }
            }
          }
          if (sink_.dir)
            for (size_t g = 0; g < ng; ++g)
              if (std::fwrite(w.pinned[b][g].get(), 16, m, files_[i0 + g]) != m) { drain_set_error(err_, DrainError::FileWrite); break; }
          if (sink_.fn && err_.load() == DrainError::None)
            for (size_t g = 0; g < ng; ++g)
              if (sink_.fn(sink_.user, i0 + g, base + off, w.pinned[b][g].get(), m) != 0) { drain_set_error(err_, DrainError::Sink); break; }
          if (err_.load() != DrainError::None) break;
          if (off + chunk < n && !copy(off + chunk, b ^ 1)) { drain_set_error(err_, DrainError::Copy); break; }
        }
      }
      { std::lock_guard<std::mutex> lk(mu_); seg_done_[j]++; }
      cv_.notify_all();
    }
  }
  gsv_drain* const d_;
  const DrainShape c_;
  const DrainSink sink_;
  std::vector<CbcMacHost>& macs_;
  const GcFiles& files_;
  std::atomic<DrainError>& err_;
  CheckpointWriter* const ckw_;
  const size_t depth_, n_groups_;
  size_t n_pushed_ = 0;                   // (the pushing thread's alone)
  std::mutex mu_;
  std::condition_variable cv_;
  std::vector<Segment> segments_;         // pushed by the device side, in stream order
  std::vector<size_t> seg_done_;          // per segment: workers that have finished it
  bool closed_ = false;
  std::vector<std::thread> threads_;      // last: everything above exists when the first worker starts
};

// BLAKE3: the group values of a segment (32 bytes per 2^k chunks and instance) are folded into the instances' hashers by a small pool
// of their own, in segment order, off the thread that launches the windows; a task is released when every thread of the pool is done with it.
// What the launching thread itself does per segment is copy those values out of the page-locked buffer (submit: 32 B x groups x
// instances, a few KiB), which has to happen before the next segment's copy lands there.
class B3Absorbers {
 public:
  // thread t of n_threads folds the values of ITS instances (t, t + n_threads, ...); false: values out of order
  using Absorb = std::function<bool(const uint8_t* vals, uint32_t groups, size_t t, size_t n_threads)>;
  B3Absorbers(size_t n_threads, Absorb absorb, std::atomic<DrainError>& err) : n_(n_threads), absorb_(std::move(absorb)), err_(err) {
    for (size_t t = 0; t < n_; ++t) threads_.emplace_back([this, t] { work(t); });
  }
  ~B3Absorbers() { finish(); }
  // after the stream the segment's hash kernels ran on has been synchronised: its group values leave the page-locked buffer
  void submit(const uint8_t* pinned, size_t bytes, uint32_t groups) {
    if (!groups) return;
    std::unique_ptr<Task> task(new Task());
    task->groups = groups;
    task->vals.assign(pinned, pinned + bytes);
    { std::lock_guard<std::mutex> lk(mu_); tasks_.push_back(std::move(task)); }
    cv_.notify_all();
  }
  void finish() {  // every submitted task absorbed, threads gone
    { std::lock_guard<std::mutex> lk(mu_); closed_ = true; }
    cv_.notify_all();
    for (std::thread& th : threads_) th.join();
    threads_.clear();
  }
  DrainError error() const { return err_.load(); }
 private:
  struct Task { std::vector<uint8_t> vals; uint32_t groups = 0; size_t done = 0; };
  void work(size_t t) {
    for (size_t j = 0;; ++j) {
      Task* task;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return j < tasks_.size() || closed_; });
        if (j >= tasks_.size()) return;
        task = tasks_[j].get();
      }
      if (!absorb_(task->vals.data(), task->groups, t, n_)) drain_set_error(err_, DrainError::B3Order);
      std::lock_guard<std::mutex> lk(mu_);
      if (++task->done == n_) tasks_[j].reset();
    }
  }
  const size_t n_;
  const Absorb absorb_;
  std::atomic<DrainError>& err_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::vector<std::unique_ptr<Task>> tasks_;
  bool closed_ = false;
  std::vector<std::thread> threads_;  // last, as in DrainWorkers
};
}  // namespace gsv
