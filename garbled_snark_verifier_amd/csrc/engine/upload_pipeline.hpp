// The host side of the streaming evaluator (engine_evaluate.ipp): the page-locked staging buffers a ciphertext source is read into, the H2D
// copies out of them, the pool of workers that folds each instance's chunks into its CBC-MAC beside the copies, and the file source.  As in
// drain_pipeline.hpp nothing here knows sessions, schedules, plans or knobs — plain values in — and nothing but the HIP runtime API,
// hip_owned.hpp, host_crypto.hpp and the standard library is needed: this header compiles alone (tests/upload_pipeline runs it against
// stand-ins for the HIP calls, also under the thread and address sanitizers).
#pragma once
#include <hip/hip_runtime_api.h>
#include <sys/types.h>

#include <algorithm>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <deque>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "hip_owned.hpp"
#include "host_crypto.hpp"

namespace gsv {
// The CBC-MAC of one instance is a serial chain, the chains of different instances are independent: one queue per worker, instance i's
// chunks go to worker i mod T and are folded there in the order they were pushed.  A chunk is read where it was staged: the buffer it
// sits in stays busy until its MAC is done (wait_free).
class MacPool {
 public:
  // `macs` must outlive this object; T workers (0: none, push must not be called) over NB staging buffers
  MacPool(std::vector<CbcMacHost>& macs, size_t T, size_t NB) : macs_(macs), q_(T), busy_(NB, 0) {
    for (size_t t = 0; t < T; ++t) threads_.emplace_back([this, t] { work(t); });
  }
  ~MacPool() { finish(); }
  void push(size_t inst, const uint8_t* p, uint64_t n, size_t buf) {
    { std::lock_guard<std::mutex> lk(mu_); busy_[buf] = 1; q_[inst % q_.size()].push_back(Job{inst, p, n, buf}); }
    cv_job_.notify_all();
  }
  void wait_free(size_t buf) { std::unique_lock<std::mutex> lk(mu_); cv_free_.wait(lk, [&] { return !busy_[buf]; }); }
  void finish() {  // every queued chunk folded, workers gone
    { std::lock_guard<std::mutex> lk(mu_); closed_ = true; }
    cv_job_.notify_all();
    for (std::thread& t : threads_) t.join();
    threads_.clear();
  }
 private:
  struct Job { size_t inst; const uint8_t* p; uint64_t n; size_t buf; };
  void work(size_t t) {
    for (;;) {
      Job j;
      { std::unique_lock<std::mutex> lk(mu_); cv_job_.wait(lk, [&] { return closed_ || !q_[t].empty(); }); if (q_[t].empty()) return; j = q_[t].front(); q_[t].pop_front(); }
      macs_[j.inst].update(j.p, j.n);
      { std::lock_guard<std::mutex> lk(mu_); busy_[j.buf] = 0; }
      cv_free_.notify_all();
    }
  }
  std::vector<CbcMacHost>& macs_;
  std::vector<std::deque<Job>> q_;
  std::vector<char> busy_;  // per staging buffer: a MAC job still reads it
  std::mutex mu_;
  std::condition_variable cv_job_, cv_free_;
  bool closed_ = false;
  std::vector<std::thread> threads_;  // last, as in DrainWorkers
};

enum class UploadError { None, EventWait, Copy, Dry, Order };  // Copy: the copy or the record of its event; Dry: the source ran out (dry_instance / dry_record); Order: `base` is not where the stream stands

// The records of a CiphertextSource on their way to a gate-order device buffer, in bounded page-locked chunks.  With T > 0 the chunks are
// read CHUNK-major (every instance's chunk at one offset, then the next offset) and instance i's chunks are folded in order by worker
// i mod T, beside the uploads; a staging buffer is reused once its copy AND its MAC are done.
class CtUploader {
 public:
  // read(instance, first_record, dst, n) -> 0, or non-zero when the source runs dry.  T: MAC workers (0: no MACs are computed).
  using Read = std::function<int(size_t, uint64_t, uint8_t*, uint64_t)>;
  CtUploader(size_t n_inst, uint64_t seg_records, uint64_t chunk, size_t T, Read read)
      : n_inst_(n_inst), seg_records_(seg_records), chunk_(chunk), T_(T), read_(std::move(read)), stage_(2 + 2 * T), stage_ev_(2 + 2 * T), macs_(n_inst), pool_(macs_, T, 2 + 2 * T) {}
  // Workers joined, then every copy out of a staging buffer finished (an error return may leave some queued on a side stream), and only
  // then the buffers released.  (An event that was never recorded counts as finished.)
  ~CtUploader() {
    pool_.finish();
    for (const Event& e : stage_ev_) if (e) (void)hipEventSynchronize(e.get());
  }
  hipError_t alloc() {  // the staging buffers and, per buffer, the event of the copy that last used it
    for (size_t k = 0; k < stage_.size(); ++k) {
      hipError_t e = stage_[k].alloc(size_t(chunk_) * 16, hipHostMallocDefault);
      if (e == hipSuccess) e = stage_ev_[k].create(hipEventDisableTiming);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }
  // A stream that goes on behind records read earlier (a later slice of a pass): the record the first upload() starts at and, with MAC
  // workers, the per-instance states to go on from (empty: h = 0).  Before the first upload(); without it the stream starts at record 0.
  void start_at(uint64_t first_record, const std::vector<CbcMacHost>& macs = std::vector<CbcMacHost>()) {
    next_ = first_record;
    if (macs.size() == n_inst_) macs_ = macs;
  }
  uint64_t next_record() const { return next_; }  // the stream index behind the last upload() that succeeded
  // `n` records per instance starting at stream index `base` -> the gate-order buffer `gate` (seg_records apart) through `st`, hashed as read.
  // The uploads of one uploader follow each other in the stream (the MAC chains are serial): any other `base` is UploadError::Order.
  UploadError upload(uint64_t base, uint64_t n, void* gate, hipStream_t st) {
    if (base != next_) return UploadError::Order;
    const size_t NB = stage_.size();
    for (uint64_t off = 0; off < n; off += chunk_)
      for (size_t i = 0; i < n_inst_; ++i, b_ = (b_ + 1) % NB) {
        const uint64_t m = std::min(chunk_, n - off);
        if (hipEventSynchronize(stage_ev_[b_].get()) != hipSuccess) return UploadError::EventWait;  // the copy that last used this staging buffer has finished
        if (T_) pool_.wait_free(b_);  // ... and so has its MAC
        uint8_t* host = stage_[b_].get();
        if (read_(i, base + off, host, m) != 0) { dry_instance_ = i; dry_record_ = base + off; return UploadError::Dry; }
        if (T_) pool_.push(i, host, m, b_);
        if (hipMemcpyAsync(static_cast<uint8_t*>(gate) + (i * seg_records_ + off) * 16, host, m * 16, hipMemcpyHostToDevice, st) != hipSuccess || hipEventRecord(stage_ev_[b_].get(), st) != hipSuccess)
          return UploadError::Copy;
      }
    next_ = base + n;
    return UploadError::None;
  }
  size_t dry_instance() const { return dry_instance_; }
  uint64_t dry_record() const { return dry_record_; }
  void finish() { pool_.finish(); }  // every queued chunk folded
  void digests(uint8_t* hashes) const { for (size_t i = 0; i < n_inst_; ++i) macs_[i].digest(hashes + 16 * i); }  // n_inst x 16, after finish()
  const std::vector<CbcMacHost>& mac_states() const { return macs_; }  // after finish(): what the next slice's start_at() takes
 private:
  const size_t n_inst_;
  const uint64_t seg_records_, chunk_;
  const size_t T_;
  const Read read_;
  std::vector<MappedHost<uint8_t>> stage_;
  std::vector<Event> stage_ev_;
  size_t b_ = 0;  // round robin over the staging buffers, across calls
  uint64_t next_ = 0;  // the stream index the next upload() must start at
  size_t dry_instance_ = 0;
  uint64_t dry_record_ = 0;
  std::vector<CbcMacHost> macs_;
  MacPool pool_;  // last: its threads read `stage_` and write `macs_`
};

// A CiphertextSource over files of 16-byte records, one per instance (FileSource, ciphertext_source.rs:14-107), closed when this goes.
// The reads of one instance are sequential in the stream, but the instances alternate: read() seeks only when the file's position is
// not the expected one.
class GcFileSource {
 public:
  GcFileSource() = default;
  GcFileSource(const GcFileSource&) = delete; GcFileSource& operator=(const GcFileSource&) = delete;
  ~GcFileSource() { for (FILE* f : files_) std::fclose(f); }
  // the file of the next instance.  False: *why names the path.
  bool add(const std::string& path, std::string* why) {
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) { *why = "cannot open " + path; return false; }
    files_.push_back(f); pos_.push_back(0);
    return true;
  }
  size_t size() const { return files_.size(); }
  FILE* file(size_t i) const { return files_[i]; }  // (for fstat; the position is read()'s)
  // records [first, first + n) of instance i -> dst; 0, or non-zero when the file ends before them (CtUploader::Read)
  int read(size_t i, uint64_t first, uint8_t* dst, uint64_t n) {
    if (pos_[i] != first) { pos_[i] = ~0ull; if (fseeko(files_[i], off_t(first * 16), SEEK_SET) != 0) return 1; pos_[i] = first; }
    if (n && std::fread(dst, 16, n, files_[i]) != n) { pos_[i] = ~0ull; return 1; }
    pos_[i] += n;
    return 0;
  }
 private:
  std::vector<FILE*> files_;
  std::vector<uint64_t> pos_;  // per file: the record its position stands at (~0 after a failed seek or a short read: the next read seeks)
};
}  // namespace gsv
