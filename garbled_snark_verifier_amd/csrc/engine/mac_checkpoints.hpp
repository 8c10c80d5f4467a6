// The CBC-MAC checkpoints of a ciphertext stream (include/gsv_engine.h, "CBC-MAC checkpoints"): the state of the reference's
// AESAccumulatingHash chain h <- AES_K(h ^ ct) after every 2^k records, kept in a file gc_<i>.mck beside gc_<i>.bin.  The chain cannot be
// computed in parallel, but with these states it can be VERIFIED in parallel: group g starts from the claimed state g - 1, runs its 2^k
// records and must arrive at the claimed state g.  If every group holds, state -1 is zero and the last state is the commitment, the
// stream's CBC-MAC is the commitment — by induction, and without any trust in the file: a checkpoint file is UNTRUSTED input.
// This header holds the format and its parser, the host writer for a file that already exists, and the host checker (groups in parallel
// over threads, CbcMacHost::update_many over independent groups); it needs host_crypto.hpp and the standard library only.  The device
// checker is cbcmac_device.hpp / MacCheckReceiver (engine_cbcmac.ipp).
#pragma once
#include <fcntl.h>
#include <sys/stat.h>
#include <sys/types.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "host_crypto.hpp"

namespace gsv {
struct MacCheckpoints {
  static constexpr size_t HEADER_BYTES = 24;
  static constexpr char MAGIC[9] = "GSVMACK\n";  // bytes 0 .. 7
  static constexpr uint32_t VERSION = 1;         // bytes 8 .. 11, little-endian
  static constexpr uint32_t MAX_K = 30;          // bytes 12 .. 15: k, little-endian; bytes 16 .. 23: n_records, little-endian
  static constexpr uint64_t MAX_RECORDS = 1ull << 58;
  uint32_t k = 0;
  uint64_t n_records = 0;

  static uint64_t state_count(uint64_t n_records, uint32_t k) { return (n_records >> k) + ((n_records & ((1ull << k) - 1)) ? 1 : 0); }
  static uint64_t file_bytes(uint64_t n_records, uint32_t k) { return HEADER_BYTES + 16 * state_count(n_records, k); }
  uint64_t states() const { return state_count(n_records, k); }
  uint64_t first_record_of_group(uint64_t g) const { return g << k; }

  static void put_header(uint8_t out[HEADER_BYTES], uint32_t k, uint64_t n_records) {
    std::memcpy(out, MAGIC, 8);
    for (int i = 0; i < 4; ++i) { out[8 + i] = uint8_t(VERSION >> (8 * i)); out[12 + i] = uint8_t(k >> (8 * i)); }
    for (int i = 0; i < 8; ++i) out[16 + i] = uint8_t(n_records >> (8 * i));
  }
  // The header alone (24 bytes): every field in range.  False: *why says what is wrong.  Nothing is sized by a field before this passes.
  static bool parse_header(const uint8_t* p, uint64_t n_bytes, MacCheckpoints* o, std::string* why) {
    if (n_bytes < HEADER_BYTES) { *why = "the checkpoint file is shorter than its 24-byte header"; return false; }
    if (std::memcmp(p, MAGIC, 8) != 0) { *why = "not a checkpoint file: wrong magic"; return false; }
    uint32_t version = 0, k = 0; uint64_t n = 0;
    for (int i = 0; i < 4; ++i) { version |= uint32_t(p[8 + i]) << (8 * i); k |= uint32_t(p[12 + i]) << (8 * i); }
    for (int i = 0; i < 8; ++i) n |= uint64_t(p[16 + i]) << (8 * i);
    if (version != VERSION) { *why = "checkpoint format version " + std::to_string(version) + " (this engine reads version " + std::to_string(VERSION) + ")"; return false; }
    if (k > MAX_K) { *why = "the checkpoint file's group size 2^" + std::to_string(k) + " is above 2^30 records"; return false; }
    if (n > MAX_RECORDS) { *why = "the checkpoint file's n_records " + std::to_string(n) + " is out of range"; return false; }
    o->k = k; o->n_records = n;
    return true;
  }
  // ... and the length the header implies, exactly
  bool length_ok(uint64_t n_bytes, std::string* why) const {
    const uint64_t want = file_bytes(n_records, k);
    if (n_bytes == want) return true;
    *why = "the checkpoint file holds " + std::to_string(n_bytes) + " bytes, but k = " + std::to_string(k) + " and n_records = " + std::to_string(n_records) + " make " + std::to_string(want);
    return false;
  }
};

// The host's half of a device check between two segments (MacCheckStream, engine_cbcmac.ipp): which of the two carry buffers the next
// segment reads, how many records of every stream and how many segments have been enqueued.  Plain values: what a restart point of a
// sliced evaluation keeps beside the carries themselves, and puts back.
struct MacCheckPosition {
  int cpar = 0;
  uint64_t records_done = 0, fed = 0;
  void advance(uint64_t n) { cpar ^= 1; records_done += n; ++fed; }  // a segment of n records per stream has been enqueued
};

// A checkpoint file that is open and has passed the header and length checks.  It is never held whole: state ranges are read as they
// are needed (1 024 instances x a 47 GB stream at k = 0 would be terabytes; even at k = 12 the files of a call are better left on disk).
class MacCheckpointFile {
 public:
  MacCheckpointFile() = default;
  MacCheckpointFile(const MacCheckpointFile&) = delete; MacCheckpointFile& operator=(const MacCheckpointFile&) = delete;
  MacCheckpointFile(MacCheckpointFile&& o) noexcept : head(o.head), fd_(o.fd_), path_(std::move(o.path_)) { o.fd_ = -1; }
  ~MacCheckpointFile() { if (fd_ >= 0) ::close(fd_); }
  MacCheckpoints head;
  bool open(const std::string& path, std::string* why) {
    path_ = path;
    fd_ = ::open(path.c_str(), O_RDONLY | O_CLOEXEC);
    if (fd_ < 0) { *why = "cannot open " + path; return false; }
    struct stat sb;
    uint8_t h[MacCheckpoints::HEADER_BYTES];
    if (fstat(fd_, &sb) != 0 || sb.st_size < 0) { *why = "cannot open " + path; return false; }
    const ssize_t got = ::pread(fd_, h, sizeof h, 0);
    if (got < 0) { *why = "read error on " + path; return false; }
    if (!MacCheckpoints::parse_header(h, uint64_t(got), &head, why) || !head.length_ok(uint64_t(sb.st_size), why)) { *why = path + ": " + *why; return false; }
    return true;
  }
  // states [s0, s0 + count) -> dst (16 bytes each); s0 = -1 names the all-zero state in front of the stream.  False: a read error.
  bool read_states(int64_t s0, uint64_t count, uint8_t* dst) const {
    if (count && s0 < 0) { std::memset(dst, 0, 16); dst += 16; ++s0; --count; }
    if (uint64_t(s0) + count > head.states()) return false;
    for (uint64_t done = 0; done < count * 16;) {
      const ssize_t r = ::pread(fd_, dst + done, size_t(count * 16 - done), off_t(MacCheckpoints::HEADER_BYTES + uint64_t(s0) * 16 + done));
      if (r <= 0) return false;
      done += uint64_t(r);
    }
    return true;
  }
  // the commitment the file claims: its last state (sixteen zero bytes for the empty stream)
  bool commitment(uint8_t out[16]) const { return head.states() ? read_states(int64_t(head.states() - 1), 1, out) : (std::memset(out, 0, 16), true); }
  const std::string& path() const { return path_; }

 private:
  int fd_ = -1;
  std::string path_;
};
// The files of ONE call: all of them must agree on k and n_records; with `n_records` >= 0 also with the streams they are checked against.
inline bool open_mac_checkpoints(const char* const* paths, size_t n, const uint64_t* n_records, std::vector<MacCheckpointFile>* out, std::string* why) {
  out->clear();
  out->resize(n);
  for (size_t i = 0; i < n; ++i) {
    MacCheckpointFile& f = (*out)[i];
    if (!f.open(paths[i], why)) return false;
    if (n_records && f.head.n_records != *n_records) { *why = f.path() + " holds the checkpoints of a stream of " + std::to_string(f.head.n_records) + " records, the stream here holds " + std::to_string(*n_records); return false; }
    if (i && (f.head.k != (*out)[0].head.k || f.head.n_records != (*out)[0].head.n_records)) {
      *why = "the checkpoint files of one call must agree: " + (*out)[0].path() + " has k = " + std::to_string((*out)[0].head.k) + " and n_records = " + std::to_string((*out)[0].head.n_records) + ", " +
             f.path() + " has k = " + std::to_string(f.head.k) + " and n_records = " + std::to_string(f.head.n_records);
      return false;
    }
  }
  return true;
}

// whole 16-byte records of the open file `fd`, `most` at the most -> *n_records.  False: *why.
inline bool mac_file_records(int fd, const std::string& path, uint64_t* n_records, std::string* why, uint64_t most = MacCheckpoints::MAX_RECORDS) {
  struct stat sb;
  if (fd < 0 || fstat(fd, &sb) != 0) { *why = "cannot open " + path; return false; }
  if (sb.st_size < 0 || (uint64_t(sb.st_size) & 15) || uint64_t(sb.st_size) / 16 > most) { *why = path + " does not hold whole 16-byte records"; return false; }
  *n_records = uint64_t(sb.st_size) / 16;
  return true;
}
// The host writer: the checkpoints of the file at `path` for groups of 2^k records -> out_path (null: nowhere); hash = the file's CBC-MAC.
// False: *why.  Memory: one read buffer.
inline bool mac_checkpoints_of_file(const char* path, uint32_t k, const char* out_path, uint8_t hash[16], std::string* why) {
  if (k > MacCheckpoints::MAX_K) { *why = "the group size must be 2^k records with k in [0, 30]"; return false; }
  FILE* f = std::fopen(path, "rb");
  if (!f) { *why = std::string("cannot open ") + path; return false; }
  struct Closer { FILE* f; ~Closer() { if (f) std::fclose(f); } } in{f}, out{nullptr};
  uint64_t n_records = 0;
  if (!mac_file_records(fileno(f), path, &n_records, why)) return false;
  if (out_path) {
    out.f = std::fopen(out_path, "wb");
    if (!out.f) { *why = std::string("cannot create ") + out_path; return false; }
  }
  uint8_t head[MacCheckpoints::HEADER_BYTES];
  MacCheckpoints::put_header(head, k, n_records);
  bool wrote = !out.f || std::fwrite(head, 1, sizeof head, out.f) == sizeof head;
  const uint64_t G = 1ull << k;
  std::vector<uint8_t> buf(size_t(std::min<uint64_t>(std::max<uint64_t>(n_records, 1), 1 << 16)) * 16), states;
  CbcMacHost mac;
  for (uint64_t done = 0; done < n_records && wrote;) {
    const uint64_t m = std::min<uint64_t>(buf.size() / 16, n_records - done);
    if (std::fread(buf.data(), 16, size_t(m), f) != m) { *why = std::string("read error on ") + path; wrote = false; break; }
    states.clear();
    for (uint64_t off = 0; off < m;) {  // split at the multiples of 2^k of the stream position
      const uint64_t step = std::min(m - off, G - ((done + off) & (G - 1)));
      mac.update(buf.data() + off * 16, step);
      off += step;
      if (((done + off) & (G - 1)) == 0 || done + off == n_records) { states.resize(states.size() + 16); mac.digest(states.data() + states.size() - 16); }
    }
    done += m;
    if (out.f && !states.empty() && std::fwrite(states.data(), 1, states.size(), out.f) != states.size()) { *why = std::string("short write to ") + out_path; wrote = false; }
  }
  if (out.f) {
    const bool closed = std::fclose(out.f) == 0;
    out.f = nullptr;
    if (!wrote || !closed) { std::remove(out_path); if (why->empty()) *why = std::string("short write to ") + out_path; return false; }
  } else if (!wrote) return false;
  mac.digest(hash);
  return true;
}

// The host checker: the file at `path` against the checkpoint file `ck` (open, well-formed, for the file's length), groups in parallel
// over n_threads threads, each advancing up to sixteen independent groups side by side (CbcMacHost::update_many).  *bad_group = the
// lowest group that does not arrive at its claimed state, or ~0 when every group holds (then the file's CBC-MAC is ck.commitment()).
// False: a read error (*why).
inline bool mac_check_file(const char* path, const MacCheckpointFile& ck, size_t n_threads, uint64_t* bad_group, std::string* why) {
  const int fd = ::open(path, O_RDONLY | O_CLOEXEC);
  struct FdCloser { int fd; ~FdCloser() { if (fd >= 0) ::close(fd); } } closer{fd};
  uint64_t n_records = 0;
  if (!mac_file_records(fd, path, &n_records, why)) return false;
  if (n_records != ck.head.n_records) { *why = ck.path() + " holds the checkpoints of a stream of " + std::to_string(ck.head.n_records) + " records, " + path + " holds " + std::to_string(n_records); return false; }
  const uint32_t k = ck.head.k;
  const uint64_t G = 1ull << k, n_groups = ck.head.states();
  constexpr size_t LANES = 16;                                   // groups side by side per thread
  const uint64_t piece = std::min<uint64_t>(G, 4096);            // records of a group per step: bounds the buffers for any k
  const size_t T = size_t(std::max<uint64_t>(1, std::min<uint64_t>(n_threads ? n_threads : 1, (n_groups + LANES - 1) / LANES)));
  std::atomic<uint64_t> bad{~0ull};
  std::atomic<bool> io_error{false};
  auto lower = [&](uint64_t g) { uint64_t cur = bad.load(); while (g < cur && !bad.compare_exchange_weak(cur, g)) {} };
  auto read_at = [&](uint8_t* dst, uint64_t first, uint64_t n) {
    for (uint64_t done = 0; done < n * 16;) {
      const ssize_t r = ::pread(fd, dst + done, size_t(n * 16 - done), off_t(first * 16 + done));
      if (r <= 0) return false;
      done += uint64_t(r);
    }
    return true;
  };
  auto work = [&](size_t t) {
    // thread t takes the batches t, t + T, ... of LANES consecutive groups
    std::vector<uint8_t> data(LANES * size_t(piece) * 16), claimed((LANES + 1) * 16);
    for (uint64_t g0 = uint64_t(t) * LANES; g0 < n_groups && !io_error; g0 += uint64_t(T) * LANES) {
      if (g0 > bad.load()) break;  // a lower group has failed already
      const size_t lanes = size_t(std::min<uint64_t>(LANES, n_groups - g0));
      if (!ck.read_states(int64_t(g0) - 1, lanes + 1, claimed.data())) { io_error = true; return; }
      // the last group of the stream may be short: it runs alone, behind the full ones
      const bool short_last = g0 + lanes == n_groups && (n_records & (G - 1));
      const size_t full = short_last ? lanes - 1 : lanes;
      CbcMacHost macs[LANES];
      CbcMacHost* mp[LANES];
      const uint8_t* cp[LANES];
      for (size_t j = 0; j < LANES; ++j) { mp[j] = &macs[j]; cp[j] = data.data() + j * size_t(piece) * 16; }
      auto run = [&](size_t j0, size_t nj, uint64_t len) {  // groups g0 + j0 .. + nj, `len` records each
        for (uint64_t off = 0; off < len; off += piece) {
          const uint64_t m = std::min(piece, len - off);
          for (size_t j = j0; j < j0 + nj; ++j) {
            uint8_t* d = data.data() + j * size_t(piece) * 16;
            if (!read_at(d, ((g0 + j) << k) + off, m)) { io_error = true; return; }
            if (off == 0) for (int b = 0; b < 16; ++b) d[b] ^= claimed[j * 16 + b];  // CbcMacHost starts from zero: h ^ ct with h = the claimed state g - 1
          }
          CbcMacHost::update_many(mp + j0, cp + j0, nj, m);
        }
      };
      if (full) run(0, full, G);
      if (short_last && !io_error) run(lanes - 1, 1, n_records & (G - 1));
      if (io_error) return;
      for (size_t j = 0; j < lanes; ++j) {
        uint8_t got[16];
        macs[j].digest(got);
        if (std::memcmp(got, claimed.data() + (j + 1) * 16, 16) != 0) { lower(g0 + j); break; }
      }
    }
  };
  if (T == 1) work(0);
  else {
    std::vector<std::thread> pool;
    for (size_t t = 0; t < T; ++t) pool.emplace_back(work, t);
    for (auto& th : pool) th.join();
  }
  if (io_error) { *why = std::string("read error on ") + path + " or " + ck.path(); return false; }
  *bad_group = bad.load();
  return true;
}
}  // namespace gsv
