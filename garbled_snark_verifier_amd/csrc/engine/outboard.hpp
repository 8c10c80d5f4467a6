// The BLAKE3 outboard of a ciphertext stream (include/gsv_engine.h, "BLAKE3 outboards"): the values the host absorbs when a stream is
// hashed on the device — one 32-byte value per aligned group of 2^k chunks, then the chunk values behind the last complete group —
// kept in a file beside gc_<i>.bin, or handed to a host callback, instead of thrown away.  One level of the tree, a format of this project's own: NOT Bao.  This
// header parses and folds an outboard, computes one on the host for a file that already exists, and loads the outboards of a set of
// streams and compares them with the values a receiver's streams hash to (B3Check); it needs host_crypto.hpp and the standard library
// only (the drain-side writer is OutboardWriter, drain_pipeline.hpp).
#pragma once
#include <sys/types.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "host_crypto.hpp"

namespace gsv {
struct Outboard {
  static constexpr size_t HEADER_BYTES = 24;
  static constexpr char MAGIC[9] = "GSVB3OB\n";  // bytes 0 .. 7
  static constexpr uint32_t VERSION = 1;         // bytes 8 .. 11, little-endian
  static constexpr uint32_t MAX_K = 20;          // bytes 12 .. 15: k, little-endian; bytes 16 .. 23: n_records, little-endian
  static constexpr uint64_t MAX_RECORDS = 1ull << 58;  // (n_records x 16 bytes fits 64 bits with room to spare)
  uint32_t k = 0;
  uint64_t n_records = 0;
  uint64_t n_groups = 0, n_pending = 0;  // floor((N - 1) / 2^k) group values, then (N - 1) mod 2^k chunk values
  const uint8_t* values = nullptr;       // (n_groups + n_pending) x 32 bytes behind the header

  static uint64_t chunks(uint64_t n_records) { return std::max<uint64_t>(1, (n_records + 63) / 64); }
  static uint64_t value_count(uint64_t n_records, uint32_t k) { const uint64_t d = chunks(n_records) - 1; return (d >> k) + (d & ((1ull << k) - 1)); }
  static uint64_t file_bytes(uint64_t n_records, uint32_t k) { return HEADER_BYTES + 32 * value_count(n_records, k); }
  // bytes of the stream's last chunk, which no outboard represents: 0 for the empty stream, else 16 .. 1024
  static uint64_t last_chunk_bytes(uint64_t n_records) { return (n_records - 64 * (chunks(n_records) - 1)) * 16; }
  uint64_t first_record_of_group(uint64_t g) const { return (g << k) * 64; }

  static void put_header(uint8_t out[HEADER_BYTES], uint32_t k, uint64_t n_records) {
    std::memcpy(out, MAGIC, 8);
    for (int i = 0; i < 4; ++i) { out[8 + i] = uint8_t(VERSION >> (8 * i)); out[12 + i] = uint8_t(k >> (8 * i)); }
    for (int i = 0; i < 8; ++i) out[16 + i] = uint8_t(n_records >> (8 * i));
  }
  // The header alone (24 bytes): every field in range.  False: *why says what is wrong.  Nothing is sized by a field before this passes.
  static bool parse_header(const uint8_t* p, uint64_t n_bytes, Outboard* o, std::string* why) {
    if (n_bytes < HEADER_BYTES) { *why = "the outboard is shorter than its 24-byte header"; return false; }
    if (std::memcmp(p, MAGIC, 8) != 0) { *why = "not an outboard: wrong magic"; return false; }
    uint32_t version = 0, k = 0; uint64_t n = 0;
    for (int i = 0; i < 4; ++i) { version |= uint32_t(p[8 + i]) << (8 * i); k |= uint32_t(p[12 + i]) << (8 * i); }
    for (int i = 0; i < 8; ++i) n |= uint64_t(p[16 + i]) << (8 * i);
    if (version != VERSION) { *why = "outboard format version " + std::to_string(version) + " (this engine reads version " + std::to_string(VERSION) + ")"; return false; }
    if (k > MAX_K) { *why = "the outboard's group size 2^" + std::to_string(k) + " is above 2^20 chunks"; return false; }
    if (n > MAX_RECORDS) { *why = "the outboard's n_records " + std::to_string(n) + " is out of range"; return false; }
    o->k = k; o->n_records = n;
    const uint64_t d = chunks(n) - 1;
    o->n_groups = d >> k; o->n_pending = d & ((1ull << k) - 1);
    o->values = nullptr;
    return true;
  }
  // ... and the whole of it: the byte length is exactly what the header's k and n_records ask for
  static bool parse(const uint8_t* p, uint64_t n_bytes, Outboard* o, std::string* why) {
    if (!parse_header(p, n_bytes, o, why)) return false;
    const uint64_t want = file_bytes(o->n_records, o->k);
    if (n_bytes != want) {
      *why = "the outboard holds " + std::to_string(n_bytes) + " bytes, but k = " + std::to_string(o->k) + " and n_records = " + std::to_string(o->n_records) + " make " + std::to_string(want);
      return false;
    }
    o->values = p + HEADER_BYTES;
    return true;
  }
  // The root: the values folded with the last chunk's bytes, as the host finishes a stream hashed on the device.
  bool root(const uint8_t* last_chunk, uint64_t last_bytes, uint8_t out[32], std::string* why) const {
    if (last_bytes != last_chunk_bytes(n_records)) {
      *why = "the last chunk of a stream of " + std::to_string(n_records) + " records holds " + std::to_string(last_chunk_bytes(n_records)) + " bytes, " + std::to_string(last_bytes) + " were given";
      return false;
    }
    Blake3Host h;
    bool ok = true;
    for (uint64_t g = 0; g < n_groups; ++g) ok = h.absorb_subtree(values + 32 * g, k) && ok;
    for (uint64_t c = 0; c < n_pending; ++c) ok = h.absorb_subtree(values + 32 * (n_groups + c), 0) && ok;
    if (last_bytes) h.update(last_chunk, last_bytes);
    if (!ok || !h.finalize(out)) { *why = "internal: outboard values out of order"; return false; }
    return true;
  }
};

// chaining value of the full 1 KiB chunk number `counter` (never the root: more input follows)
inline void outboard_chunk_value(const uint8_t* chunk, uint64_t counter, uint8_t out[32]) {
  uint32_t cv[8];
  std::memcpy(cv, Blake3Host::IV, sizeof cv);
  for (int b = 0; b < 16; ++b) {
    uint32_t w[16];
    for (int i = 0; i < 16; ++i) { const uint8_t* q = chunk + 64 * b + 4 * i; w[i] = uint32_t(q[0]) | uint32_t(q[1]) << 8 | uint32_t(q[2]) << 16 | uint32_t(q[3]) << 24; }
    Blake3Host::compress(cv, w, counter, 64, (b == 0 ? Blake3Host::CHUNK_START : 0) | (b == 15 ? Blake3Host::CHUNK_END : 0), cv);
  }
  for (int i = 0; i < 8; ++i) for (int j = 0; j < 4; ++j) out[4 * i + j] = uint8_t(cv[i] >> (8 * j));
}
// 2^k chaining values (k >= 0) reduced in place to the value of their subtree, vals[0 .. 32)
inline void outboard_reduce_group(uint8_t* vals, uint32_t k) {
  for (uint64_t n = 1ull << k; n > 1; n >>= 1)
    for (uint64_t j = 0; j < n / 2; ++j) {
      uint32_t w[16], cv[8];
      for (int i = 0; i < 16; ++i) { const uint8_t* q = vals + 64 * j + 4 * i; w[i] = uint32_t(q[0]) | uint32_t(q[1]) << 8 | uint32_t(q[2]) << 16 | uint32_t(q[3]) << 24; }
      Blake3Host::compress(Blake3Host::IV, w, 0, 64, Blake3Host::PARENT, cv);
      for (int i = 0; i < 8; ++i) for (int t = 0; t < 4; ++t) vals[32 * j + 4 * i + t] = uint8_t(cv[i] >> (8 * t));
    }
}
// The host writer: the outboard of the file at `path` (whole 16-byte records) for groups of 2^k chunks, as bytes, and its last chunk.
// False: *why.  Memory: one group's chunk values (32 B x 2^k) and the outboard itself.
inline bool outboard_of_file(const char* path, uint32_t k, std::vector<uint8_t>* ob, std::vector<uint8_t>* last_chunk, std::string* why) {
  if (k > Outboard::MAX_K) { *why = "the group size must be 2^k chunks with k in [0, 20]"; return false; }
  FILE* f = std::fopen(path, "rb");
  if (!f) { *why = std::string("cannot open ") + path; return false; }
  struct Closer { FILE* f; ~Closer() { std::fclose(f); } } closer{f};
  if (fseeko(f, 0, SEEK_END) != 0) { *why = std::string("cannot seek in ") + path; return false; }
  const off_t size = ftello(f);
  if (size < 0 || (uint64_t(size) & 15) || uint64_t(size) / 16 > Outboard::MAX_RECORDS) { *why = std::string(path) + " does not hold whole 16-byte records"; return false; }
  std::rewind(f);
  const uint64_t n_records = uint64_t(size) / 16, dev_chunks = Outboard::chunks(n_records) - 1, G = 1ull << k;
  ob->assign(Outboard::HEADER_BYTES, 0);
  ob->reserve(size_t(Outboard::file_bytes(n_records, k)));
  Outboard::put_header(ob->data(), k, n_records);
  std::vector<uint8_t> group, buf(1 << 20);
  group.reserve(size_t(std::min<uint64_t>(G, dev_chunks + 1)) * 32);
  for (uint64_t c = 0; c < dev_chunks;) {
    const size_t want = size_t(std::min<uint64_t>(buf.size() / 1024, dev_chunks - c));
    if (std::fread(buf.data(), 1024, want, f) != want) { *why = std::string("read error on ") + path; return false; }
    for (size_t j = 0; j < want; ++j, ++c) {
      uint8_t cv[32];
      outboard_chunk_value(buf.data() + 1024 * j, c, cv);
      group.insert(group.end(), cv, cv + 32);
      if (group.size() == G * 32) { outboard_reduce_group(group.data(), k); ob->insert(ob->end(), group.begin(), group.begin() + 32); group.clear(); }
    }
  }
  ob->insert(ob->end(), group.begin(), group.end());  // the chunk values behind the last complete group
  last_chunk->resize(size_t(Outboard::last_chunk_bytes(n_records)));
  if (!last_chunk->empty() && std::fread(last_chunk->data(), 1, last_chunk->size(), f) != last_chunk->size()) { *why = std::string("read error on ") + path; return false; }
  return true;
}

// The outboards a set of streams is verified against, by whoever receives the values the host absorbs (B3Receiver, engine_blake3.ipp):
// a streaming evaluation in verified mode and gsv_engine_blake3_files.  Every value is compared, in the order it arrives, with the
// outboard of its instance; the first difference — the lowest group, then the lowest instance — is kept.
struct B3Check {
  std::vector<std::vector<uint8_t>> bytes;  // per instance: a well-formed outboard for `k` and `n_records`
  uint32_t k = 0;
  uint64_t n_records = 0, n_groups = 0, n_pending = 0;
  uint64_t next = 0;                        // group values compared so far, per instance
  size_t bad_instance = 0;
  uint64_t bad_group = 0, bad_record = 0;   // the group (the open tail behind the last complete group: n_groups) and the first record the value covers
  // for n_inst streams of n_records records in groups of 2^k chunks, the outboards still to be filled in
  void shape(size_t n_inst, uint32_t k_, uint64_t n_records_) {
    const uint64_t dev_chunks = Outboard::chunks(n_records_) - 1;
    k = k_; n_records = n_records_; n_groups = dev_chunks >> k; n_pending = dev_chunks & ((1ull << k) - 1);
    bytes.resize(n_inst);
  }
  void reset() { next = 0; }  // the streams start again from group 0
  // A restart point of the comparison (a sliced evaluation rolls back to where a slice began): the position is all that moves
  uint64_t position() const { return next; }
  void rewind(uint64_t position) { next = position; }
  // is every outboard still the well-formed one of this shape?  (a host hands the in-memory outboards in again with every slice)
  bool holds(size_t n_inst, uint32_t k_, uint64_t n_records_) const {
    if (bytes.size() != n_inst || k != k_ || n_records != n_records_) return false;
    for (const std::vector<uint8_t>& b : bytes) if (b.size() != Outboard::file_bytes(n_records, k)) return false;
    return true;
  }
  const uint8_t* value(size_t i, uint64_t v) const { return bytes[i].data() + Outboard::HEADER_BYTES + 32 * v; }
  // `groups` group values per instance, [instance][group] dense
  bool groups_match(const uint8_t* vals, uint32_t groups) {
    if (next + groups > n_groups) { bad_instance = 0; bad_group = n_groups; bad_record = (n_groups << k) * 64; return false; }
    for (uint32_t g = 0; g < groups; ++g)
      for (size_t i = 0; i < bytes.size(); ++i)
        if (std::memcmp(vals + (i * groups + g) * 32, value(i, next + g), 32) != 0) { bad_instance = i; bad_group = next + g; bad_record = ((next + g) << k) * 64; return false; }
    next += groups;
    return true;
  }
  // the chunk values behind the last complete group, [instance][value] dense
  bool pending_match(const uint8_t* vals, uint32_t pend) {
    if (next != n_groups || pend != n_pending) { bad_instance = 0; bad_group = std::min(next, n_groups); bad_record = (bad_group << k) * 64; return false; }
    for (uint32_t c = 0; c < pend; ++c)
      for (size_t i = 0; i < bytes.size(); ++i)
        if (std::memcmp(vals + (i * pend + c) * 32, value(i, n_groups + c), 32) != 0) { bad_instance = i; bad_group = n_groups; bad_record = ((n_groups << k) + c) * 64; return false; }
    return true;
  }
  std::string where(const char* what) const {
    return std::string(what) + " " + std::to_string(bad_instance) + " does not match its outboard in group " + std::to_string(bad_group) + " (from record " + std::to_string(bad_record) + ")";
  }
};
// The whole of `path` (at most `most` bytes are accepted) -> *out.  False: *why.
inline bool read_small_file(const std::string& path, uint64_t most, std::vector<uint8_t>* out, std::string* why) {
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) { *why = "cannot open " + path; return false; }
  out->resize(size_t(most) + 1);
  const size_t n = std::fread(out->data(), 1, out->size(), f);
  const bool bad = std::ferror(f) != 0;
  std::fclose(f);
  if (bad) { *why = "read error on " + path; return false; }
  out->resize(n);
  return true;
}
// The outboard at `path` for a stream of n_records records in groups of 2^k chunks -> *out, parsed and bounds-checked.  A header that
// says otherwise, and a length that does not follow from it, are refused (*why names both sides).
// ... `name` being the file's path, or what else the message should call an outboard that came in memory
inline bool check_outboard(const std::string& name, const uint8_t* p, uint64_t n_bytes, uint32_t k, uint64_t n_records, std::string* why) {
  Outboard o;
  if (!Outboard::parse_header(p, n_bytes, &o, why)) { *why = name + ": " + *why; return false; }
  if (o.n_records != n_records) { *why = name + " is the outboard of a stream of " + std::to_string(o.n_records) + " records, the stream here holds " + std::to_string(n_records); return false; }
  if (o.k != k) { *why = name + " was written for groups of 2^" + std::to_string(o.k) + " chunks, this pass reduces groups of 2^" + std::to_string(k) + " (GSV_B3_SUBTREE_LOG2)"; return false; }
  if (!Outboard::parse(p, n_bytes, &o, why)) { *why = name + ": " + *why; return false; }
  return true;
}
inline bool load_outboard(const std::string& path, uint32_t k, uint64_t n_records, std::vector<uint8_t>* out, std::string* why) {
  if (!read_small_file(path, Outboard::file_bytes(n_records, k), out, why)) return false;
  return check_outboard(path, out->data(), out->size(), k, n_records, why);
}
}  // namespace gsv
