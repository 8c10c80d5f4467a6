// TEST-ONLY (tests/test_upload_resume.py): CtUploader of csrc/engine/upload_pipeline.hpp started at a record other than 0, as a later
// slice of a sliced evaluation starts it (start_at: the first record and the MAC states to go on from), against the asynchronous HIP
// stand-ins of tests/hip_standin.  Streams of different lengths around the chunk bound (16 MiB in the engine; CHUNK records here), read
// through GcFileSource from files and through a callback reader.  For every (a, b): what is staged, and the MAC folded, over [a, b)
// and then — by a fresh uploader that takes the first one's states — over [b, n) equals one read over [a, n), and equals the stream's
// own bytes and its serial MAC.  A stream that ends early is reported with the absolute record of the chunk whose read failed; an
// upload that does not follow the stream is refused.  main() returns non-zero when a check fails; a deadlock is the caller's time limit.
#include "../../garbled_snark_verifier_amd/csrc/engine/upload_pipeline.hpp"
#include "../hip_standin/hip_standin.hpp"

#include <unistd.h>

#include <fstream>

using namespace gsv;

namespace {
constexpr uint64_t CHUNK = 8, SEG = 19;  // records per staging buffer; per gate-order segment (no multiple of the chunk)
constexpr size_t N_INST = 3;

void record_bytes(size_t inst, uint64_t r, uint8_t* out) {
  uint64_t x = (uint64_t(inst) + 1) * 0x9E3779B97F4A7C15ull ^ (r + 1) * 0xC2B2AE3D27D4EB4Full;
  for (int k = 0; k < 16; ++k) { x ^= x >> 29; x *= 0xBF58476D1CE4E5B9ull; out[k] = uint8_t(x >> 56); }
}
using Streams = std::vector<std::vector<uint8_t>>;
Streams make_streams(uint64_t n_records) {
  Streams s(N_INST, std::vector<uint8_t>(size_t(n_records) * 16));
  for (size_t i = 0; i < N_INST; ++i) for (uint64_t r = 0; r < n_records; ++r) record_bytes(i, r, s[i].data() + 16 * r);
  return s;
}
// the states of the serial MACs over records [0, n) of every stream
std::vector<CbcMacHost> serial_states(const Streams& streams, uint64_t n) {
  std::vector<CbcMacHost> m(streams.size());
  for (size_t i = 0; i < streams.size(); ++i) m[i].update(streams[i].data(), n);
  return m;
}
std::vector<uint8_t> digests_of(const std::vector<CbcMacHost>& m) {
  std::vector<uint8_t> d(16 * m.size());
  for (size_t i = 0; i < m.size(); ++i) m[i].digest(d.data() + 16 * i);
  return d;
}

struct Part { std::vector<uint8_t> staged; std::vector<CbcMacHost> states; UploadError err = UploadError::None; size_t dry_instance = 0; uint64_t dry_record = 0, next = 0; };
// records [from, to) of every stream through a fresh uploader that starts at `from` with `states`, in segments of SEG records; the
// staged bytes per instance in stream order ([instance][record])
Part run(const CtUploader::Read& read, uint64_t from, uint64_t to, const std::vector<CbcMacHost>& states, size_t T) {
  Part out;
  out.staged.assign(N_INST * size_t(to - from) * 16, 0xEE);
  Stream st;
  CHECK(st.create(hipStreamNonBlocking) == hipSuccess);
  std::vector<uint8_t> gate(N_INST * SEG * 16, 0xEE);
  CtUploader up(N_INST, SEG, CHUNK, T, read);
  CHECK(up.alloc() == hipSuccess);
  CHECK(up.next_record() == 0);
  if (from || !states.empty()) up.start_at(from, states);
  CHECK(up.next_record() == from);
  for (uint64_t base = from; base < to && out.err == UploadError::None; base += SEG) {
    const uint64_t n = std::min(SEG, to - base);
    out.err = up.upload(base, n, gate.data(), st.get());
    CHECK(hipStreamSynchronize(st.get()) == hipSuccess);
    if (out.err != UploadError::None) break;
    for (size_t i = 0; i < N_INST; ++i) std::memcpy(out.staged.data() + (i * (to - from) + (base - from)) * 16, gate.data() + i * SEG * 16, n * 16);
  }
  out.dry_instance = up.dry_instance(); out.dry_record = up.dry_record(); out.next = up.next_record();
  up.finish();
  out.states = up.mac_states();
  return out;
}
std::vector<uint8_t> expect_bytes(const Streams& s, uint64_t from, uint64_t to) {
  std::vector<uint8_t> v;
  for (size_t i = 0; i < N_INST; ++i) v.insert(v.end(), s[i].begin() + from * 16, s[i].begin() + to * 16);
  return v;
}
// [a, b) then [b, n) against [a, n), for one reader
void case_split(const Streams& s, const CtUploader::Read& read, uint64_t n, uint64_t a, uint64_t b, size_t T) {
  const std::vector<CbcMacHost> at_a = T ? serial_states(s, a) : std::vector<CbcMacHost>();
  const Part whole = run(read, a, n, at_a, T);
  const Part first = run(read, a, b, at_a, T);
  const Part second = run(read, b, n, first.states, T);
  CHECK(whole.err == UploadError::None && first.err == UploadError::None && second.err == UploadError::None);
  CHECK(whole.next == n && first.next == b && second.next == n);
  CHECK(whole.staged == expect_bytes(s, a, n) && first.staged == expect_bytes(s, a, b) && second.staged == expect_bytes(s, b, n));
  CHECK(digests_of(whole.states) == digests_of(second.states));
  // with workers the MAC is the stream's own, from record 0; without, no MAC is computed and the states stay zero
  CHECK(digests_of(second.states) == (T ? digests_of(serial_states(s, n)) : std::vector<uint8_t>(16 * N_INST, 0)));
  if (T && b > a) CHECK(digests_of(first.states) == digests_of(serial_states(s, b)) && digests_of(first.states) != digests_of(at_a));
}

struct Files {
  std::string dir;
  std::vector<std::string> paths;
  Files(const std::string& d, const Streams& s) : dir(d) {
    for (size_t i = 0; i < s.size(); ++i) {
      paths.push_back(dir + "/gc_" + std::to_string(i) + ".bin");
      std::ofstream f(paths.back(), std::ios::binary);
      f.write(reinterpret_cast<const char*>(s[i].data()), std::streamsize(s[i].size()));
    }
  }
  ~Files() { for (const std::string& p : paths) std::remove(p.c_str()); }
};

void case_length(const std::string& dir, uint64_t n) {
  const Streams s = make_streams(n);
  Files files(dir, s);
  const std::vector<uint64_t> cuts = {0, 1, CHUNK - 1, CHUNK, CHUNK + 1, SEG, n / 2, n - 1, n};
  for (size_t T : {size_t(0), size_t(2)})
    for (uint64_t a : cuts)
      for (uint64_t b : cuts) {
        if (a > b || b > n) continue;
        // the file source: opened per slice, as the engine opens it, and read from the slice's first record
        GcFileSource src;
        std::string why;
        for (const std::string& p : files.paths) CHECK(src.add(p, &why));
        case_split(s, [&src](size_t i, uint64_t first, uint8_t* dst, uint64_t m) { return src.read(i, first, dst, m); }, n, a, b, T);
        // a callback reader: sees the absolute first_record of every read
        uint64_t lowest = ~0ull;
        case_split(s, [&s, &lowest](size_t i, uint64_t first, uint8_t* dst, uint64_t m) -> int {
          lowest = std::min(lowest, first);
          if ((first + m) * 16 > s[i].size()) return 1;
          std::memcpy(dst, s[i].data() + first * 16, m * 16);
          return 0;
        }, n, a, b, T);
        if (a < n) CHECK(lowest == a);  // nothing in front of the starting record is asked for
      }
}
// instance 1's stream is `missing` records short: dry at the chunk that holds the first missing record, named by its absolute first record
void case_dry(const std::string& dir, uint64_t n, uint64_t a, uint64_t missing) {
  Streams s = make_streams(n);
  s[1].resize(size_t(n - missing) * 16);
  Files files(dir, s);
  GcFileSource src;
  std::string why;
  for (const std::string& p : files.paths) CHECK(src.add(p, &why));
  const Part p = run([&src](size_t i, uint64_t first, uint8_t* dst, uint64_t m) { return src.read(i, first, dst, m); }, a, n, serial_states(s, a), 2);
  // the chunks of a segment start at base + j x CHUNK, the segments at a + q x SEG
  const uint64_t first_missing = n - missing, seg_base = a + (first_missing - a) / SEG * SEG, chunk_base = seg_base + (first_missing - seg_base) / CHUNK * CHUNK;
  CHECK(p.err == UploadError::Dry && p.dry_instance == 1 && p.dry_record == chunk_base);
  CHECK(p.next == seg_base);  // the segment that ran dry does not count as uploaded
}
void case_order() {
  const Streams s = make_streams(40);
  Stream st;
  CHECK(st.create(hipStreamNonBlocking) == hipSuccess);
  std::vector<uint8_t> gate(N_INST * SEG * 16);
  size_t reads = 0;
  CtUploader up(N_INST, SEG, CHUNK, 1, [&](size_t i, uint64_t first, uint8_t* dst, uint64_t m) -> int { ++reads; std::memcpy(dst, s[i].data() + first * 16, m * 16); return 0; });
  CHECK(up.alloc() == hipSuccess);
  up.start_at(10, serial_states(s, 10));
  CHECK(up.upload(0, 5, gate.data(), st.get()) == UploadError::Order && up.upload(11, 5, gate.data(), st.get()) == UploadError::Order && reads == 0);
  CHECK(up.upload(10, 5, gate.data(), st.get()) == UploadError::None && up.next_record() == 15);
  CHECK(up.upload(10, 5, gate.data(), st.get()) == UploadError::Order);
  CHECK(up.upload(15, 0, gate.data(), st.get()) == UploadError::None && up.upload(15, SEG, gate.data(), st.get()) == UploadError::None && up.next_record() == 15 + SEG);
  CHECK(hipStreamSynchronize(st.get()) == hipSuccess);
  up.finish();
  CHECK(digests_of(up.mac_states()) == digests_of(serial_states(s, 15 + SEG)));
  up.start_at(3, std::vector<CbcMacHost>(1));  // states for another number of instances are not taken
  CHECK(up.next_record() == 3 && digests_of(up.mac_states()) == digests_of(serial_states(s, 15 + SEG)));
}
}  // namespace

int main() {
  char tmpl[] = "/tmp/gsv_upload_resume_XXXXXX";
  const char* made = mkdtemp(tmpl);
  if (!made) { std::perror("mkdtemp"); return 3; }
  const std::string dir = made;
  for (uint64_t n : {CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, 2 * SEG + 3, 5 * CHUNK}) case_length(dir, n);
  case_dry(dir, 5 * CHUNK, 0, 1);            // record 39 is missing: segments [0, 19) [19, 38) [38, 40), the chunk at 38
  case_dry(dir, 5 * CHUNK, 7, 1);            // segments [7, 26) [26, 40), the second one's chunks at 26 and 34: the chunk at 34
  case_dry(dir, 5 * CHUNK, 7, 12);           // record 28 is missing: the chunk at 26
  case_dry(dir, 5 * CHUNK, CHUNK + 1, 20);   // record 20 is missing: segment [9, 28), its chunk at 17
  case_order();
  CHECK(::rmdir(dir.c_str()) == 0);
  if (failures) return 1;
  std::printf("upload_resume: ok, %llu copies\n", (unsigned long long)copy_seq);
  return 0;
}
