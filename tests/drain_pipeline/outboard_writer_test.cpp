// TEST-ONLY (tests/test_blake3_outboard.py): the drain-side writer of BLAKE3 outboards, OutboardFiles of csrc/engine/drain_pipeline.hpp,
// alone — behind the B3Absorbers that hand it the values, as garble_streaming_pass drives the two — and the format code of
// csrc/engine/outboard.hpp it shares with the host functions.  The hip* functions the header calls are the stand-ins of
// tests/hip_standin/hip_standin.hpp; no HIP runtime is linked, no device is needed.  main() returns non-zero when a check fails.
#include "../../garbled_snark_verifier_amd/csrc/engine/drain_pipeline.hpp"
#include "../hip_standin/hip_standin.hpp"

#include <sys/stat.h>
#include <unistd.h>

#include <fstream>
#include <iterator>

using namespace gsv;

namespace {
std::vector<uint8_t> read_file(const std::string& p) { std::ifstream f(p, std::ios::binary); return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>()); }
bool exists(const std::string& p) { struct stat sb; return ::stat(p.c_str(), &sb) == 0; }
// value v of instance i: 32 bytes that name both
void value_bytes(size_t inst, uint64_t v, uint8_t* out) { for (int k = 0; k < 32; ++k) out[k] = uint8_t(inst * 37 + v * 11 + k); }
// `count` values per instance from value `first` on, [instance][value] dense: what a segment leaves in the page-locked buffer
std::vector<uint8_t> dense(size_t n_inst, uint64_t first, uint32_t count) {
  std::vector<uint8_t> a(n_inst * size_t(count) * 32);
  for (size_t i = 0; i < n_inst; ++i) for (uint32_t g = 0; g < count; ++g) value_bytes(i, first + g, a.data() + (i * count + g) * 32);
  return a;
}
std::vector<uint8_t> expected_file(size_t inst, uint32_t k, uint64_t n_records, uint64_t first, uint64_t n_values, bool header = true) {
  std::vector<uint8_t> f(header ? Outboard::HEADER_BYTES : 0);
  if (header) Outboard::put_header(f.data(), k, n_records);
  for (uint64_t v = 0; v < n_values; ++v) { uint8_t b[32]; value_bytes(inst, first + v, b); f.insert(f.end(), b, b + 32); }
  return f;
}
// the absorbers as the drain sets them up: thread t of T writes the values of ITS instances as it receives them
struct Pass {
  OutboardFiles files;
  std::atomic<DrainError> err{DrainError::None};
  void run(size_t n_inst, size_t T, uint64_t first, const std::vector<uint32_t>& submissions) {
    B3Absorbers absorbers(T, [this](const uint8_t* vals, uint32_t groups, size_t t, size_t n) { if (!files.append(vals, groups, t, n)) drain_set_error(err, DrainError::FileWrite); return true; }, err);
    for (uint32_t groups : submissions) {
      std::vector<uint8_t> pinned = dense(n_inst, first, groups);
      absorbers.submit(pinned.data(), pinned.size(), groups);
      std::fill(pinned.begin(), pinned.end(), 0xEE);  // the next segment's copy lands there
      first += groups;
    }
    absorbers.finish();
  }
};

// 1. values arriving in several submissions (one of them empty), then the pending chunk values from the pass's own thread
void case_submissions(const std::string& dir) {
  const size_t n_inst = 5;
  const uint32_t k = 2;
  const uint64_t n_records = 64 * (6 * 4 + 2) + 1;  // 27 chunks: six groups, two pending chunk values, the last chunk
  {
    Pass p; std::string failed;
    CHECK(p.files.open(dir.c_str(), 10, n_inst, true, k, n_records, &failed) && p.files.size() == n_inst);
    p.run(n_inst, 3, 0, {2, 0, 1, 3});
    CHECK(p.err == DrainError::None);
    const std::vector<uint8_t> pend = dense(n_inst, 6, 2);
    CHECK(p.files.append(pend.data(), 2, 0, 1) && p.files.flush());
    p.files.keep();
  }
  for (size_t i = 0; i < n_inst; ++i) {
    const std::vector<uint8_t> got = read_file(OutboardFiles::path(dir.c_str(), 10 + i));
    CHECK(got == expected_file(i, k, n_records, 0, 8));
    Outboard o; std::string why;
    CHECK(Outboard::parse(got.data(), got.size(), &o, &why) && o.k == k && o.n_records == n_records && o.n_groups == 6 && o.n_pending == 2);
    CHECK(!Outboard::parse(got.data(), got.size() - 1, &o, &why) && !Outboard::parse(got.data(), 10, &o, &why));
    std::remove(OutboardFiles::path(dir.c_str(), 10 + i).c_str());
  }
}
// 2. a later slice appends; a slice restart (a new pass) truncates and writes the header again
void case_slices(const std::string& dir) {
  const size_t n_inst = 3;
  const uint32_t k = 0;
  const uint64_t n_records = 64 * 7;  // seven chunks: six values (k = 0: every value is a group value), the last chunk
  { Pass p; std::string failed; CHECK(p.files.open(dir.c_str(), 0, n_inst, true, k, n_records, &failed)); p.run(n_inst, 2, 0, {1, 2}); CHECK(p.err == DrainError::None); p.files.keep(); }
  { Pass p; std::string failed; CHECK(p.files.open(dir.c_str(), 0, n_inst, false, k, n_records, &failed)); p.run(n_inst, 2, 3, {3}); CHECK(p.err == DrainError::None); p.files.keep(); }
  for (size_t i = 0; i < n_inst; ++i) CHECK(read_file(OutboardFiles::path(dir.c_str(), i)) == expected_file(i, k, n_records, 0, 6));
  { Pass p; std::string failed; CHECK(p.files.open(dir.c_str(), 0, n_inst, true, k, n_records, &failed)); p.run(n_inst, 2, 100, {2}); CHECK(p.err == DrainError::None); p.files.keep(); }
  for (size_t i = 0; i < n_inst; ++i) {
    CHECK(read_file(OutboardFiles::path(dir.c_str(), i)) == expected_file(i, k, n_records, 100, 2));
    std::remove(OutboardFiles::path(dir.c_str(), i).c_str());
  }
}
// 3. a failed pass — the object goes away without keep() — removes its files, a first slice's and a later slice's alike; a directory
// that does not exist is reported with the path
void case_failure(const std::string& dir) {
  const size_t n_inst = 4;
  { Pass p; std::string failed; CHECK(p.files.open(dir.c_str(), 7, n_inst, true, 3, 1000, &failed)); p.run(n_inst, 2, 0, {1}); CHECK(exists(OutboardFiles::path(dir.c_str(), 7)) && exists(OutboardFiles::path(dir.c_str(), 10))); }
  for (size_t i = 0; i < n_inst; ++i) CHECK(!exists(OutboardFiles::path(dir.c_str(), 7 + i)));
  { Pass p; std::string failed; CHECK(p.files.open(dir.c_str(), 7, n_inst, true, 3, 1000, &failed)); p.files.keep(); }
  { Pass p; std::string failed; CHECK(p.files.open(dir.c_str(), 7, n_inst, false, 3, 1000, &failed)); p.run(n_inst, 2, 0, {1}); }
  for (size_t i = 0; i < n_inst; ++i) CHECK(!exists(OutboardFiles::path(dir.c_str(), 7 + i)));
  { OutboardFiles f; std::string failed; CHECK(!f.open((dir + "/none").c_str(), 3, 2, true, 3, 1000, &failed) && failed == dir + "/none/gc_3.b3o"); }
}
// 4. the writer fed with real values gives the file the host writer gives, and the root is the hash of the bytes
void case_real_values(const std::string& dir) {
  const uint32_t k = 1;
  const uint64_t n_records = 64 * 5 + 9;  // six chunks: two groups of two, one pending chunk value, a partial last chunk
  std::vector<uint8_t> stream(size_t(n_records) * 16);
  for (size_t j = 0; j < stream.size(); ++j) stream[j] = uint8_t(j * 131 + (j >> 8) * 7);
  const std::string gc = dir + "/gc_0.bin";
  { std::ofstream f(gc, std::ios::binary); f.write(reinterpret_cast<const char*>(stream.data()), std::streamsize(stream.size())); }
  std::vector<uint8_t> ob, last; std::string why;
  CHECK(outboard_of_file(gc.c_str(), k, &ob, &last, &why));
  CHECK(last.size() == 9 * 16 && ob.size() == Outboard::file_bytes(n_records, k));
  std::vector<uint8_t> cvs(5 * 32);
  for (uint64_t c = 0; c < 5; ++c) outboard_chunk_value(stream.data() + 1024 * c, c, cvs.data() + 32 * c);
  std::vector<uint8_t> groups(2 * 32);
  for (int g = 0; g < 2; ++g) { std::vector<uint8_t> pair(cvs.begin() + 64 * g, cvs.begin() + 64 * g + 64); outboard_reduce_group(pair.data(), k); std::memcpy(groups.data() + 32 * g, pair.data(), 32); }
  {
    OutboardFiles f; std::string failed;
    CHECK(f.open(dir.c_str(), 0, 1, true, k, n_records, &failed));
    CHECK(f.append(groups.data(), 1, 0, 1) && f.append(groups.data() + 32, 1, 0, 1) && f.append(cvs.data() + 4 * 32, 1, 0, 1) && f.flush());
    f.keep();
  }
  CHECK(read_file(OutboardFiles::path(dir.c_str(), 0)) == ob);
  Outboard o; uint8_t root[32], want[32];
  CHECK(Outboard::parse(ob.data(), ob.size(), &o, &why) && o.root(last.data(), last.size(), root, &why));
  Blake3Host h; h.update(stream.data(), stream.size()); CHECK(h.finalize(want));
  CHECK(std::memcmp(root, want, 32) == 0);
  CHECK(!o.root(last.data(), last.size() - 16, root, &why));  // a last chunk of another length than n_records leaves
  std::remove(gc.c_str());
  std::remove(OutboardFiles::path(dir.c_str(), 0).c_str());
}
}  // namespace

int main() {
  char tmpl[] = "/tmp/gsv_outboard_writer_XXXXXX";
  const char* made = mkdtemp(tmpl);
  if (!made) { std::perror("mkdtemp"); return 3; }
  const std::string dir = made;
  case_submissions(dir);
  case_slices(dir);
  case_failure(dir);
  case_real_values(dir);
  CHECK(::rmdir(dir.c_str()) == 0);  // nothing was left behind
  if (failures) return 1;
  std::printf("outboard_writer: ok\n");
  return 0;
}
