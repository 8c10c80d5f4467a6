// TEST-ONLY (tests/test_gc_file_source.py): GcFileSource of csrc/engine/upload_pipeline.hpp, the seek-on-demand reader over one gc file
// per instance that evaluate_streaming and gsv_engine_blake3_files share, alone.  The hip* functions the header's other classes call
// are the stand-ins of tests/hip_standin/hip_standin.hpp; no HIP runtime is linked, no device is needed.  main() returns non-zero when
// a check fails.
#include "../../garbled_snark_verifier_amd/csrc/engine/upload_pipeline.hpp"
#include "../hip_standin/hip_standin.hpp"

#include <unistd.h>

#include <fstream>

using namespace gsv;

namespace {
constexpr uint64_t RECORDS = 300;
uint8_t byte_of(size_t inst, uint64_t j) { return uint8_t(j * 131 + (j >> 8) * 7 + inst * 53 + 1); }
// records [first, first + n) of instance i are what the file holds there
bool reads(GcFileSource& src, size_t i, uint64_t first, uint64_t n) {
  std::vector<uint8_t> got(size_t(n) * 16 + 1, 0xEE);
  if (src.read(i, first, got.data(), n) != 0) return false;
  for (uint64_t j = 0; j < n * 16; ++j) if (got[j] != byte_of(i, first * 16 + j)) return false;
  return got[n * 16] == 0xEE;  // (and nothing behind them was written)
}
}  // namespace

int main() {
  char tmpl[] = "/tmp/gsv_gc_file_source_XXXXXX";
  const char* made = mkdtemp(tmpl);
  if (!made) { std::perror("mkdtemp"); return 3; }
  const std::string dir = made;
  std::vector<std::string> paths;
  for (size_t i = 0; i < 3; ++i) {
    paths.push_back(dir + "/gc_" + std::to_string(i) + ".bin");
    std::vector<uint8_t> data(RECORDS * 16);
    for (size_t j = 0; j < data.size(); ++j) data[j] = byte_of(i, j);
    std::ofstream f(paths[i], std::ios::binary);
    f.write(reinterpret_cast<const char*>(data.data()), std::streamsize(data.size()));
  }
  {
    GcFileSource src;
    std::string why;
    for (const std::string& p : paths) CHECK(src.add(p, &why));
    CHECK(src.size() == 3 && src.file(0) && src.file(2) && src.file(0) != src.file(2));
    // 1. the instances alternate, each at increasing offsets (chunk-major, as CtUploader reads)
    for (uint64_t first = 0; first < RECORDS; first += 37)
      for (size_t i = 0; i < 3; ++i) CHECK(reads(src, i, first, std::min<uint64_t>(37, RECORDS - first)));
    // 2. backwards: the pass a fallback repeats starts at record 0 again; a jump forwards; the last chunk read in front of the pass
    CHECK(reads(src, 1, 0, 64) && reads(src, 1, 64, 10));
    CHECK(reads(src, 2, 200, 50) && reads(src, 2, 10, 5));
    CHECK(reads(src, 0, 256, RECORDS - 256) && reads(src, 0, 0, 256));
    // 3. n = 0 succeeds: where the position stands, elsewhere, and at the end of the file
    CHECK(src.read(0, 256, nullptr, 0) == 0 && src.read(0, 7, nullptr, 0) == 0 && src.read(0, RECORDS, nullptr, 0) == 0);
    CHECK(reads(src, 0, 7, 3));
    // 4. a read past the end returns non-zero, from the end and across it, and the source still reads what is there
    std::vector<uint8_t> buf(64 * 16);
    CHECK(src.read(1, RECORDS, buf.data(), 1) != 0);
    CHECK(src.read(1, RECORDS - 10, buf.data(), 11) != 0);
    CHECK(reads(src, 1, RECORDS - 10, 10) && reads(src, 1, 74, 20));
    // 5. a missing file fails and names its path; the files added before stay usable
    CHECK(!src.add(dir + "/gc_9.bin", &why) && why == "cannot open " + dir + "/gc_9.bin");
    CHECK(src.size() == 3 && reads(src, 2, 15, 5));
  }
  for (const std::string& p : paths) std::remove(p.c_str());
  CHECK(::rmdir(dir.c_str()) == 0);  // nothing was left behind
  if (failures) return 1;
  std::printf("gc_file_source: ok\n");
  return 0;
}
