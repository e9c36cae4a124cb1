// Stand-alone check of the native WAVE reader (afx_wav.cpp: afx_wav_probe, afx_wav_read_raw), built with AddressSanitizer +
// UBSan by `make wav-raw-check` and run on the CPU.  It writes a few hostile files into a temporary directory, probes them,
// reads each data chunk into an exactly sized heap buffer (one byte too many is an ASan report) and compares the bytes and
// the argument checks with what the headers promise.  Exit status 0: every check held.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <unistd.h>

#include "afx.h"
#include "afx_internal.h"

namespace afx {
static std::string g_err;
void set_error(const std::string& s) { g_err = s; }          // afx_host.cpp's, which is not linked here
}  // namespace afx

namespace {

int g_fail = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { std::fprintf(stderr, "wav_raw_check: line %d: %s\n", __LINE__, #cond); ++g_fail; } \
  } while (0)

void put16(std::vector<uint8_t>& b, uint32_t v) { b.push_back(v & 255); b.push_back((v >> 8) & 255); }
void put32(std::vector<uint8_t>& b, uint32_t v) { put16(b, v & 0xffff); put16(b, v >> 16); }
void tag(std::vector<uint8_t>& b, const char* t) { b.insert(b.end(), t, t + 4); }

// a RIFF/WAVE file whose data chunk CLAIMS `claimed` bytes and holds `present` (bytes i * 7 + 3); `junk` > 0: an odd-sized
// chunk (padded to a word) between fmt and data
std::vector<uint8_t> wav(int fmt_tag, int channels, int bits, uint32_t claimed, uint32_t present, uint32_t junk = 0) {
  std::vector<uint8_t> b;
  tag(b, "RIFF"); put32(b, 36 + claimed); tag(b, "WAVE");
  tag(b, "fmt "); put32(b, 16); put16(b, fmt_tag); put16(b, channels); put32(b, 16000);
  put32(b, 16000 * channels * (bits / 8)); put16(b, channels * (bits / 8)); put16(b, bits);
  if (junk) {
    tag(b, "LIST"); put32(b, junk);
    for (uint32_t i = 0; i < junk + (junk & 1); ++i) b.push_back(0xee);
  }
  tag(b, "data"); put32(b, claimed);
  for (uint32_t i = 0; i < present; ++i) b.push_back((uint8_t)(i * 7 + 3));
  return b;
}

struct Case {
  const char* name;
  std::vector<uint8_t> bytes;
  int status;              // afx_wav_probe's
  int64_t frames, data_off, data_bytes;     // expected, when status == 0
};

}  // namespace

int main() {
  char dir[] = "/tmp/wav_raw_check_XXXXXX";
  if (!mkdtemp(dir)) { std::perror("mkdtemp"); return 2; }
  std::vector<Case> cases;
  cases.push_back({"plain_s16_stereo", wav(1, 2, 16, 400, 400), 0, 100, 44, 400});
  cases.push_back({"chunk_longer_than_file", wav(1, 1, 16, 100000, 64), 0, 32, 44, 64});
  cases.push_back({"zero_frames", wav(1, 2, 24, 0, 0), 0, 0, 44, 0});
  cases.push_back({"odd_chunk_sizes", wav(1, 1, 8, 33, 33, 5), 0, 33, 44 + 8 + 6, 33});
  cases.push_back({"s24_cut_mid_frame", wav(1, 2, 24, 600, 6 * 17 + 4), 0, 17, 44, 6 * 17 + 4});     // 4 bytes of an 18th frame
  cases.push_back({"f64_seven_channels", wav(3, 7, 64, 56 * 3, 56 * 3), 0, 3, 44, 56 * 3});
  cases.push_back({"data_size_all_ones", wav(1, 1, 16, 0xffffffffu, 10), 0, 5, 44, 10});
  cases.push_back({"no_data_chunk", std::vector<uint8_t>{'R', 'I', 'F', 'F', 4, 0, 0, 0, 'W', 'A', 'V', 'E'}, 1, 0, 0, 0});
  cases.push_back({"missing_file", {}, 2, 0, 0, 0});

  const int n = (int)cases.size();
  std::vector<std::string> paths;
  for (const Case& c : cases) {
    paths.push_back(std::string(dir) + "/" + c.name + ".wav");
    if (c.status == 2) continue;
    FILE* f = std::fopen(paths.back().c_str(), "wb");
    if (!f || std::fwrite(c.bytes.data(), 1, c.bytes.size(), f) != c.bytes.size()) { std::perror("write"); return 2; }
    std::fclose(f);
  }
  std::vector<const char*> cp;
  for (const std::string& p : paths) cp.push_back(p.c_str());

  std::vector<int32_t> info(4 * n), status(n);
  std::vector<int64_t> frames(n), data_off(n);
  for (int threads : {1, 4}) {
    CHECK(afx_wav_probe(cp.data(), n, threads, info.data(), frames.data(), data_off.data(), status.data()) == AFX_OK);
    for (int i = 0; i < n; ++i) {
      CHECK(status[i] == cases[i].status);
      if (cases[i].status == 0) { CHECK(frames[i] == cases[i].frames); CHECK(data_off[i] == cases[i].data_off); }
    }
    // the bytes of whole frames, into a buffer of exactly that many bytes: clips at 16-byte boundaries, as the device
    // decoder wants them -- except the last one, so that the buffer ends with its last byte
    std::vector<int64_t> nbytes(n), offs(n);
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
      const int64_t bpf = (int64_t)(info[4 * i + 3] / 8) * info[4 * i + 1];
      nbytes[i] = status[i] == 0 ? frames[i] * bpf : (i == n - 1 ? 24 : 0);      // the missing file: asked for 24 bytes
      offs[i] = total;
      total += i + 1 < n ? (nbytes[i] + 15) / 16 * 16 : nbytes[i];
    }
    uint8_t* out = (uint8_t*)std::malloc((size_t)total);
    std::memset(out, 0x5a, (size_t)total);
    std::vector<int32_t> rs(n, -1);
    CHECK(afx_wav_read_raw(cp.data(), n, threads, data_off.data(), nbytes.data(), out, total, offs.data(), rs.data()) == AFX_OK);
    for (int i = 0; i < n; ++i) {
      CHECK(rs[i] == (cases[i].status == 2 ? 2 : 0));
      const int64_t got = cases[i].status == 0 ? nbytes[i] : 0;
      CHECK(got <= cases[i].data_bytes);
      for (int64_t k = 0; k < got; ++k) CHECK(out[offs[i] + k] == (uint8_t)(k * 7 + 3));
      const int64_t end = i + 1 < n ? offs[i + 1] : total;
      for (int64_t k = offs[i] + got; k < end; ++k) CHECK(out[k] == 0x5a);         // padding and failed clips untouched
    }
    // argument checks: nothing may be read or written
    std::memset(out, 0x5a, (size_t)total);
    CHECK(afx_wav_read_raw(cp.data(), n, threads, data_off.data(), nbytes.data(), out, total - 1, offs.data(), rs.data()) == AFX_ERR_INVALID);
    std::vector<int64_t> bad = nbytes;
    bad[0] = total + 1;
    CHECK(afx_wav_read_raw(cp.data(), n, threads, data_off.data(), bad.data(), out, total, offs.data(), rs.data()) == AFX_ERR_INVALID);
    bad = offs;
    bad[1] = -16;
    CHECK(afx_wav_read_raw(cp.data(), n, threads, data_off.data(), nbytes.data(), out, total, bad.data(), rs.data()) == AFX_ERR_INVALID);
    bad = offs;
    bad[0] = INT64_MAX - 3;
    CHECK(afx_wav_read_raw(cp.data(), n, threads, data_off.data(), nbytes.data(), out, total, bad.data(), rs.data()) == AFX_ERR_INVALID);
    for (int64_t k = 0; k < total; ++k) CHECK(out[k] == 0x5a);
    // a read past the end of a file (the caller asks for more than the probe reported) fails that clip only
    std::vector<int64_t> more = nbytes;
    more[n - 1] = 0;
    more[4] = 6 * 18;                                                              // the 18th frame is cut
    std::vector<int64_t> o2(n);
    int64_t t2 = 0;
    for (int i = 0; i < n; ++i) { o2[i] = t2; t2 += more[i]; }
    uint8_t* out2 = (uint8_t*)std::malloc((size_t)t2);
    CHECK(afx_wav_read_raw(cp.data(), n, threads, data_off.data(), more.data(), out2, t2, o2.data(), rs.data()) == AFX_OK);
    CHECK(rs[4] == 2 && rs[0] == 0 && rs[1] == 0 && rs[5] == 0);
    for (int64_t k = 0; k < more[5]; ++k) CHECK(out2[o2[5] + k] == (uint8_t)(k * 7 + 3));
    std::free(out2);
    std::free(out);
  }
  CHECK(afx_wav_read_raw(nullptr, 0, 1, nullptr, nullptr, nullptr, 0, nullptr, nullptr) == AFX_OK);
  CHECK(afx_wav_read_raw(nullptr, 1, 1, nullptr, nullptr, nullptr, 0, nullptr, nullptr) == AFX_ERR_INVALID);

  for (const std::string& p : paths) ::unlink(p.c_str());
  ::rmdir(dir);
  if (g_fail) { std::fprintf(stderr, "wav_raw_check: %d check(s) failed\n", g_fail); return 1; }
  std::printf("wav_raw_check ok: %d files, probed and read with 1 and 4 threads\n", n);
  return 0;
}
