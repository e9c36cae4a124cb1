// Stand-alone check of the packing of a host batch (afx_host.cpp: pack_pieces, scatter_pieces -- what stage_in uploads and
// what the entry points hand back), built with AddressSanitizer + UBSan by `make stage-check` and run on the CPU.  The
// sources are exactly sized heap buffers whose last piece ends on their last byte (a read past one is an ASan report); the
// layouts are those of the entry points: slots of 4 or 8 elements of 2 or 4 bytes, slots of 16 bytes, two sources in one
// image, tail slack, an empty image.  Exit status 0: every gap byte is zero and every piece intact.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "afx_internal.h"

using namespace afx;

namespace {

int g_fail = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { std::fprintf(stderr, "stage_check: line %d: %s\n", __LINE__, #cond); ++g_fail; } \
  } while (0)

// every byte of image is its piece's source byte, or zero where no piece lies
void check_image(const std::vector<char>& image, int64_t total, const std::vector<HostPiece>& pieces) {
  CHECK((int64_t)image.size() == total);
  std::vector<char> want((size_t)total, 0);
  std::vector<char> covered((size_t)total, 0);
  for (const HostPiece& p : pieces)
    for (int64_t b = 0; b < p.n_bytes; ++b) {
      CHECK(!covered[(size_t)(p.dst_bytes + b)]);              // the layouts under test never overlap
      want[(size_t)(p.dst_bytes + b)] = ((const char*)p.src)[b];
      covered[(size_t)(p.dst_bytes + b)] = 1;
    }
  CHECK(image == want);
}

// a source of exactly `bytes` bytes, none of them zero, distinct per seed
std::vector<char> source(int64_t bytes, int seed) {
  std::vector<char> s((size_t)bytes);
  for (int64_t b = 0; b < bytes; ++b) s[(size_t)b] = (char)(1 + (b * 7 + seed * 31) % 255);
  return s;
}

// clips of `lens` elements of esz bytes, back to back in one exactly sized source, packed into slots of `align` elements;
// `order` is the order the pieces are listed in
void clips_case(const std::vector<int64_t>& lens, int64_t esz, int64_t align, const std::vector<int>& order, int64_t slack) {
  int64_t src_elems = 0;
  for (int64_t n : lens) src_elems += n;
  const std::vector<char> src = source(src_elems * esz, (int)(esz + align));
  std::vector<int64_t> src_off, dst_off;
  int64_t s = 0, in_pos = 0;
  for (int64_t n : lens) { src_off.push_back(s); dst_off.push_back(in_pos); s += n; in_pos += (n + align - 1) / align * align; }
  std::vector<HostPiece> pieces;
  for (int i : order) pieces.push_back({src.data() + src_off[i] * esz, dst_off[i] * esz, lens[i] * esz});
  std::vector<char> image(3, 'x');                             // stale content of an earlier chunk goes
  pack_pieces(image, in_pos * esz + slack, pieces);
  check_image(image, in_pos * esz + slack, pieces);
}

}  // namespace

int main() {
  const std::vector<int64_t> lens = {5, 0, 8, 1, 13, 0, 4};    // the last clip ends on the source's last byte
  const std::vector<int> fwd = {0, 1, 2, 3, 4, 5, 6}, mixed = {4, 6, 1, 0, 5, 3, 2};
  for (int64_t esz : {2, 4})
    for (int64_t align : {4, 8})
      for (const std::vector<int>& order : {fwd, mixed})
        for (int64_t slack : {0, 16}) clips_case(lens, esz, align, order, slack);
  // raw bytes in slots of 16 (afx_decode_batch): odd byte counts, one element per byte
  clips_case({3, 16, 0, 33, 1}, 1, 16, {0, 1, 2, 3, 4}, 0);
  clips_case({3, 16, 0, 33, 1}, 1, 16, {3, 0, 4, 2, 1}, 0);
  // two sources in one image (afx_compare_batch): pair q's ref slot, then its deg slot, 8 elements of 2 or 4 bytes
  for (int64_t esz : {2, 4}) {
    const std::vector<int64_t> n = {9, 0, 16, 7};
    int64_t total = 0;
    for (int64_t k : n) total += k;
    const std::vector<char> ref = source(total * esz, 1), deg = source(total * esz, 2);
    std::vector<HostPiece> pieces;
    int64_t off = 0, in_pos = 0;
    for (int64_t k : n) {
      const int64_t slot = (k + 7) / 8 * 8;
      pieces.push_back({ref.data() + off * esz, in_pos * esz, k * esz});
      pieces.push_back({deg.data() + off * esz, (in_pos + slot) * esz, k * esz});
      off += k; in_pos += 2 * slot;
    }
    std::vector<char> image;
    pack_pieces(image, in_pos * esz, pieces);
    check_image(image, in_pos * esz, pieces);
  }
  // nothing to pack: an empty image, a one-element image of zeros (the max(size, 1) callers), pieces of no bytes at a null source
  std::vector<char> image(7, 'x');
  pack_pieces(image, 0, {});
  CHECK(image.empty());
  pack_pieces(image, 4, {{nullptr, 0, 0}, {nullptr, 4, 0}});
  CHECK(image == std::vector<char>(4, 0));
  // the way back: the listed pieces land, every other byte of the destination stays as it was
  {
    const std::vector<char> packed = source(64, 3);
    std::vector<char> out(40, 'x'), want(40, 'x');
    const std::vector<HostPiece> pieces = {{packed.data() + 32, 4, 12}, {packed.data() + 60, 36, 4}, {packed.data(), 20, 0}};
    scatter_pieces(out.data(), pieces);
    std::memcpy(want.data() + 4, packed.data() + 32, 12);
    std::memcpy(want.data() + 36, packed.data() + 60, 4);
    CHECK(out == want);
    scatter_pieces(nullptr, {});                               // no piece: the destination is not touched
  }
  if (g_fail) { std::fprintf(stderr, "stage_check: %d check(s) failed\n", g_fail); return 1; }
  std::printf("stage_check: ok\n");
  return 0;
}
