// Stand-alone host program (g++ -fsanitize=address,undefined) over the segment layout of
// ovh_build_qcs (csrc/qc_segments.hpp) for tests/test_qc_segments_host.py: seeded random group-size
// vectors, the groups' votes interleaved as a batch's are. Prints "ok <cases>" and returns 0, or
// names the first property that fails. Test-only: never linked into the product.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <random>
#include <vector>

#include "../../consensus_overlord_amd/csrc/qc_segments.hpp"

namespace {
int fail(const char* what, uint32_t G, size_t n) {
  printf("FAIL %s (G = %u, n = %zu)\n", what, G, n);
  return 1;
}

int check(const std::vector<uint32_t>& sizes, std::mt19937_64& rng) {
  const uint32_t G = (uint32_t)sizes.size();
  std::vector<uint32_t> gid;
  for (uint32_t g = 0; g < G; ++g) gid.insert(gid.end(), sizes[g], g);
  std::shuffle(gid.begin(), gid.end(), rng);
  const size_t n = gid.size();
  QcSegments s;
  qc_segments(n, G, gid.data(), s);
  if (s.seg.size() != 2 * (size_t)G) return fail("segment table size", G, n);
  if (s.list.size() != (size_t)QC_SEG_CHUNK * s.chunks) return fail("list size", G, n);
  if (s.entries != (size_t)32 * s.chunks) return fail("entries", G, n);
  // the segment table matches the layout: consecutive, ceil(m / 64) chunks each
  uint32_t next = 0;
  for (uint32_t g = 0; g < G; ++g) {
    if (s.seg[2 * g] != next) return fail("segment start", G, n);
    if (s.seg[2 * g + 1] != (sizes[g] + 63) / 64) return fail("segment chunk count", G, n);
    next += s.seg[2 * g + 1];
  }
  if (next != s.chunks) return fail("chunk total", G, n);
  // every staged vote exactly once; a chunk's votes are of its segment's group, in staged order,
  // then pads only
  std::vector<uint32_t> seen(n, 0);
  for (uint32_t g = 0; g < G; ++g) {
    uint32_t cnt = 0, last = 0;
    bool pad = false;
    for (uint32_t q = 0; q < 64 * s.seg[2 * g + 1]; ++q) {
      const uint32_t v = s.list[(size_t)64 * s.seg[2 * g] + q];
      if (v == QC_SEG_NONE) {
        pad = true;
        continue;
      }
      if (pad) return fail("a vote after a pad", G, n);
      if (v >= n) return fail("list entry out of range", G, n);
      if (gid[v] != g) return fail("a chunk holds votes of two groups", G, n);
      if (cnt && v <= last) return fail("staged order within a group", G, n);
      last = v;
      ++cnt;
      ++seen[v];
    }
    if (cnt != sizes[g]) return fail("group size", G, n);
  }
  for (size_t j = 0; j < n; ++j)
    if (seen[j] != 1) return fail("vote not exactly once", G, n);
  if (s.chunks > (n + 63) / 64 + G) return fail("chunks <= ceil(n / 64) + G", G, n);
  if (2 * s.entries > n + 64 * (size_t)G) return fail("entries <= n / 2 + 32 G", G, n);
  return 0;
}
}  // namespace

int main() {
  std::mt19937_64 rng(0x5E65);
  const uint32_t edge[] = {1, 2, 63, 64, 65, 127, 128, 129, 300};
  unsigned cases = 0;
  for (uint32_t G = 1; G <= 64; ++G)
    for (int rep = 0; rep < 6; ++rep) {
      std::vector<uint32_t> sizes(G);
      for (uint32_t& m : sizes) m = rng() % 3 == 0 ? edge[rng() % 9] : 1 + (uint32_t)(rng() % 300);
      if (rep == 0) std::fill(sizes.begin(), sizes.end(), 1u);  // singleton groups: the entry bound's worst case
      if (rep == 1) sizes[0] = 63, sizes[G - 1] = 65, sizes[G / 2] = 64;
      if (check(sizes, rng)) return 1;
      ++cases;
    }
  // the shapes of DESIGN.md section 3.6: 64 singletons need 2,048 entries
  {
    std::vector<uint32_t> gid(64);
    for (uint32_t j = 0; j < 64; ++j) gid[j] = j;
    QcSegments s;
    qc_segments(64, 64, gid.data(), s);
    if (s.chunks != 64 || s.entries != 2048) return fail("64 singletons", 64, 64);
  }
  printf("ok %u\n", cases);
  return 0;
}
