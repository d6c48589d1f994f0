// Segment layout of ovh_build_qcs' masked G2 sums: pure host code, no HIP
// (tests/host/qc_segments_harness.cpp compiles it with g++ and the sanitizers).
//
// The staged votes of a batch carry a group number each (the same-message plan's gid: distinct
// hashes in first-seen staged order). k_qc_chunk sums 64 votes per one-wave workgroup, so the
// host hands it a vote list in which the votes of group g are contiguous, in staged order, and
// padded with QC_SEG_NONE to a multiple of 64: no chunk holds votes of two groups. Chunk b owns
// list[64 b .. 64 b + 63] and the tree entries A[32 b .. 32 b + 31]; group g's chunks are
// seg[2 g] .. seg[2 g] + seg[2 g + 1] - 1 and its sum ends in A[32 seg[2 g]].
//   chunks  = sum ceil(m_g / 64) <= ceil(n / 64) + G
//   entries = 32 chunks          <= n / 2 + 32 G      (32 ceil(m / 64) <= m / 2 + 31.5)
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#define QC_SEG_NONE 0xFFFFFFFFu
#define QC_SEG_CHUNK 64u

struct QcSegments {
  std::vector<uint32_t> list;  // 64 x chunks: staged vote index or QC_SEG_NONE
  std::vector<uint32_t> seg;   // per group: first chunk, chunk count
  uint32_t chunks = 0;
  size_t entries = 0;          // tree entries the layout needs (32 per chunk)
};

// gid[j] < G for every staged vote j < n; every group has at least one vote.
static inline void qc_segments(size_t n, uint32_t G, const uint32_t* gid, QcSegments& s) {
  std::vector<uint32_t> fill(G, 0);
  for (size_t j = 0; j < n; ++j) ++fill[gid[j]];
  s.seg.assign(2 * (size_t)G, 0);
  uint32_t c = 0;
  for (uint32_t g = 0; g < G; ++g) {
    s.seg[2 * g] = c;
    s.seg[2 * g + 1] = (fill[g] + QC_SEG_CHUNK - 1) / QC_SEG_CHUNK;
    c += s.seg[2 * g + 1];
    fill[g] = 0;
  }
  s.chunks = c;
  s.entries = (size_t)(QC_SEG_CHUNK / 2) * c;
  s.list.assign((size_t)QC_SEG_CHUNK * c, QC_SEG_NONE);
  for (size_t j = 0; j < n; ++j) {
    const uint32_t g = gid[j];
    s.list[(size_t)QC_SEG_CHUNK * s.seg[2 * g] + fill[g]++] = (uint32_t)j;
  }
}
