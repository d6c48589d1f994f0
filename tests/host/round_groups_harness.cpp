// Stand-alone host program (g++ -fsanitize=address,undefined) over the round numbering of
// ovh_rounds_add (csrc/qc_round_groups.hpp) and the segment input it feeds (csrc/qc_segments.hpp)
// for tests/test_round_groups_host.py. Prints "ok <cases>" and returns 0, or names the first
// property that fails. Test-only: never linked into the product.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <random>
#include <vector>

#include "../../consensus_overlord_amd/csrc/qc_round_groups.hpp"
#include "../../consensus_overlord_amd/csrc/qc_segments.hpp"

namespace {
int fail(const char* what, size_t n) {
  printf("FAIL %s (n = %zu)\n", what, n);
  return 1;
}

// ids: the caller's list; table[i]: vote i is a table voter (the batch stages those first, both
// halves in the caller's order, and no permutation at all when the halves are not mixed)
int check(const std::vector<uint64_t>& ids, const std::vector<uint8_t>& table) {
  const size_t n = ids.size();
  QcRoundGroups g;
  qc_round_number(n, ids.data(), g);
  if (g.slot.size() != n || g.pos.size() != n || g.ids.size() != g.K || g.cnt.size() != g.K) return fail("sizes", n);
  // numbering by first appearance; positions count a round's own votes in the caller's order
  std::vector<uint64_t> seen;
  std::vector<uint32_t> cnt;
  for (size_t i = 0; i < n; ++i) {
    size_t k = std::find(seen.begin(), seen.end(), ids[i]) - seen.begin();
    if (k == seen.size()) {
      seen.push_back(ids[i]);
      cnt.push_back(0);
    }
    if (g.slot[i] != k) return fail("numbering by first appearance", n);
    if (g.pos[i] != cnt[k]++) return fail("position among the round's votes", n);
  }
  if (g.K != seen.size() || g.ids != seen || g.cnt != cnt) return fail("ids / counts per number", n);
  // table-first permutation
  std::vector<uint32_t> perm;
  size_t t = 0;
  for (size_t i = 0; i < n; ++i) t += table[i];
  if (t && t < n) {
    for (size_t i = 0; i < n; ++i)
      if (table[i]) perm.push_back((uint32_t)i);
    for (size_t i = 0; i < n; ++i)
      if (!table[i]) perm.push_back((uint32_t)i);
  }
  qc_round_stage(n, perm.empty() ? nullptr : perm.data(), g);
  if (g.gid.size() != n || g.orig.size() != n) return fail("staged sizes", n);
  for (size_t j = 0; j < n; ++j) {
    const size_t i = perm.empty() ? j : perm[j];
    if (g.gid[j] != g.slot[i] || g.orig[j] != g.pos[i]) return fail("staged number / position", n);
  }
  // (number, position) names every vote once, and within a round the staged order of the table
  // votes keeps the caller's order (positions increase)
  std::vector<std::vector<uint8_t>> hit(g.K);
  for (uint32_t k = 0; k < g.K; ++k) hit[k].assign(g.cnt[k], 0);
  std::vector<int64_t> last(g.K, -1);
  for (size_t j = 0; j < n; ++j) {
    if (g.orig[j] >= g.cnt[g.gid[j]] || hit[g.gid[j]][g.orig[j]]++) return fail("(number, position) not unique", n);
    if (j < t || !t) {
      if ((int64_t)g.orig[j] <= last[g.gid[j]]) return fail("staged order within a round", n);
      last[g.gid[j]] = g.orig[j];
    }
    if (j + 1 == t) std::fill(last.begin(), last.end(), -1);
  }
  // the segment input: one segment per round, ceil(cnt / 64) chunks, its votes those of the round
  QcSegments s;
  qc_segments(n, g.K, g.gid.data(), s);
  uint32_t next = 0;
  for (uint32_t k = 0; k < g.K; ++k) {
    if (s.seg[2 * k] != next || s.seg[2 * k + 1] != (g.cnt[k] + 63) / 64) return fail("segment of a round", n);
    uint32_t m = 0;
    for (uint32_t q = 0; q < 64 * s.seg[2 * k + 1]; ++q) {
      const uint32_t v = s.list[(size_t)64 * next + q];
      if (v == QC_SEG_NONE) continue;
      if (v >= n || g.gid[v] != k) return fail("a segment holds another round's vote", n);
      ++m;
    }
    if (m != g.cnt[k]) return fail("segment vote count", n);
    next += s.seg[2 * k + 1];
  }
  return 0;
}
}  // namespace

int main() {
  std::mt19937_64 rng(0x726F756E6473);
  unsigned cases = 0;
  // seeded lists over 1 .. 16 rounds with sparse 64-bit ids, table and other voters mixed
  for (uint32_t K = 1; K <= 16; ++K)
    for (int rep = 0; rep < 8; ++rep) {
      std::vector<uint64_t> pool(K);
      for (uint64_t& id : pool) id = rng() | 1;
      const size_t n = 1 + rng() % 200;
      std::vector<uint64_t> ids(n);
      std::vector<uint8_t> table(n);
      for (size_t i = 0; i < n; ++i) {
        ids[i] = pool[rng() % K];
        table[i] = rep % 4 == 0 ? 1 : rep % 4 == 1 ? 0 : (uint8_t)(rng() % 4 != 0);
      }
      if (check(ids, table)) return 1;
      ++cases;
    }
  {  // 16 singleton rounds: 16 chunks, 512 tree entries
    std::vector<uint64_t> ids(16);
    for (uint32_t k = 0; k < 16; ++k) ids[k] = 1000 - k;
    if (check(ids, std::vector<uint8_t>(16, 1))) return 1;
    QcRoundGroups g;
    qc_round_number(16, ids.data(), g);
    qc_round_stage(16, nullptr, g);
    QcSegments s;
    qc_segments(16, g.K, g.gid.data(), s);
    if (g.K != 16 || s.chunks != 16 || s.entries != 512) return fail("16 singleton rounds", 16);
    for (uint32_t k = 0; k < 16; ++k)
      if (g.ids[k] != 1000 - k || g.pos[k] != 0) return fail("16 singleton rounds: ids", 16);
    ++cases;
  }
  {  // one round of 65 votes beside one round of 1 vote, the single vote in the middle
    std::vector<uint64_t> ids(66, 7);
    ids[40] = 3;
    std::vector<uint8_t> table(66, 1);
    table[0] = 0;  // the first vote of the large round is staged last
    if (check(ids, table)) return 1;
    QcRoundGroups g;
    qc_round_number(66, ids.data(), g);
    if (g.K != 2 || g.ids[0] != 7 || g.ids[1] != 3 || g.cnt[0] != 65 || g.cnt[1] != 1) return fail("65 + 1: numbering", 66);
    if (g.pos[40] != 0 || g.pos[39] != 39 || g.pos[41] != 40 || g.pos[65] != 64) return fail("65 + 1: positions", 66);
    std::vector<uint32_t> perm;
    for (uint32_t i = 1; i < 66; ++i) perm.push_back(i);
    perm.push_back(0);
    qc_round_stage(66, perm.data(), g);
    QcSegments s;
    qc_segments(66, g.K, g.gid.data(), s);
    if (s.chunks != 3 || s.seg[0] != 0 || s.seg[1] != 2 || s.seg[2] != 2 || s.seg[3] != 1) return fail("65 + 1: segments", 66);
    if (g.orig[65] != 0 || g.gid[65] != 0 || s.list[64] != 65 || s.list[128] != 39) return fail("65 + 1: staged", 66);
    ++cases;
  }
  printf("ok %u\n", cases);
  return 0;
}
