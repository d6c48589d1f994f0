// Stand-alone host program (g++ -fsanitize=address,undefined) over the host diff of
// ovh_update_validators (csrc/tab_diff.hpp) for tests/test_tab_diff_host.py. Reads the cases from
// the file named on the command line -- a count, then per case "n_old n_new" and that many keys of
// 96 hex digits, old list first -- checks every map against a brute-force O(n^2) restatement of its
// definition, and prints one line per case with the maps (for the comparison with
// tests/tab_model.py) and then "ok <cases>", or names the first property that fails. Test-only: never
// linked into the product.
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "../../consensus_overlord_amd/csrc/tab_diff.hpp"

namespace {
int fail(const char* what, size_t c) {
  printf("FAIL %s (case %zu)\n", what, c);
  return 1;
}

bool read_key(FILE* f, std::string& k) {
  char hex[97];
  if (fscanf(f, "%96s", hex) != 1 || strlen(hex) != 96) return false;
  k.assign(48, '\0');
  for (int i = 0; i < 48; ++i) {
    unsigned v;
    if (sscanf(hex + 2 * i, "%2x", &v) != 1) return false;
    k[i] = (char)v;
  }
  return true;
}

uint32_t first_of(const std::vector<std::string>& l, const std::string& k) {
  for (size_t i = 0; i < l.size(); ++i)
    if (l[i] == k) return (uint32_t)i;
  return TAB_NONE;
}

void line(const char* name, const std::vector<uint32_t>& v) {
  printf(" %s", name);
  for (uint32_t x : v) printf(" %u", x);
}

int check(size_t c, const std::vector<std::string>& old, const std::vector<std::string>& nw) {
  const size_t no = old.size(), n = nw.size();
  std::vector<uint8_t> flat(48 * n + 1);  // (+ 1: n == 0 still has a pointer to pass)
  for (size_t i = 0; i < n; ++i) memcpy(&flat[48 * i], nw[i].data(), 48);
  TabDiff d;
  tab_diff(old, flat.data(), n, d);
  if (d.same != (old == nw)) return fail("same", c);
  if (d.same) {
    if (!d.src.empty() || !d.dst.empty() || !d.sorted.empty()) return fail("same fills nothing in", c);
    printf("same\n");
    return 0;
  }
  if (d.src.size() != n || d.rsrc.size() != n || d.sorted.size() != n || d.rank.size() != n || d.dst.size() != no)
    return fail("sizes", c);
  // the compacted new keys: distinct, none in the old list, numbered by first appearance
  for (size_t j = 0; j < d.fresh.size(); ++j) {
    if (d.fresh[j] >= n || first_of(nw, nw[d.fresh[j]]) != d.fresh[j]) return fail("fresh names a first entry", c);
    if (first_of(old, nw[d.fresh[j]]) != TAB_NONE) return fail("fresh key is in the old list", c);
    if (j && d.fresh[j - 1] >= d.fresh[j]) return fail("fresh by first appearance", c);
  }
  uint32_t kept = 0, fresh_seen = 0;
  for (size_t i = 0; i < n; ++i) {
    const uint32_t o = first_of(old, nw[i]);
    const bool first = first_of(nw, nw[i]) == i;
    if (o != TAB_NONE) {
      ++kept;
      if (d.src[i] != o) return fail("src: the old first entry", c);
      if (d.rsrc[i] != (first ? o : TAB_NONE)) return fail("rsrc of a kept key", c);
    } else {
      if (!(d.src[i] & TAB_NEW)) return fail("src: TAB_NEW", c);
      const uint32_t j = d.src[i] & ~TAB_NEW;
      if (j >= d.fresh.size() || nw[d.fresh[j]] != nw[i]) return fail("src: the compacted key", c);
      if (first && j != fresh_seen++) return fail("src: numbering", c);
      if (d.rsrc[i] != TAB_NONE) return fail("rsrc of a new key", c);
    }
  }
  if (fresh_seen != d.fresh.size() || kept != d.kept) return fail("counts", c);
  for (size_t o = 0; o < no; ++o)
    if (d.dst[o] != first_of(nw, old[o])) return fail("dst: the new first entry", c);
  // the sorted order: a permutation, by key bytes, equal keys by entry number; rank its inverse
  std::vector<uint8_t> seen(n, 0);
  for (size_t k = 0; k < n; ++k) {
    const uint32_t e = d.sorted[k];
    if (e >= n || seen[e]++) return fail("sorted is a permutation", c);
    if (d.rank[e] != k) return fail("rank inverts sorted", c);
    if (k) {
      const uint32_t p = d.sorted[k - 1];
      if (nw[p] > nw[e] || (nw[p] == nw[e] && p > e)) return fail("sorted: stable by key bytes", c);
    }
  }
  // a rank counted the slow way: the keys below, and the equal keys in front
  for (size_t e = 0; e < n; ++e) {
    uint32_t r = 0;
    for (size_t x = 0; x < n; ++x) r += nw[x] < nw[e] || (nw[x] == nw[e] && x < e);
    if (d.rank[e] != r) return fail("rank by counting", c);
  }
  printf("diff");
  line("src", d.src);
  line("fresh", d.fresh);
  line("dst", d.dst);
  line("rsrc", d.rsrc);
  line("sorted", d.sorted);
  line("rank", d.rank);
  printf(" kept %u\n", d.kept);
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  FILE* f = argc == 2 ? fopen(argv[1], "r") : nullptr;
  if (!f) return fail("no case file", 0);
  size_t cases = 0;
  if (fscanf(f, "%zu", &cases) != 1) return fail("count", 0);
  for (size_t c = 0; c < cases; ++c) {
    size_t no, n;
    if (fscanf(f, "%zu %zu", &no, &n) != 2 || no > 4096 || n > 4096) return fail("case header", c);
    std::vector<std::string> old(no), nw(n);
    for (std::string& k : old)
      if (!read_key(f, k)) return fail("key", c);
    for (std::string& k : nw)
      if (!read_key(f, k)) return fail("key", c);
    if (check(c, old, nw)) return 1;
  }
  fclose(f);
  printf("ok %zu\n", cases);
  return 0;
}
