// The host diff of ovh_update_validators: from the validator table's key
// list and a new one, what k_tab_build and k_round_remap (tab_update.hpp) need to carry the device
// table and the open rounds over. Pure host code, no HIP: included by ovhip.hip and, alone, by
// tests/host/tab_diff_harness.cpp.
//
// Duplicate keys follow the table's rule on either side: a lookup gives a key's first entry, and the
// stable sort puts that entry first among equal keys. So a round only ever holds owner words on
// first entries, and a first entry moves to a first entry.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

#define TAB_NEW 0x80000000u   // src: the key is not in the old table; the low bits number it
#define TAB_NONE 0xFFFFFFFFu  // dst / rsrc: no such entry (QC_NONE's value: an owner word reads the same)

struct TabDiff {
  bool same = false;  // same n, same bytes, same order: nothing else is filled in
  // per new entry: the old table's first entry of its key, or TAB_NEW | j -- the j-th distinct key
  // (by first appearance in the new list) that the old table does not hold
  std::vector<uint32_t> src;
  std::vector<uint32_t> fresh;  // new entry of the j-th such key (its first): the compacted upload
  // per old entry, as a round sees it: the first new entry of its key, or TAB_NONE
  std::vector<uint32_t> dst;
  // per new entry, as a round sees it: the old first entry of its key when this is the key's first
  // new entry, else TAB_NONE (a key new to the table, or a later duplicate, which nothing indexes)
  std::vector<uint32_t> rsrc;
  std::vector<uint32_t> sorted;  // new entries by key bytes, stable
  std::vector<uint32_t> rank;    // new entry -> its position in `sorted`
  uint32_t kept = 0;             // new entries whose point comes from the old table
};

// old_keys: ValidatorTable::keys (48 bytes each); pks: n x 48 bytes
static inline void tab_diff(const std::vector<std::string>& old_keys, const uint8_t* pks, size_t n, TabDiff& d) {
  d = TabDiff{};
  if (old_keys.size() == n) {
    size_t i = 0;
    while (i < n && memcmp(old_keys[i].data(), pks + 48 * i, 48) == 0) ++i;
    if (i == n) {
      d.same = true;
      return;
    }
  }
  std::vector<std::string> keys;
  keys.reserve(n);
  for (size_t i = 0; i < n; ++i) keys.emplace_back((const char*)pks + 48 * i, 48);
  std::unordered_map<std::string, uint32_t> old_first, new_first, fresh_no;
  for (size_t o = 0; o < old_keys.size(); ++o) old_first.emplace(old_keys[o], (uint32_t)o);  // keeps the first
  for (size_t i = 0; i < n; ++i) new_first.emplace(keys[i], (uint32_t)i);
  d.src.resize(n);
  d.rsrc.assign(n, TAB_NONE);
  for (size_t i = 0; i < n; ++i) {
    auto it = old_first.find(keys[i]);
    if (it != old_first.end()) {
      d.src[i] = it->second;
      ++d.kept;
      if (new_first[keys[i]] == i) d.rsrc[i] = it->second;
    } else {
      auto f = fresh_no.emplace(keys[i], (uint32_t)d.fresh.size());
      if (f.second) d.fresh.push_back((uint32_t)i);
      d.src[i] = TAB_NEW | f.first->second;
    }
  }
  d.dst.assign(old_keys.size(), TAB_NONE);
  for (size_t o = 0; o < old_keys.size(); ++o) {
    auto it = new_first.find(old_keys[o]);
    if (it != new_first.end()) d.dst[o] = it->second;
  }
  d.sorted.resize(n);
  for (size_t i = 0; i < n; ++i) d.sorted[i] = (uint32_t)i;
  std::stable_sort(d.sorted.begin(), d.sorted.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
  d.rank.resize(n);
  for (size_t k = 0; k < n; ++k) d.rank[d.sorted[k]] = (uint32_t)k;
}
