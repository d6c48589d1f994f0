// Round numbering of ovh_rounds_add: pure host code, no HIP
// (tests/host/round_groups_harness.cpp compiles it with g++ and the sanitizers).
//
// A call names one open round per vote. The distinct ids are numbered by first appearance in the
// caller's order; a vote's position is its index among the votes of its round in that call, in
// the caller's order (the claim of the selection is the round's base + that position, so a
// round's budget counts only its own votes). The batch stages its votes table-first (perm:
// staged vote j is the caller's vote perm[j]); qc_round_stage carries number and position into
// that order: gid is the group array of the selection and of the segment layout
// (qc_segments.hpp), orig the QcSel::orig of the call.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <unordered_map>
#include <vector>

struct QcRoundGroups {
  uint32_t K = 0;
  std::vector<uint64_t> ids;   // per number: the round's id
  std::vector<uint32_t> cnt;   // per number: its votes in this call
  std::vector<uint32_t> slot;  // per vote, caller's order: its round's number
  std::vector<uint32_t> pos;   // per vote, caller's order: its position among its round's votes
  std::vector<uint32_t> gid;   // per staged vote: slot[perm[j]]
  std::vector<uint32_t> orig;  // per staged vote: pos[perm[j]]
};

static inline void qc_round_number(size_t n, const uint64_t* rounds, QcRoundGroups& g) {
  std::unordered_map<uint64_t, uint32_t> num;
  g.ids.clear();
  g.cnt.clear();
  g.slot.resize(n);
  g.pos.resize(n);
  for (size_t i = 0; i < n; ++i) {
    auto it = num.find(rounds[i]);
    uint32_t k;
    if (it == num.end()) {
      k = (uint32_t)g.ids.size();
      num.emplace(rounds[i], k);
      g.ids.push_back(rounds[i]);
      g.cnt.push_back(0);
    } else {
      k = it->second;
    }
    g.slot[i] = k;
    g.pos[i] = g.cnt[k]++;
  }
  g.K = (uint32_t)g.ids.size();
}

// perm: n entries, or null for the identity (nothing was permuted)
static inline void qc_round_stage(size_t n, const uint32_t* perm, QcRoundGroups& g) {
  g.gid.resize(n);
  g.orig.resize(n);
  for (size_t j = 0; j < n; ++j) {
    const size_t i = perm ? perm[j] : j;
    g.gid[j] = g.slot[i];
    g.orig[j] = g.pos[i];
  }
}
