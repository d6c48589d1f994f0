// The vote pool's constant table and the renumbering of the programs it runs. Plain C++ (host
// code: ovhip.hip applies it when it uploads the programs, tests/host/fp_wide_harness.cpp runs it
// on the CPU), a pure function of the generated tables.
//
// The pool's workgroups keep a compact constant table in LDS -- the fixed entries, the radix-392
// entries of vote / vote_t and what the fused fold refers to: VM_POOL_NCONST entries, entry k =
// entry VM_POOL_CONST_IDX[k] of the generated table -- where every other kernel loads the table's
// radix-384 prefix (VM_NCONST entries). It is no larger than that prefix, so the pool's LDS layout
// (SLOT_BASE_W) is the other kernels'. The pool's copies of the three programs refer to it: every
// operand field of an instruction (two 16-bit halves of w1 and w2, tools/fpvm/sched.py) that
// names a constant (bit 11) is renumbered.
#pragma once
#include <stdint.h>

namespace ovh {
namespace pool {

constexpr uint32_t REF_CONST = 0x800;  // vm::CONST_BASE

// words [12 * k, 12 * k + 12) of `out` = entry idx[k] of `table`
inline void pool_const_words(uint32_t* out, const uint32_t* table, const uint16_t* idx, uint32_t npool) {
  for (uint32_t k = 0; k < npool; ++k)
    for (uint32_t j = 0; j < 12; ++j) out[12 * k + j] = table[12 * (uint32_t)idx[k] + j];
}

// `code` (nwords = phases x lanes x 4 words, table numbering) -> `out` in the pool table's
// numbering. Returns 0, or 1 + the index of the first word that names a constant the pool table
// lacks (the caller refuses to start: a missing constant is an error, never another entry).
inline uint32_t pool_remap_code(uint32_t* out, const uint32_t* code, size_t nwords, const uint16_t* idx,
                                uint32_t npool) {
  auto map = [&](uint32_t h, bool& bad) -> uint32_t {
    if (!(h & REF_CONST)) return h;
    const uint32_t c = h & (REF_CONST - 1);
    for (uint32_t k = 0; k < npool; ++k)
      if (idx[k] == c) return (h & ~(REF_CONST - 1)) | k;
    bad = true;
    return h;
  };
  for (size_t w = 0; w < nwords; ++w) {
    const uint32_t v = code[w];
    if ((w & 3) == 1 || (w & 3) == 2) {
      bool bad = false;
      out[w] = map(v & 0xFFFF, bad) | map(v >> 16, bad) << 16;
      if (bad) return (uint32_t)w + 1;
    } else {
      out[w] = v;
    }
  }
  return 0;
}

}  // namespace pool
}  // namespace ovh
