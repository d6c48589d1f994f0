// Host build of the radix-2^392 ("wide") Montgomery product (csrc/bls/fp.hpp fp_mul_wide) and of
// the vote pool's constant-table renumbering (csrc/ovhip/pool_remap.hpp) for
// tests/test_fp_wide_host.py and tests/test_vote_radix.py. The interpreter itself runs through
// tests/host/harness.cpp (hx_vm_run: exec's default, per-phase radix). Test infrastructure only:
// never linked into the product library.
#include <stddef.h>
#include <stdint.h>

#include "../../consensus_overlord_amd/csrc/bls/fp.hpp"
#include "../../consensus_overlord_amd/csrc/ovhip/pool_remap.hpp"

using namespace ovh;

extern "C" {

// r[i] = a[i] b[i] 2^-392 mod p, 12 words per value (a, b < 4p)
void wx_fp_mul_wide(uint32_t n, const uint32_t* a, const uint32_t* b, uint32_t* r) {
  for (uint32_t i = 0; i < n; ++i) {
    Fp m;
    fp_mul_wide(m, fp_const(a + (size_t)i * 12), fp_const(b + (size_t)i * 12));
    for (int k = 0; k < 12; ++k) r[(size_t)i * 12 + k] = m.v[k];
  }
}

// the pool's table from the generated one (idx: VM_POOL_CONST_IDX)
void wx_pool_consts(uint32_t* out, const uint32_t* table, const uint16_t* idx, uint32_t npool) {
  pool::pool_const_words(out, table, idx, npool);
}

// a program's words renumbered to the pool's table; 0, or 1 + the first word naming a constant
// the pool table lacks
uint32_t wx_pool_remap(uint32_t* out, const uint32_t* code, size_t nwords, const uint16_t* idx, uint32_t npool) {
  return pool::pool_remap_code(out, code, nwords, idx, npool);
}

}
