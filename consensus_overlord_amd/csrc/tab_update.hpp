// ovh_update_validators: the device side of a validator update that keeps
// what did not change. Included by ovhip.hip after qc.hpp (QC_NONE, the bit layout of k_qc_mark and
// QcRound's layout are the rounds'); the maps come from the host diff (tab_diff.hpp).
//
//   k_tab_build    lane per new entry: its 36 plane words and its flag word from the old table or
//                  from the slab of freshly checked keys into the new table
//   k_round_remap  the open rounds onto the new table's entry numbers and key order, through a
//                  table of per-round references: owner words, bitmap, then count, merged, R and
//                  the 96 bytes as they are; lost[r] when the round took a vote of a dropped key
// The kernels keep qc.hpp's rules: no workgroup waits for another, no scratch, plain loads and
// stores (no two lanes write one word, except the equal stores of `lost`).
#pragma once

// Entry i < n of `out` <- entry src[i] of `old`, or entry src[i] & ~TAB_NEW of `fresh`. Word k of
// coordinate j of entry i sits at p[(j * 12 + k) * cap + i]: consecutive lanes store consecutive
// words and, for the usual near-identity map, load consecutive words.
__global__ __launch_bounds__(WG) void k_tab_build(uint32_t n, const uint32_t* __restrict__ src, Slab old,
                                                  const uint32_t* __restrict__ old_flags, Slab fresh,
                                                  const uint32_t* __restrict__ fresh_flags, Slab out,
                                                  uint32_t* __restrict__ out_flags) {
  const uint32_t i = blockIdx.x * WG + threadIdx.x;
  if (i >= n) return;
  const uint32_t s = src[i];
  const bool nw = (s & TAB_NEW) != 0;
  const uint32_t e = s & ~TAB_NEW;
  const uint32_t* __restrict__ in = (nw ? fresh.p : old.p) + e;
  const size_t in_cap = nw ? fresh.cap : old.cap;
  uint32_t* o = out.p + i;
#pragma unroll 12
  for (uint32_t w = 0; w < 3 * 12; ++w) o[(size_t)w * out.cap] = in[(size_t)w * in_cap];
  out_flags[i] = (nw ? fresh_flags : old_flags)[e];
}

// One open round's old and new allocation (QcRound's layout on tn / bw of either table).
struct TabRoundRef {
  const uint32_t* old_dev;
  uint32_t* new_dev;
  uint32_t tn_old, bw_old, tn_new, bw_new;
};

// Round blockIdx.y of the table, lane per word. rsrc: new entry -> the old entry whose owner word
// it inherits, or QC_NONE; dst: old entry -> its new entry, or QC_NONE; sorted: rank -> new entry.
// A taken voter is an owner word other than QC_NONE, so the bitmap is rebuilt from the owner words
// in the new key order: bit k (byte k / 8, MSB first, bytes in little-endian words) is rank k's, a
// lane per word, pad bits 0.
__global__ __launch_bounds__(WG) void k_round_remap(const TabRoundRef* __restrict__ refs,
                                                    const uint32_t* __restrict__ rsrc, const uint32_t* __restrict__ dst,
                                                    const uint32_t* __restrict__ sorted, uint32_t* __restrict__ lost) {
  const TabRoundRef r = refs[blockIdx.y];
  const uint32_t i = blockIdx.x * WG + threadIdx.x;
  const uint32_t* __restrict__ oo = r.old_dev;  // the old owner words
  if (i < r.tn_new) {
    const uint32_t s = rsrc[i];
    r.new_dev[i] = s == QC_NONE ? QC_NONE : oo[s];
  }
  if (i < r.bw_new) {
    uint32_t w = 0;
    for (uint32_t b = 0; b < 32; ++b) {
      const uint32_t k = 32 * i + b;
      if (k >= r.tn_new) break;
      const uint32_t s = rsrc[sorted[k]];
      if (s != QC_NONE && oo[s] != QC_NONE) w |= 1u << (8 * ((k >> 3) & 3) + 7 - (k & 7));
    }
    r.new_dev[r.tn_new + i] = w;
  }
  if (i < 2) r.new_dev[r.tn_new + r.bw_new + i] = oo[r.tn_old + r.bw_old + i];  // count, merged
  if (i < 6 * 12 + 96 / 4) {  // R and the 96 bytes behind it
    const uint32_t fo = (r.tn_old + r.bw_old + 2 + 15) / 16 * 16, fn = (r.tn_new + r.bw_new + 2 + 15) / 16 * 16;
    r.new_dev[fn + i] = oo[fo + i];
  }
  if (i < r.tn_old && oo[i] != QC_NONE && dst[i] == QC_NONE) lost[blockIdx.y] = 1;
}
