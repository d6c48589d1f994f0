// QC builder (ovh_build_qc): the leader's side of a round, enqueued behind the round's verify
// batch on its final stream. Included by ovhip.hip after msm.hpp (it reuses MsmArgs, msm_coord
// and msm_pair_op).
//
//   k_qc_reset   owner words to QC_NONE, bitmap words and the count to 0
//   k_qc_claim   lane per table vote with code 0: atomicMin(owner[table entry], caller's index)
//   k_qc_mark    lane per vote: taken iff it holds its voter's claim; bitmap bit (atomicOr), count
//   k_qc_chunk   masked G2 sum, tree levels 0 (madd of two affine sigma) to 5 (padd, in place)
//                of one 64-vote chunk per one-wave workgroup
//   k_qc_upper   the levels above, one workgroup over the chunk sums (loops over the pairs of a
//                level, so the launch count does not grow with log2 n)
// The sum reads the sigma planes the same-message vote program left in the state slab (affine,
// decompressed and subgroup-checked once); a vote that is not taken contributes the identity.
// The kernels keep the MSM kernels' rules: no workgroup waits for another, the levels of a
// tree hand over through the workgroup's own global lines behind __syncthreads(), one wave per
// workgroup, no scratch. The batch permutes votes table-first, so a vote's index in the caller's
// order (orig) decides between two votes of one voter, not its staged position.
#pragma once

#define QC_NONE 0xFFFFFFFFu

struct QcSel {
  const int32_t* codes;  // final per-vote codes, staged order
  const int32_t* tidx;   // table entry of staged vote j < t (first entry of a duplicate key)
  const uint32_t* orig;  // the caller's index of staged vote j (null: j)
  const uint32_t* rank;  // table entry -> its position in key-sorted order (the bitmap's bit)
  uint32_t* owner;       // per table entry: the lowest caller's index of a valid vote
  uint32_t* bitmap;      // MSB-first bytes, written as words
  uint32_t* count;
  uint32_t* taken;       // per staged vote: 1 or 0
};

__global__ __launch_bounds__(WG) void k_qc_reset(uint32_t tn, QcSel s) {
  const uint32_t e = blockIdx.x * WG + threadIdx.x;
  if (e < tn) s.owner[e] = QC_NONE;
  if (e < (tn + 31) / 32) s.bitmap[e] = 0;
  if (e == 0) *s.count = 0;
}

__global__ __launch_bounds__(WG) void k_qc_claim(uint32_t t, QcSel s) {
  const uint32_t j = blockIdx.x * WG + threadIdx.x;
  if (j < t && s.codes[j] == 0) atomicMin(&s.owner[s.tidx[j]], s.orig ? s.orig[j] : j);
}

__global__ __launch_bounds__(WG) void k_qc_mark(uint32_t n, uint32_t t, QcSel s) {
  const uint32_t j = blockIdx.x * WG + threadIdx.x;
  bool tk = false;
  if (j < t && s.codes[j] == 0) {
    const uint32_t e = (uint32_t)s.tidx[j];
    tk = s.owner[e] == (s.orig ? s.orig[j] : j);
    if (tk) {
      const uint32_t k = s.rank[e];  // bit k: byte k / 8, MSB first (little-endian words)
      atomicOr(&s.bitmap[k >> 5], 1u << (8 * ((k >> 3) & 3) + 7 - (k & 7)));
    }
  }
  if (j < n) s.taken[j] = tk ? 1u : 0u;
  const uint32_t c = (uint32_t)__popcll(__ballot(tk));
  if (threadIdx.x == 0 && c) atomicAdd(s.count, c);
}

// Levels 0 .. MSM_CH_LV - 1 of the masked sum: workgroup g owns votes 64 g .. 64 g + 63 and the
// entries A[32 g ..]; entry A[32 g + k / 2] (k even, within the chunk) holds the sum of votes
// k .. k + 2^(l+1) - 1 after level l. Level 0 is madd over the taken votes of a pair (the one
// taken vote and the identity, or -- none taken -- the identity written directly: madd's first
// operand is affine); the chunk's sum ends in A[32 g].
__global__ __launch_bounds__(64) void k_qc_chunk(uint32_t n, const uint32_t* __restrict__ taken, VmDev madd, VmDev padd,
                                                 uint32_t stride_w, const uint32_t* __restrict__ cst_g, MsmArgs a) {
  constexpr uint32_t W = VM_MADD_W, SL = 64 / W;
  MSM_VM_PROLOGUE(W);
  const uint32_t k0 = blockIdx.x << MSM_CH_LV, a0 = k0 >> 1;
  const uint32_t m = n - k0 < MSM_CH ? n - k0 : MSM_CH;  // the chunk's votes (>= 1)
  for (uint32_t lv = 0; lv < MSM_CH_LV && (lv == 0 || (1u << lv) < m); ++lv) {
    const uint32_t h = 1u << lv;
    const uint32_t np = lv == 0 ? (m + 1) / 2 : (m - h + 2 * h - 1) >> (lv + 1);
    const VmDev prog = msm_prog(lv == 0, madd, padd);
    for (uint32_t r = 0; r < np; r += SL) {
      const uint32_t p = r + slice, k = p << (lv + 1);
      bool act = p < np;
      uint32_t ka = SRC_A, ia = a0 + (k >> 1), kb = SRC_A, ib = a0 + ((k + h) >> 1);
      const uint32_t id = ia;
      if (lv == 0) {
        ka = SRC_PT, kb = SRC_ID, ia = ib = 0;
        if (act) {
          const uint32_t i0 = k0 + k, i1 = i0 + 1;
          const bool t0 = taken[i0] != 0, t1 = i1 < n && taken[i1] != 0;
          if (t0) {
            ia = 2 * i0;
            if (t1) kb = SRC_PT, ib = 2 * i1;
          } else if (t1) {
            ia = 2 * i1;
          } else {
            // ordered before the next level's loads by the pair op's barriers
            act = false;
            for (uint32_t c = lane; c < 6; c += W) {
              Fp v;
              if (c == 2) fp_one(v);
              else fp_zero(v);
              a.A.st(v, c, id);
            }
          }
        }
      }
      msm_pair_op<W>(prog, lv == 0 ? VM_MADD_NIN : VM_PADD_NIN, slots, cst, lane, act, a, ka, ia, kb, ib, SRC_A, id);
    }
  }
}

// Levels >= MSM_CH_LV: one workgroup adds the chunk sums (the entries of votes 64 j, A[32 j])
// level by level into A[0], eight pairs per run of the wave.
__global__ __launch_bounds__(64) void k_qc_upper(uint32_t n, VmDev padd, uint32_t stride_w,
                                                 const uint32_t* __restrict__ cst_g, MsmArgs a) {
  constexpr uint32_t W = VM_PADD_W, SL = 64 / W;
  MSM_VM_PROLOGUE(W);
  for (uint32_t lv = MSM_CH_LV; lv < 32 && (1u << lv) < n; ++lv) {
    const uint32_t h = 1u << lv, np = (n - h + 2 * h - 1) >> (lv + 1);
    for (uint32_t r = 0; r < np; r += SL) {
      const uint32_t p = r + slice, k = p << (lv + 1);
      const uint32_t ia = k >> 1, ib = (k + h) >> 1;
      msm_pair_op<W>(padd, VM_PADD_NIN, slots, cst, lane, p < np, a, SRC_A, ia, SRC_A, ib, SRC_A, ia);
    }
  }
}
