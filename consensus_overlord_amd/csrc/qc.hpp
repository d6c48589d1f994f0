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
//   k_qc_compress the groups' sums to 96 bytes each (ovh_build_qcs)
//   k_qc_rinit   a round's running sum to the identity (ovh_round_open)
//   k_qc_merge   a round's running sum += one add's sum (ovh_round_add)
//   k_qc_claim_r / k_qc_mark_r / k_qc_merge_seg / k_qc_rgather / k_qc_rcompress
//                the same over the open rounds of one ovh_rounds_add call, through a table of
//                round references (QcRoundRef)
// The sum reads the sigma planes the same-message vote program left in the state slab (affine,
// decompressed and subgroup-checked once); a vote that is not taken contributes the identity.
// The kernels keep the MSM kernels' rules: no workgroup waits for another, the levels of a
// tree hand over through the workgroup's own global lines behind __syncthreads(), one wave per
// workgroup, no scratch. The batch permutes votes table-first, so a vote's index in the caller's
// order (orig) decides between two votes of one voter, not its staged position.
#pragma once

#define QC_NONE 0xFFFFFFFFu

// ovh_build_qcs runs the same kernels over the groups of a mixed-hash
// batch (one group per distinct hash): the selection indexes owner, bitmap and count by the
// vote's group, and the sum reads its votes through the host's segment list (qc_segments.hpp:
// a group's votes contiguous and padded to whole chunks), one k_qc_upper workgroup per group.
struct QcSel {
  const int32_t* codes;  // final per-vote codes, staged order
  const int32_t* tidx;   // table entry of staged vote j < t (first entry of a duplicate key)
  const uint32_t* orig;  // the caller's index of staged vote j (null: j)
  const uint32_t* rank;  // table entry -> its position in key-sorted order (the bitmap's bit)
  const uint32_t* gid;   // group of staged vote j (null: one group)
  uint32_t groups;       // owner[g * tn + e], bitmap[g * bw + word], count[g]
  uint32_t bw;           // bitmap words of a group: ceil(tn / 32)
  uint32_t* owner;       // per group and table entry: the lowest caller's index of a valid vote
  uint32_t* bitmap;      // MSB-first bytes, written as words
  uint32_t* count;
  uint32_t* taken;       // per staged vote: 1 or 0
  // ovh_round_add: the votes the round took in before this call. A claim is base + the caller's
  // index, so one of an earlier add (below base) beats every claim of this one, and the owner
  // words are not reset between adds. 0: a selection that stands alone.
  uint32_t base = 0;
};

__global__ __launch_bounds__(WG) void k_qc_reset(uint32_t tn, QcSel s) {
  const uint32_t e = blockIdx.x * WG + threadIdx.x;
  if (e < s.groups * tn) s.owner[e] = QC_NONE;
  if (e < s.groups * s.bw) s.bitmap[e] = 0;
  if (e < s.groups) s.count[e] = 0;
}

__global__ __launch_bounds__(WG) void k_qc_claim(uint32_t tn, uint32_t t, QcSel s) {
  const uint32_t j = blockIdx.x * WG + threadIdx.x;
  if (j < t && s.codes[j] == 0) {
    const uint32_t g = s.gid ? s.gid[j] : 0u;
    atomicMin(&s.owner[g * tn + (uint32_t)s.tidx[j]], s.base + (s.orig ? s.orig[j] : j));
  }
}

__global__ __launch_bounds__(WG) void k_qc_mark(uint32_t tn, uint32_t n, uint32_t t, QcSel s) {
  const uint32_t j = blockIdx.x * WG + threadIdx.x;
  bool tk = false;
  uint32_t g = 0;
  if (j < t && s.codes[j] == 0) {
    const uint32_t e = (uint32_t)s.tidx[j];
    if (s.gid) g = s.gid[j];
    tk = s.owner[g * tn + e] == s.base + (s.orig ? s.orig[j] : j);
    if (tk) {
      const uint32_t k = s.rank[e];  // bit k: byte k / 8, MSB first (little-endian words)
      atomicOr(&s.bitmap[g * s.bw + (k >> 5)], 1u << (8 * ((k >> 3) & 3) + 7 - (k & 7)));
    }
  }
  if (j < n) s.taken[j] = tk ? 1u : 0u;
  if (s.gid) {  // uniform
    if (tk) atomicAdd(&s.count[g], 1u);
  } else {
    const uint32_t c = (uint32_t)__popcll(__ballot(tk));
    if (threadIdx.x == 0 && c) atomicAdd(s.count, c);
  }
}

// Levels 0 .. MSM_CH_LV - 1 of the masked sum: workgroup g owns votes 64 g .. 64 g + 63 and the
// entries A[32 g ..]; entry A[32 g + k / 2] (k even, within the chunk) holds the sum of votes
// k .. k + 2^(l+1) - 1 after level l. Level 0 is madd over the taken votes of a pair (the one
// taken vote and the identity, or -- none taken -- the identity written directly: madd's first
// operand is affine); the chunk's sum ends in A[32 g].
// SEG: the chunk's votes are list[64 g ..] (staged indices, then QC_NONE pads to the chunk's end;
// at least one vote), so a chunk never holds votes of two groups.
template <bool SEG>
__global__ __launch_bounds__(64) void k_qc_chunk(uint32_t n, const uint32_t* __restrict__ taken,
                                                 const uint32_t* __restrict__ list, VmDev madd, VmDev padd,
                                                 uint32_t stride_w, const uint32_t* __restrict__ cst_g, MsmArgs a) {
  constexpr uint32_t W = VM_MADD_W, SL = 64 / W;
  const uint32_t k0 = blockIdx.x << MSM_CH_LV, a0 = k0 >> 1;
  uint32_t m;  // the chunk's votes (>= 1)
  if (SEG) m = (uint32_t)__popcll(__ballot(list[k0 + threadIdx.x] != QC_NONE));
  else m = n - k0 < MSM_CH ? n - k0 : MSM_CH;
  MSM_VM_PROLOGUE(W);
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
          const bool two = k + 1 < m;
          const uint32_t i0 = SEG ? list[k0 + k] : k0 + k, i1 = !two ? 0u : SEG ? list[k0 + k + 1] : i0 + 1;
          const bool t0 = taken[i0] != 0, t1 = two && taken[i1] != 0;
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
// SEG: workgroup g adds the chunk sums of group g (chunks seg[2 g] .. + seg[2 g + 1] - 1, whole
// chunks: the levels above a chunk see 64 votes in each) into the first entry of its segment.
template <bool SEG>
__global__ __launch_bounds__(64) void k_qc_upper(uint32_t n, const uint32_t* __restrict__ seg, VmDev padd,
                                                 uint32_t stride_w, const uint32_t* __restrict__ cst_g, MsmArgs a) {
  constexpr uint32_t W = VM_PADD_W, SL = 64 / W;
  uint32_t a0 = 0;
  if (SEG) {
    n = seg[2 * blockIdx.x + 1] << MSM_CH_LV;
    if (n <= MSM_CH) return;  // one chunk: its sum is the group's
    a0 = seg[2 * blockIdx.x] << (MSM_CH_LV - 1);
  }
  MSM_VM_PROLOGUE(W);
  for (uint32_t lv = MSM_CH_LV; lv < 32 && (1u << lv) < n; ++lv) {
    const uint32_t h = 1u << lv, np = (n - h + 2 * h - 1) >> (lv + 1);
    for (uint32_t r = 0; r < np; r += SL) {
      const uint32_t p = r + slice, k = p << (lv + 1);
      const uint32_t ia = a0 + (k >> 1), ib = a0 + ((k + h) >> 1);
      msm_pair_op<W>(padd, VM_PADD_NIN, slots, cst, lane, p < np, a, SRC_A, ia, SRC_A, ib, SRC_A, ia);
    }
  }
}

// The groups' sums, projective (X : Y : Z) in the first entry of each segment -> 96-byte
// compressed (g2p_compress: one lane per group's workgroup, as k_g2p_compress)
__global__ __launch_bounds__(64) void k_qc_compress(Slab in, const uint32_t* __restrict__ seg, uint8_t* out) {
  if (threadIdx.x) return;
  g2p_compress(in, seg[2 * blockIdx.x] << (MSM_CH_LV - 1), out + 96 * (size_t)blockIdx.x);
}

// Rounds (ovh_round_open / _add / _qc). A round's state is one allocation:
// owner (tn words) | bitmap (bw) | count | merged, then -- from the next 16-word boundary -- the
// running sum R, a projective G2 point stored as a one-entry slab (72 words). `merged` is the
// count that R stands for: an add whose selection took nothing leaves count == merged.
__global__ __launch_bounds__(64) void k_qc_rinit(uint32_t* merged, Slab R) {
  const uint32_t c = threadIdx.x;
  if (c == 0) *merged = 0;
  if (c >= 6) return;
  Fp v;
  if (c == 2) fp_one(v);  // (0 : 1 : 0)
  else fp_zero(v);
  R.st(v, c, 0);
}

// R <- R + (this add's sum): a.U is the round's R (one entry), a.A[0] the sum that k_qc_chunk /
// k_qc_upper left in the slot's tree or, for an add of one vote, its sigma from k_vm_sigchk. One
// pair on the first slice of one one-wave workgroup. padd is the complete addition, which the merge needs:
// R is the identity until the first taken vote, the sums of two adds can be equal (a doubling) or
// opposite (the identity again), and none of these may take another path than the generic pair.
// The gate is here, not on the host: nothing is added when the add took no vote (`taken1`, the
// one vote's taken word, when the add has one vote; else the count against `merged`).
__global__ __launch_bounds__(64) void k_qc_merge(const uint32_t* __restrict__ count, uint32_t* merged,
                                                 const uint32_t* __restrict__ taken1, VmDev padd, uint32_t stride_w,
                                                 const uint32_t* __restrict__ cst_g, MsmArgs a) {
  constexpr uint32_t W = VM_PADD_W;
  const uint32_t cnt = *count;
  if (taken1 ? taken1[0] == 0 : cnt == *merged) return;  // uniform; merged is written behind the barriers below
  MSM_VM_PROLOGUE(W);
  msm_pair_op<W>(padd, VM_PADD_NIN, slots, cst, lane, slice == 0, a, SRC_U, 0, SRC_A, 0, SRC_U, 0);
  if (threadIdx.x == 0) *merged = cnt;
}

// ovh_rounds_add: one pass over votes that belong to several open rounds.
// Each round is an allocation of its own with a base of its own, so the call carries a device
// table of K <= OVH_ROUNDS_MAX references, staged with the rest of the plan; QcSel::gid is the
// vote's round number in the call (an index into the table, not the verify plan's hash group:
// two rounds may be open on one hash), QcSel::orig its position among its round's votes in the
// call. QcSel's owner / bitmap / count / groups / base are not read.
struct QcRoundRef {
  uint32_t* owner;
  uint32_t* bitmap;
  uint32_t* count;
  uint32_t* merged;
  uint32_t* R;    // the running sum, a one-entry slab
  uint32_t base;  // the votes the round took in before this call
  uint32_t pad;
};

__global__ __launch_bounds__(WG) void k_qc_claim_r(uint32_t t, QcSel s, const QcRoundRef* __restrict__ refs) {
  const uint32_t j = blockIdx.x * WG + threadIdx.x;
  if (j < t && s.codes[j] == 0) {
    const QcRoundRef& r = refs[s.gid[j]];
    atomicMin(&r.owner[(uint32_t)s.tidx[j]], r.base + s.orig[j]);
  }
}

__global__ __launch_bounds__(WG) void k_qc_mark_r(uint32_t n, uint32_t t, QcSel s, const QcRoundRef* __restrict__ refs) {
  const uint32_t j = blockIdx.x * WG + threadIdx.x;
  bool tk = false;
  if (j < t && s.codes[j] == 0) {
    const QcRoundRef& r = refs[s.gid[j]];
    const uint32_t e = (uint32_t)s.tidx[j];
    tk = r.owner[e] == r.base + s.orig[j];
    if (tk) {
      const uint32_t k = s.rank[e];
      atomicOr(&r.bitmap[k >> 5], 1u << (8 * ((k >> 3) & 3) + 7 - (k & 7)));
      atomicAdd(r.count, 1u);
    }
  }
  if (j < n) s.taken[j] = tk ? 1u : 0u;
}

// R_g <- R_g + (round g's sum of this call), workgroup g: k_qc_merge's body with R and the words
// from the table and the source entry from the segment table (k_qc_chunk<true> / k_qc_upper<true>
// leave round g's sum in A[32 seg[2 g]]). A round whose selection took nothing in this call has
// count == merged and its R is not touched.
__global__ __launch_bounds__(64) void k_qc_merge_seg(const QcRoundRef* __restrict__ refs, const uint32_t* __restrict__ seg,
                                                     VmDev padd, uint32_t stride_w, const uint32_t* __restrict__ cst_g,
                                                     MsmArgs a) {
  constexpr uint32_t W = VM_PADD_W;
  const QcRoundRef r = refs[blockIdx.x];
  const uint32_t cnt = *r.count;
  if (cnt == *r.merged) return;  // uniform; merged is written behind the barriers below
  a.U = Slab{r.R, 1};
  const uint32_t src = seg[2 * blockIdx.x] << (MSM_CH_LV - 1);
  MSM_VM_PROLOGUE(W);
  msm_pair_op<W>(padd, VM_PADD_NIN, slots, cst, lane, slice == 0, a, SRC_U, 0, SRC_A, src, SRC_U, 0);
  if (threadIdx.x == 0) *r.merged = cnt;
}

// Round g's count and bitmap words into the call's output rows (row g: count | bw bitmap words;
// bw 0: the count alone), so the host reads K rounds with one copy.
__global__ __launch_bounds__(64) void k_qc_rgather(const QcRoundRef* __restrict__ refs, uint32_t bw, uint32_t* out) {
  const QcRoundRef& r = refs[blockIdx.x];
  uint32_t* row = out + (size_t)blockIdx.x * (1 + bw);
  if (threadIdx.x == 0) row[0] = *r.count;
  for (uint32_t w = threadIdx.x; w < bw; w += 64) row[1 + w] = r.bitmap[w];
}

// Round g's R -> 96 bytes at out + 96 g (one lane, as k_qc_compress); an empty round is skipped
__global__ __launch_bounds__(64) void k_qc_rcompress(const QcRoundRef* __restrict__ refs, uint8_t* out) {
  if (threadIdx.x) return;
  const QcRoundRef& r = refs[blockIdx.x];
  if (*r.count == 0) return;
  g2p_compress(Slab{r.R, 1}, 0, out + 96 * (size_t)blockIdx.x);
}
