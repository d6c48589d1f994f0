// Pippenger MSM of the batch's sum r_i sigma_i in G2 (north_star: "Pippenger MSM for
// random-linear-combination batch verification, with buckets staged in LDS"; SURVEY.md
// Appendix C "sum r_i sigma_i G2 Pippenger share"). Included by ovhip.hip after the VM kernels.
//
// Scalars: the vote's 64-bit RLC value (a, b) stands for r = a + b lambda (lambda = -x^2), so
// r sigma = [a] sigma + [b] tau with tau = -psi^2(sigma) (the vote program stores both, affine).
// That is 2n points with 32-bit scalars, cut into four unsigned 8-bit windows: point p, window w,
// digit d = byte w of its scalar lands in bucket w * 255 + d - 1 (d = 0: nothing).
//
//   k_msm_count    lane per vote: bucket histogram in LDS, then one global add per bucket
//   k_msm_scan     one wave: bucket offsets, the prefix of the buckets' level-0 pair counts
//                  (where a bucket's tree lives in A) and of their chunk counts (k_msm_chunk's
//                  work list)
//   k_msm_scatter  lane per vote: point ids into their bucket's range (counting sort)
//   the VM pair kernels (8- or 16-lane slices, Fp-VM slots in LDS hold the operands), each
//   running several tree levels inside its one-wave workgroups:
//   k_msm_chunk    bucket tree levels 0 (madd, affine points) to 5 (padd, in place) of one
//                  64-entry chunk of a bucket
//   k_msm_upper    bucket tree levels >= 6 of one bucket (more than 64 points in it)
//   k_msm_plane    bit-plane sums T_t = sum of the buckets whose digit has bit t % 8 set
//   k_msm_comb     window combination sum_t 2^t T_t (hdbl<m>: A + [2^m] B)
// Buckets are summed as trees over the sorted entries (entry k of bucket b absorbs k + 2^l at
// level l), so a bucket of c points needs ceil(log2 c) levels and no sequential chain. Ten
// launches per batch (nine up to 32 votes); tests/test_msm_chunk_model.py restates which
// workgroup runs which pair.
#pragma once

#define MSM_NBW 255                 // buckets per window (digits 1..255)
#define MSM_NB (4 * MSM_NBW)        // buckets
#define MSM_NT 32                   // bit-plane targets: window w, bit k -> t = 8 w + k
#define MSM_TM 64                   // pairs of a target's level-0 sum (128 member buckets)
#define MSM_LV 27                   // bucket tree levels (2^26 >= 2 x 2^24 points in one bucket)
#define MSM_U (MSM_NT * MSM_TM)     // U plane entries
#define MSM_CH_LV 6                 // bucket tree levels that k_msm_chunk runs in one workgroup
#define MSM_CH (1u << MSM_CH_LV)    // entries of a chunk
#define MSM_PF_ROWS 2               // prefix rows: level-0 pairs, chunks

struct MsmArgs {
  const uint32_t* cnt;  // NB: points per bucket
  const uint32_t* off;  // NB + 1: first sorted entry of each bucket
  const uint32_t* pf;   // MSM_PF_ROWS x (NB + 1): prefix of the buckets' level-0 pairs, of their chunks
  const uint32_t* ent;  // sorted entries: point id 2 i + h (h = 1: tau of vote i)
  Slab st;              // vote state (sigma / tau planes)
  Slab A;               // bucket trees: entry k of bucket b (k even) at pf[0][b] + k / 2
  Slab U;               // bit-plane sums and window combination; U[0] = sum r_i sigma_i
};

__device__ __forceinline__ uint32_t msm_half(uint64_t r, uint32_t h) { return h ? (uint32_t)(r >> 32) : (uint32_t)r; }

// One-wave workgroups: beside two co-resident vote grids (two waves per SIMD everywhere) a
// workgroup of four or sixteen waves waits until that many slots free up on one CU -- r04w trace:
// the 256-thread count kernel averaged 0.59 ms and peaked at 8.7 ms there, holding up the final.
#define MSM_TPB 64

__global__ __launch_bounds__(MSM_TPB) void k_msm_zero(uint32_t* __restrict__ cnt) {
  const uint32_t k = blockIdx.x * MSM_TPB + threadIdx.x;
  if (k < MSM_NB) cnt[k] = 0;
}

__global__ __launch_bounds__(MSM_TPB) void k_msm_count(uint32_t n, uint64_t seed, uint64_t base,
                                                       const int32_t* __restrict__ codes, uint32_t* __restrict__ cnt) {
  __shared__ uint32_t h[MSM_NB];
  for (uint32_t k = threadIdx.x; k < MSM_NB; k += MSM_TPB) h[k] = 0;
  __syncthreads();
  const uint32_t i = blockIdx.x * MSM_TPB + threadIdx.x;
  if (i < n && codes[i] == 0) {  // failed votes contribute the identity
    const uint64_t r = vote_scalar(seed, base, i);
    for (uint32_t hh = 0; hh < 2; ++hh) {
      const uint32_t s = msm_half(r, hh);
      for (uint32_t w = 0; w < 4; ++w) {
        const uint32_t d = (s >> (8 * w)) & 255u;
        if (d) atomicAdd(&h[w * MSM_NBW + d - 1], 1u);
      }
    }
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < MSM_NB; k += MSM_TPB)
    if (h[k]) atomicAdd(&cnt[k], h[k]);
}

// Exclusive prefix over the MSM_NB values v(b) of one wave: lane t owns the 16 consecutive
// entries 16 t .. 16 t + 15 (MSM_NB <= 1024), scans them serially, and the lanes' sums are
// scanned across the wave (shuffles). out(b) = the prefix; returns the total (every lane).
template <class F, class G>
__device__ __forceinline__ uint32_t wave_scan_nb(F v, G out) {
  static_assert(MSM_NB <= 16 * 64, "16 entries per lane");
  const uint32_t t = threadIdx.x;
  uint32_t loc[16], sum = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const uint32_t b = 16 * t + j;
    loc[j] = b < MSM_NB ? v(b) : 0u;
    sum += loc[j];
  }
  uint32_t incl = sum;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t x = __shfl_up(incl, d, 64);
    if (t >= (uint32_t)d) incl += x;
  }
  uint32_t run = incl - sum;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const uint32_t b = 16 * t + j;
    if (b < MSM_NB) out(b, run);
    run += loc[j];
  }
  return __shfl(incl, 63, 64);
}

__global__ __launch_bounds__(64) void k_msm_scan(const uint32_t* __restrict__ cnt, uint32_t* __restrict__ off,
                                                 uint32_t* __restrict__ cur, uint32_t* __restrict__ pf) {
  const uint32_t tot = wave_scan_nb([&](uint32_t b) { return cnt[b]; },
                                    [&](uint32_t b, uint32_t e) {
                                      off[b] = e;
                                      cur[b] = e;
                                    });
  if (threadIdx.x == 0) off[MSM_NB] = tot;
  for (uint32_t row = 0; row < MSM_PF_ROWS; ++row) {
    // row 0: level-0 pairs, every even entry (its pair, or alone at a bucket's odd end);
    // row 1: chunks of MSM_CH entries
    uint32_t* p = pf + (size_t)row * (MSM_NB + 1);
    const uint32_t t = wave_scan_nb(
        [&](uint32_t b) {
          const uint32_t c = cnt[b];
          return row == 0 ? (c + 1) / 2 : (c + MSM_CH - 1) >> MSM_CH_LV;
        },
        [&](uint32_t b, uint32_t e) { p[b] = e; });
    if (threadIdx.x == 0) p[MSM_NB] = t;
  }
}

__global__ __launch_bounds__(MSM_TPB) void k_msm_scatter(uint32_t n, uint64_t seed, uint64_t base,
                                                         const int32_t* __restrict__ codes, uint32_t* __restrict__ cur,
                                                         uint32_t* __restrict__ ent) {
  const uint32_t i = blockIdx.x * MSM_TPB + threadIdx.x;
  if (i >= n || codes[i] != 0) return;
  const uint64_t r = vote_scalar(seed, base, i);
  for (uint32_t hh = 0; hh < 2; ++hh) {
    const uint32_t s = msm_half(r, hh);
    for (uint32_t w = 0; w < 4; ++w) {
      const uint32_t d = (s >> (8 * w)) & 255u;
      if (d) ent[atomicAdd(&cur[w * MSM_NBW + d - 1], 1u)] = 2 * i + hh;
    }
  }
}

// single-vote batch (UNIT_BASE): S = sigma (affine -> (x : y : 1)), or O if the vote failed
__global__ __launch_bounds__(64) void k_sig_as_S(Slab st, const int32_t* __restrict__ codes, Slab U) {
  const uint32_t c = threadIdx.x;
  if (c >= 6) return;
  Fp v;
  const bool ok = codes[0] == 0;
  if (ok && c < 4) st.ld(v, S_SIG + c, 0);
  else if (c == (ok ? 4u : 2u)) fp_one(v);
  else fp_zero(v);
  U.st(v, c, 0);
}

// operand source: identity, a vote's sigma / tau (affine, staged with Z = 1), A or U entry
enum : uint32_t { SRC_ID = 0, SRC_PT = 1, SRC_A = 2, SRC_U = 3 };

// bucket b with (pf[b] <= q < pf[b + 1]) in one level's prefix row (nondecreasing, pf[0] = 0)
__device__ __forceinline__ uint32_t msm_find(const uint32_t* __restrict__ row, uint32_t q) {
  uint32_t lo = 0, hi = MSM_NB;  // row[lo] <= q < row[hi]
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (row[mid] <= q) lo = mid;
    else hi = mid;
  }
  return lo;
}

// the j-th digit value (1..255) with bit k set (128 of them)
__device__ __forceinline__ uint32_t msm_member(uint32_t j, uint32_t k) {
  return ((j >> k) << (k + 1)) | (1u << k) | (j & ((1u << k) - 1));
}

// coordinate c (0..5, projective X0 X1 Y0 Y1 Z0 Z1) of an operand
__device__ __forceinline__ void msm_coord(Fp& v, const MsmArgs& a, uint32_t kind, uint32_t idx, uint32_t c) {
  if (kind == SRC_PT) {
    if (c < 4) a.st.ld(v, ((idx & 1) ? S_TAU : S_SIG) + c, idx >> 1);
    else if (c == 4) fp_one(v);
    else fp_zero(v);
  } else if (kind == SRC_A) {
    a.A.ld(v, c, idx);
  } else if (kind == SRC_U) {
    a.U.ld(v, c, idx);
  } else if (c == 2) {
    fp_one(v);  // (0 : 1 : 0)
  } else {
    fp_zero(v);
  }
}

// One pair add on the calling thread's W-lane slice: dst = A + B (madd / padd) or A + [2^m] B
// (hdbl<m>). Every thread of the workgroup calls it (the barriers); `active` marks the slices
// with a pair. The caller has loaded the constants; results go to global memory (canonical),
// and the closing __syncthreads() makes them the next level's operands within the workgroup
// (and keeps the next pair's staging behind this one's reads of the slots).
template <int W>
__device__ __forceinline__ void msm_pair_op(const VmDev& prog, uint32_t nin, uint32_t* slots, const uint32_t* cst,
                                            uint32_t lane, bool active, const MsmArgs& a, uint32_t ka, uint32_t ia,
                                            uint32_t kb, uint32_t ib, uint32_t kd, uint32_t id) {
  if (active) {
    // stage the operands: madd takes A affine (4 inputs) then B; the others A, B projective
    const uint32_t na = nin - 6;
    for (uint32_t k = lane; k < nin; k += W) {
      Fp v;
      if (k < na) msm_coord(v, a, ka, ia, k);
      else msm_coord(v, a, kb, ib, k - na);
      slot_put(slots, prog.in[k], v.v);
    }
  }
  __syncthreads();
  vm::run<false, false>(prog.code, prog.nphases, W, lane, active, slots, cst, 0, vm::Out{nullptr, 0, 0});
  if (active) {
    const Slab& d = kd == SRC_U ? a.U : a.A;
    for (uint32_t k = lane; k < 6; k += W) {
      Fp v;
      const uint32_t src = prog.out[k];
      for (int l = 0; l < 12; ++l) v.v[l] = slots[src * 12 + l];
      vm::canon(v, v);
      d.st(v, k, id);
    }
  }
  __syncthreads();
}

// the program of a level, picked field by field (kernel arguments stay in scalar registers)
__device__ __forceinline__ VmDev msm_prog(bool first, const VmDev& x, const VmDev& y) {
  VmDev r;
  r.code = first ? x.code : y.code;
  r.nphases = first ? x.nphases : y.nphases;
  r.in = first ? x.in : y.in;
  r.out = first ? x.out : y.out;
  r.trace = nullptr, r.clk = nullptr, r.side = nullptr;
  return r;
}

// The MSM's VM kernels are one-wave workgroups that own every entry they touch, so the levels
// of a tree run inside one launch: a level's results are written to the workgroup's own global
// lines, a __syncthreads() orders them before the next level's loads (one CU, one L1), and no
// workgroup ever waits for another. All of them run above the pool's waves (s_setprio 3 against
// 2, as k_vm_final): the MSM is the final stream's longest stretch beside the pool (r05y pool
// log: 1.7-2.9 ms against 0.67 alone). r05q: at 2 (with the final at 3) 1,432k verifs/s vs
// 1,131k-1,316k at 0; r05z: at 3, 1,389k-1,407k vs 1,378k-1,386k.
#define MSM_VM_PROLOGUE(W)                                    \
  __builtin_amdgcn_s_setprio(3);                              \
  extern __shared__ uint4 lds4[];                             \
  uint32_t* lds = reinterpret_cast<uint32_t*>(lds4);          \
  const uint32_t* cst = lds;                                  \
  const uint32_t slice = threadIdx.x / (W), lane = threadIdx.x % (W); \
  uint32_t* slots = lds + SLOT_BASE_W + slice * stride_w;     \
  load_consts(lds, cst_g, VM_NCONST)

// Bucket trees, levels 0 .. MSM_CH_LV - 1: workgroup g owns chunk j of bucket b (pfc[b] <= g <
// pfc[b + 1], j = g - pfc[b]), the bucket's entries 64 j .. 64 j + 63. Level 0 adds the points
// of an even entry and its successor (madd; alone at the bucket's odd end) into A, level l
// adds entry k + 2^l into entry k = j' 2^(l+1) (padd, in place): every pair of these levels
// lies inside one aligned chunk of 2^MSM_CH_LV entries. Eight pairs per run of the wave.
__global__ __launch_bounds__(64) void k_msm_chunk(VmDev madd, VmDev padd, uint32_t stride_w,
                                                  const uint32_t* __restrict__ cst_g, MsmArgs a) {
  constexpr uint32_t W = VM_MADD_W, SL = 64 / W;
  const uint32_t* rowc = a.pf + (MSM_NB + 1);
  if (blockIdx.x >= rowc[MSM_NB]) return;  // the grid is the worst case's
  MSM_VM_PROLOGUE(W);
  const uint32_t b = msm_find(rowc, blockIdx.x), k0 = (blockIdx.x - rowc[b]) << MSM_CH_LV;
  const uint32_t c = a.cnt[b], a0 = a.pf[b], e0 = a.off[b];
  const uint32_t m = c - k0 < MSM_CH ? c - k0 : MSM_CH;  // the chunk's entries (>= 1)
  for (uint32_t lv = 0; lv < MSM_CH_LV && (lv == 0 || (1u << lv) < m); ++lv) {
    const uint32_t h = 1u << lv;
    const uint32_t np = lv == 0 ? (m + 1) / 2 : (m - h + 2 * h - 1) >> (lv + 1);
    const VmDev prog = msm_prog(lv == 0, madd, padd);
    for (uint32_t r = 0; r < np; r += SL) {
      const uint32_t p = r + slice, k = k0 + (p << (lv + 1));
      const bool act = p < np;
      uint32_t ka = SRC_A, ia = a0 + (k >> 1), kb = SRC_A, ib = a0 + ((k + h) >> 1);
      const uint32_t id = ia;
      if (lv == 0) {
        ka = SRC_PT, kb = SRC_ID, ia = ib = 0;
        if (act) {
          ia = a.ent[e0 + k];
          if (k + 1 < c) kb = SRC_PT, ib = a.ent[e0 + k + 1];
        }
      }
      msm_pair_op<W>(prog, lv == 0 ? VM_MADD_NIN : VM_PADD_NIN, slots, cst, lane, act, a, ka, ia, kb, ib, SRC_A, id);
    }
  }
}

// Bucket trees, levels >= MSM_CH_LV: workgroup b owns bucket b and adds its chunks' sums
// (entries 64 j) level by level; a bucket of one chunk (every bucket of a batch whose RLC
// digits spread evenly, up to ~6,000 votes) exits at once, so a level without live pairs costs
// nothing anywhere.
__global__ __launch_bounds__(64) void k_msm_upper(VmDev padd, uint32_t stride_w, const uint32_t* __restrict__ cst_g,
                                                  MsmArgs a) {
  constexpr uint32_t W = VM_PADD_W, SL = 64 / W;
  const uint32_t c = a.cnt[blockIdx.x];
  if (c <= MSM_CH) return;
  MSM_VM_PROLOGUE(W);
  const uint32_t a0 = a.pf[blockIdx.x];
  for (uint32_t lv = MSM_CH_LV; (1u << lv) < c; ++lv) {
    const uint32_t h = 1u << lv, np = (c - h + 2 * h - 1) >> (lv + 1);
    for (uint32_t r = 0; r < np; r += SL) {
      const uint32_t p = r + slice, k = p << (lv + 1);
      const uint32_t ia = a0 + (k >> 1), ib = a0 + ((k + h) >> 1);
      msm_pair_op<W>(padd, VM_PADD_NIN, slots, cst, lane, p < np, a, SRC_A, ia, SRC_A, ib, SRC_A, ia);
    }
  }
}

// Bit-plane sums, levels lo .. hi of the 32 fixed 128-leaf trees (level 0: pairs of member
// buckets into U; level l: U[e] += U[e + 2^(l-1)], e = t TM + (i << l)): workgroup g owns the
// 2^hi level-0 pairs g 2^hi .. of target t = g / (TM >> hi), i.e. the (G >> l) pairs
// i = (g % (TM >> hi)) (G >> l) + p of level l. Two launches (0 .. 3 on 256 workgroups, 4 .. 6
// on 32) are seven runs deep; one workgroup per tree would be eighteen.
__global__ __launch_bounds__(64) void k_msm_plane(uint32_t lo, uint32_t hi, VmDev padd, uint32_t stride_w,
                                                  const uint32_t* __restrict__ cst_g, MsmArgs a) {
  constexpr uint32_t W = VM_PADD_W, SL = 64 / W;
  MSM_VM_PROLOGUE(W);
  const uint32_t per_t = MSM_TM >> hi, t = blockIdx.x / per_t, g = blockIdx.x % per_t;
  for (uint32_t lv = lo; lv <= hi; ++lv) {
    const uint32_t np = 1u << (hi - lv);
    for (uint32_t r = 0; r < np; r += SL) {
      const uint32_t p = r + slice, i = g * np + p;
      const bool act = p < np;
      uint32_t ka = SRC_U, ia = t * MSM_TM + (i << lv), kb = SRC_U, ib = ia + (lv ? 1u << (lv - 1) : 0u);
      const uint32_t id = ia;
      if (lv == 0) {
        ka = kb = SRC_ID, ia = ib = 0;
        if (act) {
          const uint32_t w = t >> 3, k = t & 7;
          const uint32_t b0 = w * MSM_NBW + msm_member(2 * i, k) - 1, b1 = w * MSM_NBW + msm_member(2 * i + 1, k) - 1;
          if (a.cnt[b0]) ka = SRC_A, ia = a.pf[b0];
          if (a.cnt[b1]) kb = SRC_A, ib = a.pf[b1];
        }
      }
      msm_pair_op<W>(padd, VM_PADD_NIN, slots, cst, lane, act, a, ka, ia, kb, ib, SRC_U, id);
    }
  }
}

// Window combination sum_t 2^t T_t, levels lo .. hi (<= lo + 2) of U[2 m q TM] += [2^m] U[(2 m q
// + m) TM], m = 2^(h-1) (programs hdbl<m>: p0 is level lo's): workgroup g owns the targets
// g 2^hi .., i.e. the 2^(hi-h) pairs q = g 2^(hi-h) + p of level h.
__global__ __launch_bounds__(64) void k_msm_comb(uint32_t lo, uint32_t hi, VmDev p0, VmDev p1, VmDev p2,
                                                 uint32_t stride_w, const uint32_t* __restrict__ cst_g, MsmArgs a) {
  constexpr uint32_t W = VM_HDBL1_W, SL = 64 / W;
  MSM_VM_PROLOGUE(W);
  for (uint32_t h = lo; h <= hi; ++h) {
    const VmDev prog = msm_prog(h == lo, p0, msm_prog(h == lo + 1, p1, p2));
    const uint32_t np = 1u << (hi - h), m = 1u << (h - 1);
    for (uint32_t r = 0; r < np; r += SL) {
      const uint32_t p = r + slice, e = 2 * m * (blockIdx.x * np + p) * MSM_TM;
      msm_pair_op<W>(prog, VM_HDBL1_NIN, slots, cst, lane, p < np, a, SRC_U, e, SRC_U, e + m * MSM_TM, SRC_U, e);
    }
  }
}
