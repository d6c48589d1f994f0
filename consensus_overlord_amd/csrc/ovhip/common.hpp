// What every kernel of the unit shares: the SoA Slab and the per-vote state planes, the RLC scalars,
// k_vote_digest and k_h2f, VmDev and ClockStamp, the LDS layout with its slot helpers and vm_lds,
// fold_unit, vote_stagger and PkSrc. Relies only on what ovhip.hip includes ahead of it (bls/,
// fpvm.hpp, the generated vm_progs.inc).
// A fragment of ovhip.hip, included there once and in order: not a header to include elsewhere.

// ------------------------------------------------------------------------ SoA helpers
struct Slab {
  uint32_t* p;
  uint32_t cap;
  __device__ __forceinline__ void ld(Fp& a, uint32_t j, uint32_t i) const {
    const uint32_t* b = p + (size_t)j * 12 * cap + i;
#pragma unroll
    for (int k = 0; k < 12; ++k) a.v[k] = b[(size_t)k * cap];
  }
  __device__ __forceinline__ void st(const Fp& a, uint32_t j, uint32_t i) const {
    uint32_t* b = p + (size_t)j * 12 * cap + i;
#pragma unroll
    for (int k = 0; k < 12; ++k) b[(size_t)k * cap] = a.v[k];
  }
  __device__ void ld2(Fp2& a, uint32_t j, uint32_t i) const {
    ld(a.c0, j, i);
    ld(a.c1, j + 1, i);
  }
  __device__ void st2(const Fp2& a, uint32_t j, uint32_t i) const {
    st(a.c0, j, i);
    st(a.c1, j + 1, i);
  }
  __device__ void ld_g2j(G2J& a, uint32_t i) const {
    ld2(a.X, 0, i);
    ld2(a.Y, 2, i);
    ld2(a.Z, 4, i);
  }
  __device__ void st_g2j(const G2J& a, uint32_t i) const {
    st2(a.X, 0, i);
    st2(a.Y, 2, i);
    st2(a.Z, 4, i);
  }
  __device__ void ld_g2a(G2A& a, uint32_t i) const {
    ld2(a.x, 0, i);
    ld2(a.y, 2, i);
  }
  __device__ void st_g2a(const G2A& a, uint32_t i) const {
    st2(a.x, 0, i);
    st2(a.y, 2, i);
  }
  __device__ void ld_g1a(G1A& a, uint32_t i) const {
    ld(a.x, 0, i);
    ld(a.y, 1, i);
  }
  __device__ void st_g1a(const G1A& a, uint32_t i) const {
    st(a.x, 0, i);
    st(a.y, 1, i);
  }
  __device__ void ld_f12(Fp12& f, uint32_t i) const {
    Fp* c = &f.c0.c0.c0;
    for (int j = 0; j < 12; ++j) ld(c[j], j, i);
  }
  __device__ void st_f12(const Fp12& f, uint32_t i) const {
    const Fp* c = &f.c0.c0.c0;
    for (int j = 0; j < 12; ++j) st(c[j], j, i);
  }
};

// Fp planes of the per-vote state slab.
enum : uint32_t {
  S_U = VM_S_U,       // 4 planes: u0, u1 (hash_to_field, Montgomery)
  S_SIG = VM_S_SIG,   // 4 planes: sigma (affine)
  S_TAU = VM_S_TAU,   // 4 planes: tau = -psi^2(sigma) (affine)
  S_F = VM_S_F,       // 12 planes: f = Miller(r pk, H)
  S_RS = VM_S_RS,     // 6 planes: r * sig (projective; bisection only, k_vm_rs)
  S_TOTAL = VM_S_TOTAL,
};
// partial = (F: 12 planes, S: 6 planes)
constexpr uint32_t PART_PLANES = 18;
// words per fin region: 16 unpacked + 4 folded partials as planes
constexpr size_t FIN_STRIDE = (size_t)PART_PLANES * 12 * 20;

enum : int { ST_H2F = 0, ST_VOTE, ST_FOLD, ST_FINAL, ST_FALLBACK, ST_MSM };
static_assert(ST_MSM + 1 == OVH_NSTAGES, "stage table");

__device__ __forceinline__ uint64_t rlc_scalar(uint64_t seed, uint64_t i) {
  // SplitMix64 on (seed, i): the 64-bit RLC coefficient of vote i (never 0). The seed is a
  // fresh secret per batch (getrandom, host side), so the coefficients are unpredictable.
  uint64_t z = seed + 0x9e3779b97f4a7c15ull * (i + 1);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  z = z ^ (z >> 31);
  return z ? z : 1;
}

// A batch of one vote checks its own pairing equation, e(pk, H) e(-G1, sigma) = 1: no random
// coefficient is needed, so its scalar is 1 (base UNIT_BASE) and the "MSM" is sigma itself
// (k_sig_as_S), which saves the MSM's launches on the per-call path (ovh_verify).
#define UNIT_BASE 0xFFFFFFFFFFFFFFFFull
__device__ __forceinline__ uint64_t vote_scalar(uint64_t seed, uint64_t base, uint64_t i) {
  return base == UNIT_BASE ? 1ull : rlc_scalar(seed, base + i);
}

// ------------------------------------------------------------------------ kernels
// Vote digests (ovh_vote_digests*): lane per vote, rlp(Vote) + SM3 (rlp.hpp, sm3.hpp).
__global__ __launch_bounds__(WG) void k_vote_digest(uint32_t n, const uint64_t* __restrict__ heights,
                                                    const uint64_t* __restrict__ rounds,
                                                    const uint8_t* __restrict__ types, const uint8_t* __restrict__ bh,
                                                    const uint8_t* __restrict__ lens, uint8_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * WG + threadIdx.x;
  if (i >= n) return;
  uint8_t h[VOTE_HASH_MAX];
  const uint32_t len = lens[i];
  uint8_t d[32];
  if (len > VOTE_HASH_MAX) {
    // lengths live in device memory (ovh_vote_digests_device cannot reject them on the host):
    // an over-long block hash gets the all-zero digest, which no vote hash equals
    for (int k = 0; k < 32; ++k) out[(size_t)i * 32 + k] = 0;
    return;
  }
  for (uint32_t k = 0; k < len; ++k) h[k] = bh[(size_t)i * VOTE_HASH_MAX + k];
  vote_digest(d, heights[i], rounds[i], types[i], h, len);
  for (int k = 0; k < 32; ++k) out[(size_t)i * 32 + k] = d[k];
}

__global__ __launch_bounds__(WG) void k_h2f(uint32_t n, const uint8_t* __restrict__ hashes, XmdTemplates t, Slab s) {
  const uint32_t i = blockIdx.x * WG + threadIdx.x;
  if (i >= n) return;
  uint32_t msg[8], uni[64];
  be_words_from_bytes(msg, hashes + (size_t)i * 32, 8);
  expand_message_xmd_256(uni, msg, t);
  Fp2 u0, u1;
  hash_to_field_fp2x2(u0, u1, uni);
  s.st2(u0, S_U, i);
  s.st2(u1, S_U + 2, i);
}

// ZCash header of a compressed point without decompression (the VM program decompresses):
// bad = BAD_ENCODING, inf = valid infinity encoding, x = masked plain limbs (x1 for G2).
__device__ void parse_hdr(const uint8_t* b, uint32_t nbytes, uint32_t* x_hi, uint32_t* x_lo, uint32_t& bad,
                          uint32_t& inf, uint32_t& sort, uint32_t& xzero) {
  const uint8_t b0 = b[0];
  bad = 0;
  inf = 0;
  sort = (b0 >> 5) & 1u;
  xzero = 0;
  uint8_t t[48];
  for (int i = 0; i < 48; ++i) t[i] = b[i];
  t[0] &= 0x1f;
  limbs_from_be48(x_hi, t);
  if (nbytes == 96) limbs_from_be48(x_lo, b + 48);
  if (!(b0 & 0x80)) {
    bad = 1;
    return;
  }
  if (b0 & 0x40) {
    uint32_t acc = b0 & 0x3f;
    for (uint32_t i = 1; i < nbytes; ++i) acc |= b[i];
    if (acc) bad = 1;
    else inf = 1;
    return;
  }
  if (!limbs_lt_p(x_hi)) bad = 1;
  if (nbytes == 96 && !limbs_lt_p(x_lo)) bad = 1;
  uint32_t z = 0;
  for (int k = 0; k < 12; ++k) z |= x_hi[k] | (nbytes == 96 ? x_lo[k] : 0u);
  xzero = z == 0;
}

struct VmDev {  // a program in device memory
  const uint4* code;
  uint32_t nphases;
  const uint16_t* in;   // device copies of the slot maps
  const uint16_t* out;
  uint64_t* trace;  // OVH_FLAG_VM_TRACE: nphases + 1 timestamps of workgroup 0, else null
  uint64_t* clk;    // OVH_FLAG_VM_CLOCK (vote / vote_t): per workgroup (d memtime, d realtime), else null
  const uint32_t* side;  // spilled programs (vote / vote_t): per-lane side words (fpvm.hpp run), else null
};
// per-vote scratch of the spilled vote programs (tools/fpvm/gen.py SPILL_K): entries of 12 words
constexpr uint32_t VOTE_NSCR = VM_VOTE_NSCR > VM_VOTE_T_NSCR ? VM_VOTE_NSCR : VM_VOTE_T_NSCR;

// OVH_FLAG_VM_CLOCK: shader-cycle and 100 MHz stamps around a workgroup's program (diagnostic
// runs of the measurement only; a null pointer executes no stamp). Capacity: VM_CLOCK_WGS
// workgroups of one launch.
#define VM_CLOCK_WGS (1u << 16)
struct ClockStamp {
  uint64_t t0 = 0, r0 = 0;
  __device__ __forceinline__ void begin(const uint64_t* clk) {
    if (clk && threadIdx.x == 0) {
      t0 = __builtin_amdgcn_s_memtime();
      r0 = __builtin_amdgcn_s_memrealtime();
    }
  }
  __device__ __forceinline__ void end(uint64_t* clk) {
    if (clk && threadIdx.x == 0 && blockIdx.x < VM_CLOCK_WGS) {
      const uint64_t t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
      clk[2 * blockIdx.x] = t1 - t0;
      clk[2 * blockIdx.x + 1] = r1 - r0;
    }
  }
};

// Batches of at most SMALL_MAX votes (one vote per wave: 1,024 waves fill the chip's SIMDs)
// take the small-batch path: votew per vote, fold, one final exponentiation (verify_small_locked).
#ifndef SMALL_MAX
#define SMALL_MAX 1024u
#endif
#define VM_SLICES 4  // 16-lane slices per 64-lane workgroup (vote, vote_t)
// LDS layout of the VM kernels (words): the constant table, then slot regions that start on a
// 128-byte boundary and repeat at 128-byte strides, so slot s and constant c share LDS banks
// exactly when s = c (mod 8) -- the rule tools/fpvm/sched.py spreads operand reads by.
constexpr uint32_t align128w(uint32_t w) { return (w + 31) / 32 * 32; }
// 256-byte alignment (one LDS row of 64 banks): slot s of every slice and constant c then sit in
// bank groups (3 s) and (3 c) mod 16 -- the model tools/fpvm/sched.py allocates slots by. A
// ds_read_b128 lane group of a 16-lane program spans two slices ({0-3,12-15} of one and {4-11}
// of the next), which only share that model when the slice stride is a multiple of 256 B.
constexpr uint32_t align256w(uint32_t w) { return (w + 63) / 64 * 64; }
constexpr uint32_t SLOT_BASE_W = align256w(VM_NCONST * 12);
constexpr uint32_t VOTE_STRIDE_W = align256w(VM_VOTE_NSLOTS * 12 + 4);  // + 4 header words
constexpr uint32_t VOTE_T_STRIDE_W = align256w(VM_VOTE_T_NSLOTS * 12 + 4);
constexpr uint32_t FOLD_STRIDE_W = align128w(VM_FOLD_NSLOTS * 12);
#define VM_FOLD_UNITS (64 / VM_FOLD_W)  // fold units per 64-lane workgroup

__device__ __forceinline__ void load_consts(uint32_t* cst, const uint32_t* __restrict__ g, uint32_t n) {
  for (uint32_t k = threadIdx.x; k < n * 12; k += blockDim.x) cst[k] = g[k];
}

__device__ __forceinline__ void slot_flag(uint32_t* slots, uint32_t s, uint32_t f) {
  uint4* d = reinterpret_cast<uint4*>(slots + s * 12);
  d[0] = make_uint4(f, 0, 0, 0);
  d[1] = make_uint4(0, 0, 0, 0);
  d[2] = make_uint4(0, 0, 0, 0);
}

__device__ __forceinline__ void slot_put(uint32_t* slots, uint32_t s, const uint32_t* v) {
  for (int k = 0; k < 12; ++k) slots[s * 12 + k] = v[k];
}

__device__ __forceinline__ uint32_t slot_flag_get(const uint32_t* slots, uint32_t s) { return slots[s * 12]; }

// Slot s as a canonical Fp: slots hold [0, 2p) representatives (fpvm.hpp); HBM planes are canonical.
__device__ __forceinline__ void slot_get_canon(const uint32_t* slots, uint32_t s, Fp& v) {
  for (int l = 0; l < 12; ++l) v.v[l] = slots[s * 12 + l];
  vm::canon(v, v);
}

// A VM kernel's dynamic LDS: the constant table, loaded here, and the slots of the unit that
// starts `off` words into the slot area. The kernels that still spell this out (rs, g1pairs, gmil,
// gfin, g2tree, pkgen, signg, g1tree, the MSM's) or the slot read above (g2tree, g1tree,
// msm_pair_op) compile to other code with the helper; they stay until a change may move it.
struct VmLds {
  uint32_t *cst, *slots;
};
__device__ __forceinline__ VmLds vm_lds(const uint32_t* __restrict__ cst_g, uint32_t off = 0) {
  extern __shared__ uint4 lds4[];
  uint32_t* lds = reinterpret_cast<uint32_t*>(lds4);
  load_consts(lds, cst_g, VM_NCONST);
  return {lds, lds + SLOT_BASE_W + off};
}

// One fold unit on a 16-lane slice: out[t] = (prod F, sum S) over in[4t .. 4t+3] (missing ->
// identity); with codes (level 0) every vote whose code is not 0 contributes the identity.
// inS.p null: every S is the identity (the batch path's S is the MSM's, msm.hpp).
// All 64 threads of the workgroup call it (the phase barrier); `active` marks the working slice.
template <int UNROLL = OVH_VM_UNROLL>
__device__ __forceinline__ void fold_unit(uint32_t t, uint32_t m, const VmDev& prog, const uint32_t* cst,
                                          uint32_t* slots, uint32_t lane, bool active, Slab inF, Slab inS,
                                          Slab out, const int32_t* __restrict__ codes) {
  if (active) {
    for (uint32_t k = lane; k < 4 * PART_PLANES; k += VM_FOLD_W) {
      const uint32_t q = k / PART_PLANES, j = k % PART_PLANES, e = 4 * t + q;
      Fp v;
      if (e < m && (!codes || codes[e] == 0) && (j < 12 || inS.p)) {
        if (j < 12) inF.ld(v, j, e);
        else inS.ld(v, j - 12, e);
      } else if (j == 0 || j == 12 + 2) {
        fp_one(v);
      } else {
        fp_zero(v);
      }
      slot_put(slots, VM_FOLD_IN[k], v.v);
    }
  }
  __syncthreads();
  VM_ASSERT_NO_INV(FOLD);
  vm::run<false, false, UNROLL>(prog.code, VM_FOLD_NPHASES, VM_FOLD_W, lane, active, slots, cst, 0,
                                vm::Out{nullptr, 0, 0});
  if (active) {
    for (uint32_t k = lane; k < PART_PLANES; k += VM_FOLD_W) {
      Fp v;
      slot_get_canon(slots, VM_FOLD_OUT[k], v);
      out.st(v, k, t);
    }
  }
}

// The vote waves of a CU run the same program in near lockstep, so every phase's operand loads
// (12 KB per wave) reach the CU's LDS at the same moment. OVH_VOTE_STAGGER > 0 offsets the start
// of the wave on SIMD s by s x OVH_VOTE_STAGGER x 64 cycles (the offset persists: every wave's
// phases take equally long), spreading those bursts. r03k A/B: 6 / 12 / 24 each +0.8-1.2%
// verifs/s against 0 (profiles/r03k_stagger_ab.txt); 12 is the default.
#ifndef OVH_VOTE_STAGGER
#define OVH_VOTE_STAGGER 12
#endif
__device__ __forceinline__ void vote_stagger() {
#if OVH_VOTE_STAGGER > 0
  const uint32_t hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);  // HW_REG_HW_ID, all 32 bits
  const uint32_t n = ((hw >> 4) & 3) * OVH_VOTE_STAGGER;          // SIMD_ID
#pragma unroll 1
  for (uint32_t k = 0; k < n; ++k) __builtin_amdgcn_s_sleep(1);
#endif
}

// Public keys given as points (ovh_set_validators table, or a QC's aggregated key): planes
// X, Y, Z (homogeneous projective, Montgomery) of `cap` entries, plus per-entry flags.
#define PKF_PARSE 1u  // the 48 bytes did not parse -> "lose public key" (102)
#define PKF_INF 2u    // the point at infinity      -> BLST_PK_IS_INFINITY (6) at verify
#define PKF_GRP 4u    // not in G1                  -> BLST_POINT_NOT_IN_GROUP (3) at verify
struct PkSrc {
  const uint32_t* planes;
  uint32_t cap;
  const uint32_t* flags;
  const int32_t* idx;  // vote i uses entry idx[i] (null: entry i)
};
