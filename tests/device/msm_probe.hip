// Device probe for the unit-level tests of the G2 Pippenger MSM (tests/test_gpu_msm_buckets.py):
// the product's own MSM kernels (csrc/msm.hpp) and its own launch code (enqueue_msm_sort,
// enqueue_msm_trees, enqueue_msm of csrc/ovhip.hip) on buckets the caller chooses. Through the
// batch path a test cannot choose them: the digits come from SplitMix64. Test infrastructure
// only: built beside libovhip.so with the product's flags, never linked into it.
//
// The product translation unit is included whole, so Slab, VmDev, the LDS layout, the programs
// and ovh_create are the product's, with the product's code generation. The library is linked
// with -Bsymbolic: its copies of ovh_* and of the kernels bind inside it, whatever else the
// process has loaded.
//
// Every entry point takes host arrays and returns 0, a HIP error code, or an OVH_ERR_* of the
// product (100 and above); bad arguments are refused (hipErrorInvalidValue) without a launch.
// Field values are 12 words, canonical Montgomery limbs; a point is 4 of them (x.c0, x.c1, y.c0,
// y.c1), a projective result 6 (X.c0, X.c1, Y.c0, Y.c1, Z.c0, Z.c1). The context is created on
// the first call (device 0) and kept until mp_close.
#include "../../consensus_overlord_amd/csrc/ovhip.hip"

namespace {

constexpr int MP_BAD = (int)hipErrorInvalidValue;
constexpr uint32_t MP_NMAX = 1u << 16;  // votes per call: tests need a few hundred
constexpr int MP_SLOT = 0;

ovh_ctx* g_mp = nullptr;
std::mutex g_mp_mu;

// the probe's context with room for n votes; nullptr -> *err
ovh_ctx* mp_ctx(uint32_t n, int* err) {
  if (!g_mp) g_mp = ovh_create(0, nullptr, 0, 0);
  if (!g_mp) {
    *err = OVH_ERR_DEVICE;
    return nullptr;
  }
  *err = hipSetDevice(g_mp->device) == hipSuccess ? ensure_cap(g_mp, n) : OVH_ERR_DEVICE;
  return *err ? nullptr : g_mp;
}

struct Mp {
  hipStream_t st;
  hipError_t err = hipSuccess;
  explicit Mp(hipStream_t s) : st(s) {}
  void up(void* dst, const void* src, size_t bytes) {
    if (err == hipSuccess && bytes) err = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
  }
  void down(void* dst, const void* src, size_t bytes) {
    if (err == hipSuccess && bytes) err = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
  }
  // launch errors, then the kernels' own
  void sync() {
    if (err == hipSuccess) err = hipGetLastError();
    if (err == hipSuccess) err = hipStreamSynchronize(st);
  }
};

// n affine points (n x 4 x 12 words) -> the 4 planes from `plane` of the slot's state slab
void put_points(Mp& m, const Slab& s, uint32_t plane, uint32_t n, const uint32_t* pts, std::vector<uint32_t>& stage) {
  stage.assign((size_t)48 * n, 0u);
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t r = 0; r < 48; ++r) stage[(size_t)r * n + i] = pts[(size_t)i * 48 + r];
  if (m.err == hipSuccess)
    m.err = hipMemcpy2DAsync(s.p + (size_t)plane * 12 * s.cap, (size_t)s.cap * 4, stage.data(), (size_t)n * 4, (size_t)n * 4,
                             48, hipMemcpyHostToDevice, m.st);
}

// A and U of the slot filled with 0xFF words (values far above p, Z != 0): an entry that a run
// reads or returns without having written it cannot pass for a sum, nor for the identity
void poison(Mp& m, const MsmArgs& a) {
  if (m.err == hipSuccess) m.err = hipMemsetAsync(a.A.p, 0xFF, (size_t)72 * a.A.cap * 4, m.st);
  if (m.err == hipSuccess) m.err = hipMemsetAsync(a.U.p, 0xFF, (size_t)72 * MSM_U * 4, m.st);
}

// entry idx of a downloaded slab (6 planes x 12 limbs x cap) -> 72 words
void get_entry(uint32_t* out, const std::vector<uint32_t>& slab, uint32_t cap, uint32_t idx) {
  for (uint32_t r = 0; r < 72; ++r) out[r] = slab[(size_t)r * cap + idx];
}

}  // namespace

extern "C" {

// The product's sort half on n votes with RLC coefficients vote_scalar(seed, base, i) and the
// given codes: cnt (MSM_NB), off (MSM_NB + 1), pf (2 x (MSM_NB + 1)), ent (room for 8 n; the
// first off[MSM_NB] are written).
int mp_sort(uint32_t n, uint64_t seed, uint64_t base, const int32_t* codes, uint32_t* cnt, uint32_t* off, uint32_t* pf,
            uint32_t* ent) {
  if (n == 0 || n > MP_NMAX || !codes || !cnt || !off || !pf || !ent) return MP_BAD;
  std::lock_guard<std::mutex> g(g_mp_mu);
  int err = 0;
  ovh_ctx* c = mp_ctx(n, &err);
  if (!c) return err;
  uint32_t* cur;
  const MsmArgs a = msm_args(c, MP_SLOT, &cur);
  int32_t* dcodes = nullptr;
  if (hipMalloc(&dcodes, (size_t)n * 4) != hipSuccess) return OVH_ERR_DEVICE;
  Mp m(c->stream);
  m.up(dcodes, codes, (size_t)n * 4);
  if (m.err == hipSuccess) m.err = hipMemsetAsync((void*)a.ent, 0xFF, (size_t)8 * n * 4, m.st);
  if (m.err == hipSuccess) enqueue_msm_sort(m.st, a, cur, n, seed, base, dcodes);
  m.sync();
  m.down(cnt, a.cnt, (size_t)MSM_NB * 4);
  m.down(off, a.off, (size_t)(MSM_NB + 1) * 4);
  m.down(pf, a.pf, (size_t)MSM_PF_ROWS * (MSM_NB + 1) * 4);
  m.down(ent, a.ent, (size_t)8 * n * 4);
  m.sync();
  (void)hipFree(dcodes);
  return (int)m.err;
}

// The product's k_msm_scan and tree half on a caller-given histogram cnt (MSM_NB) and sorted
// entries ent (sum of cnt of them, bucket after bucket; point id 2 i + h, h = 1: tau of vote i;
// an id may occur any number of times) over the n points `sigma` and the n points `tau`. The
// product's bounds are required: at most 2 n entries in a bucket, 8 n in all. Outputs:
// buckets (MSM_NB x 72 words: A[pf[0][b]], zeros for an empty bucket), T (MSM_NT x 72: U[t TM]
// after the two k_msm_plane launches, from a run that stops there), S (72: U[0] of a whole run).
// A and U are poisoned before either run.
int mp_trees(uint32_t n, const uint32_t* sigma, const uint32_t* tau, const uint32_t* cnt, const uint32_t* ent,
             uint32_t* buckets, uint32_t* T, uint32_t* S) {
  if (n == 0 || n > MP_NMAX || !sigma || !tau || !cnt || !buckets || !T || !S) return MP_BAD;
  uint64_t total = 0;
  for (uint32_t b = 0; b < MSM_NB; ++b) {
    if (cnt[b] > 2ull * n) return MP_BAD;
    total += cnt[b];
  }
  if (total > 8ull * n || (total && !ent)) return MP_BAD;
  for (uint64_t k = 0; k < total; ++k)
    if (ent[k] >= 2ull * n) return MP_BAD;
  std::lock_guard<std::mutex> g(g_mp_mu);
  int err = 0;
  ovh_ctx* c = mp_ctx(n, &err);
  if (!c) return err;
  uint32_t* cur;
  const MsmArgs a = msm_args(c, MP_SLOT, &cur);
  Mp m(c->stream);
  std::vector<uint32_t> stage_s, stage_t;
  put_points(m, a.st, S_SIG, n, sigma, stage_s);
  put_points(m, a.st, S_TAU, n, tau, stage_t);
  m.up((void*)a.cnt, cnt, (size_t)MSM_NB * 4);
  m.up((void*)a.ent, ent, (size_t)total * 4);
  std::vector<uint32_t> hU((size_t)72 * MSM_U), hA((size_t)72 * a.A.cap), hpf(MSM_NB + 1);
  poison(m, a);
  if (m.err == hipSuccess) {
    k_msm_scan<<<1, 64, 0, m.st>>>(a.cnt, (uint32_t*)a.off, cur, (uint32_t*)a.pf);
    enqueue_msm_trees(c, m.st, a, n, false);
  }
  m.sync();
  m.down(hU.data(), a.U.p, hU.size() * 4);
  m.sync();
  if (m.err != hipSuccess) return (int)m.err;
  for (uint32_t t = 0; t < MSM_NT; ++t) get_entry(T + (size_t)72 * t, hU, MSM_U, t * MSM_TM);
  poison(m, a);
  if (m.err == hipSuccess) enqueue_msm_trees(c, m.st, a, n);
  m.sync();
  m.down(hU.data(), a.U.p, hU.size() * 4);
  m.down(hA.data(), a.A.p, hA.size() * 4);
  m.down(hpf.data(), a.pf, hpf.size() * 4);
  m.sync();
  if (m.err != hipSuccess) return (int)m.err;
  get_entry(S, hU, MSM_U, 0);
  for (uint32_t b = 0; b < MSM_NB; ++b) {
    uint32_t* o = buckets + (size_t)72 * b;
    if (cnt[b] && hpf[b] < a.A.cap) get_entry(o, hA, a.A.cap, hpf[b]);
    else memset(o, 0, 72 * 4);
  }
  return 0;
}

// The product's whole enqueue_msm on n votes: S (72 words) = sum over the votes with code 0 of
// [a_i] sigma_i + [b_i] tau_i, (a_i, b_i) the halves of vote_scalar(seed, base, i).
int mp_msm(uint32_t n, const uint32_t* sigma, const uint32_t* tau, uint64_t seed, uint64_t base, const int32_t* codes,
           uint32_t* S) {
  if (n == 0 || n > MP_NMAX || !sigma || !tau || !codes || !S) return MP_BAD;
  std::lock_guard<std::mutex> g(g_mp_mu);
  int err = 0;
  ovh_ctx* c = mp_ctx(n, &err);
  if (!c) return err;
  const Slab st{c->state_slot[MP_SLOT], c->cap};
  int32_t* dcodes = nullptr;
  if (hipMalloc(&dcodes, (size_t)n * 4) != hipSuccess) return OVH_ERR_DEVICE;
  Mp m(c->stream);
  std::vector<uint32_t> stage_s, stage_t, hU((size_t)72 * MSM_U);
  put_points(m, st, S_SIG, n, sigma, stage_s);
  put_points(m, st, S_TAU, n, tau, stage_t);
  m.up(dcodes, codes, (size_t)n * 4);
  uint32_t* cur;
  poison(m, msm_args(c, MP_SLOT, &cur));
  c->slot_seed[MP_SLOT] = seed;
  c->slot_base[MP_SLOT] = base;
  if (m.err == hipSuccess) err = enqueue_msm(c, m.st, MP_SLOT, n, dcodes);
  m.sync();
  m.down(hU.data(), msm_S(c, MP_SLOT).p, hU.size() * 4);
  m.sync();
  (void)hipFree(dcodes);
  if (m.err != hipSuccess) return (int)m.err;
  if (err) return err;
  get_entry(S, hU, MSM_U, 0);
  return 0;
}

// destroys the probe's context (the next call creates a new one)
void mp_close(void) {
  std::lock_guard<std::mutex> g(g_mp_mu);
  if (g_mp) ovh_destroy(g_mp);
  g_mp = nullptr;
}

}  // extern "C"
