// Device probe for the unit-level arithmetic tests (tests/test_gpu_fp_bounds.py): the field
// primitives of csrc/bls/fp.hpp and csrc/fpvm.hpp, one thread per case, a runner for Fp-VM
// programs on one single-wave workgroup, and hash_to_field in the shape of the product's k_h2f
// (tests/test_gpu_h2c.py). Test infrastructure only: built beside libovhip.so with
// the product's flags (the product's code generation is what is under test), never linked into it.
//
// Every entry point takes host arrays (12 words per value), copies them to the device, launches
// one kernel, synchronises, copies the results back, frees the device memory and returns the
// HIP error code (0 on success). Bad arguments return an error without a launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../consensus_overlord_amd/csrc/bls/h2c.hpp"
#include "../../consensus_overlord_amd/csrc/fpvm.hpp"

using namespace ovh;

namespace {

__device__ __forceinline__ void ld12(Fp& r, const uint32_t* __restrict__ p, uint32_t i) {
#pragma unroll
  for (int k = 0; k < 12; ++k) r.v[k] = p[(size_t)i * 12 + k];
}
__device__ __forceinline__ void st12(uint32_t* __restrict__ p, uint32_t i, const Fp& v) {
#pragma unroll
  for (int k = 0; k < 12; ++k) p[(size_t)i * 12 + k] = v.v[k];
}

// VARIANT 0: ovh::fp_mul as the product library gets it; 1: fp_mul28_gfx950_2acc; 2: the portable
// fp_mul28; 3: fp_mul_gfx950. ALIAS: the same register array for both operands (b is not read).
template <int VARIANT, bool ALIAS>
__global__ __launch_bounds__(64) void k_fp_mul(uint32_t n, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                               uint32_t* __restrict__ r) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  Fp x, y, m;
  ld12(x, a, i);
  if (!ALIAS) ld12(y, b, i);
  const Fp& yy = ALIAS ? x : y;
  if (VARIANT == 0) fp_mul(m, x, yy);
#if defined(__HIP_DEVICE_COMPILE__)  // the gfx950 products exist in the device pass only (bls/fp.hpp)
  if (VARIANT == 1) fp_mul28_gfx950_2acc(m.v, x.v, yy.v);
  if (VARIANT == 2) fp_mul28(m.v, x.v, yy.v);
  if (VARIANT == 3) fp_mul_gfx950(m.v, x.v, yy.v);
#endif
  st12(r, i, m);
}

__global__ __launch_bounds__(64) void k_pre_add2(uint32_t n, const uint32_t* __restrict__ A, const uint32_t* __restrict__ B,
                                                 const uint32_t* __restrict__ C, const uint32_t* __restrict__ D,
                                                 const uint8_t* __restrict__ flags, uint32_t* __restrict__ x,
                                                 uint32_t* __restrict__ y) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  Fp a, b, c, d, X, Y;
  ld12(a, A, i);
  ld12(b, B, i);
  ld12(c, C, i);
  ld12(d, D, i);
  vm::pre_add2(X, a, b, Y, c, d, (flags[i] & 1) != 0, (flags[i] & 2) != 0);
  st12(x, i, X);
  st12(y, i, Y);
}

__global__ __launch_bounds__(64) void k_lin_unit(uint32_t n, const uint32_t* __restrict__ A, const uint32_t* __restrict__ B,
                                                 const uint32_t* __restrict__ C, const uint32_t* __restrict__ D,
                                                 const uint32_t* __restrict__ ctl, const uint32_t* __restrict__ cst,
                                                 uint32_t* __restrict__ r) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  Fp a, b, c, d, l;
  ld12(a, A, i);
  ld12(b, B, i);
  ld12(c, C, i);
  ld12(d, D, i);
  const uint32_t w = ctl[i], k = (w >> 8) & 15;
  uint32_t s[13];
  vm::lin_sum(s, a, b, c, d, 0u - (w & 1), 0u - ((w >> 1) & 1), 0u - ((w >> 2) & 1),
              w & (vm::H_LINNEG | vm::H_LINNEG2 | vm::H_LINNEG3), cst);
  vm::scale_reduce(l, s, k > 1 ? k : 1u);
  st12(r, i, l);
}

__global__ __launch_bounds__(64) void k_lin_mad(uint32_t n, const uint32_t* __restrict__ A, const uint32_t* __restrict__ B,
                                                const uint32_t* __restrict__ C, const uint32_t* __restrict__ D,
                                                const int8_t* __restrict__ coefs, uint32_t* __restrict__ r) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  Fp a, b, c, d, l;
  ld12(a, A, i);
  ld12(b, B, i);
  ld12(c, C, i);
  ld12(d, D, i);
  vm::lin_mad(l, a, b, c, d, coefs[4 * i], coefs[4 * i + 1], coefs[4 * i + 2], coefs[4 * i + 3]);
  st12(r, i, l);
}

__global__ __launch_bounds__(64) void k_canon(uint32_t n, const uint32_t* __restrict__ a, uint32_t* __restrict__ r) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  Fp x, c;
  ld12(x, a, i);
  vm::canon(c, x);
  st12(r, i, c);
}

__global__ __launch_bounds__(64) void k_fp_inv(uint32_t n, const uint32_t* __restrict__ a, const uint32_t* __restrict__ r3,
                                               uint32_t* __restrict__ r) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  Fp x, k, z;
  ld12(x, a, i);
  ld12(k, r3, 0);
  vm::fp_inv(z, x, k);
  st12(r, i, z);
}

// The shape of the product's k_h2f (csrc/ovhip.hip): the DST's templates by value in the kernel
// arguments, indexed by a run-time block number; one lane per 32-byte message; u0.c0, u0.c1,
// u1.c0, u1.c1 stored as hash_to_field leaves them (Montgomery limbs, 4 x 12 words per message).
__global__ __launch_bounds__(64) void k_h2f_probe(uint32_t n, const uint8_t* __restrict__ hashes, XmdTemplates t,
                                                  uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t msg[8], uni[64];
  const uint8_t* b = hashes + (size_t)i * 32;
  for (int w = 0; w < 8; ++w)
    msg[w] = ((uint32_t)b[4 * w] << 24) | ((uint32_t)b[4 * w + 1] << 16) | ((uint32_t)b[4 * w + 2] << 8) | b[4 * w + 3];
  expand_message_xmd_256(uni, msg, t);
  Fp2 u0, u1;
  hash_to_field_fp2x2(u0, u1, uni);
  st12(out, i * 4 + 0, u0.c0);
  st12(out, i * 4 + 1, u0.c1);
  st12(out, i * 4 + 2, u1.c0);
  st12(out, i * 4 + 3, u1.c1);
}

// LDS layout of the product's VM kernels (csrc/ovhip.hip): the constant table, then the slot
// file on a 256-byte boundary
constexpr uint32_t align256w(uint32_t w) { return (w + 63) / 64 * 64; }

// One unit of a W-lane program on a single-wave workgroup: lanes 0 .. W - 1 are the active slice,
// the rest run inactive over the same slots (as the idle slices of k_vm_fold do: they read, and
// never write).
template <bool SIDE>
__global__ __launch_bounds__(64) void k_vm_run(const uint4* __restrict__ code, uint32_t nphases, uint32_t W,
                                               const uint32_t* __restrict__ cst_g, uint32_t ncst,
                                               uint32_t* __restrict__ slots_g, uint32_t nslots, uint64_t scalar,
                                               uint32_t* __restrict__ planes, const uint32_t* __restrict__ side,
                                               uint32_t* __restrict__ scr) {
  extern __shared__ uint4 lds4[];
  uint32_t* lds = reinterpret_cast<uint32_t*>(lds4);
  uint32_t* cst = lds;
  uint32_t* slots = lds + align256w(ncst * 12);
  for (uint32_t k = threadIdx.x; k < ncst * 12; k += 64) cst[k] = cst_g[k];
  for (uint32_t k = threadIdx.x; k < nslots * 12; k += 64) slots[k] = slots_g[k];
  __syncthreads();
  const uint32_t lane = threadIdx.x % W;
  const bool active = threadIdx.x < W;
  const vm::Out out{planes, 1, 0};
  if (SIDE) vm::run<true>(code, nphases, W, lane, active, slots, cst, scalar, out, nullptr, side, scr);
  else vm::run(code, nphases, W, lane, active, slots, cst, scalar, out);
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < nslots * 12; k += 64) slots_g[k] = slots[k];
}

// Device buffers of one call: freed when the call returns, whatever its outcome.
struct Bufs {
  std::vector<void*> p;
  hipError_t err = hipSuccess;
  ~Bufs() {
    for (void* q : p) (void)hipFree(q);
  }
  // a device buffer of `bytes`, filled from `src` (zeroed when src is null)
  template <class T>
  T* up(const T* src, size_t bytes) {
    void* d = nullptr;
    if (err != hipSuccess) return nullptr;
    err = hipMalloc(&d, bytes);
    if (err != hipSuccess) return nullptr;
    p.push_back(d);
    err = src ? hipMemcpy(d, src, bytes, hipMemcpyHostToDevice) : hipMemset(d, 0, bytes);
    return static_cast<T*>(d);
  }
  void down(void* dst, const void* src, size_t bytes) {
    if (err == hipSuccess) err = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
  }
  // after a launch: launch errors, then the kernel's own
  void sync() {
    if (err == hipSuccess) err = hipGetLastError();
    if (err == hipSuccess) err = hipDeviceSynchronize();
  }
};

constexpr int BAD = (int)hipErrorInvalidValue;
inline uint32_t grid(uint32_t n) { return (n + 63) / 64; }
constexpr size_t FPB = 48;  // bytes of one value
constexpr size_t DEFAULT_DYN_LDS = 64 * 1024;  // dynamic LDS a kernel may take without the attribute

template <int V>
void launch_mul(bool alias, uint32_t n, const uint32_t* a, const uint32_t* b, uint32_t* r) {
  if (alias) k_fp_mul<V, true><<<grid(n), 64>>>(n, a, b, r);
  else k_fp_mul<V, false><<<grid(n), 64>>>(n, a, b, r);
}

}  // namespace

extern "C" {

// r = a b 2^-384 mod p, a, b < 4p. alias != 0: r = a a with one register array for both operands
// (b is ignored and may be null).
int dp_fp_mul(int variant, int alias, uint32_t n, const uint32_t* a, const uint32_t* b, uint32_t* r) {
  if (n == 0 || !a || !r || (!alias && !b) || variant < 0 || variant > 3) return BAD;
  Bufs m;
  const uint32_t* da = m.up(a, n * FPB);
  const uint32_t* db = alias ? da : m.up(b, n * FPB);
  uint32_t* dr = m.up<uint32_t>(nullptr, n * FPB);
  if (m.err != hipSuccess) return (int)m.err;
  switch (variant) {
    case 0: launch_mul<0>(alias != 0, n, da, db, dr); break;
    case 1: launch_mul<1>(alias != 0, n, da, db, dr); break;
    case 2: launch_mul<2>(alias != 0, n, da, db, dr); break;
    default: launch_mul<3>(alias != 0, n, da, db, dr); break;
  }
  m.sync();
  m.down(r, dr, n * FPB);
  return (int)m.err;
}

// flags[i]: bit 0 ny, bit 1 any_neg
int dp_pre_add2(uint32_t n, const uint32_t* A, const uint32_t* B, const uint32_t* C, const uint32_t* D,
                const uint8_t* flags, uint32_t* x, uint32_t* y) {
  if (n == 0 || !A || !B || !C || !D || !flags || !x || !y) return BAD;
  Bufs m;
  const uint32_t *dA = m.up(A, n * FPB), *dB = m.up(B, n * FPB), *dC = m.up(C, n * FPB), *dD = m.up(D, n * FPB);
  const uint8_t* df = m.up(flags, n);
  uint32_t *dx = m.up<uint32_t>(nullptr, n * FPB), *dy = m.up<uint32_t>(nullptr, n * FPB);
  if (m.err != hipSuccess) return (int)m.err;
  k_pre_add2<<<grid(n), 64>>>(n, dA, dB, dC, dD, df, dx, dy);
  m.sync();
  m.down(x, dx, n * FPB);
  m.down(y, dy, n * FPB);
  return (int)m.err;
}

// ctl[i] as hx_lin_unit; cst: ncst constant-table entries, ncst >= KTAB + 5
int dp_lin_unit(uint32_t n, const uint32_t* A, const uint32_t* B, const uint32_t* C, const uint32_t* D,
                const uint32_t* ctl, const uint32_t* cst, uint32_t ncst, uint32_t* r) {
  if (n == 0 || !A || !B || !C || !D || !ctl || !cst || !r || ncst < vm::KTAB + 5) return BAD;
  Bufs m;
  const uint32_t *dA = m.up(A, n * FPB), *dB = m.up(B, n * FPB), *dC = m.up(C, n * FPB), *dD = m.up(D, n * FPB);
  const uint32_t *dctl = m.up(ctl, n * sizeof(uint32_t)), *dcst = m.up(cst, ncst * FPB);
  uint32_t* dr = m.up<uint32_t>(nullptr, n * FPB);
  if (m.err != hipSuccess) return (int)m.err;
  k_lin_unit<<<grid(n), 64>>>(n, dA, dB, dC, dD, dctl, dcst, dr);
  m.sync();
  m.down(r, dr, n * FPB);
  return (int)m.err;
}

// coefs: 4 signed bytes per case, |c| <= 15
int dp_lin_mad(uint32_t n, const uint32_t* A, const uint32_t* B, const uint32_t* C, const uint32_t* D,
               const int8_t* coefs, uint32_t* r) {
  if (n == 0 || !A || !B || !C || !D || !coefs || !r) return BAD;
  for (size_t k = 0; k < (size_t)n * 4; ++k)
    if (coefs[k] < -15 || coefs[k] > 15) return BAD;
  Bufs m;
  const uint32_t *dA = m.up(A, n * FPB), *dB = m.up(B, n * FPB), *dC = m.up(C, n * FPB), *dD = m.up(D, n * FPB);
  const int8_t* dcf = m.up(coefs, (size_t)n * 4);
  uint32_t* dr = m.up<uint32_t>(nullptr, n * FPB);
  if (m.err != hipSuccess) return (int)m.err;
  k_lin_mad<<<grid(n), 64>>>(n, dA, dB, dC, dD, dcf, dr);
  m.sync();
  m.down(r, dr, n * FPB);
  return (int)m.err;
}

int dp_canon(uint32_t n, const uint32_t* a, uint32_t* r) {
  if (n == 0 || !a || !r) return BAD;
  Bufs m;
  const uint32_t* da = m.up(a, n * FPB);
  uint32_t* dr = m.up<uint32_t>(nullptr, n * FPB);
  if (m.err != hipSuccess) return (int)m.err;
  k_canon<<<grid(n), 64>>>(n, da, dr);
  m.sync();
  m.down(r, dr, n * FPB);
  return (int)m.err;
}

// vm::fp_inv on canonical values; r3: 12 words (raw R^3, or raw R for a raw inverse)
int dp_fp_inv(uint32_t n, const uint32_t* a, const uint32_t* r3, uint32_t* r) {
  if (n == 0 || !a || !r3 || !r) return BAD;
  Bufs m;
  const uint32_t *da = m.up(a, n * FPB), *d3 = m.up(r3, FPB);
  uint32_t* dr = m.up<uint32_t>(nullptr, n * FPB);
  if (m.err != hipSuccess) return (int)m.err;
  k_fp_inv<<<grid(n), 64>>>(n, da, d3, dr);
  m.sync();
  m.down(r, dr, n * FPB);
  return (int)m.err;
}

// The device counterpart of hx_h2f on n messages (msgs: n x 32 bytes) under one DST: out takes
// n x 4 values (u0.c0, u0.c1, u1.c0, u1.c1), nb the templates' block counts {nb0, nbi}. A DST
// that xmd_build_templates refuses (more than 255 bytes) returns an error without a launch.
int dp_h2f(uint32_t n, const uint8_t* msgs, const uint8_t* dst, size_t dst_len, uint32_t* out, uint32_t* nb) {
  if (n == 0 || n > (1u << 20) || !msgs || !out) return BAD;
  XmdTemplates t;
  if (!xmd_build_templates(t, dst, dst_len)) return BAD;
  if (nb) nb[0] = t.nb0, nb[1] = t.nbi;
  Bufs m;
  const uint8_t* dm = m.up(msgs, (size_t)n * 32);
  uint32_t* dr = m.up<uint32_t>(nullptr, (size_t)n * 4 * FPB);
  if (m.err != hipSuccess) return (int)m.err;
  k_h2f_probe<<<grid(n), 64>>>(n, dm, t, dr);
  m.sync();
  m.down(out, dr, (size_t)n * 4 * FPB);
  return (int)m.err;
}

// The device counterpart of hx_vm_run: one unit of a W-lane program (code: nphases x W x
// words_per_lane words, side: nphases x W side words or null; both get the PREFETCH trailing
// NOP phases here) on a single-wave workgroup, constants and slots in dynamic LDS. slots
// (nslots x 12 words) is read and written back; planes (nplanes x 12 words) takes the `st`
// outputs; scr: nscr scratch entries of a spilled program. A program that references a slot,
// constant (the ones exec reads implicitly included), plane or scratch entry outside what was
// passed, or needs more LDS than the device has, is refused without a launch.
int dp_vm_run(const uint32_t* code, uint32_t nphases, uint32_t W, uint32_t words_per_lane, const uint32_t* cst,
              uint32_t ncst, uint32_t* slots, uint32_t nslots, uint64_t scalar, uint32_t* planes, uint32_t nplanes,
              const uint32_t* side, uint32_t* scr, uint32_t nscr) {
  if (!code || !cst || !slots || !planes || nphases == 0 || nphases > (1u << 20) || words_per_lane != 4) return BAD;
  if (W == 0 || W > 64 || 64 % W != 0 || ncst == 0 || ncst > vm::CONST_BASE || nslots == 0 || nslots > vm::CONST_BASE ||
      nplanes == 0 || nplanes > 64)
    return BAD;
  if (side && (!scr || nscr == 0 || nscr > 4096)) return BAD;
  auto ref_ok = [&](uint32_t ref) {
    const uint32_t k = ref & (vm::CONST_BASE - 1);
    return (ref >> 12) == 0 && ((ref & vm::CONST_BASE) ? k < ncst : k < nslots);
  };
  const size_t nlanes = (size_t)nphases * W;
  for (size_t k = 0; k < nlanes; ++k) {
    const uint32_t* w = code + k * 4;
    const uint32_t op = w[0] & 31;
    if (op > vm::OP_SELB) return BAD;
    if (!ref_ok(w[1] & 0xFFFF) || !ref_ok(w[1] >> 16) || !ref_ok(w[2] & 0xFFFF) || !ref_ok(w[2] >> 16)) return BAD;
    if (((w[0] >> 5) & 0x7FF) >= nslots) return BAD;
    if (op == vm::OP_ST && ((w[0] >> 16) & 63) >= nplanes) return BAD;
    // constants exec reads by itself: the offset K = n (2p + 1), n <= 3, of a unit lin with negated
    // terms (lin_sum), and the zero constant of the selb path
    if ((w[0] & vm::H_LINNEG) && ncst < vm::KTAB + 4) return BAD;
    if ((w[0] & vm::H_SELB) && ncst <= vm::KZERO) return BAD;
    if (side && (side[k] & vm::SIDE_VALID) && ((side[k] & 0x7FF) >= nslots || ((side[k] >> 11) & 0xFFF) >= nscr))
      return BAD;
  }
  const size_t lds_bytes = ((size_t)align256w(ncst * 12) + (size_t)nslots * 12) * 4;
  int dev = 0, lds_max = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
  if (e != hipSuccess) return (int)e;
  if (lds_bytes > (size_t)lds_max) return BAD;
  // the uploaded code and side words carry PREFETCH trailing NOP phases (run()'s unrolled loops
  // read past the end)
  const size_t pad = (size_t)vm::PREFETCH * W;
  std::vector<uint32_t> hcode((nlanes + pad) * 4, 0u), hside;
  std::copy(code, code + nlanes * 4, hcode.begin());
  if (side) {
    hside.assign(nlanes + pad, 0u);
    std::copy(side, side + nlanes, hside.begin());
  }
  Bufs m;
  const uint32_t* dcode = m.up(hcode.data(), hcode.size() * 4);
  const uint32_t* dcst = m.up(cst, ncst * FPB);
  uint32_t* dslots = m.up(slots, nslots * FPB);
  uint32_t* dplanes = m.up<uint32_t>(nullptr, nplanes * FPB);
  const uint32_t* dside = side ? m.up(hside.data(), hside.size() * 4) : nullptr;
  uint32_t* dscr = side ? m.up<uint32_t>(nullptr, nscr * FPB) : nullptr;
  if (m.err != hipSuccess) return (int)m.err;
  if (lds_bytes > DEFAULT_DYN_LDS) {  // above the default limit of dynamic LDS: raised as the product's VM kernels do
    const void* kern = side ? (const void*)k_vm_run<true> : (const void*)k_vm_run<false>;
    m.err = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (m.err != hipSuccess) return (int)m.err;
  }
  const uint4* c4 = reinterpret_cast<const uint4*>(dcode);
  if (side) k_vm_run<true><<<1, 64, lds_bytes>>>(c4, nphases, W, dcst, ncst, dslots, nslots, scalar, dplanes, dside, dscr);
  else k_vm_run<false><<<1, 64, lds_bytes>>>(c4, nphases, W, dcst, ncst, dslots, nslots, scalar, dplanes, dside, dscr);
  m.sync();
  m.down(slots, dslots, nslots * FPB);
  m.down(planes, dplanes, nplanes * FPB);
  if (side) m.down(scr, dscr, nscr * FPB);
  return (int)m.err;
}

}  // extern "C"
