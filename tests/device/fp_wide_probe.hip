// Device probe for the radix-2^392 ("wide") arithmetic (tests/test_gpu_fp_wide.py): the generated
// gfx950 wide product fp_mul_wide (csrc/bls/fp.hpp, fp_mul28w_gfx950), one thread per case, and
// the Fp-VM interpreter bound to radix 392 at compile time (vm::run<.., 392>, the instantiation
// the vote pool's vote loop uses) on one single-wave workgroup. Test infrastructure only: built
// beside libovhip.so with the product's flags, never linked into it.
//
// Every entry point takes host arrays (12 words per value), copies them to the device, launches
// one kernel, synchronises, copies the results back, frees the device memory and returns the HIP
// error code (0 on success). Bad arguments return an error without a launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../consensus_overlord_amd/csrc/fpvm.hpp"

using namespace ovh;

namespace {

__global__ __launch_bounds__(64) void k_mul_wide(uint32_t n, const uint32_t* __restrict__ a,
                                                 const uint32_t* __restrict__ b, uint32_t* __restrict__ r) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  Fp x, y, m;
#pragma unroll
  for (int k = 0; k < 12; ++k) x.v[k] = a[(size_t)i * 12 + k], y.v[k] = b[(size_t)i * 12 + k];
  fp_mul_wide(m, x, y);
#pragma unroll
  for (int k = 0; k < 12; ++k) r[(size_t)i * 12 + k] = m.v[k];
}

constexpr uint32_t align256w(uint32_t w) { return (w + 63) / 64 * 64; }

// One unit of a W-lane program without side words, inversion or `st` ops, through the
// interpreter fixed to radix 392: lanes 0 .. W - 1 are the active slice.
__global__ __launch_bounds__(64) void k_vm_run392(const uint4* __restrict__ code, uint32_t nphases, uint32_t W,
                                                  const uint32_t* __restrict__ cst_g, uint32_t ncst,
                                                  uint32_t* __restrict__ slots_g, uint32_t nslots) {
  extern __shared__ uint4 lds4[];
  uint32_t* lds = reinterpret_cast<uint32_t*>(lds4);
  uint32_t* cst = lds;
  uint32_t* slots = lds + align256w(ncst * 12);
  for (uint32_t k = threadIdx.x; k < ncst * 12; k += 64) cst[k] = cst_g[k];
  for (uint32_t k = threadIdx.x; k < nslots * 12; k += 64) slots[k] = slots_g[k];
  __syncthreads();
  vm::run<false, false, 1, 392>(code, nphases, W, threadIdx.x % W, threadIdx.x < W, slots, cst, 0,
                                vm::Out{nullptr, 0, 0});
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < nslots * 12; k += 64) slots_g[k] = slots[k];
}

struct Bufs {
  std::vector<void*> p;
  hipError_t err = hipSuccess;
  ~Bufs() {
    for (void* q : p) (void)hipFree(q);
  }
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
  void sync() {
    if (err == hipSuccess) err = hipGetLastError();
    if (err == hipSuccess) err = hipDeviceSynchronize();
  }
};

constexpr int BAD = (int)hipErrorInvalidValue;
constexpr size_t FPB = 48;

}  // namespace

extern "C" {

// r = a b 2^-392 mod p for a, b < 4p (no conditional subtraction): n cases, 64 per workgroup
int dw_fp_mul_wide(uint32_t n, const uint32_t* a, const uint32_t* b, uint32_t* r) {
  if (n == 0 || n > (1u << 20) || !a || !b || !r) return BAD;
  Bufs m;
  const uint32_t *da = m.up(a, n * FPB), *db = m.up(b, n * FPB);
  uint32_t* dr = m.up<uint32_t>(nullptr, n * FPB);
  if (m.err != hipSuccess) return (int)m.err;
  k_mul_wide<<<(n + 63) / 64, 64>>>(n, da, db, dr);
  m.sync();
  m.down(r, dr, n * FPB);
  return (int)m.err;
}

// One unit of a W-lane program (nphases x W x 4 words) of products, flag ops, lin and selb-free
// light ops through vm::run<false, false, 1, 392>. A program with an op outside muls / sgn0 / lex
// / eq / lin / nop, a header bit of the rare or selb blocks, or a reference outside the slots and
// constants passed is refused without a launch.
int dw_vm_run392(const uint32_t* code, uint32_t nphases, uint32_t W, const uint32_t* cst, uint32_t ncst,
                 uint32_t* slots, uint32_t nslots) {
  if (!code || !cst || !slots || nphases == 0 || nphases > 4096) return BAD;
  if (W == 0 || W > 64 || 64 % W != 0 || ncst < vm::KTAB + 5 || ncst > 256 || nslots == 0 || nslots > 512) return BAD;
  auto ref_ok = [&](uint32_t ref) {
    const uint32_t k = ref & (vm::CONST_BASE - 1);
    return (ref >> 12) == 0 && ((ref & vm::CONST_BASE) ? k < ncst : k < nslots);
  };
  const size_t nlanes = (size_t)nphases * W;
  for (size_t k = 0; k < nlanes; ++k) {
    const uint32_t* w = code + k * 4;
    const uint32_t op = w[0] & 31;
    if (op != vm::OP_NOP && op != vm::OP_MULS && op != vm::OP_SGN0 && op != vm::OP_LEX && op != vm::OP_EQ &&
        op != vm::OP_LIN)
      return BAD;
    if (w[0] & (vm::H_RARE | vm::H_SELB)) return BAD;
    if (!ref_ok(w[1] & 0xFFFF) || !ref_ok(w[1] >> 16) || !ref_ok(w[2] & 0xFFFF) || !ref_ok(w[2] >> 16)) return BAD;
    if (((w[0] >> 5) & 0x7FF) >= nslots) return BAD;
  }
  const size_t lds_bytes = ((size_t)align256w(ncst * 12) + (size_t)nslots * 12) * 4;
  if (lds_bytes > 64 * 1024) return BAD;
  const size_t pad = (size_t)vm::PREFETCH * W;  // trailing NOP phases (run() reads past the end)
  std::vector<uint32_t> hcode((nlanes + pad) * 4, 0u);
  std::copy(code, code + nlanes * 4, hcode.begin());
  Bufs m;
  const uint32_t* dcode = m.up(hcode.data(), hcode.size() * 4);
  const uint32_t* dcst = m.up(cst, ncst * FPB);
  uint32_t* dslots = m.up(slots, nslots * FPB);
  if (m.err != hipSuccess) return (int)m.err;
  k_vm_run392<<<1, 64, lds_bytes>>>(reinterpret_cast<const uint4*>(dcode), nphases, W, dcst, ncst, dslots, nslots);
  m.sync();
  m.down(slots, dslots, nslots * FPB);
  return (int)m.err;
}

}  // extern "C"
