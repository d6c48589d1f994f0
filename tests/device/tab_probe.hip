// Device probe for the unit-level tests of ovh_update_validators' kernels
// (tests/test_gpu_tab_kernels.py): k_tab_build and k_round_remap (csrc/tab_update.hpp) behind the
// product's own launch code (enqueue_tab_build, enqueue_round_remap of csrc/ovhip.hip, QcRound's
// layout), on slabs, maps and round words the caller chooses. Through ovh_update_validators a test
// cannot choose them: the planes there are points of real keys and the owner words come from
// verified votes. Test infrastructure only: built beside libovhip.so with the product's flags,
// never linked into it.
//
// The conventions are rounds_probe.hip's: the product translation unit is included whole and the
// library is linked with -Bsymbolic; an entry point takes host arrays and returns 0 or a HIP error
// code; bad arguments are refused (hipErrorInvalidValue) without a launch. Every device allocation
// is 0xFF-filled before the caller's words go in. No context is needed: device 0, the null stream.
#include "../../consensus_overlord_amd/csrc/ovhip.hip"

namespace {

constexpr int TP_BAD = (int)hipErrorInvalidValue;
constexpr uint32_t TP_NMAX = 1u << 12;  // table entries per call
constexpr uint32_t TP_GUARD = 64;       // guard words around a destination

struct Tp {
  hipError_t err = hipSuccess;
  std::vector<void*> mem;
  ~Tp() {
    for (void* p : mem) (void)hipFree(p);
  }
  uint32_t* alloc(size_t words) {
    void* p = nullptr;
    if (err == hipSuccess) err = hipMalloc(&p, (words ? words : 1) * 4);
    if (err != hipSuccess) return nullptr;
    mem.push_back(p);
    err = hipMemsetAsync(p, 0xFF, (words ? words : 1) * 4, nullptr);
    return (uint32_t*)p;
  }
  uint32_t* put(const void* src, size_t words) {
    uint32_t* p = alloc(words);
    if (err == hipSuccess && words) err = hipMemcpyAsync(p, src, words * 4, hipMemcpyHostToDevice, nullptr);
    return p;
  }
  void down(void* dst, const void* src, size_t words) {
    if (err == hipSuccess && words) err = hipMemcpyAsync(dst, src, words * 4, hipMemcpyDeviceToHost, nullptr);
  }
  void sync() {
    if (err == hipSuccess) err = hipGetLastError();
    if (err == hipSuccess) err = hipStreamSynchronize(nullptr);
  }
};

bool cap_ok(uint32_t cap, uint32_t n) { return cap >= 1 && cap <= TP_NMAX && n <= cap; }

}  // namespace

extern "C" {

uint32_t tp_guard(void) { return TP_GUARD; }
// the words of a round's allocation on a table of tn entries, and where its R starts (QcRound)
uint32_t tp_round_words(uint32_t tn) { return (uint32_t)QcRound::words(tn, (tn + 31) / 32); }
uint32_t tp_r_off(uint32_t tn) { return (uint32_t)QcRound::r_off(tn, (tn + 31) / 32); }

// k_tab_build over n new entries. src[n]: an old entry < n_old, or TAB_NEW | j with j < n_fresh.
// old_planes: 36 x cap_old words (word w of entry i at w * cap_old + i), old_flags: cap_old;
// fresh_planes / fresh_flags the same on cap_fresh. out_planes: 36 x cap_new + TP_GUARD words and
// out_flags: cap_new + TP_GUARD words, the whole 0xFF-filled allocations after the run.
int tp_tab_build(uint32_t n, uint32_t n_old, uint32_t cap_old, uint32_t n_fresh, uint32_t cap_fresh, uint32_t cap_new,
                 const uint32_t* src, const uint32_t* old_planes, const uint32_t* old_flags, const uint32_t* fresh_planes,
                 const uint32_t* fresh_flags, uint32_t* out_planes, uint32_t* out_flags) {
  if (!cap_ok(cap_old, n_old) || !cap_ok(cap_fresh, n_fresh) || !cap_ok(cap_new, n) || n == 0) return TP_BAD;
  if (!src || !old_planes || !old_flags || !fresh_planes || !fresh_flags || !out_planes || !out_flags) return TP_BAD;
  for (uint32_t i = 0; i < n; ++i)
    if ((src[i] & TAB_NEW) ? (src[i] & ~TAB_NEW) >= n_fresh : src[i] >= n_old) return TP_BAD;
  if (hipSetDevice(0) != hipSuccess) return OVH_ERR_DEVICE;
  Tp m;
  const uint32_t* dsrc = m.put(src, n);
  uint32_t* dop = m.put(old_planes, (size_t)36 * cap_old);
  const uint32_t* dof = m.put(old_flags, cap_old);
  uint32_t* dfp = m.put(fresh_planes, (size_t)36 * cap_fresh);
  const uint32_t* dff = m.put(fresh_flags, cap_fresh);
  uint32_t* dout = m.alloc((size_t)36 * cap_new + TP_GUARD);
  uint32_t* dfl = m.alloc((size_t)cap_new + TP_GUARD);
  if (m.err != hipSuccess) return (int)m.err;
  enqueue_tab_build(nullptr, n, dsrc, Slab{dop, cap_old}, dof, Slab{dfp, cap_fresh}, dff, Slab{dout, cap_new}, dfl);
  m.sync();
  m.down(out_planes, dout, (size_t)36 * cap_new + TP_GUARD);
  m.down(out_flags, dfl, (size_t)cap_new + TP_GUARD);
  m.sync();
  return (int)m.err;
}

// k_round_remap over K rounds in one launch, from a table of tn_old entries to one of tn_new.
// rsrc[tn_new]: an old entry or QC_NONE; dst[tn_old]: a new entry or QC_NONE; sorted[tn_new]: a
// permutation. old_state: K x tp_round_words(tn_old) words (QcRound's layout). new_state: K x
// (TP_GUARD + tp_round_words(tn_new) + TP_GUARD) words: each round's new allocation, 0xFF-filled
// before the run, guards included, after it. lost: K words from the launch (zero before it).
int tp_round_remap(uint32_t K, uint32_t tn_old, uint32_t tn_new, const uint32_t* rsrc, const uint32_t* dst,
                   const uint32_t* sorted, const uint32_t* old_state, uint32_t* new_state, uint32_t* lost) {
  if (K == 0 || K > OVH_ROUNDS_MAX || tn_old == 0 || tn_old > TP_NMAX || tn_new == 0 || tn_new > TP_NMAX) return TP_BAD;
  if (!rsrc || !dst || !sorted || !old_state || !new_state || !lost) return TP_BAD;
  std::vector<uint8_t> seen(tn_new, 0);
  for (uint32_t i = 0; i < tn_new; ++i) {
    if (rsrc[i] != QC_NONE && rsrc[i] >= tn_old) return TP_BAD;
    if (sorted[i] >= tn_new || seen[sorted[i]]++) return TP_BAD;
  }
  for (uint32_t o = 0; o < tn_old; ++o)
    if (dst[o] != QC_NONE && dst[o] >= tn_new) return TP_BAD;
  if (hipSetDevice(0) != hipSuccess) return OVH_ERR_DEVICE;
  const uint32_t bwo = (tn_old + 31) / 32, bwn = (tn_new + 31) / 32;
  const size_t wo = QcRound::words(tn_old, bwo), wn = QcRound::words(tn_new, bwn), stride = wn + 2 * TP_GUARD;
  Tp m;
  std::vector<TabRoundRef> refs(K);
  std::vector<uint32_t*> dev(K);
  for (uint32_t k = 0; k < K; ++k) {
    const uint32_t* o = m.put(old_state + k * wo, wo);
    dev[k] = m.alloc(stride);
    if (m.err != hipSuccess) return (int)m.err;
    refs[k] = TabRoundRef{o, dev[k] + TP_GUARD, tn_old, bwo, tn_new, bwn};
  }
  const TabRoundRef* drefs = (const TabRoundRef*)m.put(refs.data(), sizeof(TabRoundRef) / 4 * K);
  const uint32_t* drsrc = m.put(rsrc, tn_new);
  const uint32_t* ddst = m.put(dst, tn_old);
  const uint32_t* dsorted = m.put(sorted, tn_new);
  uint32_t* dlost = m.alloc(K);
  if (m.err == hipSuccess) m.err = hipMemsetAsync(dlost, 0, (size_t)K * 4, nullptr);
  if (m.err != hipSuccess) return (int)m.err;
  enqueue_round_remap(nullptr, K, tn_old > tn_new ? tn_old : tn_new, drefs, drsrc, ddst, dsorted, dlost);
  m.sync();
  for (uint32_t k = 0; k < K; ++k) m.down(new_state + k * stride, dev[k], stride);
  m.down(lost, dlost, K);
  m.sync();
  return (int)m.err;
}

}  // extern "C"
