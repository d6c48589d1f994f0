// Device probe for the unit-level tests of ovh_rounds_add's kernels
// (tests/test_gpu_rounds_kernels.py): the selection through the table of round references
// (k_qc_claim_r, k_qc_mark_r), the segmented sum, the segmented merge (k_qc_merge_seg), the gather
// and the compression (csrc/qc.hpp) behind the product's own launch code (enqueue_qc_rounds,
// ensure_qc_cap of csrc/ovhip.hip, qc_segments, QcRound's layout), on arrays and points the caller
// chooses. Through ovh_rounds_add a test cannot choose them: every vote there is a verified
// signature of an unrelated key. Test infrastructure only: built beside libovhip.so with the
// product's flags, never linked into it.
//
// The conventions are qc_probe.hip's: the product translation unit is included whole and the
// library is linked with -Bsymbolic; the entry point takes host arrays and returns 0, a HIP error
// code, or an OVH_ERR_* of the product; bad arguments are refused (hipErrorInvalidValue) without a
// launch. Field values are 12 words, canonical Montgomery limbs; a G2 point is 4 of them, a
// projective one 6. The context is created on the first call (device 0) and kept until rp_close.
#include "../../consensus_overlord_amd/csrc/ovhip.hip"

namespace {

constexpr int RP_BAD = (int)hipErrorInvalidValue;
constexpr uint32_t RP_NMAX = 1u << 12;  // votes and table entries per call
constexpr uint32_t RP_GUARD = 64;       // guard words on both sides of a round's allocation
constexpr int RP_SLOT = 0;

ovh_ctx* g_rp = nullptr;
std::mutex g_rp_mu;

struct Rp {
  hipStream_t st;
  hipError_t err = hipSuccess;
  std::vector<void*> mem;
  explicit Rp(hipStream_t s) : st(s) {}
  ~Rp() {
    for (void* p : mem) (void)hipFree(p);
  }
  // `words` device words, every byte 0xFF
  uint32_t* alloc(size_t words) {
    void* p = nullptr;
    if (err == hipSuccess) err = hipMalloc(&p, (words ? words : 1) * 4);
    if (err != hipSuccess) return nullptr;
    mem.push_back(p);
    err = hipMemsetAsync(p, 0xFF, (words ? words : 1) * 4, st);
    return (uint32_t*)p;
  }
  uint32_t* put(const void* src, size_t words) {
    uint32_t* p = alloc(words);
    up(p, src, words * 4);
    return p;
  }
  void up(void* dst, const void* src, size_t bytes) {
    if (err == hipSuccess && bytes) err = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
  }
  void down(void* dst, const void* src, size_t bytes) {
    if (err == hipSuccess && bytes) err = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
  }
  void sync() {
    if (err == hipSuccess) err = hipGetLastError();
    if (err == hipSuccess) err = hipStreamSynchronize(st);
  }
};

}  // namespace

extern "C" {

uint32_t rp_guard(void) { return RP_GUARD; }
// the words of a round's allocation on a table of tn entries, and where its R starts (QcRound)
uint32_t rp_round_words(uint32_t tn) { return (uint32_t)QcRound::words(tn, (tn + 31) / 32); }
uint32_t rp_r_off(uint32_t tn) { return (uint32_t)QcRound::r_off(tn, (tn + 31) / 32); }

// One call's device part (enqueue_qc_rounds) over K rounds of a table of tn entries and n >= 2
// staged votes, the first t of them votes of table entries tidx[j] < tn: codes[n], tidx[t],
// orig[n] (the vote's position among its round's votes), rank[tn], gid[n] < K (every round with at
// least one vote), base[K], sigma (n x 48 words, written to the S_SIG planes).
// state: K x (RP_GUARD + rp_round_words(tn) + RP_GUARD) words, in and out. Each round is an
// allocation of its own, 0xFF-filled; the caller's words between the guards (QcRound's layout:
// owner | bitmap | count | merged | pad | R | 96 bytes) are uploaded before the run and the whole
// allocation, guards included, is returned after it. A of the slot is poisoned first.
// Outputs besides: taken[n], rows (K x (1 + ceil(tn / 32)): count | bitmap words), out96 (K x 96
// bytes from a 0xFF-filled device buffer: a round with count 0 keeps the fill).
int rp_rounds(uint32_t tn, uint32_t K, uint32_t n, uint32_t t, const int32_t* codes, const int32_t* tidx,
              const uint32_t* orig, const uint32_t* rank, const uint32_t* gid, const uint32_t* base, const uint32_t* sigma,
              uint32_t* state, uint32_t* taken, uint32_t* rows, uint8_t* out96) {
  if (n < 2 || n > RP_NMAX || tn == 0 || tn > RP_NMAX || t > n || K == 0 || K > OVH_ROUNDS_MAX) return RP_BAD;
  if (!codes || (t && !tidx) || !orig || !rank || !gid || !base || !sigma || !state || !taken || !rows || !out96) return RP_BAD;
  for (uint32_t j = 0; j < t; ++j)
    if (tidx[j] < 0 || (uint32_t)tidx[j] >= tn) return RP_BAD;
  for (uint32_t e = 0; e < tn; ++e)
    if (rank[e] >= tn) return RP_BAD;
  std::vector<uint32_t> fill(K, 0);
  for (uint32_t j = 0; j < n; ++j) {
    if (gid[j] >= K || orig[j] >= n) return RP_BAD;
    ++fill[gid[j]];
  }
  for (uint32_t k = 0; k < K; ++k)
    if (!fill[k] || base[k] > OVH_ROUND_VOTES_MAX) return RP_BAD;
  QcSegments sg;
  qc_segments(n, K, gid, sg);
  std::lock_guard<std::mutex> g(g_rp_mu);
  if (!g_rp) g_rp = ovh_create(0, nullptr, 0, 0);
  if (!g_rp || hipSetDevice(g_rp->device) != hipSuccess) return OVH_ERR_DEVICE;
  ovh_ctx* c = g_rp;
  int err = 0;
  if ((err = ensure_qc_cap(c, n, sg)) != 0) return err;
  uint32_t* cur;
  const MsmArgs a = msm_args(c, RP_SLOT, &cur);
  if (n > a.st.cap || 32 * (size_t)sg.chunks > a.A.cap) return OVH_ERR_ARG;
  const uint32_t bw = (tn + 31) / 32;
  const size_t words = QcRound::words(tn, bw), stride = words + 2 * RP_GUARD;
  Rp m(c->stream);
  // sigma into the S_SIG planes (plane-major rows of a.st.cap entries)
  std::vector<uint32_t> stage((size_t)48 * n);
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t r = 0; r < 48; ++r) stage[(size_t)r * n + i] = sigma[(size_t)i * 48 + r];
  if (m.err == hipSuccess)
    m.err = hipMemcpy2DAsync(a.st.p + (size_t)S_SIG * 12 * a.st.cap, (size_t)a.st.cap * 4, stage.data(), (size_t)n * 4,
                             (size_t)n * 4, 48, hipMemcpyHostToDevice, m.st);
  if (m.err == hipSuccess) m.err = hipMemsetAsync(a.A.p, 0xFF, (size_t)72 * a.A.cap * 4, m.st);
  std::vector<uint32_t*> dev(K);
  std::vector<QcRoundRef> refs(K);
  for (uint32_t k = 0; k < K; ++k) {
    dev[k] = m.alloc(stride);
    if (!dev[k]) return (int)m.err;
    m.up(dev[k] + RP_GUARD, state + k * stride + RP_GUARD, words * 4);
    QcRound r;
    r.dev = dev[k] + RP_GUARD;
    r.tn = tn;
    r.bw = bw;
    refs[k] = QcRoundRef{r.owner(), r.bitmap(), r.count(), r.merged(), r.R(), base[k], 0};
  }
  static_assert(sizeof(QcRoundRef) % 4 == 0, "QcRoundRef is staged as words");
  const QcRoundRef* drefs = (const QcRoundRef*)m.put(refs.data(), sizeof(QcRoundRef) / 4 * K);
  QcSel sel{};
  sel.codes = (const int32_t*)m.put(codes, n);
  sel.tidx = t ? (const int32_t*)m.put(tidx, t) : nullptr;
  sel.orig = m.put(orig, n);
  sel.rank = m.put(rank, tn);
  sel.gid = m.put(gid, n);
  sel.groups = K;
  sel.bw = bw;
  sel.taken = m.alloc(n);
  const uint32_t* dlist = m.put(sg.list.data(), sg.list.size());
  const uint32_t* dseg = m.put(sg.seg.data(), sg.seg.size());
  uint32_t* drows = m.alloc((size_t)K * (1 + bw));
  uint8_t* dout = (uint8_t*)m.alloc(24 * (size_t)K);
  if (m.err != hipSuccess) return (int)m.err;
  if ((err = enqueue_qc_rounds(c, m.st, a, n, t, sel, drefs, sg, dlist, dseg, bw, drows, dout, nullptr)) != 0) return err;
  m.sync();
  for (uint32_t k = 0; k < K; ++k) m.down(state + k * stride, dev[k], stride * 4);
  m.down(taken, sel.taken, (size_t)n * 4);
  m.down(rows, drows, (size_t)K * (1 + bw) * 4);
  m.down(out96, dout, 96 * (size_t)K);
  m.sync();
  return (int)m.err;
}

// destroys the probe's context (the next call creates a new one)
void rp_close(void) {
  std::lock_guard<std::mutex> g(g_rp_mu);
  if (g_rp) ovh_destroy(g_rp);
  g_rp = nullptr;
}

}  // extern "C"
