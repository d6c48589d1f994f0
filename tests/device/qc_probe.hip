// Device probe for the unit-level tests of the quorum-certificate kernels
// (tests/test_gpu_qc_kernels.py): the product's selection and masked-sum kernels (csrc/qc.hpp)
// behind its own launch code (enqueue_qc_select, enqueue_qc_sum, ensure_qc_cap of csrc/ovhip.hip,
// qc_segments of csrc/qc_segments.hpp), and k_qc_apk with the product's launch shape, on arrays
// the caller chooses. Through ovh_build_qc / ovh_build_qcs / ovh_verify_qc_batch a test cannot
// choose them: every vote there is a verified signature of an unrelated key. Test infrastructure
// only: built beside libovhip.so with the product's flags, never linked into it.
//
// The conventions are msm_probe.hip's: the product translation unit is included whole and the
// library is linked with -Bsymbolic; every entry point takes host arrays and returns 0, a HIP
// error code, or an OVH_ERR_* of the product (100 and above); bad arguments are refused
// (hipErrorInvalidValue) without a launch. Field values are 12 words, canonical Montgomery limbs;
// a G2 point is 4 of them (x.c0, x.c1, y.c0, y.c1), a projective result 6 (X.c0, X.c1, Y.c0,
// Y.c1, Z.c0, Z.c1), a G1 Jacobian entry 3 (X, Y, Z). The context is created on the first call
// (device 0) and kept until qp_close.
#include "../../consensus_overlord_amd/csrc/ovhip.hip"

namespace {

constexpr int QP_BAD = (int)hipErrorInvalidValue;
constexpr uint32_t QP_NMAX = 1u << 16;  // votes, table entries, list entries per call
constexpr uint32_t QP_GUARD = 64;       // guard words on both sides of a selection array
constexpr int QP_SLOT = 0;

ovh_ctx* g_qp = nullptr;
std::mutex g_qp_mu;

// the probe's context; nullptr -> *err
ovh_ctx* qp_ctx(int* err) {
  if (!g_qp) g_qp = ovh_create(0, nullptr, 0, 0);
  *err = !g_qp || hipSetDevice(g_qp->device) != hipSuccess ? OVH_ERR_DEVICE : 0;
  return *err ? nullptr : g_qp;
}

struct Qp {
  hipStream_t st;
  hipError_t err = hipSuccess;
  std::vector<void*> mem;
  explicit Qp(hipStream_t s) : st(s) {}
  ~Qp() {
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
  // a device copy of `words` host words (null: none)
  uint32_t* put(const void* src, size_t words) {
    if (!src) return nullptr;
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
  // launch errors, then the kernels' own
  void sync() {
    if (err == hipSuccess) err = hipGetLastError();
    if (err == hipSuccess) err = hipStreamSynchronize(st);
  }
};

// n affine points (n x 4 x 12 words) -> the 4 planes from `plane` of the slot's state slab
void put_points(Qp& m, const Slab& s, uint32_t plane, uint32_t n, const uint32_t* pts, std::vector<uint32_t>& stage) {
  stage.assign((size_t)48 * n, 0u);
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t r = 0; r < 48; ++r) stage[(size_t)r * n + i] = pts[(size_t)i * 48 + r];
  if (m.err == hipSuccess)
    m.err = hipMemcpy2DAsync(s.p + (size_t)plane * 12 * s.cap, (size_t)s.cap * 4, stage.data(), (size_t)n * 4, (size_t)n * 4,
                             48, hipMemcpyHostToDevice, m.st);
}

// A of the slot filled with 0xFF words (values far above p, Z != 0): an entry that a run reads
// or returns without having written it cannot pass for a sum, nor for the identity
void poison(Qp& m, const MsmArgs& a) {
  if (m.err == hipSuccess) m.err = hipMemsetAsync(a.A.p, 0xFF, (size_t)72 * a.A.cap * 4, m.st);
}

// entry idx of a device slab of `rows` limb rows -> rows words at out
void get_entry(Qp& m, uint32_t* out, const Slab& s, uint32_t rows, uint32_t idx) {
  if (m.err == hipSuccess)
    m.err = hipMemcpy2DAsync(out, 4, s.p + idx, (size_t)s.cap * 4, 4, rows, hipMemcpyDeviceToHost, m.st);
}

}  // namespace

extern "C" {

// words of guard on each side of qp_select's output arrays
uint32_t qp_guard(void) { return QP_GUARD; }

// The product's selection (enqueue_qc_select: k_qc_reset, k_qc_claim, k_qc_mark) over n staged
// votes, the first t of them votes of table entries tidx[j] < tn: codes[n], tidx[t] (may be null
// when t = 0), orig[n] (a permutation of 0 .. n - 1, or null: the staged order is the caller's),
// rank[tn] (a permutation of 0 .. tn - 1), gid[n] < groups (or null with groups = 1).
// Outputs, each with QP_GUARD words in front of and behind what the kernels own, the device
// arrays filled with 0xFF words first: owner (groups x tn), bitmap (groups x ceil(tn / 32)),
// count (groups), taken (n).
int qp_select(uint32_t tn, uint32_t n, uint32_t t, const int32_t* codes, const int32_t* tidx, const uint32_t* orig,
              const uint32_t* rank, const uint32_t* gid, uint32_t groups, uint32_t* owner, uint32_t* bitmap, uint32_t* count,
              uint32_t* taken) {
  if (n == 0 || n > QP_NMAX || tn == 0 || tn > QP_NMAX || t > n || groups == 0 || groups > OVH_QC_GROUPS_MAX) return QP_BAD;
  if (!codes || (t && !tidx) || !rank || !owner || !bitmap || !count || !taken) return QP_BAD;
  if (!gid && groups != 1) return QP_BAD;
  for (uint32_t j = 0; j < t; ++j)
    if (tidx[j] < 0 || (uint32_t)tidx[j] >= tn) return QP_BAD;
  for (uint32_t e = 0; e < tn; ++e)
    if (rank[e] >= tn) return QP_BAD;
  for (uint32_t j = 0; j < n; ++j)
    if ((gid && gid[j] >= groups) || (orig && orig[j] >= n)) return QP_BAD;
  std::lock_guard<std::mutex> g(g_qp_mu);
  int err = 0;
  ovh_ctx* c = qp_ctx(&err);
  if (!c) return err;
  const uint32_t bw = (tn + 31) / 32;
  const size_t words[4] = {(size_t)groups * tn, (size_t)groups * bw, groups, n};
  uint32_t* host[4] = {owner, bitmap, count, taken};
  uint32_t* dev[4];
  Qp m(c->stream);
  for (int k = 0; k < 4; ++k) dev[k] = m.alloc(words[k] + 2 * QP_GUARD);
  QcSel sel;
  sel.codes = (const int32_t*)m.put(codes, n);
  sel.tidx = (const int32_t*)m.put(t ? tidx : nullptr, t);
  sel.orig = m.put(orig, n);
  sel.rank = m.put(rank, tn);
  sel.gid = m.put(gid, n);
  sel.groups = groups;
  sel.bw = bw;
  if (m.err != hipSuccess) return (int)m.err;
  sel.owner = dev[0] + QP_GUARD;
  sel.bitmap = dev[1] + QP_GUARD;
  sel.count = dev[2] + QP_GUARD;
  sel.taken = dev[3] + QP_GUARD;
  enqueue_qc_select(m.st, tn, n, t, sel);
  m.sync();
  for (int k = 0; k < 4; ++k) m.down(host[k], dev[k], (words[k] + 2 * QP_GUARD) * 4);
  m.sync();
  return (int)m.err;
}

// The product's masked sum (enqueue_qc_sum: k_qc_chunk, k_qc_upper, the compression) over the n
// affine points `sigma` (written to the S_SIG planes) under the mask taken[n] (0 / 1); A is
// poisoned first. gid null (G = 1): the plain form of ovh_build_qc. Else the segmented form of
// ovh_build_qcs over gid[n] < G, every group with at least one vote: the list is the product's
// qc_segments(), the capacity the product's ensure_qc_cap(). n >= 2, as in the product (one vote
// takes the sigchk path). Outputs: sums (G x 72 words: A[32 seg[2 g]], A[0] in the plain form),
// out96 (G x 96 bytes).
int qp_sum(uint32_t n, const uint32_t* sigma, const uint32_t* taken, const uint32_t* gid, uint32_t G, uint32_t* sums,
           uint8_t* out96) {
  if (n < 2 || n > QP_NMAX || !sigma || !taken || !sums || !out96 || G == 0 || G > OVH_QC_GROUPS_MAX) return QP_BAD;
  if (!gid && G != 1) return QP_BAD;
  for (uint32_t j = 0; j < n; ++j)
    if (taken[j] > 1) return QP_BAD;
  QcSegments sg;
  if (gid) {
    std::vector<uint32_t> fill(G, 0);
    for (uint32_t j = 0; j < n; ++j) {
      if (gid[j] >= G) return QP_BAD;
      ++fill[gid[j]];
    }
    for (uint32_t g = 0; g < G; ++g)
      if (!fill[g]) return QP_BAD;
    qc_segments(n, G, gid, sg);
  }
  std::lock_guard<std::mutex> g(g_qp_mu);
  int err = 0;
  ovh_ctx* c = qp_ctx(&err);
  if (!c) return err;
  if ((err = ensure_qc_cap(c, n, sg)) != 0) return err;
  uint32_t* cur;
  const MsmArgs a = msm_args(c, QP_SLOT, &cur);
  // what the kernels index: votes in the state slab, 32 tree entries per chunk in A
  const size_t chunks = gid ? sg.chunks : (n + MSM_CH - 1) >> MSM_CH_LV;
  if (n > a.st.cap || 32 * chunks > a.A.cap) return OVH_ERR_ARG;
  Qp m(c->stream);
  std::vector<uint32_t> stage;
  put_points(m, a.st, S_SIG, n, sigma, stage);
  const uint32_t* dtaken = m.put(taken, n);
  const uint32_t* dlist = gid ? m.put(sg.list.data(), sg.list.size()) : nullptr;
  const uint32_t* dseg = gid ? m.put(sg.seg.data(), sg.seg.size()) : nullptr;
  uint8_t* dout = (uint8_t*)m.alloc(24 * (size_t)G);
  poison(m, a);
  if (m.err != hipSuccess) return (int)m.err;
  enqueue_qc_sum(c, m.st, a, n, dtaken, gid ? &sg : nullptr, dlist, dseg, dout);
  m.sync();
  for (uint32_t k = 0; k < G; ++k) get_entry(m, sums + (size_t)72 * k, a.A, 72, gid ? 32 * sg.seg[2 * k] : 0);
  m.down(out96, dout, 96 * (size_t)G);
  m.sync();
  return (int)m.err;
}

// k_qc_apk with the product's launch shape (qc_device_batch) over a table of tn Jacobian G1
// entries (tn x 3 x 12 words, uploaded into a slab of the probe's own) and nq voter lists in CSR
// form: off[nq + 1] nondecreasing from 0, ent[off[nq]] < tn. Outputs: out (nq x 36 words: the
// homogeneous (X Z : Y : Z^3)) and flags[nq].
int qp_apk(uint32_t tn, const uint32_t* table, uint32_t nq, const uint32_t* off, const uint32_t* ent, uint32_t* out,
           uint32_t* flags) {
  if (tn == 0 || tn > QP_NMAX || nq == 0 || nq > QP_NMAX || !table || !off || !out || !flags) return QP_BAD;
  if (off[0] != 0) return QP_BAD;
  for (uint32_t q = 0; q < nq; ++q)
    if (off[q + 1] < off[q] || off[q + 1] > QP_NMAX) return QP_BAD;
  const uint32_t total = off[nq];
  if (total && !ent) return QP_BAD;
  for (uint32_t k = 0; k < total; ++k)
    if (ent[k] >= tn) return QP_BAD;
  std::lock_guard<std::mutex> g(g_qp_mu);
  int err = 0;
  ovh_ctx* c = qp_ctx(&err);
  if (!c) return err;
  Qp m(c->stream);
  std::vector<uint32_t> stage((size_t)36 * tn), res((size_t)36 * nq);
  for (uint32_t e = 0; e < tn; ++e)
    for (uint32_t r = 0; r < 36; ++r) stage[(size_t)r * tn + e] = table[(size_t)e * 36 + r];
  const Slab tab{m.put(stage.data(), stage.size()), tn};
  const Slab apk{m.alloc((size_t)36 * nq), nq};
  const uint32_t* doff = m.put(off, (size_t)nq + 1);
  const uint32_t* dent = total ? m.put(ent, total) : m.alloc(1);
  uint32_t* dflags = m.alloc(nq);
  if (m.err != hipSuccess) return (int)m.err;
  k_qc_apk<<<nq, 64, 0, m.st>>>(nq, doff, dent, tab, apk, dflags);
  m.sync();
  m.down(res.data(), apk.p, res.size() * 4);
  m.down(flags, dflags, (size_t)nq * 4);
  m.sync();
  if (m.err != hipSuccess) return (int)m.err;
  for (uint32_t q = 0; q < nq; ++q)
    for (uint32_t r = 0; r < 36; ++r) out[(size_t)q * 36 + r] = res[(size_t)r * nq + q];
  return 0;
}

// destroys the probe's context (the next call creates a new one)
void qp_close(void) {
  std::lock_guard<std::mutex> g(g_qp_mu);
  if (g_qp) ovh_destroy(g_qp);
  g_qp = nullptr;
}

}  // extern "C"
