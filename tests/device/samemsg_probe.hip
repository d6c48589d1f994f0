// Device probe for the unit-level tests of the same-message path (tests/test_gpu_samemsg_kernels.py):
// the kernels and host code that build the left-hand factor of
//   prod_g e(sum_{i in g} r_i pk_i, H_g) * e(-G1, sum_i r_i sigma_i) == 1
// (k_vm_vsame<TABLE, W> in its four instantiations, k_samemsg_fix, samemsg_plan, k_vm_g1pairs,
// k_h2f + k_vm_h2g, k_vm_vote1h_b<TABLE> + k_vm_votefe of csrc/ovhip.hip) with the grid and LDS
// sizes of verify_samemsg_locked, on votes, key sums, plans and codes the caller chooses, and the
// whole path (ovh_verify_batch on a context that routes every batch of two or more votes to it)
// with the batch's verdict and intermediate values read back from the slot it used. Through the
// batch calls alone a test sees only codes, which the bisection repairs when the combined check
// fails for a wrong reason. Test infrastructure only: built beside libovhip.so with the product's
// flags plus -DVSAME8_MIN=16u (so that a batch of 16 votes or more takes the 8-lane programs and a
// smaller one the 16-lane ones), never linked into it.
//
// The conventions are pair_probe.hip's: the product translation unit is included whole and the
// library is linked with -Bsymbolic; every entry point takes host arrays and returns 0, a HIP
// error code, or an OVH_ERR_* of the product (100 and above); an index a kernel would follow out of
// its buffers (table index >= table cap, gid >= G, pair or head >= n, n above SP_VOTES_MAX) is
// refused (hipErrorInvalidValue) without a launch. Field values are 12 words, canonical Montgomery
// limbs; points are given entry after entry and laid out as planes here. Device arrays that a
// kernel writes are filled with 0xFF words first and come back with their guard entries. The
// contexts are created on the first call (device 0) and kept until sp_close.
#include "../../consensus_overlord_amd/csrc/ovhip.hip"

namespace {

constexpr int SP_BAD = (int)hipErrorInvalidValue;
constexpr uint32_t SP_VOTES_MAX = 256;  // votes per call (the tests use up to 201)
constexpr uint32_t SP_TAB_MAX = 64;     // validator-table entries per call
constexpr uint32_t SP_GUARD = 2;        // guard entries behind a kernel's output entries
static_assert(VSAME8_MIN == 16u, "the probe is compiled with -DVSAME8_MIN=16u");

ovh_ctx* g_sp = nullptr;   // the kernels' programs and constants
ovh_ctx* g_spb = nullptr;  // sp_batch: OVH_FLAG_TEST_RLC, same-message routing at any size
std::mutex g_sp_mu;

ovh_ctx* sp_ctx(int* err) {
  if (!g_sp) g_sp = ovh_create(0, nullptr, 0, 0);
  *err = !g_sp || hipSetDevice(g_sp->device) != hipSuccess ? OVH_ERR_DEVICE : 0;
  return *err ? nullptr : g_sp;
}

struct Sp {
  hipStream_t st;
  hipError_t err = hipSuccess;
  std::vector<void*> mem;
  std::vector<std::vector<uint32_t>> stages;  // host staging of the copies in flight
  explicit Sp(hipStream_t s) : st(s) {}
  ~Sp() {
    (void)hipStreamSynchronize(st);
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
  void up(void* dst, const void* src, size_t bytes) {
    if (err == hipSuccess && bytes) err = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
  }
  void down(void* dst, const void* src, size_t bytes) {
    if (err == hipSuccess && bytes) err = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
  }
  uint32_t* put(const void* src, size_t words) {
    uint32_t* p = alloc(words);
    up(p, src, words * 4);
    return p;
  }
  uint8_t* put_bytes(const void* src, size_t bytes) {
    uint8_t* p = (uint8_t*)alloc((bytes + 3) / 4);
    up(p, src, bytes);
    return p;
  }
  // n entries of `rows` words each (entry after entry) -> rows limb rows of a slab of capacity cap,
  // from entry index `at`
  void put_planes(uint32_t* dst, uint32_t cap, uint32_t rows, uint32_t n, const uint32_t* src, uint32_t at = 0) {
    if (!n) return;
    stages.emplace_back((size_t)rows * n);
    std::vector<uint32_t>& stage = stages.back();
    for (uint32_t i = 0; i < n; ++i)
      for (uint32_t r = 0; r < rows; ++r) stage[(size_t)r * n + i] = src[(size_t)i * rows + r];
    if (err == hipSuccess)
      err = hipMemcpy2DAsync(dst + at, (size_t)cap * 4, stage.data(), (size_t)n * 4, (size_t)n * 4, rows,
                             hipMemcpyHostToDevice, st);
  }
  // the reverse, after a sync: n entries from entry index `at`
  void get_planes(uint32_t* out, const uint32_t* src, uint32_t cap, uint32_t rows, uint32_t n, uint32_t at = 0) {
    if (!n) return;
    std::vector<uint32_t> stage((size_t)rows * n);
    if (err == hipSuccess)
      err = hipMemcpy2D(stage.data(), (size_t)n * 4, src + at, (size_t)cap * 4, (size_t)n * 4, rows, hipMemcpyDeviceToHost);
    if (err != hipSuccess) return;
    for (uint32_t i = 0; i < n; ++i)
      for (uint32_t r = 0; r < rows; ++r) out[(size_t)i * rows + r] = stage[(size_t)r * n + i];
  }
  // launch errors, then the kernels' own
  void sync() {
    if (err == hipSuccess) err = hipGetLastError();
    if (err == hipSuccess) err = hipStreamSynchronize(st);
  }
};

constexpr uint32_t G1P_W = 3 * 12;   // words of a projective G1 point
constexpr uint32_t G2P_W = 6 * 12;   // words of a projective G2 point
constexpr uint32_t F_W = 12 * 12;    // words of an Fp12
constexpr uint32_t VS_W = 11 * 12;   // words sp_vsame returns per entry: sigma, tau, r pk

// A caller-given validator table on the device: tcap entries of X, Y, Z (36 words each) and their
// flags; idx: cnt table indices, each below tcap (checked by the caller of this).
PkSrc sp_table(Sp& p, uint32_t tcap, const uint32_t* planes, const uint32_t* flags, const int32_t* idx, uint32_t cnt) {
  uint32_t* dp = p.alloc((size_t)G1P_W * tcap);
  p.put_planes(dp, tcap, G1P_W, tcap, planes);
  return PkSrc{dp, tcap, p.put(flags, tcap), (const int32_t*)p.put(idx, cnt)};
}

bool sp_table_ok(int table, uint32_t tcap, const uint32_t* planes, const uint32_t* flags, const int32_t* idx, uint32_t cnt,
                 const uint8_t* pks) {
  if (!table) return pks != nullptr;
  if (tcap == 0 || tcap > SP_TAB_MAX || !planes || !flags || !idx) return false;
  for (uint32_t j = 0; j < cnt; ++j)
    if (idx[j] < 0 || (uint32_t)idx[j] >= tcap) return false;
  return true;
}

}  // namespace

extern "C" {

uint32_t sp_guard(void) { return SP_GUARD; }
uint32_t sp_vsame8_min(void) { return VSAME8_MIN; }
uint32_t sp_votes_max(void) { return SP_VOTES_MAX; }

// The product's samemsg_plan on n hashes (n x 32 bytes) and perm (n words, or null: empty).
// gid: n words; ghash: up to n x 32 bytes; head: up to n words; pairs: up to 2 n words; level_off:
// up to 34 words; counts: G, the number of pairs, the number of level_off words.
int sp_plan(uint32_t n, const uint8_t* hashes, const uint32_t* perm, uint32_t* gid, uint8_t* ghash, uint32_t* head,
            uint32_t* pairs, uint32_t* level_off, uint32_t* counts) {
  if (n == 0 || n > SP_VOTES_MAX || !hashes || !gid || !ghash || !head || !pairs || !level_off || !counts) return SP_BAD;
  std::vector<uint32_t> pv;
  if (perm) {
    pv.assign(perm, perm + n);
    for (uint32_t v : pv)
      if (v >= n) return SP_BAD;
  }
  SameMsgPlan pl;
  samemsg_plan(n, hashes, pv, pl);
  if (pl.G > n || pl.pairs.size() > 2 * (size_t)n || pl.level_off.size() > 34 || pl.gid.size() != n ||
      pl.ghash.size() != 32 * (size_t)pl.G || pl.head.size() != pl.G)
    return OVH_ERR_ARG;
  memcpy(gid, pl.gid.data(), 4 * (size_t)n);
  memcpy(ghash, pl.ghash.data(), pl.ghash.size());
  memcpy(head, pl.head.data(), 4 * (size_t)pl.G);
  if (!pl.pairs.empty()) memcpy(pairs, pl.pairs.data(), 4 * pl.pairs.size());
  memcpy(level_off, pl.level_off.data(), 4 * pl.level_off.size());
  counts[0] = pl.G;
  counts[1] = (uint32_t)(pl.pairs.size() / 2);
  counts[2] = (uint32_t)pl.level_off.size();
  return 0;
}

// k_vm_vsame<table, w8 ? 8 : 16> with the grid and LDS size of verify_samemsg_locked over cnt votes
// at slab indices lo .. lo + cnt - 1: sigs (cnt x 96 bytes), pks (cnt x 48 bytes; table = 0) or the
// table (tcap entries x 36 words, tflags[tcap], tidx[cnt]; table = 1), RLC values
// vote_scalar(seed, base, lo + j). The slab has lo + cnt + sp_guard() entries, 0xFF first. codes:
// that many words, in and out. out: per entry 132 words (S_SIG 4 planes, S_TAU 4, S_F 0..2).
int sp_vsame(int table, int w8, uint32_t cnt, uint32_t lo, const uint8_t* sigs, const uint8_t* pks, uint32_t tcap,
             const uint32_t* tplanes, const uint32_t* tflags, const int32_t* tidx, uint64_t seed, uint64_t base,
             int32_t* codes, uint32_t* out) {
  if (cnt == 0 || cnt > SP_VOTES_MAX || lo > SP_VOTES_MAX || !sigs || !codes || !out || base == UNIT_BASE ||
      !sp_table_ok(table, tcap, tplanes, tflags, tidx, cnt, pks))
    return SP_BAD;
  std::lock_guard<std::mutex> g(g_sp_mu);
  int err = 0;
  ovh_ctx* c = sp_ctx(&err);
  if (!c) return err;
  Sp p(c->stream);
  const uint32_t cap = lo + cnt + SP_GUARD;
  const Slab s{p.alloc((size_t)S_TOTAL * 12 * cap), cap};
  const uint8_t* dsigs = p.put_bytes(sigs, (size_t)96 * cnt);
  int32_t* dc = (int32_t*)p.put(codes, cap);
  const uint8_t* dpks = nullptr;
  PkSrc tab{};
  if (table) tab = sp_table(p, tcap, tplanes, tflags, tidx, cnt);
  else dpks = p.put_bytes(pks, (size_t)48 * cnt);
  if (p.err != hipSuccess) return (int)p.err;
  const hipStream_t st = p.st;
  if (w8) {
    if (table)
      k_vm_vsame<true, 8><<<(cnt + 7) / 8, 64, LDS_VSAME8, st>>>(cnt, lo, c->vm_vsame8_t, c->vm_consts, nullptr, tab, dsigs,
                                                                 s, seed, base, dc);
    else
      k_vm_vsame<false, 8><<<(cnt + 7) / 8, 64, LDS_VSAME8, st>>>(cnt, lo, c->vm_vsame8, c->vm_consts, dpks, PkSrc{}, dsigs,
                                                                  s, seed, base, dc);
  } else {
    if (table)
      k_vm_vsame<true><<<(cnt + VM_SLICES - 1) / VM_SLICES, 64, LDS_VSAME, st>>>(cnt, lo, c->vm_vsame_t, c->vm_consts,
                                                                                nullptr, tab, dsigs, s, seed, base, dc);
    else
      k_vm_vsame<false><<<(cnt + VM_SLICES - 1) / VM_SLICES, 64, LDS_VSAME, st>>>(cnt, lo, c->vm_vsame, c->vm_consts, dpks,
                                                                                 PkSrc{}, dsigs, s, seed, base, dc);
  }
  p.sync();
  p.down(codes, dc, (size_t)cap * 4);
  p.sync();
  std::vector<uint32_t> part((size_t)cap * 48);
  for (uint32_t k = 0; k < 3; ++k) {  // S_SIG, S_TAU (4 planes each), S_F 0..2
    const uint32_t plane = k == 0 ? S_SIG : k == 1 ? S_TAU : S_F, rows = k == 2 ? 36 : 48, at = k * 48;
    p.get_planes(part.data(), s.p + (size_t)plane * 12 * cap, cap, rows, cap);
    for (uint32_t i = 0; i < cap && p.err == hipSuccess; ++i)
      memcpy(out + (size_t)i * VS_W + at, part.data() + (size_t)i * rows, (size_t)rows * 4);
  }
  return (int)p.err;
}

// k_samemsg_fix, then the k_vm_g1pairs levels exactly as verify_samemsg_locked launches them, over n
// votes: gid[n] < G, ghinf[G], the plan's pairs (npairs x 2, every index < n) and level_off (nlo
// words: 0 first, npairs last, non-decreasing). codes: n + sp_guard() words, in and out. P: (n +
// sp_guard()) x 36 words (X, Y, Z of every entry), in and out.
int sp_keysums(uint32_t n, const uint32_t* gid, uint32_t G, const uint32_t* ghinf, int32_t* codes, uint32_t* P,
               uint32_t npairs, const uint32_t* pairs, uint32_t nlo, const uint32_t* level_off) {
  if (n == 0 || n > SP_VOTES_MAX || G == 0 || G > n || !gid || !ghinf || !codes || !P || !level_off || nlo == 0 || nlo > 34 ||
      npairs > n || (npairs && !pairs) || level_off[0] != 0 || level_off[nlo - 1] != npairs)
    return SP_BAD;
  for (uint32_t i = 0; i < n; ++i)
    if (gid[i] >= G) return SP_BAD;
  for (uint32_t k = 0; k < 2 * npairs; ++k)
    if (pairs[k] >= n) return SP_BAD;
  for (uint32_t l = 0; l + 1 < nlo; ++l)
    if (level_off[l] > level_off[l + 1]) return SP_BAD;
  std::lock_guard<std::mutex> g(g_sp_mu);
  int err = 0;
  ovh_ctx* c = sp_ctx(&err);
  if (!c) return err;
  Sp p(c->stream);
  const uint32_t cap = n + SP_GUARD;
  const Slab Ps{p.alloc((size_t)G1P_W * cap), cap};
  p.put_planes(Ps.p, cap, G1P_W, cap, P);
  const uint32_t* dgid = p.put(gid, n);
  const uint32_t* dinf = p.put(ghinf, G);
  int32_t* dc = (int32_t*)p.put(codes, cap);
  const uint32_t* dpairs = p.put(pairs, 2 * (size_t)npairs);
  if (p.err != hipSuccess) return (int)p.err;
  k_samemsg_fix<<<nblk(n), WG, 0, p.st>>>(n, dgid, dinf, dc, Ps);
  for (uint32_t l = 0; l + 1 < nlo; ++l) {
    const uint32_t a = level_off[l], np = level_off[l + 1] - a;
    k_vm_g1pairs<<<(np + 64 / VM_G1PADD_W - 1) / (64 / VM_G1PADD_W), 64, LDS_G1PADD, p.st>>>(
        np, c->vm_g1padd, G1PADD_STRIDE_W, c->vm_consts, dpairs + 2 * (size_t)a, Ps);
  }
  p.sync();
  p.down(codes, dc, (size_t)cap * 4);
  p.sync();
  p.get_planes(P, Ps.p, cap, G1P_W, cap);
  return (int)p.err;
}

// k_h2f (hashes: G x 32 bytes) or caller-given u planes (u: G x 48 words: u0.c0, u0.c1, u1.c0,
// u1.c1; hashes null), then k_vm_h2g with the product's launch shape. H: (G + sp_guard()) x 72
// words; ghinf: G + sp_guard() words; both 0xFF where no kernel wrote.
int sp_h2g(uint32_t G, const uint8_t* hashes, const uint32_t* u, uint32_t* H, uint32_t* ghinf) {
  if (G == 0 || G > SP_VOTES_MAX || (!hashes && !u) || (hashes && u) || !H || !ghinf) return SP_BAD;
  std::lock_guard<std::mutex> g(g_sp_mu);
  int err = 0;
  ovh_ctx* c = sp_ctx(&err);
  if (!c) return err;
  Sp p(c->stream);
  const uint32_t cap = G + SP_GUARD;
  const Slab gs{p.alloc((size_t)VM_G_PLANES * 12 * cap), cap};
  uint32_t* dinf = p.alloc(cap);
  const uint8_t* dh = hashes ? p.put_bytes(hashes, (size_t)32 * G) : nullptr;
  if (u) p.put_planes(gs.p + (size_t)VM_G_U * 12 * cap, cap, 48, G, u);
  if (p.err != hipSuccess) return (int)p.err;
  if (dh) k_h2f<<<nblk(G), WG, 0, p.st>>>(G, dh, c->xmd, gs);
  k_vm_h2g<<<(G + VM_SLICES - 1) / VM_SLICES, 64, LDS_H2G, p.st>>>(G, c->vm_h2g, c->vm_consts, gs, dinf);
  p.sync();
  p.down(ghinf, dinf, (size_t)cap * 4);
  p.sync();
  p.get_planes(H, gs.p + (size_t)VM_G_H * 12 * cap, cap, G2P_W, cap);
  return (int)p.err;
}

// k_vm_vote1h_b<table> over cnt votes at slab indices lo .. lo + cnt - 1, then k_vm_votefe over
// lo + cnt votes, with the product's launch shapes, behind a verdict word of value `verdict` (0 or
// 1: the kernels take no null). Keys as sp_vsame; gid[lo + cnt] < G; gh: G x 72 words (H of every
// hash); ghinf[G]. codes: lo + cnt + sp_guard() words, in and out. f: (lo + cnt + sp_guard()) x 144
// words out (the S_F planes, 0xFF where nothing was written).
int sp_bisect(int table, uint32_t cnt, uint32_t lo, const uint8_t* sigs, const uint8_t* pks, uint32_t tcap,
              const uint32_t* tplanes, const uint32_t* tflags, const int32_t* tidx, const uint32_t* gid, uint32_t G,
              const uint32_t* gh, const uint32_t* ghinf, int32_t* codes, int verdict, uint32_t* f) {
  if (cnt == 0 || cnt > SP_VOTES_MAX || lo > SP_VOTES_MAX || !sigs || !gid || G == 0 || G > SP_VOTES_MAX || !gh || !ghinf ||
      !codes || !f || verdict < 0 || verdict > 1 || !sp_table_ok(table, tcap, tplanes, tflags, tidx, cnt, pks))
    return SP_BAD;
  for (uint32_t i = 0; i < lo + cnt; ++i)
    if (gid[i] >= G) return SP_BAD;
  std::lock_guard<std::mutex> g(g_sp_mu);
  int err = 0;
  ovh_ctx* c = sp_ctx(&err);
  if (!c) return err;
  Sp p(c->stream);
  const uint32_t N = lo + cnt, cap = N + SP_GUARD;
  const Slab s{p.alloc((size_t)S_TOTAL * 12 * cap), cap};
  const Slab gH{p.alloc((size_t)G2P_W * G), G};
  p.put_planes(gH.p, G, G2P_W, G, gh);
  const uint8_t* dsigs = p.put_bytes(sigs, (size_t)96 * cnt);
  const uint32_t* dgid = p.put(gid, N);
  const uint32_t* dinf = p.put(ghinf, G);
  int32_t* dc = (int32_t*)p.put(codes, cap);
  const uint8_t* dpks = nullptr;
  PkSrc tab{};
  if (table) tab = sp_table(p, tcap, tplanes, tflags, tidx, cnt);
  else dpks = p.put_bytes(pks, (size_t)48 * cnt);
  const int32_t v = verdict;
  const int32_t* dres = (const int32_t*)p.put(&v, 1);
  if (p.err == hipSuccess) p.err = hipStreamSynchronize(p.st);  // &v copied
  if (p.err != hipSuccess) return (int)p.err;
  if (table)
    k_vm_vote1h_b<true><<<cnt, 64, LDS_VOTE1H, p.st>>>(cnt, lo, c->vm_vote_t1h, c->vm_consts, nullptr, tab, dsigs, s, dc, dgid,
                                                       gH, dinf, dres);
  else
    k_vm_vote1h_b<false><<<cnt, 64, LDS_VOTE1H, p.st>>>(cnt, lo, c->vm_vote1h, c->vm_consts, dpks, PkSrc{}, dsigs, s, dc, dgid,
                                                        gH, dinf, dres);
  k_vm_votefe<<<N, 64, LDS_FINAL1, p.st>>>(N, c->vm_final1, c->vm_consts, s, dc, dres);
  p.sync();
  p.down(codes, dc, (size_t)cap * 4);
  p.sync();
  p.get_planes(f, s.p + (size_t)S_F * 12 * cap, cap, F_W, cap);
  return (int)p.err;
}

// ovh_verify_batch of n votes on a context with OVH_FLAG_TEST_RLC, ovh_set_test_rlc(seed, base) and
// same-message routing at any size (two votes or more with at most n / 2 distinct hashes), with
// the nval keys of vals (nval x 48 bytes; 0: no table) as its validator table. OVH_ERR_ARG when the
// batch did not take the same-message path. Read back from the slot it used: codes (n, the
// caller's order); info: verdict (result[RES_BATCH + slot]), hsel, G, the number of table votes;
// perm (n words: the caller's index of staged vote j); ghinf (G words); P (n x 36 words: the S_F
// planes 0..2 of every staged vote, the key sums at the heads); f (G x 144 words: the group slab's
// f planes).
int sp_batch(uint32_t n, const uint8_t* sigs, const uint8_t* hashes, const uint8_t* pks, uint32_t nval, const uint8_t* vals,
             uint64_t seed, uint64_t base, int32_t* codes, int32_t* info, uint32_t* perm, uint32_t* ghinf, uint32_t* P,
             uint32_t* f) {
  if (n < 2 || n > SP_VOTES_MAX || !sigs || !hashes || !pks || nval > SP_TAB_MAX || (nval && !vals) || !codes || !info ||
      !perm || !ghinf || !P || !f)
    return SP_BAD;
  std::lock_guard<std::mutex> g(g_sp_mu);
  if (!g_spb) {
    g_spb = ovh_create(0, nullptr, 0, OVH_FLAG_TEST_RLC);
    if (g_spb) g_spb->samemsg = 2;
  }
  ovh_ctx* c = g_spb;
  if (!c || hipSetDevice(c->device) != hipSuccess) return OVH_ERR_DEVICE;
  CHK(ovh_set_test_rlc(c, seed, base));
  CHK(ovh_set_validators(c, vals, nval));
  const uint64_t before = c->sm_batches;
  CHK(ovh_verify_batch(c, n, sigs, hashes, pks, codes));
  if (c->sm_batches != before + 1) return OVH_ERR_ARG;
  std::vector<uint32_t> pv;
  std::vector<int32_t> tidx;
  const size_t t = table_split(c, n, pks, pv, tidx);
  SameMsgPlan pl;
  samemsg_plan(n, hashes, pv, pl);
  const int slot = c->last_slot;
  const uint32_t G = pl.G, cap = c->cap, gcap = c->gcap[slot];
  if (G == 0 || G > n || n > cap || G > gcap || !c->gslab[slot]) return OVH_ERR_ARG;
  for (uint32_t j = 0; j < n; ++j) perm[j] = pv.empty() ? j : pv[j];
  Sp p(c->stream);
  int32_t res = 0;
  uint32_t hsel = 0;
  const uint32_t* dinf = c->gslab[slot] + (size_t)VM_G_PLANES * 12 * gcap;
  p.down(&res, c->result + RES_BATCH + slot, 4);
  p.down(&hsel, dinf + gcap, 4);
  p.down(ghinf, dinf, (size_t)G * 4);
  p.sync();
  p.get_planes(P, c->state_slot[slot] + (size_t)S_F * 12 * cap, cap, G1P_W, n);
  p.get_planes(f, c->gslab[slot] + (size_t)VM_G_F * 12 * gcap, gcap, F_W, G);
  info[0] = res;
  info[1] = (int32_t)hsel;
  info[2] = (int32_t)G;
  info[3] = (int32_t)t;
  return (int)p.err;
}

// destroys the probe's contexts (the next call creates new ones)
void sp_close(void) {
  std::lock_guard<std::mutex> g(g_sp_mu);
  if (g_sp) ovh_destroy(g_sp);
  if (g_spb) ovh_destroy(g_spb);
  g_sp = g_spb = nullptr;
}

}  // extern "C"
