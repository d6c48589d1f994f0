// Device probe for the unit-level tests of the pairing tail (tests/test_gpu_pair_kernels.py): the
// product's fold, final, final-exponentiation, bisection and same-message group kernels
// (k_vm_fold, k_vm_final, k_vm_fe, k_vm_votefe, k_vm_final1, k_vm_rs, k_vm_group, k_vm_votechk,
// k_pick_head, k_vm_gmil, k_vm_gfin of csrc/ovhip.hip) behind the product's own launch code
// (enqueue_final, enqueue_bisect) or with the product's grid and LDS sizes, on partials, Miller
// values, codes and key sums the caller chooses. Through the batch calls a test cannot choose
// them: every f there is the Miller value of a parsed vote. Test infrastructure only: built
// beside libovhip.so with the product's flags plus -DBISECT_DIRECT_MAX=32u (so that 33 to 80 votes
// take enqueue_bisect's group route), never linked into it.
//
// The conventions are msm_probe.hip's and qc_probe.hip's: the product translation unit is
// included whole and the library is linked with -Bsymbolic; every entry point takes host arrays
// and returns 0, a HIP error code, or an OVH_ERR_* of the product (100 and above); bad arguments
// are refused (hipErrorInvalidValue) without a launch. Field values are 12 words, canonical
// Montgomery limbs. A partial is 18 of them (F: 12 in the order of progs.flat12, S: X.c0, X.c1,
// Y.c0, Y.c1, Z.c0, Z.c1), entry after entry; the probe lays them out as planes. Device arrays
// that a kernel writes are filled with 0xFF words first and come back with their guard entries.
// The context is created on the first call (device 0) and kept until pp_close.
#include "../../consensus_overlord_amd/csrc/ovhip.hip"

namespace {

constexpr int PP_BAD = (int)hipErrorInvalidValue;
constexpr uint32_t PP_FOLD_MAX = 64;   // fold inputs per call (the tests use up to 17)
constexpr uint32_t PP_VOTES_MAX = 256; // votes per call (the tests use up to 80)
constexpr uint32_t PP_HASH_MAX = 256;  // distinct hashes per call (the tests use up to 70)
constexpr uint32_t PP_GUARD = 2;       // guard entries behind a kernel's output entries, guard words around codes
constexpr int PP_SLOT = 0;
static_assert(BISECT_DIRECT_MAX == 32u, "the probe is compiled with -DBISECT_DIRECT_MAX=32u");

ovh_ctx* g_pp = nullptr;
std::mutex g_pp_mu;

ovh_ctx* pp_ctx(int* err) {
  if (!g_pp) g_pp = ovh_create(0, nullptr, 0, 0);
  *err = !g_pp || hipSetDevice(g_pp->device) != hipSuccess ? OVH_ERR_DEVICE : 0;
  return *err ? nullptr : g_pp;
}

struct Pp {
  hipStream_t st;
  hipError_t err = hipSuccess;
  std::vector<void*> mem;
  std::vector<std::vector<uint32_t>> stages;  // host staging of the copies in flight
  explicit Pp(hipStream_t s) : st(s) {}
  ~Pp() {
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
  void fill(void* p, size_t words) {
    if (err == hipSuccess && words) err = hipMemsetAsync(p, 0xFF, words * 4, st);
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
    std::vector<uint32_t> stage((size_t)rows * n);
    if (err == hipSuccess)
      err = hipMemcpy2D(stage.data(), (size_t)n * 4, src + at, (size_t)cap * 4, (size_t)n * 4, rows, hipMemcpyDeviceToHost);
    if (err != hipSuccess) return;
    for (uint32_t i = 0; i < n; ++i)
      for (uint32_t r = 0; r < rows; ++r) out[(size_t)i * rows + r] = stage[(size_t)r * n + i];
  }
  // a device word holding v (gate and verdict words), or null for mode < 0
  int32_t* word(int mode) {
    if (mode < 0) return nullptr;
    const int32_t v = mode;
    stages.emplace_back(1, (uint32_t)v);
    return (int32_t*)put(stages.back().data(), 1);
  }
  // launch errors, then the kernels' own
  void sync() {
    if (err == hipSuccess) err = hipGetLastError();
    if (err == hipSuccess) err = hipStreamSynchronize(st);
  }
};

constexpr uint32_t PART_W = PART_PLANES * 12;  // words of a partial
constexpr uint32_t F_W = 12 * 12;              // words of an Fp12
constexpr uint32_t G2P_W = 6 * 12;             // words of a projective G2 point

}  // namespace

extern "C" {

uint32_t pp_guard(void) { return PP_GUARD; }
uint32_t pp_fold_units(void) { return VM_FOLD_UNITS; }
uint32_t pp_direct_max(void) { return BISECT_DIRECT_MAX; }

// k_vm_fold<1> (wide = 0: grid ceil(m / 4), LDS_FOLD1) or k_vm_fold<VM_FOLD_UNITS> (wide = 1: grid
// ceil(ceil(m / 4) / VM_FOLD_UNITS), LDS_FOLD) over m partials (m x 216 words; codes[m] or null;
// with_s = 0: inS.p null) under a gate word (gate < 0: null, else its value). out: ceil(m / 4) +
// pp_guard() partials, the device array filled with 0xFF words first.
int pp_fold(int wide, uint32_t m, const uint32_t* parts, const int32_t* codes, int with_s, int gate, uint32_t* out) {
  if (m == 0 || m > PP_FOLD_MAX || !parts || !out || gate > 1) return PP_BAD;
  std::lock_guard<std::mutex> g(g_pp_mu);
  int err = 0;
  ovh_ctx* c = pp_ctx(&err);
  if (!c) return err;
  const uint32_t mo = (m + 3) / 4, ocap = mo + PP_GUARD;
  Pp p(c->stream);
  uint32_t* in = p.alloc((size_t)PART_W * m);
  uint32_t* dout = p.alloc((size_t)PART_W * ocap);
  p.put_planes(in, m, PART_W, m, parts);
  const int32_t* dcodes = codes ? (const int32_t*)p.put(codes, m) : nullptr;
  const int32_t* dgate = p.word(gate);
  if (p.err != hipSuccess) return (int)p.err;
  const Slab inF{in, m}, inS{with_s ? in + (size_t)F_W * m : nullptr, with_s ? m : 0u}, o{dout, ocap};
  if (wide)
    k_vm_fold<VM_FOLD_UNITS><<<(mo + VM_FOLD_UNITS - 1) / VM_FOLD_UNITS, 64, LDS_FOLD, p.st>>>(m, c->vm_fold, c->vm_consts,
                                                                                             inF, inS, o, dcodes, dgate);
  else
    k_vm_fold<1><<<mo, 64, LDS_FOLD1, p.st>>>(m, c->vm_fold, c->vm_consts, inF, inS, o, dcodes, dgate);
  p.sync();
  p.get_planes(out, dout, ocap, PART_W, ocap);
  return (int)p.err;
}

// enqueue_final over m <= 4 partials (m x 216 words), xs: the 72 words of partial 0's S given
// apart (the batch's MSM result), or null. *verdict: the word k_vm_final wrote (0xFFFFFFFF first).
int pp_final(uint32_t m, const uint32_t* parts, const uint32_t* xs, int32_t* verdict) {
  if (m == 0 || m > 4 || !parts || !verdict) return PP_BAD;
  std::lock_guard<std::mutex> g(g_pp_mu);
  int err = 0;
  ovh_ctx* c = pp_ctx(&err);
  if (!c) return err;
  Pp p(c->stream);
  uint32_t* in = p.alloc((size_t)PART_W * m);
  p.put_planes(in, m, PART_W, m, parts);
  uint32_t* dxs = xs ? p.put(xs, G2P_W) : nullptr;
  int32_t* dres = (int32_t*)p.alloc(1);
  if (p.err != hipSuccess) return (int)p.err;
  enqueue_final(c, p.st, Slab{in, m}, Slab{in + (size_t)F_W * m, m}, m, dres, Slab{dxs, dxs ? 1u : 0u});
  p.sync();
  p.down(verdict, dres, 4);
  p.sync();
  return (int)p.err;
}

// k_vm_fe on one Fp12 (144 words) -> *verdict (0xFFFFFFFF first)
int pp_fe(const uint32_t* f, int32_t* verdict) {
  if (!f || !verdict) return PP_BAD;
  std::lock_guard<std::mutex> g(g_pp_mu);
  int err = 0;
  ovh_ctx* c = pp_ctx(&err);
  if (!c) return err;
  Pp p(c->stream);
  uint32_t* in = p.put(f, F_W);
  int32_t* dres = (int32_t*)p.alloc(1);
  if (p.err != hipSuccess) return (int)p.err;
  k_vm_fe<<<1, 64, LDS_FINAL1, p.st>>>(c->vm_final1, c->vm_consts, Slab{in, 1}, dres);
  p.sync();
  p.down(verdict, dres, 4);
  p.sync();
  return (int)p.err;
}

// k_vm_final1 on one Fp12 with the code word *code and the verdict word *verdict as given
int pp_final1(const uint32_t* f, int32_t* code, int32_t* verdict) {
  if (!f || !code || !verdict) return PP_BAD;
  std::lock_guard<std::mutex> g(g_pp_mu);
  int err = 0;
  ovh_ctx* c = pp_ctx(&err);
  if (!c) return err;
  Pp p(c->stream);
  uint32_t* in = p.put(f, F_W);
  int32_t* dcode = (int32_t*)p.put(code, 1);
  int32_t* dres = (int32_t*)p.put(verdict, 1);
  if (p.err != hipSuccess) return (int)p.err;
  k_vm_final1<<<1, 64, LDS_FINAL1, p.st>>>(c->vm_final1, c->vm_consts, Slab{in, 1}, dcode, dres);
  p.sync();
  p.down(code, dcode, 4);
  p.down(verdict, dres, 4);
  p.sync();
  return (int)p.err;
}

// k_vm_votefe with the product's grid (one wave per vote) over n votes whose f (n x 144 words) go
// to the S_F planes of the state slab; codes: n words with pp_guard() words on both sides, in and
// out; verdict: the value of the verdict word (0 or 1; the kernel takes no null).
int pp_votefe(uint32_t n, const uint32_t* f, int32_t* codes, int verdict) {
  if (n == 0 || n > PP_VOTES_MAX || !f || !codes || verdict < 0 || verdict > 1) return PP_BAD;
  std::lock_guard<std::mutex> g(g_pp_mu);
  int err = 0;
  ovh_ctx* c = pp_ctx(&err);
  if (!c) return err;
  if ((err = ensure_cap(c, n)) != 0) return err;
  Pp p(c->stream);
  const Slab s{c->state_slot[PP_SLOT], c->cap};
  p.fill(s.p, (size_t)S_TOTAL * 12 * s.cap);
  p.put_planes(s.p + (size_t)S_F * 12 * s.cap, s.cap, F_W, n, f);
  int32_t* dcodes = (int32_t*)p.put(codes, n + 2 * PP_GUARD);
  const int32_t* dres = p.word(verdict);
  if (p.err != hipSuccess) return (int)p.err;
  k_vm_votefe<<<n, 64, LDS_FINAL1, p.st>>>(n, c->vm_final1, c->vm_consts, s, dcodes + PP_GUARD, dres);
  p.sync();
  p.down(codes, dcodes, (size_t)(n + 2 * PP_GUARD) * 4);
  p.sync();
  return (int)p.err;
}

// enqueue_bisect as compiled (direct route up to pp_direct_max() votes, the group route above) on n
// votes given by their stored state: st8 (n x 96 words: sigma affine, tau affine -> S_SIG, S_TAU)
// and f (n x 144 words -> S_F), RLC values vote_scalar(seed, base, i). The rest of the state slab,
// the fold regions and grp_ok are filled with 0xFF words first. codes: n words with pp_guard()
// words on both sides, in and out. verdict < 0: a null verdict pointer, else the word's value.
// grp_ok: ceil(n / 16) words out.
int pp_bisect(uint32_t n, uint64_t seed, uint64_t base, const uint32_t* st8, const uint32_t* f, int32_t* codes, int verdict,
              int32_t* grp_ok) {
  if (n == 0 || n > PP_VOTES_MAX || !st8 || !f || !codes || !grp_ok || verdict > 1 || base == UNIT_BASE) return PP_BAD;
  std::lock_guard<std::mutex> g(g_pp_mu);
  int err = 0;
  ovh_ctx* c = pp_ctx(&err);
  if (!c) return err;
  if ((err = ensure_cap(c, n)) != 0) return err;
  const uint32_t ng = groups_of(n);
  if (ng > c->cap / GROUP_VOTES + 1 || (n + 3) / 4 > c->red_cap) return OVH_ERR_ARG;
  Pp p(c->stream);
  const Slab s{c->state_slot[PP_SLOT], c->cap};
  p.fill(s.p, (size_t)S_TOTAL * 12 * s.cap);
  p.fill(c->red_slot[PP_SLOT], c->red_w);
  p.fill(c->grp_ok[PP_SLOT], (size_t)c->cap / GROUP_VOTES + 1);
  p.put_planes(s.p + (size_t)S_SIG * 12 * s.cap, s.cap, 96, n, st8);
  p.put_planes(s.p + (size_t)S_F * 12 * s.cap, s.cap, F_W, n, f);
  int32_t* dcodes = (int32_t*)p.put(codes, n + 2 * PP_GUARD);
  const int32_t* dres = p.word(verdict);
  if (p.err != hipSuccess) return (int)p.err;
  c->slot_seed[PP_SLOT] = seed;
  c->slot_base[PP_SLOT] = base;
  enqueue_bisect(c, p.st, PP_SLOT, n, dcodes + PP_GUARD, dres);
  p.sync();
  p.down(codes, dcodes, (size_t)(n + 2 * PP_GUARD) * 4);
  p.down(grp_ok, c->grp_ok[PP_SLOT], (size_t)ng * 4);
  p.sync();
  return (int)p.err;
}

// k_pick_head, k_vm_gmil (when G > 1) and k_vm_gfin with the product's launch shapes over G
// distinct hashes: head[G] < np indexes the key sums P (np x 36 words: X, Y, Z), gh the hashes' H
// (G x 72 words), ghinf[G] their H = O flags; F (144 words, or null: F.p null) and S (72 words)
// are gfin's. Outputs: *sel (k_pick_head's choice), fout ((G + pp_guard()) x 144 words: the group
// slab's f planes, 0xFF where no kernel wrote), *verdict (0xFFFFFFFF first).
int pp_group(uint32_t G, const uint32_t* head, uint32_t np, const uint32_t* P, const uint32_t* gh, const uint32_t* ghinf,
             const uint32_t* F, const uint32_t* S, uint32_t* sel, uint32_t* fout, int32_t* verdict) {
  if (G == 0 || G > PP_HASH_MAX || np == 0 || np > PP_HASH_MAX || !head || !P || !gh || !ghinf || !S || !sel || !fout ||
      !verdict)
    return PP_BAD;
  for (uint32_t q = 0; q < G; ++q)
    if (head[q] >= np) return PP_BAD;
  std::lock_guard<std::mutex> g(g_pp_mu);
  int err = 0;
  ovh_ctx* c = pp_ctx(&err);
  if (!c) return err;
  Pp p(c->stream);
  const uint32_t gcap = G + PP_GUARD;
  const Slab gs{p.alloc((size_t)VM_G_PLANES * 12 * gcap), gcap};
  const Slab gH{gs.p + (size_t)VM_G_H * 12 * gcap, gcap};
  const Slab Ps{p.alloc((size_t)36 * np), np};
  p.put_planes(gH.p, gcap, G2P_W, G, gh);
  p.put_planes(Ps.p, np, 36, np, P);
  const uint32_t* dhead = p.put(head, G);
  const uint32_t* dinf = p.put(ghinf, G);
  uint32_t* dF = F ? p.put(F, F_W) : nullptr;
  uint32_t* dS = p.put(S, G2P_W);
  uint32_t* dsel = p.alloc(1);
  int32_t* dres = (int32_t*)p.alloc(1);
  if (p.err != hipSuccess) return (int)p.err;
  k_pick_head<<<1, 64, 0, p.st>>>(G, dhead, Ps, dinf, dsel);
  if (G > 1) k_vm_gmil<<<G, 64, LDS_GMIL, p.st>>>(G, dsel, c->vm_gmil, c->vm_consts, dhead, Ps, gs);
  k_vm_gfin<<<1, 64, LDS_GFIN, p.st>>>(c->vm_gfin, c->vm_consts, Slab{dF, dF ? 1u : 0u}, dhead, dsel, Ps, gH, Slab{dS, 1},
                                      dres);
  p.sync();
  p.down(sel, dsel, 4);
  p.down(verdict, dres, 4);
  p.sync();
  p.get_planes(fout, gs.p + (size_t)VM_G_F * 12 * gcap, gcap, F_W, gcap);
  return (int)p.err;
}

// destroys the probe's context (the next call creates a new one)
void pp_close(void) {
  std::lock_guard<std::mutex> g(g_pp_mu);
  if (g_pp) ovh_destroy(g_pp);
  g_pp = nullptr;
}

}  // extern "C"
