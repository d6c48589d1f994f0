// Host build of the DEVICE arithmetic (consensus_overlord_amd/csrc/bls/*.hpp) for CPU unit
// tests against the golden fixtures. Test infrastructure only: never linked into the
// product library, never a fallback.
#include <string.h>
#include "../../consensus_overlord_amd/csrc/bls/verify.hpp"
#include "../../consensus_overlord_amd/csrc/fpvm.hpp"
#include "../../consensus_overlord_amd/csrc/rlp.hpp"

using namespace ovh;

static const uint8_t DST[] = "BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_NUL_";

extern "C" {

// rlp(Vote) + SM3 of rlp.hpp (the k_vote_digest code) on the host
int hx_vote_rlp(uint8_t* out, uint64_t h, uint64_t r, uint8_t t, const uint8_t* bh, uint32_t bl) {
  return (int)rlp_vote(out, h, r, t, bh, bl);
}
void hx_vote_digest(uint8_t* out32, uint64_t h, uint64_t r, uint8_t t, const uint8_t* bh, uint32_t bl) {
  vote_digest(out32, h, r, t, bh, bl);
}

int hx_hash_to_g2(const uint8_t* msg32, const uint8_t* dst, size_t dst_len, uint8_t* out192) {
  XmdTemplates t;
  if (!xmd_build_templates(t, dst, dst_len)) return -1;
  uint32_t m[8];
  be_words_from_bytes(m, msg32, 8);
  G2J h;
  hash_to_g2(h, m, t);
  g2_serialize(out192, h);
  return 0;
}

// The field half of hash_to_G2 (what k_h2f runs per message): the DST's block templates,
// expand_message_xmd and hash_to_field. out192 = u0.c0, u0.c1, u1.c0, u1.c1 as 48-byte BE
// canonical values; nb = {nb0, nbi} of the templates. -1: the DST is refused.
int hx_h2f(const uint8_t* msg32, const uint8_t* dst, size_t dst_len, uint8_t* out192, uint32_t* nb) {
  XmdTemplates t;
  if (!xmd_build_templates(t, dst, dst_len)) return -1;
  uint32_t m[8], uni[64];
  be_words_from_bytes(m, msg32, 8);
  expand_message_xmd_256(uni, m, t);
  Fp2 u0, u1;
  hash_to_field_fp2x2(u0, u1, uni);
  const Fp* c[4] = {&u0.c0, &u0.c1, &u1.c0, &u1.c1};
  for (int i = 0; i < 4; ++i) fp_to_be48(out192 + 48 * i, *c[i]);
  if (nb) nb[0] = t.nb0, nb[1] = t.nbi;
  return 0;
}

// The curve half (h2c.hpp map2_to_g2) on field inputs given as hash_to_field gets them: in256 =
// four 64-byte big-endian integers (u0.c0, u0.c1, u1.c0, u1.c1), each reduced modulo p by
// fp_from_be64_words. out192 = the serialized point (0x40 || zeros for the identity).
void hx_map2_to_g2(const uint8_t* in256, uint8_t* out192) {
  uint32_t w[64];
  be_words_from_bytes(w, in256, 64);
  Fp2 u0, u1;
  hash_to_field_fp2x2(u0, u1, w);
  G2J h;
  map2_to_g2(h, u0, u1);
  g2_serialize(out192, h);
}

int hx_verify(const uint8_t* sig, uint32_t sl, const uint8_t* hash, uint32_t hl, const uint8_t* pk, uint32_t pl) {
  XmdTemplates t;
  xmd_build_templates(t, DST, 43);
  return verify_one(sig, sl, hash, hl, pk, pl, t);
}

int hx_g1_decode(const uint8_t* in, uint32_t len, uint8_t* out48, int* inf) {
  G1A a;
  bool i;
  int e = g1_from_bytes(a, i, in, len);
  *inf = i;
  if (e == 0) {
    G1J j;
    if (i) jac_set_inf(j); else jac_from_aff(j, a);
    g1_compress(out48, j);
  }
  return e;
}

int hx_g2_decode(const uint8_t* in, uint32_t len, uint8_t* out96, int* inf) {
  G2A a;
  bool i;
  int e = g2_from_bytes(a, i, in, len);
  *inf = i;
  if (e == 0) {
    G2J j;
    if (i) jac_set_inf(j); else jac_from_aff(j, a);
    g2_compress(out96, j);
  }
  return e;
}

// e(G1, G2)^3 via the device Miller loop + x-chain final exponentiation; 12 Fp2 coeffs
// (c0.c0.c0, c0.c0.c1, c0.c1.c0, ...) as 48-byte BE canonical values.
void hx_gt_g1g2(uint8_t* out576) {
  G1A p; fp_load(p.x, G1X_M); fp_load(p.y, G1Y_M);
  G2A q; q.x = fp2_const(G2X_C0, G2X_C1); q.y = fp2_const(G2Y_C0, G2Y_C1);
  Fp12 f;
  miller_loop(f, p, q);
  final_exponentiation(f, f);
  const Fp* c = &f.c0.c0.c0;
  for (int i = 0; i < 12; ++i) fp_to_be48(out576 + 48 * i, c[i]);
}

int hx_g2_subgroup(const uint8_t* in, uint32_t len) {
  G2A a; bool i;
  int e = g2_from_bytes(a, i, in, len);
  if (e) return -e;
  G2J j; jac_from_aff(j, a);
  return g2_in_subgroup(j) ? 1 : 0;
}

int hx_g1_subgroup(const uint8_t* in, uint32_t len) {
  G1A a; bool i;
  int e = g1_from_bytes(a, i, in, len);
  if (e) return -e;
  G1J j; jac_from_aff(j, a);
  return g1_in_subgroup(j) ? 1 : 0;
}

// The decoders' exact point (tests/point_cases.py): the code of g*_from_bytes, and the affine
// coordinates as 48-byte BE canonical values (G1: x, y; G2: x.c1, x.c0, y.c1, y.c0) whenever the
// decoder set the point: code 0 (not infinity), and code 3 for x = 0.
int hx_g1_decode_xy(const uint8_t* in, uint32_t len, uint8_t* out96, int* inf) {
  G1A a;
  bool i;
  int e = g1_from_bytes(a, i, in, len);
  *inf = i;
  if ((e == 0 && !i) || e == BLST_POINT_NOT_IN_GROUP) {
    fp_to_be48(out96, a.x);
    fp_to_be48(out96 + 48, a.y);
  }
  return e;
}

int hx_g2_decode_xy(const uint8_t* in, uint32_t len, uint8_t* out192, int* inf) {
  G2A a;
  bool i;
  int e = g2_from_bytes(a, i, in, len);
  *inf = i;
  if ((e == 0 && !i) || e == BLST_POINT_NOT_IN_GROUP) {
    fp_to_be48(out192, a.x.c1);
    fp_to_be48(out192 + 48, a.x.c0);
    fp_to_be48(out192 + 96, a.y.c1);
    fp_to_be48(out192 + 144, a.y.c0);
  }
  return e;
}

// The subgroup checks on an affine point given by its coordinates (layout as above), past the
// decoder: the order-3 points (0, +-2) reach the ladders this way. -1: a coordinate >= p.
int hx_g1_subgroup_xy(const uint8_t* xy96) {
  G1A a;
  if (!fp_from_be48_masked(a.x, xy96, false) || !fp_from_be48_masked(a.y, xy96 + 48, false)) return -1;
  G1J j; jac_from_aff(j, a);
  return g1_in_subgroup(j) ? 1 : 0;
}

int hx_g2_subgroup_xy(const uint8_t* xy192) {
  G2A a;
  if (!fp_from_be48_masked(a.x.c1, xy192, false) || !fp_from_be48_masked(a.x.c0, xy192 + 48, false) ||
      !fp_from_be48_masked(a.y.c1, xy192 + 96, false) || !fp_from_be48_masked(a.y.c0, xy192 + 144, false))
    return -1;
  G2J j; jac_from_aff(j, a);
  return g2_in_subgroup(j) ? 1 : 0;
}

// [|x|] P by jac_mul_xabs, the ladder of both subgroup checks, on an affine point (layout as
// above): 0 and the affine result, 1 for the identity, -1 for a coordinate >= p.
int hx_g1_mul_xabs_xy(const uint8_t* xy96, uint8_t* out96) {
  G1A a;
  if (!fp_from_be48_masked(a.x, xy96, false) || !fp_from_be48_masked(a.y, xy96 + 48, false)) return -1;
  G1J j, r;
  jac_from_aff(j, a);
  jac_mul_xabs(r, j);
  if (!jac_to_aff(a, r)) return 1;
  fp_to_be48(out96, a.x);
  fp_to_be48(out96 + 48, a.y);
  return 0;
}

int hx_g2_mul_xabs_xy(const uint8_t* xy192, uint8_t* out192) {
  G2A a;
  if (!fp_from_be48_masked(a.x.c1, xy192, false) || !fp_from_be48_masked(a.x.c0, xy192 + 48, false) ||
      !fp_from_be48_masked(a.y.c1, xy192 + 96, false) || !fp_from_be48_masked(a.y.c0, xy192 + 144, false))
    return -1;
  G2J j, r;
  jac_from_aff(j, a);
  jac_mul_xabs(r, j);
  if (!jac_to_aff(a, r)) return 1;
  fp_to_be48(out192, a.x.c1);
  fp_to_be48(out192 + 48, a.x.c0);
  fp_to_be48(out192 + 96, a.y.c1);
  fp_to_be48(out192 + 144, a.y.c0);
  return 0;
}

// The one-lane tower and pairing (bls/tower.hpp, bls/pairing.hpp) on crafted operands
// (tests/pairing_cases.py). An Fp12 is its 12 Fp coefficients (c0.c0.c0, c0.c0.c1, c0.c1.c0, ...)
// as 48-byte BE canonical values. -1: a coefficient >= p; -2: an unknown op.
static bool ld_fps(Fp* r, const uint8_t* in, int n) {
  for (int i = 0; i < n; ++i)
    if (!fp_from_be48_masked(r[i], in + 48 * i, false)) return false;
  return true;
}
static void st_f12(uint8_t* out576, const Fp12& f) {
  const Fp* c = &f.c0.c0.c0;
  for (int i = 0; i < 12; ++i) fp_to_be48(out576 + 48 * i, c[i]);
}

// op 0: a * b; 1: a^2 (fp12_sqr); 2: fp12_cyc_sqr; 3: fp12_frob; 4: fp12_inv; 5: fp12_cyc_exp_x;
// 6: final_exponentiation. b is read by op 0 only.
int hx_fp12_op(int op, const uint8_t* a576, const uint8_t* b576, uint8_t* out576) {
  Fp12 a, b, r;
  if (!ld_fps(&a.c0.c0.c0, a576, 12)) return -1;
  switch (op) {
    case 0:
      if (!ld_fps(&b.c0.c0.c0, b576, 12)) return -1;
      fp12_mul(r, a, b);
      break;
    case 1: fp12_sqr(r, a); break;
    case 2: fp12_cyc_sqr(r, a); break;
    case 3: fp12_frob(r, a); break;
    case 4: fp12_inv(r, a); break;
    case 5: fp12_cyc_exp_x(r, a); break;
    case 6: final_exponentiation(r, a); break;
    default: return -2;
  }
  st_f12(out576, r);
  return 0;
}

// f * (l0 + l1 v + l4 v w); l288 = l0.c0, l0.c1, l1.c0, l1.c1, l4.c0, l4.c1
int hx_fp12_mul_by_014(const uint8_t* f576, const uint8_t* l288, uint8_t* out576) {
  Fp12 f;
  Fp2 l[3];
  if (!ld_fps(&f.c0.c0.c0, f576, 12) || !ld_fps(&l[0].c0, l288, 6)) return -1;
  fp12_mul_by_014(f, l[0], l[1], l[2]);
  st_f12(out576, f);
  return 0;
}

// miller_loop(P, Q), both affine: p96 = x, y; q192 = x.c0, x.c1, y.c0, y.c1
int hx_miller_loop(const uint8_t* p96, const uint8_t* q192, uint8_t* out576) {
  G1A p;
  G2A q;
  Fp12 f;
  if (!ld_fps(&p.x, p96, 1) || !ld_fps(&p.y, p96 + 48, 1) || !ld_fps(&q.x.c0, q192, 2) || !ld_fps(&q.y.c0, q192 + 96, 2))
    return -1;
  miller_loop(f, p, q);
  st_f12(out576, f);
  return 0;
}

// The VM's modular inverse (fpvm.hpp fp_inv) on a raw canonical value: r3 = raw R turns the
// closing Montgomery product into the identity, so out = a^-1 mod p (0 -> 0).
void hx_fp_inv_raw(const uint32_t* a, const uint32_t* r_raw, uint32_t* out) {
  Fp x, r, rr;
  for (int k = 0; k < 12; ++k) x.v[k] = a[k], rr.v[k] = r_raw[k];
  ovh::vm::fp_inv(r, x, rr);
  for (int k = 0; k < 12; ++k) out[k] = r.v[k];
}

// ---- the arithmetic primitives on arrays of cases (tests/fp_cases.py; the device counterparts
// are tests/device/fp_probe.hip dp_*): n cases, 12 words per value.
static inline Fp ld12(const uint32_t* p, uint32_t i) { return fp_const(p + (size_t)i * 12); }
static inline void st12(uint32_t* p, uint32_t i, const Fp& v) {
  for (int k = 0; k < 12; ++k) p[(size_t)i * 12 + k] = v.v[k];
}

// fp_mul as this build gets it: the 12 x 32 CIOS loop (a, b < 4p)
void hx_fp_mul(uint32_t n, const uint32_t* a, const uint32_t* b, uint32_t* r) {
  for (uint32_t i = 0; i < n; ++i) {
    Fp m;
    fp_mul(m, ld12(a, i), ld12(b, i));
    st12(r, i, m);
  }
}

// flags[i]: bit 0 ny, bit 1 any_neg
void hx_pre_add2(uint32_t n, const uint32_t* A, const uint32_t* B, const uint32_t* C, const uint32_t* D,
                 const uint8_t* flags, uint32_t* x, uint32_t* y) {
  for (uint32_t i = 0; i < n; ++i) {
    Fp X, Y;
    ovh::vm::pre_add2(X, ld12(A, i), ld12(B, i), Y, ld12(C, i), ld12(D, i), (flags[i] & 1) != 0, (flags[i] & 2) != 0);
    st12(x, i, X);
    st12(y, i, Y);
  }
}

// lin_sum + scale_reduce as exec runs them. ctl[i]: bits 0..2 the negation masks of B, C, D,
// bits 8..11 the scale k, and the header's H_LINNEG / H_LINNEG2 / H_LINNEG3 bits in place.
// cst: the constant table (entries KTAB + 0..4 are read).
void hx_lin_unit(uint32_t n, const uint32_t* A, const uint32_t* B, const uint32_t* C, const uint32_t* D,
                 const uint32_t* ctl, const uint32_t* cst, uint32_t* r) {
  using namespace ovh::vm;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t c = ctl[i], k = (c >> 8) & 15;
    uint32_t s[13];
    lin_sum(s, ld12(A, i), ld12(B, i), ld12(C, i), ld12(D, i), 0u - (c & 1), 0u - ((c >> 1) & 1), 0u - ((c >> 2) & 1),
            c & (H_LINNEG | H_LINNEG2 | H_LINNEG3), cst);
    Fp l;
    scale_reduce(l, s, k > 1 ? k : 1u);
    st12(r, i, l);
  }
}

// coefs: 4 signed bytes per case
void hx_lin_mad(uint32_t n, const uint32_t* A, const uint32_t* B, const uint32_t* C, const uint32_t* D,
                const int8_t* coefs, uint32_t* r) {
  for (uint32_t i = 0; i < n; ++i) {
    Fp l;
    ovh::vm::lin_mad(l, ld12(A, i), ld12(B, i), ld12(C, i), ld12(D, i), coefs[4 * i], coefs[4 * i + 1],
                     coefs[4 * i + 2], coefs[4 * i + 3]);
    st12(r, i, l);
  }
}

void hx_canon(uint32_t n, const uint32_t* a, uint32_t* r) {
  for (uint32_t i = 0; i < n; ++i) {
    Fp c;
    ovh::vm::canon(c, ld12(a, i));
    st12(r, i, c);
  }
}

// hx_fp_inv_raw on an array (r3: 12 words, the same for every case)
void hx_fp_inv(uint32_t n, const uint32_t* a, const uint32_t* r3, uint32_t* r) {
  for (uint32_t i = 0; i < n; ++i) {
    Fp z;
    ovh::vm::fp_inv(z, ld12(a, i), fp_const(r3));
    st12(r, i, z);
  }
}

// One slice of an Fp-VM program through the interpreter (fpvm.hpp exec), lane by lane in each
// phase (a phase's writes never target a slot that phase reads: tools/fpvm/sched.py).
// slots: nslots x 12 words (in/out); planes: `st` output planes, 12 words each.
// any_all = 1 runs every wave-uniform block for every lane (all phase-header bits set).
// side / scr (spilled programs, fpvm.hpp run<true>): per-lane side words and the unit's
// scratch; after a phase's ops, its spills store their slots, then the next phase's fills land.
int hx_vm_run(const uint32_t* code, uint32_t nphases, uint32_t W, uint32_t NW, const uint32_t* cst, uint32_t* slots,
              uint64_t scalar, uint32_t* planes, uint32_t nplanes, int any_all, const uint32_t* side, uint32_t* scr) {
  using namespace ovh::vm;
  const uint32_t all =
      any_all ? (H_MUL | H_MULNEG | H_FLAG | H_LIN | H_LINNEG | H_LINNEG2 | H_LINNEG3 | H_ACC | H_RARE | H_SELB) : 0u;
  const ovh::vm::Out out{planes, 1, 0};
  (void)nplanes;
  for (uint32_t ph = 0; ph < nphases; ++ph) {
    if (ph > 0 && side)
      for (uint32_t lane = 0; lane < W; ++lane) {
        const uint32_t sw = side[(size_t)(ph - 1) * W + lane];
        if ((sw >> 30) == 2)  // spill of phase ph - 1
          for (int k = 0; k < 12; ++k) scr[((sw >> 11) & 0xFFF) * 12 + k] = slots[(sw & 0x7FF) * 12 + k];
      }
    if (ph > 0 && side)
      for (uint32_t lane = 0; lane < W; ++lane) {
        const uint32_t sw = side[(size_t)ph * W + lane];
        if ((sw >> 30) == 3)  // fill of phase ph
          for (int k = 0; k < 12; ++k) slots[(sw & 0x7FF) * 12 + k] = scr[((sw >> 11) & 0xFFF) * 12 + k];
      }
    for (uint32_t lane = 0; lane < W; ++lane) {
      const uint32_t* w = code + ((size_t)ph * W + lane) * NW;
      ovh::vm::exec(uint4{w[0] | all, w[1], w[2], w[3]}, true, slots, cst, scalar, out);
      // the interpreter's lazy-reduction invariant: every slot result lies in [0, 2p)
      const uint32_t op = w[0] & 31, dst = (w[0] >> 5) & 0x7FF;
      if (op != ovh::vm::OP_NOP && op != ovh::vm::OP_ST) {
        uint32_t br = 0;
        for (int k = 0; k < 12; ++k) (void)subc32(slots[dst * 12 + k], ovh::vm::P2_LIMBS[k], br, &br);
        if (!br) return -1 - (int)ph;
      }
    }
  }
  return 0;
}

}
