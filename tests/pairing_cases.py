"""Crafted inputs for the pairing tail -- the Fp12 tower, the Miller loop, the final
exponentiation and the fold / final / gfin / rs programs -- each with its exact expectation from
tests/pairing_ref.py (plain integers; the Miller value from the oracle's affine loop, compared
only after the reference's plain-exponent final exponentiation). Deterministic (a seeded
random.Random); built once per process. tests/test_pairing_cases.py checks the reference's own
consistency and the oracle's tower on every case; tests/pairing_vm.py runs them through the
Fp-VM; tests/test_host_pairing.py through the one-lane tower."""
import collections
import functools
import random

import bls12_381 as bls
import pairing_ref as ref
from pairing_ref import P, R

SEED = 0x9A171E
ONE_T = ref.from_poly(ref.ONE)
ZERO_T = ref.from_poly(ref.ZERO)
PM1_T = ref.unflat([P - 1] * 12)

FeCase = collections.namedtuple("FeCase", "name cls f fe ok")            # towers; fe = f^(3(p^12-1)/r)
CycCase = collections.namedtuple("CycCase", "name cls a sqr expx")       # a cyclotomic; a^2, a^x
OpCase = collections.namedtuple("OpCase", "name cls a b mul sqr inv frob")
LineCase = collections.namedtuple("LineCase", "name cls f l0 l1 l4 out")
# pairs: [(P, Q)], P = (x, y) or (X, Y, Z) in Fp, Q = (X, Y, Z) in Fp2; fe: the tower value of
# prod e(P_j, Q_j)^3
MillerCase = collections.namedtuple("MillerCase", "name cls pairs fe")
# parts: four (F tower, S projective); F, S: their exact product and sum (S affine, None = O)
FinalCase = collections.namedtuple("FinalCase", "name cls parts F S ok")
GfinCase = collections.namedtuple("GfinCase", "name cls F pk h S ok")
RsCase = collections.namedtuple("RsCase", "name z sigma tau want")

FE_CLASSES = {"one": 1, "zero": 1, "fp": 2, "fp2": 1, "fp6": 1, "pure_w": 2, "rth_power": 1, "rth_times_fp6": 1,
              "random": 2, "all_pm1": 1, "one_hot": 12, "near_rth": 1}
CYC_CLASSES = {"easy_part": 2, "one": 1, "order_r": 1}
OP_CLASSES = {"random": 2, "zero_parts": 3, "all_pm1": 1, "zero": 1}
LINE_CLASSES = {"random": 1, "l0_zero": 1, "l1_zero": 1, "l4_zero": 1, "all_pm1": 1}
MILLER_CLASSES = {"affine": 1, "scaled": 3, "signs": 3, "golden": 2, "bilinear": 1, "cancel": 1, "two_pairs": 1}
FINAL_CLASSES = {"cancels": 1, "doubles": 1, "all_inf": 2, "live": 4, "swapped": 1, "replaced": 1}
GFIN_CLASSES = {"valid": 2, "replaced": 1}
RS_Z = (0, 1, 1 << 32, (1 << 64) - 1)


def _fp(rng):
    return rng.randrange(1, P)


def _f2(rng):
    return (_fp(rng), _fp(rng))


def _f6(rng):
    return (_f2(rng), _f2(rng), _f2(rng))


def _f12(rng):
    return (_f6(rng), _f6(rng))


Z2, Z6 = (0, 0), ((0, 0), (0, 0), (0, 0))


def fe_of(t):
    return ref.from_poly(ref.final_exp(ref.to_poly(t)))


def _fe_case(name, cls, f):
    fe = fe_of(f)
    return FeCase(name, cls, f, fe, int(fe == ONE_T))


@functools.lru_cache(maxsize=None)
def fe_cases():
    rng = random.Random(SEED)
    out = [_fe_case("1", "one", ONE_T), _fe_case("0", "zero", ZERO_T)]
    for n, v in (("2", 2), ("p - 1", P - 1)):
        out.append(_fe_case(n, "fp", ref.unflat([v] + [0] * 11)))
    out.append(_fe_case("Fp2", "fp2", ((_f2(rng), Z2, Z2), Z6)))
    out.append(_fe_case("Fp6", "fp6", (_f6(rng), Z6)))
    out.append(_fe_case("w", "pure_w", (Z6, ((1, 0), Z2, Z2))))
    out.append(_fe_case("c w, c in Fp6", "pure_w", (Z6, _f6(rng))))
    g = ref.to_poly(_f12(rng))
    # g lies in no proper subfield: the maximal ones are Fp6 and Fp4
    assert ref.pow(g, P ** 6) != g and ref.pow(g, P ** 4) != g
    gr = ref.pow(g, R)
    assert gr != ref.ONE
    out.append(_fe_case("g^r", "rth_power", ref.from_poly(gr)))
    out.append(_fe_case("g^r c, c in Fp6", "rth_times_fp6", ref.from_poly(ref.mul(gr, ref.to_poly((_f6(rng), Z6))))))
    for k in range(2):
        out.append(_fe_case("random %d" % k, "random", _f12(rng)))
    out.append(_fe_case("all p - 1", "all_pm1", PM1_T))
    for j in range(12):
        v = [0] * 12
        v[j] = _fp(rng)
        out.append(_fe_case("only coefficient %d" % j, "one_hot", ref.unflat(v)))
    v = ref.flat(ref.from_poly(gr))
    j = rng.randrange(12)
    v[j] = (v[j] + 1) % P
    out.append(_fe_case("g^r with coefficient %d + 1" % j, "near_rth", ref.unflat(v)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cyc_cases():
    out = []

    def case(name, cls, a):
        out.append(CycCase(name, cls, ref.from_poly(a), ref.from_poly(ref.mul(a, a)), ref.from_poly(ref.exp_x(a))))
    rnd = [c for c in fe_cases() if c.cls == "random"]
    for c in rnd:
        case("easy part of %s" % c.name, "easy_part", ref.easy_part(ref.to_poly(c.f)))
    case("1", "one", ref.ONE)
    a = ref.to_poly(rnd[0].fe)
    assert a != ref.ONE and ref.pow(a, R) == ref.ONE
    case("order r", "order_r", a)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def op_cases():
    rng = random.Random(SEED + 1)
    pairs = [("random %d" % k, "random", _f12(rng), _f12(rng)) for k in range(2)]
    x, y = _f6(rng), _f6(rng)
    # c1 = 0 against c0 = 0; equal halves with a negated partner (a0 + a1 = 0: the Karatsuba sum
    # vanishes); Fp2 coefficients with c0 = c1 and single components
    pairs.append(("c1 = 0 by c0 = 0", "zero_parts", (x, Z6), (Z6, y)))
    pairs.append(("a0 + a1 = 0", "zero_parts", (x, tuple(((P - c[0]) % P, (P - c[1]) % P) for c in x)), (y, y)))
    k = _fp(rng)
    pairs.append(("c0 = c1, sparse", "zero_parts", (((k, k), Z2, (k, k)), (Z2, (0, k), Z2)), ((Z2, (k, 0), Z2), ((k, k), Z2, Z2))))
    pairs.append(("all p - 1", "all_pm1", PM1_T, PM1_T))
    pairs.append(("0 by random", "zero", ZERO_T, _f12(rng)))
    out = []
    for name, cls, a, b in pairs:
        pa, pb = ref.to_poly(a), ref.to_poly(b)
        out.append(OpCase(name, cls, a, b, ref.from_poly(ref.mul(pa, pb)), ref.from_poly(ref.mul(pa, pa)),
                          ref.from_poly(ref.inv(pa)), ref.from_poly(ref.frob(pa))))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def line_cases():
    rng = random.Random(SEED + 2)
    f = _f12(rng)
    rows = [("random", "random", f, _f2(rng), _f2(rng), _f2(rng)), ("l0 = 0", "l0_zero", f, Z2, _f2(rng), _f2(rng)),
            ("l1 = 0", "l1_zero", f, _f2(rng), Z2, _f2(rng)), ("l4 = 0", "l4_zero", f, _f2(rng), _f2(rng), Z2),
            ("all p - 1", "all_pm1", PM1_T, (P - 1, P - 1), (P - 1, P - 1), (P - 1, P - 1))]
    return tuple(LineCase(n, c, f_, l0, l1, l4, ref.mul_t(f_, ref.line_t(l0, l1, l4))) for n, c, f_, l0, l1, l4 in rows)


# ------------------------------------------------------------------------------ points and pairings
def g1_mul(k, pt=None):
    return bls.pt_mul(bls.FpOps, pt or bls.G1_GEN, k % R)


def g2_mul(k, pt=None):
    return bls.pt_mul(bls.Fp2Ops, pt or bls.G2_GEN, k % R)


def g2_add(a, b):
    return bls.pt_add(bls.Fp2Ops, a, b)


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def proj2(pt, z=(1, 0)):
    """affine G2 point -> (X, Y, Z) in Fp2 scaled by z; None -> (0 : 1 : 0)"""
    if pt is None:
        return (Z2, (1, 0), Z2)
    return (f2_mul(pt[0], z), f2_mul(pt[1], z), z)


def aff2(pt):
    """(X, Y, Z) in Fp2 -> affine, None for Z = 0"""
    if pt[2] == Z2:
        return None
    n = pow(pt[2][0] * pt[2][0] + pt[2][1] * pt[2][1], -1, P)
    zi = (pt[2][0] * n % P, -pt[2][1] * n % P)
    return (f2_mul(pt[0], zi), f2_mul(pt[1], zi))


def aff1(pt):
    if len(pt) == 2:
        return pt
    if pt[2] == 0:
        return None
    zi = pow(pt[2], -1, P)
    return (pt[0] * zi % P, pt[1] * zi % P)


@functools.lru_cache(maxsize=None)
def miller_ref(Pa, Qa):
    """the oracle's affine Miller value as a polynomial (1 where a side is O)"""
    return ref.to_poly(bls.miller_loop(Pa, Qa))


def pairing3(pairs):
    """prod e(P_j, Q_j)^3 as a polynomial, points affine"""
    m = ref.ONE
    for Pa, Qa in pairs:
        m = ref.mul(m, miller_ref(Pa, Qa))
    return ref.final_exp(m)


@functools.lru_cache(maxsize=None)
def golden_points():
    """(a golden key, its signature, H of its message with Z != 1), affine / affine / projective"""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_v1.json")) as fh:
        g = json.load(fh)
    pk = bls.g1_from_bytes(bytes.fromhex(g["keys"][0]["pk"]))
    sig = bls.g2_from_bytes(bytes.fromhex(g["votes"][0]["sig"]))
    H = bls.hash_to_g2(bytes.fromhex(g["votes"][0]["digest"]))
    return pk, sig, H


@functools.lru_cache(maxsize=None)
def miller_cases():
    rng = random.Random(SEED + 3)
    G1, G2 = bls.G1_GEN, bls.G2_GEN
    nG1, nG2 = bls.pt_neg(bls.FpOps, G1), bls.pt_neg(bls.Fp2Ops, G2)
    pk, sig, H = golden_points()
    out = []

    def case(name, cls, pairs, fe=None):
        want = pairing3([(aff1(p_), aff2(q_)) for p_, q_ in pairs])
        assert fe is None or fe == want, name
        out.append(MillerCase(name, cls, tuple(pairs), ref.from_poly(want)))
        return want
    e = case("(G1, G2) affine", "affine", [(G1, proj2(G2))])
    for n, lam in (("1", 1), ("p - 1", P - 1), ("random", _fp(rng))):
        case("(lambda G1, G2), lambda = %s" % n, "scaled", [((G1[0] * lam % P, G1[1] * lam % P, lam), proj2(G2))], e)
    case("(-G1, G2)", "signs", [(nG1, proj2(G2))])
    case("(G1, -G2), Z = p - 1", "signs", [(G1, proj2(nG2, (P - 1, 0)))])
    case("([r - 1] G1, -G2)", "signs", [(g1_mul(R - 1), proj2(nG2))], e)
    case("(golden key, golden signature)", "golden", [(pk, proj2(sig))])
    lam = _fp(rng)
    pkp = (pk[0] * lam % P, pk[1] * lam % P, lam)
    case("(golden key with Z != 1, golden H with Z != 1)", "golden", [(pkp, proj2(H, _f2(rng)))])
    a, b = rng.randrange(1, R), rng.randrange(1, R)
    A = g1_mul(a)
    case("([a] G1, [b] G2) against e^(ab)", "bilinear", [((A[0] * lam % P, A[1] * lam % P, lam), proj2(g2_mul(b), _f2(rng)))],
         ref.pow(e, a * b % R))
    case("(P, Q), (-P, Q)", "cancel", [(pkp, proj2(sig, _f2(rng))), (bls.pt_neg(bls.FpOps, pk), proj2(sig))], ref.ONE)
    case("(P, Q), (P', Q')", "two_pairs", [(pkp, proj2(H, _f2(rng))), (nG1, proj2(sig))])
    return tuple(out)


# ------------------------------------------------------------------------------ final / fold / gfin / rs
ID_PART = (ONE_T, (Z2, (1, 0), Z2))
NG1 = (bls.G1_GEN[0], (P - bls.G1_GEN[1]) % P)


def _final_case(name, cls, parts):
    parts = tuple(parts) + (ID_PART,) * (4 - len(parts))
    F, S = ref.ONE, None
    for f, s in parts:
        F = ref.mul(F, ref.to_poly(f))
        S = g2_add(S, aff2(s))
    fe = ref.final_exp(ref.mul(F, miller_ref(NG1, S)))     # Miller value 1 where S = O
    return FinalCase(name, cls, parts, ref.from_poly(F), S, int(fe == ref.ONE))


@functools.lru_cache(maxsize=None)
def final_cases():
    """Valid partials: F_i a Miller value of ([s_i] G1, G2) beside S_i = [s_i] G2, so that
    prod F_i * Miller(-G1, sum S_i) exponentiates to 1."""
    rng = random.Random(SEED + 4)
    G2 = bls.G2_GEN

    def part(s, z=None):
        return (ref.from_poly(miller_ref(g1_mul(s), G2)), proj2(g2_mul(s), z or _f2(rng)))
    gr = next(c.f for c in fe_cases() if c.cls == "rth_power")
    rnd = next(c.f for c in fe_cases() if c.cls == "random")
    s = [rng.randrange(1, R) for _ in range(4)]
    Q = g2_mul(s[0])
    nQ = bls.pt_neg(bls.Fp2Ops, Q)
    valid = [part(x) for x in s]
    out = [_final_case("S = Q, -Q", "cancels", [(gr, proj2(Q, _f2(rng))), (ONE_T, proj2(nQ, _f2(rng)))]),
           _final_case("S = Q, Q", "doubles", [part(s[0], (1, 0)), part(s[0], (1, 0))]),
           _final_case("S = O everywhere, F an r-th power", "all_inf", [(gr, ID_PART[1])]),
           _final_case("S = O everywhere, F random", "all_inf", [(ONE_T, ID_PART[1]), (rnd, (Z2, (7, 9), Z2))])]
    for n in range(1, 5):
        out.append(_final_case("%d live" % n, "live", valid[:n]))
    out.append(_final_case("F swapped between partials", "swapped",
                           [(valid[1][0], valid[0][1]), (valid[0][0], valid[1][1])] + valid[2:]))
    out.append(_final_case("one F replaced", "replaced", [valid[0], (valid[2][0], valid[1][1]), valid[2]]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def gfin_cases():
    """F * Miller(pk, h) * Miller(-G1, S): pk = [a] G1, h = [c] G2, F a Miller value of
    ([b] G1, [d] G2), S = [a c + b d] G2."""
    rng = random.Random(SEED + 5)
    a, b, c, d = (rng.randrange(1, R) for _ in range(4))
    lam = _fp(rng)
    A = g1_mul(a)
    pk = (A[0] * lam % P, A[1] * lam % P, lam)
    h = proj2(g2_mul(c), _f2(rng))
    Fm = ref.from_poly(miller_ref(g1_mul(b), g2_mul(d)))
    A2 = g1_mul(a + 1)
    rows = [("F = 1", "valid", ONE_T, pk, g2_mul(a * c)), ("F a Miller value", "valid", Fm, pk, g2_mul(a * c + b * d)),
            ("key sum replaced", "replaced", Fm, (A2[0], A2[1], 1), g2_mul(a * c + b * d))]
    out = []
    for name, cls, F, pk_, S in rows:
        fe = ref.final_exp(ref.mul(ref.mul(ref.to_poly(F), miller_ref(aff1(pk_), aff2(h))), miller_ref(NG1, S)))
        out.append(GfinCase(name, cls, F, pk_, h, proj2(S, _f2(rng)), int(fe == ref.ONE)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def rs_cases(rlc_scalar, lam):
    """[rlc_scalar(z)] sigma for z at the extremes and one random value; tau = [lam] sigma, the
    rs program's second input, is derived by the integers (lam: alg.LAMBDA)."""
    rng = random.Random(SEED + 6)
    sigma = golden_points()[1]
    tau = g2_mul(lam, sigma)
    return tuple(RsCase("z = %#x" % z, z, sigma, tau, g2_mul(rlc_scalar(z), sigma))
                 for z in RS_Z + (rng.getrandbits(64),))


def perturb(values):
    """`values` (a list of limb values or a dict of them) with one limb of one entry changed"""
    if isinstance(values, dict):
        k = sorted(values)[len(values) // 2]
        return dict(values, **{k: values[k] ^ (1 << 32 * 5)})
    out = list(values)
    out[len(out) // 2] ^= 1 << 32 * 5
    return out
