"""The kernels of the pairing tail and their launch code on crafted inputs against exact
expectations: k_vm_fold<1> / k_vm_fold<VM_FOLD_UNITS>, enqueue_final (k_vm_final), k_vm_fe,
k_vm_votefe, k_vm_final1, enqueue_bisect (k_vm_rs, the fold levels, k_vm_group, k_vm_votechk) and
k_pick_head / k_vm_gmil / k_vm_gfin (csrc/ovhip.hip).

Through the batch calls every f is the Miller value of a parsed vote, so a test cannot choose what
the gating and index logic of these kernels depends on. The test-only probe
(tests/device/pair_probe.hip, built by `make -C consensus_overlord_amd` as
tests/device/_build/libpairprobe.so with -DBISECT_DIRECT_MAX=32u) includes the product
translation unit whole and launches the product's kernels with the product's grid and LDS sizes, or
through the product's own enqueue_final / enqueue_bisect, on arrays the test supplies.

The reference is tests/pairing_ref.py and tests/pairing_cases.py (plain integers, the oracle's
point arithmetic). Every comparison is exact: Fp12 outputs limb for limb, points as points (a
device identity is Z = 0), codes word for word with their guard words, untouched outputs still
0xFF."""
import ctypes
import functools
import os
import random

import numpy as np
import pytest

import bls12_381 as bls
import msm_cases
import pairing_cases as pcs
import pairing_ref as ref
from pairing_ref import P, R
from vm_helpers import ROOT

import alg  # noqa: E402  (tools/fpvm: vm_helpers puts it on the path)

pytestmark = pytest.mark.gpu

PROBE = os.path.join(ROOT, "tests", "device", "_build", "libpairprobe.so")
u32p = ctypes.POINTER(ctypes.c_uint32)
i32p = ctypes.POINTER(ctypes.c_int32)
u32, u64, cint = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
MONT = pow(2, 384, P)
MONT_INV = pow(MONT, -1, P)
POISON = 0xFFFFFFFF
VERIFY_FAIL = bls.BLST_VERIFY_FAIL
HIP_INVALID_VALUE = 1
GUARD = 2
PART_W, F_W, G2_W = 216, 144, 72


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(PROBE):
        pytest.fail("%s is missing: run build() (make -C consensus_overlord_amd) first" % PROBE)
    lib = ctypes.CDLL(PROBE)
    lib.pp_fold.argtypes = [cint, u32, u32p, i32p, cint, cint, u32p]
    lib.pp_final.argtypes = [u32, u32p, u32p, i32p]
    lib.pp_fe.argtypes = [u32p, i32p]
    lib.pp_final1.argtypes = [u32p, i32p, i32p]
    lib.pp_votefe.argtypes = [u32, u32p, i32p, cint]
    lib.pp_bisect.argtypes = [u32, u64, u64, u32p, u32p, i32p, cint, i32p]
    lib.pp_group.argtypes = [u32, u32p, u32, u32p, u32p, u32p, u32p, u32p, u32p, u32p, i32p]
    for f in (lib.pp_fold, lib.pp_final, lib.pp_fe, lib.pp_final1, lib.pp_votefe, lib.pp_bisect, lib.pp_group):
        f.restype = cint
    for f in (lib.pp_guard, lib.pp_fold_units, lib.pp_direct_max):
        f.restype = u32
    lib.pp_close.restype = None
    assert lib.pp_guard() == GUARD and lib.pp_direct_max() == 32 and 64 % lib.pp_fold_units() == 0
    yield lib
    lib.pp_close()


# ------------------------------------------------------------------------------ limbs
def limbs(v):
    m = v % P * MONT % P
    return [(m >> (32 * k)) & 0xFFFFFFFF for k in range(12)]


def f12_words(t):
    return [w for c in ref.flat(t) for w in limbs(c)]


def g2_words(pt):
    return [w for c2 in pt for c in c2 for w in limbs(c)]


def part_words(f, s):
    return f12_words(f) + g2_words(s)


def value(words):
    """12 words -> the canonical value; asserts the limbs are a canonical Montgomery form"""
    m = sum(int(w) << (32 * k) for k, w in enumerate(words))
    assert m < P, "a device limb value is not below p"
    return m * MONT_INV % P


def f12_of(words):
    return ref.unflat([value(words[12 * k:12 * k + 12]) for k in range(12)])


def g2_of(words):
    v = [value(words[12 * k:12 * k + 12]) for k in range(6)]
    return ((v[0], v[1]), (v[2], v[3]), (v[4], v[5]))


def _u32(vals):
    return np.ascontiguousarray(np.array(vals, dtype=np.uint32).reshape(-1))


def _i32(vals):
    return np.ascontiguousarray(np.array(vals, dtype=np.int32).reshape(-1))


def _p(arr, t=u32p):
    return None if arr is None else arr.ctypes.data_as(t)


# ------------------------------------------------------------------------------ entry 1: the fold kernels
@functools.lru_cache(maxsize=None)
def fold_inputs():
    """17 partials: F random, S distinct points of the group (Z != 1)"""
    rng = random.Random(0xF01D)
    pts = msm_cases.pool(17, "pair-fold")
    return tuple((pcs._f12(rng), pcs.proj2(pt, pcs._f2(rng))) for pt in pts)


def fold_expected(parts, live, with_s):
    """-> [(F tower, S affine or None)] per output partial"""
    out = []
    for t in range((len(parts) + 3) // 4):
        F, S = ref.ONE, None
        for e in range(4 * t, min(4 * t + 4, len(parts))):
            if live[e]:
                F = ref.mul(F, ref.to_poly(parts[e][0]))
                if with_s:
                    S = pcs.g2_add(S, pcs.aff2(parts[e][1]))
        out.append((ref.from_poly(F), S))
    return out


def run_fold(probe, wide, parts, codes, with_s, gate):
    m = len(parts)
    live = [codes is None or codes[e] == 0 for e in range(m)]
    words = []
    for e, (f, s) in enumerate(parts):
        words += part_words(f, s) if live[e] else [POISON] * PART_W   # a vote with a code holds no planes
    mo = (m + 3) // 4
    out = np.zeros((mo + GUARD) * PART_W, dtype=np.uint32)
    ca = None if codes is None else _i32(codes)
    rc = probe.pp_fold(wide, m, _p(_u32(words)), _p(ca, i32p), int(with_s), gate, _p(out))
    assert rc == 0, "pp_fold returned %d" % rc
    out = out.tolist()
    what = "fold wide=%d m=%d codes=%s S=%s gate=%d" % (wide, m, codes is not None, with_s, gate)
    assert out[mo * PART_W:] == [POISON] * (GUARD * PART_W), what + ": words beyond ceil(m / 4) partials written"
    if gate == 1:
        assert out == [POISON] * len(out), what + ": written under gate = 1"
        return
    for t, (F, S) in enumerate(fold_expected(parts, live, with_s)):
        w = out[t * PART_W:(t + 1) * PART_W]
        assert f12_of(w[:F_W]) == F, "%s: F of partial %d" % (what, t)
        got = g2_of(w[F_W:])
        assert pcs.aff2(got) == S and (S is not None or got[1] != pcs.Z2), "%s: S of partial %d" % (what, t)


@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("m", [1, 3, 4, 5, 17])
def test_fold_kernels(probe, m, wide):
    parts = fold_inputs()[:m]
    rng = random.Random(m)
    run_fold(probe, wide, parts, None, True, -1)
    # every second entry coded, and one whole output partial (the last) without a live entry
    codes = [(2 if e % 2 else 0) for e in range(m)]
    for e in range(4 * ((m - 1) // 4), m):
        codes[e] = 5
    if m == 1:
        codes = [3]
    run_fold(probe, wide, parts, codes, True, 0)
    run_fold(probe, wide, parts, [0] * m, True, -1)
    run_fold(probe, wide, parts, [rng.choice((0, 0, 102)) for _ in range(m)], False, 0)
    run_fold(probe, wide, parts, None, False, -1)
    run_fold(probe, wide, parts, None, True, 1)


def test_fold_refuses_bad_arguments(probe):
    out = np.zeros(PART_W * 20, dtype=np.uint32)
    w = _u32(part_words(*fold_inputs()[0]))
    assert probe.pp_fold(0, 0, _p(w), None, 1, -1, _p(out)) == HIP_INVALID_VALUE
    assert probe.pp_fold(0, 65, _p(w), None, 1, -1, _p(out)) == HIP_INVALID_VALUE
    assert probe.pp_fold(0, 1, None, None, 1, -1, _p(out)) == HIP_INVALID_VALUE
    assert probe.pp_fold(0, 1, _p(w), None, 1, 2, _p(out)) == HIP_INVALID_VALUE
    assert probe.pp_final(5, _p(w), None, _p(_i32([0]), i32p)) == HIP_INVALID_VALUE
    assert probe.pp_votefe(1, _p(w), _p(_i32([0] * 5), i32p), -1) == HIP_INVALID_VALUE
    assert probe.pp_bisect(0, 1, 2, _p(w), _p(w), _p(_i32([0] * 5), i32p), 0, _p(_i32([0]), i32p)) == HIP_INVALID_VALUE
    assert probe.pp_group(0, _p(w), 1, _p(w), _p(w), _p(w), None, _p(w), _p(w), _p(w), _p(_i32([0]), i32p)) == HIP_INVALID_VALUE
    assert probe.pp_group(1, _p(_u32([1])), 1, _p(w), _p(w), _p(w), None, _p(w), _p(w), _p(w),
                          _p(_i32([0]), i32p)) == HIP_INVALID_VALUE


# ------------------------------------------------------------------------------ entry 2: enqueue_final
def run_final(probe, parts, m, xs):
    words = [w for f, s in parts[:m] for w in part_words(f, s)]
    if xs:   # partial 0's S apart, its own S planes poisoned
        words[F_W:PART_W] = [POISON] * G2_W
    v = _i32([7])
    rc = probe.pp_final(m, _p(_u32(words)), _p(_u32(g2_words(parts[0][1]))) if xs else None, _p(v, i32p))
    assert rc == 0, "pp_final returned %d" % rc
    return int(v[0])


@pytest.mark.parametrize("xs", [False, True])
def test_enqueue_final(probe, xs):
    seen = set()
    for c in pcs.final_cases():
        live = max(k + 1 for k, (f, s) in enumerate(c.parts) if (f, s) != pcs.ID_PART)
        for m in sorted({live, 4}):
            assert run_final(probe, c.parts, m, xs) == c.ok, "final on %s, m = %d, xS = %s" % (c.name, m, xs)
            seen.add(m)
    assert seen == {1, 2, 3, 4}


# ------------------------------------------------------------------------------ entry 3: the FE kernels
def test_fe_and_final1_on_every_fp12_case(probe):
    for c in pcs.fe_cases():
        f = _u32(f12_words(c.f))
        v = _i32([7])
        assert probe.pp_fe(_p(f), _p(v, i32p)) == 0
        assert int(v[0]) == c.ok, "k_vm_fe on %s" % c.name
        code, v = _i32([0]), _i32([7])
        assert probe.pp_final1(_p(f), _p(code, i32p), _p(v, i32p)) == 0
        assert (int(code[0]), int(v[0])) == ((0, 1) if c.ok else (VERIFY_FAIL, 0)), "k_vm_final1 on %s" % c.name
    # a code already set is kept and the verdict is 0, whether F would pass (1, an r-th power) or not
    for cls in ("one", "rth_power", "random"):
        c = next(c for c in pcs.fe_cases() if c.cls == cls)
        for prior in (2, 102, -1):
            code, v = _i32([prior]), _i32([7])
            assert probe.pp_final1(_p(_u32(f12_words(c.f))), _p(code, i32p), _p(v, i32p)) == 0
            assert (int(code[0]), int(v[0])) == (prior, 0), (cls, prior)
    # ... and with poisoned planes
    code, v = _i32([3]), _i32([7])
    assert probe.pp_final1(_p(_u32([POISON] * F_W)), _p(code, i32p), _p(v, i32p)) == 0
    assert (int(code[0]), int(v[0])) == (3, 0)


def test_votefe_gating(probe):
    cases = pcs.fe_cases()
    n = len(cases)
    prior = {1: 2, 8: 102, 10: 6, 13: 1}          # index -> code; 8: an r-th power that would pass, 10: random
    assert cases[8].cls == "rth_power" and cases[8].ok == 1 and cases[10].ok == 0
    poisoned = {1, 13}
    words = []
    for k, c in enumerate(cases):
        words += [POISON] * F_W if k in poisoned else f12_words(c.f)
    codes_in = [0x5A5A5A5A] * GUARD + [prior.get(k, 0) for k in range(n)] + [0x5A5A5A5A] * GUARD
    want = list(codes_in)
    for k, c in enumerate(cases):
        if k not in prior:
            want[GUARD + k] = 0 if c.ok else VERIFY_FAIL
    for verdict, exp in ((0, want), (1, codes_in)):
        codes = np.array(codes_in, dtype=np.uint32).astype(np.int32)
        assert probe.pp_votefe(n, _p(_u32(words)), _p(codes, i32p), verdict) == 0
        assert codes.astype(np.uint32).tolist() == [x & 0xFFFFFFFF for x in exp], "k_vm_votefe under verdict = %d" % verdict


# ------------------------------------------------------------------------------ entry 4: enqueue_bisect
SEED, BASE = 0x0123456789ABCDEF, 0x1000
NMAX = 80


@functools.lru_cache(maxsize=None)
def vote_pool():
    """80 crafted votes over H = [h] G2: sigma_i = [a_i h] G2, tau_i = [LAMBDA] sigma_i, and the
    Miller value the vote program would have stored, f_i with FE(f_i) = e(G1, G2)^(3 r_i a_i h):
    M^(r_i a_i h) for M a Miller value of (G1, G2), by the reference's power. bad_i uses a_i + 1."""
    rng = random.Random(0xB15EC7)
    h = rng.randrange(1, R)
    M = pcs.miller_ref(bls.G1_GEN, bls.G2_GEN)
    votes = []
    for i in range(NMAX):
        a = rng.randrange(1, R)
        r = alg.rlc_scalar(msm_cases.vote_scalar(SEED, BASE, i))
        sigma = pcs.g2_mul(a * h)
        tau = pcs.g2_mul(alg.LAMBDA, sigma)
        st8 = [w for c2 in sigma + tau for c in c2 for w in limbs(c)]
        good = f12_words(ref.from_poly(ref.pow(M, r * a * h % R)))
        bad = f12_words(ref.from_poly(ref.pow(M, r * (a + 1) * h % R)))
        votes.append((st8, good, bad, r * a * h % R))
    return tuple(votes)


def run_bisect(probe, n, invalid, prior, verdict, twist=None):
    """twist {i: d}: f_i is off by the factor M^d, so vote i fails on its own, and a group whose
    d sum to 0 mod r still passes its combined check"""
    votes = vote_pool()
    twist = twist or {}
    assert not set(twist) & (set(invalid) | set(prior))
    M = pcs.miller_ref(bls.G1_GEN, bls.G2_GEN)
    st8, f = [], []
    for i in range(n):
        if i in prior:       # a vote with a code: its planes were never written
            st8 += [POISON] * 96
            f += [POISON] * F_W
        elif i in twist:
            st8 += votes[i][0]
            f += f12_words(ref.from_poly(ref.pow(M, (votes[i][3] + twist[i]) % R)))
        else:
            st8 += votes[i][0]
            f += votes[i][2 if i in invalid else 1]
    g = 0x3C3C3C3C
    codes_in = [g] * GUARD + [prior.get(i, 0) for i in range(n)] + [g] * GUARD
    codes = np.array(codes_in, dtype=np.uint32).astype(np.int32)
    ng = (n + 15) // 16
    grp = _i32([9] * ng)
    rc = probe.pp_bisect(n, SEED, BASE, _p(_u32(st8)), _p(_u32(f)), _p(codes, i32p), verdict, _p(grp, i32p))
    assert rc == 0, "pp_bisect returned %d" % rc
    what = "bisect n=%d invalid=%s prior=%s verdict=%d" % (n, sorted(invalid), prior, verdict)
    got = codes.astype(np.uint32).tolist()
    if verdict == 1:
        assert got == codes_in, what + ": codes changed under verdict = 1"
        if n > 32:
            assert grp.tolist() == [-1] * ng, what + ": grp_ok written under verdict = 1"
        return
    # a group passes when every vote of it without a code verifies, or when its errors cancel
    exp = []
    for k in range(ng):
        ids = range(16 * k, min(16 * k + 16, n))
        exp.append(int(not any(i in invalid and i not in prior for i in ids) and sum(twist.get(i, 0) for i in ids) % R == 0))
    want = list(codes_in)
    for i in range(n):
        bad = (i in invalid and i not in prior) or twist.get(i, 0) % R != 0
        # the direct route checks every vote; the group route only the votes of failing groups
        if bad and (n <= 32 or not exp[i // 16]):
            want[GUARD + i] = VERIFY_FAIL
    assert got == want, what
    if n > 32:
        assert grp.tolist() == exp, what + ": grp_ok"


@pytest.mark.parametrize("n", [1, 16, 17, 32, 33, 48, 80])
def test_bisect_invalid_votes_at_the_edges(probe, n):
    invalid = {i for i in (0, 15, 16, n - 1) if i < n}
    prior = {i: code for i, code in ((3, 2), (20, 102), (40, 1)) if i < n - 1}
    run_bisect(probe, n, invalid, prior, -1)
    if n in (17, 80):
        run_bisect(probe, n, invalid, prior, 0)
        run_bisect(probe, n, invalid, prior, 1)
    # all valid, and every vote invalid
    run_bisect(probe, n, set(), {}, 0)
    if n in (1, 33):
        run_bisect(probe, n, set(range(n)), {}, -1)


@pytest.mark.parametrize("n", [48, 80])
def test_bisect_a_whole_invalid_group_beside_a_valid_one(probe, n):
    """group 1 wholly invalid, the others valid; votes with a code and poisoned planes inside the
    failing group (20, and an invalid one at 31 that keeps its code) and inside valid ones (3, 40)"""
    invalid = set(range(16, 32))
    prior = {3: 2, 20: 102, 31: 6, 40: 1}
    for verdict in (-1, 0, 1):
        run_bisect(probe, n, invalid, prior, verdict)


@pytest.mark.parametrize("n", [32, 48])
def test_bisect_trusts_a_group_that_passes(probe, n):
    """Votes 17 and 18 carry errors that cancel in the product (M^d and M^-d), vote 40 an error of
    its own. On the group route (48) group 1 passes its combined check, grp_ok[1] = 1, and
    k_vm_votechk leaves its votes alone; group 2 fails and only its votes are checked. On the
    direct route (32) every vote is checked on its own and 17 and 18 fail."""
    twist = {i: d for i, d in ((17, 0xD15EA5E), (18, R - 0xD15EA5E), (40, 5)) if i < n}
    run_bisect(probe, n, set(), {19: 2}, 0, twist)
    run_bisect(probe, n, set(), {19: 2}, -1, twist)


# ------------------------------------------------------------------------------ entry 5: the group kernels
def g1_words(pt):
    return [w for c in pt for w in limbs(c)]


def run_group(probe, G, keys, hs, ghinf, sel_want, F, S_scalar, key_override=None):
    """keys[q]: scalar of hash q's key sum (None: Z = 0); hs[q]: scalar of H_q; F: gfin's F, a tower or
    None (F.p null); S = [S_scalar] G2 (0: S = O). -> the verdict"""
    rng = random.Random(G * 1000 + len([k for k in keys if k]))
    np_ = G + 1
    head = [np_ - 1 - q for q in range(G)]          # entry 0 is no hash's: poisoned
    Pw = [[POISON] * 36 for _ in range(np_)]
    for q in range(G):
        if keys[q] is None:
            Pw[head[q]] = g1_words((rng.randrange(1, P), rng.randrange(1, P), 0))
        else:
            A = pcs.g1_mul(keys[q])
            lam = rng.randrange(1, P)
            Pw[head[q]] = g1_words((A[0] * lam % P, A[1] * lam % P, lam))
    if key_override is not None:
        q, pt = key_override
        Pw[head[q]] = g1_words(pt)
    gh = [w for q in range(G) for w in g2_words(pcs.proj2(pcs.g2_mul(hs[q]), pcs._f2(rng)))]
    Sp = pcs.proj2(pcs.g2_mul(S_scalar) if S_scalar else None, pcs._f2(rng))
    if not S_scalar:
        Sp = (pcs._f2(rng), pcs._f2(rng), pcs.Z2)
    sel, verdict = _u32([99]), _i32([7])
    fout = np.zeros((G + GUARD) * F_W, dtype=np.uint32)
    Fw = None if F is None else _u32(f12_words(F))
    rc = probe.pp_group(G, _p(_u32(head)), np_, _p(_u32([w for e in Pw for w in e])), _p(_u32(gh)), _p(_u32(ghinf)), _p(Fw),
                        _p(_u32(g2_words(Sp))), _p(sel), _p(fout), _p(verdict, i32p))
    assert rc == 0, "pp_group returned %d" % rc
    what = "group G=%d sel=%d" % (G, sel_want)
    assert int(sel[0]) == sel_want, what + ": k_pick_head"
    fout = fout.tolist()
    E = pcs.pairing3([(bls.G1_GEN, bls.G2_GEN)])
    written = {}
    if G > 1:
        for q in range(G):
            if q != sel_want:
                written[sel_want if q == 0 else q] = q
    for idx in range(G + GUARD):
        w = fout[idx * F_W:(idx + 1) * F_W]
        if idx not in written:
            assert w == [POISON] * F_W, "%s: f planes of index %d written" % (what, idx)
            continue
        q = written[idx]
        f = f12_of(w)
        if keys[q] is None:
            assert f == pcs.ONE_T, "%s: f of hash %d (key sum O) is not 1" % (what, q)
        else:
            assert f != pcs.ONE_T and pcs.fe_of(f) == ref.from_poly(ref.pow(E, keys[q] * hs[q] % R)), \
                "%s: f of hash %d at index %d" % (what, q, idx)
    return int(verdict[0])


def _group_setup(G, live, seed):
    rng = random.Random(seed)
    draws = [(rng.randrange(1, R), rng.randrange(1, R)) for _ in range(G)]
    keys = [k if q in live else None for q, (k, _) in enumerate(draws)]
    hs = [h for _, h in draws]
    return keys, hs


@pytest.mark.parametrize("G", [1, 2, 5, 70])
def test_group_kernels_head_at_hash_0(probe, G):
    live = {0} | {q for q in (1, 3, 64, 69) if q < G}
    keys, hs = _group_setup(G, live, G)
    ghinf = [0] * G
    S = keys[0] * hs[0] % R
    assert run_group(probe, G, keys, hs, ghinf, 0, None, S) == 1                        # F.p null
    assert run_group(probe, G, keys, hs, ghinf, 0, pcs.ONE_T, S) == 1                   # an explicit identity F
    x = 0xC0FFEE
    M = ref.from_poly(ref.pow(pcs.miller_ref(bls.G1_GEN, bls.G2_GEN), x))
    assert run_group(probe, G, keys, hs, ghinf, 0, M, (S + x) % R) == 1
    assert run_group(probe, G, keys, hs, ghinf, 0, M, S) == 0                           # F not matched by S
    A = pcs.g1_mul(keys[0] + 1)
    assert run_group(probe, G, keys, hs, ghinf, 0, None, S, key_override=(0, (A[0], A[1], 1))) == 0   # key sum replaced
    assert run_group(probe, G, keys, hs, ghinf, 0, None, 0) == 0                        # degenerate: S = O


@pytest.mark.parametrize("G", [2, 5, 70])
def test_group_kernels_head_at_a_later_hash(probe, G):
    """hash 0's key sum is O, or its H is (ghinf): the head is the first later hash with neither,
    and hash 0's f lands at the head's index"""
    head = {2: 1, 5: 3, 70: 65}[G]
    live = {head} | {q for q in (4, 66, 69) if head < q < G}
    keys, hs = _group_setup(G, live, 100 + G)
    S = keys[head] * hs[head] % R
    assert run_group(probe, G, keys, hs, [0] * G, head, None, S) == 1
    # hash 0 and another early hash carry a key sum but H = O flags: still not the head
    live2 = live | {0} | ({2} if head > 2 else set())
    keys2, hs2 = _group_setup(G, live2, 100 + G)
    assert keys2[head] == keys[head]
    ghinf = [int(q in (0, 2) and q < head) for q in range(G)]
    assert run_group(probe, G, keys2, hs2, ghinf, head, None, S) == 1
    assert run_group(probe, G, keys2, hs2, ghinf, head, None, (S + 1) % R) == 0


@pytest.mark.parametrize("G", [1, 5])
def test_group_kernels_without_any_head(probe, G):
    """every key sum O (or every H = O): k_pick_head answers 0 and gfin takes its degenerate
    branch through apk Z = 0"""
    keys, hs = _group_setup(G, set(), 7)
    assert run_group(probe, G, keys, hs, [0] * G, 0, None, 12345) == 0
    if G > 1:
        keys, hs = _group_setup(G, {0, 1}, 7)
        # flagged everywhere: no head, hash 0 still stands in; its pair is then checked as it is
        S = keys[0] * hs[0] % R
        assert run_group(probe, G, keys, hs, [1] * G, 0, None, S) == 1
