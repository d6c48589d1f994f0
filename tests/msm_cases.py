"""Crafted buckets for the unit-level tests of the G2 Pippenger MSM (csrc/msm.hpp) and their exact
expected values: plain Python integers over oracle/py/bls12_381.py, no GPU, no ctypes.

A case is a set of n votes' points (sigma_i, tau_i: any points of the twist E'(Fp2), tau
unrelated to sigma so that a swapped half shows) and, per bucket b = 255 w + d - 1 (window w,
digit d), the list of point ids (2 i + h, h = 1: tau_i) sorted into it, in order. The reference
sums them straight from the definition:

    bucket sum  B_b = sum of the bucket's points
    bit plane   T_t = sum of B_b over the buckets of window t // 8 whose digit has bit t % 8 set
    result      S   = sum_t 2^t T_t

and, as a check of the reference itself (tests/test_msm_cases.py), S = sum over the entries of
d 256^w times the point. tests/test_gpu_msm_buckets.py runs the cases through the product's
kernels (tests/device/msm_probe.hip)."""
import functools
import random

import bls12_381 as bls

F = bls.Fp2Ops
P = bls.P
NBW, NB, NT = 255, 1020, 32
CH = 64                       # entries of a chunk (k_msm_chunk runs levels 0..5 inside one)
MONT = pow(2, 384, P)         # the device's Montgomery radix (12 x 32-bit limbs)
MONT_INV = pow(MONT, -1, P)
M64 = (1 << 64) - 1
UNIT_BASE = M64

_O = (F.one, F.one, F.zero)   # the oracle's Jacobian identity


# ------------------------------------------------------------------------------ points
def psum(points):
    """sum of affine points (None: the identity), accumulated in the oracle's Jacobian form"""
    acc = _O
    for pt in points:
        acc = bls._jac_add(F, acc, bls._jac_from_aff(F, pt))
    return bls._jac_to_aff(F, acc)


def neg(pt):
    return bls.pt_neg(F, pt)


def mul(pt, k):
    return bls.pt_mul(F, pt, k)


def _batch_affine(jacs):
    """Jacobian points (none the identity) -> affine, with one inversion (Montgomery's trick)"""
    pref, acc = [], F.one
    for J in jacs:
        pref.append(acc)
        acc = F.mul(acc, J[2])
    inv, out = F.inv(acc), [None] * len(jacs)
    for k in range(len(jacs) - 1, -1, -1):
        X, Y, Z = jacs[k]
        zi = F.mul(inv, pref[k])
        inv = F.mul(inv, Z)
        zi2 = F.sqr(zi)
        out[k] = (F.mul(X, zi2), F.mul(Y, F.mul(zi2, zi)))
    return out


@functools.lru_cache(maxsize=None)
def pool(count, tag):
    """`count` points P_k = 2 P_(k-1) + D of the r-torsion, P_0 and D random multiples of the
    generator drawn from `tag`: P_k = 2^k (P_0 + D) - D, so two different sets of the same size
    never have equal sums (their sums of 2^k differ), and no point is another's negative."""
    rng = random.Random("msm-cases-%s" % tag)
    cur = bls._jac_from_aff(F, mul(bls.G2_GEN, rng.randrange(1, bls.R)))
    D = bls._jac_from_aff(F, mul(bls.G2_GEN, rng.randrange(1, bls.R)))
    jacs = []
    for _ in range(count):
        jacs.append(cur)
        cur = bls._jac_add(F, bls._jac_dbl(F, cur), D)
    pts = _batch_affine(jacs)
    assert all(bls.on_curve(F, p) for p in pts[:4] + pts[-4:])
    return tuple(pts)


def bucket(w, d):
    assert 0 <= w < 4 and 1 <= d <= 255
    return w * NBW + d - 1


class Case:
    """sigma, tau: n affine points each; buckets: {bucket index: [point ids, in sorted order]};
    expect: what the case is built to reach, {name: value} (checked by check_expectations)"""

    def __init__(self, name, sigma, tau, buckets, expect=None):
        assert len(sigma) == len(tau) and sigma
        self.name, self.sigma, self.tau = name, list(sigma), list(tau)
        self.n = len(sigma)
        self.buckets = {b: list(ids) for b, ids in sorted(buckets.items()) if ids}
        self.expect = dict(expect or {})
        assert all(0 <= b < NB for b in self.buckets)
        assert all(0 <= i < 2 * self.n for ids in self.buckets.values() for i in ids)
        # the product's bounds (a point has one digit per window)
        assert all(len(ids) <= 2 * self.n for ids in self.buckets.values())
        assert sum(len(ids) for ids in self.buckets.values()) <= 8 * self.n

    def point(self, pid):
        return (self.tau if pid & 1 else self.sigma)[pid >> 1]

    def cnt(self):
        return [len(self.buckets.get(b, ())) for b in range(NB)]

    def ent(self):
        return [i for b in sorted(self.buckets) for i in self.buckets[b]]

    # -------- reference, straight from the definition
    def bucket_sums(self):
        if not hasattr(self, "_bs"):
            self._bs = {b: psum(self.point(i) for i in ids) for b, ids in self.buckets.items()}
        return self._bs

    def plane_sums(self):
        bs = self.bucket_sums()
        return [psum(bs[b] for b in sorted(bs) if b // NBW == t >> 3 and ((b % NBW + 1) >> (t & 7)) & 1)
                for t in range(NT)]

    def result(self):
        return psum(mul(T, 1 << t) for t, T in enumerate(self.plane_sums()) if T is not None)

    def direct(self):
        """sum over the entries of (d 256^w) point, one scalar multiplication per distinct point"""
        scal = {}
        for b, ids in self.buckets.items():
            for i in ids:
                scal[i] = scal.get(i, 0) + (b % NBW + 1) * 256 ** (b // NBW)
        return psum(mul(self.point(i), k) for i, k in sorted(scal.items()))


# ------------------------------------------------------------------------------ the cases
SIZE_COUNTS = (1, 2, 3, 63, 64, 65, 66, 127, 128, 129, 192, 193, 256, 257, 513)
# both ends of every window (so both ends of the prefix rows), and a few buckets in the middle:
# every other bucket is empty, so both prefix rows have long runs of equal values
SIZE_PLACES = {0: 65, 1: 1, 254: 513, 255: 2, 509: 128, 510: 129, 764: 3, 765: 257, 1018: 64, 1019: 193,
               100: 63, 383: 66, 600: 127, 601: 192, 900: 256}
SIZE_N = 258   # 2 n >= 513 entries in one bucket, 8 n >= 2,059 entries in all


@functools.lru_cache(maxsize=None)
def size_case(order):
    """every count of SIZE_COUNTS once, distinct points inside each bucket; order 1 has the same
    set in every bucket in another order (the scatter's order is arbitrary)"""
    assert sorted(SIZE_PLACES.values()) == sorted(SIZE_COUNTS)
    pts = pool(2 * SIZE_N, "size")
    rng = random.Random(0x73697A65)
    buckets = {b: rng.sample(range(2 * SIZE_N), c) for b, c in SIZE_PLACES.items()}
    if order:
        rng = random.Random(0x6F726472)
        first = size_case(0)
        buckets = {b: rng.sample(ids, len(ids)) for b, ids in first.buckets.items()}
        buckets = {b: ids[::-1] if ids == first.buckets[b] else ids for b, ids in buckets.items()}
        assert all(sorted(buckets[b]) == sorted(first.buckets[b]) for b in buckets)
        assert all(buckets[b] != first.buckets[b] for b in buckets if len(buckets[b]) > 1)
    c = Case("sizes-order%d" % order, pts[0::2], pts[1::2], buckets)
    if order:
        c._bs = first.bucket_sums()   # the same sets: the sums are the same by definition
    return c


FULL_N = 300


@functools.lru_cache(maxsize=None)
def full_case(b):
    """all 2 n = 600 points in bucket b alone"""
    pts = pool(2 * FULL_N, "full")
    ids = list(range(2 * FULL_N))
    random.Random(b).shuffle(ids)
    return Case("full-bucket%d" % b, pts[0::2], pts[1::2], {b: ids})


FULL_BUCKETS = (bucket(0, 5), NB - 1)


def _ex(name, pts, buckets, expect):
    """a small case over the points `pts` (ids 2 k for pts[k]); tau is a pool of its own"""
    tau = pool(len(pts), "ex-tau")
    return Case(name, pts, tau, buckets, expect)


@functools.lru_cache(maxsize=None)
def exceptional_cases():
    """name -> Case: one bucket each whose tree meets P + P, P + (-P), O + O, O + Q; bit-plane
    pairs and window-combination steps that double or cancel; S = O; the empty histogram"""
    Pt, Q = pool(2, "ex-PQ")
    R = pool(32, "ex-R")
    nP, nQ = neg(Pt), neg(Q)
    b0 = bucket(1, 77)
    cases = []

    def one(name, pts, ids, want):
        """one bucket: ids index pts; want: the bucket's sum"""
        cases.append(_ex(name, pts, {b0: [2 * k for k in ids]}, {"bucket": (b0, want)}))

    base = [Pt, nP, Q, nQ]
    one("P,P", base, [0, 0], mul(Pt, 2))
    one("P,-P", base, [0, 1], None)
    one("P,P,P,P", base, [0, 0, 0, 0], mul(Pt, 4))
    one("P,-P,Q", base, [0, 1, 2], Q)
    one("P,-P,Q,-Q", base, [0, 1, 2, 3], None)
    # 64 entries need n >= 32 votes: pad the point list
    wide = base + list(R)
    one("64xP", wide, [0] * 64, mul(Pt, 64))
    # R_k and -R_k side by side: level 0 is P + (-P) (madd) 32 times, levels 1-5 are O + O, and
    # level 6 (k_msm_upper) is O + Q
    pairs = list(R) + [neg(r) for r in R] + [Q]
    one("64-cancel,Q", pairs, [j for k in range(32) for j in (k, 32 + k)] + [64], Q)
    # chunk 0: R_0..R_31 then their negatives (the halves cancel at level 5); chunk 1: R_k, R_k+1,
    # -R_k, -R_k+1 (cancelling at level 1); level 6 is O + O
    ch0 = list(range(32)) + list(range(32, 64))
    ch1 = [j for k in range(0, 32, 2) for j in (k, k + 1, 32 + k, 33 + k)]
    one("128-two-chunks-O", pairs, ch0 + ch1, None)

    # digits 1 and 3 of a window are the first level-0 pair of its bit plane 0
    for w in (0, 3):
        cases.append(_ex("plane-pair-equal-w%d" % w, base, {bucket(w, 1): [0], bucket(w, 3): [0]},
                         {"plane": (8 * w, mul(Pt, 2))}))
        cases.append(_ex("plane-pair-opposite-w%d" % w, base, {bucket(w, 1): [0], bucket(w, 3): [2]},
                         {"plane": (8 * w, None)}))
    # window combination, level h: U[0] = A + [2^m] B with m = 2^(h-1), A = T_0 here and B = T_m
    for m in (1, 2, 4, 8, 16):
        big = mul(Pt, 1 << m)
        tb = bucket(m >> 3, 1 << (m & 7))   # the bucket that is all of T_m
        cases.append(_ex("hdbl%d-cancel" % m, [Pt, neg(big)], {bucket(0, 1): [2], tb: [0]},
                         {"planes": {0: neg(big), m: Pt}, "S": None}))
        cases.append(_ex("hdbl%d-double" % m, [Pt, big], {bucket(0, 1): [2], tb: [0]},
                         {"planes": {0: big, m: Pt}, "S": mul(Pt, 2 << m)}))
    # S = O only at the last step: 5 P in window 0, 2^31 Q in window 3 and their negative, divided
    # by 256, in window 1 (the points are multiples of the generator, so the division exists)
    a, bq = 0x1234567, 0x7654321
    Pa, Qb = mul(bls.G2_GEN, a), mul(bls.G2_GEN, bq)
    N = mul(bls.G2_GEN, -(5 * a + (bq << 31)) * pow(256, -1, bls.R) % bls.R)
    cases.append(_ex("S-identity", [Pa, Qb, N], {bucket(0, 5): [0], bucket(3, 128): [2], bucket(1, 1): [4]},
                     {"S": None, "planes": {0: Pa, 2: Pa, 31: Qb, 8: N}}))
    cases.append(_ex("empty", base, {}, {"S": None}))
    return {c.name: c for c in cases}


EXCEPTIONAL_NAMES = (
    "P,P", "P,-P", "P,P,P,P", "P,-P,Q", "P,-P,Q,-Q", "64xP", "64-cancel,Q", "128-two-chunks-O",
    "plane-pair-equal-w0", "plane-pair-opposite-w0", "plane-pair-equal-w3", "plane-pair-opposite-w3",
    "hdbl1-cancel", "hdbl1-double", "hdbl2-cancel", "hdbl2-double", "hdbl4-cancel", "hdbl4-double",
    "hdbl8-cancel", "hdbl8-double", "hdbl16-cancel", "hdbl16-double", "S-identity", "empty")


def check_expectations(case):
    """the reference sums of an exceptional case really are what the case is built to reach"""
    e = case.expect
    eq = lambda x, y: bls.pt_eq(F, x, y)  # noqa: E731
    if "bucket" in e:
        b, want = e["bucket"]
        assert list(case.buckets) == [b] and eq(case.bucket_sums()[b], want), case.name
    planes = dict(e.get("planes", {}))
    if "plane" in e:
        planes[e["plane"][0]] = e["plane"][1]
    T = case.plane_sums()
    for t, want in planes.items():
        assert eq(T[t], want), (case.name, t)
    if "planes" in e:   # and no other plane holds anything
        assert all(T[t] is None for t in range(NT) if t not in planes), case.name
    if "S" in e:
        assert eq(case.result(), e["S"]), case.name


def levels(c):
    """tree levels of a bucket of c entries (level l runs while 2^l < c; level 0 always)"""
    return max(1, (c - 1).bit_length())


def chunks(c):
    return (c + CH - 1) // CH


# ------------------------------------------------------------------------------ the sort half
def splitmix(seed, i):
    """rlc_scalar of csrc/ovhip.hip, restated: SplitMix64 on (seed, i), never 0"""
    z = (seed + 0x9E3779B97F4A7C15 * (i + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z or 1


def vote_scalar(seed, base, i):
    return 1 if base == UNIT_BASE else splitmix(seed, (base + i) & M64)


def halves(r):
    """(a, b): the scalar of sigma and the scalar of tau"""
    return r & 0xFFFFFFFF, r >> 32


def sort_reference(n, seed, base, codes):
    """-> (buckets {b: sorted point ids}, cnt, off, pf row 0, pf row 1) of the counting sort"""
    buckets = {}
    for i in range(n):
        if codes[i]:
            continue
        for h, s in enumerate(halves(vote_scalar(seed, base, i))):
            for w in range(4):
                d = (s >> (8 * w)) & 255
                if d:
                    buckets.setdefault(bucket(w, d), []).append(2 * i + h)
    cnt = [len(buckets.get(b, ())) for b in range(NB)]

    def prefix(vals):
        out, run = [], 0
        for v in vals:
            out.append(run)
            run += v
        return out + [run]

    return buckets, cnt, prefix(cnt), prefix([(c + 1) // 2 for c in cnt]), prefix([chunks(c) for c in cnt])


SORT_SIZES = (1, 63, 64, 65, 257, 1000)
SORT_SEED = 0x6D736D5F736F7274
SORT_BASES = (0x0123456789ABCDEF, M64 - 2)   # the second: base + i wraps 2^64 from i = 3 on


def sort_codes(n):
    """name -> codes: all valid, all failing, alternating, only the last vote valid"""
    return {"all-valid": [0] * n, "all-failing": [5] * n, "alternating": [(i & 1) * 3 for i in range(n)],
            "last-only": [102] * (n - 1) + [0]}


def digits(n, seed, base):
    return [(s >> (8 * w)) & 255 for i in range(n) for s in halves(vote_scalar(seed, base, i)) for w in range(4)]


# ------------------------------------------------------------------------------ the whole MSM
MSM_SIZES = (1, 2, 33, 65)
MSM_SEED = 0x6D736D5F66756C6C
MSM_BASE = 0x00C0FFEE12345678


def msm_codes(n):
    """some failing votes (none at n = 1; the second of two)"""
    return [3 if (n > 1 and i % 4 == 1) else 0 for i in range(n)]


@functools.lru_cache(maxsize=None)
def msm_points(n):
    pts = pool(2 * max(MSM_SIZES), "msm")
    return pts[0:2 * n:2], pts[1:2 * n:2]


def msm_reference(n, seed, base, codes):
    """S = sum over the votes with code 0 of [a_i] sigma_i + [b_i] tau_i"""
    sigma, tau = msm_points(n)
    terms = []
    for i in range(n):
        if codes[i] == 0:
            a, b = halves(vote_scalar(seed, base, i))
            terms += [mul(sigma[i], a), mul(tau[i], b)]
    return psum(terms)


# ------------------------------------------------------------------------------ limbs
def to_words(v):
    m = v * MONT % P
    return [(m >> (32 * k)) & 0xFFFFFFFF for k in range(12)]


def point_words(pts):
    """affine points -> flat list of 48 words each (x.c0, x.c1, y.c0, y.c1; Montgomery limbs)"""
    out = []
    for (x, y) in pts:
        for v in (x[0], x[1], y[0], y[1]):
            out += to_words(v)
    return out


def from_words(ws):
    """72 words of a projective device point -> affine point or None (Z = 0)"""
    v = [sum(int(w) << (32 * k) for k, w in enumerate(ws[12 * j:12 * j + 12])) * MONT_INV % P for j in range(6)]
    X, Y, Z = (v[0], v[1]), (v[2], v[3]), (v[4], v[5])
    if F.is_zero(Z):
        return None
    zi = F.inv(Z)
    return (F.mul(X, zi), F.mul(Y, zi))
