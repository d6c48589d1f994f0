"""Crafted inputs for the unit-level tests of the quorum-certificate kernels -- the selection
(k_qc_reset / k_qc_claim / k_qc_mark), the masked G2 sum (k_qc_chunk / k_qc_upper and the
compression; csrc/qc.hpp) and the aggregated-key sum (k_qc_apk, csrc/ovhip.hip) -- with their exact
expected values: plain Python integers over oracle/py/bls12_381.py, no GPU, no ctypes.

    selection   select_reference: a plain loop over the staged votes. It extends the rule of
                tests/qc_model.py and tests/qc_groups_model.py to the arrays the kernels see: the
                table index of a staged vote (tidx), the caller's index of a staged vote (orig),
                the bitmap position of a table entry (rank) and the vote's group (gid).
    masked sum  SumCase.group_sums: per group, the sum of the taken votes' points.
                SumCase.operands restates which partial sums meet at which tree level, so that a
                case can show that it doubles or cancels where it says.
    key sum     ApkCase.sums: per QC, the sum of the listed table entries.

tests/test_qc_cases.py checks this reference without a GPU; tests/test_gpu_qc_kernels.py runs the
cases through the product's kernels and launch code (tests/device/qc_probe.hip). The comparison
helpers (*_mismatches) are shared by both, so the CPU test can show that they notice a perturbed
result."""
import functools
import random

import bls12_381 as bls
import msm_cases as mc
from msm_cases import F, MONT_INV, P, from_words, mul, neg, point_words, pool, psum, to_words  # noqa: F401

F1 = bls.FpOps
CH, CH_LV = 64, 6             # votes of a chunk (k_qc_chunk runs levels 0..5 inside one)
WG = 64                       # lanes of a selection workgroup
QC_NONE = 0xFFFFFFFF
GROUPS_MAX = 64               # OVH_QC_GROUPS_MAX
MSM_NB = mc.NB
PKF_INF = 2
GUARD = 64                    # guard words on each side of a selection array (qp_guard())
GUARD_WORD = 0xFFFFFFFF


def chunks(m):
    return (m + CH - 1) // CH


# ------------------------------------------------------------------------------ G1 points
_O1 = (F1.one, F1.one, F1.zero)


def psum1(points):
    acc = _O1
    for pt in points:
        acc = bls._jac_add(F1, acc, bls._jac_from_aff(F1, pt))
    return bls._jac_to_aff(F1, acc)


def neg1(pt):
    return bls.pt_neg(F1, pt)


def mul1(pt, k):
    return bls.pt_mul(F1, pt, k)


@functools.lru_cache(maxsize=None)
def pool1(count, tag):
    """msm_cases.pool in G1: P_k = 2 P_(k-1) + D, so no two different sets have equal sums"""
    rng = random.Random("qc-cases-g1-%s" % tag)
    cur = bls._jac_from_aff(F1, mul1(bls.G1_GEN, rng.randrange(1, bls.R)))
    D = bls._jac_from_aff(F1, mul1(bls.G1_GEN, rng.randrange(1, bls.R)))
    pts = []
    for _ in range(count):
        pts.append(bls._jac_to_aff(F1, cur))
        cur = bls._jac_add(F1, bls._jac_dbl(F1, cur), D)
    assert all(bls.on_curve(F1, p) for p in pts[:4] + pts[-4:])
    return tuple(pts)


def jac1(pt, z=1):
    """affine G1 point -> the Jacobian entry (x z^2, y z^3, z)"""
    return (pt[0] * z * z % P, pt[1] * z * z * z % P, z % P)


def aff1(J):
    return bls._jac_to_aff(F1, J)


def jac_words(entries):
    """Jacobian G1 entries -> flat list of 36 words each (X, Y, Z; Montgomery limbs)"""
    out = []
    for J in entries:
        for v in J:
            out += to_words(v)
    return out


def _values(ws, k):
    return [sum(int(w) << (32 * i) for i, w in enumerate(ws[12 * j:12 * j + 12])) * MONT_INV % P for j in range(k)]


def from_words1(ws):
    """36 words of k_qc_apk's output, the homogeneous (X Z : Y : Z^3) -> (affine point or None,
    the three values)"""
    X, Y, Z = v = _values(ws, 3)
    if Z == 0:
        return None, v
    zi = F1.inv(Z)
    return (X * zi % P, Y * zi % P), v


def proj_words(pt, z=F.one):
    """an affine G2 point (None: the identity) -> 72 words of a projective (X : Y : Z)"""
    vals = (F.zero, F.one, F.zero) if pt is None else (F.mul(pt[0], z), F.mul(pt[1], z), z)
    return [w for v in vals for c in v for w in to_words(c)]


def hom1_words(pt, z=1):
    """an affine G1 point (None: the identity) -> 36 words of a homogeneous (X : Y : Z)"""
    vals = (0, 1, 0) if pt is None else (pt[0] * z % P, pt[1] * z % P, z % P)
    return [w for v in vals for w in to_words(v)]


# ------------------------------------------------------------------------------ the selection
def select_reference(tn, codes, tidx, rank, orig=None, gid=None, groups=1, lsb_first=False):
    """-> (owner[groups tn], bitmap bytes[groups 4 bw], count[groups], taken[n]).

    Staged vote j < t = len(tidx) is a vote of table entry tidx[j] in group gid[j] (0 without gid)
    with the caller's index orig[j] (j without orig). Among the votes with code 0 of one entry in
    one group the lowest caller's index owns the entry, and that vote alone is taken: bit rank[e]
    of the group's bitmap (MSB first within a byte), one more in the group's count. Votes from t
    on are of no table entry and never taken. lsb_first: the wrong bit order, for the self-check
    of the comparison."""
    n, t = len(codes), len(tidx)
    bw = (tn + 31) // 32
    owner = [QC_NONE] * (groups * tn)
    who = lambda j: j if orig is None else orig[j]       # noqa: E731
    grp = lambda j: 0 if gid is None else gid[j]         # noqa: E731
    for j in range(t):
        if codes[j] == 0:
            k = grp(j) * tn + tidx[j]
            owner[k] = min(owner[k], who(j))
    bitmap, count, taken = bytearray(4 * groups * bw), [0] * groups, [0] * n
    for j in range(t):
        if codes[j] == 0 and owner[grp(j) * tn + tidx[j]] == who(j):
            taken[j] = 1
            k = rank[tidx[j]]
            bitmap[4 * grp(j) * bw + k // 8] |= (1 << (k % 8)) if lsb_first else (0x80 >> (k % 8))
            count[grp(j)] += 1
    return owner, bytes(bitmap), count, taken


def bitmap_words(bm):
    """the bitmap's bytes as the device's little-endian words"""
    return [int.from_bytes(bm[k:k + 4], "little") for k in range(0, len(bm), 4)]


class SelCase:
    def __init__(self, name, tn, codes, tidx, rank, orig=None, gid=None, groups=1):
        self.name, self.tn, self.codes, self.tidx, self.rank = name, tn, list(codes), list(tidx), list(rank)
        self.orig = None if orig is None else list(orig)
        self.gid = None if gid is None else list(gid)
        self.groups, self.n, self.t = groups, len(self.codes), len(self.tidx)
        self.bw = (tn + 31) // 32
        assert 0 < self.n and self.t <= self.n and 0 < groups <= GROUPS_MAX
        assert sorted(self.rank) == list(range(tn))
        assert all(0 <= e < tn for e in self.tidx)
        assert self.orig is None or sorted(self.orig) == list(range(self.n))
        assert self.gid is None or all(0 <= g < groups for g in self.gid)
        assert self.gid is not None or groups == 1

    def reference(self, **kw):
        return select_reference(self.tn, self.codes, self.tidx, self.rank, self.orig, self.gid, self.groups, **kw)

    def sizes(self):
        """words the kernels own in owner, bitmap, count, taken"""
        return self.groups * self.tn, self.groups * self.bw, self.groups, self.n


def selection_mismatches(case, owner, bitmap, count, taken):
    """device arrays (GUARD words, the kernels' words, GUARD words; sequences of ints) against the
    reference -> the names of what differs, [] when all is equal word for word"""
    r_owner, r_bm, r_count, r_taken = case.reference()
    want = (r_owner, bitmap_words(r_bm), r_count, r_taken)
    bad = []
    names = ("owner", "bitmap", "count", "taken")
    for name, got, ref, size in zip(names, (owner, bitmap, count, taken), want, case.sizes()):
        got = [int(x) for x in got]
        assert len(ref) == size and len(got) == size + 2 * GUARD, (case.name, name, len(got))
        if any(w != GUARD_WORD for w in got[:GUARD]):
            bad.append("%s: words written in front of the array" % name)
        if any(w != GUARD_WORD for w in got[GUARD + size:]):
            bad.append("%s: words written behind the array" % name)
        diff = [k for k in range(size) if got[GUARD + k] != ref[k]]
        if diff:
            bad.append("%s: %d words differ, the first at %d (got %#x, want %#x)"
                       % (name, len(diff), diff[0], got[GUARD + diff[0]], ref[diff[0]]))
    return bad


def with_guards(words):
    return [GUARD_WORD] * GUARD + list(words) + [GUARD_WORD] * GUARD


def _perm(rng, k):
    p = list(range(k))
    rng.shuffle(p)
    return p


SEL_TN = (1, 31, 32, 33, 257)
SEL_EXTRA = 7                 # votes beyond one per table entry


def sel_sized(tn, tk):
    """tn + 7 votes over a table of tn entries under a seeded rank permutation: duplicates, a
    quarter of the codes nonzero; tk names t: 0, 1, n - 1 or n. orig is a seeded permutation,
    except with t = n - 1 (the staged order is the caller's)."""
    n = tn + SEL_EXTRA
    t = {"0": 0, "1": 1, "n-1": n - 1, "n": n}[tk]
    rng = random.Random("qc-sel-%d-%s" % (tn, tk))
    tidx = [rng.randrange(tn) for _ in range(t)]
    codes = [rng.choice((0, 0, 0, 5)) for _ in range(n)]
    orig = None if tk == "n-1" else _perm(rng, n)
    return SelCase("tn%d-t%s" % (tn, tk), tn, codes, tidx, _perm(rng, tn), orig)


CONT_N, CONT_VOTES = 2 * WG + 40, 130


def sel_contention():
    """validator 3 of 5 has 130 valid votes spread over all three workgroups of the 168 staged
    votes; the caller's lowest index of them (0) is staged last, in the last workgroup. Validator
    1's lowest vote has a nonzero code: its next one is taken."""
    rng = random.Random("qc-sel-contention")
    n, tn = CONT_N, 5
    mine = sorted(rng.sample(range(n), CONT_VOTES))
    assert mine[0] < WG <= mine[64] < 2 * WG <= mine[-1]
    rest = [j for j in range(n) if j not in set(mine)]
    tidx = [3 if j in set(mine) else rng.choice((0, 1, 2, 4)) for j in range(n)]
    ones = [j for j in rest if tidx[j] == 1]
    assert len(ones) >= 3
    # caller's indices: 0 to validator 3's last staged vote, 1 to validator 1's first (code 5)
    orig = [None] * n
    orig[mine[-1]], orig[ones[0]] = 0, 1
    free = _perm(rng, n - 2)
    for j in range(n):
        if orig[j] is None:
            orig[j] = free.pop() + 2
    codes = [0] * n
    codes[ones[0]] = 5
    return SelCase("contention", tn, codes, tidx, _perm(rng, tn), orig)


def sel_all_failing():
    rng = random.Random("qc-sel-failing")
    n, tn = 70, 33
    return SelCase("all-failing", tn, [rng.choice((3, 5, 102)) for _ in range(n)], [rng.randrange(tn) for _ in range(n)],
                   _perm(rng, tn), _perm(rng, n))


def sel_groups(G):
    """G groups through gid over a table of 33 (G * tn, G * bw and G are the reset's three
    extents); with more than one group validator 3 is valid in groups 0 and G - 1, and with more
    than two, group 1 has no valid vote"""
    rng = random.Random("qc-sel-groups-%d" % G)
    tn, n = 33, 200
    gid = [j % G for j in range(n)]
    rng.shuffle(gid)
    tidx = [rng.randrange(tn) for _ in range(n - 9)]
    codes = [rng.choice((0, 0, 0, 5)) for _ in range(n)]
    if G > 1:
        if G > 2:
            codes = [5 if gid[j] == 1 else c for j, c in enumerate(codes)]
        for g in (0, G - 1):
            j = next(j for j in range(len(tidx)) if gid[j] == g)
            tidx[j], codes[j] = 3, 0
    return SelCase("groups%d" % G, tn, codes, tidx, _perm(rng, tn), _perm(rng, n), gid, G)


@functools.lru_cache(maxsize=None)
def selection_cases():
    cases = [sel_sized(tn, tk) for tn in SEL_TN for tk in ("0", "1", "n-1", "n")]
    cases += [sel_contention(), sel_all_failing()] + [sel_groups(G) for G in (1, 2, 64)]
    return {c.name: c for c in cases}


SELECTION_NAMES = tuple("tn%d-t%s" % (tn, tk) for tn in SEL_TN for tk in ("0", "1", "n-1", "n")) + (
    "contention", "all-failing", "groups1", "groups2", "groups64")


# ------------------------------------------------------------------------------ the masked sum
def segments(n, G, gid):
    """csrc/qc_segments.hpp restated -> (list, seg, chunks, entries)"""
    members = [[j for j in range(n) if gid[j] == g] for g in range(G)]
    lst, seg = [], []
    for m in members:
        seg += [len(lst) // CH, chunks(len(m))]
        lst += m + [QC_NONE] * (CH * chunks(len(m)) - len(m))
    return lst, seg, len(lst) // CH, len(lst) // 2


class SumCase:
    """points: n affine points (sigma of the staged votes); taken: n of 0 / 1; gid / G: the
    segmented form (None: the plain form, one group of all votes); expect: what the case is built
    to reach (check_sum_expectations)"""

    def __init__(self, name, points, taken, gid=None, G=1, expect=None):
        self.name, self.points, self.taken = name, list(points), [int(x) for x in taken]
        self.n, self.gid, self.G = len(self.points), None if gid is None else list(gid), G
        self.expect = dict(expect or {})
        assert self.n >= 2 and len(self.taken) == self.n and set(self.taken) <= {0, 1}
        assert (self.gid is None and G == 1) or (len(self.gid) == self.n and set(self.gid) == set(range(G)))

    def members(self, g):
        """the staged votes of group g, in the order of its list"""
        return list(range(self.n)) if self.gid is None else [j for j in range(self.n) if self.gid[j] == g]

    def masked(self, g):
        return [self.points[j] if self.taken[j] else None for j in self.members(g)]

    def group_sums(self):
        if not hasattr(self, "_sums"):
            self._sums = [psum(self.masked(g)) for g in range(self.G)]
        return self._sums

    def node(self, g, lv, k):
        """what entry k / 2 of the group's tree holds after level lv: the masked sum of the 2^(lv+1)
        votes from position k of the group's list (lv = -1: vote k itself)"""
        return psum(self.masked(g)[k:k + (1 << (lv + 1))])

    def operands(self, g, lv, k):
        """the two operands of the pair op at level lv, position k (a multiple of 2^(lv+1))"""
        assert k % (2 << lv) == 0
        return self.node(g, lv - 1, k), self.node(g, lv - 1, k + (1 << lv))


def check_sum_expectations(case):
    """the reference sums of a case really double, cancel or are the identity where it says"""
    e, eq = case.expect, lambda x, y: bls.pt_eq(F, x, y)       # noqa: E731
    for (g, lv, k) in e.get("double", ()):
        a, b = case.operands(g, lv, k)
        assert a is not None and eq(a, b), (case.name, "double", g, lv, k)
    for (g, lv, k) in e.get("cancel", ()):
        a, b = case.operands(g, lv, k)
        assert a is not None and eq(a, neg(b)) and case.node(g, lv, k) is None, (case.name, "cancel", g, lv, k)
    for (g, lv, k, which) in e.get("identity", ()):
        a, b = case.operands(g, lv, k)
        assert ((a is None) == (which in "LB")) and ((b is None) == (which in "RB")), (case.name, "identity", g, lv, k)
    for g, want in e.get("total", {}).items():
        assert eq(case.group_sums()[g], want), (case.name, "total", g)


def sum_mismatches(case, sums, out96):
    """device results (G x 72 words, G x 96 bytes) against the reference -> what differs, group
    sums first, then bytes. A device identity is Z = 0; otherwise (X / Z, Y / Z) must be the
    reference's affine point."""
    want, bad = case.group_sums(), []
    sums, out96 = [int(w) for w in sums], bytes(out96)
    assert len(sums) == 72 * case.G and len(out96) == 96 * case.G
    for g in range(case.G):
        if not bls.pt_eq(F, from_words(sums[72 * g:72 * g + 72]), want[g]):
            bad.append("group %d (%d votes, %d taken): the sum differs"
                       % (g, len(case.members(g)), sum(case.taken[j] for j in case.members(g))))
    for g in range(case.G):
        if out96[96 * g:96 * g + 96] != bls.g2_compress(want[g]):
            bad.append("group %d: the 96 compressed bytes differ" % g)
    return bad


PLAIN_SIZES = (2, 3, 63, 64, 65, 66, 127, 128, 129, 193, 1089)
# the pair count of level l, np = ceil((m - h) / 2 h) with h = 2^l, at m - h just below, at and just
# above a multiple of 2 h (m = 3 h - 1, 3 h, 3 h + 1) and at its least (m = h + 1), for every level
# inside a chunk (h = 2 .. 32, m <= 64) and for level 6 (h = 64: 191, 192; 193 is above)
NP_SIZES = (5, 6, 7, 9, 11, 12, 13, 17, 23, 24, 25, 33, 47, 48, 49, 191, 192)
PLAIN_MAX = max(PLAIN_SIZES)


def sum_points():
    return pool(PLAIN_MAX, "qc-sum")


def last_pair(m):
    """positions of the last level-0 pair of a chunk of m votes (one vote when m is odd)"""
    k = 2 * ((m - 1) // 2)
    return [k, k + 1] if k + 1 < m else [k]


def masks(n):
    """name -> taken[n]"""
    rng = random.Random("qc-masks-%d" % n)
    out = {"all": [1] * n, "none": [0] * n, "first": [1] + [0] * (n - 1), "last": [0] * (n - 1) + [1],
           "even": [1 - (j & 1) for j in range(n)], "odd": [j & 1 for j in range(n)],
           "half": [rng.randrange(2) for _ in range(n)], "sixteenth": [int(rng.randrange(16) == 0) for _ in range(n)]}
    nch = chunks(n)
    if nch >= 2:    # a whole chunk untaken: the first, a middle one, the last
        for c in sorted({0, nch // 2, nch - 1} if nch >= 3 else {0, nch - 1}):
            out["chunk%d-out" % c] = [int(j // CH != c) for j in range(n)]
    # the first and the last level-0 pair of every chunk untaken
    holes = set()
    for c in range(nch):
        m = min(CH, n - CH * c)
        holes |= {CH * c + k for k in [0, 1] + last_pair(m) if k < m}
    out["pairs-out"] = [int(j not in holes) for j in range(n)]
    return out


@functools.lru_cache(maxsize=None)
def plain_cases(n):
    """distinct points under every mask; one point everywhere under three of them"""
    pts = sum_points()[:n]
    cases = [SumCase("n%d-%s" % (n, name), pts, tk) for name, tk in masks(n).items()]
    one = pool(1, "qc-one")[0]
    for name in ("all", "even", "half"):
        tk = masks(n)[name]
        cases.append(SumCase("n%d-one-point-%s" % (n, name), [one] * n, tk, expect={"total": {0: mul(one, sum(tk))}}))
    return cases


@functools.lru_cache(maxsize=None)
def np_cases(n):
    pts = sum_points()[:n]
    return [SumCase("n%d-%s" % (n, name), pts, masks(n)[name]) for name in ("all", "half")]


def _level_block(pts, lv, sign):
    """2^(lv+1) points: a_0 .. a_(h-1), then the same (sign 1) or their negatives (sign -1)"""
    h = 1 << lv
    return list(pts[:h]) + [p if sign > 0 else neg(p) for p in pts[:h]]


@functools.lru_cache(maxsize=None)
def level_cases():
    """name -> SumCase: P + P and P + (-P) at a chosen level. Levels 0-5 fill chunk 0 of 66 votes
    with blocks that double or cancel at that level (level 0 is madd: P beside P, P beside -P);
    votes 64 and 65 are two more points, so level 6 adds O + Q where chunk 0 cancels. Levels 6 and
    7 repeat or negate whole chunks."""
    A = pool(64, "qc-level")
    Q = pool(4, "qc-level-q")
    cases = []
    for lv in range(CH_LV):
        span = 2 << lv
        for sign, word in ((1, "double"), (-1, "cancel")):
            pts = [p for k in range(0, CH, span) for p in _level_block(A[k:], lv, sign)] + list(Q[:2])
            chunk0 = mul(psum(A[k + i] for k in range(0, CH, span) for i in range(span // 2)), 2) if sign > 0 else None
            e = {word: [(0, lv, k) for k in range(0, CH, span)], "total": {0: psum([chunk0, Q[0], Q[1]])}}
            if sign < 0:
                e["identity"] = [(0, CH_LV, 0, "L")] + ([(0, lv + 1, 0, "B")] if lv + 1 < CH_LV else [])
            cases.append(SumCase("level%d-%s" % (lv, word), pts, [1] * len(pts), expect=e))
    S = psum(A)
    # level 6: chunk 1 repeats or negates chunk 0; with nothing else taken the negation is O overall
    cases.append(SumCase("level6-double", list(A) + list(A), [1] * 128,
                         expect={"double": [(0, 6, 0)], "total": {0: mul(S, 2)}}))
    cases.append(SumCase("level6-cancel", list(A) + [neg(p) for p in A], [1] * 128,
                         expect={"cancel": [(0, 6, 0)], "total": {0: None}}))
    cases.append(SumCase("level6-cancel-then-Q", list(A) + [neg(p) for p in A] + [Q[0]], [1] * 129,
                         expect={"cancel": [(0, 6, 0)], "identity": [(0, 7, 0, "L")], "total": {0: Q[0]}}))
    # level 7: chunks 2, 3 repeat or negate chunks 0, 1
    B = pool(128, "qc-level7")
    S = psum(B)
    cases.append(SumCase("level7-double", list(B) + list(B), [1] * 256,
                         expect={"double": [(0, 7, 0)], "total": {0: mul(S, 2)}}))
    cases.append(SumCase("level7-cancel", list(B) + [neg(p) for p in B], [1] * 256,
                         expect={"cancel": [(0, 7, 0)], "total": {0: None}}))
    # the identity as the left, the right and both operands of level 6 (a whole chunk untaken)
    for which, tk in (("L", [0] * 64 + [1] * 64), ("R", [1] * 64 + [0] * 64), ("B", [0] * 128)):
        cases.append(SumCase("level6-identity-%s" % which, sum_points()[:128], tk, expect={"identity": [(0, 6, 0, which)]}))
    return {c.name: c for c in cases}


LEVEL_NAMES = tuple("level%d-%s" % (lv, w) for lv in range(CH_LV) for w in ("double", "cancel")) + (
    "level6-double", "level6-cancel", "level6-cancel-then-Q", "level7-double", "level7-cancel",
    "level6-identity-L", "level6-identity-R", "level6-identity-B")

SEG_SIZES = (1, 2, 63, 64, 65, 128, 129)


def _interleaved(sizes, tag):
    gid = [g for g, m in enumerate(sizes) for _ in range(m)]
    random.Random("qc-seg-%s" % tag).shuffle(gid)
    return gid


def _by_group(gid, G, patterns):
    """points[j] = patterns[g][position of vote j in group g]"""
    pos, pts = [0] * G, []
    for g in gid:
        pts.append(patterns[g][pos[g]])
        pos[g] += 1
    return pts


@functools.lru_cache(maxsize=None)
def seg_cases():
    """name -> SumCase of the segmented form"""
    cases = []
    n = sum(SEG_SIZES)
    gid = _interleaved(SEG_SIZES, "sizes")
    pts = pool(n, "qc-seg")
    rng = random.Random("qc-seg-masks")
    empty = SEG_SIZES.index(65)
    for name, tk in (("all", [1] * n), ("half", [rng.randrange(2) for _ in range(n)]),
                     ("group-untaken", [int(g != empty) for g in gid])):
        cases.append(SumCase("seg-sizes-%s" % name, pts, tk, gid, len(SEG_SIZES),
                             expect={"total": {empty: None}} if name == "group-untaken" else None))
    # in the segmented form a chunk's vote count m comes from a ballot over the list: the sizes that
    # put every level's pair count at and beside its steps, one group each
    gid = _interleaved(NP_SIZES, "np")
    cases.append(SumCase("seg-pair-counts", pool(sum(NP_SIZES), "qc-seg-np"), [1] * sum(NP_SIZES), gid, len(NP_SIZES)))
    # 64 singleton groups at n = 64: 2,048 tree entries, more than the 2,044 of the least capacity
    gid = _perm(random.Random("qc-seg-singletons"), 64)
    for name, tk in (("all", [1] * 64), ("even", [1 - (j & 1) for j in range(64)])):
        cases.append(SumCase("seg-singletons-%s" % name, pts[:64], tk, gid, 64,
                             expect={"total": {gid[j]: pts[j] if tk[j] else None for j in range(64)}}))
    # group 0: two chunks with equal sums; group 1: two chunks with opposite sums; group 2: 66 votes,
    # its second chunk one pad-free pair; group 3: nothing taken
    A, B, C, D = pool(64, "qc-seg-a"), pool(64, "qc-seg-b"), pool(66, "qc-seg-c"), pool(5, "qc-seg-d")
    sizes = (128, 128, 66, 5)
    gid = _interleaved(sizes, "exceptional")
    pts = _by_group(gid, 4, [list(A) + list(A), list(B) + [neg(p) for p in B], list(C), list(D)])
    cases.append(SumCase("seg-exceptional", pts, [int(g != 3) for g in gid], gid, 4,
                         expect={"double": [(0, 6, 0)], "cancel": [(1, 6, 0)],
                                 "total": {0: mul(psum(A), 2), 1: None, 2: psum(C), 3: None}}))
    return {c.name: c for c in cases}


SEG_NAMES = ("seg-sizes-all", "seg-sizes-half", "seg-sizes-group-untaken", "seg-pair-counts", "seg-singletons-all",
             "seg-singletons-even", "seg-exceptional")


# ------------------------------------------------------------------------------ the key sum
APK_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 200)
APK_KEYS, APK_NEG = 200, 64   # table: 200 keys, then the negatives of the first 64
ONE_KEY = tuple((7, c) for c in APK_COUNTS) + ((10, 2), (10, 65), (10, 200))   # (entry, voters), all voters that entry


@functools.lru_cache(maxsize=None)
def apk_table():
    """264 Jacobian entries; every seventh has Z != 1"""
    K = pool1(APK_KEYS, "apk")
    rng = random.Random("qc-apk-z")
    aff = list(K) + [neg1(p) for p in K[:APK_NEG]]
    return tuple(jac1(p, rng.randrange(2, P) if e % 7 == 3 else 1) for e, p in enumerate(aff))


class ApkCase:
    """lists: per QC the table entries of its voters, in order; expect: {QC: point or None}"""

    def __init__(self, name, lists, expect=None):
        self.name, self.lists, self.expect = name, [list(x) for x in lists], dict(expect or {})
        self.nq = len(self.lists)
        assert all(0 <= e < len(apk_table()) for x in self.lists for e in x)

    def off(self):
        out = [0]
        for x in self.lists:
            out.append(out[-1] + len(x))
        return out

    def ent(self):
        return [e for x in self.lists for e in x]

    def sums(self):
        if not hasattr(self, "_sums"):
            T = [aff1(J) for J in apk_table()]
            self._sums = [psum1(T[e] for e in x) for x in self.lists]
        return self._sums


def apk_mismatches(case, out, flags):
    """device results (nq x 36 words, nq flag words) against the reference -> what differs. A
    device identity is exactly (0, 1, 0) with flag PKF_INF; otherwise the flag is 0 and
    (X / Z, Y / Z) of the homogeneous (X Z : Y : Z^3) must be the reference's affine point."""
    want, bad = case.sums(), []
    out, flags = [int(w) for w in out], [int(f) for f in flags]
    assert len(out) == 36 * case.nq and len(flags) == case.nq
    for q in range(case.nq):
        got, v = from_words1(out[36 * q:36 * q + 36])
        what = "QC %d (%d voters)" % (q, len(case.lists[q]))
        if not bls.pt_eq(F1, got, want[q]):
            bad.append(what + ": the sum differs")
        elif got is None and v != [0, 1, 0]:
            bad.append(what + ": the identity is not (0, 1, 0)")
        if flags[q] != (PKF_INF if want[q] is None else 0):
            bad.append(what + ": flag %#x" % flags[q])
    return bad


@functools.lru_cache(maxsize=None)
def apk_cases():
    rng = random.Random("qc-apk-cases")
    K = [aff1(J) for J in apk_table()]
    N = APK_KEYS                                   # entry N + i is -K_i
    distinct = lambda c: rng.sample(range(APK_KEYS), c)   # noqa: E731
    cases = [ApkCase("counts", [distinct(c) for c in APK_COUNTS]),
             ApkCase("nq1", [list(range(APK_KEYS))]),
             ApkCase("nq2", [distinct(129), distinct(1)]),
             ApkCase("nq65", [distinct(APK_COUNTS[q % 9]) for q in range(65)]),
             # one key at every selected entry (entry 10 has Z != 1): every add after the first is a
             # doubling or meets a multiple
             ApkCase("one-key", [[e] * c for e, c in ONE_KEY], {q: mul1(K[e], c) for q, (e, c) in enumerate(ONE_KEY)})]
    seq = list(range(64))
    # a key and its copy / its negation 64 entries apart: one lane's share, jac_add doubles / cancels
    cases.append(ApkCase("same-lane",
                         [seq + [0], seq + [63], seq + seq + [0], seq + [N], seq + [N + 63], [3] + seq[1:] + [N + 3]],
                         {0: psum1([K[e] for e in seq] + [K[0]]), 3: psum1(K[e] for e in seq[1:]),
                          4: psum1(K[e] for e in seq[:63])}))
    # ... in lanes that meet in the LDS tree: lanes 0 and 1 (the last step), t and t + 32 (the first)
    half = list(range(32))
    cases.append(ApkCase("tree", [[5, 5], half + half, [5, N + 5, 9], half + [N + e for e in half] + [40]],
                         {0: mul1(K[5], 2), 1: mul1(psum1(K[e] for e in half), 2), 2: K[9], 3: K[40]}))
    # the identity as a whole: flag PKF_INF, output (0, 1, 0)
    cases.append(ApkCase("identity", [[5, N + 5], half + [N + e for e in half], seq + [N + e for e in seq],
                                      [N + e for e in seq] + seq[::-1], [10, N + 10]],
                         {q: None for q in range(5)}))
    return {c.name: c for c in cases}


APK_NAMES = ("counts", "nq1", "nq2", "nq65", "one-key", "same-lane", "tree", "identity")
