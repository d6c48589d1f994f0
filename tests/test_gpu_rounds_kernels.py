"""The kernels of ovh_rounds_add on crafted rounds against exact expectations: the selection through
the table of round references (k_qc_claim_r, k_qc_mark_r), the segmented sum, the segmented merge
(k_qc_merge_seg), the gather and the compression (csrc/qc.hpp).

Through ovh_rounds_add every vote is a verified signature of an unrelated key, so a test cannot
choose the claims a round already holds, its running sum or the points of a call. The test-only
probe (tests/device/rounds_probe.hip, built by `make -C consensus_overlord_amd` as
tests/device/_build/libroundsprobe.so) includes the product translation unit whole and calls the
product's own launch code (enqueue_qc_rounds) on rounds the test lays out in QcRound's layout, each
an allocation of its own between guard words.

The expected values are plain loops and oracle/py/bls12_381.py point arithmetic on Python integers
(tests/qc_cases.py's helpers). Every comparison is exact: owner, bitmap, count and merged word for
word, guard and pad words included; an R that must not move is compared bit for bit (it is
poisoned with 0xFF words first); a merged R is Z = 0 for the identity, otherwise (X / Z, Y / Z)
must equal the affine reference; the 96 bytes must equal the oracle's compression."""
import ctypes
import os
import random

import numpy as np
import pytest

import bls12_381 as bls
import qc_cases as qc
from vm_helpers import ROOT

pytestmark = pytest.mark.gpu

PROBE = os.path.join(ROOT, "tests", "device", "_build", "libroundsprobe.so")
u32p = ctypes.POINTER(ctypes.c_uint32)
i32p = ctypes.POINTER(ctypes.c_int32)
u8p = ctypes.POINTER(ctypes.c_uint8)
u32 = ctypes.c_uint32
NONE = 0xFFFFFFFF
PAD = 0x5A5A5A5A          # the words of a round's allocation that no kernel owns (pad, ovh_round_qc's bytes)


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(PROBE):
        pytest.fail("%s is missing: run build() (make -C consensus_overlord_amd) first" % PROBE)
    lib = ctypes.CDLL(PROBE)
    lib.rp_rounds.argtypes = [u32, u32, u32, u32, i32p, i32p, u32p, u32p, u32p, u32p, u32p, u32p, u32p, u32p, u8p]
    lib.rp_rounds.restype = ctypes.c_int
    for f in (lib.rp_guard, lib.rp_round_words, lib.rp_r_off):
        f.restype = u32
    lib.rp_round_words.argtypes = lib.rp_r_off.argtypes = [u32]
    lib.rp_close.restype = None
    assert lib.rp_guard() == qc.GUARD
    yield lib
    lib.rp_close()


@pytest.fixture(scope="module")
def pts():
    return qc.pool(140, "rounds-kernels")


class Round:
    """a round's state before the call: base, the claims it holds (entry -> claim), count, merged
    and R (an affine point, None for the identity, or "poison": 0xFF words that must not move)"""

    def __init__(self, base=0, owner=None, count=0, merged=0, R=None, z=None):
        self.base, self.owner, self.count, self.merged, self.R, self.z = base, dict(owner or {}), count, merged, R, z


def _bit(words, k):
    words[k >> 5] |= 1 << (8 * ((k >> 3) & 3) + 7 - (k & 7))


def run(probe, tn, rank, rounds, votes):
    """votes: staged list of (round number, position among the round's votes, code, table entry or
    None -- those last --, point). -> nothing; asserts every output."""
    K, n = len(rounds), len(votes)
    t = sum(1 for v in votes if v[3] is not None)
    assert all(v[3] is not None for v in votes[:t]) and all(v[3] is None for v in votes[t:])
    bw = (tn + 31) // 32
    words, r_off, G = probe.rp_round_words(tn), probe.rp_r_off(tn), qc.GUARD
    assert r_off >= tn + bw + 2 and words == r_off + 72 + 24
    stride = words + 2 * G
    state = np.zeros(K * stride, dtype=np.uint32)
    want_state, want_rows, want_out, want_R = [], [], [], []
    want_taken = [0] * n
    for g, r in enumerate(rounds):
        w = [PAD] * words
        w[:tn] = [r.owner.get(e, NONE) for e in range(tn)]
        bm = [0] * bw
        for e in r.owner:
            _bit(bm, rank[e])
        w[tn:tn + bw] = bm
        w[tn + bw], w[tn + bw + 1] = r.count, r.merged
        w[r_off:r_off + 72] = [NONE] * 72 if r.R == "poison" else qc.proj_words(r.R, r.z or qc.F.one)
        state[g * stride + G:g * stride + G + words] = w
        # the reference: claims, marks, the call's sum, the gated merge
        exp = list(w)
        mine = [(j, v) for j, v in enumerate(votes) if v[0] == g]
        for j, (_, pos, code, e, _) in mine:
            if e is not None and code == 0:
                exp[e] = min(exp[e], r.base + pos)
        cnt, taken_pts = r.count, []
        for j, (_, pos, code, e, pt) in mine:
            if e is not None and code == 0 and exp[e] == r.base + pos:
                want_taken[j] = 1
                cnt += 1
                taken_pts.append(pt)
                k = rank[e]
                exp[tn + (k >> 5)] |= 1 << (8 * ((k >> 3) & 3) + 7 - (k & 7))
        exp[tn + bw] = cnt
        if cnt != r.merged:
            assert r.R != "poison"
            exp[tn + bw + 1] = cnt
            want_R.append(("point", qc.psum([r.R] + taken_pts)))
        else:
            want_R.append(("same", w[r_off:r_off + 72]))
        want_state.append(exp)
        want_rows += [cnt] + exp[tn:tn + bw]
        if r.R == "poison":
            want_out.append(None)      # the bytes of 0xFF words are nobody's business
        else:
            want_out.append(bls.g2_compress(want_R[-1][1] if want_R[-1][0] == "point" else r.R) if cnt else b"\xff" * 96)
    arr = lambda vals, dt=np.uint32: np.ascontiguousarray(np.array(vals, dtype=dt).reshape(-1))   # noqa: E731
    codes, tidx = arr([v[2] for v in votes], np.int32), arr([v[3] for v in votes[:t]] or [0], np.int32)
    orig, gid, rk = arr([v[1] for v in votes]), arr([v[0] for v in votes]), arr(rank)
    base = arr([r.base for r in rounds])
    sigma = arr(qc.point_words([v[4] for v in votes]))
    taken = np.zeros(n, dtype=np.uint32)
    rows = np.zeros(K * (1 + bw), dtype=np.uint32)
    out = np.zeros(96 * K, dtype=np.uint8)
    p = lambda a, ty=u32p: a.ctypes.data_as(ty)   # noqa: E731
    rc = probe.rp_rounds(tn, K, n, t, p(codes, i32p), p(tidx, i32p), p(orig), p(rk), p(gid), p(base), p(sigma), p(state),
                         p(taken), p(rows), p(out, u8p))
    assert rc == 0, "rp_rounds returned %d" % rc
    assert taken.tolist() == want_taken, "taken"
    for g in range(K):
        got = state[g * stride:(g + 1) * stride].tolist()
        assert got[:G] == [NONE] * G and got[G + words:] == [NONE] * G, "round %d: guard words" % g
        got, exp = got[G:G + words], want_state[g]
        assert got[:r_off] == exp[:r_off], "round %d: owner | bitmap | count | merged | pad" % g
        assert got[r_off + 72:] == exp[r_off + 72:], "round %d: the words behind R" % g
        kind, ref = want_R[g]
        if kind == "same":
            assert got[r_off:r_off + 72] == ref, "round %d: R moved though the call took nothing" % g
        else:
            assert qc.from_words(got[r_off:r_off + 72]) == ref, "round %d: merged R" % g
        assert want_out[g] is None or out[96 * g:96 * g + 96].tobytes() == want_out[g], "round %d: bytes" % g
    assert rows.tolist() == want_rows, "gathered rows"


def _rank(tn, seed):
    r = list(range(tn))
    random.Random(seed).shuffle(r)
    return r


def test_one_round(probe, pts):
    """K = 1: first merge (R is the identity), a base, a duplicate inside the call staged in reverse,
    an invalid vote, a vote of no table entry"""
    tn = 33
    votes = [(0, 3, 0, 5, pts[0]), (0, 0, 0, 5, pts[1]), (0, 1, 5, 7, pts[2]), (0, 2, 0, 32, pts[3]), (0, 4, 0, None, pts[4])]
    run(probe, tn, _rank(tn, 1), [Round(base=9)], votes)


def test_two_rounds_with_their_own_bases_and_an_earlier_claim(probe, pts):
    """K = 2: the rounds' bases differ (3 and 1,000); round 0 holds a claim of an earlier add on entry 4
    (1 < base) that beats this call's vote; the same entry in round 1 is free; round 0's R is a sum of
    earlier votes in projective form with Z != 1, round 1's the identity"""
    tn = 67
    z = (123456789, 987654321)
    r0 = Round(base=3, owner={4: 1, 60: 0}, count=2, merged=2, R=qc.psum([pts[100], pts[101]]), z=z)
    votes = [(0, 0, 0, 4, pts[0]), (1, 0, 0, 4, pts[1]), (0, 1, 0, 9, pts[2]), (1, 1, 0, 66, pts[3]), (1, 2, 3, 9, pts[4]),
             (0, 2, 0, 9, pts[5])]
    run(probe, tn, _rank(tn, 2), [r0, Round(base=1000)], votes)


def test_sixteen_rounds(probe, pts):
    """K = 16, votes interleaved: round 0 has 65 votes (the upper level of its sum runs) beside
    singleton rounds; round 3 takes nothing (its only vote loses to an earlier claim): R poisoned
    beforehand, bit-identical afterwards, merged unchanged; round 5's call sum equals its R (a
    doubling); round 6's is opposite to its R (the identity, the count still advanced); round 7's vote
    is invalid on a fresh round (count 0: no bytes); votes of no table entry at the end"""
    tn = 70
    rounds = [Round(base=g) for g in range(16)]
    by_round = {g: [] for g in range(16)}
    by_round[0] = [(0, e, pts[e]) for e in range(65)]
    rounds[3] = Round(base=50, owner={11: 7}, count=1, merged=1, R="poison")
    by_round[3] = [(0, 11, pts[66])]
    rounds[5] = Round(base=2, owner={1: 0, 2: 1}, count=2, merged=2, R=qc.psum([pts[70], pts[71]]))
    by_round[5] = [(0, 20, pts[70]), (0, 21, pts[71])]
    rounds[6] = Round(base=2, owner={1: 0, 2: 1}, count=2, merged=2, R=qc.neg(qc.psum([pts[72], pts[73]])), z=(5, 7))
    by_round[6] = [(0, 30, pts[72]), (0, 31, pts[73])]
    by_round[7] = [(5, 12, pts[74])]
    for g in (1, 2, 4, 8, 9, 10, 11, 12, 13, 14, 15):
        by_round[g] = [(0, (7 * g) % tn, pts[80 + g])]
    staged = []
    for g, vs in by_round.items():
        staged += [(g, pos, code, e, pt) for pos, (code, e, pt) in enumerate(vs)]
    random.Random(16).shuffle(staged)
    outsiders = [(0, len(by_round[0]), 0, None, pts[120]), (9, 1, 0, None, pts[121])]
    run(probe, tn, _rank(tn, 3), rounds, staged + outsiders)


def test_entry_point_refuses_bad_arguments(probe, pts):
    tn, p = 8, lambda a, ty=u32p: a.ctypes.data_as(ty)   # noqa: E731
    words = probe.rp_round_words(tn) + 2 * qc.GUARD
    a = dict(tn=tn, K=2, n=2, t=2, codes=np.zeros(2, np.int32), tidx=np.array([1, 2], np.int32), orig=np.zeros(2, np.uint32),
             rank=np.arange(tn, dtype=np.uint32), gid=np.array([0, 1], np.uint32), base=np.zeros(2, np.uint32),
             sigma=np.array(qc.point_words(pts[:2]), np.uint32), state=np.zeros(2 * words, np.uint32),
             taken=np.zeros(2, np.uint32), rows=np.zeros(4, np.uint32), out=np.zeros(192, np.uint8))

    def call(**kw):
        x = dict(a, **kw)
        return probe.rp_rounds(x["tn"], x["K"], x["n"], x["t"], p(x["codes"], i32p), p(x["tidx"], i32p), p(x["orig"]),
                               p(x["rank"]), p(x["gid"]), p(x["base"]), p(x["sigma"]), p(x["state"]), p(x["taken"]),
                               p(x["rows"]), p(x["out"], u8p))
    for kw in (dict(n=1, t=1), dict(K=0), dict(K=17), dict(t=3), dict(tn=0), dict(tidx=np.array([1, tn], np.int32)),
               dict(tidx=np.array([-1, 2], np.int32)), dict(gid=np.array([0, 2], np.uint32)),
               dict(gid=np.array([0, 0], np.uint32)),                      # round 1 without a vote
               dict(rank=np.array([0] * (tn - 1) + [tn], np.uint32)), dict(orig=np.array([0, 2], np.uint32))):
        assert call(**kw) == 1, sorted(kw)
