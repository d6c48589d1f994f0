"""Which workgroup runs which pair in the merged-level MSM kernels of
consensus_overlord_amd/csrc/msm.hpp (k_msm_chunk, k_msm_upper, k_msm_plane, k_msm_comb),
restated launch by launch and workgroup by workgroup. tests/test_msm_model.py restates the same
trees one launch per level; here the levels run inside workgroups, so the model also checks what
that relies on: a workgroup reads only entries that an earlier launch or it itself wrote, writes
only entries no other workgroup of its launch touches, and every pair of every level is run
exactly once. The group is either the integers mod r (a point is its discrete logarithm: exact
and fast, so whole 4,096-vote batches run) or the oracle's G2."""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle", "py"))

import bls12_381 as bls  # noqa: E402

NBW, NB, NT, TM = 255, 4 * 255, 32, 64
CH_LV, CH = 6, 64
SL8, SL16 = 8, 4          # pairs per run: 8-lane slices (madd, padd), 16-lane slices (hdbl)


class Store:
    """An A or U array that records, per launch, which workgroup wrote an entry."""

    def __init__(self):
        self.v = {}
        self.writer = {}      # entry -> workgroup, this launch only
        self.reader = {}

    def launch(self):
        self.writer, self.reader = {}, {}

    def rd(self, wg, i):
        assert self.writer.get(i, wg) == wg, "reads another workgroup's result of the same launch"
        self.reader.setdefault(i, set()).add(wg)
        return self.v[i]

    def wr(self, wg, i, x):
        assert self.writer.get(i, wg) == wg, "two workgroups write one entry"
        assert self.reader.get(i, {wg}) == {wg}, "writes an entry another workgroup reads"
        self.writer[i] = wg
        self.v[i] = x


def merged_msm(grp, points, tau, scalars64, valid):
    add, mul2k, ident = grp
    n = len(points)
    pt = lambda pid: (points if pid % 2 == 0 else tau)[pid // 2]   # noqa: E731
    half = lambda r, h: (r >> 32) & 0xFFFFFFFF if h else r & 0xFFFFFFFF   # noqa: E731
    digits = [(i, h, w, (half(scalars64[i], h) >> (8 * w)) & 255)
              for i in range(n) if valid[i] for h in range(2) for w in range(4)]
    cnt = [0] * NB
    for _, _, w, d in digits:
        if d:
            cnt[w * NBW + d - 1] += 1

    def prefix(f):
        row, acc = [], 0
        for c in cnt:
            row.append(acc)
            acc += f(c)
        return row + [acc]
    off = prefix(lambda c: c)
    pf0 = prefix(lambda c: (c + 1) // 2)          # k_msm_scan row 0
    pfc = prefix(lambda c: (c + CH - 1) >> CH_LV)  # row 1
    cur, ent = list(off), [None] * off[-1]
    random.Random(7).shuffle(digits)              # the device's atomics order is arbitrary
    for i, h, w, d in digits:
        if d:
            b = w * NBW + d - 1
            ent[cur[b]] = 2 * i + h
            cur[b] += 1

    def find(row, q):
        lo, hi = 0, NB
        while hi - lo > 1:
            mid = (lo + hi) >> 1
            if row[mid] <= q:
                lo = mid
            else:
                hi = mid
        return lo
    A, U = Store(), Store()
    pairs = 0
    # k_msm_chunk: grid 8n / 64 + NB, workgroups past the chunk count exit
    grid = (8 * n >> CH_LV) + NB
    assert pfc[NB] <= grid
    for g in range(pfc[NB]):
        b = find(pfc, g)
        k0 = (g - pfc[b]) << CH_LV
        c, a0, e0 = cnt[b], pf0[b], off[b]
        m = min(c - k0, CH)
        assert m >= 1
        lv = 0
        while lv < CH_LV and (lv == 0 or (1 << lv) < m):
            h = 1 << lv
            np_ = (m + 1) // 2 if lv == 0 else (m - h + 2 * h - 1) >> (lv + 1)
            for r in range(0, np_, SL8):
                for p in range(r, min(r + SL8, np_)):
                    k = k0 + (p << (lv + 1))
                    if lv == 0:
                        other = pt(ent[e0 + k + 1]) if k + 1 < c else ident
                        A.wr(g, a0 + (k >> 1), add(pt(ent[e0 + k]), other))
                    else:
                        assert k + h < c
                        ia, ib = a0 + (k >> 1), a0 + ((k + h) >> 1)
                        A.wr(g, ia, add(A.rd(g, ia), A.rd(g, ib)))
                    pairs += 1
            lv += 1
    # k_msm_upper: a workgroup per bucket, skipped by the host when no bucket can pass one chunk
    A.launch()
    if 2 * n > CH:
        for b in range(NB):
            c, a0 = cnt[b], pf0[b]
            if c <= CH:
                continue
            lv = CH_LV
            while (1 << lv) < c:
                h = 1 << lv
                np_ = (c - h + 2 * h - 1) >> (lv + 1)
                for p in range(np_):
                    k = p << (lv + 1)
                    assert k + h < c
                    ia, ib = a0 + (k >> 1), a0 + ((k + h) >> 1)
                    A.wr(b, ia, add(A.rd(b, ia), A.rd(b, ib)))
                    pairs += 1
                lv += 1
    else:
        assert max(cnt) <= CH
    # every point entered a tree once and every bucket's tree has c - 1 additions (level 0 also
    # runs the lone entry at an odd end)
    assert pairs == sum(c - 1 + (c & 1) for c in cnt if c)
    A.launch()

    def member(j, k):
        return ((j >> k) << (k + 1)) | (1 << k) | (j & ((1 << k) - 1))
    # k_msm_plane(lo, hi): 0..3 on NT * 8 workgroups, 4..6 on NT
    for lo, hi in ((0, 3), (4, 6)):
        U.launch()
        per_t = TM >> hi
        for wg in range(NT * per_t):
            t, g = wg // per_t, wg % per_t
            for lv in range(lo, hi + 1):
                np_ = 1 << (hi - lv)
                for p in range(np_):
                    i = g * np_ + p
                    assert i < (TM >> lv)
                    if lv == 0:
                        w, k = t >> 3, t & 7
                        b0 = w * NBW + member(2 * i, k) - 1
                        b1 = w * NBW + member(2 * i + 1, k) - 1
                        x = A.rd(0, pf0[b0]) if cnt[b0] else ident
                        y = A.rd(0, pf0[b1]) if cnt[b1] else ident
                        U.wr(wg, t * TM + i, add(x, y))
                    else:
                        e = t * TM + (i << lv)
                        U.wr(wg, e, add(U.rd(wg, e), U.rd(wg, e + (1 << (lv - 1)))))
    # k_msm_comb(lo, hi): 1..3 on NT / 8 workgroups, 4..5 on one
    for lo, hi in ((1, 3), (4, 5)):
        U.launch()
        for wg in range(NT >> hi):
            for h in range(lo, hi + 1):
                np_, m = 1 << (hi - h), 1 << (h - 1)
                for r in range(0, np_, SL16):
                    for p in range(r, min(r + SL16, np_)):
                        e = 2 * m * (wg * np_ + p) * TM
                        U.wr(wg, e, add(U.rd(wg, e), mul2k(U.rd(wg, e + m * TM), m)))
    return U.v[0]


R = bls.R
LAMBDA = (-(bls.X * bls.X)) % R     # tau = -psi^2(sigma) = [lambda] sigma
ZR = (lambda a, b: (a + b) % R, lambda a, m: (a << m) % R, 0)


def _zr_case(n, scal, valid, seed):
    rng = random.Random(seed)
    logs = [rng.randrange(1, R) for _ in range(n)]
    tau = [x * LAMBDA % R for x in logs]
    want = sum(x * ((r & 0xFFFFFFFF) + (r >> 32) * LAMBDA) for x, r, v in zip(logs, scal, valid) if v) % R
    assert merged_msm(ZR, logs, tau, scal, valid) == want


def test_merged_levels_random_batches():
    """the GPU test's sizes (chunk and bucket boundaries of every kernel) and a full batch"""
    for n in (1, 2, 3, 31, 32, 33, 64, 65, 129, 257, 4096):
        rng = random.Random(n)
        scal = [rng.getrandbits(64) or 1 for _ in range(n)]
        valid = [rng.randrange(8) != 0 or n < 4 for _ in range(n)]
        _zr_case(n, scal, valid, 100 + n)


def test_merged_levels_crowded_buckets():
    """every point in the same four buckets: chunks of 1 .. 64 entries at a bucket's end, several
    chunks per bucket, levels above the chunk's (k_msm_upper), and edge digits"""
    for n in (16, 32, 33, 48, 64, 65, 96, 97, 128, 129, 300, 1025):
        scal = [0x03030303_03030303] * n
        scal[0] = 0x00000001_000000FF
        scal[n // 2] = 0xFFFFFFFF_FFFFFFFF
        valid = [True] * n
        valid[n - 1] = n % 2 == 0
        _zr_case(n, scal, valid, 200 + n)
    # one point per half in one bucket each: 2n entries in bucket (0, 5) only
    for n in (32, 33, 100):
        _zr_case(n, [0x00000005_00000005] * n, [True] * n, 300 + n)
    assert merged_msm(ZR, [5, 6], [5 * LAMBDA % R, 6 * LAMBDA % R], [3, 4], [False, False]) == 0


def test_merged_levels_on_g2():
    """the same schedule over the oracle's G2 (None is the identity), crowded enough for two
    chunks and one upper level"""
    F = bls.Fp2Ops
    n = 40
    rng = random.Random(0xC17A)
    base = bls.hash_to_g2(b"\x00" * 32)
    pts = [bls.pt_mul(F, base, rng.randrange(1, 1 << 16)) for _ in range(n)]
    tau = [bls.pt_neg(F, bls.g2_psi(bls.g2_psi(p))) for p in pts]
    scal = [0x00000101_00000101 if k % 8 else rng.getrandbits(64) for k in range(n)]
    valid = [k != 7 for k in range(n)]
    grp = (lambda a, b: bls.pt_add(F, a, b), lambda a, m: bls.pt_mul(F, a, 1 << m), None)
    acc = None
    for p, r, v in zip(pts, scal, valid):
        if v:
            acc = bls.pt_add(F, acc, bls.pt_mul(F, p, ((r & 0xFFFFFFFF) + (r >> 32) * LAMBDA) % R))
    assert merged_msm(grp, pts, tau, scal, valid) == acc
