"""The expected values of tests/test_gpu_qc_kernels.py, checked without a GPU: the selection
reference of tests/qc_cases.py agrees with the models the end-to-end tests use (tests/qc_model.py,
tests/qc_groups_model.py) once its index arrays are turned back into keys and hashes; the sum and
key-sum cases reach what they are built for (a "cancel" case sums to the identity, a "double" case
has equal operands at the level it names, one point everywhere gives [popcount] P); the segment
lists are those tests/host/qc_segments_harness.cpp pins; and the comparison helpers the GPU test
uses notice a perturbed result (a taken vote dropped, orig ignored, the bitmap read LSB first)."""
import random

import pytest

import bls12_381 as bls
import qc_cases as qc
import qc_groups_model
import qc_model

F = qc.F


def same(x, y):
    return bls.pt_eq(F, x, y)


# ------------------------------------------------------------------------------ selection
def test_case_names():
    assert tuple(qc.selection_cases()) == qc.SELECTION_NAMES
    assert tuple(qc.level_cases()) == qc.LEVEL_NAMES
    assert tuple(qc.seg_cases()) == qc.SEG_NAMES
    assert tuple(qc.apk_cases()) == qc.APK_NAMES


def _as_votes(c):
    """the case in the terms of the models, in the caller's order: table keys whose sorted order
    is `rank`, a voter key per vote (a key outside the table from staged vote t on), a hash per
    vote (its group), and the caller's index of every staged vote"""
    table = [b"key%08d" % c.rank[e] for e in range(c.tn)]
    who = list(range(c.n)) if c.orig is None else c.orig
    codes, voters, hashes = [None] * c.n, [None] * c.n, [None] * c.n
    for j in range(c.n):
        codes[who[j]] = c.codes[j]
        voters[who[j]] = table[c.tidx[j]] if j < c.t else b"outsider%04d" % j
        hashes[who[j]] = b"hash%04d" % (0 if c.gid is None else c.gid[j])
    return table, who, codes, voters, hashes


@pytest.mark.parametrize("name", qc.SELECTION_NAMES)
def test_selection_reference_is_the_model(name):
    c = qc.selection_cases()[name]
    owner, bitmap, count, taken = c.reference()
    table, who, codes, voters, hashes = _as_votes(c)
    nbytes = (c.tn + 7) // 8
    if c.gid is None:
        m_taken, m_bitmap, m_cnt = qc_model.select(codes, voters, table)
        assert [m_taken[who[j]] for j in range(c.n)] == taken
        assert bitmap[:nbytes] == m_bitmap and not any(bitmap[nbytes:]) and count == [m_cnt]
    else:
        group, ghashes, m_taken, m_bitmaps, m_counts = qc_groups_model.select(codes, hashes, voters, table)
        assert [m_taken[who[j]] for j in range(c.n)] == taken
        for g in range(c.groups):       # the model numbers the groups by first appearance
            h = b"hash%04d" % g
            if h not in ghashes:
                assert g not in c.gid
                continue
            k = ghashes.index(h)
            bm = bitmap[4 * c.bw * g:4 * c.bw * (g + 1)]
            assert bm[:nbytes] == m_bitmaps[k] and not any(bm[nbytes:]) and count[g] == m_counts[k]
    # owner: QC_NONE exactly where no vote is taken for the entry
    held = {(0 if c.gid is None else c.gid[j]) * c.tn + c.tidx[j] for j in range(c.t) if taken[j]}
    assert {k for k, o in enumerate(owner) if o != qc.QC_NONE} == held
    assert sum(taken) == sum(count) == len(held)


def test_selection_cases_reach_their_edges():
    cs = qc.selection_cases()
    assert {c.tn for c in cs.values()} >= set(qc.SEL_TN)
    for tn in qc.SEL_TN:
        n = tn + qc.SEL_EXTRA
        assert [cs["tn%d-t%s" % (tn, k)].t for k in ("0", "1", "n-1", "n")] == [0, 1, n - 1, n]
        assert cs["tn%d-tn" % tn].rank != list(range(tn)) or tn == 1
    assert cs["tn33-tn-1"].orig is None and cs["tn33-tn"].orig is not None
    # contention: 130 valid votes of validator 3 in all three workgroups, the winner staged last
    c = cs["contention"]
    mine = [j for j in range(c.n) if c.tidx[j] == 3]
    assert len(mine) == qc.CONT_VOTES and all(c.codes[j] == 0 for j in mine)
    assert {j // qc.WG for j in mine} == {0, 1, 2} and c.n == qc.CONT_N
    win = min(mine, key=lambda j: c.orig[j])
    assert win == mine[-1] == max(mine) and win // qc.WG == 2 and c.orig[win] == 0
    taken = c.reference()[3]
    assert [j for j in mine if taken[j]] == [win]
    # validator 1: its lowest caller's index has a nonzero code, the next lowest is taken
    ones = sorted((j for j in range(c.n) if c.tidx[j] == 1), key=lambda j: c.orig[j])
    assert c.codes[ones[0]] != 0 and [j for j in ones if taken[j]] == [ones[1]]
    # every code nonzero
    c = cs["all-failing"]
    owner, bitmap, count, taken = c.reference()
    assert all(c.codes) and set(owner) == {qc.QC_NONE} and not any(bitmap) and count == [0] and not any(taken)
    # groups: 1, 2 and 64; a group without a valid vote; one validator valid in two groups
    for G in (2, 64):
        c = cs["groups%d" % G]
        owner, bitmap, count, taken = c.reference()
        assert c.groups == G and set(c.gid) == set(range(G)) and c.t < c.n
        assert min(count[0], count[G - 1]) > 0 and (G == 2 or (count[1] == 0 and 1 in c.gid))
        assert owner[3] != qc.QC_NONE and owner[(G - 1) * c.tn + 3] != qc.QC_NONE
    c = cs["groups64"]
    assert c.sizes()[:3] == (64 * 33, 64 * 2, 64) and c.tn % 32


def test_comparison_notices_a_wrong_selection():
    """the helper passes the reference itself and fails it with orig ignored, with the bitmap read
    LSB first, with a word written outside an array and with one owner word left unreset"""
    c = qc.selection_cases()["contention"]
    owner, bitmap, count, taken = c.reference()
    arrays = lambda o, b, n, t: [qc.with_guards(x) for x in (o, qc.bitmap_words(b), n, t)]   # noqa: E731
    assert qc.selection_mismatches(c, *arrays(owner, bitmap, count, taken)) == []
    # orig swapped for the identity: the first staged vote of a validator wins instead
    o2, b2, n2, t2 = qc.select_reference(c.tn, c.codes, c.tidx, c.rank, None, c.gid, c.groups)
    bad = qc.selection_mismatches(c, *arrays(o2, b2, n2, t2))
    assert any(x.startswith("owner") for x in bad) and any(x.startswith("taken") for x in bad)
    assert b2 == bitmap and n2 == count      # the same validators either way: only owner and taken tell
    # the bitmap LSB first
    o3, b3, n3, t3 = c.reference(lsb_first=True)
    bad = qc.selection_mismatches(c, *arrays(o3, b3, n3, t3))
    assert len(bad) == 1 and bad[0].startswith("bitmap")
    for name in ("tn33-tn", "groups64"):
        d = qc.selection_cases()[name]
        assert any(x.startswith("bitmap") for x in qc.selection_mismatches(d, *arrays(*d.reference(lsb_first=True)))), name
    # a reset one word long or one word short
    a = arrays(owner, bitmap, count, taken)
    a[0][qc.GUARD + len(owner)] = qc.QC_NONE - 1
    assert qc.selection_mismatches(c, *a) == ["owner: words written behind the array"]
    a = arrays(owner, bitmap, count, taken)
    a[2][qc.GUARD - 1] = 0
    assert qc.selection_mismatches(c, *a) == ["count: words written in front of the array"]
    a = arrays(owner[:-1] + [0x1234], bitmap, count, taken)
    assert len(qc.selection_mismatches(c, *a)) == 1


# ------------------------------------------------------------------------------ the masked sum
def test_plain_masks():
    for n in qc.PLAIN_SIZES + qc.NP_SIZES:
        m = qc.masks(n)
        assert all(len(tk) == n for tk in m.values())
        assert sum(m["all"]) == n and sum(m["none"]) == 0 and m["first"][0] == m["last"][-1] == 1
        assert sum(m["first"]) == sum(m["last"]) == 1
        assert [a + b for a, b in zip(m["even"], m["odd"])] == [1] * n
    m = qc.masks(1089)
    assert qc.chunks(1089) == 18 and {"chunk0-out", "chunk9-out", "chunk17-out"} <= set(m)
    for c in (0, 9, 17):
        assert [j for j in range(1089) if not m["chunk%d-out" % c][j]] == list(range(64 * c, min(64 * c + 64, 1089)))
    assert {"chunk0-out", "chunk1-out", "chunk2-out"} <= set(qc.masks(129)) and "chunk0-out" not in qc.masks(64)
    assert set(qc.masks(65)) >= {"chunk0-out", "chunk1-out"}
    m = qc.masks(129)["pairs-out"]
    assert [j for j in range(129) if not m[j]] == [0, 1, 62, 63, 64, 65, 126, 127, 128]
    assert [j for j in range(63) if not qc.masks(63)["pairs-out"][j]] == [0, 1, 62]
    assert 0 < sum(qc.masks(1089)["sixteenth"]) < 1089 // 8 < 1089 // 3 < sum(qc.masks(1089)["half"])


def test_np_sizes_meet_every_level():
    """np = ceil((m - h) / 2 h): the sizes put m - h at 1, 2 h - 1, 2 h and 2 h + 1 for h = 2 .. 16,
    at 1 for h = 32, and n - 64 at 127, 128, 129 for level 6"""
    have = set(qc.PLAIN_SIZES + qc.NP_SIZES)
    for h in (2, 4, 8, 16):
        assert {h + 1, 3 * h - 1, 3 * h, 3 * h + 1} <= have, h
    assert {33, 63, 64, 191, 192, 193} <= have
    assert qc.chunks(1089) == 18 and 1089 % 64 == 1     # 17 chunks and one vote: the upper loop runs 9, 5, 3, 2, 1 pairs


@pytest.mark.parametrize("n", (2, 65, 129, 1089))
def test_plain_reference(n):
    """the tree-shaped reference (SumCase.node) is the flat sum, and one point everywhere sums to
    [popcount] P"""
    top = max(0, (n - 1).bit_length() - 1)
    for c in qc.plain_cases(n):
        if n > 200 and c.name.split("-", 1)[1] not in ("all", "half", "chunk9-out", "one-point-half"):
            continue
        assert same(c.node(0, top, 0), c.group_sums()[0]), c.name
        assert bls.on_curve(F, c.group_sums()[0])
        assert (c.group_sums()[0] is None) == (sum(c.taken) == 0), c.name
        qc.check_sum_expectations(c)
    ones = [c for c in qc.plain_cases(n) if "one-point" in c.name]
    assert len(ones) == 3 and all(len(set(c.points)) == 1 for c in ones)
    assert all(same(c.group_sums()[0], qc.mul(c.points[0], sum(c.taken))) for c in ones)


@pytest.mark.parametrize("name", qc.LEVEL_NAMES)
def test_level_cases_double_and_cancel_where_they_say(name):
    c = qc.level_cases()[name]
    assert c.expect
    qc.check_sum_expectations(c)
    if name.startswith("level") and name[5].isdigit() and int(name[5]) < qc.CH_LV and "identity" not in name:
        lv = int(name[5])
        assert c.n == 66 and len(c.expect.get("double", c.expect.get("cancel"))) == 64 >> (lv + 1)
        # below the named level nothing doubles or cancels
        for low in range(lv):
            for k in range(0, 64, 2 << low):
                a, b = c.operands(0, low, k)
                assert a is not None and b is not None and not same(a, b) and not same(a, qc.neg(b)), (name, low, k)
    if name == "level6-cancel":
        assert c.group_sums() == [None] and c.node(0, 5, 0) is not None and c.node(0, 5, 64) is not None


@pytest.mark.parametrize("name", qc.SEG_NAMES)
def test_segmented_cases(name):
    c = qc.seg_cases()[name]
    qc.check_sum_expectations(c)
    lst, seg, nch, entries = qc.segments(c.n, c.G, c.gid)
    # what tests/host/qc_segments_harness.cpp pins for csrc/qc_segments.hpp
    assert len(seg) == 2 * c.G and len(lst) == 64 * nch and entries == 32 * nch
    nxt = 0
    for g in range(c.G):
        mem = c.members(g)
        assert seg[2 * g] == nxt and seg[2 * g + 1] == (len(mem) + 63) // 64
        mine = lst[64 * nxt:64 * (nxt + seg[2 * g + 1])]
        assert mine[:len(mem)] == mem == sorted(mem) and set(mine[len(mem):]) <= {qc.QC_NONE}
        nxt += seg[2 * g + 1]
    assert nxt == nch and nch <= (c.n + 63) // 64 + c.G and 2 * entries <= c.n + 64 * c.G
    assert sorted(x for x in lst if x != qc.QC_NONE) == list(range(c.n))
    # the flat sums again, from the list
    for g in range(c.G):
        mine = [j for j in lst[64 * seg[2 * g]:64 * (seg[2 * g] + seg[2 * g + 1])] if j != qc.QC_NONE]
        assert same(qc.psum(c.points[j] for j in mine if c.taken[j]), c.group_sums()[g])


def test_segmented_cases_reach_their_edges():
    cs = qc.seg_cases()
    c = cs["seg-sizes-all"]
    assert sorted(len(c.members(g)) for g in range(c.G)) == sorted(qc.SEG_SIZES)
    assert c.gid != sorted(c.gid)                                       # interleaved
    c = cs["seg-sizes-group-untaken"]
    g = qc.SEG_SIZES.index(65)
    assert c.group_sums()[g] is None and all(s is not None for k, s in enumerate(c.group_sums()) if k != g)
    c = cs["seg-pair-counts"]
    assert [len(c.members(g)) for g in range(c.G)] == list(qc.NP_SIZES) and all(c.taken)
    # 64 singletons: 2,048 entries against msm_acap(256) = 4 * 256 + MSM_NB = 2,044
    c = cs["seg-singletons-all"]
    assert c.n == 64 and c.G == 64 and qc.segments(64, 64, c.gid)[2:] == (64, 2048)
    assert 2048 > 4 * 256 + qc.MSM_NB and (2048 - qc.MSM_NB + 3) // 4 == 257
    c = cs["seg-exceptional"]
    assert [len(c.members(g)) for g in range(4)] == [128, 128, 66, 5]
    assert same(c.node(0, 5, 0), c.node(0, 5, 64)) and same(c.node(1, 5, 0), qc.neg(c.node(1, 5, 64)))
    assert c.node(2, 5, 64) is not None and not any(c.taken[j] for j in c.members(3))


def test_comparison_notices_a_dropped_vote():
    """the helper passes the reference itself (any Z) and fails the sum of all taken votes but
    one, in the sum and in the bytes; the stages come in the order sums, bytes"""
    rng = random.Random(5)
    for c in (qc.plain_cases(65)[0], qc.seg_cases()["seg-sizes-half"], qc.level_cases()["level6-cancel"]):
        want = c.group_sums()
        z = (rng.randrange(1, qc.P), rng.randrange(qc.P))
        sums = [w for s in want for w in qc.proj_words(s, z)]
        out = b"".join(bls.g2_compress(s) for s in want)
        assert qc.sum_mismatches(c, sums, out) == [], c.name
        j = next(j for j in range(c.n - 1, -1, -1) if c.taken[j])
        g = 0 if c.gid is None else c.gid[j]
        d = qc.SumCase("dropped", c.points, [int(t and k != j) for k, t in enumerate(c.taken)], c.gid, c.G)
        short = d.group_sums()
        sums = [w for s in short for w in qc.proj_words(s, z)]
        bad = qc.sum_mismatches(c, sums, b"".join(bls.g2_compress(s) for s in short))
        assert len(bad) == 2 and bad[0].startswith("group %d " % g), (c.name, bad)
        assert "sum" in bad[0] and "bytes" in bad[1], (c.name, bad)
        assert qc.sum_mismatches(c, sums, out) == bad[:1]
    # poison (0xFF words) is neither a sum nor the identity
    c = qc.level_cases()["level6-cancel"]
    bad = qc.sum_mismatches(c, [0xFFFFFFFF] * 72, bls.g2_compress(None))
    assert bad == ["group 0 (128 votes, 128 taken): the sum differs"]


# ------------------------------------------------------------------------------ the key sum
def test_apk_table():
    T = qc.apk_table()
    assert len(T) == qc.APK_KEYS + qc.APK_NEG
    aff = [qc.aff1(J) for J in T]
    assert all(bls.on_curve(qc.F1, p) for p in aff)
    assert all(bls.pt_eq(qc.F1, aff[qc.APK_KEYS + i], qc.neg1(aff[i])) for i in range(qc.APK_NEG))
    assert len({p[0] for p in aff[:qc.APK_KEYS]}) == qc.APK_KEYS
    assert [e for e, J in enumerate(T) if J[2] != 1] == list(range(3, len(T), 7)) and T[10][2] != 1
    assert bls.g1_in_subgroup(aff[0]) and bls.g1_in_subgroup(aff[199])


@pytest.mark.parametrize("name", qc.APK_NAMES)
def test_apk_reference(name):
    c = qc.apk_cases()[name]
    sums = c.sums()
    assert len(c.off()) == c.nq + 1 and c.off()[-1] == len(c.ent())
    for q, want in c.expect.items():
        assert bls.pt_eq(qc.F1, sums[q], want), (name, q)
    assert all(bls.on_curve(qc.F1, s) for s in sums)
    if name == "identity":
        assert sums == [None] * c.nq
    else:
        assert None not in sums


def test_apk_cases_reach_their_edges():
    cs = qc.apk_cases()
    assert tuple(len(x) for x in cs["counts"].lists) == qc.APK_COUNTS
    assert all(len(set(x)) == len(x) for x in cs["counts"].lists)
    assert [cs[k].nq for k in ("nq1", "nq2", "nq65")] == [1, 2, 65]
    assert len({len(x) for x in cs["nq65"].lists}) == 9 and len(cs["nq2"].lists[0]) != len(cs["nq2"].lists[1])
    T = [qc.aff1(J) for J in qc.apk_table()]
    eq, neg = lambda a, b: bls.pt_eq(qc.F1, T[a], T[b]), lambda a, b: bls.pt_eq(qc.F1, T[a], qc.neg1(T[b]))   # noqa: E731
    # one lane's share is entries t, t + 64, ...: equal or opposite keys 64 apart
    L = cs["same-lane"].lists
    assert eq(L[0][0], L[0][64]) and eq(L[1][63], L[1][64]) and eq(L[2][0], L[2][64]) and eq(L[2][0], L[2][128])
    assert neg(L[3][0], L[3][64]) and neg(L[4][63], L[4][64]) and neg(L[5][0], L[5][64]) and qc.apk_table()[3][2] != 1
    # the LDS tree adds lane t + s to lane t for s = 32, 16, .., 1
    L = cs["tree"].lists
    assert eq(L[0][0], L[0][1]) and all(eq(L[1][t], L[1][t + 32]) for t in range(32))
    assert neg(L[2][0], L[2][1]) and all(neg(L[3][t], L[3][t + 32]) for t in range(32))
    assert any(qc.apk_table()[e][2] != 1 for x in cs["identity"].lists for e in x)


def test_comparison_notices_a_wrong_key_sum():
    c = qc.apk_cases()["tree"]
    want = c.sums()
    out = [w for q, s in enumerate(want) for w in qc.hom1_words(s, 3 + q)]
    assert qc.apk_mismatches(c, out, [0] * c.nq) == []
    assert qc.apk_mismatches(c, out, [0, 0, qc.PKF_INF, 0]) == ["QC 2 (3 voters): flag 0x2"]
    wrong = list(out)
    wrong[:36] = qc.hom1_words(qc.aff1(qc.apk_table()[5]))           # P where P + P is due
    assert qc.apk_mismatches(c, wrong, [0] * c.nq) == ["QC 0 (2 voters): the sum differs"]
    c = qc.apk_cases()["identity"]
    ident = [w for _ in range(c.nq) for w in qc.hom1_words(None)]
    assert qc.apk_mismatches(c, ident, [qc.PKF_INF] * c.nq) == []
    assert len(qc.apk_mismatches(c, ident, [0] * c.nq)) == c.nq
    odd = list(ident)
    odd[0:12] = qc.to_words(7)                                        # (7, 1, 0): Z = 0, not the stated form
    assert qc.apk_mismatches(c, odd, [qc.PKF_INF] * c.nq) == ["QC 0 (2 voters): the identity is not (0, 1, 0)"]
