"""ovh_build_qcs on the GPU: the QCs of a mixed-hash vote set in one device
pass, against the C oracle (every vote under its own hash) and the grouping + selection model
(tests/qc_groups_model.py).

Every group is signed on the device (test_gpu_samemsg._round, one call per group over the same
key range, so the groups share one validator table) and the groups are interleaved with a seeded
shuffle. For every non-empty group the oracle's aggregate of the taken votes equals out_sigs[g]
and verifies over extract_voters(table, bitmaps[g]); one verify_qc_batch over all the QCs is all
0; every later verify_signature is a verdict-cache hit with the oracle's code. Outputs start as
0xEE bytes, so what the call must not write is seen. The shapes are the smallest that reach each
edge of the segment layout and the routing; each test's docstring or comment names its edge."""
import ctypes
import random

import numpy as np
import pytest

import orc
import qc_groups_model
import synth_votes as sv
from test_gpu_build_qc import _make_round, _verify_code
from test_gpu_samemsg import _round

pytestmark = pytest.mark.gpu

SENT = 0xEE


@pytest.fixture(scope="module")
def cc():
    import consensus_overlord_amd as coa
    return coa.ConsensusCrypto(bytes.fromhex("7c" * 32))


def _arr(items, w):
    return np.frombuffer(b"".join(items), dtype=np.uint8).reshape(len(items), w)


def _call(cc, sigs, hashes, voters, max_groups=64, bitmap_len=None):
    """The raw C call over sentinel-filled outputs -> (return code, dict of the arrays)."""
    n = len(sigs)
    bl = (len(cc.pubkeys) + 7) // 8 if bitmap_len is None else bitmap_len
    mg = max(max_groups, 1)
    o = {"codes": np.full(n, -1, dtype=np.int32), "taken": np.full(n, SENT, dtype=np.uint8),
         "group": np.full(n, 0xEEEEEEEE, dtype=np.uint32), "gh": np.full((mg, 32), SENT, dtype=np.uint8),
         "out": np.full((mg, 96), SENT, dtype=np.uint8), "bm": np.full((mg, max(bl, 1)), SENT, dtype=np.uint8),
         "cnt": np.full(mg, 0xEEEEEEEE, dtype=np.uint32)}
    ng = ctypes.c_uint32(0xEEEEEEEE)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    r = cc.lib.ovh_build_qcs(cc.ctx.ptr, n, b"".join(sigs), b"".join(hashes), b"".join(voters), p(o["codes"]),
                             p(o["taken"]), p(o["group"]), max_groups, ctypes.byref(ng), p(o["gh"]), p(o["out"]),
                             p(o["bm"]), bl, p(o["cnt"]))
    o["ng"] = ng.value
    return r, o


def _untouched(o):
    return (o["ng"] == 0xEEEEEEEE and (o["codes"] == -1).all() and (o["taken"] == SENT).all()
            and (o["group"] == 0xEEEEEEEE).all() and (o["gh"] == SENT).all() and (o["out"] == SENT).all()
            and (o["bm"] == SENT).all() and (o["cnt"] == 0xEEEEEEEE).all())


def _check(cc, sigs, hashes, voters, table, cache=True, wrapper=True):
    """One ovh_build_qcs call against the oracle and the model; -> (want codes, model, outputs)."""
    from consensus_overlord_amd import vote
    n = len(sigs)
    cc.update_pubkeys(table)
    bl = (len(table) + 7) // 8
    want = sv.oracle_codes(_arr(sigs, 96), _arr(hashes, 32), _arr(voters, 48))
    m_group, m_gh, m_taken, m_bm, m_cnt = qc_groups_model.select(want, hashes, voters, table)
    G = len(m_gh)
    r, o = _call(cc, sigs, hashes, voters)
    print("n", n, "G", G, "return", r, "n_signed", o["cnt"][:G].tolist(), "model", m_cnt,
          "codes", sorted(set(o["codes"].tolist())))
    assert r == 0 and o["ng"] == G
    assert o["codes"].tolist() == want.tolist()
    assert o["group"].tolist() == m_group
    assert [o["gh"][g].tobytes() for g in range(G)] == m_gh
    assert o["taken"].tolist() == m_taken
    assert o["cnt"][:G].tolist() == m_cnt
    assert [o["bm"][g, :bl].tobytes() for g in range(G)] == m_bm
    # nothing past group G - 1
    assert (o["gh"][G:] == SENT).all() and (o["out"][G:] == SENT).all() and (o["cnt"][G:] == 0xEEEEEEEE).all()
    qs, qh, qb = [], [], []
    for g in range(G):
        if not m_cnt[g]:
            assert (o["out"][g] == SENT).all(), g          # an empty group's signature is not written
            continue
        idx = [i for i in range(n) if m_group[i] == g and m_taken[i]]
        agg = o["out"][g].tobytes()
        assert (0, agg) == orc.aggregate_sigs([sigs[i] for i in idx], [voters[i] for i in idx]), g
        assert orc.verify_aggregated(agg, m_gh[g], vote.extract_voters(table, m_bm[g])) == 0, g
        qs.append(agg), qh.append(m_gh[g]), qb.append(m_bm[g])
    if qs:
        assert cc.verify_qc_batch(qs, qh, qb).tolist() == [0] * len(qs)
    if wrapper:
        qcs, codes, taken, group = cc.build_qcs(sigs, hashes, voters)
        assert codes.tolist() == want.tolist() and taken.astype(int).tolist() == m_taken and group.tolist() == m_group
        assert [(q[0], q[2], q[3]) for q in qcs] == list(zip(m_gh, m_bm, m_cnt))
        assert [q[1] for q in qcs] == [o["out"][g].tobytes() if m_cnt[g] else None for g in range(G)]
    if cache:
        h0, m0, _ = cc.cache_stats()
        for i in range(n):
            assert _verify_code(cc, sigs[i], hashes[i], voters[i]) == want[i], i
        h1, m1, _ = cc.cache_stats()
        assert h1 - h0 == n and m1 == m0
    return want, (m_group, m_gh, m_taken, m_bm, m_cnt), o


def _signed(ctx, lo, v, digests):
    """Keys lo .. lo + v - 1 signing every digest (one device call per digest) ->
    (sig[g][k] bytes, pk[k] bytes)."""
    sig, pk = [], None
    for d in digests:
        s, p = _round(ctx, lo, v, d)
        sig.append([bytes(x) for x in s])
        pk = [bytes(x) for x in p]
    return sig, pk


def _votes(sig, pk, digests, picks, seed=None):
    """picks: (group, key) pairs -> (sigs, hashes, voters), shuffled when seed is given."""
    picks = list(picks)
    if seed is not None:
        random.Random(seed).shuffle(picks)
    return [sig[g][k] for g, k in picks], [digests[g] for g, _ in picks], [pk[k] for _, k in picks]


def test_two_groups_of_one(cc):
    ds = [sv.sha(b"qcs two %d" % g) for g in range(2)]
    sig, pk = _signed(cc.ctx, 98000, 2, ds)
    _, m, _ = _check(cc, *_votes(sig, pk, ds, [(0, 0), (1, 1)]), pk)
    assert m[4] == [1, 1]


def test_non_table_voter_first_makes_its_hash_group_0(cc):
    """Staged order puts the table votes (hash A) first: the plan's group 0 is A, the caller's B."""
    A, B = sv.sha(b"qcs order A"), sv.sha(b"qcs order B")
    sig, pk = _signed(cc.ctx, 98010, 3, [A, B])
    _, m, o = _check(cc, *_votes(sig, pk, [A, B], [(1, 2), (0, 0), (0, 1)]), pk[:2])
    assert m[1] == [B, A] and m[0] == [0, 1, 1] and m[4] == [0, 2]
    assert o["bm"][0, 0] == 0 and o["bm"][1, 0] == 0b11000000


def test_groups_of_64_65_and_1_interleaved(cc):
    """Segment padding, a chunk boundary inside a group, k_qc_upper over two chunks beside groups of
    one chunk; validators 0..63 vote in two groups (equivocation), each taken in both."""
    ds = [sv.sha(b"qcs 130 %d" % g) for g in range(3)]
    sig, pk = _signed(cc.ctx, 98100, 65, ds)
    picks = [(0, k) for k in range(64)] + [(1, k) for k in range(65)] + [(2, 7)]
    want, m, _ = _check(cc, *_votes(sig, pk, ds, picks, seed=130), pk)
    assert not want.any() and sorted(m[4]) == [1, 64, 65]


def test_three_groups_of_67_with_every_corruption(cc, golden):
    """test_gpu_build_qc._make_round's corruptions (sigma + G2, sig_not_in_g2, pk_x_eq_p, an
    outsider, a duplicate, invalid-then-valid) inside each of three interleaved groups."""
    ds = [sv.sha(b"qcs 3x67 %d" % g) for g in range(3)]
    votes, table = [], None
    for d in ds:
        s, v, table = _make_round(cc.ctx, golden, 98300, 67, d)
        votes += [(x, d, y) for x, y in zip(s, v)]
    random.Random(67).shuffle(votes)
    want, m, _ = _check(cc, [x[0] for x in votes], [x[1] for x in votes], [x[2] for x in votes], table)
    assert sorted(set(want.tolist())) == [0, 3, 5, 102]
    assert want.tolist().count(0) == 3 * 63 and m[4] == [61, 61, 61]


def test_group_of_1100_beside_a_group_of_5(cc):
    """18 chunks in one group: k_qc_upper's eight-pairs-at-a-time loop, while another group has one."""
    ds = [sv.sha(b"qcs 1100 %d" % g) for g in range(2)]
    sig, pk = _signed(cc.ctx, 99000, 1100, ds)
    picks = [(0, k) for k in range(1100)] + [(1, k) for k in (3, 64, 500, 1023, 1099)]
    want, m, _ = _check(cc, *_votes(sig, pk, ds, picks, seed=1100), pk, wrapper=False)
    assert not want.any() and sorted(m[4]) == [5, 1100]


def test_equivocation_wrong_hash_and_an_all_invalid_group(cc):
    A, B, C = (sv.sha(b"qcs mix " + x) for x in (b"A", b"B", b"C"))
    sig, pk = _signed(cc.ctx, 98500, 4, [A, B, C])
    sigs = [sig[0][0], sig[1][0], sig[0][1], sig[1][2],      # key 0 valid on A and on B: taken twice
            sig[0][3],                                       # signed on A, submitted under B: 5
            sv.add_g2(sig[2][1]), sv.add_g2(sig[2][2])]      # group C: every vote fails
    hashes = [A, B, A, B, B, C, C]
    voters = [pk[0], pk[0], pk[1], pk[2], pk[3], pk[1], pk[2]]
    want, m, o = _check(cc, sigs, hashes, voters, pk)
    assert want.tolist() == [0, 0, 0, 0, 5, 5, 5]
    assert m[2] == [1, 1, 1, 1, 0, 0, 0] and m[4] == [2, 2, 0]
    assert (o["out"][2] == SENT).all() and o["bm"][2, 0] == 0


def test_one_hash_equals_build_qc_byte_for_byte(cc, golden):
    d = sv.sha(b"qcs one hash")
    sigs, voters, table = _make_round(cc.ctx, golden, 98600, 67, d)
    _, _, o = _check(cc, sigs, [d] * 67, voters, table, cache=False)
    code, agg, bitmap, codes, taken, cnt = cc.build_qc_raw(sigs, d, voters)
    assert code == 0 and o["ng"] == 1
    assert o["out"][0].tobytes() == agg and o["bm"][0, :len(bitmap)].tobytes() == bitmap and o["cnt"][0] == cnt
    assert o["codes"].tolist() == codes.tolist() and o["taken"].astype(bool).tolist() == taken.tolist()


def test_64_singleton_groups_need_the_raised_capacity():
    """2,048 tree entries against the 2,044 a 64-vote batch's slab holds; a fresh context, so the
    slab is not already large from another test."""
    import consensus_overlord_amd as coa
    c2 = coa.ConsensusCrypto(bytes.fromhex("7d" * 32))
    ds = [sv.sha(b"qcs single %d" % g) for g in range(64)]
    sigs, voters = [], []
    for g, d in enumerate(ds):
        s, p = _round(c2.ctx, 98700 + g, 1, d)
        sigs.append(bytes(s[0])), voters.append(bytes(p[0]))
    order = list(range(64))
    random.Random(64).shuffle(order)
    want, m, _ = _check(c2, [sigs[i] for i in order], [ds[i] for i in order], [voters[i] for i in order], voters)
    assert not want.any() and m[4] == [1] * 64


def test_too_many_groups_is_an_argument_error_and_writes_nothing(cc):
    d = sv.sha(b"qcs limits")
    sg, pk = _round(cc.ctx, 98800, 3, d)
    table = [bytes(x) for x in pk]
    cc.update_pubkeys(table)
    n = 65
    sigs, voters = [bytes(sg[0])] * n, [table[0]] * n
    hashes = [d] + [sv.sha(b"qcs limit %d" % i) for i in range(1, n)]
    for args, kw in (((sigs, hashes, voters), {}),                          # 65 distinct hashes
                     ((sigs[:3], hashes[:3], voters[:3]), {"max_groups": 2}),     # max_groups below G
                     ((sigs[:3], hashes[:3], voters[:3]), {"max_groups": 0}),
                     ((sigs[:3], hashes[:3], voters[:3]), {"bitmap_len": 2})):
        r, o = _call(cc, *args, **kw)
        assert r == 103 and _untouched(o), kw
    r, o = _call(cc, sigs[:3], hashes[:3], voters[:3], max_groups=3)        # exactly G: accepted
    assert r == 0 and o["ng"] == 3 and o["codes"].tolist() == [0, 5, 5] and o["cnt"][:3].tolist() == [1, 0, 0]


def test_multi_device_context(cc):
    import consensus_overlord_amd as coa
    from consensus_overlord_amd.crypto import Context
    mc = coa.ConsensusCrypto(bytes.fromhex("7b" * 32), ctx=Context(devices=[0, 0]))
    ds = [sv.sha(b"qcs multi %d" % g) for g in range(2)]
    sig, pk = _signed(cc.ctx, 98900, 40, ds)
    picks = [(0, k) for k in range(40)] + [(1, k) for k in range(30)]
    _, m, _ = _check(mc, *_votes(sig, pk, ds, picks, seed=70), pk)
    assert sorted(m[4]) == [30, 40]


def test_build_vote_qcs_prevotes_split_between_a_block_hash_and_nil(cc):
    from consensus_overlord_amd import vote
    height, round_ = 77, 1
    bh = cc.hash(b"block 77 body")
    tuples = [(height, round_, vote.PREVOTE, bh), (height, round_, vote.PREVOTE, b"")]
    ds = [vote.vote_hash(cc, *t) for t in tuples]
    assert ds[0] != ds[1]
    sig, pk = _signed(cc.ctx, 98950, 10, ds)
    picks = [(1, 9)] + [(0, k) for k in range(7)] + [(1, k) for k in range(7, 9)]       # a nil vote arrives first
    sigs, hashes, voters = _votes(sig, pk, ds, picks)
    cc.update_pubkeys(pk)
    qcs, codes, taken, group = cc.build_vote_qcs(sigs, [tuples[g] for g, _ in picks], voters)
    assert not codes.any() and taken.all() and group.tolist() == [0] + [1] * 7 + [0] * 2
    assert [q[0] for q in qcs] == [tuples[1], tuples[0]]
    assert [q[1] for q in qcs] == [ds[1], ds[0]]
    assert [q[4] for q in qcs] == [3, 7]
    for t, h, agg, bitmap, cnt in qcs:
        assert orc.verify_aggregated(agg, h, vote.extract_voters(pk, bitmap)) == 0
    assert cc.verify_qc_batch([q[2] for q in qcs], [q[1] for q in qcs], [q[3] for q in qcs]).tolist() == [0, 0]
