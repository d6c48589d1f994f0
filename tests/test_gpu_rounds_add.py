"""ovh_rounds_add on the GPU: a flush's votes added to several open rounds
in one device pass, end to end through the C ABI.

Every round is signed on the device (test_gpu_samemsg._round, test_gpu_build_qc._make_round: rounds
made from the same keys and size share their validator table and the places of their corrupted
votes). What a call must give comes from the C oracle's codes, the model of a multi-round call
(tests/rounds_model.py: one round_model.RoundModel per round, each fed the sub-list of its votes)
and orc.aggregate_sigs of the taken votes of each round's prefix, and -- at the end -- from
ovh_build_qc over the concatenation of each round's votes. Never from ovh_rounds_add itself.

A call of one vote or on one round is ovh_round_add; 2 to 1,024 votes take the small-batch path with
per-vote hashes; more (or OVH_SAMEMSG=2) the same-message plan, whose groups are hashes while the
selection and the sums go by round."""
import ctypes
import random

import numpy as np
import pytest

import bls12_381 as bls
import orc
import rounds_model
import synth_votes as sv
from test_gpu_build_qc import _make_round, _mirror, _oracle_codes, _verify_code, _votes
from test_gpu_rounds import _sum_vote
from test_gpu_samemsg import _cc

pytestmark = pytest.mark.gpu

SENT = 0xA5


@pytest.fixture(scope="module")
def cc():
    import consensus_overlord_amd as coa
    return coa.ConsensusCrypto(bytes.fromhex("7d" * 32))


@pytest.fixture(scope="module")
def cc_plan():
    """every batch on the same-message plan route, at any size"""
    return _cc("7e")


class Rounds:
    """open rounds of one context by key, the model beside them, and every vote added so far"""

    def __init__(self, cc, table, digests):
        self.cc, self.table, self.digests = cc, table, dict(digests)
        cc.update_pubkeys(table)
        self.model = rounds_model.RoundsModel(table)
        self.rd, self.votes, self.taken = {}, {}, {}
        for k, d in self.digests.items():
            self.rd[k] = cc.open_round(d)
            self.model.open(k)
            self.votes[k], self.taken[k] = [], []

    def close(self):
        for r in self.rd.values():
            r.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def prefix_qc(self, k):
        ts = [(s, p) for (s, p), t in zip(self.votes[k], self.taken[k]) if t]
        code, agg = orc.aggregate_sigs([s for s, _ in ts], [p for _, p in ts])
        assert code == 0
        return agg

    def add(self, votes):
        """votes: (key, sig, voter, the oracle's code). One add_rounds call, asked for the QCs; codes,
        taken, count, bitmap and 96 bytes per round against the model and the oracle's aggregate of
        the round's prefix."""
        keys = [v[0] for v in votes]
        code, codes, taken, per_round = self.cc.add_rounds_raw([self.rd[k] for k in keys], [v[1] for v in votes],
                                                               [v[2] for v in votes], want_qc=True)
        m_taken, _, m_per = self.model.add(keys, [v[3] for v in votes], [v[2] for v in votes])
        for (k, s, p, _), t in zip(votes, m_taken):
            self.votes[k].append((s, p))
            self.taken[k].append(t)
        print("call of", len(votes), "return", code, "rounds", [(k, c) for k, _, c in m_per], "got",
              [c for _, c, _, _ in per_round])
        assert code == 0
        assert codes.tolist() == [v[3] for v in votes]
        assert taken.astype(int).tolist() == m_taken
        assert [r for r, _, _, _ in per_round] == [self.rd[k] for k, _, _ in m_per]       # first appearance
        for (_, cnt, agg, bitmap), (k, m_bitmap, m_cnt) in zip(per_round, m_per):
            assert (cnt, bitmap) == (m_cnt, m_bitmap), k
            assert agg == (self.prefix_qc(k) if m_cnt else None), k
        return per_round

    def check_one_shot(self, one_shot=None):
        """the defining property at the end: every round equals ovh_build_qc over its votes"""
        for k, r in self.rd.items():
            if not self.votes[k]:
                continue
            sigs, voters = [s for s, _ in self.votes[k]], [p for _, p in self.votes[k]]
            code, agg, bitmap, _, taken, cnt = one_shot[k] if one_shot else self.cc.build_qc_raw(sigs, self.digests[k], voters)
            assert taken.astype(int).tolist() == self.taken[k], k
            assert r.qc_raw() == (code, agg, bitmap, cnt), k


def _labelled(key, r):
    return [(key, s, p, int(c)) for s, p, c in zip(r["sigs"], r["voters"], r["want"])]


def _prepare(cc, golden, lo, n, tag, table=None):
    digest = sv.sha(tag)
    sigs, voters, tb = _make_round(cc.ctx, golden, lo, n, digest)
    want = _oracle_codes(sigs, digest, voters)
    table = table or tb
    cc.update_pubkeys(table)
    one_shot = cc.build_qc_raw(sigs, digest, voters)
    assert one_shot[3].tolist() == want.tolist()
    return {"digest": digest, "sigs": sigs, "voters": voters, "table": table, "want": want, "one_shot": one_shot}


def _cut(cc, rounds, order, cut):
    """rounds: key -> _prepare(); order: the labelled votes of one flush sequence; added in calls of
    the sizes in cut"""
    assert sum(cut) == len(order)
    table = next(iter(rounds.values()))["table"]
    with Rounds(cc, table, {k: r["digest"] for k, r in rounds.items()}) as R:
        lo = 0
        for k in cut:
            R.add(order[lo:lo + k])
            lo += k
        R.check_one_shot({k: r["one_shot"] for k, r in rounds.items()})


# ------------------------------------------------------------------- two rounds, whole and in cuts
@pytest.fixture(scope="module")
def pair67(cc, golden):
    a = _prepare(cc, golden, 140000, 67, b"rounds add 67 a")
    b = _prepare(cc, golden, 140000, 67, b"rounds add 67 b")
    assert a["table"] == b["table"] and a["voters"] == b["voters"]
    assert sorted(set(a["want"].tolist())) == [0, 3, 5, 102] == sorted(set(b["want"].tolist()))
    A, B = _labelled("a", a), _labelled("b", b)
    # vote by vote: a b a b a b a | b b b a b b b b (one vote of a beside seven of b) | alternating
    order = [A[0], B[0], A[1], B[1], A[2], B[2], A[3]] + B[3:6] + [A[4]] + B[6:10]
    ia, ib = 5, 10
    while ia < 67 or ib < 67:
        if ia < 67:
            order.append(A[ia])
            ia += 1
        if ib < 67:
            order.append(B[ib])
            ib += 1
    assert len(order) == 134
    return {"a": a, "b": b}, order


@pytest.mark.parametrize("cut", [(134,), (1, 1, 2, 3, 127), (1, 1, 2, 3, 8, 119)], ids=lambda c: "-".join(map(str, c)))
def test_two_corrupted_rounds_whole_and_in_cuts(cc, pair67, cut):
    rounds, order = pair67
    if len(cut) == 6:
        assert [v[0] for v in order[7:15]].count("a") == 1
    _cut(cc, rounds, order, cut)


def test_pairs_split_over_calls_and_an_equivocating_voter(cc):
    """the invalid-then-valid pair and the duplicate pair of one voter split over two calls; a voter
    with valid votes in both rounds is taken in both"""
    da, db = sv.sha(b"rounds add pairs a"), sv.sha(b"rounds add pairs b")
    va, vb = _votes(cc.ctx, 141000, 5, da), _votes(cc.ctx, 141000, 5, db)
    table = [p for _, p in va]
    assert table == [p for _, p in vb]
    bad2 = (sv.add_g2(va[2][0]), va[2][1])
    first = [("a", bad2), ("b", vb[1]), ("a", va[3]), ("b", vb[3]), ("a", va[0])]
    second = [("a", va[2]), ("b", vb[1]), ("a", va[3]), ("b", vb[4]), ("b", vb[3])]

    def lab(xs):
        return [(k, s, p, orc.verify(s, da if k == "a" else db, p)) for k, (s, p) in xs]
    with Rounds(cc, table, {"a": da, "b": db}) as R:
        R.add(lab(first))
        assert R.taken == {"a": [0, 1, 1], "b": [1, 1]}               # voter 3 in both rounds
        R.add(lab(second))
        assert R.taken == {"a": [0, 1, 1, 1, 0], "b": [1, 1, 0, 1, 0]}
        R.check_one_shot()


# ------------------------------------------------------------------- three rounds, 131 votes
@pytest.fixture(scope="module")
def three131(cc, golden):
    a = _prepare(cc, golden, 142000, 65, b"rounds add 131 a")
    rounds = {"a": a}
    for k in ("b", "c"):
        rounds[k] = _prepare(cc, golden, 142000, 33, b"rounds add 131 " + k.encode(), table=a["table"])
    # a seeded interleaving that keeps every round's own order (the one-shot reference's order)
    left = {k: _labelled(k, r) for k, r in rounds.items()}
    rng, order = random.Random(131), []
    while any(left.values()):
        k = rng.choice([k for k, vs in left.items() for _ in vs])
        order.append(left[k].pop(0))
    return rounds, order


def test_three_rounds_131_votes_one_round_of_65(cc, three131):
    """one call: the round of 65 votes runs the upper level of the sum beside two one-chunk rounds"""
    rounds, order = three131
    assert len(order) == 131
    _cut(cc, rounds, order, (131,))


# ------------------------------------------------------------------- 1,030 votes over two rounds
@pytest.fixture(scope="module")
def pair1030(cc, golden):
    a = _prepare(cc, golden, 143000, 515, b"rounds add 1030 a")
    b = _prepare(cc, golden, 143000, 515, b"rounds add 1030 b")
    order = [v for pair in zip(_labelled("a", a), _labelled("b", b)) for v in pair]
    return {"a": a, "b": b}, order


@pytest.mark.parametrize("cut", [(1026, 4), (4, 1026)], ids=lambda c: "-".join(map(str, c)))
def test_1030_votes_over_two_rounds_take_the_plan_route(cc, pair1030, cut):
    rounds, order = pair1030
    before = cc.samemsg_stats()[0]
    _cut(cc, rounds, order, cut)
    # the 1,026-vote call and nothing else of the cut (the two one-shot ovh_build_qc were made before)
    assert cc.samemsg_stats()[0] == before + 1


# ------------------------------------------------------------------- 16 rounds
def _raw(cc, ids, sigs, voters, max_rounds=16, bl=None, want_out=True, n=None):
    """ovh_rounds_add itself over sentinel-filled outputs -> (return code, dict of the outputs)"""
    n = len(sigs) if n is None else n
    bl = (len(cc.pubkeys) + 7) // 8 if bl is None else bl
    m = max(n, 1)
    o = {"codes": np.full(m, -7, dtype=np.int32), "taken": np.full(m, SENT, dtype=np.uint8),
         "slot": np.full(m, 0xA5A5A5A5, dtype=np.uint32), "rid": np.full(16, 0xA5A5, dtype=np.uint64),
         "cnt": np.full(16, 0xA5A5, dtype=np.uint32), "out": np.full((16, 96), SENT, dtype=np.uint8),
         "bm": np.full((16, max(bl, 1)), SENT, dtype=np.uint8)}
    nr = ctypes.c_uint32(0xA5A5)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    idv = np.array(list(ids) or [0], dtype=np.uint64)
    r = cc.lib.ovh_rounds_add(cc.ctx.ptr, n, b"".join(sigs), p(idv), b"".join(voters), p(o["codes"]), p(o["taken"]),
                              p(o["slot"]), max_rounds, ctypes.byref(nr), p(o["rid"]), p(o["cnt"]),
                              p(o["out"]) if want_out else None, p(o["bm"]), bl)
    o["nr"] = nr.value
    return r, o


def _untouched(o):
    return ((o["codes"] == -7).all() and (o["taken"] == SENT).all() and (o["slot"] == 0xA5A5A5A5).all()
            and (o["rid"] == 0xA5A5).all() and (o["cnt"] == 0xA5A5).all() and (o["out"] == SENT).all()
            and (o["bm"] == SENT).all() and o["nr"] == 0xA5A5)


def test_16_rounds_one_vote_each_then_half_of_them_only_invalid_votes(cc):
    digests = [sv.sha(b"rounds add 16 %d" % k) for k in range(16)]
    votes = [_votes(cc.ctx, 144000, 3, d) for d in digests]
    table = [p for _, p in votes[0]]
    cc.update_pubkeys(table)
    rds = [cc.open_round(d) for d in digests]
    try:
        # call 1: validator k % 3 votes in round k; round 15's vote is invalid (an empty round)
        first = [votes[k][k % 3] for k in range(16)]
        first[15] = (sv.add_g2(first[15][0]), first[15][1])
        r, o = _raw(cc, [x.id for x in rds], [s for s, _ in first], [p for _, p in first])
        assert r == 0 and o["nr"] == 16 and o["rid"].tolist() == [x.id for x in rds]
        assert o["slot"].tolist() == list(range(16)) and o["codes"].tolist() == [0] * 15 + [5]
        assert o["taken"].tolist() == [1] * 15 + [0] and o["cnt"].tolist() == [1] * 15 + [0]
        rank = sorted(table)
        for k in range(15):
            assert o["out"][k].tobytes() == first[k][0]                         # one signature: the sum is it
            assert o["bm"][k].tobytes() == bytes([0x80 >> rank.index(first[k][1])])
        assert (o["out"][15] == SENT).all() and o["bm"][15].tobytes() == bytes(1)  # reports 0, its slot untouched
        assert rds[15].qc_raw() == (4, None, bytes(1), 0)
        before = [x.qc_raw() for x in rds]
        # call 2, rounds in reverse order: rounds 0..7 get an invalid vote each (their R must not
        # move), rounds 8..15 a valid vote of the next validator
        second, ids = [], []
        for k in reversed(range(16)):
            s, p = votes[k][(k + 1) % 3]
            second.append((sv.add_g2(s), p) if k < 8 else (s, p))
            ids.append(rds[k].id)
        r, o = _raw(cc, ids, [s for s, _ in second], [p for _, p in second])
        assert r == 0 and o["nr"] == 16 and o["rid"].tolist() == ids
        assert o["codes"].tolist() == [0] * 8 + [5] * 8 and o["taken"].tolist() == [1] * 8 + [0] * 8
        assert o["cnt"].tolist() == [1] + [2] * 7 + [1] * 8
        for k in range(8):
            assert rds[k].qc_raw() == before[k]
            assert o["out"][15 - k].tobytes() == before[k][1] and o["bm"][15 - k].tobytes() == before[k][2]
        for k in range(8, 16):
            sigs = ([] if k == 15 else [first[k][0]]) + [votes[k][(k + 1) % 3][0]]
            pks = ([] if k == 15 else [first[k][1]]) + [votes[k][(k + 1) % 3][1]]
            assert (0, o["out"][15 - k].tobytes()) == orc.aggregate_sigs(sigs, pks)
            assert rds[k].qc_raw()[1] == o["out"][15 - k].tobytes()
    finally:
        for x in rds:
            x.close()


# ------------------------------------------------------------------- two rounds on one hash
@pytest.mark.parametrize("route", ["small", "plan"])
def test_two_rounds_opened_on_the_same_hash_fill_independently(cc, cc_plan, route):
    c = cc if route == "small" else cc_plan
    d, e = sv.sha(b"rounds add same hash"), sv.sha(b"rounds add same hash, another")
    v, w = _votes(c.ctx, 145000, 6, d), _votes(c.ctx, 145000, 6, e)
    table = [p for _, p in v]
    before = c.samemsg_stats()[0]
    with Rounds(c, table, {"x": d, "y": d, "z": e}) as R:
        assert R.rd["x"].id != R.rd["y"].id
        order = [("x", v[0]), ("y", v[0]), ("z", w[0]), ("y", v[1]), ("x", v[2]), ("y", v[0]), ("z", w[2]), ("y", v[3])]
        R.add([(k, s, p, 0) for k, (s, p) in order])
        assert R.taken == {"x": [1, 1], "y": [1, 1, 0, 1], "z": [1, 1]}
        R.add([("y", v[2][0], v[2][1], 0), ("x", v[3][0], v[3][1], 0), ("x", v[0][0], v[0][1], 0)])
        assert R.taken["x"] == [1, 1, 1, 0] and R.taken["y"] == [1, 1, 0, 1, 1]
        R.check_one_shot()
    if route == "plan":
        assert c.samemsg_stats()[0] >= before + 2


# ------------------------------------------------------------------- mirror and sum votes
def test_a_call_sum_cancels_r_then_a_third_vote_and_a_call_sum_doubles_r(cc):
    da, db = sv.sha(b"rounds add mirror a"), sv.sha(b"rounds add mirror b")
    va, vb = _votes(cc.ctx, 146000, 4, da), _votes(cc.ctx, 146000, 4, db)
    m = _mirror(*va[0])
    c = _sum_vote(va[1], va[2])
    assert orc.verify(m[0], da, m[1]) == 0 and orc.verify(c[0], da, c[1]) == 0
    table = [p for _, p in va] + [m[1], c[1]]
    inf = bls.g2_compress(None)
    with Rounds(cc, table, {"a": da, "b": db}) as R:
        R.add([("a", va[0][0], va[0][1], 0), ("b", vb[0][0], vb[0][1], 0)])
        per = R.add([("b", vb[1][0], vb[1][1], 0), ("a", m[0], m[1], 0)])
        assert per[1][1:3] == (2, inf)                       # two votes taken, R the identity again
        per = R.add([("a", va[3][0], va[3][1], 0), ("b", vb[2][0], vb[2][1], 0)])
        assert per[0][1:3] == (3, va[3][0])                  # the third vote is the whole sum
        R.check_one_shot()
    with Rounds(cc, table, {"a": da, "b": db}) as R:
        R.add([("a", va[1][0], va[1][1], 0), ("b", vb[0][0], vb[0][1], 0), ("a", va[2][0], va[2][1], 0)])
        per = R.add([("a", c[0], c[1], 0), ("b", vb[3][0], vb[3][1], 0)])      # the call's sum equals R
        want = orc.aggregate_sigs([va[1][0], va[2][0], c[0]], [va[1][1], va[2][1], c[1]])[1]
        assert per[0][1:3] == (3, want) and want != inf
        R.check_one_shot()


# ------------------------------------------------------------------- interleaving and refusals
def test_round_add_build_qc_and_build_qcs_between_the_calls_disturb_nothing(cc, three131):
    rounds, order = three131
    a, b = rounds["a"], rounds["b"]
    with Rounds(cc, a["table"], {k: r["digest"] for k, r in rounds.items()}) as R:
        lo = 0
        for step, k in enumerate((9, 40, 2, 79)):
            R.add(order[lo:lo + k])
            lo += k
            assert cc.build_qc_raw(a["sigs"][:5], a["digest"], a["voters"][:5])[0] in (0, 4)
            qcs = cc.build_qcs(a["sigs"][:3] + b["sigs"][:3], [a["digest"]] * 3 + [b["digest"]] * 3,
                               a["voters"][:3] + b["voters"][:3])[0]
            assert len(qcs) == 2
            if step == 1:        # one ovh_round_add in between, of a vote the round has not seen
                key, s, p, w = order[lo]
                codes, taken, cnt = R.rd[key].add([s], [p])
                m_taken, m_bitmap, m_cnt = R.model.rounds[key].add([w], [p])
                R.votes[key].append((s, p))
                R.taken[key].append(m_taken[0])
                assert (codes.tolist(), taken.astype(int).tolist(), cnt) == ([w], m_taken, m_cnt)
                lo += 1
        assert lo == 131
        R.check_one_shot({k: r["one_shot"] for k, r in rounds.items()})


def test_refused_calls_change_nothing(cc, three131):
    rounds, order = three131
    bl = (len(rounds["a"]["table"]) + 7) // 8
    with Rounds(cc, rounds["a"]["table"], {k: r["digest"] for k, r in rounds.items()}) as R:
        R.add(order[:50])
        nxt = order[50:60]
        ids = [R.rd[v[0]].id for v in nxt]
        sigs, voters = [v[1] for v in nxt], [v[2] for v in nxt]
        assert len(set(ids)) == 3
        closed = cc.open_round(sv.sha(b"rounds add closed"))
        stale = closed.id
        closed.close()
        for kw in (dict(ids=ids[:4] + [0x7FFFFFFFFFFF] + ids[5:]),          # one unknown id among valid ones
                   dict(ids=ids[:9] + [stale]),                              # a closed id
                   dict(max_rounds=2),                                       # three distinct ids
                   dict(max_rounds=0),
                   dict(n=0),
                   dict(bl=bl - 1), dict(bl=bl + 1)):
            a = dict(dict(ids=ids, max_rounds=16, bl=None, n=None), **kw)
            r, o = _raw(cc, a["ids"], sigs, voters, max_rounds=a["max_rounds"], bl=a["bl"], n=a["n"])
            assert r == 103 and _untouched(o), sorted(kw)
        # the next valid calls behave as if the refused ones had never been made
        R.add(order[50:60])
        R.add(order[60:])
        R.check_one_shot({k: r["one_shot"] for k, r in rounds.items()})


# ------------------------------------------------------------------- the verdict cache
def test_the_adds_fill_the_verdict_cache(cc, three131):
    rounds, order = three131
    assert cc.lib.ovh_cache_config(cc.ctx.ptr, 0) == 0          # forget what the tests above entered
    assert cc.lib.ovh_cache_config(cc.ctx.ptr, 1 << 16) == 0
    with Rounds(cc, rounds["a"]["table"], {k: r["digest"] for k, r in rounds.items()}) as R:
        assert cc.cache_stats()[2] == 0
        R.cc.add_rounds([R.rd[v[0]] for v in order[:20]], [v[1] for v in order[:20]], [v[2] for v in order[:20]])
        R.cc.add_rounds([R.rd[v[0]] for v in order[20:]], [v[1] for v in order[20:]], [v[2] for v in order[20:]])
        h0, m0, entries = cc.cache_stats()
        assert entries == len({(v[0], v[1], v[2]) for v in order})
        for key, s, p, w in order:
            assert _verify_code(cc, s, R.digests[key], p) == w
        h1, m1, _ = cc.cache_stats()
        assert h1 - h0 == len(order) and m1 == m0


# ------------------------------------------------------------------- one vote, one round
def test_single_vote_and_single_round_calls_equal_round_add(cc, pair67):
    """two rounds on one hash: one filled by ovh_round_add, its twin by ovh_rounds_add calls that name
    one round only -- the same codes, taken, count, bitmap and bytes after every call"""
    rounds, _ = pair67
    a = rounds["a"]
    cc.update_pubkeys(a["table"])
    bl = (len(a["table"]) + 7) // 8
    with cc.open_round(a["digest"]) as r1, cc.open_round(a["digest"]) as r2:
        lo = 0
        for k in (1, 5, 1, 60):
            sigs, voters = a["sigs"][lo:lo + k], a["voters"][lo:lo + k]
            lo += k
            code, codes, taken, cnt, agg, bitmap = r1.add_raw(sigs, voters, want_qc=True)
            r, o = _raw(cc, [r2.id] * k, sigs, voters)
            assert (r, o["nr"], o["rid"][0]) == (0, 1, r2.id) and code == 0
            assert o["slot"].tolist() == [0] * k and (o["rid"][1:] == 0xA5A5).all() and (o["cnt"][1:] == 0xA5A5).all()
            assert o["codes"].tolist() == codes.tolist() and o["taken"].astype(bool).tolist() == taken.tolist()
            assert o["cnt"][0] == cnt and o["bm"][0, :bl].tobytes() == bitmap
            assert (o["out"][0].tobytes() if cnt else None) == agg
            assert (o["out"][1:] == SENT).all() and (o["bm"][1:] == SENT).all()
        assert lo == 67 and r1.qc() == r2.qc() == (a["one_shot"][1], a["one_shot"][2], a["one_shot"][5])
