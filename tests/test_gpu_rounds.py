"""Rounds on the GPU (ovh_round_open / _add / _qc / _close): a round's votes
added in pieces against the one-shot ovh_build_qc over the whole list.

Every round is signed on the device (test_gpu_samemsg._round, test_gpu_build_qc._make_round). What
an add must give comes from the C oracle's codes, the round model (tests/round_model.py) and
orc.aggregate_sigs of the taken votes of the prefix, and from ovh_build_qc on the concatenation --
never from the round API itself. An add takes one of three routes: one vote the per-call path, 2 to
1,024 votes the small-batch path (sigma from one sigchk launch), more the same-message route. The
cuts put an add of one vote before, between and behind larger ones, cross the 64-vote chunk inside an
add (65 of 131 votes: the upper levels run), split the duplicate and the invalid-then-valid pairs of
the corrupted round over two adds, and -- in the 1,030-vote round -- put an add on the same-message
route before and behind a small one. The corrupted rounds hold a voter outside the table, so their
adds stage table-first and run as two parts."""
import ctypes

import numpy as np
import pytest

import bls12_381 as bls
import orc
import qc_model
import round_model
import synth_votes as sv
from test_gpu_build_qc import _make_round, _mirror, _oracle_codes, _verify_code, _votes
from test_gpu_samemsg import _round

pytestmark = pytest.mark.gpu

SENTINEL = b"\xa5" * 96


@pytest.fixture(scope="module")
def cc():
    import consensus_overlord_amd as coa
    return coa.ConsensusCrypto(bytes.fromhex("7c" * 32))


def _prepare(cc, golden, lo, n, tag):
    """a corrupted round, the oracle's codes and ovh_build_qc's outputs over the whole list (computed
    once per module and left unchanged)"""
    digest = sv.sha(tag)
    sigs, voters, table = _make_round(cc.ctx, golden, lo, n, digest)
    want = _oracle_codes(sigs, digest, voters)
    cc.update_pubkeys(table)
    one_shot = cc.build_qc_raw(sigs, digest, voters)
    assert one_shot[3].tolist() == want.tolist()
    return {"digest": digest, "sigs": sigs, "voters": voters, "table": table, "want": want, "one_shot": one_shot}


@pytest.fixture(scope="module")
def round67(cc, golden):
    r = _prepare(cc, golden, 120000, 67, b"rounds 67")
    assert sorted(set(r["want"].tolist())) == [0, 3, 5, 102]
    return r


@pytest.fixture(scope="module")
def round131(cc, golden):
    return _prepare(cc, golden, 121000, 131, b"rounds 131")


@pytest.fixture(scope="module")
def round1030(cc, golden):
    return _prepare(cc, golden, 127000, 1030, b"rounds 1030")


def _prefix_qc(sigs, voters, taken):
    ts = [s for s, t in zip(sigs, taken) if t]
    tv = [p for p, t in zip(voters, taken) if t]
    code, agg = orc.aggregate_sigs(ts, tv)
    assert code == 0
    return agg


def _add_in_pieces(cc, rd, sigs, voters, table, want, cut, model=None, taken_all=None, lo=0):
    """adds sigs[lo:] in pieces of `cut`, asking for the QC on every add; after each the count, the
    bitmap and the 96 bytes equal the model and the oracle's aggregate of the prefix"""
    model = model or round_model.RoundModel(table)
    taken_all = [] if taken_all is None else taken_all
    codes_all = []
    for k in cut:
        code, codes, taken, cnt, agg, bitmap = rd.add_raw(sigs[lo:lo + k], voters[lo:lo + k], want_qc=True)
        m_taken, m_bitmap, m_cnt = model.add(want[lo:lo + k], voters[lo:lo + k])
        lo += k
        taken_all += m_taken
        codes_all += codes.tolist()
        print("add", k, "return", code, "n_signed", cnt, "model", m_cnt)
        assert code == 0
        assert codes.tolist() == list(want[lo - k:lo])
        assert taken.astype(int).tolist() == m_taken
        assert cnt == m_cnt and bitmap == m_bitmap
        assert agg == (_prefix_qc(sigs[:lo], voters[:lo], taken_all) if m_cnt else None)
    return model, taken_all, lo


def _check_cut(cc, r, cut):
    cc.update_pubkeys(r["table"])
    sigs, voters, table, want = r["sigs"], r["voters"], r["table"], r["want"].tolist()
    code1, agg1, bitmap1, codes1, taken1, cnt1 = r["one_shot"]
    with cc.open_round(r["digest"]) as rd:
        _, taken_all, lo = _add_in_pieces(cc, rd, sigs, voters, table, want, cut)
        assert lo == len(sigs)
        # the defining property: everything equals ovh_build_qc over the concatenation
        assert taken_all == taken1.astype(int).tolist() == qc_model.select(want, voters, table)[0]
        assert rd.qc() == (agg1, bitmap1, cnt1) and code1 == 0


@pytest.mark.parametrize("cut", [(67,), (1, 1, 2, 3, 60), (64, 3), (3, 64), (65, 2)], ids=lambda c: "-".join(map(str, c)))
def test_cut_invariance_67(cc, round67, cut):
    _check_cut(cc, round67, cut)


@pytest.mark.parametrize("cut", [(65, 1, 65), (131,)], ids=lambda c: "-".join(map(str, c)))
def test_cut_invariance_131(cc, round131, cut):
    _check_cut(cc, round131, cut)


@pytest.mark.parametrize("cut", [(1026, 4), (4, 1026)], ids=lambda c: "-".join(map(str, c)))
def test_cut_invariance_1030_same_message_route(cc, round1030, cut):
    before = cc.samemsg_stats()[0]
    _check_cut(cc, round1030, cut)
    assert cc.samemsg_stats()[0] == before + 1          # the 1,026-vote add, and only it


def test_trickle_one_vote_at_a_time(cc):
    """5 validators, one vote per add; a duplicate and an invalid single among them move nothing"""
    digest = sv.sha(b"rounds trickle")
    v = _votes(cc.ctx, 122000, 5, digest)
    table = [p for _, p in v]
    votes = [v[0], v[1], v[1], (sv.add_g2(v[2][0]), v[2][1]), v[3], v[2], v[4], v[0]]
    sigs, voters = [s for s, _ in votes], [p for _, p in votes]
    want = _oracle_codes(sigs, digest, voters).tolist()
    assert want == [0, 0, 0, 5, 0, 0, 0, 0]
    cc.update_pubkeys(table)
    with cc.open_round(digest) as rd:
        before = None
        model, taken_all, lo = None, None, 0
        for i in range(len(votes)):
            model, taken_all, lo = _add_in_pieces(cc, rd, sigs, voters, table, want, (1,), model, taken_all, lo)
            now = rd.qc()
            if i in (2, 3, 7):                     # the duplicates and the invalid vote: R did not move
                assert now == before and taken_all[i] == 0
            before = now
        assert taken_all == [1, 1, 0, 0, 1, 1, 1, 0]
        code, agg, bitmap, _, taken, cnt = cc.build_qc_raw(sigs, digest, voters)
        assert code == 0 and rd.qc() == (agg, bitmap, cnt) and cnt == 5 and bitmap == bytes([0xF8])


def _sum_vote(a, b):
    """(sigma_a + sigma_b, pk_a + pk_b): the valid vote of the validator with secret sk_a + sk_b"""
    sig = bls.pt_add(bls.Fp2Ops, bls.g2_from_bytes(a[0]), bls.g2_from_bytes(b[0]))
    pk = bls.pt_add(bls.FpOps, bls.g1_from_bytes(a[1]), bls.g1_from_bytes(b[1]))
    return bls.g2_compress(sig), bls.g1_compress(pk)


def _related(cc, digest, pieces):
    """pieces of valid votes of distinct validators, one add each -> the QC bytes after each add"""
    votes = [x for p in pieces for x in p]
    sigs, voters = [s for s, _ in votes], [p for _, p in votes]
    want = _oracle_codes(sigs, digest, voters).tolist()
    assert not any(want) and len(set(voters)) == len(voters)
    cc.update_pubkeys(voters)
    out = []
    with cc.open_round(digest) as rd:
        model, taken_all, lo = None, None, 0
        for p in pieces:
            model, taken_all, lo = _add_in_pieces(cc, rd, sigs, voters, voters, want, (len(p),), model, taken_all, lo)
            out.append(rd.qc()[0])
        code, agg, bitmap, _, _, cnt = cc.build_qc_raw(sigs, digest, voters)
        assert code == 0 and rd.qc() == (agg, bitmap, cnt) and cnt == len(votes)
    return out


def test_mirror_across_the_merge_cancels_then_a_third_vote(cc):
    """a validator, then its mirror (sk and r - sk) in the next add: R is the identity with two votes
    taken, the QC bytes are the infinity encoding; a third validator's vote then is the whole sum"""
    digest = sv.sha(b"rounds mirror")
    v, w = _votes(cc.ctx, 123000, 2, digest)
    m = _mirror(*v)
    assert orc.verify(m[0], digest, m[1]) == 0
    inf = bls.g2_compress(None)
    for first, second in ((v, m), (m, v)):
        qcs = _related(cc, digest, [[first], [second], [w]])
        assert qcs == [first[0], inf, w[0]]
    # the same across adds of more than one vote: {v, w} then {mirror of v, mirror of w}
    assert _related(cc, digest, [[v, w], [m, _mirror(*w)]])[1] == inf


def test_merge_of_two_equal_sums_doubles(cc):
    """{A, B} then C with sk_C = sk_A + sk_B: the add's sum equals R"""
    digest = sv.sha(b"rounds doubling")
    a, b = _votes(cc.ctx, 123100, 2, digest)
    c = _sum_vote(a, b)
    assert orc.verify(c[0], digest, c[1]) == 0
    want = orc.aggregate_sigs([a[0], b[0], c[0]], [a[1], b[1], c[1]])[1]
    assert _related(cc, digest, [[a, b], [c]])[1] == want
    assert _related(cc, digest, [[c], [a, b]])[1] == want
    assert want != bls.g2_compress(None)


def _add_c(cc, rid, sigs, voters, bl, out=None, bitmap=None):
    """ovh_round_add itself -> (return code, codes, n_signed)"""
    n = len(sigs)
    codes = np.full(max(n, 1), -7, dtype=np.int32)
    cnt = ctypes.c_uint32(0xFFFF)
    r = cc.lib.ovh_round_add(cc.ctx.ptr, rid, n, b"".join(sigs), b"".join(voters), codes.ctypes.data_as(ctypes.c_void_p),
                             None, ctypes.byref(cnt), out, bitmap, bl)
    return r, codes[:n].tolist(), cnt.value


def test_empty_round_and_an_add_of_only_invalid_votes(cc, golden):
    digest = sv.sha(b"rounds empty")
    v = _votes(cc.ctx, 124000, 3, digest)
    table = [p for _, p in v]
    cc.update_pubkeys(table)
    with cc.open_round(digest) as rd:
        assert rd.qc_raw() == (4, None, bytes(1), 0)
        out = ctypes.create_string_buffer(SENTINEL, 96)
        bm = ctypes.create_string_buffer(b"\xff", 1)
        cnt = ctypes.c_uint32(9)
        assert cc.lib.ovh_round_qc(cc.ctx.ptr, rd.id, out, bm, 1, ctypes.byref(cnt)) == 4
        assert out.raw == SENTINEL and bm.raw == bytes(1) and cnt.value == 0
        bad = [sv.add_g2(s) for s, _ in v]
        for sigs, voters in ((bad, table), (bad[:1], table[:1])):      # the batch route and the per-call one
            out = ctypes.create_string_buffer(SENTINEL, 96)
            bm = ctypes.create_string_buffer(b"\xff", 1)
            r, codes, n_signed = _add_c(cc, rd.id, sigs, voters, 1, out, bm)
            assert (r, codes, n_signed) == (0, [5] * len(sigs), 0)
            assert out.raw == SENTINEL and bm.raw == bytes(1)
        assert rd.qc_raw() == (4, None, bytes(1), 0)
        # the round still works: the invalid votes blocked nobody
        codes, taken, n_signed, agg, bitmap = rd.add([s for s, _ in v], table, want_qc=True)
        assert codes.tolist() == [0, 0, 0] and taken.all() and n_signed == 3
        assert (0, agg) == orc.aggregate_sigs([s for s, _ in v], table) and bitmap == bytes([0xE0])


def test_two_rounds_and_build_qc_in_between_do_not_disturb_each_other(cc):
    from consensus_overlord_amd import vote
    bh = sv.sha(b"rounds block")
    hp = vote.vote_hash(cc, 7, 0, vote.PREVOTE, bh)
    hc = vote.vote_hash(cc, 7, 0, vote.PRECOMMIT, bh)
    n = 9
    sp, pk = _round(cc.ctx, 125000, n, hp)
    sc, pk2 = _round(cc.ctx, 125000, n, hc)
    table = [bytes(p) for p in pk]
    assert table == [bytes(p) for p in pk2]
    sp, sc = [bytes(s) for s in sp], [bytes(s) for s in sc]
    sp[2] = sv.add_g2(sp[2])
    cc.update_pubkeys(table)
    one_p = cc.build_qc_raw(sp, hp, table)
    one_c = cc.build_qc_raw(sc, hc, table)
    with cc.open_round(hp) as rp, cc.open_round(hc) as rc:
        assert rp.id != rc.id and rp.id and rc.id
        for lo, hi in ((0, 1), (1, 5), (5, 9)):
            assert rp.add(sp[lo:hi], table[lo:hi])[0].tolist() == one_p[3][lo:hi].tolist()
            assert cc.build_qc_raw(sc[:4], hc, table[:4])[5] == 4      # the table's own scratch, between adds
            assert rc.add(sc[lo:hi], table[lo:hi])[2] == hi
            assert cc.build_qcs(sp[:3] + sc[:3], [hp] * 3 + [hc] * 3, table[:3] * 2)[0][0][3] == 2
        assert rp.qc() == (one_p[1], one_p[2], one_p[5]) and one_p[5] == n - 1
        assert rc.qc() == (one_c[1], one_c[2], one_c[5]) and one_c[5] == n


def test_lifecycle_and_refused_calls(cc):
    digest = sv.sha(b"rounds lifecycle")
    v = _votes(cc.ctx, 126000, 13, digest)
    sigs, table = [s for s, _ in v], [p for _, p in v]
    cc.update_pubkeys(table)
    lib, ptr = cc.lib, cc.ctx.ptr
    rid = ctypes.c_uint64(0)
    assert lib.ovh_round_open(ptr, digest, 31, ctypes.byref(rid)) == 100 and rid.value == 0
    # a wrong bitmap_len is refused and changes nothing: the next add gives what it would have given
    rd = cc.open_round(digest)
    assert rd.add(sigs[:5], table[:5])[2] == 5
    for bl in (1, 3):
        bm = ctypes.create_string_buffer(b"\xee" * 4, 4)
        r, codes, n_signed = _add_c(cc, rd.id, sigs[5:9], table[5:9], bl, None, bm)
        assert (r, codes, n_signed) == (103, [-7] * 4, 0xFFFF) and bm.raw == b"\xee" * 4
    assert _add_c(cc, rd.id, [], [], 2)[0] == 103                       # n == 0
    codes, taken, n_signed, agg, bitmap = rd.add(sigs[5:], table[5:], want_qc=True)
    one = cc.build_qc_raw(sigs, digest, table)
    assert taken.all() and (agg, bitmap, n_signed) == (one[1], one[2], one[5]) and n_signed == 13
    # an id is stale after close, and is never handed out again
    old = rd.id
    rd.close()
    assert _add_c(cc, old, sigs[:1], table[:1], 2)[0] == 103
    out, bm, cnt = ctypes.create_string_buffer(96), ctypes.create_string_buffer(2), ctypes.c_uint32(0)
    assert lib.ovh_round_qc(ptr, old, out, bm, 2, ctypes.byref(cnt)) == 103
    assert lib.ovh_round_close(ptr, old) == 103 and lib.ovh_round_close(ptr, 0) == 103
    # the 17th open is refused; after a close there is room again
    rounds = [cc.open_round(sv.sha(b"rounds lifecycle %d" % k)) for k in range(cc.ROUNDS_MAX)]
    assert len({r.id for r in rounds}) == cc.ROUNDS_MAX and old not in {r.id for r in rounds}
    with pytest.raises(ValueError):
        cc.open_round(digest)
    rounds[3].close()
    extra = cc.open_round(digest)
    assert extra.add(sigs[:2], table[:2])[2] == 2
    # update_pubkeys closes every open round
    ids = [r.id for r in rounds if r.id is not None] + [extra.id]
    cc.update_pubkeys(table)
    for i in ids:
        assert _add_c(cc, i, sigs[:1], table[:1], 2)[0] == 103
    with pytest.raises(ValueError):
        extra.qc()
    fresh = cc.open_round(digest)
    assert fresh.id not in ids and fresh.add(sigs[:1], table[:1])[2] == 1
    fresh.close()
    for r in rounds + [extra]:
        r.close()                                                       # closing a stale round is no error


def test_adds_fill_the_verdict_cache(cc, round67):
    r = round67
    cc.update_pubkeys(r["table"])
    sigs, voters, want = r["sigs"], r["voters"], r["want"].tolist()
    assert cc.lib.ovh_cache_config(cc.ctx.ptr, 0) == 0          # forget what the tests above entered
    assert cc.lib.ovh_cache_config(cc.ctx.ptr, 1 << 16) == 0 and cc.cache_stats()[2] == 0
    with cc.open_round(r["digest"]) as rd:
        rd.add(sigs[:1], voters[:1])
        rd.add(sigs[1:], voters[1:])
        h0, m0, entries = cc.cache_stats()
        assert entries == len(set(zip(sigs, voters)))
        for i in range(len(sigs)):
            assert _verify_code(cc, sigs[i], r["digest"], voters[i]) == want[i], i
        h1, m1, _ = cc.cache_stats()
        assert h1 - h0 == len(sigs) and m1 == m0
