"""The signature-point cache on the GPU: every fill site, then
ovh_aggregate_sigs on the cache route against the C oracle's bytes.

All inputs are made on the CPU (tests/agg_cases.py: the C oracle signs), so the library is compared
with bytes it had no part in; expected bytes come from orc.aggregate_sigs, never from the library's
other route. Every test asserts the ovh_agg_stats counters of the route it means to exercise, so
none can pass on the full path (or the other way round for the miss cases).

The calls that fill mix table voters with voters outside the table (agg_cases.interleaved), so the
batch stages its votes in another order than the caller's; aggregating each signature alone
(aggregate([sigma]) == sigma) then shows whether an entry holds the point of the bytes it is
registered under. Counts 64, 65 and 129 cross the masked sum's chunk (one chunk, two, three with
an upper level)."""
import os

import pytest

import agg_cases as ac
import orc

pytestmark = pytest.mark.gpu

REG, ENT, ROUTE, OLD, MISS = 0, 1, 2, 3, 4


def _new_cc(samemsg=None):
    import consensus_overlord_amd as coa
    from consensus_overlord_amd.crypto import FLAG_SK_RAW, Context
    old = os.environ.get("OVH_SAMEMSG")
    if samemsg is not None:
        os.environ["OVH_SAMEMSG"] = samemsg
    try:
        return coa.ConsensusCrypto(ac.validators(ac.TABLE_N)[0][0], ctx=Context(flags=FLAG_SK_RAW))
    finally:
        if samemsg is not None:
            if old is None:
                del os.environ["OVH_SAMEMSG"]
            else:
                os.environ["OVH_SAMEMSG"] = old


@pytest.fixture(scope="module")
def cc():
    c = _new_cc()
    assert c.name == ac.validators(ac.TABLE_N)[0][1]
    return c


def _delta(cc, fn):
    s0 = cc.agg_stats()
    out = fn()
    s1 = cc.agg_stats()
    return out, [b - a for a, b in zip(s0, s1)], s1


def _aggregate(cc, sigs, pks, route, miss=None):
    """aggregate_signatures on the route named, equal to the oracle's bytes"""
    out, d, _ = _delta(cc, lambda: cc.aggregate_signatures(sigs, pks))
    print("aggregate n", len(sigs), "delta", d)
    assert (d[ROUTE], d[OLD]) == ((1, 0) if route else (0, 1))
    if miss is not None:
        assert d[MISS] == miss
    assert (0, out) == orc.aggregate_sigs(sigs, pks)
    return out


def _singles(cc, votes, table):
    """each table voter's signature alone on the cache route: the entry holds that signature's point"""
    for s, p in votes:
        if p in table:
            assert _aggregate(cc, [s], [p], True) == s


def _verify_code(cc, s, h, p):
    return cc.lib.ovh_verify(cc.ctx.ptr, s, len(s), h, len(h), p, len(p))


def test_fill_sign(cc):
    d = ac.sha(b"sc sign")
    cc.update_pubkeys([p for _, p in ac.validators(ac.TABLE_N)])
    sig, dl, _ = _delta(cc, lambda: cc.sign(d))
    assert dl[REG] == 1 and sig == ac.votes(d, 1)[0][0]
    assert _aggregate(cc, [sig], [cc.name], True) == sig
    # signing the same bytes again registers nothing new
    _, dl, _ = _delta(cc, lambda: cc.sign(d))
    assert dl[REG] == 0


def test_fill_per_call_verify(cc):
    d = ac.sha(b"sc verify")
    table = [p for _, p in ac.validators(ac.TABLE_N)]
    cc.update_pubkeys(table)
    (s1, p1), (s2, p2) = ac.votes(d, 3)[1:]
    code, dl, _ = _delta(cc, lambda: _verify_code(cc, s1, d, p1))
    assert code == 0 and dl[REG] == 1
    assert _aggregate(cc, [s1], [p1], True) == s1
    # a vote with code 5 is not registered: the aggregate over it misses, on the full path
    code, dl, _ = _delta(cc, lambda: _verify_code(cc, s2, d, p1))
    assert code == 5 == orc.verify(s2, d, p1) and dl[REG] == 0
    _aggregate(cc, [s1, s2], [p1, p1], False, miss=1)
    # a vote that was never verified
    _aggregate(cc, [s2], [p2], False, miss=1)


@pytest.mark.parametrize("n", [2, 5])
def test_fill_prefetch(cc, n):
    d = ac.sha(b"sc prefetch %d" % n)
    order, table = ac.interleaved(d)
    cc.update_pubkeys(table)
    part = order[:n] if n == 5 else order[1:3]          # 5: outsider, 3 table voters, outsider; 2: table voters
    _, dl, _ = _delta(cc, lambda: cc.prefetch([s for s, _ in part], [d] * n, [p for _, p in part]))
    assert dl[REG] == n
    _singles(cc, part, table)
    tv = [(s, p) for s, p in part if p in table]
    _aggregate(cc, [s for s, _ in tv][::-1], [p for _, p in tv][::-1], True)


def test_fill_round_add_3(cc):
    d = ac.sha(b"sc round add")
    order, table = ac.interleaved(d)
    cc.update_pubkeys(table)
    part = order[3:6]                                     # table, outsider, table
    assert [p in table for _, p in part] == [True, False, True]
    with cc.open_round(d) as rd:
        (code, codes, taken, cnt, _, _), dl, _ = _delta(cc, lambda: rd.add_raw([s for s, _ in part], [p for _, p in part]))
        assert code == 0 and codes.tolist() == [0, 0, 0] and cnt == 2
        assert dl[REG] == 3
    _singles(cc, part, table)
    _aggregate(cc, [part[2][0], part[0][0]], [part[2][1], part[0][1]], True)


def test_fill_same_message_route_scatter():
    """6 votes over 2 hashes under OVH_SAMEMSG=2: k_sc_scatter copies the code-0 votes' sigma"""
    cc = _new_cc("2")
    da, db = ac.sha(b"sc same A"), ac.sha(b"sc same B")
    table = [p for _, p in ac.validators(ac.TABLE_N)]
    cc.update_pubkeys(table)
    va, vb, out = ac.votes(da, 4), ac.votes(db, 4), ac.votes(da, 1, lo=1000)[0]
    # outsider first (staged last), an invalid vote (B's signature on A) in the middle
    votes = [(out[0], da, out[1]), (va[1][0], da, va[1][1]), (vb[2][0], db, vb[2][1]), (vb[3][0], da, vb[3][1]),
             (va[2][0], da, va[2][1]), (vb[1][0], db, vb[1][1])]
    want = [orc.verify(s, h, p) for s, h, p in votes]
    assert want == [0, 0, 0, 5, 0, 0]
    b0 = cc.samemsg_stats()[0]
    codes, dl, _ = _delta(cc, lambda: cc.verify_batch([v[0] for v in votes], [v[1] for v in votes], [v[2] for v in votes]))
    assert codes.tolist() == want and cc.samemsg_stats()[0] == b0 + 1
    assert dl[REG] == 5
    for i, (s, h, p) in enumerate(votes):
        if p in table:
            out96 = _aggregate(cc, [s], [p], want[i] == 0, miss=None if want[i] == 0 else 1)
            assert out96 == s
    good = [v for v, w in zip(votes, want) if w == 0 and v[2] in table]
    _aggregate(cc, [v[0] for v in good][::-1], [v[2] for v in good][::-1], True)


@pytest.fixture(scope="module")
def eleven(cc):
    """the interleaved call of 11 votes, prefetched once (the small route)"""
    d = ac.sha(b"sc eleven")
    order, table = ac.interleaved(d)
    cc.update_pubkeys(table)
    _, dl, _ = _delta(cc, lambda: cc.prefetch([s for s, _ in order], [d] * len(order), [p for _, p in order]))
    assert dl[REG] == len(order)
    return d, order, table, [(s, p) for s, p in order if p in table]


def test_aggregate_all_subsets_and_a_duplicate(cc, eleven):
    d, order, table, tv = eleven
    cc.update_pubkeys(table)
    _singles(cc, order, table)
    sigs, pks = [s for s, _ in tv], [p for _, p in tv]
    _aggregate(cc, sigs, pks, True)
    _aggregate(cc, sigs[::-1], pks[::-1], True)
    pick = [5, 0, 7, 2]
    _aggregate(cc, [sigs[i] for i in pick], [pks[i] for i in pick], True)
    # one signature twice: summed with its multiplicity (adjacent: a doubling at level 0; apart)
    _aggregate(cc, [sigs[1], sigs[1], sigs[4]], [pks[1], pks[1], pks[4]], True)
    _aggregate(cc, [sigs[1], sigs[4], sigs[1]], [pks[1], pks[4], pks[1]], True)
    ds, dp, two = ac.doubled(d)
    assert ds[0] == sigs[0]
    assert _aggregate(cc, ds, dp, True) == two


def test_misses_take_the_full_path(cc, eleven):
    d, order, table, tv = eleven
    cc.update_pubkeys(table)
    sigs, pks = [s for s, _ in tv], [p for _, p in tv]
    # a voter outside the table (its signature is cached: the key decides)
    o = next((s, p) for s, p in order if p not in table)
    _aggregate(cc, sigs[:2] + [o[0]], pks[:2] + [o[1]], False, miss=0)
    # an uncompressed signature
    u = ac.uncompressed(sigs[0])
    out, dl, _ = _delta(cc, lambda: cc.aggregate_signatures([u, sigs[1]], [pks[0], pks[1]]))
    assert (dl[ROUTE], dl[OLD]) == (0, 1)
    assert (0, out) == orc.aggregate_sigs([u, sigs[1]], [pks[0], pks[1]]) == orc.aggregate_sigs(sigs[:2], pks[:2])
    # a signature that was never verified by this context
    fresh = ac.votes(ac.sha(b"sc never verified"), 2)
    _aggregate(cc, [sigs[0], fresh[1][0]], [pks[0], fresh[1][1]], False, miss=1)


def test_mirror_pair_sums_to_the_identity(cc):
    d = ac.sha(b"sc mirror")
    a, b = ac.mirror_pair(d)
    cc.update_pubkeys([a[1], b[1]])
    _, dl, _ = _delta(cc, lambda: cc.prefetch([a[0], b[0]], [d, d], [a[1], b[1]]))
    assert dl[REG] == 2
    assert _aggregate(cc, [a[0], b[0]], [a[1], b[1]], True) == ac.IDENTITY_G2
    assert _aggregate(cc, [b[0], a[0]], [b[1], a[1]], True) == ac.IDENTITY_G2


@pytest.fixture(scope="module")
def big(cc):
    """129 validators' votes, prefetched once in one call (the small route)"""
    d = ac.sha(b"sc 129")
    v = ac.votes(d, 129)
    cc.update_pubkeys([p for _, p in v])
    _, dl, _ = _delta(cc, lambda: cc.prefetch([s for s, _ in v], [d] * 129, [p for _, p in v]))
    assert dl[REG] == 129
    return d, v


@pytest.mark.parametrize("n", [64, 65, 129])
def test_chunk_boundaries(cc, big, n):
    d, v = big
    cc.update_pubkeys([p for _, p in v])
    sigs, pks = [s for s, _ in v], [p for _, p in v]
    _aggregate(cc, sigs[:n], pks[:n], True)
    _aggregate(cc, sigs[129 - n:][::-1], pks[129 - n:][::-1], True)


def test_capacity_8_evicts_in_order_and_0_turns_it_off():
    cc = _new_cc()
    d = ac.sha(b"sc capacity")
    v = ac.votes(d, 12)
    table = [p for _, p in v]
    cc.update_pubkeys(table)
    cc.sig_cache_config(8)
    for k in range(0, 12, 4):
        cc.prefetch([s for s, _ in v[k:k + 4]], [d] * 4, table[k:k + 4])
    st = cc.agg_stats()
    assert st[REG] == 12 and st[ENT] == 8
    sigs = [s for s, _ in v]
    _aggregate(cc, sigs[4:], table[4:], True)                 # the eight retained ones
    _aggregate(cc, sigs[3:6], table[3:6], False, miss=1)      # vote 3 was evicted
    _aggregate(cc, sigs[:4], table[:4], False, miss=4)
    # a call of more votes than the ring holds fills nothing and evicts nothing
    _, dl, s1 = _delta(cc, lambda: cc.prefetch(sigs[:9], [d] * 9, table[:9]))
    assert dl[REG] == 0 and s1[ENT] == 8
    # off mid-stream: emptied, the full path, nothing registered
    cc.sig_cache_config(0)
    assert cc.agg_stats()[ENT] == 0
    _aggregate(cc, sigs[4:], table[4:], False, miss=0)
    _, dl, _ = _delta(cc, lambda: cc.prefetch(sigs[:4], [d] * 4, table[:4]))
    assert dl[REG] == 0
    # on again: empty, then filled again
    cc.sig_cache_config(8)
    _aggregate(cc, sigs[4:], table[4:], False, miss=8)
    cc.prefetch(sigs[4:8], [d] * 4, table[4:8])
    _aggregate(cc, sigs[4:8], table[4:8], True)
    with pytest.raises(ValueError):
        cc.sig_cache_config(65537)


def test_rounds_are_unchanged_with_the_cache_on(cc):
    """the round API's bytes equal ovh_build_qc's over the same votes, cache on, and the aggregate
    of the taken votes then runs on the cache route"""
    d = ac.sha(b"sc rounds")
    order, table = ac.interleaved(d)
    cc.update_pubkeys(table)
    sigs, pks = [s for s, _ in order], [p for _, p in order]
    agg, bitmap, codes, taken = cc.build_qc(sigs, d, pks)
    assert codes.tolist() == [0] * 11 and taken.tolist() == [p in table for p in pks]
    with cc.open_round(d) as rd:
        rd.add(sigs[:1], pks[:1])
        rd.add(sigs[1:4], pks[1:4])
        rd.add(sigs[4:], pks[4:])
        assert rd.qc() == (agg, bitmap, 8)
    ts = [s for s, t in zip(sigs, taken) if t]
    tp = [p for p, t in zip(pks, taken) if t]
    assert _aggregate(cc, ts, tp, True) == agg
