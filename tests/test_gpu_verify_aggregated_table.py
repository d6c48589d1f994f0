"""ovh_verify_aggregated on the validator table and the message table
against the C oracle's codes.

Inputs come from tests/agg_cases.py (made on the CPU by the C oracle), expected codes from
orc.verify_aggregated. Every call goes through _check, which asserts the ovh_agg_stats counter of
the route the case means to take -- the table route (stats[5]), on a message-table H or not
(stats[6]), or the full path (stats[7]) -- and that ovh_msg_cache_stats is the same before and
after: the route looks the hash up and never enters it. Voter counts 1, 2, 3, 64 and 65 cross
k_qc_apk's 64 lanes (one key per lane, then a second round for lane 0)."""
import ctypes
import os
import random

import pytest

import agg_cases as ac
import orc

pytestmark = pytest.mark.gpu

TABLE, ON_H, FULL = 5, 6, 7


def _new_cc(mode=None):
    import consensus_overlord_amd as coa
    old = os.environ.get("OVH_QC_TABLE")
    if mode is not None:
        os.environ["OVH_QC_TABLE"] = mode
    try:
        return coa.ConsensusCrypto(bytes.fromhex("7e" * 32))
    finally:
        if mode is not None:
            if old is None:
                del os.environ["OVH_QC_TABLE"]
            else:
                os.environ["OVH_QC_TABLE"] = old


@pytest.fixture(scope="module")
def cc():
    """OVH_QC_TABLE=2: the route on every hash, so each case runs on it whether or not its hash
    is primed (the default takes it on a primed hash only: the last test)"""
    return _new_cc("2")


def _msg_stats(cc):
    st = (ctypes.c_uint64 * 2)()
    assert cc.lib.ovh_msg_cache_stats(cc.ctx.ptr, st) == 0
    return tuple(st)


def _check(cc, agg, h, voters, route, on_h=False):
    """the call's code equals the oracle's; the counters name the route; the message table's
    counters do not move"""
    from consensus_overlord_amd.crypto import _concat
    vd, vl = _concat(voters)
    m0, s0 = _msg_stats(cc), cc.agg_stats()
    code = cc.lib.ovh_verify_aggregated(cc.ctx.ptr, agg, len(agg), h, len(h), vd, vl, len(voters))
    m1, s1 = _msg_stats(cc), cc.agg_stats()
    d = [b - a for a, b in zip(s0, s1)]
    want = orc.verify_aggregated(agg, h, voters)
    print("voters", len(voters), "code", code, "oracle", want, "delta", d[TABLE:])
    assert code == want
    assert (d[TABLE], d[ON_H], d[FULL]) == ((1, int(on_h), 0) if route else (0, 0, 1))
    assert m0 == m1
    return code


def _agg(votes):
    code, agg = orc.aggregate_sigs([s for s, _ in votes], [p for _, p in votes])
    assert code == 0
    return agg


@pytest.fixture(scope="module")
def round65(cc):
    d = ac.sha(b"vat 65")
    v = ac.votes(d, 65)
    return d, v, [p for _, p in v]


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65])
def test_table_voters(cc, round65, n):
    d, v, table = round65
    cc.update_pubkeys(table)
    agg = _agg(v[:n])
    assert _check(cc, agg, d, table[:n], True) == 0
    # the same voters out of sorted (and out of table) order
    shuffled = table[:n][::-1]
    random.Random(n).shuffle(shuffled)
    assert _check(cc, agg, d, shuffled, True) == 0
    if n > 1:
        # a missing voter, and a voter too many
        assert _check(cc, agg, d, table[:n - 1], True) == 5
        assert _check(cc, agg, d, table[:n] + table[64:65], True) == 5


def test_duplicated_voter(cc, round65):
    d, v, table = round65
    cc.update_pubkeys(table)
    # the list counts a voter twice: valid exactly when its signature was summed twice
    assert _check(cc, _agg([v[0], v[1], v[0]]), d, [table[0], table[1], table[0]], True) == 0
    assert _check(cc, _agg([v[0], v[1], v[0]]), d, [table[0], table[0], table[1]], True) == 0
    assert _check(cc, _agg([v[0], v[1]]), d, [table[0], table[1], table[0]], True) == 5
    assert _check(cc, _agg([v[0], v[1], v[0]]), d, [table[0], table[1]], True) == 5


def test_wrong_hash(cc, round65):
    d, v, table = round65
    cc.update_pubkeys(table)
    assert _check(cc, _agg(v[:3]), ac.sha(b"vat another hash"), table[:3], True) == 5


def test_edge_signatures(cc, round65):
    d, v, table = round65
    cc.update_pubkeys(table)
    e = ac.edge_signatures()
    assert _check(cc, e["bad_encoding"], d, table[:3], True) == 1
    assert _check(cc, e["off_curve"], d, table[:3], True) == 2
    assert _check(cc, e["outside_g2"], d, table[:3], True) == 3
    # the identity as a signature, over keys whose sum is not the identity
    assert _check(cc, ac.IDENTITY_G2, d, table[:2], True) == orc.verify_aggregated(ac.IDENTITY_G2, d, table[:2])


def test_mirror_keys_aggregate_to_the_identity(cc):
    d = ac.sha(b"vat mirror")
    a, b = ac.mirror_pair(d)
    cc.update_pubkeys([a[1], b[1]])
    assert _check(cc, _agg([a, b]), d, [a[1], b[1]], True) == 6
    assert _check(cc, a[0], d, [a[1], b[1]], True) == 6
    assert _check(cc, a[0], d, [a[1]], True) == 0


def test_unparsable_table_key_answers_102(cc, round65):
    d, v, table = round65
    bad = ac.unparsable_key()
    cc.update_pubkeys(table[:4] + [bad])
    assert _check(cc, _agg(v[:2]), d, [table[0], bad, table[1]], True) == 102
    # before the signature is looked at, as the full path parses every key first
    assert _check(cc, ac.edge_signatures()["bad_encoding"], d, [table[0], bad], True) == 102
    assert _check(cc, _agg(v[:2]), d, table[:2], True) == 0


def test_table_key_outside_g1_takes_the_full_path(cc, round65):
    d, v, table = round65
    out = ac.outside_g1_key()
    cc.update_pubkeys(table[:4] + [out])
    assert _check(cc, _agg(v[:2]), d, [table[0], table[1], out], False) == 3
    assert _check(cc, _agg(v[:2]), d, table[:2], True) == 0


def test_voter_outside_the_table_takes_the_full_path(cc, round65):
    d, v, table = round65
    cc.update_pubkeys(table[:8])
    assert _check(cc, _agg(v[:9]), d, table[:9], False) == 0
    assert _check(cc, _agg(v[:8]), d, table[:8], True) == 0
    # other sizes of signature and hash: the full path decides
    assert _check(cc, ac.uncompressed(_agg(v[:2])), d, table[:2], False) == 0
    assert _check(cc, _agg(v[:2]), d[:31], table[:2], False) == orc.verify_aggregated(_agg(v[:2]), d[:31], table[:2])


def test_primed_hash_runs_on_the_message_table(cc):
    da, db = ac.sha(b"vat primed"), ac.sha(b"vat unprimed")
    va, vb = ac.votes(da, 3), ac.votes(db, 3)
    table = [p for _, p in va]
    cc.update_pubkeys(table)
    p0 = cc.prime_stats()
    cc.prime([da])
    assert cc.prime_stats()[0] == p0[0] + 1
    assert _check(cc, _agg(va), da, table, True, on_h=True) == 0
    assert _check(cc, _agg(vb), db, table, True, on_h=False) == 0
    # the unprimed hash was not entered: still a miss; and a wrong QC on the primed hash fails on H
    assert _check(cc, _agg(vb), db, table, True, on_h=False) == 0
    assert _check(cc, _agg(vb), da, table, True, on_h=True) == 5
    assert _check(cc, ac.edge_signatures()["outside_g2"], da, table, True, on_h=True) == 3


def test_default_takes_the_route_on_a_primed_hash_only():
    cc = _new_cc()
    da, db = ac.sha(b"vat default primed"), ac.sha(b"vat default unprimed")
    va, vb = ac.votes(da, 3), ac.votes(db, 3)
    table = [p for _, p in va]
    cc.update_pubkeys(table)
    cc.prime([da])
    assert _check(cc, _agg(va), da, table, True, on_h=True) == 0
    assert _check(cc, _agg(vb), db, table, False) == 0
    assert _check(cc, _agg(vb), da, table[::-1], True, on_h=True) == 5
    # a hash the per-call verify has seen is in the message table as well
    s, p = vb[0]
    assert cc.lib.ovh_verify(cc.ctx.ptr, s, 96, db, 32, p, 48) == 0
    assert _check(cc, _agg(vb), db, table, True, on_h=True) == 0
    # an unparsable table key answers 102 from the host on any hash
    cc.update_pubkeys(table + [ac.unparsable_key()])
    assert _check(cc, _agg(vb), ac.sha(b"vat default third"), [table[0], ac.unparsable_key()], True) == 102
