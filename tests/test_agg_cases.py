"""The crafted inputs of tests/agg_cases.py are what they claim, checked on the CPU against the C
oracle and the Python curve code: the GPU tests (test_gpu_sig_cache.py,
test_gpu_verify_aggregated_table.py) rely on these properties and never re-derive them."""
import agg_cases as ac
import bls12_381 as bls
import orc

D = ac.sha(b"agg cases check")


def test_votes_are_valid_and_distinct():
    v = ac.votes(D, ac.TABLE_N)
    assert len({s for s, _ in v}) == len({p for _, p in v}) == ac.TABLE_N
    for s, p in v:
        assert len(s) == 96 and len(p) == 48 and orc.verify(s, D, p) == 0


def test_interleaved_call_is_not_in_staged_order():
    order, table = ac.interleaved(D)
    assert len(order) == ac.TABLE_N + ac.OUTSIDERS and len(table) == ac.TABLE_N
    in_table = [p in table for _, p in order]
    assert in_table.count(True) == ac.TABLE_N
    # table-first staging moves votes: the first and the last vote are outsiders, one stands inside
    assert not in_table[0] and not in_table[-1] and not all(in_table[1:-1])
    assert in_table != sorted(in_table, reverse=True)
    for s, p in order:
        assert orc.verify(s, D, p) == 0


def test_mirror_pair_sums_to_the_identity_encoding():
    a, b = ac.mirror_pair(D)
    assert a[0] != b[0] and a[1] != b[1]
    assert orc.verify(a[0], D, a[1]) == 0 and orc.verify(b[0], D, b[1]) == 0
    assert orc.aggregate_sigs([a[0], b[0]], [a[1], b[1]]) == (0, ac.IDENTITY_G2)
    assert ac.IDENTITY_G2 == bls.g2_compress(None)
    code, apk = orc.aggregate_pks([a[1], b[1]])
    assert code == 0 and apk == bls.g1_compress(None)
    # the aggregated key is the identity: blst answers PK_IS_INFINITY
    assert orc.verify_aggregated(ac.IDENTITY_G2, D, [a[1], b[1]]) == 6


def test_doubled_list_is_two_sigma():
    sigs, pks, two = ac.doubled(D)
    assert sigs[0] == sigs[1]
    assert orc.aggregate_sigs(sigs, pks) == (0, two)
    assert two != sigs[0] and two != ac.IDENTITY_G2


def test_outside_g1_key_is_on_the_curve_and_outside_g1():
    pk = ac.outside_g1_key()
    pt = bls.g1_from_bytes(pk)
    assert pt is not None and not bls.g1_in_subgroup(pt)
    # the key parses (the aggregate of keys does not ask for the subgroup) ...
    assert orc.aggregate_pks([pk])[0] == 0
    # ... and a QC over it fails the sum's group check
    s, p = ac.votes(D, 1)[0]
    assert orc.verify_aggregated(s, D, [p, pk]) == 3


def test_unparsable_key_and_edge_signatures():
    s, p = ac.votes(D, 1)[0]
    assert orc.verify_aggregated(s, D, [p, ac.unparsable_key()]) == 102
    e = ac.edge_signatures()
    assert orc.verify_aggregated(e["bad_encoding"], D, [p]) == 1
    assert orc.verify_aggregated(e["off_curve"], D, [p]) == 2
    assert orc.verify_aggregated(e["outside_g2"], D, [p]) == 3
    assert all(len(x) == 96 for x in e.values())


def test_uncompressed_is_the_same_point():
    s, p = ac.votes(D, 1)[0]
    u = ac.uncompressed(s)
    assert len(u) == 192 and orc.verify(u, D, p) == 0
    assert orc.aggregate_sigs([u], [p]) == (0, s)
