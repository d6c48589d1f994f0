"""ovh_build_qc on the GPU: the leader's verify + select + aggregate of a
round in one device pass, against the C oracle and the selection model (tests/qc_model.py).

Every round is signed on the device (test_gpu_samemsg._round) and its validator table is the
round's keys. Round sizes hit the structural edges of the sum and the routing: 1 (the per-call
path), 2 and 3 (odd tail at level 0), 64 and 65 (chunk boundary), 67 (config 2), 1,025 (just above
the small-batch size) and 4,161 (65 chunks + 1: the upper workgroup loops). Rounds of 64 votes
and more carry every corruption of the list below at seeded positions; the rounds of 1, 2 and 3
votes have no room for them and are clean, and three small hand-made rounds cover a duplicate,
invalid-then-valid and a non-member at those sizes.

    sigma + G2 (code 5), the golden sig_not_in_g2 (3), the golden pk_x_eq_p (102), a validly
    signed vote from a key outside the table, an exact duplicate of a valid vote, a voter whose
    first vote is sigma + G2 and whose second is valid.

The last three tests are rounds of related keys (a validator beside its mirror, a validator that
is a combination of three others): their sums double and cancel, which unrelated keys never do."""
import ctypes
import random

import numpy as np
import pytest

import bls12_381 as bls
import orc
import qc_model
import synth_votes as sv
from test_gpu_samemsg import _named, _round

pytestmark = pytest.mark.gpu

CORRUPT_MIN = 64


@pytest.fixture(scope="module")
def cc():
    import consensus_overlord_amd as coa
    return coa.ConsensusCrypto(bytes.fromhex("7a" * 32))


def _make_round(ctx, golden, lo, n, digest, corrupt=True):
    """-> (sigs, voters, table): n votes as bytes lists, and the validator keys (config order =
    signing order, which is not the sorted order)."""
    if not corrupt or n < CORRUPT_MIN:
        sigs, pks = _round(ctx, lo, n, digest)
        return [bytes(s) for s in sigs], [bytes(p) for p in pks], [bytes(p) for p in pks]
    v = n - 3                                        # validators; + outsider, duplicate, second vote
    sg, pk = _round(ctx, lo, v + 1, digest)
    votes = [[bytes(sg[i]), bytes(pk[i])] for i in range(v)]
    table = [bytes(p) for p in pk[:v]]
    rng = random.Random(n * 7919 + lo)
    a, b, c, d, e = rng.sample(range(v), 5)
    votes[a][0] = sv.add_g2(votes[a][0])                                   # 5
    votes[b][0] = bytes(_named(golden, "sig_not_in_g2", "sig"))            # 3
    votes[c][1] = bytes(_named(golden, "pk_x_eq_p", "pk"))                 # 102
    dup = list(votes[d])
    second = list(votes[e])                                                # e's valid vote
    votes[e][0] = sv.add_g2(votes[e][0])                                   # e's first vote
    first_e = votes[e]
    extra = [[bytes(sg[v]), bytes(pk[v])], dup, second]
    for x in extra:
        votes.insert(rng.randrange(len(votes) + 1), x)
    i1 = next(i for i, x in enumerate(votes) if x is first_e)
    i2 = next(i for i, x in enumerate(votes) if x is second)
    if i2 < i1:
        votes[i1], votes[i2] = votes[i2], votes[i1]
    assert len(votes) == n
    return [x[0] for x in votes], [x[1] for x in votes], table


def _oracle_codes(sigs, digest, voters):
    n = len(sigs)
    return sv.oracle_codes(np.frombuffer(b"".join(sigs), dtype=np.uint8).reshape(n, 96),
                           np.tile(np.frombuffer(digest, dtype=np.uint8), (n, 1)),
                           np.frombuffer(b"".join(voters), dtype=np.uint8).reshape(n, 48))


def _verify_code(cc, sig, digest, voter):
    from consensus_overlord_amd.crypto import ConsensusError, CryptoErr
    try:
        cc.verify_signature(sig, digest, voter)
        return 0
    except CryptoErr as e:
        return e.code
    except ConsensusError:
        return 102


def _check_round(cc, sigs, voters, table, digest, cache=True, qc_code=0):
    """qc_code: what verifying the built QC must give (None: whatever the oracle gives)"""
    from consensus_overlord_amd import vote
    n = len(sigs)
    cc.update_pubkeys(table)
    want = _oracle_codes(sigs, digest, voters)
    m_taken, m_bitmap, m_cnt = qc_model.select(want, voters, table)
    code, agg, bitmap, codes, taken, cnt = cc.build_qc_raw(sigs, digest, voters)
    print("n", n, "return", code, "n_signed", cnt, "model", m_cnt, "codes", sorted(set(codes.tolist())))
    assert codes.tolist() == want.tolist()
    assert taken.astype(int).tolist() == m_taken
    assert bitmap == m_bitmap and cnt == m_cnt
    assert code == (0 if m_cnt else 4)
    if m_cnt:
        ts = [s for s, t in zip(sigs, m_taken) if t]
        tv = [p for p, t in zip(voters, m_taken) if t]
        assert (0, agg) == orc.aggregate_sigs(ts, tv)
        want_qc = orc.verify_aggregated(agg, digest, vote.extract_voters(table, bitmap))
        assert qc_code is None or want_qc == qc_code
        assert cc.verify_qc_batch([agg], [digest], [bitmap]).tolist() == [want_qc]
        assert agg == cc.aggregate_signatures(ts, tv)          # the two-call path agrees
        got = cc.build_qc(sigs, digest, voters)
        assert got[0] == agg and got[1] == bitmap
    if cache:
        h0, m0, _ = cc.cache_stats()
        for i in range(n):
            assert _verify_code(cc, sigs[i], digest, voters[i]) == want[i], i
        h1, m1, _ = cc.cache_stats()
        assert h1 - h0 == n and m1 == m0
    return want, m_taken, bitmap, agg


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 67, 1025, 4161])
def test_round_matches_oracle_and_model(cc, golden, n):
    digest = sv.sha(b"build_qc round %d" % n)
    sigs, voters, table = _make_round(cc.ctx, golden, 90000 + 5000 * (n % 13), n, digest)
    want, taken, _, _ = _check_round(cc, sigs, voters, table, digest)
    if n >= CORRUPT_MIN:
        assert sorted(set(want.tolist())) == [0, 3, 5, 102]
        assert want.tolist().count(0) == n - 4        # a, b, c and e's first vote fail
        assert sum(taken) == n - 6                    # ... and the outsider and one of the duplicates stay out


def test_small_rounds_duplicate_invalid_then_valid_non_member(cc):
    digest = sv.sha(b"build_qc small")
    sg, pk = _round(cc.ctx, 97000, 3, digest)
    s, p = [bytes(x) for x in sg], [bytes(x) for x in pk]
    table = p[:2]                                                     # p[2] is not a validator
    _check_round(cc, [s[0], s[0]], [p[0], p[0]], table, digest)       # exact duplicate
    _check_round(cc, [sv.add_g2(s[1]), s[0], s[1]], [p[1], p[0], p[1]], table, digest)   # invalid, then valid
    _check_round(cc, [s[2], s[1], s[2]], [p[2], p[1], p[2]], table, digest)              # non-member, twice
    _check_round(cc, [s[2]], [p[2]], table, digest)                   # one vote, not taken -> 4
    _check_round(cc, [sv.add_g2(s[0])], [p[0]], table, digest)        # one vote, invalid -> 4


def test_every_vote_fails_returns_4_with_exact_codes(cc, golden):
    from consensus_overlord_amd.crypto import CryptoErr
    digest = sv.sha(b"build_qc all fail")
    sg, pk = _round(cc.ctx, 97100, 5, digest)
    table = [bytes(x) for x in pk]
    sigs = [sv.add_g2(bytes(x)) for x in sg]
    sigs[3] = bytes(_named(golden, "sig_not_in_g2", "sig"))
    want, taken, bitmap, _ = _check_round(cc, sigs, table, table, digest)
    assert want.tolist() == [5, 5, 5, 3, 5] and sum(taken) == 0 and bitmap == bytes(1)
    with pytest.raises(CryptoErr) as ei:
        cc.build_qc(sigs, digest, table)
    assert ei.value.code == 4


def test_clean_round_sets_every_bit(cc, golden):
    digest = sv.sha(b"build_qc clean")
    sigs, voters, table = _make_round(cc.ctx, golden, 97200, 100, digest, corrupt=False)
    want, taken, bitmap, _ = _check_round(cc, sigs, voters, table, digest)
    assert not want.any() and all(taken)
    assert bitmap == bytes([0xFF] * 12 + [0xF0])


def test_build_proof_round_trips_through_check_block(cc):
    from consensus_overlord_amd import vote
    height, round_, data = 41, 2, b"block 41 body"
    bh = cc.hash(data)
    vh = vote.vote_hash(cc, height, round_, vote.PRECOMMIT, bh)
    sg, pk = _round(cc.ctx, 97400, 10, vh)
    table = [bytes(x) for x in pk]
    cc.update_pubkeys(table)
    sigs = [bytes(x) for x in sg]
    sigs[4] = sv.add_g2(sigs[4])
    proof = cc.build_proof(height, round_, bh, sigs, table)
    assert cc.check_block(height, data, proof) is True
    assert cc.check_blocks([(height, data, proof)]).tolist() == [True]
    h, r, b, sig, bitmap = vote.decode_proof(proof)
    assert bin(int.from_bytes(bitmap, "big")).count("1") == 9
    flipped = bytes([bitmap[0] ^ 0x40]) + bitmap[1:]
    assert cc.check_block(height, data, vote.encode_proof(h, r, b, sig, flipped)) is False


def test_13_key_table_pad_bits_and_wrong_bitmap_len(cc):
    digest = sv.sha(b"build_qc 13")
    sg, pk = _round(cc.ctx, 97500, 13, digest)
    table = [bytes(x) for x in pk]
    sigs = [bytes(x) for x in sg]
    _, _, bitmap, _ = _check_round(cc, sigs, table, table, digest)
    assert bitmap == bytes([0xFF, 0xF8]) and bitmap[1] & 0b111 == 0
    codes = np.zeros(13, dtype=np.int32)
    out = ctypes.create_string_buffer(96)
    cnt = ctypes.c_uint32(0)
    for bl in (1, 3):
        bm = ctypes.create_string_buffer(4)
        r = cc.lib.ovh_build_qc(cc.ctx.ptr, 13, b"".join(sigs), digest, 32, b"".join(table),
                                codes.ctypes.data_as(ctypes.c_void_p), None, out, bm, bl, ctypes.byref(cnt))
        assert r == 103
    bm = ctypes.create_string_buffer(2)
    assert cc.lib.ovh_build_qc(cc.ctx.ptr, 13, b"".join(sigs), digest, 31, b"".join(table),
                               codes.ctypes.data_as(ctypes.c_void_p), None, out, bm, 2, ctypes.byref(cnt)) == 100
    assert cc.lib.ovh_build_qc(cc.ctx.ptr, 13, b"".join(sigs), digest, 32, b"".join(table),
                               codes.ctypes.data_as(ctypes.c_void_p), None, out, bm, 2, ctypes.byref(cnt)) == 0
    assert bm.raw == bitmap and cnt.value == 13            # taken may be NULL


def test_multi_device_context(cc, golden):
    import consensus_overlord_amd as coa
    from consensus_overlord_amd.crypto import Context
    mc = coa.ConsensusCrypto(bytes.fromhex("7b" * 32), ctx=Context(devices=[0, 0]))
    digest = sv.sha(b"build_qc multi")
    sigs, voters, table = _make_round(cc.ctx, golden, 97600, 70, digest)
    _check_round(mc, sigs, voters, table, digest)


# ------------------------------------------------------------------------------ related keys
# Votes whose keys and signatures are related, made from device-signed votes without any secret:
# the sums of a round's sigma (and of a QC's keys) then double or cancel, which unrelated keys
# never do. Where they meet in the device's trees depends on the staging; the exact-placement
# claims are tests/test_gpu_qc_kernels.py's.
def _mirror(sig, pk):
    """(-sigma, -pk): the valid vote of the validator with secret r - sk (the sign bit of both
    compressed encodings flipped)"""
    return bytes([sig[0] ^ 0x20]) + sig[1:], bytes([pk[0] ^ 0x20]) + pk[1:]


def _combination(a, b, c):
    """(sigma_a + sigma_b - sigma_c, pk_a + pk_b - pk_c) of three (sig, pk): the valid vote of the
    validator with secret sk_a + sk_b - sk_c, over the Python oracle"""
    F2, F1 = bls.Fp2Ops, bls.FpOps
    s = [bls.g2_from_bytes(x[0]) for x in (a, b, c)]
    k = [bls.g1_from_bytes(x[1]) for x in (a, b, c)]
    sig = bls.pt_add(F2, bls.pt_add(F2, s[0], s[1]), bls.pt_neg(F2, s[2]))
    pk = bls.pt_add(F1, bls.pt_add(F1, k[0], k[1]), bls.pt_neg(F1, k[2]))
    return bls.g2_compress(sig), bls.g1_compress(pk)


def _votes(ctx, lo, n, digest):
    sg, pk = _round(ctx, lo, n, digest)
    return [(bytes(s), bytes(p)) for s, p in zip(sg, pk)]


def _check_related(cc, votes, digest):
    sigs, voters = [v[0] for v in votes], [v[1] for v in votes]
    assert len(set(voters)) == len(voters)
    want, taken, _, agg = _check_round(cc, sigs, voters, voters, digest, qc_code=None)
    assert not want.any() and all(taken)
    return agg


def test_round_of_a_validator_and_its_mirror(cc):
    """sigma + (-sigma): the aggregate is the compressed identity, the aggregated key is infinite"""
    digest = sv.sha(b"build_qc mirror")
    v = _votes(cc.ctx, 98000, 1, digest)[0]
    m = _mirror(*v)
    assert orc.verify(m[0], digest, m[1]) == 0
    assert _check_related(cc, [v, m], digest) == bls.g2_compress(None)
    assert _check_related(cc, [m, v], digest) == bls.g2_compress(None)


def test_round_with_a_combination_validator(cc):
    """votes a, b, c, d = a + b - c at positions 0 to 3 of a round of 8: sigma_a + sigma_b equals
    sigma_c + sigma_d"""
    digest = sv.sha(b"build_qc combination")
    v = _votes(cc.ctx, 98100, 7, digest)
    d = _combination(v[0], v[1], v[2])
    assert orc.verify(d[0], digest, d[1]) == 0
    agg = _check_related(cc, v[:3] + [d] + v[3:], digest)
    assert agg != bls.g2_compress(None)


def test_round_whose_second_chunk_mirrors_its_first(cc):
    """130 votes: votes 64 .. 127 are the mirrors of votes 0 .. 63, two more follow; the aggregate
    is the sum of the last two"""
    digest = sv.sha(b"build_qc mirrored chunk")
    v = _votes(cc.ctx, 98200, 66, digest)
    votes = v[:64] + [_mirror(*x) for x in v[:64]] + v[64:]
    agg = _check_related(cc, votes, digest)
    assert (0, agg) == orc.aggregate_sigs([x[0] for x in v[64:]], [x[1] for x in v[64:]])
