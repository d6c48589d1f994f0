"""ovh_check_blocks (ConsensusCrypto.check_block_batch): Consensus::check_block for many blocks in
one device pass, against the oracle-backed mirror of tests/test_check_block.py (its cases, its
validators, its OracleCrypto) and against the Python composition check_blocks. The reasons are
checked against the same mirror: 300 / 301 / the C oracle's verify_aggregated code."""
import hashlib

import numpy as np
import pytest

from consensus_overlord_amd import vote
from consensus_overlord_amd.crypto import ConsensusCrypto
from test_check_block import OracleCrypto, cases, net  # noqa: F401  (net: module fixture, 100 validators)

pytestmark = pytest.mark.gpu


def sm3(b):
    return hashlib.new("sm3", bytes(b)).digest()


def reason(pks, height, data, proof):
    """check_block's steps with the C oracle in place of the device: 0, or why not."""
    import orc
    try:
        h, r, bh, sig, bm = vote.decode_proof(proof)
    except ValueError:
        return 300
    if bytes(bh) != sm3(data) or h != height:
        return 301
    voters = vote.extract_voters(pks, bm)
    return orc.verify_aggregated(bytes(sig), sm3(vote.rlp_vote(h, r, vote.PRECOMMIT, bh)), voters)


def crypto(pks, key="96"):
    import consensus_overlord_amd as coa
    cc = coa.ConsensusCrypto(bytes.fromhex(key * 32))
    if pks is not None:
        cc.update_pubkeys(pks)
    return cc


def check(cc, pks, blocks):
    """One check_block_batch call compared with the mirror; returns (ok, reasons)."""
    ok, rs = cc.check_block_batch(blocks)
    want = [reason(pks, *b) for b in blocks]
    assert rs.tolist() == want
    assert ok.tolist() == [w == 0 for w in want]
    return ok, rs


@pytest.fixture(scope="module")
def small():
    """8 validators (oracle signing stays short) and a QC maker: 6 signers by default."""
    import orc
    sks = [(int.from_bytes(hashlib.sha256(b"check_blocks validator %d" % i).digest(), "big") >> 2).to_bytes(32, "big")
           for i in range(8)]
    pks = [orc.sk_to_pk(sk)[1] for sk in sks]
    order = {pk: i for i, pk in enumerate(sorted(pks))}

    def block(height, round_, data, signers=range(6), nbytes=1, extra_bits=(), signed_round=None):
        bh = sm3(data)
        vh = sm3(vote.rlp_vote(height, round_ if signed_round is None else signed_round, vote.PRECOMMIT, bh))
        sigs = [orc.sign(sks[i], vh)[1] for i in signers]
        agg = orc.aggregate_sigs(sigs, [pks[i] for i in signers])[1]
        bm = bytearray(nbytes)
        for k in [order[pks[i]] for i in signers] + list(extra_bits):
            if k // 8 < nbytes:
                bm[k // 8] |= 0x80 >> (k % 8)
        return (height, data, vote.encode_proof(height, round_, bh, agg, bytes(bm)))
    return pks, block


def test_the_check_block_cases(net):
    cc = crypto(net[0])
    cs = cases(net)
    blocks = [args for _, args, _ in cs]
    ok, rs = check(cc, net[0], blocks)
    assert ok.tolist() == [w for _, _, w in cs], [(n, g) for (n, _, _), g in zip(cs, ok.tolist())]
    assert ok.tolist() == cc.check_blocks(blocks).tolist()
    by_name = {n: int(r) for (n, _, _), r in zip(cs, rs)}
    assert by_name["undecodable proof"] == 300 and by_name["not a proof"] == 300
    assert by_name["proposal height differs"] == 301 and by_name["proposal data differs"] == 301
    assert by_name["empty bitmap"] == 4
    # the 95-byte signature takes the per-call path: the same answer as check_block
    short = blocks[[n for n, _, _ in cs].index("short signature")]
    assert cc.check_block(*short) is False and by_name["short signature"] != 0
    # the oracle-backed mirror of test_check_block.py says the same
    oc = OracleCrypto(net[0])
    assert [ConsensusCrypto.check_block(oc, *b) for b in blocks] == ok.tolist()


def test_proposal_sizes_around_the_sm3_block(small):
    pks, block = small
    cc = crypto(pks)
    blocks = [block(20 + i, i, bytes((7 * i + k) % 251 for k in range(n))) for i, n in enumerate((0, 55, 56, 64, 5000))]
    ok, _ = check(cc, pks, blocks)
    assert ok.all()


def test_batch_of_24_with_three_invalid_in_the_middle(small):
    pks, block = small
    cc = crypto(pks)
    blocks = [block(100 + i, i % 3, b"proposal %d " % i * (1 + i % 5)) for i in range(24)]
    h, d, p = blocks[10]
    blocks[10] = (h, d + b"!", p)                                       # data differs: 301, rides in the batch
    blocks[11] = block(111, 2, b"proposal 11", signed_round=1)          # QC signed for another round: 5
    hh, rr, bh, sig, bm = vote.decode_proof(blocks[13][2])
    blocks[13] = (blocks[13][0], blocks[13][1], vote.encode_proof(hh, rr, bh, b"\xff" * 96, bm))  # not a point
    ok, rs = check(cc, pks, blocks)                                     # exact verdicts (bisection)
    assert [i for i in range(24) if not ok[i]] == [10, 11, 13]
    assert rs[10] == 301 and rs[11] == 5 and rs[13] not in (0, 5, 300, 301)
    for i in (10, 11, 13):                                              # the same three alone, n = 1
        ok1, rs1 = check(cc, pks, [blocks[i]])
        assert (ok1.tolist(), rs1.tolist()) == ([False], [int(rs[i])])
    ok1, _ = check(cc, pks, [blocks[0]])
    assert ok1.tolist() == [True]


def test_bitmaps_of_different_lengths_in_one_call(small):
    pks, block = small
    cc = crypto(pks)
    exact = block(7, 0, b"exact bitmap")
    longer = block(8, 1, b"one byte longer", nbytes=2, extra_bits=(8, 9, 15))   # bits past the list are ignored
    hh, rr, bh, sig, _ = vote.decode_proof(exact[2])
    empty = (7, exact[1], vote.encode_proof(hh, rr, bh, sig, b""))
    ok, rs = check(cc, pks, [exact, longer, empty, exact])
    assert ok.tolist() == [True, True, False, True] and rs[2] == 4
    assert ok.tolist() == cc.check_blocks([exact, longer, empty, exact]).tolist()


def test_no_validator_table(small):
    pks, block = small
    blocks = [block(1, 0, b"a"), block(2, 0, b"bb"), (3, b"c", b"\xc0")]
    cc = crypto(None, key="95")
    for _ in range(2):   # never set, then set to the empty list
        ok, rs = cc.check_block_batch(blocks)
        assert ok.tolist() == [False] * 3 and (rs != 0).all()
        assert cc.check_blocks(blocks).tolist() == [False] * 3
        cc.update_pubkeys([])
    assert isinstance(ok, np.ndarray) and ok.dtype == bool
