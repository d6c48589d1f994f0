"""The MSM kernels that run several tree levels per launch (csrc/msm.hpp: k_msm_chunk,
k_msm_upper, k_msm_plane, k_msm_comb) through the batch path of a context created with
OVH_SMALL_MAX=0 (pool + MSM + final for every size), at the sizes around their block boundaries.

S = sum r_i sigma_i is checked two ways. The per-vote codes must equal the C oracle's; and the
shard partial of the same votes (ovh_batch_partial_device: the folded Miller product and the
MSM's S) must pass or fail the combined check prod f * e(-G1, S) == 1 exactly as the votes
demand -- with every counted vote valid it passes only if S is exact, whatever the bisection
would repair afterwards. The RLC digits spread evenly, so below ~6,000 votes no bucket has more
than one 64-entry chunk; the 8,192-vote case is the one that runs chunks 1.. and k_msm_upper
(tests/test_msm_chunk_model.py walks those paths on the CPU with crowded buckets, and
tests/test_gpu_msm_buckets.py runs the kernels on crafted buckets against exact sums). The
replayed votes are what a Byzantine validator can send: one vote many times puts identical points
into every bucket, and sigma beside -sigma makes buckets cancel."""
import os
import random

import numpy as np
import pytest

import synth_votes as sv

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 31, 32, 33, 64, 65, 129, 257)
NMAX = max(SIZES)
RLC_SEED = 0x6D736D5F6C766C73


def _ctx(flags=0):
    import consensus_overlord_amd as coa
    from consensus_overlord_amd.crypto import Context
    old = os.environ.get("OVH_SMALL_MAX")
    os.environ["OVH_SMALL_MAX"] = "0"
    try:
        return coa.ConsensusCrypto(bytes.fromhex("6d" * 32), ctx=Context(flags=flags))
    finally:
        if old is None:
            os.environ.pop("OVH_SMALL_MAX", None)
        else:
            os.environ["OVH_SMALL_MAX"] = old


@pytest.fixture(scope="module")
def plain():
    return _ctx()


@pytest.fixture(scope="module")
def fixed():
    """predictable coefficients (tests only), so that a failure reproduces"""
    from consensus_overlord_amd.crypto import FLAG_TEST_RLC
    c = _ctx(FLAG_TEST_RLC)
    c.ctx.set_test_rlc(RLC_SEED, 0)
    return c


@pytest.fixture(scope="module")
def votes(plain):
    """NMAX device-signed votes (numpy), all valid by the oracle; the sizes take prefixes"""
    sigs, hs, pks = sv.make(plain.ctx, NMAX, lo=120000)
    assert (sv.oracle_codes(sigs, hs, pks) == 0).all()
    return sigs, hs, pks


def _run(cc, sigs, hs, pks):
    """-> (per-vote codes of the batch path, codes of the shard partial, its combined verdict)"""
    import torch
    from consensus_overlord_amd import device as dev
    d = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (sigs, hs, pks)]
    n = d[0].shape[0]
    codes = dev.verify_batch(cc.ctx, *d).cpu().numpy()
    part = torch.empty((1, 864), dtype=torch.uint8, device="cuda")
    pcodes = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    dev.batch_partial(cc.ctx, *d, pcodes, part[0])
    return codes, pcodes.cpu().numpy(), dev.combine_partials(cc.ctx, part)


@pytest.mark.parametrize("n", SIZES)
def test_all_valid(plain, fixed, votes, n):
    sigs, hs, pks = (x[:n] for x in votes)
    for cc in (plain, fixed):
        codes, pcodes, verdict = _run(cc, sigs, hs, pks)
        assert (codes == 0).all() and (pcodes == 0).all()
        assert verdict, "S of the MSM is not sum r_i sigma_i"


@pytest.mark.parametrize("n", SIZES)
def test_one_vote_plus_g2(plain, fixed, votes, n):
    """sigma + G2 at a seeded position: that position alone is flagged, and the combined check
    over the partial (which counts the vote: its code is 0 before any pairing) fails"""
    sigs, hs, pks = (x[:n].copy() for x in votes)
    i = random.Random(n).randrange(n)
    sigs[i] = np.frombuffer(sv.add_g2(bytes(sigs[i])), dtype=np.uint8)
    want = sv.oracle_codes(sigs, hs, pks)
    assert [k for k in range(n) if want[k]] == [i]
    for cc in (plain, fixed):
        codes, pcodes, verdict = _run(cc, sigs, hs, pks)
        assert codes.tolist() == want.tolist()
        assert (pcodes == 0).all() and not verdict


@pytest.mark.parametrize("n", (65, 257))
def test_failed_votes_are_skipped(plain, fixed, votes, golden, n):
    """keys that do not parse and signatures outside G2 among the valid votes: their codes are the
    oracle's, the MSM leaves them out (as the fold does), and the rest still passes"""
    sigs, hs, pks = (x[:n].copy() for x in votes)
    case = {c["name"]: c for c in golden["verify"]}
    bad_pk = np.frombuffer(bytes.fromhex(case["pk_x_eq_p"]["pk"]), dtype=np.uint8)
    bad_sig = np.frombuffer(bytes.fromhex(case["sig_not_in_g2"]["sig"]), dtype=np.uint8)
    where = random.Random(1000 + n).sample(range(n), 6)
    for i in where[:3]:
        pks[i] = bad_pk
    for i in where[3:]:
        sigs[i] = bad_sig
    want = sv.oracle_codes(sigs, hs, pks)
    assert sorted(k for k in range(n) if want[k]) == sorted(where)
    assert {int(want[i]) for i in where[:3]} == {102} and {int(want[i]) for i in where[3:]} == {3}
    for cc in (plain, fixed):
        codes, pcodes, verdict = _run(cc, sigs, hs, pks)
        assert codes.tolist() == want.tolist() and pcodes.tolist() == want.tolist()
        assert verdict, "S of the MSM is not the sum over the votes with code 0"


REPLAYS = (2, 33, 65, 257)


@pytest.mark.parametrize("n", REPLAYS)
def test_one_vote_replayed(plain, fixed, votes, n):
    """a validator's vote sent n times: every bucket's points are copies of sigma (or of tau), so
    every pair add of the bucket trees is a doubling; all copies are valid and S is exact"""
    sigs, hs, pks = (np.repeat(x[7:8], n, axis=0) for x in votes)
    for cc in (plain, fixed):
        codes, pcodes, verdict = _run(cc, sigs, hs, pks)
        assert (codes == 0).all() and (pcodes == 0).all()
        assert verdict, "S of the MSM is not (sum r_i) sigma"


@pytest.mark.parametrize("n", REPLAYS)
def test_one_vote_replayed_with_negated_copies(plain, fixed, votes, n):
    """the same, with -sigma in the odd copies: buckets hold sigma and -sigma and cancel. The
    negated copies fail as the oracle says; the partial counts every copy (a vote's code is 0
    before any pairing), so its combined check fails"""
    import bls12_381 as bls
    sigs, hs, pks = (np.repeat(x[7:8], n, axis=0) for x in votes)
    neg = bls.g2_compress(bls.pt_neg(bls.Fp2Ops, bls.g2_from_bytes(bytes(sigs[0]))))
    sigs[1::2] = np.frombuffer(neg, dtype=np.uint8)
    want = sv.oracle_codes(sigs, hs, pks)
    assert want.tolist() == [5 * (k & 1) for k in range(n)]
    for cc in (plain, fixed):
        codes, pcodes, verdict = _run(cc, sigs, hs, pks)
        assert codes.tolist() == want.tolist()
        assert (pcodes == 0).all() and not verdict


def test_buckets_of_several_chunks(fixed):
    """8,192 votes: 64.2 points per bucket on average, so about half the buckets have a second
    chunk and a level-6 pair (k_msm_upper). The combined check over the partial proves S; one
    vote plus G2 must fail it."""
    import torch
    from consensus_overlord_amd import device as dev
    from test_gpu_parity import _synth
    n = 8192
    sks, hs = _synth(n, seed=0x6D73)
    pks = dev.sk_to_pk_batch(fixed.ctx, sks)
    sigs = dev.sign_batch(fixed.ctx, sks, hs)
    part = torch.empty((1, 864), dtype=torch.uint8, device="cuda")
    codes = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    dev.batch_partial(fixed.ctx, sigs, hs, pks, codes, part[0])
    assert (codes.cpu().numpy() == 0).all()
    assert dev.combine_partials(fixed.ctx, part), "S of the MSM is not sum r_i sigma_i"
    i = 4097
    s_host = sigs.cpu().numpy().copy()
    s_host[i] = np.frombuffer(sv.add_g2(bytes(s_host[i])), dtype=np.uint8)
    sigs2 = torch.from_numpy(s_host).cuda()
    torch.cuda.synchronize()
    dev.batch_partial(fixed.ctx, sigs2, hs, pks, codes, part[0])
    assert not dev.combine_partials(fixed.ctx, part)
    got = dev.verify_batch(fixed.ctx, sigs2, hs, pks).cpu().numpy()
    assert [k for k in range(n) if got[k]] == [i] and got[i] == 5
