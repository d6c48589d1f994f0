"""Point decoding and the subgroup checks on the GPU, on the crafted points of
tests/point_cases.py (expectations from plain integers; tests/test_point_cases.py ties them to
the Python oracle and the host build):

- the Fp-VM programs on one wave of the device interpreter (dp_vm_run of
  tests/device/fp_probe.hip): sigchk / pkchk / pkdec on every case, the lex / sgn0 program, and
  the whole-vote programs on one case per class == the simulator == the cases;
- the C ABI with crafted keys and signatures among valid votes at every launch site that decodes
  a point: ovh_verify (first call: vote1; message-cache hit: vote1h; uncompressed: k_canon_one),
  the small-batch path on fresh and on primed hashes (votew, votewh; the route asserted with
  prime_stats), the pool and same-message paths, the validator table in contexts of its own
  (votew_t, vote_t, vote_t1, vote_t1h, votewh_t), ovh_verify_aggregated (the VM route,
  k_canon_qc for an uncompressed aggregate, and the parse codes of the one-lane k_verify_agg),
  ovh_verify_qc_batch, ovh_aggregate_sigs and ovh_aggregate_pks. Codes and bytes == the C
  oracle's, and the codes == the class's own (key off-curve, x = 0 or x >= p: 102; key outside
  G1: 3; signature x >= p: 1, off-curve: 2, outside G2: 3)."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

import orc
import overlord_oracle as ov
import point_cases as pc
import point_vm
from vm_helpers import ROOT

pytestmark = pytest.mark.gpu

PROBE = os.path.join(ROOT, "tests", "device", "_build", "libfpprobe.so")
NKEYS = 6
SKS = [ov.synth_sk(0x901D00 + i).to_bytes(32, "big") for i in range(NKEYS)]


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(PROBE):
        pytest.fail("%s is missing: run build() (make -C consensus_overlord_amd) first" % PROBE)
    return ctypes.CDLL(PROBE)


# ------------------------------------------------------------------------------ the device interpreter
def test_check_programs_on_every_case_on_device(probe):
    g1, g2 = pc.cases()
    want = 2 * sum(c.program for c in g1) + sum(c.program for c in g2)
    assert point_vm.run_single(probe, True) == want


def test_lex_sgn0_program_on_device(probe):
    assert point_vm.run_lex(probe, True) == 20


@pytest.mark.parametrize("name", point_vm.WHOLE)
def test_vote_programs_on_one_case_per_class_on_device(probe, name):
    assert point_vm.run_whole(probe, True, name) >= 6


# ------------------------------------------------------------------------------ the C ABI
def _h(tag, i=0):
    return hashlib.sha256(b"crafted points %s %d" % (tag, i)).digest()


def _sign(sk, h):
    code, sig = orc.sign(sk, h)
    assert code == 0
    return sig


def _ctx(key, **env):
    """A ConsensusCrypto created under the given environment (the context reads it once)."""
    import consensus_overlord_amd as coa
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return coa.ConsensusCrypto(bytes.fromhex(key * 32))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _class_code(c):
    """The code of a vote whose key or signature is case c beside a valid other half: the
    class's parse / group code, or VERIFY_FAIL for a subgroup point (none of them is the
    signer's key or the vote's signature)."""
    return c.code() or 5


class World:
    """Valid votes of NKEYS synthetic keys and one vote per crafted case, on distinct hashes and
    on one shared hash, with the C oracle's codes."""

    def __init__(self):
        g1, g2 = pc.cases()
        self.cases = list(g1) + list(g2)
        self.pks = []
        for sk in SKS:
            code, pk = orc.sk_to_pk(sk)
            assert code == 0
            self.pks.append(pk)
        self.shared = _h(b"round")
        self.distinct = self._votes(lambda i: _h(b"vote", i))
        self.same = self._votes(lambda i: self.shared)

    def _votes(self, hash_of):
        """-> (sigs, hashes, voters, cases): a valid vote before every fourth crafted one"""
        sigs, hs, vs, cs = [], [], [], []
        for i, c in enumerate(self.cases):
            k = i % NKEYS
            if i % 4 == 0:
                h = hash_of(1000 + i)
                sigs.append(_sign(SKS[k], h)), hs.append(h), vs.append(self.pks[k]), cs.append(None)
            h = hash_of(i)
            good = _sign(SKS[k], h)
            sigs.append(good if c.group == 1 else c.enc)
            vs.append(c.enc if c.group == 1 else self.pks[k])
            hs.append(h), cs.append(c)
        n = len(sigs)
        want = orc.verify_many(np.frombuffer(b"".join(sigs), dtype=np.uint8).reshape(n, 96),
                               np.frombuffer(b"".join(hs), dtype=np.uint8).reshape(n, 32),
                               np.frombuffer(b"".join(vs), dtype=np.uint8).reshape(n, 48), threads=4).tolist()
        assert want == [0 if c is None else _class_code(c) for c in cs]
        assert set(want) == {0, 1, 2, 3, 5, 102}
        return sigs, hs, vs, cs, want


@pytest.fixture(scope="module")
def world():
    return World()


@pytest.fixture(scope="module")
def small():
    cc = _ctx("71")
    yield cc
    cc.ctx.close()


@pytest.fixture(scope="module")
def pool():
    cc = _ctx("72", OVH_SMALL_MAX="0")
    yield cc
    cc.ctx.close()


def test_verify_first_call_then_message_cache_hit(world, small):
    """ovh_verify on every crafted vote: the first call on a hash runs vote1 (a miss of the
    message cache), the second one vote1h on the cached H; both answer as the oracle."""
    sigs, hs, vs, cs, want = world.distinct
    h0, m0 = _msg_stats(small)
    n = len(sigs)
    assert n <= 256   # the message table's capacity: no entry of the first pass is evicted
    for rnd in range(2):
        got = [small.lib.ovh_verify(small.ctx.ptr, s, 96, h, 32, v, 48) for s, h, v in zip(sigs, hs, vs)]
        assert got == want, [(c.name if c else "valid", g, w) for c, g, w in zip(cs, got, want) if g != w]
        h1, m1 = _msg_stats(small)
        assert (h1 - h0, m1 - m0) == ((0, n) if rnd == 0 else (n, n))


def test_verify_uncompressed(world, small):
    """k_canon_one: the uncompressed encoding of every crafted point (the one-lane decoder and
    compressor, then vote1) == the oracle == the class's code."""
    for i, c in enumerate(world.cases):
        if c.unc is None:
            continue
        h = _h(b"unc", i)
        good = _sign(SKS[0], h)
        s, v = (good, c.unc) if c.group == 1 else (c.unc, world.pks[0])
        want = orc.verify(s, h, v)
        assert want == _class_code(c), (c.name, want)
        assert small.lib.ovh_verify(small.ctx.ptr, s, len(s), h, 32, v, len(v)) == want, c.name


def _msg_stats(cc):
    st = (ctypes.c_uint64 * 2)()
    assert cc.lib.ovh_msg_cache_stats(cc.ctx.ptr, st) == 0
    return st[0], st[1]


def test_small_batch_path(world):
    """A context that has seen none of the hashes: k_h2f + votew decode the crafted points (no
    part runs on cached H: prime_stats); after prime() of every hash the same batch runs votewh
    on the message table's H (one such part)."""
    sigs, hs, vs, _, want = world.distinct
    assert 2 <= len(sigs) <= 256   # the small-batch size, and the message table holds every hash
    cc = _ctx("74")
    try:
        p0 = cc.prime_stats()
        assert cc.verify_batch(sigs, hs, vs).tolist() == want
        assert cc.prime_stats()[3] == p0[3]
        cc.prime(hs)
        assert cc.verify_batch(sigs, hs, vs).tolist() == want
        assert cc.prime_stats()[3] == p0[3] + 1
    finally:
        cc.ctx.close()


def test_pool_path(world, pool):
    sigs, hs, vs, _, want = world.distinct
    assert pool.verify_batch(sigs, hs, vs).tolist() == want


def test_same_message_path(world):
    sigs, hs, vs, _, want = world.same
    cc = _ctx("73", OVH_SAMEMSG="2")
    try:
        b0 = cc.samemsg_stats()
        assert cc.verify_batch(sigs, hs, vs).tolist() == want
        b1 = cc.samemsg_stats()
        assert (b1[0] - b0[0], b1[1] - b0[1], b1[2] - b0[2]) == (1, len(sigs), 1)
    finally:
        cc.ctx.close()


@pytest.mark.parametrize("which", ["small", "pool"])
def test_validator_table_path(world, which):
    """update_pubkeys with the signers' and every crafted key, in a context of its own that has
    seen none of the hashes: the table's pkchk decodes the keys; the batch (every voter a table
    key, one part) runs votew_t, or vote_t in the pool, on no cached H; the per-call verify then
    runs vote_t1 (every hash a miss of the message table) and vote_t1h (every hash a hit); after
    that the small batch runs votewh_t on the table's H (one part), the pool as before."""
    cc = _ctx("75") if which == "small" else _ctx("76", OVH_SMALL_MAX="0")
    sigs, hs, vs, _, want = world.distinct
    n = len(sigs)
    table = list(world.pks) + sorted({c.enc for c in world.cases if c.group == 1})
    try:
        cc.update_pubkeys(table)
        p0 = cc.prime_stats()
        assert cc.verify_batch(sigs, hs, vs).tolist() == want
        assert cc.prime_stats()[3] == p0[3]
        h0, m0 = _msg_stats(cc)
        for rnd in range(2):
            got = [cc.lib.ovh_verify(cc.ctx.ptr, s, 96, h, 32, v, 48) for s, h, v in zip(sigs, hs, vs)]
            assert got == want
            h1, m1 = _msg_stats(cc)
            assert (h1 - h0, m1 - m0) == ((0, n) if rnd == 0 else (n, n))
        assert cc.verify_batch(sigs, hs, vs).tolist() == want
        assert cc.prime_stats()[3] == p0[3] + (1 if which == "small" else 0)
    finally:
        cc.ctx.close()


def _vagg(cc, agg, h, voters):
    pd, pl = orc._lens(voters)
    return cc.lib.ovh_verify_aggregated(cc.ctx.ptr, agg, len(agg), h, len(h), pd, pl, len(voters))


def test_verify_aggregated_routes(world, small):
    """ovh_verify_aggregated with a crafted point as the aggregate (compressed: qcpre on the VM;
    uncompressed: k_canon_qc first) or among the keys (pkchk, the sum's group check), and with a
    31-byte hash, which the VM route hands to the one-lane k_verify_agg (its decoder answers
    before the hash length does, so its parse codes are checked and its group verdict is not):
    codes == the oracle's."""
    h = world.shared
    signers = world.pks[:3]
    code, agg = orc.aggregate_sigs([_sign(sk, h) for sk in SKS[:3]], signers)
    assert code == 0 and orc.verify_aggregated(agg, h, signers) == 0
    assert _vagg(small, agg, h, signers) == 0
    seen = set()
    for c in world.cases:
        for data in (c.enc, c.unc):
            if data is None:
                continue
            if c.group == 1:
                runs = [(agg, h, signers + [data]), (agg, h, [data])]
            else:
                runs = [(data, h, signers), (data, h[:31], signers)]
            for a, hh, voters in runs:
                want = orc.verify_aggregated(a, hh, voters)
                assert _vagg(small, a, hh, voters) == want, (c.name, len(data), len(hh), want)
                seen.add(want)
                if len(hh) == 31:
                    # the decoder's code comes before the hash length's, and no group check before
                    # either: of k_verify_agg only the parse codes show, not its group verdict
                    assert want == (c.parse or 100), c.name
    assert seen >= {1, 2, 3, 5, 102}


def test_verify_qc_batch(world, small):
    """QCs over a table that holds the crafted keys: a crafted signature as the QC of one signer,
    and a valid signature whose bitmap also names a crafted key."""
    from consensus_overlord_amd import vote
    h = world.shared
    keys = sorted({c.enc for c in world.cases if c.group == 1})
    table = [world.pks[0]] + keys
    skeys = sorted(table)
    nb = (len(table) + 7) // 8

    def bm(voters):
        b = bytearray(nb)
        for v in voters:
            i = skeys.index(v)
            b[i // 8] |= 0x80 >> (i % 8)
        assert vote.extract_voters(table, bytes(b)) == sorted(voters)
        return bytes(b)
    good = _sign(SKS[0], h)
    qcs = [(good, [world.pks[0]])]
    qcs += [(c.enc, [world.pks[0]]) for c in world.cases if c.group == 2]
    qcs += [(good, [world.pks[0], k]) for k in keys]
    want = [orc.verify_aggregated(s, h, sorted(v)) for s, v in qcs]
    assert want[0] == 0 and set(want) >= {0, 1, 2, 3, 5, 102}
    small.update_pubkeys(table)
    try:
        got = small.verify_qc_batch([q[0] for q in qcs], [h] * len(qcs), [bm(q[1]) for q in qcs])
        assert got.tolist() == want
    finally:
        small.update_pubkeys([])


def _agg_sigs(cc, sigs, pks):
    sd, sl = orc._lens(sigs)
    pd, pl = orc._lens(pks)
    out = ctypes.create_string_buffer(96)
    c = cc.lib.ovh_aggregate_sigs(cc.ctx.ptr, sd, sl, len(sigs), pd, pl, len(pks), out)
    return c, (out.raw if c == 0 else None)


def test_aggregate_sigs(world, small):
    """ovh_aggregate_sigs with a crafted signature, compressed (sigchk on the VM) and
    uncompressed (k_canon_sig_list), between two valid ones: code and bytes == the oracle's."""
    h = world.shared
    a, b = _sign(SKS[0], h), _sign(SKS[1], h)
    codes = set()
    for c in world.cases:
        if c.group != 2:
            continue
        for data in (c.enc, c.unc):
            if data is None:
                continue
            want = orc.aggregate_sigs([a, data, b], world.pks[:3])
            assert _agg_sigs(small, [a, data, b], world.pks[:3]) == want, (c.name, len(data), want[0])
            codes.add(want[0])
    assert codes >= {0, 1, 2, 3}


def _agg_pks(cc, keys):
    pd, pl = orc._lens(keys)
    out = ctypes.create_string_buffer(48)
    c = cc.lib.ovh_aggregate_pks(cc.ctx.ptr, pd, pl, len(keys), out)
    return c, (out.raw if c == 0 else None)


def test_aggregate_pks_round_trip(world, small, golden):
    """ovh_aggregate_pks does not group-check, so the decoded sign shows in its bytes: a single
    on-curve key comes back byte-identical, {K, golden key}, K between two valid keys and
    {K, -K} == the oracle's bytes and code; every lex-boundary and small-order key among them,
    and both encodings."""
    gk = bytes.fromhex(golden["keys"][0]["pk"])
    classes = set()
    for c in world.cases:
        if c.group != 1:
            continue
        neg = bytes([c.enc[0] ^ 0x20]) + c.enc[1:]
        for data in (c.enc, c.unc):
            if data is None:
                continue
            one = _agg_pks(small, [data])
            assert one == orc.aggregate_pks([data]), (c.name, len(data))
            if c.parse == 0:
                assert one == (0, c.enc), c.name
                classes.add(c.cls)
            for keys in ([data, gk], [gk, data], [world.pks[1], data, world.pks[2]], [data, neg]):
                assert _agg_pks(small, keys) == orc.aggregate_pks(keys), (c.name, len(data), len(keys))
        if c.parse == 0:
            assert orc.aggregate_pks([c.enc, neg]) == (0, bytes([0xC0]) + bytes(47)), c.name
    assert classes >= {"both_flags", "lex_boundary", "extreme_x", "small_order", "in_group"}
