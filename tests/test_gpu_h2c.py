"""hash_to_G2 on the GPU away from the default DST and from SHA-256-made field elements
(tests/h2c_cases.py; the host build runs the same cases in tests/test_h2c_host.py):

- the probe's dp_h2f (tests/device/fp_probe.hip: k_h2f's shape, XmdTemplates by value in the
  kernel arguments) for every DST length 0 .. 255 against the Python oracle's hash_to_field;
- the VM programs on the exceptional field inputs through the device interpreter against the
  simulator;
- contexts created under DSTs of every block-count class, every k_h2f launch site and
  k_verify_agg's templates under a 1-byte and a 255-byte DST, a multi-device context, and the
  refusal of longer DSTs -- codes and signature bytes against the C oracle set to the same DST."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

import bls12_381 as bls
import h2c_cases as hc
import orc
import overlord_oracle as ov
import qc_groups_model
import synth_votes as sv
from test_gpu_build_qc import _verify_code
from vm_helpers import ROOT, _int, assert_same, build_all, run_vm

pytestmark = pytest.mark.gpu

PROBE = os.path.join(ROOT, "tests", "device", "_build", "libfpprobe.so")
R = pow(2, 384, hc.P)
NKEYS = 5
SKS = [ov.synth_sk(0xD57000 + i).to_bytes(32, "big") for i in range(NKEYS)]
CLASS_LENGTHS = [0, 19, 20, 22, 84, 86, 148, 150, 211, 212, 214, 255]


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(PROBE):
        pytest.fail("%s is missing: run build() (make -C consensus_overlord_amd) first" % PROBE)
    return ctypes.CDLL(PROBE)


@pytest.fixture(scope="module")
def pks():
    out = []
    for sk in SKS:
        code, pk = orc.sk_to_pk(sk)
        assert code == 0
        out.append(pk)
    return out


def _h(tag, i=0):
    return hashlib.sha256(b"h2c dst %s %d" % (tag, i)).digest()


def _sign(o, sk, h):
    code, sig = o.sign(sk, h)
    assert code == 0
    return sig


def _codes(o, sigs, hs, voters):
    n = len(sigs)
    return o.verify_many(np.frombuffer(b"".join(sigs), dtype=np.uint8).reshape(n, 96),
                         np.frombuffer(b"".join(hs), dtype=np.uint8).reshape(n, 32),
                         np.frombuffer(b"".join(voters), dtype=np.uint8).reshape(n, 48), threads=4).tolist()


def _crypto(dst, small=True, **kw):
    """A ConsensusCrypto on key 0 (raw scalar) under `dst`; small=False: a context that skips the
    small-batch path (created under OVH_SMALL_MAX=0), so batches go to the vote pool."""
    import consensus_overlord_amd as coa
    from consensus_overlord_amd.crypto import FLAG_SK_RAW, Context
    old = os.environ.get("OVH_SMALL_MAX")
    if not small:
        os.environ["OVH_SMALL_MAX"] = "0"
    try:
        return coa.ConsensusCrypto(SKS[0], ctx=Context(dst=dst, flags=FLAG_SK_RAW, **kw))
    finally:
        if old is None:
            os.environ.pop("OVH_SMALL_MAX", None)
        else:
            os.environ["OVH_SMALL_MAX"] = old


# ------------------------------------------------------------------------------ D.1: hash_to_field
def test_h2f_every_dst_length_on_device(probe):
    """dp_h2f once per DST length 0 .. 255 on 65 messages (one full wave and a second workgroup's
    single lane): every stored limb vector is below p and equals the Python oracle's
    hash_to_field value in Montgomery form; the templates' block counts are the class's."""
    u8p, u32p = ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32)
    probe.dp_h2f.argtypes = [ctypes.c_uint32, u8p, u8p, ctypes.c_size_t, u32p, u32p]
    n = 65
    msgs = hc.MESSAGES + [_h(b"msg", i) for i in range(n - len(hc.MESSAGES))]
    cat = b"".join(msgs)
    bad = []
    for L in range(256):
        dst = hc.dst_for(L)
        out = np.zeros(n * 48, dtype=np.uint32)
        nb = (ctypes.c_uint32 * 2)()
        err = probe.dp_h2f(n, cat, dst, L, out.ctypes.data_as(u32p), nb)
        assert err == 0, "dp_h2f: HIP error %d at L = %d" % (err, L)
        assert tuple(nb) == hc.nb_of(L), L
        for i, msg in enumerate(msgs):
            (a0, a1), (b0, b1) = bls.hash_to_field_fp2(msg, dst, 2)
            for j, want in enumerate((a0, a1, b0, b1)):
                got = _int(out[(i * 4 + j) * 12:(i * 4 + j) * 12 + 12])
                if got >= hc.P or got != want * R % hc.P:
                    bad.append((L, i, j, hex(got)))
    assert not bad, "%d values differ, first: %s" % (len(bad), bad[:4])
    # refused without a launch, as ovh_create refuses them
    out = np.zeros(48, dtype=np.uint32)
    assert probe.dp_h2f(1, cat, bytes(256), 256, out.ctypes.data_as(u32p), None) != 0
    assert probe.dp_h2f(1, cat, hc.DEFAULT_DST, 2 ** 32 + 43, out.ctypes.data_as(u32p), None) != 0


# ------------------------------------------------------------------------------ D.2: VM programs
def test_vm_programs_exceptional_inputs_on_device(probe):
    """h2g on the nine u cases, vote / qcpre / votew on (b), (e), (f), on one wave of the device
    interpreter == the simulator (which tests/test_h2c_host.py ties to the oracle)."""
    consts, progs_ = build_all()
    for name, case, inp, r, sim in hc.vm_runs():
        _, sc, words, _, _ = progs_[name]
        assert sim["h_inf"] == (1 if case == "f" else 0)
        assert_same(run_vm(probe, consts, sc, words, inp, r, 0, device=True), sim, "%s case %s" % (name, case))


# ------------------------------------------------------------------------------ D.3: one context per class
@pytest.mark.parametrize("L", CLASS_LENGTHS)
def test_context_per_dst_class(pks, L):
    """A context under a DST of each (nb0, nbi) class: sign == the oracle's signature under that
    DST byte for byte, it verifies, a signature made under the default DST gets 5, and a 3-vote
    batch [good, default-DST signature, good] returns [0, 5, 0]."""
    dst = hc.dst_for(L)
    hs = [_h(b"class", k) for k in range(3)]
    default_sigs = [_sign(orc, SKS[k], hs[k]) for k in range(3)]
    with hc.orc_dst(dst) as o:
        sigs = [_sign(o, SKS[k], hs[k]) for k in range(3)]
        mixed = [sigs[0], default_sigs[1], sigs[2]]
        want = _codes(o, mixed, hs, pks[:3])
        assert o.verify(default_sigs[0], hs[0], pks[0]) == 5
    assert want == [0, 5, 0]
    assert sigs[0] != default_sigs[0]
    cc = _crypto(dst)
    try:
        assert cc.name == pks[0]
        assert cc.sign(hs[0]) == sigs[0]
        assert _verify_code(cc, sigs[0], hs[0], pks[0]) == 0
        assert _verify_code(cc, default_sigs[0], hs[0], pks[0]) == 5
        assert cc.verify_batch(mixed, hs, pks[:3]).tolist() == want
    finally:
        cc.ctx.close()


# ------------------------------------------------------------------------------ D.4: every launch site
class Site:
    """The oracle's votes and verdicts under one DST, and the two contexts."""

    def __init__(self, L, pks):
        self.L, self.dst, self.pks = L, hc.dst_for(L), pks
        self.hs = [_h(b"site%d" % L, k) for k in range(NKEYS)]
        self.hA, self.hB, self.hC = (_h(b"site%d round" % L, k) for k in range(3))
        with hc.orc_dst(self.dst) as o:
            # five votes on distinct hashes, vote 3 invalid (sigma + G2)
            self.sigs = [_sign(o, SKS[k], self.hs[k]) for k in range(NKEYS)]
            self.sigs[3] = sv.add_g2(self.sigs[3])
            self.codes = _codes(o, self.sigs, self.hs, pks)
            # every key on hA and on hB; keys 0, 1 on hC
            self.sA = [_sign(o, SKS[k], self.hA) for k in range(NKEYS)]
            self.sB = [_sign(o, SKS[k], self.hB) for k in range(NKEYS)]
            self.sC = [_sign(o, SKS[k], self.hC) for k in range(2)]
        assert self.codes == [0, 0, 0, 5, 0]
        self.small = _crypto(self.dst)
        self.pool = _crypto(self.dst, small=False)

    def oracle(self):
        return hc.orc_dst(self.dst)

    def close(self):
        self.small.ctx.close()
        self.pool.ctx.close()


@pytest.fixture(scope="module", params=[1, 255])
def site(request, pks):
    s = Site(request.param, pks)
    yield s
    s.close()


def test_small_batch_path(site):
    """verify_small_locked's k_h2f (5 votes on distinct hashes, one invalid), and enqueue_sign's."""
    assert site.small.verify_batch(site.sigs, site.hs, site.pks).tolist() == site.codes
    assert site.small.sign(site.hs[0]) == site.sigs[0]


def test_pool_path(site):
    """batch_front's k_h2f: the same votes in a context that skips the small-batch path."""
    assert site.pool.verify_batch(site.sigs, site.hs, site.pks).tolist() == site.codes


def test_message_cache_hit(site):
    """verify_signature on hC misses (k_h2f of one hash, the h2g-carrying program), the next vote
    on hC runs vote1h on the cached H: both answer as the oracle under this DST."""
    cc = site.small
    st = (ctypes.c_uint64 * 2)()
    assert cc.lib.ovh_msg_cache_stats(cc.ctx.ptr, st) == 0
    h0, m0 = st[0], st[1]
    with site.oracle() as o:
        want = [o.verify(site.sC[0], site.hC, site.pks[0]), o.verify(site.sC[1], site.hC, site.pks[1]),
                o.verify(site.sC[0], site.hC, site.pks[1])]
    assert want == [0, 0, 5]
    assert _verify_code(cc, site.sC[0], site.hC, site.pks[0]) == 0
    assert _verify_code(cc, site.sC[1], site.hC, site.pks[1]) == 0
    assert _verify_code(cc, site.sC[0], site.hC, site.pks[1]) == 5
    assert cc.lib.ovh_msg_cache_stats(cc.ctx.ptr, st) == 0
    assert (st[0] - h0, st[1] - m0) == (2, 1)


def test_verify_aggregated(site):
    """verify_aggregated_signature over 4 keys (k_h2f on the side stream, qcpre / qcmil), and with
    one wrong key: code 5, as the oracle."""
    from consensus_overlord_amd.crypto import CryptoErr
    with site.oracle() as o:
        code, agg = o.aggregate_sigs(site.sA[:4], site.pks[:4])
        assert code == 0
        wrong = site.pks[:3] + [site.pks[4]]
        assert o.verify_aggregated(agg, site.hA, site.pks[:4]) == 0
        assert o.verify_aggregated(agg, site.hA, wrong) == 5
    for cc in (site.small, site.pool):
        assert cc.aggregate_signatures(site.sA[:4], site.pks[:4]) == agg
        cc.verify_aggregated_signature(agg, site.hA, site.pks[:4])
        with pytest.raises(CryptoErr) as ei:
            cc.verify_aggregated_signature(agg, site.hA, wrong)
        assert ei.value.code == 5


def test_verify_qc_batch(site):
    """Two QCs over a 4-key table (all four keys on hA, the first three of the sorted table on
    hB), then the pair with the second bitmap naming a key that did not sign: [0, 0], [0, 5]."""
    from consensus_overlord_amd import vote
    table = site.pks[:4]
    order = sorted(range(4), key=lambda k: table[k])
    three = order[:3]
    bm4, bm3 = bytes([0xF0]), bytes([0xE0])
    assert vote.extract_voters(table, bm3) == [table[k] for k in three]
    with site.oracle() as o:
        _, qa = o.aggregate_sigs(site.sA[:4], table)
        _, qb = o.aggregate_sigs([site.sB[k] for k in three], [table[k] for k in three])
        want = [o.verify_aggregated(qa, site.hA, vote.extract_voters(table, bm4)),
                o.verify_aggregated(qb, site.hB, vote.extract_voters(table, bm3)),
                o.verify_aggregated(qb, site.hB, vote.extract_voters(table, bm4))]
    assert want == [0, 0, 5]
    cc = site.small
    cc.update_pubkeys(table)
    try:
        assert cc.verify_qc_batch([qa, qb], [site.hA, site.hB], [bm4, bm3]).tolist() == want[:2]
        assert cc.verify_qc_batch([qa, qb], [site.hA, site.hB], [bm4, bm4]).tolist() == [0, 5]
    finally:
        cc.update_pubkeys([])


def test_build_qcs_two_hashes(site):
    """build_qcs with 6 votes on two hashes (the same-message path and its per-group k_h2f):
    codes, grouping, bitmaps and both aggregates equal the oracle's under this DST."""
    table = site.pks[:4]
    sigs = [site.sA[0], site.sB[0], site.sA[1], site.sB[1], site.sA[2], sv.add_g2(site.sB[2])]
    hashes = [site.hA, site.hB] * 3
    voters = [site.pks[0], site.pks[0], site.pks[1], site.pks[1], site.pks[2], site.pks[2]]
    cc = site.small
    cc.update_pubkeys(table)
    try:
        with site.oracle() as o:
            want = np.array(_codes(o, sigs, hashes, voters), dtype=np.int32)
            assert want.tolist() == [0, 0, 0, 0, 0, 5]
            m_group, m_gh, m_taken, m_bm, m_cnt = qc_groups_model.select(want, hashes, voters, table)
            aggs = []
            for g in range(2):
                idx = [i for i in range(6) if m_group[i] == g and m_taken[i]]
                code, agg = o.aggregate_sigs([sigs[i] for i in idx], [voters[i] for i in idx])
                assert code == 0
                aggs.append(agg)
        qcs, codes, taken, group = cc.build_qcs(sigs, hashes, voters)
        assert codes.tolist() == want.tolist()
        assert group.tolist() == m_group and taken.astype(int).tolist() == m_taken
        assert m_cnt == [3, 2]
        assert [(q[0], q[1], q[2], q[3]) for q in qcs] == list(zip(m_gh, aggs, m_bm, m_cnt))
    finally:
        cc.update_pubkeys([])


# ------------------------------------------------------------------------------ D.5: multi-device
def test_multi_device_context_with_dst(pks):
    """ovh_create_multi's root object builds no templates of its own (only the sub-contexts do):
    sign, verify_signature and a 5-vote batch under an 86-byte DST through Context(devices=[0, 0])
    answer as the oracle, so no entry point reads the root's."""
    dst = hc.dst_for(86)
    hs = [_h(b"multi", k) for k in range(NKEYS)]
    with hc.orc_dst(dst) as o:
        sigs = [_sign(o, SKS[k], hs[k]) for k in range(NKEYS)]
        sigs[1] = sv.add_g2(sigs[1])
        want = _codes(o, sigs, hs, pks)
        s0 = _sign(o, SKS[0], hs[4])
    assert want == [0, 5, 0, 0, 0]
    mc = _crypto(dst, devices=[0, 0])
    try:
        assert mc.ctx.device_count == 2
        assert mc.sign(hs[4]) == s0
        assert _verify_code(mc, s0, hs[4], pks[0]) == 0
        assert _verify_code(mc, sigs[1], hs[1], pks[1]) == 5
        assert mc.verify_batch(sigs, hs, pks).tolist() == want
    finally:
        mc.ctx.close()


# ------------------------------------------------------------------------------ D.6: refusals
def test_oversize_dst_refused(golden):
    """ovh_create returns NULL for a 256-byte DST and for dst_len = 2^32 + 43 over a 43-byte
    buffer (no truncation to the default's length); the context created next verifies a golden
    vote; the Python Context raises ValueError before it calls the library."""
    import consensus_overlord_amd as coa
    from consensus_overlord_amd import _lib
    from consensus_overlord_amd.crypto import Context
    lib = _lib.load()
    assert not lib.ovh_create(0, bytes(256), 256, 0)
    assert not lib.ovh_create(0, hc.DEFAULT_DST, 2 ** 32 + 43, 0)
    assert not lib.ovh_create_multi((ctypes.c_int * 2)(0, 0), 2, bytes(300), 300, 0)
    with pytest.raises(ValueError):
        Context(dst=bytes(256))
    with pytest.raises(ValueError):
        Context(devices=[0, 0], dst=bytes(256))
    cc = coa.ConsensusCrypto(bytes.fromhex("7d" * 32), ctx=Context())
    try:
        v, k = golden["votes"][0], golden["keys"][0]
        assert _verify_code(cc, bytes.fromhex(v["sig"]), bytes.fromhex(v["digest"]), bytes.fromhex(k["pk"])) == 0
        other = golden["votes"][1]
        assert _verify_code(cc, bytes.fromhex(other["sig"]), bytes.fromhex(v["digest"]), bytes.fromhex(k["pk"])) == 5
    finally:
        cc.ctx.close()
