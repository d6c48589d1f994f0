"""The vote pool on its radix-2^392 programs (ovhip/pool.hpp vote_quad: vm::run<.., 392> on `vote`
and `vote_t`, which convert at their own edges): batches of n = 5 (two quads, the second with one
active slice and three inactive) and n = 4 (one full quad) through the pool -- the context is
created with OVH_SMALL_MAX=0 -- once with the keys as bytes (ovh_verify_batch_device, program
`vote`) and once with every key in the validator table (the host form, program `vote_t`).

The two batches mix valid votes with one vote of each failure kind the C oracle distinguishes:
bad key encoding (102), key outside G1 (3), bad signature encoding (1), signature off the curve
(2), signature outside G2 (3) and a wrong signature (sigma + G2: 5, found by the combined check
and its bisection). The per-vote codes are exactly the oracle's, so the bisection flags the wrong
signature and nothing else. This is the smallest shape that runs the input conversions, the
conversion of the stored f, sigma and tau into the fold / MSM / final planes (all still
value * 2^384) and a partial quad."""
import os

import numpy as np
import pytest

import synth_votes as sv

pytestmark = pytest.mark.gpu


def _named(golden, name, field):
    return np.frombuffer(bytes.fromhex([x for x in golden["verify"] if x["name"] == name][0][field]), dtype=np.uint8)


@pytest.fixture(scope="module")
def setup(golden):
    import consensus_overlord_amd as coa
    from consensus_overlord_amd.crypto import Context
    old = os.environ.get("OVH_SMALL_MAX")
    os.environ["OVH_SMALL_MAX"] = "0"
    try:
        cc = coa.ConsensusCrypto(bytes.fromhex("5b" * 32), ctx=Context(0))
    finally:
        if old is None:
            os.environ.pop("OVH_SMALL_MAX", None)
        else:
            os.environ["OVH_SMALL_MAX"] = old
    s, h, p = sv.make(cc.ctx, 9, lo=93000)
    s, h, p = s.copy(), h.copy(), p.copy()
    # batch A = votes 0..4: valid, bad key encoding, signature off the curve, wrong signature, valid
    p[1] = _named(golden, "pk_compressed_bit_clear", "pk")
    s[2] = _named(golden, "sig_not_on_curve", "sig")
    s[3] = np.frombuffer(sv.add_g2(bytes(s[3])), dtype=np.uint8)
    # batch B = votes 5..8: key outside G1, bad signature encoding, signature outside G2, valid
    p[5] = _named(golden, "pk_not_in_g1", "pk")
    s[6] = _named(golden, "sig_compressed_bit_clear", "sig")
    s[7] = _named(golden, "sig_not_in_g2", "sig")
    batches = [tuple(a[0:5] for a in (s, h, p)), tuple(a[5:9] for a in (s, h, p))]
    want = [sv.oracle_codes(*b) for b in batches]
    assert want[0].tolist() == [0, 102, 2, 5, 0] and want[1].tolist() == [3, 1, 3, 0], (want[0], want[1])
    yield cc, batches, want
    cc.ctx.close()


@pytest.mark.parametrize("k", [0, 1], ids=["n5", "n4"])
def test_key_bytes_batches(setup, k):
    """program `vote` (ovh_verify_batch_device)"""
    import torch
    from consensus_overlord_amd import device as dev
    cc, batches, want = setup
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in batches[k]]
    codes = torch.full((len(batches[k][0]),), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dev.verify_batch(cc.ctx, d[0], d[1], d[2], codes)
    torch.cuda.synchronize()
    got = codes.cpu().numpy().tolist()
    print(got, want[k].tolist())
    assert got == want[k].tolist()


def test_table_batches(setup):
    """program `vote_t`: every voter key, the two bad ones included, is a validator-table entry"""
    cc, batches, want = setup
    cc.update_pubkeys([bytes(x) for b in batches for x in b[2]])
    for k, b in enumerate(batches):
        codes = np.full(len(b[0]), -1, dtype=np.int32)
        cc.verify_batch_async([bytes(x) for x in b[0]], [bytes(x) for x in b[1]], [bytes(x) for x in b[2]], codes)
        cc.wait()
        print(codes.tolist(), want[k].tolist())
        assert codes.tolist() == want[k].tolist(), k
