"""The vote pool's one interpreter loop for both vote programs (ovhip.hip vote_quad, DESIGN.md
section 4.7): batches whose keys come as bytes (program `vote`) and batches whose keys are in the
validator table (program `vote_t`) alternate in ONE context with no wait between them, so the
same persistent workgroups run quads of either kind back to back through the shared loop -- slot
count, stride, phase count, maps, code and side words all chosen per quad.

Sizes n = 1, 4 and 5: one slice of a quad, a full quad, a quad plus a one-slice quad. Every batch
has one invalid vote, a wrong signature in one kind and a key outside G1 in the other; the codes
are the C oracle's, in both orders of the two kinds.

The context is created with OVH_SMALL_MAX=0, so every size takes the pool. Key-bytes batches go
through ovh_verify_batch_device_async. That call never consults the validator table; table batches
reach the pool through the pipelined host form, ovh_verify_batch_async, which splits a batch into
its table votes and the others and enqueues each part as a pool batch of its own. Its one-vote
batches take the per-call path, so the n = 1 table batch is the table part of a two-vote batch
(the other part: one more key-bytes batch of one vote)."""
import os

import numpy as np
import pytest

import synth_votes as sv

pytestmark = pytest.mark.gpu

SIZES = (1, 4, 5)
NT = 6   # validators: table votes 0..4 and, last, the key outside G1


@pytest.fixture(scope="module")
def setup(golden):
    import consensus_overlord_amd as coa
    from consensus_overlord_amd.crypto import Context
    old = os.environ.get("OVH_SMALL_MAX")
    os.environ["OVH_SMALL_MAX"] = "0"
    try:
        cc = coa.ConsensusCrypto(bytes.fromhex("5a" * 32), ctx=Context(0))
    finally:
        if old is None:
            os.environ.pop("OVH_SMALL_MAX", None)
        else:
            os.environ["OVH_SMALL_MAX"] = old
    s, h, p = sv.make(cc.ctx, 12, lo=91000)
    not_g1 = np.frombuffer(bytes.fromhex([x for x in golden["verify"] if x["name"] == "pk_not_in_g1"][0]["pk"]),
                           dtype=np.uint8)
    # validators: the keys of votes 0..4 and the key outside G1; votes 6..11 stay key-bytes votes
    cc.update_pubkeys([bytes(p[i]) for i in range(NT - 1)] + [bytes(not_g1)])
    yield cc, s, h, p, not_g1
    cc.ctx.close()


def _batch(s, h, p, idx, wrong_sig, key):
    """Votes idx with the last one made invalid: sigma + G2 (wrong_sig) or the voter key `key`."""
    bs, bh, bp = s[idx].copy(), h[idx].copy(), p[idx].copy()
    if wrong_sig:
        bs[-1] = np.frombuffer(sv.add_g2(bytes(bs[-1])), dtype=np.uint8)
    else:
        bp[-1] = key
    return bs, bh, bp


@pytest.mark.parametrize("bytes_first", [True, False], ids=["bytes_then_table", "table_then_bytes"])
def test_alternating_vote_and_vote_t_batches(setup, bytes_first):
    import torch
    from consensus_overlord_amd import device as dev
    cc, s, h, p, not_g1 = setup
    # the first kind of the order gets the key outside G1, the second the wrong signature
    jobs = []
    for n in SIZES:
        # key-bytes votes 6.., with a key that is in no table (a key outside G1 that IS a validator
        # would make the host form route the vote to the table; the device form never does)
        kb = _batch(s, h, p, np.arange(6, 6 + n), wrong_sig=not bytes_first, key=not_g1)
        # table votes 0..n-1; the invalid one's key becomes the table's last entry, outside G1
        tb = _batch(s, h, p, np.arange(0, n), wrong_sig=bytes_first, key=not_g1)
        if n == 1:   # + one key-bytes vote, so the table part is a pool batch of one vote
            tb = tuple(np.concatenate([a, b[11:12]]) for a, b in zip(tb, (s, h, p)))
        jobs.append((kb, tb))
    want = [(sv.oracle_codes(*kb), sv.oracle_codes(*tb)) for kb, tb in jobs]
    for (wk, wt), n in zip(want, SIZES):   # one invalid vote per batch, of the intended kind
        assert (wk != 0).sum() == 1 and (wt != 0).sum() == 1, (n, wk, wt)
        assert {int(wk[n - 1]), int(wt[n - 1])} == {3, 5}, (n, wk, wt)

    d_in = [tuple(torch.from_numpy(a).cuda() for a in kb) for kb, _ in jobs]
    d_codes = [torch.full((len(kb[0]),), -1, dtype=torch.int32, device="cuda") for kb, _ in jobs]
    h_codes = [np.full(len(tb[0]), -1, dtype=np.int32) for _, tb in jobs]
    torch.cuda.synchronize()
    for k, (_, tb) in enumerate(jobs):   # enqueued back to back: nothing waits before cc.wait()
        def table():
            cc.verify_batch_async([bytes(x) for x in tb[0]], [bytes(x) for x in tb[1]],
                                  [bytes(x) for x in tb[2]], h_codes[k])

        def keyed():
            dev.verify_batch_async(cc.ctx, d_in[k][0], d_in[k][1], d_in[k][2], d_codes[k])
        for f in ((keyed, table) if bytes_first else (table, keyed)):
            f()
    cc.wait()
    torch.cuda.synchronize()
    for k, n in enumerate(SIZES):
        print(n, "keyed", d_codes[k].cpu().numpy().tolist(), want[k][0].tolist(),
              "table", h_codes[k].tolist(), want[k][1].tolist())
    for k, n in enumerate(SIZES):
        assert d_codes[k].cpu().numpy().tolist() == want[k][0].tolist(), ("keyed", n)
        assert h_codes[k].tolist() == want[k][1].tolist(), ("table", n)
