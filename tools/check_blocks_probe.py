#!/usr/bin/env python
"""ovh_check_blocks against the Python composition it replaces, and the bulk SM3 against the host
SM3, on one context with 100 validators, 67 of them signing every QC:
  arm 1   check_blocks       ConsensusCrypto.check_blocks: per block a host SM3 of the proposal
                             bytes and a Python proof decode, then ovh_vote_digests and
                             ovh_verify_qc_batch (two host round trips)
          check_block_batch  one ovh_check_blocks call (SM3, gate, vote digests, QC batch on the
                             device behind one synchronisation)
  arm 2   sm3_batch          one ovh_sm3_batch call over the 256 proposals (host buffers in and out)
          sm3_host           ovh_sm3 in a host loop over the same proposals
for 256 valid blocks of 256 B, 4 KB and 64 KB of proposal data, in several interleaved rounds (a
round = every size, each path REPS times in turn). Prints one JSON line per round and size, then
a summary line per size (median, min, max over the rounds' medians; GB/s of the proposal bytes).
   python tools/check_blocks_probe.py [--rounds 5] [--reps 5]"""
import argparse
import ctypes
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (256, 4096, 65536)
BLOCKS = 256
N_VAL, N_SIGN = 100, 67


def _ms(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def make_blocks(cc, ctx, sks, pks, size):
    """BLOCKS valid (height, data, proof) tuples: the QCs signed and aggregated on the device."""
    import torch
    from consensus_overlord_amd import device as dev
    from consensus_overlord_amd import vote
    rng = np.random.default_rng(size)
    order = {pk: i for i, pk in enumerate(sorted(pks))}
    datas = [rng.integers(0, 256, size, dtype=np.uint8).tobytes() for _ in range(BLOCKS)]
    bhs = cc.hash_batch(datas)
    assert bhs[0] == hashlib.new("sm3", datas[0]).digest()
    vhs = cc.vote_digests([(1000 + j, j % 4, vote.PRECOMMIT, bhs[j]) for j in range(BLOCKS)])
    d_sks = torch.from_numpy(np.tile(sks[:N_SIGN], (BLOCKS, 1))).cuda()
    d_hs = torch.from_numpy(np.repeat(np.frombuffer(b"".join(vhs), dtype=np.uint8).reshape(BLOCKS, 32), N_SIGN, axis=0)).cuda()
    sigs = dev.sign_batch(ctx, d_sks, d_hs).cpu().numpy().reshape(BLOCKS, N_SIGN, 96)
    bm = bytearray((N_VAL + 7) // 8)
    for pk in pks[:N_SIGN]:
        bm[order[pk] // 8] |= 0x80 >> (order[pk] % 8)
    blocks = []
    for j in range(BLOCKS):
        agg = cc.aggregate_signatures([s.tobytes() for s in sigs[j]], pks[:N_SIGN])
        blocks.append((1000 + j, datas[j], vote.encode_proof(1000 + j, j % 4, bhs[j], agg, bytes(bm))))
    return blocks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    import bench
    from consensus_overlord_amd import device as dev
    from consensus_overlord_amd.crypto import ConsensusCrypto, Context
    ctx = Context(0)
    lib = ctx.lib
    cc = ConsensusCrypto(hashlib.sha256(b"check_blocks probe").digest(), ctx=ctx)
    sks, _ = bench.synth_inputs(lib, 0, N_VAL)
    pk = dev.sk_to_pk_batch(ctx, torch.from_numpy(sks).cuda()).cpu().numpy()
    pks = [pk[i].tobytes() for i in range(N_VAL)]
    cc.update_pubkeys(pks)
    blocks = {size: make_blocks(cc, ctx, sks, pks, size) for size in SIZES}
    keys = ("check_blocks_ms", "check_block_batch_ms", "sm3_batch_ms", "sm3_host_ms")
    rows = {size: [] for size in SIZES}
    out32 = ctypes.create_string_buffer(32)
    for rnd in range(args.rounds + 1):          # round 0 warms every path up and is not recorded
        for size in SIZES:
            bl = blocks[size]
            datas = [b[1] for b in bl]
            got = {}

            def composed():
                got["py"] = cc.check_blocks(bl)

            def one_pass():
                got["ok"], got["why"] = cc.check_block_batch(bl)

            def sm3_batch():
                got["dig"] = cc.hash_batch(datas)

            def sm3_host():
                for m in datas:
                    lib.ovh_sm3(m, len(m), out32)

            t = {k: [] for k in keys}
            for _ in range(args.reps):
                t["check_blocks_ms"].append(_ms(composed))
                t["check_block_batch_ms"].append(_ms(one_pass))
                assert got["py"].all() and got["ok"].all() and not got["why"].any()
                t["sm3_batch_ms"].append(_ms(sm3_batch))
                t["sm3_host_ms"].append(_ms(sm3_host))
                assert got["dig"][-1] == out32.raw
            row = {k: round(float(np.median(v)), 4) for k, v in t.items()}
            if rnd:
                rows[size].append(row)
                print(json.dumps({"round": rnd, "bytes": size, **row}), flush=True)
    for size in SIZES:
        s = {"bytes": size, "blocks": BLOCKS, "rounds": args.rounds, "reps": args.reps}
        for k in keys:
            v = [r[k] for r in rows[size]]
            s[k] = {"median": round(float(np.median(v)), 4), "min": min(v), "max": max(v)}
        gb = size * BLOCKS / 1e9
        for k in ("sm3_batch", "sm3_host"):
            s[k + "_GBps"] = round(gb / (s[k + "_ms"]["median"] * 1e-3), 4)
        print(json.dumps({"summary": s}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
