#!/usr/bin/env python
"""What the validator update of a committed block costs, on one context,
for tables of 67 and 1,024 keys with four rounds open (each holding one taken vote), three arms:
  set_same      ovh_set_validators with the list the table holds: today's update_pubkeys, which
                uploads and checks every key again and closes the rounds (they are opened again,
                outside the timer, before the next call)
  update_same   ovh_update_validators with the same list: the every-block case
  update_swap   ovh_update_validators with one key swapped for one the table does not hold (the
                lists alternate, so every call finds exactly one new key); the swapped key has not
                voted, so the four rounds are carried over
The median of --reps calls (default 50) after --warmup calls (default 5), in microseconds, and the
counters of ovh_table_stats at the end. Prints one JSON line.
  python tools/bench_table_update.py [--reps 50] [--warmup 5]"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TABLES = (67, 1024)
ROUNDS = 4


def _us(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e6


def _scalars(n):
    # 32-byte secrets below the group order (the top three bits clear)
    ds = [hashlib.sha256(b"table update %d" % i).digest() for i in range(n)]
    return np.frombuffer(b"".join(bytes([d[0] >> 3]) + d[1:] for d in ds), dtype=np.uint8).reshape(n, 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch

    import consensus_overlord_amd as coa
    from consensus_overlord_amd import device as dev

    cc = coa.ConsensusCrypto(bytes.fromhex("5e" * 32))
    hashes = [hashlib.sha256(b"table update round %d" % k).digest() for k in range(ROUNDS)]
    out = {"tool": "bench_table_update", "device": torch.cuda.get_device_name(0), "rounds_open": ROUNDS,
           "reps": args.reps, "warmup": args.warmup, "unit": "us", "tables": {}}
    for n in TABLES:
        sks = torch.from_numpy(_scalars(n + 1).copy()).cuda()
        pks = [bytes(p) for p in dev.sk_to_pk_batch(cc.ctx, sks).cpu().numpy()]
        # the first ROUNDS validators vote, one per round
        hs = torch.from_numpy(np.frombuffer(b"".join(hashes), dtype=np.uint8).reshape(ROUNDS, 32).copy()).cuda()
        sigs = [bytes(s) for s in dev.sign_batch(cc.ctx, sks[:ROUNDS], hs).cpu().numpy()]
        base, swapped = pks[:n], pks[:n - 1] + [pks[n]]
        rounds = []

        def open_rounds():
            for r in rounds:
                r.close()
            rounds[:] = [cc.open_round(h) for h in hashes]
            for k, r in enumerate(rounds):
                assert r.add([sigs[k]], [pks[k]])[2] == 1

        def arm(name):
            ts = []
            for i in range(args.warmup + args.reps):
                if name == "set_same":
                    open_rounds()
                    t = _us(lambda: cc.update_pubkeys(base))
                elif name == "update_same":
                    t = _us(lambda: cc.update_pubkeys(base, keep_rounds=True))
                else:
                    keys = swapped if i % 2 == 0 else base
                    t = _us(lambda: cc.update_pubkeys(keys, keep_rounds=True))
                if i >= args.warmup:
                    ts.append(t)
            return {"median": round(statistics.median(ts), 1), "min": round(min(ts), 1), "max": round(max(ts), 1)}

        res = {}
        cc.update_pubkeys(base)
        res["set_same"] = arm("set_same")
        cc.update_pubkeys(base)
        open_rounds()
        res["update_same"] = arm("update_same")
        res["update_swap"] = arm("update_swap")
        for k, r in enumerate(rounds):   # the rounds came through every update
            assert r.qc()[2] == 1
            r.close()
        rounds[:] = []
        out["tables"][str(n)] = res
    out["table_stats"] = list(cc.table_stats())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
