#!/usr/bin/env python
"""What the last flush of a round costs a leader, on one context, for
validator tables of 67 and 1,024 keys, every validator voting once, every vote valid, the round's
hash seen before (message cache warm) in every arm:
  parent     ovh_prefetch of the round's last k votes, then ovh_aggregate_sigs over all N votes,
             timed together (the trait path: the verdict cache answers overlord's verify_signature
             calls, aggregate_signatures decompresses and subgroup-checks the quorum again)
  build_qc   ovh_build_qc over all N votes, timed beside it (it verifies the earlier flushes again)
  round      ovh_round_add of the same last k votes with out_sig and bitmap requested; the round was
             opened and the first N - k votes were added before the timer starts
for k = 1 and k = 8. One process; a repetition runs the three arms in turn; repetition 0 warms every
path up and is not recorded. The three arms must build the same signature. Prints one JSON line
per (N, k) with the medians, minima and maxima in ms.   python tools/round_probe.py [--reps 25]"""
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

TABLES = (67, 1024)
LAST = (1, 8)


def _ms(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    args = ap.parse_args()
    assert args.reps >= 20, "medians of at least 20 repetitions"
    import torch
    import bench
    from consensus_overlord_amd import device as dev
    from consensus_overlord_amd.crypto import Context
    ctx = Context(0)
    lib = ctx.lib
    vp = ctypes.c_void_p
    p = lambda a: a.ctypes.data_as(vp)   # noqa: E731
    for n in TABLES:
        sks_h, _ = bench.synth_inputs(lib, 0, n)
        sks = torch.from_numpy(sks_h).cuda()
        h = hashlib.sha256(b"round probe %d" % n).digest()
        hs_h = np.tile(np.frombuffer(h, dtype=np.uint8), (n, 1))
        pk = dev.sk_to_pk_batch(ctx, sks).cpu().numpy()
        sg = dev.sign_batch(ctx, sks, torch.from_numpy(hs_h).cuda()).cpu().numpy()
        sgb, hsb, pkb = sg.tobytes(), hs_h.tobytes(), pk.tobytes()
        assert lib.ovh_set_validators(ctx.ptr, pkb, n) == 0
        bl = (n + 7) // 8
        lens96 = (ctypes.c_size_t * n)(*([96] * n))
        lens48 = (ctypes.c_size_t * n)(*([48] * n))
        for k in LAST:
            lo = n - k
            tail_s, tail_h, tail_p = sg[lo:].tobytes(), hs_h[lo:].tobytes(), pk[lo:].tobytes()
            head_s, head_p = sg[:lo].tobytes(), pk[:lo].tobytes()
            res = {}

            def parent():
                out = ctypes.create_string_buffer(96)
                assert lib.ovh_prefetch(ctx.ptr, k, tail_s, tail_h, tail_p) == 0
                assert lib.ovh_aggregate_sigs(ctx.ptr, sgb, lens96, n, pkb, lens48, n, out) == 0
                res["parent"] = out.raw

            def build_qc():
                codes, taken = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint8)
                out, bm, cnt = ctypes.create_string_buffer(96), ctypes.create_string_buffer(bl), ctypes.c_uint32(0)
                assert lib.ovh_build_qc(ctx.ptr, n, sgb, h, 32, pkb, p(codes), p(taken), out, bm, bl, ctypes.byref(cnt)) == 0
                assert cnt.value == n
                res["build_qc"] = out.raw

            def round_arm():
                rid = ctypes.c_uint64(0)
                assert lib.ovh_round_open(ctx.ptr, h, 32, ctypes.byref(rid)) == 0
                codes, cnt = np.zeros(n, dtype=np.int32), ctypes.c_uint32(0)
                assert lib.ovh_round_add(ctx.ptr, rid.value, lo, head_s, head_p, p(codes), None, ctypes.byref(cnt), None,
                                         None, 0) == 0 and cnt.value == lo
                out, bm = ctypes.create_string_buffer(96), ctypes.create_string_buffer(bl)

                def last():
                    assert lib.ovh_round_add(ctx.ptr, rid.value, k, tail_s, tail_p, p(codes), None, ctypes.byref(cnt), out,
                                             bm, bl) == 0
                ms = _ms(last)
                assert cnt.value == n and not codes[:k].any()
                assert lib.ovh_round_close(ctx.ptr, rid.value) == 0
                res["round"] = out.raw
                return ms

            t = {"parent_ms": [], "build_qc_ms": [], "round_ms": []}
            for rep in range(args.reps + 1):
                a, b, c = _ms(parent), _ms(build_qc), round_arm()
                assert res["parent"] == res["build_qc"] == res["round"]
                if rep:
                    t["parent_ms"].append(a)
                    t["build_qc_ms"].append(b)
                    t["round_ms"].append(c)
            row = {"validators": n, "last_k": k, "reps": args.reps}
            for name, v in t.items():
                row[name] = {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
            row["round_le_parent"] = row["round_ms"]["median"] <= row["parent_ms"]["median"]
            print(json.dumps(row), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
