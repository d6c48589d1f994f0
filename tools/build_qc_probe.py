#!/usr/bin/env python
"""ovh_build_qc against the two-call sequence it replaces, on one context:
  build_qc   one ovh_build_qc call (verify + select + aggregate in one device pass)
  two_call   ovh_verify_batch, a host filter of the valid votes, ovh_aggregate_sigs of those
for clean rounds of n = 67 (config 2), 1,024 and 4,096 validators that all sign one hash, in
several interleaved rounds (a round = every size, each path REPS times in turn). The library
calls take prebuilt byte buffers; the filter (numpy on the host) is timed on its own and left
out of two_call_ms, so the comparison is between library calls only. build_qc also enters the
verdicts in the verdict cache (ovh_verify_batch does not): build_qc_nocache_ms is the same call
with the cache switched off (ovh_cache_config 0), i.e. without that host work.
Prints one JSON line per round and size, then a summary line per size (median, min, max over
the rounds' medians).   python tools/build_qc_probe.py [--rounds 5] [--reps 7]"""
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

SIZES = (67, 1024, 4096)


def _ms(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import torch
    import bench
    from consensus_overlord_amd import device as dev
    from consensus_overlord_amd.crypto import Context
    ctx = Context(0)
    lib = ctx.lib
    data = {}
    for n in SIZES:
        sks_h, _ = bench.synth_inputs(lib, 0, n)
        sks = torch.from_numpy(sks_h).cuda()
        d = hashlib.sha256(b"build_qc probe %d" % n).digest()
        hs = torch.from_numpy(np.tile(np.frombuffer(d, dtype=np.uint8), (n, 1))).cuda()
        pk = dev.sk_to_pk_batch(ctx, sks).cpu().numpy()
        sg = dev.sign_batch(ctx, sks, hs).cpu().numpy()
        data[n] = (d, sg, pk, sg.tobytes(), pk.tobytes(), d * n)
    vp = ctypes.c_void_p
    rows = {n: [] for n in SIZES}
    for rnd in range(args.rounds + 1):          # round 0 warms every path up and is not recorded
        for n in SIZES:
            d, sg, pk, sgb, pkb, hsb = data[n]
            assert lib.ovh_set_validators(ctx.ptr, pkb, n) == 0
            codes = np.zeros(n, dtype=np.int32)
            taken = np.zeros(n, dtype=np.uint8)
            bl = (n + 7) // 8
            bitmap = ctypes.create_string_buffer(bl)
            out = ctypes.create_string_buffer(96)
            out2 = ctypes.create_string_buffer(96)
            cnt = ctypes.c_uint32(0)
            lens_s = (ctypes.c_size_t * n)(*([96] * n))
            lens_p = (ctypes.c_size_t * n)(*([48] * n))
            sel = {}

            def build():
                assert lib.ovh_build_qc(ctx.ptr, n, sgb, d, 32, pkb, codes.ctypes.data_as(vp), taken.ctypes.data_as(vp),
                                        out, bitmap, bl, ctypes.byref(cnt)) == 0

            def verify():
                assert lib.ovh_verify_batch(ctx.ptr, n, sgb, hsb, pkb, codes.ctypes.data_as(vp)) == 0

            def filt():
                ok = codes == 0
                sel["s"], sel["p"], sel["k"] = sg[ok].tobytes(), pk[ok].tobytes(), int(ok.sum())

            def aggregate():
                k = sel["k"]
                assert lib.ovh_aggregate_sigs(ctx.ptr, sel["s"], lens_s, k, sel["p"], lens_p, k, out2) == 0

            t = {"build_qc_ms": [], "build_qc_nocache_ms": [], "verify_ms": [], "filter_ms": [], "aggregate_ms": []}
            for _ in range(args.reps):
                t["build_qc_ms"].append(_ms(build))
                assert cnt.value == n and out.raw != bytes(96)
                t["verify_ms"].append(_ms(verify))
                t["filter_ms"].append(_ms(filt))
                t["aggregate_ms"].append(_ms(aggregate))
                assert out2.raw == out.raw
                assert lib.ovh_cache_config(ctx.ptr, 0) == 0
                t["build_qc_nocache_ms"].append(_ms(build))
                assert lib.ovh_cache_config(ctx.ptr, 1 << 16) == 0
            row = {k: round(float(np.median(v)), 4) for k, v in t.items()}
            row["two_call_ms"] = round(row["verify_ms"] + row["aggregate_ms"], 4)
            if rnd:
                rows[n].append(row)
                print(json.dumps({"round": rnd, "n": n, **row}), flush=True)
    for n in SIZES:
        s = {"n": n, "rounds": args.rounds, "reps": args.reps}
        for k in ("build_qc_ms", "build_qc_nocache_ms", "two_call_ms", "verify_ms", "aggregate_ms", "filter_ms"):
            v = [r[k] for r in rows[n]]
            s[k] = {"median": round(float(np.median(v)), 4), "min": min(v), "max": max(v)}
        print(json.dumps({"summary": s}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
