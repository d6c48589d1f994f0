#!/usr/bin/env python
"""ovh_build_qcs against the sequence it replaces, on one context:
  build_qcs  one ovh_build_qcs call over the mixed-hash vote set
  sequence   the host split of the set by hash, then one ovh_build_qc call per hash over that
             hash's votes, one after the other
for clean vote sets (every vote valid, every voter a validator, the groups interleaved by a seeded
shuffle): 67 votes as 45 + 22, 1,024 as 700 + 324, 1,024 as 8 x 128 and 4,096 as 2,731 + 1,365,
in several interleaved rounds (a round = every shape, each path REPS times in turn). The library
calls take prebuilt byte buffers; the split (numpy on the host) is timed on its own and left out
of sequence_ms, so the comparison is between library calls only. Both paths enter their verdicts
in the verdict cache. Prints one JSON line per round and shape, then a summary line per shape
(median, min, max over the rounds' medians).   python tools/build_qcs_probe.py [--rounds 5] [--reps 7]"""
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

SHAPES = (("67=45+22", (45, 22)), ("1024=700+324", (700, 324)), ("1024=8x128", (128,) * 8),
          ("4096=2731+1365", (2731, 1365)))


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
    for name, sizes in SHAPES:
        n, G = sum(sizes), len(sizes)
        sks_h, _ = bench.synth_inputs(lib, 0, n)
        sks = torch.from_numpy(sks_h).cuda()
        gh = np.stack([np.frombuffer(hashlib.sha256(b"build_qcs probe %s %d" % (name.encode(), g)).digest(),
                                     dtype=np.uint8) for g in range(G)])
        gid = np.repeat(np.arange(G), sizes)
        np.random.RandomState(n + G).shuffle(gid)
        hs_h = gh[gid]
        pk = dev.sk_to_pk_batch(ctx, sks).cpu().numpy()
        sg = dev.sign_batch(ctx, sks, torch.from_numpy(hs_h).cuda()).cpu().numpy()
        data[name] = (n, G, sizes, gh, hs_h, sg, pk, sg.tobytes(), hs_h.tobytes(), pk.tobytes())
    vp = ctypes.c_void_p
    p = lambda a: a.ctypes.data_as(vp)   # noqa: E731
    rows = {name: [] for name, _ in SHAPES}
    for rnd in range(args.rounds + 1):          # round 0 warms every path up and is not recorded
        for name, _ in SHAPES:
            n, G, sizes, gh, hs_h, sg, pk, sgb, hsb, pkb = data[name]
            assert lib.ovh_set_validators(ctx.ptr, pkb, n) == 0
            bl = (n + 7) // 8
            codes, taken, group = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint32)
            ghs, outs = np.zeros((64, 32), dtype=np.uint8), np.zeros((64, 96), dtype=np.uint8)
            bms, cnts = np.zeros((64, bl), dtype=np.uint8), np.zeros(64, dtype=np.uint32)
            ng = ctypes.c_uint32(0)
            parts = {}
            seq = {"out": [None] * G, "bm": [None] * G, "cnt": [0] * G}

            def grouped():
                assert lib.ovh_build_qcs(ctx.ptr, n, sgb, hsb, pkb, p(codes), p(taken), p(group), 64, ctypes.byref(ng),
                                         p(ghs), p(outs), p(bms), bl, p(cnts)) == 0

            def split():
                _, first, inv = np.unique(hs_h, axis=0, return_index=True, return_inverse=True)
                order = np.argsort(np.argsort(first))          # groups numbered by first appearance
                g_of = order[inv.reshape(-1)]
                for g in range(G):
                    m = g_of == g
                    parts[g] = (int(m.sum()), sg[m].tobytes(), hs_h[m][0].tobytes(), pk[m].tobytes())

            def sequence():
                for g in range(G):
                    k, s, h, v = parts[g]
                    c, t = np.zeros(k, dtype=np.int32), np.zeros(k, dtype=np.uint8)
                    out, bm, cnt = ctypes.create_string_buffer(96), ctypes.create_string_buffer(bl), ctypes.c_uint32(0)
                    assert lib.ovh_build_qc(ctx.ptr, k, s, h, 32, v, p(c), p(t), out, bm, bl, ctypes.byref(cnt)) == 0
                    seq["out"][g], seq["bm"][g], seq["cnt"][g] = out.raw, bm.raw, cnt.value

            t = {"build_qcs_ms": [], "split_ms": [], "sequence_ms": []}
            for _ in range(args.reps):
                t["build_qcs_ms"].append(_ms(grouped))
                assert ng.value == G and int(cnts[:G].sum()) == n and not codes.any()
                t["split_ms"].append(_ms(split))
                t["sequence_ms"].append(_ms(sequence))
                for g in range(G):                          # the two paths build the same QCs
                    assert parts[g][2] == ghs[g].tobytes() and seq["cnt"][g] == cnts[g]
                    assert seq["out"][g] == outs[g].tobytes() and seq["bm"][g] == bms[g].tobytes()
            row = {k: round(float(np.median(v)), 4) for k, v in t.items()}
            if rnd:
                rows[name].append(row)
                print(json.dumps({"round": rnd, "shape": name, **row}), flush=True)
    for name, sizes in SHAPES:
        s = {"shape": name, "groups": len(sizes), "rounds": args.rounds, "reps": args.reps}
        for k in ("build_qcs_ms", "sequence_ms", "split_ms"):
            v = [r[k] for r in rows[name]]
            s[k] = {"median": round(float(np.median(v)), 4), "min": min(v), "max": max(v)}
        print(json.dumps({"summary": s}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
