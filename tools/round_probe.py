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
per (N, k) with the medians, minima and maxima in ms.   python tools/round_probe.py [--reps 25]
With --split: a last flush split over several hashes, one ovh_round_add per hash against one
ovh_rounds_add (split_main)."""
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


SPLITS = ((6, 2), (4, 3, 1), (34, 33))   # the last flush's votes per hash


def split_main(args):
    """--split: what a last flush that is split over several hashes costs, per validator table and
    per shape of SPLITS, every round filled up to its last votes before the timer starts, QC bytes
    and bitmaps requested:
      per_round   one ovh_round_add per hash in sequence (only calls that exist since section 3.8:
                  the same script gives the baseline on a library without ovh_rounds_add)
      rounds_add  one ovh_rounds_add over the flush in arrival order (hashes interleaved)
    A repetition opens fresh rounds for each arm; repetition 0 is not recorded; both arms must give
    the same bytes, bitmap and count per round. One JSON line per (N, shape)."""
    import torch
    import bench
    from consensus_overlord_amd import device as dev
    from consensus_overlord_amd.crypto import Context
    ctx = Context(0)
    lib = ctx.lib
    vp = ctypes.c_void_p
    p = lambda a: a.ctypes.data_as(vp)   # noqa: E731
    have = hasattr(lib, "ovh_rounds_add")
    for n in TABLES:
        sks_h, _ = bench.synth_inputs(lib, 0, n)
        sks = torch.from_numpy(sks_h).cuda()
        pk = dev.sk_to_pk_batch(ctx, sks).cpu().numpy()
        assert lib.ovh_set_validators(ctx.ptr, pk.tobytes(), n) == 0
        bl = (n + 7) // 8
        for shape in SPLITS:
            # hash g has the votes of size[g] validators of its own (the whole table when the flush
            # is the whole round), the first size[g] - shape[g] of them added before the timer starts
            G = len(shape)
            size = [max(m, n // G) for m in shape]
            off = [sum(size[:g]) for g in range(G)]
            assert sum(size) <= n
            hashes = [hashlib.sha256(b"round probe split %d %d %d" % (n, G, g)).digest() for g in range(G)]
            sg = [dev.sign_batch(ctx, sks[off[g]:off[g] + size[g]],
                                 torch.from_numpy(np.tile(np.frombuffer(hashes[g], dtype=np.uint8), (size[g], 1))).cuda())
                  .cpu().numpy() for g in range(G)]
            pkg = [pk[off[g]:off[g] + size[g]] for g in range(G)]
            # the flush in arrival order: the hashes' last votes, round-robin
            flush = []
            left = list(shape)
            while any(left):
                for g in range(G):
                    if left[g]:
                        flush.append((g, size[g] - left[g]))
                        left[g] -= 1
            k = len(flush)
            fl_s = b"".join(sg[g][i].tobytes() for g, i in flush)
            fl_p = b"".join(pkg[g][i].tobytes() for g, i in flush)

            def fill():
                """fresh rounds with everything but the flush added"""
                ids = []
                codes, cnt = np.zeros(max(size), dtype=np.int32), ctypes.c_uint32(0)
                for g in range(G):
                    rid = ctypes.c_uint64(0)
                    assert lib.ovh_round_open(ctx.ptr, hashes[g], 32, ctypes.byref(rid)) == 0
                    lo = size[g] - shape[g]
                    if lo:
                        assert lib.ovh_round_add(ctx.ptr, rid.value, lo, sg[g][:lo].tobytes(), pkg[g][:lo].tobytes(),
                                                 p(codes), None, ctypes.byref(cnt), None, None, 0) == 0 and cnt.value == lo
                    ids.append(rid.value)
                return ids

            def close(ids):
                for rid in ids:
                    assert lib.ovh_round_close(ctx.ptr, rid) == 0

            def per_round():
                ids = fill()
                outs = [(ctypes.create_string_buffer(96), ctypes.create_string_buffer(bl), ctypes.c_uint32(0)) for _ in ids]
                codes = np.zeros(k, dtype=np.int32)

                def last():
                    for g, rid in enumerate(ids):
                        lo = size[g] - shape[g]
                        assert lib.ovh_round_add(ctx.ptr, rid, shape[g], sg[g][lo:].tobytes(), pkg[g][lo:].tobytes(),
                                                 p(codes), None, ctypes.byref(outs[g][2]), outs[g][0], outs[g][1], bl) == 0
                ms = _ms(last)
                close(ids)
                return ms, [(o.raw, b.raw, c.value) for o, b, c in outs]

            def rounds_add():
                ids = fill()
                idv = np.array([ids[g] for g, _ in flush], dtype=np.uint64)
                codes = np.zeros(k, dtype=np.int32)
                rid, cnt = np.zeros(16, dtype=np.uint64), np.zeros(16, dtype=np.uint32)
                out, bm = np.zeros((16, 96), dtype=np.uint8), np.zeros((16, bl), dtype=np.uint8)
                nr = ctypes.c_uint32(0)

                def last():
                    assert lib.ovh_rounds_add(ctx.ptr, k, fl_s, p(idv), fl_p, p(codes), None, None, 16, ctypes.byref(nr),
                                              p(rid), p(cnt), p(out), p(bm), bl) == 0
                ms = _ms(last)
                assert nr.value == G and rid[:G].tolist() == ids and not codes.any()
                close(ids)
                return ms, [(out[g].tobytes(), bm[g].tobytes(), int(cnt[g])) for g in range(G)]

            t = {"per_round_ms": [], "rounds_add_ms": []}
            for rep in range(args.reps + 1):
                a, qa = per_round()
                assert [q[2] for q in qa] == size
                if have:
                    b, qb = rounds_add()
                    assert qa == qb, "the two arms disagree"
                if rep:
                    t["per_round_ms"].append(a)
                    if have:
                        t["rounds_add_ms"].append(b)
            row = {"validators": n, "split": list(shape), "reps": args.reps}
            for name, v in t.items():
                if v:
                    row[name] = {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
            print(json.dumps(row), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--split", action="store_true", help="a last flush split over several hashes (section 3.9)")
    args = ap.parse_args()
    assert args.reps >= 20, "medians of at least 20 repetitions"
    if args.split:
        return split_main(args)
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
