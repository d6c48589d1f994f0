#!/usr/bin/env python
"""What the two trait calls of a round's QC cost, on one library, in one
process, on the contexts named by --contexts, side by side: `route` (created with the defaults of
the environment it finds), `full` (created under OVH_SIG_CACHE=0 and OVH_QC_TABLE=0: the full paths)
and `always` (OVH_QC_TABLE=2: the table route on unprimed hashes too). A repetition runs every arm
on every context in turn; repetition 0 warms every path up and is not recorded. Two contexts in one
process share the runtime's hardware queues, which can put a context's side stream on its main
stream's queue and cost the full paths their overlap (0.5 to 1.4 ms): compare one-context runs
(--contexts route, --contexts full) where the absolute figure matters.

  leader   every one of S signers votes once on a hash that is new in every repetition (primed
           at "proposal receipt" on both contexts). Untimed: the context's own vote (ovh_sign) and
           the prefetch of the first S - 1 - k others. Timed: ovh_prefetch of the last k votes,
           then ovh_aggregate_sigs over all S signers; reported apart and summed. S = 67 of a
           67-key table and 683 of a 1,024-key table; k = 1 and 8. The bytes must equal on both
           contexts in every repetition.
  replica  ovh_verify_aggregated over 67 of 100 and 683 of 1,024 table voters, on a primed hash
           and on one that is in no table; every code must be 0.

--lib names the library: the parent commit's build ignores the environment variables, so each of
its contexts runs the full paths (its rows are the baseline). Prints one JSON line per row: medians with minima and maxima, in ms.
    python tools/agg_probe.py [--lib PATH] [--reps 25] [--tag NAME]"""
import argparse
import ctypes
import hashlib
import json
import os
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEADER = ((67, 67), (683, 1024))      # (signers, validators)
REPLICA = ((67, 100), (683, 1024))
LAST = (1, 8)
FLAG_SK_RAW = 0x10


def _ms(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def _stat(v):
    return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "consensus_overlord_amd", "libovhip.so"))
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--tag", default="this")
    ap.add_argument("--contexts", default="route,full")
    args = ap.parse_args()
    assert args.reps >= 20, "medians of at least 20 repetitions"
    import torch   # first: the library binds to torch's HIP runtime
    lib = ctypes.CDLL(args.lib)
    vp, sz, cp = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p
    szp = ctypes.POINTER(sz)
    lib.ovh_create.restype = vp
    lib.ovh_create.argtypes = [ctypes.c_int, cp, sz, ctypes.c_uint32]
    lib.ovh_destroy.argtypes = [vp]
    lib.ovh_sign.argtypes = [vp, cp, sz, cp, sz, cp]
    lib.ovh_prefetch.argtypes = [vp, sz, cp, cp, cp]
    lib.ovh_set_validators.argtypes = [vp, cp, sz]
    lib.ovh_prime_hashes.argtypes = [vp, sz, cp]
    lib.ovh_aggregate_sigs.argtypes = [vp, cp, szp, sz, cp, szp, sz, cp]
    lib.ovh_verify_aggregated.argtypes = [vp, cp, sz, cp, sz, cp, szp, sz]
    lib.ovh_sign_batch_device.argtypes = [vp, sz, vp, vp, vp]
    lib.ovh_sk_to_pk_batch_device.argtypes = [vp, sz, vp, vp]
    has_stats = hasattr(lib, "ovh_agg_stats")
    if has_stats:
        lib.ovh_agg_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]

    def create(**env):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            c = lib.ovh_create(0, None, 0, FLAG_SK_RAW)
        finally:
            for k, v in old.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v
        assert c
        return c

    kinds = {"route": {}, "full": {"OVH_SIG_CACHE": "0", "OVH_QC_TABLE": "0"}, "always": {"OVH_QC_TABLE": "2"}}
    ctxs = {name: create(**kinds[name]) for name in args.contexts.split(",")}
    first = next(iter(ctxs.values()))

    def stats(c):
        st = (ctypes.c_uint64 * 8)()
        if has_stats:
            assert lib.ovh_agg_stats(c, st) == 0
        return [int(x) for x in st]

    nmax = 1024
    rng = np.random.default_rng(0xA661)
    sks_h = rng.integers(0, 256, size=(nmax, 32), dtype=np.uint8)
    sks_h[:, 0] &= 0x3F                      # below the group order
    sks = torch.from_numpy(sks_h).cuda()
    pks_d = torch.empty((nmax, 48), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert lib.ovh_sk_to_pk_batch_device(first, nmax, sks.data_ptr(), pks_d.data_ptr()) == 0
    pks = pks_d.cpu().numpy()
    sk0 = sks_h[0].tobytes()

    def sign_all(h, n):
        hs = torch.from_numpy(np.tile(np.frombuffer(h, dtype=np.uint8), (n, 1))).cuda()
        out = torch.empty((n, 96), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert lib.ovh_sign_batch_device(first, n, sks.data_ptr(), hs.data_ptr(), out.data_ptr()) == 0
        return out.cpu().numpy()

    def set_table(nv):
        for c in ctxs.values():
            assert lib.ovh_set_validators(c, pks[:nv].tobytes(), nv) == 0

    # ---- leader
    for s, nv in LEADER:
        set_table(nv)
        lens96 = (sz * s)(*([96] * s))
        lens48 = (sz * s)(*([48] * s))
        pkb = pks[:s].tobytes()
        for k in LAST:
            t = {name: {"prefetch": [], "aggregate": [], "sum": []} for name in ctxs}
            st0 = {name: stats(c) for name, c in ctxs.items()}
            for rep in range(args.reps + 1):
                h = hashlib.sha256(b"agg probe leader %d %d %d" % (s, k, rep)).digest()
                sg = sign_all(h, s)
                lo = s - k
                outs = {}
                for name, c in ctxs.items():
                    assert lib.ovh_prime_hashes(c, 1, h) == 0
                    own = ctypes.create_string_buffer(96)
                    assert lib.ovh_sign(c, sk0, 32, h, 32, own) == 0 and own.raw == sg[0].tobytes()
                    if lo > 1:
                        assert lib.ovh_prefetch(c, lo - 1, sg[1:lo].tobytes(), h * (lo - 1), pks[1:lo].tobytes()) == 0
                    tail = (sg[lo:].tobytes(), h * k, pks[lo:s].tobytes())
                    out = ctypes.create_string_buffer(96)
                    sgb, rc = sg.tobytes(), []
                    a = _ms(lambda: rc.append(lib.ovh_prefetch(c, k, *tail)))
                    b = _ms(lambda: rc.append(lib.ovh_aggregate_sigs(c, sgb, lens96, s, pkb, lens48, s, out)))
                    assert rc == [0, 0]
                    outs[name] = out.raw
                    if rep:
                        t[name]["prefetch"].append(a)
                        t[name]["aggregate"].append(b)
                        t[name]["sum"].append(a + b)
                assert len(set(outs.values())) == 1, "the contexts disagree"
            row = {"lib": args.tag, "arm": "leader", "signers": s, "validators": nv, "last_k": k, "reps": args.reps}
            for name, c in ctxs.items():
                row[name] = {col: _stat(v) for col, v in t[name].items()}
                d = [b - a for a, b in zip(st0[name], stats(c))]
                row[name]["calls_on_cache_route"], row[name]["calls_on_full_path"] = d[2], d[3]
            print(json.dumps(row), flush=True)

    # ---- replica
    for s, nv in REPLICA:
        set_table(nv)
        lens96 = (sz * s)(*([96] * s))
        lens48 = (sz * s)(*([48] * s))
        pkb = pks[:s].tobytes()
        qcs = {}
        for mode in ("primed", "unprimed"):
            h = hashlib.sha256(b"agg probe replica %d %s" % (s, mode.encode())).digest()
            sg = sign_all(h, s)
            agg = ctypes.create_string_buffer(96)
            assert lib.ovh_aggregate_sigs(first, sg.tobytes(), lens96, s, pkb, lens48, s, agg) == 0
            qcs[mode] = (h, agg.raw)
        for c in ctxs.values():
            assert lib.ovh_prime_hashes(c, 1, qcs["primed"][0]) == 0
        t = {(name, mode): [] for name in ctxs for mode in qcs}
        st0 = {name: stats(c) for name, c in ctxs.items()}
        for rep in range(args.reps + 1):
            for mode, (h, agg) in qcs.items():
                for name, c in ctxs.items():
                    code = []
                    ms = _ms(lambda: code.append(lib.ovh_verify_aggregated(c, agg, 96, h, 32, pkb, lens48, s)))
                    assert code == [0]
                    if rep:
                        t[(name, mode)].append(ms)
        row = {"lib": args.tag, "arm": "replica", "voters": s, "validators": nv, "reps": args.reps}
        for name, c in ctxs.items():
            row[name] = {mode: _stat(t[(name, mode)]) for mode in qcs}
            d = [b - a for a, b in zip(st0[name], stats(c))]
            row[name]["calls_on_table_route"], row[name]["of_those_on_cached_h"], row[name]["calls_on_full_path"] = d[5], d[6], d[7]
        print(json.dumps(row), flush=True)
    for c in ctxs.values():
        lib.ovh_destroy(c)


if __name__ == "__main__":
    main()
