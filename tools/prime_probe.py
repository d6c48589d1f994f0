#!/usr/bin/env python
"""The primed routes (ovh_prime_hashes) against the unprimed ones, on one
context of one library:
  sign            ovh_sign on a hash that is not in the message cache / on a primed one
  batch           ovh_verify_batch of n = 67 and 1,024 votes on one hash, all valid and with 1%
                  swapped signatures, on a hash that is not cached / on a primed one
  prime_wait      prime a fresh hash, wait max_delay (2 ms, the ingress shim's deadline), batch;
                  the whole sequence and the batch alone
  prime_behind    the batch enqueued right behind the prime of its fresh hash (the shim's case
                  when a group fills at once)
in several interleaved rounds (a round = every case, each REPS times in turn). --lib names the
library: a build without ovh_prime_hashes (the parent commit's) runs the same calls with no
prime, so its "primed" columns are its unprimed route again and prime_wait is the bare wait plus
the batch. Prints one JSON line per round, then a summary line (median, min, max over the rounds'
medians), all in ms.   python tools/prime_probe.py [--lib PATH] [--rounds 5] [--reps 7]"""
import argparse
import ctypes
import hashlib
import json
import os
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (67, 1024)
MAX_DELAY_S = 0.002
FLAG_SK_RAW = 0x10


def _ms(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "consensus_overlord_amd", "libovhip.so"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tag", default="this")
    args = ap.parse_args()
    import torch   # first: the library binds to torch's HIP runtime
    lib = ctypes.CDLL(args.lib)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    lib.ovh_create.restype = vp
    lib.ovh_create.argtypes = [ctypes.c_int, ctypes.c_char_p, sz, ctypes.c_uint32]
    lib.ovh_destroy.argtypes = [vp]
    lib.ovh_sign.argtypes = [vp, ctypes.c_char_p, sz, ctypes.c_char_p, sz, ctypes.c_char_p]
    lib.ovh_verify_batch.argtypes = [vp, sz, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, vp]
    lib.ovh_sign_batch_device.argtypes = [vp, sz, vp, vp, vp]
    lib.ovh_sk_to_pk_batch_device.argtypes = [vp, sz, vp, vp]
    has_prime = hasattr(lib, "ovh_prime_hashes")
    if has_prime:
        lib.ovh_prime_hashes.argtypes = [vp, sz, ctypes.c_char_p]
        lib.ovh_prime_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    ctx = lib.ovh_create(0, None, 0, FLAG_SK_RAW)
    assert ctx

    def prime(h):
        if has_prime:
            assert lib.ovh_prime_hashes(ctx, 1, h) == 0

    def pstats():
        st = (ctypes.c_uint64 * 4)()
        if has_prime:
            assert lib.ovh_prime_stats(ctx, st) == 0
        return [int(x) for x in st]

    nmax = max(SIZES)
    rng = np.random.default_rng(0x9117)
    sks_h = rng.integers(0, 256, size=(nmax, 32), dtype=np.uint8)
    sks_h[:, 0] &= 0x3F                      # below the group order
    sks = torch.from_numpy(sks_h).cuda()
    pks_d = torch.empty((nmax, 48), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert lib.ovh_sk_to_pk_batch_device(ctx, nmax, sks.data_ptr(), pks_d.data_ptr()) == 0
    pks = pks_d.cpu().numpy()

    def votes(h, n, invalid):
        """(sigs, hashes, pks) bytes of n votes on hash h; invalid: 1% carry the next vote's signature"""
        hs = torch.from_numpy(np.tile(np.frombuffer(h, dtype=np.uint8), (n, 1))).cuda()
        out = torch.empty((n, 96), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert lib.ovh_sign_batch_device(ctx, n, sks.data_ptr(), hs.data_ptr(), out.data_ptr()) == 0
        sg = out.cpu().numpy().copy()
        bad = sorted(np.random.default_rng(n).choice(n, max(1, n // 100), replace=False).tolist()) if invalid else []
        orig = sg.copy()
        for i in bad:
            sg[i] = orig[(i + 1) % n]
        return sg.tobytes(), h * n, pks[:n].tobytes(), bad

    hu = hashlib.sha256(b"prime probe: never cached").digest()
    hp = hashlib.sha256(b"prime probe: primed").digest()
    fixed = {(n, inv, name): votes(h, n, inv) for n in SIZES for inv in (0, 1) for name, h in (("u", hu), ("p", hp))}
    nfresh = (args.rounds + 1) * args.reps
    fresh = {(n, mode): [] for n in SIZES for mode in ("wait", "behind")}
    for key in fresh:
        for j in range(nfresh):
            h = hashlib.sha256(b"prime probe fresh %d %s %d" % (key[0], key[1].encode(), j)).digest()
            fresh[key].append((h, votes(h, key[0], 0)))
    sk = sks_h[0].tobytes()
    sig = ctypes.create_string_buffer(96)

    def batch(v):
        n = len(v[1]) // 32
        codes = (ctypes.c_int32 * n)()
        assert lib.ovh_verify_batch(ctx, n, v[0], v[1], v[2], ctypes.cast(codes, vp)) == 0
        assert [i for i in range(n) if codes[i] != 0] == v[3]

    rows = []
    for rnd in range(args.rounds + 1):          # round 0 warms every path up and is not recorded
        prime(hp)                               # (skipped while cached; the fresh hashes age it out)
        t = {}
        for rep in range(args.reps):
            for name, h in (("sign_unprimed_ms", hu), ("sign_primed_ms", hp)):
                t.setdefault(name, []).append(_ms(lambda: lib.ovh_sign(ctx, sk, 32, h, 32, sig)))
            for n in SIZES:
                for inv in (0, 1):
                    for name in ("u", "p"):
                        key = "batch%d_%s_%s_ms" % (n, "inv1pct" if inv else "valid", "unprimed" if name == "u" else "primed")
                        t.setdefault(key, []).append(_ms(lambda: batch(fixed[(n, inv, name)])))
                h, v = fresh[(n, "wait")][rnd * args.reps + rep]
                t0 = time.perf_counter()
                prime(h)
                while time.perf_counter() - t0 < MAX_DELAY_S:
                    pass
                t1 = time.perf_counter()
                batch(v)
                t2 = time.perf_counter()
                t.setdefault("prime_wait_batch%d_total_ms" % n, []).append((t2 - t0) * 1e3)
                t.setdefault("prime_wait_batch%d_batch_ms" % n, []).append((t2 - t1) * 1e3)
                h, v = fresh[(n, "behind")][rnd * args.reps + rep]
                t0 = time.perf_counter()
                prime(h)
                batch(v)
                t.setdefault("prime_behind_batch%d_ms" % n, []).append((time.perf_counter() - t0) * 1e3)
        row = {k: round(float(np.median(v)), 4) for k, v in t.items()}
        if rnd:
            rows.append(row)
            print(json.dumps({"lib": args.tag, "round": rnd, **row}), flush=True)
    s = {"lib": args.tag, "has_prime": has_prime, "rounds": args.rounds, "reps": args.reps, "prime_stats": pstats()}
    for k in rows[0]:
        v = [r[k] for r in rows]
        s[k] = {"median": round(float(np.median(v)), 4), "min": min(v), "max": max(v)}
    print(json.dumps({"summary": s}), flush=True)
    lib.ovh_destroy(ctx)


if __name__ == "__main__":
    main()
