"""Shared by the Fp-VM tests (tests/test_vm_host.py on the host build of the interpreter,
tests/test_gpu_fp_bounds.py on the device): running one unit of a scheduled program through
hx_vm_run (tests/host/harness.cpp) or dp_vm_run (tests/device/fp_probe.hip), the comparison
with the slot-level simulator, and the golden votes' program inputs."""
import ctypes
import functools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "fpvm"))

import gen  # noqa: E402
import sched  # noqa: E402
from ir import P  # noqa: E402

R = pow(2, 384, P)
RAW_INPUTS = {"pk_sort", "sig_sort"}   # flags the vote prologue writes as plain limbs
NPLANES = 64
u32p = ctypes.POINTER(ctypes.c_uint32)


@functools.lru_cache(maxsize=None)
def build_all():
    """gen.build_all() (constant table, scheduled and encoded programs), generated once per
    process however many test modules ask for it."""
    return gen.build_all()


def _words(v):
    return [(v >> (32 * k)) & 0xFFFFFFFF for k in range(12)]


def _int(ws):
    return sum(int(w) << (32 * k) for k, w in enumerate(ws))


def run_vm(hx, consts, sc, words, inputs, scalar, any_all, raw_slots=None, device=False):
    """One unit of program `sc` / `words` on `inputs` (canonical values, stored in Montgomery
    form; raw_slots: {input name: limbs value} written as they are instead). hx: the host
    harness, run with `any_all` (every wave-uniform block for every lane); device=True: `hx` is
    the device probe, and the phase headers decide as on the GPU. -> {output name: limbs value}."""
    prog = sc.prog
    slots = np.zeros(sc.nslots * 12, dtype=np.uint32)
    for name, v in prog.inputs.items():
        if v in sc.slot_of:
            s = sc.slot_of[v]
            if raw_slots is not None and name in raw_slots:
                slots[s * 12:s * 12 + 12] = _words(raw_slots[name])
                continue
            val = inputs[name] % P
            slots[s * 12:s * 12 + 12] = _words(val if name in RAW_INPUTS else val * R % P)
    code = np.asarray(words, dtype=np.uint32)
    cst = np.asarray(consts.words(), dtype=np.uint32).ravel()
    planes = np.zeros(NPLANES * 12, dtype=np.uint32)
    # spilled programs (sched.spill_pass): side words and the unit's scratch
    nscr = getattr(sc, "nscr", 0)
    side = np.asarray(sc.side_words, dtype=np.uint32) if nscr else None
    scr = np.zeros(max(nscr, 1) * 12, dtype=np.uint32)
    side_p = side.ctypes.data_as(u32p) if side is not None else None
    if device:
        hx.dp_vm_run.argtypes = [u32p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, u32p, ctypes.c_uint32, u32p,
                                 ctypes.c_uint32, ctypes.c_uint64, u32p, ctypes.c_uint32, u32p, u32p, ctypes.c_uint32]
        err = hx.dp_vm_run(code.ctypes.data_as(u32p), sc.nrounds, sc.W, sched.words_per_lane(prog),
                           cst.ctypes.data_as(u32p), len(cst) // 12, slots.ctypes.data_as(u32p), sc.nslots, scalar,
                           planes.ctypes.data_as(u32p), NPLANES, side_p, scr.ctypes.data_as(u32p) if nscr else None,
                           nscr)
        assert err == 0, "dp_vm_run(%s): HIP error %d" % (prog.name, err)
    else:
        hx.hx_vm_run.argtypes = [u32p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, u32p, u32p, ctypes.c_uint64,
                                 u32p, ctypes.c_uint32, ctypes.c_int, u32p, u32p]
        assert hx.hx_vm_run(code.ctypes.data_as(u32p), sc.nrounds, sc.W, sched.words_per_lane(prog),
                            cst.ctypes.data_as(u32p), slots.ctypes.data_as(u32p), scalar, planes.ctypes.data_as(u32p),
                            NPLANES, any_all, side_p, scr.ctypes.data_as(u32p)) == 0
    out = {}
    for name, v in prog.outputs.items():
        op = prog.ops[v]
        if op.kind == "st":
            out[name] = _int(planes[op.imm * 12:op.imm * 12 + 12])
        else:
            s = sc.slot_of[v]
            out[name] = _int(slots[s * 12:s * 12 + 12])
    return out


def assert_same(dev, sim, what):
    for name, s in sim.items():
        d = dev[name]
        # a Montgomery representative in [0, 2p) (canonical for `st` planes) or a raw flag
        ok = (d % P == s * R % P and d < (P if name.startswith("st:") else 2 * P)) or (s in (0, 1) and d == s)
        assert ok, "%s: output %s interpreter %x, simulator %x" % (what, name, d, s)


def load_golden():
    with open(os.path.join(ROOT, "tests", "golden", "golden_v1.json")) as fh:
        return json.load(fh)


def golden_vote_inputs():
    """Program inputs of two valid golden votes and one whose verification fails."""
    g = load_golden()
    bls = gen._oracle()
    out = []
    for v, k in list(zip(g["votes"], g["keys"]))[:2]:
        out.append(gen.vote_inputs(bls, bytes.fromhex(k["pk"]), bytes.fromhex(v["sig"]), bytes.fromhex(v["digest"])))
    bad = [c for c in g["verify"] if c["code"] == 3 and len(c["sig"]) == 192 and len(c["pk"]) == 96]
    for c in bad[:1]:
        out.append(gen.vote_inputs(bls, bytes.fromhex(c["pk"]), bytes.fromhex(c["sig"]), bytes.fromhex(c["hash"])))
    return out
