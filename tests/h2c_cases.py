"""Shared by the hash-to-G2 tests (tests/test_h2c_host.py on the host build, tests/test_gpu_h2c.py
on the device): DSTs of every length, the messages, the exceptional field inputs of the map to
the curve with their oracle results, and the VM programs' inputs on those cases with the
simulator's outputs (computed once per process)."""
import contextlib
import functools
import random

import bls12_381 as bls

P = bls.P
DEFAULT_DST = bls.DST_NUL

# (nb0, nbi) of XmdTemplates by DST length: b_0's tail is 36 + L bytes and b_i's message 34 + L,
# each padded with 0x80 and the 8-byte bit count to whole 64-byte blocks
NB_CLASSES = [(0, 19, (1, 1)), (20, 21, (2, 1)), (22, 83, (2, 2)), (84, 85, (3, 2)), (86, 147, (3, 3)),
              (148, 149, (4, 3)), (150, 211, (4, 4)), (212, 213, (5, 4)), (214, 255, (5, 5))]
# both ends of every class
EDGE_LENGTHS = [0, 19, 20, 21, 22, 83, 84, 85, 86, 147, 148, 149, 150, 211, 212, 213, 214, 255]


def nb_of(L):
    for lo, hi, nb in NB_CLASSES:
        if lo <= L <= hi:
            return nb
    raise ValueError(L)


def dst_for(L):
    """A DST of L bytes that varies with the position and with L (no repeated byte pattern that
    would hide a shifted or truncated copy)."""
    return bytes((37 * i + 101 * L + (i * i >> 3) + 1) & 0xFF for i in range(L))


MESSAGES = [bytes(32), b"\xff" * 32, bytes(range(1, 33)), random.Random(0x48324632).randbytes(32)]


def u_cases():
    """The field inputs of the map to the curve that no hashed message reaches, by name:
    (u0, u1) as canonical Fp2 pairs. a, b: seeded random elements."""
    rng = random.Random(0x55535755)
    a = (rng.randrange(1, P), rng.randrange(1, P))
    b = (rng.randrange(1, P), rng.randrange(1, P))
    z = (0, 0)
    return {
        "a": (a, b),                                   # the general case
        "b": (z, b),                                   # u0 = 0: SSWU's tv1 = 0 branch
        "c": (a, z),
        "d": (z, z),                                   # both exceptional, and Q0 = Q1
        "e": (a, a),                                   # Q0 + Q1 is a doubling
        "f": (a, bls.f2_neg(a)),                       # Q1 = -Q0: H is the identity
        "g": ((0, a[1]), (b[0], 0)),                   # sgn0 falls through to c1 / c1 = 0
        "h": ((P - 1, P - 1), (1, P - 1)),
        "i": ((1, 0), (0, 1)),
    }


VM_CASES = ("b", "e", "f")   # the cases that go through the whole-vote programs


def map2_ref(u0, u1):
    """The oracle's curve half of hash_to_G2: affine point, or None for the identity."""
    q0 = bls.iso_map_g2(bls.map_to_curve_sswu(u0))
    q1 = bls.iso_map_g2(bls.map_to_curve_sswu(u1))
    return bls.clear_cofactor_g2(bls.pt_add(bls.Fp2Ops, q0, q1))


@functools.lru_cache(maxsize=None)
def map2_refs():
    return {name: map2_ref(*u) for name, u in u_cases().items()}


def u_inputs(u0, u1):
    return {"u00": u0[0], "u01": u0[1], "u10": u1[0], "u11": u1[1]}


VM_SCALAR = 0xA5C3E1F00F1E3C5B


@functools.lru_cache(maxsize=None)
def vm_runs():
    """[(program name, case name, inputs, scalar, simulator outputs)]: h2g on all nine cases;
    vote, qcpre and votew on VM_CASES with a golden vote's other inputs. The simulator
    (tools/fpvm/sched.simulate) runs once per process."""
    from vm_helpers import build_all, golden_vote_inputs, sched
    import progs
    _, progs_ = build_all()
    vote = golden_vote_inputs()[0]
    runs = []
    for case, (u0, u1) in u_cases().items():
        _, sc, words, _, _ = progs_["h2g"]
        inp = u_inputs(u0, u1)
        runs.append(("h2g", case, inp, 0, sched.simulate(sc, words, inp, 0)))
    for name, ins in (("vote", progs.VOTE_IN), ("qcpre", progs.QCPRE_IN), ("votew", progs.VOTE_IN)):
        _, sc, words, _, _ = progs_[name]
        for case in VM_CASES:
            inp = {n: vote[n] for n in ins}
            inp.update(u_inputs(*u_cases()[case]))
            r = 0 if name == "qcpre" else VM_SCALAR
            runs.append((name, case, inp, r, sched.simulate(sc, words, inp, r)))
    return runs


@contextlib.contextmanager
def orc_dst(dst):
    """The C oracle under another DST (its DST is a process global), restored on exit."""
    import orc
    lib = orc.load()
    lib.orc_set_dst(dst, len(dst))
    try:
        yield orc
    finally:
        lib.orc_set_dst(None, 0)
