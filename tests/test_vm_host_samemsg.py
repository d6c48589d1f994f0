"""The per-vote programs of the same-message path (vsame, vsame_t, vsame8, vsame8_t) and the
key-sum addition (g1padd) on the interpreter's own code (consensus_overlord_amd/csrc/fpvm.hpp exec,
host build), in both interpreter modes: interpreter == slot-level simulator == integers. The
8-lane programs run every same-message batch of VSAME8_MIN votes or more and otherwise meet no
interpreter below the whole-batch GPU tests.

Each program runs golden vote 0 under the RLC edge values of tests/samemsg_cases.py (a = 0, b = 0,
a = b, bit 31, bit 63, all ones, 0) and a random one: the flags, sigma, tau = -psi^2(sigma), and
r pk = [rlc_scalar(r)] pk compared projectively (Z = 0 at r = 0). g1padd runs the doubling,
cancelling and identity operands of the key-sum cases. The point classes reach the four programs
through point_vm.WHOLE (tests/test_vm_host_points.py)."""
import random

import pytest

import bls12_381 as bls
import point_vm
import samemsg_cases as sc
from test_host_harness import hx  # noqa: F401  (module fixture: builds libhx.so)
from vm_helpers import P, build_all, golden_vote_inputs, load_golden

SCALARS = tuple(sc.RLC_EDGES) + (("random", random.Random(0x51C).getrandbits(64)),)
PROGRAMS = ("vsame", "vsame_t", "vsame8", "vsame8_t")


def _golden_points():
    g = load_golden()
    pk = bls.g1_from_bytes(bytes.fromhex(g["keys"][0]["pk"]))
    sig = bls.g2_from_bytes(bytes.fromhex(g["votes"][0]["sig"]))
    return pk, sig


@pytest.mark.parametrize("any_all", [0, 1])
@pytest.mark.parametrize("name", PROGRAMS)
def test_vsame_programs_on_the_rlc_edges(hx, name, any_all):  # noqa: F811
    _, progs_ = build_all()
    ins = progs_[name][3]
    pk, sig = _golden_points()
    base = dict(golden_vote_inputs()[0])
    base.update(pk_X=pk[0] * 11 % P, pk_Y=pk[1] * 11 % P, pk_Z=11)
    inp = {k: base[k] for k in ins}
    tau = sc.tau_of(sig)
    for label, z in SCALARS:
        sim = point_vm._run(hx, False, any_all, name, "golden 0, r %s" % label, inp, z)
        what = "%s r=%s" % (name, label)
        assert sim["sig_ok"] == sim["sig_grp"] == 1, what
        if "pk_x" in ins:
            assert sim["pk_ok"] == sim["pk_grp"] == 1, what
        assert tuple(sim["st:q%d" % k] for k in range(4)) == sig[0] + sig[1], what + ": sigma"
        assert tuple(sim["st:t%d" % k] for k in range(4)) == tau[0] + tau[1], what + ": tau"
        X, Y, Z = (sim["st:r%d" % k] for k in range(3))
        if z == 0:      # the kernels never pass 0 (vote_scalar gives 1 for it); the program gives the identity
            assert Z == 0 and Y != 0, what + ": r pk at r = 0"
        else:
            zi = pow(Z, -1, P)
            assert (X * zi % P, Y * zi % P) == bls.pt_mul(sc.F1, pk, sc.rlc_scalar(z)), what + ": r pk"


def _proj(pt, z):
    return (0, z, 0) if pt is None else (pt[0] * z % P, pt[1] * z % P, z)


@pytest.mark.parametrize("any_all", [0, 1])
def test_g1padd_on_doubling_cancelling_and_identity_operands(hx, any_all):  # noqa: F811
    s, t = 0x1234567, 0x89ABCDE
    A, B = sc.g1_mul(s), sc.g1_mul(t)
    nA = bls.pt_neg(sc.F1, A)
    ops = [("A + B", _proj(A, 5), _proj(B, 7), sc.g1_mul(s + t)),
           ("A + A", _proj(A, 1), _proj(A, 1), sc.g1_mul(2 * s)),
           ("A + A, other Z", _proj(A, 5), _proj(A, 9), sc.g1_mul(2 * s)),
           ("A + (-A)", _proj(A, 5), _proj(nA, 5), None),
           ("A + (-A), other Z", _proj(A, 3), _proj(nA, 8), None),
           ("O + A, (0 : 1 : 0)", _proj(None, 1), _proj(A, 4), A),
           ("A + O, (0 : z : 0)", _proj(A, 4), _proj(None, 0xABCDEF), A),
           ("O + O", _proj(None, 1), _proj(None, 77), None)]
    for label, a, b, want in ops:
        inp = dict(zip(["a0", "a1", "a2", "b0", "b1", "b2"], a + b))
        sim = point_vm._run(hx, False, any_all, "g1padd", label, inp)
        X, Y, Z = sim["s0"], sim["s1"], sim["s2"]
        if want is None:
            assert Z == 0 and Y != 0, label
        else:
            zi = pow(Z, -1, P)
            assert (X * zi % P, Y * zi % P) == want, label
