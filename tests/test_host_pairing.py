"""The one-lane tower and pairing (consensus_overlord_amd/csrc/bls/tower.hpp, pairing.hpp: what
k_verify_agg and the host build run), compiled for the host (tests/host/harness.cpp), on the
crafted cases of tests/pairing_cases.py against the plain-integer reference
(tests/pairing_ref.py): fp12_mul, fp12_sqr, fp12_cyc_sqr, fp12_frob, fp12_inv, fp12_mul_by_014,
fp12_cyc_exp_x and final_exponentiation value for value, miller_loop after the reference's final
exponentiation."""
import ctypes

import pairing_cases as pcs
import pairing_ref as ref
from test_host_harness import hx  # noqa: F401  (module fixture: builds libhx.so)

MUL, SQR, CYC_SQR, FROB, INV, EXP_X, FE = range(7)


def _be(vals):
    return b"".join(int(v).to_bytes(48, "big") for v in vals)


def _tower(buf):
    return ref.unflat([int.from_bytes(buf.raw[48 * i:48 * i + 48], "big") for i in range(12)])


def _op(hx, op, a, b=None):  # noqa: F811
    out = ctypes.create_string_buffer(576)
    assert hx.hx_fp12_op(op, _be(ref.flat(a)), _be(ref.flat(b)) if b is not None else None, out) == 0
    return _tower(out)


def test_tower_ops_on_every_case(hx):  # noqa: F811
    n = 0
    for c in pcs.op_cases():
        assert _op(hx, MUL, c.a, c.b) == c.mul, c.name
        assert _op(hx, MUL, c.b, c.a) == c.mul, c.name
        assert _op(hx, SQR, c.a) == c.sqr, c.name
        assert _op(hx, FROB, c.a) == c.frob, c.name
        assert _op(hx, INV, c.a) == c.inv, c.name      # 0 -> 0 included
        n += 1
    for c in pcs.fe_cases():
        p = ref.to_poly(c.f)
        assert _op(hx, FROB, c.f) == ref.from_poly(ref.frob(p)), c.name
        assert _op(hx, SQR, c.f) == ref.from_poly(ref.mul(p, p)), c.name
        assert _op(hx, INV, c.f) == ref.from_poly(ref.inv(p)), c.name
        n += 1
    assert n == 7 + 26


def test_mul_by_014_on_every_line(hx):  # noqa: F811
    for c in pcs.line_cases():
        out = ctypes.create_string_buffer(576)
        assert hx.hx_fp12_mul_by_014(_be(ref.flat(c.f)), _be(c.l0 + c.l1 + c.l4), out) == 0
        assert _tower(out) == c.out, c.name
    assert len(pcs.line_cases()) == 5


def test_cyclotomic_square_and_exp_x(hx):  # noqa: F811
    for c in pcs.cyc_cases():
        assert _op(hx, CYC_SQR, c.a) == c.sqr, c.name
        assert _op(hx, EXP_X, c.a) == c.expx, c.name
    assert len(pcs.cyc_cases()) == 4


def test_final_exponentiation_on_every_case(hx):  # noqa: F811
    for c in pcs.fe_cases():
        assert _op(hx, FE, c.f) == c.fe, c.name
    assert len(pcs.fe_cases()) == 26


def test_miller_loop_after_the_reference_fe(hx):  # noqa: F811
    """every pair of every Miller case, affine on both sides (this loop takes no projective
    input): the product of the values exponentiates to the case's pairing"""
    n = 0
    for c in pcs.miller_cases():
        m = ref.ONE
        for p_, q_ in c.pairs:
            pa, qa = pcs.aff1(p_), pcs.aff2(q_)
            out = ctypes.create_string_buffer(576)
            assert hx.hx_miller_loop(_be(pa), _be(qa[0] + qa[1]), out) == 0
            m = ref.mul(m, ref.to_poly(_tower(out)))
            n += 1
        assert ref.from_poly(ref.final_exp(m)) == c.fe, c.name
    assert n == 14


def test_bad_arguments_are_refused(hx):  # noqa: F811
    out = ctypes.create_string_buffer(576)
    one = _be(ref.flat(pcs.ONE_T))
    assert hx.hx_fp12_op(7, one, one, out) == -2
    assert hx.hx_fp12_op(SQR, _be([ref.P] + [0] * 11), None, out) == -1
