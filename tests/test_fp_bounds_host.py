"""The interpreter's arithmetic primitives (csrc/bls/fp.hpp, csrc/fpvm.hpp; host build in
tests/host/harness.cpp) on the boundary tables of tests/fp_cases.py against exact Python
integers: the product's operand range [0, 4p), the skewed carry / borrow chains of pre_add2 and
lin_sum, the f32 quotient estimate of scale_reduce and lin_mad where k s sits one above or below
a multiple of p, and canon. The host product is the 12 x 32 CIOS loop (congruence and the
derived bound only); the 28-bit device products are checked limb for limb by
tests/test_gpu_fp_bounds.py, which also requires the device's limbs to equal this build's."""
import pytest

import fp_cases as fc
import vm_edge
from fp_run import Backend, first_failures
from test_host_harness import hx  # noqa: F401  (module fixture: builds libhx.so)


@pytest.fixture(scope="module")
def host(hx):  # noqa: F811
    return Backend(hx, device=False)


def test_case_table():
    """The table itself: sizes, ranges, and the closed-form product inside its derived bounds."""
    e = fc.product_edges()
    assert len(set(e)) == len(e) and all(0 <= v < 4 * fc.P for v in e)
    assert {0, fc.P, 4 * fc.P - 1, 2 ** 382, fc.R % fc.P} <= set(e)
    pairs = fc.product_cases()
    assert len(pairs) == len(e) ** 2 + 4096 + 1024
    worst = 0
    for a, b in pairs + fc.square_cases():
        r = fc.mont28(a, b)
        assert r % fc.P == a * b * fc.RINV % fc.P and r < fc.product_bound(a, b)
        worst = max(worst, r)
    assert worst < 1.63 * fc.P   # fp_mul28.hpp: r < 1.63 p
    for c in fc.pre_add2_cases():
        assert all(0 <= v < 2 * fc.P for v in c[:4]) and (c[5] or not c[4])
    units = fc.lin_unit_cases()
    assert all(0 <= v < 2 * fc.P for c in units for v in c[:4]) and all(1 <= c[7] <= 15 for c in units)
    assert {(c[4], c[5], c[6], c[8]) for c in units} == {(x, y, z, h) for x in (0, 1) for y in (0, 1)
                                                          for z in (0, 1) for h in (0, 1)}
    # the adversarial sums: for every k and every multiple m p up to 8 k p some case has k s within
    # k of it on either side
    for k in (1, 7, 15):
        ks = sorted(k * fc.lin_unit_sum(*c[:7]) for c in units if c[7] == k)
        for m in range(1, 8 * k):
            assert any(0 <= v - m * fc.P <= k + 2 for v in ks) and any(0 < m * fc.P - v <= 2 * k + 2 for v in ks), (k, m)
    assert len(fc.lin_mad_cases()) == 625 * 6 + 81 * 4
    assert all(0 <= v < 2 * fc.P for v in fc.canon_cases())
    assert len(fc.fp_inv_values()) == 513 and all(0 <= v < fc.P for v in fc.fp_inv_values())


def test_product_host(host):
    pairs = fc.product_cases() + fc.square_cases()
    got = host.fp_mul(pairs)
    first_failures([fc.check_product(a, b, r, exact=False) for (a, b), r in zip(pairs, got)], "host fp_mul")


def test_pre_add2_exact(host):
    cases = fc.pre_add2_cases()
    got = host.pre_add2(cases)
    first_failures([None if g == fc.pre_add2_expect(*c) else "pre_add2 %s: got %x, %x" % (fc._show(c), g[0], g[1])
                    for c, g in zip(cases, got)], "pre_add2")


def test_lin_unit_bounds(host):
    cases = fc.lin_unit_cases() + fc.lin_unit_flip_cases()
    got = host.lin_unit(cases)
    first_failures([fc.check_lin_unit(c, r) for c, r in zip(cases, got)], "lin_sum + scale_reduce")
    # the flip cases reach both answers of the estimate: the floor, and one less
    n = len(fc.lin_unit_cases())
    short = [(c[7] * fc.lin_unit_sum(*c[:7]) - r) // fc.P < c[7] * fc.lin_unit_sum(*c[:7]) // fc.P
             for c, r in zip(cases[n:], got[n:])]
    assert any(short) and not all(short)


def test_lin_mad_bounds(host):
    cases = fc.lin_mad_cases() + fc.lin_mad_flip_cases()
    got = host.lin_mad(cases)
    first_failures([fc.check_lin_mad(c, r) for c, r in zip(cases, got)], "lin_mad")
    # the flip cases bracket the estimate's step for every quotient m: q = m - 1 at the lowest
    # offset, m at the highest (seven offsets per m)
    n = len(fc.lin_mad_cases())
    qs = [(c[4] * sum(c[:4]) - r) // fc.P for c, r in zip(cases[n:], got[n:])]
    for m in range(1, 120):
        assert qs[7 * (m - 1)] == m - 1 and qs[7 * (m - 1) + 6] == m, (m, qs[7 * (m - 1):7 * m])


def test_canon(host):
    vals = fc.canon_cases()
    assert host.canon(vals) == [v % fc.P for v in vals]


def test_fp_inv_array(host):
    vals = fc.fp_inv_values()
    assert host.fp_inv(vals) == [fc.fp_inv_expect(a) for a in vals]


@pytest.mark.parametrize("any_all", [0, 1])
def test_vm_edge_program_on_interpreter(hx, any_all):  # noqa: F811
    """The synthetic edge program (tests/vm_edge.py) through the host interpreter: flags and
    stored planes equal the Python evaluation modulo p, each lane alone and with every
    wave-uniform block run for every lane."""
    vm_edge.run_and_check(hx, device=False, any_all=any_all)
