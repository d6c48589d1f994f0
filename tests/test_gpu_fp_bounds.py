"""Unit-level device tests of the gfx950 field arithmetic: each primitive of csrc/bls/fp.hpp and
csrc/fpvm.hpp runs on the GPU through the test-only probe (tests/device/fp_probe.hip, built by
`make -C consensus_overlord_amd` as tests/device/_build/libfpprobe.so) on the boundary tables of
tests/fp_cases.py, and is compared with exact Python integers -- and, for the code the host build
shares, with the host harness's limbs bit for bit (both run the same C++ with the same f32
quotient estimate: a difference is a finding about float semantics or code generation). The
Fp-VM programs then run on one wave through the device interpreter (the LDS address select, the
read-first-lane phase header, the prefetch ring, spills and fills) against the simulator.

Each test prints its case count and the largest result in units of p before it asserts (pytest
-s shows them): how close the hardware runs to each bound of the contract."""
import ctypes
import os

import pytest

import fp_cases as fc
import vm_edge
from fp_run import Backend, first_failures
from test_host_harness import hx  # noqa: F401  (module fixture: builds libhx.so)
from vm_helpers import ROOT, assert_same, build_all, gen, golden_vote_inputs, load_golden, run_vm, sched

import progs  # noqa: E402  (tools/fpvm: vm_helpers puts it on the path)

pytestmark = pytest.mark.gpu

PROBE = os.path.join(ROOT, "tests", "device", "_build", "libfpprobe.so")


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(PROBE):
        pytest.fail("%s is missing: run build() (make -C consensus_overlord_amd) first" % PROBE)
    return ctypes.CDLL(PROBE)


@pytest.fixture(scope="module")
def dev(probe):
    return Backend(probe, device=True)


@pytest.fixture(scope="module")
def host(hx):  # noqa: F811
    return Backend(hx, device=False)


def report(what, results):
    print("\n%s: %d cases, largest result %.6f p" % (what, len(results), max(results) / fc.P))


# ------------------------------------------------------------------------------ products
@pytest.fixture(scope="module")
def product_table():
    """The pairs, the aliased squares, and their closed-form results (computed once)."""
    pairs, squares = fc.product_cases(), fc.square_cases()
    return pairs, squares, [fc.mont28(a, b) for a, b in pairs], [fc.mont28(a, a) for a, _ in squares]


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_products_exact(dev, product_table, variant):
    """fp_mul as the product library gets it (0), fp_mul28_gfx950_2acc (1) and the portable
    fp_mul28 (2): output limbs equal the closed-form Montgomery result on every pair, and on
    every edge squared with one register array for both operands."""
    pairs, squares, want, want_sq = product_table
    got = dev.fp_mul(pairs, variant)
    got_sq = dev.fp_mul(squares, variant, alias=True)
    report("product variant %d" % variant, got + got_sq)
    first_failures(["a=%x b=%x: got %x, want %x" % (a, b, g, w) if g != w else None
                    for (a, b), g, w in zip(pairs, got, want)], "variant %d" % variant)
    first_failures(["a=%x squared (aliased): got %x, want %x" % (a, g, w) if g != w else None
                    for (a, _), g, w in zip(squares, got_sq, want_sq)], "variant %d, aliased squares" % variant)


def test_product32_congruent(dev):
    """fp_mul_gfx950 (the 12 x 32 product of the A/B build, R = 2^384): the congruence and the
    derived bound r < max(p, ceil(a b / 2^384))."""
    pairs, squares = fc.product_cases(), fc.square_cases()
    got = dev.fp_mul(pairs, 3)
    got_sq = dev.fp_mul(squares, 3, alias=True)
    report("product variant 3", got + got_sq)
    first_failures([fc.check_product(a, b, r, exact=False) for (a, b), r in zip(pairs + squares, got + got_sq)],
                   "fp_mul_gfx950")


# ------------------------------------------------------------------------------ linear ops
def same_limbs(what, cases, got, ref):
    first_failures(["%s %s: device %s, host %s" % (what, fc._show(c), g, h) if g != h else None
                    for c, g, h in zip(cases, got, ref)], "%s, device limbs against the host build's" % what)


def test_pre_add2_exact(dev, host):
    cases = fc.pre_add2_cases()
    got = dev.pre_add2(cases)
    report("pre_add2", [max(g) for g in got])
    first_failures([None if g == fc.pre_add2_expect(*c) else "pre_add2 %s: got %x, %x" % (fc._show(c), g[0], g[1])
                    for c, g in zip(cases, got)], "pre_add2")
    same_limbs("pre_add2", cases, got, host.pre_add2(cases))


def test_lin_unit_bounds(dev, host):
    cases = fc.lin_unit_cases() + fc.lin_unit_flip_cases()
    got = dev.lin_unit(cases)
    report("lin_sum + scale_reduce", got)
    first_failures([fc.check_lin_unit(c, r) for c, r in zip(cases, got)], "lin_sum + scale_reduce")
    same_limbs("lin_unit", cases, got, host.lin_unit(cases))


def test_lin_mad_bounds(dev, host):
    cases = fc.lin_mad_cases() + fc.lin_mad_flip_cases()
    got = dev.lin_mad(cases)
    report("lin_mad", got)
    first_failures([fc.check_lin_mad(c, r) for c, r in zip(cases, got)], "lin_mad")
    same_limbs("lin_mad", cases, got, host.lin_mad(cases))


def test_canon(dev, host):
    vals = fc.canon_cases()
    got = dev.canon(vals)
    report("canon", got)
    assert got == [v % fc.P for v in vals]
    assert got == host.canon(vals)


def test_fp_inv_device(dev, host):
    vals = fc.fp_inv_values()
    got = dev.fp_inv(vals)
    report("fp_inv", got)
    first_failures(["fp_inv(%x): got %x" % (a, g) if g != fc.fp_inv_expect(a) else None for a, g in zip(vals, got)],
                   "fp_inv")
    assert got == host.fp_inv(vals)


def test_probe_rejects_bad_arguments(probe):
    """The wrappers refuse empty and null inputs, unknown variants and programs that reference
    what was not passed -- with an error code, before any launch."""
    u32p = ctypes.POINTER(ctypes.c_uint32)
    buf = (ctypes.c_uint32 * 48)()
    p = ctypes.cast(buf, u32p)
    probe.dp_fp_mul.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, u32p, u32p, u32p]
    assert probe.dp_fp_mul(0, 0, 0, p, p, p) != 0
    assert probe.dp_fp_mul(4, 0, 1, p, p, p) != 0
    assert probe.dp_fp_mul(0, 0, 1, p, None, p) != 0
    probe.dp_canon.argtypes = [ctypes.c_uint32, u32p, u32p]
    assert probe.dp_canon(1, None, p) != 0
    probe.dp_vm_run.argtypes = [u32p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, u32p, ctypes.c_uint32, u32p,
                                ctypes.c_uint32, ctypes.c_uint64, u32p, ctypes.c_uint32, u32p, u32p, ctypes.c_uint32]
    # one NOP phase of one lane: fine with 1 slot and 1 constant; refused when operand A names slot 3
    # of 1 or a constant past the table, when an `st` names plane 5 of 1, and when the header has
    # a block run that reads constants the table lacks (H_LINNEG: KTAB + n, H_SELB: KZERO)
    for w0, w1, ok in ((0, 0, True), (0, 3, False), (0, 0x800 | 2, False), (11 | 5 << 16 | 1 << 28, 0, False),
                       (1 << 25 | 1 << 26, 0, False), (1 << 25 | 1 << 29, 0, False)):
        code = (ctypes.c_uint32 * 4)(w0, w1, 0, 0)
        err = probe.dp_vm_run(ctypes.cast(code, u32p), 1, 1, 4, p, 1, p, 1, 0, p, 1, None, None, 0)
        assert (err == 0) == ok, (hex(w0), hex(w1), err)


# ------------------------------------------------------------------------------ VM programs
@pytest.fixture(scope="module")
def built():
    return build_all()


@pytest.fixture(scope="module")
def golden_votes():
    return golden_vote_inputs()


def test_vm_programs_on_device(probe, built, golden_votes):
    """The generated programs on one wave of the device interpreter == the simulator, on the
    golden votes: vote (the spilled form gen.py builds, with side words), vote_t, rs, fold,
    final, sigchk, pkchk, vsame, h2g, votew, final1. Every output: congruent, below 2p, and
    canonical for `st` planes."""
    consts, progs_ = built
    P = fc.P
    g = golden_votes
    bls = gen._oracle()

    def run(name, inp, scalar=0):
        _, sc, words, _, _ = progs_[name]
        sim = sched.simulate(sc, words, inp, scalar)
        assert_same(run_vm(probe, consts, sc, words, inp, scalar, 0, device=True), sim, name)
        return sim

    assert getattr(progs_["vote"][1], "nscr", 0) > 0, "the vote program is built with spills"
    r = 0xD7A1C3B5E9F20486
    parts = []
    for k, inp in enumerate(g):
        o = run("vote", inp, r)
        run("sigchk", {n: inp[n] for n in progs.SIGCHK_IN})
        run("pkchk", {n: inp[n] for n in progs.PKCHK_IN})
        run("vsame", {n: inp[n] for n in progs.VSAME_IN}, r)
        if k < 2:
            o = {(n[3:] if n.startswith("st:") else n): v for n, v in o.items()}
            rsim = run("rs", {n: o[n] for n in progs.RS_IN}, r)
            o.update({n[3:]: v for n, v in rsim.items()})
            parts.append(o)
    gold = load_golden()
    pk = bls.g1_from_bytes(bytes.fromhex(gold["keys"][0]["pk"]))
    tin = {n: g[0][n] for n in ("sig_x0", "sig_x1", "sig_sort", "u00", "u01", "u10", "u11")}
    tin.update(pk_X=pk[0] * 5 % P, pk_Y=pk[1] * 5 % P, pk_Z=5)
    run("vote_t", tin, r)
    run("h2g", {n: g[0][n] for n in progs.H2G_IN})
    fin = {}
    for k in range(progs.FOLD_K):
        for j in range(12):
            fin["F%d_%d" % (k, j)] = parts[k]["f%d" % j] if k < len(parts) else (1 if j == 0 else 0)
        for j in range(6):
            fin["S%d_%d" % (k, j)] = parts[k]["s%d" % j] if k < len(parts) else (1 if j == 2 else 0)
    run("fold", fin)
    assert run("final", fin) == {"ok": 1}
    o = run("votew", g[0], 0x9E3779B97F4A7C15)
    assert run("final1", {"f%d" % j: o["st:f%d" % j] for j in range(12)}) == {"ok": 1}


def test_vm_edge_program_on_device(probe):
    """The synthetic edge program (tests/vm_edge.py: raw slots p, 2p - 1, p - 1, 0; pre-adds up
    to 4p - 1; equality of values equal only modulo p) on the device interpreter: flags and
    stored planes equal the Python evaluation modulo p."""
    vm_edge.run_and_check(probe, device=True)
