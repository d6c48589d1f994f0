"""The radix-2^392 ("wide") arithmetic on gfx950 through the test-only probe
tests/device/fp_wide_probe.hip (built by `make -C consensus_overlord_amd` as
tests/device/_build/libfpwideprobe.so): the generated wide product fp_mul28w_gfx950 on the operand
table of the host test (tests/fp_wide_cases.py: range edges, limb-edge patterns, 300 seeded random
pairs; 64 lanes per workgroup, a handful of workgroups) with the same two assertions against
exact integers -- r = a b 2^-392 mod p and r <= p + floor(a b / 2^392) -- and the hand-encoded
product and flag phases through vm::run<.., 392>, the compile-time radix the vote pool binds."""
import ctypes
import os

import numpy as np
import pytest

import fp_wide_cases as wc
from test_fp_wide_host import mul_wide, u32p
from vm_helpers import ROOT

pytestmark = pytest.mark.gpu

PROBE = os.path.join(ROOT, "tests", "device", "_build", "libfpwideprobe.so")


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(PROBE):
        pytest.fail("%s is missing: run build() (make -C consensus_overlord_amd) first" % PROBE)
    lib = ctypes.CDLL(PROBE)
    lib.dw_fp_mul_wide.argtypes = [ctypes.c_uint32, u32p, u32p, u32p]
    lib.dw_vm_run392.argtypes = [u32p, ctypes.c_uint32, ctypes.c_uint32, u32p, ctypes.c_uint32, u32p, ctypes.c_uint32]
    return lib


def test_wide_product_device(probe):
    pairs = wc.product_pairs()
    got = mul_wide(probe.dw_fp_mul_wide, pairs)
    print("\nwide product (gfx950): %d pairs, largest result %.6f p" % (len(pairs), max(got) / wc.P))
    bad = [e for e in (wc.check_product(a, b, r) for (a, b), r in zip(pairs, got)) if e]
    assert not bad, "%d of %d: %s" % (len(bad), len(pairs), bad[:3])


@pytest.mark.parametrize("phase", ["muls", "flags"])
def test_wide_phase_fixed_radix(probe, phase):
    ph = wc.muls_phase() if phase == "muls" else wc.flag_phase()
    code, slots = ph.encode()
    code = np.array(code, dtype=np.uint32)
    slots = np.array(slots, dtype=np.uint32)
    cst = np.array(wc.fixed_table(), dtype=np.uint32).ravel()
    err = probe.dw_vm_run392(code.ctypes.data_as(u32p), 1, ph.W, cst.ctypes.data_as(u32p), len(cst) // 12,
                             slots.ctypes.data_as(u32p), len(slots) // 12)
    assert err == 0, "dw_vm_run392: HIP error %d" % err
    bad = ph.check(slots)
    assert not bad, bad[:3]


def test_probe_rejects_bad_arguments(probe):
    p = ctypes.cast((ctypes.c_uint32 * 96)(), u32p)
    assert probe.dw_fp_mul_wide(0, p, p, p) != 0
    assert probe.dw_fp_mul_wide(1, p, None, p) != 0
    # operand A names slot 3 of 1; a constant past the table; an `st` op
    for w0, w1 in ((1, 3), (1, 0x800 | 9), (11, 0)):
        code = (ctypes.c_uint32 * 4)(w0, w1, 0, 0)
        assert probe.dw_vm_run392(ctypes.cast(code, u32p), 1, 1, p, 7, p, 1) != 0
