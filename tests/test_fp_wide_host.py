"""The radix-2^392 ("wide") Montgomery product on the host build: fp_mul_wide (csrc/bls/fp.hpp)
through tests/host/fp_wide_harness.cpp against exact Python integers -- every pair of the range
edges {0, 1, p - 1, p, p + 1, 2p - 1, 2p, 4p - 1}, limb-edge patterns (28-bit and 32-bit limbs all
ones / all zero, the largest top limb below 4p) and 300 seeded random pairs: r = a b 2^-392 mod p
and r <= p + floor(a b / 2^392), the bound the interpreter's missing conditional subtraction rests
on. Then the interpreter's default (per-phase) radix path, exec in tests/host/harness.cpp's
hx_vm_run, on hand-encoded one-phase programs whose ops carry the WIDE bit (tests/fp_wide_cases.py):
products with both pre-adds and a negated y, and eq / sgn0 / lex of the raw values 0, p, 2p, 3p,
1, p + 1, (p +- 1) / 2 + p (and representatives of the values 0, 1, (p -+ 1) / 2, where the flags
flip), whose flags must be those of the value x stands for, x 2^-392 mod p: the same for every
representative of x mod p. Test-only builds."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import fp_wide_cases as wc
from test_host_harness import hx  # noqa: F401  (module fixture: builds libhx.so)
from vm_helpers import ROOT

u32p = ctypes.POINTER(ctypes.c_uint32)
u16p = ctypes.POINTER(ctypes.c_uint16)


def build_wx():
    """libwx.so from tests/host/fp_wide_harness.cpp (built under a per-process name and renamed:
    parallel workers never load a half-written library)"""
    out = os.path.join(ROOT, "tests", "host", "_build", "libwx.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    tmp = "%s.%d" % (out, os.getpid())
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", tmp,
                           os.path.join(ROOT, "tests", "host", "fp_wide_harness.cpp")])
    os.replace(tmp, out)
    lib = ctypes.CDLL(out)
    lib.wx_fp_mul_wide.argtypes = [ctypes.c_uint32, u32p, u32p, u32p]
    lib.wx_fp_mul_wide.restype = None
    lib.wx_pool_consts.argtypes = [u32p, u32p, u16p, ctypes.c_uint32]
    lib.wx_pool_consts.restype = None
    lib.wx_pool_remap.argtypes = [u32p, u32p, ctypes.c_size_t, u16p, ctypes.c_uint32]
    lib.wx_pool_remap.restype = ctypes.c_uint32
    return lib


@pytest.fixture(scope="module")
def wx():
    return build_wx()


def mul_wide(fn, pairs):
    """fn(n, a, b, r) over the pairs -> result integers"""
    a = np.array([w for x, _ in pairs for w in wc.words(x)], dtype=np.uint32)
    b = np.array([w for _, y in pairs for w in wc.words(y)], dtype=np.uint32)
    r = np.zeros(len(pairs) * 12, dtype=np.uint32)
    rc = fn(len(pairs), a.ctypes.data_as(u32p), b.ctypes.data_as(u32p), r.ctypes.data_as(u32p))
    assert not rc, rc
    return [wc.value(r[12 * i:12 * i + 12]) for i in range(len(pairs))]


def test_wide_product_host(wx):
    pairs = wc.product_pairs()
    got = mul_wide(wx.wx_fp_mul_wide, pairs)
    print("\nwide product (host): %d pairs, largest result %.6f p" % (len(pairs), max(got) / wc.P))
    bad = [e for e in (wc.check_product(a, b, r) for (a, b), r in zip(pairs, got)) if e]
    assert not bad, "%d of %d: %s" % (len(bad), len(pairs), bad[:3])


def run_phase_host(hx, ph):  # noqa: F811
    code, slots = ph.encode()
    code = np.array(code, dtype=np.uint32)
    slots = np.array(slots, dtype=np.uint32)
    cst = np.array(wc.fixed_table(), dtype=np.uint32).ravel()
    planes = np.zeros(12, dtype=np.uint32)
    hx.hx_vm_run.argtypes = [u32p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, u32p, u32p, ctypes.c_uint64,
                             u32p, ctypes.c_uint32, ctypes.c_int, u32p, u32p]
    rc = hx.hx_vm_run(code.ctypes.data_as(u32p), 1, ph.W, 4, cst.ctypes.data_as(u32p), slots.ctypes.data_as(u32p), 0,
                      planes.ctypes.data_as(u32p), 1, 0, None, None)
    assert rc == 0, "hx_vm_run: a result outside [0, 2p) (phase %d)" % (-1 - rc)
    return slots


@pytest.mark.parametrize("phase", ["muls", "flags"])
def test_wide_phase_default_path(hx, phase):  # noqa: F811
    """exec's default radix parameter reads the WIDE bit of the phase's product ops."""
    ph = wc.muls_phase() if phase == "muls" else wc.flag_phase()
    bad = ph.check(run_phase_host(hx, ph))
    assert not bad, bad[:3]


def test_same_phase_without_the_bit_is_radix_384(hx):  # noqa: F811
    """The same products without the WIDE bit are a b 2^-384: the bit, nothing else, picks the radix."""
    ph = wc.muls_phase()
    for w in ph.lanes:
        w[3] &= ~wc.sched.WIDE
    out = run_phase_host(hx, ph)
    r384 = pow(1 << 384, -1, wc.P)
    for dst, _, x, y in ph.expect:
        assert wc.value(out[12 * dst:12 * dst + 12]) % wc.P == x * y * r384 % wc.P
