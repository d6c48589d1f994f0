"""Runs the case tables of tests/fp_cases.py through one backend: the host harness
(tests/host/harness.cpp hx_*) or the device probe (tests/device/fp_probe.hip dp_*, which return
a HIP error code). Every function returns Python integers, one per case."""
import ctypes

import numpy as np

import fp_cases as fc

u32p = ctypes.POINTER(ctypes.c_uint32)
u8p = ctypes.POINTER(ctypes.c_uint8)
i8p = ctypes.POINTER(ctypes.c_int8)
u32 = ctypes.c_uint32


def _p(arr, t=u32p):
    return arr.ctypes.data_as(t)


class Backend:
    def __init__(self, lib, device):
        self.lib = lib
        self.device = device
        self.pre = "dp_" if device else "hx_"

    def _call(self, name, argtypes, *args):
        fn = getattr(self.lib, self.pre + name)
        fn.argtypes = argtypes
        fn.restype = ctypes.c_int if self.device else None
        err = fn(*args)
        assert not self.device or err == 0, "%s%s: HIP error %d" % (self.pre, name, err)

    def fp_mul(self, pairs, variant=0, alias=False):
        """variant / alias: the device probe's (the host build has its one fp_mul)."""
        a = fc.pack([x for x, _ in pairs])
        b = fc.pack([y for _, y in pairs])
        r = np.zeros_like(a)
        if self.device:
            self._call("fp_mul", [ctypes.c_int, ctypes.c_int, u32, u32p, u32p, u32p], variant, int(alias), len(pairs),
                       _p(a), None if alias else _p(b), _p(r))
        else:
            assert variant == 0 and not alias
            self._call("fp_mul", [u32, u32p, u32p, u32p], len(pairs), _p(a), _p(b), _p(r))
        return fc.unpack(r)

    def _abcd(self, cases):
        return [fc.pack([c[j] for c in cases]) for j in range(4)]

    def pre_add2(self, cases):
        A, B, C, D = self._abcd(cases)
        flags = np.array([c[4] | c[5] << 1 for c in cases], dtype=np.uint8)
        x, y = np.zeros_like(A), np.zeros_like(A)
        self._call("pre_add2", [u32, u32p, u32p, u32p, u32p, u8p, u32p, u32p], len(cases), _p(A), _p(B), _p(C), _p(D),
                   _p(flags, u8p), _p(x), _p(y))
        return list(zip(fc.unpack(x), fc.unpack(y)))

    def lin_unit(self, cases):
        A, B, C, D = self._abcd(cases)
        ctl = np.array([fc.lin_ctl(*c[4:]) for c in cases], dtype=np.uint32)
        cst = fc.const_table()
        r = np.zeros_like(A)
        if self.device:
            self._call("lin_unit", [u32, u32p, u32p, u32p, u32p, u32p, u32p, u32, u32p], len(cases), _p(A), _p(B), _p(C),
                       _p(D), _p(ctl), _p(cst), len(cst), _p(r))
        else:
            self._call("lin_unit", [u32, u32p, u32p, u32p, u32p, u32p, u32p, u32p], len(cases), _p(A), _p(B), _p(C),
                       _p(D), _p(ctl), _p(cst), _p(r))
        return fc.unpack(r)

    def lin_mad(self, cases):
        A, B, C, D = self._abcd(cases)
        cf = np.array([c[4:8] for c in cases], dtype=np.int8).ravel()
        r = np.zeros_like(A)
        self._call("lin_mad", [u32, u32p, u32p, u32p, u32p, i8p, u32p], len(cases), _p(A), _p(B), _p(C), _p(D),
                   _p(cf, i8p), _p(r))
        return fc.unpack(r)

    def canon(self, vals):
        a = fc.pack(vals)
        r = np.zeros_like(a)
        self._call("canon", [u32, u32p, u32p], len(vals), _p(a), _p(r))
        return fc.unpack(r)

    def fp_inv(self, vals):
        """Raw inverses: r3 = raw R makes the closing Montgomery product the identity."""
        a = fc.pack(vals)
        r3 = fc.pack([fc.R % fc.P])
        r = np.zeros_like(a)
        self._call("fp_inv", [u32, u32p, u32p, u32p], len(vals), _p(a), _p(r3), _p(r))
        return fc.unpack(r)


def first_failures(msgs, what, limit=8):
    """assert that no check returned a message; the report names the first `limit` cases."""
    bad = [m for m in msgs if m]
    assert not bad, "%s: %d of %d cases fail\n%s" % (what, len(bad), len(msgs), "\n".join(bad[:limit]))
