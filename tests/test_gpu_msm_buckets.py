"""The G2 Pippenger MSM kernels (csrc/msm.hpp) on crafted buckets against exact sums.

Through the batch path the MSM's shape follows the RLC digits, which are SplitMix64 outputs: a
test cannot choose them, and evenly spread digits never fill a bucket. The test-only probe
(tests/device/msm_probe.hip, built by `make -C consensus_overlord_amd` as
tests/device/_build/libmsmprobe.so) includes the product translation unit whole and calls the
product's own launch code on a histogram and sorted entries the test supplies: buckets of
1 .. 513 entries (tree levels 0-9, up to ten 64-entry chunks), everything in one bucket, and
buckets, bit planes and window-combination steps whose sums double, cancel, or add identities.

The reference is tests/msm_cases.py: oracle/py/bls12_381.py point arithmetic on Python integers,
summed straight from the definition (tests/test_msm_cases.py checks it without a GPU). The
comparison is exact: the device limbs leave Montgomery form, a device identity is Z = 0,
otherwise (X/Z, Y/Z) must equal the affine reference. Every case compares every non-empty
bucket's sum, all 32 bit-plane sums and S, in that order, so a failure names the stage."""
import ctypes
import os

import numpy as np
import pytest

import bls12_381 as bls
import msm_cases as mc
from vm_helpers import ROOT

pytestmark = pytest.mark.gpu

PROBE = os.path.join(ROOT, "tests", "device", "_build", "libmsmprobe.so")
u32p = ctypes.POINTER(ctypes.c_uint32)
i32p = ctypes.POINTER(ctypes.c_int32)
HIP_INVALID_VALUE = 1


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(PROBE):
        pytest.fail("%s is missing: run build() (make -C consensus_overlord_amd) first" % PROBE)
    lib = ctypes.CDLL(PROBE)
    lib.mp_sort.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, i32p, u32p, u32p, u32p, u32p]
    lib.mp_trees.argtypes = [ctypes.c_uint32, u32p, u32p, u32p, u32p, u32p, u32p, u32p]
    lib.mp_msm.argtypes = [ctypes.c_uint32, u32p, u32p, ctypes.c_uint64, ctypes.c_uint64, i32p, u32p]
    for f in (lib.mp_sort, lib.mp_trees, lib.mp_msm):
        f.restype = ctypes.c_int
    lib.mp_close.restype = None
    yield lib
    lib.mp_close()


def _u32(vals):
    return np.ascontiguousarray(np.array(vals, dtype=np.uint32).reshape(-1))


def _p(arr, t=u32p):
    return arr.ctypes.data_as(t)


def run_trees(probe, case):
    """-> ({bucket: point}, [T_t], S) of the device, as affine points (None: the identity)"""
    sigma, tau = _u32(mc.point_words(case.sigma)), _u32(mc.point_words(case.tau))
    cnt, ent = _u32(case.cnt()), _u32(case.ent() or [0])
    B = np.zeros(mc.NB * 72, dtype=np.uint32)
    T = np.zeros(mc.NT * 72, dtype=np.uint32)
    S = np.zeros(72, dtype=np.uint32)
    rc = probe.mp_trees(case.n, _p(sigma), _p(tau), _p(cnt), _p(ent), _p(B), _p(T), _p(S))
    assert rc == 0, "mp_trees(%s) returned %d" % (case.name, rc)
    return ({b: mc.from_words(B[72 * b:72 * b + 72]) for b in case.buckets},
            [mc.from_words(T[72 * t:72 * t + 72]) for t in range(mc.NT)], mc.from_words(S))


def same(x, y):
    return bls.pt_eq(mc.F, x, y)


def check_case(probe, case):
    got_b, got_t, got_s = run_trees(probe, case)
    want_b, want_t, want_s = case.bucket_sums(), case.plane_sums(), case.result()
    assert sorted(got_b) == sorted(want_b)
    bad = [(b, len(case.buckets[b])) for b in sorted(want_b) if not same(got_b[b], want_b[b])]
    assert not bad, "%s: bucket sums differ (bucket, entries): %s" % (case.name, bad)
    bad = [t for t in range(mc.NT) if not same(got_t[t], want_t[t])]
    assert not bad, "%s: bit-plane sums T_t differ at t = %s" % (case.name, bad)
    assert same(got_s, want_s), "%s: S differs from sum_t 2^t T_t" % case.name


# ------------------------------------------------------------------------------ bucket sizes
@pytest.mark.parametrize("order", (0, 1))
def test_bucket_sizes(probe, order):
    """counts 1 .. 513 at both ends of every window and in the middle, the rest empty; the second
    run has every bucket's entries in another order and must give the same sums"""
    case = mc.size_case(order)
    cnt = case.cnt()
    assert sorted(c for c in cnt if c) == sorted(mc.SIZE_COUNTS)
    assert max(mc.levels(c) for c in cnt if c) == 10 and max(mc.chunks(c) for c in cnt) >= 9
    check_case(probe, case)


@pytest.mark.parametrize("b", mc.FULL_BUCKETS)
def test_one_bucket_holds_everything(probe, b):
    case = mc.full_case(b)
    assert case.cnt()[b] == 600 == 2 * case.n and sum(case.cnt()) == 600
    check_case(probe, case)


# ------------------------------------------------------------------------------ exceptional sums
@pytest.mark.parametrize("name", mc.EXCEPTIONAL_NAMES)
def test_exceptional_sums(probe, name):
    case = mc.exceptional_cases()[name]
    mc.check_expectations(case)   # the reference really is the identity / the doubling
    check_case(probe, case)


def test_trees_refuse_bad_arguments(probe):
    """more entries than a sort of n votes can produce, or a point id past the planes, never
    reach a kernel"""
    case = mc.exceptional_cases()["P,P"]
    sigma, tau = _u32(mc.point_words(case.sigma)), _u32(mc.point_words(case.tau))
    out = [np.zeros(k, dtype=np.uint32) for k in (mc.NB * 72, mc.NT * 72, 72)]

    def call(n, cnt, ent):
        return probe.mp_trees(n, _p(sigma), _p(tau), _p(_u32(cnt)), _p(_u32(ent)), *[_p(o) for o in out])

    one = [0] * mc.NB
    one[7] = 2
    assert call(case.n, one, [0, 2 * case.n - 1]) == 0
    assert call(case.n, one, [0, 2 * case.n]) == HIP_INVALID_VALUE      # id past the last point
    assert call(0, one, [0, 1]) == HIP_INVALID_VALUE
    big = [0] * mc.NB
    big[7] = 2 * case.n + 1                                             # > 2 n in one bucket
    assert call(case.n, big, [0] * big[7]) == HIP_INVALID_VALUE
    wide = [0] * mc.NB
    for b in range(5):
        wide[b] = 2 * case.n                                            # 10 n > 8 n in all
    assert call(case.n, wide, [0] * (10 * case.n)) == HIP_INVALID_VALUE


# ------------------------------------------------------------------------------ the sort half
@pytest.mark.parametrize("n", mc.SORT_SIZES)
def test_sort_half(probe, n):
    """k_msm_zero / count / scan / scatter: the histogram, the offsets, both prefix rows, and each
    bucket's slice of the sorted entries as a set (the scatter's order inside a bucket is
    arbitrary), under every code pattern and under a base whose index wraps 2^64"""
    for base in mc.SORT_BASES:
        for pattern, codes in mc.sort_codes(n).items():
            what = "n=%d base=%#x codes=%s" % (n, base, pattern)
            want_b, want_cnt, want_off, want_pf0, want_pf1 = mc.sort_reference(n, mc.SORT_SEED, base, codes)
            dcodes = np.array(codes, dtype=np.int32)
            cnt = np.zeros(mc.NB, dtype=np.uint32)
            off = np.zeros(mc.NB + 1, dtype=np.uint32)
            pf = np.zeros(2 * (mc.NB + 1), dtype=np.uint32)
            ent = np.zeros(8 * n, dtype=np.uint32)
            rc = probe.mp_sort(n, mc.SORT_SEED, base, _p(dcodes, i32p), _p(cnt), _p(off), _p(pf), _p(ent))
            assert rc == 0, "%s: mp_sort returned %d" % (what, rc)
            assert cnt.tolist() == want_cnt, what
            assert off.tolist() == want_off, what
            assert pf[:mc.NB + 1].tolist() == want_pf0, what
            assert pf[mc.NB + 1:].tolist() == want_pf1, what
            total = want_off[-1]
            got = ent.tolist()
            for b in range(mc.NB):
                assert sorted(got[want_off[b]:want_off[b + 1]]) == sorted(want_b.get(b, ())), (what, b)
            assert all(e == 0xFFFFFFFF for e in got[total:]), "%s: entries written past the total" % what
            if pattern == "all-failing":
                assert total == 0
            if pattern == "last-only":
                assert {e >> 1 for e in got[:total]} <= {n - 1}


# ------------------------------------------------------------------------------ the whole MSM
def run_msm(probe, n, seed, base, codes):
    sigma, tau = mc.msm_points(n)
    ws, wt = _u32(mc.point_words(sigma)), _u32(mc.point_words(tau))
    dcodes = np.array(codes, dtype=np.int32)
    S = np.zeros(72, dtype=np.uint32)
    rc = probe.mp_msm(n, _p(ws), _p(wt), seed, base, _p(dcodes, i32p), _p(S))
    assert rc == 0, "mp_msm(n=%d) returned %d" % (n, rc)
    return mc.from_words(S)


@pytest.mark.parametrize("n", mc.MSM_SIZES)
def test_whole_msm(probe, n):
    """enqueue_msm whole, non-unit base, some failing votes: S = sum (a_i sigma_i + b_i tau_i)"""
    codes = mc.msm_codes(n)
    want = mc.msm_reference(n, mc.MSM_SEED, mc.MSM_BASE, codes)
    assert want is not None
    assert same(run_msm(probe, n, mc.MSM_SEED, mc.MSM_BASE, codes), want)


def test_whole_msm_all_failing_and_unit_base(probe):
    """no valid vote: S = O; the unit base of a single vote checked alone: S = sigma, or O if the
    vote failed (k_sig_as_S)"""
    assert run_msm(probe, 2, mc.MSM_SEED, mc.MSM_BASE, [5, 3]) is None
    sigma, _ = mc.msm_points(1)
    assert same(run_msm(probe, 1, mc.MSM_SEED, mc.UNIT_BASE, [0]), sigma[0])
    assert run_msm(probe, 1, mc.MSM_SEED, mc.UNIT_BASE, [5]) is None


# ------------------------------------------------------------------------------ test index bases
def test_test_rlc_refuses_bases_that_can_reach_the_unit_base():
    """ovh_set_test_rlc: an index base of 2^63 or more is refused (the paths add vote offsets to it,
    and index 2^64 - 1 means "scalar 1"); 2^63 - 1 is accepted"""
    import consensus_overlord_amd as coa
    from consensus_overlord_amd.crypto import FLAG_TEST_RLC, Context
    cc = coa.ConsensusCrypto(bytes.fromhex("6d" * 32), ctx=Context(flags=FLAG_TEST_RLC))
    try:
        cc.ctx.set_test_rlc(1, (1 << 63) - 1)
        cc.ctx.set_test_rlc(1, 0)
        for base in (1 << 63, (1 << 63) + 1, mc.UNIT_BASE - 1, mc.UNIT_BASE):
            with pytest.raises(ValueError):
                cc.ctx.set_test_rlc(1, base)
    finally:
        cc.ctx.close()
