"""The expected values of tests/test_gpu_msm_buckets.py, checked without a GPU: for every crafted
case of tests/msm_cases.py the bucket-wise reference (bucket sums, bit-plane sums T_t, S = sum_t
2^t T_t) equals the direct sum over the entries of (d 256^w) times the point, and the cases reach
what they are built for -- by plain arithmetic on the crafted counts and on the reference sums,
not by running any kernel model."""
import pytest

import bls12_381 as bls
import msm_cases as mc


def same(x, y):
    return bls.pt_eq(mc.F, x, y)


def test_size_case_coverage():
    c = mc.size_case(0)
    cnt = c.cnt()
    assert sorted(x for x in cnt if x) == sorted(mc.SIZE_COUNTS)         # every listed count occurs
    assert max(mc.levels(x) for x in cnt if x) == 10 and 1 << 9 < max(cnt)  # levels 0..9 run
    assert max(mc.chunks(x) for x in cnt) >= 9
    assert {64, 65, 128, 129} <= set(cnt)
    # the ends of all four windows, i.e. of both prefix rows, are taken; the rest is mostly empty
    assert all(cnt[b] for b in (0, 1, 254, 255, 509, 510, 764, 765, 1018, 1019))
    assert sum(1 for x in cnt if x == 0) == mc.NB - len(mc.SIZE_COUNTS)
    assert all(len(set(ids)) == len(ids) for ids in c.buckets.values())  # distinct points inside a bucket
    # the product's bounds on what a sort of n votes can produce
    assert sum(cnt) == 2059 <= 8 * c.n and max(cnt) <= 2 * c.n
    d = mc.size_case(1)
    assert d.cnt() == cnt and all(sorted(d.buckets[b]) == sorted(c.buckets[b]) for b in c.buckets)
    assert all(d.buckets[b] != c.buckets[b] for b in c.buckets if cnt[b] > 1)


def test_size_case_reference_is_the_direct_sum():
    c = mc.size_case(0)
    S = c.result()
    assert S is not None and bls.on_curve(mc.F, S)
    assert same(S, c.direct())


def test_size_case_orders_share_the_sums():
    """the reordered case's bucket sums, summed in its own order, are the first case's"""
    c, d = mc.size_case(0), mc.size_case(1)
    for b in (1, 255, 764, 100, 1018):
        assert same(mc.psum(d.point(i) for i in d.buckets[b]), c.bucket_sums()[b])


@pytest.mark.parametrize("b", mc.FULL_BUCKETS)
def test_full_bucket_reference_is_the_direct_sum(b):
    c = mc.full_case(b)
    assert c.cnt()[b] == 2 * c.n == 600 and sum(c.cnt()) == 600
    assert mc.levels(600) == 10 and mc.chunks(600) == 10
    S = c.result()
    assert S is not None and same(S, c.direct())


def test_exceptional_names():
    assert tuple(mc.exceptional_cases()) == mc.EXCEPTIONAL_NAMES


@pytest.mark.parametrize("name", mc.EXCEPTIONAL_NAMES)
def test_exceptional_reference(name):
    """the reference is the direct sum, and the sums are the identity or the doubling the case
    says they are"""
    c = mc.exceptional_cases()[name]
    assert same(c.result(), c.direct())
    mc.check_expectations(c)


def test_exceptional_cases_reach_their_levels():
    ex = mc.exceptional_cases()
    cnt = lambda name: max(ex[name].cnt())  # noqa: E731
    assert cnt("64xP") == 64 and mc.levels(64) == 6 and mc.chunks(64) == 1
    assert cnt("64-cancel,Q") == 65 and mc.levels(65) == 7          # level 6 in k_msm_upper: O + Q
    assert cnt("128-two-chunks-O") == 128 and mc.chunks(128) == 2 and mc.levels(128) == 7
    c = ex["64-cancel,Q"]
    ids = c.buckets[mc.bucket(1, 77)]
    assert all(same(c.point(ids[k]), mc.neg(c.point(ids[k + 1]))) for k in range(0, 64, 2))
    c = ex["128-two-chunks-O"]
    ids = c.buckets[mc.bucket(1, 77)]
    for lo in (0, 64):
        assert mc.psum(c.point(i) for i in ids[lo:lo + 64]) is None
    assert mc.psum(c.point(i) for i in ids[:32]) is not None        # chunk 0 cancels at level 5 only
    assert all(mc.psum(c.point(i) for i in ids[k:k + 2]) is not None for k in range(64, 128, 2))
    assert all(mc.psum(c.point(i) for i in ids[k:k + 4]) is None for k in range(64, 128, 4))
    assert sum(ex["empty"].cnt()) == 0


def test_sort_reference_digits():
    """the n = 1000 sort case meets a zero digit (a point left out of a window) and digit 255
    (the last bucket of a window) under both bases, and the wrapping base is not the unit base"""
    for base in mc.SORT_BASES:
        d = mc.digits(1000, mc.SORT_SEED, base)
        assert 0 in d and 255 in d
        assert base != mc.UNIT_BASE
    assert mc.SORT_BASES[1] + 1000 > mc.M64 + 1
    # SplitMix64's published test vector (seed 1234567: the first output), i = 0 adds the first gamma
    assert mc.splitmix(1234567, 0) == 6457827717110365317
    buckets, cnt, off, pf0, pf1 = mc.sort_reference(65, mc.SORT_SEED, mc.SORT_BASES[0], mc.sort_codes(65)["alternating"])
    assert sum(cnt) == off[-1] == sum(len(v) for v in buckets.values())
    assert all(i >> 1 in range(0, 65, 2) for v in buckets.values() for i in v)   # the odd votes failed
    assert pf0[-1] == sum((c + 1) // 2 for c in cnt) and pf1[-1] == sum(1 for c in cnt if c)


@pytest.mark.parametrize("n", mc.MSM_SIZES)
def test_msm_reference_is_the_bucket_reference(n):
    """sum (a_i sigma_i + b_i tau_i) over the valid votes equals the bucket-wise reference of the
    sorted digits"""
    codes = mc.msm_codes(n)
    assert n == 1 or any(codes)
    assert 0 in codes
    buckets = mc.sort_reference(n, mc.MSM_SEED, mc.MSM_BASE, codes)[0]
    sigma, tau = mc.msm_points(n)
    c = mc.Case("msm-%d" % n, sigma, tau, buckets)
    assert same(c.result(), mc.msm_reference(n, mc.MSM_SEED, mc.MSM_BASE, codes))
