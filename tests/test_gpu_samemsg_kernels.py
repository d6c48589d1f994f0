"""The kernels and host code that build the left-hand factor of the same-message equation
(DESIGN.md section 3.3),

    prod_g e(sum_{i in g} r_i pk_i, H_g) * e(-G1, sum_i r_i sigma_i) == 1,

on crafted rounds against exact expectations: samemsg_plan, k_vm_vsame<TABLE, W> in its four
instantiations, k_samemsg_fix and the k_vm_g1pairs levels, k_h2f + k_vm_h2g, k_vm_vote1h_b<TABLE> +
k_vm_votefe, and the whole path through ovh_verify_batch with the batch's verdict, head hash, key
sums and per-hash Miller values read back (csrc/ovhip.hip verify_samemsg_locked).

tests/test_gpu_samemsg.py compares codes with the oracle. Codes cannot show a combined check that
fails for a wrong reason: the bisection recomputes every vote from its bytes and the codes still
come out right, several times slower. Here the verdict of every valid crafted round must be 1.

The test-only probe (tests/device/samemsg_probe.hip, built by `make -C consensus_overlord_amd` as
tests/device/_build/libsmprobe.so with -DVSAME8_MIN=16u) includes the product translation unit whole
and launches the product's kernels with the product's grid and LDS sizes on arrays the test
supplies. The reference is tests/samemsg_cases.py (plain integers, the oracle's point arithmetic,
tests/pairing_ref.py for the final power). Every comparison is exact: affine points limb for limb,
projective points as points (a device identity is Z = 0), codes and plan words word for word with
their guard words, untouched outputs still 0xFF."""
import ctypes
import os

import numpy as np
import pytest

import samemsg_cases as sc
from vm_helpers import ROOT

pytestmark = pytest.mark.gpu

PROBE = os.path.join(ROOT, "tests", "device", "_build", "libsmprobe.so")
u8p = ctypes.c_char_p
u32p = ctypes.POINTER(ctypes.c_uint32)
i32p = ctypes.POINTER(ctypes.c_int32)
u32, u64, cint = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
HIP_INVALID_VALUE = 1
GUARD = sc.GUARD


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(PROBE):
        pytest.fail("%s is missing: run build() (make -C consensus_overlord_amd) first" % PROBE)
    lib = ctypes.CDLL(PROBE)
    lib.sp_plan.argtypes = [u32, u8p, u32p, u32p, u8p, u32p, u32p, u32p, u32p]
    lib.sp_vsame.argtypes = [cint, cint, u32, u32, u8p, u8p, u32, u32p, u32p, i32p, u64, u64, i32p, u32p]
    lib.sp_keysums.argtypes = [u32, u32p, u32, u32p, i32p, u32p, u32, u32p, u32, u32p]
    lib.sp_h2g.argtypes = [u32, u8p, u32p, u32p, u32p]
    lib.sp_bisect.argtypes = [cint, u32, u32, u8p, u8p, u32, u32p, u32p, i32p, u32p, u32, u32p, u32p, i32p, cint, u32p]
    lib.sp_batch.argtypes = [u32, u8p, u8p, u8p, u32, u8p, u64, u64, i32p, i32p, u32p, u32p, u32p, u32p]
    for f in (lib.sp_plan, lib.sp_vsame, lib.sp_keysums, lib.sp_h2g, lib.sp_bisect, lib.sp_batch):
        f.restype = cint
    for f in (lib.sp_guard, lib.sp_vsame8_min, lib.sp_votes_max):
        f.restype = u32
    lib.sp_close.restype = None
    assert lib.sp_guard() == GUARD and lib.sp_vsame8_min() == sc.VSAME8_MIN and lib.sp_votes_max() >= 201
    yield lib
    lib.sp_close()


def _u32(vals):
    return np.ascontiguousarray(np.array(vals, dtype=np.uint32).reshape(-1))


def _i32(vals):
    return np.ascontiguousarray(np.array([v & 0xFFFFFFFF for v in vals], dtype=np.uint32).astype(np.int32).reshape(-1))


def _p(arr, t=u32p):
    return None if arr is None else arr.ctypes.data_as(t)


# ------------------------------------------------------------------------------ samemsg_plan
def run_plan(probe, hashes, perm):
    n = len(hashes)
    gid, head, pairs, lo, cnt = (np.full(k, 0xEEEEEEEE, dtype=np.uint32) for k in (n, n, 2 * n, 34, 3))
    ghash = ctypes.create_string_buffer(32 * n)
    rc = probe.sp_plan(n, b"".join(hashes), _p(_u32(perm)) if perm else None, _p(gid), ghash, _p(head), _p(pairs), _p(lo), _p(cnt))
    assert rc == 0, "sp_plan returned %d" % rc
    G, npairs, nlo = (int(x) for x in cnt)
    return (G, gid.tolist(), [ghash.raw[32 * g:32 * g + 32] for g in range(G)], head[:G].tolist(),
            [tuple(pairs[2 * k:2 * k + 2].tolist()) for k in range(npairs)], lo[:nlo].tolist())


def test_plan_equals_the_model_word_for_word(probe):
    seen = 0
    for c in sc.keysum_cases():
        hashes = [bytes([g]) * 32 for g in c.gid]
        pl = sc.plan(hashes)
        assert run_plan(probe, hashes, None) == (pl.G, pl.gid, pl.ghash, pl.head, pl.pairs, pl.level_off), c.name
        seen += 1
    for rd in sc.batch_rounds():          # with the staged order of a mixed table / bytes round
        ex = sc.batch_expect(rd)
        hashes = [v.hash for v in rd.votes]
        perm = ex.perm if ex.perm != list(range(len(hashes))) else None
        pl = ex.plan
        assert run_plan(probe, hashes, perm) == (pl.G, pl.gid, pl.ghash, pl.head, pl.pairs, pl.level_off), rd.name
        seen += perm is not None
    assert seen >= 10
    one = [b"\x07" * 32]
    assert run_plan(probe, one, None) == (1, [0], one, [0], [], [0])


# ------------------------------------------------------------------------------ k_vm_vsame
def run_vsame(probe, run):
    sigs, pks, tw, tf, tidx, codes_in = sc.vsame_inputs(run)
    n = len(run.votes)
    cap = run.lo + n + GUARD
    codes = _i32(codes_in)
    out = np.zeros(cap * sc.VS_W, dtype=np.uint32)
    rc = probe.sp_vsame(run.table, run.w8, n, run.lo, sigs, pks, len(tf), _p(_u32(tw)), _p(_u32(tf)), _p(_i32(tidx), i32p),
                        run.seed, run.base, _p(codes, i32p), _p(out))
    assert rc == 0, "sp_vsame returned %d on %s" % (rc, run.name)
    sc.check_vsame(run, codes_in, codes.tolist(), out.tolist())


@pytest.mark.parametrize("table", [0, 1])
@pytest.mark.parametrize("w8", [0, 1])
def test_vsame_every_instantiation(probe, w8, table):
    """k_vm_vsame<table, w8 ? 8 : 16>: slices and tails, table indices permuted and repeated,
    base + i across 2^32 and 2^63, the RLC edge values, one vote per point class and the flagged
    table entries over poisoned planes; codes, sigma and tau exact, r pk as a point, the entries
    and code words outside the launch untouched"""
    runs = [r for r in sc.vsame_runs() if (r.w8, r.table) == (w8, table)]
    assert {r.cls for r in runs} == {"slices", "rlc", "classes"} and len(runs) == 3 + len(sc.RLC_EDGES) + 1
    for r in runs:
        run_vsame(probe, r)


# ------------------------------------------------------------------------------ the key sums
@pytest.mark.parametrize("k", range(6))
def test_keysums(probe, k):
    c = sc.keysum_cases()[k]
    words_in = sc.keysum_words(c)
    codes = _i32(list(c.codes) + [sc.CODE_GUARD] * GUARD)
    P = _u32(words_in)
    pairs = _u32([x for ab in c.plan.pairs for x in ab] or [0])
    rc = probe.sp_keysums(c.n, _p(_u32(c.gid)), c.G, _p(_u32(c.ghinf)), _p(codes, i32p), _p(P), len(c.plan.pairs), _p(pairs),
                          len(c.plan.level_off), _p(_u32(c.plan.level_off)))
    assert rc == 0, "sp_keysums returned %d on %s" % (rc, c.name)
    sc.check_keysums(c, words_in, codes.tolist(), P.tolist())


def test_keysum_cases_are_all_run():
    assert len(sc.keysum_cases()) == 6


# ------------------------------------------------------------------------------ hash_to_G2 per hash
def test_h2g_equals_the_oracle(probe):
    for case in sc.h2g_cases():
        name, hashes, us, want = case
        G = len(want)
        H = np.zeros((G + GUARD) * sc.G2_W, dtype=np.uint32)
        inf = np.zeros(G + GUARD, dtype=np.uint32)
        uw = None if us is None else _u32([w for u0, u1 in us for c in u0 + u1 for w in sc.limbs(c)])
        rc = probe.sp_h2g(G, b"".join(hashes) if hashes else None, _p(uw), _p(H), _p(inf))
        assert rc == 0, "sp_h2g returned %d on %s" % (rc, name)
        sc.check_h2g(case, H.tolist(), inf.tolist())


# ------------------------------------------------------------------------------ the bisection
@pytest.mark.parametrize("table", [0, 1])
def test_bisect_behind_the_verdict(probe, table):
    """nothing written under verdict 1; under verdict 0 BLST_VERIFY_FAIL exactly on the wrong votes
    (another signer's signature, the other hash's gid, a hash with H = O), earlier codes kept over
    poisoned bytes"""
    run = sc.bisect_runs()[table]
    assert run.table == table
    sigs, pks, tw, tf, tidx, gid, gh, ghinf, codes_in = sc.bisect_inputs(run)
    n = len(run.votes)
    cap = run.lo + n + GUARD
    for verdict in (1, 0):
        codes = _i32(codes_in)
        f = np.zeros(cap * sc.F_W, dtype=np.uint32)
        rc = probe.sp_bisect(table, n, run.lo, sigs, pks, len(tf), _p(_u32(tw)), _p(_u32(tf)), _p(_i32(tidx), i32p), _p(_u32(gid)),
                             len(run.hs), _p(_u32(gh)), _p(_u32(ghinf)), _p(codes, i32p), verdict, _p(f))
        assert rc == 0, "sp_bisect returned %d" % rc
        sc.check_bisect(run, verdict, codes.tolist(), f.tolist())


# ------------------------------------------------------------------------------ whole rounds
@pytest.mark.parametrize("k", range(10))
def test_batch_verdict_and_intermediate_values(probe, k):
    """ovh_verify_batch on a crafted round: verdict 1 on every valid round (0 with invalid votes),
    exact codes, the head hash, the key sums at the heads, FE_ref(f_g) = e(apk_g, H_g)^3"""
    rd = sc.batch_rounds()[k]
    ex = sc.batch_expect(rd)
    n = len(rd.votes)
    codes = _i32([-1] * n)
    info = _i32([-1] * 4)
    perm, ghinf = _u32([0] * n), _u32([9] * n)
    Pw, fw = np.zeros(n * sc.G1_W, dtype=np.uint32), np.zeros(n * sc.F_W, dtype=np.uint32)
    rc = probe.sp_batch(n, b"".join(v.sig for v in rd.votes), b"".join(v.hash for v in rd.votes), b"".join(v.pk for v in rd.votes),
                        len(rd.validators), b"".join(rd.validators) or None, rd.seed, rd.base, _p(codes, i32p), _p(info, i32p),
                        _p(perm), _p(ghinf), _p(Pw), _p(fw))
    assert rc == 0, "sp_batch returned %d on %s" % (rc, rd.name)
    print("%s: verdict %d hsel %d G %d T %d codes %s" % ((rd.name,) + tuple(info.tolist()) + (codes.tolist(),)))
    sc.check_batch(rd, ex, codes.tolist(), info.tolist(), perm.tolist(), ghinf.tolist(), Pw.tolist(), fw.tolist())


def test_batch_rounds_are_all_run():
    rounds = sc.batch_rounds()
    assert len(rounds) == 10
    ns = [len(r.votes) for r in rounds]
    assert min(ns) < sc.VSAME8_MIN <= max(ns)             # both slice widths
    ts = {(sc.batch_expect(r).t, len(r.votes)) for r in rounds}
    assert {(0, 5), (3, 9), (8, 9), (9, 9)} <= ts         # every table / bytes split


# ------------------------------------------------------------------------------ refusals
def test_probe_refuses_what_would_leave_its_buffers(probe):
    """no launch (hipErrorInvalidValue) for a table index >= the table's capacity, gid >= G, a pair
    or perm entry >= n, n above the maximum"""
    run = next(r for r in sc.vsame_runs() if r.table and r.cls == "slices" and len(r.votes) == 4)
    sigs, pks, tw, tf, tidx, codes_in = sc.vsame_inputs(run)
    n = len(run.votes)
    codes, out = _i32(codes_in), np.zeros((run.lo + n + GUARD) * sc.VS_W, dtype=np.uint32)
    args = lambda idx, cnt=n: (1, 0, cnt, run.lo, sigs, None, len(tf), _p(_u32(tw)), _p(_u32(tf)), _p(_i32(idx), i32p),  # noqa: E731
                               run.seed, run.base, _p(codes, i32p), _p(out))
    assert probe.sp_vsame(*args(tidx[:-1] + [len(tf)])) == HIP_INVALID_VALUE
    assert probe.sp_vsame(*args(tidx[:-1] + [-1])) == HIP_INVALID_VALUE
    assert probe.sp_vsame(*args(tidx, 257)) == HIP_INVALID_VALUE
    assert probe.sp_vsame(0, 0, n, 0, sigs, None, 0, None, None, None, 1, 2, _p(codes, i32p), _p(out)) == HIP_INVALID_VALUE
    assert probe.sp_vsame(0, 0, n, 0, sigs, sigs, 0, None, None, None, 1, (1 << 64) - 1, _p(codes, i32p), _p(out)) == HIP_INVALID_VALUE
    assert codes.tolist() == _i32(codes_in).tolist() and not out.any()
    c = sc.keysum_cases()[2]
    P, cd = _u32(sc.keysum_words(c)), _i32(list(c.codes) + [0] * GUARD)
    flat = [x for ab in c.plan.pairs for x in ab]
    ks = lambda gid, pairs, lo: probe.sp_keysums(c.n, _p(_u32(gid)), c.G, _p(_u32(c.ghinf)), _p(cd, i32p), _p(P), len(pairs) // 2,  # noqa: E731
                                                 _p(_u32(pairs)), len(lo), _p(_u32(lo)))
    assert ks(list(c.gid[:-1]) + [c.G], flat, c.plan.level_off) == HIP_INVALID_VALUE
    assert ks(c.gid, flat[:-1] + [c.n], c.plan.level_off) == HIP_INVALID_VALUE
    assert ks(c.gid, flat, c.plan.level_off[:-1] + [len(flat) // 2 + 1]) == HIP_INVALID_VALUE
    assert ks(c.gid, flat, [0, 3, 2, len(flat) // 2]) == HIP_INVALID_VALUE
    assert P.tolist() == sc.keysum_words(c)
    hashes = b"\x01" * 64
    z = _u32([0] * 8)
    assert probe.sp_plan(2, hashes, _p(_u32([0, 2])), _p(z), ctypes.create_string_buffer(64), _p(z), _p(z), _p(_u32([0] * 34)),
                         _p(z)) == HIP_INVALID_VALUE
    assert probe.sp_plan(257, hashes, None, _p(z), ctypes.create_string_buffer(64), _p(z), _p(z), _p(_u32([0] * 34)),
                         _p(z)) == HIP_INVALID_VALUE
    run = sc.bisect_runs()[0]
    sigs, pks, tw, tf, tidx, gid, gh, ghinf, codes_in = sc.bisect_inputs(run)
    n = len(run.votes)
    f = np.zeros((run.lo + n + GUARD) * sc.F_W, dtype=np.uint32)
    bis = lambda gid_, verdict: probe.sp_bisect(0, n, run.lo, sigs, pks, 0, None, None, None, _p(_u32(gid_)), len(run.hs), _p(_u32(gh)),  # noqa: E731
                                                _p(_u32(ghinf)), _p(_i32(codes_in), i32p), verdict, _p(f))
    assert bis(gid[:-1] + [len(run.hs)], 0) == HIP_INVALID_VALUE
    assert bis(gid, -1) == HIP_INVALID_VALUE and bis(gid, 2) == HIP_INVALID_VALUE       # the kernels take no null verdict
    assert not f.any()
