"""tests/samemsg_cases.py checked against itself and the oracle, on the CPU: the laws of the plan
model, the class counts, the same-message equation on every crafted round (it holds on the valid
ones and fails when one r_i, one key or one group assignment is changed), and the comparison
helpers of tests/test_gpu_samemsg_kernels.py on what a right device would return and on the same
with one limb, one code or one verdict changed."""
import random

import pytest

import bls12_381 as bls
import msm_cases
import samemsg_cases as sc
from vm_helpers import ROOT  # noqa: F401  (puts tools/fpvm on the path)

import alg  # noqa: E402

R = bls.R


# ------------------------------------------------------------------------------ scalars
def test_scalars_match_the_generator_and_the_inverse_mix():
    rng = random.Random(5)
    for z in [e[1] for e in sc.RLC_EDGES] + [rng.getrandbits(64) for _ in range(50)]:
        assert sc.rlc_scalar(z) == alg.rlc_scalar(z)
        for base, i in ((0, 0), (0x77, 2), ((1 << 63) - 3, 5), ((1 << 64) - 2, 7)):
            assert msm_cases.vote_scalar(sc.seed_for(z, base, i), base, i) == (z or 1)
    assert sc.LAMBDA == alg.LAMBDA
    # phi(pk) = [LAMBDA] pk and tau = [LAMBDA] sigma: the halves of an RLC value act alike on both sides
    sg = sc.sig_of(0, 0)
    assert sc.tau_of(sg) == bls.pt_mul(sc.F2, sg, sc.LAMBDA)


# ------------------------------------------------------------------------------ the plan model
def _plans():
    for c in sc.keysum_cases():
        yield c.name, c.plan, c.n
    for rd in sc.batch_rounds():
        ex = sc.batch_expect(rd)
        yield rd.name, ex.plan, len(rd.votes)
    rng = random.Random(11)
    for n in (1, 2, 3, 16, 17, 100):
        hashes = [bytes([rng.randrange(1 + n // 3)]) * 32 for _ in range(n)]
        perm = list(range(n))
        rng.shuffle(perm)
        yield "random n=%d" % n, sc.plan(hashes, perm), n


def test_plan_laws():
    """every member of a group is absorbed exactly once, the pairs of a level are disjoint and stay
    inside one group, the root is head, the groups are in first-seen order"""
    count = 0
    for name, pl, n in _plans():
        assert sorted(j for m in pl.members for j in m) == list(range(n)), name
        assert pl.head == [m[0] for m in pl.members] and pl.head == sorted(pl.head), name
        assert [pl.gid[h] for h in pl.head] == list(range(pl.G)), name
        assert pl.level_off[0] == 0 and pl.level_off[-1] == len(pl.pairs) and pl.level_off == sorted(pl.level_off), name
        absorbed = []
        for l in range(len(pl.level_off) - 1):
            level = pl.pairs[pl.level_off[l]:pl.level_off[l + 1]]
            assert level, name
            touched = [x for ab in level for x in ab]
            assert len(set(touched)) == len(touched), "%s: level %d is not disjoint" % (name, l)
            assert all(pl.gid[a] == pl.gid[b] and a < b for a, b in level), name
            assert not set(touched) & set(absorbed), "%s: an absorbed entry is used again" % name
            absorbed += [b for _, b in level]
        assert sorted(absorbed) == sorted(j for m in pl.members for j in m[1:]), name + ": absorbed exactly once"
        assert len(pl.level_off) - 1 == max(len(m) - 1 for m in pl.members).bit_length(), name
        count += 1
    assert count >= 20


def test_plan_with_perm_is_the_plan_of_the_staged_hashes():
    rng = random.Random(3)
    hashes = [bytes([rng.randrange(4)]) * 32 for _ in range(23)]
    perm = list(range(23))
    rng.shuffle(perm)
    assert sc.plan(hashes, perm) == sc.plan([hashes[i] for i in perm])
    assert sc.plan(hashes, []) == sc.plan(hashes, None) == sc.plan(hashes, list(range(23)))


def test_integer_evaluation_equals_the_plain_sum():
    """on scalars for every plan, and on points of the curve for the G = 5 case"""
    for name, pl, n in _plans():
        vals = [random.Random(name).randrange(R) + j for j in range(n)]
        after, written = sc.evaluate(pl, vals, lambda a, b: (a + b) % R)
        for g, m in enumerate(pl.members):
            assert after[pl.head[g]] == sum(vals[j] for j in m) % R, name
        assert written == {a for a, _ in pl.pairs}
    c = sc.keysum_cases()[3]
    codes, after, _ = sc.keysum_expect(c)
    pts = [None if cd else sc.g1_mul(s) for cd, s in zip(codes, c.scal)]
    summed, _ = sc.evaluate(c.plan, pts, sc.g1_add)
    for g, m in enumerate(c.plan.members):
        plain = None
        for j in m:
            plain = sc.g1_add(plain, pts[j])
        assert summed[c.plan.head[g]] == plain == sc.g1_mul(after[c.plan.head[g]]), (c.name, g)
    assert summed[c.plan.head[1]] is None and summed[c.plan.head[3]] is None     # every vote failed; H = O


def test_table_split_model():
    vals = [b"k%046d" % k for k in (5, 3, 5, 9)]
    pks = [b"k%046d" % k for k in (1, 5, 2, 9, 3)]
    assert sc.table_split(pks, vals) == ([1, 3, 4, 0, 2], [0, 3, 1])
    assert sc.table_split(pks, []) == (None, [])
    assert sc.table_split(pks[1:2] + pks[3:], vals) == (None, [0, 3, 1])


# ------------------------------------------------------------------------------ the classes
def test_class_counts():
    import point_cases as pc
    counts = sc.class_counts()
    assert counts == {"vsame slices": 12, "vsame rlc": 28, "vsame classes": 4, "vsame votes": 172, "keysum cases": 6,
                      "keysum entries": 347, "h2g cases": 4, "bisect runs": 2, "batch rounds": 10, "batch rounds valid": 7}
    runs = sc.vsame_runs()
    assert {(r.w8, r.table, len(r.votes)) for r in runs if r.cls == "slices"} == \
        {(0, t, n) for t in (0, 1) for n in (1, 4, 5)} | {(1, t, n) for t in (0, 1) for n in (8, 9, 17)}
    for r in runs:
        assert r.base != msm_cases.UNIT_BASE
    crossed = {b for r in runs if r.cls == "slices" for b in (1 << 32, 1 << 63) if r.base + r.lo < b <= r.base + r.lo + len(r.votes) - 1}
    assert crossed == {1 << 32, 1 << 63}
    # every class of both groups (and both infinities) reaches the key-bytes programs, every signature
    # class and every table flag the table programs; every code of the precedence occurs
    for r in (r for r in runs if r.cls == "classes"):
        names = [v.name for v in r.votes]
        if r.table:
            assert sorted(r.entries[e][1] for e in r.tidx[-3:]) == [sc.PKF_PARSE, sc.PKF_INF, sc.PKF_GRP]
            assert len(names) == len(pc.G2_CLASSES) + 1 + 3
        else:
            assert len(names) == len(pc.G1_CLASSES) + len(pc.G2_CLASSES) + 2
        codes = {e[0] for e in sc.vsame_expect(r)}
        assert codes >= {0, sc.BAD_ENCODING, sc.NOT_ON_CURVE, sc.NOT_IN_GROUP, sc.VERIFY_FAIL, sc.PK_IS_INFINITY, sc.ERR_PUBKEY}
    for r in (r for r in runs if r.table and r.cls == "slices" and len(r.votes) > 6):
        assert len(set(r.tidx)) < len(r.tidx) and list(r.tidx) != sorted(r.tidx)      # repeated and permuted
    sizes = sorted(len(m) for c in sc.keysum_cases() for m in c.plan.members)
    assert set(sc.SIZES) <= set(sizes) and {c.G for c in sc.keysum_cases()} >= {1, 2, 5, 11, 70}
    for c in sc.keysum_cases():               # interleaved, not contiguous
        if c.G > 1:
            assert any(c.gid[j] != c.gid[j + 1] for j in range(c.n - 1)) and c.plan.members[0][1:2] != [1]


def test_format_code_precedence():
    g1, g2 = __import__("point_cases").cases()
    off1 = next(c for c in g1 if c.cls == "off_curve")
    grp1 = next(c for c in g1 if c.cls == "small_order")
    off2 = next(c for c in g2 if c.cls == "off_curve")
    assert sc.format_code(sc.with_key(off1).kcode, sc.with_sig(off2).scode) == sc.ERR_PUBKEY
    assert sc.format_code(sc.with_key(grp1).kcode, sc.with_sig(off2).scode) == sc.NOT_ON_CURVE
    assert sc.format_code(sc.with_key(None).kcode, sc.with_sig(None).scode) == sc.PK_IS_INFINITY
    assert sc.format_code(sc.with_key(grp1).kcode, sc.with_sig(None).scode) == sc.NOT_IN_GROUP
    assert sc.format_code(0, sc.with_sig(None).scode) == sc.VERIFY_FAIL
    v = sc.good(3, 1)
    assert bls.core_verify(v.kpt, v.spt, v.hash) == 0 and bls.core_verify(v.kpt, sc.wrong(3, 1).spt, v.hash) == sc.VERIFY_FAIL


# ------------------------------------------------------------------------------ the equation
@pytest.mark.parametrize("k", range(10))
def test_equation_on_every_round(k):
    rd = sc.batch_rounds()[k]
    ex = sc.batch_expect(rd)
    assert sc.equation_holds(rd, ex) == bool(ex.verdict), rd.name
    assert ex.verdict == int(all(v.valid for v, c in zip(ex.staged, ex.pre) if c == 0))
    # the codes are the oracle's, vote by vote (the first twelve, and every vote that is not valid)
    for k, (v, code) in enumerate(zip(rd.votes, ex.codes)):
        if k >= 12 and v.valid:
            assert code == 0
        elif v.kpt is not None and v.spt is not None:
            assert bls.core_verify(v.kpt, v.spt, v.hash) == code, (rd.name, v.name)
        else:
            assert code == sc.format_code(v.kcode, v.scode) != 0


def test_equation_fails_on_one_changed_scalar_key_or_group():
    rd = next(r for r in sc.batch_rounds() if r.name.startswith("valid n=9 G=2 T=3"))
    ex = sc.batch_expect(rd)
    assert sc.equation_holds(rd, ex)
    g = ex.plan.gid[4]
    # one r_i off by one: the key sum gains a pk_i
    apk = list(ex.apk)
    apk[g] = sc.g1_add(apk[g], ex.staged[4].kpt)
    assert not sc.equation_holds(rd, ex, apk=apk)
    # one key replaced by another signer's
    r4 = sc.rlc_scalar(msm_cases.vote_scalar(rd.seed, rd.base, 4))
    apk = list(ex.apk)
    other = sc.signers()[11][1]
    apk[g] = sc.g1_add(sc.g1_add(apk[g], bls.pt_neg(sc.F1, bls.pt_mul(sc.F1, ex.staged[4].kpt, r4))), bls.pt_mul(sc.F1, other, r4))
    assert not sc.equation_holds(rd, ex, apk=apk)
    # one vote summed into the other group
    apk = list(ex.apk)
    t = bls.pt_mul(sc.F1, ex.staged[4].kpt, r4)
    apk[g] = sc.g1_add(apk[g], bls.pt_neg(sc.F1, t))
    apk[1 - g] = sc.g1_add(apk[1 - g], t)
    assert not sc.equation_holds(rd, ex, apk=apk)
    # the two hashes swapped
    assert not sc.equation_holds(rd, ex, hashes=ex.plan.ghash[::-1])


# ------------------------------------------------------------------------------ the comparison helpers
def _caught(fn, *args):
    with pytest.raises(AssertionError):
        fn(*args)


def test_helpers_accept_a_right_result_and_notice_one_changed_word():
    rng = random.Random(0x5A3E)
    for run in (sc.vsame_runs()[3], sc.vsame_runs()[-1]):
        _, _, _, _, _, codes_in = sc.vsame_inputs(run)
        codes, out = sc.synth_vsame(run)
        sc.check_vsame(run, codes_in, codes, out)
        exp = sc.vsame_expect(run)
        j = run.lo + max(k for k, e in enumerate(exp) if e[1] is not None and e[3] is not None)
        for at in (j * sc.VS_W + 5, j * sc.VS_W + 60, j * sc.VS_W + 100, 0, len(out) - 1):      # sigma, tau, r pk, the guards
            bad = list(out)
            bad[at] ^= 1
            _caught(sc.check_vsame, run, codes_in, codes, bad)
        for at in (j, 0 if run.lo else len(codes) - 1, len(codes) - 1):
            bad = list(codes)
            bad[at] ^= 2
            _caught(sc.check_vsame, run, codes_in, bad, out)
    for c in sc.keysum_cases()[3:6:2]:
        words_in = sc.keysum_words(c)
        codes, words = sc.synth_keysums(c)
        sc.check_keysums(c, words_in, codes, words)
        want, _, written = sc.keysum_expect(c)
        root = c.plan.head[next(g for g, m in enumerate(c.plan.members) if len(m) > 1)]
        leaf = next(i for i in range(c.n) if i not in written and not want[i])
        failed = next((i for i in range(c.n) if i not in written and want[i]), None)
        for i in [root, leaf, c.n] + ([failed] if failed is not None else []):
            bad = list(words)
            bad[i * sc.G1_W + rng.randrange(sc.G1_W)] ^= 1 << 3
            _caught(sc.check_keysums, c, words_in, codes, bad)
        bad = list(codes)
        bad[leaf] = 5
        _caught(sc.check_keysums, c, words_in, bad, words)
    case = sc.h2g_cases()[-1]
    H, inf = sc.synth_h2g(case)
    sc.check_h2g(case, H, inf)
    _caught(sc.check_h2g, case, H[:7] + [H[7] ^ 1] + H[8:], inf)
    _caught(sc.check_h2g, case, H, [inf[0], 0] + inf[2:])
    _caught(sc.check_h2g, case, H, inf[:-1] + [0])


def test_batch_helper_notices_a_changed_verdict_code_head_sum_or_miller_value():
    rd = next(r for r in sc.batch_rounds() if r.name.startswith("first hash all malformed"))
    ex = sc.batch_expect(rd)
    assert ex.hsel == 1 and ex.apk[0] is None and ex.verdict == 1
    codes, info, perm, ghinf, Pw, fw = sc.synth_batch(rd, ex)
    sc.check_batch(rd, ex, codes, info, perm, ghinf, Pw, fw)
    _caught(sc.check_batch, rd, ex, codes, [0] + info[1:], perm, ghinf, Pw, fw)                  # the verdict
    _caught(sc.check_batch, rd, ex, codes, [info[0], 0] + info[2:], perm, ghinf, Pw, fw)        # hsel
    _caught(sc.check_batch, rd, ex, codes[:4] + [5] + codes[5:], info, perm, ghinf, Pw, fw)     # one code
    _caught(sc.check_batch, rd, ex, codes, info, perm, [0, 1, 0], Pw, fw)                       # ghinf
    h = ex.plan.head[1] * sc.G1_W
    _caught(sc.check_batch, rd, ex, codes, info, perm, ghinf, Pw[:h] + [Pw[h] ^ 1] + Pw[h + 1:], fw)      # a key sum
    at = 2 * sc.F_W + 17
    _caught(sc.check_batch, rd, ex, codes, info, perm, ghinf, Pw, fw[:at] + [fw[at] ^ 1] + fw[at + 1:])   # a Miller value
    at = 1 * sc.F_W                                                                             # hash 0's f (= 1) at the head's index
    _caught(sc.check_batch, rd, ex, codes, info, perm, ghinf, Pw, fw[:at] + [fw[at] ^ 1] + fw[at + 1:])
