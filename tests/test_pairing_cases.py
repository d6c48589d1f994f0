"""The crafted pairing cases (tests/pairing_cases.py) and their plain-integer reference
(tests/pairing_ref.py) on the CPU: the reference's own consistency (round trips, inverse,
Frobenius of order 12, bilinearity), the class counts and class properties of the cases, the
oracle's tower, Miller loops and x-chain (oracle/py/bls12_381.py) against the reference on every
case, and the comparison helper of the interpreter tests on a perturbed result."""
import collections
import random

import bls12_381 as bls
import pairing_cases as pcs
import pairing_ref as ref
import pairing_vm
from pairing_ref import P, R


def _count(cases):
    return dict(collections.Counter(c.cls for c in cases))


def test_class_counts():
    """every class of the issue is there, none filtered out"""
    assert _count(pcs.fe_cases()) == pcs.FE_CLASSES
    assert _count(pcs.cyc_cases()) == pcs.CYC_CLASSES
    assert _count(pcs.op_cases()) == pcs.OP_CLASSES
    assert _count(pcs.line_cases()) == pcs.LINE_CLASSES
    assert _count(pcs.miller_cases()) == pcs.MILLER_CLASSES
    assert _count(pcs.final_cases()) == pcs.FINAL_CLASSES
    assert _count(pcs.gfin_cases()) == pcs.GFIN_CLASSES
    zs = [c.z for c in pcs.rs_cases(pairing_vm.rlc_scalar, pairing_vm.LAMBDA)]
    assert tuple(zs[:4]) == pcs.RS_Z and len(zs) == 5 and zs[4] not in pcs.RS_Z
    assert sum(pcs.FE_CLASSES.values()) == 26 and len(pcs.FE_CLASSES) == 12


def test_reference_round_trips_and_field_laws():
    rng = random.Random(0x7E57)
    a, b, c = (pcs._f12(rng) for _ in range(3))
    pa, pb, pc_ = ref.to_poly(a), ref.to_poly(b), ref.to_poly(c)
    for t in (a, b, pcs.ONE_T, pcs.ZERO_T, pcs.PM1_T):
        assert ref.from_poly(ref.to_poly(t)) == t and ref.unflat(ref.flat(t)) == t
    assert ref.to_poly(ref.from_poly(pa)) == pa
    assert ref.to_poly(pcs.ONE_T) == ref.ONE and ref.to_poly(pcs.ZERO_T) == ref.ZERO
    # u = w^6 - 1 squares to -1; v = w^2 cubes to xi = 1 + u; w squares to v
    u = ref.to_poly((((0, 1), pcs.Z2, pcs.Z2), pcs.Z6))
    v = ref.to_poly((((0, 0), (1, 0), pcs.Z2), pcs.Z6))
    w = ref.to_poly((pcs.Z6, ((1, 0), pcs.Z2, pcs.Z2)))
    assert ref.mul(u, u) == (P - 1,) + (0,) * 11
    assert ref.pow(v, 3) == ref.to_poly((((1, 1), pcs.Z2, pcs.Z2), pcs.Z6)) and ref.mul(w, w) == v
    assert ref.mul(pa, pb) == ref.mul(pb, pa)
    assert ref.mul(ref.mul(pa, pb), pc_) == ref.mul(pa, ref.mul(pb, pc_))
    s = tuple((x + y) % P for x, y in zip(pb, pc_))
    assert ref.mul(pa, s) == tuple((x + y) % P for x, y in zip(ref.mul(pa, pb), ref.mul(pa, pc_)))
    assert ref.mul(ref.inv(pa), pa) == ref.ONE and ref.inv(ref.ZERO) == ref.ZERO
    f = pa
    for k in range(12):
        assert (f == pa) == (k == 0)
        f = ref.frob(f)
    assert f == pa
    assert ref.frob(ref.mul(pa, pb)) == ref.mul(ref.frob(pa), ref.frob(pb))
    assert ref.conj(pa) == ref.to_poly((a[0], tuple((-x[0] % P, -x[1] % P) for x in a[1])))
    assert ref.pow(ref.final_exp(pa), R) == ref.ONE


def test_reference_pairing_is_bilinear():
    """e([a] P, [b] Q) = e(P, Q)^(ab) and e(P, Q) e(-P, Q) = 1 with the reference's power; the
    pairing is not degenerate"""
    e = pcs.pairing3([(bls.G1_GEN, bls.G2_GEN)])
    assert e != ref.ONE and ref.pow(e, R) == ref.ONE
    a, b = 0xA5A5A5A5A5A5A5A5A5, R - 0x1234567
    assert pcs.pairing3([(pcs.g1_mul(a), pcs.g2_mul(b))]) == ref.pow(e, a * b % R)
    assert pcs.pairing3([(pcs.g1_mul(a), bls.G2_GEN)]) == pcs.pairing3([(bls.G1_GEN, pcs.g2_mul(a))]) == ref.pow(e, a)
    assert ref.mul(e, pcs.pairing3([(pcs.NG1, bls.G2_GEN)])) == ref.ONE
    by_name = {c.name: c for c in pcs.miller_cases()}
    assert by_name["(G1, G2) affine"].fe == ref.from_poly(e)
    for c in pcs.miller_cases():
        if c.cls in ("scaled",) or c.name == "([r - 1] G1, -G2)":
            assert c.fe == ref.from_poly(e), c.name
        if c.cls == "cancel":
            assert c.fe == pcs.ONE_T
    assert by_name["(-G1, G2)"].fe == by_name["(G1, -G2), Z = p - 1"].fe == ref.from_poly(ref.inv(e))


def test_case_classes_have_their_property():
    fe = pcs.fe_cases()
    for c in fe:
        assert c.ok == int(c.fe == pcs.ONE_T), c.name
        want = {"zero": 0, "random": 0, "all_pm1": 0, "near_rth": 0}.get(c.cls, 1)
        assert c.ok == want, (c.name, c.ok)
        if c.cls == "one_hot":
            assert sum(x != 0 for x in ref.flat(c.f)) == 1
    assert {ref.flat(c.f).index(max(ref.flat(c.f))) for c in fe if c.cls == "one_hot"} == set(range(12))
    assert next(c for c in fe if c.cls == "zero").fe == pcs.ZERO_T
    gr = next(c for c in fe if c.cls == "rth_power")
    near = next(c for c in fe if c.cls == "near_rth")
    assert gr.f != pcs.ONE_T and sum(x != y for x, y in zip(ref.flat(gr.f), ref.flat(near.f))) == 1
    for c in pcs.cyc_cases():      # cyclotomic: a^(p^4 - p^2 + 1) = 1, so conjugate = inverse
        a = ref.to_poly(c.a)
        assert ref.mul(a, ref.conj(a)) == ref.ONE and ref.pow(a, P ** 4 - P ** 2 + 1) == ref.ONE, c.name
        assert ref.mul(ref.to_poly(c.expx), ref.pow(a, ref.X_ABS)) == ref.ONE, c.name
    for c in pcs.final_cases():
        want = {"replaced": 0}.get(c.cls, 1) if c.name != "S = O everywhere, F random" else 0
        assert c.ok == want, c.name
        if c.cls in ("cancels", "all_inf"):
            assert c.S is None
        else:
            assert c.S is not None and bls.on_curve(bls.Fp2Ops, c.S)
        live = int(c.name[0]) if c.cls == "live" else {"all_inf": 0, "swapped": 4, "replaced": 3}.get(c.cls, 2)
        assert sum(pcs.aff2(s) is not None for _, s in c.parts) == live, c.name
    assert [int(c.name[0]) for c in pcs.final_cases() if c.cls == "live"] == [1, 2, 3, 4]
    d = next(c for c in pcs.final_cases() if c.cls == "doubles")
    assert pcs.aff2(d.parts[0][1]) == pcs.aff2(d.parts[1][1])
    assert [c.ok for c in pcs.gfin_cases()] == [1, 1, 0]
    for c in pcs.rs_cases(pairing_vm.rlc_scalar, pairing_vm.LAMBDA):
        assert (c.want is None) == (c.z == 0)
        # tau as the product derives it: -psi^2(sigma)
        assert c.tau == bls.pt_neg(bls.Fp2Ops, bls.g2_psi(bls.g2_psi(c.sigma)))


def test_oracle_tower_agrees_with_reference_on_every_case():
    for c in pcs.op_cases():
        assert bls.f12_mul(c.a, c.b) == c.mul, c.name
        assert bls.f12_sqr(c.a) == c.sqr, c.name
        assert bls.f12_frob(c.a) == c.frob, c.name
        assert bls.f12_conj(c.a) == ref.from_poly(ref.conj(ref.to_poly(c.a))), c.name
        if c.a != pcs.ZERO_T:
            assert bls.f12_inv(c.a) == c.inv, c.name
    for c in pcs.line_cases():
        assert bls.f12_mul_by_014(c.f, c.l0, c.l1, c.l4) == c.out, c.name
    for c in pcs.cyc_cases():
        assert bls.f12_sqr(c.a) == c.sqr and bls.f12_cyc_exp_x(c.a) == c.expx, c.name
    for c in pcs.fe_cases():
        assert bls.f12_frob(c.f) == ref.from_poly(ref.frob(ref.to_poly(c.f))), c.name
        if c.cls != "zero":     # the oracle inverts by Fp inversion, undefined at 0
            assert bls.final_exponentiation_x_chain(c.f) == c.fe, c.name
            fe1 = bls.final_exponentiation(c.f)
            assert bls.f12_mul(bls.f12_sqr(fe1), fe1) == c.fe, c.name
        assert bls.f12_is_one(c.fe) == bool(c.ok)


def test_oracle_miller_loops_agree_after_the_reference_fe():
    """the oracle's projective loop (the shape the VM's follows) against its affine one"""
    for c in pcs.miller_cases():
        m = bls.F12_ONE
        for p_, q_ in c.pairs:
            m = bls.f12_mul(m, bls.miller_loop_proj(pcs.aff1(p_), pcs.aff2(q_)))
        assert pcs.fe_of(m) == c.fe, c.name


def test_comparison_helper_rejects_one_limb_and_a_flipped_ok():
    """vm_helpers.assert_same, through which every interpreter result of the pairing tests is
    compared with the simulator: equal results pass; one limb of one coefficient changed, a
    flipped ok bit, and a non-canonical stored plane do not."""
    RM = pairing_vm.R
    c = next(c for c in pcs.fe_cases() if c.cls == "random")
    sim = {"st:f%d" % k: v for k, v in enumerate(ref.flat(c.fe))}
    sim["ok"] = 0
    good = {n: (v * RM % P if n != "ok" else v) for n, v in sim.items()}
    assert pairing_vm.same_outputs(good, sim)
    for k in range(12):
        for limb in (0, 5, 11):
            bad = dict(good)
            bad["st:f%d" % k] ^= 1 << (32 * limb)
            assert not pairing_vm.same_outputs(bad, sim), (k, limb)
    assert pairing_vm.same_outputs(pcs.perturb(good), sim) is False
    assert not pairing_vm.same_outputs(dict(good, ok=1), sim)
    assert not pairing_vm.same_outputs(dict(good, ok=RM), sim)
    assert not pairing_vm.same_outputs(dict(good, **{"st:f3": good["st:f3"] + P}), sim)
    sim1 = dict(sim, ok=1)
    assert pairing_vm.same_outputs(dict(good, ok=1), sim1) and not pairing_vm.same_outputs(dict(good, ok=0), sim1)
    # the value-level comparison of the simulator with the reference is plain equality of towers
    assert pairing_vm.tower_out(sim) == c.fe and pairing_vm.tower_out(pcs.perturb(sim)) != c.fe
