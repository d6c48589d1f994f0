"""The crafted points of tests/point_cases.py through the generated Fp-VM programs on the
interpreter's own code (consensus_overlord_amd/csrc/fpvm.hpp exec, host build), in both
interpreter modes: interpreter == slot-level simulator == the cases' big-integer expectations
(tests/point_vm.py). sigchk / pkchk / pkdec take every case; the whole-vote programs take one
case per class. Alg.f2_sqrt (the norm method, no generated program uses it by default) is
evaluated on the DAG."""
import pytest

import point_cases as pc
import point_vm
from test_host_harness import hx  # noqa: F401  (module fixture: builds libhx.so)

import ir  # noqa: E402  (tools/fpvm: vm_helpers, imported by point_vm, puts it on the path)
from alg import Alg  # noqa: E402


@pytest.mark.parametrize("any_all", [0, 1])
def test_check_programs_on_every_case(hx, any_all):  # noqa: F811
    g1, g2 = pc.cases()
    want = 2 * sum(c.program for c in g1) + sum(c.program for c in g2)
    assert point_vm.run_single(hx, False, any_all) == want


@pytest.mark.parametrize("any_all", [0, 1])
def test_lex_sgn0_program(hx, any_all):  # noqa: F811
    assert point_vm.run_lex(hx, False, any_all) == 20


@pytest.mark.parametrize("any_all", [0, 1])
@pytest.mark.parametrize("name", point_vm.WHOLE)
def test_vote_programs_on_one_case_per_class(hx, name, any_all):  # noqa: F811
    pairs = point_vm.vote_pairs()
    keys = {k.cls for k, _ in pairs if k is not None}
    sigs = {s.cls for _, s in pairs if s is not None}
    assert keys == set(pc.G1_CLASSES) - {"x_ge_p"} and sigs == set(pc.G2_CLASSES) - {"x_ge_p"}
    n = point_vm.run_whole(hx, False, name, any_all)
    assert n == (len(pairs) if name not in point_vm.NO_KEY else len(sigs))


def test_norm_method_sqrt_on_g2_cases():
    """Alg.f2_sqrt on x^3 + 4 + 4i of every G2 case (ir.Prog.evaluate): the same `ok` as the
    case, and a root whose square is the right-hand side; g2_decompress over it (fast_sqrt off)
    gives the case's exact y."""
    pr = ir.Prog("normsqrt")
    a = Alg(pr, fast_sqrt=False)
    x = (pr.input("x0"), pr.input("x1"))
    rhs = a.f2_add(a.f2_mul(x, a.f2_sqr(x)), a.c2((4, 4)))
    ok, r = a.f2_sqrt(rhs)
    dok, (_, y) = a.g2_decompress(x, pr.input("sort"))
    outs = {"ok": ok, "r0": r[0], "r1": r[1], "dok": dok, "y0": y[0], "y1": y[1]}
    n = 0
    for c in pc.cases()[1]:
        if not c.program:
            continue
        vals = pr.evaluate({"x0": c.x[0], "x1": c.x[1], "sort": c.sort}, 0)
        got = {k: vals[v.id] for k, v in outs.items()}
        assert got["ok"] == got["dok"] == int(c.on_curve), c.name
        if c.on_curve:
            root = (got["r0"], got["r1"])
            assert pc.Fp2.mul(root, root) == pc.rhs(pc.Fp2, c.x), c.name
            assert (got["y0"], got["y1"]) == c.y, c.name
        n += 1
    assert n >= 40


def test_pt_eq_with_a_side_at_infinity():
    """Alg.pt_eq leaves infinity to its callers; what it answers there is pinned on the DAG: a
    finite point against (0 : Y : 0), Y != 0 (what the complete formulas give for O) is unequal
    on both curves, in either order; two such infinities are equal; a point equals a rescaled
    copy of itself and differs from its negative."""
    g1, g2 = pc.cases()
    A1 = next(c for c in g1 if c.name == "order 11").point
    A2 = next(c for c in g2 if c.name == "order 13").point
    pr = ir.Prog("pteq")
    a = Alg(pr)
    names = ["X", "Y", "Z", "U", "V", "W"]
    one = [pr.input("a" + n) for n in names[:3]], [pr.input("b" + n) for n in names[:3]]
    two = tuple(tuple((pr.input("%s%s0" % (s_, n)), pr.input("%s%s1" % (s_, n))) for n in names[:3]) for s_ in "cd")
    e1 = a.pt_eq("fp", tuple(one[0]), tuple(one[1]))
    e2 = a.pt_eq("f2", two[0], two[1])

    def run(P1, Q1, P2, Q2):
        inp = {}
        for s_, pt in (("a", P1), ("b", Q1)):
            inp.update({s_ + n: v for n, v in zip(names, pt)})
        for s_, pt in (("c", P2), ("d", Q2)):
            for n, v in zip(names, pt):
                inp["%s%s0" % (s_, n)], inp["%s%s1" % (s_, n)] = v
        vals = pr.evaluate(inp, 0)
        return vals[e1.id], vals[e2.id]
    f1, f2 = (A1[0], A1[1], 1), (A2[0], A2[1], (1, 0))
    k = 0x1234567
    s1 = (A1[0] * k % pc.P, A1[1] * k % pc.P, k)
    s2 = (pc.Fp2.mul(A2[0], (k, 3)), pc.Fp2.mul(A2[1], (k, 3)), (k, 3))
    n1, n2 = (A1[0], pc.P - A1[1], 1), (A2[0], pc.Fp2.neg(A2[1]), (1, 0))
    o1, o2 = (0, 5, 0), ((0, 0), (5, 7), (0, 0))
    p1, p2 = (0, 9, 0), ((0, 0), (0, 2), (0, 0))
    assert run(f1, s1, f2, s2) == (1, 1)
    assert run(f1, n1, f2, n2) == (0, 0)
    assert run(f1, o1, f2, o2) == (0, 0)
    assert run(o1, f1, o2, f2) == (0, 0)
    assert run(o1, p1, o2, p2) == (1, 1)
