"""The tower and pairing ops of tools/fpvm/alg.py as test-only Fp-VM programs, one per op
(f12_mul, f12_sqr, f12_cyc_sqr, f12_frob, f12_inv, f12_mul_014, f12_exp_x, final_exp, f12_eq_one
and miller_loop_multi for one affine pair, one projective pair and two pairs), scheduled and
encoded with the product's sched.schedule / sched.encode at W = 64 and W = 16, and the product's
own fold / final / final1 / gfin / qcmil / gmil / rs programs, all on the crafted inputs of
tests/pairing_cases.py:

    ir.Prog.evaluate == sched.simulate == the plain-integer reference (tests/pairing_ref.py),
    interpreter (host build: tests/test_vm_host_pairing.py, every case in both any_all modes;
    one wave of the device interpreter: tests/test_gpu_pairing.py) == simulator.

Miller values are compared after the reference's final exponentiation. Programs and simulations
are kept per process."""
import functools

import pairing_cases as pcs
import pairing_ref as ref
from vm_helpers import P, R, assert_same, build_all, gen, run_vm, sched

import ir  # noqa: E402  (tools/fpvm: vm_helpers puts it on the path)
import progs  # noqa: E402
from alg import LAMBDA, Alg, rlc_scalar  # noqa: E402

WIDTHS = (64, 16)
F12 = progs.f12_names
OPS = ("f12_mul", "f12_sqr", "f12_cyc_sqr", "f12_frob", "f12_inv", "f12_mul_014", "f12_exp_x", "final_exp",
       "f12_eq_one", "miller_aff", "miller_proj", "miller_two")
INV_OP = {"f12_inv", "final_exp"}      # as final / final1 / gfin build theirs
_sims = {}


def _in12(pr, prefix):
    return progs.unflat12([pr.input(n) for n in F12(prefix)])


def _in_g2(pr, prefix):
    return progs.unflat_g2p([pr.input(n) for n in progs.g2p_names(prefix)])


def _build(name, pr, a):
    """the op's value(s): a tower element to store, or a flag to put out"""
    if name == "f12_mul":
        return a.f12_mul(_in12(pr, "a"), _in12(pr, "b"))
    if name in ("f12_sqr", "f12_cyc_sqr", "f12_frob", "f12_inv", "f12_exp_x", "final_exp"):
        return getattr(a, name)(_in12(pr, "a"))
    if name == "f12_mul_014":
        ls = [(pr.input("l%d0" % k), pr.input("l%d1" % k)) for k in (0, 1, 4)]
        return a.f12_mul_014(_in12(pr, "a"), *ls)
    if name == "f12_eq_one":
        return a.f12_eq_one(_in12(pr, "a"))
    if name == "miller_aff":
        return a.miller_loop_multi([((pr.input("px"), pr.input("py")), _in_g2(pr, "q"))])
    if name == "miller_proj":
        return a.miller_loop_multi([((pr.input("pX"), pr.input("pY"), pr.input("pZ")), _in_g2(pr, "q"))])
    assert name == "miller_two"   # a projective pair beside an affine one, as gfin pairs them
    return a.miller_loop_multi([((pr.input("pX"), pr.input("pY"), pr.input("pZ")), _in_g2(pr, "q")),
                                ((pr.input("rx"), pr.input("ry")), _in_g2(pr, "s"))])


def _consts():
    consts = sched.ConstTable()
    consts.ref(1, True)
    assert consts.ref(0, False) - sched.CONST_BASE == gen.KZERO
    for n in range(5):
        assert consts.ref(n * (2 * P + 1), True) - sched.CONST_BASE == gen.KTAB + n
    return consts


@functools.lru_cache(maxsize=None)
def program(name, W):
    """-> (consts, prog, sc, words), scheduled as gen.build_all() schedules final / gmil"""
    pr = ir.Prog("t_" + name)
    a = Alg(pr, inv_op=name in INV_OP, use_sop=progs.USE_SOP)
    v = _build(name, pr, a)
    if name == "f12_eq_one":
        pr.output("ok", v)
    else:
        for k, c in enumerate(progs.flat12(v)):
            pr.store("f%d" % k, c, k)
    pr.fuse()
    consts = _consts()
    sc = sched.schedule(pr, W, consts, max_slots=2048, hoist=50, stretch=1.0, mixed=True)
    return consts, pr, sc, sched.encode(sc)


def evaluate(pr, inp, scalar=0):
    """ir.Prog.evaluate -> {output name: value} with the names sched.simulate uses"""
    vals = pr.evaluate(inp, scalar)
    out = {}
    for name, vid in pr.outputs.items():
        op = pr.ops[vid]
        out[name] = vals[op.srcs[0]] if op.kind == "st" else vals[vid]
    return out


def _named(prefix, t):
    return dict(zip(F12(prefix), ref.flat(t)))


def _g2_named(prefix, pt):
    return dict(zip(progs.g2p_names(prefix), progs.flat_g2p(pt)))


def tower_out(sim, prefix="st:f"):
    return ref.unflat([sim["%s%d" % (prefix, k)] for k in range(12)])


def op_runs(name):
    """-> [(case key, inputs, check(sim))]: what program `name` runs on and what its simulator
    outputs must equal"""
    def eq(want):
        return lambda sim: tower_out(sim) == want

    def fe_eq(want):
        return lambda sim: pcs.fe_of(tower_out(sim)) == want
    runs = []
    if name in ("f12_mul", "f12_sqr", "f12_inv", "f12_frob"):
        for c in pcs.op_cases():
            inp = _named("a", c.a)
            if name == "f12_mul":
                inp.update(_named("b", c.b))
            runs.append((c.name, inp, eq(getattr(c, name[4:]))))
            if name != "f12_mul":
                want = {"f12_sqr": ref.mul_t(c.b, c.b), "f12_inv": ref.from_poly(ref.inv(ref.to_poly(c.b))),
                        "f12_frob": ref.from_poly(ref.frob(ref.to_poly(c.b)))}[name]
                runs.append((c.name + " (b)", _named("a", c.b), eq(want)))
        if name == "f12_frob":   # every case of the final exponentiation too: sparse and subfield inputs
            for c in pcs.fe_cases():
                runs.append(("fe " + c.name, _named("a", c.f), eq(ref.from_poly(ref.frob(ref.to_poly(c.f))))))
    elif name == "f12_mul_014":
        for c in pcs.line_cases():
            inp = _named("a", c.f)
            for k, l in ((0, c.l0), (1, c.l1), (4, c.l4)):
                inp["l%d0" % k], inp["l%d1" % k] = l
            runs.append((c.name, inp, eq(c.out)))
    elif name in ("f12_cyc_sqr", "f12_exp_x"):
        for c in pcs.cyc_cases():
            runs.append((c.name, _named("a", c.a), eq(c.sqr if name == "f12_cyc_sqr" else c.expx)))
    elif name == "final_exp":
        for c in pcs.fe_cases():
            runs.append((c.name, _named("a", c.f), eq(c.fe)))
    elif name == "f12_eq_one":
        for c in pcs.fe_cases():
            runs.append((c.name, _named("a", c.f), lambda sim, c=c: sim["ok"] == int(c.f == pcs.ONE_T)))
            runs.append(("FE of " + c.name, _named("a", c.fe), lambda sim, c=c: sim["ok"] == c.ok))
    else:
        for c in pcs.miller_cases():
            (p0, q0) = c.pairs[0]
            if name == "miller_two":
                if len(c.pairs) != 2:
                    continue
                (p1, q1) = c.pairs[1]
                inp = dict(pX=p0[0], pY=p0[1], pZ=p0[2], rx=p1[0], ry=p1[1])
                inp.update(_g2_named("q", q0))
                inp.update(_g2_named("s", q1))
            elif len(c.pairs) != 1 or (len(p0) == 3) != (name == "miller_proj"):
                continue
            elif name == "miller_aff":
                inp = dict(px=p0[0], py=p0[1], **_g2_named("q", q0))
            else:
                inp = dict(pX=p0[0], pY=p0[1], pZ=p0[2], **_g2_named("q", q0))
            runs.append((c.name, inp, fe_eq(c.fe)))
    assert runs, name
    return runs


def _sim(key, pr, sc, words, inp, scalar=0):
    if key not in _sims:
        sim = sched.simulate(sc, words, inp, scalar)
        assert sim == evaluate(pr, inp, scalar), ("simulator != DAG evaluation", key)
        _sims[key] = sim
    return _sims[key]


def _interp(lib, device, any_all, consts, sc, words, inp, sim, what, scalar=0, raw_slots=None):
    got = run_vm(lib, consts, sc, words, inp, scalar, any_all, raw_slots=raw_slots, device=device)
    assert_same(got, sim, what)
    return got


def same_outputs(got, sim):
    """The comparison the interpreter runs go through (vm_helpers.assert_same) as a predicate, so
    that a test can show it rejects a perturbed result."""
    try:
        assert_same(got, sim, "")
    except AssertionError:
        return False
    return True


def run_op(lib, device, name, W, any_all=0):
    """Program `name` at width W on every one of its cases: simulator == DAG == reference,
    interpreter == simulator -> number of runs"""
    consts, pr, sc, words = program(name, W)
    runs = op_runs(name)
    n = 0
    for key, inp, check in runs:
        what = "%s W=%d on %s" % (name, W, key)
        sim = _sim((name, W, key), pr, sc, words, inp)
        assert check(sim), what + ": simulator != reference"
        if lib is not None:
            _interp(lib, device, any_all, consts, sc, words, inp, sim, what)
        n += 1
    return n


def run_eq_one_raw(lib, device, W, any_all=0):
    """f12_eq_one on slot representatives that equal one and zero only modulo p: R + p in place
    0 and p in the others (ok = 1), and the same with one place 2p - 1 (ok = 0)."""
    consts, pr, sc, words = program("f12_eq_one", W)
    names = F12("a")
    RM = R % P
    n = 0
    for tweak, want in ((None, 1), (5, 0), (0, 0)):
        raw = {nm: P for nm in names}
        raw[names[0]] = RM + P
        if tweak is not None:
            raw[names[tweak]] = 2 * P - 1
        canon = {nm: v * pow(R, -1, P) % P for nm, v in raw.items()}
        sim = sched.simulate(sc, words, canon, 0)
        assert sim == {"ok": want} == evaluate(pr, canon)
        got = run_vm(lib, consts, sc, words, {}, 0, any_all, raw_slots=raw, device=device)
        assert got == {"ok": want}, (W, tweak, got)
        n += 1
    return n


# ------------------------------------------------------------------------------ the product programs
ID_F = [1] + [0] * 11
ID_S = [0, 0, 1, 0, 0, 0]


def final_inputs(c):
    inp = {}
    for k, (f, s) in enumerate(c.parts):
        inp.update(_named("F%d_" % k, f))
        inp.update(_g2_named("S%d_" % k, s))
    return inp


def product_runs(name):
    """-> [(class, key, inputs, scalar, check(sim))] for a program of gen.build_all()"""
    runs = []
    if name == "final":
        for c in pcs.final_cases():
            runs.append((c.cls, c.name, final_inputs(c), 0, lambda sim, c=c: sim == {"ok": c.ok}))
    elif name == "fold":
        for c in pcs.final_cases():
            def check(sim, c=c):
                S = progs.unflat_g2p([sim["S%d" % k] for k in range(6)])
                return tower_out(sim, "F") == c.F and pcs.aff2(S) == c.S and (c.S is not None or S[1] != pcs.Z2)
            runs.append((c.cls, c.name, final_inputs(c), 0, check))
    elif name == "final1":
        for c in pcs.fe_cases():
            runs.append((c.cls, c.name, _named("f", c.f), 0, lambda sim, c=c: sim == {"ok": c.ok}))
    elif name == "gfin":
        for c in pcs.gfin_cases():
            inp = _named("F", c.F)
            inp.update(pk_X=c.pk[0], pk_Y=c.pk[1], pk_Z=c.pk[2], **_g2_named("h", c.h))
            inp.update(_g2_named("S", c.S))
            runs.append((c.cls, c.name, inp, 0, lambda sim, c=c: sim == {"ok": c.ok}))
    elif name in ("gmil", "qcmil"):
        g = next(c.f for c in pcs.fe_cases() if c.cls == "random")
        for c in pcs.miller_cases():
            (p0, q0) = c.pairs[0]
            if len(c.pairs) != 1 or len(p0) != 3:
                continue
            inp = dict(pk_X=p0[0], pk_Y=p0[1], pk_Z=p0[2], **_g2_named("h", q0))
            want = c.fe
            if name == "qcmil":      # f = Miller(apk, H) * g
                inp.update(_named("g", g))
                want = ref.mul_t(c.fe, pcs.fe_of(g))
            runs.append((c.cls, c.name, inp, 0, lambda sim, want=want: pcs.fe_of(tower_out(sim)) == want))
    else:
        assert name == "rs"
        for c in pcs.rs_cases(rlc_scalar, LAMBDA):
            inp = dict(zip(progs.RS_IN, [c.sigma[0][0], c.sigma[0][1], c.sigma[1][0], c.sigma[1][1],
                                         c.tau[0][0], c.tau[0][1], c.tau[1][0], c.tau[1][1]]))

            def check(sim, c=c):
                S = progs.unflat_g2p([sim["st:s%d" % k] for k in range(6)])
                return pcs.aff2(S) == c.want and (c.want is not None or S[1] != pcs.Z2)
            runs.append((c.name, c.name, inp, c.z, check))   # every z a class of its own
    assert runs, name
    return runs


PRODUCT = ("final", "final1", "gfin", "fold", "qcmil", "gmil", "rs")


def run_product(lib, device, name, any_all=0, one_per_class=False):
    """Program `name` as gen.build_all() builds it on its crafted cases: simulator == reference,
    interpreter == simulator -> number of runs"""
    consts, progs_ = build_all()
    pr, sc, words, _, _ = progs_[name]
    seen, n = set(), 0
    for cls, key, inp, scalar, check in product_runs(name):
        if one_per_class and cls in seen:
            continue
        seen.add(cls)
        what = "%s on %s" % (name, key)
        sim = _sim((name, None, key), pr, sc, words, inp, scalar)
        assert check(sim), what + ": simulator != reference"
        if lib is not None:
            _interp(lib, device, any_all, consts, sc, words, inp, sim, what, scalar)
        n += 1
    return n
