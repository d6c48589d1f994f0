"""The crafted points of tests/point_cases.py through the Fp-VM programs that decompress and
group-check (tools/fpvm/alg.py g1_decompress, g2_decompress, f2_sqrt9, f2_lex, g1_in_group,
g2_in_group, pt_eq; each program has its own schedule and encoding): one unit through the host
interpreter (tests/test_vm_host_points.py) or one wave of the device interpreter
(tests/test_gpu_points.py), compared with the slot-level simulator, and the simulator's flags
and coordinates with the case's big-integer expectation. Simulations are kept per process."""
import itertools

import point_cases as pc
from vm_helpers import P, R, assert_same, build_all, golden_vote_inputs, load_golden, gen, run_vm, sched

FLAGS = ("pk_ok", "pk_grp", "sig_ok", "sig_grp", "h_inf", "ok")
SINGLE = ("pkchk", "pkdec", "sigchk")
WHOLE = ("vote", "vote_t", "vote1", "vote1h", "votew", "votewh", "vsame", "qcpre", "vsame_t", "vsame8", "vsame8_t")
NO_KEY = ("vote_t", "qcpre", "vsame_t", "vsame8_t")   # the key is a validator-table point, or the QC's sum
SCALAR = {"vote1": 1, "vote1h": 1}
RLC = 0xA5C3E1F00F1E3C5B
_sims = {}


def _sim(name, key, inp, scalar=0):
    k = (name, key, scalar)
    if k not in _sims:
        _, progs_ = build_all()
        _, sc, words, _, _ = progs_[name]
        _sims[k] = sched.simulate(sc, words, inp, scalar)
    return _sims[k]


def _run(lib, device, any_all, name, key, inp, scalar=0):
    """interpreter == simulator (flags as raw 0 / 1 limbs, values as Montgomery representatives
    below 2p); -> the simulator's outputs"""
    consts, progs_ = build_all()
    _, sc, words, _, _ = progs_[name]
    sim = _sim(name, key, inp, scalar)
    got = run_vm(lib, consts, sc, words, inp, scalar, any_all, device=device)
    what = "%s on %s" % (name, key)
    assert_same(got, sim, what)
    for n, s in sim.items():
        if n in FLAGS:
            assert s in (0, 1) and got[n] == s, (what, n, got[n], s)
        else:
            assert got[n] < 2 * P and got[n] % P == s * R % P, (what, n)
    return sim


# What each program puts out besides pk_ok / sig_ok: whether it group-checks the key, and the
# outputs that hold the decoded key (x, y) and signature (x0, x1, y0, y1). Stated per program, so
# that a renamed output fails here instead of dropping a comparison.
ST_Q = tuple("st:q%d" % k for k in range(4))
KEY_OUT = {"pkchk": (True, ("p0", "p1")), "pkdec": (False, None), "vote": (True, None), "vote1": (True, None),
           "vote1h": (True, None), "votew": (True, None), "votewh": (True, None), "vsame": (True, None), "vsame8": (True, None)}
SIG_OUT = {"sigchk": ("q0", "q1", "q2", "q3"), "vote": ST_Q, "vote_t": ST_Q, "vsame": ST_Q, "vsame_t": ST_Q, "vsame8": ST_Q,
           "vsame8_t": ST_Q, "vote1": None,
           "vote1h": None, "votew": None, "votewh": None, "qcpre": None}


def expect_key(c, sim, name):
    """the simulator's key flags and coordinates == the case"""
    grp, coords = KEY_OUT[name]
    assert ("pk_grp" in sim) == grp and all(n in sim for n in coords or ()), name
    assert sim["pk_ok"] == int(c.on_curve), (name, c.name)
    if c.on_curve:
        if grp:
            assert sim["pk_grp"] == int(c.in_group), (name, c.name)
        if coords:
            assert [sim[n] for n in coords] == [c.x, c.y], (name, c.name)


def expect_sig(c, sim, name):
    coords = SIG_OUT[name]
    assert all(n in sim for n in coords or ()), name
    assert (coords is not None) == any(n in sim for n in ST_Q + ("q0",)), name
    assert sim["sig_ok"] == int(c.on_curve), (name, c.name)
    if c.on_curve:
        assert sim["sig_grp"] == int(c.in_group), (name, c.name)
        if coords:
            assert [sim[n] for n in coords] == [c.x[0], c.x[1], c.y[0], c.y[1]], (name, c.name)


def run_single(lib, device, any_all=0):
    """pkchk and pkdec on every G1 case, sigchk on every G2 case -> the number of runs"""
    g1, g2 = pc.cases()
    n = 0
    for c in g1:
        if c.program:
            for name in ("pkchk", "pkdec"):
                expect_key(c, _run(lib, device, any_all, name, "G1 " + c.name, c.inputs()), name)
                n += 1
    for c in g2:
        if c.program:
            expect_sig(c, _run(lib, device, any_all, "sigchk", "G2 " + c.name, c.inputs()), "sigchk")
            n += 1
    return n


def vote_pairs():
    """One case per class of each group, a key beside a signature (the flags of the two halves
    are separate outputs); the shorter list is filled with the golden vote's own side (None)."""
    g1, g2 = pc.cases()
    pairs = list(itertools.zip_longest(pc.subset(g1), pc.subset(g2)))
    assert 0 < len(pairs) <= 10
    return pairs


def _golden_h():
    """H of golden vote 0, projective, as vote1 stores it (the input of vote1h / votewh)"""
    sim = _sim("vote1", "golden 0", golden_vote_inputs()[0], 1)
    assert sim["pk_ok"] == sim["pk_grp"] == sim["sig_ok"] == sim["sig_grp"] == 1
    return {"h%d" % k: sim["st:h%d" % k] for k in range(6)}


def run_whole(lib, device, name, any_all=0):
    """Program `name` on golden vote 0 with a crafted key and / or signature in place of its own:
    flags (and the stored sigma, where the program stores it) == the cases' -> number of runs"""
    _, progs_ = build_all()
    ins = progs_[name][3]
    gold = golden_vote_inputs()[0]
    takes_key = "pk_x" in ins
    base = dict(gold)
    if "h0" in ins:
        base.update(_golden_h())
    if "pk_X" in ins:
        bls = gen._oracle()
        pk = bls.g1_from_bytes(bytes.fromhex(load_golden()["keys"][0]["pk"]))
        base.update(pk_X=pk[0] * 5 % P, pk_Y=pk[1] * 5 % P, pk_Z=5)
    scalar = SCALAR.get(name, RLC)
    n = 0
    for kc, sc_ in vote_pairs():
        if not takes_key:
            kc = None
            if sc_ is None:
                continue
        inp = {k: base[k] for k in ins}
        if kc is not None:
            inp.update(kc.inputs())
        if sc_ is not None:
            inp.update(sc_.inputs())
        key = "key %s | sig %s" % (kc.name if kc else "golden", sc_.name if sc_ else "golden")
        sim = _run(lib, device, any_all, name, key, inp, scalar)
        if takes_key:
            if kc is not None:
                expect_key(kc, sim, name)
            else:
                assert sim["pk_ok"] == sim["pk_grp"] == 1, name
        if sc_ is not None:
            expect_sig(sc_, sim, name)
        else:
            assert sim["sig_ok"] == sim["sig_grp"] == 1, name
        n += 1
    return n


def run_lex(lib, device, any_all=0):
    """The lex / sgn0 program on raw representatives m and m + p of (p - 1) / 2, (p + 1) / 2, 0, 1
    and p - 1: interpreter == simulator == the integers."""
    consts, pr, sc, words = pc.lex_prog()
    want = pc.lex_expected()
    sim = sched.simulate(sc, words, pc.lex_canon_inputs(), 0)
    assert sim == want
    vals = pr.evaluate(pc.lex_canon_inputs(), 0)
    assert {n: vals[v] for n, v in pr.outputs.items()} == want
    got = run_vm(lib, consts, sc, words, {}, 0, any_all, raw_slots=pc.lex_raw_inputs(), device=device)
    assert got == want, {n: (got[n], want[n]) for n in want if got[n] != want[n]}
    return len(want)
