"""The programs of the primed routes (tools/fpvm/progs.py votewh, votewh_t, signg0h: votew /
votew_t / signg0 with H = hash_to_G2(hash) as an input) executed by the interpreter's own code
(consensus_overlord_amd/csrc/fpvm.hpp exec, host build in tests/host/harness.cpp): lane by lane
and with every wave-uniform block forced, against the traced DAG's values (which equal votew's /
votew_t's / signg0's for the same scalar: gen.check_votewh, gen.check_signg0h) with every output
a Montgomery representative in [0, 2p)."""
import pytest

from test_host_harness import hx  # noqa: F401  (module fixture: builds libhx.so)
from vm_helpers import P, assert_same, build_all, gen, golden_vote_inputs, load_golden, run_vm, sched

import progs  # noqa: E402  (tools/fpvm: vm_helpers puts it on the path)


@pytest.fixture(scope="module")
def built():
    return build_all()


@pytest.fixture(scope="module")
def cases(built):
    """Per golden vote input (two valid votes, one that fails): the H that vote1 stores."""
    _, progs_ = built
    v1 = progs_["vote1"][0]
    out = []
    for inp in golden_vote_inputs():
        vals = v1.evaluate(inp, 1)
        out.append((inp, {"h%d" % k: vals[v1.outputs["st:h%d" % k]] for k in range(6)}))
    return out


def _run(hx, built, name, inp, scalar, any_all):  # noqa: F811
    consts, progs_ = built
    prog, sc, words, ins, _ = progs_[name]
    assert set(inp) == set(ins)
    vals = prog.evaluate(inp, scalar)
    dag = {n: vals[i] for n, i in prog.outputs.items()}
    assert sched.simulate(sc, words, inp, scalar) == dag, name + ": simulator != DAG"
    assert_same(run_vm(hx, consts, sc, words, inp, scalar, any_all), dag, name)
    return dag


@pytest.mark.parametrize("any_all", [0, 1])
def test_votewh_programs_on_interpreter(hx, built, cases, any_all):  # noqa: F811
    _, progs_ = built
    wp, tp = progs_["votew"][0], progs_["votew_t"][0]
    bls = gen._oracle()
    g = load_golden()
    r = 0x9E3779B97F4A7C15
    for k, (inp, H) in enumerate(cases):
        hin = {n: inp[n] for n in ("pk_x", "pk_sort", "sig_x0", "sig_x1", "sig_sort")}
        hin.update(H)
        o = _run(hx, built, "votewh", hin, r, any_all)
        wv = wp.evaluate(inp, r)
        assert [o["st:f%d" % j] for j in range(12)] == [wv[wp.outputs["st:f%d" % j]] for j in range(12)], k
        if k >= 2:
            continue
        pk = bls.g1_from_bytes(bytes.fromhex(g["keys"][k]["pk"]))
        tin = {n: inp[n] for n in ("sig_x0", "sig_x1", "sig_sort")}
        tin.update(pk_X=pk[0] * 5 % P, pk_Y=pk[1] * 5 % P, pk_Z=5)
        tin.update(H)
        o = _run(hx, built, "votewh_t", tin, r, any_all)
        win = {n: inp[n] for n in ("sig_x0", "sig_x1", "sig_sort", "u00", "u01", "u10", "u11")}
        win.update(pk_X=tin["pk_X"], pk_Y=tin["pk_Y"], pk_Z=5)
        tv = tp.evaluate(win, r)
        assert [o["st:f%d" % j] for j in range(12)] == [tv[tp.outputs["st:f%d" % j]] for j in range(12)], k


@pytest.mark.parametrize("any_all", [0, 1])
def test_signg0h_program_on_interpreter(hx, built, cases, any_all):  # noqa: F811
    _, progs_ = built
    p0 = progs_["signg0"][0]
    g = load_golden()
    for k, (inp, H) in enumerate(cases[:2]):
        sc = gen.signg_scalar(gen.gls_digits(int(g["keys"][k]["sk"], 16)), 0)
        o = _run(hx, built, "signg0h", dict(H), sc, any_all)
        want = p0.evaluate({n: inp[n] for n in progs.SIGN0_IN}, sc)
        assert o == {n: want[i] for n, i in p0.outputs.items()}, k
