"""A small synthetic Fp-VM program over raw slot representatives at the edges of the
interpreter's lazy-reduction contract (csrc/fpvm.hpp): the input slots hold p, 2p - 1, p - 1 and
0 as written, so pre-adds reach 4p - 2 and 4p - 1, the equality tests compare values that are
equal only modulo p, and the unit and general linear blocks see the extremes of [0, 2p).
Run on the host interpreter by tests/test_fp_bounds_host.py and on the device by
tests/test_gpu_fp_bounds.py; the expectation is the Python evaluation of the same ops modulo p
(ir.Prog.evaluate, and sched.simulate on the encoded stream)."""
import random

from vm_helpers import P, assert_same, gen, run_vm, sched

import ir  # tools/fpvm: vm_helpers puts it on the path

W = 16
RINV = pow(1 << 384, -1, P)
SCALARS = (1, 1 << 63)   # selb reads bits 0 and 63


def raw_inputs():
    """Slot contents as written (Montgomery representatives below 2p)."""
    rng = random.Random(0xED6E)
    raw = {"a": P, "b": 2 * P - 1, "c": P - 1, "z": 0}
    raw.update({n: rng.randrange(2 * P) for n in ("u", "v", "w")})
    return raw


def build():
    """-> (consts, prog, sc, words)"""
    consts = sched.ConstTable()
    consts.ref(1, True)
    assert consts.ref(0, False) - sched.CONST_BASE == gen.KZERO
    for n in range(5):
        assert consts.ref(n * (2 * P + 1), True) - sched.CONST_BASE == gen.KTAB + n
    pr = ir.Prog("edge")
    a, b, c, z, u, v, w = (pr.input(n) for n in ("a", "b", "c", "z", "u", "v", "w"))
    vals = {}
    # products: a negated y operand, a negated x operand (the encoder moves it to y), and the
    # largest pre-adds: x = (2p - 1) + (2p - 1) = 4p - 2, y = (2p - 1) + (2p - 0) = 4p - 1
    vals["m_negy"] = pr.muls(u, 1, v, w, -1, b)
    vals["m_negx"] = pr.muls(u, -1, b, w, 1, v)
    vals["m_top"] = pr.muls(b, 1, b, b, -1, z)
    vals["m_plain"] = pr.muls(a, 1, c, b, 1, b)
    # unit sums with 1, 2 and 3 negated terms, and scaled ones (k = 3, 5, 15)
    vals["l_neg1"] = pr.lin([(1, u), (1, v), (1, w), (-1, b)])
    vals["l_neg2"] = pr.lin([(1, u), (1, v), (-1, c), (-1, b)])
    vals["l_neg3"] = pr.lin([(1, u), (-1, a), (-1, c), (-1, b)])
    vals["l_zero3"] = pr.lin([(1, z), (-1, z), (-1, a), (-1, b)])
    vals["l_k3"] = pr.lin([(3, u), (-3, b)])
    vals["l_k5"] = pr.lin([(5, u), (5, v), (-5, w), (-5, b)])
    vals["l_k15"] = pr.lin([(15, b), (15, c), (15, w), (-15, z)])
    # general coefficients, +-15 on the extremes. Each takes a scaled sum, so it is scheduled after
    # all of them: a phase with a general lin runs every lin op in the general block (sched.encode),
    # and the scaled unit sums must reach lin_sum + scale_reduce (check_coverage)
    vals["g_mix"] = pr.lin([(15, vals["l_neg1"]), (-15, vals["l_neg2"]), (7, vals["l_k3"]), (-15, b)])
    vals["g_neg"] = pr.lin([(-15, b), (-15, vals["l_neg3"]), (-15, c), (-15, vals["l_k5"])])
    vals["g_pos"] = pr.lin([(15, b), (15, vals["l_k15"]), (15, vals["m_top"]), (-1, z)])
    # flags: equal only modulo p (p vs 0, 2p - 1 vs p - 1), unequal, parity and order of the
    # canonical from-Montgomery value
    flags = {"e_p_0": pr.eq(a, z), "e_2p1_p1": pr.eq(b, c), "e_ne": pr.eq(u, v), "e_self": pr.eq(vals["m_top"], vals["m_top"]),
             "s_u": pr.sgn0(u), "s_b": pr.sgn0(b), "s_a": pr.sgn0(a), "x_u": pr.lex(u), "x_c": pr.lex(c), "x_a": pr.lex(a)}
    flags["f_and"] = pr.f_and(flags["e_p_0"], flags["e_ne"])
    flags["f_or"] = pr.f_or(flags["e_p_0"], flags["e_ne"])
    flags["f_xor"] = pr.f_xor(flags["e_2p1_p1"], flags["s_u"])
    vals["sel_t"] = pr.sel(flags["e_p_0"], u, b)
    vals["sel_f"] = pr.sel(flags["e_ne"], u, b)
    vals["selb0"] = pr.selb(0, v, b)
    vals["selb63"] = pr.selb(63, w, a)
    vals["in_b"] = b   # `st` canonicalises a raw 2p - 1 and a raw p
    vals["in_a"] = a
    for k, (name, val) in enumerate(vals.items()):
        pr.store(name, val, k)
    for name, val in flags.items():
        pr.output(name, val)
    sc = sched.schedule(pr, W, consts, max_slots=128)
    words = sched.encode(sc)
    return consts, pr, sc, words


def header_bits(sc, words):
    """The union of the phase headers, and the set of distinct headers."""
    hdrs = {words[t * sc.W * 4] & ~0x3FFFFF for t in range(sc.nrounds)}
    union = 0
    for h in hdrs:
        union |= h
    return union, hdrs


def check_coverage(sc, words):
    """The schedule exercises what the program is for: products with a negated operand, flag
    products, the unit block with each of its three negation chains and with scales above 1 (read
    from the encoded lanes, not assumed from the source), the general block, selb and the rare
    ops."""
    union, hdrs = header_bits(sc, words)
    for bit in (sched.H_MUL, sched.H_MULNEG, sched.H_FLAG, sched.H_LIN, sched.H_LINNEG, sched.H_LINNEG2,
                sched.H_LINNEG3, sched.H_ACC, sched.H_RARE, sched.H_SELB):
        assert union & bit, "no phase of the edge program sets header bit %#x" % bit
    # the unit block (lin_sum + scale_reduce) runs lin lanes with each scale of the program, every
    # scaled one with a negated term, and unscaled ones with 1, 2 and 3 negated terms
    scales, negs = set(), set()
    for t in range(sc.nrounds):
        lanes = [words[(t * sc.W + l) * 4:(t * sc.W + l) * 4 + 4] for l in range(sc.W)]
        if not lanes[0][0] & sched.H_LIN or lanes[0][0] & sched.H_ACC:
            continue
        for w in lanes:
            if w[0] & 31 == sched.OPC["lin"]:
                assert not w[3] & sched.FORCE_ACC
                nneg = sum(sched._s5((w[3] >> (5 * q)) & 31) < 0 for q in range(1, 4))
                k = (w[3] >> 20) & 15
                if k > 1:
                    assert nneg >= 1, "scaled unit lin without a negated term"
                    scales.add(k)
                else:
                    negs.add(nneg)
    assert scales == {3, 5, 15}, "scaled unit lins in the unit block: %s" % sorted(scales)
    assert negs >= {1, 2, 3}, "negated terms of the unscaled unit lins: %s" % sorted(negs)


def expected(pr, sc, words, scalar):
    raw = raw_inputs()
    canon = {n: x * RINV % P for n, x in raw.items()}
    sim = sched.simulate(sc, words, canon, scalar)
    vals = pr.evaluate(canon, scalar)
    for name, vid in pr.outputs.items():
        op = pr.ops[vid]
        want = vals[op.srcs[0]] if op.kind == "st" else vals[vid]
        assert sim[name] == want, (name, sim[name], want)
    # the cases where canonicalisation decides the flag
    assert sim["e_p_0"] == 1 and sim["e_2p1_p1"] == 1 and sim["e_ne"] == 0 and sim["e_self"] == 1
    return sim


def run_and_check(lib, device, any_all=0):
    consts, pr, sc, words = build()
    check_coverage(sc, words)
    for scalar in SCALARS:
        sim = expected(pr, sc, words, scalar)
        got = run_vm(lib, consts, sc, words, {}, scalar, any_all, raw_slots=raw_inputs(), device=device)
        assert_same(got, sim, "edge program, scalar %#x" % scalar)
        # flags are raw 0 / 1 limbs exactly
        for name, vid in pr.outputs.items():
            if pr.ops[vid].kind != "st":
                assert got[name] == sim[name], (name, got[name], sim[name])
    return got
