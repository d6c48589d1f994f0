"""The radix a program carries (tools/fpvm): `vote` and `vote_t`, the vote pool's programs, are
radix 2^392 and every other program 2^384; every product op of the two carries the WIDE bit and
no other instruction anywhere does; the conversion products at the two programs' edges stay
within their budget against the radix-384 programs they replaced; and the vote pool's compact
constant table with its renumbered copies of the programs (csrc/ovhip/pool_remap.hpp, run here
through the host harness) computes exactly what the generated table and code compute, which is
what the slot-level simulator computes."""
import ctypes

import numpy as np
import pytest

from test_fp_wide_host import build_wx, u16p, u32p
from test_host_harness import hx  # noqa: F401  (module fixture: builds libhx.so)
from vm_helpers import assert_same, build_all, gen, golden_vote_inputs, run_vm, sched

import progs  # noqa: E402  (tools/fpvm: vm_helpers puts it on the path)

WIDE_PROGRAMS = ("vote", "vote_t")
PRODUCT_OPCODES = {sched.OPC[k] for k in sched.PRODUCTS}
# the programs before the change (radix 384, no conversions): Montgomery products and phases
BEFORE = {"vote": (18318, 2716), "vote_t": (16691, 2705)}
MAX_EXTRA_PRODUCTS, MAX_EXTRA_PHASES = 30, 4


@pytest.fixture(scope="module")
def built():
    return build_all()


def test_radix_of_every_program(built):
    _, progs_ = built
    assert set(WIDE_PROGRAMS) <= set(progs_)
    for name, (prog, _, _, _, _) in progs_.items():
        assert prog.radix == (392 if name in WIDE_PROGRAMS else 384), name


def test_wide_bit_on_product_ops_only(built):
    _, progs_ = built
    for name, (prog, sc, words, _, _) in progs_.items():
        products = wide = 0
        for k in range(0, len(words), 4):
            is_product = (words[k] & 31) in PRODUCT_OPCODES
            products += is_product
            if words[k + 3] & sched.WIDE:
                assert is_product and name in WIDE_PROGRAMS, (name, k // 4, hex(words[k]))
                wide += 1
        assert wide == (products if name in WIDE_PROGRAMS else 0), (name, wide, products)
        if name in WIDE_PROGRAMS:
            assert products == sc.stats()["heavy_ops"]   # no inversion: every heavy op is a product
            # the radix is read from the first lane of a product phase (fpvm.hpp exec)
            for t in range(sc.nrounds):
                w = words[t * sc.W * 4:t * sc.W * 4 + 4]
                if w[0] & sched.H_MUL:
                    assert w[3] & sched.WIDE, (name, t)


@pytest.mark.parametrize("name", WIDE_PROGRAMS)
def test_conversion_budget(built, name):
    st = built[1][name][1].stats()
    products, phases = BEFORE[name]
    print("\n%s: %d products (+%d), %d phases (%+d)" % (name, st["heavy_ops"], st["heavy_ops"] - products,
                                                        st["phases"], st["phases"] - phases))
    assert 0 < st["heavy_ops"] - products <= MAX_EXTRA_PRODUCTS
    assert st["phases"] - phases <= MAX_EXTRA_PHASES


def test_pool_table_is_no_larger_than_the_prefix(built):
    consts, progs_ = built
    pidx = gen.pool_table(consts, progs_)
    assert len(pidx) <= len(consts.entries)
    assert pidx[:sched.NFIXED] == list(range(sched.NFIXED))
    # every wide entry once, at a pool index in its table index's bank residue (the padding before
    # them repeats the zero entry)
    npre = len(consts.entries)
    wide = [(k, g) for k, g in enumerate(pidx) if g >= npre]
    assert [g for _, g in wide] == list(range(npre, npre + len(consts.wide)))
    assert all((k - g) % sched.BANK_MOD == 0 for k, g in wide)
    assert all(g < sched.NFIXED or g >= npre or g == gen.KZERO or g in pidx[:wide[0][0]] for g in pidx)
    assert len(consts.words()) == npre + len(consts.wide)


class PoolConsts:
    """What run_vm asks of a constant table: words()"""

    def __init__(self, rows):
        self.rows = rows

    def words(self):
        return self.rows


@pytest.fixture(scope="module")
def pool_side(built):
    """The pool's table and its copies of vote, vote_t and fold, made by the C++ the library
    uploads them with."""
    consts, progs_ = built
    wx = build_wx()
    pidx = gen.pool_table(consts, progs_)
    idx = np.array(pidx, dtype=np.uint16)
    table = np.array(consts.words(), dtype=np.uint32).ravel()
    out = np.zeros(len(pidx) * 12, dtype=np.uint32)
    wx.wx_pool_consts(out.ctypes.data_as(u32p), table.ctypes.data_as(u32p), idx.ctypes.data_as(u16p), len(pidx))
    codes = {}
    for name in WIDE_PROGRAMS + ("fold",):
        words = np.array(progs_[name][2], dtype=np.uint32)
        pc = np.zeros_like(words)
        assert wx.wx_pool_remap(pc.ctypes.data_as(u32p), words.ctypes.data_as(u32p), len(words),
                                idx.ctypes.data_as(u16p), len(pidx)) == 0, name
        codes[name] = [int(w) for w in pc]
        # the generator's own statement of the same function
        assert codes[name] == gen.pool_remap(pidx, progs_[name][2], len(consts.words())), name
    return PoolConsts(out.reshape(-1, 12).tolist()), codes, wx, idx


def test_pool_remap_refuses_a_missing_constant(built, pool_side):
    consts, progs_ = built
    _, _, wx, idx = pool_side
    # `final` names constants of the 384 prefix the pool table does not carry
    words = np.array(progs_["final"][2], dtype=np.uint32)
    pc = np.zeros_like(words)
    assert wx.wx_pool_remap(pc.ctypes.data_as(u32p), words.ctypes.data_as(u32p), len(words), idx.ctypes.data_as(u16p),
                            len(idx)) != 0


def test_pool_copies_compute_what_the_table_computes(hx, built, pool_side):  # noqa: F811
    """vote on the golden inputs (two valid votes, one failing), vote_t on the first with a
    projective key: compact table + renumbered code == generated table + code == simulator."""
    consts, progs_ = built
    pconsts, pcodes, _, _ = pool_side
    r = 0xD7A1C3B5E9F20486
    g = golden_vote_inputs()
    bls = gen._oracle()
    import json
    import os
    with open(os.path.join(os.path.dirname(__file__), "golden", "golden_v1.json")) as fh:
        pk = bls.g1_from_bytes(bytes.fromhex(json.load(fh)["keys"][0]["pk"]))
    tin = {n: g[0][n] for n in ("sig_x0", "sig_x1", "sig_sort", "u00", "u01", "u10", "u11")}
    tin.update(pk_X=pk[0] * 5 % gen.P, pk_Y=pk[1] * 5 % gen.P, pk_Z=5)
    for name, inp in [("vote", x) for x in g] + [("vote_t", tin)]:
        _, sc, words, _, _ = progs_[name]
        sim = sched.simulate(sc, words, inp, r)
        a = run_vm(hx, consts, sc, words, inp, r, 0)
        b = run_vm(hx, pconsts, sc, pcodes[name], inp, r, 0)
        assert a == b, name
        assert_same(a, sim, name)


def test_edge_contract_in_the_simulator(built):
    """Seen from outside the two programs are what they were: the simulator on the first golden vote
    stores the signature's coordinates (value, not value * 2^-8) and raw 0 / 1 flags."""
    _, progs_ = built
    g = golden_vote_inputs()[0]
    _, sc, words, _, _ = progs_["vote"]
    sim = sched.simulate(sc, words, g, 1)
    x1, x0 = g["sig_x1"] * pow(2, 384, gen.P) % gen.P, g["sig_x0"] * pow(2, 384, gen.P) % gen.P
    assert (sim["st:q0"], sim["st:q1"]) == (x0, x1)
    assert [sim[n] for n in progs.VOTE_OUT] == [1, 1, 1, 1, 0]
