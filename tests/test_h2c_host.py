"""hash_to_G2 of the device headers (csrc/bls/h2c.hpp, host build in tests/host/harness.cpp) away
from the one DST and the SHA-256-made field elements the rest of the suite uses: every DST length
0 .. 255 through the block templates (each (nb0, nbi) class, the length byte and the 0x80 pad on
block edges), lengths past 255 refused without truncation, and the map to the curve on the
exceptional field inputs (u = 0, u0 = u1, u1 = -u0, zero components, p - 1) -- the one-lane map
directly, and the VM programs through the simulator and the interpreter's own code. Every
expected value comes from the oracles (oracle/py, oracle/c) at test time."""
import ctypes

import pytest

import bls12_381 as bls
import h2c_cases as hc
import orc
from test_host_harness import hx  # noqa: F401  (module fixture: builds libhx.so)
from vm_helpers import assert_same, build_all, gen, load_golden, run_vm

import progs  # noqa: E402  (tools/fpvm: vm_helpers puts it on the path)

P = hc.P


@pytest.fixture(scope="module")
def h2f(hx):  # noqa: F811
    hx.hx_h2f.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p,
                          ctypes.POINTER(ctypes.c_uint32)]

    def call(msg, dst, dst_len=None):
        out = ctypes.create_string_buffer(192)
        nb = (ctypes.c_uint32 * 2)()
        r = hx.hx_h2f(msg, dst, len(dst) if dst_len is None else dst_len, out, nb)
        if r != 0:
            return r, None, None
        return 0, [int.from_bytes(out.raw[48 * i:48 * i + 48], "big") for i in range(4)], tuple(nb)
    return call


def _hash_to_g2(hx, msg, dst, dst_len=None):  # noqa: F811
    o = ctypes.create_string_buffer(192)
    r = hx.hx_hash_to_g2(msg, dst, len(dst) if dst_len is None else dst_len, o)
    return r, o.raw


def test_h2f_every_dst_length(h2f):
    """hx_h2f (template build + expand_message_xmd_256 + hash_to_field_fp2x2) == the hashlib-based
    bls.hash_to_field_fp2 for every DST length 0 .. 255 on four messages, and the templates' block
    counts are those of the length's class."""
    for L in range(256):
        dst = hc.dst_for(L)
        for msg in hc.MESSAGES:
            r, got, nb = h2f(msg, dst)
            assert r == 0, L
            (a0, a1), (b0, b1) = bls.hash_to_field_fp2(msg, dst, 2)
            assert got == [a0, a1, b0, b1], (L, msg.hex())
            assert nb == hc.nb_of(L), (L, nb)


def test_class_table_covers_every_length():
    """NB_CLASSES restates the padding rule: ceil((36 + L + 9) / 64), ceil((34 + L + 9) / 64)."""
    for L in range(256):
        assert hc.nb_of(L) == ((36 + L + 9 + 63) // 64, (34 + L + 9 + 63) // 64)
    assert sorted({e for lo, hi, _ in hc.NB_CLASSES for e in (lo, hi)}) == hc.EDGE_LENGTHS


@pytest.mark.parametrize("L", hc.EDGE_LENGTHS)
def test_hash_to_g2_at_class_edges(hx, L):  # noqa: F811
    """hx_hash_to_g2 at both ends of every block-count class == the C oracle under that DST; at
    L = 0, 20, 212, 255 also == the Python oracle."""
    dst = hc.dst_for(L)
    for k, msg in enumerate(hc.MESSAGES):
        r, got = _hash_to_g2(hx, msg, dst)
        assert r == 0
        assert got == orc.hash_to_g2(msg, dst), (L, k)
        if L in (0, 20, 212, 255) and k == 3:
            assert got == bls.g2_serialize(bls.hash_to_g2(msg, dst)), L


def test_oversize_dst_refused(hx, h2f):  # noqa: F811
    """256 bytes, and a length of 2^32 + 43 over a 43-byte buffer (which a 32-bit cast would turn
    into the default DST's length), are refused; 255 is taken."""
    msg = hc.MESSAGES[2]
    assert _hash_to_g2(hx, msg, bytes(256))[0] == -1
    assert h2f(msg, bytes(256))[0] == -1
    assert _hash_to_g2(hx, msg, hc.DEFAULT_DST, 2 ** 32 + 43)[0] == -1
    assert h2f(msg, hc.DEFAULT_DST, 2 ** 32 + 43)[0] == -1
    assert h2f(msg, hc.DEFAULT_DST, 2 ** 32)[0] == -1
    assert _hash_to_g2(hx, msg, bytes(255))[0] == 0


def _map2(hx, vals):  # noqa: F811
    """hx_map2_to_g2 on four integers below 2^512 (u0.c0, u0.c1, u1.c0, u1.c1)."""
    hx.hx_map2_to_g2.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    hx.hx_map2_to_g2.restype = None
    o = ctypes.create_string_buffer(192)
    hx.hx_map2_to_g2(b"".join(v.to_bytes(64, "big") for v in vals), o)
    return o.raw


@pytest.mark.parametrize("case", sorted(hc.u_cases()))
def test_map2_to_g2_exceptional_inputs(hx, case):  # noqa: F811
    """The one-lane map2_to_g2 (SSWU, isogeny, add, cofactor clearing) == the oracle's
    iso_map_g2(map_to_curve_sswu(.)) added and cofactor-cleared; u1 = -u0 gives the identity."""
    u0, u1 = hc.u_cases()[case]
    want = hc.map2_refs()[case]
    assert (want is None) == (case == "f")
    assert _map2(hx, [u0[0], u0[1], u1[0], u1[1]]) == bls.g2_serialize(want)


def test_map2_to_g2_unreduced_field_input(hx):  # noqa: F811
    """The 64-byte field input as hash_to_field gets it: case (a) plus multiples of p up to the
    largest below 2^512 gives case (a)'s point, and 2^512 - 1, 2^384 and 2^384 - 1 reduce as the
    oracle's integers do."""
    u0, u1 = hc.u_cases()["a"]
    vals = [u0[0], u0[1], u1[0], u1[1]]
    top = [(2 ** 512 - 1 - v) // P for v in vals]
    want = bls.g2_serialize(hc.map2_refs()["a"])
    for ks in (top, [1, 2, 3, 4], [top[0], 1, (1 << 128) - 1, top[3] - 1]):
        big = [v + k * P for v, k in zip(vals, ks)]
        assert all(v < 2 ** 512 for v in big)
        assert _map2(hx, big) == want, ks
    assert top[0] * P + vals[0] + P >= 2 ** 512
    raw = [2 ** 512 - 1, 2 ** 384, 2 ** 384 - 1, 2 ** 512 - 1]
    r = [v % P for v in raw]
    assert _map2(hx, raw) == bls.g2_serialize(hc.map2_ref((r[0], r[1]), (r[2], r[3])))


# ------------------------------------------------------------------------------ VM programs
def _proj_aff(v):
    return gen._to_aff(bls, v)


def test_vm_simulator_against_oracle():
    """The programs' own hash_to_G2 (tools/fpvm/alg.py map_to_curve_sswu's select for u = 0, the
    doubling and the identity sum) in the simulator == the oracle: h2g's and qcpre's stored H on
    every case, h_inf = 1 exactly for the opposite pair in every program."""
    refs = hc.map2_refs()
    seen = set()
    for name, case, inp, r, sim in hc.vm_runs():
        seen.add((name, case))
        assert sim["h_inf"] == (1 if case == "f" else 0), (name, case)
        if name in ("h2g", "qcpre"):
            assert _proj_aff([sim["st:h%d" % k] for k in range(6)]) == refs[case], (name, case)
        if name in ("vote", "votew", "qcpre"):
            assert [sim[n] for n in ("sig_ok", "sig_grp")] == [1, 1], (name, case)
    assert seen == {("h2g", c) for c in hc.u_cases()} | {(n, c) for n in ("vote", "qcpre", "votew") for c in hc.VM_CASES}


def test_vote_program_pairs_with_oracle_H():
    """vote on (b) and (e): the stored f is Miller(r pk, H) for the oracle's H of those inputs
    (equal after the final exponentiation), so the exceptional H reaches the Miller loop whole."""
    g = load_golden()
    pk = bls.g1_from_bytes(bytes.fromhex(g["keys"][0]["pk"]))
    refs = hc.map2_refs()
    for name, case, inp, r, sim in hc.vm_runs():
        if name != "vote" or case == "f":
            continue
        f = progs.unflat12([sim["st:f%d" % j] for j in range(12)])
        rP = bls.pt_mul(bls.FpOps, pk, gen.alg.rlc_scalar(r))
        assert bls.f12_eq(bls.final_exponentiation_x_chain(f),
                          bls.final_exponentiation_x_chain(bls.miller_loop(rP, refs[case]))), case


@pytest.mark.parametrize("any_all", [0, 1])
def test_vm_programs_on_interpreter(hx, any_all):  # noqa: F811
    """The same runs through the interpreter's own code (fpvm.hpp exec, host build), each lane
    alone and with every wave-uniform block run for every lane == the simulator."""
    consts, progs_ = build_all()
    for name, case, inp, r, sim in hc.vm_runs():
        _, sc, words, _, _ = progs_[name]
        assert_same(run_vm(hx, consts, sc, words, inp, r, any_all), sim, "%s case %s" % (name, case))
