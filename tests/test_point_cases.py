"""The crafted G1 / G2 points of tests/point_cases.py (expectations from plain integers: own
square root, curve equation, [r]P) against the Python oracle and against the host build of the
one-lane device code (consensus_overlord_amd/csrc/bls/ec.hpp through tests/host/harness.cpp:
g*_from_bytes, fp2_sqrt, fp*_lex_largest, g*_in_subgroup on jac_add / jac_dbl, verify_one).
All comparisons are exact integers or bytes."""
import ctypes

import bls12_381 as bls
import orc
import point_cases as pc
from test_host_harness import hx  # noqa: F401  (module fixture: builds libhx.so)


def _all():
    g1, g2 = pc.cases()
    return list(g1) + list(g2)


def _oracle_decode(c):
    """-> (code, point) of the oracle's compressed decoder"""
    try:
        return 0, (bls._g1_uncompress if c.group == 1 else bls._g2_uncompress)(c.enc)
    except bls.BlstError as e:
        return e.code, None


def test_classes_present():
    g1, g2 = pc.cases()
    for cs, classes in ((g1, pc.G1_CLASSES), (g2, pc.G2_CLASSES)):
        per = pc.by_class(cs, classes)
        assert all(per[cl] for cl in classes), {cl: len(v) for cl, v in per.items()}
    per1, per2 = pc.by_class(g1, pc.G1_CLASSES), pc.by_class(g2, pc.G2_CLASSES)
    # what each class is for
    assert {c.sort for c in per1["both_flags"]} == {0, 1}
    ys = [c.y for c in per1["lex_boundary"]]
    assert any(0 <= pc.HALF - y < 64 for y in ys) and any(0 < y - pc.HALF < 64 for y in ys)
    assert any(c.x == pc.P - 1 for c in per1["extreme_x"]) and any(c.x == 1 for c in per1["extreme_x"])
    assert {c.x for c in per1["x_ge_p"]} == {pc.P, 2 ** 381 - 1}
    assert sorted(c.y for c in per1["x_zero"]) == [2, pc.P - 2]
    assert any(c.on_curve and c.y[1] == 0 for c in per2["rhs_in_fp"])       # the f2_lex fallback
    assert any(c.on_curve and c.y[0] == 0 for c in per2["rhs_in_fp"])
    assert sum(1 for c in per2["rhs_in_fp"] if c.y[1] == 0) >= 4 and sum(1 for c in per2["rhs_in_fp"] if c.y[0] == 0) >= 4
    assert all(c.y[0] in (c.y[1], pc.P - c.y[1]) for c in per2["rhs_in_ifp"])
    ys = [c.y for c in per2["lex_boundary"]]
    assert any(y[1] == 0 and abs(y[0] - pc.HALF) < 64 for y in ys)
    assert any(y[1] and abs(y[1] - pc.HALF) < 64 and y[1] <= pc.HALF for y in ys)
    assert any(y[1] and abs(y[1] - pc.HALF) < 64 and y[1] > pc.HALF for y in ys)
    assert any(y[0] == 0 and 0 < y[1] < 64 for y in ys) and any(pc.P - y[1] < 64 for y in ys)
    for cs, orders in ((per1["small_order"], pc.G1_ORDERS), (per2["small_order"], pc.G2_ORDERS)):
        F = bls.FpOps if cs[0].group == 1 else bls.Fp2Ops
        found = {ell for ell in orders for c in cs if bls.pt_mul(F, c.point, ell) is None}
        assert found == set(orders)
    # the ladder by |x| adds Q to O on G2 (order 13, at bit 7), and meets O, Q and -Q on G1
    assert (7, "O") in next(c for c in per2["small_order"] if c.name == "order 13").events
    assert {e[-1] for c in g1 for e in c.events} >= {"O", "Q", "-Q"}


def test_cases_equal_python_oracle():
    """on_curve, the decoded y and in_group against _g*_uncompress, [r]P and the fast checks."""
    for c in _all():
        F = bls.FpOps if c.group == 1 else bls.Fp2Ops
        code, pt = _oracle_decode(c)
        assert code == c.parse, (c.name, code)
        assert (code != 2) == (c.on_curve or c.parse == 1), c.name
        if code == 0:
            assert pt == c.point, c.name
        if c.on_curve:
            A = c.point
            assert bls.on_curve(F, A), c.name
            slow = (bls.g1_in_subgroup if c.group == 1 else bls.g2_in_subgroup)(A)
            fast = (bls.g1_in_subgroup_fast if c.group == 1 else bls.g2_in_subgroup_fast)(A)
            assert slow == fast == c.in_group, (c.name, slow, fast)
            if c.group == 1:
                assert c.unc == bls.g1_serialize(A) and bls.g1_compress(A) == c.enc, c.name
                assert bls.fp_lex_largest(c.y) == bool(c.sort), c.name
            else:
                assert c.unc == bls.g2_serialize(A) and bls.g2_compress(A) == c.enc, c.name
                assert bls.f2_lex_largest(c.y) == bool(c.sort), c.name
        elif c.program:
            # off the curve by the oracle's own root too
            x = c.x
            if c.group == 1:
                assert bls.fp_sqrt((x ** 3 + 4) % pc.P) is None, c.name
            else:
                assert bls.f2_sqrt(bls.f2_add(bls.f2_mul(bls.f2_sqr(x), x), bls.B2)) is None, c.name


def _replay(F, A, k=pc.X_ABS):
    """ladder_events with the oracle's Jacobian arithmetic"""
    acc, base, ev = (F.one, F.one, F.zero), bls._jac_from_aff(F, A), []
    for n, bit in enumerate(bin(k)[2:], 1):
        acc = bls._jac_dbl(F, acc)
        if bit == "1":
            aff = bls._jac_to_aff(F, acc)
            if n > 1:
                if aff is None:
                    ev.append((n, "O"))
                elif bls.pt_eq(F, aff, A):
                    ev.append((n, "Q"))
                elif bls.pt_eq(F, aff, bls.pt_neg(F, A)):
                    ev.append((n, "-Q"))
            acc = bls._jac_add(F, acc, base)
    return ev, bls._jac_to_aff(F, acc)


def test_ladder_events_match_replay():
    for c in _all():
        if not c.on_curve:
            assert c.events == []
            continue
        if c.group == 2:
            ev, t = _replay(bls.Fp2Ops, c.point)
            assert c.events == ev and c.xabs == t, c.name
        else:
            e1, t = _replay(bls.FpOps, c.point)
            assert t is not None and t == c.xabs
            e2 = _replay(bls.FpOps, t)[0]
            assert c.events == [(1,) + e for e in e1] + [(2,) + e for e in e2], c.name


def _decode(hx, c, data):  # noqa: F811
    """hx_g*_decode and hx_g*_decode_xy on `data` -> (code, compressed bytes, coordinates)"""
    n = 48 * c.group
    comp, xy, inf = ctypes.create_string_buffer(n), ctypes.create_string_buffer(2 * n), ctypes.c_int(0)
    dec, dxy = (hx.hx_g1_decode, hx.hx_g1_decode_xy) if c.group == 1 else (hx.hx_g2_decode, hx.hx_g2_decode_xy)
    e = dec(data, len(data), comp, ctypes.byref(inf))
    assert dxy(data, len(data), xy, ctypes.byref(inf)) == e and inf.value == 0
    return e, comp.raw, xy.raw


def test_host_decoders_and_subgroup_checks(hx):  # noqa: F811
    """g*_from_bytes on the compressed and the uncompressed encoding: the expected code and the
    exact x and y (not only a point that compresses back: the sign rule is used by both
    directions); g*_in_subgroup == [r]P == O, through the decoder and, for x = 0, past it."""
    sub = {1: hx.hx_g1_subgroup, 2: hx.hx_g2_subgroup}
    sub_xy = {1: hx.hx_g1_subgroup_xy, 2: hx.hx_g2_subgroup_xy}
    for c in _all():
        e, comp, xy = _decode(hx, c, c.enc)
        assert e == c.parse, (c.name, e)
        if c.on_curve:
            assert xy == c.unc, c.name
        if e == 0:
            assert comp == c.enc, c.name
            assert sub[c.group](c.enc, len(c.enc)) == int(c.in_group), c.name
        else:
            assert sub[c.group](c.enc, len(c.enc)) == -e, c.name
        if c.unc is not None:
            e, comp, xy = _decode(hx, c, c.unc)
            assert e == c.parse and xy == c.unc, (c.name, e)
            if e == 0:
                assert comp == c.enc, c.name
                assert sub[c.group](c.unc, len(c.unc)) == int(c.in_group), c.name
            assert sub_xy[c.group](c.unc) == int(c.in_group), c.name
            # the ladder's exact result: a wrong special case of jac_add leaves most verdicts
            # "outside the group" as they were, but not [|x|]P
            out = ctypes.create_string_buffer(len(c.unc))
            r = (hx.hx_g1_mul_xabs_xy if c.group == 1 else hx.hx_g2_mul_xabs_xy)(c.unc, out)
            assert r == (1 if c.xabs is None else 0), c.name
            if c.xabs is not None:
                assert out.raw == (pc.ser_g1 if c.group == 1 else pc.ser_g2)(c.xabs), c.name
            # a set sort flag on an uncompressed encoding is refused
            bad = bytes([c.unc[0] | 0x20]) + c.unc[1:]
            assert _decode(hx, c, bad)[0] == 1, c.name


def test_host_verify_with_crafted_key_or_signature(hx, golden):  # noqa: F811
    """verify_one (host build) == the C oracle == the class's code when a crafted key or signature
    replaces one side of a golden vote, in both encodings."""
    v, k = golden["votes"][0], golden["keys"][0]
    sig, h, pk = bytes.fromhex(v["sig"]), bytes.fromhex(v["digest"]), bytes.fromhex(k["pk"])
    assert orc.verify(sig, h, pk) == 0
    seen = set()
    for c in _all():
        for data in (c.enc, c.unc):
            if data is None:
                continue
            s, p = (sig, data) if c.group == 1 else (data, pk)
            want = orc.verify(s, h, p)
            if c.code():
                assert want == c.code(), (c.name, want)
            else:
                assert want == (0 if data in (sig, pk) or c.point in (bls.g1_from_bytes(pk), bls.g2_from_bytes(sig))
                                else 5), (c.name, want)
            assert hx.hx_verify(s, len(s), h, len(h), p, len(p)) == want, (c.name, want)
            seen.add(want)
    assert seen >= {0, 1, 2, 3, 5, 102}
