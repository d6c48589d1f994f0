"""Crafted G1 / G2 points for the decoders and the fast subgroup checks, with exact expectations
computed here on Python integers: an own square root (Fp by the (p + 1) / 4 power, Fp2 by the
norm method, each checked by squaring), the curve equation, and membership as [r]P == O by plain
affine double-and-add. Nothing of tools/fpvm/alg.py or the oracles is used for an expectation;
tests/test_point_cases.py cross-checks every case against oracle/py/bls12_381.py.

A case (Case) carries the encodings, the program inputs of the Fp-VM programs (x as the plain
value the prologue writes, and the sort flag), on_curve, the exact decoded y, in_group and its
class. Classes (G1_CLASSES / G2_CLASSES): off-curve x, both sort flags, y at the (p - 1) / 2 |
(p + 1) / 2 boundary of the ZCash "lexicographically largest" rule (x from a cube root of
y^2 - b), extreme x, x = 0, points of small prime order on the cofactor torsion and their sums
with subgroup points, and subgroup points; on G2 also x whose x^3 + b lies in Fp or in i Fp (a
square root with a zero component, or with y0 = +-y1).

cases() is generated once per process. lex_prog() is a small Fp-VM program that applies `lex` and
`sgn0` to raw representatives of (p - 1) / 2, (p + 1) / 2, 0, 1 and p - 1."""
import functools
import json
import os
from dataclasses import dataclass, field

P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R_ORD = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
X_ABS = 0xD201000000010000
XP = -X_ABS
H1 = (XP - 1) ** 2 // 3
H2 = (XP ** 8 - 4 * XP ** 7 + 5 * XP ** 6 - 4 * XP ** 4 + 6 * XP ** 3 - 4 * XP ** 2 - 4 * XP + 13) // 9
HALF = (P - 1) // 2          # lex_largest(y) <=> y > HALF
G1_ORDERS = (11, 10177, 859267, 52437899)
G2_ORDERS = (13, 23, 2713, 11953, 262069)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

G1_GEN = (0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB,
          0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1)
G2_GEN = ((0x024AA2B2F08F0A91260805272DC51051C6E47AD4FA403B02B4510B647AE3D1770BAC0326A805BBEFD48056C8C121BDB8,
           0x13E02B6052719F607DACD3A088274F65596BD0D09920B61AB5DA61BBDC7F5049334CF11213945D57E5AC7D055D042B7E),
          (0x0CE5D527727D6E118CC9CDC6DA2E351AADFD9BAA8CBDD3A76D429A695160D12C923AC9CC3BACA289E193548608B82801,
           0x0606C4A02EA734CC32ACD2B02BC28B99CB3E287E85A763AF267492AB572E99AB3F370D275CEC1DA1AAA9075FF05F79BE))


# ---------------------------------------------------------------------------------------- fields
class Fp:
    """Fp on ints."""
    zero, one, b = 0, 1, 4
    order = P

    @staticmethod
    def add(a, b):
        return (a + b) % P

    @staticmethod
    def sub(a, b):
        return (a - b) % P

    @staticmethod
    def mul(a, b):
        return a * b % P

    @staticmethod
    def inv(a):
        return pow(a, -1, P)

    @staticmethod
    def neg(a):
        return -a % P

    @staticmethod
    def sqrt(a):
        """A root of a, or None (p = 3 mod 4)."""
        s = pow(a, (P + 1) // 4, P)
        return s if s * s % P == a % P else None


class Fp2:
    """Fp[i] / (i^2 + 1) on pairs (c0, c1)."""
    zero, one, b = (0, 0), (1, 0), (4, 4)
    order = P * P

    @staticmethod
    def add(a, b):
        return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)

    @staticmethod
    def sub(a, b):
        return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)

    @staticmethod
    def mul(a, b):
        return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)

    @staticmethod
    def inv(a):
        n = pow(a[0] * a[0] + a[1] * a[1], -1, P)
        return (a[0] * n % P, -a[1] * n % P)

    @staticmethod
    def neg(a):
        return (-a[0] % P, -a[1] % P)

    @staticmethod
    def sqrt(a):
        """A root of a, or None. a1 = 0: (sqrt(a0), 0), or (0, sqrt(-a0)) as -1 is a non-residue;
        otherwise the norm method: n^2 = a0^2 + a1^2, x0^2 = (a0 +- n) / 2, x1 = a1 / (2 x0)."""
        a0, a1 = a[0] % P, a[1] % P
        if a1 == 0:
            s = Fp.sqrt(a0)
            if s is not None:
                return (s, 0)
            return (0, Fp.sqrt(-a0 % P))
        n = Fp.sqrt((a0 * a0 + a1 * a1) % P)
        if n is None:
            return None
        inv2 = (P + 1) // 2
        x0 = Fp.sqrt((a0 + n) * inv2 % P)
        if x0 is None:
            x0 = Fp.sqrt((a0 - n) * inv2 % P)
        r = (x0, a1 * pow(2 * x0, -1, P) % P)
        assert Fp2.mul(r, r) == (a0, a1)
        return r


def f_pow(F, a, e):
    r = F.one
    for bit in bin(e)[2:]:
        r = F.mul(r, r)
        if bit == "1":
            r = F.mul(r, a)
    return r


def rhs(F, x):
    """x^3 + b"""
    return F.add(F.mul(F.mul(x, x), x), F.b)


def cube_roots(F, c):
    """Every cube root of c in F. |F*| = 9 t with 3 not dividing t: w = c^(1/3 mod t) cubes to c
    times a cube root of unity, so one of the nine 9th roots of unity (they lie in Fp) times w is
    a root; each candidate is checked by cubing."""
    n = F.order - 1
    assert n % 9 == 0 and (n // 9) % 3
    t = n // 9
    w = f_pow(F, c, pow(3, -1, t))
    g = 2
    while pow(g, (P - 1) // 3, P) == 1:
        g += 1
    z = pow(g, (P - 1) // 9, P)   # a primitive 9th root of unity
    out = []
    for k in range(9):
        zk = pow(z, k, P)
        cand = w * zk % P if F is Fp else (w[0] * zk % P, w[1] * zk % P)
        if F.mul(F.mul(cand, cand), cand) == c and cand not in out:
            out.append(cand)
    return out


def lex_fp(y):
    return y > HALF


def lex_fp2(y):
    """ZCash: by c1, by c0 only when c1 = 0."""
    return lex_fp(y[1]) if y[1] else lex_fp(y[0])


# ---------------------------------------------------------------------------------------- points
def pt_add(F, A, B):
    """Affine chord-and-tangent; None is O."""
    if A is None:
        return B
    if B is None:
        return A
    (x1, y1), (x2, y2) = A, B
    if x1 == x2:
        if y1 != y2 or y1 == F.zero:
            return None
        xx = F.mul(x1, x1)
        lam = F.mul(F.add(F.add(xx, xx), xx), F.inv(F.add(y1, y1)))
    else:
        lam = F.mul(F.sub(y2, y1), F.inv(F.sub(x2, x1)))
    x3 = F.sub(F.sub(F.mul(lam, lam), x1), x2)
    return (x3, F.sub(F.mul(lam, F.sub(x1, x3)), y1))


def pt_neg(F, A):
    return None if A is None else (A[0], F.neg(A[1]))


def pt_mul(F, A, k):
    """[k]A, k >= 0, double-and-add from the top bit."""
    acc = None
    for bit in bin(k)[2:] if k else "":
        acc = pt_add(F, acc, acc)
        if bit == "1":
            acc = pt_add(F, acc, A)
    return acc


def on_curve(F, A):
    return F.mul(A[1], A[1]) == rhs(F, A[0])


def ladder_events(F, A, k=X_ABS):
    """[k]A by the ladder the subgroup checks run (acc = O; acc = 2 acc, then acc += A at a set
    bit): the additions whose accumulator is O, A or -A just before them, as (bit, kind) with bit
    counted from 1 at the top. The first addition (bit 1, O + A) is every ladder's and is left
    out. -> (events, [k]A)"""
    acc, ev = None, []
    for n, bit in enumerate(bin(k)[2:], 1):
        acc = pt_add(F, acc, acc)
        if bit == "1":
            if n > 1:
                if acc is None:
                    ev.append((n, "O"))
                elif acc == A:
                    ev.append((n, "Q"))
                elif acc == pt_neg(F, A):
                    ev.append((n, "-Q"))
            acc = pt_add(F, acc, A)
    return ev, acc


def small_order_point(F, ell, start):
    """A point of order exactly ell on E(F): the first on-curve x at or after `start`, times the
    curve order without its ell-part, then times ell while that is not O yet."""
    h = H1 if F is Fp else H2
    assert h % ell == 0
    cof = h
    while cof % ell == 0:
        cof //= ell
    x = start
    while True:
        y = F.sqrt(rhs(F, x))
        if y is not None:
            T = pt_mul(F, (x, y), cof * R_ORD)
            if T is not None:
                while True:
                    N = pt_mul(F, T, ell)
                    if N is None:
                        return T
                    T = N
        x = (x + 1) % P if F is Fp else ((x[0] + 1) % P, x[1])


# ---------------------------------------------------------------------------------------- cases
@dataclass
class Case:
    group: int              # 1 or 2
    cls: str
    name: str
    x: object               # int (G1) or (c0, c1) (G2); may be >= p for the rejected encodings
    sort: int
    on_curve: bool
    y: object               # the decoded y for this sort flag (None off the curve)
    in_group: bool
    parse: int              # the decoder's code for `enc`: 0, 1 bad encoding, 2 off-curve, 3 x = 0
    enc: bytes              # compressed
    unc: bytes = None       # uncompressed, where the point exists
    program: bool = True    # x < p: the Fp-VM programs take (x, sort) as inputs
    events: list = field(default_factory=list)   # ladder_events (G1: of both |x| ladders)
    xabs: object = None     # [|x|] of the point, None for O (on-curve cases)

    @property
    def point(self):
        return (self.x, self.y) if self.on_curve else None

    def inputs(self):
        """Program inputs as sched.simulate takes them (canonical values; run_vm stores x R, so
        x R^-1 here puts the plain x in the slot, as the vote prologue does)."""
        rinv = pow(1 << 384, -1, P)
        if self.group == 1:
            return {"pk_x": self.x * rinv % P, "pk_sort": self.sort}
        return {"sig_x0": self.x[0] * rinv % P, "sig_x1": self.x[1] * rinv % P, "sig_sort": self.sort}

    def code(self):
        """What the C ABI answers for this key (its parse failures are the trait's 102) or
        signature when the rest of the vote is valid."""
        if self.group == 1:
            return 102 if self.parse else (0 if self.in_group else 3)
        return self.parse if self.parse else (0 if self.in_group else 3)


def _i2b(v, n=48):
    return int(v).to_bytes(n, "big")


def enc_g1(x, sort):
    b = bytearray(_i2b(x))
    assert not b[0] & 0xE0
    b[0] |= 0x80 | (0x20 if sort else 0)
    return bytes(b)


def enc_g2(x, sort):
    b = bytearray(_i2b(x[1]) + _i2b(x[0]))
    assert not b[0] & 0xE0
    b[0] |= 0x80 | (0x20 if sort else 0)
    return bytes(b)


def ser_g1(A):
    return _i2b(A[0]) + _i2b(A[1])


def ser_g2(A):
    return _i2b(A[0][1]) + _i2b(A[0][0]) + _i2b(A[1][1]) + _i2b(A[1][0])


def _in_group(F, A):
    return pt_mul(F, A, R_ORD) is None


def _g1_events(A):
    """-> (events of [|x|]A and of [|x|]([|x|]A), [|x|]A)"""
    e1, t = ladder_events(Fp, A)
    e2 = ladder_events(Fp, t)[0] if t is not None else [(0, "base O")]
    return [(1,) + e for e in e1] + [(2,) + e for e in e2], t


def g1_case(cls, name, x, sort):
    """The G1 case of the compressed encoding (x, sort), everything computed here."""
    if x >= P:
        return Case(1, cls, name, x, sort, False, None, False, 1, enc_g1(x, sort), program=False)
    y = Fp.sqrt(rhs(Fp, x))
    if y is None:
        return Case(1, cls, name, x, sort, False, None, False, 2, enc_g1(x, sort))
    if lex_fp(y) != bool(sort):
        y = P - y
    assert on_curve(Fp, (x, y)) and lex_fp(y) == bool(sort)
    A = (x, y)
    ev, t = _g1_events(A)
    return Case(1, cls, name, x, sort, True, y, _in_group(Fp, A), 3 if x == 0 else 0, enc_g1(x, sort),
                unc=ser_g1(A), events=ev, xabs=t)


def g2_case(cls, name, x, sort):
    if max(x) >= P:
        return Case(2, cls, name, x, sort, False, None, False, 1, enc_g2(x, sort), program=False)
    y = Fp2.sqrt(rhs(Fp2, x))
    if y is None:
        return Case(2, cls, name, x, sort, False, None, False, 2, enc_g2(x, sort))
    if lex_fp2(y) != bool(sort):
        y = Fp2.neg(y)
    assert on_curve(Fp2, (x, y)) and lex_fp2(y) == bool(sort)
    A = (x, y)
    ev, t = ladder_events(Fp2, A)
    return Case(2, cls, name, x, sort, True, y, _in_group(Fp2, A), 0, enc_g2(x, sort),
                unc=ser_g2(A), events=ev, xabs=t)


def _of_point(group, cls, name, A):
    """The case of an on-curve point: its own sort flag."""
    if group == 1:
        c = g1_case(cls, name, A[0], int(lex_fp(A[1])))
    else:
        c = g2_case(cls, name, A[0], int(lex_fp2(A[1])))
    assert c.y == A[1], name
    return c


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "golden_v1.json")) as fh:
        return json.load(fh)


def _x_of(b):
    return int.from_bytes(bytes([b[0] & 0x1F]) + b[1:48], "big")


def _golden_points(g, n=2):
    """The first n golden keys and signatures as points: x and the sort flag from the encoding, y
    by this module's root."""
    keys, sigs = [], []
    for k in g["keys"][:n]:
        b = bytes.fromhex(k["pk"])
        c = g1_case("", "", _x_of(b), (b[0] >> 5) & 1)
        keys.append(c.point)
    for v in g["votes"][:n]:
        b = bytes.fromhex(v["sig"])
        c = g2_case("", "", (int.from_bytes(b[48:96], "big"), _x_of(b)), (b[0] >> 5) & 1)
        sigs.append(c.point)
    return keys, sigs


def _g1_cases(gold_keys):
    out = []
    # off-curve, and an on-curve x with each flag
    x = 0x0FACE
    while Fp.sqrt(rhs(Fp, x)) is not None:
        x += 1
    out += [g1_case("off_curve", "x=%#x s%d" % (x, s), x, s) for s in (0, 1)]
    x = 0x0C0DE
    while Fp.sqrt(rhs(Fp, x)) is None:
        x += 1
    pair = [g1_case("both_flags", "x=%#x s%d" % (x, s), x, s) for s in (0, 1)]
    assert pair[0].y + pair[1].y == P and not lex_fp(pair[0].y) and lex_fp(pair[1].y)
    out += pair
    # y at the boundary of the lex rule: y^2 - 4 a cube
    for side, y0, step in (("below", HALF, -1), ("above", HALF + 1, 1)):
        k = 0
        while True:
            y = y0 + step * k
            roots = cube_roots(Fp, (y * y - 4) % P)
            if roots:
                break
            k += 1
        x = min(roots)
        for s in (0, 1):
            c = g1_case("lex_boundary", "%s offset %d s%d" % (side, k, s), x, s)
            assert c.y == (y if s == int(lex_fp(y)) else P - y)
            out.append(c)
    # extreme x
    for nm, x0, step in (("p-1", P - 1, -1), ("1", 1, 1)):
        out.append(g1_case("extreme_x", "x=%s s0" % nm, x0, 0))
        x = x0
        while Fp.sqrt(rhs(Fp, x)) is None:
            x += step
        out += [g1_case("extreme_x", "on-curve x nearest %s (%+d) s%d" % (nm, x - x0, s), x, s) for s in (0, 1)]
    out.append(g1_case("x_ge_p", "x=p", P, 0))
    out.append(g1_case("x_ge_p", "x=2^381-1", (1 << 381) - 1, 1))
    # the order-3 points (0, +-2)
    zero = [g1_case("x_zero", "x=0 s%d" % s, 0, s) for s in (0, 1)]
    assert [c.y for c in zero] == [2, P - 2] and not zero[0].in_group
    assert pt_mul(Fp, zero[0].point, 3) is None
    out += zero
    # small orders on the cofactor torsion, and their sums with subgroup points
    for k, ell in enumerate(G1_ORDERS):
        T = small_order_point(Fp, ell, 5 + 16 * k)
        assert T is not None and pt_mul(Fp, T, ell) is None
        out.append(_of_point(1, "small_order", "order %d" % ell, T))
        out.append(_of_point(1, "small_order", "order %d + G1" % ell, pt_add(Fp, T, G1_GEN)))
        out.append(_of_point(1, "small_order", "order %d + golden key" % ell, pt_add(Fp, T, gold_keys[k % len(gold_keys)])))
    assert not any(c.in_group for c in out if c.cls == "small_order")
    # the subgroup
    for k, A in enumerate(gold_keys):
        out.append(_of_point(1, "in_group", "golden key %d" % k, A))
    out.append(_of_point(1, "in_group", "G1", G1_GEN))
    out.append(_of_point(1, "in_group", "-G1", pt_neg(Fp, G1_GEN)))
    out.append(_of_point(1, "in_group", "[r-1]G1", pt_mul(Fp, G1_GEN, R_ORD - 1)))
    assert all(c.in_group for c in out if c.cls == "in_group")
    return out


def _g2_cases(gold_sigs):
    out = []
    out += [g2_case("off_curve", "x=0 s%d" % s, (0, 0), s) for s in (0, 1)]
    assert not out[0].on_curve   # 4 + 4i is no square
    x = (0xBEEF, 0xF00D)
    while Fp2.sqrt(rhs(Fp2, x)) is not None:
        x = (x[0] + 1, x[1])
    out.append(g2_case("off_curve", "x=(%#x,%#x) s1" % x, x, 1))
    out.append(g2_case("x_ge_p", "x0=p", (P, 1), 0))
    out.append(g2_case("x_ge_p", "x1=p", (1, P), 1))
    # rhs in Fp: a^2 = (b^3 - 4) / (3 b) clears the imaginary part; y = (s, 0) or (0, s)
    kinds = {"y=(s,0)": 0, "y=(0,s)": 0}
    b = 1
    while min(kinds.values()) < 2:
        a = Fp.sqrt((b ** 3 - 4) * pow(3 * b, -1, P) % P)
        if a is not None:
            x = (a, b)
            assert rhs(Fp2, x)[1] == 0
            c0 = g2_case("rhs_in_fp", "", x, 0)
            kind = "y=(s,0)" if c0.y[1] == 0 else "y=(0,s)"
            assert c0.y[0] == 0 or c0.y[1] == 0
            if kinds[kind] < 2:
                kinds[kind] += 1
                out += [g2_case("rhs_in_fp", "b=%d %s s%d" % (b, kind, s), x, s) for s in (0, 1)]
        b += 1
    # rhs in i Fp: c^2 = (a^3 + 4) / (3 a) clears the real part; y0 = +-y1
    a, found = 1, 0
    while found < 3:
        c = Fp.sqrt((a ** 3 + 4) * pow(3 * a, -1, P) % P)
        if c is not None:
            x = (a, c)
            assert rhs(Fp2, x)[0] == 0
            cs = [g2_case("rhs_in_ifp", "a=%d s%d" % (a, s), x, s) for s in (0, 1)]
            assert cs[0].y[0] in (cs[0].y[1], P - cs[0].y[1])
            out += cs
            found += 1
        a += 1
    # y at the boundaries of the lex rule: y^2 - (4 + 4i) a cube
    def boundary(name, make):
        k = 0
        while True:
            y = make(k)
            roots = cube_roots(Fp2, Fp2.sub(Fp2.mul(y, y), Fp2.b))
            if roots:
                break
            k += 1
        x = min(roots, key=lambda r: (r[1], r[0]))
        for s in (0, 1):
            c = g2_case("lex_boundary", "%s offset %d s%d" % (name, k, s), x, s)
            assert c.y == (y if s == int(lex_fp2(y)) else Fp2.neg(y))
            out.append(c)
    boundary("c1 below (p-1)/2, c0=7", lambda k: (7, HALF - k))
    boundary("c1 above (p+1)/2, c0=7", lambda k: (7, HALF + 1 + k))
    boundary("c1=0, c0 below (p-1)/2", lambda k: (HALF - k, 0))
    boundary("c1=0, c0 above (p+1)/2", lambda k: (HALF + 1 + k, 0))
    boundary("c0=0, c1 small", lambda k: (0, 1 + k))
    boundary("c1 near p-1, c0=7", lambda k: (7, P - 1 - k))
    # small orders on the cofactor torsion
    for k, ell in enumerate(G2_ORDERS):
        T = small_order_point(Fp2, ell, (3 + 16 * k, 1))
        assert T is not None and pt_mul(Fp2, T, ell) is None
        out.append(_of_point(2, "small_order", "order %d" % ell, T))
        out.append(_of_point(2, "small_order", "order %d + G2" % ell, pt_add(Fp2, T, G2_GEN)))
        out.append(_of_point(2, "small_order", "order %d + golden signature" % ell,
                             pt_add(Fp2, T, gold_sigs[k % len(gold_sigs)])))
    small = [c for c in out if c.cls == "small_order"]
    assert not any(c.in_group for c in small)
    assert any(kind == "O" for c in small for _, kind in c.events), "no G2 case adds Q to O"
    for k, A in enumerate(gold_sigs):
        out.append(_of_point(2, "in_group", "golden signature %d" % k, A))
    out.append(_of_point(2, "in_group", "G2", G2_GEN))
    out.append(_of_point(2, "in_group", "-G2", pt_neg(Fp2, G2_GEN)))
    assert all(c.in_group for c in out if c.cls == "in_group")
    return out


G1_CLASSES = ("off_curve", "both_flags", "lex_boundary", "extreme_x", "x_ge_p", "x_zero", "small_order", "in_group")
G2_CLASSES = ("off_curve", "x_ge_p", "rhs_in_fp", "rhs_in_ifp", "lex_boundary", "small_order", "in_group")


@functools.lru_cache(maxsize=None)
def cases():
    """-> (G1 cases, G2 cases), generated once per process."""
    assert on_curve(Fp, G1_GEN) and on_curve(Fp2, G2_GEN)
    keys, sigs = _golden_points(_golden())
    g1, g2 = _g1_cases(keys), _g2_cases(sigs)
    for cs, classes in ((g1, G1_CLASSES), (g2, G2_CLASSES)):
        for cl in classes:
            assert any(c.cls == cl for c in cs), "class %s is empty" % cl
        assert {c.cls for c in cs} == set(classes)
    return tuple(g1), tuple(g2)


def by_class(cs, classes):
    return {cl: [c for c in cs if c.cls == cl] for cl in classes}


def subset(cs, limit=10):
    """One case per class that the programs can take (x < p), at most `limit`: the first of each
    class, preferring a case whose ladder meets O, Q or -Q."""
    out = []
    for cl in dict.fromkeys(c.cls for c in cs):
        group = [c for c in cs if c.cls == cl and c.program]
        if group:
            out.append(next((c for c in group if c.events), group[0]))
    assert len(out) <= limit
    return out


# ---------------------------------------------------------------------------------------- lex / sgn0
LEX_VALUES = (("half", HALF), ("half1", HALF + 1), ("zero", 0), ("one", 1), ("pm1", P - 1))


def lex_raw_inputs():
    """{input name: raw slot limbs}: each value's Montgomery representative m, and m + p where
    that is below 2p (always: m < p)."""
    r = (1 << 384) % P
    raw = {}
    for name, v in LEX_VALUES:
        m = v * r % P
        raw[name] = m
        assert m + P < 2 * P
        raw[name + "_p"] = m + P
    return raw


def lex_expected():
    """{output name: 0 / 1} from the integers."""
    out = {}
    for name, v in LEX_VALUES:
        for sfx in ("", "_p"):
            out["lex_" + name + sfx] = int(v > HALF)
            out["sgn_" + name + sfx] = v & 1
    return out


@functools.lru_cache(maxsize=None)
def lex_prog():
    """-> (consts, prog, sc, words): lex and sgn0 of every raw input, built the way
    tests/vm_edge.py builds its program."""
    from vm_helpers import gen, sched
    import ir
    consts = sched.ConstTable()
    consts.ref(1, True)
    assert consts.ref(0, False) - sched.CONST_BASE == gen.KZERO
    for n in range(5):
        assert consts.ref(n * (2 * P + 1), True) - sched.CONST_BASE == gen.KTAB + n
    pr = ir.Prog("lexedge")
    for name in lex_raw_inputs():
        v = pr.input(name)
        pr.output("lex_" + name, pr.lex(v))
        pr.output("sgn_" + name, pr.sgn0(v))
    sc = sched.schedule(pr, 16, consts, max_slots=128)
    return consts, pr, sc, sched.encode(sc)


def lex_canon_inputs():
    rinv = pow(1 << 384, -1, P)
    return {n: x * rinv % P for n, x in lex_raw_inputs().items()}
