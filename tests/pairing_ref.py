"""An exact reference for the pairing tail in plain integers, independent of the tower code it
checks (tools/fpvm/alg.py, csrc/bls/tower.hpp, oracle/py/bls12_381.py): Fp12 as the polynomial
ring Fp[w] / (w^12 - 2 w^6 + 2). With u = w^6 - 1 (u^2 = -1), v = w^2 and xi = 1 + u = w^6 (v^3 = xi,
w^2 = v) this is the field the project's tower Fp2[v] / (v^3 - xi) [w] / (w^2 - v) builds.

Nothing here uses a Karatsuba step, a Frobenius constant or an addition chain: `mul` is the
schoolbook product with the reduction w^12 = 2 w^6 - 2, `pow` is square-and-multiply, the inverse
is a^(p^12 - 2), Frobenius is a^p, conjugation is a^(p^6) and the final exponentiation is the
power by the plain exponent 3 (p^12 - 1) / r. A tower element is ((a0, a1, a2), (b0, b1, b2)) of
Fp2 pairs (the layout of progs.flat12); a polynomial is a tuple of 12 integers below p, lowest
degree first. Powers are kept per process (one takes a few tenths of a second)."""
import functools

P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
X_ABS = 0xD201000000010000
assert (P ** 12 - 1) % R == 0
FE_EXP = 3 * (P ** 12 - 1) // R                 # what the x-chain computes
EASY_EXP = (P ** 6 - 1) * (P ** 2 + 1)
ONE = (1,) + (0,) * 11
ZERO = (0,) * 12


def to_poly(t):
    """tower -> polynomial: coefficient (c0, c1) = c0 + c1 u of v^k w^h is c0 - c1 at w^(2k+h)
    and c1 at w^(2k+h+6)"""
    out = [0] * 12
    for h in range(2):
        for k in range(3):
            c0, c1 = t[h][k]
            out[2 * k + h] = (c0 - c1) % P
            out[2 * k + h + 6] = c1 % P
    return tuple(out)


def from_poly(a):
    return tuple(tuple(((a[2 * k + h] + a[2 * k + h + 6]) % P, a[2 * k + h + 6] % P) for k in range(3))
                 for h in range(2))


def flat(t):
    """tower -> its 12 Fp coefficients in the order of progs.flat12"""
    return [c for f6 in t for f2 in f6 for c in f2]


def unflat(v):
    v = [x % P for x in v]
    return ((tuple(v[0:2]), tuple(v[2:4]), tuple(v[4:6])), (tuple(v[6:8]), tuple(v[8:10]), tuple(v[10:12])))


def mul(a, b):
    acc = [0] * 23
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                acc[i + j] += x * y
    for d in range(22, 11, -1):                 # w^d = 2 w^(d-6) - 2 w^(d-12)
        c = acc[d]
        acc[d - 6] += 2 * c
        acc[d - 12] -= 2 * c
    return tuple(x % P for x in acc[:12])


@functools.lru_cache(maxsize=None)
def pow(a, e):  # noqa: A001  (the issue's name for it)
    assert e >= 0
    r = ONE
    for bit in bin(e)[2:]:
        r = mul(r, r)
        if bit == "1":
            r = mul(r, a)
    return r


def inv(a):
    """a^(p^12 - 2); 0 for 0 (what the interpreter's inv op gives)"""
    return pow(a, P ** 12 - 2)


def frob(a):
    return pow(a, P)


def conj(a):
    return pow(a, P ** 6)


def final_exp(a):
    return pow(a, FE_EXP)


def easy_part(a):
    return pow(a, EASY_EXP)


def exp_x(a):
    """a^x, x = -|x|, for a in the cyclotomic subgroup: the plain power by |x|, then the conjugate"""
    return conj(pow(a, X_ABS))


def mul_t(a, b):
    return from_poly(mul(to_poly(a), to_poly(b)))


def final_exp_t(t):
    return from_poly(final_exp(to_poly(t)))


def line_t(l0, l1, l4):
    """the sparse element l0 + l1 v + l4 v w of f12_mul_014"""
    z = (0, 0)
    return ((l0, l1, z), (z, l4, z))
