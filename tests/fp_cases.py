"""Operands and exact expected values for the unit-level tests of the gfx950 field arithmetic
(tests/test_fp_bounds_host.py on the host build, tests/test_gpu_fp_bounds.py on the device):
plain Python integers, no GPU, no ctypes. Every table is chosen where the representation can
break (limb boundaries of the 14 x 28-bit product, the top of the permitted operand ranges, sums
that sit one above or below a multiple of p), plus seeded random values.

Ranges are the contracts written in csrc/fpvm.hpp and csrc/bls/fp_mul28.hpp: product operands in
[0, 4p), slot values in [0, 2p), linear coefficients |c| <= 15."""
import functools
import itertools
import random

import numpy as np

P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R = 1 << 384
RINV = pow(R, -1, P)
M28 = (1 << 28) - 1

# fpvm.hpp: constant-table entries the primitives read, and the unit-lin header bits
KZERO, KTAB = 1, 2
H_LINNEG, H_LINNEG2, H_LINNEG3 = 1 << 26, 1 << 30, 1 << 31


def words(v, n=12):
    assert 0 <= v < 1 << (32 * n), hex(v)
    return [(v >> (32 * k)) & 0xFFFFFFFF for k in range(n)]


def pack(vals):
    """list of integers -> (n, 12) uint32 array"""
    return np.array([words(v) for v in vals], dtype=np.uint32).reshape(len(vals), 12)


def unpack(arr):
    return [sum(int(w) << (32 * k) for k, w in enumerate(row)) for row in np.asarray(arr).reshape(-1, 12)]


def const_table():
    """The fixed head of the interpreter's constant table (tools/fpvm/gen.py build_all): entry 0
    the plain 1, KZERO the zero, KTAB + n = n (2p + 1) as raw limbs for n = 0..4."""
    return pack([1, 0] + [n * (2 * P + 1) for n in range(5)])


# ------------------------------------------------------------------------------ products
@functools.lru_cache(maxsize=None)
def product_edges():
    e = [0, 1, 2, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, 3 * P, 4 * P - 2, 4 * P - 1,
         2 ** 381 - 1, 2 ** 381, 2 ** 382 - 1, 2 ** 382, R % P, R * R % P, (2 ** 392 - 1) % (4 * P)]
    e += [(4 * P - 1) & ~(M28 << (28 * k)) for k in range(14)]
    e += [M28 << (28 * k) for k in range(13)]
    e += [0xFFFFFFFF << (32 * k) for k in range(11)]
    out = []
    for v in e:
        if v < 4 * P and v not in out:
            out.append(v)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def product_cases():
    """(a, b) pairs: the full cross product of the edges, 4,096 seeded pairs below 4p and 1,024
    below p."""
    e = product_edges()
    rng = random.Random(0xF9A5)
    cases = list(itertools.product(e, e))
    cases += [(rng.randrange(4 * P), rng.randrange(4 * P)) for _ in range(4096)]
    cases += [(rng.randrange(P), rng.randrange(P)) for _ in range(1024)]
    return tuple(cases)


def square_cases():
    """Every edge squared (the device test passes one register array for both operands)."""
    return tuple((e, e) for e in product_edges())


PINV392 = pow(-P, -1, 1 << 392)


def mont28(a, b):
    """The exact result of the three 28-bit forms: Montgomery reduction of (a 2^8) b with
    R = 2^392, then one conditional subtraction."""
    x = (a << 8) * b
    m = x * PINV392 % (1 << 392)
    t, rem = divmod(x + m * P, 1 << 392)
    assert rem == 0
    return t - P if t >= P else t


def product_bound(a, b):
    """r < max(p, ceil(a b / 2^384)): from T < a b / 2^384 + p and one conditional subtraction
    (holds for any Montgomery radix, so for the 12 x 32 forms too)."""
    return max(P, -(-(a * b) // R))


def check_product(a, b, r, exact):
    """-> None or a message. exact: limbs equal mont28 (the 28-bit forms); the congruence and
    the derived bound are required of every form."""
    if exact:
        want = mont28(a, b)
        assert want % P == a * b * RINV % P and want < product_bound(a, b)
        if r != want:
            return "a=%x b=%x: got %x, want %x" % (a, b, r, want)
        return None
    if r % P != a * b * RINV % P:
        return "a=%x b=%x: %x is not a b / R mod p" % (a, b, r)
    if r >= product_bound(a, b):
        return "a=%x b=%x: %x = %.4f p exceeds the bound" % (a, b, r, r / P)
    return None


# ------------------------------------------------------------------------------ slot values
@functools.lru_cache(maxsize=None)
def slot_values():
    """Slot contents, all below 2p: the edges, then 5 seeded random values."""
    rng = random.Random(0x51C7)
    return (0, 1, P - 1, P, 2 * P - 2, 2 * P - 1, 2 ** 381) + tuple(rng.randrange(2 * P) for _ in range(5))


@functools.lru_cache(maxsize=None)
def pre_add2_cases():
    """(A, B, C, D, ny, any_neg): every 4-tuple of the slot values with the seven edges and one
    random value, and seeded picks of the rest, in each (ny, any_neg) combination with
    ny => any_neg."""
    sv = slot_values()
    rng = random.Random(0xADD2)
    quads = list(itertools.product(sv[:8], repeat=4))
    quads += [tuple(rng.choice(sv) for _ in range(4)) for _ in range(256)]
    return tuple(q + f for q in quads for f in ((0, 0), (0, 1), (1, 1)))


def pre_add2_expect(A, B, C, D, ny, any_neg):
    return A + B, (C + 2 * P - D) if ny else C + D


# ------------------------------------------------------------------------------ unit lin
def lin_ctl(mb, mc, md, k, all_bits):
    """The control word of one lin_unit case: bits 0..2 the negation masks of B, C, D, bits
    8..11 the scale k, and the phase-header bits in their own positions -- the minimal ones for
    the masks (tools/fpvm/sched.py phase_bits), or all three. The scheduler puts negated terms last,
    so it never emits a lane with B negated and D not; for those masks "minimal" is this table's own
    reading of lin_sum (H_LINNEG3 applies all three masks), not something phase_bits produces."""
    hdr = (H_LINNEG if (mb or mc or md) else 0) | (H_LINNEG2 if mc else 0) | (H_LINNEG3 if mb else 0)
    if all_bits:
        hdr = H_LINNEG | H_LINNEG2 | H_LINNEG3
    return mb | mc << 1 | md << 2 | k << 8 | hdr


def _split_sum(s, want_mask, greedy):
    """Four terms X_t < 2p and masks whose unreduced sum A + B' + C' + D' (X' = 2p - X for a
    negated term) is exactly s < 8p - 3. A negated term needs a share in [1, 2p]."""
    top = 2 * P - 1
    if greedy:
        ys, rest = [], s
        for _ in range(4):
            ys.append(min(rest, top))
            rest -= ys[-1]
    else:
        q = s // 4
        ys = [q, q, q, s - 3 * q]
    assert sum(ys) == s and all(0 <= y <= top for y in ys), hex(s)
    masks = [0] + [1 if (want_mask >> (2 - t)) & 1 and ys[t + 1] >= 1 else 0 for t in range(3)]
    xs = [2 * P - y if m else y for y, m in zip(ys, masks)]
    assert all(0 <= x < 2 * P for x in xs)
    return xs, masks[1:]


@functools.lru_cache(maxsize=None)
def lin_unit_cases():
    """(A, B, C, D, mb, mc, md, k, all_bits) for lin_sum + scale_reduce as exec runs them.
    Generic: every mask combination x minimal / all header bits x k = 1..15 on rotating edge
    values and seeded picks. Adversarial: for each k and m in [0, 8k], unreduced sums
    s = ceil((m p + d) / k) and floor((m p + d) / k), d in -2..2, so that k s sits just above and
    just below m p."""
    sv = slot_values()
    rng = random.Random(0x11F0)
    cases = []
    n = 0
    for mask in range(8):
        mb, mc, md = mask >> 2 & 1, mask >> 1 & 1, mask & 1
        for all_bits in (0, 1):
            for k in range(1, 16):
                for pick in range(4):
                    if pick == 0:
                        t = tuple(sv[(n + j) % 7] for j in range(4))
                    elif pick == 1:
                        # the extremes of the unreduced sum: 0 or 2p - 1 in, 2p or 1 after negation
                        t = tuple((2 * P - 1) if (n >> j) & 1 else 0 for j in range(4))
                    else:
                        t = tuple(rng.choice(sv) for _ in range(4))
                    n += 1
                    cases.append(t + (mb, mc, md, k, all_bits))
    seen = set()
    for k in range(1, 16):
        for m in range(8 * k + 1):
            # ceil puts k s in [m p + d, m p + d + k), floor in (m p + d - k, m p + d]: both sides of m p
            for d, up in itertools.product(range(-2, 3), (1, 0)):
                s = min(max(-(-(m * P + d) // k) if up else (m * P + d) // k, 0), 8 * P - 4)
                if (k, s) in seen:
                    continue
                seen.add((k, s))
                i = len(seen)
                xs, (mb, mc, md) = _split_sum(s, i % 8, (i >> 3) & 1)
                cases.append(tuple(xs) + (mb, mc, md, k, (i >> 4) & 1))
    return tuple(cases)


def lin_unit_sum(A, B, C, D, mb, mc, md):
    """The unreduced sum lin_sum forms (a negated term enters as 2p - X)."""
    return A + (2 * P - B if mb else B) + (2 * P - C if mc else C) + (2 * P - D if md else D)


def check_lin_unit(case, r):
    A, B, C, D, mb, mc, md, k, _ = case
    want = k * (A + (-B if mb else B) + (-C if mc else C) + (-D if md else D)) % P
    if r % P != want:
        return "lin_unit %s: %x is not congruent to %x" % (_show(case), r, want)
    if not 0 <= r < 2 * P:
        return "lin_unit %s: %x = %.4f p leaves [0, 2p)" % (_show(case), r, r / P)
    return None


# ------------------------------------------------------------------------------ lin_mad
@functools.lru_cache(maxsize=None)
def lin_mad_cases():
    """(A, B, C, D, ca, cb, cc, cd): {-15, -1, 0, 1, 15}^4 on six seeded operand picks each, and
    {-15, 0, 15}^4 on the four extreme vectors (all-negative tuples on 2p - 1 reach top <= 0,
    all +-15 tuples reach s' ~ 120p)."""
    sv = slot_values()
    rng = random.Random(0x3AD0)
    top = 2 * P - 1
    cases = []
    for cf in itertools.product((-15, -1, 0, 1, 15), repeat=4):
        for _ in range(6):
            cases.append(tuple(rng.choice(sv) for _ in range(4)) + cf)
    for cf in itertools.product((-15, 0, 15), repeat=4):
        for vec in ((0, 0, 0, 0), (top, top, top, top), (top, 0, top, 0), (0, top, 0, top)):
            cases.append(vec + cf)
    return tuple(cases)


def check_lin_mad(case, r):
    want = sum(c * x for x, c in zip(case[:4], case[4:])) % P
    if r % P != want:
        return "lin_mad %s: %x is not congruent to %x" % (_show(case), r, want)
    if not 0 <= r < 2 * P:
        return "lin_mad %s: %x = %.4f p leaves [0, 2p)" % (_show(case), r, r / P)
    return None


# ------------------------------------------------------------------------------ quot_est flips
# quot_est (fpvm.hpp) returns trunc(f32(t) * QS) for t = x >> 359: the quotient m is first
# estimated as m (no longer m - 1) near t = m (Pt + 1) / (1 - 2^-20), Pt = p >> 359. Either
# answer keeps the result in [0, 2p), but this is where a difference in f32 conversion, rounding
# or contraction between the host compiler and the device compiler would change the limbs, so
# the device test compares them there. f32 holds 24 bits of t < 2^30: the flip is smeared over
# +-64 around that t, which the offsets below sample.
PT1 = (P >> 359) + 1


def _flip_t(m):
    return (m * PT1 << 20) // ((1 << 20) - 1)


@functools.lru_cache(maxsize=None)
def lin_unit_flip_cases():
    """lin_unit cases whose k (s >> 359) brackets the flip of each quotient m < 8k."""
    rng = random.Random(0xF11B)
    cases = []
    for k in range(1, 16):
        for m in range(1, 8 * k):
            u0 = _flip_t(m) // k
            for u in (u0, u0 + 1):
                s = min((u << 359) + rng.randrange(1 << 359), 8 * P - 4)
                i = len(cases)
                xs, (mb, mc, md) = _split_sum(s, i % 8, (i >> 3) & 1)
                cases.append(tuple(xs) + (mb, mc, md, k, (i >> 4) & 1))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def lin_mad_flip_cases():
    """lin_mad cases c (A + B + C + D) whose sum's top bits sit at and around the flip of each
    quotient m < 120."""
    rng = random.Random(0xF11C)
    cases = []
    for m in range(1, 120):
        c = m // 8 + 1
        for d in (-64, -32, -1, 0, 1, 32, 64):
            y = min(-(-((_flip_t(m) + d) << 359) // c) + rng.randrange(1 << 300), 8 * P - 4)
            xs, _ = _split_sum(y, 0, len(cases) & 1)
            cases.append(tuple(xs) + (c, c, c, c))
    return tuple(cases)


def _show(case):
    return "(" + ", ".join("%x" % v if v > 99 else str(v) for v in case) + ")"


# ------------------------------------------------------------------------------ canon, inverse
@functools.lru_cache(maxsize=None)
def canon_cases():
    rng = random.Random(0xCA20)
    return (0, 1, P - 1, P, P + 1, 2 * P - 1) + tuple(rng.randrange(2 * P) for _ in range(58))


@functools.lru_cache(maxsize=None)
def fp_inv_values():
    """Canonical values for the divsteps inverse: edges, seeded random values, and values with
    long runs of zero / one bits (shared by tests/test_vm_host.py::test_fp_inv and the device
    test)."""
    rng = np.random.default_rng(0xB1A5)
    vals = [0, 1, 2, 3, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, 2 ** 380, 2 ** 381 - 1 - P + P // 3,
            (1 << 32) - 1, 1 << 200, P - (1 << 300)]
    vals += [int.from_bytes(rng.bytes(48), "little") % P for _ in range(400)]
    vals += [int.from_bytes(rng.bytes(48), "little") % (1 << int(rng.integers(1, 381))) for _ in range(100)]
    return tuple(a % P for a in vals)


def fp_inv_expect(a):
    return pow(a, -1, P) if a else 0
