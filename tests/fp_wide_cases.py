"""Operands and hand-encoded one-phase programs for the radix-2^392 ("wide") Montgomery product
(csrc/bls/fp.hpp fp_mul_wide, fpvm.hpp's wide path), shared by tests/test_fp_wide_host.py (host
build) and tests/test_gpu_fp_wide.py (gfx950). Expectations are exact Python integers.

The wide product takes a, b < 4p and returns r = a b 2^-392 mod p with NO conditional
subtraction; the interpreter skips it because r <= p + floor(a b / 2^392) < 1.0064 p < 2p. That
bound, not just r < 2p, is what check_product asserts."""
import random

from vm_helpers import P, sched

WIDE_BITS = 392
RW_INV = pow(1 << WIDE_BITS, -1, P)
EDGES = [0, 1, P - 1, P, P + 1, 2 * P - 1, 2 * P, 4 * P - 1]


def _limb_patterns():
    """Values below 4p whose 28-bit or 32-bit limbs are all ones or all zero in alternation, and
    the largest top limb 4p - 1 allows over zero and all-one lower limbs."""
    out = []
    for bits in (28, 32):
        n = -(-384 // bits)
        m = (1 << bits) - 1
        for phase in (0, 1):
            v = sum(m << (bits * k) for k in range(n) if k % 2 == phase)
            out.append(v)
        out.append(sum(m << (bits * k) for k in range(n)))   # every limb all ones
        for k in range(1, n):                                   # one boundary: ones below, zero above
            out.append((1 << (bits * k)) - 1)
            out.append(1 << (bits * k))
    top = (4 * P - 1) >> 352
    out += [top << 352, (top << 352) | ((1 << 352) - 1), ((top - 1) << 352) | ((1 << 352) - 1)]
    top28 = (4 * P - 1) >> 364
    out += [top28 << 364, ((top28 - 1) << 364) | ((1 << 364) - 1)]
    # a pattern that reaches past 4p (> 2^382) enters cut to its low 382 bits
    return sorted({v if v < 4 * P else v & ((1 << 382) - 1) for v in out} | {4 * P - 1})


def product_pairs():
    """Every pair of the range edges, the limb patterns against themselves, the edges and each
    other, and 300 seeded random pairs below 4p."""
    rng = random.Random(0x392)
    pats = _limb_patterns()
    pairs = [(a, b) for a in EDGES for b in EDGES]
    pairs += [(a, a) for a in pats]
    pairs += [(a, b) for a in pats for b in (4 * P - 1, P, 1)]
    pairs += [(pats[i], pats[-1 - i]) for i in range(len(pats))]
    pairs += [(rng.randrange(4 * P), rng.randrange(4 * P)) for _ in range(300)]
    return pairs


def check_product(a, b, r):
    """None, or what is wrong with r as the wide product of a and b."""
    if r % P != a * b * RW_INV % P:
        return "a=%x b=%x: r=%x is not a b 2^-392 mod p" % (a, b, r)
    if r > P + (a * b >> WIDE_BITS):
        return "a=%x b=%x: r=%x above p + floor(a b / 2^392)" % (a, b, r)
    return None


def words(v):
    return [(v >> (32 * k)) & 0xFFFFFFFF for k in range(12)]


def value(ws):
    return sum(int(w) << (32 * k) for k, w in enumerate(ws))


# ---------------------------------------------------------------- hand-encoded phases
def fixed_table():
    """The constant table's fixed entries alone (plain 1, zero, n (2p + 1))."""
    consts = sched.ConstTable()
    consts.ref(1, True)
    consts.ref(0, False)
    for n in range(5):
        consts.ref(n * (2 * P + 1), True)
    return consts.words()


ONE, ZERO = sched.CONST_BASE + 0, sched.CONST_BASE + 1
# raw operands of the flag ops: the multiples of p (whose wide product by 1 is p itself, the one
# non-canonical value the flag ops must treat as 0), 1 and p + 1 (the same value), and (p +- 1) / 2 + p; on top of
# them the representatives of the values 0, 1, (p - 1) / 2 and (p + 1) / 2, where sgn0 and lex flip
_RW = pow(2, WIDE_BITS, P)
FLAG_X = [0, P, 2 * P, 3 * P, 1, P + 1, (P + 1) // 2 + P, (P - 1) // 2 + P,
          _RW, _RW + 2 * P, (P - 1) // 2 * _RW % P + P, (P + 1) // 2 * _RW % P + 3 * P]


def _split(x):
    """x < 4p as a pre-add A + B of two slot values"""
    a = min(x, 2 * P - 1)
    return a, x - a


class Phase:
    """One phase of W lanes, every lane an op of its own over raw slot contents."""

    def __init__(self, W):
        self.W = W
        self.slots = []
        self.lanes = []     # (w0, w1, w2, w3) without the header
        self.expect = []    # (dst slot, kind, x, y)

    def slot(self, v):
        self.slots.append(v)
        return len(self.slots) - 1

    def op(self, kind, A, B, C, D, neg_y, x, y):
        dst = self.slot(0)
        w3 = 1 | 1 << 5 | 1 << 10 | ((-1 if neg_y else 1) & 31) << 15 | sched.WIDE
        self.lanes.append([sched.OPC[kind] | dst << 5, A | B << 16, C | D << 16, w3])
        self.expect.append((dst, kind, x, y))

    def muls(self, a, b, c, d, neg):
        """(a + b) (c + d), or (a + b) (c + 2p - d)"""
        self.op("muls", self.slot(a), self.slot(b), self.slot(c), self.slot(d), neg, a + b,
                c + (2 * P - d if neg else d))

    def flag(self, kind, x):
        """sgn0 / lex of the raw x = A + B times the plain 1; eq of C - D = x as C + 2p - D"""
        if kind == "eq":
            c, d = (x - 2 * P, 0) if x >= 2 * P else (0, 2 * P - x)
            self.op("eq", ONE, ZERO, self.slot(c), self.slot(d), True, 1, x)
        else:
            a, b = _split(x)
            self.op(kind, self.slot(a), self.slot(b), ONE, ZERO, False, x, 1)

    def encode(self):
        assert 0 < len(self.lanes) <= self.W
        hdr = 0
        for w in self.lanes:
            hdr |= sched.phase_bits(w)
        code = []
        for k in range(self.W):
            w = self.lanes[k] if k < len(self.lanes) else [0, self.lanes[0][1], self.lanes[0][2], 0]
            code += [w[0] | hdr] + w[1:]
        slots = [x for v in self.slots for x in words(v)]
        return code, slots

    def check(self, slots_out):
        """Failures of the phase's results (slot words after the run) against exact integers."""
        bad = []
        for dst, kind, x, y in self.expect:
            r = value(slots_out[12 * dst:12 * dst + 12])
            if kind == "muls":
                e = check_product(x, y, r)
                if e is None and r >= 2 * P:
                    e = "x=%x y=%x: r=%x not below 2p" % (x, y, r)
            else:
                # the value the raw operand stands for, x 2^-392 mod p (the other operand is the
                # plain 1): the same for every representative of x mod p
                v = x * y * RW_INV % P
                want = {"sgn0": v & 1, "lex": int(v > (P - 1) // 2), "eq": int(v == 0)}[kind]
                e = None if r == want else "%s of raw %x: flag %x, want %d" % (kind, x * y, r, want)
            if e:
                bad.append(e)
        return bad


def muls_phase():
    """Sixteen products with both pre-adds, eight of them with a negated y, up to x = 4p - 2 and
    y = 4p - 1; no flag op, so no lane of the phase is canonicalised."""
    rng = random.Random(0x28E)
    ph = Phase(16)
    top = 2 * P - 1
    quads = [(top, top, top, top), (top, top, top, 0), (P, P - 1, P + 1, 1), (0, 0, top, top), (1, 0, 0, top)]
    quads += [tuple(rng.randrange(2 * P) for _ in range(4)) for _ in range(3)]
    for q in quads:
        ph.muls(*q, neg=False)
        ph.muls(*q, neg=True)
    return ph


def flag_phase():
    """sgn0, lex and eq of the raw values FLAG_X (3p by a pre-add; eq's operand through the
    negation chain), beside two plain products: 38 ops on a 64-lane slice."""
    ph = Phase(64)
    for kind in ("sgn0", "lex", "eq"):
        for x in FLAG_X:
            ph.flag(kind, x)
    ph.muls(2 * P - 1, 2 * P - 1, 2 * P - 1, 0, neg=True)
    ph.muls(P, 0, 1, 0, neg=False)
    return ph
