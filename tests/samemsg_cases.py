"""Crafted rounds for the unit-level tests of the same-message path (csrc/ovhip.hip
verify_samemsg_locked) and their exact expectations, on plain integers and
the Python oracle (oracle/py/bls12_381.py) only: no GPU, no ctypes, nothing of tools/fpvm.

The path decides a batch of n votes over G distinct hashes with one equation,

    prod_g e(sum_{i in g} r_i pk_i, H_g) * e(-G1, sum_i r_i sigma_i) == 1,

and this module restates everything that builds its left-hand factor:

  plan()            samemsg_plan: the distinct hashes in first-seen order, gid, head, and the pairs
                    (a, b): P[a] += P[b], level by level with level_off, over the staged order perm
  Vote              a vote's bytes with what the per-vote programs must answer for it: the code in
                    the reference precedence, sigma, tau = -psi^2(sigma) and
                    r pk = [rlc_scalar(vote_scalar(seed, base, i))] pk
  vsame_runs()      launches of k_vm_vsame<TABLE, W>: slices and tails, table indices that are
                    permuted and repeated, flagged table entries over poisoned planes, base + i
                    crossing 2^32 and 2^63, chosen RLC values (seed_for inverts SplitMix64), one
                    vote per class of tests/point_cases.py
  keysum_cases()    k_samemsg_fix + the k_vm_g1pairs levels on chosen key sums: group sizes 1 .. 65,
                    G = 1, 2, 5, 11, 70, members interleaved, doublings and cancellations at level
                    0 and above, identities, failed votes over poison, a hash with H = O
  h2g_cases()       k_h2f + k_vm_h2g on hashes, and on chosen u with H = O
  bisect_runs()     k_vm_vote1h_b + k_vm_votefe behind a verdict word
  batch_rounds()    whole rounds through ovh_verify_batch: valid ones (verdict 1) and ones with
                    invalid votes, on both slice widths, every table / bytes split

The check_* helpers compare what a device returned (words, as the probe of
tests/device/samemsg_probe.hip lays them out) with these expectations, exactly; the synth_*
helpers build the words a right device would return, so that tests/test_samemsg_cases.py can show
that a helper notices one changed limb, code or verdict. Everything is deterministic and built
once per process."""
import collections
import functools
import hashlib
import random

import bls12_381 as bls
import msm_cases
import pairing_cases as pcs
import pairing_ref as ref
import point_cases as pc

P, R = bls.P, bls.R
F1, F2 = bls.FpOps, bls.Fp2Ops
M64 = (1 << 64) - 1
LAMBDA = (-(bls.X * bls.X)) % R        # phi(P) = [LAMBDA] P on G1, tau = -psi^2(sigma) = [LAMBDA] sigma
MONT = pow(2, 384, P)
MONT_INV = pow(MONT, -1, P)
POISON = 0xFFFFFFFF
GUARD = 2                               # sp_guard()
VSAME8_MIN = 16                         # the probe's -DVSAME8_MIN
VS_W, G1_W, G2_W, F_W = 132, 36, 72, 144
BAD_ENCODING, NOT_ON_CURVE, NOT_IN_GROUP, VERIFY_FAIL, PK_IS_INFINITY, ERR_PUBKEY = 1, 2, 3, 5, 6, 102
PKF_PARSE, PKF_INF, PKF_GRP = 1, 2, 4
FLAG_CODE = {0: 0, PKF_PARSE: ERR_PUBKEY, PKF_INF: PK_IS_INFINITY, PKF_GRP: NOT_IN_GROUP}
NG1 = (bls.G1_GEN[0], (P - bls.G1_GEN[1]) % P)


# ------------------------------------------------------------------------------ scalars
def rlc_scalar(z):
    """the effective scalar of the 64-bit RLC value z = a + 2^32 b: a + b LAMBDA"""
    return ((z & 0xFFFFFFFF) + (z >> 32) * LAMBDA) % R


def _unshift(z, s):
    """x with x ^ (x >> s) == z"""
    x = z
    for _ in range(64 // s + 1):
        x = z ^ (x >> s)
    return x


def seed_for(z, base, i):
    """The seed under which vote_scalar(seed, base, i) is z (SplitMix64 is a bijection of
    seed + 0x9E37... (base + i + 1)); z = 0 gives the seed whose mix is 0, which the device and
    msm_cases.splitmix replace by 1."""
    x = _unshift(z, 31)
    x = x * pow(0x94D049BB133111EB, -1, 1 << 64) & M64
    x = _unshift(x, 27)
    x = x * pow(0xBF58476D1CE4E5B9, -1, 1 << 64) & M64
    x = _unshift(x, 30)
    seed = (x - 0x9E3779B97F4A7C15 * (((base + i) & M64) + 1)) & M64
    assert msm_cases.vote_scalar(seed, base, i) == (z or 1)
    return seed


# RLC values by their halves (a: the low word, sigma's and pk's scalar; b: the high word, tau's and
# phi(pk)'s): a = 0, b = 0, a = b, a single bit 31 or 63, all ones, and 0 (which becomes 1)
RLC_EDGES = (("a_zero", 0xDEADBEEF00000000), ("b_zero", 0x00000000CAFEF00D), ("a_eq_b", 0x8765432187654321),
             ("bit31", 1 << 31), ("bit63", 1 << 63), ("ones", M64), ("zero", 0))


# ------------------------------------------------------------------------------ limbs
def limbs(v):
    m = v % P * MONT % P
    return [(m >> (32 * k)) & 0xFFFFFFFF for k in range(12)]


def value(words):
    """12 words -> the canonical value; asserts the limbs are a canonical Montgomery form"""
    m = sum(int(w) << (32 * k) for k, w in enumerate(words))
    assert m < P, "a device limb value is not below p"
    return m * MONT_INV % P


def g1_words(pt):
    return [w for c in pt for w in limbs(c)]


def g1_of(words):
    return tuple(value(words[12 * k:12 * k + 12]) for k in range(3))


def g2a_words(pt):
    """affine G2 point -> x.c0, x.c1, y.c0, y.c1"""
    return [w for c2 in pt for c in c2 for w in limbs(c)]


def g2p_words(pt):
    return [w for c2 in pt for c in c2 for w in limbs(c)]


def g2p_of(words):
    v = [value(words[12 * k:12 * k + 12]) for k in range(6)]
    return ((v[0], v[1]), (v[2], v[3]), (v[4], v[5]))


def f12_of(words):
    return ref.unflat([value(words[12 * k:12 * k + 12]) for k in range(12)])


def g1_mul(k, pt=None):
    return bls.pt_mul(F1, pt or bls.G1_GEN, k % R) if k % R else None


def g1_add(a, b):
    return bls.pt_add(F1, a, b)


def tau_of(sigma):
    return bls.pt_neg(F2, bls.g2_psi(bls.g2_psi(sigma)))


# ------------------------------------------------------------------------------ the plan
Plan = collections.namedtuple("Plan", "G gid ghash head pairs level_off members")


def plan(hashes, perm=None):
    """samemsg_plan: hashes[i] of the caller's vote i, staged vote j = the caller's perm[j] (perm
    None or empty: j). gid, head, pairs index staged votes; pairs is the flat list of (a, b),
    level_off the pair offsets of the levels, one past the last."""
    n = len(hashes)
    index, members, gid, ghash = {}, [], [], []
    for j in range(n):
        h = hashes[perm[j] if perm else j]
        if h not in index:
            index[h] = len(members)
            members.append([])
            ghash.append(h)
        gid.append(index[h])
        members[index[h]].append(j)
    pairs, level_off, stride = [], [0], 1
    while True:
        level = [(m[q], m[q + stride]) for m in members for q in range(0, len(m) - stride, 2 * stride)]
        if not level:
            break
        pairs += level
        level_off.append(len(pairs))
        stride *= 2
    return Plan(len(members), gid, ghash, [m[0] for m in members], pairs, level_off, members)


def evaluate(pl, values, add):
    """the pairs applied level by level to a copy of `values` (one per staged vote) -> (every
    entry afterwards, the set of entries some pair wrote)"""
    v = list(values)
    written = set()
    for l in range(len(pl.level_off) - 1):
        for a, b in pl.pairs[pl.level_off[l]:pl.level_off[l + 1]]:
            v[a] = add(v[a], v[b])
            written.add(a)
    return v, written


def table_split(pks, validators):
    """table_split of csrc/ovhip.hip: -> (perm or None, the table index of every staged table
    vote): table votes first, each part in the caller's order; a key's first table entry"""
    first = {}
    for e, k in enumerate(validators):
        first.setdefault(k, e)
    ent = [first.get(k, -1) for k in pks]
    t = sum(e >= 0 for e in ent)
    if t == len(pks) or t == 0:
        return None, [e for e in ent if e >= 0]
    perm = [i for i, e in enumerate(ent) if e >= 0] + [i for i, e in enumerate(ent) if e < 0]
    return perm, [ent[i] for i in perm[:t]]


# ------------------------------------------------------------------------------ signers, hashes, votes
NSIGNERS, NHASHES = 12, 6


@functools.lru_cache(maxsize=None)
def signers():
    """(secret key, key point) of NSIGNERS signers"""
    rng = random.Random("samemsg-signers")
    sks = [rng.randrange(1, R) for _ in range(NSIGNERS)]
    return tuple((sk, bls.pt_mul(F1, bls.G1_GEN, sk)) for sk in sks)


def hash_of(k):
    return hashlib.sha256(b"samemsg-case-hash-%d" % k).digest()


@functools.lru_cache(maxsize=None)
def H_of(k):
    return bls.hash_to_g2(hash_of(k))


@functools.lru_cache(maxsize=None)
def sig_of(s, k):
    return bls.pt_mul(F2, H_of(k), signers()[s][0])


# pk: 48 bytes; sig: 96 bytes; hash: 32 bytes; kpt / spt: the key / signature as an affine point of
# the group when the encoding is one (else None); kcode / scode: what the key / the signature
# alone makes of the vote (0, ERR_PUBKEY, PK_IS_INFINITY, NOT_IN_GROUP; 0, BAD_ENCODING,
# NOT_ON_CURVE, NOT_IN_GROUP, VERIFY_FAIL for the infinite signature); valid: sigma = [sk] H(hash)
Vote = collections.namedtuple("Vote", "name pk sig hash kpt spt kcode scode valid")
INF_PK = bytes([0xC0]) + bytes(47)
INF_SIG = bytes([0xC0]) + bytes(95)


def good(s, k):
    sk, pk = signers()[s % NSIGNERS]
    sg = sig_of(s % NSIGNERS, k)
    return Vote("signer %d hash %d" % (s % NSIGNERS, k), bls.g1_compress(pk), bls.g2_compress(sg), hash_of(k), pk, sg, 0, 0, True)


def wrong(s, k):
    """a well-formed vote whose signature is another signer's"""
    v, o = good(s, k), good(s + 1, k)
    return v._replace(name=v.name + " wrong signer", sig=o.sig, spt=o.spt, valid=False)


def with_key(c, k=0, s=0):
    """the vote of signer s with the crafted G1 case c (tests/point_cases.py), or INF_PK, as its key"""
    v = good(s, k)
    if c is None:
        return v._replace(name="key at infinity", pk=INF_PK, kpt=None, kcode=PK_IS_INFINITY, valid=False)
    code = c.code()
    return v._replace(name="key " + c.name, pk=c.enc, kpt=c.point if code == 0 else None, kcode=code, valid=False)


def with_sig(c, k=0, s=0):
    v = good(s, k)
    if c is None:
        return v._replace(name="signature at infinity", sig=INF_SIG, spt=None, scode=VERIFY_FAIL, valid=False)
    code = c.code()
    return v._replace(name="sig " + c.name, sig=c.enc, spt=c.point if code == 0 else None, scode=code, valid=False)


def format_code(kcode, scode):
    """the reference precedence (consensus.rs:397-416) before the pairing: a key that does not
    parse, the signature's decoding and group check, the key at infinity or outside the group, the
    signature at infinity"""
    if kcode == ERR_PUBKEY:
        return ERR_PUBKEY
    if scode in (BAD_ENCODING, NOT_ON_CURVE, NOT_IN_GROUP):
        return scode
    if kcode:
        return kcode
    return scode


def _first(cs, cl):
    """the first case of a class, preferring one whose subgroup-check ladder meets O, Q or -Q"""
    group = [c for c in cs if c.cls == cl]
    return next((c for c in group if c.events), group[0])


def class_votes(keys=True):
    """one vote per class of the crafted G1 cases (keys) beside a good signature, one per class of
    the G2 cases beside a good key, and both infinities"""
    g1, g2 = pc.cases()
    out = []
    if keys:
        for cl in pc.G1_CLASSES:
            out.append(with_key(_first(g1, cl)))
        out.append(with_key(None))
    for cl in pc.G2_CLASSES:
        out.append(with_sig(_first(g2, cl), s=len(out)))
    out.append(with_sig(None))
    return out


# ------------------------------------------------------------------------------ k_vm_vsame
# entries: [(affine key point or None, flags)] of the caller-given table; tidx: one entry per vote
VsameRun = collections.namedtuple("VsameRun", "name cls table w8 lo votes seed base entries tidx")


def table_words(entries, rng):
    """-> (tcap x 36 words, flags): a usable entry as (X z : Y z : z), z != 1; a flagged entry's
    planes hold poison"""
    words, flags = [], []
    for pt, fl in entries:
        if fl:
            words += [POISON] * G1_W
        else:
            z = rng.randrange(2, P)
            words += g1_words((pt[0] * z % P, pt[1] * z % P, z))
        flags.append(fl)
    return words, flags


def vsame_expect(run):
    """per vote -> (code, sigma or None, tau or None, r pk or None): None where the encoding has no
    point of the group, and nothing is asserted of the planes"""
    out = []
    for j, v in enumerate(run.votes):
        z = msm_cases.vote_scalar(run.seed, run.base, run.lo + j)
        if run.table:
            kpt, fl = run.entries[run.tidx[j]]
            kcode = FLAG_CODE[fl]
            kpt = None if fl else kpt
        else:
            kpt, kcode = v.kpt, v.kcode
        rpk = bls.pt_mul(F1, kpt, rlc_scalar(z)) if kpt is not None else None
        out.append((format_code(kcode, v.scode), v.spt, tau_of(v.spt) if v.spt is not None else None, rpk))
    return out


def _table_for(n):
    """24 entries, more than any run has votes: signers 0..5, the three flags over poisoned planes,
    signers 6..11, and flagged entries to the end; indices permuted and repeated"""
    ent = [(signers()[s][1], 0) for s in range(6)] + [(None, PKF_PARSE), (None, PKF_INF), (None, PKF_GRP)]
    ent += [(signers()[s][1], 0) for s in range(6, 12)] + [(None, PKF_PARSE)] * 9
    tidx = [(5 * j + 3) % 6 for j in range(n)]
    return ent, tidx


@functools.lru_cache(maxsize=None)
def vsame_runs():
    runs = []
    bases = (0x1000, (1 << 32) - 3, (1 << 63) - 3)
    # slices and tails: 16-lane slices four to a workgroup, 8-lane slices eight
    for k, (w8, n) in enumerate(((0, 1), (0, 4), (0, 5), (1, 8), (1, 9), (1, 17))):
        for table in (0, 1):
            ent, tidx = _table_for(n)
            lo = 0 if table else 3            # the key-bytes launch starts behind the table votes
            votes = []
            for j in range(n):
                s = tidx[j] if table else j
                votes.append(good(s, j % 2))
            if n > 1:                          # the last vote of the tail fails on its own
                votes[-1] = with_sig(pc.cases()[1][0], s=tidx[-1] if table else n - 1)
            runs.append(VsameRun("n=%d w8=%d table=%d" % (n, w8, table), "slices", table, w8, lo, tuple(votes),
                                 0x5EED0000 + n, bases[(k + table) % 3], tuple(ent), tuple(tidx)))
    # chosen RLC values, every program
    for name, z in RLC_EDGES:
        for table in (0, 1):
            for w8 in (0, 1):
                lo, base = 2, 0x77
                ent, tidx = _table_for(1)
                runs.append(VsameRun("rlc %s w8=%d table=%d" % (name, w8, table), "rlc", table, w8, lo,
                                     (good(tidx[0] if table else 4, 1),), seed_for(z, base, lo), base, tuple(ent), tuple(tidx)))
    # one vote per class, every program; the table programs meet the key classes as flags
    for table in (0, 1):
        for w8 in (0, 1):
            votes = class_votes(keys=not table)
            ent, _ = _table_for(1)
            tidx = [j % 6 for j in range(len(votes))]
            if table:
                votes = [good(tidx[j], 0)._replace(name=v.name, sig=v.sig, spt=v.spt, scode=v.scode, valid=False)
                         for j, v in enumerate(votes)]
                votes += [good(0, 0)] * 3     # good signatures under PKF_PARSE, PKF_INF, PKF_GRP over poisoned planes
                tidx += [6, 7, 8]
            runs.append(VsameRun("classes w8=%d table=%d" % (w8, table), "classes", table, w8, 1, tuple(votes),
                                 0xC1A55E5, 0x2000, tuple(ent), tuple(tidx)))
    return tuple(runs)


def vsame_inputs(run):
    """-> (sigs bytes, pks bytes or None, table words, flags, tidx, codes_in)"""
    n = len(run.votes)
    cap = run.lo + n + GUARD
    rng = random.Random("vsame-" + run.name)
    tw, tf = table_words(run.entries, rng)
    codes_in = [0x5A5A5A00 + i for i in range(cap)]
    return (b"".join(v.sig for v in run.votes), None if run.table else b"".join(v.pk for v in run.votes), tw, tf,
            list(run.tidx), codes_in)


def check_vsame(run, codes_in, codes, out):
    """codes (lo + n + GUARD words) and out ((lo + n + GUARD) x 132 words) of sp_vsame == the run"""
    n, lo = len(run.votes), run.lo
    cap = lo + n + GUARD
    assert len(codes) == cap and len(out) == cap * VS_W
    for i in list(range(lo)) + list(range(lo + n, cap)):
        assert codes[i] & 0xFFFFFFFF == codes_in[i] & 0xFFFFFFFF, "%s: code word %d outside the launch written" % (run.name, i)
        assert out[i * VS_W:(i + 1) * VS_W] == [POISON] * VS_W, "%s: planes of entry %d outside the launch written" % (run.name, i)
    for j, (code, sigma, tau, rpk) in enumerate(vsame_expect(run)):
        what = "%s vote %d (%s)" % (run.name, j, run.votes[j].name)
        w = out[(lo + j) * VS_W:(lo + j + 1) * VS_W]
        assert codes[lo + j] == code, "%s: code %d, expected %d" % (what, codes[lo + j], code)
        if sigma is not None:
            assert w[:48] == g2a_words(sigma), what + ": sigma"
            assert w[48:96] == g2a_words(tau), what + ": tau"
        if rpk is not None:
            got = g1_of(w[96:132])
            assert got[2] != 0 and pcs.aff1(got) == rpk, what + ": r pk"


def synth_vsame(run):
    """what a right device returns for the run: (codes, out)"""
    _, _, _, _, _, codes = vsame_inputs(run)
    n, lo = len(run.votes), run.lo
    out = [POISON] * ((lo + n + GUARD) * VS_W)
    for j, (code, sigma, tau, rpk) in enumerate(vsame_expect(run)):
        codes[lo + j] = code
        w = [0x11111111] * VS_W
        if sigma is not None:
            w[:96] = g2a_words(sigma) + g2a_words(tau)
        if rpk is not None:
            w[96:] = g1_words((rpk[0] * 7 % P, rpk[1] * 7 % P, 7))
        out[(lo + j) * VS_W:(lo + j + 1) * VS_W] = w
    return codes, out


# ------------------------------------------------------------------------------ the key sums
# scal[i]: the entry is [scal] G1 (0: the identity), as (X z : Y z : z) with z = zs[i], or
# (0 : zs[i] : 0) for the identity; None: poisoned planes (a vote that carries a code)
KeysumCase = collections.namedtuple("KeysumCase", "name n G gid ghinf codes scal zs plan")


def _interleave(sizes):
    """group labels, round-robin over the groups that still have members left"""
    left, out = list(sizes), []
    while any(left):
        for g, c in enumerate(left):
            if c:
                out.append(g)
                left[g] -= 1
    return out


def _keysum_case(name, sizes, tag, fix=None, ghinf=None, codes=None):
    """fix: {(group, member): scalar} in place of the random one; codes: {(group, member): code}"""
    rng = random.Random("keysum-" + tag)
    labels = _interleave(sizes)
    pl = plan([bytes([g]) * 32 for g in labels])
    assert [len(m) for m in pl.members] == list(sizes)
    n = len(labels)
    scal, zs, cd = [rng.randrange(1, R) for _ in range(n)], [rng.randrange(2, P) for _ in range(n)], [0] * n
    for (g, k), s in (fix or {}).items():
        scal[pl.members[g][k]] = s % R
    for (g, k), c in (codes or {}).items():
        cd[pl.members[g][k]] = c
        scal[pl.members[g][k]] = None
    return KeysumCase(name, n, pl.G, tuple(pl.gid), tuple(ghinf or [0] * pl.G), tuple(cd), tuple(scal), tuple(zs), pl)


SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 33, 64, 65)


@functools.lru_cache(maxsize=None)
def keysum_cases():
    s, t = 0x1234567, 0x89ABCDE
    out = [
        _keysum_case("sizes 1..65, G = 11", SIZES, "sizes"),
        _keysum_case("G = 1", (9,), "g1"),
        _keysum_case("G = 2", (3, 5), "g2"),
        # group 1: every vote failed; group 3: H = O; failed votes elsewhere, at a head, inside, at a tail
        _keysum_case("G = 5, failed votes, H = O", (4, 3, 7, 2, 6), "g5", ghinf=[0, 0, 0, 1, 0],
                     codes={(1, 0): 102, (1, 1): 2, (1, 2): 6, (0, 0): 3, (2, 3): 1, (2, 6): 5, (4, 1): 102, (4, 2): 102}),
        _keysum_case("G = 70", (2,) * 5 + (1,) * 65, "g70", codes={(1, 1): 2, (69, 0): 102}),
        _keysum_case("doublings, cancellations, identities", (2, 2, 4, 4, 3, 2, 2, 8, 5), "sums", fix={
            (0, 0): s, (0, 1): s,                                    # P + P at level 0
            (1, 0): s, (1, 1): -s,                                   # P + (-P) at level 0
            (2, 0): s, (2, 1): t, (2, 2): t, (2, 3): s,              # (s + t) + (t + s): a doubling at level 1
            (3, 0): s, (3, 1): t, (3, 2): -s, (3, 3): -t,            # a cancellation at level 1
            (4, 0): s, (4, 1): t, (4, 2): -(s + t),                  # a whole group summing to O
            (5, 0): 0, (5, 1): 0,                                    # O + O, as (0 : z : 0)
            (6, 0): 0, (6, 1): t,                                    # O + P
            (7, 0): s, (7, 1): 0, (7, 2): t, (7, 3): t, (7, 4): -s, (7, 5): 0, (7, 6): -t, (7, 7): -t,   # O at level 2
            (8, 4): 0}),                                             # P + O at the last level
    ]
    # an identity given as (0 : 1 : 0) exactly
    c = out[-1]
    zs = list(c.zs)
    zs[c.plan.members[5][0]] = 1
    out[-1] = c._replace(zs=tuple(zs))
    return tuple(out)


def keysum_words(c):
    """-> (n + GUARD) x 36 words of P"""
    w = []
    for s, z in zip(c.scal, c.zs):
        if s is None:
            w += [POISON] * G1_W
        elif s == 0:
            w += g1_words((0, z, 0))
        else:
            A = g1_mul(s)
            w += g1_words((A[0] * z % P, A[1] * z % P, z))
    return w + [POISON] * (GUARD * G1_W)


def keysum_expect(c):
    """-> (codes out, scalar of every entry after the levels, entries the levels wrote)"""
    codes = [VERIFY_FAIL if cd == 0 and c.ghinf[g] else cd for cd, g in zip(c.codes, c.gid)]
    start = [0 if cd else s for cd, s in zip(codes, c.scal)]
    after, written = evaluate(c.plan, start, lambda a, b: (a + b) % R)
    return codes, after, written


CODE_GUARD = 0x3C3C3C3C


def check_keysums(c, words_in, codes, words):
    """codes (n + GUARD) and P ((n + GUARD) x 36 words) of sp_keysums == the case: codes exact; every
    entry a pair wrote (the roots among them) equals the integer sum as a point; a failed vote no
    pair wrote holds (0 : 1 : 0) exactly; every other entry and the guard are untouched"""
    want, after, written = keysum_expect(c)
    assert [x & 0xFFFFFFFF for x in codes] == want + [CODE_GUARD] * GUARD, c.name + ": codes"
    identity = g1_words((0, 1, 0))
    for i in range(c.n + GUARD):
        w = words[i * G1_W:(i + 1) * G1_W]
        what = "%s: entry %d" % (c.name, i)
        if i in written:
            got = g1_of(w)
            exp = g1_mul(after[i])
            assert pcs.aff1(got) == exp and (exp is not None or got[1] != 0), what + " is not the sum of its subtree"
        elif i < c.n and want[i]:
            assert w == identity, what + ": a failed vote's planes are not (0 : 1 : 0)"
        else:
            assert w == words_in[i * G1_W:(i + 1) * G1_W], what + " is outside the plan and was written"
    for g, h in enumerate(c.plan.head):
        assert (h in written) == (len(c.plan.members[g]) > 1)


def synth_keysums(c):
    want, after, written = keysum_expect(c)
    words = keysum_words(c)
    for i in range(c.n):
        if i in written:
            A = g1_mul(after[i])
            words[i * G1_W:(i + 1) * G1_W] = g1_words((0, 5, 0) if A is None else (A[0] * 3 % P, A[1] * 3 % P, 3))
        elif want[i]:
            words[i * G1_W:(i + 1) * G1_W] = g1_words((0, 1, 0))
    return want + [CODE_GUARD] * GUARD, words


# ------------------------------------------------------------------------------ hash_to_G2 per hash
def h_of_u(u0, u1):
    """hash_to_G2 from its field elements, as bls.hash_to_g2 continues after hash_to_field"""
    q0 = bls.iso_map_g2(bls.map_to_curve_sswu(u0))
    q1 = bls.iso_map_g2(bls.map_to_curve_sswu(u1))
    return bls.clear_cofactor_g2_psi(bls.pt_add(F2, q0, q1))


@functools.lru_cache(maxsize=None)
def h2g_cases():
    """-> [(name, hashes or None, u pairs or None, [H affine or None])]: G = 1, 5 (two workgroups
    of four slices) and 6 on hashes; on chosen u: u1 = -u0 maps to H = O (map(-u) = -map(u)),
    beside two ordinary pairs"""
    hs = [hash_of(k) for k in range(NHASHES)]
    out = [("G = %d" % G, tuple(hs[:G]), None, tuple(H_of(k) for k in range(G))) for G in (1, 5, 6)]
    rng = random.Random("h2g-u")
    us = [((rng.randrange(P), rng.randrange(P)), (rng.randrange(P), rng.randrange(P))) for _ in range(3)]
    us[1] = (us[1][0], bls.f2_neg(us[1][0]))
    want = tuple(h_of_u(*u) for u in us)
    assert want[1] is None and want[0] is not None and want[2] is not None
    assert h_of_u(*bls.hash_to_field_fp2(hs[0], bls.DST_NUL, 2)) == H_of(0)
    out.append(("given u, H = O in the middle", None, tuple(us), want))
    return tuple(out)


def check_h2g(case, H, ghinf):
    name, hashes, us, want = case
    G = len(want)
    assert list(ghinf[G:]) == [POISON] * GUARD and H[G * G2_W:] == [POISON] * (GUARD * G2_W), name + ": guard written"
    for q, exp in enumerate(want):
        got = g2p_of(H[q * G2_W:(q + 1) * G2_W])
        assert ghinf[q] == int(exp is None), "%s: ghinf[%d]" % (name, q)
        assert pcs.aff2(got) == exp, "%s: H of hash %d" % (name, q)


def synth_h2g(case):
    want = case[3]
    H, inf = [], []
    for exp in want:
        H += g2p_words(pcs.proj2(exp, (3, 4)) if exp is not None else ((5, 6), (7, 8), (0, 0)))
        inf.append(int(exp is None))
    return H + [POISON] * (GUARD * G2_W), inf + [POISON] * GUARD


# ------------------------------------------------------------------------------ the bisection
# votes at slab indices lo ..; gid of every index below lo + n; hs: the hash number of every group;
# prior: {vote: code} carried in, over poisoned bytes
BisectRun = collections.namedtuple("BisectRun", "name table lo votes gid hs ghinf prior entries tidx")


@functools.lru_cache(maxsize=None)
def bisect_runs():
    runs = []
    for table in (0, 1):
        ent, _ = _table_for(1)
        lo = 0 if table else 2
        # two groups with different H; vote 3 carries the other group's gid; 1 is another signer's;
        # 4 and 6 carry a code over poisoned bytes; 7's hash has H = O (group 2)
        hs = (0, 1, 2)
        gid_v = [0, 1, 0, 0, 1, 1, 0, 2, 1]
        own = [0, 1, 0, 1, 1, 1, 0, 2, 1]                  # the hash each vote signed
        tidx = [(2 * j + 1) % 6 for j in range(len(own))]
        votes = [good(tidx[j] if table else j, own[j]) for j in range(len(own))]
        votes[1] = wrong(tidx[1] if table else 1, own[1])
        prior = {4: ERR_PUBKEY, 6: NOT_ON_CURVE}
        gid = [0] * lo + gid_v
        runs.append(BisectRun("table=%d" % table, table, lo, tuple(votes), tuple(gid), hs, (0, 0, 1), prior, tuple(ent),
                              tuple(tidx)))
    return tuple(runs)


def bisect_expect(run, verdict):
    """-> the code of every vote after k_vm_vote1h_b + k_vm_votefe"""
    out = []
    for j, v in enumerate(run.votes):
        g = run.gid[run.lo + j]
        if verdict == 1 or j in run.prior:
            out.append(run.prior.get(j, 0))
        elif run.ghinf[g]:
            out.append(VERIFY_FAIL)
        else:
            out.append(0 if v.valid and hash_of(run.hs[g]) == v.hash else VERIFY_FAIL)
    return out


def bisect_inputs(run):
    """-> (sigs, pks or None, table words, flags, tidx, gid, gh words, ghinf, codes_in)"""
    rng = random.Random("bisect-" + run.name)
    n = len(run.votes)
    sigs = b"".join(b"\xff" * 96 if j in run.prior else v.sig for j, v in enumerate(run.votes))
    pks = None if run.table else b"".join(b"\xff" * 48 if j in run.prior else v.pk for j, v in enumerate(run.votes))
    tw, tf = table_words(run.entries, rng)
    gh = []
    for k, inf in zip(run.hs, run.ghinf):
        z = (rng.randrange(1, P), rng.randrange(1, P))
        gh += [POISON] * G2_W if inf else g2p_words(pcs.proj2(H_of(k), z))
    codes = [CODE_GUARD] * run.lo + [run.prior.get(j, 0) for j in range(n)] + [CODE_GUARD] * GUARD
    return sigs, pks, tw, tf, list(run.tidx), list(run.gid), gh, list(run.ghinf), codes


def check_bisect(run, verdict, codes, f):
    n, lo = len(run.votes), run.lo
    want = [CODE_GUARD] * lo + bisect_expect(run, verdict) + [CODE_GUARD] * GUARD
    assert [x & 0xFFFFFFFF for x in codes] == want, "%s verdict %d: codes %s, expected %s" % (run.name, verdict, list(codes), want)
    for i in range(lo + n + GUARD):
        j = i - lo
        live = verdict == 0 and 0 <= j < n and j not in run.prior
        w = f[i * F_W:(i + 1) * F_W]
        if not live:
            assert w == [POISON] * F_W, "%s verdict %d: f planes of entry %d written" % (run.name, verdict, i)
        elif not run.ghinf[run.gid[i]]:
            assert w != [POISON] * F_W and (pcs.fe_of(f12_of(w)) == pcs.ONE_T) == (want[i] == 0), \
                "%s: f of vote %d against its code" % (run.name, j)


# ------------------------------------------------------------------------------ whole rounds
BatchRound = collections.namedtuple("BatchRound", "name votes validators seed base")
BatchExpect = collections.namedtuple("BatchExpect", "perm t plan staged pre codes verdict hsel apk S")


def _round(name, n, nh, table_of, bad=None, seed=0xBA7C4, base=0x100, first=None):
    """n votes over nh hashes, interleaved round-robin; table_of(i): the vote's key is a validator;
    bad: {vote: replacement}; first: hashes of the leading votes (else i % nh)"""
    votes = []
    for i in range(n):
        k = first[i] if first and i < len(first) else i % nh
        votes.append(good(i, k))
    for i, v in (bad or {}).items():
        votes[i] = v(votes[i]) if callable(v) else v
    # the table: a stranger's key, the chosen votes' keys in reverse, and the first of them again
    vals = [votes[i].pk for i in range(n) if table_of(i)][::-1]
    if vals:
        vals = [bls.g1_compress(g1_mul(0xABCDEF))] + vals + vals[:1]
    t = sum(v.pk in vals for v in votes)
    return BatchRound("%s n=%d G=%d T=%d" % (name, n, len({v.hash for v in votes}), t), tuple(votes), tuple(vals), seed, base)


@functools.lru_cache(maxsize=None)
def batch_rounds():
    g2 = pc.cases()[1]
    off = next(c for c in g2 if c.cls == "off_curve")
    rounds = [
        # 16-lane slices (fewer than VSAME8_MIN votes): every table / bytes split of 9 votes, G = 1, 2
        _round("valid", 5, 1, lambda i: False),
        _round("valid", 9, 2, lambda i: i in (1, 4, 8)),
        _round("valid", 9, 2, lambda i: i != 2, base=(1 << 32) - 4),
        _round("valid", 9, 2, lambda i: True),
        _round("valid", 12, 5, lambda i: i % 2 == 1, base=(1 << 62) + 5),
        # 8-lane slices
        _round("valid", 17, 2, lambda i: i % 3 == 0),
        _round("valid", 40, 3, lambda i: i % 12 in (0, 2, 3, 7)),
        # invalid votes: another signer's signature in the table part and in the bytes part
        _round("two wrong", 9, 2, lambda i: i in (1, 4, 8), bad={4: lambda v: wrong(4, 0), 6: lambda v: wrong(6, 0)}),
        _round("wrong + malformed", 17, 2, lambda i: i % 3 == 0,
               bad={0: lambda v: wrong(0, 0), 16: lambda v: with_sig(off, 0, 16), 5: lambda v: with_key(None, 1, 5)}),
        # hash 0's every vote malformed: the head is hash 1 and hash 0's Miller value goes to its f index
        _round("first hash all malformed", 9, 3, lambda i: i in (0, 5),
               bad={0: lambda v: with_sig(off, 0, 0), 3: lambda v: with_sig(None, 0, 3), 6: lambda v: with_key(None, 0, 6)}),
    ]
    return tuple(rounds)


def batch_expect(rd):
    """the whole path on integers: the staged order, the plan, every vote's code before the
    combined check (pre) and after the batch, the key sum of every hash over the votes with pre = 0,
    S = sum r_i sigma_i over them, the head hash and the verdict"""
    n = len(rd.votes)
    perm, tidx = table_split([v.pk for v in rd.votes], rd.validators)
    pl = plan([v.hash for v in rd.votes], perm)
    staged = [rd.votes[perm[j] if perm else j] for j in range(n)]
    pre = [format_code(v.kcode, v.scode) for v in staged]
    r = [rlc_scalar(msm_cases.vote_scalar(rd.seed, rd.base, j)) for j in range(n)]
    apk, S = [], None
    for m in pl.members:
        a = None
        for j in m:
            if pre[j] == 0:
                a = g1_add(a, bls.pt_mul(F1, staged[j].kpt, r[j]))
        apk.append(a)
    for j in range(n):
        if pre[j] == 0:
            S = bls.pt_add(F2, S, bls.pt_mul(F2, staged[j].spt, r[j]))
    final = [c if c else (0 if v.valid else VERIFY_FAIL) for c, v in zip(pre, staged)]
    verdict = int(any(c == 0 for c in pre) and all(v.valid for c, v in zip(pre, staged) if c == 0))
    hsel = next((g for g, a in enumerate(apk) if a is not None), 0)
    codes = [0] * n
    for j in range(n):
        codes[perm[j] if perm else j] = final[j]
    return BatchExpect(perm or list(range(n)), len(tidx), pl, staged, pre, codes, verdict, hsel, apk, S)


def equation_holds(rd, ex=None, apk=None, hashes=None):
    """prod_g e(apk_g, H_g) * e(-G1, S) == 1 by the reference's Miller loop and plain final power"""
    ex = ex or batch_expect(rd)
    apk = apk or ex.apk
    hashes = hashes or ex.plan.ghash
    pairs = [(a, bls.hash_to_g2(h)) for a, h in zip(apk, hashes) if a is not None]
    if ex.S is not None:
        pairs.append((NG1, ex.S))
    return pcs.pairing3(pairs) == ref.ONE


def same_pairing(f, A, Q):
    """FE_ref(f) == e(A, Q)^3 for the tower value f: one plain power, of f times the conjugate (the
    p^6 Frobenius: the odd part in w negated) of the oracle's Miller value -- FE_ref of a conjugate
    is the inverse, as FE_ref's values lie in the cyclotomic subgroup"""
    m = ref.from_poly(pcs.miller_ref(A, Q))
    conj = (m[0], tuple(((-c[0]) % P, (-c[1]) % P) for c in m[1]))
    return f != pcs.ZERO_T and ref.final_exp(ref.mul(ref.to_poly(f), ref.to_poly(conj))) == ref.ONE


def check_batch(rd, ex, codes, info, perm, ghinf, Pw, fw):
    """what sp_batch read back == the expectation: codes, verdict, hsel, G, T, perm, ghinf, the key
    sums at the heads (under verdict 1), and FE_ref(f_g) = e(apk_g, H_g)^3 for every hash but the head"""
    n, G = len(rd.votes), ex.plan.G
    assert list(info[2:4]) == [G, ex.t] and list(perm) == ex.perm, rd.name + ": staging"
    assert info[0] == ex.verdict, "%s: verdict %d, expected %d" % (rd.name, info[0], ex.verdict)
    assert list(codes) == ex.codes, "%s: codes %s, expected %s" % (rd.name, list(codes), ex.codes)
    assert info[1] == ex.hsel, "%s: hsel %d, expected %d" % (rd.name, info[1], ex.hsel)
    assert list(ghinf[:G]) == [0] * G, rd.name + ": ghinf"
    # the key sums live in the first three f planes of the state slab, which the bisection of a
    # batch with verdict 0 overwrites with its per-vote Miller values
    for g, h in enumerate(ex.plan.head if ex.verdict else ()):
        got = g1_of(Pw[h * G1_W:(h + 1) * G1_W])
        assert pcs.aff1(got) == ex.apk[g] and (ex.apk[g] is not None or got[1] != 0), "%s: key sum of hash %d" % (rd.name, g)
    for g in range(G):
        if g == ex.hsel:
            continue
        f = f12_of(fw[(ex.hsel if g == 0 else g) * F_W:][:F_W])
        if ex.apk[g] is None:
            assert f == pcs.ONE_T, "%s: f of hash %d (key sum O) is not 1" % (rd.name, g)
        else:
            assert same_pairing(f, ex.apk[g], bls.hash_to_g2(ex.plan.ghash[g])), "%s: f of hash %d" % (rd.name, g)


def synth_batch(rd, ex):
    """-> (codes, info, perm, ghinf, P words, f words) a right device would give; f_g = the
    oracle's Miller value"""
    n, G = len(rd.votes), ex.plan.G
    Pw = [0x22222222] * (n * G1_W)
    for g, h in enumerate(ex.plan.head):
        a = ex.apk[g]
        Pw[h * G1_W:(h + 1) * G1_W] = g1_words((0, 9, 0) if a is None else (a[0] * 5 % P, a[1] * 5 % P, 5))
    fw = [POISON] * (G * F_W)
    for g in range(G):
        if g != ex.hsel:
            a = ex.apk[g]
            t = pcs.ONE_T if a is None else ref.from_poly(pcs.miller_ref(a, bls.hash_to_g2(ex.plan.ghash[g])))
            at = ex.hsel if g == 0 else g
            fw[at * F_W:(at + 1) * F_W] = [w for c in ref.flat(t) for w in limbs(c)]
    return list(ex.codes), [ex.verdict, ex.hsel, G, ex.t], list(ex.perm), [0] * G, Pw, fw


def class_counts():
    """{class: count} of everything above, for the records and tests/test_samemsg_cases.py"""
    out = collections.Counter()
    for r in vsame_runs():
        out["vsame " + r.cls] += 1
        out["vsame votes"] += len(r.votes)
    out["keysum cases"] = len(keysum_cases())
    out["keysum entries"] = sum(c.n for c in keysum_cases())
    out["h2g cases"] = len(h2g_cases())
    out["bisect runs"] = len(bisect_runs())
    out["batch rounds"] = len(batch_rounds())
    out["batch rounds valid"] = sum(all(v.valid for v in r.votes) for r in batch_rounds())
    return dict(out)
