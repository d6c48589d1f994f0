"""GPU parity of priming (include/ovhip.h ovh_prime_hashes): H = hash_to_G2(hash) enqueued ahead
of use on a side stream, then consumed by the per-call verify (a message-cache hit on the first
vote), by ovh_sign (program signg0h) and by small batches whose hashes are all cached (k_vm_votewh,
programs votewh / votewh_t). Expected values come from the C oracle (orc) and the golden
fixtures; the library's own unprimed route is a second reference, never the only one."""
import ctypes
import hashlib
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def _b(h):
    return bytes.fromhex(h)


def _pstats(ctx):
    from consensus_overlord_amd import _lib
    st = (ctypes.c_uint64 * 4)()
    assert _lib.load().ovh_prime_stats(ctx.ptr, st) == 0
    return tuple(int(x) for x in st)


def _mstats(ctx):
    from consensus_overlord_amd import _lib
    st = (ctypes.c_uint64 * 2)()
    assert _lib.load().ovh_msg_cache_stats(ctx.ptr, st) == 0
    return int(st[0]), int(st[1])


def _prime(ctx, hashes):
    from consensus_overlord_amd import _lib
    hs = [bytes(h) for h in hashes]
    return _lib.load().ovh_prime_hashes(ctx.ptr, len(hs), b"".join(hs))


def _sign(ctx, key, h):
    from consensus_overlord_amd import _lib
    out = ctypes.create_string_buffer(96)
    assert _lib.load().ovh_sign(ctx.ptr, key, len(key), h, len(h), out) == 0
    return out.raw


def _verify(ctx, sig, h, pk):
    from consensus_overlord_amd import _lib
    return _lib.load().ovh_verify(ctx.ptr, sig, len(sig), h, len(h), pk, len(pk))


def _batch(ctx, votes):
    """ovh_verify_batch of (sig, hash, pk) triples -> list of codes."""
    from consensus_overlord_amd import _lib
    n = len(votes)
    codes = (ctypes.c_int32 * n)(*([-1] * n))
    r = _lib.load().ovh_verify_batch(ctx.ptr, n, b"".join(v[0] for v in votes), b"".join(v[1] for v in votes),
                                     b"".join(v[2] for v in votes), ctypes.cast(codes, ctypes.c_void_p))
    assert r == 0
    return list(codes)


def _set_table(ctx, keys):
    from consensus_overlord_amd import _lib
    assert _lib.load().ovh_set_validators(ctx.ptr, b"".join(keys), len(keys)) == 0


@pytest.fixture(scope="module")
def ctxs():
    """(primed, unprimed) contexts taking raw scalars, and (primed, unprimed) taking KeyGen keys."""
    from consensus_overlord_amd.crypto import FLAG_SK_RAW, Context
    return Context(flags=FLAG_SK_RAW), Context(flags=FLAG_SK_RAW), Context(), Context()


@pytest.fixture(scope="module")
def pool(golden):
    """Votes over two hashes A, B with their oracle codes, computed once: the eight golden keys'
    valid signatures on both hashes (orc.sign), every fixed-size golden negative on A or B, and a
    valid signature presented under the other hash."""
    import orc
    A, B = _b(golden["votes"][0]["digest"]), _b(golden["votes"][1]["digest"])
    pks = [_b(k["pk"]) for k in golden["keys"]]
    valid = {}
    for h in (A, B):
        for j, k in enumerate(golden["keys"]):
            c, s = orc.sign(_b(k["sk"]), h)
            assert c == 0
            valid[(h, j)] = (s, h, pks[j])
    neg = [(_b(c["sig"]), _b(c["hash"]), _b(c["pk"])) for c in golden["verify"]
           if c["code"] != 0 and len(c["sig"]) == 192 and len(c["pk"]) == 96 and _b(c["hash"]) in (A, B)]
    names = {c["name"] for c in golden["verify"] if c["code"] != 0 and _b(c["hash"]) in (A, B)}
    # bad encoding, off curve, outside the group, infinity key, unparsable key
    assert {"sig_compressed_bit_clear", "sig_not_on_curve", "sig_not_in_g2", "pk_not_in_g1", "pk_infinity",
            "pk_not_on_curve", "sig_infinity"} <= names
    other = (valid[(A, 2)][0], B, pks[2])   # valid under A, presented under B
    want = {}
    for v in list(valid.values()) + neg + [other]:
        want[v] = orc.verify(*v)
    assert want[other] == 5 and all(want[v] == 0 for v in valid.values()) and all(want[v] != 0 for v in neg)
    return {"A": A, "B": B, "pks": pks, "valid": valid, "neg": neg, "other": other, "want": want}


def _votes(pool, n):
    """n votes over A and B: a valid one on A, the valid-under-the-other-hash one, a valid one on
    B, then every golden negative that fits, then valid votes on alternating hashes."""
    A, B, valid = pool["A"], pool["B"], pool["valid"]
    out = [valid[(A, 0)], pool["other"], valid[(B, 1)]][:n]
    out += pool["neg"][:max(0, n - len(out))]
    j = 0
    while len(out) < n:
        out.append(valid[((A, B)[j & 1], (3 + j) % 8)])
        j += 1
    return out


def test_prime_then_per_call_verify(ctxs, golden):
    ctx = ctxs[0]
    v, k = golden["votes"], golden["keys"]
    h = _b(v[3]["digest"])
    p0, m0 = _pstats(ctx), _mstats(ctx)
    assert _prime(ctx, [h]) == 0
    assert _verify(ctx, _b(v[3]["sig"]), h, _b(k[3]["pk"])) == 0
    m1 = _mstats(ctx)
    assert (m1[0] - m0[0], m1[1] - m0[1]) == (1, 0)
    assert _verify(ctx, _b(v[4]["sig"]), h, _b(k[3]["pk"])) == 5
    p1 = _pstats(ctx)
    assert (p1[0] - p0[0], p1[1] - p0[1]) == (1, 0)
    assert _prime(ctx, [h, h]) == 0
    p2 = _pstats(ctx)
    assert p2[0] == p1[0] and p2[1] == p1[1] + 2
    # argument errors enqueue nothing
    assert _prime(ctx, []) == 0
    from consensus_overlord_amd import _lib
    assert _lib.load().ovh_prime_hashes(ctx.ptr, 65, bytes(65 * 32)) == 103
    assert _lib.load().ovh_prime_hashes(ctx.ptr, 1, None) == 103
    assert _pstats(ctx) == p2


def test_primed_sign_bytes(ctxs, golden):
    import orc
    rp, ru, kp, ku = ctxs
    h = hashlib.sha256(b"primed sign").digest()
    h2 = hashlib.sha256(b"unprimed sign").digest()
    raw = [_b(k["sk"]) for k in golden["keys"]] + [(1).to_bytes(32, "big"), (R_ORDER - 1).to_bytes(32, "big")]
    ikm = bytes(range(7, 47))
    c, scalar = orc.sk_keygen(ikm)
    assert c == 0
    for ctx_p, ctx_u, keys, scal in ((rp, ru, raw, raw), (kp, ku, [ikm], [scalar])):
        p0 = _pstats(ctx_p)
        assert _prime(ctx_p, [h]) == 0
        for key, sc in zip(keys, scal):
            want = orc.sign(sc, h)
            assert want[0] == 0
            assert _sign(ctx_p, key, h) == want[1] == _sign(ctx_u, key, h)
        p1 = _pstats(ctx_p)
        assert p1[2] - p0[2] == len(keys)
        # an unprimed hash: the old route, no counter moves (sign never inserts)
        m1 = _mstats(ctx_p)
        assert _sign(ctx_p, keys[0], h2) == orc.sign(scal[0], h2)[1]
        assert _pstats(ctx_p) == p1 and _mstats(ctx_p) == m1
        assert _pstats(ctx_u)[2] == 0


@pytest.mark.parametrize("layout", ["none", "all", "mixed", "mixed_single"])
def test_small_batches_on_primed_hashes(ctxs, pool, layout):
    """n in {2, 3, 5, 67} over two primed hashes, per key layout: codes == the oracle's per vote ==
    an unprimed context's; stats[3] rises by the parts routed, and by 0 with one hash unprimed."""
    from consensus_overlord_amd.crypto import Context
    cp, cu = Context(), ctxs[3]
    A, B, want = pool["A"], pool["B"], pool["want"]
    try:
        assert _prime(cp, [A, B]) == 0
        for n in (2, 3, 5, 67):
            votes = _votes(pool, n)
            keys = list(dict.fromkeys(v[2] for v in votes))
            if layout == "none":
                table = []
            elif layout == "all":
                table = keys
            elif layout == "mixed":
                table = keys[::2]
            else:   # the non-table part is a single vote: its key appears once
                once = [k for k in keys if sum(v[2] == k for v in votes) == 1]
                table = [k for k in keys if k != once[-1]]
            for c in (cp, cu):
                _set_table(c, table)
            nt = sum(v[2] in table for v in votes)
            parts = sum(1 for cnt in (nt, n - nt) if cnt >= 2)
            if layout == "mixed_single":
                assert n - nt == 1
            p0 = _pstats(cp)
            got = _batch(cp, votes)
            assert got == [want[v] for v in votes], (layout, n)
            assert got == _batch(cu, votes), (layout, n)
            assert _pstats(cp)[3] - p0[3] == parts, (layout, n)
        # one hash left unprimed (a fresh context primes A only): no part is routed, same codes
        c1 = Context()
        try:
            _set_table(c1, table)
            assert _prime(c1, [A]) == 0
            votes = _votes(pool, 67)
            assert _batch(c1, votes) == [want[v] for v in votes]
            assert _pstats(c1)[3] == 0
        finally:
            c1.close()
    finally:
        _set_table(cu, [])
        cp.close()


def test_no_host_wait_between_prime_and_use(pool, golden):
    """ovh_prime_hashes followed at once by ovh_sign and ovh_verify_batch on the same hashes,
    from the same thread: the device-side ordering alone makes the results right."""
    import orc
    from consensus_overlord_amd.crypto import FLAG_SK_RAW, Context
    ctx = Context(flags=FLAG_SK_RAW)
    try:
        A, B, want = pool["A"], pool["B"], pool["want"]
        sk = _b(golden["keys"][5]["sk"])
        assert _prime(ctx, [A, B]) == 0
        sig = _sign(ctx, sk, A)
        votes = _votes(pool, 5)
        got = _batch(ctx, votes)
        assert sig == orc.sign(sk, A)[1]
        assert got == [want[v] for v in votes]
        st = _pstats(ctx)
        assert st[0] == 2 and st[2] == 1 and st[3] == 1
    finally:
        ctx.close()


def test_eviction(golden):
    """256 + 8 hashes primed in calls of at most 64: the first 8 were evicted (sign and a 2-vote
    batch take the old route), the last 8 are cached (the primed route); both are correct."""
    import orc
    from consensus_overlord_amd.crypto import FLAG_SK_RAW, Context
    ctx = Context(flags=FLAG_SK_RAW)
    try:
        hs = [hashlib.sha256(b"evict %d" % i).digest() for i in range(264)]
        for k in range(0, 264, 64):
            assert _prime(ctx, hs[k:k + 64]) == 0
        assert _pstats(ctx)[:2] == (264, 0)
        sks = [_b(k["sk"]) for k in golden["keys"][:2]]
        pks = [_b(k["pk"]) for k in golden["keys"][:2]]
        for idx, primed in ((range(0, 8), 0), (range(256, 264), 1)):
            for i in idx:
                p0 = _pstats(ctx)
                sig = _sign(ctx, sks[0], hs[i])
                assert sig == orc.sign(sks[0], hs[i])[1]
                sig1 = orc.sign(sks[1], hs[i])[1]
                assert _batch(ctx, [(sig, hs[i], pks[0]), (sig, hs[i], pks[1])]) == [0, 5]
                assert _batch(ctx, [(sig, hs[i], pks[0]), (sig1, hs[i], pks[1])]) == [0, 0]
                p1 = _pstats(ctx)
                assert (p1[2] - p0[2], p1[3] - p0[3]) == (primed, 2 * primed), i
    finally:
        ctx.close()


def test_two_threads_on_one_context(pool, golden):
    """One thread primes fresh hashes while the other runs per-call verifies and small batches on
    other hashes; afterwards batches on the first thread's hashes take the primed route."""
    import orc
    from consensus_overlord_amd.crypto import Context
    ctx = Context()
    try:
        fresh = [hashlib.sha256(b"thread %d" % i).digest() for i in range(24)]
        v, k = golden["votes"], golden["keys"]
        want = pool["want"]
        votes = _votes(pool, 5)
        err = []

        def primer():
            try:
                for j in range(0, 24, 4):
                    assert _prime(ctx, fresh[j:j + 4]) == 0
            except BaseException as e:   # noqa: BLE001
                err.append(e)

        def verifier():
            try:
                for j in range(6):
                    assert _verify(ctx, _b(v[j]["sig"]), _b(v[j]["digest"]), _b(k[j]["pk"])) == 0
                    assert _batch(ctx, votes) == [want[x] for x in votes]
            except BaseException as e:   # noqa: BLE001
                err.append(e)

        ts = [threading.Thread(target=primer), threading.Thread(target=verifier)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(60)
            assert not t.is_alive()
        assert not err, err
        sk, pk = _b(k[6]["sk"]), _b(k[6]["pk"])
        p0 = _pstats(ctx)
        assert p0[0] == 24
        for h in (fresh[0], fresh[23]):
            good, bad = orc.sign(sk, h)[1], orc.sign(_b(k[7]["sk"]), h)[1]
            assert _batch(ctx, [(good, h, pk), (bad, h, pk), (good, h, pk)]) == [0, 5, 0]
        assert _pstats(ctx)[3] - p0[3] == 2
    finally:
        ctx.close()


def test_multi_device_context_primes_every_device(golden):
    """ovh_create_multi over {0, 0}: one prime call, two per-call verifies (one per sub-context,
    pick_sub rotates) report 2 hits and 0 misses."""
    from consensus_overlord_amd.crypto import Context
    ctx = Context(devices=[0, 0])
    try:
        v, k = golden["votes"][2], golden["keys"][2]
        h = _b(v["digest"])
        assert _prime(ctx, [h]) == 0
        assert _pstats(ctx)[:2] == (2, 0)
        for _ in range(2):
            assert _verify(ctx, _b(v["sig"]), h, _b(k["pk"])) == 0
        assert _mstats(ctx) == (2, 0)
    finally:
        ctx.close()


def test_vote_ingress_round_takes_the_primed_route():
    """A VoteIngress round of 67 validators over a real ConsensusCrypto with two bad signatures:
    the shim primes the round's hash on the first vote, the flush's parts run on cached H, and
    every forwarded message's verify_signature is a verdict-cache hit with the oracle's code."""
    import orc
    import consensus_overlord_amd as coa
    from consensus_overlord_amd import ingress as ing
    from consensus_overlord_amd import vote as _v
    from consensus_overlord_amd.crypto import CryptoErr
    nval = 67
    sks = [(1000 + i).to_bytes(32, "big") for i in range(nval)]
    pks = [orc.sk_to_pk(s)[1] for s in sks]
    cc = coa.ConsensusCrypto(bytes.fromhex("6b" * 32))
    cc.update_pubkeys(pks)
    bh = cc.hash(b"block 9")
    d = cc.hash(_v.rlp_vote(9, 0, _v.PREVOTE, bh))
    bad = {5, 40}
    msgs = []
    for i in range(nval):
        sig = orc.sign(sks[(i + 1) % nval] if i in bad else sks[i], d)[1]
        msgs.append(ing.encode_signed_vote(ing.SignedVote(sig, 9, 0, _v.PREVOTE, bh, pks[i])))
    out = []
    vi = ing.VoteIngress(cc, lambda kind, m: out.append((kind, m)), batch_size=nval)
    p0 = cc.prime_stats()
    for m in msgs:
        vi.proc_network_msg(ing.SIGNED_VOTE, m)
    assert vi.stats["batches"] == 1 and len(out) == nval
    p1 = cc.prime_stats()
    assert p1[0] - p0[0] == 1 and p1[3] - p0[3] >= 1
    c0 = cc.cache_stats()
    for i, (kind, m) in enumerate(out):
        want = orc.verify(m.signature, d, m.voter)
        assert want == (5 if i in bad else 0)
        try:
            ing.overlord_verify(cc, kind, m)
            got = 0
        except CryptoErr as e:
            got = e.code
        assert got == want, i
    c1 = cc.cache_stats()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (nval, 0)
