"""Crafted inputs for the tests of the signature-point cache and of the table route of
ovh_verify_aggregated. Everything is made on the CPU with the C oracle
(orc.sign / orc.sk_to_pk over raw scalars) and the Python curve code, so the GPU tests compare the
library with bytes it had no part in; tests/test_agg_cases.py confirms against the oracle that the
cases are what they claim.

    validators(n)      n (scalar bytes, pk) pairs, deterministic
    votes(digest, n)   their signatures on one digest
    interleaved(...)   8 table voters and 3 voters outside the table in one call, outsiders first,
                       in the middle and last, so the staged (table-first) order differs from the
                       caller's
    mirror_pair        keys sk and r - sk: sigma + (-sigma) = O, pk + (-pk) = O
    doubled            one signature twice: 2 sigma
    outside_g1_key     the golden key on the curve and outside G1
    unparsable_key     the golden key with x = p
"""
import functools
import hashlib
import json
import os

import bls12_381 as bls
import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = b"agg cases v1 "
TABLE_N = 8
OUTSIDERS = 3
COUNTS = (1, 2, 3, 64, 65, 129)      # k_qc_chunk / k_qc_apk boundaries
IDENTITY_G2 = bytes([0xC0]) + bytes(95)


def sha(b: bytes) -> bytes:
    return hashlib.sha256(b).digest()


def scalar(i: int) -> int:
    return int.from_bytes(sha(SEED + b"%d" % i), "big") % (bls.R - 1) + 1


def _pair(s: int):
    skb = s.to_bytes(32, "big")
    code, pk = orc.sk_to_pk(skb)
    assert code == 0
    return skb, pk


@functools.lru_cache(maxsize=None)
def validators(n: int, lo: int = 0):
    return tuple(_pair(scalar(lo + i)) for i in range(n))


def sign(skb: bytes, digest: bytes) -> bytes:
    code, sig = orc.sign(skb, digest)
    assert code == 0
    return sig


@functools.lru_cache(maxsize=None)
def votes(digest: bytes, n: int, lo: int = 0):
    """-> ((sig, pk), ...) of validators(n, lo) on digest"""
    return tuple((sign(skb, digest), pk) for skb, pk in validators(n, lo))


@functools.lru_cache(maxsize=None)
def interleaved(digest: bytes):
    """-> (votes in the caller's order, table): 11 votes, 8 of table voters; the outsiders stand
    first, in the middle and last"""
    tv = votes(digest, TABLE_N)
    ov = votes(digest, OUTSIDERS, lo=1000)
    order = [ov[0], tv[0], tv[1], tv[2], ov[1], tv[3], tv[4], tv[5], tv[6], tv[7], ov[2]]
    return tuple(order), tuple(pk for _, pk in tv)


@functools.lru_cache(maxsize=None)
def mirror_pair(digest: bytes):
    """-> ((sig, pk), (sig', pk')) for the secrets sk and r - sk"""
    s = scalar(7000)
    a, b = _pair(s), _pair(bls.R - s)
    return (sign(a[0], digest), a[1]), (sign(b[0], digest), b[1])


def doubled(digest: bytes):
    """-> ([sig, sig], [pk, pk], 2 sigma compressed by the Python curve code)"""
    sig, pk = votes(digest, 1)[0]
    two = bls.pt_mul(bls.Fp2Ops, bls.g2_from_bytes(sig), 2)
    return [sig, sig], [pk, pk], bls.g2_compress(two)


@functools.lru_cache(maxsize=None)
def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "golden_v1.json")) as fh:
        return json.load(fh)


def golden_verify(name: str) -> dict:
    return {k: (bytes.fromhex(v) if isinstance(v, str) and k != "name" else v)
            for k, v in next(c for c in _golden()["verify"] if c["name"] == name).items()}


def outside_g1_key() -> bytes:
    return golden_verify("pk_not_in_g1")["pk"]


def unparsable_key() -> bytes:
    return golden_verify("pk_x_eq_p")["pk"]


def edge_signatures():
    """-> {name: 96 bytes}: bad encoding, off the curve, outside G2 (the golden file's)"""
    return {"bad_encoding": golden_verify("sig_x1_eq_p")["sig"],
            "off_curve": golden_verify("sig_not_on_curve")["sig"],
            "outside_g2": golden_verify("sig_not_in_g2")["sig"]}


def uncompressed(sig: bytes) -> bytes:
    """the 192-byte encoding of a compressed signature's point"""
    return bls.g2_serialize(bls.g2_from_bytes(sig))
