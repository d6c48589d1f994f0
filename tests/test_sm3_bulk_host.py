"""The bulk SM3 core (consensus_overlord_amd/csrc/sm3_bulk.hpp) and the strict Proof decoder
(csrc/proof.hpp) compiled for the host with g++ (tests/host/sm3_bulk_harness.cpp): the digests
against hashlib's SM3 and the GB/T 32905 vectors at every alignment, the decoder against
vote.decode_proof. Test-only build: it is never linked into the product."""
import ctypes
import hashlib
import os
import random
import subprocess

import pytest

from consensus_overlord_amd import vote

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# block boundaries (55/56: one or two padded blocks; 63/64/65; the same one block later), the
# empty message, sub-word tails, and lengths of many blocks
LENGTHS = [0, 1, 3, 4, 5, 55, 56, 57, 63, 64, 65, 119, 120, 121, 127, 128, 129, 191, 192, 1000, 4097]


def sm3(b):
    return hashlib.new("sm3", bytes(b)).digest()


def message(n, salt=0):
    return random.Random(0x5A3 + 131 * n + salt).randbytes(n)


@pytest.fixture(scope="module")
def hx():
    out = os.path.join(ROOT, "tests", "host", "_build", "libhxsm3b.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    # built under a per-process name and renamed into place: parallel workers (pytest -n) never
    # load a half-written library
    tmp = "%s.%d" % (out, os.getpid())
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", tmp,
                           os.path.join(ROOT, "tests", "host", "sm3_bulk_harness.cpp")])
    os.replace(tmp, out)
    lib = ctypes.CDLL(out)
    lib.hxb_sm3_at.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint, ctypes.c_char_p]
    lib.hxb_sm3_batch.argtypes = [ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint,
                                  ctypes.c_char_p]
    lib.hxb_decode_proof.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def digest_at(hx, msg, shift):
    out = ctypes.create_string_buffer(32)
    assert hx.hxb_sm3_at(msg, len(msg), shift, out) == 0
    return out.raw


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_lengths_at_every_alignment(hx, shift):
    for n in LENGTHS:
        m = message(n)
        assert digest_at(hx, m, shift) == sm3(m), (n, shift)


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_standard_vectors(hx, shift):
    assert digest_at(hx, b"abc", shift).hex() == "66c7f0f462eeedd9d1f2d46bdc10e4e24167c4875cf2f7a2297da02b8f4ba8e0"
    assert digest_at(hx, b"abcd" * 16, shift).hex() == (
        "debe9ff92275b8a138604889c18e5a4d6fdb70e5387e5765293dcba39c0c5732")


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_batch_items_and_reversed_offsets(hx, shift):
    """The kernel's per-message step: neighbours packed back to back (a byte of the next message
    shares a word with the last byte of this one), and an end below its start."""
    msgs = [message(n, 7) for n in LENGTHS]
    data = b"".join(msgs)
    off = [0]
    for m in msgs:
        off.append(off[-1] + len(m))
    arr = (ctypes.c_uint64 * len(off))(*off)
    out = ctypes.create_string_buffer(32 * len(msgs))
    assert hx.hxb_sm3_batch(len(msgs), data, len(data), arr, shift, out) == 0
    assert [out.raw[32 * i:32 * i + 32] for i in range(len(msgs))] == [sm3(m) for m in msgs]
    # entry 1 ends below its start: the zero digest; entry 0 and 2 as their offsets say
    arr = (ctypes.c_uint64 * 4)(0, 200, 100, 300)
    out = ctypes.create_string_buffer(96)
    assert hx.hxb_sm3_batch(3, data, len(data), arr, shift, out) == 0
    assert out.raw == sm3(data[:200]) + bytes(32) + sm3(data[100:300])


# ---- csrc/proof.hpp against vote.decode_proof ----

def decode(hx, p):
    hr = (ctypes.c_uint64 * 2)()
    sp = (ctypes.c_uint64 * 6)()
    if not hx.hxb_decode_proof(bytes(p), len(p), hr, sp):
        return None
    return (int(hr[0]), int(hr[1])) + tuple(bytes(p[sp[2 * k]:sp[2 * k] + sp[2 * k + 1]]) for k in range(3))


# the malformed inputs of tests/test_check_block.py::test_decode_proof_rejects_malformed
MALFORMED = [
    b"", b"\xc0", b"\x80", b"\xc4\x01\x02\x03\x04",
    bytes.fromhex("c701020380c2c0c0"),
    bytes.fromhex("c8820001028080c28080"),
    bytes.fromhex("cc890102030405060708090280c28080"),
    bytes.fromhex("c6010280c28080") + b"\x00",
    bytes.fromhex("c7010280c28080"),
    bytes.fromhex("c6010280c2817f"),
]


@pytest.mark.parametrize("bad", MALFORMED)
def test_proof_decoder_rejects_malformed(hx, bad):
    with pytest.raises(ValueError):
        vote.decode_proof(bad)
    assert decode(hx, bad) is None


def test_proof_decoder_round_trips(hx):
    rng = random.Random(0xB10C)
    for _ in range(200):
        h, r = rng.getrandbits(rng.choice((0, 8, 32, 64))), rng.getrandbits(rng.choice((0, 7, 16)))
        bh = bytes(rng.randrange(256) for _ in range(rng.choice((0, 1, 32, 55, 56, 64))))
        sig = bytes(rng.randrange(256) for _ in range(rng.choice((0, 1, 96, 300))))
        bm = bytes(rng.randrange(256) for _ in range(rng.choice((0, 1, 13, 60))))
        p = vote.encode_proof(h, r, bh, sig, bm)
        assert decode(hx, p) == (h, r, bh, sig, bm) == vote.decode_proof(p)
        # every strict prefix and a trailing byte are refused by both
        cut = p[:rng.randrange(len(p))]
        assert decode(hx, cut) is None and decode(hx, p + b"\x00") is None
        with pytest.raises(ValueError):
            vote.decode_proof(cut)


def test_proof_decoder_agrees_on_mutations(hx):
    """Single-byte mutations of a valid proof: the C++ decoder accepts exactly what
    vote.decode_proof accepts, with the same fields."""
    rng = random.Random(0xDEC0DE)
    p0 = vote.encode_proof(1 << 40, 3, bytes(range(32)), bytes(range(96)), bytes(13))
    for _ in range(400):
        p = bytearray(p0)
        p[rng.randrange(8) if rng.random() < 0.5 else rng.randrange(len(p))] = rng.randrange(256)
        try:
            want = vote.decode_proof(bytes(p))
        except ValueError:
            want = None
        assert decode(hx, bytes(p)) == want, bytes(p).hex()
