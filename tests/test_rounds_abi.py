"""CPU checks of the rounds' boundary (include/ovhip.h: ovh_round_open, ovh_round_add, ovh_round_qc,
ovh_round_close): the four symbols are exported and refuse a NULL context without touching a device
or an output, the header, ffi.rs and the ctypes signatures name them identically and agree on the
two constants, crypto.py exposes ConsensusCrypto.open_round and Round, and the pure-Python model of
a round (tests/round_model.py: qc_model.select folded over the pieces with a running base, the
specification tests/test_gpu_rounds.py compares the device with) equals qc_model.select of the
concatenation -- on seeded random rounds under random cuts and on every cut of a 12-vote list with
duplicates, invalid-then-valid and non-members."""
import ctypes
import itertools
import os
import random
import re

import qc_model
import round_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ovh_round_open", "ovh_round_add", "ovh_round_qc", "ovh_round_close")


def test_the_four_symbols_are_exported():
    from consensus_overlord_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        assert getattr(lib, name) is not None, name


def test_null_context_is_an_argument_error_and_writes_nothing():
    from consensus_overlord_amd import _lib
    lib = _lib.load()
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)   # noqa: E731
    rid = ctypes.c_uint64(0x1234)
    assert lib.ovh_round_open(None, bytes(32), 32, ctypes.byref(rid)) == 103 and rid.value == 0x1234
    codes = (ctypes.c_int32 * 2)(9, 9)
    taken = ctypes.create_string_buffer(b"\x07\x07", 2)
    cnt = ctypes.c_uint32(77)
    out = ctypes.create_string_buffer(b"\xbb" * 96, 96)
    bm = ctypes.create_string_buffer(b"\xcc" * 2, 2)
    assert lib.ovh_round_add(None, 1, 2, bytes(192), bytes(96), p(codes), p(taken), ctypes.byref(cnt), p(out), p(bm),
                             2) == 103
    assert list(codes) == [9, 9] and taken.raw == b"\x07\x07" and cnt.value == 77
    assert out.raw == b"\xbb" * 96 and bm.raw == b"\xcc" * 2
    assert lib.ovh_round_qc(None, 1, p(out), p(bm), 2, ctypes.byref(cnt)) == 103
    assert out.raw == b"\xbb" * 96 and bm.raw == b"\xcc" * 2 and cnt.value == 77
    assert lib.ovh_round_close(None, 1) == 103


def _header_args(hdr, name):
    m = re.search(r"^int %s\(([^;]*)\);" % name, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), flags=re.M)
    assert m, name
    return [re.sub(r"\[\d+\]$", "", a.split()[-1].lstrip("*")) for a in " ".join(m.group(1).split()).split(",")]


def test_names_in_header_ffi_and_binding_and_the_constants():
    from consensus_overlord_amd import _lib, ingress
    from consensus_overlord_amd.crypto import ConsensusCrypto
    hdr = open(os.path.join(ROOT, "include", "ovhip.h")).read()
    ffi = open(os.path.join(ROOT, "overlord-hip", "src", "ffi.rs")).read()
    lib = open(os.path.join(ROOT, "overlord-hip", "src", "lib.rs")).read()
    want = {
        "ovh_round_open": ["ctx", "hash", "hash_len", "round"],
        "ovh_round_add": ["ctx", "round", "n", "sigs", "pks", "codes", "taken", "n_signed", "out_sig", "bitmap",
                          "bitmap_len"],
        "ovh_round_qc": ["ctx", "round", "out_sig", "bitmap", "bitmap_len", "n_signed"],
        "ovh_round_close": ["ctx", "round"],
    }
    for name in NAMES:
        names = _header_args(hdr, name)
        assert names == want[name], name
        f = re.search(r"pub fn %s\((.*?)\) -> i32;" % name, ffi)
        assert f and [a.split(":")[0].strip() for a in f.group(1).split(",")] == names, name
        sig = [a for n, _, a in _lib.SIGNATURES if n == name]
        assert len(sig) == 1 and len(sig[0]) == len(names), name
        assert "ffi::%s(" % name in lib, name
    assert "pub fn open_round(" in lib and "pub struct Round" in lib and "impl Drop for Round" in lib
    rmax = int(re.search(r"#define OVH_ROUNDS_MAX (\d+)", hdr).group(1))
    vmax = re.search(r"#define OVH_ROUND_VOTES_MAX \(1u << (\d+)\)", hdr)
    assert rmax == 16 == ConsensusCrypto.ROUNDS_MAX == ingress.ROUNDS_MAX
    assert vmax and 1 << int(vmax.group(1)) == 1 << 24 == ConsensusCrypto.ROUND_VOTES_MAX
    assert re.search(r"pub const OVH_ROUNDS_MAX: usize = %d;" % rmax, ffi)
    assert re.search(r"pub const OVH_ROUND_VOTES_MAX: usize = 1 << %s;" % vmax.group(1), ffi)
    # the header states the defining property and what a refused call leaves behind
    text = " ".join(hdr.replace("*", " ").split())
    assert "any cut of V into consecutive pieces" in text
    assert "A refused call changes nothing" in text


def test_crypto_exposes_open_round_and_round():
    from consensus_overlord_amd import crypto
    assert callable(crypto.ConsensusCrypto.open_round)
    for name in ("add", "add_raw", "qc", "qc_raw", "close", "__enter__", "__exit__"):
        assert callable(getattr(crypto.Round, name)), name


# ------------------------------------------------------------------------------ the model
K = [bytes([b]) * 48 for b in (0x50, 0x10, 0x30, 0x20, 0x40, 0x60)]   # config order
OUT = [bytes([0x99]) * 48, bytes([0x98]) * 48]                          # not validators


def _cuts(n):
    """every cut of n votes into consecutive non-empty pieces (2^(n-1) of them)"""
    for marks in itertools.product((0, 1), repeat=n - 1):
        cut, run = [], 1
        for m in marks:
            if m:
                cut.append(run)
                run = 1
            else:
                run += 1
        yield cut + [run]


def _same_as_one_shot(codes, voters, table, cut):
    want = qc_model.select(codes, voters, table)
    taken, bitmap, cnt, steps = round_model.fold(codes, voters, table, cut)
    assert (taken, bitmap, cnt) == want, cut
    lo = 0
    for k, (bm, c) in zip(cut, steps):   # after every add: the one-shot rule over the prefix
        lo += k
        assert (bm, c) == qc_model.select(codes[:lo], voters[:lo], table)[1:], (cut, lo)


def test_model_every_cut_of_a_12_vote_list():
    # K[1] twice (exact duplicate), K[2] invalid then valid, K[3] valid then invalid, two outsiders
    # (one twice), K[4] with code 102, K[0] valid once, K[5] never valid
    voters = [K[1], K[2], OUT[0], K[1], K[3], K[2], K[4], OUT[1], K[3], K[0], OUT[0], K[5]]
    codes = [0, 5, 0, 0, 0, 0, 102, 0, 3, 0, 0, 5]
    assert qc_model.select(codes, voters, K)[0] == [1, 0, 0, 0, 1, 1, 0, 0, 0, 1, 0, 0]
    n = 0
    for cut in _cuts(12):
        _same_as_one_shot(codes, voters, K, cut)
        n += 1
    assert n == 2048


def test_model_seeded_random_rounds_and_cuts():
    rng = random.Random(0x524F554E)
    for _ in range(200):
        tn = rng.randrange(1, 40)
        table = [rng.randbytes(48) for _ in range(tn)]
        if tn > 3 and rng.random() < 0.3:
            table[rng.randrange(tn)] = table[0]          # a key listed twice
        pool = table + [rng.randbytes(48) for _ in range(3)]
        n = rng.randrange(1, 90)
        voters = [rng.choice(pool) for _ in range(n)]
        codes = [rng.choice((0, 0, 0, 5, 3, 102)) for _ in range(n)]
        for _ in range(4):
            cut, left = [], n
            while left:
                k = rng.randrange(1, left + 1) if rng.random() < 0.5 else 1
                cut.append(k)
                left -= k
            _same_as_one_shot(codes, voters, table, cut)


def test_model_invalid_first_vote_does_not_block_a_later_add():
    m = round_model.RoundModel(K)
    assert m.add([5], [K[2]]) == ([0], bytes(1), 0)
    assert m.add([0, 0], [K[2], K[2]]) == ([1, 0], bytes([0b00100000]), 1)     # K[2] is rank 2
    assert m.add([0], [K[2]]) == ([0], bytes([0b00100000]), 1)                 # held by the earlier add
    assert m.base == 4
