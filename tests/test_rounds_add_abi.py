"""CPU checks of ovh_rounds_add's boundary (include/ovhip.h): the symbol is exported and refuses a
NULL context without touching a device or an output; the header, ffi.rs and the ctypes signature
name its arguments identically; lib.rs calls it; the header states the defining property and what a
refused call leaves behind; crypto.py exposes add_rounds. Then the model of a multi-round call
(tests/rounds_model.py: one round_model.RoundModel per round, each fed the sub-list of its votes):
on seeded random labelled vote lists cut into random calls every round equals qc_model.select of
the concatenation of its votes, and two rounds on one hash stay apart."""
import ctypes
import os
import random
import re

import qc_model
import rounds_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ovh_rounds_add"
ARGS = ["ctx", "n", "sigs", "rounds", "pks", "codes", "taken", "slot", "max_rounds", "n_rounds", "round_ids", "n_signed",
        "out_sigs", "bitmaps", "bitmap_len"]


def test_the_symbol_is_exported():
    from consensus_overlord_amd import _lib
    assert getattr(_lib.load(), NAME) is not None


def test_null_context_is_an_argument_error_and_writes_nothing():
    from consensus_overlord_amd import _lib
    lib = _lib.load()
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)   # noqa: E731
    ids = (ctypes.c_uint64 * 2)(1, 2)
    codes = (ctypes.c_int32 * 2)(9, 9)
    taken = ctypes.create_string_buffer(b"\x07\x07", 2)
    slot = (ctypes.c_uint32 * 2)(55, 55)
    nr = ctypes.c_uint32(77)
    rid = (ctypes.c_uint64 * 2)(0x1234, 0x1234)
    cnt = (ctypes.c_uint32 * 2)(66, 66)
    out = ctypes.create_string_buffer(b"\xbb" * 192, 192)
    bm = ctypes.create_string_buffer(b"\xcc" * 4, 4)
    assert lib.ovh_rounds_add(None, 2, bytes(192), p(ids), bytes(96), p(codes), p(taken), p(slot), 2, ctypes.byref(nr),
                              p(rid), p(cnt), p(out), p(bm), 2) == 103
    assert list(codes) == [9, 9] and taken.raw == b"\x07\x07" and list(slot) == [55, 55] and nr.value == 77
    assert list(rid) == [0x1234] * 2 and list(cnt) == [66, 66] and out.raw == b"\xbb" * 192 and bm.raw == b"\xcc" * 4


def _header_args(hdr, name):
    m = re.search(r"^int %s\(([^;]*)\);" % name, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), flags=re.M)
    assert m, name
    return [re.sub(r"\[\d+\]$", "", a.split()[-1].lstrip("*")) for a in " ".join(m.group(1).split()).split(",")]


def test_names_in_header_ffi_binding_and_crate():
    from consensus_overlord_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ovhip.h")).read()
    ffi = open(os.path.join(ROOT, "overlord-hip", "src", "ffi.rs")).read()
    lib = open(os.path.join(ROOT, "overlord-hip", "src", "lib.rs")).read()
    assert _header_args(hdr, NAME) == ARGS
    f = re.search(r"pub fn %s\((.*?)\) -> i32;" % NAME, ffi)
    assert f and [a.split(":")[0].strip() for a in f.group(1).split(",")] == ARGS
    sig = [a for n, _, a in _lib.SIGNATURES if n == NAME]
    assert len(sig) == 1 and len(sig[0]) == len(ARGS)
    assert "ffi::%s(" % NAME in lib and "pub fn rounds_add(" in lib
    # the header states the defining property, the routes and what a refused call leaves behind
    text = " ".join(hdr.replace("*", " ").split())
    doc = text[text.index("A flush's votes added to several open rounds"):text.index("int ovh_rounds_add(")]
    assert "would have written in its place" in doc
    assert "ovh_build_qc over the concatenation of that round's votes" in doc
    assert "is taken in both" in doc
    assert "A refused call changes nothing" in doc
    assert "OVH_SMALL_MAX" in doc and "same-message route" in doc and "is ovh_round_add itself" in doc


def test_crypto_and_ingress_expose_the_call():
    from consensus_overlord_amd import crypto, ingress
    assert callable(crypto.ConsensusCrypto.add_rounds) and callable(crypto.ConsensusCrypto.add_rounds_raw)
    sh = ingress.VoteIngress(type("C", (), {"open_round": None})(), lambda k, m: None, rounds=True)
    assert sh.stats["round_passes"] == 0
    assert "round_passes" not in ingress.VoteIngress(object(), lambda k, m: None).stats


# ------------------------------------------------------------------------------ the model
def _check(rng, n_rounds, same_hash=False):
    tn = rng.randrange(1, 30)
    table = [rng.randbytes(48) for _ in range(tn)]
    if tn > 3 and rng.random() < 0.3:
        table[rng.randrange(tn)] = table[0]          # a key listed twice
    pool = table + [rng.randbytes(48) for _ in range(2)]
    n = rng.randrange(1, 120)
    rids = [rng.randrange(n_rounds) for _ in range(n)]
    voters = [rng.choice(pool) for _ in range(n)]
    codes = [rng.choice((0, 0, 0, 5, 3, 102)) for _ in range(n)]
    m = rounds_model.RoundsModel(table)
    for r in range(n_rounds):
        m.open(r)
    taken, lo = [], 0
    last = {}
    while lo < n:
        k = rng.randrange(1, n - lo + 1) if rng.random() < 0.5 else 1
        t, slot, per_round = m.add(rids[lo:lo + k], codes[lo:lo + k], voters[lo:lo + k])
        # numbered by first appearance in the call
        seen = []
        for r in rids[lo:lo + k]:
            if r not in seen:
                seen.append(r)
        assert [r for r, _, _ in per_round] == seen and slot == [seen.index(r) for r in rids[lo:lo + k]]
        taken += t
        lo += k
        for r, bitmap, cnt in per_round:
            last[r] = (bitmap, cnt)
            # after every call: the one-shot rule over the round's prefix
            idx = [i for i in range(lo) if rids[i] == r]
            assert (bitmap, cnt) == qc_model.select([codes[i] for i in idx], [voters[i] for i in idx], table)[1:]
    for r in set(rids):
        idx = [i for i in range(n) if rids[i] == r]
        want = qc_model.select([codes[i] for i in idx], [voters[i] for i in idx], table)
        assert ([taken[i] for i in idx], ) + last[r] == want, r
        assert m.rounds[r].base == len(idx)          # a round's budget counts only its own votes


def test_model_seeded_random_labelled_lists_cut_into_random_calls():
    rng = random.Random(0x524F554E4453)
    for _ in range(150):
        _check(rng, rng.choice((1, 2, 3, 16)))


def test_model_two_rounds_on_one_hash_stay_apart():
    # the model keys rounds by id: the same voters, valid under the one hash, fill both rounds
    K = [bytes([b]) * 48 for b in (0x50, 0x10, 0x30, 0x20)]
    m = rounds_model.RoundsModel(K)
    m.open("a")
    m.open("b")
    taken, slot, per_round = m.add(["a", "b", "a", "b", "b"], [0, 0, 0, 0, 0], [K[0], K[0], K[1], K[0], K[2]])
    assert taken == [1, 1, 1, 0, 1] and slot == [0, 1, 0, 1, 1]
    # key-sorted ranks: K[1] 0, K[3] 1, K[2] 2, K[0] 3
    assert per_round == [("a", bytes([0b10010000]), 2), ("b", bytes([0b00110000]), 2)]
    assert m.rounds["a"].base == 2 and m.rounds["b"].base == 3
    # a later single-round call: K[0] is held in "a" by the earlier call, K[3] is new
    taken, _, per_round = m.add(["a", "a"], [0, 0], [K[0], K[3]])
    assert taken == [0, 1] and per_round == [("a", bytes([0b11010000]), 3)]
