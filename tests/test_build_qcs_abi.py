"""CPU checks of ovh_build_qcs' boundary (include/ovhip.h): the symbol is exported and rejects a
NULL context without touching a device or an output, crypto.py exposes build_qcs_raw / build_qcs /
build_vote_qcs, the header, ffi.rs, lib.rs and the ctypes signature agree for this entry point
(tests/test_abi.py and tests/test_crate_ffi.py check every entry point; here this one by name),
and the pure-Python model of grouping + selection (tests/qc_groups_model.py, the specification
tests/test_gpu_build_qcs.py compares the device with) gives the documented groups, taken flags
and bitmaps on hand-written vote sets."""
import ctypes
import os
import re

import qc_groups_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_null_context_is_an_argument_error_and_writes_nothing():
    from consensus_overlord_amd import _lib
    lib = _lib.load()
    codes = (ctypes.c_int32 * 2)(9, 9)
    taken = ctypes.create_string_buffer(b"\x07\x07", 2)
    group = (ctypes.c_uint32 * 2)(5, 5)
    ng = ctypes.c_uint32(7)
    gh = ctypes.create_string_buffer(b"\xaa" * 64, 64)
    out = ctypes.create_string_buffer(b"\xbb" * 192, 192)
    bm = ctypes.create_string_buffer(b"\xcc" * 2, 2)
    cnt = (ctypes.c_uint32 * 2)(3, 3)
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)   # noqa: E731
    r = lib.ovh_build_qcs(None, 2, bytes(192), bytes(64), bytes(96), p(codes), p(taken), p(group), 2, ctypes.byref(ng),
                          p(gh), p(out), p(bm), 1, p(cnt))
    assert r == 103
    assert list(codes) == [9, 9] and taken.raw == b"\x07\x07" and list(group) == [5, 5] and ng.value == 7
    assert gh.raw == b"\xaa" * 64 and out.raw == b"\xbb" * 192 and bm.raw == b"\xcc" * 2 and list(cnt) == [3, 3]


def test_crypto_exposes_the_three_methods():
    from consensus_overlord_amd.crypto import ConsensusCrypto
    for name in ("build_qcs_raw", "build_qcs", "build_vote_qcs"):
        assert callable(getattr(ConsensusCrypto, name)), name


def test_prototype_in_header_ffi_lib_and_binding():
    from consensus_overlord_amd import _lib
    from consensus_overlord_amd.crypto import ConsensusCrypto
    hdr = open(os.path.join(ROOT, "include", "ovhip.h")).read()
    ffi = open(os.path.join(ROOT, "overlord-hip", "src", "ffi.rs")).read()
    lib = open(os.path.join(ROOT, "overlord-hip", "src", "lib.rs")).read()
    m = re.search(r"^int ovh_build_qcs\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), flags=re.M)
    assert m
    names = [a.split()[-1].lstrip("*") for a in " ".join(m.group(1).split()).split(",")]
    assert names == ["ctx", "n", "sigs", "hashes", "pks", "codes", "taken", "group", "max_groups", "n_groups",
                     "group_hashes", "out_sigs", "bitmaps", "bitmap_len", "n_signed"]
    f = re.search(r"pub fn ovh_build_qcs\((.*?)\) -> i32;", ffi)
    assert f and [a.split(":")[0].strip() for a in f.group(1).split(",")] == names
    assert "pub fn build_qcs(" in lib and "ffi::ovh_build_qcs(" in lib
    sig = [a for n, _, a in _lib.SIGNATURES if n == "ovh_build_qcs"]
    assert len(sig) == 1 and len(sig[0]) == len(names)
    gmax = int(re.search(r"#define OVH_QC_GROUPS_MAX (\d+)", hdr).group(1))
    assert gmax == 64 == ConsensusCrypto.QC_GROUPS_MAX
    assert re.search(r"pub const OVH_QC_GROUPS_MAX: usize = %d;" % gmax, ffi)
    # the header comment states the equivocation rule and the numbering
    text = " ".join(hdr.replace("*", " ").split())
    assert "(equivocation) is taken in both" in text
    assert "numbered by first appearance in the caller's order" in text


K = [bytes([b]) * 48 for b in (0x50, 0x10, 0x30, 0x20, 0x40)]   # config order; sorted: 10 20 30 40 50
OUT = bytes([0x99]) * 48                                         # not a validator
A, B, C = (bytes([x]) * 32 for x in (0xA1, 0xB2, 0xC3))


def test_model_equivocation_in_two_groups():
    # K[1] (rank 0) signs A and B validly: taken in both; B appears first, so it is group 0
    group, gh, taken, bm, cnt = qc_groups_model.select([0, 0, 0], [B, A, A], [K[1], K[1], K[0]], K)
    assert group == [0, 1, 1] and gh == [B, A]
    assert taken == [1, 1, 1] and cnt == [1, 2]
    assert bm == [bytes([0b10000000]), bytes([0b10001000])]


def test_model_duplicate_within_a_group_interleaved_with_another_group():
    # K[2] (rank 2) votes twice on A with a vote on B between them; K[3] (rank 1) on B
    group, gh, taken, bm, cnt = qc_groups_model.select([0, 0, 0, 0], [A, B, A, B], [K[2], K[3], K[2], OUT], K)
    assert group == [0, 1, 0, 1] and gh == [A, B]
    assert taken == [1, 1, 0, 0] and cnt == [1, 1]
    assert bm == [bytes([0b00100000]), bytes([0b01000000])]


def test_model_group_whose_votes_are_all_invalid():
    group, gh, taken, bm, cnt = qc_groups_model.select([5, 0, 3, 0, 102], [A, B, A, C, A], [K[0], K[4], K[1], K[4], K[2]], K)
    assert group == [0, 1, 0, 2, 0] and gh == [A, B, C]
    assert taken == [0, 1, 0, 1, 0] and cnt == [0, 1, 1]
    assert bm == [bytes(1), bytes([0b00010000]), bytes([0b00010000])]


def test_model_one_group_is_the_single_hash_rule():
    import qc_model
    codes, voters = [0, 5, 0, 0, 0], [K[1], K[2], K[1], OUT, K[2]]
    group, gh, taken, bm, cnt = qc_groups_model.select(codes, [A] * 5, voters, K)
    assert group == [0] * 5 and gh == [A]
    assert (taken, bm[0], cnt[0]) == qc_model.select(codes, voters, K)
