"""CPU checks of ovh_build_qc's boundary (include/ovhip.h): the symbol is exported and rejects
a NULL context without touching a device, crypto.py exposes build_qc / build_proof, the three
prototype lists agree (tests/test_abi.py and tests/test_crate_ffi.py check that for every entry
point; here for this one by name), and the pure-Python model of the selection rule
(tests/qc_model.py, the specification tests/test_gpu_build_qc.py compares the device with)
gives the documented taken flags and bitmap on hand-written rounds."""
import ctypes
import os
import re

import qc_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_null_context_is_an_argument_error():
    from consensus_overlord_amd import _lib
    lib = _lib.load()
    codes = (ctypes.c_int32 * 1)()
    taken = ctypes.create_string_buffer(1)
    out = ctypes.create_string_buffer(96)
    bitmap = ctypes.create_string_buffer(1)
    cnt = ctypes.c_uint32(7)
    r = lib.ovh_build_qc(None, 1, bytes(96), bytes(32), 32, bytes(48), codes, taken, out, bitmap, 1, ctypes.byref(cnt))
    assert r == 103
    assert cnt.value == 7 and out.raw == bytes(96)   # nothing written


def test_crypto_exposes_build_qc_and_build_proof():
    from consensus_overlord_amd.crypto import ConsensusCrypto
    assert callable(ConsensusCrypto.build_qc) and callable(ConsensusCrypto.build_proof)


def test_prototype_in_header_ffi_and_binding():
    from consensus_overlord_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ovhip.h")).read()
    ffi = open(os.path.join(ROOT, "overlord-hip", "src", "ffi.rs")).read()
    lib = open(os.path.join(ROOT, "overlord-hip", "src", "lib.rs")).read()
    assert re.search(r"^int ovh_build_qc\(ovh_ctx\* ctx, size_t n,", hdr, flags=re.M)
    # the header comment states the duplicate-key rule
    assert "occurs twice in the table counts at its first position in sorted order" in " ".join(
        hdr.replace("*", " ").split())
    assert "pub fn ovh_build_qc(" in ffi
    assert "pub fn build_qc(" in lib and "ffi::ovh_build_qc(" in lib
    sig = [a for n, _, a in _lib.SIGNATURES if n == "ovh_build_qc"]
    assert len(sig) == 1 and len(sig[0]) == 12


K = [bytes([b]) * 48 for b in (0x50, 0x10, 0x30, 0x20, 0x40)]   # config order; sorted: 10 20 30 40 50
OUT = bytes([0x99]) * 48                                         # not a validator


def test_model_duplicate_voter():
    # K[1] (rank 0) votes twice: the lower index is taken; K[0] is rank 4
    taken, bitmap, cnt = qc_model.select([0, 0, 0], [K[1], K[0], K[1]], K)
    assert taken == [1, 1, 0] and bitmap == bytes([0b10001000]) and cnt == 2


def test_model_invalid_then_valid_same_voter():
    # an invalid earlier vote does not block the voter's later valid one; K[2] is rank 2
    taken, bitmap, cnt = qc_model.select([5, 0, 0], [K[2], K[3], K[2]], K)
    assert taken == [0, 1, 1] and bitmap == bytes([0b01100000]) and cnt == 2


def test_model_non_member():
    taken, bitmap, cnt = qc_model.select([0, 0], [OUT, K[4]], K)
    assert taken == [0, 1] and bitmap == bytes([0b00010000]) and cnt == 1


def test_model_none_valid():
    taken, bitmap, cnt = qc_model.select([5, 3, 102, 0], [K[0], K[1], K[2], OUT], K)
    assert taken == [0, 0, 0, 0] and bitmap == bytes(1) and cnt == 0


def test_model_pad_bits_and_duplicate_table_key():
    # 13 keys -> 2 bytes, 3 pad bits; a key listed twice counts at its first sorted position
    table = [bytes([b]) * 48 for b in range(12, 0, -1)] + [bytes([5]) * 48]
    srt = sorted(table)
    assert srt[4] == srt[5] == bytes([5]) * 48
    taken, bitmap, cnt = qc_model.select([0, 0, 0], [bytes([5]) * 48, bytes([12]) * 48, bytes([5]) * 48], table)
    assert taken == [1, 1, 0] and cnt == 2
    assert bitmap == bytes([0b00001000, 0b00001000]) and bitmap[1] & 0b111 == 0
