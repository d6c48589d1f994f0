"""CPU checks of the block-sync boundary: ovh_sm3_batch, ovh_sm3_batch_device and
ovh_check_blocks are exported, refuse a NULL context without writing, and are named by the
header, the Rust crate and the Python bindings (no compute calls: there is no GPU here)."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ovh_sm3_batch", "ovh_sm3_batch_device", "ovh_check_blocks")
ERR_ARG = 103


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_symbols_exported():
    from consensus_overlord_amd import _lib
    lib = _lib.load()
    for n in NAMES:
        assert hasattr(lib, n), n


def test_null_context_is_refused_and_nothing_is_written():
    from consensus_overlord_amd import _lib
    lib = _lib.load()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    data = np.frombuffer(b"abc" * 10, dtype=np.uint8)
    off = np.array([0, 10, 30], dtype=np.uint64)
    dig = np.full(64, 0xEE, dtype=np.uint8)
    assert lib.ovh_sm3_batch(None, 2, ptr(data), ptr(off), ptr(dig)) == ERR_ARG
    assert lib.ovh_sm3_batch_device(None, 2, ptr(data), ptr(off), ptr(dig)) == ERR_ARG
    assert (dig == 0xEE).all()
    heights = np.array([1, 2], dtype=np.uint64)
    ok = np.full(2, 0xEE, dtype=np.uint8)
    reasons = np.full(2, -7, dtype=np.int32)
    assert lib.ovh_check_blocks(None, 2, ptr(heights), ptr(data), ptr(off), ptr(data), ptr(off), ptr(ok),
                                ptr(reasons)) == ERR_ARG
    assert (ok == 0xEE).all() and (reasons == -7).all()


def test_named_in_header_crate_and_bindings():
    from consensus_overlord_amd import _lib
    hdr, ffi, lib = read("include", "ovhip.h"), read("overlord-hip", "src", "ffi.rs"), read("overlord-hip", "src", "lib.rs")
    sigs = {n for n, _, _ in _lib.SIGNATURES}
    for n in NAMES:
        assert re.search(r"^int %s\(ovh_ctx\* ctx, size_t n," % n, hdr, flags=re.M), n
        assert re.search(r"pub fn %s\(ctx: \*mut OvhCtx, n: usize," % n, ffi), n
        assert n in sigs, n
    for name, val in (("OVH_CB_PROOF_DECODE", 300), ("OVH_CB_MISMATCH", 301)):
        assert re.search(r"#define %s +%d\b" % (name, val), hdr), name
        assert re.search(r"pub const %s: i32 = %d;" % (name, val), ffi), name
    # the crate's safe wrappers over them
    assert re.search(r"pub fn hash_batch\(&self", lib) and "ffi::ovh_sm3_batch(" in lib
    assert re.search(r"pub fn check_blocks\(&self", lib) and "ffi::ovh_check_blocks(" in lib


def test_crypto_exposes_the_batched_forms():
    from consensus_overlord_amd.crypto import ConsensusCrypto
    for m in ("hash_batch", "check_block_batch", "check_blocks", "check_block"):
        assert callable(getattr(ConsensusCrypto, m)), m
