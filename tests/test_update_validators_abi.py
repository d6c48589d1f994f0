"""CPU checks of the boundary of ovh_update_validators and ovh_table_stats (include/ovhip.h): both
symbols are exported and refuse a NULL context (103) without touching a device or an output, the
header, ffi.rs and the ctypes signatures name the arguments identically, lib.rs has
update_pubkeys_keep_rounds, OVH_TABLE_NSTATS agrees everywhere, and crypto.py / ingress.py expose
the calls."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ovh_update_validators", "ovh_table_stats")


def test_both_symbols_are_exported():
    from consensus_overlord_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        assert getattr(lib, name) is not None, name


def test_null_context_is_an_argument_error_and_writes_nothing():
    from consensus_overlord_amd import _lib
    lib = _lib.load()
    closed = (ctypes.c_uint64 * 16)(*([0x77] * 16))
    n_closed = ctypes.c_uint32(0x55)
    assert lib.ovh_update_validators(None, bytes(96), 2, closed, ctypes.byref(n_closed)) == 103
    assert list(closed) == [0x77] * 16 and n_closed.value == 0x55
    assert lib.ovh_update_validators(None, None, 0, None, None) == 103
    stats = (ctypes.c_uint64 * 8)(*([0x99] * 8))
    assert lib.ovh_table_stats(None, stats) == 103
    assert list(stats) == [0x99] * 8


def _header_args(hdr, name):
    # (tests/test_rounds_abi.py's)
    m = re.search(r"^int %s\(([^;]*)\);" % name, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), flags=re.M)
    assert m, name
    return [re.sub(r"\[\d+\]$", "", a.split()[-1].lstrip("*")) for a in " ".join(m.group(1).split()).split(",")]


def test_names_in_header_ffi_and_binding_and_the_constant():
    from consensus_overlord_amd import _lib
    from consensus_overlord_amd.crypto import ConsensusCrypto
    hdr = open(os.path.join(ROOT, "include", "ovhip.h")).read()
    ffi = open(os.path.join(ROOT, "overlord-hip", "src", "ffi.rs")).read()
    lib = open(os.path.join(ROOT, "overlord-hip", "src", "lib.rs")).read()
    want = {
        "ovh_update_validators": ["ctx", "pks", "n", "closed", "n_closed"],
        "ovh_table_stats": ["ctx", "stats"],
    }
    for name in NAMES:
        names = _header_args(hdr, name)
        assert names == want[name], name
        f = re.search(r"pub fn %s\((.*?)\) -> i32;" % name, ffi)
        assert f and [a.split(":")[0].strip() for a in f.group(1).split(",")] == names, name
        sig = [a for n, _, a in _lib.SIGNATURES if n == name]
        assert len(sig) == 1 and len(sig[0]) == len(names), name
        assert "ffi::%s(" % name in lib, name
    assert "pub async fn update_pubkeys_keep_rounds<" in lib and "pub async fn update_pubkeys<" in lib
    nst = int(re.search(r"#define OVH_TABLE_NSTATS (\d+)", hdr).group(1))
    assert nst == 8 == ConsensusCrypto.TABLE_NSTATS
    assert re.search(r"pub const OVH_TABLE_NSTATS: usize = %d;" % nst, ffi)
    assert "uint64_t stats[%d] /* OVH_TABLE_NSTATS */" % nst in hdr
    # the header states the identical-list promise, the defining property and what a refusal leaves
    text = " ".join(hdr.replace("*", " ").split())
    assert "No device call, no stream is waited for" in text
    assert "a fresh round on the new table to which T was added" in text
    assert "changes and writes nothing" in text


def test_crypto_and_ingress_expose_the_calls():
    from consensus_overlord_amd import crypto, ingress
    p = inspect.signature(crypto.ConsensusCrypto.update_pubkeys).parameters
    assert p["keep_rounds"].default is False                   # the default is the plain call
    assert callable(crypto.ConsensusCrypto.table_stats)
    assert callable(ingress.VoteIngress.update_pubkeys)
    assert isinstance(crypto.Round.bitmap_len, property)       # a carried round follows the table
