"""CPU checks of the boundary of the signature-point cache and the aggregation counters
(include/ovhip.h ovh_sig_cache_config / ovh_agg_stats): the symbols are exported and reject a NULL
context or NULL stats without touching a device or an output; the header, ffi.rs, lib.rs and the
ctypes signatures agree for these entry points (tests/test_abi.py and tests/test_crate_ffi.py check
every entry point; here these two by name); crypto.py exposes sig_cache_config / agg_stats; the
header states the routes' conditions at the two trait calls."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_null_arguments_are_argument_errors_and_write_nothing():
    from consensus_overlord_amd import _lib
    lib = _lib.load()
    assert lib.ovh_sig_cache_config(None, 0) == 103
    assert lib.ovh_sig_cache_config(None, 4096) == 103
    st = (ctypes.c_uint64 * 8)(*([7] * 8))
    assert lib.ovh_agg_stats(None, st) == 103
    assert list(st) == [7] * 8
    assert lib.ovh_agg_stats(None, None) == 103


def test_crypto_exposes_the_two_methods():
    from consensus_overlord_amd.crypto import ConsensusCrypto
    for name in ("sig_cache_config", "agg_stats"):
        assert callable(getattr(ConsensusCrypto, name)), name


def test_prototypes_in_header_ffi_lib_and_binding():
    from consensus_overlord_amd import _lib
    from consensus_overlord_amd.crypto import ConsensusCrypto
    hdr = open(os.path.join(ROOT, "include", "ovhip.h")).read()
    ffi = open(os.path.join(ROOT, "overlord-hip", "src", "ffi.rs")).read()
    lib = open(os.path.join(ROOT, "overlord-hip", "src", "lib.rs")).read()
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for fn, names in (("ovh_sig_cache_config", ["ctx", "capacity"]), ("ovh_agg_stats", ["ctx", "stats"])):
        m = re.search(r"^int %s\(([^;]*)\);" % fn, plain, flags=re.M)
        assert m, fn
        got = [re.sub(r"\[\d+\]$", "", a.split()[-1].lstrip("*")) for a in " ".join(m.group(1).split()).split(",")]
        assert got == names
        f = re.search(r"pub fn %s\((.*?)\) -> i32;" % fn, ffi)
        assert f and [a.split(":")[0].strip() for a in f.group(1).split(",")] == names
        assert "ffi::%s(" % fn in lib
        sig = [a for n, _, a in _lib.SIGNATURES if n == fn]
        assert len(sig) == 1 and len(sig[0]) == len(names)
    assert "pub fn sig_cache_config(" in lib and "pub fn agg_stats(" in lib
    assert re.search(r"int ovh_agg_stats\(ovh_ctx\* ctx, uint64_t stats\[8\]\);", plain)
    dflt = int(re.search(r"#define OVH_SIG_CACHE_DEFAULT (\d+)", hdr).group(1))
    assert dflt == 4096 == ConsensusCrypto.SIG_CACHE_DEFAULT
    assert re.search(r"pub const OVH_SIG_CACHE_DEFAULT: usize = %d;" % dflt, ffi)
    cmax = int(re.search(r"#define OVH_SIG_CACHE_MAX (\d+)", hdr).group(1))
    assert cmax == 65536 and re.search(r"pub const OVH_SIG_CACHE_MAX: usize = %d;" % cmax, ffi)


def test_header_states_the_routes_at_the_trait_calls():
    hdr = open(os.path.join(ROOT, "include", "ovhip.h")).read()
    text = " ".join(hdr.replace("*", " ").split())
    agg = text[text.index("Crypto::aggregate_signatures"):text.index("int ovh_aggregate_sigs(")]
    assert "does not change what the call returns" in agg and "every signature is in the cache" in agg
    assert "no partial mode" in agg
    ver = text[text.index("Crypto::verify_aggregated_signature"):text.index("int ovh_verify_aggregated(")]
    assert "does not change what the call returns" in ver and "never entered" in ver and "answers 102" in ver
    assert "OVH_SIG_CACHE" in text and "OVH_QC_TABLE" in text
