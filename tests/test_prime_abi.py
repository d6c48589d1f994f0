"""CPU checks of the priming boundary (include/ovhip.h ovh_prime_hashes / ovh_prime_stats): the
symbols are exported and reject a NULL context without touching a device or an output; the header,
ffi.rs, lib.rs and the ctypes signatures agree for these entry points (tests/test_abi.py and
tests/test_crate_ffi.py check every entry point; here these two by name); crypto.py exposes prime /
prime_votes / prime_stats; and VoteIngress primes once per distinct signed hash per flush window,
chokes included, and works unchanged over a crypto without `prime`."""
import ctypes
import hashlib
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_null_context_is_an_argument_error_and_writes_nothing():
    from consensus_overlord_amd import _lib
    lib = _lib.load()
    assert lib.ovh_prime_hashes(None, 1, bytes(32)) == 103
    assert lib.ovh_prime_hashes(None, 0, None) == 103
    st = (ctypes.c_uint64 * 4)(7, 7, 7, 7)
    assert lib.ovh_prime_stats(None, st) == 103
    assert list(st) == [7, 7, 7, 7]


def test_crypto_exposes_the_three_methods():
    from consensus_overlord_amd.crypto import ConsensusCrypto
    for name in ("prime", "prime_votes", "prime_stats"):
        assert callable(getattr(ConsensusCrypto, name)), name


def test_prototypes_in_header_ffi_lib_and_binding():
    from consensus_overlord_amd import _lib
    from consensus_overlord_amd.crypto import ConsensusCrypto
    hdr = open(os.path.join(ROOT, "include", "ovhip.h")).read()
    ffi = open(os.path.join(ROOT, "overlord-hip", "src", "ffi.rs")).read()
    lib = open(os.path.join(ROOT, "overlord-hip", "src", "lib.rs")).read()
    ing = open(os.path.join(ROOT, "overlord-hip", "src", "ingress.rs")).read()
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for fn, names in (("ovh_prime_hashes", ["ctx", "k", "hashes"]), ("ovh_prime_stats", ["ctx", "stats"])):
        m = re.search(r"^int %s\(([^;]*)\);" % fn, plain, flags=re.M)
        assert m, fn
        got = [re.sub(r"\[\d+\]$", "", a.split()[-1].lstrip("*")) for a in " ".join(m.group(1).split()).split(",")]
        assert got == names
        f = re.search(r"pub fn %s\((.*?)\) -> i32;" % fn, ffi)
        assert f and [a.split(":")[0].strip() for a in f.group(1).split(",")] == names
        assert "ffi::%s(" % fn in lib
        sig = [a for n, _, a in _lib.SIGNATURES if n == fn]
        assert len(sig) == 1 and len(sig[0]) == len(names)
    assert "pub fn prime_hashes(" in lib and "pub fn prime_stats(" in lib
    assert "crypto.prime_hashes(" in ing
    pmax = int(re.search(r"#define OVH_PRIME_MAX (\d+)", hdr).group(1))
    assert pmax == 64 == ConsensusCrypto.PRIME_MAX
    assert re.search(r"pub const OVH_PRIME_MAX: usize = %d;" % pmax, ffi)
    text = " ".join(hdr.replace("*", " ").split())
    assert "returns without waiting for the device" in text
    assert "never waits for it" in text


class _Stub:
    """What VoteIngress needs of a crypto, with a record of the calls."""

    def __init__(self):
        self.primes, self.prefetched = [], []

    def hash(self, msg):
        return hashlib.sha256(bytes(msg)).digest()

    def prefetch(self, sigs, hashes, voters):
        self.prefetched.append(list(hashes))


class _Priming(_Stub):
    def prime(self, hashes):
        self.primes.append([bytes(h) for h in hashes])


def _feed(crypto, batch_size):
    from consensus_overlord_amd import ingress as ing
    from consensus_overlord_amd import vote as _v
    out = []
    vi = ing.VoteIngress(crypto, lambda kind, m: out.append((kind, m)), batch_size=batch_size, max_delay_s=1e9)
    sig, pk = bytes(96), bytes(48)
    for i in range(3):   # three prevotes on one block, a nil prevote, two chokes
        vi.proc_network_msg(ing.SIGNED_VOTE, ing.encode_signed_vote(ing.SignedVote(sig, 7, 0, _v.PREVOTE, b"\x11" * 32, pk)))
    vi.proc_network_msg(ing.SIGNED_VOTE, ing.encode_signed_vote(ing.SignedVote(sig, 7, 0, _v.PREVOTE, b"", pk)))
    frm = _v._rlp_list([_v._rlp_uint(2), _v._rlp_bytes(b"")])
    for i in range(2):
        vi.proc_network_msg(ing.SIGNED_CHOKE, ing.encode_signed_choke(ing.SignedChoke(sig, 7, 0, frm, pk)))
    return vi, out


def test_ingress_primes_once_per_hash_per_flush_window():
    from consensus_overlord_amd import ingress as ing
    from consensus_overlord_amd import vote as _v
    c = _Priming()
    vi, out = _feed(c, batch_size=100)
    h_vote = c.hash(_v.rlp_vote(7, 0, _v.PREVOTE, b"\x11" * 32))
    h_nil = c.hash(_v.rlp_vote(7, 0, _v.PREVOTE, b""))
    h_choke = c.hash(_v._rlp_list([_v._rlp_uint(7), _v._rlp_uint(0)]))
    assert c.primes == [[h_vote], [h_nil], [h_choke]] and not out
    vi.flush()
    assert len(out) == 6 and c.prefetched == [[h_vote] * 3 + [h_nil] + [h_choke] * 2]
    # the next window primes the same hash again (the library skips what is still cached)
    vi.proc_network_msg(ing.SIGNED_VOTE, ing.encode_signed_vote(
        ing.SignedVote(bytes(96), 7, 0, _v.PREVOTE, b"\x11" * 32, bytes(48))))
    assert c.primes[3:] == [[h_vote]]


def test_ingress_without_prime_is_unchanged():
    a, b = _Stub(), _Priming()
    (via, outa), (vib, outb) = _feed(a, batch_size=3), _feed(b, batch_size=3)
    via.flush()
    vib.flush()
    assert a.primes == [] and a.prefetched == b.prefetched
    assert via.stats == vib.stats and [k for k, _ in outa] == [k for k, _ in outb] and len(outa) == 6
