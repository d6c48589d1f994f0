"""The host index of the signature-point cache (consensus_overlord_amd/csrc/sig_cache.hpp, pure host
code): tests/host/sig_cache_harness.cpp is a stand-alone program that checks claim, register and
find, the eviction order, that an entry claimed but never registered is not found, re-registering a
key that is still present, capacities 1 and 2, the wrap of a contiguous claim past the ring's end,
the off state, and seeded random runs against a plain model. Built with g++ once plainly and once
under AddressSanitizer and UBSan. Test-only builds: never linked into the product."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


@pytest.mark.parametrize("name,flags", [("sig_cache_harness", []), ("sig_cache_harness_san", SAN)], ids=["plain", "sanitizers"])
def test_sig_cache_index(name, flags):
    out = os.path.join(ROOT, "tests", "host", "_build", name)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    tmp = "%s.%d" % (out, os.getpid())       # renamed into place: parallel workers never run a half-written file
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags +
                          ["-o", tmp, os.path.join(ROOT, "tests", "host", "sig_cache_harness.cpp")])
    os.replace(tmp, out)
    r = subprocess.run([out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert r.stdout.startswith("ok "), r.stdout
    assert int(r.stdout.split()[1]) > 2000
