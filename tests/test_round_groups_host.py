"""The round numbering of ovh_rounds_add (consensus_overlord_amd/csrc/qc_round_groups.hpp, pure host
code) under AddressSanitizer and UBSan: tests/host/round_groups_harness.cpp is a stand-alone program
that checks, over seeded random id lists (1 to 16 rounds, sparse 64-bit ids, table voters and
others mixed), that the distinct ids are numbered by first appearance in the caller's order, that a
vote's position counts only the votes of its own round, that number and position follow the
table-first permutation of the staging, and that the segment input (qc_segments.hpp) has one
segment per round holding exactly that round's votes; then 16 singleton rounds and one round of 65
votes beside one round of 1 vote. Test-only build: never linked into the product."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_round_numbering_under_sanitizers():
    out = os.path.join(ROOT, "tests", "host", "_build", "round_groups_harness")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    tmp = "%s.%d" % (out, os.getpid())       # renamed into place: parallel workers never run a half-written file
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", tmp,
                           os.path.join(ROOT, "tests", "host", "round_groups_harness.cpp")])
    os.replace(tmp, out)
    r = subprocess.run([out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert r.stdout.startswith("ok "), r.stdout
    assert int(r.stdout.split()[1]) == 16 * 8 + 2
