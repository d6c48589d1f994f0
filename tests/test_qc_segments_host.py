"""The segment layout of ovh_build_qcs' masked sums (consensus_overlord_amd/csrc/qc_segments.hpp,
pure host code) under AddressSanitizer and UBSan: tests/host/qc_segments_harness.cpp is a
stand-alone program that checks, over seeded random group-size vectors (1 to 64 groups, sizes 1
to 300 with 63, 64 and 65 among them), that every staged vote appears exactly once, no chunk
holds votes of two groups, pads are NONE, the segment table matches the layout, and the chunk and
entry bounds of DESIGN.md section 3.6 hold. Test-only build: never linked into the product."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_segment_layout_under_sanitizers():
    out = os.path.join(ROOT, "tests", "host", "_build", "qc_segments_harness")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    tmp = "%s.%d" % (out, os.getpid())       # renamed into place: parallel workers never run a half-written file
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", tmp, os.path.join(ROOT, "tests", "host", "qc_segments_harness.cpp")])
    os.replace(tmp, out)
    r = subprocess.run([out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert r.stdout.startswith("ok "), r.stdout
    assert int(r.stdout.split()[1]) >= 64 * 6
