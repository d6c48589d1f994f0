"""k_sm3_bulk keeps its message schedule and state in registers: a translation unit that includes
only consensus_overlord_amd/csrc/sm3_bulk.hpp, cross-compiled for gfx950 with the Makefile's
HIPFLAGS, reports 0 bytes of scratch per lane (the naive form, sm3.hpp's w[68] / w1[64] behind a
lane-per-message kernel, takes 544). No GPU needed: the compiler's resource remarks are read."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "consensus_overlord_amd")


def makefile_var(name, text):
    m = re.search(r"^%s \?= (.*)$" % name, text, flags=re.M)
    assert m, name
    return m.group(1).strip()


def test_k_sm3_bulk_uses_no_scratch(tmp_path):
    mk = open(os.path.join(PKG, "Makefile")).read()
    hipcc = os.environ.get("HIPCC") or makefile_var("HIPCC", mk)
    flags = makefile_var("HIPFLAGS", mk).replace("$(ARCH)", makefile_var("ARCH", mk)).split()
    tu = tmp_path / "sm3_bulk_only.hip"
    tu.write_text('#include "sm3_bulk.hpp"\n')
    r = subprocess.run([hipcc] + flags + ["-I" + os.path.join(PKG, "csrc"), "-Rpass-analysis=kernel-resource-usage",
                                          "-c", str(tu), "-o", str(tmp_path / "sm3_bulk_only.o")],
                       cwd=PKG, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    # the remarks of one kernel follow its "Function Name" line
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    mine = [b for b in blocks if "k_sm3_bulk" in b.split()[0]]
    assert len(mine) == 1, [b.split()[0] for b in blocks]
    m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", mine[0])
    assert m, mine[0]
    assert int(m.group(1)) == 0, mine[0]
    assert re.search(r"VGPRs Spill: 0\b", mine[0]) and re.search(r"Dynamic Stack: False", mine[0]), mine[0]
