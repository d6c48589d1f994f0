"""Code size of the Fp-VM kernels in the built libovhip.so.

A VM kernel is mostly its inlined copies of the interpreter's `exec` (csrc/fpvm.hpp). The vote
pool once carried twelve (two vote programs x the loop unrolled three times, a fused fold loop
with three more, the inversion in every one): 261,776 B, four times its siblings. This test
unbundles the gfx950 code object of the library with the ROCm LLVM tools and reads symbol sizes
only (no GPU): the pool stays no larger than the largest VM kernel of that commit, and no VM
kernel is larger than it was then."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "consensus_overlord_amd", "libovhip.so")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"

# the largest VM kernel (k_vm_votew<false>) when the pool was 261,776 B
POOL_MAX = 68280
# code bytes before the interpreter's INV / UNROLL parameters and the pool's shared loop
# (hipcc -O3 --offload-arch=gfx950, llvm-readelf -s)
BEFORE = {
    "k_vm_pool": 261776,
    "k_msm_plane": 66300, "k_msm_chunk": 65656, "k_msm_comb": 63100, "k_msm_upper": 62792,
    "k_qc_chunk": 65652, "k_qc_upper": 62756,
    "k_vm_final": 62760, "k_vm_fold<1>": 62560,
    "k_vm_rs": 63440, "k_vm_group": 62096, "k_vm_votechk": 62168,
    "k_vm_g1grp": 61396, "k_vm_pkchk": 63468, "k_vm_pkdec": 62808, "k_vm_pkgen": 97300,
    "k_vm_qcmil": 63552, "k_vm_qcpre": 65932, "k_vm_signg": 232356,
    "k_vm_vote1<false>": 67976, "k_vm_vote1<true>": 66636,
    "k_vm_votew<false>": 68280, "k_vm_votew<true>": 66952,
    "k_vm_vsame<false, 16u>": 66812, "k_vm_vsame<false, 8u>": 66812,
    "k_vm_vsame<true, 16u>": 65504, "k_vm_vsame<true, 8u>": 65504,
    "k_vm_final1": 61408, "k_vm_g1tree": 62476, "k_vm_g2tree": 62488, "k_vm_sigchk": 63952,
    "k_vm_vote1h<false>": 68012, "k_vm_vote1h<true>": 66680, "k_vm_votefe": 61436,
    "k_vm_g1pairs": 62340,
    "k_vm_vote1h_b<false>": 68132, "k_vm_vote1h_b<true>": 66764,
    "k_vm_fe": 61308, "k_vm_h2g": 63288, "k_vm_gfin": 63640, "k_vm_gmil": 63944,
}


def _tool(name):
    roots = [os.environ.get("ROCM_PATH"), os.environ.get("ROCM_HOME"), "/opt/rocm"]
    for r in filter(None, roots):
        for sub in ("lib/llvm/bin", "llvm/bin", "bin"):
            p = os.path.join(r, sub, name)
            if os.access(p, os.X_OK):
                return p
    p = shutil.which(name)
    assert p, "ROCm LLVM tool %s not found (ROCM_PATH)" % name
    return p


@pytest.fixture(scope="module")
def sizes(tmp_path_factory):
    """{kernel name as written in the source, template arguments included: code bytes}"""
    assert os.path.exists(LIB), "libovhip.so is not built (make -C consensus_overlord_amd)"
    d = tmp_path_factory.mktemp("codeobj")
    fat, co = str(d / "fat.bin"), str(d / "gfx950.co")
    subprocess.check_call([_tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, LIB, str(d / "rest.so")])
    subprocess.check_call([_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET,
                           "--input=" + fat, "--output=" + co])
    out = subprocess.check_output([_tool("llvm-readelf"), "-sW", "--demangle", co], text=True)
    got = {}
    for line in out.splitlines():
        # Num: Value Size Type Bind Vis Ndx Name
        m = re.match(r"\s*\d+:\s+[0-9a-f]+\s+(\d+)\s+FUNC\s+\S+\s+\S+\s+\S+\s+(.*)$", line)
        if not m:
            continue
        name = re.sub(r"^void ", "", m.group(2).strip())
        depth, cut = 0, len(name)
        for k, ch in enumerate(name):   # the argument list starts at the first '(' outside <>
            depth += ch == "<"
            depth -= ch == ">"
            if ch == "(" and depth == 0:
                cut = k
                break
        got[name[:cut]] = int(m.group(1))
    assert got, "no function symbols in the gfx950 code object"
    return got


def _vm_kernels(sizes):
    return {k: v for k, v in sizes.items() if re.match(r"k_(vm|msm_(plane|chunk|comb|upper)|qc_(chunk|upper))", k)}


def test_pool_is_no_larger_than_its_siblings(sizes):
    assert "k_vm_pool" in sizes, sorted(sizes)[:20]
    print("k_vm_pool", sizes["k_vm_pool"])
    assert sizes["k_vm_pool"] <= POOL_MAX


def test_no_vm_kernel_grew(sizes):
    vm = _vm_kernels(sizes)
    for k in ("k_vm_pool", "k_msm_plane", "k_msm_chunk", "k_msm_comb", "k_msm_upper", "k_vm_final", "k_vm_fold<1>",
              "k_vm_rs", "k_vm_group", "k_vm_votechk"):
        assert k in vm, (k, sorted(vm))
    grew = {k: (v, BEFORE[k]) for k, v in vm.items() if k in BEFORE and v > BEFORE[k]}
    print({k: v for k, v in sorted(vm.items())})
    assert not grew, grew
    # a VM kernel added since is held to the same ceiling as the pool
    new = {k: v for k, v in vm.items() if k not in BEFORE and v > POOL_MAX}
    assert not new, new
