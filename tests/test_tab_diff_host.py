"""The host diff of ovh_update_validators (consensus_overlord_amd/csrc/tab_diff.hpp, pure host code)
under AddressSanitizer and UBSan: tests/host/tab_diff_harness.cpp is a stand-alone program that
checks every map of the diff against a brute-force restatement of its definition, over the seeded
cases of tests/test_tab_model.py (tables of 1 to 40 keys with duplicates; identity, permutation, one
add, one removal, one swap, all-new, empty) and these sizes besides: n = 0 on either side, n = 1,
64 -> 65 entries (the cap grows), 65 -> 64, and lists whose every key is the same. The maps it
prints are then compared with tests/tab_model.py's. Test-only build: never linked into the product."""
import os
import random
import subprocess

import tab_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    out = []
    for kind in tab_model.KINDS:
        for seed in range(40):
            out.append(tab_model.case(random.Random("%s/%d" % (kind, seed)), kind))
    rng = random.Random(0x7AB)
    k = [rng.randbytes(48) for _ in range(66)]
    out += [([], []), ([], k[:1]), (k[:1], []), (k[:1], k[:1]), (k[:1], k[1:2]), (k[:1], k[:2]), (k[:2], k[1::-1]),
            (k[:64], k[:65]), (k[:64], k[64:65] + k[:64]), (k[:65], k[:64]), (k[:65], k[1:65] + k[65:66]),
            ([k[0]] * 7, [k[0]] * 7), ([k[0]] * 7, [k[0]] * 9), ([k[0]] * 7, [k[1]] * 5), ([k[0]] * 3, [k[1], k[0], k[0], k[1]])]
    return out


def test_tab_diff_under_sanitizers(tmp_path):
    out = os.path.join(ROOT, "tests", "host", "_build", "tab_diff_harness")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    tmp = "%s.%d" % (out, os.getpid())       # renamed into place: parallel workers never run a half-written file
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", tmp,
                           os.path.join(ROOT, "tests", "host", "tab_diff_harness.cpp")])
    os.replace(tmp, out)
    cases = _cases()
    path = tmp_path / "cases.txt"
    with open(path, "w") as fh:
        fh.write("%d\n" % len(cases))
        for old, new in cases:
            fh.write("%d %d\n" % (len(old), len(new)))
            for key in old + new:
                fh.write(key.hex() + "\n")
    r = subprocess.run([out, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok %d" % len(cases) and len(lines) == len(cases) + 1, r.stdout[-2000:]
    n_same = 0
    for (old, new), line in zip(cases, lines):
        want = tab_model.diff(old, new)
        if want["same"]:
            assert line == "same", (len(old), len(new))
            n_same += 1
            continue
        tok = line.split()
        assert tok[0] == "diff"
        got, name = {}, None
        for t in tok[1:]:
            if t.isdigit():
                got[name].append(int(t))
            else:
                name = t
                got[name] = []
        for name in ("src", "fresh", "dst", "rsrc", "sorted", "rank"):
            assert got[name] == want[name], (name, len(old), len(new))
        assert got["kept"] == [want["kept"]]
    assert n_same >= 40 + 3     # every identity case, and the hand-made ones
