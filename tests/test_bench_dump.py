"""bench.py --dump-outputs: the writer of the last timed batch's codes and votes (CPU only)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _votes(n):
    rng = np.random.default_rng(7)
    return (np.arange(n, dtype=np.int32) % 7 - 1, rng.integers(0, 256, (n, 96), dtype=np.uint8),
            rng.integers(0, 256, (n, 48), dtype=np.uint8))


def test_dump_outputs_writes_float32_arrays(tmp_path):
    import bench

    codes, sigs, pks = _votes(5)
    out = tmp_path / "new" / "dir"          # created on demand
    bench.dump_outputs(str(out), codes, sigs, pks)
    assert sorted(os.listdir(out)) == ["codes.npy", "pks.npy", "sigs.npy"]
    for name, want in (("codes", codes), ("sigs", sigs), ("pks", pks)):
        got = np.load(out / (name + ".npy"))
        assert got.dtype == np.float32 and got.shape == want.shape
        assert (got == want).all()


def test_dump_outputs_samples_large_batches_the_same_way(tmp_path, monkeypatch):
    import bench

    codes, sigs, pks = _votes(64)
    monkeypatch.setattr(bench, "DUMP_BYTES", 10 * 4 * (1 + 96 + 48))   # room for 10 votes
    bench.dump_outputs(str(tmp_path / "a"), codes, sigs, pks, "_rank1")
    bench.dump_outputs(str(tmp_path / "b"), codes, sigs, pks, "_rank1")
    a = {k: np.load(tmp_path / "a" / (k + "_rank1.npy")) for k in ("codes", "sigs", "pks")}
    b = {k: np.load(tmp_path / "b" / (k + "_rank1.npy")) for k in ("codes", "sigs", "pks")}
    assert all((a[k] == b[k]).all() for k in a)
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_BYTES and len(a["codes"]) == 10
    # the same votes in every array: each sampled row is a row of the input, in order
    rows = [next(i for i in range(64) if (sigs[i] == r).all()) for r in a["sigs"]]
    assert rows == sorted(rows) and (a["pks"] == pks[rows]).all() and (a["codes"] == codes[rows]).all()
