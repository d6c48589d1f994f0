"""Unit-level checks of ovh_update_validators' kernels (consensus_overlord_amd/csrc/tab_update.hpp)
on slabs, maps and round words chosen here, which no test through ovh_update_validators can choose:
there the planes are points of real keys and the owner words come from verified votes. The probe
(tests/device/tab_probe.hip, built by `make -C consensus_overlord_amd` as
tests/device/_build/libtabprobe.so) includes the product translation unit whole and calls the
product's own launch code.

k_tab_build: entry counts old -> new 1 -> 1, 5 -> 6, 6 -> 5, 64 -> 65 (cap 64 -> 128) and 65 -> 130
(cap 128 -> 256), each under the identity, the reversal, the rotation by one, all new, and none new
with duplicate keys. The source slabs hold a distinct word per (slab, coordinate word, entry); the
destination is 0xFF-filled with guard words behind it. Every word of the entries < n and every flag
is compared, the entries from n to the cap and the guards must keep the fill.

k_round_remap: tn old -> new among 31, 32, 33, 64, 65 (the bitmap's word and byte boundaries), 16
rounds in one launch: nothing taken, everything taken, only the first entry, only the last entry,
only entries that survive, exactly one dropped entry taken (lost = 1), taken entries whose bit moves
across a word boundary, then seeded subsets. Owner words, bitmap words (pad bits 0), count, merged,
R, the 96 bytes, lost and the guard words around every new allocation (and the pad words, which no
kernel owns) are compared word for word with tests/tab_model.py."""
import ctypes
import os
import random

import numpy as np
import pytest

import tab_model
from tab_model import NONE, TAB_NEW
from vm_helpers import ROOT

pytestmark = pytest.mark.gpu

PROBE = os.path.join(ROOT, "tests", "device", "_build", "libtabprobe.so")
u32p = ctypes.POINTER(ctypes.c_uint32)
u32 = ctypes.c_uint32
FILL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(PROBE):
        pytest.fail("%s is missing: run build() (make -C consensus_overlord_amd) first" % PROBE)
    lib = ctypes.CDLL(PROBE)
    lib.tp_tab_build.argtypes = [u32] * 6 + [u32p] * 7
    lib.tp_tab_build.restype = ctypes.c_int
    lib.tp_round_remap.argtypes = [u32] * 3 + [u32p] * 6
    lib.tp_round_remap.restype = ctypes.c_int
    for f in (lib.tp_guard, lib.tp_round_words, lib.tp_r_off):
        f.restype = u32
    lib.tp_round_words.argtypes = lib.tp_r_off.argtypes = [u32]
    return lib


def _p(a):
    return a.ctypes.data_as(u32p)


def _cap(n):
    cap = 64
    while cap < n:
        cap <<= 1
    return cap


def _src(kind, no, nn):
    """-> (src[nn], the number of compacted new keys)"""
    new = lambda j: TAB_NEW | j   # noqa: E731
    if kind == "identity":
        return [i if i < no else new(i - no) for i in range(nn)], max(nn - no, 0)
    if kind == "reversal":
        return [no - 1 - i if i < no else new(i - no) for i in range(nn)], max(nn - no, 0)
    if kind == "rotation":
        return [(i + 1) % no if i < no else new(i - no) for i in range(nn)], max(nn - no, 0)
    if kind == "all_new":
        return [new(nn - 1 - i) for i in range(nn)], nn
    assert kind == "duplicates"      # none new: every second entry names the key of the one before
    return [(i // 2 * 3) % no for i in range(nn)], 0


@pytest.mark.parametrize("no,nn", [(1, 1), (5, 6), (6, 5), (64, 65), (65, 130)])
@pytest.mark.parametrize("kind", ["identity", "reversal", "rotation", "all_new", "duplicates"])
def test_tab_build(probe, kind, no, nn):
    src, nf = _src(kind, no, nn)
    co, cf, cn, G = _cap(no), _cap(max(nf, 1)), _cap(nn), probe.tp_guard()
    assert (co, cn) == {(1, 1): (64, 64), (5, 6): (64, 64), (6, 5): (64, 64), (64, 65): (64, 128),
                        (65, 130): (128, 256)}[(no, nn)]
    w, e = np.meshgrid(np.arange(36, dtype=np.uint32), np.arange(co, dtype=np.uint32), indexing="ij")
    old = (0x10000000 | (w << 16) | e).astype(np.uint32)            # [36][cap]: a word per (word, entry)
    w, e = np.meshgrid(np.arange(36, dtype=np.uint32), np.arange(cf, dtype=np.uint32), indexing="ij")
    fresh = (0x20000000 | (w << 16) | e).astype(np.uint32)
    oflags = (0x40000000 | np.arange(co, dtype=np.uint32)).astype(np.uint32)
    fflags = (0x50000000 | np.arange(cf, dtype=np.uint32)).astype(np.uint32)
    asrc = np.array(src, dtype=np.uint32)
    out = np.zeros(36 * cn + G, dtype=np.uint32)
    flags = np.zeros(cn + G, dtype=np.uint32)
    old_c, fresh_c = np.ascontiguousarray(old), np.ascontiguousarray(fresh)
    assert probe.tp_tab_build(nn, no, co, nf, cf, cn, _p(asrc), _p(old_c), _p(oflags), _p(fresh_c), _p(fflags), _p(out),
                              _p(flags)) == 0
    rows, want_flags = tab_model.build_table(src, old.tolist(), oflags.tolist(), fresh.tolist(), fflags.tolist())
    got = out[:36 * cn].reshape(36, cn)
    assert got[:, :nn].tolist() == rows
    assert flags[:nn].tolist() == want_flags
    assert (got[:, nn:] == FILL).all() and (flags[nn:cn] == FILL).all()         # no entry beyond n is written
    assert (out[36 * cn:] == FILL).all() and (flags[cn:] == FILL).all()         # the guards


def test_tab_build_refuses_a_source_out_of_range(probe):
    z = np.zeros(36 * 64 + 64, dtype=np.uint32)
    bad = np.array([5], dtype=np.uint32)
    assert probe.tp_tab_build(1, 5, 64, 0, 64, 64, _p(bad), _p(z), _p(z), _p(z), _p(z), _p(z), _p(z)) != 0
    bad = np.array([TAB_NEW | 0], dtype=np.uint32)
    assert probe.tp_tab_build(1, 5, 64, 0, 64, 64, _p(bad), _p(z), _p(z), _p(z), _p(z), _p(z), _p(z)) != 0


def _tables(rng, tno, tnn):
    """Key lists of tno and tnn entries: the new one is the old one rotated (bits move across byte
    and word boundaries), without old entry 3 and -- when it has to shrink -- the entries in front
    of the last, with new keys put in to reach tnn; one key is listed twice on either side."""
    old = [rng.randbytes(48) for _ in range(tno)]
    old[9] = old[4]
    keep = [k for e, k in enumerate(old) if e != 3]
    while len(keep) > tnn - 3:
        del keep[-2]
    s = 11 % len(keep)
    new = keep[s:] + keep[:s]
    while len(new) < tnn - 1:
        new.insert(rng.randrange(len(new) + 1), rng.randbytes(48))
    new.insert(rng.randrange(len(new) + 1), old[1])
    assert len(new) == tnn and new.count(old[1]) == 2
    return old, new


@pytest.mark.parametrize("tno,tnn", [(31, 32), (32, 33), (33, 31), (64, 65), (65, 64), (32, 32), (33, 64), (65, 33)])
def test_round_remap(probe, tno, tnn):
    rng = random.Random("remap %d %d" % (tno, tnn))
    old, new = _tables(rng, tno, tnn)
    d, do = tab_model.diff(old, new), tab_model.diff([], old)
    first = [e for e in range(tno) if old.index(old[e]) == e]        # the entries a vote can index
    alive = [e for e in first if d["dst"][e] != NONE]
    dead = [e for e in first if d["dst"][e] == NONE]
    assert 3 in dead and 0 in alive and tno - 1 in alive
    moved = [e for e in alive if do["rank"][e] // 32 != d["rank"][d["dst"][e]] // 32]
    if tno > 32 or tnn > 32:
        assert moved
    sets = [[], first, [0], [tno - 1], alive, [dead[0]], moved]
    while len(sets) < 16:
        pick = [e for e in alive if rng.random() < rng.choice((0.2, 0.5, 0.9))]
        sets.append(pick + ([rng.choice(dead)] if len(sets) % 3 == 0 else []))
    K, G = 16, probe.tp_guard()
    wo, wn = probe.tp_round_words(tno), probe.tp_round_words(tnn)
    assert (wo, wn) == (tab_model.round_words(tno), tab_model.round_words(tnn))
    assert probe.tp_r_off(tnn) == tab_model.r_off(tnn)
    state, want, want_lost = [], [], []
    for taken in sets:
        claims = rng.sample(range(1 << 24), tno)
        owner = [claims[e] if e in taken else NONE for e in range(tno)]
        merged = len(taken) if rng.random() < 0.7 else rng.randrange(len(taken) + 1)
        w = tab_model.make_round(tno, do["rank"], owner, merged, [rng.getrandbits(32) for _ in range(96)])
        state += w
        nw, lost = tab_model.remap_round(w, tno, tnn, d["rsrc"], d["dst"], d["sorted"])
        assert lost == int(any(e in dead for e in taken))
        want.append(nw)
        want_lost.append(lost)
    assert want_lost[:7] == [0, 1, 0, 0, 0, 1, 0]
    old_state = np.array(state, dtype=np.uint32)
    new_state = np.zeros(K * (wn + 2 * G), dtype=np.uint32)
    lost = np.full(K, 7, dtype=np.uint32)
    rsrc, dst, order = (np.array(d[k], dtype=np.uint32) for k in ("rsrc", "dst", "sorted"))
    assert probe.tp_round_remap(K, tno, tnn, _p(rsrc), _p(dst), _p(order), _p(old_state), _p(new_state), _p(lost)) == 0
    assert lost.tolist() == want_lost
    bw, off = (tnn + 31) // 32, tab_model.r_off(tnn)
    for r in range(K):
        got = new_state[r * (wn + 2 * G):(r + 1) * (wn + 2 * G)].tolist()
        assert got[:G] == [FILL] * G and got[G + wn:] == [FILL] * G, r                 # the guards
        got = got[G:G + wn]
        exp = [FILL if x is None else x for x in want[r]]                               # the pad keeps the fill
        assert got[:tnn] == exp[:tnn], ("owner", r)
        assert got[tnn:tnn + bw] == exp[tnn:tnn + bw], ("bitmap", r)
        assert got[tnn + bw:tnn + bw + 2] == exp[tnn + bw:tnn + bw + 2], ("count, merged", r)
        assert got[tnn + bw + 2:off] == exp[tnn + bw + 2:off], ("pad", r)
        assert got[off:off + 72] == exp[off:off + 72], ("R", r)
        assert got[off + 72:] == exp[off + 72:], ("96 bytes", r)
        # the pad bits of the last bitmap word are 0
        if tnn % 32:
            bm = b"".join(x.to_bytes(4, "little") for x in got[tnn:tnn + bw])
            assert all(not bm[k // 8] & (0x80 >> (k % 8)) for k in range(tnn, 32 * bw)), r
