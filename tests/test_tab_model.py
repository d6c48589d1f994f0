"""CPU checks of the model of ovh_update_validators (tests/tab_model.py), the specification the host
harness, the probe and the device tests compare with.

The law: a re-tabled round model, continued with further adds, equals a fresh RoundModel on the new
table that was fed T (the votes the round had taken, in order) and then the same adds -- taken flags,
bitmap and count after every add. Inputs are seeded: tables of 1 to 40 keys with duplicates, each of
identity, permutation, one add, one removal, one swap, all-new and empty. The comparison itself is
checked to notice a perturbed bitmap bit and a perturbed owner map, and the diff's maps are checked
against their definitions."""
import random

import pytest
import qc_model
import round_model
import tab_model
from tab_model import NONE, TAB_NEW

SEEDS = range(40)


def _votes(rng, pool, n):
    voters = [rng.choice(pool) for _ in range(n)]
    codes = [rng.choice((0, 0, 0, 5, 3, 102)) for _ in range(n)]
    return codes, voters


def _seen(m):
    """what a caller can see of a round, and what decides its future: bitmap, count, taken voters"""
    return bytes(m.bitmap), m.n_signed, frozenset(m.owner)


def _run(rng, old, new):
    """-> (re-tabled model or None, fresh model fed T or None, the pool of voters)"""
    pool = old + new + [rng.randbytes(48) for _ in range(3)]
    m = round_model.RoundModel(old)
    T = []
    for _ in range(rng.randrange(0, 4)):
        codes, voters = _votes(rng, pool, rng.randrange(1, 30))
        taken, _, _ = m.add(codes, voters)
        T += [v for t, v in zip(taken, voters) if t]
    r = tab_model.retable(m, new)
    if r is None:
        assert not new or any(v not in new for v in T)
        return None, None, pool
    assert all(v in new for v in T)
    f = round_model.RoundModel(new)
    if T:
        taken, _, _ = f.add([0] * len(T), T)
        assert taken == [1] * len(T)      # every taken voter is a key of the new list, once
    return r, f, pool


@pytest.mark.parametrize("kind", tab_model.KINDS)
def test_retabled_round_continues_as_a_fresh_round_fed_the_taken_votes(kind):
    closed = carried = 0
    for seed in SEEDS:
        rng = random.Random("%s/%d" % (kind, seed))
        old, new = tab_model.case(rng, kind)
        r, f, pool = _run(rng, old, new)
        if r is None:
            closed += 1
            continue
        carried += 1
        assert _seen(r) == _seen(f), (kind, seed)
        assert len(r.bitmap) == (len(new) + 7) // 8
        for _ in range(3):
            codes, voters = _votes(rng, pool, rng.randrange(1, 30))
            assert r.add(codes, voters) == f.add(codes, voters), (kind, seed)
            assert _seen(r) == _seen(f)
    if kind == "empty":
        assert carried == 0 and closed == len(SEEDS)
    elif kind in ("identity", "permutation", "add"):
        assert closed == 0                    # no key is dropped
    else:
        assert carried and closed             # both outcomes are exercised


def test_the_comparison_notices_a_perturbed_bitmap_bit_and_owner_map():
    rng = random.Random(7)
    old = [rng.randbytes(48) for _ in range(12)]
    new = old[3:] + old[:3] + [rng.randbytes(48)]
    m = round_model.RoundModel(old)
    m.add([0] * 5, old[:5])
    r = tab_model.retable(m, new)
    f = round_model.RoundModel(new)
    f.add([0] * 5, old[:5])
    assert _seen(r) == _seen(f)
    bad = tab_model.retable(m, new)
    bad.bitmap[0] ^= 0x10
    assert _seen(bad) != _seen(f)
    bad = tab_model.retable(m, new)
    del bad.owner[old[2]]
    assert _seen(bad) != _seen(f)
    assert bad.add([0], [old[2]])[0] != f.add([0], [old[2]])[0]     # and it would take the voter twice
    bad = tab_model.retable(m, new)
    bad.owner[new[-1]] = 0
    assert bad.add([0], [new[-1]])[0] == [0] and f.add([0], [new[-1]])[0] == [1]


@pytest.mark.parametrize("kind", tab_model.KINDS)
def test_diff_maps_against_their_definitions(kind):
    for seed in SEEDS:
        rng = random.Random("d%s/%d" % (kind, seed))
        old, new = tab_model.case(rng, kind)
        d = tab_model.diff(old, new)
        assert d["same"] == (old == new)
        if d["same"]:
            continue
        fresh_keys = [new[i] for i in d["fresh"]]
        assert len(set(fresh_keys)) == len(fresh_keys) and not set(fresh_keys) & set(old)
        for i, s in enumerate(d["src"]):
            if s & TAB_NEW:
                assert new[i] not in old and fresh_keys[s & ~TAB_NEW] == new[i]
            else:
                assert old[s] == new[i] and old.index(new[i]) == s
            first = new.index(new[i]) == i
            assert d["rsrc"][i] == (s if first and not s & TAB_NEW else NONE)
        for o, t in enumerate(d["dst"]):
            assert t == (new.index(old[o]) if old[o] in new else NONE)
        assert d["kept"] == sum(1 for k in new if k in old)
        assert sorted(d["sorted"]) == list(range(len(new)))
        assert [new[e] for e in d["sorted"]] == sorted(new)
        for k, e in enumerate(d["sorted"]):
            assert d["rank"][e] == k
            if k and new[d["sorted"][k - 1]] == new[e]:
                assert d["sorted"][k - 1] < e                       # stable
        # the rank of a key's first entry is the bit qc_model.select gives the key
        for e, key in enumerate(new):
            if new.index(key) == e:
                assert qc_model.select([0], [key], new)[1] == bytes(
                    (0x80 >> (d["rank"][e] % 8)) if b == d["rank"][e] // 8 else 0 for b in range((len(new) + 7) // 8))


def test_device_words_of_a_remapped_round():
    # 5 -> 6 entries: entry 1 is dropped, a new key arrives in front, the rest rotate
    old = [bytes([b]) * 48 for b in (0x50, 0x10, 0x30, 0x20, 0x40)]
    new = [bytes([0x05]) * 48, old[4], old[0], old[2], old[3], bytes([0x60]) * 48]
    d, do = tab_model.diff(old, new), tab_model.diff([], old)
    tail = list(range(1000, 1096))
    for taken, lost in (((0, 3), 0), ((1,), 1), ((), 0)):
        owner = [7 + e if e in taken else NONE for e in range(5)]
        w = tab_model.make_round(5, do["rank"], owner, len(taken), tail)
        assert len(w) == tab_model.round_words(5) == 16 + 96
        got, gl = tab_model.remap_round(w, 5, 6, d["rsrc"], d["dst"], d["sorted"])
        assert gl == lost and len(got) == tab_model.round_words(6)
        m = round_model.RoundModel(old)
        m.add([0] * len(taken), [old[e] for e in taken])
        if lost:
            assert tab_model.retable(m, new) is None
            continue
        want = tab_model.retable(m, new)
        assert got[:6] == [owner[s] if s != NONE else NONE for s in d["rsrc"]]
        assert got[6].to_bytes(4, "little")[:1] == bytes(want.bitmap) and got[6] >> 8 == 0
        assert got[7:9] == [len(taken), len(taken)] and got[16:] == tail
