"""ovh_update_validators (include/ovhip.h) in plain Python: the host diff of two key lists
(csrc/tab_diff.hpp), the re-tabling of a round model, and the device words that k_tab_build and
k_round_remap (csrc/tab_update.hpp) must leave -- the specification the tests compare the harness,
the probe and the device with (test infrastructure, no crypto).

round_model.RoundModel is keyed by voter bytes, so re-tabling a round is: recompute the bitmap over
the new sorted table; closed if a taken voter is missing."""
import random
from typing import List, Optional, Sequence

import round_model

TAB_NEW = 0x80000000
NONE = 0xFFFFFFFF


def diff(old: Sequence[bytes], new: Sequence[bytes]) -> dict:
    """-> same, src, fresh, dst, rsrc, sorted, rank, kept (TabDiff's fields). Duplicate keys: a
    lookup gives a key's first entry; the stable sort puts that entry first among equals."""
    old, new = [bytes(k) for k in old], [bytes(k) for k in new]
    if old == new:
        return {"same": True}
    fresh, src, rsrc = [], [], []
    for i, k in enumerate(new):
        if k in old:
            src.append(old.index(k))
            rsrc.append(old.index(k) if new.index(k) == i else NONE)
        else:
            first = new.index(k)
            if first == i:
                fresh.append(i)
            src.append(TAB_NEW | fresh.index(first))
            rsrc.append(NONE)
    dst = [new.index(k) if k in new else NONE for k in old]
    order = sorted(range(len(new)), key=lambda i: (new[i], i))
    rank = [0] * len(new)
    for k, e in enumerate(order):
        rank[e] = k
    return {"same": False, "src": src, "fresh": fresh, "dst": dst, "rsrc": rsrc, "sorted": order, "rank": rank,
            "kept": sum(1 for s in src if not s & TAB_NEW)}


def retable(m: round_model.RoundModel, new: Sequence[bytes]) -> Optional[round_model.RoundModel]:
    """The round on the new table: None when it is closed (a taken voter is not a key of the new
    list, or the list is empty), else a model with the same claims, count and base whose bitmap is
    recomputed in the new key order."""
    new = [bytes(k) for k in new]
    if not new or any(v not in new for v in m.owner):
        return None
    r = round_model.RoundModel(new)
    r.owner = dict(m.owner)
    r.base = m.base
    r.n_signed = m.n_signed
    order = sorted(new)
    for v in m.owner:
        k = order.index(v)
        r.bitmap[k // 8] |= 0x80 >> (k % 8)
    return r


def state(m: round_model.RoundModel):
    """what the comparison of two round models looks at"""
    return (m.table, dict(m.owner), bytes(m.bitmap), m.n_signed, m.base)


# ---------------------------------------------------------------------------- device words
def r_off(tn: int) -> int:
    """QcRound's layout: owner (tn) | bitmap (bw) | count | merged | pad to 16 words | R (72) | 96 bytes"""
    return (tn + (tn + 31) // 32 + 2 + 15) // 16 * 16


def round_words(tn: int) -> int:
    return r_off(tn) + 72 + 24


def bitmap_words(tn: int, ranks) -> List[int]:
    """the bitmap of the taken ranks as the device keeps it: MSB-first bytes read as little-endian words"""
    b = bytearray((tn + 31) // 32 * 4)
    for k in ranks:
        b[k // 8] |= 0x80 >> (k % 8)
    return [int.from_bytes(b[4 * w:4 * w + 4], "little") for w in range(len(b) // 4)]


def make_round(tn: int, rank: Sequence[int], owner: Sequence[int], merged: int, tail: Sequence[int]) -> List[int]:
    """A round's words on a table of tn entries: owner words as given (NONE: not taken), the bitmap
    and the count that follow from them, `merged`, zero pad, and the 96 words of R and the output."""
    assert len(owner) == tn and len(tail) == 96
    taken = [e for e in range(tn) if owner[e] != NONE]
    w = list(owner) + bitmap_words(tn, [rank[e] for e in taken]) + [len(taken), merged]
    return w + [0] * (r_off(tn) - len(w)) + list(tail)


def remap_round(old_words: Sequence[int], tn_old: int, tn_new: int, rsrc, dst, order):
    """k_round_remap on one round -> (the new allocation's words with None where the kernel writes
    nothing (the pad), lost)"""
    bwo = (tn_old + 31) // 32
    owner_old = list(old_words[:tn_old])
    owner = [NONE if s == NONE else owner_old[s] for s in rsrc]
    rank = {e: k for k, e in enumerate(order)}
    w = owner + bitmap_words(tn_new, [rank[e] for e in range(tn_new) if owner[e] != NONE])
    w += list(old_words[tn_old + bwo:tn_old + bwo + 2])
    w += [None] * (r_off(tn_new) - len(w)) + list(old_words[r_off(tn_old):r_off(tn_old) + 96])
    lost = int(any(owner_old[o] != NONE and dst[o] == NONE for o in range(tn_old)))
    return w, lost


def build_table(src, old_planes, old_flags, fresh_planes, fresh_flags):
    """k_tab_build: planes as [36][entries] lists -> (36 rows of the new entries, flags)"""
    rows = [[(fresh_planes if s & TAB_NEW else old_planes)[w][s & ~TAB_NEW] for s in src] for w in range(36)]
    return rows, [(fresh_flags if s & TAB_NEW else old_flags)[s & ~TAB_NEW] for s in src]


# ---------------------------------------------------------------------------- seeded cases
KINDS = ("identity", "permutation", "add", "remove", "swap", "all_new", "empty")


def case(rng: random.Random, kind: str):
    """(old, new) key lists: old has 1 to 40 keys, sometimes one listed twice"""
    n = rng.randrange(1, 41)
    old = [rng.randbytes(48) for _ in range(n)]
    if n > 2 and rng.random() < 0.4:
        old[rng.randrange(1, n)] = old[0]
    new = list(old)
    if kind == "permutation":
        rng.shuffle(new)
    elif kind == "add":
        new.insert(rng.randrange(n + 1), rng.randbytes(48))
    elif kind == "remove":
        del new[rng.randrange(n)]
    elif kind == "swap":
        new[rng.randrange(n)] = rng.randbytes(48)
    elif kind == "all_new":
        new = [rng.randbytes(48) for _ in range(rng.randrange(1, 41))]
        if len(new) > 2 and rng.random() < 0.4:
            new[-1] = new[0]
    elif kind == "empty":
        new = []
    else:
        assert kind == "identity"
    return old, new
