"""The selection rule of ovh_round_add (include/ovhip.h) in plain Python: qc_model.select folded
over the pieces of a round with a running `base`, as the device does it (test infrastructure, no
crypto). A claim is base + the vote's index in its add, kept per voter across adds: one of an
earlier add is below every later base, so it always wins."""
from typing import Dict, List, Sequence, Tuple

import qc_model

LOST = -1   # a code no verify returns: the vote of a voter whose claim an earlier add holds


class RoundModel:
    def __init__(self, table: Sequence[bytes]):
        self.table = [bytes(t) for t in table]
        self.owner: Dict[bytes, int] = {}          # voter -> the claim that holds it
        self.bitmap = bytearray((len(self.table) + 7) // 8)
        self.n_signed = 0
        self.base = 0                               # votes added so far

    def add(self, codes: Sequence[int], voters: Sequence[bytes]) -> Tuple[List[int], bytes, int]:
        """-> (taken of this add's votes, cumulative bitmap, cumulative n_signed)"""
        voters = [bytes(v) for v in voters]
        assert all(c < self.base for c in self.owner.values())
        masked = [LOST if v in self.owner else int(c) for c, v in zip(codes, voters)]
        taken, bitmap, cnt = qc_model.select(masked, voters, self.table)
        for i, (t, v) in enumerate(zip(taken, voters)):
            if t:
                self.owner[v] = self.base + i
        self.bitmap = bytearray(a | b for a, b in zip(self.bitmap, bitmap))
        self.n_signed += cnt
        self.base += len(voters)
        return taken, bytes(self.bitmap), self.n_signed


def fold(codes: Sequence[int], voters: Sequence[bytes], table: Sequence[bytes], cut: Sequence[int]):
    """The votes added in consecutive pieces of the sizes in `cut` -> (concatenated taken, final
    bitmap, final n_signed, [(bitmap, n_signed) after each add])."""
    assert sum(cut) == len(codes) == len(voters)
    m = RoundModel(table)
    taken, steps, lo = [], [], 0
    for k in cut:
        t, bitmap, cnt = m.add(codes[lo:lo + k], voters[lo:lo + k])
        taken += t
        steps.append((bitmap, cnt))
        lo += k
    return taken, bytes(m.bitmap), m.n_signed, steps
