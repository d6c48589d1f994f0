"""The rule of ovh_rounds_add (include/ovhip.h) in plain Python: one round_model.RoundModel per
open round, and a call that feeds each round the sub-list of its votes in the caller's order (test
infrastructure, no crypto). Rounds are keyed by their id, not by their hash: two rounds opened on
one hash stay two rounds."""
from typing import Dict, Hashable, List, Sequence, Tuple

import round_model


class RoundsModel:
    def __init__(self, table: Sequence[bytes]):
        self.table = [bytes(t) for t in table]
        self.rounds: Dict[Hashable, round_model.RoundModel] = {}

    def open(self, rid: Hashable) -> None:
        assert rid not in self.rounds
        self.rounds[rid] = round_model.RoundModel(self.table)

    def add(self, rids: Sequence[Hashable], codes: Sequence[int], voters: Sequence[bytes]):
        """One call: vote i is for round rids[i]. -> (taken per vote, slot per vote, per distinct
        round in order of first appearance: (rid, cumulative bitmap, cumulative n_signed))"""
        assert len(rids) == len(codes) == len(voters)
        order: List[Hashable] = []
        for r in rids:
            if r not in order:
                order.append(r)
        taken = [0] * len(rids)
        per_round: List[Tuple[Hashable, bytes, int]] = []
        for r in order:
            idx = [i for i, x in enumerate(rids) if x == r]
            t, bitmap, cnt = self.rounds[r].add([codes[i] for i in idx], [voters[i] for i in idx])
            for i, v in zip(idx, t):
                taken[i] = v
            per_round.append((r, bitmap, cnt))
        return taken, [order.index(r) for r in rids], per_round
