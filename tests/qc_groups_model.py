"""The grouping and selection rule of ovh_build_qcs (include/ovhip.h) in plain Python: the
specification the GPU tests compare the device against (test infrastructure, no crypto). The
groups are the distinct hashes, numbered by first appearance; inside a group the rule is
ovh_build_qc's (tests/qc_model.py)."""
from typing import List, Sequence, Tuple

import qc_model


def select(codes: Sequence[int], hashes: Sequence[bytes], voters: Sequence[bytes], table: Sequence[bytes]
           ) -> Tuple[List[int], List[bytes], List[int], List[bytes], List[int]]:
    """-> (group[n], group_hashes[G], taken[n] as 0 / 1, bitmaps[G], n_signed[G])."""
    number, group = {}, []
    for h in hashes:
        group.append(number.setdefault(bytes(h), len(number)))
    ghashes = sorted(number, key=number.get)
    taken = [0] * len(group)
    bitmaps, counts = [], []
    for g in range(len(ghashes)):
        idx = [i for i, x in enumerate(group) if x == g]
        tk, bm, cnt = qc_model.select([codes[i] for i in idx], [voters[i] for i in idx], table)
        for i, x in zip(idx, tk):
            taken[i] = x
        bitmaps.append(bm)
        counts.append(cnt)
    return group, ghashes, taken, bitmaps, counts
