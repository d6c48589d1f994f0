"""The selection rule of ovh_build_qc (include/ovhip.h) in plain Python: the specification the
GPU tests compare the device against (test infrastructure, no crypto)."""
from typing import List, Sequence, Tuple


def select(codes: Sequence[int], voters: Sequence[bytes], table: Sequence[bytes]) -> Tuple[List[int], bytes, int]:
    """-> (taken[n] as 0 / 1, bitmap, n_signed). Vote i is taken iff codes[i] == 0, its voter is
    in the validator table, and no vote with a lower index is taken for the same voter. The
    bitmap is MSB first over the table sorted by key bytes (vote.extract_voters order),
    ceil(len(table) / 8) bytes; a key that occurs twice in the table counts at its first
    position in sorted order."""
    rank = {}
    for k, key in enumerate(sorted(bytes(t) for t in table)):
        rank.setdefault(key, k)
    bitmap = bytearray((len(table) + 7) // 8)
    taken, seen = [], set()
    for code, voter in zip(codes, voters):
        voter = bytes(voter)
        ok = int(code) == 0 and voter in rank and voter not in seen
        taken.append(1 if ok else 0)
        if ok:
            seen.add(voter)
            k = rank[voter]
            bitmap[k // 8] |= 0x80 >> (k % 8)
    return taken, bytes(bitmap), sum(taken)
