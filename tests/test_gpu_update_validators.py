"""ovh_update_validators end to end (include/ovhip.h): a validator update
that keeps the device table and the open rounds. Keys and votes are signed on the device as the
round tests do; tables have 5 to 8, 33 and 64 to 68 keys and no list is longer than 67 votes.
Expected values come from the Python models (qc_model, round_model, tab_model), the C oracle and
ovh_set_validators on a second context, never from the call under test.

1. Table equivalence: context A does set_validators(old) then update(new), context B does
   set_validators(new); verify_batch over votes of kept, added and dropped voters, verify_qc_batch on
   bitmaps in the new order, build_qc_raw's codes, taken, bitmap, count and bytes and the table route
   of ovh_verify_aggregated agree between A, B and the oracle -- for identical, permuted, one added
   (7 -> 8, 64 -> 65: the cap grows), one removed, one swapped at 67, a duplicated key, and a key
   that does not parse and a key outside G1 (tests/point_cases.py), once kept and once new.
2. The counters of ovh_table_stats.
3. Round continuity: the corrupted 67-vote round of test_gpu_build_qc._make_round cut into adds with
   the update between two of them (identical, permuted, the outside voter added, an untaken
   validator removed): after every add the codes, taken, count, bitmap and 96 bytes equal the
   re-tabled RoundModel and the oracle's aggregate of the taken votes.
4. Closed rounds: only the round that took the dropped voter is closed; n == 0 closes all.
5. ovh_rounds_add over two carried rounds. 6. Batches in flight. 7. A multi-device context {0, 0}."""
import numpy as np
import pytest

import orc
import qc_model
import round_model
import synth_votes as sv
import tab_model
from test_gpu_build_qc import _make_round, _oracle_codes, _votes
from test_gpu_rounds import _add_in_pieces, _prefix_qc

pytestmark = pytest.mark.gpu

D = sv.sha(b"update_validators pool")
D67 = sv.sha(b"update_validators round 67")


def _new_cc(key, **kw):
    import consensus_overlord_amd as coa
    from consensus_overlord_amd.crypto import Context
    return coa.ConsensusCrypto(bytes.fromhex(key * 32), ctx=Context(**kw) if kw else None)


@pytest.fixture(scope="module")
def A():
    return _new_cc("7d")


@pytest.fixture(scope="module")
def B():
    return _new_cc("7e")


@pytest.fixture(scope="module")
def pool(A):
    """70 (signature, key) votes on D, device-signed once and left unchanged"""
    return _votes(A.ctx, 150000, 70, D)


@pytest.fixture(scope="module")
def bad_keys():
    import point_cases as pc
    g1 = pc.by_class(pc.cases()[0], pc.G1_CLASSES)
    unparsed = next(c for c in g1["off_curve"] if c.parse == 2)
    outside = next(c for c in g1["small_order"] if c.parse == 0 and not c.in_group)
    return unparsed.enc, outside.enc


@pytest.fixture(scope="module")
def round67(A, golden):
    sigs, voters, table = _make_round(A.ctx, golden, 151000, 67, D67)
    want = _oracle_codes(sigs, D67, voters).tolist()
    assert sorted(set(want)) == [0, 3, 5, 102] and len(table) == 64
    return {"sigs": sigs, "voters": voters, "table": table, "want": want}


def _vagg(cc, agg, digest, voters):
    from consensus_overlord_amd.crypto import ConsensusError, CryptoErr
    try:
        cc.verify_aggregated_signature(agg, digest, voters)
        return 0
    except CryptoErr as e:
        return e.code
    except ConsensusError:
        return 102


def _keep_update(cc, keys):
    closed = cc.update_pubkeys(keys, keep_rounds=True)
    assert isinstance(closed, list)
    return closed


def _same_table(A, B, new, votes, pool, routes=True):
    """every reader of the table on A (updated) and B (set) against each other and the oracle;
    votes: (sig, key) pairs on D, at most 67. routes: also that ovh_verify_aggregated takes its table
    route on both (single-device contexts, H(D) primed)"""
    from consensus_overlord_amd import vote
    assert len(votes) <= 67
    sigs, voters = [v[0] for v in votes], [v[1] for v in votes]
    want = _oracle_codes(sigs, D, voters).tolist()
    for cc in (A, B):
        assert cc.verify_batch(sigs, [D] * len(sigs), voters).tolist() == want
    # ovh_build_qc: the selection and the bitmap in the new key order
    m_taken, m_bitmap, m_cnt = qc_model.select(want, voters, new)
    ts = [s for s, t in zip(sigs, m_taken) if t]
    tv = [p for p, t in zip(voters, m_taken) if t]
    for cc in (A, B):
        code, agg, bitmap, codes, taken, cnt = cc.build_qc_raw(sigs, D, voters)
        assert codes.tolist() == want and taken.astype(int).tolist() == m_taken
        assert (bitmap, cnt, code) == (m_bitmap, m_cnt, 0 if m_cnt else 4)
        assert agg == (orc.aggregate_sigs(ts, tv)[1] if m_cnt else None)
    if not m_cnt:
        return
    agg = orc.aggregate_sigs(ts, tv)[1]
    # ovh_verify_qc_batch: the full bitmap, one with a bit cleared (the sum no longer matches), and --
    # where the table has an entry the QC did not take -- one with a bit too many
    maps = [m_bitmap]
    k = next(i for i in range(len(new)) if m_bitmap[i // 8] & (0x80 >> (i % 8)))
    maps.append(bytes(b ^ (0x80 >> (k % 8)) if i == k // 8 else b for i, b in enumerate(m_bitmap)))
    free = [i for i in range(len(new)) if not m_bitmap[i // 8] & (0x80 >> (i % 8))]
    if free:
        maps.append(bytes(b | (0x80 >> (free[0] % 8)) if i == free[0] // 8 else b for i, b in enumerate(m_bitmap)))
    want_qc = [orc.verify_aggregated(agg, D, vote.extract_voters(new, bm)) for bm in maps]
    assert want_qc[0] == 0
    for cc in (A, B):
        assert cc.verify_qc_batch([agg] * len(maps), [D] * len(maps), maps).tolist() == want_qc
    # ovh_verify_aggregated: explicit voters that are table keys take the table route (H(D) is in
    # the message cache), a list with a key outside the table the full path
    lists = [tv, tv[1:] if len(tv) > 1 else tv, tv + [pool[69][1]]]
    for cc in (A, B):
        cc.prime([D])
        before = cc.agg_stats()
        for vs in lists:
            assert _vagg(cc, agg, D, vs) == orc.verify_aggregated(agg, D, vs)
        if routes:
            assert [x - y for x, y in zip(cc.agg_stats(), before)][5:] == [2, 2, 1]


CASES = {
    # name: (old entries, new entries) as indices into the pool; "u" / "g": the key that does not
    # parse / the key outside G1
    "identical": (range(7), range(7)),
    "permuted": (range(7), (3, 0, 6, 5, 1, 2, 4)),
    "added_7_8": (range(7), (0, 1, 2, 60, 3, 4, 5, 6)),
    "added_64_65": (range(64), tuple(range(64)) + (64,)),
    "removed": (range(8), (0, 1, 2, 4, 5, 6, 7)),
    "swapped_67": (range(67), tuple(range(30)) + (67,) + tuple(range(31, 67))),
    "duplicated": (range(6), (0, 1, 5, 1, 2, 3, 4)),
    "shrunk_33_5": (range(33), (32, 0, 31, 7, 8)),
    "bad_kept": ((0, "u", 1, 2, "g", 3), (3, "g", 0, 4, "u", 1)),
    "bad_new": ((0, 1, 2, 3, 4), (0, "u", 1, 2, 5, "g", 3)),
}


def _lists(name, pool, bad_keys):
    key = lambda x: bad_keys[0] if x == "u" else bad_keys[1] if x == "g" else pool[x][1]   # noqa: E731
    oi, ni = (list(x) for x in CASES[name])
    old, new = [key(x) for x in oi], [key(x) for x in ni]
    # votes of kept voters (the first 60), then of every added and every dropped one, a vote of an
    # outsider, and -- under a signature of another voter -- of the two bad keys where they occur
    kept = [x for x in ni if x in oi and x not in ("u", "g")]
    other = [x for x in list(dict.fromkeys(ni + oi)) if x not in kept and x not in ("u", "g")]
    votes = [pool[x] for x in kept[:60] + other] + [pool[68]]
    votes += [(pool[0][0], key(x)) for x in ("u", "g") if x in oi + ni]
    return old, new, votes


@pytest.mark.parametrize("name", list(CASES))
def test_table_equivalence(A, B, pool, bad_keys, name):
    old, new, votes = _lists(name, pool, bad_keys)
    A.update_pubkeys(old)
    s0 = A.table_stats()
    assert _keep_update(A, new) == []
    s1 = A.table_stats()
    B.update_pubkeys(new)
    assert A.pubkeys == B.pubkeys == new
    d = tab_model.diff(old, new)
    if d["same"]:
        assert [b - a for a, b in zip(s0, s1)] == [0, 1, 0, 0, 0, 0, 0, 0]
    else:
        assert [b - a for a, b in zip(s0, s1)] == [0, 0, 1, len(d["fresh"]), d["kept"], 0, 0, len(new) - len(old)]
    _same_table(A, B, new, votes, pool)
    if name in ("bad_kept", "bad_new"):
        want = _oracle_codes([v[0] for v in votes], D, [v[1] for v in votes]).tolist()
        assert want[-2:] == [102, 3]          # the key that does not parse, the key outside G1


def test_counters(A, pool):
    keys = [v[1] for v in pool]
    A.update_pubkeys(keys[:67])
    s = [A.table_stats()]
    _keep_update(A, keys[:67])                              # identical
    s.append(A.table_stats())
    _keep_update(A, keys[:30] + keys[67:68] + keys[30:67])  # one added at 67
    s.append(A.table_stats())
    _keep_update(A, keys[29::-1] + keys[67:68] + keys[30:67])   # a permutation of the 68
    s.append(A.table_stats())
    A.update_pubkeys(keys[:5])
    s.append(A.table_stats())
    delta = [[b - a for a, b in zip(x, y)][:7] for x, y in zip(s, s[1:])]
    assert delta[0] == [0, 1, 0, 0, 0, 0, 0]
    assert delta[1] == [0, 0, 1, 1, 67, 0, 0]
    assert delta[2] == [0, 0, 1, 0, 68, 0, 0]
    assert delta[3] == [1, 0, 0, 0, 0, 0, 0]                # [0] counts ovh_set_validators alone
    assert [x[7] for x in s] == [67, 67, 68, 68, 5]


def _continuity(cc, r, new_of, k1, resend=None):
    """r's votes in the adds (k1, 3, the rest), the update to new_of(table) after the first; with
    `resend` that vote is sent once more at the end. -> the round, the model, everything taken"""
    sigs, voters, want, table = list(r["sigs"]), list(r["voters"]), list(r["want"]), r["table"]
    if resend is not None:
        sigs.append(sigs[resend])
        voters.append(voters[resend])
        want.append(want[resend])
    cc.update_pubkeys(table)
    rd = cc.open_round(D67)
    model, taken_all, lo = _add_in_pieces(cc, rd, sigs, voters, table, want, (k1,))
    new = new_of(table)
    s0 = cc.table_stats()
    assert _keep_update(cc, new) == []
    s1 = cc.table_stats()
    assert s1[5] - s0[5] == (0 if new == table else 1) and s1[6] == s0[6]
    model = tab_model.retable(model, new)
    assert model is not None and rd.bitmap_len == (len(new) + 7) // 8
    # read at once, before any further add: the QC of the taken votes on the new table
    if model.n_signed:
        assert rd.qc() == (_prefix_qc(sigs[:lo], voters[:lo], taken_all), bytes(model.bitmap), model.n_signed)
    cut = (3, 67 - k1 - 3) + ((1,) if resend is not None else ())
    model, taken_all, lo = _add_in_pieces(cc, rd, sigs, voters, new, want, cut, model=model, taken_all=taken_all, lo=lo)
    assert lo == len(sigs)
    # the defining property of a carried round: a fresh round on the new table fed T, then the adds
    fresh = round_model.RoundModel(new)
    T = [voters[i] for i in range(k1) if taken_all[i]]
    if T:
        fresh.add([0] * len(T), T)
    fresh.add(want[k1:], voters[k1:])
    assert (bytes(fresh.bitmap), fresh.n_signed, set(fresh.owner)) == (bytes(model.bitmap), model.n_signed, set(model.owner))
    return rd, model, taken_all, sigs, voters, want


def test_round_across_an_identical_update_equals_build_qc(A, round67):
    rd, model, taken_all, sigs, voters, want = _continuity(A, round67, lambda t: list(t), 20)
    code, agg, bitmap, codes, taken, cnt = A.build_qc_raw(sigs, D67, voters)
    assert code == 0 and codes.tolist() == want
    assert taken.astype(int).tolist() == taken_all                # this is the existing defining property,
    assert rd.qc() == (agg, bitmap, cnt)                          # now across a commit
    rd.close()


def test_round_across_a_permuted_update(A, round67):
    rd, model, taken_all, sigs, voters, want = _continuity(A, round67, lambda t: t[::-1], 20)
    assert taken_all == qc_model.select(want, voters, round67["table"])[0]    # the same votes, another order
    rd.close()


def test_round_when_the_outside_voter_joins_the_table(A, round67):
    r = round67
    out = next(i for i, v in enumerate(r["voters"]) if v not in r["table"] and r["want"][i] == 0)
    k1 = max(out + 1, 20)
    assert k1 <= 60            # its first vote comes before the update, as a voter outside the table
    rd, model, taken_all, sigs, voters, want = _continuity(A, r, lambda t: t[:10] + [r["voters"][out]] + t[10:], k1,
                                                           resend=out)
    assert taken_all[out] == 0 and taken_all[-1] == 1             # re-sent after the update, it is taken
    assert model.n_signed == sum(qc_model.select(r["want"], r["voters"], r["table"])[0]) + 1
    rd.close()


def test_round_when_an_untaken_validator_leaves_the_table(A, round67):
    r = round67
    k1 = 20
    gone = next(v for v in r["table"] if v not in r["voters"][:k1] and r["want"][r["voters"].index(v)] == 0)
    rd, model, taken_all, sigs, voters, want = _continuity(A, r, lambda t: [k for k in t if k != gone], k1)
    i = voters.index(gone)
    assert i >= k1 and want[i] == 0 and taken_all[i] == 0         # verified, but no longer a table voter
    assert model.n_signed == sum(qc_model.select(want, voters, r["table"])[0]) - 1
    rd.close()


def _open_three(cc, pool, table):
    """three rounds on D over `table` (pool indices): they take the voters (0, 1), (2, last), (3,)"""
    keys = [pool[x][1] for x in table]
    cc.update_pubkeys(keys)
    rounds, models = [], []
    for idx in ((0, 1), (2, len(table) - 1), (3,)):
        rd, m = cc.open_round(D), round_model.RoundModel(keys)
        vs = [pool[table[i]] for i in idx]
        codes, taken, cnt = rd.add([v[0] for v in vs], [v[1] for v in vs])
        assert (codes.tolist(), taken.astype(int).tolist(), cnt) == ([0] * len(vs), [1] * len(vs), len(vs))
        m.add([0] * len(vs), [v[1] for v in vs])
        rounds.append(rd)
        models.append(m)
    return keys, rounds, models


def test_only_the_round_that_took_the_dropped_voter_is_closed(A, pool):
    table = list(range(8))
    keys, rounds, models = _open_three(A, pool, table)
    new = [keys[5], keys[0], keys[1], keys[2], keys[3], keys[4], pool[20][1], keys[6]]     # keys[7] is dropped
    s0 = A.table_stats()
    assert _keep_update(A, new) == [rounds[1].id]
    s1 = A.table_stats()
    assert (s1[5] - s0[5], s1[6] - s0[6]) == (2, 1)
    code = rounds[1].add_raw([pool[4][0]], [pool[4][1]])[0]
    assert code == 103
    with pytest.raises(ValueError):
        rounds[1].qc_raw()
    # the other two go on: a taken voter again, a new table key, an outsider, the dropped voter
    vs = [pool[0], pool[20], pool[3], pool[30], pool[7], pool[4]]
    for k in (0, 2):
        m = tab_model.retable(models[k], new)
        code, codes, taken, cnt, agg, bitmap = rounds[k].add_raw([v[0] for v in vs], [v[1] for v in vs], want_qc=True)
        m_taken, m_bitmap, m_cnt = m.add([0] * len(vs), [v[1] for v in vs])
        assert code == 0 and codes.tolist() == [0] * len(vs)
        assert (taken.astype(int).tolist(), bitmap, cnt) == (m_taken, m_bitmap, m_cnt)
        tv = [v for v in pool if v[1] in m.owner]
        assert agg == orc.aggregate_sigs([v[0] for v in tv], [v[1] for v in tv])[1]
        rounds[k].close()


def test_an_empty_list_closes_every_round(A, pool):
    keys, rounds, _ = _open_three(A, pool, list(range(5)))
    s0 = A.table_stats()
    assert sorted(_keep_update(A, [])) == sorted(r.id for r in rounds)
    s1 = A.table_stats()
    assert (s1[5] - s0[5], s1[6] - s0[6], s1[7]) == (0, 3, 0)
    for rd in rounds:
        assert rd.add_raw([pool[4][0]], [pool[4][1]])[0] == 103
    _keep_update(A, keys)                                   # from the empty table: every key is new
    s2 = A.table_stats()
    assert (s2[3] - s1[3], s2[4] - s1[4], s2[7]) == (5, 0, 5)
    with A.open_round(D) as rd:
        assert rd.add([pool[1][0]], [pool[1][1]])[2] == 1


def test_rounds_add_over_two_carried_rounds(A, pool):
    table = list(range(33))
    keys, rounds, models = _open_three(A, pool, table)
    new = keys[8:31] + [pool[40][1]] + keys[:8] + keys[31:]         # 34 keys: a rotation and one added
    assert _keep_update(A, new) == []
    r0, r2 = rounds[0], rounds[2]
    m0, m2 = tab_model.retable(models[0], new), tab_model.retable(models[2], new)
    # one flush over both: taken voters again, the new key in both, new votes, an outsider
    flush = [(r0, 0), (r2, 3), (r0, 40), (r2, 40), (r0, 9), (r2, 0), (r0, 50), (r2, 31), (r0, 32), (r2, 10)]
    codes, taken, per_round = A.add_rounds([r for r, _ in flush], [pool[x][0] for _, x in flush],
                                           [pool[x][1] for _, x in flush], want_qc=True)
    assert codes.tolist() == [0] * len(flush) and [p[0] for p in per_round] == [r0, r2]
    for (rd, cnt, agg, bitmap), m in zip(per_round, (m0, m2)):
        mine = [i for i, (r, _) in enumerate(flush) if r is rd]
        m_taken, m_bitmap, m_cnt = m.add([0] * len(mine), [pool[flush[i][1]][1] for i in mine])   # round_add's rule
        assert [int(taken[i]) for i in mine] == m_taken and (bitmap, cnt) == (m_bitmap, m_cnt)
        tv = [v for v in pool if v[1] in m.owner]
        assert agg == orc.aggregate_sigs([v[0] for v in tv], [v[1] for v in tv])[1]
        assert rd.qc() == (agg, bitmap, cnt)
    for rd in rounds:
        rd.close()


@pytest.mark.parametrize("changed", [False, True], ids=["identical", "changed"])
def test_batches_in_flight(A, pool, changed):
    keys = [v[1] for v in pool[:33]]
    A.update_pubkeys(keys)
    rng = np.random.default_rng(5)
    batches = []
    for b in range(6):
        idx = rng.permutation(40)[:24].tolist()                   # table voters and a few others
        sigs = [pool[i][0] if (i + b) % 5 else pool[(i + 1) % 40][0] for i in idx]     # some under a wrong signature
        voters = [pool[i][1] for i in idx]
        codes = np.full(len(idx), -7, dtype=np.int32)
        A.verify_batch_async(sigs, [D] * len(idx), voters, codes)
        batches.append((sigs, voters, codes))
    _keep_update(A, keys[::-1][:30] + [pool[50][1]] if changed else keys)
    A.wait()
    for sigs, voters, codes in batches:
        assert codes.tolist() == _oracle_codes(sigs, D, voters).tolist()
    st = A.table_stats()
    assert st[7] == (31 if changed else 33)


def test_multi_device_context(B, pool, round67):
    M = _new_cc("7f", devices=[0, 0])
    old, new, votes = _lists("added_7_8", pool, None)
    M.update_pubkeys(old)
    assert _keep_update(M, new) == []
    B.update_pubkeys(new)
    _same_table(M, B, new, votes, pool, routes=False)
    assert M.table_stats()[:5] == (1, 0, 1, 1, 7) and M.table_stats()[7] == 8
    rd, model, taken_all, sigs, voters, want = _continuity(M, round67, lambda t: list(t), 20)
    code, agg, bitmap, codes, taken, cnt = M.build_qc_raw(sigs, D67, voters)
    assert rd.qc() == (agg, bitmap, cnt) and taken.astype(int).tolist() == taken_all
    rd.close()
