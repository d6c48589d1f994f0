"""The ingress shim's one-pass flush (consensus_overlord_amd/ingress.py, rounds=True with a crypto
that has add_rounds) over a fake Crypto backed by the C oracle and the round model, as
OracleRoundCrypto of tests/test_ingress_rounds.py is: a flush over three hashes is one add_rounds
call in arrival order and one device pass, and qc(hash) per hash is the per-hash oracle result; a
flush on one hash still uses Round.add; an 18-hash flush is cut into calls of at most ROUNDS_MAX
rounds and never closes a round before it was added to; a crypto without add_rounds sees today's
call sequence."""
import orc
from consensus_overlord_amd import ingress as ig
from consensus_overlord_amd import vote
from test_ingress import sm3
from test_ingress_rounds import OracleRoundCrypto, _keys


class OracleRoundsCrypto(OracleRoundCrypto):
    """OracleRoundCrypto with add_rounds: every round gets the sub-list of its votes, in the
    caller's order, through its own OracleRound.add (the defining property of ovh_rounds_add)."""

    def add_rounds(self, rounds, signatures, voters, want_qc=False):
        assert not want_qc and len(rounds) == len(signatures) == len(voters)
        order = []
        for r in rounds:
            assert not r.closed, "add_rounds on a closed round"
            if r not in order:
                order.append(r)
        assert 2 <= len(order) <= ig.ROUNDS_MAX
        self.calls.append(("add_rounds", [r.hash for r in rounds]))
        codes, taken, per_round = [None] * len(rounds), [None] * len(rounds), []
        mark = len(self.calls)
        for r in order:
            idx = [i for i, x in enumerate(rounds) if x is r]
            c, t, cnt = r.add([signatures[i] for i in idx], [voters[i] for i in idx])
            for i, ci, ti in zip(idx, c, t):
                codes[i], taken[i] = ci, ti
            per_round.append((r, cnt, None, None))
        del self.calls[mark:]          # the per-round adds above are the fake's inside, not calls of the shim
        return codes, taken, per_round


def _vote(sks, pks, i, height, round_, kind, bh):
    d = sm3(vote.rlp_vote(height, round_, kind, bh))
    return d, ig.SignedVote(orc.sign(sks[i], d)[1], height, round_, kind, bh, pks[i])


def _shim(oc, fwd=None):
    return ig.VoteIngress(oc, (lambda k, m: fwd.append(m)) if fwd is not None else (lambda k, m: None), batch_size=1000,
                          max_delay_s=1e9, clock=lambda: 0.0, rounds=True)


def test_a_flush_over_three_hashes_is_one_pass():
    nval = 5
    sks, pks = _keys(b"rounds add", nval)
    bh = sm3(b"block 21")
    # the block's prevotes, two nil prevotes, late precommits of the previous round; one duplicate
    # and one vote signed with the wrong key among them
    plan = [(0, 4, vote.PREVOTE, bh), (1, 4, vote.PREVOTE, b""), (2, 4, vote.PREVOTE, bh), (3, 3, vote.PRECOMMIT, bh),
            (0, 4, vote.PREVOTE, bh), (4, 4, vote.PREVOTE, b""), (1, 3, vote.PRECOMMIT, bh), (3, 4, vote.PREVOTE, bh)]
    msgs = [_vote(sks, pks, i, 21, r, k, h) for i, r, k, h in plan]
    d_bad, m_bad = _vote(sks, pks, 2, 21, 3, vote.PRECOMMIT, bh)
    msgs.append((d_bad, ig.SignedVote(m_bad.signature, 21, 3, vote.PRECOMMIT, bh, pks[4])))     # pks[4] did not sign it
    oc = OracleRoundsCrypto(pks)
    fwd = []
    sh = _shim(oc, fwd)
    for _, m in msgs:
        sh.proc_network_msg("SignedVote", ig.encode_signed_vote(m))
    sh.flush()
    hashes = [d for d, _ in msgs]
    distinct = list(dict.fromkeys(hashes))
    assert len(distinct) == 3
    # all rounds are resolved before the one call, which carries the votes in arrival order
    assert oc.calls == [("open", h) for h in distinct] + [("add_rounds", hashes)]
    assert fwd == [m for _, m in msgs]
    assert sh.stats["round_passes"] == 1 and sh.stats["round_adds"] == 3 and sh.stats["round_votes"] == len(msgs)
    assert sh.stats["batches"] == 0
    for h in distinct:      # qc(hash): the per-hash oracle result over the first valid vote of each voter
        seen, sigs, voters = set(), [], []
        for d, m in msgs:
            if d == h and m.voter not in seen and orc.verify(m.signature, d, m.voter) == 0:
                seen.add(m.voter)
                sigs.append(m.signature)
                voters.append(m.voter)
        agg, bitmap, cnt = sh.qc(h)
        assert cnt == len(sigs) and (0, agg) == orc.aggregate_sigs(sigs, voters)
        rank = sorted(pks)
        assert bitmap == bytes([sum(0x80 >> rank.index(v) for v in voters)])
    assert [sh.qc(h)[2] for h in distinct] == [3, 2, 2]
    # every vote is a cache hit for overlord's serial checks
    for d, m in msgs:
        try:
            oc.verify_signature(m.signature, d, m.voter)
        except Exception:
            pass
    assert oc.hits == len(msgs) and oc.misses == 0
    # a second flush on one hash: Round.add, one more pass
    d, m = _vote(sks, pks, 4, 21, 4, vote.PREVOTE, bh)
    sh.proc_network_msg("SignedVote", ig.encode_signed_vote(m))
    sh.flush()
    assert oc.calls[-1] == ("add", d, 1) and sh.stats["round_passes"] == 2 and sh.stats["round_adds"] == 4
    assert sh.qc(d)[2] == 4


def test_a_flush_on_one_hash_still_uses_round_add():
    sks, pks = _keys(b"rounds add one", 3)
    oc = OracleRoundsCrypto(pks)
    sh = _shim(oc)
    bh = sm3(b"block 22")
    msgs = [_vote(sks, pks, i, 22, 0, vote.PREVOTE, bh) for i in range(3)]
    for _, m in msgs:
        sh.proc_network_msg("SignedVote", ig.encode_signed_vote(m))
    sh.flush()
    assert oc.calls == [("open", msgs[0][0]), ("add", msgs[0][0], 3)]
    assert sh.stats["round_passes"] == 1 and sh.stats["round_adds"] == 1 and sh.stats["round_votes"] == 3


def test_an_18_hash_flush_never_closes_a_round_before_it_was_added_to():
    sks, pks = _keys(b"rounds add 18", 2)
    oc = OracleRoundsCrypto(pks)
    sh = _shim(oc)
    bh = sm3(b"block 23")
    # three rounds are open from an earlier flush; the 18-hash flush needs two of them again
    old = [_vote(sks, pks, 0, 23, r, vote.PREVOTE, bh) for r in (100, 3, 15)]
    for _, m in old:
        sh.proc_network_msg("SignedVote", ig.encode_signed_vote(m))
    sh.flush()
    assert sh.stats["round_passes"] == 1 and len(sh.rounds) == 3
    oc.calls.clear()
    msgs = [_vote(sks, pks, i, 23, r, vote.PREVOTE, bh) for r in range(18) for i in range(2)]
    for _, m in msgs:
        sh.proc_network_msg("SignedVote", ig.encode_signed_vote(m))
    sh.flush()
    calls = [c for c in oc.calls if c[0] == "add_rounds"]
    assert [len(set(c[1])) for c in calls] == [16, 2] and sh.stats["round_passes"] == 3
    assert sh.stats["round_adds"] == 3 + 18 and sh.stats["round_votes"] == 3 + 36
    # OracleRoundsCrypto.add_rounds refuses a closed round; beyond that: every round of the flush
    # was added to before anything closed it, and the rounds needed again were not reopened
    added = set()
    for c in oc.calls:
        if c[0] == "add_rounds":
            added |= set(c[1])
        elif c[0] == "close":
            assert c[1] in added or c[1] == old[0][0], "closed before it was added to"
    flush_hashes = list(dict.fromkeys(d for d, _ in msgs))
    assert [c[1] for c in oc.calls if c[0] == "open"] == [h for h in flush_hashes if h not in (old[1][0], old[2][0])]
    for r in oc.opened:
        if r.hash in flush_hashes:
            assert sum(len(a) for a in r.adds) == (3 if r.hash in (old[1][0], old[2][0]) else 2)
    assert len(sh.rounds) == ig.ROUNDS_MAX and all(not r.closed for r in sh.rounds.values())
    assert sh.qc(flush_hashes[-1])[2] == 2
    # the second call made room by closing the two rounds opened first, after the first call had
    # added to them (voter 0 again: a duplicate, so two signers each)
    assert [r.hash for r in oc.opened if r.closed] == [d for d, _ in old]
    assert [r.model.n_signed for r in oc.opened[:3]] == [1, 2, 2]


def test_a_crypto_without_add_rounds_sees_todays_calls():
    sks, pks = _keys(b"rounds add none", 3)
    bh = sm3(b"block 24")
    msgs = [_vote(sks, pks, i, 24, 0, k, bh) for i in range(3) for k in (vote.PREVOTE, vote.PRECOMMIT)]
    oc = OracleRoundCrypto(pks)
    assert not hasattr(oc, "add_rounds")
    sh = _shim(oc)
    for _, m in msgs:
        sh.proc_network_msg("SignedVote", ig.encode_signed_vote(m))
    sh.flush()
    hp, hc = msgs[0][0], msgs[1][0]
    assert oc.calls == [("open", hp), ("add", hp, 3), ("open", hc), ("add", hc, 3)]
    assert sh.stats["round_adds"] == 2 and sh.stats["round_votes"] == 6 and sh.stats["round_passes"] == 2
