"""The ingress shim's opt-in device rounds (consensus_overlord_amd/ingress.py, rounds=True) over a
fake Crypto whose Round is backed by the C oracle and the round model (tests/round_model.py), in
the style of OracleCrypto in tests/test_ingress.py: a flush hands the fixed-size SignedVotes of each
signed hash, in arrival order, to that hash's Round.add in place of prefetch; chokes still reach
prefetch; the verdict cache is filled the same way; VoteIngress.qc(hash) is the round's QC; the
17th hash closes the round opened first; and with rounds=False the calls are exactly the old ones."""
import pytest

import round_model
from consensus_overlord_amd import ingress as ig
from consensus_overlord_amd import vote
from test_ingress import OracleCrypto, _stream, sm3


class OracleRound:
    def __init__(self, crypto, hash_):
        self.crypto, self.hash = crypto, bytes(hash_)
        self.model = round_model.RoundModel(crypto.pubkeys)
        self.taken_votes = []
        self.adds = []
        self.closed = False

    def add(self, signatures, voters, want_qc=False):
        import orc
        assert not self.closed and not want_qc
        sigs, voters = [bytes(s) for s in signatures], [bytes(v) for v in voters]
        self.adds.append(list(zip(sigs, voters)))
        self.crypto.calls.append(("add", self.hash, len(sigs)))
        codes = [orc.verify(s, self.hash, v) for s, v in zip(sigs, voters)]
        for s, v, c in zip(sigs, voters, codes):
            self.crypto.cache[(s, self.hash, v)] = c
        taken, _, cnt = self.model.add(codes, voters)
        self.taken_votes += [(s, v) for s, v, t in zip(sigs, voters, taken) if t]
        return codes, taken, cnt

    def qc(self):
        import orc
        assert not self.closed
        code, agg = orc.aggregate_sigs([s for s, _ in self.taken_votes], [v for _, v in self.taken_votes])
        assert code == 0
        return agg, bytes(self.model.bitmap), self.model.n_signed

    def close(self):
        self.closed = True
        self.crypto.calls.append(("close", self.hash))


class OracleRoundCrypto(OracleCrypto):
    def __init__(self, pubkeys):
        super().__init__(pubkeys)
        self.calls = []
        self.opened = []

    def prefetch(self, sigs, hashes, voters):
        self.calls.append(("prefetch", [bytes(h) for h in hashes]))
        super().prefetch(sigs, hashes, voters)

    def open_round(self, hash_):
        r = OracleRound(self, hash_)
        self.opened.append(r)
        self.calls.append(("open", r.hash))
        return r


def _keys(tag, n):
    import orc
    sks = [(int.from_bytes(sm3(b"%s %d" % (tag, i)), "big") >> 3).to_bytes(32, "big") for i in range(n)]
    return sks, [orc.sk_to_pk(k)[1] for k in sks]


def _payload(kind, m):
    return ig.encode_signed_vote(m) if kind == "SignedVote" else ig.encode_signed_choke(m)


def test_votes_reach_their_rounds_grouped_by_hash_in_arrival_order():
    import orc
    nval = 5
    sks, pks = _keys(b"rounds", nval)
    bh = sm3(b"block 9")
    msgs = _stream(nval, 9, 0, bh, lambda i, d: orc.sign(sks[i], d)[1], pks, chokes=2)
    pre, com, chokes = msgs[:nval], msgs[nval:2 * nval], msgs[2 * nval:]
    # arrival: the two vote kinds interleaved, a choke in the middle, a vote with a short signature,
    # a duplicate of a prevote, a second choke
    odd = ("SignedVote", ig.SignedVote(b"\x01" * 95, 9, 0, vote.PREVOTE, bh, pks[0]))
    arrival = [pre[0], com[0], pre[1], chokes[0], com[1], pre[2], odd, pre[1], com[2], chokes[1]]
    oc = OracleRoundCrypto(pks)
    fwd = []
    now = [0.0]
    sh = ig.VoteIngress(oc, lambda k, m: fwd.append((k, m)), batch_size=100, max_delay_s=0.01, clock=lambda: now[0],
                        rounds=True)
    for k, m in arrival:
        sh.proc_network_msg(k, _payload(k, m))
    assert fwd == [] and oc.calls == []
    now[0] = 0.02
    sh.poll()
    hp, hc = sm3(vote.rlp_vote(9, 0, vote.PREVOTE, bh)), sm3(vote.rlp_vote(9, 0, vote.PRECOMMIT, bh))
    hk = sm3(chokes[0][1].hash_rlp())
    # rounds in order of first appearance, one add each, the chokes in one prefetch behind them
    assert oc.calls == [("open", hp), ("add", hp, 4), ("open", hc), ("add", hc, 3), ("prefetch", [hk, hk])]
    rp, rc = oc.opened
    assert rp.adds == [[(m.signature, m.voter) for _, m in (pre[0], pre[1], pre[2], pre[1])]]
    assert rc.adds == [[(m.signature, m.voter) for _, m in (com[0], com[1], com[2])]]
    assert [m for _, m in fwd] == [m for _, m in arrival]               # forwarded in arrival order
    assert sh.stats["round_adds"] == 2 and sh.stats["round_votes"] == 7 and sh.stats["unbatched"] == 1
    assert sh.stats["batches"] == 1 and sh.stats["prefetched"] == 2
    # overlord's serial checks: every fixed-size message is a cache hit, the odd one a miss
    for k, m in fwd:
        if m == odd[1]:
            continue
        ig.overlord_verify(oc, k, m)
    assert oc.hits == len(arrival) - 1 and oc.misses == 0
    # the QC of what was flushed: the duplicate prevote is not counted twice
    agg, bitmap, cnt = sh.qc(hp)
    assert cnt == 3 and (0, agg) == orc.aggregate_sigs([m.signature for _, m in pre[:3]], [m.voter for _, m in pre[:3]])
    assert bin(int.from_bytes(bitmap, "big")).count("1") == 3
    # a second flush adds to the same rounds: no second open, and the cross-add duplicate loses
    for k, m in (pre[3], pre[0], com[3]):
        sh.proc_network_msg(k, _payload(k, m))
    sh.flush()
    assert oc.calls[5:] == [("add", hp, 2), ("add", hc, 1)]
    assert sh.qc(hp)[2] == 4 and sh.qc(hc)[2] == 4
    with pytest.raises(KeyError):
        sh.qc(bytes(32))
    sh.close_rounds()
    assert rp.closed and rc.closed and not sh.rounds


def test_the_17th_hash_closes_the_round_opened_first():
    import orc
    sks, pks = _keys(b"rounds17", 2)
    oc = OracleRoundCrypto(pks)
    sh = ig.VoteIngress(oc, lambda k, m: None, batch_size=1, rounds=True)
    hashes = []
    for r in range(ig.ROUNDS_MAX + 1):
        bh = sm3(b"block 17")
        d = sm3(vote.rlp_vote(17, r, vote.PREVOTE, bh))
        hashes.append(d)
        m = ig.SignedVote(orc.sign(sks[0], d)[1], 17, r, vote.PREVOTE, bh, pks[0])
        sh.proc_network_msg("SignedVote", ig.encode_signed_vote(m))
        if r == ig.ROUNDS_MAX - 1:
            assert len(sh.rounds) == ig.ROUNDS_MAX and not any(x.closed for x in oc.opened)
    assert len(oc.opened) == ig.ROUNDS_MAX + 1 and len(sh.rounds) == ig.ROUNDS_MAX
    assert [x.closed for x in oc.opened] == [True] + [False] * ig.ROUNDS_MAX
    assert oc.calls[-3:] == [("close", hashes[0]), ("open", hashes[-1]), ("add", hashes[-1], 1)]
    assert hashes[0] not in sh.rounds and list(sh.rounds) == hashes[1:]


def test_rounds_false_makes_exactly_the_old_calls():
    import orc
    nval = 4
    sks, pks = _keys(b"rounds off", nval)
    msgs = _stream(nval, 11, 1, sm3(b"block 11"), lambda i, d: orc.sign(sks[i], d)[1], pks, chokes=1)

    def run(crypto, **kw):
        fwd = []
        sh = ig.VoteIngress(crypto, lambda k, m: fwd.append((k, m)), max_delay_s=1e9, clock=lambda: 0.0, **kw)
        for k, m in msgs:
            sh.proc_network_msg(k, _payload(k, m))
        sh.flush()
        return sh, fwd

    old = OracleCrypto(pks)                       # no open_round at all
    sh0, fwd0 = run(old)
    off = OracleRoundCrypto(pks)                  # has open_round, not asked for
    sh1, fwd1 = run(off)
    sh2, fwd2 = run(off.__class__(pks), rounds=False)
    assert fwd0 == fwd1 == fwd2
    assert off.opened == [] and all(c[0] == "prefetch" for c in off.calls)
    assert off.prefetch_calls == old.prefetch_calls == [nval, nval, 1]
    assert sh0.stats == sh1.stats == sh2.stats and "round_adds" not in sh1.stats and not sh1.rounds
    # a crypto without open_round: rounds=True falls back to today's calls
    plain = OracleCrypto(pks)
    sh3, fwd3 = run(plain, rounds=True)
    assert fwd3 == fwd0 and plain.prefetch_calls == old.prefetch_calls and not sh3.use_rounds
