"""VoteIngress.update_pubkeys (consensus_overlord_amd/ingress.py) over a fake Crypto, in the style of
tests/test_ingress_rounds.py: with rounds=True and a crypto whose update_pubkeys takes keep_rounds
the shim updates with keep_rounds=True and forgets exactly the rounds whose ids came back closed --
the next flush on a surviving hash reuses its Round, one on a forgotten hash opens a new one; with a
crypto that has no keep_rounds, or with rounds=False, every round is closed first and the update is
the plain one."""
import itertools

from consensus_overlord_amd import ingress as ig
from consensus_overlord_amd import vote
from test_ingress import _stream, sm3
from test_ingress_rounds import OracleRound, OracleRoundCrypto, _keys, _payload


class IdRound(OracleRound):
    ids = itertools.count(1)

    def __init__(self, crypto, hash_):
        super().__init__(crypto, hash_)
        self.id = next(IdRound.ids)


class KeepCrypto(OracleRoundCrypto):
    """update_pubkeys(keys, keep_rounds): closes the rounds named in `drop` (by hash), as the device
    closes those that took a vote of a dropped validator"""

    def __init__(self, pubkeys):
        super().__init__(pubkeys)
        self.drop = []

    def open_round(self, hash_):
        r = IdRound(self, hash_)
        self.opened.append(r)
        self.calls.append(("open", r.hash))
        return r

    def update_pubkeys(self, keys, keep_rounds=False):
        self.calls.append(("update", len(keys), keep_rounds))
        self.pubkeys = list(keys)
        if not keep_rounds:
            return None
        return [r.id for r in self.opened if r.hash in self.drop and not r.closed]


class PlainCrypto(OracleRoundCrypto):
    def update_pubkeys(self, keys):
        self.calls.append(("update", len(keys)))
        self.pubkeys = list(keys)


def _shim(oc, rounds=True):
    fwd = []
    sh = ig.VoteIngress(oc, lambda k, m: fwd.append((k, m)), batch_size=100, max_delay_s=0.01, clock=lambda: 0.0,
                        rounds=rounds)
    return sh, fwd


def _feed(sh, msgs):
    for k, m in msgs:
        sh.proc_network_msg(k, _payload(k, m))
    sh.flush()


def _setup(cls):
    import orc
    nval = 5
    sks, pks = _keys(b"update", nval)
    bh = sm3(b"block 4")
    msgs = _stream(nval, 4, 0, bh, lambda i, d: orc.sign(sks[i], d)[1], pks)
    hp, hc = sm3(vote.rlp_vote(4, 0, vote.PREVOTE, bh)), sm3(vote.rlp_vote(4, 0, vote.PRECOMMIT, bh))
    return cls(pks), pks, msgs[:nval], msgs[nval:], hp, hc


def test_only_the_returned_ids_are_forgotten_and_a_surviving_round_is_reused():
    oc, pks, pre, com, hp, hc = _setup(KeepCrypto)
    sh, _ = _shim(oc)
    _feed(sh, pre[:2] + com[:2])
    rp, rc = oc.opened
    assert set(sh.rounds) == {hp, hc}
    # the every-block call: nothing comes back, nothing is forgotten, no round is closed
    oc.calls.clear()
    sh.update_pubkeys(pks)
    assert oc.calls == [("update", 5, True)] and set(sh.rounds) == {hp, hc}
    # a changed list whose update closes the precommit round
    oc.drop = [hc]
    oc.calls.clear()
    sh.update_pubkeys(pks[:4])
    assert oc.calls == [("update", 4, True), ("close", hc)] and set(sh.rounds) == {hp}
    assert sh.rounds[hp] is rp and not rp.closed and rc.closed
    # the next flush: the surviving hash reuses its Round, the forgotten hash opens a new one
    oc.calls.clear()
    _feed(sh, pre[2:4] + com[2:4])
    assert ("open", hp) not in oc.calls and ("open", hc) in oc.calls
    assert len(rp.adds) == 2 and len(rc.adds) == 1
    assert sh.rounds[hp] is rp and sh.rounds[hc] is oc.opened[2] and oc.opened[2] is not rc
    assert len(oc.opened[2].adds) == 1


def test_without_keep_rounds_support_every_round_is_closed_first():
    oc, pks, pre, com, hp, hc = _setup(PlainCrypto)
    sh, _ = _shim(oc)
    _feed(sh, pre[:2] + com[:2])
    assert len(sh.rounds) == 2
    oc.calls.clear()
    sh.update_pubkeys(pks[:4])
    assert sorted(oc.calls[:2]) == sorted([("close", hp), ("close", hc)]) and oc.calls[2:] == [("update", 4)]
    assert not sh.rounds and all(r.closed for r in oc.opened)


def test_rounds_off_is_the_plain_update():
    oc, pks, pre, com, hp, hc = _setup(KeepCrypto)
    sh, _ = _shim(oc, rounds=False)
    _feed(sh, pre[:2])
    oc.calls.clear()
    sh.update_pubkeys(pks[:4])
    assert oc.calls == [("update", 4, False)] and oc.opened == []
