"""Host-side mirror of the reference's `ConsensusCrypto` (src/consensus.rs:334-463) over the
libovhip C ABI: same method names, argument meaning and error behaviour. Every method runs
its arithmetic in HIP kernels on the context's MI355X (hash/SM3 runs on the host, as in the
reference, util.rs:83-87).

Errors mirror `ConsensusError` (src/error.rs:20-44): `Other(String)` for the hash-length,
length-mismatch and "lose public key" cases, `CryptoErr(code)` for blst errors.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import numpy as np

from . import _lib

OK = 0
ERR_HASH_LEN = 100
ERR_LEN_MISMATCH = 101
ERR_PUBKEY = 102
ERR_ARG = 103
ERR_DEVICE = 200
ERR_RNG = 201

# include/ovhip.h context flags
FLAG_AGG_NO_GROUPCHECK = 0x1
FLAG_PROFILE = 0x2
FLAG_VM_TRACE = 0x4
FLAG_TEST_RLC = 0x8     # tests only: predictable batch coefficients (Context.set_test_rlc)
FLAG_SK_RAW = 0x10      # private key = raw scalar 0 < sk < r instead of IETF KeyGen
FLAG_VM_CLOCK = 0x20    # diagnostics: clock stamps around every vote workgroup (pool log)
FLAG_POOL_RESERVE = 0x40  # the vote pool leaves 8 CUs to the caller's collective (shard contexts)

BLST_ERRORS = {
    1: "BLST_BAD_ENCODING",
    2: "BLST_POINT_NOT_ON_CURVE",
    3: "BLST_POINT_NOT_IN_GROUP",
    4: "BLST_AGGR_TYPE_MISMATCH",
    5: "BLST_VERIFY_FAIL",
    6: "BLST_PK_IS_INFINITY",
    7: "BLST_BAD_SCALAR",
}


class ConsensusError(Exception):
    """src/error.rs:20 ConsensusError."""


class Other(ConsensusError):
    """ConsensusError::Other(String)."""


class CryptoErr(ConsensusError):
    """ConsensusError::CryptoErr(Box<ophelia::Error>)."""

    def __init__(self, code: int):
        super().__init__("Crypto error %s" % BLST_ERRORS.get(code, code))
        self.code = code


class DeviceError(ConsensusError):
    pass


def raise_for(code: int) -> None:
    if code == OK:
        return
    if code == ERR_HASH_LEN:
        raise Other("failed to convert hash value")
    if code == ERR_LEN_MISMATCH:
        raise Other("signatures length does not match voters length")
    if code == ERR_PUBKEY:
        raise Other("lose public key")
    if 1 <= code <= 7:
        raise CryptoErr(code)
    if code == ERR_ARG:
        raise ValueError("invalid argument")
    raise DeviceError("libovhip device error (code %d)" % code)


def _concat(items: Sequence[bytes]):
    items = [bytes(x) for x in items]
    lens = (ctypes.c_size_t * max(1, len(items)))(*[len(x) for x in items])
    return b"".join(items), lens


class Context:
    """One libovhip context (device memory, streams, DST) on HIP device `device`, or over
    several devices of this process (`devices=[...]`, ovh_create_multi). `dst`: None for the
    default DST, else 0-255 bytes (b"" is the empty DST); a longer one raises ValueError."""

    def __init__(self, device: int = 0, dst: Optional[bytes] = None, flags: int = 0,
                 devices: Optional[Sequence[int]] = None):
        self.lib = _lib.load()
        d = None if dst is None else bytes(dst)
        if d is not None and len(d) > 255:
            raise ValueError("the DST is 0-255 bytes (RFC 9380 5.3.1), got %d" % len(d))
        if devices:
            arr = (ctypes.c_int * len(devices))(*devices)
            self.ptr = self.lib.ovh_create_multi(arr, len(devices), d, 0 if d is None else len(d), flags)
            device = devices[0]
        else:
            self.ptr = self.lib.ovh_create(device, d, 0 if d is None else len(d), flags)
        if not self.ptr:
            raise DeviceError("ovh_create failed on device %d (no usable MI355X?)" % device)
        self.device = device
        self.flags = flags

    @property
    def device_count(self) -> int:
        return self.lib.ovh_device_count(self.ptr)

    def peer_matrix(self):
        """ovh_multi_peer_matrix: n x n rows, [a][b] True when device a reaches b's memory
        directly (xGMI peer access) or a and b are one device."""
        buf = ctypes.create_string_buffer(64)
        n = self.lib.ovh_multi_peer_matrix(self.ptr, buf, 64)
        raise_for(n if n < 0 else 0)
        return [[bool(buf.raw[a * n + b]) for b in range(n)] for a in range(n)]

    def set_test_rlc(self, seed: int, index_base: int = 0) -> None:
        """Tests only (context made with FLAG_TEST_RLC): reproducible batch coefficients."""
        raise_for(self.lib.ovh_set_test_rlc(self.ptr, seed & 0xFFFFFFFFFFFFFFFF, index_base))

    def close(self):
        if getattr(self, "ptr", None):
            self.lib.ovh_destroy(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self) -> int:
        return self.lib.ovh_stream(self.ptr)


class ConsensusCrypto:
    """Mirror of `ConsensusCrypto` / overlord's `Crypto` trait (consensus.rs:339-463)."""

    def __init__(self, private_key: bytes, device: int = 0, dst: Optional[bytes] = None, ctx: Optional[Context] = None):
        """consensus.rs:347-359 `new`: the private key file's bytes (hex text or raw bytes),
        parsed as ophelia-blst's BlsPrivateKey::try_from (IETF KeyGen by default, see
        ovh_sk_parse); name = the 48-byte compressed public key; common_ref = ''."""
        if isinstance(private_key, str):
            private_key = bytes.fromhex(private_key.strip())
        self.ctx = ctx if ctx is not None else Context(device, dst)
        self.lib = self.ctx.lib
        self.private_key = bytes(private_key)
        self.common_ref = ""
        out = ctypes.create_string_buffer(48)
        raise_for(self.lib.ovh_sk_to_pk(self.ctx.ptr, self.private_key, len(self.private_key), out))
        self.name = out.raw
        self.pubkeys: List[bytes] = []

    @classmethod
    def from_key_file(cls, path: str, **kw) -> "ConsensusCrypto":
        with open(path) as fh:
            return cls(bytes.fromhex(fh.read().strip()), **kw)

    def update_pubkeys(self, new_pubkeys: Sequence[bytes], keep_rounds: bool = False) -> Optional[List[int]]:
        """consensus.rs:361-363 (callers :131-136, :622-629): the validator keys, 48-byte
        compressed, in config order -> the device validator table (ovh_set_validators), which
        closes every open round.
        keep_rounds=True (ovh_update_validators), for the call on every committed block: nothing
        happens when the list is the one the table holds; else only the keys new to the table are
        checked again, and every open round that has taken no vote of a dropped key is carried
        over to the new table (its Round goes on as a fresh round on the new table would after the
        same taken votes). Returns the ids of the rounds the update closed (Round.id)."""
        keys = [bytes(p) for p in new_pubkeys]
        if any(len(k) != 48 for k in keys):
            raise Other("lose public key")
        if not keep_rounds:
            self.pubkeys = keys
            raise_for(self.lib.ovh_set_validators(self.ctx.ptr, b"".join(keys), len(keys)))
            return None
        closed = (ctypes.c_uint64 * self.ROUNDS_MAX)()
        n_closed = ctypes.c_uint32(0)
        raise_for(self.lib.ovh_update_validators(self.ctx.ptr, b"".join(keys), len(keys), closed, ctypes.byref(n_closed)))
        self.pubkeys = keys
        return [int(closed[k]) for k in range(int(n_closed.value))]

    TABLE_NSTATS = 8           # include/ovhip.h OVH_TABLE_NSTATS

    def table_stats(self):
        """(ovh_set_validators calls, keep_rounds updates that found the list unchanged, ... that
        rebuilt the table, keys those sent through the decompression and subgroup check, keys they
        carried over, rounds they carried over, rounds they closed, table entries now) since the
        context was created (ovh_table_stats)."""
        st = (ctypes.c_uint64 * self.TABLE_NSTATS)()
        raise_for(self.lib.ovh_table_stats(self.ctx.ptr, st))
        return tuple(int(x) for x in st)

    def scalar(self) -> bytes:
        """The 32-byte scalar the private key parses to (ovh_sk_parse)."""
        out = ctypes.create_string_buffer(32)
        raise_for(self.lib.ovh_sk_parse(self.ctx.ptr, self.private_key, len(self.private_key), out))
        return out.raw

    # ---- overlord::Crypto ----
    def hash(self, msg: bytes) -> bytes:
        """consensus.rs:386-388 -> util.rs:83-87 (SM3)."""
        msg = bytes(msg)
        out = ctypes.create_string_buffer(32)
        raise_for(self.lib.ovh_sm3(msg, len(msg), out))
        return out.raw

    def sign(self, hash_: bytes) -> bytes:
        """consensus.rs:390-395."""
        hash_ = bytes(hash_)
        out = ctypes.create_string_buffer(96)
        raise_for(self.lib.ovh_sign(self.ctx.ptr, self.private_key, len(self.private_key), hash_, len(hash_), out))
        return out.raw

    def verify_signature(self, signature: bytes, hash_: bytes, voter: bytes) -> None:
        """consensus.rs:397-416."""
        s, h, v = bytes(signature), bytes(hash_), bytes(voter)
        raise_for(self.lib.ovh_verify(self.ctx.ptr, s, len(s), h, len(h), v, len(v)))

    def aggregate_signatures(self, signatures: Sequence[bytes], voters: Sequence[bytes]) -> bytes:
        """consensus.rs:418-444."""
        sd, sl = _concat(signatures)
        vd, vl = _concat(voters)
        out = ctypes.create_string_buffer(96)
        raise_for(self.lib.ovh_aggregate_sigs(self.ctx.ptr, sd, sl, len(signatures), vd, vl, len(voters), out))
        return out.raw

    def verify_aggregated_signature(self, aggregated_signature: bytes, hash_: bytes, voters: Sequence[bytes]) -> None:
        """consensus.rs:446-462."""
        a, h = bytes(aggregated_signature), bytes(hash_)
        vd, vl = _concat(voters)
        raise_for(self.lib.ovh_verify_aggregated(self.ctx.ptr, a, len(a), h, len(h), vd, vl, len(voters)))

    # ---- extensions ----
    def vote_digests(self, votes) -> List[bytes]:
        """hash(rlp(Vote)) of many votes on the device (ovh_vote_digests: overlord Vote RLP +
        SM3, consensus.rs:169-175, util.rs:83-87). votes: (height, round, vote_type,
        block_hash) tuples, block_hash <= 64 bytes (empty for a nil vote)."""
        n = len(votes)
        if n == 0:
            return []
        h = np.array([v[0] for v in votes], dtype=np.uint64)
        r = np.array([v[1] for v in votes], dtype=np.uint64)
        t = np.array([v[2] for v in votes], dtype=np.uint8)
        lens = np.array([len(v[3]) for v in votes], dtype=np.uint8)
        if any(len(v[3]) > 64 for v in votes):
            raise ValueError("block hashes of up to 64 bytes")
        bh = np.zeros((n, 64), dtype=np.uint8)
        for i, v in enumerate(votes):
            bh[i, :len(v[3])] = np.frombuffer(bytes(v[3]), dtype=np.uint8)
        out = np.zeros((n, 32), dtype=np.uint8)
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
        raise_for(self.lib.ovh_vote_digests(self.ctx.ptr, n, ptr(h), ptr(r), ptr(t), ptr(bh), ptr(lens), ptr(out)))
        return [out[i].tobytes() for i in range(n)]

    @staticmethod
    def _packed(items):
        """Byte strings -> (one concatenated uint8 array, uint64 offsets[n + 1])."""
        items = [bytes(x) for x in items]
        off = np.zeros(len(items) + 1, dtype=np.uint64)
        off[1:] = np.cumsum(np.array([len(x) for x in items], dtype=np.uint64))
        data = np.frombuffer(b"".join(items) or b"\0", dtype=np.uint8)
        return data, off

    def hash_batch(self, msgs: Sequence[bytes]) -> List[bytes]:
        """Crypto::hash of many messages on the device (ovh_sm3_batch: one lane per message),
        element i == hash(msgs[i])."""
        n = len(msgs)
        if n == 0:
            return []
        data, off = self._packed(msgs)
        out = np.zeros((n, 32), dtype=np.uint8)
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
        raise_for(self.lib.ovh_sm3_batch(self.ctx.ptr, n, ptr(data), ptr(off), ptr(out)))
        return [out[i].tobytes() for i in range(n)]

    def aggregate_public_keys(self, voters: Sequence[bytes]) -> bytes:
        """BlsPublicKey::aggregate (consensus.rs:371) -> 48-byte compressed."""
        vd, vl = _concat(voters)
        out = ctypes.create_string_buffer(48)
        raise_for(self.lib.ovh_aggregate_pks(self.ctx.ptr, vd, vl, len(voters), out))
        return out.raw

    @staticmethod
    def _fixed(signatures, hashes, voters):
        n = len(signatures)
        if not (len(hashes) == len(voters) == n):
            raise ValueError("batch lists must have equal length")
        sig = b"".join(bytes(s) for s in signatures)
        hs = b"".join(bytes(h) for h in hashes)
        pk = b"".join(bytes(v) for v in voters)
        if len(sig) != 96 * n or len(hs) != 32 * n or len(pk) != 48 * n:
            raise ValueError("batches take 96-byte signatures, 32-byte hashes, 48-byte voters")
        return n, sig, hs, pk

    def verify_batch(self, signatures, hashes, voters) -> np.ndarray:
        """Batched verify_signature: returns int32 codes[n], codes[i] == the ovh_verify result
        for vote i (0 = Ok). Fixed-size inputs: 96-byte sigs, 32-byte hashes, 48-byte pks."""
        n, sig, hs, pk = self._fixed(signatures, hashes, voters)
        codes = np.zeros(max(n, 1), dtype=np.int32)
        raise_for(self.lib.ovh_verify_batch(self.ctx.ptr, n, sig, hs, pk, codes.ctypes.data_as(ctypes.c_void_p)))
        return codes[:n]

    def verify_batch_async(self, signatures, hashes, voters, codes: np.ndarray) -> None:
        """Pipelined verify_batch (ovh_verify_batch_async, any context kind): returns at once;
        `codes` (int32[n], kept alive by this object until wait) is final after wait()."""
        n, sig, hs, pk = self._fixed(signatures, hashes, voters)
        if codes.dtype != np.int32 or codes.shape != (n,) or not codes.flags.c_contiguous:
            raise ValueError("codes must be a contiguous int32[n] array")
        self._inflight = getattr(self, "_inflight", [])
        self._inflight.append(codes)
        raise_for(self.lib.ovh_verify_batch_async(self.ctx.ptr, n, sig, hs, pk, codes.ctypes.data_as(ctypes.c_void_p)))

    def wait(self) -> None:
        """ovh_batch_wait: every batch in flight is complete, its codes written."""
        raise_for(self.lib.ovh_batch_wait(self.ctx.ptr))
        self._inflight = []

    def prefetch(self, signatures, hashes, voters) -> None:
        """Vote-batching ingress (ovh_prefetch): batch-verify the votes now; later
        verify_signature calls on the same bytes are answered from the context's cache."""
        n, sig, hs, pk = self._fixed(signatures, hashes, voters)
        raise_for(self.lib.ovh_prefetch(self.ctx.ptr, n, sig, hs, pk))

    PRIME_MAX = 64   # include/ovhip.h OVH_PRIME_MAX

    def prime(self, hashes) -> None:
        """Prime H(m) of 32-byte hashes this node is about to sign or verify (ovh_prime_hashes):
        hash_to_G2 of every hash not yet in the message cache is enqueued on a side stream and
        the call returns without waiting for the device. The first verify_signature on a primed
        hash, sign on it and a small verify_batch / prefetch whose hashes are all primed then
        skip hash_to_G2. Call it at proposal receipt (prevote and precommit hashes of the
        block), at round start (the nil votes and the choke) and on the first vote of a group."""
        hs = [bytes(h) for h in hashes]
        if any(len(h) != 32 for h in hs):
            raise ValueError("32-byte hashes")
        for k in range(0, len(hs), self.PRIME_MAX):
            chunk = hs[k:k + self.PRIME_MAX]
            raise_for(self.lib.ovh_prime_hashes(self.ctx.ptr, len(chunk), b"".join(chunk)))

    def prime_votes(self, votes) -> None:
        """prime() of hash(rlp(Vote)) for (height, round, vote_type, block_hash) tuples: the host
        SM3 of about 50 bytes each (no device round trip before the prime)."""
        from . import vote as _vote
        self.prime([self.hash(_vote.rlp_vote(h, r, t, bytes(bh))) for h, r, t, bh in votes])

    def prime_stats(self):
        """(hashes enqueued, hashes skipped as cached or repeated, signs served from the cache,
        small-batch parts run on cached H) since the context was created (ovh_prime_stats)."""
        st = (ctypes.c_uint64 * 4)()
        raise_for(self.lib.ovh_prime_stats(self.ctx.ptr, st))
        return tuple(int(x) for x in st)

    SIG_CACHE_DEFAULT = 4096   # include/ovhip.h OVH_SIG_CACHE_DEFAULT

    def sig_cache_config(self, capacity: int) -> None:
        """Capacity of the signature-point cache (ovh_sig_cache_config): the decompressed points
        of signatures this context signed or verified with code 0, which aggregate_signatures
        sums without decompressing them again. 0 disables and empties it; a new capacity empties
        it; at most 65,536 entries."""
        raise_for(self.lib.ovh_sig_cache_config(self.ctx.ptr, int(capacity)))

    def agg_stats(self):
        """(sigma entries registered, entries now, aggregate_signatures calls on the cache route,
        ... on the full path, signatures of those not found in the cache,
        verify_aggregated_signature calls on the table route, of those on a message-cache H,
        ... on the full path) since the context was created (ovh_agg_stats)."""
        st = (ctypes.c_uint64 * 8)()
        raise_for(self.lib.ovh_agg_stats(self.ctx.ptr, st))
        return tuple(int(x) for x in st)

    def cache_stats(self):
        """(hits, misses, entries) of the verdict cache."""
        st = (ctypes.c_uint64 * 3)()
        raise_for(self.lib.ovh_cache_stats(self.ctx.ptr, st))
        return tuple(int(x) for x in st)

    def samemsg_stats(self):
        """(batches, votes, distinct hashes) checked by the same-message path (ovh_samemsg_stats)."""
        st = (ctypes.c_uint64 * 3)()
        raise_for(self.lib.ovh_samemsg_stats(self.ctx.ptr, st))
        return tuple(int(x) for x in st)

    def verify_qc_batch(self, signatures, hashes, bitmaps) -> np.ndarray:
        """Batched QC check (ovh_verify_qc_batch): QC j signed by the validators (update_pubkeys)
        selected by bitmaps[j] over the key-sorted validator list; codes[j] equals
        verify_aggregated_signature(signatures[j], hashes[j], those voters)."""
        n = len(signatures)
        if not (len(hashes) == len(bitmaps) == n):
            raise ValueError("QC lists must have equal length")
        bl = len(bitmaps[0]) if n else 0
        if any(len(b) != bl for b in bitmaps):
            raise ValueError("bitmaps must have equal length")
        sig = b"".join(bytes(s) for s in signatures)
        hs = b"".join(bytes(h) for h in hashes)
        if len(sig) != 96 * n or len(hs) != 32 * n:
            raise ValueError("QC batches take 96-byte signatures and 32-byte hashes")
        codes = np.zeros(max(n, 1), dtype=np.int32)
        raise_for(self.lib.ovh_verify_qc_batch(self.ctx.ptr, n, sig, hs, b"".join(bytes(b) for b in bitmaps), bl,
                                               codes.ctypes.data_as(ctypes.c_void_p)))
        return codes[:n]

    def build_qc_raw(self, signatures, hash_, voters):
        """ovh_build_qc without raising on "no vote taken": (code, aggregated_signature or None,
        bitmap, codes int32[n], taken bool[n], n_signed). code is 0 or 4; anything else raises."""
        n = len(signatures)
        if len(voters) != n:
            raise Other("signatures length does not match voters length")
        sig = b"".join(bytes(s) for s in signatures)
        pk = b"".join(bytes(v) for v in voters)
        if len(sig) != 96 * n or len(pk) != 48 * n:
            raise ValueError("build_qc takes 96-byte signatures and 48-byte voters")
        h = bytes(hash_)
        codes = np.zeros(max(n, 1), dtype=np.int32)
        taken = np.zeros(max(n, 1), dtype=np.uint8)
        bl = (len(self.pubkeys) + 7) // 8
        bitmap = ctypes.create_string_buffer(max(bl, 1))
        out = ctypes.create_string_buffer(96)
        cnt = ctypes.c_uint32(0)
        code = self.lib.ovh_build_qc(self.ctx.ptr, n, sig, h, len(h), pk, codes.ctypes.data_as(ctypes.c_void_p),
                                     taken.ctypes.data_as(ctypes.c_void_p), out, bitmap, bl, ctypes.byref(cnt))
        if code not in (OK, 4):
            raise_for(code)
        return code, (out.raw if code == OK else None), bitmap.raw[:bl], codes[:n], taken[:n].astype(bool), int(cnt.value)

    def build_qc(self, signatures, hash_, voters):
        """The leader's side of a round in one device pass (ovh_build_qc): verify the round's
        votes on `hash_`, take per validator (update_pubkeys) its first valid vote, aggregate the
        taken signatures. Returns (aggregated_signature, bitmap, codes, taken): the bitmap is MSB
        first over the key-sorted validator list (extract_voters / verify_qc_batch order), codes[i]
        the verify_signature result of vote i (also entered in the verdict cache), taken bool[n].
        Raises CryptoErr(4) when no vote is taken, as aggregate_signatures of an empty list."""
        code, agg, bitmap, codes, taken, _ = self.build_qc_raw(signatures, hash_, voters)
        raise_for(code)
        return agg, bitmap, codes, taken

    QC_GROUPS_MAX = 64   # include/ovhip.h OVH_QC_GROUPS_MAX

    def build_qcs_raw(self, signatures, hashes, voters):
        """ovh_build_qcs' raw arrays: (n_groups, group_hashes uint8[G, 32], out_sigs uint8[G, 96],
        bitmaps uint8[G, bitmap_len], n_signed uint32[G], codes int32[n], taken bool[n],
        group uint32[n]). out_sigs[g] is meaningful only where n_signed[g] > 0."""
        n, sig, hs, pk = self._fixed(signatures, hashes, voters)
        mg = self.QC_GROUPS_MAX
        bl = (len(self.pubkeys) + 7) // 8
        codes = np.zeros(max(n, 1), dtype=np.int32)
        taken = np.zeros(max(n, 1), dtype=np.uint8)
        group = np.zeros(max(n, 1), dtype=np.uint32)
        gh = np.zeros((mg, 32), dtype=np.uint8)
        out = np.zeros((mg, 96), dtype=np.uint8)
        bm = np.zeros((mg, max(bl, 1)), dtype=np.uint8)
        cnt = np.zeros(mg, dtype=np.uint32)
        ng = ctypes.c_uint32(0)
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
        raise_for(self.lib.ovh_build_qcs(self.ctx.ptr, n, sig, hs, pk, ptr(codes), ptr(taken), ptr(group), mg,
                                         ctypes.byref(ng), ptr(gh), ptr(out), ptr(bm), bl, ptr(cnt)))
        g = int(ng.value)
        return g, gh[:g], out[:g], bm[:g, :bl], cnt[:g], codes[:n], taken[:n].astype(bool), group[:n]

    def build_qcs(self, signatures, hashes, voters):
        """The QCs of a mixed-hash vote set in one device pass (ovh_build_qcs): every vote is
        verified under its own hash, and each distinct hash (a group, numbered by first
        appearance) gets its own selection and aggregate. Returns (qcs, codes, taken, group):
        qcs[g] = (hash, aggregated_signature or None when no vote of the group is taken, bitmap,
        n_signed); codes[i] the verify_signature result of vote i (also in the verdict cache),
        taken bool[n], group[i] the index of vote i's QC. A validator with valid votes on two
        hashes is taken in both groups: each QC stands alone."""
        g, gh, out, bm, cnt, codes, taken, group = self.build_qcs_raw(signatures, hashes, voters)
        qcs = [(gh[k].tobytes(), out[k].tobytes() if cnt[k] else None, bm[k].tobytes(), int(cnt[k])) for k in range(g)]
        return qcs, codes, taken, group

    def build_vote_qcs(self, signatures, votes, voters):
        """The leader's inbox as ingress.decode_signed_vote delivers it: votes are (height, round,
        vote_type, block_hash) tuples (an empty block_hash is the nil vote). The signed hashes come
        from the device (vote_digests), then build_qcs. Returns (qcs, codes, taken, group) with
        qcs[g] = (vote tuple, hash, aggregated_signature or None, bitmap, n_signed)."""
        hashes = self.vote_digests(votes)
        qcs, codes, taken, group = self.build_qcs(signatures, hashes, voters)
        first = {}
        for i, g in enumerate(group.tolist()):
            first.setdefault(g, i)
        return [(tuple(votes[first[g]]),) + q for g, q in enumerate(qcs)], codes, taken, group

    ROUNDS_MAX = 16            # include/ovhip.h OVH_ROUNDS_MAX
    ROUND_VOTES_MAX = 1 << 24  # include/ovhip.h OVH_ROUND_VOTES_MAX

    def open_round(self, hash_: bytes) -> "Round":
        """A round on the device (ovh_round_open): build_qc for votes that arrive in several
        flushes. Round.add verifies and adds the new votes only; the QC of everything added so far
        is read without a second pass over the quorum. Needs update_pubkeys, which also closes
        every open round."""
        return Round(self, hash_)

    def add_rounds_raw(self, rounds, signatures, voters, want_qc: bool = False):
        """ovh_rounds_add without raising on its return code. rounds: one open Round per vote (the
        round the vote is for; the vote is verified under that round's hash). Returns (code, codes
        int32[n], taken bool[n], per_round); per_round lists the distinct rounds in order of first
        appearance as (Round, n_signed, aggregated_signature or None, bitmap or None) -- the
        round's cumulative count and, with want_qc only, its cumulative QC (the signature is None
        while nothing is taken). per_round is empty when the call was refused."""
        n = len(signatures)
        if len(voters) != n or len(rounds) != n:
            raise Other("signatures length does not match voters length")
        sig = b"".join(bytes(s) for s in signatures)
        pk = b"".join(bytes(v) for v in voters)
        if len(sig) != 96 * n or len(pk) != 48 * n:
            raise ValueError("add_rounds takes 96-byte signatures and 48-byte voters")
        by_id = {}
        for r in rounds:
            by_id.setdefault(r._id(), r)
        ids = np.array([r._id() for r in rounds] or [0], dtype=np.uint64)
        mr = self.ROUNDS_MAX
        bl = (len(self.pubkeys) + 7) // 8
        codes = np.zeros(max(n, 1), dtype=np.int32)
        taken = np.zeros(max(n, 1), dtype=np.uint8)
        rid = np.zeros(mr, dtype=np.uint64)
        cnt = np.zeros(mr, dtype=np.uint32)
        out = np.zeros((mr, 96), dtype=np.uint8)
        bm = np.zeros((mr, max(bl, 1)), dtype=np.uint8)
        nr = ctypes.c_uint32(0)
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
        code = self.lib.ovh_rounds_add(self.ctx.ptr, n, sig, ptr(ids), pk, ptr(codes), ptr(taken), None, mr,
                                       ctypes.byref(nr), ptr(rid), ptr(cnt), ptr(out) if want_qc else None,
                                       ptr(bm) if want_qc else None, bl if want_qc else 0)
        per_round = []
        if code == OK:
            for k in range(int(nr.value)):
                per_round.append((by_id[int(rid[k])], int(cnt[k]),
                                  out[k].tobytes() if want_qc and cnt[k] else None,
                                  bm[k, :bl].tobytes() if want_qc else None))
        return code, codes[:n], taken[:n].astype(bool), per_round

    def add_rounds(self, rounds, signatures, voters, want_qc: bool = False):
        """A flush's votes added to several open rounds in one device pass (ovh_rounds_add): vote i
        goes to rounds[i]. Every round ends exactly as if Round.add had been called with the
        sub-list of its votes, in the caller's order. Returns (codes, taken, per_round) as
        add_rounds_raw; raises on a refused call, which changes nothing."""
        code, codes, taken, per_round = self.add_rounds_raw(rounds, signatures, voters, want_qc)
        raise_for(code)
        return codes, taken, per_round

    def build_proof(self, height: int, round_: int, block_hash: bytes, signatures, voters) -> bytes:
        """The overlord Proof of a block from the round's precommits: the vote hash
        hash(rlp(Vote{height, round, Precommit, block_hash})), build_qc over it, and the Proof's
        RLP bytes (vote.encode_proof), which check_block accepts."""
        from . import vote as _vote
        vh = _vote.vote_hash(self, height, round_, _vote.PRECOMMIT, block_hash)
        agg, bitmap, _, _ = self.build_qc(signatures, vh, voters)
        return _vote.encode_proof(height, round_, block_hash, agg, bitmap)

    # ---- Consensus::check_block (consensus.rs:143-207) over the Crypto surface ----
    def check_block(self, proposal_height: int, proposal_data: bytes, proof: bytes,
                    authority_list: Optional[Sequence[bytes]] = None) -> bool:
        """consensus.rs:143-207: sm3(proposal data) (:148); decode the overlord Proof (:158,
        layout in vote.py); proof.block_hash == that hash and proof.height == proposal height
        (:165); voters = extract_voters(authority list, bitmap) (:166-167); vote hash =
        hash(rlp(Vote{height, round, Precommit, block_hash})) (:169-175);
        verify_aggregated_signature(...).is_ok() (:176-183). authority_list: the brain's node
        addresses, i.e. the validator keys (util.rs validators_to_nodes); default = the keys
        given to update_pubkeys. Every failure returns False, as the reference does."""
        from . import vote as _vote
        auth = self.pubkeys if authority_list is None else [bytes(a) for a in authority_list]
        block_hash = self.hash(proposal_data)
        try:
            height, round_, bh, sig, bitmap = _vote.decode_proof(proof)
        except ValueError:
            return False
        if bytes(bh) != block_hash or height != proposal_height:
            return False
        voters = _vote.extract_voters(auth, bitmap)
        vh = self.hash(_vote.rlp_vote(height, round_, _vote.PRECOMMIT, bh))
        try:
            self.verify_aggregated_signature(sig, vh, voters)
        except ConsensusError:
            return False
        return True

    def check_block_batch(self, blocks):
        """check_block for many blocks in one device pass (ovh_check_blocks) against the validator
        table (update_pubkeys): blocks = (proposal_height, proposal_data, proof) tuples ->
        (ok bool[n], reasons int32[n]); ok[j] == check_block(*blocks[j]), reasons[j] is 0 or why
        not: 300 the proof does not decode, 301 height or block hash differ, else the
        verify_aggregated_signature code of the QC. The proposal hashes (SM3), the proof decoding
        and the QC batch all run inside the library, behind one host synchronisation;
        check_blocks below is the same composed in Python."""
        n = len(blocks)
        if n == 0:
            return np.zeros(0, dtype=bool), np.zeros(0, dtype=np.int32)
        heights = np.array([b[0] for b in blocks], dtype=np.uint64)
        data, data_off = self._packed([b[1] for b in blocks])
        proofs, proof_off = self._packed([b[2] for b in blocks])
        ok = np.zeros(n, dtype=np.uint8)
        reasons = np.zeros(n, dtype=np.int32)
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
        raise_for(self.lib.ovh_check_blocks(self.ctx.ptr, n, ptr(heights), ptr(data), ptr(data_off), ptr(proofs),
                                            ptr(proof_off), ptr(ok), ptr(reasons)))
        return ok.astype(bool), reasons

    def check_blocks(self, blocks) -> np.ndarray:
        """Many check_block calls against the validator table (update_pubkeys) in one pass:
        blocks = (proposal_height, proposal_data, proof) tuples -> bool[n], element j ==
        check_block(*blocks[j]). Vote hashes come from ovh_vote_digests and the aggregated
        signatures are checked by ovh_verify_qc_batch (bitmaps over the key-sorted table, the
        extract_voters order), one batch per bitmap length."""
        from . import vote as _vote
        n = len(blocks)
        ok = np.zeros(n, dtype=bool)
        live = []
        for j, (ph, data, proof) in enumerate(blocks):
            try:
                height, round_, bh, sig, bitmap = _vote.decode_proof(proof)
            except ValueError:
                continue
            if bytes(bh) != self.hash(data) or height != ph:
                continue
            if len(sig) != 96 or len(bh) > 64:
                # the QC batch takes compressed signatures only; anything else goes the scalar way
                ok[j] = self.check_block(ph, data, proof)
                continue
            live.append((j, height, round_, bytes(bh), bytes(sig), bytes(bitmap)))
        if not live:
            return ok
        if not self.pubkeys:
            # no validator table (update_pubkeys never called, or given []): check_block answers
            # every block itself (empty authority list -> no voters -> False, consensus.rs:167-183)
            for j, *_ in live:
                ok[j] = self.check_block(*blocks[j])
            return ok
        digests = self.vote_digests([(h, r, _vote.PRECOMMIT, bh) for _, h, r, bh, _, _ in live])
        groups = {}
        for (j, _, _, _, sig, bm), d in zip(live, digests):
            groups.setdefault(len(bm), []).append((j, sig, d, bm))
        for items in groups.values():
            codes = self.verify_qc_batch([s for _, s, _, _ in items], [d for _, _, d, _ in items],
                                         [b for _, _, _, b in items])
            for (j, _, _, _), c in zip(items, codes):
                ok[j] = c == 0
        return ok


class Round:
    """One open round of a ConsensusCrypto (ovh_round_open .. ovh_round_close): the votes on one
    hash, added as they arrive. For any cut of a vote list into consecutive adds the codes, the
    taken flags, the count, the bitmap and the aggregated signature equal build_qc's over the
    whole list. Use as a context manager, or close() it; update_pubkeys closes it as well (every
    later call then raises ValueError), and so does update_pubkeys(keep_rounds=True) when it returns
    the round's id; a round that call carries over goes on with the new table's bitmap length."""

    def __init__(self, crypto: ConsensusCrypto, hash_: bytes):
        self.crypto = crypto
        self.lib = crypto.lib
        self.hash = bytes(hash_)
        rid = ctypes.c_uint64(0)
        raise_for(self.lib.ovh_round_open(crypto.ctx.ptr, self.hash, len(self.hash), ctypes.byref(rid)))
        self.id: Optional[int] = int(rid.value)

    @property
    def bitmap_len(self) -> int:
        """ceil(n / 8) of the table the round is on now (a carried round follows the update)"""
        return (len(self.crypto.pubkeys) + 7) // 8

    def _id(self) -> int:
        if self.id is None:
            raise ValueError("the round is closed")
        return self.id

    def add_raw(self, signatures, voters, want_qc: bool = False):
        """ovh_round_add without raising on its return code: (code, codes int32[n], taken bool[n],
        n_signed, aggregated_signature or None, bitmap or None). The signature and the bitmap are
        asked for only with want_qc (the signature is None while nothing is taken)."""
        n = len(signatures)
        if len(voters) != n:
            raise Other("signatures length does not match voters length")
        sig = b"".join(bytes(s) for s in signatures)
        pk = b"".join(bytes(v) for v in voters)
        if len(sig) != 96 * n or len(pk) != 48 * n:
            raise ValueError("Round.add takes 96-byte signatures and 48-byte voters")
        codes = np.zeros(max(n, 1), dtype=np.int32)
        taken = np.zeros(max(n, 1), dtype=np.uint8)
        cnt = ctypes.c_uint32(0)
        bl = self.bitmap_len
        out = ctypes.create_string_buffer(96) if want_qc else None
        bitmap = ctypes.create_string_buffer(max(bl, 1)) if want_qc else None
        code = self.lib.ovh_round_add(self.crypto.ctx.ptr, self._id(), n, sig, pk, codes.ctypes.data_as(ctypes.c_void_p),
                                      taken.ctypes.data_as(ctypes.c_void_p), ctypes.byref(cnt), out, bitmap,
                                      bl if want_qc else 0)
        ok = code == OK
        return (code, codes[:n], taken[:n].astype(bool), int(cnt.value),
                out.raw if ok and want_qc and cnt.value else None, bitmap.raw[:bl] if ok and want_qc else None)

    def add(self, signatures, voters, want_qc: bool = False):
        """Verify the new votes on the round's hash, select, and add the taken signatures to the
        round's sum, in one device pass over these votes only. Returns (codes, taken, n_signed):
        codes[i] the verify_signature result of vote i (also entered in the verdict cache), taken
        bool[n], n_signed the round's cumulative count. With want_qc -- pass it when this add is
        expected to cross the threshold -- (codes, taken, n_signed, aggregated_signature, bitmap)
        of everything added so far, in the same pass; the signature is None while nothing is taken."""
        code, codes, taken, cnt, sig, bitmap = self.add_raw(signatures, voters, want_qc)
        raise_for(code)
        return (codes, taken, cnt, sig, bitmap) if want_qc else (codes, taken, cnt)

    def qc_raw(self):
        """ovh_round_qc: (code, aggregated_signature or None, bitmap, n_signed); code is 0, or 4
        while nothing is taken. Anything else raises."""
        bl = self.bitmap_len
        out = ctypes.create_string_buffer(96)
        bitmap = ctypes.create_string_buffer(max(bl, 1))
        cnt = ctypes.c_uint32(0)
        code = self.lib.ovh_round_qc(self.crypto.ctx.ptr, self._id(), out, bitmap, bl, ctypes.byref(cnt))
        if code not in (OK, 4):
            raise_for(code)
        return code, (out.raw if code == OK else None), bitmap.raw[:bl], int(cnt.value)

    def qc(self):
        """The QC of what has been added so far, with no verification: (aggregated_signature,
        bitmap, n_signed). Raises CryptoErr(4) while nothing is taken, as build_qc does."""
        code, agg, bitmap, cnt = self.qc_raw()
        raise_for(code)
        return agg, bitmap, cnt

    def close(self) -> None:
        """ovh_round_close. Closing twice, or a round that update_pubkeys closed, is no error."""
        rid, self.id = self.id, None
        if rid is not None and getattr(self.crypto.ctx, "ptr", None):
            self.lib.ovh_round_close(self.crypto.ctx.ptr, rid)

    def __enter__(self) -> "Round":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
