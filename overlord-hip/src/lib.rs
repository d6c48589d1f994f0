//! overlord-hip: the MI355X backend of consensus_overlord's `Crypto` trait.
//!
//! `HipCrypto` is a drop-in for `ConsensusCrypto` (reference `src/consensus.rs:334-463`): the same
//! five trait methods with the same error precedence, over libovhip.so (include/ovhip.h). A node
//! selects it by config (`crypto_backend = "hip"` beside `src/config.rs:18-31`); nothing else in
//! the node changes. The arithmetic runs on the GPU (gfx950 HIP kernels); there is no CPU path.
//!
//! Like `ConsensusCrypto` (`#[derive(Clone)]`, consensus.rs:339) it is cheap to clone:
//! `Consensus::new` clones it into `Brain`, into the `Arc` overlord holds and into itself
//! (consensus.rs:61-76). The clones share one device context (`Arc<Ctx>`: the last clone to drop
//! destroys it, never twice) and one key list, as the reference's clones share
//! `Arc<RwLock<Vec<BlsPublicKey>>>`. `update_pubkeys` is `async` and takes the reference callers'
//! `Vec<BlsPublicKey>` (consensus.rs:131-136, :622-629) through ophelia's `PublicKey` trait.
//!
//! Error mapping (reference `src/error.rs:20-44`, `consensus.rs:391-462`): code 100 is
//! `Other("failed to convert hash value")`, 101 `Other("signatures length does not match voters
//! length")`, 102 `Other("lose public key")`, 1..=7 a blst error (`CryptoErr`), anything else a
//! device error. The variants and their Display follow the reference's `ConsensusError`
//! (derive_more `{_0:?}` / `"Crypto error {_0:?}"`); overlord only observes Ok / Err.
//!
//! Not compiled in this repository's image (no Rust toolchain): `tests/test_crate_ffi.py` checks
//! the FFI block against the header and the drop-in shape (Clone, `update_pubkeys`, the ingress
//! module's calls) textually.
pub mod ffi;
pub mod ingress;

use bytes::Bytes;
use overlord::Crypto as OverlordCrypto;
use std::error::Error;
use std::fmt;
use std::sync::atomic::{AtomicI32, Ordering};
use std::sync::Arc;
use tokio::sync::RwLock;

/// The reference's `ConsensusError` variants this backend can return (`src/error.rs:20-44`).
#[derive(Debug)]
pub enum HipCryptoError {
    /// `ConsensusError::Other(String)`: hash length, list length mismatch, key parse.
    Other(String),
    /// `ConsensusError::CryptoErr`: a blst error code (1 BAD_ENCODING ... 7 BAD_SCALAR).
    CryptoErr(i32),
    /// The device or the OS random source failed (codes 103, 200, 201).
    Device(i32),
}

impl fmt::Display for HipCryptoError {
    fn fmt(&self, f: &mut fmt::Formatter<'_>) -> fmt::Result {
        match self {
            HipCryptoError::Other(s) => write!(f, "{s:?}"),
            HipCryptoError::CryptoErr(c) => write!(f, "Crypto error {c:?}"),
            HipCryptoError::Device(c) => write!(f, "hip device error {c}"),
        }
    }
}

impl Error for HipCryptoError {}

/// As the reference's `impl From<ConsensusError> for Box<dyn Error + Send>` (error.rs:41-45).
impl From<HipCryptoError> for Box<dyn Error + Send> {
    fn from(error: HipCryptoError) -> Self {
        Box::new(error) as Box<dyn Error + Send>
    }
}

pub(crate) fn to_err(code: i32) -> Box<dyn Error + Send> {
    match code {
        ffi::OVH_ERR_HASH_LEN => HipCryptoError::Other("failed to convert hash value".into()),
        ffi::OVH_ERR_LEN_MISMATCH => {
            HipCryptoError::Other("signatures length does not match voters length".into())
        }
        ffi::OVH_ERR_PUBKEY => HipCryptoError::Other("lose public key".into()),
        1..=7 => HipCryptoError::CryptoErr(code),
        c => HipCryptoError::Device(c),
    }
    .into()
}

pub(crate) fn check(code: i32) -> Result<(), Box<dyn Error + Send>> {
    if code == ffi::OVH_OK {
        Ok(())
    } else {
        Err(to_err(code))
    }
}

/// `Vec<Bytes>` across the C ABI: one concatenated buffer plus the item lengths.
fn concat(v: &[Bytes]) -> (Vec<u8>, Vec<usize>) {
    (v.iter().flat_map(|b| b.iter().copied()).collect(), v.iter().map(|b| b.len()).collect())
}

/// The device context. Owned through `Arc` by every clone of `HipCrypto` (and by the blocking
/// tasks `update_pubkeys` and the ingress shim start); `ovh_destroy` runs once, when the last
/// owner drops it.
pub(crate) struct Ctx(pub(crate) *mut ffi::OvhCtx);
// libovhip serialises every entry point on the context's own mutex (include/ovhip.h: the trait
// object is Send + Sync and is called by overlord and the check_block handler concurrently).
unsafe impl Send for Ctx {}
unsafe impl Sync for Ctx {}

impl Drop for Ctx {
    fn drop(&mut self) {
        unsafe { ffi::ovh_destroy(self.0) }
    }
}

/// The GPU `Crypto` of a node: its private key (as `ConsensusCrypto::new` reads it), the name
/// (48-byte compressed public key) and the validator keys (`ConsensusCrypto::pubkeys`).
#[derive(Clone)]
pub struct HipCrypto {
    ctx: Arc<Ctx>,
    private_key: Arc<Vec<u8>>,
    pub name: Bytes,
    /// The validator keys as last given to `update_pubkeys` (the device table holds them
    /// decompressed and group-checked); shared by every clone, as the reference's field.
    pub pubkeys: Arc<RwLock<Vec<Bytes>>>,
    /// The code of the last failed device table upload (0: none); `update_pubkeys` returns
    /// nothing, as the reference's does.
    table_error: Arc<AtomicI32>,
}

impl HipCrypto {
    /// `ConsensusCrypto::new` (consensus.rs:347-359): hex key file -> key bytes -> name. `devices`
    /// empty: GPU 0; several: one context over those GPUs (batches shard across them).
    pub fn new(private_key_path: &str, devices: &[i32]) -> Result<Self, Box<dyn Error + Send>> {
        let text = std::fs::read_to_string(private_key_path)
            .map_err(|e| Box::new(HipCryptoError::Other(e.to_string())) as Box<dyn Error + Send>)?;
        let key = hex::decode(text.trim())
            .map_err(|e| Box::new(HipCryptoError::Other(e.to_string())) as Box<dyn Error + Send>)?;
        Self::from_key(key, devices)
    }

    pub fn from_key(private_key: Vec<u8>, devices: &[i32]) -> Result<Self, Box<dyn Error + Send>> {
        let ctx = unsafe {
            match devices.len() {
                0 => ffi::ovh_create(0, std::ptr::null(), 0, 0),
                1 => ffi::ovh_create(devices[0], std::ptr::null(), 0, 0),
                n => ffi::ovh_create_multi(devices.as_ptr(), n as i32, std::ptr::null(), 0, 0),
            }
        };
        if ctx.is_null() {
            return Err(to_err(ffi::OVH_ERR_DEVICE));
        }
        let ctx = Ctx(ctx);
        let mut name = [0u8; 48];
        check(unsafe {
            ffi::ovh_sk_to_pk(ctx.0, private_key.as_ptr(), private_key.len(), name.as_mut_ptr())
        })?;
        Ok(HipCrypto {
            ctx: Arc::new(ctx),
            private_key: Arc::new(private_key),
            name: Bytes::copy_from_slice(&name),
            pubkeys: Arc::new(RwLock::new(Vec::new())),
            table_error: Arc::new(AtomicI32::new(0)),
        })
    }

    pub(crate) fn raw(&self) -> *mut ffi::OvhCtx {
        self.ctx.0
    }

    /// `ConsensusCrypto::update_pubkeys` (consensus.rs:361-363), same shape: `async`, no result,
    /// takes the callers' `Vec<BlsPublicKey>` (consensus.rs:131-136, :622-629) -- any ophelia
    /// `PublicKey`. The keys go to the device table (decompressed and group-checked once, on a
    /// blocking task: never on the reactor). A key the device cannot parse stays in the table as
    /// unparsed, and a vote by it answers "lose public key" exactly as the key path does; a
    /// failed upload leaves the table empty (every vote then takes the key path, still exact)
    /// and is reported by `table_error`.
    pub async fn update_pubkeys<K: ophelia::PublicKey>(&self, new_pubkeys: Vec<K>) {
        let keys: Vec<Bytes> = new_pubkeys.iter().map(|k| k.to_bytes()).collect();
        let ctx = self.ctx.clone();
        let n = keys.len();
        let all48 = keys.iter().all(|k| k.len() == 48);
        let flat: Vec<u8> = keys.iter().flat_map(|k| k.iter().copied()).collect();
        let code = tokio::task::spawn_blocking(move || {
            if all48 {
                unsafe { ffi::ovh_set_validators(ctx.0, flat.as_ptr(), n) }
            } else {
                // not compressed G1 keys: an empty table (the key path serves every vote)
                let c = unsafe { ffi::ovh_set_validators(ctx.0, std::ptr::null(), 0) };
                if c == ffi::OVH_OK {
                    ffi::OVH_ERR_PUBKEY
                } else {
                    c
                }
            }
        })
        .await
        .unwrap_or(ffi::OVH_ERR_DEVICE);
        self.table_error.store(code, Ordering::Relaxed);
        *self.pubkeys.write().await = keys;
    }

    /// `update_pubkeys` for a node that keeps rounds open across commits (`ovh_update_validators`),
    /// for the call on every committed block (consensus.rs:622-629): nothing happens when the list
    /// is the one the table holds; else only the keys new to the table are checked again, and every
    /// open round that has taken no vote of a dropped key is carried over to the new table. Returns
    /// the ids of the rounds the update closed (their later calls return `CryptoErr(OVH_ERR_ARG)`);
    /// keys that are not 48 bytes long empty the table as `update_pubkeys` does, which closes every
    /// round (their `Round`s then answer `OVH_ERR_ARG` as well).
    pub async fn update_pubkeys_keep_rounds<K: ophelia::PublicKey>(&self, new_pubkeys: Vec<K>) -> Vec<u64> {
        let keys: Vec<Bytes> = new_pubkeys.iter().map(|k| k.to_bytes()).collect();
        let ctx = self.ctx.clone();
        let n = keys.len();
        let all48 = keys.iter().all(|k| k.len() == 48);
        let flat: Vec<u8> = keys.iter().flat_map(|k| k.iter().copied()).collect();
        let (code, closed) = tokio::task::spawn_blocking(move || {
            let mut ids = [0u64; ffi::OVH_ROUNDS_MAX];
            let mut cnt = 0u32;
            let c = if all48 {
                unsafe { ffi::ovh_update_validators(ctx.0, flat.as_ptr(), n, ids.as_mut_ptr(), &mut cnt) }
            } else {
                let c = unsafe { ffi::ovh_update_validators(ctx.0, std::ptr::null(), 0, ids.as_mut_ptr(), &mut cnt) };
                if c == ffi::OVH_OK {
                    ffi::OVH_ERR_PUBKEY
                } else {
                    c
                }
            };
            (c, ids[..cnt as usize].to_vec())
        })
        .await
        .unwrap_or((ffi::OVH_ERR_DEVICE, Vec::new()));
        self.table_error.store(code, Ordering::Relaxed);
        *self.pubkeys.write().await = keys;
        closed
    }

    /// `ovh_table_stats`: [`ovh_set_validators` calls, updates that found the list unchanged,
    /// updates that rebuilt the table, keys those checked again, keys they carried over, rounds
    /// they carried over, rounds they closed, table entries now].
    pub fn table_stats(&self) -> Result<[u64; ffi::OVH_TABLE_NSTATS], Box<dyn Error + Send>> {
        let mut st = [0u64; ffi::OVH_TABLE_NSTATS];
        check(unsafe { ffi::ovh_table_stats(self.raw(), st.as_mut_ptr()) })?;
        Ok(st)
    }

    /// The code of the last failed `update_pubkeys` upload (0 when the table is current).
    pub fn table_error(&self) -> i32 {
        self.table_error.load(Ordering::Relaxed)
    }

    /// The vote-batching hook at `proc_network_msg` (consensus.rs:210-262, `ingress::VoteIngress`):
    /// batch-verify held votes; later `verify_signature` calls on them are answered from the
    /// verdict cache. Blocking: call from `spawn_blocking`, never on the reactor.
    pub fn prefetch(&self, sigs: &[[u8; 96]], hashes: &[[u8; 32]], voters: &[[u8; 48]]) -> Result<(), Box<dyn Error + Send>> {
        if sigs.len() != hashes.len() || sigs.len() != voters.len() {
            return Err(to_err(ffi::OVH_ERR_LEN_MISMATCH));
        }
        check(unsafe {
            ffi::ovh_prefetch(self.raw(), sigs.len(), sigs.as_ptr() as *const u8, hashes.as_ptr() as *const u8,
                              voters.as_ptr() as *const u8)
        })
    }

    /// Prime H(m) of hashes this node is about to sign or verify (`ovh_prime_hashes`): enqueues
    /// hash_to_G2 of every hash not yet in the context's message cache on a side stream and
    /// returns without waiting for the device. Call it at proposal receipt (the block's prevote
    /// and precommit hashes), at round start (the nil votes and the choke) and from the ingress
    /// shim on the first vote of a group. Chunks by `OVH_PRIME_MAX`.
    pub fn prime_hashes(&self, hashes: &[[u8; 32]]) -> Result<(), Box<dyn Error + Send>> {
        for chunk in hashes.chunks(ffi::OVH_PRIME_MAX) {
            check(unsafe { ffi::ovh_prime_hashes(self.raw(), chunk.len(), chunk.as_ptr() as *const u8) })?;
        }
        Ok(())
    }

    /// `ovh_prime_stats`: [hashes enqueued, hashes skipped (cached or repeated), signs served
    /// from the cache, small-batch parts run on cached H].
    pub fn prime_stats(&self) -> Result<[u64; 4], Box<dyn Error + Send>> {
        let mut st = [0u64; 4];
        check(unsafe { ffi::ovh_prime_stats(self.raw(), st.as_mut_ptr()) })?;
        Ok(st)
    }

    /// Capacity of the signature-point cache (`ovh_sig_cache_config`): the decompressed points of
    /// signatures this context signed or verified with code 0, which `aggregate_signatures` sums
    /// without decompressing them again. 0 disables and empties it; at most
    /// `OVH_SIG_CACHE_MAX` entries.
    pub fn sig_cache_config(&self, capacity: usize) -> Result<(), Box<dyn Error + Send>> {
        check(unsafe { ffi::ovh_sig_cache_config(self.raw(), capacity) })
    }

    /// `ovh_agg_stats`: [sigma entries registered, entries now, aggregate_signatures calls on the
    /// cache route, on the full path, their signatures not found in the cache,
    /// verify_aggregated_signature calls on the table route, of those on a message-cache H, on
    /// the full path].
    pub fn agg_stats(&self) -> Result<[u64; 8], Box<dyn Error + Send>> {
        let mut st = [0u64; 8];
        check(unsafe { ffi::ovh_agg_stats(self.raw(), st.as_mut_ptr()) })?;
        Ok(st)
    }

    /// hash(rlp(Vote)) of n votes on the device (`ovh_vote_digests`: rlp + SM3 per vote, the
    /// bytes overlord signs, consensus.rs:169-175). `block_hashes` holds one hash per vote of at
    /// most OVH_VOTE_HASH_MAX bytes. Blocking.
    pub fn vote_digests(&self, heights: &[u64], rounds: &[u64], vote_types: &[u8], block_hashes: &[Bytes]) -> Result<Vec<[u8; 32]>, Box<dyn Error + Send>> {
        let n = heights.len();
        if rounds.len() != n || vote_types.len() != n || block_hashes.len() != n {
            return Err(to_err(ffi::OVH_ERR_LEN_MISMATCH));
        }
        let mut hb = vec![0u8; n * ffi::OVH_VOTE_HASH_MAX];
        let mut hl = vec![0u8; n];
        for (i, h) in block_hashes.iter().enumerate() {
            if h.len() > ffi::OVH_VOTE_HASH_MAX {
                return Err(to_err(ffi::OVH_ERR_ARG));
            }
            hb[i * ffi::OVH_VOTE_HASH_MAX..i * ffi::OVH_VOTE_HASH_MAX + h.len()].copy_from_slice(h);
            hl[i] = h.len() as u8;
        }
        let mut out = vec![[0u8; 32]; n];
        check(unsafe {
            ffi::ovh_vote_digests(self.raw(), n, heights.as_ptr(), rounds.as_ptr(), vote_types.as_ptr(), hb.as_ptr(),
                                  hl.as_ptr(), out.as_mut_ptr() as *mut u8)
        })?;
        Ok(out)
    }

    /// n x `verify_signature` in one call: codes[i] is the per-call code of vote i (0 = Ok).
    pub fn verify_batch(&self, sigs: &[[u8; 96]], hashes: &[[u8; 32]], voters: &[[u8; 48]]) -> Result<Vec<i32>, Box<dyn Error + Send>> {
        if sigs.len() != hashes.len() || sigs.len() != voters.len() {
            return Err(to_err(ffi::OVH_ERR_LEN_MISMATCH));
        }
        let mut codes = vec![0i32; sigs.len()];
        check(unsafe {
            ffi::ovh_verify_batch(self.raw(), sigs.len(), sigs.as_ptr() as *const u8, hashes.as_ptr() as *const u8,
                                  voters.as_ptr() as *const u8, codes.as_mut_ptr())
        })?;
        Ok(codes)
    }

    /// The leader's side of a round in one device pass (`ovh_build_qc`): verify the round's votes
    /// on `hash`, take per validator its first valid vote, and aggregate the taken signatures.
    /// Returns the QC's signature, the address bitmap (MSB first over the key-sorted table of
    /// `update_pubkeys`, the `extract_voters` order), the per-vote codes (the per-call
    /// `verify_signature` results, also entered in the verdict cache) and the taken flags; the
    /// caller compares the number of taken votes with its threshold. `CryptoErr(4)` when no vote
    /// is taken, as `aggregate_signatures` of an empty list. Blocking.
    #[allow(clippy::type_complexity)]
    pub fn build_qc(&self, sigs: &[[u8; 96]], hash: &[u8], voters: &[[u8; 48]]) -> Result<(Bytes, Bytes, Vec<i32>, Vec<u8>), Box<dyn Error + Send>> {
        if sigs.len() != voters.len() {
            return Err(to_err(ffi::OVH_ERR_LEN_MISMATCH));
        }
        let table = self.pubkeys.blocking_read().len();
        let mut codes = vec![0i32; sigs.len()];
        let mut taken = vec![0u8; sigs.len()];
        let mut bitmap = vec![0u8; (table + 7) / 8];
        let mut out = [0u8; 96];
        let mut n_signed = 0u32;
        check(unsafe {
            ffi::ovh_build_qc(self.raw(), sigs.len(), sigs.as_ptr() as *const u8, hash.as_ptr(), hash.len(),
                              voters.as_ptr() as *const u8, codes.as_mut_ptr(), taken.as_mut_ptr(), out.as_mut_ptr(),
                              bitmap.as_mut_ptr(), bitmap.len(), &mut n_signed)
        })?;
        Ok((Bytes::copy_from_slice(&out), Bytes::from(bitmap), codes, taken))
    }

    /// The QCs of a mixed-hash vote set in one device pass (`ovh_build_qcs`): the leader's inbox as
    /// it arrives, every vote verified under its own hash, one QC per distinct hash. Returns the
    /// groups in order of first appearance as (hash, signature or `None` when no vote of the
    /// group is taken, bitmap, number of taken votes), then the per-vote codes, taken flags and
    /// group numbers. A validator with valid votes on two hashes is taken in both groups: each QC
    /// stands alone, the equivocation is the caller's to handle. `CryptoErr(OVH_ERR_ARG)` for more
    /// than `OVH_QC_GROUPS_MAX` distinct hashes. Blocking.
    #[allow(clippy::type_complexity)]
    pub fn build_qcs(&self, sigs: &[[u8; 96]], hashes: &[[u8; 32]], voters: &[[u8; 48]]) -> Result<(Vec<([u8; 32], Option<Bytes>, Bytes, u32)>, Vec<i32>, Vec<u8>, Vec<u32>), Box<dyn Error + Send>> {
        if sigs.len() != hashes.len() || sigs.len() != voters.len() {
            return Err(to_err(ffi::OVH_ERR_LEN_MISMATCH));
        }
        let bl = (self.pubkeys.blocking_read().len() + 7) / 8;
        let mg = ffi::OVH_QC_GROUPS_MAX;
        let mut codes = vec![0i32; sigs.len()];
        let mut taken = vec![0u8; sigs.len()];
        let mut group = vec![0u32; sigs.len()];
        let mut n_groups = 0u32;
        let mut group_hashes = vec![[0u8; 32]; mg];
        let mut out_sigs = vec![[0u8; 96]; mg];
        let mut bitmaps = vec![0u8; mg * bl];
        let mut n_signed = vec![0u32; mg];
        check(unsafe {
            ffi::ovh_build_qcs(self.raw(), sigs.len(), sigs.as_ptr() as *const u8, hashes.as_ptr() as *const u8,
                               voters.as_ptr() as *const u8, codes.as_mut_ptr(), taken.as_mut_ptr(), group.as_mut_ptr(),
                               mg, &mut n_groups, group_hashes.as_mut_ptr() as *mut u8, out_sigs.as_mut_ptr() as *mut u8,
                               bitmaps.as_mut_ptr(), bl, n_signed.as_mut_ptr())
        })?;
        let qcs = (0..n_groups as usize)
            .map(|g| {
                let sig = if n_signed[g] > 0 { Some(Bytes::copy_from_slice(&out_sigs[g])) } else { None };
                (group_hashes[g], sig, Bytes::copy_from_slice(&bitmaps[g * bl..(g + 1) * bl]), n_signed[g])
            })
            .collect();
        Ok((qcs, codes, taken, group))
    }

    /// `Crypto::hash` of many messages on the device (`ovh_sm3_batch`: one lane per message),
    /// digest i = SM3(msgs[i]). Blocking.
    pub fn hash_batch(&self, msgs: &[Bytes]) -> Result<Vec<[u8; 32]>, Box<dyn Error + Send>> {
        let mut off = Vec::with_capacity(msgs.len() + 1);
        let mut data = Vec::with_capacity(msgs.iter().map(|m| m.len()).sum());
        off.push(0u64);
        for m in msgs {
            data.extend_from_slice(m);
            off.push(data.len() as u64);
        }
        let mut out = vec![[0u8; 32]; msgs.len()];
        check(unsafe {
            ffi::ovh_sm3_batch(self.raw(), msgs.len(), data.as_ptr(), off.as_ptr(), out.as_mut_ptr() as *mut u8)
        })?;
        Ok(out)
    }

    /// `Consensus::check_block` (consensus.rs:143-207) for many blocks in one device pass
    /// (`ovh_check_blocks`) against the validator table of `update_pubkeys`: blocks are (proposal
    /// height, proposal data, the overlord Proof's RLP bytes). Returns per block whether
    /// check_block accepts it and, when not, why: OVH_CB_PROOF_DECODE, OVH_CB_MISMATCH or the
    /// `verify_aggregated_signature` code of its QC. Blocking: call from `spawn_blocking`.
    pub fn check_blocks(&self, blocks: &[(u64, Bytes, Bytes)]) -> Result<(Vec<bool>, Vec<i32>), Box<dyn Error + Send>> {
        let n = blocks.len();
        let heights: Vec<u64> = blocks.iter().map(|b| b.0).collect();
        let (mut data, mut proofs) = (Vec::new(), Vec::new());
        let (mut data_off, mut proof_off) = (vec![0u64], vec![0u64]);
        for (_, d, p) in blocks {
            data.extend_from_slice(d);
            data_off.push(data.len() as u64);
            proofs.extend_from_slice(p);
            proof_off.push(proofs.len() as u64);
        }
        let mut ok = vec![0u8; n];
        let mut reasons = vec![0i32; n];
        check(unsafe {
            ffi::ovh_check_blocks(self.raw(), n, heights.as_ptr(), data.as_ptr(), data_off.as_ptr(), proofs.as_ptr(),
                                  proof_off.as_ptr(), ok.as_mut_ptr(), reasons.as_mut_ptr())
        })?;
        Ok((ok.into_iter().map(|b| b == 1).collect(), reasons))
    }

    /// A round on the device (`ovh_round_open`): `build_qc` for votes that arrive in several
    /// flushes. `hash` is the 32-byte hash the round's votes sign. The round holds the context
    /// alive and closes itself when dropped; `update_pubkeys` closes every open round (their
    /// later calls return `CryptoErr(OVH_ERR_ARG)`). At most `OVH_ROUNDS_MAX` are open. Blocking.
    pub fn open_round(&self, hash: &[u8]) -> Result<Round, Box<dyn Error + Send>> {
        let mut id = 0u64;
        check(unsafe { ffi::ovh_round_open(self.raw(), hash.as_ptr(), hash.len(), &mut id) })?;
        Ok(Round { ctx: self.ctx.clone(), id, bitmap_len: (self.pubkeys.blocking_read().len() + 7) / 8 })
    }

    /// A flush's votes added to several open rounds in one device pass (`ovh_rounds_add`):
    /// `rounds[i]` is the round vote `i` is for, and the vote is verified under that round's hash.
    /// Every round ends as if `Round::add` had been called with the sub-list of its votes.
    /// Returns the per-vote codes and taken flags, then per distinct round, in order of first
    /// appearance: (round id, cumulative count, signature when `want_qc` and the count is not 0,
    /// bitmap when `want_qc`). `CryptoErr(OVH_ERR_ARG)` changes nothing; a device error closes the
    /// rounds of the call. Blocking.
    pub fn rounds_add(&self, rounds: &[&Round], sigs: &[[u8; 96]], voters: &[[u8; 48]], want_qc: bool) -> Result<RoundsAdd, Box<dyn Error + Send>> {
        if sigs.len() != voters.len() || sigs.len() != rounds.len() {
            return Err(to_err(ffi::OVH_ERR_LEN_MISMATCH));
        }
        let ids: Vec<u64> = rounds.iter().map(|r| r.id).collect();
        let mr = ffi::OVH_ROUNDS_MAX;
        let bl = (self.pubkeys.blocking_read().len() + 7) / 8;
        let mut codes = vec![0i32; sigs.len()];
        let mut taken = vec![0u8; sigs.len()];
        let mut n_rounds = 0u32;
        let mut round_ids = vec![0u64; mr];
        let mut n_signed = vec![0u32; mr];
        let mut out_sigs = vec![[0u8; 96]; mr];
        let mut bitmaps = vec![0u8; mr * bl];
        let (po, pb) = if want_qc { (out_sigs.as_mut_ptr() as *mut u8, bitmaps.as_mut_ptr()) } else { (std::ptr::null_mut(), std::ptr::null_mut()) };
        check(unsafe {
            ffi::ovh_rounds_add(self.raw(), sigs.len(), sigs.as_ptr() as *const u8, ids.as_ptr(), voters.as_ptr() as *const u8,
                                codes.as_mut_ptr(), taken.as_mut_ptr(), std::ptr::null_mut(), mr, &mut n_rounds,
                                round_ids.as_mut_ptr(), n_signed.as_mut_ptr(), po, pb, bl)
        })?;
        let per_round = (0..n_rounds as usize)
            .map(|k| {
                let sig = if want_qc && n_signed[k] > 0 { Some(Bytes::copy_from_slice(&out_sigs[k])) } else { None };
                let bm = if want_qc { Some(Bytes::copy_from_slice(&bitmaps[k * bl..(k + 1) * bl])) } else { None };
                (round_ids[k], n_signed[k], sig, bm)
            })
            .collect();
        Ok((codes, taken, per_round))
    }
}

/// What `HipCrypto::rounds_add` returns: per-vote codes and taken flags, then per distinct round
/// (id, cumulative count, signature, bitmap).
pub type RoundsAdd = (Vec<i32>, Vec<u8>, Vec<(u64, u32, Option<Bytes>, Option<Bytes>)>);

/// One open round of a `HipCrypto` (`ovh_round_open` .. `ovh_round_close`). For any cut of a vote
/// list into consecutive `add`s the codes, the taken flags, the count, the bitmap and the
/// signature equal `build_qc`'s over the whole list.
pub struct Round {
    ctx: Arc<Ctx>,
    id: u64,
    bitmap_len: usize,
}

/// What `Round::add` returns: the per-vote codes and taken flags of this add, the round's
/// cumulative count, and -- when asked for -- the cumulative QC (signature, bitmap); the
/// signature is `None` while nothing is taken.
pub type RoundAdd = (Vec<i32>, Vec<u8>, u32, Option<(Option<Bytes>, Bytes)>);

impl Round {
    /// The id `ovh_round_open` gave the round.
    pub fn id(&self) -> u64 {
        self.id
    }

    /// Verify `sigs.len()` more votes on the round's hash, select, and add the taken signatures
    /// to the round's sum, in one device pass over these votes only (`ovh_round_add`). Pass
    /// `want_qc` when this add is expected to cross the threshold: the compression then rides
    /// in the same pass. The verdicts enter the verdict cache. Blocking.
    pub fn add(&self, sigs: &[[u8; 96]], voters: &[[u8; 48]], want_qc: bool) -> Result<RoundAdd, Box<dyn Error + Send>> {
        if sigs.len() != voters.len() {
            return Err(to_err(ffi::OVH_ERR_LEN_MISMATCH));
        }
        let mut codes = vec![0i32; sigs.len()];
        let mut taken = vec![0u8; sigs.len()];
        let mut bitmap = vec![0u8; self.bitmap_len];
        let mut out = [0u8; 96];
        let mut n_signed = 0u32;
        let (po, pb) = if want_qc { (out.as_mut_ptr(), bitmap.as_mut_ptr()) } else { (std::ptr::null_mut(), std::ptr::null_mut()) };
        check(unsafe {
            ffi::ovh_round_add(self.ctx.0, self.id, sigs.len(), sigs.as_ptr() as *const u8, voters.as_ptr() as *const u8,
                               codes.as_mut_ptr(), taken.as_mut_ptr(), &mut n_signed, po, pb, self.bitmap_len)
        })?;
        let qc = if want_qc {
            let sig = if n_signed > 0 { Some(Bytes::copy_from_slice(&out)) } else { None };
            Some((sig, Bytes::from(bitmap)))
        } else {
            None
        };
        Ok((codes, taken, n_signed, qc))
    }

    /// The QC of what has been added so far, without any verification (`ovh_round_qc`):
    /// signature, bitmap, number of taken votes. `CryptoErr(4)` while nothing is taken. Blocking.
    pub fn qc(&self) -> Result<(Bytes, Bytes, u32), Box<dyn Error + Send>> {
        let mut bitmap = vec![0u8; self.bitmap_len];
        let mut out = [0u8; 96];
        let mut n_signed = 0u32;
        check(unsafe {
            ffi::ovh_round_qc(self.ctx.0, self.id, out.as_mut_ptr(), bitmap.as_mut_ptr(), self.bitmap_len, &mut n_signed)
        })?;
        Ok((Bytes::copy_from_slice(&out), Bytes::from(bitmap), n_signed))
    }
}

impl Drop for Round {
    fn drop(&mut self) {
        // an id that update_pubkeys already closed is refused (OVH_ERR_ARG): nothing to do
        unsafe { ffi::ovh_round_close(self.ctx.0, self.id) };
    }
}

impl OverlordCrypto for HipCrypto {
    /// consensus.rs:386-388 -> util.rs:81-87 (SM3).
    fn hash(&self, msg: Bytes) -> Bytes {
        let mut out = [0u8; 32];
        unsafe { ffi::ovh_sm3(msg.as_ptr(), msg.len(), out.as_mut_ptr()) };
        Bytes::copy_from_slice(&out)
    }

    /// consensus.rs:390-395: hash length (100), then sigma = sk H(hash), compressed.
    fn sign(&self, hash: Bytes) -> Result<Bytes, Box<dyn Error + Send>> {
        let mut out = [0u8; 96];
        check(unsafe {
            ffi::ovh_sign(self.raw(), self.private_key.as_ptr(), self.private_key.len(), hash.as_ptr(), hash.len(),
                          out.as_mut_ptr())
        })?;
        Ok(Bytes::copy_from_slice(&out))
    }

    /// consensus.rs:397-416: hash length (100), pk parse (102), sig parse (1..3), verify (3, 5, 6).
    fn verify_signature(&self, signature: Bytes, hash: Bytes, voter: Bytes) -> Result<(), Box<dyn Error + Send>> {
        check(unsafe {
            ffi::ovh_verify(self.raw(), signature.as_ptr(), signature.len(), hash.as_ptr(), hash.len(),
                            voter.as_ptr(), voter.len())
        })
    }

    /// consensus.rs:418-444: length check (101), per pair sig parse then pk parse (102), empty
    /// (4), sum in G2, compressed.
    fn aggregate_signatures(&self, signatures: Vec<Bytes>, voters: Vec<Bytes>) -> Result<Bytes, Box<dyn Error + Send>> {
        let (s, sl) = concat(&signatures);
        let (v, vl) = concat(&voters);
        let mut out = [0u8; 96];
        check(unsafe {
            ffi::ovh_aggregate_sigs(self.raw(), s.as_ptr(), sl.as_ptr(), sl.len(), v.as_ptr(), vl.as_ptr(), vl.len(),
                                    out.as_mut_ptr())
        })?;
        Ok(Bytes::copy_from_slice(&out))
    }

    /// consensus.rs:446-462 + 365-382: pk parse (102), aggregate (4), sig parse, hash length
    /// (100), verify.
    fn verify_aggregated_signature(&self, aggregated_signature: Bytes, hash: Bytes, voters: Vec<Bytes>) -> Result<(), Box<dyn Error + Send>> {
        let (v, vl) = concat(&voters);
        check(unsafe {
            ffi::ovh_verify_aggregated(self.raw(), aggregated_signature.as_ptr(), aggregated_signature.len(),
                                       hash.as_ptr(), hash.len(), v.as_ptr(), vl.as_ptr(), vl.len())
        })
    }
}

/// Backend selection beside `ConsensusConfig` (reference `src/config.rs:18-31`): the node reads
/// `crypto_backend` ("blst", the default, or "hip") and `crypto_devices` from its
/// `[consensus_overlord]` section and builds `ConsensusCrypto` or `HipCrypto` accordingly; the
/// `Overlord<…, C, …>` type parameter becomes an enum forwarding the five trait methods.
#[derive(Clone, Debug, PartialEq)]
pub enum CryptoBackend {
    Blst,
    Hip { devices: Vec<i32> },
}

impl CryptoBackend {
    pub fn from_config(backend: &str, devices: &[i32]) -> Option<Self> {
        match backend {
            "" | "blst" => Some(CryptoBackend::Blst),
            "hip" => Some(CryptoBackend::Hip { devices: devices.to_vec() }),
            _ => None,
        }
    }
}
