/*
 * libovhip — MI355X (gfx950) BLS12-381 signature backend for the overlord `Crypto` trait of
 * cita-cloud/consensus_overlord. C ABI: plain pointers and sizes, caller-owned host buffers,
 * no pointer is retained after a call returns. All curve arithmetic runs in HIP kernels; there
 * is no CPU fallback (a missing/failed device returns OVH_ERR_DEVICE). Every entry point is
 * thread-safe: a context serialises its device work internally (the trait object is Send +
 * Sync and is called concurrently by overlord and the gRPC check_block handler,
 * src/main.rs:107-127 -> src/consensus.rs:176).
 *
 * Return codes (int):
 *   0        OK
 *   1..7     BLST_ERROR of the failing signature parse / aggregate / verify
 *            (BAD_ENCODING, POINT_NOT_ON_CURVE, POINT_NOT_IN_GROUP, AGGR_TYPE_MISMATCH,
 *             VERIFY_FAIL, PK_IS_INFINITY, BAD_SCALAR)   -> ConsensusError::CryptoErr
 *   100      hash is not 32 bytes      -> ConsensusError::Other("failed to convert hash value")
 *   101      len(signatures) != len(voters)
 *                                     -> Other("signatures length does not match voters length")
 *   102      a public key does not parse -> Other("lose public key")
 *   103      invalid argument (NULL pointer, n too large, wrong context kind)
 *   200      HIP device error
 *   201      the OS random source (getrandom) failed
 *
 * Variable-length lists (Rust `Vec<Bytes>`) are passed as one concatenated byte buffer plus
 * an array of item lengths.
 */
#ifndef OVHIP_H
#define OVHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ovh_ctx ovh_ctx;

#define OVH_OK 0
#define OVH_ERR_HASH_LEN 100
#define OVH_ERR_LEN_MISMATCH 101
#define OVH_ERR_PUBKEY 102
#define OVH_ERR_ARG 103
/* A HIP error, or a batch's final stream gave up waiting for the vote pool. The latter is
 * sticky: every later synchronising call of the context (ovh_batch_wait, the synchronous batch
 * and partial / combine / fallback entry points) returns it, and the context must be destroyed. */
#define OVH_ERR_DEVICE 200
#define OVH_ERR_RNG 201

/* Flags for ovh_create / ovh_create_multi. */
#define OVH_FLAG_AGG_NO_GROUPCHECK 0x1u /* aggregate_signatures without the G2 subgroup check */
#define OVH_FLAG_PROFILE 0x2u           /* record HIP events around every batch stage */
#define OVH_FLAG_VM_TRACE 0x4u          /* diagnostics: per-phase clock of the VM kernels' workgroup 0 */
#define OVH_FLAG_TEST_RLC 0x8u          /* TESTS ONLY: batch coefficients from ovh_set_test_rlc (predictable) */
#define OVH_FLAG_SK_RAW 0x10u           /* private key = 32-byte big-endian scalar 0 < sk < r (blst
                                           SecretKey::from_bytes) instead of KeyGen (see ovh_sk_parse) */
#define OVH_FLAG_VM_CLOCK 0x20u         /* diagnostics: shader / wall clock stamps around every vote
                                           workgroup's program (ovh_vm_clock) */
#define OVH_FLAG_POOL_RESERVE 0x40u     /* the vote pool leaves 8 compute units (one per XCD; env
                                           OVH_POOL_RESERVE: another multiple of 8, <= 64) free for
                                           other kernels -- the caller's collective between shard
                                           batches -- and shard batches (ovh_batch_partial_device*,
                                           ovh_create_multi) share the persistent pool instead of a grid
                                           per batch. Use for a context whose partials cross RCCL. */

/* Batch stages (ovh_stage_name gives the label). Each stage is one or more kernels. */
#define OVH_NSTAGES 6

/* Create a context on HIP device `device` with hash-to-curve domain separation tag `dst`
 * (NULL -> "BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_NUL_", the believed ophelia-blst DST).
 * `dst` is 0-255 bytes (RFC 9380 5.3.1); longer returns NULL (the hashed oversize DST of 5.3.3
 * is not implemented); `dst != NULL` with length 0 is the empty DST.
 * Replaces ConsensusCrypto::new's crypto state (src/consensus.rs:347-359). NULL on failure. */
ovh_ctx* ovh_create(int device, const uint8_t* dst, size_t dst_len, uint32_t flags);
/* One context over several GPUs of this process: ovh_verify_batch and
 * ovh_prefetch split a batch into contiguous shards, one per device; each device computes its
 * shard's 864-byte partial, the partials are copied peer-to-peer (xGMI) to devices[0], which
 * runs the one combined check; on failure every device bisects its own shard. Single-call
 * entry points rotate over the devices. Devices may repeat (tests use {0, 0}); 1 <= ndev <= 8. */
ovh_ctx* ovh_create_multi(const int* devices, int ndev, const uint8_t* dst, size_t dst_len, uint32_t flags);
/* Peer access of a context's devices: out[a * n + b] = 1 when device a reaches device b's memory
 * directly (xGMI; enabled by ovh_create_multi for every pair hipDeviceCanAccessPeer allows) or a
 * and b are one device, 0 when copies between them stage through the host. Returns n (the
 * device count), or OVH_ERR_ARG when cap < n * n. The pipelined combined check
 * (ovh_verify_batch_async) rotates over the devices with peer access to and from every other. */
int ovh_multi_peer_matrix(ovh_ctx* ctx, uint8_t* out, size_t cap);
/* Synchronises every stream of the context and frees its device memory. The streams themselves
 * are not destroyed: they are parked per device and priority and handed to later contexts of
 * that device, so an ovh_stream handle -- and any event a caller recorded on it, e.g. torch's
 * pinned-host allocator after a non-blocking copy issued on ExternalStream(ovh_stream(ctx)) --
 * stays valid for the life of the process. Work a caller enqueued on ovh_stream before
 * ovh_destroy completes before the call returns. */
void ovh_destroy(ovh_ctx* ctx);
/* Number of devices of the context (1 for ovh_create). */
int ovh_device_count(ovh_ctx* ctx);
/* The HIP stream (hipStream_t) the context's per-vote kernels run on (first device). */
void* ovh_stream(ovh_ctx* ctx);

/* Crypto::hash -> util.rs:83-87 sm3_hash. */
int ovh_sm3(const uint8_t* msg, size_t len, uint8_t out[32]);
/* Crypto::hash in bulk (util.rs:83-87): digest i = SM3(data[off[i] .. off[i+1])), i < n, on the
 * device (one lane per message; csrc/sm3_bulk.hpp). Host form: host buffers, synchronous;
 * OVH_ERR_ARG for a NULL pointer, n > 2^24, offsets that decrease or more than 2^32 - 1 bytes in
 * all; n == 0 returns 0. _device: every pointer is device memory (d_data at any byte alignment),
 * the kernel is enqueued on ovh_stream and the call returns without waiting (stream order), as
 * ovh_vote_digests_device; an entry whose end offset is below its start gets the all-zero digest
 * and nothing of it is read. The kernel reads aligned 32-bit words, so it may touch up to 3 bytes
 * before the first and after the last byte of a message, inside the words that hold them. A
 * multi-device context uses its first device. */
int ovh_sm3_batch(ovh_ctx* ctx, size_t n, const uint8_t* data, const uint64_t* off /* n+1 */, uint8_t* digests /* n x 32 */);
int ovh_sm3_batch_device(ovh_ctx* ctx, size_t n, const uint8_t* d_data, const uint64_t* d_off, uint8_t* d_digests);

/* Vote digests on the device: digest i = SM3(rlp(Vote{height, round,
 * vote_type, block_hash})), the hash overlord signs and Consensus::check_block rebuilds
 * (consensus.rs:169-175 -> util.rs:83-87), so the batching shim can ship raw votes and feed the
 * digests straight to ovh_verify_batch_device. Vote i's block hash is the first hash_lens[i]
 * (<= OVH_VOTE_HASH_MAX; 0 = the empty hash of a nil vote) bytes at block_hashes + 64 i.
 * _device: every pointer is device memory, the kernel is enqueued on ovh_stream and the call
 * returns without waiting (stream order). Host form: host buffers, synchronous. */
#define OVH_VOTE_HASH_MAX 64
int ovh_vote_digests_device(ovh_ctx* ctx, size_t n, const uint64_t* heights, const uint64_t* rounds,
                            const uint8_t* vote_types, const uint8_t* block_hashes, const uint8_t* hash_lens,
                            uint8_t* digests);
int ovh_vote_digests(ovh_ctx* ctx, size_t n, const uint64_t* heights, const uint64_t* rounds, const uint8_t* vote_types,
                     const uint8_t* block_hashes, const uint8_t* hash_lens, uint8_t* digests);

/* BlsPrivateKey::try_from (consensus.rs:349-350, ophelia-blst [dep]): the 32-byte scalar the
 * context signs with, big-endian. Default: IETF KeyGen (blst SecretKey::key_gen(key, ""):
 * HKDF-SHA256, key >= 32 bytes) -- the reference's own example/private_key is >= r, so the
 * parse cannot be blst's strict from_bytes. With OVH_FLAG_SK_RAW: 32 bytes, 0 < sk < r.
 * BLST_BAD_ENCODING (1) when the key does not parse. Host only (no device work). */
int ovh_sk_parse(ovh_ctx* ctx, const uint8_t* key, size_t key_len, uint8_t out_scalar[32]);

/* Crypto::sign (consensus.rs:390-395): sigma = sk * H(hash), 96-byte compressed; `key` is the
 * private key bytes as ConsensusCrypto::new reads them (ovh_sk_parse). */
int ovh_sign(ovh_ctx* ctx, const uint8_t* key, size_t key_len, const uint8_t* hash, size_t hash_len, uint8_t out[96]);
/* BlsPrivateKey::pub_key + to_bytes (consensus.rs:352,357): 48-byte compressed pk. */
int ovh_sk_to_pk(ovh_ctx* ctx, const uint8_t* key, size_t key_len, uint8_t out[48]);

/* Crypto::verify_signature (consensus.rs:397-416). Answers from the verdict cache when the
 * (sig, hash, voter) triple was batch-verified by ovh_prefetch; otherwise one device check. */
int ovh_verify(ovh_ctx* ctx, const uint8_t* sig, size_t sig_len, const uint8_t* hash, size_t hash_len,
               const uint8_t* pk, size_t pk_len);

/* Crypto::aggregate_signatures (consensus.rs:418-444): 96-byte compressed sum.
 *
 * The route does not change what the call returns. On a single-device context with the
 * signature-point cache on (ovh_sig_cache_config), a call with n >= 1 in which every signature
 * has 96 and every key 48 bytes, every voter is a validator-table entry (ovh_set_validators)
 * whose key parsed and lies in G1, and every signature is in the cache sums the cached points: it
 * uploads 4 n bytes, decompresses and subgroup-checks nothing and waits for the device once. Any
 * other call runs the full path from its start (there is no partial mode). */
int ovh_aggregate_sigs(ovh_ctx* ctx, const uint8_t* sigs, const size_t* sig_lens, size_t n_sigs,
                       const uint8_t* pks, const size_t* pk_lens, size_t n_pks, uint8_t out[96]);

/* BlsPublicKey::aggregate (consensus.rs:371): 48-byte compressed sum. */
int ovh_aggregate_pks(ovh_ctx* ctx, const uint8_t* pks, const size_t* pk_lens, size_t n, uint8_t out[48]);

/* Crypto::verify_aggregated_signature (consensus.rs:446-462, 365-382).
 *
 * The route does not change what the call returns. With a 96-byte signature, a 32-byte hash,
 * n >= 1, every key of 48 bytes and every voter found in the validator table, the call sums the
 * table's points of the voters (any order, duplicates counted) and runs the per-call check on
 * that key, as ovh_verify_qc_batch does for one QC: no key bytes go up and no key is decompressed
 * (an entry whose key did not parse answers 102; one whose key lies outside G1 sends the call to
 * the full path, where the sum's own group check decides). The hash is looked up in the message
 * cache (ovh_prime_hashes) and never entered: on a hit the check runs without hash_to_G2, and
 * ovh_msg_cache_stats does not move either way. The environment variable OVH_QC_TABLE (read at
 * ovh_create) selects 0 = never, 1 = only for a hash that is in the message cache (default: on
 * a hash that is not, the full path is as fast), 2 = for every hash. A
 * multi-device context takes the route on the device the call lands on. */
int ovh_verify_aggregated(ovh_ctx* ctx, const uint8_t* agg_sig, size_t agg_len, const uint8_t* hash, size_t hash_len,
                          const uint8_t* pks, const size_t* pk_lens, size_t n);

/* ConsensusCrypto::update_pubkeys (consensus.rs:361-363; callers proc_reconfigure :131-136 and
 * Brain::commit :622-629): n x 48-byte compressed validator keys, in the order the node's config
 * lists them. Each key is decompressed and group-checked once on the device and kept as a
 * point in HBM. ovh_verify_batch / ovh_prefetch then skip the per-vote key decompression for
 * voters found in the table, and ovh_verify_qc_batch selects QC voters from it. Keys that do
 * not parse are kept (their votes answer 102, as the reference's per-call parse would). */
int ovh_set_validators(ovh_ctx* ctx, const uint8_t* pks, size_t n);

/* ConsensusCrypto::update_pubkeys for a node that keeps rounds open across commits. The reference
 * calls update_pubkeys on every committed block (Brain::commit), almost always with the list of the
 * block before, while the rounds of the next height are already open.
 * The table: every later call of the context that reads the validator table returns the same bytes
 * and codes as after ovh_set_validators(ctx, pks, n). A key's point and flags depend only on its 48
 * bytes, so they are copied from the old table, also for keys that do not parse or lie outside G1.
 *   Identical list (same n, bytes and order): returns 0 after a host comparison under the context
 *   mutex. No device call, no stream is waited for (batches in flight included), no round is touched.
 *   Changed list (any other, a permutation included): waits for the context's streams as
 *   ovh_set_validators does; only the keys whose bytes the old table does not hold are decompressed
 *   and subgroup-checked; the new table is built beside the old one and then swapped in.
 * Open rounds: a round is carried over when every voter it has taken is a key of the new list. It
 * keeps its id, hash, count, sum and budget. The defining property: let T be the votes it has taken
 * so far, in order; from the call on, n_signed, the bitmap (new length ceil(n / 8), new key order)
 * and the 96 bytes are those of a fresh round on the new table to which T was added, and so after
 * any further adds, for the codes and the taken flags of the new votes as well. A voter taken
 * before is still not taken twice, a key new to the table can be taken from then on, an invalid
 * vote still blocks nobody. A round that has taken a vote of a key the new list drops is closed
 * (its sum holds that signature), and every round is when n == 0: its id is written to closed[]
 * and is unknown from then on, as after ovh_round_close. *n_closed gets their number.
 * On a context without a table the call is ovh_set_validators. A multi-device context updates every
 * device's table; its rounds live on the first device. OVH_ERR_ARG (NULL context, NULL pks with
 * n > 0, n > 2^20) changes and writes nothing. */
int ovh_update_validators(ovh_ctx* ctx, const uint8_t* pks /* n x 48 */, size_t n,
                          uint64_t* closed /* OVH_ROUNDS_MAX ids, may be NULL */,
                          uint32_t* n_closed /* may be NULL */);

/* Counters of the validator table since ovh_create: [0] ovh_set_validators calls, [1] update calls
 * that found the list unchanged, [2] update calls that rebuilt the table, [3] keys that updates
 * sent through the decompression and subgroup check, [4] keys that updates carried over, [5] rounds
 * carried over by rebuilding updates, [6] rounds closed by updates, [7] table entries now.
 * OVH_ERR_ARG for a NULL context or NULL stats, which writes nothing. */
#define OVH_TABLE_NSTATS 8
int ovh_table_stats(ovh_ctx* ctx, uint64_t stats[8] /* OVH_TABLE_NSTATS */);

/* Batched verify_signature over n votes (fixed-size compressed encodings):
 * sigs n x 96 B, hashes n x 32 B, pks n x 48 B -> codes[n], codes[i] == the ovh_verify result
 * for vote i. One random-linear-combination check with secret 64-bit coefficients (a fresh
 * getrandom seed per batch) and, when it fails, a bisection: 16-vote groups, then per-vote
 * checks in the failing groups on the device-resident Miller outputs. Host buffers. */
int ovh_verify_batch(ovh_ctx* ctx, size_t n, const uint8_t* sigs, const uint8_t* hashes, const uint8_t* pks,
                     int32_t* codes);

/* Vote-batching ingress: batch-verify n votes as they arrive at
 * proc_network_msg (consensus.rs:210-262) and keep each verdict in the context's cache, keyed
 * by the exact (sig, hash, voter) bytes; overlord's later serial verify_signature calls
 * (ovh_verify) are then answered from the cache. Bounded FIFO cache (ovh_cache_config). */
int ovh_prefetch(ovh_ctx* ctx, size_t n, const uint8_t* sigs, const uint8_t* hashes, const uint8_t* pks);
/* Cache capacity in entries (0 disables the cache and empties it). Default 65536. */
int ovh_cache_config(ovh_ctx* ctx, size_t capacity);
/* stats[0] = hits, stats[1] = misses (fixed-size triples not in the cache), stats[2] = entries. */
int ovh_cache_stats(ovh_ctx* ctx, uint64_t stats[3]);
/* Same-message batches (ovh_verify_batch / ovh_prefetch on one device): when the n votes of a
 * call sign at most n / 2 distinct hashes (a round's votes all sign hash(rlp(Vote)), which has no
 * voter field: consensus.rs:169-175), the batch is checked as prod_g e(sum_{i in g} r_i pk_i, H_g)
 * e(-G1, sum_i r_i sigma_i) == 1 with one hash_to_G2 and one Miller loop per distinct hash
 * (per vote only the key and signature checks and r_i pk_i), then bisected per vote on failure;
 * the codes are the per-call codes as for any batch. By default the path takes batches of more
 * than OVH_SMALL_MAX (1,024) votes: below that the small-batch path (one wave per vote, one final
 * exponentiation) has the lower latency. The environment variable
 * OVH_SAMEMSG (read at ovh_create) selects 0 = never, 1 = above the small-batch size (default),
 * 2 = every batch with at most n / 2 distinct hashes (the least device work per vote). Counters
 * since ovh_create: stats[0] such batches, stats[1] their votes, stats[2] their distinct hashes. */
int ovh_samemsg_stats(ovh_ctx* ctx, uint64_t stats[3]);
/* Message cache of the per-call verify (ovh_verify, ovh_verify_batch with n = 1): H =
 * hash_to_G2(hash) of the last 256 hashes verified per call, so every later vote on a hash (all
 * votes of a round sign the same hash, consensus.rs:397-416) skips hash_to_G2. stats[0] = hits,
 * stats[1] = misses, summed over a multi-device context's devices. */
int ovh_msg_cache_stats(ovh_ctx* ctx, uint64_t stats[2]);
/* Prime the message cache ahead of a round: the bytes a node signs or verifies are known before
 * the signature is made or arrives (hash(rlp(Vote{height, round, type, block_hash})) carries no
 * voter: at proposal receipt the block's prevote and precommit hashes, at round start the nil
 * votes and the choke). Enqueues hash_to_G2 of every one of the k hashes (k x 32 bytes, k <=
 * OVH_PRIME_MAX) that is not in the 256-entry message cache, on a side stream of the context,
 * and returns without waiting for the device; hashes already cached or repeated in the call cost
 * no device work. Work that reads or fills the cache afterwards waits for the prime on the
 * device; work that does not touch the cache never waits for it. Consumers of a primed hash:
 * the per-call verify (a cache hit on the first vote), ovh_sign (the signature bytes are those of
 * an unprimed sign; a hash not in the cache is signed as before and is not entered), and
 * ovh_verify_batch / ovh_prefetch on one device for a part (the table-key votes or the other
 * votes of a call) of 2 .. OVH_SMALL_MAX votes outside the same-message route whose hashes are
 * all in the cache. The environment variables OVH_PRIME_SIGN and OVH_PRIME_BATCH (read at
 * ovh_create, 1 / 0) turn the sign and batch consumers on or off (defaults: DESIGN.md section
 * 3.6). A multi-device context primes every device. Returns OVH_ERR_ARG for a NULL context, NULL
 * hashes with k > 0 or k > OVH_PRIME_MAX (nothing is enqueued), 0 for k = 0. */
#define OVH_PRIME_MAX 64
int ovh_prime_hashes(ovh_ctx* ctx, size_t k, const uint8_t* hashes /* k x 32 */);
/* stats[0] = hashes for which device work was enqueued, stats[1] = hashes skipped (cached or
 * repeated), stats[2] = ovh_sign calls served from the cache, stats[3] = small-batch parts run on
 * cached H; since ovh_create, summed over a multi-device context's devices. */
int ovh_prime_stats(ovh_ctx* ctx, uint64_t stats[4]);

/* The signature-point cache: per single-device context, the decompressed
 * affine G2 point of fixed-size signatures that this context returned from ovh_sign or verified
 * with code 0 (the fill never adds a host synchronisation; a single vote's runs on a side stream
 * beside the check) -- by ovh_verify on the device, by ovh_verify_batch / ovh_prefetch of one vote, of
 * 2 .. OVH_SMALL_MAX votes or on the same-message route, by ovh_build_qc / ovh_build_qcs, and by
 * ovh_round_add / ovh_rounds_add -- keyed by the exact 96 signature bytes, FIFO replacement. The
 * device-pointer, pipelined, asynchronous and sharded entry points, multi-device contexts and
 * aggregated signatures fill nothing. ovh_aggregate_sigs reads it (see there); nothing else
 * does, and ovh_set_validators leaves it alone (a signature's point does not depend on the
 * table). `capacity` entries of 480 bytes; 0 disables the cache and empties it, a new capacity
 * empties it, the current one keeps it. The environment variable OVH_SIG_CACHE (read at
 * ovh_create) sets the initial capacity; the default is OVH_SIG_CACHE_DEFAULT, four full vote sets
 * of a 1,024-validator table. Returns OVH_ERR_ARG for a NULL context or a capacity above
 * OVH_SIG_CACHE_MAX (nothing changes); 0 on a multi-device context, which keeps no cache. */
#define OVH_SIG_CACHE_DEFAULT 4096
#define OVH_SIG_CACHE_MAX 65536
int ovh_sig_cache_config(ovh_ctx* ctx, size_t capacity);
/* Counters since ovh_create, summed over a multi-device context's devices:
 *   stats[0] signature points registered in the cache   stats[1] entries now
 *   stats[2] ovh_aggregate_sigs calls on the cache route stats[3] ... on the full path
 *   stats[4] signatures of fixed-size full-path calls that were not found in the cache
 *   stats[5] ovh_verify_aggregated calls on the table route
 *   stats[6] of those, calls whose hash was in the message cache
 *   stats[7] ovh_verify_aggregated calls on the full path
 * Returns OVH_ERR_ARG for a NULL context or NULL stats (nothing is written). */
int ovh_agg_stats(ovh_ctx* ctx, uint64_t stats[8]);

/* Batched QC verification for block sync (check_block, consensus.rs:143-207): QC j = aggregated
 * signature sigs[j] (96 B) over hashes[j] (32 B, the SM3 of rlp(Vote{h, r, Precommit, block})),
 * signed by the validators whose bits are set in bitmaps[j] (bitmap_len bytes, MSB first) over
 * the validator table sorted by key bytes (overlord extract_voters over the address-sorted
 * authority list; validators_to_nodes uses the key bytes as the address, util.rs:69-77).
 * codes[j] == ovh_verify_aggregated(sigs[j], hashes[j], those voters). One RLC batch over all
 * QCs. Needs ovh_set_validators. */
int ovh_verify_qc_batch(ovh_ctx* ctx, size_t nq, const uint8_t* sigs, const uint8_t* hashes, const uint8_t* bitmaps,
                        size_t bitmap_len, int32_t* codes);

/* Block sync in one device pass: Consensus::check_block (consensus.rs:143-207) for n blocks
 * against the validator table (ovh_set_validators). Block j = proposal height heights[j], proposal
 * data data[data_off[j] .. data_off[j+1]) and the overlord Proof's RLP bytes
 * proofs[proof_off[j] .. proof_off[j+1]).
 *   ok[j]       1 exactly when check_block(heights[j], data_j, proof_j) returns true, else 0.
 *   reasons[j]  (may be NULL) 0 when ok[j] is 1, else, in the reference's order: OVH_CB_PROOF_DECODE
 *               (Proof::decode failed, :158), OVH_CB_MISMATCH (proof.block_hash != sm3(data) or
 *               proof.height != height, :165), then the ovh_verify_aggregated code of the QC over
 *               hash(rlp(Vote{height, round, Precommit, block_hash})) and the voters of the bitmap
 *               (1..7, 102; no bit set: 4). The bitmap length is each proof's own.
 * The host decodes the proofs and expands the bitmaps; the device hashes the proposal bytes
 * (SM3 in bulk), compares, builds the vote digests and the aggregated keys and checks every QC in
 * one verify batch (secret coefficients, bisection: exact verdicts); the host waits once, after
 * everything is enqueued. A proof whose signature is not 96 bytes, or that selects a key outside
 * G1, is checked per call (ovh_verify_aggregated's path). Host buffers, synchronous,
 * thread-safe; a multi-device context runs it on its first device. Returns 0 when the verdicts
 * were written -- also with no validator table: every ok 0, as the reference with an empty
 * authority list; OVH_ERR_ARG for a NULL pointer, offsets that decrease, n > 2^20 or more than
 * 2^32 - 1 bytes of data or of proofs; device / RNG errors as elsewhere. */
#define OVH_CB_PROOF_DECODE 300 /* Proof::decode failed (consensus.rs:158) */
#define OVH_CB_MISMATCH 301     /* proof.block_hash != sm3(data) or proof.height != height (:165) */
int ovh_check_blocks(ovh_ctx* ctx, size_t n, const uint64_t* heights, const uint8_t* data,
                     const uint64_t* data_off /* n+1 */, const uint8_t* proofs, const uint64_t* proof_off /* n+1 */,
                     uint8_t* ok /* n */, int32_t* reasons /* n, may be NULL */);

/* The leader's side of a round in one device pass: verify the round's n votes on `hash` (the
 * SM3 of rlp(Vote), hash_len 32), select the votes that count, and aggregate their signatures
 * into the QC that ovh_verify_qc_batch and check_block consume. Replaces, for a round, overlord's
 * per-vote verify_signature (consensus.rs:397-416), the host's filtering and bitmap, and
 * aggregate_signatures (consensus.rs:418-444). sigs n x 96 B, pks n x 48 B; needs
 * ovh_set_validators. Host buffers, synchronous, thread-safe; a multi-device context runs it on
 * its first device, as ovh_verify_qc_batch.
 *   codes[i]   exactly the ovh_verify(sig_i, hash, pk_i) result of every vote, taken or not (the
 *              batch check of ovh_verify_batch: secret coefficients, bisection). The verdicts enter
 *              the verdict cache as ovh_prefetch's do.
 *   taken[i]   (may be NULL) 1 when vote i is taken, else 0. Vote i is taken iff codes[i] == 0, its
 *              voter is in the validator table, and no vote with a lower index is taken for the same
 *              voter (an invalid earlier vote of a voter does not block a later valid one).
 *   out_sig    the 96-byte compressed sum of the taken signatures.
 *   bitmap     bitmap_len == ceil(table size / 8) bytes, MSB first over the table sorted by key
 *              bytes (the extract_voters order, exactly what ovh_verify_qc_batch reads): one bit per
 *              taken voter, pad bits 0. A key that occurs twice in the table counts at its first
 *              position in sorted order.
 *   *n_signed  the number of taken votes (every validator has weight 1; the caller compares it
 *              with its threshold).
 * Returns 0; BLST_AGGR_TYPE_MISMATCH (4, aggregate_signatures of an empty list) when no vote is
 * taken -- codes, taken, a zero bitmap and *n_signed = 0 are still written, out_sig is not;
 * OVH_ERR_HASH_LEN when hash_len != 32; OVH_ERR_ARG for a NULL pointer, no validator table, a
 * wrong bitmap_len, n == 0 or n above the batch limit (2^24); device / RNG errors as elsewhere.
 * On the device the signatures are parsed and subgroup-checked once (by the verify batch, whose
 * points the sum reuses) and the host waits once, after everything is enqueued. */
int ovh_build_qc(ovh_ctx* ctx, size_t n, const uint8_t* sigs /* n x 96 */, const uint8_t* hash, size_t hash_len,
                 const uint8_t* pks /* n x 48 */, int32_t* codes /* n */, uint8_t* taken /* n, may be NULL */,
                 uint8_t out_sig[96], uint8_t* bitmap, size_t bitmap_len, uint32_t* n_signed);

/* The QCs of a mixed-hash vote set in one device pass: a leader's inbox as it arrives (the votes
 * of one (height, round, type) split between the block hash and the nil vote, late votes of the
 * previous round beside them), without knowing the winning hash first and without one device pass
 * per hash. One verify batch over all n votes (one hash_to_G2 and one Miller loop per distinct
 * hash, one MSM, one final exponentiation, exact per-vote bisection), then per distinct hash the
 * selection, the sum of the taken signatures and its compression, behind one synchronisation.
 * sigs n x 96 B, hashes n x 32 B, pks n x 48 B; needs ovh_set_validators. Host buffers,
 * synchronous, thread-safe; a multi-device context runs it on its first device. One vote (n == 1)
 * takes the per-call path, as in ovh_build_qc.
 *   groups        the distinct values among the rows of `hashes`, numbered by first appearance in
 *                 the caller's order. group[i] (may be NULL) is vote i's group, group_hashes[g]
 *                 that group's 32-byte hash, *n_groups their number G.
 *   codes[i]      exactly the ovh_verify(sig_i, hashes_i, pk_i) result of every vote, each under
 *                 its own hash. The verdicts enter the verdict cache as ovh_prefetch's do.
 *   taken[i]      (may be NULL) vote i is taken iff codes[i] == 0, its voter is in the validator
 *                 table, and no vote with a lower index of the same voter in the same group is
 *                 taken. A voter with valid votes in two groups (equivocation) is taken in both:
 *                 each QC stands alone, and what to do about the equivocation is the caller's
 *                 business.
 *   out_sigs[g]   (96 B each) the compressed sum of group g's taken signatures; not written for a
 *                 group with n_signed[g] == 0.
 *   bitmaps[g]    (bitmap_len == ceil(table size / 8) bytes each) ovh_build_qc's bitmap rule per
 *                 group: MSB first over the key-sorted table, a duplicated table key counts at its
 *                 first sorted position, pad bits 0; all zero for a group without a taken vote.
 *   n_signed[g]   the number of taken votes of group g.
 * Returns 0 whenever the outputs were written, also when some or all groups are empty (the caller
 * reads n_signed); OVH_ERR_ARG for a NULL required pointer, no validator table, a wrong
 * bitmap_len, n == 0, n > 2^24, max_groups == 0, or more distinct hashes than
 * min(max_groups, OVH_QC_GROUPS_MAX) -- the group count is decided on the host before any device
 * work, and nothing is written; device / RNG errors as elsewhere. With every row of `hashes`
 * equal, codes, taken, bitmap, count and the 96 signature bytes equal ovh_build_qc's. */
#define OVH_QC_GROUPS_MAX 64
int ovh_build_qcs(ovh_ctx* ctx, size_t n, const uint8_t* sigs /* n x 96 */, const uint8_t* hashes /* n x 32 */,
                  const uint8_t* pks /* n x 48 */, int32_t* codes /* n */, uint8_t* taken /* n, may be NULL */,
                  uint32_t* group /* n, may be NULL */, size_t max_groups, uint32_t* n_groups,
                  uint8_t* group_hashes /* max_groups x 32 */, uint8_t* out_sigs /* max_groups x 96 */,
                  uint8_t* bitmaps /* max_groups x bitmap_len */, size_t bitmap_len, uint32_t* n_signed /* max_groups */);

/* Rounds on the device: ovh_build_qc for votes that arrive in several flushes. A round keeps, in
 * device memory, which table entries have a taken vote, the bitmap, the count and the running sum
 * of the taken signatures; each ovh_round_add is one device pass over the new votes only, and the
 * QC is read without a second pass over the quorum. Needs ovh_set_validators. Host buffers,
 * synchronous, thread-safe (the context mutex, as ovh_build_qc); a multi-device context runs its
 * rounds on its first device.
 * The defining property: for any list of votes V on the round's hash and any cut of V into
 * consecutive pieces V1 .. Vk (pieces of one vote included), added in order, the concatenated
 * codes and taken equal what ovh_build_qc(V) writes, and after the last add *n_signed, the bitmap
 * and the 96 signature bytes equal ovh_build_qc(V)'s, byte for byte. So codes[i] is exactly the
 * ovh_verify result, and a vote is taken iff its code is 0, its voter is in the validator table
 * and no earlier vote of that voter was taken -- earlier in this add or in any earlier add of the
 * round. An invalid earlier vote does not block a later valid one, across adds too.
 *   ovh_round_open   opens a round on `hash` (the SM3 of rlp(Vote), hash_len 32); *round gets a
 *                    non-zero id that this context never reuses. At most OVH_ROUNDS_MAX are open.
 *                    The hash is primed as by ovh_prime_hashes (no wait), so the adds find H(hash)
 *                    in the message cache.
 *   ovh_round_add    verifies n more votes (sigs n x 96 B, pks n x 48 B), selects, and adds the
 *                    taken signatures to the round's sum. codes, taken (may be NULL): this add's
 *                    votes, as ovh_build_qc's. *n_signed: the round's cumulative count. bitmap
 *                    (may be NULL; else bitmap_len == ceil(table size / 8), checked only then):
 *                    the cumulative bitmap, ovh_build_qc's layout. out_sig (may be NULL): the
 *                    compressed cumulative sum, written only when *n_signed > 0 -- pass it when
 *                    this add is expected to cross the threshold: the compression then rides in
 *                    the same pass, behind the same single host synchronisation. The verdicts
 *                    enter the verdict cache as ovh_build_qc's do. Returns 0 whenever the outputs
 *                    were written, also when nothing was taken. A round accepts
 *                    OVH_ROUND_VOTES_MAX votes over all its adds. The votes are verified as
 *                    ovh_prefetch verifies a batch of that size: one vote per call, up to
 *                    OVH_SMALL_MAX on the small-batch path, more on the same-message route.
 *   ovh_round_qc     the QC of what has been added so far, without any verification: returns 0
 *                    and out_sig, bitmap, *n_signed; BLST_AGGR_TYPE_MISMATCH (4) while nothing is
 *                    taken (a zero bitmap and *n_signed = 0 are written, out_sig is not).
 *   ovh_round_close  frees the round; its id is unknown from then on.
 * Errors: OVH_ERR_HASH_LEN for hash_len != 32; OVH_ERR_ARG for a NULL required pointer, no
 * validator table, an unknown or closed id, n == 0, an open beyond OVH_ROUNDS_MAX, an add that
 * would take the round past OVH_ROUND_VOTES_MAX, or a wrong bitmap_len. A refused call changes
 * nothing: the next call behaves as if it had never been made. An add that fails with a device or
 * RNG error closes its round. ovh_set_validators closes every open round (the selection indexes
 * table entries, so their ids go stale); ovh_destroy frees them. ovh_build_qc / ovh_build_qcs
 * calls between the adds of a round do not disturb it. */
#define OVH_ROUNDS_MAX 16              /* rounds open per context */
#define OVH_ROUND_VOTES_MAX (1u << 24) /* votes a round accepts over all its adds */
int ovh_round_open(ovh_ctx* ctx, const uint8_t* hash, size_t hash_len, uint64_t* round);
int ovh_round_add(ovh_ctx* ctx, uint64_t round, size_t n, const uint8_t* sigs /* n x 96 */,
                  const uint8_t* pks /* n x 48 */, int32_t* codes /* n */, uint8_t* taken /* n, may be NULL */,
                  uint32_t* n_signed, uint8_t* out_sig /* 96, may be NULL */, uint8_t* bitmap /* may be NULL */,
                  size_t bitmap_len);
int ovh_round_qc(ovh_ctx* ctx, uint64_t round, uint8_t out_sig[96], uint8_t* bitmap, size_t bitmap_len,
                 uint32_t* n_signed);
int ovh_round_close(ovh_ctx* ctx, uint64_t round);

/* A flush's votes added to several open rounds in one device pass: the votes of one flush split
 * between the block hash and the nil vote, with late votes of another round beside them, and one
 * ovh_round_add per hash pays the fixed latency of a device pass each time. rounds[i] is the id
 * of the open round that vote i is for; that round's hash is the hash the vote is verified under.
 * One verify of all n votes, one final exponentiation, then selection, sum and merge per round,
 * behind one host synchronisation. Host buffers, synchronous, thread-safe; a multi-device context
 * runs the call on its first device.
 * The defining property: take any call and any round r named in it. The codes and taken of r's
 * votes, and r's n_signed, bitmap and 96 bytes after the call, equal what ovh_round_add(r, the
 * sub-list of r's votes in the caller's order) would have written in its place. Hence any
 * interleaving of ovh_rounds_add and ovh_round_add calls leaves every round equal, byte for byte,
 * to ovh_build_qc over the concatenation of that round's votes. A voter with valid votes in two
 * rounds is taken in both: each QC stands alone, as in ovh_build_qcs. Two rounds opened on the
 * same hash stay two rounds.
 *   numbering     the distinct ids are numbered by first appearance in the caller's order: slot[i]
 *                 (may be NULL) is vote i's number, round_ids[k] the id of number k, *n_rounds
 *                 their count K.
 *   codes, taken  per vote, as ovh_round_add's. The verdicts enter the verdict cache.
 *   n_signed[k]   the cumulative count of round k.
 *   bitmaps[k]    (may be NULL; else bitmap_len == ceil(table size / 8) bytes each, checked only
 *                 then) the cumulative bitmap of round k, ovh_build_qc's layout.
 *   out_sigs[k]   (may be NULL; 96 B each) the compressed cumulative sum of round k, written only
 *                 when n_signed[k] > 0. With NULL no compression runs.
 * A round's budget (OVH_ROUND_VOTES_MAX) counts only its own votes.
 * Routes: n == 1, or every vote on one round, is ovh_round_add itself. Else 2 .. OVH_SMALL_MAX
 * votes are verified as ovh_prefetch verifies those votes with their per-vote hashes (the
 * small-batch path, on the message cache's H where ovh_round_open primed it), and more votes (or
 * OVH_SAMEMSG=2) on the same-message route over the per-vote hashes, as ovh_build_qcs.
 * Returns 0 whenever the outputs were written, also when nothing was taken. OVH_ERR_ARG for a NULL
 * required pointer, n == 0, no validator table, any id that is unknown or closed, more distinct
 * ids than max_rounds (or than OVH_ROUNDS_MAX), a round that would pass OVH_ROUND_VOTES_MAX, or a
 * wrong bitmap_len: all decided on the host before any device work. A refused call changes
 * nothing: no round's budget moves and no device word is touched. A device or RNG error closes
 * every round named in the call. */
int ovh_rounds_add(ovh_ctx* ctx, size_t n, const uint8_t* sigs /* n x 96 */, const uint64_t* rounds /* n */,
                   const uint8_t* pks /* n x 48 */, int32_t* codes /* n */, uint8_t* taken /* n, may be NULL */,
                   uint32_t* slot /* n, may be NULL */, size_t max_rounds, uint32_t* n_rounds,
                   uint64_t* round_ids /* max_rounds */, uint32_t* n_signed /* max_rounds */,
                   uint8_t* out_sigs /* max_rounds x 96, may be NULL */,
                   uint8_t* bitmaps /* max_rounds x bitmap_len, may be NULL */, size_t bitmap_len);

/* TESTS ONLY (context created with OVH_FLAG_TEST_RLC, else OVH_ERR_ARG): vote i of every
 * following batch gets the coefficient SplitMix64(seed, index_base + i). Predictable
 * coefficients let an adversary cancel invalid signatures inside the combined check
 * (tests/test_rlc_soundness.py); production contexts never use this. index_base must be below
 * 2^63 (else OVH_ERR_ARG): the batch and shard paths add vote offsets to it, and the index
 * 2^64 - 1 is reserved for the unit scalar of a single vote checked alone. */
int ovh_set_test_rlc(ovh_ctx* ctx, uint64_t seed, uint64_t index_base);

/* The same as ovh_verify_batch with device-resident inputs/outputs (pointers into HBM), enqueued
 * on the context's streams; returns after the batch completed. */
int ovh_verify_batch_device(ovh_ctx* ctx, size_t n, const uint8_t* d_sigs, const uint8_t* d_hashes,
                            const uint8_t* d_pks, int32_t* d_codes);

/* Multi-GPU split of ovh_verify_batch_device (one process per GPU): per-shard partial =
 * {Fp12 product of the shard's Miller outputs (576 B), projective G2 sum of r_i sigma_i
 * (288 B)} = 864 bytes, written to d_partial (device memory); per-vote parse/subgroup codes go
 * to d_codes. The G2 sum is in homogeneous projective coordinates (X : Y : Z), O = (0 : 1 : 0).
 * Stream order: `stream` (a hipStream_t of the caller, e.g. torch's current stream) -- the
 * partial is written after the work already on `stream` (so a gather buffer can be reused) and
 * `stream` waits for the write; the call returns without blocking. stream NULL: the call
 * returns once d_partial is written. The inputs (d_sigs, d_hashes, d_pks) are read in
 * ovh_stream(ctx) order: a caller that produced them on another stream first makes ovh_stream
 * wait for it (shard.py does, through an event). */
#define OVH_PARTIAL_BYTES 864
int ovh_batch_partial_device(ovh_ctx* ctx, size_t n, const uint8_t* d_sigs, const uint8_t* d_hashes,
                             const uint8_t* d_pks, int32_t* d_codes, uint8_t* d_partial, void* stream);
/* Combine k partials (device memory, k x 864 B): *verdict = 1 if prod f * e(-G1, sum S) == 1
 * after the final exponentiation, else 0. Synchronous; returns 0 or an error code. */
int ovh_combine_partials_device(ovh_ctx* ctx, size_t k, const uint8_t* d_partials, int32_t* verdict);
/* Bisection of the last ovh_batch_partial_device shard (its combined check failed): d_codes[i]
 * still 0 -> the exact per-vote verify result. Synchronous. */
int ovh_batch_fallback_device(ovh_ctx* ctx, size_t n, int32_t* d_codes);

/* Pipelined batches. ovh_verify_batch_device_async enqueues one batch and returns without
 * waiting: the batch is staged and published on ovh_stream (its signatures and keys copied into
 * the library's own buffer, its hashes through hash_to_field), its per-vote work runs in the
 * context's vote pool (persistent workgroups that take 4-vote quads of the published batches in
 * order), and its combined check and (device-gated) bisection on a lower-priority final stream,
 * so batch k's final exponentiation overlaps later batches' per-vote work. The inputs are read
 * in ovh_stream order: they must be ready when the work enqueued there before the call is done,
 * and work enqueued there after the call may overwrite them. Up to OVH_BATCH_SLOTS batches may be
 * in flight per context; the d_codes of a batch must stay untouched until ovh_batch_wait
 * returns, after which they hold exactly the per-vote ovh_verify results. */
#define OVH_BATCH_SLOTS 6 /* batches in flight per context (state slots) */
int ovh_verify_batch_device_async(ovh_ctx* ctx, size_t n, const uint8_t* d_sigs, const uint8_t* d_hashes,
                                  const uint8_t* d_pks, int32_t* d_codes);
/* The pipelined same-message form: n votes in device memory that all sign the 32-byte `hash`
 * (host memory, read before the call returns) -- a round's precommits. One hash_to_G2 and one
 * key-sum Miller loop for the batch, the per-vote key and signature checks and RLC products on
 * two per-vote streams in turn (consecutive batches co-resident); codes
 * as ovh_verify_batch_device_async (exactly the per-vote ovh_verify results after
 * ovh_batch_wait, the same OVH_BATCH_SLOTS limit). The inputs are read after the caller's work
 * enqueued on ovh_stream before the call, and -- unlike that API's -- must stay untouched until
 * ovh_batch_wait returns, like the codes. Replaces,
 * for a round's votes, overlord calling Crypto::verify_signature (consensus.rs:397-416) once per
 * SignedVote. Single-device contexts. */
int ovh_verify_samemsg_device_async(ovh_ctx* ctx, size_t n, const uint8_t* d_sigs, const uint8_t* hash,
                                    const uint8_t* d_pks, int32_t* d_codes);
/* The pipelined form with host buffers, for single- and multi-device contexts (a node with no
 * torch; ovh_create_multi is its multi-GPU path): the inputs are copied into pinned staging
 * before the call returns (the caller may reuse them at once); `codes` (host, n entries) must
 * stay valid and is written by a later call of this function or ovh_batch_wait. Per batch each
 * device runs its shard's per-vote stages on its own pipeline, the partials go peer-to-peer
 * (xGMI) to the batch's final device, which rotates over the devices batch by batch, and each
 * device bisects its own shard when the combined check fails. At most OVH_BATCH_SLOTS batches
 * are in flight: a further call first completes the oldest. The caller's current HIP device is
 * unchanged on return. */
int ovh_verify_batch_async(ovh_ctx* ctx, size_t n, const uint8_t* sigs, const uint8_t* hashes, const uint8_t* pks,
                           int32_t* codes);
/* Completes every batch in flight on the context (device or host form, any context kind). */
int ovh_batch_wait(ovh_ctx* ctx);
/* Multi-GPU form: after ovh_batch_partial_device (n votes of this rank) and the all-gather of
 * the k <= 16 partials on `stream`, enqueue (stream-ordered after the gather) the combined check
 * and, if it fails, the bisection of this rank's n votes into d_codes; `stream` waits until the
 * partials were read. ovh_batch_wait completes it. */
int ovh_combine_partials_device_async(ovh_ctx* ctx, size_t k, const uint8_t* d_partials, size_t n,
                                      int32_t* d_codes, void* stream);

/* Device time (ms, HIP events) of each stage of the most recent batch call on a context created
 * with OVH_FLAG_PROFILE; stages that did not run read 0. Fills min(max, OVH_NSTAGES) entries
 * and returns that count (0 without the flag, <0 on error). */
int ovh_stage_times(ovh_ctx* ctx, float* ms, size_t max);
const char* ovh_stage_name(int stage);
/* Diagnostics (context created with OVH_FLAG_PROFILE): (start, end) in ms, relative to the
 * first, of the vote kernels of the last batches (up to 256, oldest first) -- pipelined vote
 * grids of consecutive batches overlap, so their device-level rate is the work over the union of
 * these spans. Writes min(count, max / 2) pairs and returns that number; max = 0 forgets the
 * batches recorded so far. */
int ovh_vote_spans(ovh_ctx* ctx, float* ms, size_t max);

/* Diagnostics (context created with OVH_FLAG_VM_TRACE): the wall clock (100 MHz counter) of
 * workgroup 0 of the last launch of VM program `prog` (0 vote, 1 fold, 2 final, 3 vote_t)
 * read after each phase barrier: copies min(max, nphases + 1) stamps, returns nphases + 1
 * (0 without the flag, <0 on error). */
int ovh_vm_trace(ovh_ctx* ctx, int prog, uint64_t* stamps, size_t max);
/* Diagnostics: `reps` batches of n zero votes through a VM program, *ms = wall time. prog 0:
 * vsame launches on one stream (streams = 1) or alternating over two (streams = 2: two
 * launches co-resident when the LDS allows, i.e. two waves per SIMD). prog 1: the vote pool,
 * batches published back to back (staging, hash_to_field, publication; no final-stream work).
 * prog 2: the vote pool with all reps <= OVH_BATCH_SLOTS batches published before its grids
 * start (no gap: the PMC passes' counters cover the batches and no idle wait). */
int ovh_diag_vm_occupancy(ovh_ctx* ctx, int prog, size_t n, int reps, int streams, float* ms);
/* Diagnostics (context created with OVH_FLAG_VM_CLOCK): per workgroup of the last vote / vote_t
 * launch, (delta s_memtime, delta s_memrealtime) around its VM program -- shader cycles and
 * 100 MHz ticks, so the clock the kernel held is delta_memtime / delta_realtime x 100 MHz
 * (MI355X_MICROARCH.md, DVFS give-back). Copies min(max, 2 x workgroups) values, returns
 * 2 x workgroups (0 without the flag, <0 on error). The stamps go to a buffer nothing else
 * reads; without the flag no stamp executes. */
int ovh_vm_clock(ovh_ctx* ctx, uint64_t* stamps, size_t max);

/* Diagnostics (context created with OVH_FLAG_VM_CLOCK): the vote pool's log, a ring of 64 batch
 * records of 2,064 words -- 100 MHz stamps of the batch's stream events (publication, pool done,
 * folds, MSM, final, bisection; word 15 its sequence number), then per quad (< 1,024) its start
 * (bits 0..47; bits 48..59 the SIMD it ran on: XCC, SE, SA, CU, SIMD as 3+2+1+4+2 bits; bits 60..63 how
 * its claim went: 1 last published batch, 2 its SIMD busy, 4 deferred, 8 busy and not deferred) and end. Copies up to `max` words after synchronising;
 * returns the log's size in words (0 without the flag, <0 on error). */
int ovh_pool_log(ovh_ctx* ctx, uint64_t* words, size_t max);

/* Batched helpers used to synthesise workloads on the device; d_sks are 32-byte big-endian
 * scalars (not key files). */
int ovh_sign_batch_device(ovh_ctx* ctx, size_t n, const uint8_t* d_sks, const uint8_t* d_hashes, uint8_t* d_sigs);
int ovh_sk_to_pk_batch_device(ovh_ctx* ctx, size_t n, const uint8_t* d_sks, uint8_t* d_pks);

#ifdef __cplusplus
}
#endif

#endif /* OVHIP_H */
