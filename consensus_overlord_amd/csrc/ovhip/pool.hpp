// The vote pool: the device queue and its log, PoolBatch, k_pool_publish / announce / wait,
// pool_claim, vote_quad, k_vm_pool and k_pool_stage. Relies on common.hpp.
// A fragment of ovhip.hip, included there once and in order: not a header to include elsewhere.

// ------------------------------------------------------------------------ the vote pool
// The per-vote work of every batch ("Vote pool"). A batch is published to a
// device queue as a descriptor; the pool kernel's workgroups (one wave each, four 16-lane vote
// slices) claim 4-vote quads from the queue in publication order -- across batches -- and run
// the "vote" / "vote_t" program on each, so a workgroup that finishes batch k's quad takes batch
// k + 1's at once: no grid boundary, no per-grid tail, no stream-order wait between batches. One
// pool grid is launched (on the pool stream) after each publication, which guarantees that some
// grid runs after the batch appeared; a workgroup exits when the queue is empty, so the grid
// launched for batch k + 1 usually finds batch k's grid still working and its own workgroups do
// nothing. A batch's final stream waits for its quads with k_pool_wait (done counter).
//
// Queue words (uint64, each on its own 128-byte line): cur = the oldest batch that may still have
// unclaimed quads; npub = batches published; slot_of[seq % POOL_SEQR] = the batch slot of batch
// seq; per slot, claim = (seq << 32) | quads claimed of the slot's batch and done = quads
// completed. A workgroup claims with ONE fetch-add on the claim word of batch cur's slot (no
// compare-and-swap window: r05a's CAS on a shared cursor handed out one quad per ~25 us). The
// claim word carries the batch it counts for, so a claim through a stale cur / slot_of is still
// exact: it is quad `count` of batch `seq` (processed iff count < that batch's nq, after its
// publication). Batches take batch slots (take_slot) and a slot is reused only after its batch
// completed; every quad a workgroup claimed below nq is processed, so a slot is never
// republished under a workgroup that holds one of its quads.
#define POOL_SEQR 16u
#define POOL_QW 16u  // uint64 words per 128-byte line
enum : uint32_t {
  PQ_CUR = 0,
  PQ_NPUB = POOL_QW,
  PQ_SLOTOF = 2 * POOL_QW,
  PQ_NANN = 3 * POOL_QW,
  PQ_DONE = 4 * POOL_QW,
  PQ_CLAIM = PQ_DONE + OVH_BATCH_SLOTS * POOL_QW,
  PQ_INFL = PQ_CLAIM + OVH_BATCH_SLOTS * POOL_QW,  // quads claimed and not yet done (all batches)
  PQ_OCC = PQ_INFL + POOL_QW,  // POOL_OCC_N uint32: pool quads running on each SIMD (simd_key)
};
constexpr uint32_t POOL_OCC_N = 4096;
constexpr uint32_t PQ_WORDS = PQ_OCC + POOL_OCC_N / 2;
static_assert(POOL_SEQR > OVH_BATCH_SLOTS && POOL_SEQR / 2 <= POOL_QW, "pool queue layout");
// A workgroup that finds the queue empty polls it for POOL_IDLE_TICKS (20 us) before it exits --
// or, while a batch is announced but not yet published (nann > npub: its staging and
// hash_to_field are on ovh_stream) or another workgroup still runs a quad (infl > 0: more batches
// are likely on their way), for up to POOL_WAIT_TICKS (20 ms). A grid whose spare workgroups left
// while the rest kept working holds its stream (the next batches' grids queue behind it), and the
// pool ran on the 1,024 workgroups that had found a quad: r05h without the announcement; r05x
// (pool log) with it, the host still enqueueing batch k's final stream 50 us after batch k's
// publication, before it announced batch k + 1.
#define POOL_IDLE_TICKS 2000ull
#define POOL_WAIT_TICKS 2000000ull

// The SIMD a wave runs on, as a 12-bit key: XCC (3 bits) | SE (2) | SA (1) | CU (4) | SIMD (2) from
// HW_REG_XCC_ID and HW_REG_HW_ID (amd_device_functions.h bit layout for gfx950); the pool log
// records it per quad (ovh_pool_log, tools/pool_timeline.py)
__device__ __forceinline__ uint32_t simd_key() {
  const uint32_t hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);   // HW_REG_HW_ID, all 32 bits
  const uint32_t xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20);  // HW_REG_XCC_ID bits 3:0
  return (xcc & 7u) << 9 | ((hw >> 13) & 3u) << 7 | ((hw >> 12) & 1u) << 6 | ((hw >> 8) & 15u) << 2 |
         ((hw >> 4) & 3u);
}
__device__ __forceinline__ uint32_t* pq_occ(uint64_t* q) { return reinterpret_cast<uint32_t*>(q + PQ_OCC); }
// SIMD spreading: while the current batch is the last published and its unclaimed quads fit the
// SIMDs that run no pool quad (estimate: SIMDs - quads in flight), a workgroup whose SIMD already
// runs a pool quad leaves the claim to one on an idle SIMD for up to POOL_SPREAD_TICKS (200 us):
// a lone batch's 1,024 quads then take 1,024 SIMDs (two quads on a SIMD take 4.6-5.6 ms, one
// 3.8, r05az) -- with the pool's grids dealt one wave per SIMD (pool_grid0)
#define POOL_SPREAD_TICKS 20000ull

struct PoolBatch {  // one published batch (written by k_pool_publish, read by the pool)
  uint64_t seq;          // its sequence number (written last: a claimer checks it, pool_claim)
  uint32_t n, nq;
  uint32_t table;        // 1: keys are points (program vote_t), 0: n x 48 compressed bytes (vote)
  uint32_t has_idx;      // vote_t: vote i uses table entry idx[i] (staged after the keys), else i
  uint64_t seed, base;   // RLC coefficients (vote_scalar)
  int32_t* codes;
  const uint32_t* planes;  // vote_t: key points (X, Y, Z planes of `pcap` entries) and flags
  const uint32_t* flags;
  uint32_t pcap, cap;    // cap: the state slab's
  uint32_t* state;       // the slot's state slab (u planes in; sigma, tau, f planes out)
  uint32_t* part0;       // fold region R0 (one partial per quad) of `part_cap` entries
  const uint8_t* stage;  // staged signatures | keys | table indices (k_pool_stage)
  uint64_t* clk;         // OVH_FLAG_VM_CLOCK: per-workgroup stamps, else null
  uint32_t part_cap, pad;
  uint64_t* plog;        // OVH_FLAG_VM_CLOCK: this batch's pool-log record (ovh_pool_log), else null
};

// Pool log (OVH_FLAG_VM_CLOCK diagnostics, ovh_pool_log): a ring of PLOG_RING batch records of
// PLOG_WORDS u64: [0..15] 100 MHz stamps of the batch's stream events (PLOG_EV_*) and its seq,
// then per quad (< PLOG_QUADS) its start (bits 0..47) with the SIMD it ran on (simd_key, bits 48..59), the
// claim flags (pool_claim, bits 60..63) and end.
#define PLOG_RING 64u
#define PLOG_QUADS 1024u
#define PLOG_WORDS (16u + 2u * PLOG_QUADS)
// then per pool grid launch (a ring of PLOG_GRIDS) and workgroup (< PLOG_WGS): entry and exit
// stamps, the quads it ran and how it left (1: idle with nothing announced, 2: POOL_WAIT_TICKS,
// 3: the claim loop's bound)
#define PLOG_GRIDS 64u
#define PLOG_WGS 1024u
#define PLOG_WG_WORDS 4u
#define PLOG_GRID_BASE ((size_t)PLOG_RING * PLOG_WORDS)
#define PLOG_TOTAL (PLOG_GRID_BASE + (size_t)PLOG_GRIDS * (4 + PLOG_WGS * PLOG_WG_WORDS))
// (the shard path's combine: GATH on the caller's stream when ovh_combine_partials_device_async is
// called -- after its all-gather --, COMB once the final stream read the partials, FE after the
// combined check's final exponentiation)
enum : uint32_t { PLOG_EV_PUB = 0, PLOG_EV_DONE = 1, PLOG_EV_FOLD = 2, PLOG_EV_MSM = 3, PLOG_EV_FINAL = 4,
                  PLOG_EV_BACK = 5, PLOG_EV_GATH = 6, PLOG_EV_COMB = 7, PLOG_EV_FE = 8, PLOG_EV_SEQ = 15 };
__global__ void k_grid_hdr(uint64_t* g, uint64_t seq, uint32_t par, uint32_t wgs) {
  for (uint32_t k = threadIdx.x; k < PLOG_WGS * PLOG_WG_WORDS; k += blockDim.x) g[4 + k] = 0;
  __syncthreads();
  if (threadIdx.x == 0) {
    g[0] = seq;
    g[1] = par;
    g[2] = wgs;
    g[3] = __builtin_amdgcn_s_memrealtime();  // its launch point on the pool stream
  }
}
__global__ void k_stamp(uint64_t* p, uint64_t v) {
  if (threadIdx.x == 0) {
    p[0] = __builtin_amdgcn_s_memrealtime();
    if (v != ~0ull) p[PLOG_EV_SEQ] = v;
  }
}

// The pool kernel's arguments: the queue, the descriptors, the two vote programs' instruction
// and side-word streams, the fold program (all three renumbered to the pool's constant table,
// `cst`: ovhip/pool_remap.hpp) and the spill scratch. Everything
// per batch is in the descriptor and read where it is used.
struct PoolArgs {
  uint64_t* q;
  const PoolBatch* descs;
  const uint4* pv_code;
  const uint32_t* pv_side;
  const uint4* pt_code;
  const uint32_t* pt_side;
  const uint4* fold_code;
  const uint32_t* cst;
  uint32_t* scr;  // VM_SLICES x VOTE_NSCR entries per workgroup
  uint64_t* wlog;  // OVH_FLAG_VM_CLOCK: this grid's workgroup log (PLOG_WG_WORDS per workgroup), else null
  uint64_t only;   // ~0: claim any batch; else this grid's own batch: its workgroups leave once
                   // `cur` has passed it (the shard path's grid per batch, ovh_batch_partial_device)
  uint32_t nsimd;  // SIMDs the pool runs on (SIMD spreading, pool_claim)
  uint32_t skip_cu;  // OVH_FLAG_POOL_RESERVE: workgroups on CUs 0 .. skip_cu - 1 of SE 0 / SA 0 of
                     // every XCC leave at once (those CUs stay free for other kernels); 0: none
};

__device__ __forceinline__ uint64_t* pq_done(uint64_t* q, uint32_t slot) { return q + PQ_DONE + slot * POOL_QW; }
__device__ __forceinline__ uint64_t* pq_claim(uint64_t* q, uint32_t slot) { return q + PQ_CLAIM + slot * POOL_QW; }
__device__ __forceinline__ uint32_t* pq_slot_of(uint64_t* q) { return reinterpret_cast<uint32_t*>(q + PQ_SLOTOF); }
__device__ __forceinline__ uint64_t qld(const uint64_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Publish batch `seq` in slot `slot` (one lane; ovh_stream, after the batch's hash_to_field and
// staging): the descriptor, then (behind a release) its seq, done = 0, the claim word and
// slot_of, then (behind a release) npub.
__global__ __launch_bounds__(64) void k_pool_publish(PoolBatch b, uint32_t slot, uint64_t seq, uint64_t* q,
                                                     PoolBatch* descs) {
  if (threadIdx.x) return;
  b.seq = ~0ull;
  descs[slot] = b;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __hip_atomic_store(&descs[slot].seq, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(pq_done(q, slot), 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(pq_claim(q, slot), seq << 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(pq_slot_of(q) + seq % POOL_SEQR, slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (MI355X_MICROARCH.md: the wait the compiler may drop)
  __hip_atomic_store(q + PQ_NPUB, seq + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Announce batch seq: nann = seq + 1 tells idle pool workgroups that a publication is on its way
// (pool_take_slot: on ovh_stream ahead of the slot wait, so the announcement of the next batch
// follows the publication of the previous one and never waits for a slot).
__global__ __launch_bounds__(64) void k_pool_announce(uint64_t* q, uint64_t n) {
  if (threadIdx.x == 0) __hip_atomic_store(q + PQ_NANN, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Claim the next quad (the whole wave, in wave-uniform control flow: every lane reads the same
// queue words, lane 0 alone performs the atomics and the result is broadcast -- r05c ran the
// claim loop in a lane-0 branch, and the workgroup's later quads ran with lane 0 alone active).
// Returns 1 and the quad's slot and index, or 0 when the queue stays empty for
// POOL_IDLE_TICKS. Every quad is handed out by exactly one fetch-add on its batch's claim word; a
// claim past the batch's nq moves `cur` on.
__device__ __forceinline__ uint64_t lane0_fetch_add(uint64_t* p, uint64_t v) {
  uint64_t r = 0;
  if (threadIdx.x == 0) r = __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(r >> 32)) << 32) |
         __builtin_amdgcn_readfirstlane((uint32_t)r);
}
__device__ __forceinline__ uint32_t lane0_fetch_add32(uint32_t* p, uint32_t v) {
  uint32_t r = 0;
  if (threadIdx.x == 0) r = __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return __builtin_amdgcn_readfirstlane(r);
}
__device__ __forceinline__ void lane0_cas(uint64_t* p, uint64_t expect, uint64_t want) {
  if (threadIdx.x == 0) {
    uint64_t e = expect;
    (void)__hip_atomic_compare_exchange_strong(p, &e, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
  }
}
__device__ __forceinline__ uint64_t wclock() {
  const uint64_t t = wall_clock64();
  return ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(t >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)t);
}
__device__ __forceinline__ uint64_t qldu(const uint64_t* p) {
  const uint64_t v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)v);
}
__device__ uint32_t pool_claim(uint64_t* q, const PoolBatch* descs, uint32_t* slot_out, uint32_t* quad_out,
                               uint32_t* why, uint64_t only, uint32_t nsimd, uint32_t* how) {
  uint64_t t0 = wclock(), tdef = 0;
  uint32_t hw = 0;  // how the claim went (pool log): 1 last published, 2 SIMD busy, 4 deferred, 8 busy and not deferred
  uint32_t* occ = pq_occ(q) + simd_key();
  *why = 3;
#pragma unroll 1
  for (uint32_t tries = 0; tries < (1u << 22); ++tries) {
    const uint64_t s = qldu(q + PQ_CUR), np = qldu(q + PQ_NPUB);
    if (s > only) {  // a grid of one batch: that batch is fully claimed
      *why = 4;
      return 0;
    }
    if (s >= np) {
      const uint64_t idle = wclock() - t0;
      if (idle > POOL_WAIT_TICKS ||
          (idle > POOL_IDLE_TICKS && qldu(q + PQ_NANN) <= np && qldu(q + PQ_INFL) == 0)) {
        *why = idle > POOL_WAIT_TICKS ? 2 : 1;
        return 0;
      }
      // past the idle window, poll ~16x less often: 1,700 waiting workgroups polling two queue
      // words every ~0.2 us kept a shard batch's all-gather and combine from running while the
      // pool waited for that batch's slot (r06i / r06j pool logs: 20 ms stalls)
      if (idle > POOL_IDLE_TICKS) __builtin_amdgcn_s_sleep(127);
      else __builtin_amdgcn_s_sleep(8);
      continue;
    }
    const uint32_t slot = __builtin_amdgcn_readfirstlane(
        __hip_atomic_load(pq_slot_of(q) + s % POOL_SEQR, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    // SIMD spreading: this SIMD's occupancy is taken first (one fetch-add, so two workgroups of a
    // SIMD polling the same publication cannot both see it idle), then the claim is deferred
    // while the SIMD was busy
    bool held = false;
    if (np == s + 1) {
      hw |= 1u;
      bool busy;
      if (tdef && __builtin_amdgcn_readfirstlane(__hip_atomic_load(occ, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
        busy = true;  // deferring: a plain load while the SIMD stays busy
      } else {
        busy = lane0_fetch_add32(occ, 1u) != 0;
        held = true;
      }
      if (busy) {
        hw |= 2u;
        const uint64_t cw = qldu(pq_claim(q, slot));
        const uint32_t nq = __builtin_amdgcn_readfirstlane(
            __hip_atomic_load(&descs[slot].nq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        const uint64_t infl = qldu(q + PQ_INFL);
        const uint32_t taken = (uint32_t)cw;
        // (a slack of nsimd / 16: at nsimd exactly, a lone batch's late arrivals claimed next to a
        // running quad instead of deferring -- pool-log claim flags 11, r05bj)
        if ((cw >> 32) == s && taken < nq && (uint64_t)(nq - taken) + infl <= nsimd + nsimd / 16) {
          const uint64_t now = wclock();
          if (!tdef) tdef = now;
          if (now - tdef < POOL_SPREAD_TICKS) {
            hw |= 4u;
            if (held) (void)lane0_fetch_add32(occ, ~0u);
            __builtin_amdgcn_s_sleep(32);
            continue;
          }
        }
        hw |= 8u;
      }
    }
    if (!held) (void)lane0_fetch_add32(occ, 1u);
    const uint64_t old = lane0_fetch_add(pq_claim(q, slot), 1ull);
    const uint64_t seq = old >> 32;
    const uint32_t idx = (uint32_t)old;
    // the claim counts for batch `seq` (a stale slot_of may have led here): wait for its publication
    const uint64_t tw = wclock();
    while (qldu(q + PQ_NPUB) <= seq && wclock() - tw < 100000000ull) __builtin_amdgcn_s_sleep(2);
    const uint32_t nq = __builtin_amdgcn_readfirstlane(
        __hip_atomic_load(&descs[slot].nq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint64_t dseq = qldu(&descs[slot].seq);
    // dseq != seq: the slot was republished, so batch seq completed -- every quad of it below nq
    // was claimed by others, this one is past its end
    const bool mine = dseq == seq && idx < nq;
    // batch s is fully claimed when this claim went past its end, or when its slot already holds
    // a later batch (seq != s: a slot is republished only after its batch completed): move cur on
    // (whoever wins; a claim that took exactly the last quad does not, the next claimer does)
    if (seq != s || !mine) lane0_cas(q + PQ_CUR, s, s + 1);
    if (mine) {
      (void)lane0_fetch_add(q + PQ_INFL, 1ull);
      *slot_out = slot;
      *quad_out = idx;
      *how = hw;
      return 1;
    }
    (void)lane0_fetch_add32(occ, ~0u);  // - 1: no quad after all
    tdef = 0;
    t0 = wclock();  // progress: the idle window restarts
  }
  return 0;
}

// Descriptor fields are read where they are used (relaxed agent-scope loads: vector loads, never
// the scalar cache), so no batch state stays live across the VM program: the vote program
// already needs every VGPR of a two-waves-per-SIMD budget and most SGPRs.
template <typename T>
__device__ __forceinline__ T dget(const T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename T>
__device__ __forceinline__ T* dgetp(T* const* p) {
  return reinterpret_cast<T*>(__hip_atomic_load(reinterpret_cast<const uint64_t*>(p), __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t uni64(uint64_t v) {
  return ((uint64_t)uni((uint32_t)(v >> 32)) << 32) | uni((uint32_t)v);
}
template <typename T>
__device__ __forceinline__ T* unip(T* p) {
  return reinterpret_cast<T*>(uni64(reinterpret_cast<uint64_t>(p)));
}

// One quad of a batch: votes 4 quad .. 4 quad + 3 on the four slices -- inputs, the vote / vote_t
// program, the per-vote code in the reference's precedence, then fold level 0 of the quad's f
// (fused: -> partial `quad` of R0, the identity for failed votes). Only the VM's own operands
// stay in registers across the program: the slot and quad wait in the LDS header words of slice
// 2 and the clock stamps (OVH_FLAG_VM_CLOCK) in those of slices 0 and 1.
// TABLE (wave-uniform: the batch's keys come from the validator table, program vote_t, or as
// bytes, program vote) picks the slot count, stride, phase count, maps, code and side words, the
// prologue and the epilogue -- all values or uniform branches around the one interpreter loop
// both kinds of quad go through (two instantiations doubled the kernel's code).
// The pool's vote loop is the throughput stage: it keeps the loop unrolled over its register
// rings whatever OVH_VM_UNROLL gives the other kernels (A/B: DESIGN 4.7).
#ifndef OVH_POOL_UNROLL
#define OVH_POOL_UNROLL 3
#endif
__device__ __forceinline__ void vote_quad(const PoolArgs& a, uint32_t slot_in, uint32_t quad_in, uint32_t* lds,
                                          const bool TABLE) {
  // the vote loop's interpreter: no inversion, radix 2^392 (products without the conditional
  // subtraction, fpvm.hpp); the programs convert at their own edges (tools/fpvm/progs.py), so the
  // prologue, the epilogue, the fused fold and every plane keep value * 2^384
  VM_ASSERT_NO_INV_ANY_RADIX(VOTE);
  VM_ASSERT_NO_INV_ANY_RADIX(VOTE_T);
  VM_ASSERT_RADIX(VOTE, 392);
  VM_ASSERT_RADIX(VOTE_T, 392);
  const uint32_t NSLOTS = TABLE ? VM_VOTE_T_NSLOTS : VM_VOTE_NSLOTS;
  const uint32_t STRIDE = TABLE ? VOTE_T_STRIDE_W : VOTE_STRIDE_W;
  const uint32_t NPH = TABLE ? VM_VOTE_T_NPHASES : VM_VOTE_NPHASES;
  const uint16_t* IN = TABLE ? VM_VOTE_T_IN : VM_VOTE_IN;
  const uint16_t* OUT = TABLE ? VM_VOTE_T_OUT : VM_VOTE_OUT;
  uint32_t* cst = lds;
  const uint32_t slice = threadIdx.x / VM_VOTE_W, lane = threadIdx.x % VM_VOTE_W;
  uint32_t* slots = lds + SLOT_BASE_W + slice * STRIDE;
  uint32_t* hdr = slots + NSLOTS * 12;  // [sig flags, pk flags, (slice 0..2: stamps, slot, quad)]
  uint32_t* park = lds + SLOT_BASE_W + 2 * STRIDE + NSLOTS * 12 + 2;  // slice 2's hdr[2..3]
  {
    const PoolBatch* bd = a.descs + slot_in;
    const uint32_t i = (quad_in & 0x0FFFFFFFu) * VM_SLICES + slice;  // (top bits: the claim flags)
    const uint32_t n = uni(dget(&bd->n));
    const bool active = i < n;
    const uint8_t* sigs = unip(dgetp(&bd->stage));
    const Slab s{unip(dgetp(&bd->state)), uni(dget(&bd->cap))};
    if (active) {
      if (lane == 0) {
        uint32_t x1[12], x0[12], bad, inf, sort, xz;
        parse_hdr(sigs + (size_t)i * 96, 96, x1, x0, bad, inf, sort, xz);
        slot_put(slots, IN[TABLE ? VM_VOTE_T_IN_SIG_X1 : VM_VOTE_IN_SIG_X1], x1);
        slot_put(slots, IN[TABLE ? VM_VOTE_T_IN_SIG_X0 : VM_VOTE_IN_SIG_X0], x0);
        slot_flag(slots, IN[TABLE ? VM_VOTE_T_IN_SIG_SORT : VM_VOTE_IN_SIG_SORT], sort);
        hdr[0] = bad | inf << 1 | xz << 2;
      } else if (lane >= 2 && lane < 6) {
        Fp u;
        s.ld(u, S_U + (lane - 2), i);
        slot_put(slots, IN[(TABLE ? VM_VOTE_T_IN_U00 : VM_VOTE_IN_U00) + (lane - 2)], u.v);
      }
    }
    if (threadIdx.x == 0) {
      park[0] = slot_in;
      park[1] = quad_in;
      if (dgetp(&bd->plog)) {
        uint32_t* h3 = lds + SLOT_BASE_W + 3 * STRIDE + NSLOTS * 12 + 2;
        const uint64_t t = __builtin_amdgcn_s_memrealtime();
        h3[0] = (uint32_t)t;
        h3[1] = (uint32_t)(t >> 32);
      }
    }
    __syncthreads();
    if (active) {
      if (TABLE) {
        const int32_t* idx = reinterpret_cast<const int32_t*>(sigs + (size_t)n * 144);
        const uint32_t e = uni(dget(&bd->has_idx)) ? (uint32_t)idx[i] : i;
        if (lane == 1) {
          hdr[1] = unip(dgetp(&bd->flags))[e];
        } else if (lane >= 6 && lane < 9) {
          Fp v;
          Slab{const_cast<uint32_t*>(unip(dgetp(&bd->planes))), uni(dget(&bd->pcap))}.ld(v, lane - 6, e);
          slot_put(slots, IN[VM_VOTE_T_IN_PK_X + (lane - 6)], v.v);
        }
      } else {
        if (lane == 1) {
          uint32_t x[12], bad, inf, sort, xz;
          parse_hdr(sigs + (size_t)n * 96 + (size_t)i * 48, 48, x, x, bad, inf, sort, xz);
          slot_put(slots, IN[VM_VOTE_IN_PK_X], x);
          slot_flag(slots, IN[VM_VOTE_IN_PK_SORT], sort);
          hdr[1] = bad | inf << 1 | xz << 2;
        }
      }
    }
    if (threadIdx.x == 0 && dgetp(&bd->clk)) {
      const uint64_t t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
      uint32_t* h0 = lds + SLOT_BASE_W + NSLOTS * 12 + 2;
      uint32_t* h1 = lds + SLOT_BASE_W + STRIDE + NSLOTS * 12 + 2;
      h0[0] = (uint32_t)t0;
      h0[1] = (uint32_t)(t0 >> 32);
      h1[0] = (uint32_t)r0;
      h1[1] = (uint32_t)(r0 >> 32);
    }
    __syncthreads();
    const uint64_t scalar = vote_scalar(uni64(dget(&bd->seed)), uni64(dget(&bd->base)), i);
    vm::run<true, false, OVH_POOL_UNROLL, 392>(
        TABLE ? a.pt_code : a.pv_code, NPH, VM_VOTE_W, lane, active, slots, cst, scalar, vm::Out{s.p, s.cap, i},
        nullptr, TABLE ? a.pt_side : a.pv_side,
        a.scr + (size_t)blockIdx.x * VM_SLICES * VOTE_NSCR * 12 + slice * VOTE_NSCR * 12);
  }
  // after the program: the slot and quad back from LDS (run ends with an LDS wait + barrier)
  const uint32_t slot = uni(park[0]), quad = uni(park[1]) & 0x0FFFFFFFu, how = uni(park[1]) >> 28;
  const PoolBatch* bd = a.descs + slot;
  const uint32_t i = quad * VM_SLICES + slice;
  const uint32_t n = uni(dget(&bd->n));
  int32_t* codes = unip(dgetp(&bd->codes));
  if (uint64_t* clk = dgetp(&bd->clk); clk && threadIdx.x == 0 && blockIdx.x < VM_CLOCK_WGS) {
    const uint32_t* h0 = lds + SLOT_BASE_W + NSLOTS * 12 + 2;
    const uint32_t* h1 = lds + SLOT_BASE_W + STRIDE + NSLOTS * 12 + 2;
    const uint64_t t0 = h0[0] | (uint64_t)h0[1] << 32, r0 = h1[0] | (uint64_t)h1[1] << 32;
    clk[2 * blockIdx.x] = __builtin_amdgcn_s_memtime() - t0;
    clk[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime() - r0;
  }
  if (i < n && lane == 0) {
    const uint32_t sf = hdr[0], pf = hdr[1];
    const uint32_t sg_bad = sf & 1, sg_inf = (sf >> 1) & 1, sg_xz = (sf >> 2) & 1;
    const uint32_t sg_ok = slot_flag_get(slots, OUT[TABLE ? VM_VOTE_T_OUT_SIG_OK : VM_VOTE_OUT_SIG_OK]);
    const uint32_t sg_grp = slot_flag_get(slots, OUT[TABLE ? VM_VOTE_T_OUT_SIG_GRP : VM_VOTE_OUT_SIG_GRP]);
    const uint32_t h_inf = slot_flag_get(slots, OUT[TABLE ? VM_VOTE_T_OUT_H_INF : VM_VOTE_OUT_H_INF]);
    // consensus.rs:397-416: pk parse (102) > sig parse (1..3) > [core_verify] sig group (3) >
    // pk infinity (6) > pk group (3) > H(m) = O or sig = O (5) > pairing (batch)
    uint32_t pk_parse, pk_inf, pk_grp;
    if (TABLE) {
      pk_parse = pf & PKF_PARSE;
      pk_inf = pf & PKF_INF;
      pk_grp = !(pf & PKF_GRP);
    } else {
      const uint32_t pk_bad = pf & 1, pk_xz = (pf >> 2) & 1;
      pk_inf = (pf >> 1) & 1;
      const uint32_t pk_ok = slot_flag_get(slots, OUT[VM_VOTE_OUT_PK_OK]);
      pk_grp = slot_flag_get(slots, OUT[VM_VOTE_OUT_PK_GRP]);
      pk_parse = pk_bad || (!pk_inf && (!pk_ok || pk_xz));
    }
    int32_t c;
    if (pk_parse) c = OVH_ERR_PUBKEY;
    else if (sg_bad) c = BLST_BAD_ENCODING;
    else if (!sg_inf && !sg_ok) c = BLST_POINT_NOT_ON_CURVE;
    else if (!sg_inf && (sg_xz || !sg_grp)) c = BLST_POINT_NOT_IN_GROUP;
    else if (pk_inf) c = BLST_PK_IS_INFINITY;
    else if (!pk_grp) c = BLST_POINT_NOT_IN_GROUP;
    else if (h_inf || sg_inf) c = BLST_VERIFY_FAIL;
    else c = 0;
    codes[i] = c;
  }
  // fold level 0, fused: the quad's 4 votes -> partial `quad` of R0 (F planes 0..11, S planes
  // 12..17), the identity for failed votes. The slices' `st` outputs (HBM) and codes are made
  // visible to the workgroup first; the fold reuses the vote slots' LDS.
  __threadfence();
  __syncthreads();
  // the pool log's pointer and the quad's start stamp (slice 3's LDS header) into registers now:
  // fold_unit reuses the slot LDS, and once done reaches nq the slot may carry the next batch
  // 
  uint64_t* const pl = threadIdx.x == 0 && quad < PLOG_QUADS ? dgetp(&bd->plog) : nullptr;
  uint64_t pl_start = 0;
  if (pl) {
    const uint32_t* h3 = lds + SLOT_BASE_W + 3 * STRIDE + NSLOTS * 12 + 2;
    pl_start = (uint64_t)h3[0] | (uint64_t)(h3[1] & 0xFFFFu) << 32;
  }
  const Slab s{unip(dgetp(&bd->state)), uni(dget(&bd->cap))};
  VmDev fold{};
  fold.code = a.fold_code;
  // (the fold's 17 phases per quad take the one-copy loop whatever OVH_VM_UNROLL says: it is a
  // second loop in this kernel)
  fold_unit<1>(quad, n, fold, cst, lds + SLOT_BASE_W, threadIdx.x % VM_FOLD_W, threadIdx.x < VM_FOLD_W,
            Slab{s.p + (size_t)S_F * 12 * s.cap, s.cap}, Slab{nullptr, 0},
            Slab{unip(dgetp(&bd->part0)), uni(dget(&bd->part_cap))}, codes);
  if (pl) {  // the quad's pool-log record, ahead of the release below
    pl[16 + 2 * quad] = pl_start | (uint64_t)simd_key() << 48 | (uint64_t)how << 60;
    pl[16 + 2 * quad + 1] = __builtin_amdgcn_s_memrealtime();
  }
  // the quad's codes, planes, partial and log record, then its done count (k_pool_wait)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (threadIdx.x == 0) {
    __hip_atomic_fetch_add(pq_done(a.q, slot), 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(a.q + PQ_INFL, ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // - 1
    __hip_atomic_fetch_add(pq_occ(a.q) + simd_key(), ~0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// The pool: each workgroup claims quads until the queue stays empty (pool_claim), then exits.
// LDS: constants + four slices of the larger of the vote / vote_t slot files; scratch: the
// workgroup's own spill area (4 x VOTE_NSCR entries), reused quad after quad. Two waves per SIMD
// are declared (the register budget that makes two pool workgroups share a SIMD).
__global__ __launch_bounds__(64, 2) void k_vm_pool(PoolArgs a) {
  __builtin_amdgcn_s_setprio(2);  // above the final streams' fold checks, below k_vm_final (3)
  extern __shared__ uint4 lds4[];
  // reserved CUs (OVH_FLAG_POOL_RESERVE): simd_key bits 2..8 = SE | SA | CU (wave-uniform)
  if (a.skip_cu && ((simd_key() >> 2) & 0x7Fu) < a.skip_cu) return;
  uint32_t* lds = reinterpret_cast<uint32_t*>(lds4);
  load_consts(lds, a.cst, VM_POOL_NCONST);  // the pool's own table (ovhip/pool_remap.hpp)
  const uint64_t t_in = __builtin_amdgcn_s_memrealtime();
  vote_stagger();
  uint32_t nquads = 0, why = 0;
#pragma unroll 1
  for (;; ++nquads) {
    uint32_t slot = 0, quad = 0, how = 0;
    if (!pool_claim(a.q, a.descs, &slot, &quad, &why, a.only, a.nsimd, &how)) break;
    slot = uni(slot);
    quad = uni(quad) | uni(how) << 28;  // the claim's flags ride in the top bits to the pool log
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // this batch's descriptor and inputs, fresh
    vote_quad(a, slot, quad, lds, uni(dget(&a.descs[slot].table)) != 0);
  }
  if (a.wlog && threadIdx.x == 0 && blockIdx.x < PLOG_WGS) {
    uint64_t* w = a.wlog + (size_t)blockIdx.x * PLOG_WG_WORDS;
    w[0] = t_in;
    w[1] = __builtin_amdgcn_s_memrealtime();
    w[2] = nquads;
    w[3] = why;
  }
}

// A batch's final stream waits here until the pool completed all `nq` quads of the slot's batch
// (one lane, bounded: after `ticks` of the 100 MHz clock it flags *err and returns, and the host
// reports OVH_ERR_DEVICE at the next synchronisation).
__global__ __launch_bounds__(64) void k_pool_wait(uint64_t* q, uint32_t slot, uint32_t nq, uint64_t ticks,
                                                  uint32_t* err) {
  if (threadIdx.x) return;
  const uint64_t t0 = wall_clock64();
  while (__hip_atomic_load(pq_done(q, slot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < nq) {
    if (wall_clock64() - t0 > ticks) {
      __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      return;
    }
    __builtin_amdgcn_s_sleep(32);
  }
}

// Staging of a pool batch (ovh_stream, before its publication): the signatures and keys (or
// table indices) into the slot's own buffer, so the caller's buffers are free once ovh_stream
// has passed this kernel (the pool reads the batch later, on its own schedule).
__global__ __launch_bounds__(WG) void k_pool_stage(uint32_t n, const uint8_t* __restrict__ sigs,
                                                   const uint8_t* __restrict__ pks, const int32_t* __restrict__ idx,
                                                   uint8_t* __restrict__ dst) {
  const size_t nb = (size_t)n * 96 + (pks ? (size_t)n * 48 : 0);
  uint8_t* di = dst + (size_t)n * 144;
  for (size_t k = (size_t)blockIdx.x * WG + threadIdx.x; k < nb + (idx ? (size_t)n * 4 : 0);
       k += (size_t)gridDim.x * WG) {
    if (k < (size_t)n * 96) dst[k] = sigs[k];
    else if (k < nb) dst[k] = pks[k - (size_t)n * 96];
    else di[k - nb] = reinterpret_cast<const uint8_t*>(idx)[k - nb];
  }
}
