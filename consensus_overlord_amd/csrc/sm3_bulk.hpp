// SM3 of many variable-length messages (Crypto::hash in bulk, src/util.rs:83-87): the core behind
// ovh_sm3_batch* and the proposal hashes of ovh_check_blocks. One lane per message -- SM3 is a
// serial chain inside a message -- 64 messages per wave; the host forms order the messages by
// block count so the lanes of a wave run similar lengths.
//
// Compression: a rolling 16-word schedule and 64 unrolled rounds on compile-time indices, so the
// state stays in registers (no scratch; sm3.hpp's w[68] / w1[64] form is kept for the <= 88-byte
// vote digests). Loading: a message may start at any byte address; the reader takes the aligned
// 32-bit words that hold a byte of the message -- never a word that holds none, so it stays
// inside the caller's buffer up to the words of the first and last byte -- and funnels two
// neighbours into a message word (v_alignbyte_b32 on the device). A block that lies inside the
// message with its 17 words loads them unguarded (adjacent dword loads the compiler may merge);
// the last full block of some messages and the one or two padded blocks take the guarded reader,
// which also places 0x80, the zeros and the bit length. Both readers feed one copy of the rounds.
//
// Host/device portable (the SM3_HD pattern of sm3.hpp): tests/host/sm3_bulk_harness.cpp runs the
// same core under g++. Little-endian hosts only, as the device.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#ifndef SM3_HD
#if defined(__HIPCC__)
#define SM3_HD __host__ __device__ inline
#else
#define SM3_HD inline
#endif
#endif
#define SM3B_INL SM3_HD __attribute__((always_inline))

namespace ovh {

// 0 < n < 32
SM3B_INL uint32_t sm3b_rotl(uint32_t x, uint32_t n) {
#if defined(__clang__)
  return __builtin_rotateleft32(x, n);
#else
  return (x << n) | (x >> (32 - n));
#endif
}

// the 32 bits at byte offset a (0..3) of the little-endian pair {hi, lo}
SM3B_INL uint32_t sm3b_funnel(uint32_t hi, uint32_t lo, uint32_t a) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbyte(hi, lo, a);
#else
  return a ? (lo >> (8 * a)) | (hi << (32 - 8 * a)) : lo;
#endif
}

// one aligned 32-bit word (p is 4-byte aligned)
SM3B_INL uint32_t sm3b_ldw(const uint8_t* p) {
  uint32_t x;
  __builtin_memcpy(&x, __builtin_assume_aligned(p, 4), 4);
  return x;
}

// CF of GB/T 32905 on the block whose 16 big-endian words are in w (overwritten: the window rolls)
SM3B_INL void sm3b_compress(uint32_t v[8], uint32_t w[16]) {
  uint32_t a = v[0], b = v[1], c = v[2], d = v[3], e = v[4], f = v[5], g = v[6], h = v[7];
#pragma unroll
  for (int j = 0; j < 64; ++j) {
    if (j >= 12) {  // W[j + 4] replaces W[j - 12], which no later round or expansion reads
      const int t = j + 4;
      uint32_t x = w[(t - 16) & 15] ^ w[(t - 9) & 15] ^ sm3b_rotl(w[(t - 3) & 15], 15);
      x = x ^ sm3b_rotl(x, 15) ^ sm3b_rotl(x, 23);
      w[t & 15] = x ^ sm3b_rotl(w[(t - 13) & 15], 7) ^ w[(t - 6) & 15];
    }
    const uint32_t wj = w[j & 15], wj4 = w[(j + 4) & 15];
    const uint32_t t0 = j < 16 ? 0x79cc4519u : 0x7a879d8au;
    const uint32_t tj = (j & 31) ? (t0 << (j & 31)) | (t0 >> (32 - (j & 31))) : t0;
    const uint32_t a12 = sm3b_rotl(a, 12);
    const uint32_t ss1 = sm3b_rotl(a12 + e + tj, 7);
    const uint32_t ss2 = ss1 ^ a12;
    const uint32_t ff = j < 16 ? (a ^ b ^ c) : ((a & b) | (a & c) | (b & c));
    const uint32_t gg = j < 16 ? (e ^ f ^ g) : ((e & f) | (~e & g));
    const uint32_t tt1 = ff + d + ss2 + (wj ^ wj4);
    const uint32_t tt2 = gg + h + ss1 + wj;
    d = c;
    c = sm3b_rotl(b, 9);
    b = a;
    a = tt1;
    h = g;
    g = sm3b_rotl(f, 19);
    f = e;
    e = tt2 ^ sm3b_rotl(tt2, 9) ^ sm3b_rotl(tt2, 17);
  }
  v[0] ^= a;
  v[1] ^= b;
  v[2] ^= c;
  v[3] ^= d;
  v[4] ^= e;
  v[5] ^= f;
  v[6] ^= g;
  v[7] ^= h;
}

// Message word at byte position pos of a message of len bytes, from the raw big-endian word read
// there: the message's bytes, then 0x80, then zeros (the bit length is ORed in by the caller).
SM3B_INL uint32_t sm3b_pad(uint32_t raw, uint64_t pos, uint64_t len) {
  if (pos + 4 <= len) return raw;
  if (pos > len) return 0;
  const uint32_t k = (uint32_t)(len - pos);  // 0..3 message bytes in this word
  const uint32_t keep = k ? ~(0xffffffffu >> (8 * k)) : 0u;
  return (raw & keep) | (0x80000000u >> (8 * k));
}

// v = the SM3 state after the padded message msg[0 .. len); msg may be unaligned. Reads only
// aligned 32-bit words that hold at least one byte of the message.
SM3B_INL void sm3b_hash(const uint8_t* msg, uint64_t len, uint32_t v[8]) {
  v[0] = 0x7380166fu;
  v[1] = 0x4914b2b9u;
  v[2] = 0x172442d7u;
  v[3] = 0xda8a0600u;
  v[4] = 0xa96f30bcu;
  v[5] = 0x163138aau;
  v[6] = 0xe38dee4du;
  v[7] = 0xb0fb0e4eu;
  const uint32_t a = (uint32_t)((uintptr_t)msg & 3);
  const uint8_t* wp = msg - a;                            // the aligned word of the first byte
  const uint64_t nw = len ? (a + len + 3) >> 2 : 0;       // aligned words that hold a message byte
  const uint64_t nblk = (len >> 6) + 1 + ((len & 63) >= 56);  // blocks of the padded message
  // blocks that are whole message bytes and whose 17 aligned words all hold some: unguarded loads
  uint64_t nfast = len >> 6;
  const uint64_t cap = nw ? (nw - 1) >> 4 : 0;
  if (cap < nfast) nfast = cap;
  uint32_t c0 = nw ? sm3b_ldw(wp) : 0;  // word 16 b, carried from block to block
  for (uint64_t b = 0; b < nblk; ++b) {
    uint32_t w[16];
    const uint8_t* q = wp + (b << 6);
    if (b < nfast) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const uint32_t x = sm3b_ldw(q + 4 * (j + 1));
        w[j] = __builtin_bswap32(sm3b_funnel(x, c0, a));
        c0 = x;
      }
    } else {
      const uint64_t g0 = b << 4;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const uint64_t g = g0 + j;
        const uint32_t x = g + 1 < nw ? sm3b_ldw(q + 4 * (j + 1)) : 0;
        w[j] = sm3b_pad(__builtin_bswap32(sm3b_funnel(x, c0, a)), g << 2, len);
        c0 = x;
      }
      if (b == nblk - 1) {  // the 64-bit bit length closes the last block
        w[14] |= (uint32_t)(len >> 29);
        w[15] |= (uint32_t)(len << 3);
      }
    }
    sm3b_compress(v, w);
  }
}

// digest bytes of a state
SM3B_INL void sm3b_store(const uint32_t v[8], uint8_t out[32]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    out[4 * i] = (uint8_t)(v[i] >> 24);
    out[4 * i + 1] = (uint8_t)(v[i] >> 16);
    out[4 * i + 2] = (uint8_t)(v[i] >> 8);
    out[4 * i + 3] = (uint8_t)v[i];
  }
}

// Message i of a batch: data[off[i] .. off[i + 1]). An end below its start (the device form
// cannot reject it on the host) gets the all-zero digest, which no SM3 output equals in
// practice, and nothing is read -- the precedent of k_vote_digest's over-long hashes.
SM3B_INL void sm3b_batch_item(const uint8_t* data, const uint64_t* off, size_t i, uint32_t v[8]) {
  const uint64_t s = off[i], e = off[i + 1];
  if (e < s) {
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = 0;
    return;
  }
  sm3b_hash(data + s, e - s, v);
}

#if defined(__HIPCC__)
// Lane t hashes message order[t] (order null: message t) and writes its 32 digest bytes.
__global__ __launch_bounds__(64) void k_sm3_bulk(uint32_t n, const uint8_t* __restrict__ data,
                                                 const uint64_t* __restrict__ off,
                                                 const uint32_t* __restrict__ order, uint8_t* __restrict__ out) {
  const uint32_t t = blockIdx.x * 64 + threadIdx.x;
  if (t >= n) return;
  const uint32_t i = order ? order[t] : t;
  uint32_t v[8];
  sm3b_batch_item(data, off, i, v);
  uint8_t* o = out + (size_t)i * 32;
  if (((uintptr_t)out & 3) == 0) {  // wave-uniform
    uint32_t* o32 = (uint32_t*)o;
#pragma unroll
    for (int k = 0; k < 8; ++k) o32[k] = __builtin_bswap32(v[k]);
  } else {
    sm3b_store(v, o);
  }
}
#endif

}  // namespace ovh
