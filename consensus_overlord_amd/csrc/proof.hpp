// The overlord 0.4 `Proof` RLP that Consensus::check_block decodes (consensus.rs:158), strict, on
// the host: rlp([height u64, round u64, block_hash bytes, rlp([signature bytes, address_bitmap
// bytes])]) -- the rules of consensus_overlord_amd/vote.py::decode_proof: a 4-item list whose 4th
// item is a 2-item list, canonical lengths (no long form below 56, no leading zero in a length, no
// 0x81 xx for a byte below 0x80), u64 without leading zeros and at most 8 bytes, nothing after
// the item. Host only; the views point into the caller's bytes.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace ovh {

struct ProofView {
  uint64_t height, round;
  const uint8_t *block_hash, *sig, *bitmap;
  size_t hash_len, sig_len, bitmap_len;
};

struct RlpItem {
  bool list;
  const uint8_t* p;  // payload
  size_t len;        // payload bytes
  size_t total;      // header + payload
};

// the big-endian length of a long form: ln bytes at b (n available), no leading zero
inline bool rlp_long_len(const uint8_t* b, size_t n, size_t ln, uint64_t* out) {
  if (ln == 0 || ln > 8 || n < ln || b[0] == 0) return false;
  uint64_t v = 0;
  for (size_t k = 0; k < ln; ++k) v = (v << 8) | b[k];
  *out = v;
  return true;
}

// the item that starts at b[0 .. n)
inline bool rlp_item(const uint8_t* b, size_t n, RlpItem* it) {
  if (n == 0) return false;
  const uint8_t h = b[0];
  size_t off = 1;
  uint64_t len;
  if (h < 0x80) {
    *it = RlpItem{false, b, 1, 1};
    return true;
  }
  if (h < 0xB8) {
    len = h - 0x80u;
    if (n - 1 < len || (len == 1 && b[1] < 0x80)) return false;
    it->list = false;
  } else if (h < 0xC0) {
    const size_t ln = h - 0xB7u;
    if (!rlp_long_len(b + 1, n - 1, ln, &len) || len < 56) return false;
    off = 1 + ln;
    it->list = false;
  } else if (h < 0xF8) {
    len = h - 0xC0u;
    it->list = true;
  } else {
    const size_t ln = h - 0xF7u;
    if (!rlp_long_len(b + 1, n - 1, ln, &len) || len < 56) return false;
    off = 1 + ln;
    it->list = true;
  }
  if (n - off < len) return false;
  it->p = b + off;
  it->len = (size_t)len;
  it->total = off + (size_t)len;
  return true;
}

inline bool rlp_u64(const RlpItem& it, uint64_t* out) {
  if (it.list || it.len > 8 || (it.len && it.p[0] == 0)) return false;
  uint64_t v = 0;
  for (size_t k = 0; k < it.len; ++k) v = (v << 8) | it.p[k];
  *out = v;
  return true;
}

// the items of a list payload: exactly `want` of them, the payload used up
inline bool rlp_items(const uint8_t* p, size_t n, RlpItem* items, size_t want) {
  for (size_t k = 0; k < want; ++k) {
    if (!rlp_item(p, n, &items[k])) return false;
    p += items[k].total;
    n -= items[k].total;
  }
  return n == 0;
}

// Proof::decode: false when the bytes are not a Proof
inline bool decode_proof(const uint8_t* b, size_t n, ProofView* pv) {
  RlpItem top, f[4], agg[2];
  if (!rlp_item(b, n, &top) || !top.list || top.total != n) return false;
  if (!rlp_items(top.p, top.len, f, 4)) return false;
  if (!rlp_u64(f[0], &pv->height) || !rlp_u64(f[1], &pv->round) || f[2].list || !f[3].list) return false;
  if (!rlp_items(f[3].p, f[3].len, agg, 2) || agg[0].list || agg[1].list) return false;
  pv->block_hash = f[2].p;
  pv->hash_len = f[2].len;
  pv->sig = agg[0].p;
  pv->sig_len = agg[0].len;
  pv->bitmap = agg[1].p;
  pv->bitmap_len = agg[1].len;
  return true;
}

}  // namespace ovh
