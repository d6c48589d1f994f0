// Host index of the signature-point cache: pure host code, no HIP
// (tests/host/sig_cache_harness.cpp compiles it with g++ and the sanitizers).
//
// The cache is a slab of `cap` entries in device memory, each the affine G2 point of one
// signature; this index maps the exact 96 signature bytes to the entry that holds their point.
// Entries are handed out in ring order (FIFO replacement), a batch's entries as one contiguous
// run so that one launch can fill them: a run that would pass the ring's end starts at entry 0
// instead, and the entries it skipped keep their keys until the ring comes round to them.
//
//   sc_claim     the next run of m entries; their old keys leave the index at once, before the
//                caller overwrites the points. SC_NONE when the cache is off or m > cap.
//   sc_register  enter a key for a claimed entry, once its fill was accepted by the device and
//                its vote's code 0 is known. A key that is still present moves to the new entry;
//                the old entry stays allocated but is no longer found.
//   sc_find      the entry registered under a key.
// An entry that was claimed and never registered has no key and is never found.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <string>
#include <unordered_map>
#include <vector>

#define SC_NONE 0xFFFFFFFFu
#define SC_KEY_BYTES 96

struct SigCache {
  uint32_t cap = 0;   // 0: off
  uint32_t next = 0;  // the ring's head: the first entry of the next claim
  std::vector<std::string> keys;  // per entry: its registered key, or empty
  std::unordered_map<std::string, uint32_t> index;
  uint64_t registered = 0;  // sc_register calls since the context was created (never reset)
};

// Empties the index and sets the capacity (0: off). The device slab is the caller's business.
static inline void sc_reset(SigCache& s, uint32_t cap) {
  s.cap = cap;
  s.next = 0;
  s.keys.assign(cap, std::string());
  s.index.clear();
}

static inline uint32_t sc_claim(SigCache& s, uint32_t m) {
  if (!s.cap || !m || m > s.cap) return SC_NONE;
  if (s.next + m > s.cap) s.next = 0;  // m <= cap: no overflow in the sum (cap <= 65536)
  const uint32_t e0 = s.next;
  for (uint32_t e = e0; e < e0 + m; ++e) {
    std::string& k = s.keys[e];
    if (k.empty()) continue;
    auto it = s.index.find(k);
    if (it != s.index.end() && it->second == e) s.index.erase(it);
    k.clear();
  }
  s.next = e0 + m == s.cap ? 0 : e0 + m;
  return e0;
}

static inline void sc_register(SigCache& s, uint32_t e, const uint8_t* key) {
  if (e >= s.cap) return;
  std::string k((const char*)key, SC_KEY_BYTES);
  auto it = s.index.find(k);
  if (it != s.index.end()) {
    if (it->second != e) s.keys[it->second].clear();
    it->second = e;
  } else {
    s.index.emplace(k, e);
  }
  std::string& old = s.keys[e];
  if (!old.empty() && old != k) {  // registered twice without a claim between: the later key holds
    auto io = s.index.find(old);
    if (io != s.index.end() && io->second == e) s.index.erase(io);
  }
  old = std::move(k);
  ++s.registered;
}

static inline bool sc_find(const SigCache& s, const uint8_t* key, uint32_t* e) {
  if (!s.cap) return false;
  auto it = s.index.find(std::string((const char*)key, SC_KEY_BYTES));
  if (it == s.index.end()) return false;
  *e = it->second;
  return true;
}

static inline size_t sc_entries(const SigCache& s) { return s.index.size(); }
