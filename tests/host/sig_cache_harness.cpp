// Stand-alone host program (g++, also with -fsanitize=address,undefined) over the host index of
// the signature-point cache (csrc/sig_cache.hpp) for tests/test_sig_cache_host.py: named cases on
// small rings, then a seeded random run of claims and registers against a plain model (the last
// registration of every entry, the last entry of every key). Prints "ok <checks>" and returns 0,
// or names the first property that fails. Test-only: never linked into the product.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <map>
#include <random>
#include <vector>

#include "../../consensus_overlord_amd/csrc/sig_cache.hpp"

namespace {
unsigned checks = 0;

struct Key {
  uint8_t b[SC_KEY_BYTES];
};
Key key(uint32_t v) {  // distinct in the first and in the last bytes
  Key k;
  memset(k.b, 0xA5, sizeof k.b);
  memcpy(k.b, &v, 4);
  memcpy(k.b + SC_KEY_BYTES - 4, &v, 4);
  return k;
}
bool has(const SigCache& s, uint32_t v, uint32_t* e = nullptr) {
  uint32_t x = SC_NONE;
  const bool f = sc_find(s, key(v).b, &x);
  if (e) *e = x;
  return f;
}
#define REQUIRE(cond, what)            \
  do {                                 \
    ++checks;                          \
    if (!(cond)) {                     \
      printf("FAIL %s (line %d)\n", what, __LINE__); \
      return 1;                        \
    }                                  \
  } while (0)

int named_cases() {
  uint32_t e;
  {  // claim, register, find; a claimed entry that was never registered is not found
    SigCache s;
    sc_reset(s, 8);
    REQUIRE(!has(s, 1), "empty cache finds nothing");
    const uint32_t e0 = sc_claim(s, 3);
    REQUIRE(e0 == 0 && s.next == 3, "first claim starts at 0");
    REQUIRE(!has(s, 1), "claimed, unregistered: not found");
    sc_register(s, e0, key(1).b);
    sc_register(s, e0 + 2, key(3).b);  // the vote of e0 + 1 was invalid
    REQUIRE(has(s, 1, &e) && e == 0, "find key 1");
    REQUIRE(has(s, 3, &e) && e == 2, "find key 3");
    REQUIRE(!has(s, 2), "unregistered entry of a run");
    REQUIRE(sc_entries(s) == 2 && s.registered == 2, "counts");
    // a key that differs only in its last byte is another key
    Key k = key(1);
    k.b[SC_KEY_BYTES - 1] ^= 1;
    REQUIRE(!sc_find(s, k.b, &e), "exact 96 bytes");
  }
  {  // eviction order: FIFO by entry
    SigCache s;
    sc_reset(s, 4);
    for (uint32_t v = 0; v < 4; ++v) sc_register(s, sc_claim(s, 1), key(v).b);
    REQUIRE(sc_entries(s) == 4, "ring full");
    sc_register(s, sc_claim(s, 1), key(4).b);
    REQUIRE(!has(s, 0) && has(s, 1) && has(s, 2) && has(s, 3) && has(s, 4, &e) && e == 0, "oldest evicted first");
    const uint32_t e0 = sc_claim(s, 2);  // evicts 1 and 2 at the claim, before any register
    REQUIRE(e0 == 1 && !has(s, 1) && !has(s, 2) && has(s, 3) && has(s, 4), "claim drops the old keys at once");
    REQUIRE(sc_entries(s) == 2, "entries after a claim");
  }
  {  // re-registering a key that is still present: it moves, and the old entry's turn does not evict it
    SigCache s;
    sc_reset(s, 4);
    sc_register(s, sc_claim(s, 1), key(7).b);  // entry 0
    sc_register(s, sc_claim(s, 1), key(8).b);  // entry 1
    sc_register(s, sc_claim(s, 1), key(7).b);  // entry 2: key 7 again
    REQUIRE(has(s, 7, &e) && e == 2 && sc_entries(s) == 2, "key moved to the new entry");
    REQUIRE(sc_claim(s, 1) == 3, "entry 3");
    REQUIRE(sc_claim(s, 1) == 0, "entry 0 again");  // held key 7 once: must not drop the moved key
    REQUIRE(has(s, 7, &e) && e == 2, "stale entry's claim leaves the moved key");
    REQUIRE(sc_claim(s, 1) == 1 && !has(s, 8), "entry 1 evicts key 8");
    REQUIRE(sc_claim(s, 1) == 2 && !has(s, 7), "entry 2 evicts key 7");
  }
  {  // capacity 1
    SigCache s;
    sc_reset(s, 1);
    REQUIRE(sc_claim(s, 2) == SC_NONE, "a run longer than the ring");
    sc_register(s, sc_claim(s, 1), key(1).b);
    REQUIRE(has(s, 1, &e) && e == 0, "capacity 1 holds one");
    sc_register(s, sc_claim(s, 1), key(2).b);
    REQUIRE(!has(s, 1) && has(s, 2, &e) && e == 0 && sc_entries(s) == 1, "capacity 1 replaces");
  }
  {  // capacity 2
    SigCache s;
    sc_reset(s, 2);
    REQUIRE(sc_claim(s, 2) == 0 && s.next == 0, "a run of the whole ring");
    sc_register(s, 0, key(1).b);
    sc_register(s, 1, key(2).b);
    REQUIRE(sc_claim(s, 1) == 0 && !has(s, 1) && has(s, 2), "capacity 2, first out");
    REQUIRE(sc_claim(s, 2) == 0 && !has(s, 2), "a whole-ring run from the middle starts at 0");
  }
  {  // wrap of a contiguous claim past the ring's end
    SigCache s;
    sc_reset(s, 8);
    for (uint32_t v = 0; v < 6; ++v) sc_register(s, sc_claim(s, 1), key(v).b);  // entries 0..5, next = 6
    const uint32_t e0 = sc_claim(s, 3);  // 6 + 3 > 8: the run is 0..2
    REQUIRE(e0 == 0 && s.next == 3, "wrapped run starts at 0");
    REQUIRE(!has(s, 0) && !has(s, 1) && !has(s, 2) && has(s, 3) && has(s, 4) && has(s, 5), "wrapped run evicts 0..2 only");
    for (uint32_t j = 0; j < 3; ++j) sc_register(s, e0 + j, key(10 + j).b);
    REQUIRE(sc_claim(s, 5) == 3 && s.next == 0, "a run that ends at the ring's end");
    REQUIRE(!has(s, 3) && !has(s, 5) && has(s, 10) && has(s, 12), "entries 3..7 claimed");
  }
  {  // off, and emptied by a reset
    SigCache s;
    REQUIRE(sc_claim(s, 1) == SC_NONE && !has(s, 1), "capacity 0 is off");
    sc_reset(s, 4);
    sc_register(s, sc_claim(s, 1), key(1).b);
    sc_reset(s, 0);
    REQUIRE(!has(s, 1) && sc_entries(s) == 0 && s.registered == 1, "reset empties; the counter stays");
    sc_register(s, 0, key(1).b);  // out of range: ignored
    REQUIRE(!has(s, 1), "register past the capacity is ignored");
  }
  return 0;
}

// Random runs against a model: where[key] = the entry of its last registration, unless that entry
// was claimed since.
int random_run(uint32_t cap, std::mt19937_64& rng) {
  SigCache s;
  sc_reset(s, cap);
  std::map<uint32_t, uint32_t> where;       // key -> entry
  std::vector<int64_t> holds(cap, -1);      // entry -> key
  const uint32_t nkeys = 3 * cap + 2;
  for (int step = 0; step < 400; ++step) {
    const uint32_t m = 1 + (uint32_t)(rng() % (cap < 5 ? cap : 5));
    const uint32_t e0 = sc_claim(s, m);
    REQUIRE(e0 != SC_NONE && e0 + m <= cap, "run inside the ring");
    for (uint32_t e = e0; e < e0 + m; ++e) {
      if (holds[e] >= 0 && where.count((uint32_t)holds[e]) && where[(uint32_t)holds[e]] == e) where.erase((uint32_t)holds[e]);
      holds[e] = -1;
    }
    for (uint32_t j = 0; j < m; ++j) {
      if (rng() % 4 == 0) continue;  // an invalid vote: stays unregistered
      const uint32_t v = (uint32_t)(rng() % nkeys);
      sc_register(s, e0 + j, key(v).b);
      if (where.count(v)) holds[where[v]] = -1;
      where[v] = e0 + j;
      holds[e0 + j] = v;
    }
    REQUIRE(sc_entries(s) == where.size(), "entry count equals the model's");
    for (uint32_t v = 0; v < nkeys; ++v) {
      uint32_t e;
      const bool f = has(s, v, &e);
      if (f != (where.count(v) != 0) || (f && e != where[v])) {
        printf("FAIL model mismatch (cap %u, step %d, key %u)\n", cap, step, v);
        return 1;
      }
    }
    ++checks;
  }
  return 0;
}
}  // namespace

int main() {
  if (named_cases()) return 1;
  std::mt19937_64 rng(0x51C);
  for (uint32_t cap : {1u, 2u, 3u, 8u, 67u})
    if (random_run(cap, rng)) return 1;
  printf("ok %u\n", checks);
  return 0;
}
