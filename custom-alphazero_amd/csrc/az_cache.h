// az_cache.h -- the transposition cache both engines share: the state word,
// the bucket scan and victim choice (pure, host and device) and the lock-free
// lookup and claim on a bucket (device).  Keys, payloads and the publish of a
// claimed entry are the engines' own (az_tree.hip, az_chess_mcts.hip).
#pragma once
#include "az_device.h"

namespace az {

// Transposition cache = the reference's plays_inferences (mcts/mcts.py:122-143,
// utils.py:38-39): board -> (probs, value), shared by every game on the
// device, cleared when the weights change.  Set-associative: a board hashes
// to one bucket of kCacheBucket slots (its state words are one 64-B segment,
// read in one round trip); inserts take the bucket's first reusable slot and
// are dropped when every slot is live.  (Round 2 probed linearly across the
// table: once stale entries had filled it, a miss walked max_probe = 32
// acquire loads one after another, and games/s fell the longer a run went.)
// The evaluator is deterministic per board, so hits never change a search.
//
// Eviction: least recently used, by generations (the reference's dict grows
// without bound until the next model; a fixed table keeps what it can).
// Every Ready entry is live -- a lookup accepts any of them, so the whole
// table serves as plays_inferences.  Each `gen_size` inserts start a new
// generation; a hit on an entry of an older generation moves it into the
// current one (one CAS per entry per generation), so an entry's generation
// is when it was last used.  An insert takes the bucket's first empty slot,
// else its least recently used entry at least kCacheEvictAge generations old
// (dropped when every entry is younger: a bucket of boards all in use).
//
// Overwrite safety: a reader finds an entry and reads its payload later.
// Every hit leaves the lookup stamped with the reader's generation G (an
// older entry's refresh CAS must win; when it loses, the slot may be being
// overwritten and the board counts as a miss).  While fewer than gen_size
// inserts fall inside a reader's window (cache_gen_size), at most one
// generation turn does, an insert sees the entry at most 1 generation old,
// and kCacheEvictAge = 2 keeps it.  Connect-N reads the payload one launch
// after the lookup (az_engine.hip bounds the window); chess copies it right
// after the probe, inside the launch (az_chess_mcts.hip).
//
// State word: [31:16] 16-bit fingerprint (hash bits 48-63, so most probes
// need no key read), [15:2] generation mod 2^14, [1:0] status.
enum : uint32_t { kCacheEmpty = 0, kCacheClaimed = 1, kCacheReady = 2 };
constexpr uint32_t kCacheGenMask = 0x3fff;
constexpr uint32_t kCacheGenDiv = 16;   // a generation = capacity / kCacheGenDiv inserts
constexpr uint32_t kCacheEvictAge = 2;  // an insert may overwrite entries this many generations old
constexpr int kCacheBucket = 16;        // slots per bucket (cache_log2 >= 4)
AZ_HD uint32_t cache_fp(uint64_t h) { return (uint32_t)(h >> 48); }
AZ_HD uint32_t cache_age(uint32_t st, uint32_t gen) { return (gen - (st >> 2)) & kCacheGenMask; }
AZ_HD uint32_t cache_word(uint32_t fp, uint32_t gen, uint32_t status) {
  return (fp << 16) | ((gen & kCacheGenMask) << 2) | status;
}
AZ_HD uint32_t cache_bucket(uint32_t mask, uint64_t h) {  // mask = cap - 1: the bucket's first slot
  return (uint32_t)h & mask & ~(uint32_t)(kCacheBucket - 1);
}

// The Ready slots of a bucket (its state words w) that carry fingerprint fp,
// as a bit mask.  Inserts fill a bucket in slot order: nothing past an empty
// slot.  (Constant indices here and below: w stays in VGPRs.)
AZ_HD uint32_t cache_candidates(const uint32_t (&w)[kCacheBucket], uint32_t fp) {
  uint32_t cm = 0;
  bool stop = false;
#pragma unroll
  for (int k = 0; k < kCacheBucket; ++k) {
    const uint32_t st = w[k];
    if (stop) continue;
    if (st == kCacheEmpty) stop = true;
    else if ((st & 3u) == kCacheReady && (st >> 16) == fp) cm |= 1u << k;
  }
  return cm;
}

// The slot an insert claims: the first empty slot not in `tried`, else (with
// eviction on: gen_size != 0) the oldest entry kCacheEvictAge+ generations
// old, the first of equal ages; slot < 0: none, every entry of the bucket is
// in use.  (gen_size as the cache holds it, not a bool: the compiler then
// splits the claim loop on it once, as it did the engines' own loops.)
struct CacheVictim {
  int slot;
  uint32_t word;  // the state word the claim's CAS expects there
  bool empty;
};
AZ_HD CacheVictim cache_victim(const uint32_t (&w)[kCacheBucket], uint32_t gen, uint32_t tried,
                               unsigned long long gen_size) {
  int pick = -1;
  uint32_t pst = 0, page = 0;
  bool pempty = false;
#pragma unroll
  for (int k = 0; k < kCacheBucket; ++k) {
    const uint32_t st = w[k];
    if (pempty || ((tried >> k) & 1u)) continue;
    if (st == kCacheEmpty) {
      pick = k, pst = st, pempty = true;
    } else if (gen_size) {
      const uint32_t age = cache_age(st, gen);
      if (age >= kCacheEvictAge && age > page) pick = k, pst = st, page = age;
    }
  }
  return {pick, pst, pempty};
}

// Inserts per generation for a table of cap entries whose readers hold an
// entry while at most reader_window_inserts inserts happen: cap / kCacheGenDiv,
// or the window + 1 when that is more; 0 = no eviction (the table only fills)
// when that exceeds cap / 4 (four generations per turnover keep the LRU order
// meaningful).
AZ_HD unsigned long long cache_gen_size(unsigned long long cap, unsigned long long reader_window_inserts) {
  const unsigned long long window = reader_window_inserts + 1;
  const unsigned long long g = cap / kCacheGenDiv > window ? cap / kCacheGenDiv : window;
  return g <= cap / 4 ? g : 0;
}

// The kernels' view of a cache: the key-independent part, and an engine's keys and payloads.
struct CacheCore {
  uint32_t* state = nullptr;          // [cap] state words
  unsigned long long* ctl = nullptr;  // device [0] generation, [1] inserts since the last clear,
                                      // [2] of them into empty slots (= entries held)
  uint32_t mask = 0;                  // cap - 1
  int enabled = 0;
  unsigned long long gen_size = 0;    // inserts per generation; 0 = no eviction
};
template <typename Key>
struct Cache : CacheCore {
  Key* keys = nullptr;   // [cap]
  float* pay = nullptr;  // [cap][the engine's payload floats]
};

// A bucket as one lookup or claim sees it: the generation and the bucket's
// state words, read at once with relaxed loads and scanned in registers.
struct CacheBucket {
  uint32_t gen, fp, base;
  uint32_t w[kCacheBucket];
};
__device__ __forceinline__ CacheBucket cache_load(const CacheCore& c, uint64_t h) {
  CacheBucket b;
  b.gen = (uint32_t)__hip_atomic_load(c.ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  b.fp = cache_fp(h);
  b.base = cache_bucket(c.mask, h);
#pragma unroll
  for (int k = 0; k < kCacheBucket; ++k)
    b.w[k] = __hip_atomic_load(c.state + b.base + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return b;
}

// The entry holding the bucket's key, or -1; same_key(i): entry i's key is
// the one looked up.  Entries may be published concurrently by an insert: the
// acquire fence pairs with its release, so a Ready entry's key and payload
// are complete (a Claimed one reads as absent).  The fingerprint matches,
// then ONE acquire -- a fence per candidate had the wave invalidating its
// CU's L1 (the tower tiles' weight fragments too) up to 16 times -- then the
// keys in slot order.
template <typename SameKey>
__device__ __forceinline__ int cache_lookup(const CacheCore& c, const CacheBucket& b, SameKey same_key) {
  int hit = -1;
  uint32_t hst = 0;
  uint32_t cm = cache_candidates(b.w, b.fp);
  if (cm) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    for (; cm; cm &= cm - 1) {
      const int k = __builtin_ctz(cm);
      if (same_key(b.base + k)) {
        hit = k;
#pragma unroll
        for (int kk = 0; kk < kCacheBucket; ++kk)
          if (kk == k) hst = b.w[kk];
        break;
      }
    }
  }
  bool use = hit >= 0;
  if (use && cache_age(hst, b.gen) != 0) {
    // a hit on an older generation moves the entry into the current one
    // (its last use: inserts evict the least recently used), at most one CAS
    // per entry per generation.  The CAS must win -- or find the entry
    // already moved by another reader and still this key -- else an insert
    // may be overwriting the slot and the key counts as a miss
    const uint32_t want = cache_word(b.fp, b.gen, kCacheReady);
    const uint32_t prev = atomicCAS(c.state + b.base + hit, hst, want);
    if (prev != hst) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      use = prev == want && same_key(b.base + hit);
    }
  }
  return use ? (int)(b.base + hit) : -1;
}

// Claims an entry of the bucket for an insert (its state word Claimed, to be
// published Ready by the caller); a lost race -- the slot claimed or
// refreshed meanwhile -- moves on to the next candidate.  idx < 0: dropped,
// the key is evaluated again when met.
struct CacheClaim {
  int idx;
  bool was_empty;
};
__device__ __forceinline__ CacheClaim cache_claim(const CacheCore& c, const CacheBucket& b) {
  int idx = -1;
  bool was_empty = false;
  uint32_t tried = 0;  // slots whose CAS lost
  for (int attempt = 0; attempt < kCacheBucket && idx < 0; ++attempt) {
    const CacheVictim v = cache_victim(b.w, b.gen, tried, c.gen_size);
    if (v.slot < 0) break;
    if (atomicCAS(c.state + b.base + v.slot, v.word, cache_word(b.fp, b.gen, kCacheClaimed)) == v.word) {
      idx = (int)(b.base + v.slot);
      was_empty = v.empty;
    } else {
      tried |= 1u << v.slot;
    }
  }
  return {idx, was_empty};
}
// n: the inserts since the clear, this one counted; every gen_size-th opens a new generation
__device__ __forceinline__ void cache_turn(const CacheCore& c, unsigned long long n) {
  if (c.gen_size && n % c.gen_size == 0) atomicAdd(c.ctl, 1ull);
}

}  // namespace az
