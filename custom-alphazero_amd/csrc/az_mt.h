// az_mt.h -- the one MT19937 stream of both engines: legacy np.random.seed /
// random_sample (init_genrand, genrand_int32, the 53-bit double from two
// outputs), one generator per game slot.  Everything is host + device, so the
// stream is pinned against np.random.RandomState without a GPU
// (tests/native/mt_check.cpp, tests/test_mt_cpu.py).
//
// A slot's state is stored word-major, [625][slots]: word w of slot s at
// mt[w * slots + s], the index (0..624) as word 624 -- a wave touching the
// same word of 64 generators reads one line.  MtStream is one slot's view of
// that array; the engines build it from their own structs,
// {t.mt + s, (size_t)t.mt_stride}.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "az_device.h"

namespace az {

constexpr int kMtN = 624;
constexpr int kMtShift = 397;
constexpr int kMtTail = kMtN - kMtShift;  // 227

AZ_HD uint32_t mt_temper(uint32_t y) {
  y ^= y >> 11;
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= y >> 18;
  return y;
}

// genrand's regeneration of one word: new[i] from cur = old[i],
// next = word i + 1 and far = word i + 397 (both mod 624, as they stand when
// the serial loop reaches i).  Every schedule of a whole-state twist -- the
// batched one below, az_dirichlet_wave.h's lane-parallel phases -- calls this.
AZ_HD uint32_t mt_regen_word(uint32_t cur, uint32_t next, uint32_t far) {
  const uint32_t y = (cur & 0x80000000u) | (next & 0x7fffffffu);
  return far ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

// numpy legacy_double / random_sample of two tempered words:
// ((w0 >> 5) * 2^26 + (w1 >> 6)) / 2^53
AZ_HD double legacy_double_of(uint32_t w0, uint32_t w1) {
  const uint32_t a = w0 >> 5;
  const uint32_t b = w1 >> 6;
  return ((double)a * 67108864.0 + (double)b) / 9007199254740992.0;
}

struct MtStream {  // one slot's state: word w at m[w * stride], the index at m[kMtN * stride]
  uint32_t* m;
  size_t stride;
};

AZ_HD void mt_seed(MtStream r, uint32_t seed) {  // init_genrand
  uint32_t prev = seed;
  r.m[0] = seed;
  for (int i = 1; i < kMtN; ++i) {
    prev = 1812433253u * (prev ^ (prev >> 30)) + (uint32_t)i;
    r.m[(size_t)i * r.stride] = prev;
  }
  r.m[(size_t)kMtN * r.stride] = kMtN;  // force a twist on first use
}

// One twist of the state in place, the serial loop's arithmetic in its order:
// word i takes words i, i+1 as they were and word i+397 (as it was below
// i = 227, already new from there on; word 0 is new when i = 623 reads it as
// i+1).  A batch of kTwistB words loads every operand before its first store
// -- none of a batch's loads reads a word that batch writes before that
// word's own update, and the words from earlier batches are stored ahead of
// them in program order -- so a twist is 39 memory round trips instead of 624
// dependent load-store chains (a Connect-N game's reset twists once:
// slot_reset).  Batches of 48 words (13 round trips) cost 3% of games/s
// (profiles/r6/ab_exp5.txt).
AZ_HD void mt_twist(MtStream r) {
  constexpr int kTwistB = 16;
  static_assert(kMtN % kTwistB == 0 && kMtTail >= kTwistB, "batches never read their own stores");
  uint32_t* m = r.m;
  const size_t slots = r.stride;
  uint32_t cur = m[0];
  for (int i0 = 0; i0 < kMtN; i0 += kTwistB) {
    uint32_t nx[kTwistB], far[kTwistB];
#pragma unroll
    for (int k = 0; k < kTwistB; ++k) {
      const int i = i0 + k;
      nx[k] = m[(size_t)(i + 1 < kMtN ? i + 1 : 0) * slots];
      far[k] = m[(size_t)(i + kMtShift < kMtN ? i + kMtShift : i - kMtTail) * slots];
    }
#pragma unroll
    for (int k = 0; k < kTwistB; ++k) {
      m[(size_t)(i0 + k) * slots] = mt_regen_word(cur, nx[k], far[k]);
      cur = nx[k];
    }
  }
}

AZ_HD uint32_t mt_next(MtStream r) {  // genrand_int32
  uint32_t pos = r.m[(size_t)kMtN * r.stride];
  if (pos >= (uint32_t)kMtN) {
    mt_twist(r);
    pos = 0;
  }
  const uint32_t y = r.m[(size_t)pos * r.stride];
  r.m[(size_t)kMtN * r.stride] = pos + 1;
  return mt_temper(y);
}

AZ_HD double mt_uniform(MtStream r) {  // legacy random_sample
  const uint32_t w0 = mt_next(r);
  const uint32_t w1 = mt_next(r);
  return legacy_double_of(w0, w1);
}

// The state n mt_next calls would leave, the words skipped, not drawn: a twist
// whenever the index runs out, then the index (no 2 dependent round trips per
// word).
AZ_HD void mt_skip(MtStream r, int n) {
  if (n <= 0) return;
  uint32_t pos = r.m[(size_t)kMtN * r.stride];
  while (n > 0) {
    if (pos >= (uint32_t)kMtN) {
      mt_twist(r);
      pos = 0;
    }
    const int k = n < kMtN - (int)pos ? n : kMtN - (int)pos;
    pos += (uint32_t)k;
    n -= k;
  }
  r.m[(size_t)kMtN * r.stride] = pos;
}

}  // namespace az
