// az_dirichlet_wave.h -- numpy's legacy RandomState.dirichlet(alpha * ones(k))
// drawn by 64 lanes at once, bit for bit the serial draw of az_random.h.
//
// legacy_standard_gamma(shape < 1) consumes two legacy_doubles (U, V) = four
// MT19937 words in every turn of its rejection loop, whichever branch the
// turn takes and whether it accepts.  So ATTEMPT t after stream position p is
// a pure function of words p + 4t .. p + 4t + 3, component j of the vector is
// the j-th accepted attempt, and the draw leaves the stream 4 (t_k + 1) words
// further, t_k the attempt that gave component k - 1.  shape == 1 is the
// exponential: two words per attempt, every attempt accepted.  A round is 64
// consecutive attempts, one per lane; a ballot of the accepts and a prefix
// popcount number the components in attempt order.  The sum runs over the
// components left to right, as mtrand's loop does.
//
// A round is speculative: it reads 64 attempts' words and may use fewer (the
// last round of a draw).  When its words run past word 623 of the MT19937
// state, the next state is computed beside the current one (the lane-parallel
// twist below) and replaces it only if the words the round USED run past 623;
// otherwise the next draw still needs the old words.
//
// Everything here is AZ_HD: the chess select kernel calls it per lane, and
// tests/native/chess_noise_check.cpp drives the same functions from a host
// loop over the 64 lanes.
//
// This file owns the schedule only: which lane makes which attempt, which
// words a round used, and the three-phase order of the regeneration.  The
// attempt itself (gamma_attempt, draw_words_per_attempt) is az_random.h's;
// the MT19937 constants, the per-word regeneration formula (mt_regen_word),
// mt_temper and legacy_double_of are az_mt.h's.
#pragma once
#include <stdint.h>

#include "az_random.h"

namespace az {

// the state's size under the name tests/native/chess_noise_check.cpp sizes its
// host streams with (that check is kept as it was); csrc/ itself uses kMtN
constexpr int kMtWords = kMtN;
constexpr int kDrawLanes = 64;
// a draw's round cap: k <= 256 components need 4 rounds of all-accepted
// attempts; the acceptance rate of a valid shape is above 85 %, so 64 rounds
// (4096 attempts) are out of reach and mean a defect, not bad luck
constexpr int kDrawMaxRounds = 64;

// ------------------------------------------------- lane-parallel twist
// genrand's regeneration, new[i] = mt_regen_word(old[i], next, far) with
//   next = old[i + 1] (new[0] for i = 623)
//   far  = old[i + 397] for i < 227, else new[i - 227]
// in three phases whose words depend only on old words and on new words of
// EARLIER phases, so the lanes of a phase may run in any order:
//   phase 0  i in [0, 227)    old words only
//   phase 1  i in [227, 454)  new words [0, 227)            (phase 0)
//   phase 2  i in [454, 624)  new words [227, 397) and, for i = 623, new[0]
AZ_HD int mt_phase_begin(int phase) { return phase * kMtTail; }
AZ_HD int mt_phase_end(int phase) { return phase == 2 ? kMtN : (phase + 1) * kMtTail; }
// word i of the next state; old(i) / nw(i) read the current / the next state
template <typename Old, typename New>
AZ_HD uint32_t mt_twist_word(int i, Old&& old, New&& nw) {
  const uint32_t cur = old(i);
  const uint32_t next = i == kMtN - 1 ? nw(0) : old(i + 1);
  const uint32_t far = i < kMtTail ? old(i + kMtShift) : nw(i - kMtTail);
  return mt_regen_word(cur, next, far);
}

// ------------------------------------------------------ round accounting
// accepted: the round's ballot (bit l = lane l's attempt accepted); have:
// components before this round; k: components wanted.
// the component lane `lane`'s accepted attempt gives (>= k: not needed)
AZ_HD int draw_component(uint64_t accepted, int lane, int have) {
  return have + __builtin_popcountll(accepted & ((1ull << lane) - 1ull));
}
// attempts of the round the draw consumes: all 64 while components are still
// missing after it, else up to and including the attempt of component k - 1
AZ_HD int draw_round_used(uint64_t accepted, int have, int k) {
  if (have + __builtin_popcountll(accepted) < k) return kDrawLanes;
  for (int n = k - have - 1; n > 0; --n) accepted &= accepted - 1;
  return __builtin_ctzll(accepted) + 1;
}
// the stream position after a round from position pos (0..624) that used
// `used` attempts of wpa words: *commit = the next state replaces the current
// one (the used words ran past word 623)
AZ_HD int draw_round_advance(int pos, int used, int wpa, bool* commit) {
  const int np = pos + used * wpa;
  *commit = np > kMtN;
  return *commit ? np - kMtN : np;
}
// a round from pos reads words [pos, pos + 64 wpa): does it need the next state
AZ_HD bool draw_round_needs_next(int pos, int wpa) { return pos + kDrawLanes * wpa > kMtN; }

}  // namespace az
