// Host build of the chess select kernel's wave-parallel Dirichlet draw
// (csrc/az_dirichlet_wave.h), test infrastructure for
// tests/test_chess_noise_cpu.py.  The kernel's lanes become a loop over 64
// lane indices; the functions called per lane are the kernel's own.
//   chess_noise_check draw SEED K ALPHA N -> N draws of Dirichlet(ALPHA * ones(K))
//       from MT19937(SEED), one per line in hex, one random_sample (serial
//       genrand) after every 7th draw on a line "u <hex>", and after the run
//       "next <hex> <stream position> <regenerations>"
//   chess_noise_check twist SEED REVERSE N -> the 624 state words after N
//       lane-parallel regenerations, each phase's lanes in forward (0) or
//       reverse (1) order
// Built with -ffp-contract=off like the tree kernels that include the header.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../custom-alphazero_amd/csrc/az_dirichlet_wave.h"

namespace {

struct Stream {
  uint32_t mt[az::kMtWords];
  uint32_t next[az::kMtWords];  // the staged next state (the kernel's LDS copy)
  int pos = az::kMtWords;
  long regenerations = 0;
};

void seed(Stream& s, uint32_t v) {  // init_genrand
  s.mt[0] = v;
  for (int i = 1; i < az::kMtWords; ++i) s.mt[i] = 1812433253u * (s.mt[i - 1] ^ (s.mt[i - 1] >> 30)) + (uint32_t)i;
  s.pos = az::kMtWords;
}

// the next state into s.next: every phase's lanes in forward or reverse order
void stage_next(Stream& s, bool reverse) {
  auto old = [&](int i) { return s.mt[i]; };
  auto nw = [&](int i) { return s.next[i]; };
  for (int i = 0; i < az::kMtWords; ++i) s.next[i] = 0xdeadbeefu;  // (a word read before its phase shows)
  for (int ph = 0; ph < 3; ++ph) {
    const int b = az::mt_phase_begin(ph), e = az::mt_phase_end(ph);
    for (int n = 0; n < e - b; ++n) {
      const int i = reverse ? e - 1 - n : b + n;
      s.next[i] = az::mt_twist_word(i, old, nw);
    }
  }
}

// genrand_int32, serial (numpy's own loop): the sampler's independent neighbour on the stream
uint32_t serial_next(Stream& s) {
  if (s.pos >= az::kMtWords) {
    for (int i = 0; i < az::kMtWords; ++i) {
      const uint32_t y = (s.mt[i] & 0x80000000u) | (s.mt[(i + 1) % az::kMtWords] & 0x7fffffffu);
      s.mt[i] = s.mt[(i + az::kMtShift) % az::kMtWords] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
    }
    s.pos = 0;
    ++s.regenerations;
  }
  return az::mt_temper(s.mt[s.pos++]);
}
double serial_uniform(Stream& s) {
  const uint32_t a = serial_next(s), b = serial_next(s);
  return az::legacy_double_of(a, b);
}

// dirichlet_wave of az_chess_mcts.hip, the wave's lanes one after another
bool draw(Stream& s, int k, double shape, double* d) {
  const double inv = 1.0 / shape;
  const int wpa = az::draw_words_per_attempt(shape);
  int have = 0;
  for (int round = 0; have < k; ++round) {
    if (round >= az::kDrawMaxRounds || s.pos > az::kMtWords) return false;
    const bool staged = az::draw_round_needs_next(s.pos, wpa);
    if (staged) stage_next(s, (round & 1) != 0);
    double x[az::kDrawLanes];
    uint64_t accepted = 0;
    for (int lane = 0; lane < az::kDrawLanes; ++lane) {
      uint32_t w[4] = {0u, 0u, 0u, 0u};
      for (int q = 0; q < wpa; ++q) {
        const int i = s.pos + lane * wpa + q;
        w[q] = az::mt_temper(i < az::kMtWords ? s.mt[i] : s.next[i - az::kMtWords]);
      }
      if (az::gamma_attempt(w, shape, inv, &x[lane])) accepted |= 1ull << lane;
    }
    for (int lane = 0; lane < az::kDrawLanes; ++lane) {
      const int j = az::draw_component(accepted, lane, have);
      if (((accepted >> lane) & 1ull) && j < k) d[j] = x[lane];
    }
    const int used = az::draw_round_used(accepted, have, k);
    bool commit;
    s.pos = az::draw_round_advance(s.pos, used, wpa, &commit);
    if (commit) {
      memcpy(s.mt, s.next, sizeof(s.mt));
      ++s.regenerations;
    }
    have += __builtin_popcountll(accepted);
  }
  double acc = 0.0;
  for (int j = 0; j < k; ++j) acc = acc + d[j];
  const double invacc = 1 / acc;
  for (int j = 0; j < k; ++j) d[j] = d[j] * invacc;
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 6 && !strcmp(argv[1], "draw")) {
    Stream s;
    seed(s, (uint32_t)strtoul(argv[2], nullptr, 10));
    const int k = atoi(argv[3]);
    const double alpha = strtod(argv[4], nullptr);
    const long n = atol(argv[5]);
    if (k < 1 || k > 256) return 2;
    double d[256];
    for (long i = 0; i < n; ++i) {
      if (!draw(s, k, alpha, d)) {
        fprintf(stderr, "round cap\n");
        return 3;
      }
      for (int j = 0; j < k; ++j) printf("%a%c", d[j], j + 1 < k ? ' ' : '\n');
      if (i % 7 == 6) printf("u %a\n", serial_uniform(s));
    }
    // the position first: the uniform after it moves the stream
    const int pos = s.pos;
    const long regen = s.regenerations;
    printf("next %a %d %ld\n", serial_uniform(s), pos, regen);
    return 0;
  }
  if (argc >= 5 && !strcmp(argv[1], "twist")) {
    Stream s;
    seed(s, (uint32_t)strtoul(argv[2], nullptr, 10));
    const bool reverse = atoi(argv[3]) != 0;
    const int n = atoi(argv[4]);
    for (int r = 0; r < n; ++r) {
      stage_next(s, reverse);
      memcpy(s.mt, s.next, sizeof(s.mt));
    }
    for (int i = 0; i < az::kMtWords; ++i) printf("%u\n", s.mt[i]);
    return 0;
  }
  fprintf(stderr, "usage\n");
  return 2;
}
