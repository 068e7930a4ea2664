// book_check.cpp -- the opening book's per-position functions (csrc/az_book.h)
// on the host, without a GPU:
//
//  * decode_key then cur + mask is the identity, mirror_key is an involution
//    and commutes with play, canonical_key agrees for a position and its
//    mirror: on every reachable position of 4x4 (W even) and on the first
//    levels of 5-wide-4-high (W odd, a middle column), 4-wide-5-high, 5x5 n=3;
//  * a book built here from those functions (expand, std::sort + unique, scores
//    of the deepest level, retrograde) has the canonical level counts, and on
//    4x4 at full depth every score of every level equals a plain memoised
//    negamax written in this file on cell arrays (it shares no function with
//    csrc/); a missing or unscored child is flagged, never scored;
//  * the file writer and reader round-trip, and each refusal of the reader fires.
//
// usage: book_check [TMPDIR]      prints "ok" or the first failure.  Built by
// tests/test_solver_book_cpu.py with -fsanitize=address,undefined.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../custom-alphazero_amd/csrc/az_book.h"

namespace sv = az::solver;
namespace bk = az::solver::book;

#define REQUIRE(cond, ...)                                       \
  do {                                                           \
    if (!(cond)) {                                               \
      fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
      fprintf(stderr, __VA_ARGS__);                              \
      fprintf(stderr, "\n");                                     \
      exit(1);                                                   \
    }                                                            \
  } while (0)

// ------------------------------------------------------------ the reference
// Cells [H][W], row 0 the top row, +1 the side to move.
struct Ref {
  int H, W, N;
  std::unordered_map<std::string, int> memo;

  int at(const std::string& b, int r, int c) const {
    return (r < 0 || r >= H || c < 0 || c >= W) ? 0 : (int)(int8_t)b[r * W + c];
  }
  bool makes_line(const std::string& b, int r, int c) const {
    static const int dr[4] = {0, 1, 1, 1}, dc[4] = {1, 0, 1, -1};
    const int who = at(b, r, c);
    for (int d = 0; d < 4; ++d) {
      int run = 1;
      for (int s = 1; at(b, r + s * dr[d], c + s * dc[d]) == who; ++s) ++run;
      for (int s = 1; at(b, r - s * dr[d], c - s * dc[d]) == who; ++s) ++run;
      if (run >= N) return true;
    }
    return false;
  }
  int value(const std::string& b) {
    auto it = memo.find(b);
    if (it != memo.end()) return it->second;
    int stones = 0;
    for (char v : b) stones += v != 0;
    int best = -1000;
    for (int c = 0; c < W; ++c) {
      int r = H - 1;
      while (r >= 0 && b[r * W + c] != 0) --r;
      if (r < 0) continue;
      std::string nb = b;
      nb[r * W + c] = 1;
      int v;
      if (makes_line(nb, r, c)) {
        v = (H * W + 2 - (stones + 1)) / 2;
      } else if (stones + 1 == H * W) {
        v = 0;
      } else {
        for (char& x : nb) x = (char)-(int8_t)x;
        v = -value(nb);
      }
      best = std::max(best, v);
    }
    memo.emplace(b, best);
    return best;
  }
};

// (cur, mask) as the reference's cells, written out here bit by bit
static std::string cells_of(const sv::Geo& g, uint64_t cur, uint64_t mask) {
  std::string b((size_t)g.HW, 0);
  for (int c = 0; c < g.W; ++c)
    for (int r = 0; r < g.H; ++r) {
      const uint64_t bit = 1ull << (c * g.H1 + r);
      if (mask & bit) b[(size_t)((g.H - 1 - r) * g.W + c)] = (cur & bit) ? 1 : (char)-1;
    }
  return b;
}

static uint64_t mirror_bits(const sv::Geo& g, uint64_t x) {  // a bitboard, column by column
  uint64_t m = 0;
  for (int c = 0; c < g.W; ++c) m |= (x >> (c * g.H1) & ((1ull << g.H1) - 1)) << ((g.W - 1 - c) * g.H1);
  return m;
}

// ------------------------------------------------------------ per-position identities
static void check_position(const sv::Geo& g, uint64_t cur, uint64_t mask) {
  const uint64_t key = cur + mask;
  uint64_t c2, m2;
  bk::decode_key(g, key, &c2, &m2);
  REQUIRE(c2 == cur && m2 == mask, "decode_key(%llx) gave %llx %llx, not %llx %llx", (unsigned long long)key,
          (unsigned long long)c2, (unsigned long long)m2, (unsigned long long)cur, (unsigned long long)mask);
  const uint64_t mk = bk::mirror_key(g, key);
  REQUIRE(bk::mirror_key(g, mk) == key, "mirror_key is no involution on %llx", (unsigned long long)key);
  const uint64_t mcur = mirror_bits(g, cur), mmask = mirror_bits(g, mask);
  REQUIRE(mk == mcur + mmask, "mirror_key(%llx) is not the mirrored position's key", (unsigned long long)key);
  REQUIRE(bk::canonical_key(g, key) == bk::canonical_key(g, mk), "canonical_key differs for %llx and its mirror",
          (unsigned long long)key);
  REQUIRE(bk::canonical_key(g, key) == std::min(key, mk), "canonical_key(%llx) is not the smaller key",
          (unsigned long long)key);
  int8_t board[64];
  bk::key_to_board(g, key, board);
  REQUIRE(std::string((const char*)board, (size_t)g.HW) == cells_of(g, cur, mask), "key_to_board(%llx)",
          (unsigned long long)key);
  for (int c = 0; c < g.W; ++c) {  // play commutes with the mirror
    uint64_t a, b;
    const int ka = bk::child_key(g, cur, mask, c, &a);
    const int kb = bk::child_key(g, mcur, mmask, g.W - 1 - c, &b);
    REQUIRE(ka == kb && a == b, "column %d of %llx and its mirror image disagree", c, (unsigned long long)key);
    const uint64_t mv = (mask + g.bottom) & g.board & (g.col0 << (c * g.H1));
    REQUIRE((ka == bk::kChildNone) == (mv == 0), "child_key's full-column test, %llx column %d",
            (unsigned long long)key, c);
    if (ka == bk::kChildLive) {
      const uint64_t child = (cur ^ mask) + (mask | mv);  // the mover's stones become the other side's
      REQUIRE(a == std::min(child, bk::mirror_key(g, child)), "child_key(%llx, %d)", (unsigned long long)key, c);
    }
  }
}

// every reachable unfinished position with at most `depth` stones, not reduced: check_position on
// each; counts per level
static std::vector<int64_t> walk_all(const sv::Geo& g, int depth) {
  std::vector<sv::Pos> level{{0, 0}};
  std::vector<int64_t> counts;
  for (int t = 0; t <= depth; ++t) {
    counts.push_back((int64_t)level.size());
    std::unordered_set<uint64_t> seen;
    std::vector<sv::Pos> next;
    for (const sv::Pos& p : level) {
      check_position(g, p.cur, p.mask);
      for (int c = 0; c < g.W; ++c) {
        const uint64_t mv = (p.mask + g.bottom) & g.board & (g.col0 << (c * g.H1));
        if (!mv) continue;
        const uint64_t mine = p.cur | mv, all = p.mask | mv;
        if (sv::has_line(mine, g) || all == g.board) continue;
        if (seen.insert((mine ^ all) + all).second) next.push_back(sv::Pos{mine ^ all, all});
      }
    }
    level.swap(next);
  }
  return counts;
}

// ------------------------------------------------------------ the host book
static bk::HostBook enumerate(const sv::Geo& g, int depth) {
  bk::HostBook b;
  b.H = g.H, b.W = g.W, b.n = g.n, b.depth = depth, b.state = bk::kBuilding;
  b.keys.assign((size_t)depth + 1, {}), b.scores.assign((size_t)depth + 1, {});
  b.keys[0] = {0};
  for (int t = 0; t < depth; ++t) {
    std::vector<uint64_t> out;
    for (uint64_t key : b.keys[(size_t)t]) {
      uint64_t cur, mask, ck;
      bk::decode_key(g, key, &cur, &mask);
      for (int c = 0; c < g.W; ++c) {
        bk::child_key(g, cur, mask, c, &ck);
        out.push_back(ck);  // kNoKey for none, as the device writes it
      }
    }
    std::sort(out.begin(), out.end());
    out.erase(std::unique(out.begin(), out.end()), out.end());
    if (!out.empty() && out.back() == bk::kNoKey) out.pop_back();
    b.keys[(size_t)t + 1] = out;
  }
  for (int t = 0; t <= depth; ++t) b.scores[(size_t)t].assign(b.keys[(size_t)t].size(), bk::kNoScore);
  return b;
}

static int64_t retrograde(const sv::Geo& g, bk::HostBook& b) {  // -> positions flagged bad
  int64_t bad_total = 0;
  for (int t = b.depth - 1; t >= 0; --t) {
    const auto& nk = b.keys[(size_t)t + 1];
    const auto& ns = b.scores[(size_t)t + 1];
    for (size_t i = 0; i < b.keys[(size_t)t].size(); ++i) {
      bool bad;
      b.scores[(size_t)t][i] = bk::retro_value(g, b.keys[(size_t)t][i], t, nk.data(), ns.data(), (int64_t)nk.size(), &bad);
      REQUIRE(!bad || b.scores[(size_t)t][i] == bk::kNoScore, "a flagged position got a score");
      bad_total += bad;
    }
  }
  return bad_total;
}

static void check_counts(const char* name, int H, int W, int n, int depth, const std::vector<int64_t>& canonical,
                         const std::vector<int64_t>& full) {
  const sv::Geo g = sv::make_geo(H, W, n);
  const std::vector<int64_t> walked = walk_all(g, depth);
  if (!full.empty()) REQUIRE(walked == full, "%s: the full level counts differ", name);
  const bk::HostBook b = enumerate(g, depth);
  for (int t = 0; t <= depth; ++t) {
    REQUIRE((int64_t)b.keys[(size_t)t].size() == canonical[(size_t)t], "%s: level %d has %zu canonical positions, not %lld",
            name, t, b.keys[(size_t)t].size(), (long long)canonical[(size_t)t]);
    for (size_t i = 1; i < b.keys[(size_t)t].size(); ++i) REQUIRE(b.keys[(size_t)t][i - 1] < b.keys[(size_t)t][i], "order");
  }
}

static void check_4x4_scores() {
  const sv::Geo g = sv::make_geo(4, 4, 4);
  Ref ref{4, 4, 4, {}};
  bk::HostBook b = enumerate(g, 15);
  int64_t total = 0;
  for (const auto& k : b.keys) total += (int64_t)k.size();
  REQUIRE(total == 1 + 2 + 8 + 26 + 82 + 218 + 564 + 1226 + 2524 + 4378 + 7176 + 9749 + 12365 + 11902 + 10447 + 6495,
          "4x4: %lld canonical positions", (long long)total);
  auto want = [&](uint64_t key) {
    uint64_t cur, mask;
    bk::decode_key(g, key, &cur, &mask);
    return ref.value(cells_of(g, cur, mask));
  };
  for (size_t i = 0; i < b.keys[15].size(); ++i) b.scores[15][i] = (int8_t)want(b.keys[15][i]);  // brute force
  REQUIRE(retrograde(g, b) == 0, "4x4: the retrograde pass flagged a position of a complete book");
  for (int t = 0; t <= 15; ++t)
    for (size_t i = 0; i < b.keys[(size_t)t].size(); ++i)
      REQUIRE(b.scores[(size_t)t][i] == want(b.keys[(size_t)t][i]), "4x4 level %d entry %zu: %d, the negamax says %d", t,
              i, b.scores[(size_t)t][i], want(b.keys[(size_t)t][i]));
  REQUIRE(b.scores[0][0] == 0, "the empty 4x4 board is a draw");

  // a shallower book from the same deepest scores gives the same upper levels
  bk::HostBook s = enumerate(g, 9);
  for (size_t i = 0; i < s.keys[9].size(); ++i) s.scores[9][i] = (int8_t)want(s.keys[9][i]);
  REQUIRE(retrograde(g, s) == 0, "4x4 depth 9");
  for (int t = 0; t <= 9; ++t) REQUIRE(s.keys[(size_t)t] == b.keys[(size_t)t] && s.scores[(size_t)t] == b.scores[(size_t)t], "4x4 depth 9, level %d", t);

  // an unscored child, and a child missing from its level: flagged, and no score comes out
  bk::HostBook u = s;
  u.scores[9][u.scores[9].size() / 2] = bk::kNoScore;
  REQUIRE(retrograde(g, u) > 0 && u.scores[0][0] == bk::kNoScore, "an unscored entry went unnoticed");
  bk::HostBook m = s;
  m.keys[9].erase(m.keys[9].begin() + 5);
  m.scores[9].erase(m.scores[9].begin() + 5);
  REQUIRE(retrograde(g, m) > 0 && m.scores[0][0] == bk::kNoScore, "a missing entry went unnoticed");
}

// ------------------------------------------------------------ the file
static std::vector<unsigned char> slurp(const std::string& path) {
  FILE* f = fopen(path.c_str(), "rb");
  REQUIRE(f, "cannot read %s", path.c_str());
  std::vector<unsigned char> out;
  for (int ch; (ch = fgetc(f)) != EOF;) out.push_back((unsigned char)ch);
  fclose(f);
  return out;
}

static void spill(const std::string& path, const std::vector<unsigned char>& bytes) {
  FILE* f = fopen(path.c_str(), "wb");
  REQUIRE(f, "cannot write %s", path.c_str());
  REQUIRE(bytes.empty() || fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size(), "short write");
  fclose(f);
}

static void expect_refusal(const std::string& path, const sv::Geo& g, const char* word) {
  bk::HostBook out;
  const std::string why = bk::read_book(path.c_str(), g, &out);
  REQUIRE(why.find(word) != std::string::npos, "expected a refusal naming \"%s\", got \"%s\"", word, why.c_str());
}

static void check_file(const std::string& dir) {
  const sv::Geo g = sv::make_geo(4, 4, 4);
  bk::HostBook b = enumerate(g, 6);
  for (int t = 0; t <= 6; ++t)
    for (size_t i = 0; i < b.scores[(size_t)t].size(); ++i) b.scores[(size_t)t][i] = (int8_t)((int)(i % 17) - 8);
  b.scores[6][3] = bk::kNoScore;
  b.next = 4;
  const std::string path = dir + "/book_check.book", bad = dir + "/book_check_bad.book";
  REQUIRE(bk::write_book(path.c_str(), b).empty(), "write_book failed");
  bk::HostBook r;
  const std::string why = bk::read_book(path.c_str(), g, &r);
  REQUIRE(why.empty(), "read_book: %s", why.c_str());
  REQUIRE(r.H == 4 && r.W == 4 && r.n == 4 && r.depth == 6 && r.state == bk::kBuilding && r.next == 4, "header");
  REQUIRE(r.keys == b.keys && r.scores == b.scores, "the levels did not round-trip");
  REQUIRE(bk::write_book(bad.c_str(), r).empty() && slurp(bad) == slurp(path), "a second write differs");

  const std::vector<unsigned char> bytes = slurp(path);
  expect_refusal(dir + "/book_check_missing.book", g, "cannot read");
  expect_refusal(path, sv::make_geo(4, 5, 4), "another geometry");
  expect_refusal(path, sv::make_geo(4, 4, 3), "another geometry");
  std::vector<unsigned char> x = bytes;
  x[0] ^= 1;
  spill(bad, x);
  expect_refusal(bad, g, "wrong magic");
  for (size_t keep : {(size_t)0, (size_t)7, (size_t)20, (size_t)60, bytes.size() / 2, bytes.size() - 1}) {
    spill(bad, std::vector<unsigned char>(bytes.begin(), bytes.begin() + (long)keep));
    expect_refusal(bad, g, "short file");
  }
  x = bytes;
  x.push_back(0);
  spill(bad, x);
  expect_refusal(bad, g, "checksum mismatch");
  for (size_t flip : {(size_t)32, bytes.size() / 2, bytes.size() - 12, bytes.size() - 1}) {
    x = bytes;
    x[flip] ^= 0x10;
    spill(bad, x);
    expect_refusal(bad, g, "checksum mismatch");
  }
  bk::HostBook o = b;  // a valid checksum over a level that is out of order
  std::swap(o.keys[5][10], o.keys[5][11]);
  REQUIRE(bk::write_book(bad.c_str(), o).empty(), "write_book failed");
  expect_refusal(bad, g, "not strictly ascending");
  o = b;
  o.keys[4][7] = o.keys[4][6];
  REQUIRE(bk::write_book(bad.c_str(), o).empty(), "write_book failed");
  expect_refusal(bad, g, "not strictly ascending");
  remove(path.c_str());
  remove(bad.c_str());
}

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  check_counts("4x4", 4, 4, 4, 15,
               {1, 2, 8, 26, 82, 218, 564, 1226, 2524, 4378, 7176, 9749, 12365, 11902, 10447, 6495}, {});
  {
    int64_t total = 0;
    for (int64_t c : walk_all(sv::make_geo(4, 4, 4), 15)) total += c;
    REQUIRE(total == 134289, "4x4 has %lld reachable unfinished positions", (long long)total);
  }
  check_counts("7x6", 6, 7, 4, 6, {1, 4, 25, 121, 568, 2144, 8231}, {1, 7, 49, 238, 1120, 4263, 16422});
  check_counts("5 wide 4 high", 4, 5, 4, 6, {1, 3, 13, 49, 177, 542, 1626}, {});
  check_counts("4 wide 5 high", 5, 4, 4, 6, {1, 2, 8, 26, 82, 220, 600}, {});
  check_counts("5x5 n=3", 5, 5, 3, 5, {1, 3, 13, 49, 177, 495}, {});
  check_4x4_scores();
  check_file(dir);
  printf("ok\n");
  return 0;
}
