// az_book.h -- the exact solver's opening book, host + device: the functions of
// one position (mirror, canonical key, key -> bitboards, a move's child, the
// value of a position from the scored level below) that the gfx950 kernels
// (az_book.hip) and a plain host build (tests/native/book_check.cpp) both run,
// and the book's file.  Nothing here needs the HIP runtime.
//
// A book of depth D holds, for every t in 0..D, the keys (az_solver.h: cur +
// mask) of all unfinished positions with t stones that play can reach from the
// empty board, each reduced by the left-right mirror to min(key, mirror(key)),
// strictly ascending, and an int8 score per key in the solver's convention
// (kNoScore: none yet).  Level D is scored by the search, the levels above it
// by one negamax step each from the level below.
#pragma once
#include "az_solver.h"

namespace az {
namespace solver {
namespace book {

constexpr int8_t kNoScore = -128;
constexpr uint64_t kNoKey = ~0ull;  // above every key: keys stay below 2^56
enum : int32_t { kNone = 0, kBuilding = 1, kFinished = 2 };

// cur + mask never carries from one column into the next, so the key is W
// fields of H + 1 bits and the mirror reverses their order.
AZ_HD uint64_t mirror_key(const Geo& g, uint64_t key) {
  const uint64_t field = (1ull << g.H1) - 1;
  uint64_t m = 0;
  for (int c = 0; c < g.W; ++c) m |= (key >> (c * g.H1) & field) << ((g.W - 1 - c) * g.H1);
  return m;
}

AZ_HD uint64_t canonical_key(const Geo& g, uint64_t key) {
  const uint64_t m = mirror_key(g, key);
  return m < key ? m : key;
}

// A column of height h holds mask = 2^h - 1 and cur below 2^h, so its field
// plus one is cur + 2^h: the highest set bit of key + bottom gives the height.
// Any key below 2^(W * (H + 1)) decodes to some cur within mask within the
// board or its spare bits; only keys of real positions decode to themselves.
AZ_HD void decode_key(const Geo& g, uint64_t key, uint64_t* cur, uint64_t* mask) {
  const uint64_t field = (1ull << g.H1) - 1;
  uint64_t cu = 0, ma = 0;
  for (int c = 0; c < g.W; ++c) {
    const uint64_t f = (key >> (c * g.H1) & field) + 1;
    int h = 0;
    for (int r = 1; r <= g.H1; ++r)
      if (f >> r & 1) h = r;
    const uint64_t top = 1ull << h;
    ma |= ((top - 1) & field) << (c * g.H1);
    cu |= ((f - top) & (top - 1) & field) << (c * g.H1);
  }
  *cur = cu, *mask = ma;
}

// The child test.  Playing column c in (cur, mask), the side to move's stones
// and all stones: kChildNone when the column is full, kChildEnds when the
// stone completes a line or fills the board, else kChildLive and the child's
// canonical key.
enum : int { kChildNone = 0, kChildEnds = 1, kChildLive = 2 };

AZ_HD int child_key(const Geo& g, uint64_t cur, uint64_t mask, int c, uint64_t* key) {
  const uint64_t mv = (mask + g.bottom) & g.board & (g.col0 << (c * g.H1));
  *key = kNoKey;
  if (!mv) return kChildNone;
  const uint64_t mine = cur | mv, all = mask | mv;
  if (has_line(mine, g) || all == g.board) return kChildEnds;
  *key = canonical_key(g, (mine ^ all) + all);
  return kChildLive;
}

// index of `key` in the strictly ascending keys[0..n), or -1; at most 64 halvings
AZ_HD int64_t find_key(const uint64_t* keys, int64_t n, uint64_t key) {
  int64_t lo = 0, hi = n;
  for (int it = 0; it < 64 && lo < hi; ++it) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return (lo < n && keys[lo] == key) ? lo : -1;
}

// The retrograde value of a position with t stones from the scored level t + 1
// (next_keys, next_scores, next_n): a win at once, else the best of 0 for a
// child that fills the board and minus the child's score.  kNoScore, with *bad
// set, when a child is missing from the level or has no score.
AZ_HD int8_t retro_value(const Geo& g, uint64_t key, int t, const uint64_t* next_keys, const int8_t* next_scores,
                         int64_t next_n, bool* bad) {
  uint64_t cur, mask;
  decode_key(g, key, &cur, &mask);
  *bad = false;
  if (wins_now(cur, mask, g)) return (int8_t)win_score(g, t + 1);
  int best = -127;
  for (int c = 0; c < g.W; ++c) {
    uint64_t ck;
    const int kind = child_key(g, cur, mask, c, &ck);
    if (kind == kChildNone) continue;
    int v = 0;  // kChildEnds without a win at once: the board is full
    if (kind == kChildLive) {
      const int64_t at = find_key(next_keys, next_n, ck);
      if (at < 0 || next_scores[at] == kNoScore) {
        *bad = true;
        return kNoScore;
      }
      v = -next_scores[at];
    }
    if (v > best) best = v;
  }
  if (best == -127) *bad = true;  // an unfinished position has a move
  return best == -127 ? kNoScore : (int8_t)best;
}

// A book entry as the ABI's board: [H][W] int8, row 0 the top row, +1 the side to move.
AZ_HD void key_to_board(const Geo& g, uint64_t key, int8_t* b) {
  uint64_t cur, mask;
  decode_key(g, key, &cur, &mask);
  for (int c = 0; c < g.W; ++c)
    for (int r = 0; r < g.H; ++r) {
      const uint64_t bit = 1ull << (c * g.H1 + r);
      b[(g.H - 1 - r) * g.W + c] = (int8_t)((mask & bit) ? ((cur & bit) ? 1 : -1) : 0);
    }
}

}  // namespace book
}  // namespace solver
}  // namespace az

// ---------------------------------------------------------------- host only
#include <stdio.h>
#include <string.h>

namespace az {
namespace solver {
namespace book {

// The book on the host, as the file holds it.  `next` is where the level-D
// solve goes on (the first entry the current pass has not tried); 0 once finished.
struct HostBook {
  int32_t H = 0, W = 0, n = 0, depth = -1, state = kNone;
  int64_t next = 0;
  std::vector<std::vector<uint64_t>> keys;   // [depth + 1]
  std::vector<std::vector<int8_t>> scores;   // [depth + 1]
};

constexpr char kMagic[8] = {'A', 'Z', 'B', 'O', 'O', 'K', 0, 0};
constexpr uint32_t kFileVersion = 1;

// FNV-1a, 64 bits
struct Checksum {
  uint64_t h = 0xCBF29CE484222325ull;
  void add(const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001B3ull;
  }
};

namespace detail {

template <typename T>
inline void put_le(std::vector<unsigned char>& out, T v) {
  for (size_t i = 0; i < sizeof(T); ++i) out.push_back((unsigned char)((uint64_t)v >> (8 * i) & 255));
}

template <typename T>
inline T get_le(const unsigned char* p) {
  uint64_t v = 0;
  for (size_t i = 0; i < sizeof(T); ++i) v |= (uint64_t)p[i] << (8 * i);
  return (T)v;
}

}  // namespace detail

// Little endian: magic, version, H, W, n, depth, state (int32 each), next and
// the depth + 1 level counts (int64), per level the keys (uint64) then the
// scores (int8), and the FNV-1a checksum of everything before it.  "" or why not.
inline std::string write_book(const char* path, const HostBook& b) {
  std::vector<unsigned char> head(kMagic, kMagic + 8);
  detail::put_le<uint32_t>(head, kFileVersion);
  for (int32_t v : {b.H, b.W, b.n, b.depth, b.state}) detail::put_le<int32_t>(head, v);
  detail::put_le<int64_t>(head, b.next);
  for (int t = 0; t <= b.depth; ++t) detail::put_le<int64_t>(head, (int64_t)b.keys[t].size());
  FILE* f = fopen(path, "wb");
  if (!f) return std::string("cannot write ") + path;
  Checksum sum;
  bool ok = fwrite(head.data(), 1, head.size(), f) == head.size();
  sum.add(head.data(), head.size());
  std::vector<unsigned char> buf;
  for (int t = 0; t <= b.depth && ok; ++t) {
    buf.clear();
    buf.reserve(b.keys[t].size() * 9);
    for (uint64_t k : b.keys[t]) detail::put_le<uint64_t>(buf, k);
    for (int8_t s : b.scores[t]) buf.push_back((unsigned char)s);
    ok = buf.empty() || fwrite(buf.data(), 1, buf.size(), f) == buf.size();
    sum.add(buf.data(), buf.size());
  }
  buf.clear();
  detail::put_le<uint64_t>(buf, sum.h);
  ok = ok && fwrite(buf.data(), 1, buf.size(), f) == buf.size();
  ok = (fclose(f) == 0) && ok;
  return ok ? "" : std::string("short write to ") + path;
}

// Reads a book for geometry g; "" or which refusal: the magic, the geometry, a
// short file, the checksum, a level whose keys are not strictly ascending.
inline std::string read_book(const char* path, const Geo& g, HostBook* out) {
  FILE* f = fopen(path, "rb");
  if (!f) return std::string("cannot read ") + path;
  std::vector<unsigned char> all;
  unsigned char chunk[1 << 16];
  for (size_t got; (got = fread(chunk, 1, sizeof(chunk), f)) > 0;) all.insert(all.end(), chunk, chunk + got);
  fclose(f);
  const size_t fixed = 8 + 4 + 5 * 4 + 8;
  if (all.size() >= 8 && memcmp(all.data(), kMagic, 8) != 0) return "wrong magic: not a book file";
  if (all.size() < fixed) return "short file: the header is cut off";
  const unsigned char* p = all.data() + 8;
  if (detail::get_le<uint32_t>(p) != kFileVersion) return "wrong magic: another file version";
  HostBook b;
  b.H = detail::get_le<int32_t>(p + 4), b.W = detail::get_le<int32_t>(p + 8), b.n = detail::get_le<int32_t>(p + 12);
  b.depth = detail::get_le<int32_t>(p + 16), b.state = detail::get_le<int32_t>(p + 20);
  b.next = detail::get_le<int64_t>(p + 24);
  if (b.H != g.H || b.W != g.W || b.n != g.n)
    return "another geometry: the file is " + std::to_string(b.W) + "x" + std::to_string(b.H) +
           " n=" + std::to_string(b.n) + ", the solver " + std::to_string(g.W) + "x" + std::to_string(g.H) +
           " n=" + std::to_string(g.n);
  if (b.depth < 0 || b.depth > g.HW - 1 || (b.state != kBuilding && b.state != kFinished))
    return "short file: a header field is out of range";
  size_t at = fixed + (size_t)(b.depth + 1) * 8;
  if (all.size() < at + 8) return "short file: the level counts are cut off";
  std::vector<int64_t> counts(b.depth + 1);
  size_t need = at + 8;
  for (int t = 0; t <= b.depth; ++t) {
    counts[t] = detail::get_le<int64_t>(all.data() + fixed + (size_t)t * 8);
    if (counts[t] < 0 || (uint64_t)counts[t] > all.size()) return "short file: a level is cut off";
    need += (size_t)counts[t] * 9;
  }
  if (all.size() < need) return "short file: a level is cut off";
  Checksum sum;
  sum.add(all.data(), need - 8);
  if (all.size() != need || sum.h != detail::get_le<uint64_t>(all.data() + need - 8)) return "checksum mismatch";
  const uint64_t limit = 1ull << (g.W * g.H1);
  b.keys.resize(b.depth + 1), b.scores.resize(b.depth + 1);
  for (int t = 0; t <= b.depth; ++t) {
    const size_t n = (size_t)counts[t];
    b.keys[t].resize(n), b.scores[t].resize(n);
    for (size_t i = 0; i < n; ++i) {
      const uint64_t k = detail::get_le<uint64_t>(all.data() + at + i * 8);
      if ((i > 0 && k <= b.keys[t][i - 1]) || k >= limit)
        return "level " + std::to_string(t) + " has keys that are not strictly ascending";
      b.keys[t][i] = k;
    }
    at += n * 8;
    for (size_t i = 0; i < n; ++i) b.scores[t][i] = (int8_t)all[at + i];
    at += n;
  }
  if (b.next < 0 || b.next > counts[b.depth]) return "short file: a header field is out of range";
  *out = std::move(b);
  return "";
}

}  // namespace book
}  // namespace solver
}  // namespace az
