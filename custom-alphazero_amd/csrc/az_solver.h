// az_solver.h -- the exact Connect-N solver's search, host + device: one step
// function (an iterative negamax with an explicit stack, one node per call)
// that the gfx950 kernel (az_solver.hip) and a plain host build
// (tests/native/solver_check.cpp) both run, and the host code around it: board
// validation and the split of shallow positions into frontier jobs.  Nothing
// here needs the HIP runtime, so a host compiler builds it under sanitizers.
//
// Position: gravity boards as column-major bitboards, H + 1 bits a column
// (cell (col, row) is bit col * (H + 1) + row, row 0 the bottom; the spare
// top bit of a column stays empty, so `mask + bottom` is the playable cell of
// every column at once).  `cur` holds the stones of the side to move, `mask`
// all stones; cur + mask is a unique key below 2^(W * (H + 1)) <= 2^56.
//
// Score, for the side to move: the winner of a game whose last stone leaves t
// stones on the board scores (H*W + 2 - t) / 2, the loser the negative, a
// draw 0 (the c4solver's convention: 7x6 won with the 7th stone is 18).
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#include "az_device.h"
#else
#ifndef AZ_HD
#define AZ_HD inline
#endif
#endif

namespace az {
namespace solver {

constexpr int kMaxWidth = 16;
constexpr int kMaxBits = 56;  // W * (H + 1): the key and an 8-bit bound share one 64-bit table word

struct Geo {
  int32_t H, W, n, H1, HW;
  uint64_t bottom;  // row 0 of every column
  uint64_t board;   // every cell (no spare bits)
  uint64_t col0;    // the cells of column 0
};

AZ_HD Geo make_geo(int H, int W, int n) {
  Geo g;
  g.H = H, g.W = W, g.n = n, g.H1 = H + 1, g.HW = H * W;
  g.col0 = (1ull << H) - 1;
  g.bottom = 0;
  for (int c = 0; c < W; ++c) g.bottom |= 1ull << (c * g.H1);
  g.board = g.bottom * g.col0;
  return g;
}

// 0 when (H, W, n) is a board the solver takes, else which limit it breaks (1..4)
AZ_HD int geo_limit(int H, int W, int n) {
  if (H < 2 || W < 2) return 1;
  if (W > kMaxWidth) return 2;
  if (W * (H + 1) > kMaxBits) return 3;
  if (n < 2 || n > (H > W ? H : W)) return 4;
  return 0;
}

AZ_HD int popc(uint64_t x) { return __builtin_popcountll(x); }

// Cells x that would complete n in a row of p along shift d: k stones of p on
// the low side of x and n - 1 - k on the high side, for some k.  A line that
// leaves the board steps onto a spare bit or past the word, where p is empty.
// Every shift is by d < 64 (repeated), the same amount in every lane.
AZ_HD uint64_t line_cells(uint64_t p, int d, int n, bool low_only) {
  uint64_t r = 0;
  for (int k = low_only ? n - 1 : 0; k < n; ++k) {
    uint64_t t = ~0ull, q = p;
    for (int i = 0; i < k; ++i) t &= (q <<= d);
    q = p;
    for (int i = 0; i < n - 1 - k; ++i) t &= (q >>= d);
    r |= t;
  }
  return r;
}

// The empty cells where a stone of p makes n in a row (playable now or later).
// Vertically only the stones below count: above an empty cell nothing lies.
AZ_HD uint64_t winning_cells(uint64_t p, uint64_t mask, const Geo& g) {
  const uint64_t r = line_cells(p, 1, g.n, true) | line_cells(p, g.H, g.n, false) |
                     line_cells(p, g.H1, g.n, false) | line_cells(p, g.H + 2, g.n, false);
  return r & (g.board ^ mask);
}

AZ_HD bool has_line(uint64_t p, const Geo& g) {
  const int ds[4] = {1, g.H, g.H1, g.H + 2};
  for (int a = 0; a < 4; ++a) {
    uint64_t t = p, q = p;
    for (int i = 1; i < g.n; ++i) t &= (q >>= ds[a]);
    if (t) return true;
  }
  return false;
}

// what the side to move can play at once and win with
AZ_HD uint64_t wins_now(uint64_t cur, uint64_t mask, const Geo& g) {
  return winning_cells(cur, mask, g) & (mask + g.bottom) & g.board;
}

// the winner's score when its last stone leaves t stones on the board
AZ_HD int win_score(const Geo& g, int t) { return (g.HW + 2 - t) / 2; }

// centre-first: slot j of a node's move list is this column
AZ_HD int slot_column(const Geo& g, int j) { return g.W / 2 + (1 - 2 * (j % 2)) * (j + 1) / 2; }

// ---------------------------------------------------------------- table
// One 64-bit word an entry: the key in the high 56 bits, the bound in the low
// 8 (0: empty; 1..127: value <= b - 64; 128..255: value >= b - 192).  Always
// replace.  A word is read and written as one aligned 8-byte access and a hit
// is compared with the whole key, so whatever another lane stored, and
// whenever it becomes visible, a hit is a true bound of this position: a lost
// or stale entry costs nodes, never the result.
struct Table {
  uint64_t* e;
  int32_t shift;  // 64 - log2(entries)
};

AZ_HD size_t table_slot(const Table& t, uint64_t key) { return (size_t)((key * 0x9E3779B97F4A7C15ull) >> t.shift); }
AZ_HD void table_put_upper(const Table& t, uint64_t key, int v) { t.e[table_slot(t, key)] = key << 8 | (uint64_t)(v + 64); }
AZ_HD void table_put_lower(const Table& t, uint64_t key, int v) { t.e[table_slot(t, key)] = key << 8 | (uint64_t)(v + 192); }

// ---------------------------------------------------------------- search state
// A lane's whole state between two steps; with the lane's stack it is what a
// launch writes back and the next one reloads.
enum : int8_t { kIdle = 0, kEnter = 1, kReturn = 2, kDone = 3 };

struct Lane {
  uint64_t cur, mask;
  uint64_t nodes;
  int32_t job;
  int32_t sp;          // frames on the stack = depth of the node at hand
  int8_t mode;         // kEnter: (alpha, beta) is the window of the node at hand; kReturn: ret is its value
  int8_t ret;
  int8_t alpha, beta;
  int8_t lo, hi, med;  // the exact score lies in lo..hi; the root's window is (med, med + 1)
  int8_t pad;
};

// A frame is 12 bytes: the moves still to try as a nibble per centre-first
// slot (threat count + 1; 0: none or tried), and alpha, beta and the slot
// being searched.  Frame f of a lane is at [f * stride]: a wave touches one
// line per array.  The position is not stored: a move is undone from its bit.
struct Stack {
  uint64_t* moves;
  uint32_t* ab;
  size_t stride;
};

// the next null window of the root (the c4solver's choice of med)
AZ_HD void next_window(Lane& s) {
  const int lo = s.lo, hi = s.hi;
  int med = lo + (hi - lo) / 2;
  if (med <= 0 && lo / 2 < med)
    med = lo / 2;
  else if (med >= 0 && hi / 2 > med)
    med = hi / 2;
  s.med = (int8_t)med;
  s.alpha = (int8_t)med;
  s.beta = (int8_t)(med + 1);
  s.sp = 0;
  s.mode = kEnter;
}

// Begin the exact score of a position that is not over and where the side to
// move has no winning move at once (the host resolves those, wins_now).
AZ_HD void start(Lane& s, const Geo& g, uint64_t cur, uint64_t mask, int job) {
  const int moves = popc(mask);
  s.cur = cur, s.mask = mask, s.nodes = 0, s.job = job;
  s.ret = 0, s.pad = 0;
  s.lo = (int8_t)(-((g.HW - moves) / 2));
  s.hi = (int8_t)((g.HW + 1 - moves) / 2);
  next_window(s);
}

// One step of a lane whose mode is kEnter or kReturn: every lane of a wave runs
// this same body, its three parts predicated.
//   enter  (kEnter): the node at hand is evaluated: a value at once (lost,
//          drawn, window closed by the score bounds or the table), or a frame;
//   pop    (kReturn): the parent's frame comes back, the move is undone, the
//          child's value updates the window: a cutoff, or the frame goes on;
//   pick   (a frame goes on): its best move left is played and the child becomes
//          the node at hand, or none is left and the node's value is alpha.
// A lane whose node ended in `enter` pops in the same step, so a step visits
// one new node unless values are still travelling up.  The root's return
// closes one null window; the last one leaves kDone and the score in lo.
AZ_HD void step(Lane& s, const Geo& g, const Table& tt, const Stack& st) {
  if (s.mode == kReturn && s.sp == 0) {
    if (s.ret <= s.med)
      s.hi = s.ret < s.lo ? s.lo : s.ret;
    else
      s.lo = s.ret > s.hi ? s.hi : s.ret;
    if (s.lo >= s.hi) {
      s.mode = kDone;
      return;
    }
    next_window(s);
  }
  uint64_t cur = s.cur, mask = s.mask, left = 0;
  int alpha = s.alpha, beta = s.beta, sp = s.sp;
  bool pick = false;

  if (s.mode == kEnter) {
    s.nodes++;
    const int moves = popc(mask);
    const uint64_t oppwin = winning_cells(cur ^ mask, mask, g);
    uint64_t possible = (mask + g.bottom) & g.board;
    const uint64_t forced = possible & oppwin;
    if (forced) possible = (forced & (forced - 1)) ? 0 : forced;
    possible &= ~(oppwin >> 1);
    int v = 0;
    bool leaf = true;
    if (!possible) {
      v = -((g.HW - moves) / 2);  // every move lets the other side win with its next stone
    } else if (moves >= g.HW - 2) {
      v = 0;
    } else {
      const int mn = -((g.HW - 2 - moves) / 2), mx = (g.HW - 1 - moves) / 2;
      leaf = false;
      if (alpha < mn) {
        alpha = mn;
        if (alpha >= beta) leaf = true, v = alpha;
      }
      if (!leaf && beta > mx) {
        beta = mx;
        if (alpha >= beta) leaf = true, v = beta;
      }
      if (!leaf) {
        const uint64_t key = cur + mask;
        const uint64_t e = tt.e[table_slot(tt, key)];
        const int b = (int)(e & 255);
        if ((e >> 8) == key && b) {
          if (b >= 128) {
            if (alpha < b - 192) {
              alpha = b - 192;
              if (alpha >= beta) leaf = true, v = alpha;
            }
          } else if (beta > b - 64) {
            beta = b - 64;
            if (alpha >= beta) leaf = true, v = beta;
          }
        }
      }
      if (!leaf) {
        for (int j = 0; j < g.W; ++j) {
          const uint64_t mv = possible & (g.col0 << (slot_column(g, j) * g.H1));
          if (mv) {
            const int threats = popc(winning_cells(cur | mv, mask | mv, g));
            left |= (uint64_t)((threats > 14 ? 14 : threats) + 1) << (4 * j);
          }
        }
        pick = true;
      }
    }
    if (leaf) {
      s.ret = (int8_t)v;
      s.mode = kReturn;
    }
  }

  if (s.mode == kReturn && sp > 0) {
    --sp;
    left = st.moves[(size_t)sp * st.stride];
    const uint32_t ab = st.ab[(size_t)sp * st.stride];
    alpha = (int8_t)(ab & 255), beta = (int8_t)(ab >> 8 & 255);
    const uint64_t m = mask & (g.col0 << (slot_column(g, (int)(ab >> 16 & 15)) * g.H1));
    mask ^= m & ~(m >> 1);  // the column's top stone
    cur ^= mask;
    const int v = -s.ret;
    if (v >= beta) {
      table_put_lower(tt, cur + mask, v);
      s.ret = (int8_t)v;
    } else {
      if (v > alpha) alpha = v;
      pick = true;
    }
  }

  if (pick) {
    if (!left) {
      table_put_upper(tt, cur + mask, alpha);
      s.ret = (int8_t)alpha;
      s.mode = kReturn;
    } else {
      int best = 0, slot = 0;
      for (int j = 0; j < g.W; ++j) {
        const int sc = (int)(left >> (4 * j) & 15);
        if (sc > best) best = sc, slot = j;
      }
      left &= ~(15ull << (4 * slot));
      st.moves[(size_t)sp * st.stride] = left;
      st.ab[(size_t)sp * st.stride] = (uint32_t)(alpha & 255) | (uint32_t)(beta & 255) << 8 | (uint32_t)slot << 16;
      ++sp;
      const uint64_t mv = (mask + g.bottom) & (g.col0 << (slot_column(g, slot) * g.H1));
      cur ^= mask;
      mask |= mv;
      s.alpha = (int8_t)-beta, s.beta = (int8_t)-alpha;
      s.mode = kEnter;
    }
  }
  s.cur = cur, s.mask = mask, s.sp = sp;
}

}  // namespace solver
}  // namespace az

// ---------------------------------------------------------------- host only
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

namespace az {
namespace solver {

struct Pos {
  uint64_t cur, mask;
};

// A board [H][W] int8, row 0 the top row, +1 the side to move's stones, -1 the
// other side's, as bitboards; "" or why it is refused.
inline std::string parse_board(const Geo& g, const int8_t* b, Pos* out) {
  uint64_t cur = 0, mask = 0;
  int mine = 0, theirs = 0;
  for (int c = 0; c < g.W; ++c) {
    bool open = false;  // an empty cell was seen below
    for (int r = 0; r < g.H; ++r) {
      const int v = b[(g.H - 1 - r) * g.W + c];
      if (v != 0 && v != 1 && v != -1) return "holds a value other than -1, 0 and +1";
      if (v == 0) {
        open = true;
        continue;
      }
      if (open) return "has a floating stone";
      const uint64_t bit = 1ull << (c * g.H1 + r);
      mask |= bit;
      if (v == 1) cur |= bit, ++mine; else ++theirs;
    }
  }
  if (mine != theirs && mine + 1 != theirs) return "has a stone count of the wrong parity for the side to move";
  if (has_line(cur, g) || has_line(cur ^ mask, g)) return "is already won";
  if (mine + theirs == g.HW) return "is full";
  out->cur = cur, out->mask = mask;
  return "";
}

// The split of shallow positions.  A root with fewer than `split` stones is
// expanded move by move to the positions with exactly `split` stones (or that
// end sooner); those become ordinary jobs, shared by key among all roots of
// the plan, and their exact scores are backed up by negamax.  Exact, but the
// expanded levels are searched without pruning.
struct Plan {
  std::vector<Pos> jobs;
  std::unordered_map<uint64_t, int32_t> job_of;  // key -> index into jobs
  struct Root {
    Pos p;
    int32_t split;  // 0: resolved without a job, or one job (the root itself)
    bool over;      // its frontier passed max_jobs: unsolved, nothing searched
  };
  std::vector<Root> roots;
};

namespace detail {

inline void frontier(const Geo& g, Pos p, int split, size_t max_jobs, std::unordered_set<uint64_t>& seen,
                     std::vector<Pos>& leaves) {
  if (leaves.size() > max_jobs) return;
  if (!seen.insert(p.cur + p.mask).second) return;
  if (wins_now(p.cur, p.mask, g)) return;
  const uint64_t playable = (p.mask + g.bottom) & g.board;
  if (!playable) return;
  if (popc(p.mask) >= split) {
    leaves.push_back(p);
    return;
  }
  for (int c = 0; c < g.W; ++c) {
    const uint64_t mv = playable & (g.col0 << (c * g.H1));
    if (mv) frontier(g, Pos{p.cur ^ p.mask, p.mask | mv}, split, max_jobs, seen, leaves);
  }
}

constexpr int kUnsolved = 1 << 20;

struct Backup {
  const Geo& g;
  const Plan& plan;
  int split;
  const int32_t* score;
  const uint8_t* status;
  const int64_t* jnodes;
  std::unordered_map<uint64_t, int> memo;
  int64_t nodes = 0;

  int value(Pos p) {
    const uint64_t key = p.cur + p.mask;
    auto it = memo.find(key);
    if (it != memo.end()) return it->second;
    int v;
    const uint64_t playable = (p.mask + g.bottom) & g.board;
    if (wins_now(p.cur, p.mask, g)) {
      v = win_score(g, popc(p.mask) + 1);
    } else if (!playable) {
      v = 0;
    } else if (popc(p.mask) >= split) {
      const int32_t j = plan.job_of.at(key);
      nodes += jnodes[j];
      v = status[j] ? kUnsolved : score[j];
    } else {
      v = -kUnsolved;
      bool open = false;
      for (int c = 0; c < g.W; ++c) {
        const uint64_t mv = playable & (g.col0 << (c * g.H1));
        if (!mv) continue;
        const int cv = value(Pos{p.cur ^ p.mask, p.mask | mv});
        if (cv == kUnsolved) open = true; else if (-cv > v) v = -cv;
      }
      if (open) v = kUnsolved;
    }
    memo.emplace(key, v);
    return v;
  }
};

}  // namespace detail

// the order the queue hands jobs out in: most stones first (stable), so deeper
// results are in the table when shallower searches want them
inline std::vector<int32_t> most_stones_first(const std::vector<Pos>& jobs) {
  std::vector<size_t> at(65, 0);  // a counting sort on 64 - stones
  for (const Pos& p : jobs) ++at[64 - popc(p.mask)];
  size_t sum = 0;
  for (size_t& a : at) {
    const size_t c = a;
    a = sum;
    sum += c;
  }
  std::vector<int32_t> order(jobs.size());
  for (size_t i = 0; i < jobs.size(); ++i) order[at[64 - popc(jobs[i].mask)]++] = (int32_t)i;
  return order;
}

inline int32_t plan_job(Plan& plan, Pos p) {
  auto ins = plan.job_of.emplace(p.cur + p.mask, (int32_t)plan.jobs.size());
  if (ins.second) plan.jobs.push_back(p);
  return ins.first->second;
}

inline void plan_add(Plan& plan, const Geo& g, Pos p, int split_stones, int64_t max_jobs) {
  Plan::Root root{p, 0, false};
  if (!wins_now(p.cur, p.mask, g)) {
    if (popc(p.mask) >= split_stones) {
      plan_job(plan, p);
    } else {
      std::unordered_set<uint64_t> seen;
      std::vector<Pos> leaves;
      detail::frontier(g, p, split_stones, (size_t)max_jobs, seen, leaves);
      root.split = split_stones;
      root.over = leaves.size() > (size_t)max_jobs;
      if (!root.over)
        for (const Pos& q : leaves) plan_job(plan, q);
    }
  }
  plan.roots.push_back(root);
}

// root r's result from the jobs' (score, status 0 solved / 1 unsolved, nodes): false when unsolved
inline bool plan_result(const Plan& plan, const Geo& g, size_t r, const int32_t* score, const uint8_t* status,
                        const int64_t* nodes, int32_t* out_score, int64_t* out_nodes) {
  const Plan::Root& root = plan.roots[r];
  *out_score = 0, *out_nodes = 0;
  if (root.over) return false;
  if (wins_now(root.p.cur, root.p.mask, g)) {
    *out_score = win_score(g, popc(root.p.mask) + 1);
    return true;
  }
  detail::Backup b{g, plan, root.split ? root.split : popc(root.p.mask), score, status, nodes, {}, 0};
  const int v = b.value(root.p);
  *out_nodes = b.nodes;
  if (v == detail::kUnsolved) return false;
  *out_score = v;
  return true;
}

}  // namespace solver
}  // namespace az
