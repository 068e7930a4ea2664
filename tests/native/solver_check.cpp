// solver_check.cpp -- the exact Connect-N solver without a GPU.  Two solvers:
//
//  * an independent reference written here: boards as row-major int8 arrays
//    (row 0 the top row, +1 the side to move: the ABI's own form), a plain
//    negamax with a memo table, no heuristic, no null window, no move order;
//    for 7x6 the same recursion with a plain alpha-beta window and a memo of
//    bounds, taking a stone that ends the game before it searches.  It shares
//    no function with csrc/.
//  * the host build of csrc/az_solver.h's step function, driven serially with a
//    private table, and again with its state written out to a byte buffer and
//    reloaded every k steps, as the device does between launches.
//
// usage: solver_check check NAME            one named check; prints "ok" or fails
//        solver_check table H W N OUT       every reachable unfinished position with its score
//        solver_check random H W N COUNT SEED LO HI OUT
//                                           seeded random-playout positions with LO..HI stones
//        solver_check scores H W N IN OUT   the reference's scores of the boards in IN (H*W int8 each)
// OUT holds records of H*W int8 (the board), int8 (the reference score), int64
// (the host build's node count, little endian).  Built by tests/test_solver_cpu.py
// with -fsanitize=address,undefined.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../custom-alphazero_amd/csrc/az_solver.h"

namespace sv = az::solver;

#define REQUIRE(cond, ...)                                  \
  do {                                                      \
    if (!(cond)) {                                          \
      fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
      fprintf(stderr, __VA_ARGS__);                         \
      fprintf(stderr, "\n");                                \
      exit(1);                                              \
    }                                                       \
  } while (0)

// ------------------------------------------------------------ the reference
struct Ref {
  int H, W, N;
  std::unordered_map<std::string, int> memo;                   // exact scores (plain)

  Ref(int h, int w, int n) : H(h), W(w), N(n) {}

  int at(const std::string& b, int r, int c) const {
    return (r < 0 || r >= H || c < 0 || c >= W) ? 0 : (int)(int8_t)b[r * W + c];
  }
  // the row a stone dropped into column c lands in, -1 when the column is full
  int landing(const std::string& b, int c) const {
    int r = H - 1;
    while (r >= 0 && b[r * W + c] != 0) --r;
    return r;
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
  static int stones(const std::string& b) {
    int n = 0;
    for (char v : b) n += v != 0;
    return n;
  }
  static std::string flipped(std::string b) {
    for (char& v : b) v = (char)-(int8_t)v;
    return b;
  }
  int win_value(int t) const { return (H * W + 2 - t) / 2; }

  // exact, no pruning: fills memo with every unfinished position reachable from b
  int plain(const std::string& b) {
    auto it = memo.find(b);
    if (it != memo.end()) return it->second;
    const int t = stones(b) + 1;
    int best = -1000;
    for (int c = 0; c < W; ++c) {
      const int r = landing(b, c);
      if (r < 0) continue;
      std::string nb = b;
      nb[r * W + c] = 1;
      int v;
      if (makes_line(nb, r, c))
        v = win_value(t);
      else if (t == H * W)
        v = 0;
      else
        v = -plain(flipped(nb));
      best = std::max(best, v);
    }
    memo.emplace(b, best);
    return best;
  }

  // The same recursion inside a plain alpha-beta window, with a memo of proven
  // bounds: what finishes 7x6 in seconds.  Stones keep their colours on one
  // array (make / unmake), `who` is the colour to move; the memo key packs two
  // bits a cell, row-major, and the colour to move.
  struct Key {
    uint64_t lo, hi;
    bool operator==(const Key& o) const { return lo == o.lo && hi == o.hi; }
  };
  struct KeyHash {
    size_t operator()(const Key& k) const { return (size_t)((k.lo * 0x9E3779B97F4A7C15ull) ^ (k.hi * 0xC2B2AE3D27D4EB4Full)); }
  };
  std::unordered_map<Key, std::pair<int8_t, int8_t>, KeyHash> bound;  // lower, upper
  std::string cells;
  Key key{0, 0};

  void toggle(int i, int who) {
    const uint64_t code = who > 0 ? 1 : 2;
    if (i < 32) key.lo ^= code << (2 * i); else key.hi ^= code << (2 * (i - 32));
  }
  int window(int who, int count, int alpha, int beta) {
    Key k = key;
    if (who < 0) k.hi |= 1ull << 63;
    auto it = bound.find(k);
    if (it != bound.end()) {
      if (it->second.first >= beta) return it->second.first;
      if (it->second.second <= alpha) return it->second.second;
      if (it->second.first == it->second.second) return it->second.first;
      alpha = std::max<int>(alpha, it->second.first);
      beta = std::min<int>(beta, it->second.second);
    }
    const int t = count + 1, a0 = alpha;
    int best = -100;
    // a stone that ends the game at once is the best there is (every later win scores less)
    for (int c = 0; c < W && best == -100; ++c) {
      const int r = landing(cells, c);
      if (r < 0) continue;
      cells[r * W + c] = (char)who;
      if (makes_line(cells, r, c)) best = win_value(t);
      cells[r * W + c] = 0;
    }
    for (int c = 0; c < W && best < beta && best != win_value(t); ++c) {
      const int r = landing(cells, c);
      if (r < 0) continue;
      cells[r * W + c] = (char)who;
      int v;
      if (t == H * W) {
        v = 0;
      } else {
        toggle(r * W + c, who);
        v = -window(-who, t, -beta, -std::max(alpha, best));
        toggle(r * W + c, who);
      }
      cells[r * W + c] = 0;
      best = std::max(best, v);
    }
    std::pair<int8_t, int8_t>& e = bound.emplace(k, std::make_pair((int8_t)-100, (int8_t)100)).first->second;
    if (best <= a0)
      e.second = std::min<int8_t>(e.second, (int8_t)best);
    else if (best >= beta)
      e.first = std::max<int8_t>(e.first, (int8_t)best);
    else
      e.first = e.second = (int8_t)best;
    return best;
  }
  int ab(const std::string& b) {
    cells = b;
    key = Key{0, 0};
    for (int i = 0; i < H * W; ++i)
      if (b[i]) toggle(i, (int8_t)b[i]);
    return window(1, stones(b), -100, 100);
  }
};

// ------------------------------------------------------------ the host build
struct Host {
  sv::Geo g;
  std::vector<uint64_t> words;
  sv::Table tt;
  std::vector<uint64_t> frames_moves;
  std::vector<uint32_t> frames_ab;
  int split = 0;
  int64_t max_jobs = 1 << 20;
  int every = 0;  // write the lane out and reload it every `every` steps (0: never)

  Host(int H, int W, int n, int tt_log2) : g(sv::make_geo(H, W, n)) {
    words.assign((size_t)1 << tt_log2, 0);
    tt = sv::Table{words.data(), 64 - tt_log2};
    frames_moves.assign(g.HW, 0);
    frames_ab.assign(g.HW, 0);
  }

  // one job: false when the budget ran out
  bool job(sv::Pos p, uint64_t budget, int* score, int64_t* nodes) {
    const sv::Stack st{frames_moves.data(), frames_ab.data(), 1};
    sv::Lane s;
    memset(&s, 0, sizeof(s));
    sv::start(s, g, p.cur, p.mask, 0);
    unsigned char saved[sizeof(sv::Lane)];
    for (uint64_t steps = 1;; ++steps) {
      if (s.mode == sv::kDone) break;
      if (s.nodes >= budget) {
        *nodes = (int64_t)s.nodes;
        return false;
      }
      REQUIRE(s.sp >= 0 && s.sp < g.HW - 1, "stack depth %d", s.sp);
      sv::step(s, g, tt, st);
      if (every && steps % every == 0) {
        memcpy(saved, &s, sizeof(s));
        memset(&s, 0xA5, sizeof(s));
        memcpy(&s, saved, sizeof(s));
      }
    }
    *score = s.lo;
    *nodes = (int64_t)s.nodes;
    return true;
  }

  // boards in the ABI's form, through parse_board and the plan, as az_solver_solve does
  void solve(const std::vector<std::string>& boards, uint64_t budget, std::vector<int>& score,
             std::vector<uint8_t>& status, std::vector<int64_t>& nodes) {
    sv::Plan plan;
    for (const std::string& b : boards) {
      sv::Pos p;
      const std::string why = sv::parse_board(g, (const int8_t*)b.data(), &p);
      REQUIRE(why.empty(), "board refused: %s", why.c_str());
      sv::plan_add(plan, g, p, split, max_jobs);
    }
    const size_t n = plan.jobs.size();
    std::vector<int32_t> js(n, 0);
    std::vector<uint8_t> jst(n, 1);
    std::vector<int64_t> jn(n, 0);
    const std::vector<int32_t> order = sv::most_stones_first(plan.jobs);
    std::vector<char> seen(n, 0);
    for (size_t i = 0; i < n; ++i) {
      REQUIRE(order[i] >= 0 && (size_t)order[i] < n && !seen[order[i]], "the job order is no permutation at %zu", i);
      seen[order[i]] = 1;
      REQUIRE(i == 0 || __builtin_popcountll(plan.jobs[order[i - 1]].mask) >= __builtin_popcountll(plan.jobs[order[i]].mask),
              "job %zu has more stones than the one before it", i);
    }
    for (int32_t j : order) {
      int v = 0;
      jst[j] = job(plan.jobs[j], budget, &v, &jn[j]) ? 0 : 1;
      js[j] = v;
    }
    score.assign(boards.size(), 0), status.assign(boards.size(), 0), nodes.assign(boards.size(), 0);
    for (size_t r = 0; r < boards.size(); ++r) {
      int32_t v = 0;
      status[r] = sv::plan_result(plan, g, r, js.data(), jst.data(), jn.data(), &v, &nodes[r]) ? 0 : 1;
      score[r] = v;
    }
  }
};

// ------------------------------------------------------------ positions
static std::vector<std::string> random_positions(Ref& ref, int count, uint64_t seed, int lo, int hi) {
  std::mt19937_64 rng(seed);
  std::vector<std::string> out;
  while ((int)out.size() < count) {
    const int target = lo + (int)(rng() % (uint64_t)(hi - lo + 1));
    std::string b((size_t)ref.H * ref.W, 0);
    bool over = false;
    for (int t = 0; t < target && !over; ++t) {
      std::vector<int> cols;
      for (int c = 0; c < ref.W; ++c)
        if (ref.landing(b, c) >= 0) cols.push_back(c);
      if (cols.empty()) {
        over = true;
        break;
      }
      const int c = cols[rng() % cols.size()], r = ref.landing(b, c);
      b[r * ref.W + c] = 1;
      over = ref.makes_line(b, r, c);
      b = Ref::flipped(b);
    }
    if (!over && Ref::stones(b) < ref.H * ref.W) out.push_back(b);
  }
  return out;
}

static const uint64_t kNoBudget = ~0ull;

// every board: the host build, serial and interrupted every 1, 7 and 1000 steps, equals `want`
static void agree(int H, int W, int n, const std::vector<std::string>& boards, const std::vector<int>& want,
                  std::vector<int64_t>* nodes_out = nullptr) {
  for (int every : {0, 1, 7, 1000}) {
    Host h(H, W, n, 16);
    h.every = every;
    std::vector<int> score;
    std::vector<uint8_t> status;
    std::vector<int64_t> nodes;
    h.solve(boards, kNoBudget, score, status, nodes);
    for (size_t i = 0; i < boards.size(); ++i)
      REQUIRE(status[i] == 0 && score[i] == want[i], "%dx%d n=%d every=%d board %zu: got %d (status %d), want %d", W, H,
              n, every, i, score[i], status[i], want[i]);
    if (every == 0 && nodes_out) *nodes_out = nodes;
  }
}

static void exhaustive(int H, int W, int n, std::vector<std::string>* boards, std::vector<int>* want) {
  Ref ref(H, W, n);
  ref.plain(std::string((size_t)H * W, 0));
  for (const auto& kv : ref.memo) {
    boards->push_back(kv.first);
    want->push_back(kv.second);
  }
}

static void sampled(int H, int W, int n, int count, uint64_t seed, int lo, int hi, bool windowed,
                    std::vector<std::string>* boards, std::vector<int>* want) {
  Ref ref(H, W, n);
  *boards = random_positions(ref, count, seed, lo, hi);
  for (const std::string& b : *boards) want->push_back(windowed ? ref.ab(b) : ref.plain(b));
}

static void write_records(const char* path, const std::vector<std::string>& boards, const std::vector<int>& want,
                          const std::vector<int64_t>& nodes) {
  FILE* f = fopen(path, "wb");
  REQUIRE(f, "cannot write %s", path);
  for (size_t i = 0; i < boards.size(); ++i) {
    const int8_t s = (int8_t)want[i];
    const int64_t n = nodes[i];
    fwrite(boards[i].data(), 1, boards[i].size(), f);
    fwrite(&s, 1, 1, f);
    fwrite(&n, 8, 1, f);
  }
  fclose(f);
}

// ------------------------------------------------------------ checks
static void check_exhaustive(int H, int W, int n) {
  std::vector<std::string> boards;
  std::vector<int> want;
  exhaustive(H, W, n, &boards, &want);
  REQUIRE(boards.size() > 100, "only %zu positions", boards.size());
  agree(H, W, n, boards, want);
  printf("%zu positions\n", boards.size());
}

static void check_sampled(int H, int W, int n, int count, int lo, int hi, bool windowed) {
  std::vector<std::string> boards;
  std::vector<int> want;
  sampled(H, W, n, count, 20261020, lo, hi, windowed, &boards, &want);
  agree(H, W, n, boards, want);
}

static void check_tables() {
  // 2^4 entries (collisions, replacement) against 2^20; then the warm table again
  std::vector<std::string> boards;
  std::vector<int> want;
  sampled(4, 5, 4, 100, 7, 2, 14, false, &boards, &want);
  for (int log2 : {4, 20}) {
    Host h(4, 5, 4, log2);
    std::vector<int> score;
    std::vector<uint8_t> status;
    std::vector<int64_t> cold, warm;
    h.solve(boards, kNoBudget, score, status, cold);
    for (size_t i = 0; i < boards.size(); ++i) REQUIRE(score[i] == want[i], "tt 2^%d board %zu", log2, i);
    h.solve(boards, kNoBudget, score, status, warm);
    for (size_t i = 0; i < boards.size(); ++i) REQUIRE(score[i] == want[i], "warm tt 2^%d board %zu", log2, i);
    if (log2 == 20) {
      int64_t c = 0, w = 0;
      for (size_t i = 0; i < boards.size(); ++i) c += cold[i], w += warm[i];
      REQUIRE(w < c, "the warm pass searched %lld nodes, the cold one %lld", (long long)w, (long long)c);
    }
  }
}

static void check_split() {
  std::vector<std::string> boards;
  std::vector<int> want;
  sampled(4, 5, 4, 12, 11, 0, 10, false, &boards, &want);
  boards.push_back(std::string(20, 0));
  {
    Ref ref(4, 5, 4);
    want.push_back(ref.plain(boards.back()));
  }
  for (size_t i = 0; i < boards.size(); ++i) {
    const int stones = Ref::stones(boards[i]);
    for (int split : {0, stones + 1, stones + 2, stones + 4}) {
      Host h(4, 5, 4, 16);
      h.split = split;
      std::vector<int> score;
      std::vector<uint8_t> status;
      std::vector<int64_t> nodes;
      h.solve({boards[i]}, kNoBudget, score, status, nodes);
      REQUIRE(status[0] == 0 && score[0] == want[i], "board %zu split %d: got %d want %d", i, split, score[0], want[i]);
    }
  }
  // a frontier over max_jobs: unsolved, and nothing searched
  Host h(4, 5, 4, 16);
  h.split = 6;
  h.max_jobs = 10;
  std::vector<int> score;
  std::vector<uint8_t> status;
  std::vector<int64_t> nodes;
  h.solve({std::string(20, 0)}, kNoBudget, score, status, nodes);
  REQUIRE(status[0] == 1 && nodes[0] == 0, "status %d nodes %lld", status[0], (long long)nodes[0]);
  for (uint64_t w : h.words) REQUIRE(w == 0, "the table was written");
}

static void check_budget() {
  Ref ref(6, 7, 4);
  std::vector<std::string> boards = random_positions(ref, 8, 5, 20, 22);
  Host h(6, 7, 4, 20);
  std::vector<int> score;
  std::vector<uint8_t> status;
  std::vector<int64_t> nodes;
  h.solve(boards, kNoBudget, score, status, nodes);
  size_t hard = 0;
  for (size_t i = 1; i < boards.size(); ++i)
    if (nodes[i] > nodes[hard]) hard = i;
  REQUIRE(nodes[hard] > 40, "no position needs more than 40 nodes");
  const int want = score[hard];
  Host h2(6, 7, 4, 20);
  const uint64_t small = (uint64_t)nodes[hard] / 2;
  h2.solve({boards[hard]}, small, score, status, nodes);
  REQUIRE(status[0] == 1, "solved within half its nodes");
  REQUIRE(nodes[0] <= (int64_t)small, "%lld nodes on a budget of %llu", (long long)nodes[0], (unsigned long long)small);
  // the aborted job's table entries are true bounds: the same table serves the full search
  h2.solve({boards[hard]}, kNoBudget, score, status, nodes);
  REQUIRE(status[0] == 0 && score[0] == want, "after the abort: %d, want %d", score[0], want);
}

static void check_validation() {
  const sv::Geo g = sv::make_geo(4, 4, 4);
  sv::Pos p;
  auto refuse = [&](std::vector<int> cells, const char* word) {
    std::string b(16, 0);
    for (size_t i = 0; i < cells.size(); ++i) b[i] = (char)cells[i];
    const std::string why = sv::parse_board(g, (const int8_t*)b.data(), &p);
    REQUIRE(why.find(word) != std::string::npos, "expected '%s', got '%s'", word, why.c_str());
  };
  // rows top to bottom
  refuse({0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 0, 0}, "floating");
  refuse({0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0}, "parity");    // the side to move is one ahead
  refuse({0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, -1, -1, 0, 0}, "parity");  // the other side is two ahead
  refuse({0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0, -1, -1, -1, -1}, "already won");
  refuse({0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, -1, 0, 0}, "other than");
  refuse({1, -1, 1, -1, 1, -1, 1, -1, -1, 1, -1, 1, -1, 1, -1, 1}, "full");
  std::string ok(16, 0);
  ok[12] = -1;
  REQUIRE(sv::parse_board(g, (const int8_t*)ok.data(), &p).empty(), "a legal board was refused");
  REQUIRE(p.mask == 1 && p.cur == 0, "bitboards of one stone");
  REQUIRE(sv::geo_limit(6, 7, 4) == 0 && sv::geo_limit(6, 8, 4) == 0 && sv::geo_limit(5, 9, 4) == 0 &&
              sv::geo_limit(7, 6, 4) == 0 && sv::geo_limit(4, 5, 5) == 0,
          "an accepted board was refused");
  REQUIRE(sv::geo_limit(1, 7, 2) && sv::geo_limit(2, 17, 2) && sv::geo_limit(7, 8, 4) && sv::geo_limit(6, 7, 8) &&
              sv::geo_limit(6, 7, 1),
          "a board outside the limits was accepted");
  // the score convention: 7x6 won with the 7th stone is 18
  REQUIRE(sv::win_score(sv::make_geo(6, 7, 4), 7) == 18, "win_score");
}

int main(int argc, char** argv) {
  if (argc >= 3 && !strcmp(argv[1], "check")) {
    const std::string name = argv[2];
    if (name == "exhaustive_4x4") check_exhaustive(4, 4, 4);
    else if (name == "exhaustive_4x3_n3") check_exhaustive(3, 4, 3);
    else if (name == "random_5x4") check_sampled(4, 5, 4, 2000, 0, 19, false);
    else if (name == "random_4x5") check_sampled(5, 4, 4, 2000, 0, 19, false);
    else if (name == "random_5x5_n3") check_sampled(5, 5, 3, 2000, 0, 24, false);
    else if (name == "c4_7x6") check_sampled(6, 7, 4, 256, 18, 36, true);
    else if (name == "tables") check_tables();
    else if (name == "split") check_split();
    else if (name == "budget") check_budget();
    else if (name == "validation") check_validation();
    else REQUIRE(false, "unknown check %s", name.c_str());
    printf("ok\n");
    return 0;
  }
  if (argc == 6 && !strcmp(argv[1], "table")) {
    const int H = atoi(argv[2]), W = atoi(argv[3]), n = atoi(argv[4]);
    std::vector<std::string> boards;
    std::vector<int> want;
    exhaustive(H, W, n, &boards, &want);
    write_records(argv[5], boards, want, std::vector<int64_t>(boards.size(), 0));
    printf("%zu\n", boards.size());
    return 0;
  }
  if (argc == 10 && !strcmp(argv[1], "random")) {
    const int H = atoi(argv[2]), W = atoi(argv[3]), n = atoi(argv[4]);
    std::vector<std::string> boards;
    std::vector<int> want;
    std::vector<int64_t> nodes;
    sampled(H, W, n, atoi(argv[5]), strtoull(argv[6], nullptr, 10), atoi(argv[7]), atoi(argv[8]), H * W > 25, &boards,
            &want);
    Host h(H, W, n, 20);
    std::vector<int> score;
    std::vector<uint8_t> status;
    h.solve(boards, kNoBudget, score, status, nodes);
    for (size_t i = 0; i < boards.size(); ++i) REQUIRE(score[i] == want[i], "board %zu", i);
    write_records(argv[9], boards, want, nodes);
    printf("%zu\n", boards.size());
    return 0;
  }
  if (argc == 7 && !strcmp(argv[1], "scores")) {
    const int H = atoi(argv[2]), W = atoi(argv[3]), n = atoi(argv[4]);
    FILE* f = fopen(argv[5], "rb");
    REQUIRE(f, "cannot read %s", argv[5]);
    std::vector<std::string> boards;
    std::vector<int> want;
    std::string b((size_t)H * W, 0);
    Ref ref(H, W, n);
    while (fread(&b[0], 1, b.size(), f) == b.size()) {
      boards.push_back(b);
      want.push_back(ref.ab(b));
    }
    fclose(f);
    write_records(argv[6], boards, want, std::vector<int64_t>(boards.size(), 0));
    printf("%zu\n", boards.size());
    return 0;
  }
  fprintf(stderr,
          "usage: solver_check check NAME | table H W N OUT | random H W N COUNT SEED LO HI OUT | scores H W N IN OUT\n");
  return 2;
}
