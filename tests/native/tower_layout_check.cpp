// States the layout the one-launch tower gets for a Connect-N network: what
// libaz.so's own chooser az::tower16_choose_layout (csrc/az_tower16.hip; the
// function load_network, the launchers and the stats read) returns.  Only
// presentation is added here: the name of the slot plan's form and the FLOP
// of the same tiles without a plan.  CUs and lanes are fixed (256, 1): the
// dual launch's threshold is not printed.
// argv: groups of H W A depth hidden -> one JSON object per group.
// --sweep: every Connect-N shape the tower takes (H, W >= 2, HW <= 128; A = W
// or HW; depth 1, 4, 16; hidden 1, 64, 255, 256), each chosen layout checked
// against the library's other tower16_* functions ->
// {"shapes", "not_ok": [shapes without a layout], "failures": [shape + what]}.
// --rows-stem, then groups of depth hidden: the chess network's input-row form
// (H = W = 8, A = 1880) -> per group tower, tile_rows, boards, dbuf, the staged
// prefix, the LDS bytes of the chosen form and of the in-place one, and the
// issued FLOP per board with 2 (self-play) and with 4 stem chunks.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "az_tower_layout.h"

namespace {
using az::TowerLayout;
using az::TowerTiles;

TowerLayout layout_of(int H, int W, int A, int depth, int hidden) {
  az::TowerShape s;
  s.H = H, s.W = W, s.A = A, s.depth = depth, s.hidden = hidden, s.cus = 256, s.lanes = 1;
  return az::tower16_choose_layout(s);
}
double natural_flop(const TowerTiles& t, int HW, int depth) {
  const int none[2] = {0, 0};
  return az::tower16_issued_flop_per_board(HW, t.rows, depth, none, false, 2);
}
// wv1, wpd, plan, skipped, flop, flop_natural of one tile height, each key with `pre` in front
void print_tiles(const TowerTiles& t, const char* pre, bool xtile, int HW, int depth) {
  // skipped block-taps over both M halves: four border blocks (top, bottom | left, right) skip 3 taps each,
  // top | bottom alone 6
  const int k = __builtin_popcount(t.skip[0]) + __builtin_popcount(t.skip[1]);
  const char* form = t.slot_pix.empty() ? "none" : k == 12 ? "four_borders" : k == 6 ? "top_bottom" : "other";
  printf(", \"%swv1\": \"%s\", \"%swpd\": \"%s\", \"%splan\": \"%s\", \"%sskipped\": %d, \"%sflop\": %.17g, "
         "\"%sflop_natural\": %.17g",
         pre, xtile ? "xtile" : t.wv1_lds ? "lds" : "l2", pre, t.wpd_lds ? "lds" : "l2", pre, form, pre, k, pre,
         t.issued_flop_per_board, pre, natural_flop(t, HW, depth));
}

// what one tile height of a chosen layout gets wrong; "" when its invariants hold
std::string fault_of(const TowerLayout& L, const TowerTiles& t, bool dbuf, int H, int W, int A, int depth, int hidden) {
  const int HW = H * W, bpt = az::tower16_boards_per_tile(HW, t.rows), staged = t.staged_floats;
  if (az::tower16_lds_bytes(HW, t.rows, staged, dbuf) > az::kTowerLdsMax) return "lds";
  if (!az::tower16_heads_fit(HW, t.rows, A, hidden, dbuf)) return "heads";
  if (staged != L.blob.floats && staged != L.blob.off_wv1 && staged != L.blob.off_wpd) return "prefix";
  if (t.wv1_lds != (staged == L.blob.floats) || t.wpd_lds != (staged >= L.blob.off_wv1)) return "staging flags";
  if (t.wv1_lds && !t.wpd_lds) return "wv1 without wpd";
  const double flop = t.issued_flop_per_board, natural = natural_flop(t, HW, depth);
  if (t.slot_pix.empty()) return t.skip[0] || t.skip[1] ? "skips without a plan" : flop != natural ? "flop" : "";
  if ((int)t.slot_pix.size() != t.rows) return "plan size";
  std::vector<int> seen(bpt * HW, 0);  // every pixel of the tile's boards once, every other slot an empty word
  for (int v : t.slot_pix) {
    const int b = v >> 16, y = (v >> 8) & 255, x = v & 255;
    if (y != 127 && (b < 0 || b >= bpt || y >= H || x >= W || seen[b * HW + y * W + x]++)) return "plan pixel";
  }
  for (int c : seen)
    if (!c) return "plan misses a pixel";
  return flop < natural ? "" : "flop";
}

int sweep() {
  int shapes = 0;
  std::string not_ok, failures;
  for (int H = 2; H <= 64; ++H)
    for (int W = 2; H * W <= 128; ++W)
      for (int A : {W, H * W})
        for (int depth : {1, 4, 16})
          for (int hidden : {1, 64, 255, 256}) {
            const TowerLayout L = layout_of(H, W, A, depth, hidden);
            char at[96];
            ++shapes;
            snprintf(at, sizeof at, "[%d, %d, %d, %d, %d", H, W, A, depth, hidden);
            auto add = [&](std::string& list, const std::string& end) { list += (list.empty() ? "" : ", ") + (at + end); };
            std::string fault = L.ok ? fault_of(L, L.main, L.dbuf, H, W, A, depth, hidden) : "";
            if (fault.empty() && L.alt.rows) fault = fault_of(L, L.alt, true, H, W, A, depth, hidden);
            if (!L.ok) add(not_ok, "]");
            if (!fault.empty()) add(failures, ", \"" + fault + "\"]");
          }
  printf("{\"shapes\": %d, \"not_ok\": [%s], \"failures\": [%s]}\n", shapes, not_ok.c_str(), failures.c_str());
  return 0;
}

// the chess network's layout (TowerShape::rows_stem, H = W = 8, A = 1880): the heads' dense layers run in
// kernels of their own, so the staged prefix ends before bpd and tower16_heads_fit does not apply
int rows_stem(int argc, char** argv) {
  printf("[");
  for (int a = 2; a + 1 < argc; a += 2) {
    az::TowerShape s;
    s.H = s.W = 8, s.A = 1880, s.depth = atoi(argv[a]), s.hidden = atoi(argv[a + 1]), s.cus = 256, s.lanes = 1;
    s.rows_stem = true;
    const TowerLayout L = az::tower16_choose_layout(s);
    printf("%s{\"depth\": %d, \"hidden\": %d, \"tower\": %d", a > 2 ? ",\n" : "", s.depth, s.hidden, (int)L.ok);
    if (L.ok) {
      const TowerTiles& t = L.main;
      const int k = __builtin_popcount(t.skip[0]) + __builtin_popcount(t.skip[1]);
      printf(", \"tile_rows\": %d, \"boards\": %d, \"dbuf\": %d, \"staged\": %d, \"off_bpd\": %d, \"lds_bytes\": %zu, "
             "\"lds_bytes_in_place\": %zu, \"dual\": %d, \"skipped\": %d, \"flop\": %.17g, \"flop_chunks2\": %.17g, "
             "\"flop_chunks4\": %.17g",
             t.rows, az::tower16_boards_per_tile(64, t.rows), (int)L.dbuf, t.staged_floats, L.blob.off_bpd,
             az::tower16_lds_bytes(64, t.rows, t.staged_floats, L.dbuf),
             az::tower16_lds_bytes(64, t.rows, t.staged_floats, false), (int)(L.alt.rows != 0), k,
             t.issued_flop_per_board, az::tower16_issued_flop_per_board(64, t.rows, s.depth, t.skip, true, 2),
             az::tower16_issued_flop_per_board(64, t.rows, s.depth, t.skip, true, 4));
    }
    printf("}");
  }
  printf("]\n");
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "--sweep")) return sweep();
  if (argc >= 2 && !strcmp(argv[1], "--rows-stem")) {
    if (argc % 2) {
      fprintf(stderr, "usage: tower_layout_check --rows-stem (depth hidden)...\n");
      return 2;
    }
    return rows_stem(argc, argv);
  }
  if ((argc - 1) % 5) {
    fprintf(stderr, "usage: tower_layout_check (H W A depth hidden)... | --sweep | --rows-stem (depth hidden)...\n");
    return 2;
  }
  printf("[");
  for (int a = 1; a + 4 < argc; a += 5) {
    const int H = atoi(argv[a]), W = atoi(argv[a + 1]), A = atoi(argv[a + 2]), depth = atoi(argv[a + 3]),
              hidden = atoi(argv[a + 4]), HW = H * W;
    const TowerLayout L = layout_of(H, W, A, depth, hidden);
    printf("%s{\"H\": %d, \"W\": %d, \"A\": %d, \"depth\": %d, \"hidden\": %d, \"tower\": %d", a > 1 ? ",\n" : "", H, W, A,
           depth, hidden, (int)L.ok);
    if (L.ok) {
      const int bpt = az::tower16_boards_per_tile(HW, L.main.rows);
      printf(", \"tile_rows\": %d, \"boards\": %d, \"pads\": %d, \"dbuf\": %d", L.main.rows, bpt, L.main.rows - bpt * HW,
             (int)L.dbuf);
      print_tiles(L.main, "", L.wv1_xtile, HW, depth);
      printf(", \"dual\": %d", (int)(L.alt.rows != 0));
      // (the X-tile DMA of wv1 is the main tiles' alone: the alt tiles have it staged or from L2)
      if (L.alt.rows) print_tiles(L.alt, "alt_", false, HW, depth);
    }
    printf("}");
  }
  printf("]\n");
  return 0;
}
