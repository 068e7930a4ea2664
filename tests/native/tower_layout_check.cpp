// States the layout the one-launch tower gets for a network, from libaz.so's
// own host functions (az::tower16_*), walking load_network's order of
// preference (csrc/az_engine.hip): the tile height of the board, double-
// buffered before in place, and per layout the largest staging of the
// small-weight blob that the LDS holds (the whole blob, then without wv1,
// then without wpd too); the wv1 DMA into X's tile; the slot plan; the dual
// launch's 96-row tiles with a staging and a plan of their own.
//
// Two things cannot be read from the library and are restated here: the
// blob's three prefixes (load_network's `put` order, every part padded to a
// multiple of four floats) and the LDS budget kTowerLdsMax (csrc/az_nn.h).
// tests/test_forward_layouts_gpu.py pins what the restatement leads to -- tile
// rows, boards per tile and the plan's skips -- against the engine's own
// issued_flop_per_board.
//
// argv: groups of H W A depth hidden.  One JSON object per group on stdout.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace az {
void tower16_slot_plan(int H, int W, int tile_rows, std::vector<int>& slot_pix, int skip[2]);
double tower16_issued_flop_per_board(int HW, int tile_rows, int depth, const int skip[2], bool rows_stem,
                                     int stem_chunks);
int tower16_tile_rows(int HW);
int tower16_boards_per_tile(int HW, int tile_rows);
size_t tower16_lds_bytes(int HW, int tile_rows, int staged_floats, bool dbuf);
bool tower16_heads_fit(int HW, int tile_rows, int A, int hidden, bool dbuf);
bool tower16_wv1_xtile_fits(int HW, int tile_rows, int hidden);
}  // namespace az

namespace {
const size_t kLdsMax = 160 * 1024;  // csrc/az_nn.h kTowerLdsMax
const int F = 128;

int pad4(int n) { return (n + 3) & ~3; }

struct Plan {
  const char* form;
  int skipped;  // block-taps over both M halves
  double flop, flop_natural;
};

Plan plan_of(int H, int W, int tr, int depth) {
  std::vector<int> pix;
  int skip[2] = {0, 0};
  const int none[2] = {0, 0};
  az::tower16_slot_plan(H, W, tr, pix, skip);
  if (pix.empty()) skip[0] = skip[1] = 0;  // load_network uploads no plan: natural order
  int skipped = 0;
  for (int h = 0; h < 2; ++h) skipped += __builtin_popcount(skip[h]);
  // four border blocks (top, bottom | left, right) skip 3 taps each, top | bottom alone 6
  const char* form = pix.empty() ? "none" : skipped == 12 ? "four_borders" : skipped == 6 ? "top_bottom" : "other";
  return {form, skipped, az::tower16_issued_flop_per_board(H * W, tr, depth, skip, false, 2),
          az::tower16_issued_flop_per_board(H * W, tr, depth, none, false, 2)};
}
}  // namespace

int main(int argc, char** argv) {
  if ((argc - 1) % 5) {
    fprintf(stderr, "usage: tower_layout_check (H W A depth hidden)...\n");
    return 2;
  }
  printf("[");
  for (int a = 1; a + 4 < argc; a += 5) {
    const int H = atoi(argv[a]), W = atoi(argv[a + 1]), A = atoi(argv[a + 2]), depth = atoi(argv[a + 3]),
              hidden = atoi(argv[a + 4]), HW = H * W;
    // the blob (load_network): b1, b2 [depth][F], stem bias [F], wpc [F][2], wvc [F], hb [4], bpd [A],
    // bv1 [hidden], wv2 [hidden], then wpd [2HW][A] and wv1 [HW][hidden]
    const int off_wpd = 2 * pad4(depth * F) + pad4(F) + pad4(2 * F) + pad4(F) + 4 + pad4(A) + 2 * pad4(hidden);
    const int off_wv1 = off_wpd + pad4(2 * HW * A), blob = off_wv1 + pad4(HW * hidden);
    const int prefix[3] = {blob, off_wv1, off_wpd};
    const int tr = az::tower16_tile_rows(HW);
    bool found = false, db = false;
    int staged = -1;
    if (depth >= 1 && depth <= 16 && hidden <= 256)  // az_engine_create: use_tower
      for (int li = 0; li < 2 && !found; ++li) {
        const bool d = li == 0;
        if (!tr || !az::tower16_heads_fit(HW, tr, A, hidden, d)) continue;
        for (int i = 0; i < 3 && !found; ++i)
          if (az::tower16_lds_bytes(HW, tr, prefix[i], d) <= kLdsMax) {
            found = true;
            db = d;
            staged = i;
          }
      }
    printf("%s{\"H\": %d, \"W\": %d, \"A\": %d, \"depth\": %d, \"hidden\": %d, \"tower\": %d", a > 1 ? ",\n" : "", H, W, A,
           depth, hidden, (int)found);
    if (found) {
      const int bpt = az::tower16_boards_per_tile(HW, tr);
      const bool xtile = db && staged != 0 && az::tower16_wv1_xtile_fits(HW, tr, hidden);
      const Plan p = plan_of(H, W, tr, depth);
      printf(", \"tile_rows\": %d, \"boards\": %d, \"pads\": %d, \"dbuf\": %d, \"wv1\": \"%s\", \"wpd\": \"%s\", "
             "\"plan\": \"%s\", \"skipped\": %d, \"flop\": %.17g, \"flop_natural\": %.17g",
             tr, bpt, tr - bpt * HW, (int)db, staged == 0 ? "lds" : xtile ? "xtile" : "l2", staged <= 1 ? "lds" : "l2",
             p.form, p.skipped, p.flop, p.flop_natural);
      const bool dual = tr == 128 && db && bpt == 3 && az::tower16_boards_per_tile(HW, 96) == 2 &&
                        az::tower16_heads_fit(HW, 96, A, hidden, true);
      printf(", \"dual\": %d", (int)dual);
      if (dual) {
        int alt = -1;
        for (int i = 0; i < 3 && alt < 0; ++i)
          if (az::tower16_lds_bytes(HW, 96, prefix[i], true) <= kLdsMax) alt = i;
        const Plan q = plan_of(H, W, 96, depth);
        // (the X-tile DMA of wv1 is the primary tile height's alone: here staged or from L2)
        printf(", \"alt_wv1\": \"%s\", \"alt_wpd\": \"%s\", \"alt_plan\": \"%s\", \"alt_skipped\": %d, "
               "\"alt_flop\": %.17g, \"alt_flop_natural\": %.17g",
               alt < 0 ? "none" : alt == 0 ? "lds" : "l2", alt < 0 ? "none" : alt <= 1 ? "lds" : "l2", q.form, q.skipped,
               q.flop, q.flop_natural);
      }
    }
    printf("}");
  }
  printf("]\n");
  return 0;
}
