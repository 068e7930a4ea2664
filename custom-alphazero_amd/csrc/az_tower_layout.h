// az_tower_layout.h (part of az_nn.h) -- how the one-launch tower (az_tower16.hip) is laid out for
// a network: tile heights, LDS staging, slot plans.  Host only and free of HIP: load_network, the
// launchers, the stats and tests/native/tower_layout_check.cpp read this one definition.
#pragma once
#include <cstddef>
#include <vector>

namespace az {

constexpr int kTowerMaxDepth = 16;   // residual blocks
constexpr int kTowerMaxBoards = 8;   // boards per workgroup tile
constexpr size_t kTowerLdsMax = 160 * 1024;

struct TowerShape {  // everything the choice depends on; no device, no weights
  int H = 0, W = 0, A = 0, depth = 0, hidden = 0;
  bool rows_stem = false;      // chess: the input-row stem, no dense heads in the kernel
  bool natural_order = false;  // az_config.tower_natural_order: no slot plan
  int lanes = 1, cus = 1;      // a dual launch's threshold: 2 * max(1, cus / max(1, lanes)) boards
};
struct TowerBlob {  // TowerNet::blob from sizes alone: its parts' offsets (floats, multiples of 4) in order, its size
  int off_b1 = 0, off_b2 = 0, off_stemb = 0, off_wpc = 0, off_wvc = 0, off_hb = 0, off_bpd = 0, off_bv1 = 0,
      off_wv2 = 0, off_wpd = 0, off_wv1 = 0, floats = 0;
};
struct TowerTiles {  // one tile height
  int rows = 0;                // pixel rows per workgroup tile: 96, 128 or 192 (0: none)
  int staged_floats = 0;       // the blob prefix copied into LDS: the largest of three that fits
  bool wpd_lds = false, wv1_lds = false;  // whether that prefix holds the policy dense / value dense1
  std::vector<int> slot_pix;   // the slot plan (tower16_slot_plan); empty: natural order, no skips
  int skip[2] = {0, 0};
  double issued_flop_per_board = 0;  // tower16_issued_flop_per_board of this height and plan (az_stats)
};
struct TowerLayout {
  bool ok = false;         // false: the network does not fit the tower (the per-layer kernels instead)
  bool dbuf = false;       // two activation tiles (else one, updated in place)
  bool wv1_xtile = false;  // wv1 not staged, but DMA'd behind the heads' partials in X's tile (main tiles)
  TowerBlob blob;
  // main: the board's tile height.  alt (rows == 0: none): the dual launch's shorter tiles, run by
  // launches of at most alt_max_boards live boards
  TowerTiles main, alt;
  int alt_max_boards = -1;
};
TowerBlob tower16_blob_offsets(int depth, int HW, int A, int hidden);
// The layout of a network, in order of preference: the board's tile height double-buffered, then
// in place; per form the largest staging the LDS holds (the whole blob, then without wv1, then
// without wpd too).  Calls no HIP API.
TowerLayout tower16_choose_layout(const TowerShape& s);

// the slot plan of a 192-, 128- or 96-row tile: border blocks (16 slots whose pixels all sit on
// one board edge) skip the three taps that read past that edge; empty when no plan applies
void tower16_slot_plan(int H, int W, int tile_rows, std::vector<int>& slot_pix, int skip[2]);
// MFMA FLOP tower16_kernel issues per board: a full tile's stem + 2 depth
// convs (+ the 1x1 projection k-steps) less the plan's skipped taps, / boards
// (rows_stem: the input-row stem, stem_chunks of its 4 input chunks computed)
double tower16_issued_flop_per_board(int HW, int tile_rows, int depth, const int skip[2], bool rows_stem = false,
                                     int stem_chunks = 4);
// 0 when the board does not fit a tile (HW > 128); 192 for boards of 65-96 pixels (12 M blocks,
// a wave 96 rows x 32 channels: half the weight stream per board; in place only); else 96 or 128
int tower16_tile_rows(int HW);
int tower16_boards_per_tile(int HW, int tile_rows);
// LDS of one workgroup: activation rows (one or two tiles + zero rows) +
// bookkeeping + staged blob floats
size_t tower16_lds_bytes(int HW, int tile_rows, int staged_floats, bool dbuf);
// whether the heads' scratch (features, logits, partials) fits the tiles
bool tower16_heads_fit(int HW, int tile_rows, int A, int hidden, bool dbuf);
// whether wv1 [HW][hidden] fits X's tile behind the heads' partials (dbuf)
bool tower16_wv1_xtile_fits(int HW, int tile_rows, int hidden);

}  // namespace az
