// az_net_form.h (part of az_nn.h) -- which of its four forms a network's forward runs in, decided
// in one place.  Host only and free of HIP: both engines' create calls (the refusals), load_network
// (the plan), the stats and tests/native/net_form_check.cpp read this one definition.
//
//   Connect-N (4 input planes)                          chess (118 planes, 8x8, 1880 actions)
//   DIRECT, or depth 0             Direct               depth 0, or DIRECT             Direct
//   LAYERS                         Layers16             LAYERS                         Layers16
//   F16X2, 1 <= depth <= 16,                            F16X2, 1 <= depth <= 16,
//     hidden <= 256, a layout      Tower                  a layout (any hidden)        TowerRows
//   F16X2 otherwise                Layers16, or         F16X2 otherwise                Layers16
//                                  Direct if W > 16
//   F16                            Tower, or refused    F16                            TowerRows, or refused
//
// (the per-layer fp16 kernels take boards up to 16 columns, and run the heads' 1x1 convs in the last
// block's conv2: boards wider than that and networks without a block take the fp32 MFMA chain)
#pragma once
#include <utility>

#include "../../include/az.h"
#include "az_tower_layout.h"

namespace az {

enum class NetForm {
  kDirect,     // the per-layer fp32 MFMA chain (conv3x3_mfma_kernel), fp32 activations
  kLayers16,   // the per-layer fp16x2 chain (conv16_kernel), split16 activations
  kTower,      // the whole forward in one launch, on boards (tower16_kernel)
  kTowerRows,  // the stem, the tower and the heads' 1x1 convs in one launch on input rows, then the dense heads
};

struct NetRequest {  // everything the choice depends on; no device, no weights
  int conv_algo = AZ_CONV_F16X2;
  int in_ch = 4;  // input planes: 4 (Connect-N) or 118 (chess, padded to F)
  int H = 0, W = 0, A = 0, depth = 0, hidden = 256;
  bool natural_order = false;     // az_config.tower_natural_order: no slot plan (A/B, bitwise the same)
  int lanes = 1, cus = 1;         // the engine's lanes, the device's CUs: the tower's dual-launch threshold
  bool network_evaluator = true;  // AZ_EVAL_NETWORK: the engine searches with this network
};

struct NetStatus {
  int code = AZ_OK;
  const char* message = "";
};

// whether conv_algo asks for the one-launch tower and the network is one it is built for
// (a layout besides: tower16_choose_layout, which needs the device's CUs -- plan_network)
inline bool tower_possible(const NetRequest& r) {
  return (r.conv_algo == AZ_CONV_F16X2 || r.conv_algo == AZ_CONV_F16) && r.depth >= 1 && r.depth <= kTowerMaxDepth &&
         (r.in_ch > 4 || r.hidden <= 256);
}

// What *_engine_create refuses about the network's form, before it opens a device.
inline NetStatus check_net_request(const NetRequest& r) {
  if (r.conv_algo != AZ_CONV_F16X2 && r.conv_algo != AZ_CONV_DIRECT && r.conv_algo != AZ_CONV_F16X2_LAYERS &&
      r.conv_algo != AZ_CONV_F16)
    return {AZ_E_INVALID, "conv_algo must be AZ_CONV_F16X2, AZ_CONV_DIRECT, AZ_CONV_F16X2_LAYERS or AZ_CONV_F16"};
  // the one-term arithmetic exists on the one-launch tower only: no other form stands in for it
  if (r.conv_algo == AZ_CONV_F16 && !tower_possible(r))
    return {AZ_E_INVALID, r.in_ch > 4
                              ? "AZ_CONV_F16 needs the one-launch tower: 1 <= depth <= 16"
                              : "AZ_CONV_F16 needs the one-launch tower: 1 <= depth <= 16 and value_hidden <= 256"};
  if (r.network_evaluator && r.conv_algo == AZ_CONV_F16X2_LAYERS && r.W > 16)
    return {AZ_E_INVALID, "AZ_CONV_F16X2_LAYERS supports boards up to 16 columns"};
  return {};
}

struct NetPlan {
  NetStatus status;
  NetForm form = NetForm::kDirect;
  int terms = 3;       // fp16 products per MAC on the tower: 3, or 1 (AZ_CONV_F16: the same packs and input
                       // rows, the one-term kernels)
  TowerLayout layout;  // the tower forms': tile heights, staging, slot plans, issued FLOP; all-default otherwise
};

// The form of a network's forward; the library's one caller of tower16_choose_layout.  AZ_CONV_F16X2
// falls back quietly to the same arithmetic per layer (every form within NET_TOL); AZ_CONV_F16 does not.
inline NetPlan plan_network(const NetRequest& r) {
  NetPlan p;
  p.status = check_net_request(r);
  if (p.status.code != AZ_OK) return p;
  p.terms = r.conv_algo == AZ_CONV_F16 ? 1 : 3;
  const bool chess = r.in_ch > 4;
  if (r.depth == 0 || r.conv_algo == AZ_CONV_DIRECT) return p;
  p.form = !chess && r.W > 16 ? NetForm::kDirect : NetForm::kLayers16;  // without a tower
  if (!tower_possible(r)) return p;
  TowerShape s;
  s.H = r.H, s.W = r.W, s.A = r.A, s.depth = r.depth, s.hidden = r.hidden;
  s.rows_stem = chess, s.natural_order = r.natural_order, s.lanes = r.lanes, s.cus = r.cus;
  TowerLayout L = tower16_choose_layout(s);
  if (L.ok) {
    p.form = chess ? NetForm::kTowerRows : NetForm::kTower;
    p.layout = std::move(L);
  } else if (r.conv_algo == AZ_CONV_F16) {
    p.status = {AZ_E_INVALID, "AZ_CONV_F16 needs the one-launch tower, and this network has no layout for it"};
  }
  return p;
}

// MFMA FLOP the forward issues per board (az_stats): the tower's main tiles, and its alt tiles where a
// dual launch has them; 0 for the per-layer forms.  AZ_CONV_F16 issues one of the three products.
struct IssuedFlop {
  double main = 0, alt = 0;
};
inline IssuedFlop issued_flop_per_board(NetForm form, int terms, const TowerLayout& L) {
  if (form != NetForm::kTower && form != NetForm::kTowerRows) return {};
  const int per_mac = terms == 1 ? 3 : 1;
  return {L.main.issued_flop_per_board / per_mac, L.alt.issued_flop_per_board / per_mac};
}

}  // namespace az
