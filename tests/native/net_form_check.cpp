// States the form a network's forward gets: what the library's own rule
// az::plan_network (csrc/az_net_form.h; the function both engines' create
// calls, load_network and the stats read) answers, with libaz.so's chooser
// behind it.  CUs and lanes are fixed (256, 1), the evaluator is the network.
// argv: groups of conv_algo in_ch H W A depth hidden -> one JSON object per
// group: status, message, form, terms, and whether the plan carries a layout.
// --sweep: tower_layout_check --sweep's Connect-N shapes under AZ_CONV_F16X2 ->
// {"shapes", "not_ok": [shapes whose form is not the tower], "failures":
// [shape + what]}: the form is the tower exactly where the chooser says ok
// (else the per-layer form of the board's width, with an all-default layout),
// and the plan's layout is the chooser's.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "az_net_form.h"

namespace {
const char* form_name(az::NetForm f) {
  switch (f) {
    case az::NetForm::kDirect: return "direct";
    case az::NetForm::kLayers16: return "layers16";
    case az::NetForm::kTower: return "tower";
    case az::NetForm::kTowerRows: return "tower_rows";
  }
  return "?";
}

bool same_tiles(const az::TowerTiles& a, const az::TowerTiles& b) {
  return a.rows == b.rows && a.staged_floats == b.staged_floats && a.wpd_lds == b.wpd_lds && a.wv1_lds == b.wv1_lds &&
         a.slot_pix == b.slot_pix && a.skip[0] == b.skip[0] && a.skip[1] == b.skip[1] &&
         a.issued_flop_per_board == b.issued_flop_per_board;
}
bool same_layout(const az::TowerLayout& a, const az::TowerLayout& b) {
  return a.ok == b.ok && a.dbuf == b.dbuf && a.wv1_xtile == b.wv1_xtile && a.blob.floats == b.blob.floats &&
         a.blob.off_wpd == b.blob.off_wpd && a.blob.off_wv1 == b.blob.off_wv1 && same_tiles(a.main, b.main) &&
         same_tiles(a.alt, b.alt) && a.alt_max_boards == b.alt_max_boards;
}

int sweep() {
  int shapes = 0;
  std::string not_ok, failures;
  for (int H = 2; H <= 64; ++H)
    for (int W = 2; H * W <= 128; ++W)
      for (int A : {W, H * W})
        for (int depth : {1, 4, 16})
          for (int hidden : {1, 64, 255, 256}) {
            az::NetRequest r;
            r.H = H, r.W = W, r.A = A, r.depth = depth, r.hidden = hidden, r.cus = 256, r.lanes = 1;
            az::TowerShape s;
            s.H = H, s.W = W, s.A = A, s.depth = depth, s.hidden = hidden, s.cus = 256, s.lanes = 1;
            const az::NetPlan p = az::plan_network(r);
            const az::TowerLayout L = az::tower16_choose_layout(s);
            char at[96];
            ++shapes;
            snprintf(at, sizeof at, "[%d, %d, %d, %d, %d", H, W, A, depth, hidden);
            auto add = [&](std::string& list, const std::string& end) { list += (list.empty() ? "" : ", ") + (at + end); };
            const bool tower = p.form == az::NetForm::kTower;
            if (!tower) add(not_ok, "]");
            const char* fault = "";
            if (p.status.code != AZ_OK || p.terms != 3) fault = "status";
            else if (tower != L.ok) fault = "form";
            else if (!tower && p.form != (W > 16 ? az::NetForm::kDirect : az::NetForm::kLayers16)) fault = "fallback";
            else if (!same_layout(p.layout, tower ? L : az::TowerLayout{})) fault = "layout";
            if (*fault) add(failures, std::string(", \"") + fault + "\"]");
          }
  printf("{\"shapes\": %d, \"not_ok\": [%s], \"failures\": [%s]}\n", shapes, not_ok.c_str(), failures.c_str());
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "--sweep")) return sweep();
  if ((argc - 1) % 7) {
    fprintf(stderr, "usage: net_form_check (conv_algo in_ch H W A depth hidden)... | --sweep\n");
    return 2;
  }
  printf("[");
  for (int a = 1; a + 6 < argc; a += 7) {
    az::NetRequest r;
    r.conv_algo = atoi(argv[a]), r.in_ch = atoi(argv[a + 1]), r.H = atoi(argv[a + 2]), r.W = atoi(argv[a + 3]);
    r.A = atoi(argv[a + 4]), r.depth = atoi(argv[a + 5]), r.hidden = atoi(argv[a + 6]), r.cus = 256, r.lanes = 1;
    const az::NetPlan p = az::plan_network(r);
    const az::NetStatus early = az::check_net_request(r);
    printf("%s{\"status\": %d, \"message\": \"%s\", \"at_create\": %d, \"form\": \"%s\", \"terms\": %d, \"layout\": %d, "
           "\"tile_rows\": %d, \"flop\": %.17g}",
           a > 1 ? ",\n" : "", p.status.code, p.status.message, (int)(early.code != AZ_OK),
           p.status.code == AZ_OK ? form_name(p.form) : "refused", p.terms, (int)p.layout.ok, p.layout.main.rows,
           az::issued_flop_per_board(p.form, p.terms, p.layout).main);
  }
  printf("]\n");
  return 0;
}
