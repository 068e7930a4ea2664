// Host build of the best-edge choice (csrc/az_device.h: select_key,
// select_edge, select_merge), test infrastructure for
// tests/test_select_order_cpu.py.  The same functions the descents call are
// run over simulated lanes, the partner steps applied in the kernels' order:
//   serial   az_tree.hip select_body: one loop over the node's edges
//   group L  az_tree.hip select_group_body, L = 8, 16, 32, 64: lane j holds
//            edge j (lanes past the count hold "no edge"), then steps
//            xor 1, xor 2, half-mirror of 8, mirror of 16, xor 16, xor 32
//            (group_partner<K>), the first log2(L) of them
//   chess    az_chess_mcts.hip select_slot: 64 lanes, lane l loops over edges
//            l, l + 64, ..., then the butterfly xor 32, 16, 8, 4, 2, 1
// select_check FILE: records of i32 cnt, then cnt f64 (little endian).  One
// line per record: "<serial> <g8> <g16> <g32> <g64> <chess> <agree>", each
// the index lane 0 ends with (-1: the count does not fit the group), agree 1
// when every lane of every form ended with its lane 0's index.  The test
// computes what it expects with numpy.
#include <stdio.h>

#include <vector>

#include "../../custom-alphazero_amd/csrc/az_device.h"

namespace {

int partner(int k, int i) {
  switch (k) {
    case 0: return i ^ 1;
    case 1: return i ^ 2;
    case 2: return (i & ~7) | (7 - (i & 7));
    case 3: return (i & ~15) | (15 - (i & 15));
    case 4: return i ^ 16;
    default: return i ^ 32;
  }
}

// every lane steps at once, as a wave does: the partners' values are the ones before the step
void step(std::vector<az::SelectBest>& lanes, int (*other)(int, int), int k) {
  const std::vector<az::SelectBest> before = lanes;
  for (size_t i = 0; i < lanes.size(); ++i) {
    const az::SelectBest o = before[(size_t)other(k, (int)i)];
    lanes[i] = az::select_merge(before[i], o.key, o.idx);
  }
}

int settle(const std::vector<az::SelectBest>& lanes, bool* agree) {
  for (const az::SelectBest& l : lanes)
    if (l.idx != lanes[0].idx || l.key != lanes[0].key) *agree = false;
  return lanes[0].idx;
}

int group(const double* v, int cnt, int L, bool* agree) {
  if (cnt > L) return -1;
  std::vector<az::SelectBest> lanes((size_t)L, az::select_none());
  for (int j = 0; j < cnt; ++j) lanes[(size_t)j] = az::select_edge(az::select_none(), v[j], j);
  for (int k = 0; (1 << k) < L; ++k) step(lanes, partner, k);
  return settle(lanes, agree);
}

int xor_partner(int off, int i) { return i ^ off; }

int chess(const double* v, int cnt, bool* agree) {
  std::vector<az::SelectBest> lanes(64, az::select_none());
  for (int l = 0; l < 64; ++l)
    for (int j = l; j < cnt; j += 64) lanes[(size_t)l] = az::select_edge(lanes[(size_t)l], v[j], j);
  for (int off = 32; off > 0; off >>= 1) step(lanes, xor_partner, off);
  return settle(lanes, agree);
}

int serial(const double* v, int cnt) {
  az::SelectBest sel = az::select_none();
  for (int i = 0; i < cnt; ++i) sel = az::select_edge(sel, v[i], i);
  return sel.idx;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t cnt;
  std::vector<double> v;
  while (fread(&cnt, sizeof(cnt), 1, f) == 1) {
    if (cnt < 1 || cnt > 256) return 3;
    v.resize((size_t)cnt);
    if (fread(v.data(), sizeof(double), (size_t)cnt, f) != (size_t)cnt) return 3;
    bool agree = true;
    const int s = serial(v.data(), cnt);
    const int g8 = group(v.data(), cnt, 8, &agree), g16 = group(v.data(), cnt, 16, &agree);
    const int g32 = group(v.data(), cnt, 32, &agree), g64 = group(v.data(), cnt, 64, &agree);
    const int c = chess(v.data(), cnt, &agree);
    printf("%d %d %d %d %d %d %d\n", s, g8, g16, g32, g64, c, (int)agree);
  }
  fclose(f);
  return 0;
}
