// az_net_load.hip -- a network's weights from the caller's tensors to the device: BatchNorm folded
// into the convs (in host doubles: built with -ffp-contract=off, the fold's bits are part of every
// forward output), the folded weights packed for each kernel family, and the one-launch tower's
// view of them for the form plan_network (az_net_form.h) names.  Both engines load through here.
#include <math.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/az.h"
#include "az_host.h"
#include "az_nn.h"

namespace {

constexpr auto& fail = az::fail_abi;

// ------------------------------------------------------------ weight folding
int fetch(const std::map<std::string, const az_tensor*>& m, const std::string& name,
          int64_t numel, std::vector<double>& out) {
  auto it = m.find(name);
  if (it == m.end()) return fail(AZ_E_INVALID, "missing weight tensor '" + name + "'");
  const az_tensor* t = it->second;
  if (t->numel != numel)
    return fail(AZ_E_INVALID, "weight '" + name + "' has " + std::to_string(t->numel) +
                                  " elements, expected " + std::to_string(numel));
  std::vector<float> tmp(numel);
  if (t->on_device) {
    AZ_HIP(hipMemcpy(tmp.data(), t->data, numel * sizeof(float), hipMemcpyDeviceToHost));
  } else {
    memcpy(tmp.data(), t->data, numel * sizeof(float));
  }
  out.assign(tmp.begin(), tmp.end());
  return 0;
}

// InnerConvBlock (base_layers.py:20-66): conv kernel [kh][kw][cin][cout] +
// bias, BatchNorm(gamma, beta, moving mean/var).  Returns the folded kernel in
// Keras layout (double) and folded bias.
int fold_unit(const std::map<std::string, const az_tensor*>& m, const std::string& u, int kk,
              int cin, int cout, double eps, std::vector<double>& w, std::vector<double>& b) {
  std::vector<double> gamma, beta, mean, var;
  int rc;
  if ((rc = fetch(m, u + ".kernel", (int64_t)kk * kk * cin * cout, w))) return rc;
  if ((rc = fetch(m, u + ".bias", cout, b))) return rc;
  if ((rc = fetch(m, u + ".gamma", cout, gamma))) return rc;
  if ((rc = fetch(m, u + ".beta", cout, beta))) return rc;
  if ((rc = fetch(m, u + ".mean", cout, mean))) return rc;
  if ((rc = fetch(m, u + ".var", cout, var))) return rc;
  for (int n = 0; n < cout; ++n) {
    const double sc = gamma[n] / sqrt(var[n] + eps);
    for (int i = 0; i < kk * kk * cin; ++i) w[(size_t)i * cout + n] *= sc;
    b[n] = (b[n] - mean[n]) * sc + beta[n];
  }
  return 0;
}

// [n][K] (K contiguous) -> MFMA fragment order of conv3x3_mfma_kernel:
// float4 index ((c*4 + tile)*4 + q)*64 + lane holds W[k][n] for
// k = 32c + 16*(lane>>5) + 4q + e (e = 0..3), n = 32*tile + (lane&31).
std::vector<float> pack_fragments(const std::vector<float>& wt, int N, int K) {
  std::vector<float> p((size_t)N * K);
  const int chunks = K / 32, tiles = N / 32;
  for (int c = 0; c < chunks; ++c)
    for (int t = 0; t < tiles; ++t)
      for (int q = 0; q < 4; ++q)
        for (int lane = 0; lane < 64; ++lane)
          for (int e = 0; e < 4; ++e) {
            const int k = 32 * c + 16 * (lane >> 5) + 4 * q + e;
            const int n = 32 * t + (lane & 31);
            p[((((size_t)c * tiles + t) * 4 + q) * 64 + lane) * 4 + e] = wt[(size_t)n * K + k];
          }
  return p;
}

// a host array into device memory that `owned` frees
template <typename T>
int upload_new(az::DeviceAllocs& owned, T** dst, const std::vector<T>& src) {
  AZ_TRY(owned.alloc(dst, src.size(), false));
  AZ_HIP(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}

// conv16_kernel pack (az_conv16.hip) of a folded 3x3 conv [3][3][cin][F] (+ the
// 1x1 residual [F][F]): fp16 bits, uploaded as raw storage; *scale = 2^(e-12)
int upload_conv16(az::DeviceAllocs& owned, uint16_t** dst, float* scale, const std::vector<double>& w3, int cin,
                  const std::vector<double>* wr) {
  const int e = az::conv16_prescale(w3.data(), w3.size(), wr ? wr->data() : nullptr, wr ? wr->size() : 0);
  std::vector<uint16_t> pack;
  az::conv16_pack(w3.data(), cin, wr ? wr->data() : nullptr, e, pack);
  *scale = std::ldexp(1.f, e - 12);
  return upload_new(owned, dst, pack);
}

// (a set tensor keeps its buffer: az_engine_set_weights again)
int upload(az::DeviceAllocs& owned, float** dst, const std::vector<float>& src) {
  if (!*dst) AZ_TRY(owned.alloc(dst, src.size(), false));
  AZ_HIP(hipMemcpy(*dst, src.data(), src.size() * sizeof(float), hipMemcpyHostToDevice));
  return 0;
}

// The network folded (BatchNorm into conv) on the host: kernels in Keras
// layout and biases, in double.
struct FoldedUnit {
  std::vector<double> w, b;
};
struct FoldedNet {
  FoldedUnit stem;  // [3][3][in_ch][F]
  struct Block {
    FoldedUnit conv1, conv2, res;  // [3][3][F][F] twice, the 1x1 projection [F][F]
  };
  std::vector<Block> blocks;
  FoldedUnit pc, vc;      // head 1x1 convs: policy [F][2], value [F][1]
  FoldedUnit pd, v1, v2;  // dense (no BatchNorm): policy [2HW][A], value [HW][hidden], [hidden][1]
};

int fold_network(const std::map<std::string, const az_tensor*>& m, int in_ch, int depth, int HW, int A, int hidden,
                 double eps, FoldedNet& f) {
  const int F = 128;
  const int64_t K = 2 * HW;
  AZ_TRY(fold_unit(m, "stem", 3, in_ch, F, eps, f.stem.w, f.stem.b));
  f.blocks.resize(depth);
  for (int d = 0; d < depth; ++d) {
    const std::string p = "block" + std::to_string(d);
    FoldedNet::Block& k = f.blocks[d];
    AZ_TRY(fold_unit(m, p + ".conv1", 3, F, F, eps, k.conv1.w, k.conv1.b));
    AZ_TRY(fold_unit(m, p + ".conv2", 3, F, F, eps, k.conv2.w, k.conv2.b));
    AZ_TRY(fold_unit(m, p + ".res", 1, F, F, eps, k.res.w, k.res.b));
  }
  AZ_TRY(fold_unit(m, "policy.conv", 1, F, 2, eps, f.pc.w, f.pc.b));
  AZ_TRY(fold_unit(m, "value.conv", 1, F, 1, eps, f.vc.w, f.vc.b));
  AZ_TRY(fetch(m, "policy.dense.kernel", K * A, f.pd.w));
  AZ_TRY(fetch(m, "policy.dense.bias", A, f.pd.b));
  AZ_TRY(fetch(m, "value.dense1.kernel", (int64_t)HW * hidden, f.v1.w));
  AZ_TRY(fetch(m, "value.dense1.bias", hidden, f.v1.b));
  AZ_TRY(fetch(m, "value.dense2.kernel", hidden, f.v2.w));
  return fetch(m, "value.dense2.bias", 1, f.v2.b);
}

std::vector<float> to_float(const std::vector<double>& v) { return {v.begin(), v.end()}; }

// a block's 3x3 conv (+ its 1x1 residual), uploaded in this order: the direct kernel's fragments of
// [F][9F] (with the residual [F][10F]), the conv16 pack, the folded bias (+ the residual's)
int upload_block_conv(az::DeviceAllocs& owned, const FoldedUnit& c, const FoldedUnit* res, float** frag,
                      uint16_t** pack, float* scale, float** bias) {
  const int F = 128, K = (res ? 10 : 9) * F;
  std::vector<float> wt((size_t)F * K), bt(F);
  for (int n = 0; n < F; ++n) {
    for (int k = 0; k < 9 * F; ++k) wt[(size_t)n * K + k] = (float)c.w[(size_t)k * F + n];
    for (int ch = 0; res && ch < F; ++ch) wt[(size_t)n * K + 9 * F + ch] = (float)res->w[(size_t)ch * F + n];
    bt[n] = (float)(res ? c.b[n] + res->b[n] : c.b[n]);
  }
  AZ_TRY(upload(owned, frag, pack_fragments(wt, F, K)));
  AZ_TRY(upload_conv16(owned, pack, scale, c.w, F, res ? &res->w : nullptr));
  return upload(owned, bias, bt);
}

// the per-layer kernels' buffers (both conv algorithms; the tower reads the conv16 packs too)
int upload_layers(az::NetDev& net, const FoldedNet& f, az::DeviceAllocs& owned) {
  const int F = 128, in_ch = net.req.in_ch, HW = net.req.H * net.req.W, A = net.req.A;
  AZ_TRY(upload(owned, &net.stem_b, to_float(f.stem.b)));
  if (in_ch == 4) {  // [3][3][4][F]: Keras order == [tap*4 + c][F]
    AZ_TRY(upload(owned, &net.stem_w, to_float(f.stem.w)));
  } else {  // [3][3][in_ch][F]: the conv16 pack pads the channels; direct: [3][3][F][F] zero-padded
    AZ_TRY(upload_conv16(owned, &net.stem_k, &net.stem_scale, f.stem.w, in_ch, nullptr));
    std::vector<float> wt((size_t)F * 9 * F, 0.f);
    for (int tap = 0; tap < 9; ++tap)
      for (int c = 0; c < in_ch; ++c)
        for (int o = 0; o < F; ++o)
          wt[(size_t)o * 9 * F + tap * F + c] = (float)f.stem.w[((size_t)tap * in_ch + c) * F + o];
    AZ_TRY(upload(owned, &net.stem_d, pack_fragments(wt, F, 9 * F)));
  }
  const int depth = (int)f.blocks.size();
  for (auto* v : {&net.c1_w, &net.c1_b, &net.c2_w, &net.c2_b}) v->assign(depth, nullptr);
  for (auto* v : {&net.k1, &net.k2}) v->assign(depth, nullptr);
  for (auto* v : {&net.k1_scale, &net.k2_scale}) v->assign(depth, 1.f);
  for (int d = 0; d < depth; ++d) {
    const FoldedNet::Block& k = f.blocks[d];
    AZ_TRY(upload_block_conv(owned, k.conv1, nullptr, &net.c1_w[d], &net.k1[d], &net.k1_scale[d], &net.c1_b[d]));
    AZ_TRY(upload_block_conv(owned, k.conv2, &k.res, &net.c2_w[d], &net.k2[d], &net.k2_scale[d], &net.c2_b[d]));
  }
  AZ_TRY(upload(owned, &net.pc_w, to_float(f.pc.w)));
  AZ_TRY(upload(owned, &net.pc_b, to_float(f.pc.b)));
  AZ_TRY(upload(owned, &net.vc_w, to_float(f.vc.w)));
  AZ_TRY(upload(owned, &net.vc_b, to_float(f.vc.b)));
  const std::vector<float> pdw = to_float(f.pd.w);
  AZ_TRY(upload(owned, &net.pd_w, pdw));
  AZ_TRY(upload(owned, &net.pd_b, to_float(f.pd.b)));
  if (A > az::kMaxActions) {
    const int K = 2 * HW, tiles = (A + 63) / 64;
    std::vector<float> t((size_t)tiles * K * 64, 0.f);
    for (int k = 0; k < K; ++k)
      for (int o = 0; o < A; ++o) t[((size_t)(o / 64) * K + k) * 64 + (o % 64)] = pdw[(size_t)k * A + o];
    AZ_TRY(upload(owned, &net.pd_wt, t));
  }
  AZ_TRY(upload(owned, &net.v1_w, to_float(f.v1.w)));
  AZ_TRY(upload(owned, &net.v1_b, to_float(f.v1.b)));
  AZ_TRY(upload(owned, &net.v2_w, to_float(f.v2.w)));
  return upload(owned, &net.v2_b, to_float(f.v2.b));
}

// the tower's small-weight blob (TowerNet::blob) in the order and at the offsets tower16_blob_offsets states
int tower_blob(const FoldedNet& f, const az::TowerBlob& at, std::vector<float>& blob) {
  bool drift = false;
  auto put = [&](int off, const std::vector<float>& v) {
    drift = drift || off != (int)blob.size();
    blob.insert(blob.end(), v.begin(), v.end());
    while (blob.size() % 4) blob.push_back(0.f);
  };
  std::vector<float> b1, b2;
  for (const FoldedNet::Block& k : f.blocks)
    for (size_t i = 0; i < k.conv1.b.size(); ++i) {
      b1.push_back((float)k.conv1.b[i]);
      b2.push_back((float)(k.conv2.b[i] + k.res.b[i]));
    }
  put(at.off_b1, b1);
  put(at.off_b2, b2);
  put(at.off_stemb, to_float(f.stem.b));
  put(at.off_wpc, to_float(f.pc.w));
  put(at.off_wvc, to_float(f.vc.w));
  put(at.off_hb, {(float)f.pc.b[0], (float)f.pc.b[1], (float)f.vc.b[0], (float)f.v2.b[0]});
  put(at.off_bpd, to_float(f.pd.b));
  put(at.off_bv1, to_float(f.v1.b));
  put(at.off_wv2, to_float(f.v2.w));
  put(at.off_wpd, to_float(f.pd.w));
  put(at.off_wv1, to_float(f.v1.w));
  if (drift || (int)blob.size() != at.floats)
    return fail(AZ_E_STATE, "internal: the tower's blob and tower16_blob_offsets disagree");
  return 0;
}

// The one place that writes TowerNet's layout fields: the layout, the blob
// and the slot plans uploaded, the device view filled from them.
int upload_tower(az::NetDev& net, const az::TowerLayout& L, const FoldedNet& f, bool rows_stem,
                 az::DeviceAllocs& owned) {
  const int depth = net.req.depth;
  az::TowerNet tn{};
  tn.stem_s = 1.f;
  if (!rows_stem) {  // the 4-plane stem as a pack of its own; the input-row form reads the conv16 pack stem_k
    const int e = az::conv16_prescale(f.stem.w.data(), f.stem.w.size(), nullptr, 0);
    std::vector<uint16_t> pack;
    az::tower16_stem_pack(f.stem.w.data(), e, pack);
    uint16_t* stem16 = nullptr;
    AZ_TRY(upload_new(owned, &stem16, pack));
    tn.stem16 = reinterpret_cast<const uint4*>(stem16);
    tn.stem_s = std::ldexp(1.f, e - 12);
  }
  for (int d = 0; d < depth; ++d) {
    tn.k1[d] = reinterpret_cast<const uint4*>(net.k1[d]);
    tn.k2[d] = reinterpret_cast<const uint4*>(net.k2[d]);
    tn.s1[d] = net.k1_scale[d];
    tn.s2[d] = net.k2_scale[d];
  }
  tn.stem_k = rows_stem ? reinterpret_cast<const uint4*>(net.stem_k) : nullptr;
  tn.stem_ks = net.stem_scale;
  const az::TowerBlob& b = L.blob;
  tn.blob_floats = b.floats;
  tn.off_b1 = b.off_b1;
  tn.off_b2 = b.off_b2;
  tn.off_stemb = b.off_stemb;
  tn.off_wpc = b.off_wpc;
  tn.off_wvc = b.off_wvc;
  tn.off_hb = b.off_hb;
  tn.off_bpd = b.off_bpd;
  tn.off_bv1 = b.off_bv1;
  tn.off_wv2 = b.off_wv2;
  tn.off_wpd = b.off_wpd;
  tn.off_wv1 = b.off_wv1;
  tn.wv1_xtile = L.wv1_xtile;
  tn.dbuf = L.dbuf;
  tn.depth = depth;
  tn.hidden = net.req.hidden;
  // one tile height's fields (a null slot_pix: natural order)
  auto tiles = [&](const az::TowerTiles& t, int& rows, int& staged, int& wpd, int& wv1, const int** pix, int skip[2]) {
    rows = t.rows;
    staged = t.staged_floats;
    wpd = t.wpd_lds;
    wv1 = t.wv1_lds;
    skip[0] = t.skip[0];
    skip[1] = t.skip[1];
    return t.slot_pix.empty() ? 0 : upload_new(owned, const_cast<int**>(pix), t.slot_pix);
  };
  AZ_TRY(tiles(L.main, tn.tile_rows, tn.staged_floats, tn.wpd_lds, tn.wv1_lds, &tn.slot_pix, tn.skip));
  AZ_TRY(tiles(L.alt, tn.alt_rows, tn.alt_staged_floats, tn.alt_wpd_lds, tn.alt_wv1_lds, &tn.alt_slot_pix,
               tn.alt_skip));
  tn.alt_max_boards = L.alt_max_boards;
  if (!net.tower) AZ_TRY(owned.alloc(&net.tower, 1, false));
  std::vector<float> blob;
  float* qb = nullptr;
  AZ_TRY(tower_blob(f, L.blob, blob));
  AZ_TRY(upload_new(owned, &qb, blob));
  tn.blob = qb;
  AZ_HIP(hipMemcpy(net.tower, &tn, sizeof(az::TowerNet), hipMemcpyHostToDevice));
  return 0;
}

}  // namespace

namespace az {
// Keras names of custom_alphazero/model/weights.py.  in_ch = 4: the Connect-N
// stem kernels (stem_w [36][F]; the one-launch tower's stem16 pack and its
// small-weight blob); in_ch > 4 (chess, 118 planes): the stem is one more
// conv16 3x3 conv over the input zero-padded to F channels (stem_k), which is
// also the stem of the tower's input-row form.
int load_network(NetDev& net, const az_tensor* tensors, int n, double eps, DeviceAllocs& owned) {
  std::map<std::string, const az_tensor*> m;
  for (int i = 0; i < n; ++i) {
    if (!tensors[i].name || !tensors[i].data) return fail(AZ_E_INVALID, "tensor without name/data");
    m[tensors[i].name] = &tensors[i];
  }
  NetRequest& r = net.req;
  if (r.in_ch < 1 || r.in_ch > 128) return fail(AZ_E_INVALID, "input planes must be 1..128");
  FoldedNet f;
  AZ_TRY(fold_network(m, r.in_ch, r.depth, r.H * r.W, r.A, r.hidden, eps, f));
  AZ_TRY(upload_layers(net, f, owned));  // both per-layer packs (the tower reads the conv16 ones too)
  int dev = 0;
  AZ_HIP(hipGetDevice(&dev));
  AZ_HIP(hipDeviceGetAttribute(&r.cus, hipDeviceAttributeMultiprocessorCount, dev));
  NetPlan plan = plan_network(r);
  if (plan.status.code != AZ_OK) return fail(plan.status.code, plan.status.message);
  net.form = plan.form;
  net.terms = plan.terms;
  net.layout = std::move(plan.layout);
  if (net.form == NetForm::kTower || net.form == NetForm::kTowerRows)
    AZ_TRY(upload_tower(net, net.layout, f, net.form == NetForm::kTowerRows, owned));
  net.ready = true;
  return 0;
}
}  // namespace az
