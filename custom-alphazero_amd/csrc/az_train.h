// az_train.h -- the training step of the policy/value network, Connect-N
// (4 input planes, at most 128 actions) and chess (118 planes, 1880 actions):
// az_trainer_* in include/az.h, az_chess_trainer_create in include/az_chess.h;
// shapes and launchers of csrc/az_train.hip.
//
// Everything is fp32.  Activations are NHWC rows [n*HW][C]; weights stay in
// their Keras layouts (kernel [tap][cin][cout], dense [in][out]) inside one
// flat parameter blob, so no per-step repack is needed: the forward reads
// B[k][n] = W[tap][k][n] (coalesced over n), the data gradient reads the same
// tensor transposed, B[k][n] = W[tap][n][k] (one 16-byte load per lane).
#ifndef AZ_TRAIN_H_
#define AZ_TRAIN_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace az {
namespace train {

constexpr int kF = 128;              // tower channels (ConfigModel.filters)
constexpr int kRowsPerPart = 64;     // rows one workgroup reduces in a two-stage column sum
constexpr int kBoardsPerPart = 8;    // boards one split-K part of a weight gradient covers
constexpr int kMaxCellsTrain = 128;  // H*W the engine accepts (az_device.h kMaxCells)
constexpr int kMaxHidden = 1024;     // ValueHead hidden_dim the heads kernel holds in LDS
constexpr int kChessPlanes = 118;    // Board.full_state's planes (include/az_chess.h AZ_CHESS_PLANES)
constexpr int kChessActions = 1880;  // AZ_CHESS_ACTIONS
constexpr int kChessCells = 64;

// The factor the moving variance applies to the batch's biased variance
// (TF's fused BatchNormalization feeds the moving average Bessel's corrected
// variance); N = n*H*W rows.
inline double moving_variance_factor(int64_t N) { return N > 1 ? (double)N / (double)(N - 1) : 1.0; }

inline int row_parts(int rows) { return (rows + kRowsPerPart - 1) / kRowsPerPart; }
inline int board_parts(int n) { return (n + kBoardsPerPart - 1) / kBoardsPerPart; }

struct Geo {
  int H, W, HW, A, hidden;
  const uint16_t* tapmask;  // [HW]: bit t = neighbour (dy, dx) = (t/3-1, t%3-1) is on the board
};

// ---- convolutions (F -> F on the fp32 MFMA; stem and heads on the VALU)
void conv_forward(hipStream_t s, const Geo& g, int taps, const float* in, const float* w, const float* bias,
                  float* y, int rows);
// dx = dgrad(dy, w) [+ dgrad1x1(dy2, w2)]
void conv_dgrad(hipStream_t s, const Geo& g, int taps, const float* dy, const float* w, const float* dy2,
                const float* w2, float* dx, int rows);
// dw[tap][ci][co] = sum_rows x[row + tap][ci] dy[row][co]; partial: board_parts(n) * taps * F * F floats
void conv_wgrad(hipStream_t s, const Geo& g, int taps, const float* x, const float* dy, float* partial, float* dw,
                int n);
void stem_forward(hipStream_t s, const Geo& g, const float* x, const float* w, const float* bias, float* y, int rows);
void stem_wgrad(hipStream_t s, const Geo& g, const float* x, const float* dy, float* partial, float* dw, int rows);
// the chess stem, 118 -> F on the fp32 MFMA: x [rows][118] as the caller gave it (no padded copy);
// dw [9][118][F], partial: board_parts(n) * 9 * 118 * F floats.  The stem has no data gradient.
void chess_stem_forward(hipStream_t s, const Geo& g, const float* x, const float* w, const float* bias, float* y,
                        int rows);
void chess_stem_wgrad(hipStream_t s, const Geo& g, const float* x, const float* dy, float* partial, float* dw,
                      int n);
void headconv_forward(hipStream_t s, const float* h, const float* wp, const float* bp, const float* wv,
                      const float* bv, float* yp, float* yv, int rows);
void headconv_wgrad(hipStream_t s, const float* h, const float* dyp, const float* dyv, float* partial, float* dwp,
                    float* dwv, int rows);
void headconv_dgrad(hipStream_t s, const float* dyp, const float* dyv, const float* wp, const float* wv, float* dh,
                    int rows);

// ---- BatchNormalization in training mode over [rows][C]
// mean / var (biased) / invstd [C]; partial: 4 * row_parts(rows) * C floats (float64 sums, 8-byte aligned)
void bn_stats(hipStream_t s, const float* y, int rows, int C, float eps, float* partial, float* mean, float* var,
              float* invstd);
// out = relu?(gamma*yhat + beta [+ gamma2*yhat2 + beta2])
void bn_apply(hipStream_t s, const float* y, const float* mean, const float* invstd, const float* gamma,
              const float* beta, const float* y2, const float* mean2, const float* invstd2, const float* gamma2,
              const float* beta2, bool relu, float* out, int rows, int C);
// gm = g * (mask_out > 0); dbeta = sum gm, dgamma = sum gm*yhat, dy = gamma*invstd*(gm - dbeta/N - yhat*dgamma/N)
void bn_backward(hipStream_t s, const float* g, const float* mask_out, const float* y, const float* mean,
                 const float* invstd, const float* gamma, float* partial, float* dgamma, float* dbeta, float* dy,
                 int rows, int C);

// ---- heads, losses, update
struct HeadsArgs {
  const float *hp, *hv;            // [n][HW][2], [n][HW]: the head convs' outputs after BN + ReLU
  const float *wpd, *bpd;          // policy.dense
  const float *wv1, *bv1, *wv2, *bv2;
  const float *pi, *z;             // targets [n][A], [n]
  float *dlogit, *d1, *dpre1, *dpre2;  // [n][A], [n][hidden], [n][hidden], [n]
  float *ghp, *ghv;                // gradients of hp, hv
  float *lossp, *lossv;            // per board
};
void heads_forward_backward(hipStream_t s, const Geo& g, const HeadsArgs& a, int n);  // A <= 128
// the same for the chess heads (HW = 64, A = 1880): the policy head spread over the workgroup
void chess_heads_forward_backward(hipStream_t s, const Geo& g, const HeadsArgs& a, int n);
// dw[i][j] = sum_b x[b][i] d[b][j], db[j] = sum_b d[b][j]
void dense_wgrad(hipStream_t s, const float* x, const float* d, float* dw, float* db, int n, int I, int J);
// the same sums for the chess policy layer (I = 128, J = 1880), each dlogit loaded once for eight inputs
void chess_policy_wgrad(hipStream_t s, const float* x, const float* d, float* dw, float* db, int n);
// losses[3] = total, policy, value; sq_partial: (n_l2 + 4095) / 4096 doubles
void losses(hipStream_t s, const float* w, int64_t n_l2, double l2, const float* lossp, const float* lossv, int n,
            double* sq_partial, float* out);
// g += 2*l2*w on the first n_l2 elements (the .kernel tensors); a = mom*a - lr*g; w += a
void sgd_update(hipStream_t s, float* w, float* g, float* m, int64_t n_train, int64_t n_l2, float lr, float mom,
                float l2);
// moving = m*moving + take*batch*factor, take = 1 - m as the caller rounds it; means then variances, n_stats each
void moving_update(hipStream_t s, float* moving, const float* batch, int64_t n_stats, float m, float take,
                   float var_factor);

}  // namespace train
}  // namespace az

#endif  // AZ_TRAIN_H_
