// az_train.hip -- one training step of the policy/value network on gfx950:
// forward with batch statistics, backward, SGD with momentum (az_trainer_* in
// include/az.h; semantics in DESIGN.md, "Trainer").  Two networks share the
// tower, the BatchNormalization, the head convs and the update: Connect-N
// (az_trainer_create: 4 input planes, at most 128 actions) and chess
// (az_chess_trainer_create: 118 planes, 1880 actions), which has a stem and
// heads of its own (chess_stem_*, chess_heads_kernel).
//
// fp32 throughout.  The F -> F convolutions, their data gradients and their
// weight gradients are implicit GEMMs on v_mfma_f32_32x32x2_f32 (an exact fp32
// FMA chain, as conv3x3_mfma_kernel in az_nn.hip).  No floating-point atomic
// anywhere: every reduction that crosses workgroups writes per-part partial
// sums that a second kernel adds in part order, so a step is a pure function
// of the trainer's state and its batch.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "../../include/az.h"
#include "../../include/az_chess.h"
#include "az_host.h"
#include "az_replay.h"
#include "az_train.h"

namespace az {
namespace train {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ------------------------------------------------- F -> F conv: forward, dgrad
// out[r][n] = sum_tap sum_k A[nbr(r, tap)][k] * B_tap[k][n]  (+ bias[n])
//   forward: A = x,  nbr = r + (dy, dx),  B_tap[k][n] = w[tap][k][n]
//   DGRAD:   A = dy, nbr = r - (dy, dx),  B_tap[k][n] = w[tap][n][k]
//   SECOND (DGRAD only): + sum_k A2[r][k] * w2[n][k], the 1x1 projection's share
// Workgroup = 4 waves = a 32-row x 128-column tile, wave w owns columns
// [32w, +32).  Lane (h, r32) holds A's row r32 and B's column r32; one 16-byte
// A load covers k = c0+4h .. c0+4h+3, consumed by four MFMAs (the MFMA sums the
// lane halves' k pair).  Off-board neighbours contribute zeros.
template <int TAPS, bool DGRAD, bool SECOND>
__global__ __launch_bounds__(256) void conv_mfma_kernel(const float* __restrict__ a, const float* __restrict__ w,
                                                        const float* __restrict__ a2, const float* __restrict__ w2,
                                                        const float* __restrict__ bias, float* __restrict__ out,
                                                        int rows, int HW, int W,
                                                        const uint16_t* __restrict__ tapmask) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, r32 = lane & 31;
  const int row0 = blockIdx.x * 32;
  const int row = row0 + r32;
  const bool valid = row < rows;
  const int mask = valid ? tapmask[row % HW] : 0;
  const int col = wave * 32 + r32;

  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
  // The forward keeps its fp32 MFMA chains 32 channels short: after every 32-wide K chunk the
  // accumulator is added into a float64 sum and cleared.  One chain over K = 1152 left the
  // activations ~1e-6 from float64, which the value head's cancelling sums (one scalar for
  // value.conv's beta) turned into gradient errors past the tolerance; the flushes cost 16
  // conversions and adds per 16 MFMAs.
  constexpr bool WIDE = !DGRAD;
  double wide[WIDE ? 16 : 1];
#pragma unroll
  for (int i = 0; i < (WIDE ? 16 : 1); ++i) wide[i] = 0.0;

  for (int t = 0; t < TAPS; ++t) {
    const int tg = TAPS == 1 ? 4 : (DGRAD ? 8 - t : t);  // the geometric tap this lane's A row comes from
    const int off = (tg / 3 - 1) * W + (tg % 3 - 1);
    const bool ok = (mask >> tg) & 1;
    const float* ap = a + (size_t)(ok ? row + off : 0) * kF + 4 * h;
    const float* wt = w + (size_t)t * kF * kF;
    for (int c1 = 0; c1 < kF; c1 += 32) {
#pragma unroll
      for (int c0 = c1; c0 < c1 + 32; c0 += 8) {
        float4 av = *reinterpret_cast<const float4*>(ap + c0);
        if (!ok) av = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 bv;
        if constexpr (DGRAD) {
          bv = *reinterpret_cast<const float4*>(wt + (size_t)col * kF + c0 + 4 * h);
        } else {
          const float* wk = wt + (size_t)(c0 + 4 * h) * kF + col;
          bv = make_float4(wk[0], wk[kF], wk[2 * kF], wk[3 * kF]);
        }
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc, 0, 0, 0);
      }
      if constexpr (WIDE) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          wide[i] += (double)acc[i];
          acc[i] = 0.0f;
        }
      }
    }
  }
  if constexpr (SECOND) {
    const float* ap = a2 + (size_t)(valid ? row : 0) * kF + 4 * h;
#pragma unroll 4
    for (int c0 = 0; c0 < kF; c0 += 8) {
      float4 av = *reinterpret_cast<const float4*>(ap + c0);
      if (!valid) av = make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 bv = *reinterpret_cast<const float4*>(w2 + (size_t)col * kF + c0 + 4 * h);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc, 0, 0, 0);
    }
  }
  // C/D map: col = lane & 31, row = (i & 3) + 8 * (i >> 2) + 4 * h
  const float bcol = bias ? bias[col] : 0.0f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int r = row0 + (i & 3) + 8 * (i >> 2) + 4 * h;
    if (r < rows) out[(size_t)r * kF + col] = WIDE ? (float)(wide[i] + (double)bcol) : acc[i] + bcol;
  }
}

// ------------------------------------------------- F -> F conv: weight gradient
// partial[part][tap][ci][co] = sum over the part's rows of x[row + tap][ci] * dy[row][co]:
// a 128 x 128 GEMM per tap with K = the part's rows.  Workgroup = (tap, part),
// 4 waves; wave w owns ci in [32w, +32) and all four 32-wide co blocks.  The K
// loop walks a board's cells in pairs (the two lane halves), so a cell's edge
// mask is a table lookup and no k pair straddles two boards.
template <int TAPS>
__global__ __launch_bounds__(256) void wgrad_mfma_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                         float* __restrict__ partial, int n, int HW, int W,
                                                         const uint16_t* __restrict__ tapmask) {
  __shared__ uint8_t okc[kMaxCellsTrain];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, r32 = lane & 31;
  const int t = blockIdx.x, part = blockIdx.y;
  const int tg = TAPS == 1 ? 4 : t;
  const int off = (tg / 3 - 1) * W + (tg % 3 - 1);
  for (int i = tid; i < HW; i += 256) okc[i] = (tapmask[i] >> tg) & 1;
  __syncthreads();
  const int b0 = part * kBoardsPerPart;
  const int b1 = min(n, b0 + kBoardsPerPart);

  f32x16 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[j][i] = 0.0f;

  for (int b = b0; b < b1; ++b) {
    const size_t base = (size_t)b * HW;
    for (int p = 0; p < HW; p += 2) {
      const int pos = p + h;
      const bool in = pos < HW;
      const bool ok = in && okc[in ? pos : 0];
      float av = x[(base + (ok ? pos + off : 0)) * kF + wave * 32 + r32];
      if (!ok) av = 0.0f;
      const float* dp = dy + (base + (in ? pos : 0)) * kF + r32;
      float bv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bv[j] = dp[32 * j];
        if (!in) bv[j] = 0.0f;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[j], acc[j], 0, 0, 0);
    }
  }
  float* po = partial + ((size_t)part * TAPS + t) * kF * kF;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int ci = wave * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
      po[(size_t)ci * kF + 32 * j + r32] = acc[j][i];
    }
}

// out[i] = partial[0][i] + partial[1][i] + ... in part order (float64 running sum)
__global__ void reduce_parts_kernel(const float* __restrict__ partial, int parts, int64_t count,
                                    float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  double s = 0.0;
  for (int p = 0; p < parts; ++p) s += (double)partial[(size_t)p * count + i];
  out[i] = (float)s;
}

// ------------------------------------------------- stem (4 planes, K = 36)
__global__ void stem_forward_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                    const float* __restrict__ bias, float* __restrict__ y, int rows, int HW, int W,
                                    const uint16_t* __restrict__ tapmask) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)rows * kF) return;
  const int row = (int)(i / kF), co = (int)(i % kF);
  const int mask = tapmask[row % HW];
  float acc = 0.0f;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    if (!((mask >> t) & 1)) continue;
    const float4 xv = *reinterpret_cast<const float4*>(x + (size_t)(row + (t / 3 - 1) * W + (t % 3 - 1)) * 4);
    const float* wk = w + (size_t)t * 4 * kF + co;
    acc = fmaf(xv.x, wk[0], acc);
    acc = fmaf(xv.y, wk[kF], acc);
    acc = fmaf(xv.z, wk[2 * kF], acc);
    acc = fmaf(xv.w, wk[3 * kF], acc);
  }
  y[i] = acc + bias[co];
}

// partial[part][tap*4 + ci][co] over the part's kRowsPerPart rows; grid (18, parts), 256 threads
__global__ void stem_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                  float* __restrict__ partial, int rows, int HW, int W,
                                  const uint16_t* __restrict__ tapmask) {
  const int o = blockIdx.x * 256 + threadIdx.x;  // < 36 * 128
  const int k = o / kF, co = o % kF;
  const int t = k >> 2, ci = k & 3;
  const int off = (t / 3 - 1) * W + (t % 3 - 1);
  const int r0 = blockIdx.y * kRowsPerPart;
  const int r1 = min(rows, r0 + kRowsPerPart);
  int pos = r0 % HW;
  float acc = 0.0f;
  for (int r = r0; r < r1; ++r) {
    if ((tapmask[pos] >> t) & 1) acc = fmaf(x[(size_t)(r + off) * 4 + ci], dy[(size_t)r * kF + co], acc);
    if (++pos == HW) pos = 0;
  }
  partial[(size_t)blockIdx.y * (36 * kF) + o] = acc;
}

// ------------------------------------------------- chess stem (118 planes, K = 9 * 118)
// conv_mfma_kernel's forward tile (32 rows x 128 columns, wave w owns columns
// [32w, +32), the accumulator added into float64 after every 32 k) over rows of
// 118 floats.  A row is 472 bytes, so a lane's four k come as two 8-byte loads
// (a 16-byte load of an odd row would be misaligned).  118 = 14 * 8 + 6: the
// last chunk's upper lane half holds k = 116, 117 and nothing at 118, 119,
// where neither x (the next row) nor w (the next tap, or the next tensor) is
// read and both MFMA operands are exact zeros.
__global__ __launch_bounds__(256) void chess_stem_forward_kernel(const float* __restrict__ x,
                                                                 const float* __restrict__ w,
                                                                 const float* __restrict__ bias,
                                                                 float* __restrict__ out, int rows, int HW, int W,
                                                                 const uint16_t* __restrict__ tapmask) {
  constexpr int kC = kChessPlanes;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, r32 = lane & 31;
  const int row0 = blockIdx.x * 32;
  const int row = row0 + r32;
  const bool valid = row < rows;
  const int mask = valid ? tapmask[row % HW] : 0;
  const int col = wave * 32 + r32;

  f32x16 acc;
  double wide[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.0f, wide[i] = 0.0;

  for (int t = 0; t < 9; ++t) {
    const int off = (t / 3 - 1) * W + (t % 3 - 1);
    const bool ok = (mask >> t) & 1;
    const float* ap = x + (size_t)(ok ? row + off : 0) * kC + 4 * h;
    const float* wt = w + ((size_t)t * kC + 4 * h) * kF + col;
#pragma unroll
    for (int c1 = 0; c1 < kF; c1 += 32) {
#pragma unroll
      for (int c0 = c1; c0 < c1 + 32 && c0 < kC; c0 += 8) {
        const bool hi = c0 + 4 * h + 2 < kC;  // false for k = 118, 119 only
        float2 a01 = *reinterpret_cast<const float2*>(ap + c0);
        float2 a23 = *reinterpret_cast<const float2*>(ap + c0 + (hi ? 2 : 0));
        const float* wk = wt + (size_t)c0 * kF;
        float b0 = wk[0], b1 = wk[kF], b2 = wk[hi ? 2 * kF : 0], b3 = wk[hi ? 3 * kF : 0];
        if (!hi) a23 = make_float2(0.f, 0.f), b2 = 0.f, b3 = 0.f;
        if (!ok) a01 = make_float2(0.f, 0.f), a23 = make_float2(0.f, 0.f);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a01.x, b0, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a01.y, b1, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a23.x, b2, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a23.y, b3, acc, 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        wide[i] += (double)acc[i];
        acc[i] = 0.0f;
      }
    }
  }
  const float bcol = bias[col];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int r = row0 + (i & 3) + 8 * (i >> 2) + 4 * h;
    if (r < rows) out[(size_t)r * kF + col] = (float)(wide[i] + (double)bcol);
  }
}

// partial[part][tap][ci < 118][co]: wgrad_mfma_kernel over rows of 118 floats.  Wave 3 owns
// ci in [96, 128): its lanes at ci >= 118 feed zeros and store nothing.
__global__ __launch_bounds__(256) void chess_stem_wgrad_kernel(const float* __restrict__ x,
                                                               const float* __restrict__ dy,
                                                               float* __restrict__ partial, int n,
                                                               const uint16_t* __restrict__ tapmask) {
  constexpr int kC = kChessPlanes, HW = kChessCells, W = 8;
  __shared__ uint8_t okc[HW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, r32 = lane & 31;
  const int t = blockIdx.x, part = blockIdx.y;
  const int off = (t / 3 - 1) * W + (t % 3 - 1);
  for (int i = tid; i < HW; i += 256) okc[i] = (tapmask[i] >> t) & 1;
  __syncthreads();
  const int b0 = part * kBoardsPerPart;
  const int b1 = min(n, b0 + kBoardsPerPart);
  const int ci_in = wave * 32 + r32;
  const bool has_ci = ci_in < kC;

  f32x16 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[j][i] = 0.0f;

  // HW = 64 is even: every k pair is two cells of one board.  Four pairs' loads are issued together
  // (the loop is bound by their latency, not by the MFMAs); each accumulator still sums in cell order.
  for (int b = b0; b < b1; ++b) {
    const size_t base = (size_t)b * HW;
#pragma unroll 2
    for (int p0 = 0; p0 < HW; p0 += 8) {
      float av[4], bv[4][4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int pos = p0 + 2 * u + h;
        const bool ok = okc[pos] && has_ci;
        av[u] = x[(base + (ok ? pos + off : 0)) * kC + (has_ci ? ci_in : 0)];
        if (!ok) av[u] = 0.0f;
        const float* dp = dy + (base + pos) * kF + r32;
#pragma unroll
        for (int j = 0; j < 4; ++j) bv[u][j] = dp[32 * j];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u][j], acc[j], 0, 0, 0);
    }
  }
  float* po = partial + ((size_t)part * 9 + t) * kC * kF;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int ci = wave * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
      if (ci < kC) po[(size_t)ci * kF + 32 * j + r32] = acc[j][i];
    }
}

// ------------------------------------------------- head convs (1x1, F -> 2 and F -> 1)
// one wave per row
__global__ __launch_bounds__(256) void headconv_forward_kernel(const float* __restrict__ hin,
                                                               const float* __restrict__ wp,
                                                               const float* __restrict__ bp,
                                                               const float* __restrict__ wv,
                                                               const float* __restrict__ bv, float* __restrict__ yp,
                                                               float* __restrict__ yv, int rows) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float x0 = hin[(size_t)row * kF + lane], x1 = hin[(size_t)row * kF + 64 + lane];
  float s0 = fmaf(x1, wp[(64 + lane) * 2], x0 * wp[lane * 2]);
  float s1 = fmaf(x1, wp[(64 + lane) * 2 + 1], x0 * wp[lane * 2 + 1]);
  float s2 = fmaf(x1, wv[64 + lane], x0 * wv[lane]);
  s0 = wave_sum(s0);
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  if (lane == 0) {
    yp[(size_t)row * 2] = s0 + bp[0];
    yp[(size_t)row * 2 + 1] = s1 + bp[1];
    yv[row] = s2 + bv[0];
  }
}

// partial[part][c*2 + o] (policy, 256 floats) then [256 + c] (value): 384 floats per part; 128 threads
__global__ void headconv_wgrad_kernel(const float* __restrict__ hin, const float* __restrict__ dyp,
                                      const float* __restrict__ dyv, float* __restrict__ partial, int rows) {
  const int c = threadIdx.x;
  const int r0 = blockIdx.x * kRowsPerPart;
  const int r1 = min(rows, r0 + kRowsPerPart);
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  for (int r = r0; r < r1; ++r) {
    const float xv = hin[(size_t)r * kF + c];
    a0 = fmaf(xv, dyp[(size_t)r * 2], a0);
    a1 = fmaf(xv, dyp[(size_t)r * 2 + 1], a1);
    a2 = fmaf(xv, dyv[r], a2);
  }
  float* po = partial + (size_t)blockIdx.x * 384;
  po[c * 2] = a0;
  po[c * 2 + 1] = a1;
  po[256 + c] = a2;
}

__global__ void headconv_dgrad_kernel(const float* __restrict__ dyp, const float* __restrict__ dyv,
                                      const float* __restrict__ wp, const float* __restrict__ wv,
                                      float* __restrict__ dh, int rows) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)rows * kF) return;
  const int row = (int)(i / kF), c = (int)(i % kF);
  float g = dyp[(size_t)row * 2] * wp[c * 2];
  g = fmaf(dyp[(size_t)row * 2 + 1], wp[c * 2 + 1], g);
  g = fmaf(dyv[row], wv[c], g);
  dh[i] = g;
}

// ------------------------------------------------- BatchNormalization
// Column sums in two stages, every order fixed.  Stage 1: one workgroup per
// kRowsPerPart rows, thread = (channel, one of kPhases row phases); the phases'
// sums are added in phase order.  Stage 2 (parts_sum): thread = (channel, one
// of kChunks runs of consecutive parts), the runs' float64 sums added in run order.
// MODE 0: sum y; MODE 1: sum (y - mean)^2 (the centred second pass).
constexpr int kPhases = 4;
constexpr int kChunks = 8;

template <int MODE>
__global__ void bn_sum_kernel(const float* __restrict__ y, const float* __restrict__ mean,
                              double* __restrict__ partial, int rows, int C, int CT) {
  __shared__ double red[kPhases * kF];
  const int c = threadIdx.x % CT, ph = threadIdx.x / CT;  // blockDim.x = CT * kPhases, C <= CT <= kF
  const int r0 = blockIdx.x * kRowsPerPart;
  const int r1 = min(rows, r0 + kRowsPerPart);
  double s = 0.0;  // float64 running sums: a channel's sum can be far smaller than its terms
  if (c < C) {
    const float mu = MODE == 1 ? mean[c] : 0.0f;
    for (int r = r0 + ph; r < r1; r += kPhases) {
      const float v = y[(size_t)r * C + c] - mu;
      s += (double)(MODE == 1 ? v * v : v);
    }
  }
  red[ph * CT + c] = s;
  __syncthreads();
  if (ph == 0 && c < C)
    partial[(size_t)blockIdx.x * C + c] = ((red[c] + red[CT + c]) + red[2 * CT + c]) + red[3 * CT + c];
}

// sum over p of partial[p * stride + c] for the 32 channels of this workgroup; 256 threads, all must call
__device__ double parts_sum(const double* __restrict__ partial, int parts, size_t stride, int c, bool active,
                            double* red) {
  const int lc = threadIdx.x & 31, q = threadIdx.x >> 5;
  const int chunk = (parts + kChunks - 1) / kChunks;
  const int p1 = min(parts, (q + 1) * chunk);
  double s = 0.0;
  if (active)
    for (int p = q * chunk; p < p1; ++p) s += partial[(size_t)p * stride + c];
  __syncthreads();
  red[q * 32 + lc] = s;
  __syncthreads();
  double t = red[lc];
#pragma unroll
  for (int k = 1; k < kChunks; ++k) t += red[k * 32 + lc];
  return t;
}

template <int MODE>
__global__ __launch_bounds__(256) void bn_stats_final_kernel(const double* __restrict__ partial, int parts, int rows,
                                                             int C, float eps, float* __restrict__ mean,
                                                             float* __restrict__ var, float* __restrict__ invstd) {
  __shared__ double red[kChunks * 32];
  const int c = blockIdx.x * 32 + (threadIdx.x & 31);
  const double s = parts_sum(partial, parts, C, c, c < C, red);
  if (c >= C || threadIdx.x >= 32) return;
  const float m = (float)(s / (double)rows);
  if (MODE == 0) {
    mean[c] = m;
  } else {
    var[c] = m;
    invstd[c] = 1.0f / sqrtf(m + eps);
  }
}

__global__ void bn_apply_kernel(const float* __restrict__ y, const float* __restrict__ mean,
                                const float* __restrict__ invstd, const float* __restrict__ gamma,
                                const float* __restrict__ beta, const float* __restrict__ y2,
                                const float* __restrict__ mean2, const float* __restrict__ invstd2,
                                const float* __restrict__ gamma2, const float* __restrict__ beta2, int relu,
                                float* __restrict__ out, int64_t total, int C) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C);
  float v = fmaf(gamma[c], (y[i] - mean[c]) * invstd[c], beta[c]);
  if (y2) v += fmaf(gamma2[c], (y2[i] - mean2[c]) * invstd2[c], beta2[c]);
  out[i] = relu ? fmaxf(v, 0.0f) : v;
}

// partial[part][0][c] = sum gm, partial[part][1][c] = sum gm * yhat
__global__ void bn_bwd_sum_kernel(const float* __restrict__ g, const float* __restrict__ mask_out,
                                  const float* __restrict__ y, const float* __restrict__ mean,
                                  const float* __restrict__ invstd, double* __restrict__ partial, int rows, int C,
                                  int CT) {
  __shared__ double redb[kPhases * kF];
  __shared__ double redg[kPhases * kF];
  const int c = threadIdx.x % CT, ph = threadIdx.x / CT;
  const int r0 = blockIdx.x * kRowsPerPart;
  const int r1 = min(rows, r0 + kRowsPerPart);
  double sb = 0.0, sg = 0.0;
  if (c < C) {
    const float mu = mean[c], is = invstd[c];
    for (int r = r0 + ph; r < r1; r += kPhases) {
      const size_t i = (size_t)r * C + c;
      const float gm = mask_out[i] > 0.0f ? g[i] : 0.0f;
      sb += (double)gm;
      sg += (double)(gm * ((y[i] - mu) * is));
    }
  }
  redb[ph * CT + c] = sb;
  redg[ph * CT + c] = sg;
  __syncthreads();
  if (ph == 0 && c < C) {
    partial[((size_t)blockIdx.x * 2) * C + c] = ((redb[c] + redb[CT + c]) + redb[2 * CT + c]) + redb[3 * CT + c];
    partial[((size_t)blockIdx.x * 2 + 1) * C + c] = ((redg[c] + redg[CT + c]) + redg[2 * CT + c]) + redg[3 * CT + c];
  }
}

__global__ __launch_bounds__(256) void bn_bwd_final_kernel(const double* __restrict__ partial, int parts, int C,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta) {
  __shared__ double red[kChunks * 32];
  const int c = blockIdx.x * 32 + (threadIdx.x & 31);
  const double sb = parts_sum(partial, parts, (size_t)2 * C, c, c < C, red);
  const double sg = parts_sum(partial + C, parts, (size_t)2 * C, c, c < C, red);
  if (c >= C || threadIdx.x >= 32) return;
  dbeta[c] = (float)sb;
  dgamma[c] = (float)sg;
}

__global__ void bn_bwd_apply_kernel(const float* __restrict__ g, const float* __restrict__ mask_out,
                                    const float* __restrict__ y, const float* __restrict__ mean,
                                    const float* __restrict__ invstd, const float* __restrict__ gamma,
                                    const float* __restrict__ dgamma, const float* __restrict__ dbeta,
                                    float* __restrict__ dy, int64_t total, int C, float inv_n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C);
  const float gm = mask_out[i] > 0.0f ? g[i] : 0.0f;
  const float yh = (y[i] - mean[c]) * invstd[c];
  dy[i] = gamma[c] * invstd[c] * (gm - dbeta[c] * inv_n - yh * (dgamma[c] * inv_n));
}

// ------------------------------------------------- heads: dense layers, losses, their backward
// One workgroup per board.  Policy: logits = flat(hp) W + b, p = softmax,
// Lp_b = -sum pi log(p + 1e-7), g_a = -pi_a / (p_a + 1e-7) / n,
// dlogit_a = p_a (g_a - sum_c p_c g_c) (the 1e-7 sits inside the log, so no
// p - pi shortcut).  Value: d1 = relu(flat(hv) W1 + b1), v = tanh(d1 W2 + b2),
// Lv_b = (v - z)^2.  Every sum runs in index order on one thread.
__global__ __launch_bounds__(256) void heads_kernel(HeadsArgs a, int n, int HW, int A, int hidden) {
  __shared__ float fp[2 * kMaxCellsTrain];
  __shared__ float fv[kMaxCellsTrain];
  __shared__ float lg[kMaxCellsTrain];   // logits, then probabilities
  __shared__ float dl[kMaxCellsTrain];   // dlogit
  __shared__ float d1[kMaxHidden];
  __shared__ float dp1[kMaxHidden];
  __shared__ float sc[2];
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < 2 * HW; i += 256) fp[i] = a.hp[(size_t)b * 2 * HW + i];
  for (int i = tid; i < HW; i += 256) fv[i] = a.hv[(size_t)b * HW + i];
  __syncthreads();
  // every dot product and the softmax / tanh run in float64 and round once: the heads'
  // gradients feed sums with heavy cancellation (a head conv's beta gradient is one scalar)
  if (tid < A) {
    double s = 0.0;
    for (int i = 0; i < 2 * HW; ++i) s += (double)fp[i] * (double)a.wpd[(size_t)i * A + tid];
    lg[tid] = (float)(s + (double)a.bpd[tid]);
  }
  for (int j = tid; j < hidden; j += 256) {
    double s = 0.0;
    for (int i = 0; i < HW; ++i) s += (double)fv[i] * (double)a.wv1[(size_t)i * hidden + j];
    const float r = fmaxf((float)(s + (double)a.bv1[j]), 0.0f);
    d1[j] = r;
    a.d1[(size_t)b * hidden + j] = r;
  }
  __syncthreads();
  if (tid == 0) {
    float mx = lg[0];
    for (int k = 1; k < A; ++k) mx = fmaxf(mx, lg[k]);
    double sum = 0.0;
    for (int k = 0; k < A; ++k) sum += exp((double)lg[k] - (double)mx);
    double lp = 0.0, dot = 0.0;
    for (int k = 0; k < A; ++k) {
      const double p = exp((double)lg[k] - (double)mx) / sum;
      const double pi = (double)a.pi[(size_t)b * A + k];
      lp -= pi * log(p + 1e-7);
      const double gk = -pi / (p + 1e-7) / (double)n;
      dot += p * gk;
    }
    for (int k = 0; k < A; ++k) {
      const double p = exp((double)lg[k] - (double)mx) / sum;
      const double gk = -(double)a.pi[(size_t)b * A + k] / (p + 1e-7) / (double)n;
      dl[k] = (float)(p * (gk - dot));
      a.dlogit[(size_t)b * A + k] = dl[k];
    }
    a.lossp[b] = (float)lp;
  } else if (tid == 64) {
    double s = 0.0;
    for (int j = 0; j < hidden; ++j) s += (double)d1[j] * (double)a.wv2[j];
    const double v = tanh(s + (double)a.bv2[0]);
    const double e = v - (double)a.z[b];
    a.lossv[b] = (float)(e * e);
    const float dpre2 = (float)(2.0 * e / (double)n * (1.0 - v * v));
    a.dpre2[b] = dpre2;
    sc[0] = dpre2;
  }
  __syncthreads();
  const float dpre2 = sc[0];
  for (int j = tid; j < hidden; j += 256) {
    const float d = d1[j] > 0.0f ? dpre2 * a.wv2[j] : 0.0f;
    dp1[j] = d;
    a.dpre1[(size_t)b * hidden + j] = d;
  }
  for (int i = tid; i < 2 * HW; i += 256) {
    double s = 0.0;
    for (int k = 0; k < A; ++k) s += (double)dl[k] * (double)a.wpd[(size_t)i * A + k];
    a.ghp[(size_t)b * 2 * HW + i] = (float)s;
  }
  __syncthreads();
  for (int i = tid; i < HW; i += 256) {
    double s = 0.0;
    for (int j = 0; j < hidden; ++j) s += (double)dp1[j] * (double)a.wv1[(size_t)i * hidden + j];
    a.ghv[(size_t)b * HW + i] = (float)s;
  }
}

// ------------------------------------------------- chess heads (HW = 64, A = 1880)
// sum of v over the workgroup's 256 threads in a fixed tree; every thread calls, every thread gets it
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  const double s = red[0];
  __syncthreads();
  return s;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// heads_kernel's arithmetic (float64 dots, softmax and losses, one rounding each) with the policy
// head's work spread over the workgroup: thread t owns the actions a = t + 256 j, j < 8 (its
// logits, its terms of the softmax sum, of the loss and of sum p g, its dlogits), each total is
// the threads' partial sums (in j order) added in block_sum's tree; wave w owns ghp's inputs
// i in [32w, +32), a dot over the 1880 dlogits as lane-strided partials added in wave_sum_f64's
// butterfly.  Every order is fixed by the thread index alone.  The value head is heads_kernel's.
// LDS: 7.5 KB of logits (then dlogits), 8 KB d1 / dpre1, 2 KB of reduction scratch.
__global__ __launch_bounds__(256) void chess_heads_kernel(HeadsArgs a, int n, int hidden) {
  constexpr int HW = kChessCells, A = kChessActions, PER = (A + 255) / 256;
  __shared__ float fp[2 * HW];
  __shared__ float fv[HW];
  __shared__ float lg[A];  // logits, then dlogit
  __shared__ float d1[kMaxHidden];
  __shared__ float dp1[kMaxHidden];
  __shared__ double red[256];
  __shared__ float sc[2];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < 2 * HW; i += 256) fp[i] = a.hp[(size_t)b * 2 * HW + i];
  for (int i = tid; i < HW; i += 256) fv[i] = a.hv[(size_t)b * HW + i];
  __syncthreads();
  double s[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) s[j] = 0.0;
  // actions t + 256 j exist for every j < PER - 1; the last only for t < A - 256 (PER - 1) = 88.
  // Four inputs' loads are in flight together; each sum still runs in input order.
  const bool last = tid + 256 * (PER - 1) < A;
#pragma unroll 4
  for (int i = 0; i < 2 * HW; ++i) {
    const double f = (double)fp[i];
    const float* wr = a.wpd + (size_t)i * A + tid;
    float wj[PER];
#pragma unroll
    for (int j = 0; j < PER - 1; ++j) wj[j] = wr[256 * j];
    wj[PER - 1] = last ? wr[256 * (PER - 1)] : 0.0f;
#pragma unroll
    for (int j = 0; j < PER; ++j) s[j] += f * (double)wj[j];
  }
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int k = tid + 256 * j;
    if (k < A) {
      lg[k] = (float)(s[j] + (double)a.bpd[k]);
      mx = fmaxf(mx, lg[k]);
    }
  }
  for (int j = tid; j < hidden; j += 256) {
    double t = 0.0;
    for (int i = 0; i < HW; ++i) t += (double)fv[i] * (double)a.wv1[(size_t)i * hidden + j];
    const float r = fmaxf((float)(t + (double)a.bv1[j]), 0.0f);
    d1[j] = r;
    a.d1[(size_t)b * hidden + j] = r;
  }
  // the maximum: exact in any order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if (lane == 0) red[wave] = (double)mx;
  __syncthreads();  // also publishes lg and d1
  mx = fmaxf(fmaxf((float)red[0], (float)red[1]), fmaxf((float)red[2], (float)red[3]));
  __syncthreads();
  if (tid == 64) {
    double t = 0.0;
    for (int j = 0; j < hidden; ++j) t += (double)d1[j] * (double)a.wv2[j];
    const double v = tanh(t + (double)a.bv2[0]);
    const double e = v - (double)a.z[b];
    a.lossv[b] = (float)(e * e);
    const float dpre2 = (float)(2.0 * e / (double)n * (1.0 - v * v));
    a.dpre2[b] = dpre2;
    sc[1] = dpre2;
  }
  double ex[PER];
  double part = 0.0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int k = tid + 256 * j;
    ex[j] = k < A ? exp((double)lg[k] - (double)mx) : 0.0;
    part += ex[j];
  }
  const double sum = block_sum(part, red);
  double gk[PER];
  double lp = 0.0, dot = 0.0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int k = tid + 256 * j;
    const double p = ex[j] / sum;
    const double pi = k < A ? (double)a.pi[(size_t)b * A + k] : 0.0;
    lp -= pi * log(p + 1e-7);
    gk[j] = -pi / (p + 1e-7) / (double)n;
    dot += p * gk[j];
    ex[j] = p;
  }
  lp = block_sum(lp, red);
  dot = block_sum(dot, red);
  if (tid == 0) a.lossp[b] = (float)lp;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int k = tid + 256 * j;
    if (k < A) {
      const float d = (float)(ex[j] * (gk[j] - dot));
      lg[k] = d;
      a.dlogit[(size_t)b * A + k] = d;
    }
  }
  __syncthreads();  // the dlogits; sc[1] (block_sum's barriers came after thread 64 wrote it)
  const float dpre2 = sc[1];
  for (int j = tid; j < hidden; j += 256) {
    const float d = d1[j] > 0.0f ? dpre2 * a.wv2[j] : 0.0f;
    dp1[j] = d;
    a.dpre1[(size_t)b * hidden + j] = d;
  }
  // a lane's actions lane + 64 k exist for every k < 29; the last (k = 29) only for lane < 24
  constexpr int FULL = A / 64;
  for (int i0 = wave * 32; i0 < wave * 32 + 32; i0 += 8) {
    double g[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) g[q] = 0.0;
    const float* wr = a.wpd + (size_t)i0 * A + lane;
#pragma unroll 2
    for (int k = 0; k < FULL; ++k) {
      const double d = (double)lg[lane + 64 * k];
#pragma unroll
      for (int q = 0; q < 8; ++q) g[q] += d * (double)wr[(size_t)q * A + 64 * k];
    }
    if (lane + 64 * FULL < A) {
      const double d = (double)lg[lane + 64 * FULL];
#pragma unroll
      for (int q = 0; q < 8; ++q) g[q] += d * (double)wr[(size_t)q * A + 64 * FULL];
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const double t = wave_sum_f64(g[q]);
      if (lane == 0) a.ghp[(size_t)b * 2 * HW + i0 + q] = (float)t;
    }
  }
  __syncthreads();
  for (int i = tid; i < HW; i += 256) {
    double t = 0.0;
    for (int j = 0; j < hidden; ++j) t += (double)dp1[j] * (double)a.wv1[(size_t)i * hidden + j];
    a.ghv[(size_t)b * HW + i] = (float)t;
  }
}

// dw[i][j] = sum_b x[b][i] d[b][j] for i < I; i == I is the bias row db[j] = sum_b d[b][j]
__global__ void dense_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ d, float* __restrict__ dw,
                                   float* __restrict__ db, int n, int I, int J) {
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= (I + 1) * J) return;
  const int i = o / J, j = o % J;
  float s = 0.0f;
  if (i < I) {
    for (int b = 0; b < n; ++b) s = fmaf(x[(size_t)b * I + i], d[(size_t)b * J + j], s);
    dw[o] = s;
  } else {
    double t = 0.0;
    for (int b = 0; b < n; ++b) t += (double)d[(size_t)b * J + j];
    db[j] = (float)t;
  }
}

// dense_wgrad_kernel's sums (boards in order, an fp32 fmaf chain; the bias row in float64) for the
// chess policy layer, I = 128 inputs x J = 1880 actions.  A thread owns one action and eight
// inputs, so a dlogit is loaded once for eight outputs: dense_wgrad_kernel would read the batch's
// 1.9 MB of dlogits 129 times.  grid (ceil(J / 256), I / 8)
__global__ __launch_bounds__(256) void chess_policy_wgrad_kernel(const float* __restrict__ x,
                                                                 const float* __restrict__ d,
                                                                 float* __restrict__ dw, float* __restrict__ db,
                                                                 int n) {
  constexpr int I = 2 * kChessCells, J = kChessActions, TI = 8;
  const int j = blockIdx.x * 256 + threadIdx.x;
  const int i0 = blockIdx.y * TI;
  if (j >= J) return;
  float s[TI];
#pragma unroll
  for (int q = 0; q < TI; ++q) s[q] = 0.0f;
  double t = 0.0;
  for (int b = 0; b < n; ++b) {
    const float dv = d[(size_t)b * J + j];
    const float* xb = x + (size_t)b * I + i0;
#pragma unroll
    for (int q = 0; q < TI; ++q) s[q] = fmaf(xb[q], dv, s[q]);
    t += (double)dv;
  }
#pragma unroll
  for (int q = 0; q < TI; ++q) dw[(size_t)(i0 + q) * J + j] = s[q];
  if (blockIdx.y == 0) db[j] = (float)t;
}

// sum of squares of 4096 weights per workgroup (fixed tree)
__global__ __launch_bounds__(256) void sqsum_kernel(const float* __restrict__ w, int64_t count,
                                                    double* __restrict__ partial) {
  __shared__ double red[256];
  const int64_t base = (int64_t)blockIdx.x * 4096;
  double s = 0.0;
  for (int k = 0; k < 16; ++k) {
    const int64_t i = base + k * 256 + threadIdx.x;
    if (i < count) s += (double)w[i] * (double)w[i];
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

__global__ void loss_final_kernel(const double* __restrict__ sq_partial, int sq_parts, double l2,
                                  const float* __restrict__ lossp, const float* __restrict__ lossv, int n,
                                  float* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double sq = 0.0, lp = 0.0, lv = 0.0;
  for (int p = 0; p < sq_parts; ++p) sq += sq_partial[p];
  for (int b = 0; b < n; ++b) {
    lp += (double)lossp[b];
    lv += (double)lossv[b];
  }
  lp /= (double)n;
  lv /= (double)n;
  out[0] = (float)(lp + lv + l2 * sq);
  out[1] = (float)lp;
  out[2] = (float)lv;
}

__global__ void sgd_update_kernel(float* __restrict__ w, float* __restrict__ g, float* __restrict__ m,
                                  int64_t n_train, int64_t n_l2, float lr, float mom, float l2x2) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_train) return;
  const float wi = w[i];
  float gi = g[i];
  if (i < n_l2) gi = fmaf(l2x2, wi, gi);
  g[i] = gi;
  const float ai = mom * m[i] - lr * gi;
  m[i] = ai;
  w[i] = wi + ai;
}

__global__ void moving_update_kernel(float* __restrict__ moving, const float* __restrict__ batch, int64_t n_stats,
                                     float m, float take, float var_factor) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * n_stats) return;
  const float v = i < n_stats ? batch[i] : batch[i] * var_factor;
  moving[i] = m * moving[i] + take * v;
}

inline unsigned blocks(int64_t total, int per) { return (unsigned)((total + per - 1) / per); }

}  // namespace

// ------------------------------------------------------------------ launchers
void conv_forward(hipStream_t s, const Geo& g, int taps, const float* in, const float* w, const float* bias,
                  float* y, int rows) {
  const dim3 grid(blocks(rows, 32));
  if (taps == 9)
    conv_mfma_kernel<9, false, false><<<grid, 256, 0, s>>>(in, w, nullptr, nullptr, bias, y, rows, g.HW, g.W, g.tapmask);
  else
    conv_mfma_kernel<1, false, false><<<grid, 256, 0, s>>>(in, w, nullptr, nullptr, bias, y, rows, g.HW, g.W, g.tapmask);
}

void conv_dgrad(hipStream_t s, const Geo& g, int taps, const float* dy, const float* w, const float* dy2,
                const float* w2, float* dx, int rows) {
  const dim3 grid(blocks(rows, 32));
  if (taps == 9 && dy2)
    conv_mfma_kernel<9, true, true><<<grid, 256, 0, s>>>(dy, w, dy2, w2, nullptr, dx, rows, g.HW, g.W, g.tapmask);
  else if (taps == 9)
    conv_mfma_kernel<9, true, false><<<grid, 256, 0, s>>>(dy, w, nullptr, nullptr, nullptr, dx, rows, g.HW, g.W, g.tapmask);
  else
    conv_mfma_kernel<1, true, false><<<grid, 256, 0, s>>>(dy, w, nullptr, nullptr, nullptr, dx, rows, g.HW, g.W, g.tapmask);
}

void conv_wgrad(hipStream_t s, const Geo& g, int taps, const float* x, const float* dy, float* partial, float* dw,
                int n) {
  const int parts = board_parts(n);
  if (taps == 9)
    wgrad_mfma_kernel<9><<<dim3(9, parts), 256, 0, s>>>(x, dy, partial, n, g.HW, g.W, g.tapmask);
  else
    wgrad_mfma_kernel<1><<<dim3(1, parts), 256, 0, s>>>(x, dy, partial, n, g.HW, g.W, g.tapmask);
  const int64_t count = (int64_t)taps * kF * kF;
  reduce_parts_kernel<<<blocks(count, 256), 256, 0, s>>>(partial, parts, count, dw);
}

void stem_forward(hipStream_t s, const Geo& g, const float* x, const float* w, const float* bias, float* y,
                  int rows) {
  stem_forward_kernel<<<blocks((int64_t)rows * kF, 256), 256, 0, s>>>(x, w, bias, y, rows, g.HW, g.W, g.tapmask);
}

void stem_wgrad(hipStream_t s, const Geo& g, const float* x, const float* dy, float* partial, float* dw, int rows) {
  const int parts = row_parts(rows);
  stem_wgrad_kernel<<<dim3(36 * kF / 256, parts), 256, 0, s>>>(x, dy, partial, rows, g.HW, g.W, g.tapmask);
  reduce_parts_kernel<<<blocks(36 * kF, 256), 256, 0, s>>>(partial, parts, 36 * kF, dw);
}

void chess_stem_forward(hipStream_t s, const Geo& g, const float* x, const float* w, const float* bias, float* y,
                        int rows) {
  chess_stem_forward_kernel<<<blocks(rows, 32), 256, 0, s>>>(x, w, bias, y, rows, g.HW, g.W, g.tapmask);
}

void chess_stem_wgrad(hipStream_t s, const Geo& g, const float* x, const float* dy, float* partial, float* dw,
                      int n) {
  const int parts = board_parts(n);
  chess_stem_wgrad_kernel<<<dim3(9, parts), 256, 0, s>>>(x, dy, partial, n, g.tapmask);
  const int64_t count = (int64_t)9 * kChessPlanes * kF;
  reduce_parts_kernel<<<blocks(count, 256), 256, 0, s>>>(partial, parts, count, dw);
}

void headconv_forward(hipStream_t s, const float* h, const float* wp, const float* bp, const float* wv,
                      const float* bv, float* yp, float* yv, int rows) {
  headconv_forward_kernel<<<blocks(rows, 4), 256, 0, s>>>(h, wp, bp, wv, bv, yp, yv, rows);
}

void headconv_wgrad(hipStream_t s, const float* h, const float* dyp, const float* dyv, float* partial, float* dwp,
                    float* dwv, int rows) {
  const int parts = row_parts(rows);
  headconv_wgrad_kernel<<<parts, kF, 0, s>>>(h, dyp, dyv, partial, rows);
  // a part's 384 floats are [policy 256][value 128]: reduce each range into its tensor
  reduce_parts_kernel<<<2, 256, 0, s>>>(partial, parts, 384, dwp);
  (void)dwv;  // dwp and dwv are adjacent (see az_trainer_create: value.conv.kernel follows policy.conv.kernel)
}

void headconv_dgrad(hipStream_t s, const float* dyp, const float* dyv, const float* wp, const float* wv, float* dh,
                    int rows) {
  headconv_dgrad_kernel<<<blocks((int64_t)rows * kF, 256), 256, 0, s>>>(dyp, dyv, wp, wv, dh, rows);
}

void bn_stats(hipStream_t s, const float* y, int rows, int C, float eps, float* partial, float* mean, float* var,
              float* invstd) {
  const int parts = row_parts(rows);
  const int CT = C < 64 ? 64 : kF;
  double* dpart = reinterpret_cast<double*>(partial);  // float64 partial sums (4 * parts * C floats at most)
  bn_sum_kernel<0><<<parts, CT * kPhases, 0, s>>>(y, nullptr, dpart, rows, C, CT);
  bn_stats_final_kernel<0><<<blocks(C, 32), 256, 0, s>>>(dpart, parts, rows, C, eps, mean, var, invstd);
  bn_sum_kernel<1><<<parts, CT * kPhases, 0, s>>>(y, mean, dpart, rows, C, CT);
  bn_stats_final_kernel<1><<<blocks(C, 32), 256, 0, s>>>(dpart, parts, rows, C, eps, mean, var, invstd);
}

void bn_apply(hipStream_t s, const float* y, const float* mean, const float* invstd, const float* gamma,
              const float* beta, const float* y2, const float* mean2, const float* invstd2, const float* gamma2,
              const float* beta2, bool relu, float* out, int rows, int C) {
  const int64_t total = (int64_t)rows * C;
  bn_apply_kernel<<<blocks(total, 256), 256, 0, s>>>(y, mean, invstd, gamma, beta, y2, mean2, invstd2, gamma2, beta2,
                                                     relu ? 1 : 0, out, total, C);
}

void bn_backward(hipStream_t s, const float* g, const float* mask_out, const float* y, const float* mean,
                 const float* invstd, const float* gamma, float* partial, float* dgamma, float* dbeta, float* dy,
                 int rows, int C) {
  const int parts = row_parts(rows);
  const int CT = C < 64 ? 64 : kF;
  double* dpart = reinterpret_cast<double*>(partial);
  bn_bwd_sum_kernel<<<parts, CT * kPhases, 0, s>>>(g, mask_out, y, mean, invstd, dpart, rows, C, CT);
  bn_bwd_final_kernel<<<blocks(C, 32), 256, 0, s>>>(dpart, parts, C, dgamma, dbeta);
  const int64_t total = (int64_t)rows * C;
  bn_bwd_apply_kernel<<<blocks(total, 256), 256, 0, s>>>(g, mask_out, y, mean, invstd, gamma, dgamma, dbeta, dy,
                                                         total, C, 1.0f / (float)rows);
}

void heads_forward_backward(hipStream_t s, const Geo& g, const HeadsArgs& a, int n) {
  heads_kernel<<<n, 256, 0, s>>>(a, n, g.HW, g.A, g.hidden);
}

void chess_heads_forward_backward(hipStream_t s, const Geo& g, const HeadsArgs& a, int n) {
  chess_heads_kernel<<<n, 256, 0, s>>>(a, n, g.hidden);
}

void dense_wgrad(hipStream_t s, const float* x, const float* d, float* dw, float* db, int n, int I, int J) {
  dense_wgrad_kernel<<<blocks((int64_t)(I + 1) * J, 256), 256, 0, s>>>(x, d, dw, db, n, I, J);
}

void chess_policy_wgrad(hipStream_t s, const float* x, const float* d, float* dw, float* db, int n) {
  chess_policy_wgrad_kernel<<<dim3(blocks(kChessActions, 256), 2 * kChessCells / 8), 256, 0, s>>>(x, d, dw, db, n);
}

void losses(hipStream_t s, const float* w, int64_t n_l2, double l2, const float* lossp, const float* lossv, int n,
            double* sq_partial, float* out) {
  const int parts = (int)blocks(n_l2, 4096);
  sqsum_kernel<<<parts, 256, 0, s>>>(w, n_l2, sq_partial);
  loss_final_kernel<<<1, 64, 0, s>>>(sq_partial, parts, l2, lossp, lossv, n, out);
}

void sgd_update(hipStream_t s, float* w, float* g, float* m, int64_t n_train, int64_t n_l2, float lr, float mom,
                float l2) {
  sgd_update_kernel<<<blocks(n_train, 256), 256, 0, s>>>(w, g, m, n_train, n_l2, lr, mom, 2.0f * l2);
}

void moving_update(hipStream_t s, float* moving, const float* batch, int64_t n_stats, float m, float take,
                   float var_factor) {
  moving_update_kernel<<<blocks(2 * n_stats, 256), 256, 0, s>>>(moving, batch, n_stats, m, take, var_factor);
}

}  // namespace train
}  // namespace az

// ====================================================================== C ABI
namespace {

using az::fail_abi;
namespace T = az::train;

struct Tensor {
  int64_t off = 0, numel = 0;
  bool trainable = true;
};

// One InnerConvBlock: conv + bias -> BatchNormalization (-> ReLU)
struct Unit {
  std::string name;
  int taps = 9, cin = T::kF, cout = T::kF;
  int64_t kernel = 0, bias = 0, gamma = 0, beta = 0;  // offsets into the parameter blob
  int64_t stat = 0;                                   // offset of this unit's channels in the statistics
  float* y = nullptr;                                 // pre-BN output [rows][cout], kept for the backward
};

}  // namespace

struct az_trainer {
  int device = 0;
  hipStream_t stream = nullptr;
  az_config cfg{};
  int max_batch = 0, depth = 0;
  int cin = 4;  // input planes: 4 (Connect-N) or 118 (chess, with its own stem and heads kernels)
  int A = 0;    // actions: W or H*W (Connect-N), 1880 (chess)
  T::Geo geo{};
  bool has_weights = false;
  std::map<std::string, Tensor> tensors;
  std::vector<Unit> units;  // stem, block d: conv1, conv2, res, ..., policy.conv, value.conv
  int64_t n_l2 = 0, n_train = 0, n_stats = 0;
  // blob: [.kernel tensors (L2) | other trainables | moving means | moving variances]
  float *w = nullptr, *g = nullptr, *m = nullptr;
  float *bmean = nullptr, *bvar = nullptr, *invstd = nullptr;  // batch statistics [2 * n_stats] (mean | var), [n_stats]
  float* x = nullptr;
  float *pi = nullptr, *z = nullptr;
  std::vector<float*> h;   // h[0] the stem's output, h[d + 1] block d's
  std::vector<float*> a1;  // block d's conv1 output after BN + ReLU
  float *hp = nullptr, *hv = nullptr;
  float *ga = nullptr, *gb = nullptr, *dy1 = nullptr, *dy2 = nullptr;  // [rows][F] gradient scratch
  float *ghp = nullptr, *ghv = nullptr, *dyp = nullptr, *dyv = nullptr;
  float *dlogit = nullptr, *d1 = nullptr, *dpre1 = nullptr, *dpre2 = nullptr, *lossp = nullptr, *lossv = nullptr;
  float* partial = nullptr;
  double* sq_partial = nullptr;
  float* losses = nullptr;
  uint16_t* tapmask = nullptr;
  az::DeviceAllocs mem;  // every buffer starts zeroed
};

namespace {

void free_trainer(az_trainer* tr) {
  (void)hipSetDevice(tr->device);
  if (tr->stream) (void)hipStreamSynchronize(tr->stream);
  tr->mem.free_all();
  if (tr->stream) (void)hipStreamDestroy(tr->stream);
  delete tr;
}

int build_trainer(az_trainer* tr) {
  const az_config& c = tr->cfg;
  const int H = c.board_height, W = c.board_width, HW = H * W, F = T::kF;
  const int A = tr->A, hidden = c.value_hidden, depth = c.depth;
  // ---- the tensor table: weights.weight_spec's names; .kernel tensors first (the L2 range)
  std::vector<Unit>& U = tr->units;
  auto add_unit = [&](const std::string& name, int taps, int cin, int cout) {
    Unit u;
    u.name = name, u.taps = taps, u.cin = cin, u.cout = cout;
    U.push_back(u);
  };
  add_unit("stem", 9, tr->cin, F);
  for (int d = 0; d < depth; ++d) {
    const std::string b = "block" + std::to_string(d);
    add_unit(b + ".conv1", 9, F, F);
    add_unit(b + ".conv2", 9, F, F);
    add_unit(b + ".res", 1, F, F);
  }
  add_unit("policy.conv", 1, F, 2);
  add_unit("value.conv", 1, F, 1);  // must follow policy.conv: headconv_wgrad writes both kernels' gradients at once
  int64_t off = 0;
  auto place = [&](const std::string& name, int64_t numel, bool trainable) {
    Tensor t;
    t.off = off, t.numel = numel, t.trainable = trainable;
    tr->tensors[name] = t;
    off += numel;
    return t.off;
  };
  for (Unit& u : U) u.kernel = place(u.name + ".kernel", (int64_t)u.taps * u.cin * u.cout, true);
  place("policy.dense.kernel", (int64_t)2 * HW * A, true);
  place("value.dense1.kernel", (int64_t)HW * hidden, true);
  place("value.dense2.kernel", hidden, true);
  tr->n_l2 = off;
  for (Unit& u : U) {
    u.bias = place(u.name + ".bias", u.cout, true);
    u.gamma = place(u.name + ".gamma", u.cout, true);
    u.beta = place(u.name + ".beta", u.cout, true);
  }
  place("policy.dense.bias", A, true);
  place("value.dense1.bias", hidden, true);
  place("value.dense2.bias", 1, true);
  tr->n_train = off;
  int64_t ns = 0;
  for (Unit& u : U) {
    u.stat = ns;
    ns += u.cout;
  }
  tr->n_stats = ns;
  for (Unit& u : U) place(u.name + ".mean", u.cout, false);
  for (Unit& u : U) place(u.name + ".var", u.cout, false);
  if (off != tr->n_train + 2 * ns) return fail_abi(AZ_E_STATE, "az_trainer: tensor table size");

  // ---- device memory, once for max_batch
  const size_t rows = (size_t)tr->max_batch * HW, B = tr->max_batch;
  AZ_TRY(tr->mem.alloc(&tr->w, off, true));
  AZ_TRY(tr->mem.alloc(&tr->g, tr->n_train, true));
  AZ_TRY(tr->mem.alloc(&tr->m, tr->n_train, true));
  AZ_TRY(tr->mem.alloc(&tr->bmean, 2 * ns, true));
  tr->bvar = tr->bmean + ns;
  AZ_TRY(tr->mem.alloc(&tr->invstd, ns, true));
  AZ_TRY(tr->mem.alloc(&tr->x, rows * tr->cin, true));
  AZ_TRY(tr->mem.alloc(&tr->pi, B * A, true));
  AZ_TRY(tr->mem.alloc(&tr->z, B, true));
  for (Unit& u : U) AZ_TRY(tr->mem.alloc(&u.y, rows * u.cout, true));
  tr->h.resize(depth + 1);
  tr->a1.resize(depth);
  for (auto& p : tr->h) AZ_TRY(tr->mem.alloc(&p, rows * F, true));
  for (auto& p : tr->a1) AZ_TRY(tr->mem.alloc(&p, rows * F, true));
  AZ_TRY(tr->mem.alloc(&tr->hp, rows * 2, true));
  AZ_TRY(tr->mem.alloc(&tr->hv, rows, true));
  AZ_TRY(tr->mem.alloc(&tr->ga, rows * F, true));
  AZ_TRY(tr->mem.alloc(&tr->gb, rows * F, true));
  AZ_TRY(tr->mem.alloc(&tr->dy1, rows * F, true));
  AZ_TRY(tr->mem.alloc(&tr->dy2, rows * F, true));
  AZ_TRY(tr->mem.alloc(&tr->ghp, rows * 2, true));
  AZ_TRY(tr->mem.alloc(&tr->ghv, rows, true));
  AZ_TRY(tr->mem.alloc(&tr->dyp, rows * 2, true));
  AZ_TRY(tr->mem.alloc(&tr->dyv, rows, true));
  AZ_TRY(tr->mem.alloc(&tr->dlogit, B * A, true));
  AZ_TRY(tr->mem.alloc(&tr->d1, B * hidden, true));
  AZ_TRY(tr->mem.alloc(&tr->dpre1, B * hidden, true));
  AZ_TRY(tr->mem.alloc(&tr->dpre2, B, true));
  AZ_TRY(tr->mem.alloc(&tr->lossp, B, true));
  AZ_TRY(tr->mem.alloc(&tr->lossv, B, true));
  AZ_TRY(tr->mem.alloc(&tr->losses, 4, true));
  const size_t rp = T::row_parts((int)rows), bp = T::board_parts(tr->max_batch);
  // the stem's split-K parts: rows of 64 (Connect-N, 36 x F) or boards of 8 (chess, 9 x 118 x F)
  const size_t stem_partial = tr->cin == T::kChessPlanes ? bp * 9 * T::kChessPlanes * F : rp * 36 * F;
  const size_t partial = std::max(std::max(bp * 9 * F * F, stem_partial), std::max(rp * 4 * F, rp * 384));
  AZ_TRY(tr->mem.alloc(&tr->partial, partial, true));
  AZ_TRY(tr->mem.alloc(&tr->sq_partial, (size_t)(tr->n_l2 + 4095) / 4096, true));
  AZ_TRY(tr->mem.alloc(&tr->tapmask, HW, true));
  std::vector<uint16_t> mask(HW);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      int mk = 0;
      for (int t = 0; t < 9; ++t) {
        const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) mk |= 1 << t;
      }
      mask[y * W + x] = (uint16_t)mk;
    }
  AZ_HIP(hipMemcpy(tr->tapmask, mask.data(), HW * sizeof(uint16_t), hipMemcpyHostToDevice));
  tr->geo = T::Geo{H, W, HW, A, hidden, tr->tapmask};
  AZ_HIP(hipStreamCreateWithFlags(&tr->stream, hipStreamNonBlocking));
  AZ_HIP(hipDeviceSynchronize());  // the allocations' memsets ran on the null stream
  return AZ_OK;
}

// The step on the batch already in tr->x, tr->pi, tr->z (n boards) on tr's stream, and the wait for
// it: what az_trainer_step runs after its copies and az_trainer_step_replay after its gather.
int step_on_device_batch(az_trainer* tr, int n, double lr, double momentum, double l2, double bn_momentum,
                         float* losses) {
  hipStream_t s = tr->stream;
  const T::Geo& g = tr->geo;
  const int HW = g.HW, A = g.A, hidden = g.hidden, depth = tr->depth;
  const int rows = n * HW;
  const float eps = (float)tr->cfg.bn_epsilon;
  const bool chess = tr->cin == T::kChessPlanes;
  float *w = tr->w, *gr = tr->g;
  auto tw = [&](const char* name) { return w + tr->tensors[name].off; };
  auto tg = [&](const char* name) { return gr + tr->tensors[name].off; };
  auto stats = [&](const Unit& u) {
    T::bn_stats(s, u.y, rows, u.cout, eps, tr->partial, tr->bmean + u.stat, tr->bvar + u.stat, tr->invstd + u.stat);
  };
  auto apply = [&](const Unit& u, const Unit* u2, bool relu, float* out) {
    T::bn_apply(s, u.y, tr->bmean + u.stat, tr->invstd + u.stat, w + u.gamma, w + u.beta, u2 ? u2->y : nullptr,
                u2 ? tr->bmean + u2->stat : nullptr, u2 ? tr->invstd + u2->stat : nullptr,
                u2 ? w + u2->gamma : nullptr, u2 ? w + u2->beta : nullptr, relu, out, rows, u.cout);
  };
  auto bn_bwd = [&](const Unit& u, const float* gin, const float* mask_out, float* dy) {
    T::bn_backward(s, gin, mask_out, u.y, tr->bmean + u.stat, tr->invstd + u.stat, w + u.gamma, tr->partial,
                   gr + u.gamma, gr + u.beta, dy, rows, u.cout);
  };
  std::vector<Unit>& U = tr->units;
  Unit& stem = U[0];
  Unit& upol = U[1 + 3 * depth];
  Unit& uval = U[2 + 3 * depth];

  // ---- forward
  if (chess)
    T::chess_stem_forward(s, g, tr->x, w + stem.kernel, w + stem.bias, stem.y, rows);
  else
    T::stem_forward(s, g, tr->x, w + stem.kernel, w + stem.bias, stem.y, rows);
  stats(stem);
  apply(stem, nullptr, true, tr->h[0]);
  for (int d = 0; d < depth; ++d) {
    Unit &c1 = U[1 + 3 * d], &c2 = U[2 + 3 * d], &rs = U[3 + 3 * d];
    T::conv_forward(s, g, 9, tr->h[d], w + c1.kernel, w + c1.bias, c1.y, rows);
    stats(c1);
    apply(c1, nullptr, true, tr->a1[d]);
    T::conv_forward(s, g, 9, tr->a1[d], w + c2.kernel, w + c2.bias, c2.y, rows);
    stats(c2);
    T::conv_forward(s, g, 1, tr->h[d], w + rs.kernel, w + rs.bias, rs.y, rows);
    stats(rs);
    apply(c2, &rs, true, tr->h[d + 1]);
  }
  const float* top = tr->h[depth];
  T::headconv_forward(s, top, w + upol.kernel, w + upol.bias, w + uval.kernel, w + uval.bias, upol.y, uval.y, rows);
  stats(upol);
  stats(uval);
  apply(upol, nullptr, true, tr->hp);
  apply(uval, nullptr, true, tr->hv);

  // ---- heads: dense layers, losses and their gradients
  T::HeadsArgs ha{};
  ha.hp = tr->hp, ha.hv = tr->hv;
  ha.wpd = tw("policy.dense.kernel"), ha.bpd = tw("policy.dense.bias");
  ha.wv1 = tw("value.dense1.kernel"), ha.bv1 = tw("value.dense1.bias");
  ha.wv2 = tw("value.dense2.kernel"), ha.bv2 = tw("value.dense2.bias");
  ha.pi = tr->pi, ha.z = tr->z;
  ha.dlogit = tr->dlogit, ha.d1 = tr->d1, ha.dpre1 = tr->dpre1, ha.dpre2 = tr->dpre2;
  ha.ghp = tr->ghp, ha.ghv = tr->ghv, ha.lossp = tr->lossp, ha.lossv = tr->lossv;
  if (chess)
    T::chess_heads_forward_backward(s, g, ha, n);
  else
    T::heads_forward_backward(s, g, ha, n);
  T::losses(s, w, tr->n_l2, l2, tr->lossp, tr->lossv, n, tr->sq_partial, tr->losses);
  if (chess)
    T::chess_policy_wgrad(s, tr->hp, tr->dlogit, tg("policy.dense.kernel"), tg("policy.dense.bias"), n);
  else
    T::dense_wgrad(s, tr->hp, tr->dlogit, tg("policy.dense.kernel"), tg("policy.dense.bias"), n, 2 * HW, A);
  T::dense_wgrad(s, tr->hv, tr->dpre1, tg("value.dense1.kernel"), tg("value.dense1.bias"), n, HW, hidden);
  T::dense_wgrad(s, tr->d1, tr->dpre2, tg("value.dense2.kernel"), tg("value.dense2.bias"), n, hidden, 1);

  // ---- backward through the head convs into the tower's output
  bn_bwd(upol, tr->ghp, tr->hp, tr->dyp);
  bn_bwd(uval, tr->ghv, tr->hv, tr->dyv);
  T::headconv_wgrad(s, top, tr->dyp, tr->dyv, tr->partial, gr + upol.kernel, gr + uval.kernel, rows);
  float *gh = tr->ga, *gx = tr->gb;  // gradient of h[d + 1]; scratch
  T::headconv_dgrad(s, tr->dyp, tr->dyv, w + upol.kernel, w + uval.kernel, gh, rows);
  // the bias of a conv in front of a training-mode BN has an exactly zero gradient: the
  // gradient blob's bias entries of every unit stay at the zeros they were allocated with

  // ---- backward through the tower
  for (int d = depth - 1; d >= 0; --d) {
    Unit &c1 = U[1 + 3 * d], &c2 = U[2 + 3 * d], &rs = U[3 + 3 * d];
    bn_bwd(c2, gh, tr->h[d + 1], tr->dy2);
    T::conv_wgrad(s, g, 9, tr->a1[d], tr->dy2, tr->partial, gr + c2.kernel, n);
    T::conv_dgrad(s, g, 9, tr->dy2, w + c2.kernel, nullptr, nullptr, gx, rows);  // gradient of a1
    bn_bwd(rs, gh, tr->h[d + 1], tr->dy2);                                       // dy of the projection
    T::conv_wgrad(s, g, 1, tr->h[d], tr->dy2, tr->partial, gr + rs.kernel, n);
    bn_bwd(c1, gx, tr->a1[d], tr->dy1);
    T::conv_wgrad(s, g, 9, tr->h[d], tr->dy1, tr->partial, gr + c1.kernel, n);
    T::conv_dgrad(s, g, 9, tr->dy1, w + c1.kernel, tr->dy2, w + rs.kernel, gx, rows);  // gradient of h[d]
    std::swap(gh, gx);
  }
  bn_bwd(stem, gh, tr->h[0], tr->dy1);
  if (chess)
    T::chess_stem_wgrad(s, g, tr->x, tr->dy1, tr->partial, gr + stem.kernel, n);
  else
    T::stem_wgrad(s, g, tr->x, tr->dy1, tr->partial, gr + stem.kernel, rows);

  // ---- update
  T::sgd_update(s, w, gr, tr->m, tr->n_train, tr->n_l2, (float)lr, (float)momentum, (float)l2);
  // 1 - m: the Connect-N trainer keeps the fp32 difference it has always used (1 - 0.99f is 9.5e-7
  // short of 0.01); the chess trainer rounds the float64 difference once.  A moving mean is one
  // scalar a channel, m * mean + (1 - m) * mu can cancel, and with the chess test's value head
  // (0.0035 left of terms of 0.018) the short factor alone put it 1.8e-6 from float64.
  const float take = chess ? (float)(1.0 - bn_momentum) : 1.0f - (float)bn_momentum;
  T::moving_update(s, w + tr->n_train, tr->bmean, tr->n_stats, (float)bn_momentum, take,
                   (float)T::moving_variance_factor(rows));
  AZ_HIP(hipGetLastError());
  float host_losses[3];
  AZ_HIP(hipMemcpyAsync(host_losses, tr->losses, sizeof(host_losses), hipMemcpyDeviceToHost, s));
  AZ_HIP(hipStreamSynchronize(s));
  if (losses) memcpy(losses, host_losses, sizeof(host_losses));
  return AZ_OK;
}

}  // namespace

extern "C" {

int az_trainer_create(int device, const az_config* cfg, int max_batch, az_trainer** out) {
  if (!cfg || !out) return fail_abi(AZ_E_INVALID, "az_trainer_create: null argument");
  const az_config& c = *cfg;
  if (c.board_height < 2 || c.board_width < 2 || c.board_height * c.board_width > T::kMaxCellsTrain)
    return fail_abi(AZ_E_INVALID, "az_trainer_create: board must be at least 2x2 and at most 128 cells");
  if (c.filters != T::kF) return fail_abi(AZ_E_INVALID, "az_trainer_create: only filters = 128 is implemented");
  if (c.depth < 1 || c.depth > 16) return fail_abi(AZ_E_INVALID, "az_trainer_create: depth must be 1..16");
  if (c.value_hidden < 1 || c.value_hidden > T::kMaxHidden)
    return fail_abi(AZ_E_INVALID, "az_trainer_create: value_hidden must be 1..1024");
  if (!(c.bn_epsilon > 0)) return fail_abi(AZ_E_INVALID, "az_trainer_create: bn_epsilon must be positive");
  if (max_batch < 1 || (int64_t)max_batch * c.board_height * c.board_width * T::kF >= (1ll << 31))
    return fail_abi(AZ_E_INVALID, "az_trainer_create: max_batch must be >= 1 and max_batch*H*W*128 < 2^31");
  if (device < 0) return fail_abi(AZ_E_INVALID, "az_trainer_create: bad device ordinal");
  AZ_TRY(az::open_device(device, "az_trainer_create: device ordinal out of range"));
  az_trainer* tr = new az_trainer();
  tr->device = device;
  tr->cfg = c;
  tr->max_batch = max_batch;
  tr->depth = c.depth;
  tr->cin = 4;
  tr->A = c.gravity ? c.board_width : c.board_height * c.board_width;
  const int rc = build_trainer(tr);
  if (rc != AZ_OK) {
    free_trainer(tr);
    return rc;
  }
  *out = tr;
  return AZ_OK;
}

int az_chess_trainer_create(int device, const az_chess_config* cfg, int max_batch, az_trainer** out) {
  if (!cfg || !out) return fail_abi(AZ_E_INVALID, "az_chess_trainer_create: null argument");
  if (cfg->filters != T::kF)
    return fail_abi(AZ_E_INVALID, "az_chess_trainer_create: only filters = 128 is implemented");
  if (cfg->depth < 1 || cfg->depth > 16)
    return fail_abi(AZ_E_INVALID, "az_chess_trainer_create: depth must be 1..16");
  if (cfg->value_hidden < 1 || cfg->value_hidden > T::kMaxHidden)
    return fail_abi(AZ_E_INVALID, "az_chess_trainer_create: value_hidden must be 1..1024");
  if (!(cfg->bn_epsilon > 0)) return fail_abi(AZ_E_INVALID, "az_chess_trainer_create: bn_epsilon must be positive");
  if (max_batch < 1 || (int64_t)max_batch * T::kChessCells * T::kF >= (1ll << 31))
    return fail_abi(AZ_E_INVALID, "az_chess_trainer_create: max_batch must be >= 1 and max_batch*64*128 < 2^31");
  if (device < 0) return fail_abi(AZ_E_INVALID, "az_chess_trainer_create: bad device ordinal");
  AZ_TRY(az::open_device(device, "az_chess_trainer_create: device ordinal out of range"));
  az_trainer* tr = new az_trainer();
  tr->device = device;
  // the shared code reads the board and the network's sizes from an az_config
  tr->cfg.board_height = tr->cfg.board_width = 8;
  tr->cfg.filters = cfg->filters;
  tr->cfg.depth = cfg->depth;
  tr->cfg.value_hidden = cfg->value_hidden;
  tr->cfg.bn_epsilon = cfg->bn_epsilon;
  tr->max_batch = max_batch;
  tr->depth = cfg->depth;
  tr->cin = T::kChessPlanes;
  tr->A = T::kChessActions;
  const int rc = build_trainer(tr);
  if (rc != AZ_OK) {
    free_trainer(tr);
    return rc;
  }
  *out = tr;
  return AZ_OK;
}

int az_trainer_destroy(az_trainer* tr) {
  if (!tr) return AZ_OK;
  free_trainer(tr);
  return AZ_OK;
}

int az_trainer_set_weights(az_trainer* tr, const az_tensor* tensors, int n) {
  if (!tr || !tensors) return fail_abi(AZ_E_INVALID, "az_trainer_set_weights: null argument");
  if (n != (int)tr->tensors.size())
    return fail_abi(AZ_E_INVALID, "az_trainer_set_weights: expected " + std::to_string(tr->tensors.size()) +
                                      " tensors, got " + std::to_string(n));
  std::map<std::string, int> seen;
  for (int i = 0; i < n; ++i) {
    if (!tensors[i].name || !tensors[i].data) return fail_abi(AZ_E_INVALID, "az_trainer_set_weights: null tensor");
    auto it = tr->tensors.find(tensors[i].name);
    if (it == tr->tensors.end())
      return fail_abi(AZ_E_INVALID, std::string("az_trainer_set_weights: unknown tensor ") + tensors[i].name);
    if (it->second.numel != tensors[i].numel)
      return fail_abi(AZ_E_INVALID, std::string("az_trainer_set_weights: wrong numel for ") + tensors[i].name);
    if (seen[tensors[i].name]++)
      return fail_abi(AZ_E_INVALID, std::string("az_trainer_set_weights: duplicate tensor ") + tensors[i].name);
  }
  AZ_HIP(hipSetDevice(tr->device));
  AZ_HIP(hipStreamSynchronize(tr->stream));
  for (int i = 0; i < n; ++i) {
    const Tensor& t = tr->tensors[tensors[i].name];
    AZ_HIP(hipMemcpy(tr->w + t.off, tensors[i].data, t.numel * sizeof(float),
                     tensors[i].on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  }
  AZ_HIP(hipDeviceSynchronize());
  tr->has_weights = true;
  return AZ_OK;
}

int az_trainer_reset_momentum(az_trainer* tr) {
  if (!tr) return fail_abi(AZ_E_INVALID, "az_trainer_reset_momentum: null trainer");
  AZ_HIP(hipSetDevice(tr->device));
  AZ_HIP(hipMemsetAsync(tr->m, 0, tr->n_train * sizeof(float), tr->stream));
  AZ_HIP(hipStreamSynchronize(tr->stream));
  return AZ_OK;
}

int az_trainer_read(az_trainer* tr, int what, const char* name, float* out, int64_t numel) {
  if (!tr || !name || !out) return fail_abi(AZ_E_INVALID, "az_trainer_read: null argument");
  auto it = tr->tensors.find(name);
  if (it == tr->tensors.end()) return fail_abi(AZ_E_INVALID, std::string("az_trainer_read: unknown tensor ") + name);
  const Tensor& t = it->second;
  if (t.numel != numel) return fail_abi(AZ_E_INVALID, std::string("az_trainer_read: wrong numel for ") + name);
  const float* src = nullptr;
  if (what == AZ_TRAIN_WEIGHT)
    src = tr->w;
  else if ((what == AZ_TRAIN_GRAD || what == AZ_TRAIN_MOMENTUM) && t.trainable)
    src = what == AZ_TRAIN_GRAD ? tr->g : tr->m;
  else
    return fail_abi(AZ_E_INVALID, "az_trainer_read: `what` must be AZ_TRAIN_WEIGHT, or GRAD / MOMENTUM of a "
                                  "trainable tensor");
  AZ_HIP(hipSetDevice(tr->device));
  AZ_HIP(hipStreamSynchronize(tr->stream));
  AZ_HIP(hipMemcpy(out, src + t.off, numel * sizeof(float), hipMemcpyDeviceToHost));
  return AZ_OK;
}

int az_trainer_step(az_trainer* tr, const float* x, const float* pi, const float* z, int n, double lr,
                    double momentum, double l2, double bn_momentum, float* losses) {
  if (!tr || !x || !pi || !z) return fail_abi(AZ_E_INVALID, "az_trainer_step: null argument");
  // one board is a batch: every BatchNormalization takes its statistics over the n*H*W rows
  if (n < 1 || n > tr->max_batch) return fail_abi(AZ_E_INVALID, "az_trainer_step: n must be 1..max_batch");
  if (!tr->has_weights) return fail_abi(AZ_E_STATE, "az_trainer_step: no weights (az_trainer_set_weights first)");
  AZ_HIP(hipSetDevice(tr->device));
  hipStream_t s = tr->stream;
  const size_t rows = (size_t)n * tr->geo.HW;
  AZ_HIP(hipMemcpyAsync(tr->x, x, rows * tr->cin * sizeof(float), hipMemcpyHostToDevice, s));
  AZ_HIP(hipMemcpyAsync(tr->pi, pi, (size_t)n * tr->geo.A * sizeof(float), hipMemcpyHostToDevice, s));
  AZ_HIP(hipMemcpyAsync(tr->z, z, (size_t)n * sizeof(float), hipMemcpyHostToDevice, s));
  return step_on_device_batch(tr, n, lr, momentum, l2, bn_momentum, losses);
}

int az_trainer_step_replay(az_trainer* tr, az_chess_replay* rp, const int64_t* idx, int n, double lr,
                           double momentum, double l2, double bn_momentum, float* losses) {
  if (!tr || !rp || !idx) return fail_abi(AZ_E_INVALID, "az_trainer_step_replay: null argument");
  if (tr->cin != T::kChessPlanes)
    return fail_abi(AZ_E_INVALID, "az_trainer_step_replay: the trainer is not the chess network's "
                                  "(az_chess_trainer_create)");
  if (n < 1 || n > tr->max_batch)
    return fail_abi(AZ_E_INVALID, "az_trainer_step_replay: n must be 1..max_batch");
  if (!tr->has_weights)
    return fail_abi(AZ_E_STATE, "az_trainer_step_replay: no weights (az_trainer_set_weights first)");
  if (az::replay::device_of(rp) != tr->device)
    return fail_abi(AZ_E_INVALID, "az_trainer_step_replay: the replay is on another device than the trainer");
  AZ_HIP(hipSetDevice(tr->device));
  // the batch goes from the window straight into the step's own input buffers
  AZ_TRY(az::replay::gather_on(rp, idx, n, tr->stream, tr->x, tr->pi, tr->z, "az_trainer_step_replay"));
  return step_on_device_batch(tr, n, lr, momentum, l2, bn_momentum, losses);
}

}  // extern "C"
