// az_replay.hip -- the chess replay window on the device: az_chess_replay_*
// (include/az_chess.h) and the gather kernel az_trainer_step_replay launches
// (az_replay.h).  Samples are held as self-play hands them over (80-byte
// positions, the sparse MCTS policy), about 3.2 KB each; a training batch is
// gathered, encoded and scattered to its dense form by one launch.
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/az.h"
#include "az_chess.h"
#include "az_host.h"
#include "az_replay.h"

using az::fail_abi;

// Ring slot of window index i (0 = oldest) is (head + i) % cap.  One thread
// drives a replay: no call runs beside another on the same handle.
struct az_chess_replay {
  int device = 0;
  hipStream_t stream = nullptr;
  int64_t cap = 0, head = 0, size = 0;
  az_chess_pos* hist = nullptr;  // [cap][8]
  uint8_t* valid = nullptr;      // [cap][8]
  int32_t* policy_n = nullptr;   // [cap]
  int16_t* actions = nullptr;    // [cap][256]
  double* probs = nullptr;       // [cap][256]
  float* z = nullptr;            // [cap]
  int64_t* idx = nullptr;        // [idx_cap]: the batch indices of the launch in flight
  int idx_cap = 0;
  az::DeviceAllocs mem;
};

namespace azc {

constexpr int kGatherThreads = 256;
static_assert(kGatherThreads >= AZ_CHESS_MAX_MOVES, "one thread per policy entry");
static_assert(AZ_CHESS_ACTIONS % 4 == 0 && (64 * AZ_CHESS_PLANES) % 4 == 0, "16-byte rows");

// One workgroup per batch row: the sample at window index idx[row] as the
// trainer takes it.  x: Board.full_state by encode_kernel's arithmetic
// (full_state_block).  pi: the dense row built in LDS -- zero, barrier,
// row[action[j]] = (float)prob[j] (round to nearest, as numpy's astype), barrier
// -- and stored 16 bytes a lane; push refused repeated and out-of-range actions,
// so the scatter has no write conflict and needs no range check.  z: copied.
__global__ void __launch_bounds__(kGatherThreads)
    gather_kernel(const az_chess_pos* __restrict__ hist, const uint8_t* __restrict__ valid,
                  const int32_t* __restrict__ policy_n, const int16_t* __restrict__ actions,
                  const double* __restrict__ probs, const float* __restrict__ zs, long long head, long long cap,
                  const int64_t* __restrict__ idx, float* __restrict__ x, float* __restrict__ pi,
                  float* __restrict__ z) {
  __shared__ FullStateLds lds;
  __shared__ __attribute__((aligned(16))) float prow[AZ_CHESS_ACTIONS];
  const int row = blockIdx.x, tid = threadIdx.x;
  const size_t slot = (size_t)((head + idx[row]) % cap);
  if (pi) {
    const int pn = policy_n[slot];
    int a = 0;
    float p = 0.f;
    if (tid < pn) {
      a = actions[slot * AZ_CHESS_MAX_MOVES + tid];
      p = (float)probs[slot * AZ_CHESS_MAX_MOVES + tid];
    }
    for (int i = tid; i < AZ_CHESS_ACTIONS; i += kGatherThreads) prow[i] = 0.f;
    __syncthreads();
    if (tid < pn) prow[a] = p;
    __syncthreads();
    float4* o = reinterpret_cast<float4*>(pi + (size_t)row * AZ_CHESS_ACTIONS);
    const float4* r = reinterpret_cast<const float4*>(prow);
    for (int i = tid; i < AZ_CHESS_ACTIONS / 4; i += kGatherThreads) o[i] = r[i];
  }
  if (z && tid == 0) z[row] = zs[slot];
  if (x)
    full_state_block(lds, hist + slot * AZ_CHESS_HISTORY, valid + slot * AZ_CHESS_HISTORY,
                     x + (size_t)row * 64 * AZ_CHESS_PLANES);
}

}  // namespace azc

namespace {

void free_replay(az_chess_replay* rp) {
  (void)hipSetDevice(rp->device);
  if (rp->stream) (void)hipStreamSynchronize(rp->stream);
  rp->mem.free_all();
  if (rp->idx) (void)hipFree(rp->idx);
  if (rp->stream) (void)hipStreamDestroy(rp->stream);
  delete rp;
}

// rows [first, first + k) of a host array into ring slots at..at + k - 1 (mod cap), `per` elements a row
template <class T>
int copy_rows(az_chess_replay* rp, T* ring, const T* src, int64_t first, int64_t k, int64_t at, size_t per) {
  const int64_t k0 = std::min(k, rp->cap - at);
  AZ_HIP(hipMemcpyAsync(ring + (size_t)at * per, src + (size_t)first * per, (size_t)k0 * per * sizeof(T),
                        hipMemcpyHostToDevice, rp->stream));
  if (k > k0)
    AZ_HIP(hipMemcpyAsync(ring, src + (size_t)(first + k0) * per, (size_t)(k - k0) * per * sizeof(T),
                          hipMemcpyHostToDevice, rp->stream));
  return AZ_OK;
}

}  // namespace

namespace az {
namespace replay {

int device_of(const az_chess_replay* rp) { return rp->device; }

int gather_on(az_chess_replay* rp, const int64_t* idx, int n, hipStream_t s, float* x, float* pi, float* z,
              const char* who) {
  if (rp->size == 0) return fail_abi(AZ_E_STATE, std::string(who) + ": the replay is empty");
  for (int i = 0; i < n; ++i)
    if (idx[i] < 0 || idx[i] >= rp->size)
      return fail_abi(AZ_E_INVALID, std::string(who) + ": index " + std::to_string(idx[i]) + " outside 0.." +
                                        std::to_string(rp->size - 1));
  if (n > rp->idx_cap) {
    if (rp->idx) AZ_HIP(hipFree(rp->idx));
    rp->idx = nullptr, rp->idx_cap = 0;
    AZ_HIP(hipMalloc(&rp->idx, (size_t)n * sizeof(int64_t)));
    rp->idx_cap = n;
  }
  AZ_HIP(hipMemcpyAsync(rp->idx, idx, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, s));
  azc::gather_kernel<<<n, azc::kGatherThreads, 0, s>>>(rp->hist, rp->valid, rp->policy_n, rp->actions, rp->probs,
                                                       rp->z, (long long)rp->head, (long long)rp->cap, rp->idx, x,
                                                       pi, z);
  AZ_HIP(hipGetLastError());
  return AZ_OK;
}

}  // namespace replay
}  // namespace az

// -------------------------------------------------------------------- ABI
extern "C" {

int az_chess_replay_create(int device, int64_t capacity, az_chess_replay** out) {
  if (!out) return fail_abi(AZ_E_INVALID, "az_chess_replay_create: null argument");
  if (capacity < 1 || capacity > (1ll << 31))
    return fail_abi(AZ_E_INVALID, "az_chess_replay_create: capacity must be 1..2^31");
  if (device < 0) return fail_abi(AZ_E_INVALID, "az_chess_replay_create: bad device ordinal");
  AZ_TRY(az::open_device(device, "az_chess_replay_create: device ordinal out of range"));
  az_chess_replay* rp = new az_chess_replay();
  rp->device = device;
  rp->cap = capacity;
  const size_t cap = (size_t)capacity;
  int rc = AZ_OK;
  if (hipStreamCreateWithFlags(&rp->stream, hipStreamNonBlocking) != hipSuccess)
    rc = fail_abi(AZ_E_HIP, "az_chess_replay_create: hipStreamCreate failed");
  if (rc == AZ_OK) rc = rp->mem.alloc(&rp->hist, cap * AZ_CHESS_HISTORY, true);
  if (rc == AZ_OK) rc = rp->mem.alloc(&rp->valid, cap * AZ_CHESS_HISTORY, true);
  if (rc == AZ_OK) rc = rp->mem.alloc(&rp->policy_n, cap, true);
  if (rc == AZ_OK) rc = rp->mem.alloc(&rp->actions, cap * AZ_CHESS_MAX_MOVES, true);
  if (rc == AZ_OK) rc = rp->mem.alloc(&rp->probs, cap * AZ_CHESS_MAX_MOVES, true);
  if (rc == AZ_OK) rc = rp->mem.alloc(&rp->z, cap, true);
  if (rc != AZ_OK) {
    free_replay(rp);
    return rc;
  }
  *out = rp;
  return AZ_OK;
}

int az_chess_replay_destroy(az_chess_replay* rp) {
  if (!rp) return AZ_OK;
  free_replay(rp);
  return AZ_OK;
}

int az_chess_replay_push(az_chess_replay* rp, const az_chess_pos* hist, const uint8_t* valid,
                         const int32_t* policy_n, const int16_t* policy_actions, const double* policy_probs,
                         const float* z, int64_t n) {
  if (!rp || n < 0 || (n > 0 && (!hist || !valid || !policy_n || !policy_actions || !policy_probs || !z)))
    return fail_abi(AZ_E_INVALID, "az_chess_replay_push: bad arguments");
  // every row is checked before anything is copied: a refused push changes nothing
  std::vector<int64_t> seen(AZ_CHESS_ACTIONS, -1);  // the last row that used the action
  for (int64_t i = 0; i < n; ++i) {
    const int pn = policy_n[i];
    if (pn < 0 || pn > AZ_CHESS_MAX_MOVES)
      return fail_abi(AZ_E_INVALID, "az_chess_replay_push: policy_n of sample " + std::to_string(i) + " is " +
                                        std::to_string(pn) + ", outside 0..256");
    for (int j = 0; j < pn; ++j) {
      const int a = policy_actions[(size_t)i * AZ_CHESS_MAX_MOVES + j];
      if (a < 0 || a >= AZ_CHESS_ACTIONS)
        return fail_abi(AZ_E_INVALID, "az_chess_replay_push: action " + std::to_string(a) + " of sample " +
                                          std::to_string(i) + " is outside 0..1879");
      if (seen[a] == i)
        return fail_abi(AZ_E_INVALID, "az_chess_replay_push: action " + std::to_string(a) +
                                          " is repeated in sample " + std::to_string(i));
      seen[a] = i;
    }
  }
  if (n == 0) return AZ_OK;
  AZ_HIP(hipSetDevice(rp->device));
  const int64_t k = std::min(n, rp->cap), first = n - k;  // a push past the capacity keeps its last `cap`
  const int64_t at = (rp->head + rp->size) % rp->cap;
  AZ_TRY(copy_rows(rp, rp->hist, hist, first, k, at, AZ_CHESS_HISTORY));
  AZ_TRY(copy_rows(rp, rp->valid, valid, first, k, at, AZ_CHESS_HISTORY));
  AZ_TRY(copy_rows(rp, rp->policy_n, policy_n, first, k, at, 1));
  AZ_TRY(copy_rows(rp, rp->actions, policy_actions, first, k, at, AZ_CHESS_MAX_MOVES));
  AZ_TRY(copy_rows(rp, rp->probs, policy_probs, first, k, at, AZ_CHESS_MAX_MOVES));
  AZ_TRY(copy_rows(rp, rp->z, z, first, k, at, 1));
  AZ_HIP(hipStreamSynchronize(rp->stream));
  const int64_t over = std::max<int64_t>(rp->size + k - rp->cap, 0);  // the oldest samples overwritten
  rp->head = (rp->head + over) % rp->cap;
  rp->size = rp->size + k - over;
  return AZ_OK;
}

int az_chess_replay_size(az_chess_replay* rp, int64_t* size, int64_t* capacity) {
  if (!rp) return fail_abi(AZ_E_INVALID, "az_chess_replay_size: null replay");
  if (size) *size = rp->size;
  if (capacity) *capacity = rp->cap;
  return AZ_OK;
}

int az_chess_replay_clear(az_chess_replay* rp) {
  if (!rp) return fail_abi(AZ_E_INVALID, "az_chess_replay_clear: null replay");
  rp->head = rp->size = 0;
  return AZ_OK;
}

int az_chess_replay_gather(az_chess_replay* rp, const int64_t* idx, int n, float* x, float* pi, float* z) {
  if (!rp || n < 0 || (n > 0 && !idx)) return fail_abi(AZ_E_INVALID, "az_chess_replay_gather: bad arguments");
  if (n == 0) return rp->size ? AZ_OK : fail_abi(AZ_E_STATE, "az_chess_replay_gather: the replay is empty");
  AZ_HIP(hipSetDevice(rp->device));
  const size_t per = (size_t)64 * AZ_CHESS_PLANES;
  struct Scratch {
    az::DeviceAllocs mem;
    ~Scratch() { mem.free_all(); }
  } tmp;
  float *dx = nullptr, *dpi = nullptr, *dz = nullptr;
  if (x) AZ_TRY(tmp.mem.alloc(&dx, (size_t)n * per, false));
  if (pi) AZ_TRY(tmp.mem.alloc(&dpi, (size_t)n * AZ_CHESS_ACTIONS, false));
  if (z) AZ_TRY(tmp.mem.alloc(&dz, (size_t)n, false));
  hipStream_t s = rp->stream;
  int rc = az::replay::gather_on(rp, idx, n, s, dx, dpi, dz, "az_chess_replay_gather");
  if (rc != AZ_OK) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  hipError_t e = hipSuccess;
  if (x) e = hipMemcpyAsync(x, dx, (size_t)n * per * sizeof(float), hipMemcpyDeviceToHost, s);
  if (pi && e == hipSuccess)
    e = hipMemcpyAsync(pi, dpi, (size_t)n * AZ_CHESS_ACTIONS * sizeof(float), hipMemcpyDeviceToHost, s);
  if (z && e == hipSuccess) e = hipMemcpyAsync(z, dz, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s);
  const hipError_t es = hipStreamSynchronize(s);  // before the scratch is freed, whatever failed
  AZ_HIP(e);
  AZ_HIP(es);
  return AZ_OK;
}

}  // extern "C"
