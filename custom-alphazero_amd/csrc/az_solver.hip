// az_solver.hip -- the exact Connect-N solver on the device: az_solver_*
// (include/az.h).  One serial alpha-beta search per lane (az_solver.h's step
// function), many positions at once: lanes take jobs from a queue (one atomic
// counter, most stones first, so deeper results are in the table when
// shallower searches want them), a launch runs a fixed number of steps per
// lane and writes every lane's state back, and the host relaunches until every
// job is solved or has used its node budget.  No kernel waits for another
// workgroup: there is no lock, no spin and no loop on a condition some other
// lane must satisfy.  Search stacks live in global memory as [frame][lane].
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "az_solver_handle.h"

using az::fail_abi;
namespace sv = az::solver;
using sv::kMaxLanes;
using sv::kWave;
using sv::Queue;

namespace {

constexpr int kDrained = -2;  // Lane::job of an idle lane that found the queue empty

}  // namespace

namespace az {
namespace solver {

__device__ __forceinline__ void retire(Lane& s, unsigned long long budget, int32_t* jscore, uint8_t* jstatus,
                                       int64_t* jnodes, Queue* q) {
  const bool over = (s.mode == kEnter || s.mode == kReturn) && s.nodes >= budget;
  if (s.mode == kDone || over) {
    jscore[s.job] = s.lo;
    jstatus[s.job] = over ? AZ_SOLVER_UNSOLVED : AZ_SOLVER_SOLVED;
    jnodes[s.job] = (int64_t)s.nodes;
    s.mode = kIdle;  // an unfinished stack is simply dropped: the table holds only true bounds
    atomicAdd(&q->done, 1);
  }
}

// grid * kWave == nlanes exactly; a lane's frames are at [f * nlanes + lane], f < H*W
// (a node descends only with fewer than H*W - 2 stones, so f <= H*W - 3).
__global__ void __launch_bounds__(kWave)
    solve_kernel(Geo g, Table tt, Lane* __restrict__ lanes, uint64_t* __restrict__ st_moves,
                 uint32_t* __restrict__ st_ab, unsigned nlanes, const Pos* __restrict__ jobs, int njobs, Queue* q,
                 unsigned long long budget, int steps, int32_t* __restrict__ jscore, uint8_t* __restrict__ jstatus,
                 int64_t* __restrict__ jnodes) {
  const unsigned lane = blockIdx.x * kWave + threadIdx.x;
  Lane s = lanes[lane];
  const Stack st{st_moves + lane, st_ab + lane, nlanes};
  for (int it = 0; it < steps; ++it) {
    retire(s, budget, jscore, jstatus, jnodes, q);
    if (s.mode == kIdle && s.job != kDrained) {
      const int j = atomicAdd(&q->next, 1);
      if (j < njobs)
        start(s, g, jobs[j].cur, jobs[j].mask, j);
      else
        s.job = kDrained;
    }
    if (__ballot(s.mode != kIdle) == 0) break;  // the whole wave is out of work
    if (s.mode != kIdle) step(s, g, tt, st);
  }
  retire(s, budget, jscore, jstatus, jnodes, q);
  lanes[lane] = s;
}

}  // namespace solver
}  // namespace az

namespace {

void free_solver(az_solver* s) {
  (void)hipSetDevice(s->device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  sv::book::drop(s);
  s->mem.free_all();
  for (void* p : {(void*)s->jobs, (void*)s->jscore, (void*)s->jstatus, (void*)s->jnodes})
    if (p) (void)hipFree(p);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;
}

int grow_jobs(az_solver* s, size_t n) {
  if (n <= s->job_cap) return AZ_OK;
  for (void* p : {(void*)s->jobs, (void*)s->jscore, (void*)s->jstatus, (void*)s->jnodes})
    if (p) AZ_HIP(hipFree(p));
  s->jobs = nullptr, s->jscore = nullptr, s->jstatus = nullptr, s->jnodes = nullptr, s->job_cap = 0;
  AZ_HIP(hipMalloc(&s->jobs, n * sizeof(sv::Pos)));
  AZ_HIP(hipMalloc(&s->jscore, n * sizeof(int32_t)));
  AZ_HIP(hipMalloc(&s->jstatus, n));
  AZ_HIP(hipMalloc(&s->jnodes, n * sizeof(int64_t)));
  s->job_cap = n;
  return AZ_OK;
}

}  // namespace

// the jobs' exact scores on the device: relaunch until all are retired
int az::solver::run_jobs(az_solver* s, const std::vector<sv::Pos>& jobs, int64_t budget, std::vector<int32_t>& score,
             std::vector<uint8_t>& status, std::vector<int64_t>& nodes) {
  const size_t n = jobs.size();
  score.assign(n, 0), status.assign(n, AZ_SOLVER_UNSOLVED), nodes.assign(n, 0);
  if (n == 0) return AZ_OK;
  const std::vector<int32_t> order = sv::most_stones_first(jobs);
  std::vector<sv::Pos> sorted(n);
  for (size_t i = 0; i < n; ++i) sorted[i] = jobs[order[i]];
  AZ_TRY(grow_jobs(s, n));
  hipStream_t st = s->stream;
  const unsigned waves = (unsigned)std::min<size_t>((n + kWave - 1) / kWave, kMaxLanes / kWave);
  const unsigned nlanes = waves * kWave;
  AZ_HIP(hipMemcpyAsync(s->jobs, sorted.data(), n * sizeof(sv::Pos), hipMemcpyHostToDevice, st));
  AZ_HIP(hipMemsetAsync(s->lanes, 0, (size_t)nlanes * sizeof(sv::Lane), st));  // every lane idle
  AZ_HIP(hipMemsetAsync(s->queue, 0, sizeof(Queue), st));
  Queue q{0, 0};
  // a job holds a lane for at most two steps a node (one down, one up) and one per null window
  const double max_launches = ((double)n / nlanes + 2.0) * ((2.0 * (double)budget + 128.0) / s->steps + 2.0);
  for (double launches = 0; (size_t)q.done < n; launches += 1.0) {
    if (launches > max_launches) return fail_abi(AZ_E_DEVICE, "az_solver_solve: the search made no progress");
    sv::solve_kernel<<<waves, kWave, 0, st>>>(s->geo, s->table, s->lanes, s->st_moves, s->st_ab, nlanes, s->jobs,
                                              (int)n, s->queue, (unsigned long long)budget, s->steps, s->jscore,
                                              s->jstatus, s->jnodes);
    AZ_HIP(hipGetLastError());
    AZ_HIP(hipMemcpyAsync(&q, s->queue, sizeof(q), hipMemcpyDeviceToHost, st));
    AZ_HIP(hipStreamSynchronize(st));
  }
  std::vector<int32_t> sc(n);
  std::vector<uint8_t> stt(n);
  std::vector<int64_t> nd(n);
  AZ_HIP(hipMemcpyAsync(sc.data(), s->jscore, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  AZ_HIP(hipMemcpyAsync(stt.data(), s->jstatus, n, hipMemcpyDeviceToHost, st));
  AZ_HIP(hipMemcpyAsync(nd.data(), s->jnodes, n * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  AZ_HIP(hipStreamSynchronize(st));
  for (size_t i = 0; i < n; ++i) score[order[i]] = sc[i], status[order[i]] = stt[i], nodes[order[i]] = nd[i];
  return AZ_OK;
}

namespace {

std::string limits_text() {
  return "the solver takes gravity boards with H, W >= 2, W <= 16, W * (H + 1) <= 56 and 2 <= n <= max(H, W)";
}

}  // namespace

// -------------------------------------------------------------------- ABI
extern "C" {

int az_solver_create(int device, int height, int width, int n, int tt_log2, az_solver** out) {
  if (!out) return fail_abi(AZ_E_INVALID, "az_solver_create: null argument");
  if (sv::geo_limit(height, width, n))
    return fail_abi(AZ_E_INVALID, "az_solver_create: " + std::to_string(width) + "x" + std::to_string(height) +
                                      " n=" + std::to_string(n) + " is outside the limit: " + limits_text());
  if (tt_log2 < 4 || tt_log2 > 30) return fail_abi(AZ_E_INVALID, "az_solver_create: tt_log2 must be 4..30");
  if (device < 0) return fail_abi(AZ_E_INVALID, "az_solver_create: bad device ordinal");
  AZ_TRY(az::open_device(device, "az_solver_create: device ordinal out of range"));
  az_solver* s = new az_solver();
  s->device = device;
  s->geo = sv::make_geo(height, width, n);
  s->tt_log2 = tt_log2;
  s->table.shift = 64 - tt_log2;
  const size_t frames = (size_t)s->geo.HW * kMaxLanes;
  int rc = AZ_OK;
  if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess)
    rc = fail_abi(AZ_E_HIP, "az_solver_create: hipStreamCreate failed");
  if (rc == AZ_OK) rc = s->mem.alloc(&s->table.e, (size_t)1 << tt_log2, true);
  if (rc == AZ_OK) rc = s->mem.alloc(&s->lanes, kMaxLanes, true);
  if (rc == AZ_OK) rc = s->mem.alloc(&s->st_moves, frames, false);
  if (rc == AZ_OK) rc = s->mem.alloc(&s->st_ab, frames, false);
  if (rc == AZ_OK) rc = s->mem.alloc(&s->queue, 1, true);
  if (rc != AZ_OK) {
    free_solver(s);
    return rc;
  }
  *out = s;
  return AZ_OK;
}

int az_solver_destroy(az_solver* s) {
  if (!s) return AZ_OK;
  free_solver(s);
  return AZ_OK;
}

int az_solver_clear(az_solver* s) {
  if (!s) return fail_abi(AZ_E_INVALID, "az_solver_clear: null solver");
  AZ_HIP(hipSetDevice(s->device));
  AZ_HIP(hipMemsetAsync(s->table.e, 0, sizeof(uint64_t) << s->tt_log2, s->stream));
  AZ_HIP(hipStreamSynchronize(s->stream));
  return AZ_OK;
}

int az_solver_configure(az_solver* s, int split_stones, int64_t max_jobs, int steps_per_launch) {
  if (!s) return fail_abi(AZ_E_INVALID, "az_solver_configure: null solver");
  if (split_stones < 0 || max_jobs < 0 || steps_per_launch < 0 || max_jobs > (1ll << 30) ||
      steps_per_launch > (1 << 20))
    return fail_abi(AZ_E_INVALID,
                    "az_solver_configure: split_stones >= 0, 0 <= max_jobs <= 2^30, 0 <= steps_per_launch <= 2^20");
  if (split_stones) s->split_stones = split_stones;
  if (max_jobs) s->max_jobs = max_jobs;
  if (steps_per_launch) s->steps = steps_per_launch;
  return AZ_OK;
}

int az_solver_solve(az_solver* s, const int8_t* boards, int64_t count, int64_t node_budget, int32_t* scores,
                    uint8_t* status, int64_t* nodes) {
  if (!s || count < 0 || (count > 0 && (!boards || !scores || !status || !nodes)))
    return fail_abi(AZ_E_INVALID, "az_solver_solve: bad arguments");
  if (node_budget <= 0) return fail_abi(AZ_E_INVALID, "az_solver_solve: node_budget must be > 0");
  const sv::Geo& g = s->geo;
  std::vector<sv::Pos> roots((size_t)count);
  for (int64_t i = 0; i < count; ++i) {
    const std::string why = sv::parse_board(g, boards + (size_t)i * g.HW, &roots[i]);
    if (!why.empty()) return fail_abi(AZ_E_INVALID, "az_solver_solve: board " + std::to_string(i) + " " + why);
  }
  AZ_HIP(hipSetDevice(s->device));
  // a finished book answers the roots it holds; the others go on as without one
  std::vector<uint8_t> hit;
  std::vector<int32_t> book_score;
  if (sv::book::lookup_depth(s) >= 0) AZ_TRY(sv::book::lookup(s, roots, hit, book_score));
  sv::Plan plan;
  std::vector<int64_t> root_of((size_t)count, -1);  // board -> its root in the plan
  for (int64_t i = 0; i < count; ++i) {
    if (!hit.empty() && hit[i]) continue;
    root_of[i] = (int64_t)plan.roots.size();
    sv::plan_add(plan, g, roots[i], s->split_stones, s->max_jobs);
    if (plan.jobs.size() > ((size_t)1 << 30))
      return fail_abi(AZ_E_INVALID, "az_solver_solve: more than 2^30 jobs in one call");
  }
  std::vector<int32_t> jscore;
  std::vector<uint8_t> jstatus;
  std::vector<int64_t> jnodes;
  AZ_TRY(sv::run_jobs(s, plan.jobs, node_budget, jscore, jstatus, jnodes));
  for (int64_t i = 0; i < count; ++i) {
    if (root_of[i] < 0) {
      scores[i] = book_score[i], status[i] = AZ_SOLVER_SOLVED, nodes[i] = 0;
      continue;
    }
    const bool ok = sv::plan_result(plan, g, (size_t)root_of[i], jscore.data(), jstatus.data(), jnodes.data(),
                                    scores + i, nodes + i);
    status[i] = ok ? AZ_SOLVER_SOLVED : AZ_SOLVER_UNSOLVED;
  }
  return AZ_OK;
}

}  // extern "C"
