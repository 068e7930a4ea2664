// az_solver_handle.h -- struct az_solver, shared by the solver's two
// translation units: az_solver.hip (the search, az_solver_solve) and
// az_book.hip (the opening book, az_solver_book_*), and what each needs from
// the other.
#pragma once
#include <vector>

#include "../../include/az.h"
#include "az_host.h"
#include "az_solver.h"

namespace az {
namespace solver {

constexpr int kWave = 64;
// 1024 waves: one a SIMD on the MI355X's 256 CUs.  A wave is its own workgroup,
// so a handful of jobs still spreads over the chip.
constexpr int kMaxLanes = 1024 * kWave;
// Steps a lane runs per launch.  With every lane busy on 7x6 a lane ran 78.7 k
// steps/s on the MI355X, so a launch takes 26 ms: short enough to share the
// device.  512 and 8192 steps gave the same throughput within 2 %
// (DESIGN.md "Exact solver").
constexpr int kDefaultSteps = 2048;
// Positions with fewer stones are split on the host.  8 serves the boards the
// solver finishes from the empty board (up to about 6x5); a 7x6 position that
// shallow is out of reach either way (DESIGN.md has the sweep).
constexpr int kDefaultSplit = 8;
constexpr int64_t kDefaultMaxJobs = 1 << 20;

struct Queue {
  int32_t next;  // the next job to hand out
  int32_t done;  // jobs retired
};

namespace book {
struct DeviceBook;  // az_book.hip
}

}  // namespace solver
}  // namespace az

struct az_solver {
  int device = 0;
  hipStream_t stream = nullptr;
  az::solver::Geo geo{};
  az::solver::Table table{};
  int tt_log2 = 0;
  int split_stones = az::solver::kDefaultSplit;
  int64_t max_jobs = az::solver::kDefaultMaxJobs;
  int steps = az::solver::kDefaultSteps;
  az::solver::Lane* lanes = nullptr;  // [kMaxLanes]
  uint64_t* st_moves = nullptr;       // [H*W][kMaxLanes]
  uint32_t* st_ab = nullptr;          // [H*W][kMaxLanes]
  az::solver::Queue* queue = nullptr;
  az::DeviceAllocs mem;
  // per call, grown on demand
  size_t job_cap = 0;
  az::solver::Pos* jobs = nullptr;
  int32_t* jscore = nullptr;
  uint8_t* jstatus = nullptr;
  int64_t* jnodes = nullptr;
  az::solver::book::DeviceBook* book = nullptr;  // owned; null until book_begin or book_load
};

namespace az {
namespace solver {

// az_solver.hip: the jobs' exact scores on the device, relaunching until all are retired
int run_jobs(az_solver* s, const std::vector<Pos>& jobs, int64_t budget, std::vector<int32_t>& score,
             std::vector<uint8_t>& status, std::vector<int64_t>& nodes);

namespace book {

// az_book.hip.  drop: frees s->book.  lookup_depth: the finished book's depth,
// -1 without one.  lookup: one launch for all roots; hit[i] != 0 where the book
// holds roots[i] (then score[i] is its score).
void drop(az_solver* s);
int lookup_depth(const az_solver* s);
int lookup(az_solver* s, const std::vector<Pos>& roots, std::vector<uint8_t>& hit, std::vector<int32_t>& score);

}  // namespace book
}  // namespace solver
}  // namespace az
