// az_book.hip -- the exact solver's opening book on the device:
// az_solver_book_* (include/az.h).  The levels are enumerated breadth first
// (one thread per parent and column writes the child's canonical key, rocPRIM
// sorts and removes duplicates), the deepest level is scored by the search in
// chunks through the solver's own job path, the levels above it by one
// retrograde launch each, and a finished book answers az_solver_solve's shallow
// roots from one lookup launch.  Every kernel here is one pass over its items:
// no kernel waits for another workgroup, every loop has a bound known at
// launch and every index is checked against its array's length.
#include <cstring>  // before rocPRIM: its headers use memcpy without naming it

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>

#include <string>
#include <vector>

#include "az_book.h"
#include "az_solver_handle.h"

using az::fail_abi;
namespace sv = az::solver;
namespace bk = az::solver::book;

namespace az {
namespace solver {
namespace book {

struct Level {
  uint64_t* keys;
  int8_t* scores;
  int64_t n;
};

struct DeviceBook {
  int depth = -1;
  int state = kNone;
  int64_t next = 0;                    // level `depth`: the first entry this pass has not tried
  std::vector<Level> lv;               // [depth + 1], device pointers
  Level* d_lv = nullptr;               // the same on the device, for the lookup
  unsigned long long* err = nullptr;   // positions the retrograde pass could not score
  size_t q_cap = 0;                    // lookup buffers, grown on demand
  Pos* q_pos = nullptr;
  uint8_t* q_hit = nullptr;
  int8_t* q_score = nullptr;
};

constexpr int kBlock = 256;

// item i = parent i / W, column i % W -> the live child's canonical key, else kNoKey
__global__ void __launch_bounds__(kBlock)
    expand_kernel(Geo g, const uint64_t* __restrict__ parents, int64_t n, uint64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n * g.W) return;
  uint64_t cur, mask, key;
  decode_key(g, parents[i / g.W], &cur, &mask);
  child_key(g, cur, mask, (int)(i % g.W), &key);
  out[i] = key;
}

// level t from the scored level t + 1
__global__ void __launch_bounds__(kBlock)
    retro_kernel(Geo g, const uint64_t* __restrict__ keys, int8_t* __restrict__ scores, int64_t n, int t,
                 const uint64_t* __restrict__ next_keys, const int8_t* __restrict__ next_scores, int64_t next_n,
                 unsigned long long* err) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  bool bad;
  scores[i] = retro_value(g, keys[i], t, next_keys, next_scores, next_n, &bad);
  if (bad) atomicAdd(err, 1ull);
}

__global__ void __launch_bounds__(kBlock)
    lookup_kernel(Geo g, const Level* __restrict__ lv, int depth, const Pos* __restrict__ q, int64_t nq,
                  uint8_t* __restrict__ hit, int8_t* __restrict__ score) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= nq) return;
  const int t = popc(q[i].mask);
  uint8_t h = 0;
  int8_t s = kNoScore;
  if (t <= depth) {
    const Level l = lv[t];
    const int64_t at = find_key(l.keys, l.n, canonical_key(g, q[i].cur + q[i].mask));
    if (at >= 0 && l.scores[at] != kNoScore) h = 1, s = l.scores[at];
  }
  hit[i] = h, score[i] = s;
}

// entries first, first + stride, ... of a level as boards and scores
__global__ void __launch_bounds__(kBlock)
    level_kernel(Geo g, const uint64_t* __restrict__ keys, const int8_t* __restrict__ scores, int64_t n,
                 int64_t first, int64_t count, int64_t stride, int8_t* __restrict__ boards,
                 int8_t* __restrict__ out_scores) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= count) return;
  const int64_t at = first + i * stride;
  if (at < 0 || at >= n) return;
  key_to_board(g, keys[at], boards + i * g.HW);
  out_scores[i] = scores[at];
}

// The chunk's entries idx[0..m) of level t as jobs.  A position the side to
// move wins at once is scored here (as plan_add resolves it) and marked by
// mask = kNoKey, which no job has.
__global__ void __launch_bounds__(kBlock)
    pick_kernel(Geo g, const uint64_t* __restrict__ keys, int8_t* __restrict__ scores, int64_t n, int t,
                const int64_t* __restrict__ idx, int64_t m, Pos* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= m) return;
  const int64_t at = idx[i];
  Pos p{0, kNoKey};
  if (at >= 0 && at < n) {
    uint64_t cur, mask;
    decode_key(g, keys[at], &cur, &mask);
    if (wins_now(cur, mask, g))
      scores[at] = (int8_t)win_score(g, t + 1);
    else
      p = Pos{cur, mask};
  }
  out[i] = p;
}

__global__ void __launch_bounds__(kBlock)
    store_kernel(int8_t* __restrict__ scores, int64_t n, const int64_t* __restrict__ idx,
                 const int8_t* __restrict__ vals, int64_t m) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= m) return;
  const int64_t at = idx[i];
  if (at >= 0 && at < n && vals[i] != kNoScore) scores[at] = vals[i];
}

}  // namespace book
}  // namespace solver
}  // namespace az

namespace {

unsigned blocks_for(int64_t items) { return (unsigned)((items + bk::kBlock - 1) / bk::kBlock); }

// a device buffer freed when it leaves scope
struct Scratch {
  void* p = nullptr;
  ~Scratch() {
    if (p) (void)hipFree(p);
  }
  template <typename T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

int alloc_level(bk::Level* l, int64_t n) {
  l->n = n;
  AZ_HIP(hipMalloc(&l->keys, std::max<int64_t>(n, 1) * sizeof(uint64_t)));
  AZ_HIP(hipMalloc(&l->scores, std::max<int64_t>(n, 1)));
  return AZ_OK;
}

// the level pointers where the lookup reads them
int publish_levels(az_solver* s) {
  bk::DeviceBook* b = s->book;
  if (!b->d_lv) AZ_HIP(hipMalloc(&b->d_lv, sizeof(bk::Level) * (size_t)s->geo.HW));
  AZ_HIP(hipMemcpyAsync(b->d_lv, b->lv.data(), sizeof(bk::Level) * b->lv.size(), hipMemcpyHostToDevice, s->stream));
  AZ_HIP(hipStreamSynchronize(s->stream));
  return AZ_OK;
}

int new_book(az_solver* s, int depth) {
  bk::drop(s);
  s->book = new bk::DeviceBook();
  s->book->depth = depth;
  s->book->lv.assign((size_t)depth + 1, bk::Level{nullptr, nullptr, 0});
  AZ_HIP(hipMalloc(&s->book->err, sizeof(unsigned long long)));
  return AZ_OK;
}

// level t + 1 of the book from level t
int expand_level(az_solver* s, int t) {
  bk::DeviceBook* b = s->book;
  const sv::Geo& g = s->geo;
  hipStream_t st = s->stream;
  const bk::Level& from = b->lv[t];
  const int64_t m = from.n * g.W;
  if (m >= (1ll << 31))
    return fail_abi(AZ_E_INVALID, "az_solver_book_begin: level " + std::to_string(t + 1) + " has more than 2^31 candidates");
  if (m == 0) return alloc_level(&b->lv[t + 1], 0);
  Scratch a, c, tmp, cnt;
  AZ_HIP(hipMalloc(&a.p, (size_t)m * sizeof(uint64_t)));
  AZ_HIP(hipMalloc(&c.p, (size_t)m * sizeof(uint64_t)));
  AZ_HIP(hipMalloc(&cnt.p, sizeof(unsigned long long)));
  bk::expand_kernel<<<blocks_for(m), bk::kBlock, 0, st>>>(g, from.keys, from.n, a.as<uint64_t>());
  AZ_HIP(hipGetLastError());
  const unsigned bits = (unsigned)(g.W * g.H1);  // kNoKey's low bits are above every key's
  size_t sort_bytes = 0, unique_bytes = 0;
  AZ_HIP(rocprim::radix_sort_keys(nullptr, sort_bytes, a.as<uint64_t>(), c.as<uint64_t>(), (size_t)m, 0u, bits, st));
  AZ_HIP(rocprim::unique(nullptr, unique_bytes, c.as<uint64_t>(), a.as<uint64_t>(), cnt.as<unsigned long long>(),
                         (size_t)m, rocprim::equal_to<uint64_t>(), st));
  AZ_HIP(hipMalloc(&tmp.p, std::max<size_t>(std::max(sort_bytes, unique_bytes), 16)));
  AZ_HIP(rocprim::radix_sort_keys(tmp.p, sort_bytes, a.as<uint64_t>(), c.as<uint64_t>(), (size_t)m, 0u, bits, st));
  AZ_HIP(rocprim::unique(tmp.p, unique_bytes, c.as<uint64_t>(), a.as<uint64_t>(), cnt.as<unsigned long long>(),
                         (size_t)m, rocprim::equal_to<uint64_t>(), st));
  unsigned long long count = 0;
  AZ_HIP(hipMemcpyAsync(&count, cnt.p, sizeof(count), hipMemcpyDeviceToHost, st));
  AZ_HIP(hipStreamSynchronize(st));
  if (count > (unsigned long long)m) return fail_abi(AZ_E_DEVICE, "az_solver_book_begin: the unique count is out of range");
  if (count > 0) {  // "none" sorts last and is one entry after unique
    uint64_t last = 0;
    AZ_HIP(hipMemcpyAsync(&last, a.as<uint64_t>() + (count - 1), sizeof(last), hipMemcpyDeviceToHost, st));
    AZ_HIP(hipStreamSynchronize(st));
    if (last == bk::kNoKey) --count;
  }
  bk::Level& to = b->lv[t + 1];
  AZ_TRY(alloc_level(&to, (int64_t)count));
  AZ_HIP(hipMemcpyAsync(to.keys, a.p, (size_t)count * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
  AZ_HIP(hipMemsetAsync(to.scores, 0x80, std::max<size_t>((size_t)count, 1), st));
  AZ_HIP(hipStreamSynchronize(st));
  return AZ_OK;
}

int count_unscored(az_solver* s, std::vector<int8_t>* host, int64_t* remaining) {
  const bk::Level& l = s->book->lv[s->book->depth];
  host->resize((size_t)l.n);
  if (l.n) AZ_HIP(hipMemcpyAsync(host->data(), l.scores, (size_t)l.n, hipMemcpyDeviceToHost, s->stream));
  AZ_HIP(hipStreamSynchronize(s->stream));
  *remaining = 0;
  for (int8_t v : *host) *remaining += v == bk::kNoScore;
  return AZ_OK;
}

int to_host(az_solver* s, bk::HostBook* h) {
  const bk::DeviceBook* b = s->book;
  h->H = s->geo.H, h->W = s->geo.W, h->n = s->geo.n, h->depth = b->depth, h->state = b->state;
  h->next = b->state == bk::kFinished ? 0 : b->next;
  h->keys.resize(b->lv.size()), h->scores.resize(b->lv.size());
  for (size_t t = 0; t < b->lv.size(); ++t) {
    const bk::Level& l = b->lv[t];
    h->keys[t].resize((size_t)l.n), h->scores[t].resize((size_t)l.n);
    if (!l.n) continue;
    AZ_HIP(hipMemcpyAsync(h->keys[t].data(), l.keys, (size_t)l.n * sizeof(uint64_t), hipMemcpyDeviceToHost, s->stream));
    AZ_HIP(hipMemcpyAsync(h->scores[t].data(), l.scores, (size_t)l.n, hipMemcpyDeviceToHost, s->stream));
    AZ_HIP(hipStreamSynchronize(s->stream));
  }
  return AZ_OK;
}

}  // namespace

void bk::drop(az_solver* s) {
  DeviceBook* b = s->book;
  if (!b) return;
  for (Level& l : b->lv) {
    if (l.keys) (void)hipFree(l.keys);
    if (l.scores) (void)hipFree(l.scores);
  }
  for (void* p : {(void*)b->d_lv, (void*)b->err, (void*)b->q_pos, (void*)b->q_hit, (void*)b->q_score})
    if (p) (void)hipFree(p);
  delete b;
  s->book = nullptr;
}

int bk::lookup_depth(const az_solver* s) { return s->book && s->book->state == kFinished ? s->book->depth : -1; }

int bk::lookup(az_solver* s, const std::vector<Pos>& roots, std::vector<uint8_t>& hit, std::vector<int32_t>& score) {
  DeviceBook* b = s->book;
  const size_t n = roots.size();
  hit.assign(n, 0), score.assign(n, 0);
  if (n == 0 || !b || b->state != kFinished) return AZ_OK;
  if (n > b->q_cap) {
    for (void* p : {(void*)b->q_pos, (void*)b->q_hit, (void*)b->q_score})
      if (p) AZ_HIP(hipFree(p));
    b->q_pos = nullptr, b->q_hit = nullptr, b->q_score = nullptr, b->q_cap = 0;
    AZ_HIP(hipMalloc(&b->q_pos, n * sizeof(Pos)));
    AZ_HIP(hipMalloc(&b->q_hit, n));
    AZ_HIP(hipMalloc(&b->q_score, n));
    b->q_cap = n;
  }
  hipStream_t st = s->stream;
  std::vector<int8_t> sc(n);
  AZ_HIP(hipMemcpyAsync(b->q_pos, roots.data(), n * sizeof(Pos), hipMemcpyHostToDevice, st));
  lookup_kernel<<<blocks_for((int64_t)n), kBlock, 0, st>>>(s->geo, b->d_lv, b->depth, b->q_pos, (int64_t)n, b->q_hit,
                                                           b->q_score);
  AZ_HIP(hipGetLastError());
  AZ_HIP(hipMemcpyAsync(hit.data(), b->q_hit, n, hipMemcpyDeviceToHost, st));
  AZ_HIP(hipMemcpyAsync(sc.data(), b->q_score, n, hipMemcpyDeviceToHost, st));
  AZ_HIP(hipStreamSynchronize(st));
  for (size_t i = 0; i < n; ++i) score[i] = sc[i];
  return AZ_OK;
}

// -------------------------------------------------------------------- ABI
extern "C" {

int az_solver_book_begin(az_solver* s, int depth, int64_t* level_counts) {
  if (!s || !level_counts) return fail_abi(AZ_E_INVALID, "az_solver_book_begin: null argument");
  if (depth < 0 || depth > s->geo.HW - 1)
    return fail_abi(AZ_E_INVALID, "az_solver_book_begin: depth must be 0.." + std::to_string(s->geo.HW - 1));
  AZ_HIP(hipSetDevice(s->device));
  AZ_TRY(new_book(s, depth));
  bk::DeviceBook* b = s->book;
  int rc = alloc_level(&b->lv[0], 1);  // the empty board: key 0
  if (rc == AZ_OK && (hipMemsetAsync(b->lv[0].keys, 0, sizeof(uint64_t), s->stream) != hipSuccess ||
                      hipMemsetAsync(b->lv[0].scores, 0x80, 1, s->stream) != hipSuccess))
    rc = fail_abi(AZ_E_HIP, "az_solver_book_begin: hipMemset failed");
  for (int t = 0; t < depth && rc == AZ_OK; ++t) rc = expand_level(s, t);
  if (rc == AZ_OK) rc = publish_levels(s);
  if (rc != AZ_OK) {
    bk::drop(s);
    return rc;
  }
  b->state = bk::kBuilding;
  for (int t = 0; t <= depth; ++t) level_counts[t] = b->lv[t].n;
  return AZ_OK;
}

int az_solver_book_solve(az_solver* s, int64_t max_positions, int64_t node_budget, int64_t* remaining,
                         int64_t* unsolved) {
  if (!s || !remaining || !unsolved) return fail_abi(AZ_E_INVALID, "az_solver_book_solve: null argument");
  if (max_positions <= 0 || max_positions > (1ll << 30) || node_budget <= 0)
    return fail_abi(AZ_E_INVALID, "az_solver_book_solve: 0 < max_positions <= 2^30 and node_budget > 0");
  bk::DeviceBook* b = s->book;
  if (!b || b->state != bk::kBuilding)
    return fail_abi(AZ_E_STATE, "az_solver_book_solve: no book is being built (book_begin or book_load first)");
  AZ_HIP(hipSetDevice(s->device));
  hipStream_t st = s->stream;
  const bk::Level& l = b->lv[b->depth];
  std::vector<int8_t> have;
  AZ_TRY(count_unscored(s, &have, remaining));
  *unsolved = 0;
  if (*remaining == 0) return AZ_OK;
  // the chunk: entries without a score from `next` on; a pass ends at the level's end
  if (b->next >= l.n) b->next = 0;
  std::vector<int64_t> idx;
  int64_t at = b->next;
  for (; at < l.n && (int64_t)idx.size() < max_positions; ++at)
    if (have[(size_t)at] == bk::kNoScore) idx.push_back(at);
  b->next = at;
  const int64_t m = (int64_t)idx.size();
  if (m == 0) return AZ_OK;  // the rest of this pass was scored already: the next call starts a new one
  Scratch d_idx, d_pos, d_val;
  AZ_HIP(hipMalloc(&d_idx.p, (size_t)m * sizeof(int64_t)));
  AZ_HIP(hipMalloc(&d_pos.p, (size_t)m * sizeof(sv::Pos)));
  AZ_HIP(hipMalloc(&d_val.p, (size_t)m));
  std::vector<sv::Pos> pos((size_t)m);
  AZ_HIP(hipMemcpyAsync(d_idx.p, idx.data(), (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice, st));
  bk::pick_kernel<<<blocks_for(m), bk::kBlock, 0, st>>>(s->geo, l.keys, l.scores, l.n, b->depth, d_idx.as<int64_t>(), m,
                                                        d_pos.as<sv::Pos>());
  AZ_HIP(hipGetLastError());
  AZ_HIP(hipMemcpyAsync(pos.data(), d_pos.p, (size_t)m * sizeof(sv::Pos), hipMemcpyDeviceToHost, st));
  AZ_HIP(hipStreamSynchronize(st));
  std::vector<sv::Pos> jobs;
  std::vector<int64_t> job_of((size_t)m, -1);
  for (int64_t i = 0; i < m; ++i)
    if (pos[(size_t)i].mask != bk::kNoKey) job_of[(size_t)i] = (int64_t)jobs.size(), jobs.push_back(pos[(size_t)i]);
  std::vector<int32_t> jscore;
  std::vector<uint8_t> jstatus;
  std::vector<int64_t> jnodes;
  AZ_TRY(sv::run_jobs(s, jobs, node_budget, jscore, jstatus, jnodes));
  std::vector<int8_t> vals((size_t)m, bk::kNoScore);  // kNoScore: nothing to store
  int64_t scored = 0;
  for (int64_t i = 0; i < m; ++i) {
    const int64_t j = job_of[(size_t)i];
    if (j < 0) {
      ++scored;  // won at once: pick_kernel stored it
    } else if (jstatus[(size_t)j] == AZ_SOLVER_SOLVED) {
      vals[(size_t)i] = (int8_t)jscore[(size_t)j];
      ++scored;
    } else {
      ++*unsolved;
    }
  }
  AZ_HIP(hipMemcpyAsync(d_val.p, vals.data(), (size_t)m, hipMemcpyHostToDevice, st));
  bk::store_kernel<<<blocks_for(m), bk::kBlock, 0, st>>>(l.scores, l.n, d_idx.as<int64_t>(), d_val.as<int8_t>(), m);
  AZ_HIP(hipGetLastError());
  AZ_HIP(hipStreamSynchronize(st));
  *remaining -= scored;
  return AZ_OK;
}

int az_solver_book_finish(az_solver* s) {
  if (!s) return fail_abi(AZ_E_INVALID, "az_solver_book_finish: null solver");
  bk::DeviceBook* b = s->book;
  if (!b || b->state == bk::kNone) return fail_abi(AZ_E_STATE, "az_solver_book_finish: the solver has no book");
  if (b->state == bk::kFinished) return AZ_OK;
  AZ_HIP(hipSetDevice(s->device));
  hipStream_t st = s->stream;
  std::vector<int8_t> have;
  int64_t remaining = 0;
  AZ_TRY(count_unscored(s, &have, &remaining));
  if (remaining > 0)
    return fail_abi(AZ_E_STATE, "az_solver_book_finish: " + std::to_string(remaining) + " positions of level " +
                                    std::to_string(b->depth) + " have no score yet (book_solve)");
  AZ_HIP(hipMemsetAsync(b->err, 0, sizeof(unsigned long long), st));
  for (int t = b->depth - 1; t >= 0; --t) {
    const bk::Level &l = b->lv[t], &nx = b->lv[t + 1];
    if (l.n == 0) continue;
    bk::retro_kernel<<<blocks_for(l.n), bk::kBlock, 0, st>>>(s->geo, l.keys, l.scores, l.n, t, nx.keys, nx.scores, nx.n,
                                                             b->err);
    AZ_HIP(hipGetLastError());
  }
  unsigned long long bad = 0;
  AZ_HIP(hipMemcpyAsync(&bad, b->err, sizeof(bad), hipMemcpyDeviceToHost, st));
  AZ_HIP(hipStreamSynchronize(st));
  if (bad)
    return fail_abi(AZ_E_DEVICE, "az_solver_book_finish: book inconsistent: " + std::to_string(bad) +
                                     " positions have a child that is missing from the next level or has no score");
  b->state = bk::kFinished;
  b->next = 0;
  return AZ_OK;
}

int az_solver_book_save(az_solver* s, const char* path) {
  if (!s || !path) return fail_abi(AZ_E_INVALID, "az_solver_book_save: null argument");
  if (!s->book || s->book->state == bk::kNone) return fail_abi(AZ_E_STATE, "az_solver_book_save: the solver has no book");
  AZ_HIP(hipSetDevice(s->device));
  bk::HostBook h;
  AZ_TRY(to_host(s, &h));
  const std::string why = bk::write_book(path, h);
  if (!why.empty()) return fail_abi(AZ_E_INVALID, "az_solver_book_save: " + why);
  return AZ_OK;
}

int az_solver_book_load(az_solver* s, const char* path) {
  if (!s || !path) return fail_abi(AZ_E_INVALID, "az_solver_book_load: null argument");
  bk::HostBook h;
  const std::string why = bk::read_book(path, s->geo, &h);
  if (!why.empty()) return fail_abi(AZ_E_INVALID, "az_solver_book_load: " + std::string(path) + ": " + why);
  AZ_HIP(hipSetDevice(s->device));
  AZ_TRY(new_book(s, h.depth));
  bk::DeviceBook* b = s->book;
  int rc = AZ_OK;
  for (int t = 0; t <= h.depth && rc == AZ_OK; ++t) {
    bk::Level& l = b->lv[t];
    rc = alloc_level(&l, (int64_t)h.keys[t].size());
    if (rc != AZ_OK || l.n == 0) continue;
    if (hipMemcpyAsync(l.keys, h.keys[t].data(), (size_t)l.n * sizeof(uint64_t), hipMemcpyHostToDevice, s->stream) !=
            hipSuccess ||
        hipMemcpyAsync(l.scores, h.scores[t].data(), (size_t)l.n, hipMemcpyHostToDevice, s->stream) != hipSuccess ||
        hipStreamSynchronize(s->stream) != hipSuccess)
      rc = fail_abi(AZ_E_HIP, "az_solver_book_load: the copy to the device failed");
  }
  if (rc == AZ_OK) rc = publish_levels(s);
  if (rc != AZ_OK) {
    bk::drop(s);
    return rc;
  }
  b->state = h.state;
  b->next = h.state == bk::kFinished ? 0 : h.next;
  return AZ_OK;
}

int az_solver_book_info(az_solver* s, int32_t* depth, int32_t* state, int64_t* level_counts) {
  if (!s || !depth || !state || !level_counts) return fail_abi(AZ_E_INVALID, "az_solver_book_info: null argument");
  for (int t = 0; t < s->geo.HW; ++t) level_counts[t] = 0;
  *depth = s->book ? s->book->depth : -1;
  *state = s->book ? s->book->state : bk::kNone;
  if (s->book)
    for (size_t t = 0; t < s->book->lv.size(); ++t) level_counts[t] = s->book->lv[t].n;
  return AZ_OK;
}

int az_solver_book_level(az_solver* s, int stones, int64_t first, int64_t count, int64_t stride, int8_t* boards,
                         int8_t* scores) {
  if (!s || count < 0 || (count > 0 && (!boards || !scores)))
    return fail_abi(AZ_E_INVALID, "az_solver_book_level: bad arguments");
  const bk::DeviceBook* b = s->book;
  if (!b || b->state == bk::kNone) return fail_abi(AZ_E_STATE, "az_solver_book_level: the solver has no book");
  if (stones < 0 || stones > b->depth)
    return fail_abi(AZ_E_INVALID, "az_solver_book_level: the book holds levels 0.." + std::to_string(b->depth));
  const bk::Level& l = b->lv[stones];
  if (count == 0) return AZ_OK;
  if (first < 0 || stride < 1 || first >= l.n || (count - 1) > (l.n - 1 - first) / stride)
    return fail_abi(AZ_E_INVALID, "az_solver_book_level: first + (count - 1) * stride passes the level's " +
                                      std::to_string(l.n) + " entries");
  AZ_HIP(hipSetDevice(s->device));
  hipStream_t st = s->stream;
  const size_t cells = (size_t)count * (size_t)s->geo.HW;
  Scratch d_boards, d_scores;
  AZ_HIP(hipMalloc(&d_boards.p, cells));
  AZ_HIP(hipMalloc(&d_scores.p, (size_t)count));
  bk::level_kernel<<<blocks_for(count), bk::kBlock, 0, st>>>(s->geo, l.keys, l.scores, l.n, first, count, stride,
                                                             d_boards.as<int8_t>(), d_scores.as<int8_t>());
  AZ_HIP(hipGetLastError());
  AZ_HIP(hipMemcpyAsync(boards, d_boards.p, cells, hipMemcpyDeviceToHost, st));
  AZ_HIP(hipMemcpyAsync(scores, d_scores.p, (size_t)count, hipMemcpyDeviceToHost, st));
  AZ_HIP(hipStreamSynchronize(st));
  return AZ_OK;
}

}  // extern "C"
