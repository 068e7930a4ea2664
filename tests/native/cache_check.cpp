// Host build of the transposition cache's pure parts (csrc/az_cache.h: the
// state word, cache_bucket, cache_candidates, cache_victim, cache_gen_size),
// test infrastructure for tests/test_cache_cpu.py.  Each command reads FILE,
// little-endian records of the words listed, and prints one line per record
// with what the header returns; the test computes what it expects itself.
//   cache_check word FILE      u32 fp, gen, status, now -> "<cache_word> <cache_age(word, now)>"
//   cache_check fp FILE        u64 hash                 -> "<cache_fp>"
//   cache_check bucket FILE    u64 hash, mask           -> "<cache_bucket>"
//   cache_check scan FILE      u32 w[16], fp            -> "<cache_candidates>"
//   cache_check victim FILE    u32 w[16], gen, tried, gen_size -> "<slot> <word> <empty>"
//   cache_check gen_size FILE  u64 cap, reader window   -> "<cache_gen_size>"
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../custom-alphazero_amd/csrc/az_cache.h"

namespace {

template <typename T>
bool read_records(const char* path, size_t words, std::vector<T>* out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  T v;
  while (fread(&v, sizeof(T), 1, f) == 1) out->push_back(v);
  fclose(f);
  return out->size() % words == 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const std::string cmd = argv[1];
  std::vector<uint32_t> u;
  std::vector<uint64_t> q;
  constexpr int B = az::kCacheBucket;
  if (cmd == "word" && read_records(argv[2], 4, &u)) {
    for (size_t i = 0; i < u.size(); i += 4) {
      const uint32_t w = az::cache_word(u[i], u[i + 1], u[i + 2]);
      printf("%u %u\n", w, az::cache_age(w, u[i + 3]));
    }
  } else if (cmd == "fp" && read_records(argv[2], 1, &q)) {
    for (uint64_t h : q) printf("%u\n", az::cache_fp(h));
  } else if (cmd == "bucket" && read_records(argv[2], 2, &q)) {
    for (size_t i = 0; i < q.size(); i += 2) printf("%u\n", az::cache_bucket((uint32_t)q[i + 1], q[i]));
  } else if (cmd == "scan" && read_records(argv[2], B + 1, &u)) {
    for (size_t i = 0; i < u.size(); i += B + 1) {
      uint32_t w[B];
      memcpy(w, &u[i], sizeof(w));
      printf("%u\n", az::cache_candidates(w, u[i + B]));
    }
  } else if (cmd == "victim" && read_records(argv[2], B + 3, &u)) {
    for (size_t i = 0; i < u.size(); i += B + 3) {
      uint32_t w[B];
      memcpy(w, &u[i], sizeof(w));
      const az::CacheVictim v = az::cache_victim(w, u[i + B], u[i + B + 1], u[i + B + 2]);
      printf("%d %u %d\n", v.slot, v.word, (int)v.empty);
    }
  } else if (cmd == "gen_size" && read_records(argv[2], 2, &q)) {
    for (size_t i = 0; i < q.size(); i += 2) printf("%llu\n", az::cache_gen_size(q[i], q[i + 1]));
  } else {
    return 3;
  }
  return 0;
}
