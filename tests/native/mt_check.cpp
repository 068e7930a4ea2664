// Host build of the engines' shared MT19937 stream (csrc/az_mt.h) and numpy
// pairwise sum (csrc/az_device.h pairwise_sum), test infrastructure for
// tests/test_mt_cpu.py.  The stream lives in a word-major array of STRIDE
// slots as on the device; with STRIDE > 1 it is slot 1 and the other slots
// hold a sentinel that every command checks afterwards (exit 4 when a
// neighbour was written; "neighbours untouched" on the last line otherwise).
//   mt_check seed SEED STRIDE       -> the 624 state words after mt_seed, then "index <i>"
//   mt_check uniform SEED STRIDE N  -> N mt_uniform values in hex, then "index <i>"
//   mt_check skip SEED STRIDE N     -> "index <i>" after mt_seed + mt_skip(N), then the next mt_uniform in hex
//   mt_check sum f32|f64 FILE N...  -> per N: "<N> <pairwise_sum<256>> <pairwise_sum<128> or ->" of the
//                                      first N values of FILE (raw float32 / float64), in hex
// Built with -ffp-contract=off like the tree kernels that include the headers.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../custom-alphazero_amd/csrc/az_mt.h"

namespace {

constexpr uint32_t kSentinel = 0xa5a5a5a5u;

struct Slots {
  std::vector<uint32_t> words;
  size_t stride;
  az::MtStream stream;
  explicit Slots(size_t n) : words((az::kMtN + 1) * n, kSentinel), stride(n) {
    stream = {words.data() + (n > 1 ? 1 : 0), n};
  }
  int finish() const {
    for (size_t w = 0; w <= (size_t)az::kMtN; ++w)
      for (size_t s = 0; s < stride; ++s)
        if (stride > 1 && s != 1 && words[w * stride + s] != kSentinel) {
          fprintf(stderr, "word %zu of slot %zu was written\n", w, s);
          return 4;
        }
    printf("neighbours untouched\n");
    return 0;
  }
  unsigned index() const { return stream.m[(size_t)az::kMtN * stride]; }
};

template <typename T>
int sums(const char* path, int argc, char** argv) {
  std::vector<T> a(256);
  FILE* f = fopen(path, "rb");
  if (!f || fread(a.data(), sizeof(T), a.size(), f) != a.size()) return 3;
  fclose(f);
  for (int i = 0; i < argc; ++i) {
    const int n = atoi(argv[i]);
    if (n < 0 || n > 256) return 2;
    printf("%d %a", n, (double)az::pairwise_sum<256>(a.data(), n));
    if (n <= 128)
      printf(" %a\n", (double)az::pairwise_sum<128>(a.data(), n));
    else
      printf(" -\n");
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 4 && !strcmp(argv[1], "sum")) {
    if (!strcmp(argv[2], "f32")) return sums<float>(argv[3], argc - 4, argv + 4);
    if (!strcmp(argv[2], "f64")) return sums<double>(argv[3], argc - 4, argv + 4);
  }
  if (argc >= 4 && (!strcmp(argv[1], "seed") || !strcmp(argv[1], "uniform") || !strcmp(argv[1], "skip"))) {
    const int stride = atoi(argv[3]);
    const long n = argc >= 5 ? atol(argv[4]) : 0;
    if (stride < 1 || n < 0 || (strcmp(argv[1], "seed") && argc < 5)) return 2;
    Slots s((size_t)stride);
    az::mt_seed(s.stream, (uint32_t)strtoul(argv[2], nullptr, 10));
    if (!strcmp(argv[1], "seed")) {
      for (int w = 0; w < az::kMtN; ++w) printf("%u\n", s.stream.m[(size_t)w * s.stride]);
      printf("index %u\n", s.index());
    } else if (!strcmp(argv[1], "uniform")) {
      for (long i = 0; i < n; ++i) printf("%a\n", az::mt_uniform(s.stream));
      printf("index %u\n", s.index());
    } else {
      az::mt_skip(s.stream, (int)n);
      printf("index %u\n", s.index());
      printf("%a\n", az::mt_uniform(s.stream));
    }
    return s.finish();
  }
  fprintf(stderr, "usage\n");
  return 2;
}
