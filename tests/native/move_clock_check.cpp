// The drain's rule for the move whose snapshot it may read (az_move_clock.h),
// on its five cases.  Host only: the header includes nothing of HIP.
#include <stdio.h>

#include <initializer_list>

#include "az_move_clock.h"

static int failures = 0;

static void expect(const char* what, int64_t last, int64_t first, bool last_done, int64_t move, bool wait) {
  const az::DrainMove k = az::drainable_move(last, first, last_done);
  if (k.move == move && (move < 0 || k.wait == wait)) return;
  printf("FAIL %s: last=%lld first=%lld last_done=%d -> move=%lld wait=%d, expected move=%lld wait=%d\n", what,
         (long long)last, (long long)first, (int)last_done, (long long)k.move, (int)k.wait, (long long)move, (int)wait);
  ++failures;
}

int main() {
  // moves are numbered over the engine's life: a batch begun after `first`
  // moves owns the moves first, first + 1, ...; last = moves_issued - 1
  for (int64_t first : {(int64_t)0, (int64_t)1, (int64_t)7, (int64_t)1 << 40}) {
    // 1. no move issued since begin_batch (the earlier batch's last move has finished, or never ran)
    expect("no move issued", first - 1, first, true, -1, false);
    expect("no move issued", first - 1, first, false, -1, false);
    for (int64_t n = 1; n <= 9; ++n) {  // n moves issued in this batch (past the 4-slot ring too)
      const int64_t last = first + n - 1;
      // 2. the last move finished on every lane: that move, no wait
      expect("last move finished", last, first, true, last, false);
      if (n >= 2)  // 3. the last move running, a move of this batch before it: that one, with a wait
        expect("last running, one before it", last, first, false, last - 1, true);
      else  // 4. the last move running and it is the batch's first
        expect("last running, batch's first", last, first, false, -1, false);
    }
    // 5. never a move of an earlier batch, whatever the events say
    for (int64_t last = first - 3; last <= first + 9; ++last)
      for (bool done : {false, true}) {
        const az::DrainMove k = az::drainable_move(last, first, done);
        if (k.move >= 0 && k.move < first) {
          printf("FAIL earlier batch: last=%lld first=%lld last_done=%d -> move=%lld\n", (long long)last,
                 (long long)first, (int)done, (long long)k.move);
          ++failures;
        }
      }
  }
  printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
