// az_move_clock.h -- which self-play move a drain may read.  No HIP here:
// the rule is a pure function, tested on the host (tests/native/move_clock_check.cpp).
#pragma once
#include <stdint.h>

namespace az {

// Moves are numbered over the engine's life; a batch (*_selfplay_begin) owns
// the moves from batch_first_move on.  A move's games-finished snapshot is
// complete once every lane has finished the move.
struct DrainMove {
  int64_t move;  // the newest move whose snapshot may be read, -1: none
  bool wait;     // it may still be running on some lane: wait for its events first
};

// last: the last move issued (moves_issued - 1); last_done: every lane has
// finished it.  A drain never waits for the running move, only for the one
// before it, and never reads a snapshot of an earlier batch.
inline DrainMove drainable_move(int64_t last, int64_t batch_first_move, bool last_done) {
  if (last >= batch_first_move && last_done) return {last, false};
  if (last - 1 >= batch_first_move) return {last - 1, true};
  return {-1, false};
}

}  // namespace az
