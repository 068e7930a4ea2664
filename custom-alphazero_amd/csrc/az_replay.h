// az_replay.h -- the chess replay window on the device (az_chess_replay_* in
// include/az_chess.h, csrc/az_replay.hip), as the trainer sees it
// (az_trainer_step_replay, csrc/az_train.hip).
//
// A ring of `capacity` compact samples, a structure of arrays: the 8 history
// positions and their valid flags (az_chess_encode's form), the sparse policy
// (count, action indices, float64 probabilities) and the value.  One kernel
// gathers a batch by window index, encodes it to Board.full_state planes and
// scatters the policy to dense float32 rows.
#ifndef AZ_REPLAY_H_
#define AZ_REPLAY_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/az_chess.h"

namespace az {
namespace replay {

int device_of(const az_chess_replay* rp);

// Checks idx [n] (host; 0 = the oldest sample held) against the window, copies it to the
// device on `s` and launches the gather there: x [n][8][8][118], pi [n][1880], z [n] are
// device buffers, any of them null.  AZ_E_STATE on an empty window, AZ_E_INVALID on an index
// outside it; `who` names the caller in the message.  Does not synchronise: idx must stay
// valid, and the replay untouched, until `s` has run the launch.
int gather_on(az_chess_replay* rp, const int64_t* idx, int n, hipStream_t s, float* x, float* pi, float* z,
              const char* who);

}  // namespace replay
}  // namespace az

#endif  // AZ_REPLAY_H_
