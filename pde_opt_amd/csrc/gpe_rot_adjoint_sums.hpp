// The gather-form reductions shared by the frozen and the stirred adjoint of the rotating-frame split step
// (gpe_rot_adjoint.hip): a fixed partition of kRadjBlocks workgroups per environment, every workgroup leaves one
// fp64 partial per sum (block_sum of block_sums.hpp), and whoever needs a total adds the partials in one fixed order.
// No atomics: a repeat gives the same bits.
#pragma once

#include <cstdint>

#include "block_sums.hpp"
#include "common.hpp"

namespace pdeopt {

constexpr int kRadjBlocks = 128;  // workgroups per environment: the fixed partition of every reduction

// the sum of one slot over the partition (part: [batch][kRadjBlocks][slots]), every caller in the same order (one wave:
// threads 0 .. 63); valid in lane 0
__device__ __forceinline__ double radj_slot_total(const double* part, int slots, int b, int slot, int lane) {
  const double* p = part + (int64_t)b * kRadjBlocks * slots + slot;
  double v = 0.0;
  for (int q = lane; q < kRadjBlocks; q += 64) v += p[(int64_t)q * slots];
  return wave_sum(v);
}

}  // namespace pdeopt
