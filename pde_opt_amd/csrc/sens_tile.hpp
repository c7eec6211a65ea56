// What the tangent kernels (sens.hip) and the field-mu kernels (fieldmu.hip) share: the geometry of the 16 x 32 tile with
// its 2-cell ring (the derivative of a closure with respect to its argument, closure_dc, is in closures.hpp).
#pragma once

#include "closures.hpp"
#include "common.hpp"

namespace pdeopt {

// Output tile TR x TC; the stencil reads u on a 2-cell ring (mu at the 1-cell ring needs lap u there).
constexpr int kTR = 16, kTC = 32, kR2 = kTR + 4, kC2 = kTC + 4, kR1 = kTR + 2, kC1 = kTC + 2;

// periodic index of g in [-2, n + kTC + 1]: one add or subtract, the division only on grids smaller than a tile
__device__ __forceinline__ int wrap_idx(int g, int n) {
  g = g < 0 ? g + n : (g >= n ? g - n : g);
  if ((unsigned)g >= (unsigned)n) g = ((g % n) + n) % n;
  return g;
}

}  // namespace pdeopt
