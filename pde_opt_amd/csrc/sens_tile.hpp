// What the tangent kernels (sens.hip) and the field-mu kernels (fieldmu.hip) share: the derivative of a closure of the
// in-kernel family with respect to its argument, and the geometry of the 16 x 32 tile with its 2-cell ring.
#pragma once

#include "closures.hpp"
#include "common.hpp"

namespace pdeopt {

// df/dc at c, where f = closure_generic(s, coef, c) is passed in (the exp-wrapped value when EXP_WRAP is set)
template <typename T>
__device__ __forceinline__ T closure_dc(const ClosureSpec& s, const T* __restrict__ coef, T c, T f) {
  T d = T(0);
  if (s.kind == PDEOPT_CL_POLY) {
    for (int k = s.n - 1; k >= 1; --k) d = d * c + T(k) * coef[k];
  } else {
    // d/dc sum_k a_k P_k(2c - 1) = 2 sum_k a_k P'_k(x),  P'_{k+1} = P'_{k-1} + (2k + 1) P_k
    const T x = T(2) * c - T(1);
    T pm = T(1), pc = x, dpm = T(0), dpc = T(1);
    if (s.n > 1) d = coef[1];
    for (int k = 1; k + 1 < s.n; ++k) {
      const T pn = (T(2 * k + 1) * x * pc - T(k) * pm) / T(k + 1);
      const T dpn = dpm + T(2 * k + 1) * pc;
      d += coef[k + 1] * dpn;
      pm = pc;
      pc = pn;
      dpm = dpc;
      dpc = dpn;
    }
    d *= T(2);
  }
  if (s.flags & PDEOPT_CL_LOGIT_PRIOR) d += T(1) / (c * (T(1) - c));
  if (s.flags & PDEOPT_CL_MIX_ENTROPY) d += t_logit<T>(c);
  if (s.flags & PDEOPT_CL_EXP_WRAP) d *= f;
  return d;
}

// Output tile TR x TC; the stencil reads u on a 2-cell ring (mu at the 1-cell ring needs lap u there).
constexpr int kTR = 16, kTC = 32, kR2 = kTR + 4, kC2 = kTC + 4, kR1 = kTR + 2, kC1 = kTC + 2;

// periodic index of g in [-2, n + kTC + 1]: one add or subtract, the division only on grids smaller than a tile
__device__ __forceinline__ int wrap_idx(int g, int n) {
  g = g < 0 ? g + n : (g >= n ? g - n : g);
  if ((unsigned)g >= (unsigned)n) g = ((g % n) + n) % n;
  return g;
}

}  // namespace pdeopt
