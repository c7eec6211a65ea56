// What the tangent kernels (sens.hip, sens_sbm.hip) and the field-mu kernels (fieldmu.hip) share: the geometry of the
// 16 x 32 tile with its 2-cell ring, and the derivative of a closure with respect to one of its coefficients (the
// derivative with respect to its argument, closure_dc, is in closures.hpp).
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

// ---- stencil primitives on a tile in LDS (row pitch ld): the forward kernels' expressions, in their order -----------
// Users: the operator kernels of the implicit step (implicit.hip).  The tangent kernels of sens.hip keep these same
// expressions written out in their bodies, so that they compile to what they always compiled to.

// 5-point Laplacian of s at offset o
template <typename T>
__device__ __forceinline__ T tile_lap5(const T* __restrict__ s, int o, int ld, T rhx2, T rhy2) {
  const T c = s[o];
  return (s[o + ld] - T(2) * c + s[o - ld]) * rhx2 + (s[o + 1] - T(2) * c + s[o - 1]) * rhy2;
}

// the linearised Cahn-Hilliard flux through the face between the cells at offsets a (lower index) and b of a tile:
// avg(dD) grad(mu) + avg(D) grad(dmu)
template <typename T>
__device__ __forceinline__ T tile_tangent_flux(const T* __restrict__ smu, const T* __restrict__ sD, const T* __restrict__ sdmu,
                                               const T* __restrict__ sdD, int a, int b, T rh) {
  return T(0.5) * (sdD[a] + sdD[b]) * ((smu[b] - smu[a]) * rh) + T(0.5) * (sD[a] + sD[b]) * ((sdmu[b] - sdmu[a]) * rh);
}

// ---- closure derivatives (the family of include/pdeopt_hip.h; values from closure_generic) ------------------------

// 1 / q of the Legendre recurrence below: a multiply per term instead of a division (the tangent kernels evaluate
// the basis once per cell and tangent)
[[maybe_unused]] static __constant__ double kRecip[PDEOPT_CLOSURE_MAX_COEF] = {
    0.0,     1.0,     1.0 / 2,  1.0 / 3,  1.0 / 4,  1.0 / 5,  1.0 / 6,  1.0 / 7,
    1.0 / 8, 1.0 / 9, 1.0 / 10, 1.0 / 11, 1.0 / 12, 1.0 / 13, 1.0 / 14, 1.0 / 15};

// df/dcoef[k] at c: the basis function B_k(c) = c^k or P_k(2c - 1), times f under EXP_WRAP
template <typename T>
__device__ __forceinline__ T closure_dcoef(const ClosureSpec& s, int k, T c, T f) {
  T b = T(1);
  if (s.kind == PDEOPT_CL_POLY) {
    for (int q = 0; q < k; ++q) b *= c;
  } else if (k > 0) {
    const T x = T(2) * c - T(1);
    T pm = T(1);
    b = x;
    for (int q = 2; q <= k; ++q) {
      const T pn = (T(2 * q - 1) * x * b - T(q - 1) * pm) * T(kRecip[q]);
      pm = b;
      b = pn;
    }
  }
  if (s.flags & PDEOPT_CL_EXP_WRAP) b *= f;
  return b;
}

}  // namespace pdeopt
