// Helpers the split-step translation units share (strang_fused.hip, gpe_rot.hip): the unit-modulus factor
// exp(i x) in the working precision, the dynamic-LDS opt-in of a kernel, and the twiddle table of a transform.
#pragma once

#include <cmath>
#include <vector>

#include "common.hpp"
#include "fft_lds.hpp"

namespace pdeopt {

template <typename T>
__device__ __forceinline__ void sincos_t(T x, T* s, T* c);
// fp32: hardware v_sin_f32 / v_cos_f32 (arguments in revolutions) behind a two-term reduction of
// x / 2 pi, instead of ocml's sincosf (~45 VALU instructions per call plus a private-memory slow
// path): the row pass evaluates one per cell and was VALU-bound on it.  Absolute error ~2e-7 on a
// unit-modulus factor, below the fp32 rounding of the transforms around it; fp64 keeps sincos().
template <>
__device__ __forceinline__ void sincos_t<float>(float x, float* s, float* c) {
  const float c1 = 0.15915494f;        // fl(1 / 2 pi)
  const float c2 = 6.4206383e-09f;     // 1 / 2 pi - c1
  const float hi = x * c1;
  const float lo = __builtin_fmaf(x, c1, -hi) + x * c2;
  const float r = __builtin_amdgcn_fractf(hi) + lo;  // revolutions, |lo| tiny: sin / cos are 1-periodic in r
  *s = __builtin_amdgcn_sinf(r);
  *c = __builtin_amdgcn_cosf(r);
}
template <>
__device__ __forceinline__ void sincos_t<double>(double x, double* s, double* c) { sincos(x, s, c); }
template <typename T>
__device__ __forceinline__ T exp_t(T x);
template <>
__device__ __forceinline__ float exp_t<float>(float x) { return expf(x); }
template <>
__device__ __forceinline__ double exp_t<double>(double x) { return exp(x); }

template <typename K>
int allow_lds(pdeopt_ctx* ctx, K kernel, size_t bytes) {
  if (bytes > 48 * 1024)
    PDEOPT_HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return PDEOPT_OK;
}

// exp(-2 pi i k / n), k < n, in the problem dtype
template <typename T>
int upload_table(pdeopt_ctx* ctx, DeviceBuffer& dev, int n) {
  std::vector<Cx<T>> h((size_t)n);
  for (int k = 0; k < n; ++k) {
    const double a = -2.0 * M_PI * (double)k / (double)n;
    h[k] = Cx<T>{(T)std::cos(a), (T)std::sin(a)};
  }
  int rc = ensure_buffer(ctx, dev, h.size() * sizeof(Cx<T>));
  if (rc) return rc;
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(dev.get(), h.data(), h.size() * sizeof(Cx<T>), hipMemcpyHostToDevice, ctx->stream));
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PDEOPT_OK;
}

}  // namespace pdeopt
