// The line operator of the rotating-frame split step, shared by the step (gpe_rot.hip) and its adjoint
// (gpe_rot_adjoint.hip), frozen and stirred: the multiplier of a line is a 1-D kinetic table per axis,
// exp(tau/2 0.5j (2 pi i k)^2) / N, times the rotation factor exp(-/+ Omega coord (2 pi i k) tau/2), evaluated
// in-kernel from Omega (EnvParams: one per environment), the line's coordinate and k: no N^2 table.
#pragma once

#include <cmath>
#include <complex>
#include <vector>

#include "common.hpp"
#include "fft_lds.hpp"
#include "split_step_util.hpp"

namespace pdeopt {

// one axis's line operator: theta = a k_signed with a = w Omega coord, w = -/+ 2 pi / (N h) (the sign of the
// rotation term: - for lines along x, + for lines along y), s = tau / 2 = sr + i si
template <typename T>
struct RotAxis {
  T w, c_first, c_step, sr, si;
};

// kin * exp(i theta s) = kin * exp(-theta si) (cos(theta sr) + i sin(theta sr)),  theta = a * fftfreq index of f
template <typename T>
__device__ __forceinline__ Cx<T> rot_mult(Cx<T> kin, T a, int f, int n, T sr, T si) {
  const int ks = f < (n + 1) / 2 ? f : f - n;
  const T th = a * T(ks);
  T sn, cs;
  sincos_t<T>(th * sr, &sn, &cs);
  const T mag = (si == T(0)) ? T(1) : exp_t<T>(-th * si);
  return cmul(kin, Cx<T>{mag * cs, mag * sn});
}

// Omega(t) of an environment: one fused multiply-add everywhere (the rstir_ kernels of the step and the rsadj_ kernels
// of its adjoint), so every kernel forms the same number
__device__ __forceinline__ float rot_omega_at(const EnvParams<float>& e, float t) {
  return __builtin_fmaf(e.gpe_omega_rate, t, e.gpe_omega);
}
__device__ __forceinline__ double rot_omega_at(const EnvParams<double>& e, double t) {
  return __builtin_fma(e.gpe_omega_rate, t, e.gpe_omega);
}

template <typename T>
RotAxis<T> rot_axis(const pdeopt_ctx* ctx, int axis, std::complex<double> half_tau) {
  const pdeopt_problem& p = ctx->prob;
  RotAxis<T> a;
  if (axis == 0) {  // lines along x: -Omega y (2 pi i kx)
    a.w = (T)(-2.0 * M_PI / ((double)p.nx * p.hx));
    a.c_first = (T)ctx->rot_y_first;
    a.c_step = (T)p.hy;
  } else {          // lines along y: +Omega x (2 pi i ky)
    a.w = (T)(2.0 * M_PI / ((double)p.ny * p.hy));
    a.c_first = (T)ctx->rot_x_first;
    a.c_step = (T)p.hx;
  }
  a.sr = (T)half_tau.real();
  a.si = (T)half_tau.imag();
  return a;
}

template <typename T>
int upload_kinetic(pdeopt_ctx* ctx, DeviceBuffer& dev, int n, double h, std::complex<double> half_tau) {
  std::vector<Cx<T>> t((size_t)n);
  for (int f = 0; f < n; ++f) {
    const int ks = f < (n + 1) / 2 ? f : f - n;
    const double k = (double)ks / ((double)n * h);
    const std::complex<double> ik(0.0, 2.0 * M_PI * k);
    const std::complex<double> e = std::exp(half_tau * std::complex<double>(0.0, 0.5) * ik * ik) / (double)n;
    t[f] = Cx<T>{(T)e.real(), (T)e.imag()};
  }
  int rc = ensure_buffer(ctx, dev, t.size() * sizeof(Cx<T>));
  if (rc) return rc;
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(dev.get(), t.data(), t.size() * sizeof(Cx<T>), hipMemcpyHostToDevice, ctx->stream));
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PDEOPT_OK;
}

}  // namespace pdeopt
