// One substep of the discrete adjoint of StrangSplitting.step for the GPE whose control field is a sum of Gaussian
// spots (pdeopt_set_gpe_spots): the reverse-mode gradient of a scalar objective of the solution over the spots' numbers
// (the reference's PDEModel.optimize differentiates this solve with generic reverse-mode AD, pde_model.py:462-551).
//
// Forward substep (strang_fused.hip:4-6), tau = dt * time_scale, E = exp(A_term tau / 2), K v = ifft2(E fft2 v),
// h^2 = strang_dx^2:
//   a = K psi0;  beta = -(V_trap + lights(t0) + k |psi0|^2)  (PRE-half-step state);  c = a exp(i beta tau)
//   n = sqrt(h^2 sum |c|^2);  d = c / n;  psi1 = K d
// Cotangents are complex fields dJ/dRe + i dJ/dIm in the state's (re, im) storage, the inner product is the real one.
// With K^H v = ifft2(conj(E) fft2 v) and lambda1 the cotangent of psi1:
//   lambda_d = K^H lambda1;  s = h^2 sum Re(conj(d) lambda_d);  lambda_c = (lambda_d - s d) / n
//   lambda_a = lambda_c conj(exp(i beta tau));  g_beta = Re(conj(i tau c) lambda_c)
//   lambda0 = K^H lambda_a - 2 k g_beta psi0;  dJ/dtheta += sum over cells of (-g_beta) dlights(t0)/dtheta
//
// Per substep: three transform round trips on the library's rocFFT plans (a, lambda_d, K^H lambda_a: every grid the
// forward step takes) and three passes over the field between them:
//   recompute : c from a, partial sums of |c|^2 and of Re(conj(c) lambda_d)
//   pointwise : lambda_a, the direct term -2 k g_beta psi0, partial sums of the spots' partials
//   finish    : lambda0 = K^H lambda_a + direct term; one workgroup per environment sums the spot partials
// Every reduction is in gather form, no atomics: a fixed partition (kBlocks workgroups per environment), fp64
// partials summed in a fixed order -- the scheme of the norm reduction of the forward step.  A repeat gives the same bits.
#include <cmath>
#include <complex>

#include "block_sums.hpp"
#include "common.hpp"

namespace pdeopt {

struct GpeAdjoint : Feature {
  DeviceBuffer work;    // a, then c               [batch][nx][ny] complex
  DeviceBuffer direct;  // -2 k g_beta psi0        same
  DeviceBuffer mult;    // E / (nx ny)             [nx][ny] complex
  DeviceBuffer part;    // doubles [batch][kBlocks][2]
  DeviceBuffer spart;   // doubles [batch][kBlocks][kSpotSums]
  DeviceBuffer gacc;    // doubles [batch][PDEOPT_MAX_SPOTS][7]: staging of a host gradient block
  bool mult_valid = false;
  double key_dt = NAN, key_tr = NAN, key_ti = NAN;

  void invalidate() override { mult_valid = false; }
};

namespace {

constexpr int kBlocks = 128;                      // workgroups per environment: the fixed partition of every reduction
constexpr int kSpotSums = 4 * PDEOPT_MAX_SPOTS;   // independent sums per environment (spot_partials)

template <typename T>
struct C2 {
  T re, im;
};

template <typename T>
struct GpeAdjArgs {
  C2<T>* work;            // recompute: a in, c out; pointwise: c
  const C2<T>* psi0;
  C2<T>* lam;             // lambda_d in (recompute, pointwise), lambda_a out (pointwise)
  C2<T>* direct;
  const T* pot;           // trap potential, nullptr: none
  int64_t pot_stride;     // elements between environments (0: shared)
  const EnvParams<T>* ep;
  T tr, ti;               // tau
  int64_t cells;
  int ny;
  double h2;
  double* part;
  double* spart;
  SpotArgs<T> spots;
};

template <typename T>
__device__ __forceinline__ void adj_sincos(T x, T* s, T* c);
template <>
__device__ __forceinline__ void adj_sincos<float>(float x, float* s, float* c) { sincosf(x, s, c); }
template <>
__device__ __forceinline__ void adj_sincos<double>(double x, double* s, double* c) { sincos(x, s, c); }
template <typename T>
__device__ __forceinline__ T adj_exp(T x);
template <>
__device__ __forceinline__ float adj_exp<float>(float x) { return expf(x); }
template <>
__device__ __forceinline__ double adj_exp<double>(double x) { return exp(x); }

// exp(i beta tau) = exp(-i w tau), w = V + k |psi0|^2 + lights(t0): the expression of strang_b_kernel
template <typename T>
__device__ __forceinline__ C2<T> phase_factor(const GpeAdjArgs<T>& a, int env, int64_t i, C2<T> p0, T kk) {
  T w = (a.pot ? a.pot[(int64_t)env * a.pot_stride + i] : T(0)) + kk * (p0.re * p0.re + p0.im * p0.im);
  if (a.spots.n)
    w += spots_value<T>(a.spots, env, a.spots.x_first + T(i / a.ny) * a.spots.hx, a.spots.y_first + T(i % a.ny) * a.spots.hy);
  T sn, cs;
  adj_sincos<T>(w * a.tr, &sn, &cs);
  const T mag = (a.ti == T(0)) ? T(1) : adj_exp<T>(w * a.ti);
  return C2<T>{mag * cs, -mag * sn};
}

// c[b][cell] *= m[cell] or conj(m[cell])
template <typename T, bool CONJ>
__global__ __launch_bounds__(256) void gpe_adjoint_mul_kernel(C2<T>* __restrict__ c, const C2<T>* __restrict__ m, int64_t cells) {
  C2<T>* cb = c + (int64_t)blockIdx.y * cells;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (int64_t)gridDim.x * 256) {
    const C2<T> v = cb[i];
    C2<T> w = m[i];
    if (CONJ) w.im = -w.im;
    cb[i] = C2<T>{v.re * w.re - v.im * w.im, v.re * w.im + v.im * w.re};
  }
}

// work: a -> c = a exp(i beta tau);  part[b][block] = (sum |c|^2, sum Re(conj(c) lambda_d))
template <typename T>
__global__ __launch_bounds__(256) void gpe_adjoint_recompute_kernel(const GpeAdjArgs<T> a) {
  __shared__ double sh[4];
  const int b = blockIdx.y;
  const int64_t o = (int64_t)b * a.cells;
  const T kk = a.ep[b].gpe_k;
  double acc_n = 0.0, acc_s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.cells; i += (int64_t)gridDim.x * 256) {
    const C2<T> e = phase_factor<T>(a, b, i, a.psi0[o + i], kk);
    const C2<T> v = a.work[o + i], l = a.lam[o + i];
    const C2<T> c{v.re * e.re - v.im * e.im, v.re * e.im + v.im * e.re};
    a.work[o + i] = c;
    acc_n += (double)c.re * (double)c.re + (double)c.im * (double)c.im;
    acc_s += (double)c.re * (double)l.re + (double)c.im * (double)l.im;
  }
  const double sn = block_sum(acc_n, sh);
  const double ss = block_sum(acc_s, sh);
  if (threadIdx.x == 0) {
    double* p = a.part + ((int64_t)b * kBlocks + blockIdx.x) * 2;
    p[0] = sn;
    p[1] = ss;
  }
}

// lam: lambda_d -> lambda_a;  direct = -2 k g_beta psi0;  spart[b][block][4 s + q] = sum of -g_beta x partial q of spot s
template <typename T>
__global__ __launch_bounds__(256) void gpe_adjoint_pointwise_kernel(const GpeAdjArgs<T> a) {
  __shared__ double sh[4];
  __shared__ double tot[2];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t o = (int64_t)b * a.cells;
  // the two sums of this environment, every workgroup in the same order
  if (tid < 64) {
    const double* p = a.part + (int64_t)b * kBlocks * 2;
    double sn = 0.0, ss = 0.0;
    for (int q = tid; q < kBlocks; q += 64) {
      sn += p[2 * q];
      ss += p[2 * q + 1];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {  // (two wave_sum calls lengthen this kernel by 14 instructions)
      sn += __shfl_down(sn, off, 64);
      ss += __shfl_down(ss, off, 64);
    }
    if (tid == 0) {
      tot[0] = sn;
      tot[1] = ss;
    }
  }
  __syncthreads();
  const double nrm = sqrt(tot[0] * a.h2);
  const T inv_n = (T)(1.0 / nrm);
  const T s_over_n = (T)(a.h2 * tot[1] / (nrm * nrm));  // s / n with s = h^2 sum Re(conj(c) lambda_d) / n
  const T kk = a.ep[b].gpe_k;
  const int ns = a.spots.n;
  double acc[kSpotSums];
#pragma unroll
  for (int q = 0; q < kSpotSums; ++q) acc[q] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < a.cells; i += (int64_t)gridDim.x * 256) {
    const C2<T> p0 = a.psi0[o + i];
    const C2<T> e = phase_factor<T>(a, b, i, p0, kk);
    const C2<T> c = a.work[o + i], ld = a.lam[o + i];
    // lambda_c = (lambda_d - s d) / n, d = c / n
    const C2<T> lc{(ld.re - s_over_n * c.re) * inv_n, (ld.im - s_over_n * c.im) * inv_n};
    // lambda_a = lambda_c conj(e)
    a.lam[o + i] = C2<T>{lc.re * e.re + lc.im * e.im, lc.im * e.re - lc.re * e.im};
    // g_beta = Re(conj(i tau c) lambda_c), i tau = -ti + i tr
    const T zr = -a.ti * c.re - a.tr * c.im, zi = a.tr * c.re - a.ti * c.im;
    const T gb = zr * lc.re + zi * lc.im;
    const T f = T(-2) * kk * gb;
    a.direct[o + i] = C2<T>{f * p0.re, f * p0.im};
    const T x = a.spots.x_first + T(i / a.ny) * a.spots.hx, y = a.spots.y_first + T(i % a.ny) * a.spots.hy;
#pragma unroll
    for (int s = 0; s < PDEOPT_MAX_SPOTS; ++s) {
      if (s < ns) {
        T d[4];
        spot_partials<T>(a.spots, b, s, x, y, d);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[4 * s + q] -= (double)gb * (double)d[q];
      }
    }
  }
  double* out = a.spart + ((int64_t)b * kBlocks + blockIdx.x) * kSpotSums;
#pragma unroll
  for (int q = 0; q < kSpotSums; ++q) {
    const double v = block_sum(acc[q], sh);
    if (tid == 0) out[q] = v;
  }
}

// lam += direct;  workgroup 0 of every environment: grad[b][s][0..6] += the spot sums (rates: t x their value's sum)
template <typename T>
__global__ __launch_bounds__(256) void gpe_adjoint_finish_kernel(C2<T>* __restrict__ lam, const C2<T>* __restrict__ direct,
                                                                 int64_t cells, const double* __restrict__ spart,
                                                                 double* __restrict__ grad, int n_spots, double t) {
  const int b = blockIdx.y;
  const int64_t o = (int64_t)b * cells;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (int64_t)gridDim.x * 256) {
    const C2<T> d = direct[o + i];
    C2<T> l = lam[o + i];
    l.re += d.re;
    l.im += d.im;
    lam[o + i] = l;
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < 4 * n_spots) {
    const int s = threadIdx.x >> 2, q = threadIdx.x & 3;
    const double* p = spart + (int64_t)b * kBlocks * kSpotSums + 4 * s + q;
    double v = 0.0;
    for (int k = 0; k < kBlocks; ++k) v += p[(int64_t)k * kSpotSums];
    double* g = grad + ((int64_t)b * n_spots + s) * 7;  // amp0, amp_rate, x0, x_rate, y0, y_rate, inv_two_w2
    if (q == 3) {
      g[6] += v;
    } else {
      g[2 * q] += v;
      g[2 * q + 1] += t * v;
    }
  }
}

template <typename T>
int ensure_mult(pdeopt_ctx* ctx, GpeAdjoint& ga, double dt) {
  if (ga.mult_valid && ga.key_dt == dt && ga.key_tr == ctx->ts_re && ga.key_ti == ctx->ts_im) return PDEOPT_OK;
  std::vector<std::complex<double>> at;
  int rc = spectral_fetch_complex_aux(ctx, PDEOPT_AUX_GPE_A_TERM, at);
  if (rc) return rc;
  const std::complex<double> tau = dt * std::complex<double>(ctx->ts_re, ctx->ts_im);
  const double inv_n = 1.0 / (double)at.size();
  std::vector<C2<T>> m(at.size());
  for (size_t i = 0; i < at.size(); ++i) {
    const std::complex<double> e = std::exp(at[i] * 0.5 * tau) * inv_n;
    m[i] = C2<T>{(T)e.real(), (T)e.imag()};
  }
  if ((rc = ensure_buffer(ctx, ga.mult, m.size() * sizeof(C2<T>)))) return rc;
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(ga.mult.get(), m.data(), m.size() * sizeof(C2<T>), hipMemcpyHostToDevice, ctx->stream));
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  ga.mult_valid = true;
  ga.key_dt = dt;
  ga.key_tr = ctx->ts_re;
  ga.key_ti = ctx->ts_im;
  return PDEOPT_OK;
}

// buf <- ifft2(M fft2 buf), M = E / (nx ny) or its conjugate
template <typename T, bool CONJ>
int round_trip(pdeopt_ctx* ctx, GpeAdjoint& ga, void* buf, dim3 grid, int64_t cells) {
  int rc = spectral_c2c(ctx, true, buf);
  if (rc) return rc;
  hipLaunchKernelGGL((gpe_adjoint_mul_kernel<T, CONJ>), grid, dim3(256), 0, ctx->stream, (C2<T>*)buf, ga.mult.as<const C2<T>>(), cells);
  return spectral_c2c(ctx, false, buf);
}

template <typename T>
int adjoint_step_t(pdeopt_ctx* ctx, double t0, double dt, const void* psi0, void* lam, double* grad_dev) {
  GpeAdjoint& ga = *ctx->features.get<GpeAdjoint>(FS_GPE_ADJOINT);
  const pdeopt_problem& p = ctx->prob;
  const int64_t cells = (int64_t)p.nx * p.ny;
  int rc = ensure_mult<T>(ctx, ga, dt);
  if (rc) return rc;
  const dim3 grid(kBlocks, p.batch);
  const AuxField& pot = ctx->aux[PDEOPT_AUX_GPE_POTENTIAL];
  const std::complex<double> tau = dt * std::complex<double>(ctx->ts_re, ctx->ts_im);
  GpeAdjArgs<T> a{};
  a.work = ga.work.as<C2<T>>();
  a.psi0 = (const C2<T>*)psi0;
  a.lam = (C2<T>*)lam;
  a.direct = ga.direct.as<C2<T>>();
  a.pot = pot.dev.as<const T>();
  a.pot_stride = pot.per_env ? cells : 0;
  a.ep = env_params<T>(ctx, 0);
  a.tr = (T)tau.real();
  a.ti = (T)tau.imag();
  a.cells = cells;
  a.ny = p.ny;
  a.h2 = ctx->strang_dx * ctx->strang_dx;
  a.part = ga.part.as<double>();
  a.spart = ga.spart.as<double>();
  a.spots = make_spot_args<T>(ctx, 0, t0);
  // a = K psi0
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(ga.work.get(), psi0, ctx->total_bytes, hipMemcpyDeviceToDevice, ctx->stream));
  if ((rc = round_trip<T, false>(ctx, ga, ga.work.get(), grid, cells))) return rc;
  // lambda_d = K^H lambda1
  if ((rc = round_trip<T, true>(ctx, ga, lam, grid, cells))) return rc;
  hipLaunchKernelGGL(gpe_adjoint_recompute_kernel<T>, grid, dim3(256), 0, ctx->stream, a);
  hipLaunchKernelGGL(gpe_adjoint_pointwise_kernel<T>, grid, dim3(256), 0, ctx->stream, a);
  // lambda0 = K^H lambda_a + direct
  if ((rc = round_trip<T, true>(ctx, ga, lam, grid, cells))) return rc;
  hipLaunchKernelGGL(gpe_adjoint_finish_kernel<T>, grid, dim3(256), 0, ctx->stream, (C2<T>*)lam, ga.direct.as<const C2<T>>(), cells,
                     ga.spart.as<const double>(), grad_dev, ctx->n_spots, t0);
  ctx->n_stage_launches += 12;  // 6 transforms, 3 multiplies, 3 passes
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  return PDEOPT_OK;
}

}  // namespace

}  // namespace pdeopt

using namespace pdeopt;

extern "C" {

int pdeopt_gpe_adjoint_step(pdeopt_ctx* ctx, double t0, double dt, const void* psi0_dev, void* lam_dev, double* grad) {
  if (!ctx) return PDEOPT_EINVAL;
  if (!ctx->configured) return fail(ctx, PDEOPT_ESTATE, "pdeopt_configure has not been called");
  const pdeopt_problem& p = ctx->prob;
  if (p.equation != PDEOPT_EQ_GPE) return fail(ctx, PDEOPT_EINVAL, "the adjoint of the Strang step needs the GPE");
  if (ctx->n_spots < 1)
    return fail(ctx, PDEOPT_ESTATE, "the adjoint of the Strang step differentiates Gaussian spots: pdeopt_set_gpe_spots has set none");
  if (!ctx->aux[PDEOPT_AUX_GPE_A_TERM].dev) return fail(ctx, PDEOPT_ESTATE, "Strang splitting needs the GPE_A_TERM aux field");
  if (ctx->aux[PDEOPT_AUX_GPE_A_TERM].per_env)
    return fail(ctx, PDEOPT_EINVAL, "the adjoint of the Strang step needs one A_term shared by the batch");
  if (has_time_aux(ctx, PDEOPT_AUX_GPE_POTENTIAL))
    return fail(ctx, PDEOPT_EINVAL, "a potential registered through pdeopt_set_aux_time_fn is a host callable: it has no parameters "
                                    "to differentiate (give the control as spots)");
  if (!(dt > 0)) return fail(ctx, PDEOPT_EINVAL, "dt = %g", dt);
  if (!psi0_dev || !lam_dev || !grad || (uintptr_t)psi0_dev % ctx->esize || (uintptr_t)lam_dev % ctx->esize || (uintptr_t)grad % 8)
    return fail(ctx, PDEOPT_EINVAL, "psi0_dev / lam_dev are device fields [batch][nx][ny][2] in the problem dtype, grad is "
                                    "[batch][n_spots][7] doubles, all aligned to their type");
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  // grad: device memory is added into by the kernel; anything else is host memory, staged through a device block
  hipPointerAttribute_t attr{};
  bool grad_on_device = false;
  if (hipPointerGetAttributes(&attr, grad) == hipSuccess) grad_on_device = attr.type == hipMemoryTypeDevice;
  else (void)hipGetLastError();  // an unregistered host pointer: not an error of the ctx
  const size_t gbytes = sizeof(double) * (size_t)p.batch * ctx->n_spots * 7;
  const auto overlap = [](const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
  };
  if (overlap(lam_dev, ctx->total_bytes, psi0_dev, ctx->total_bytes) ||
      (grad_on_device && (overlap(grad, gbytes, lam_dev, ctx->total_bytes) || overlap(grad, gbytes, psi0_dev, ctx->total_bytes))))
    return fail(ctx, PDEOPT_EINVAL, "lam_dev and grad are written: they must not overlap each other or psi0_dev");
  GpeAdjoint& ga = ctx->features.ensure<GpeAdjoint>(FS_GPE_ADJOINT);
  int rc;
  if ((rc = ensure_buffer(ctx, ga.work, ctx->total_bytes))) return rc;
  if ((rc = ensure_buffer(ctx, ga.direct, ctx->total_bytes))) return rc;
  if ((rc = ensure_buffer(ctx, ga.part, sizeof(double) * (size_t)p.batch * kBlocks * 2))) return rc;
  if ((rc = ensure_buffer(ctx, ga.spart, sizeof(double) * (size_t)p.batch * kBlocks * kSpotSums))) return rc;
  if ((rc = ensure_buffer(ctx, ga.gacc, sizeof(double) * (size_t)p.batch * PDEOPT_MAX_SPOTS * 7))) return rc;
  double* gdev = grad;
  if (!grad_on_device) {
    gdev = ga.gacc.as<double>();
    PDEOPT_HIP_CHECK(ctx, hipMemsetAsync(gdev, 0, gbytes, ctx->stream));
  }
  rc = with_dtype(ctx, [&](auto t) { return adjoint_step_t<decltype(t)>(ctx, t0, dt, psi0_dev, lam_dev, gdev); });
  if (rc) return rc;
  if (!grad_on_device) {
    std::vector<double> h(gbytes / sizeof(double));
    PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(h.data(), gdev, gbytes, hipMemcpyDeviceToHost, ctx->stream));
    PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < h.size(); ++i) grad[i] += h[i];
  }
  ctx->last_kernel = "strang_adjoint_rocfft_c2c";
  return PDEOPT_OK;
}

}  // extern "C"
