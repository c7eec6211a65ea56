// One substep of the discrete adjoint of the stirred, ramped rotating-frame split step (gpe_rot_stir.hip, DESIGN.md
// section 4.13): the adjoint of gpe_rot_adjoint.hip (section 4.12) with Gaussian light spots in the potential and
// Omega(t) = omega + rate t in the line operators, and with it the gradient over the rate and over the seven numbers of
// every spot.
//
// Forward substep starting at local time t0, s = tau / 2, tau = dt * time_scale, h^2 = strang_dx^2:
//   Omega0 = omega + rate t0 (one fused multiply-add, rot_omega_at: the forward step's number) in all four operators
//   w = V + spots(t0, x, y) + k |psi0|^2
//   u1 = Lx psi0;  a = Ly u1;  c = a exp(-i w tau);  n = sqrt(h^2 sum |c|^2);  d = c / n;  psi1 = Lx Ly d
// The cotangent chain is that of gpe_rot_adjoint.hip:1-19 with Omega0 in the factors and the spots in w.  With
// g_w = Re(conj(-i tau c) lambda_c) and S_Omega the four operator sums (S3, S4 divided by n):
//   dJ/domega += S_Omega;  dJ/drate += t0 S_Omega
//   dJ/d(amp0, x0, y0, inv_two_w2) of spot s += sum over cells of g_w spot_partials(s)[0 .. 3]   (w enters, sign +)
//   dJ/d(amp_rate, x_rate, y_rate) of spot s += t0 x (the sums of amp0, x0, y0);  dJ/dk, dJ/de as before.
//
// The schedule is gpe_rot_adjoint.hip:21-37's: the primal first, keeping S1 .. S3; 15 batched 1-D transforms on the
// library's rocFFT plans, 1 copy and 11 passes over the field.  The kernels are this file's own (rsadj_), so those of
// gpe_rot_adjoint.hip keep their instructions and a frozen problem its bits there.  Every reduction is in gather form
// (gpe_rot_adjoint_sums.hpp): the partial block of a workgroup has 8 + 4 PDEOPT_MAX_SPOTS slots.
#include <algorithm>
#include <cmath>
#include <complex>

#include "common.hpp"
#include "gpe_rot_adjoint_sums.hpp"
#include "gpe_rot_line.hpp"

namespace pdeopt {

struct GpeRotStirAdjoint {
  void* work = nullptr;   // the running primal field, at the end S4     [batch][nx][ny] complex
  void* cbuf = nullptr;   // c, then the direct term 2 k g_w psi0         same
  void* spec[3] = {nullptr, nullptr, nullptr};  // S1, S2, S3              same
  void* kin_x = nullptr;  // exp(tau/2 0.5j (2 pi i kx)^2) / nx, complex [nx]
  void* kin_y = nullptr;
  double* part = nullptr; // [batch][kRadjBlocks][kSlots]
  double* gacc = nullptr; // [batch][4]: staging of a host gradient block
  double* sacc = nullptr; // [batch][PDEOPT_MAX_SPOTS][7]: staging of a host spot block
  double key_dt = NAN, key_tr = NAN, key_ti = NAN, key_hx = NAN, key_hy = NAN;
  bool valid = false;
};

namespace {

constexpr int kBlocks = kRadjBlocks;
constexpr int kSpotSums = 4 * PDEOPT_MAX_SPOTS;  // independent sums per environment (spot_partials)
// the sums of one environment: those of gpe_rot_adjoint.hip, then 4 per spot
enum { kNorm = 0, kSigma = 1, kGradK = 2, kGradE = 3, kOmega1 = 4, kOmega2 = 5, kOmega3 = 6, kOmega4 = 7, kSpot0 = 8,
       kSlots = kSpot0 + kSpotSums };

__device__ __forceinline__ double rsadj_total(const double* part, int b, int slot, int lane) {
  return radj_slot_total(part, kSlots, b, slot, lane);
}

// The primal's multiply at Omega0 = Omega(t0): buf[b][ix][iy] *= kin[k] * rotation factor, the product kept in `save`
// too (nullptr: not).  The line coefficient is formed as rstir_mul_kernel forms it: Omega0 * (w * coord).
template <typename T, int AXIS>
__global__ __launch_bounds__(256) void rsadj_mul_kernel(Cx<T>* __restrict__ buf, Cx<T>* __restrict__ save,
                                                        const Cx<T>* __restrict__ kin, const EnvParams<T>* __restrict__ ep,
                                                        const RotAxis<T> ax, int nx, int ny, T t0) {
  const int b = blockIdx.y;
  const int64_t cells = (int64_t)nx * ny, o = (int64_t)b * cells;
  const T om = rot_omega_at(ep[b], t0);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (int64_t)gridDim.x * 256) {
    const int ix = (int)(i / ny), iy = (int)(i - (int64_t)ix * ny);
    const int k = AXIS == 0 ? ix : iy, n = AXIS == 0 ? nx : ny, line = AXIS == 0 ? iy : ix;
    const Cx<T> m = rot_mult<T>(kin[k], om * (ax.w * (ax.c_first + T(line) * ax.c_step)), k, n, ax.sr, ax.si);
    const Cx<T> r = cmul(buf[o + i], m);
    buf[o + i] = r;
    if (save) save[o + i] = r;
  }
}

// The cotangent's multiply at Omega0: lam^ *= conj(kin[k] * rotation factor), and beside it the Omega sum of this
// operator (radj_conj_mul_kernel), part[b][block][slot];  SIGMA: part[b][block][kSigma] = sum Re(conj(prim) lam^).
template <typename T, int AXIS, bool SIGMA>
__global__ __launch_bounds__(256) void rsadj_conj_mul_kernel(Cx<T>* __restrict__ lam, const Cx<T>* __restrict__ prim,
                                                             const Cx<T>* __restrict__ kin,
                                                             const EnvParams<T>* __restrict__ ep, const RotAxis<T> ax,
                                                             int nx, int ny, double* __restrict__ part, int slot, T t0) {
  __shared__ double sh[4];
  const int b = blockIdx.y;
  const int64_t cells = (int64_t)nx * ny, o = (int64_t)b * cells;
  const T om = rot_omega_at(ep[b], t0);
  double acc_o = 0.0, acc_s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (int64_t)gridDim.x * 256) {
    const int ix = (int)(i / ny), iy = (int)(i - (int64_t)ix * ny);
    const int k = AXIS == 0 ? ix : iy, n = AXIS == 0 ? nx : ny, line = AXIS == 0 ? iy : ix;
    const T wc = ax.w * (ax.c_first + T(line) * ax.c_step);
    const Cx<T> m = rot_mult<T>(kin[k], om * wc, k, n, ax.sr, ax.si);  // the primal's factor, bit for bit
    const Cx<T> l = lam[o + i], v = prim[o + i];
    const int ks = k < (n + 1) / 2 ? k : k - n;
    // (sr + i si) i v = (-si v.re - sr v.im) + i (sr v.re - si v.im)
    const T zr = -ax.si * v.re - ax.sr * v.im, zi = ax.sr * v.re - ax.si * v.im;
    acc_o += (double)(wc * T(ks)) * ((double)l.re * (double)zr + (double)l.im * (double)zi);
    if (SIGMA) acc_s += (double)v.re * (double)l.re + (double)v.im * (double)l.im;
    lam[o + i] = cmul(l, Cx<T>{m.re, -m.im});
  }
  double* out = part + ((int64_t)b * kBlocks + blockIdx.x) * kSlots;
  const double so = radj_block_sum(acc_o, sh);
  if (threadIdx.x == 0) out[slot] = so;
  if (SIGMA) {
    const double ss = radj_block_sum(acc_s, sh);
    if (threadIdx.x == 0) out[kSigma] = ss;
  }
}

template <typename T>
struct RsadjArgs {
  Cx<T>* work;            // recompute: a in, c out
  Cx<T>* cbuf;            // recompute: c out; pointwise: c in, the direct term out
  const Cx<T>* psi0;
  Cx<T>* lam;             // pointwise: lambda_d in, lambda_a out
  const T* pot;           // trap potential, nullptr: none
  int64_t pot_stride;     // elements between environments (0: shared)
  const EnvParams<T>* ep;
  T tr, ti;               // tau
  T x_first, y_first, hx, hy;
  int64_t cells;
  int ny;
  double h2;
  double* part;
  SpotArgs<T> spots;      // the spots at t0 (spots.n == 0: none)
};

// exp(-i w tau), w = V + spots(t0) + k |psi0|^2 at cell (x, y): the expression of rstir_b_kernel
template <typename T>
__device__ __forceinline__ Cx<T> rsadj_phase(const RsadjArgs<T>& a, int env, int64_t i, T x, T y, Cx<T> p0, T kk) {
  T w = a.pot ? a.pot[(int64_t)env * a.pot_stride + i] : T(0);
  if (a.spots.n) w += spots_value<T>(a.spots, env, x, y);
  w += kk * (p0.re * p0.re + p0.im * p0.im);
  T sn, cs;
  sincos_t<T>(w * a.tr, &sn, &cs);
  const T mag = (a.ti == T(0)) ? T(1) : exp_t<T>(w * a.ti);
  return Cx<T>{mag * cs, -mag * sn};
}

// work: a -> c = a exp(-i w tau), cbuf = c;  part[b][block][kNorm] = sum |c|^2
template <typename T>
__global__ __launch_bounds__(256) void rsadj_recompute_kernel(const RsadjArgs<T> a) {
  __shared__ double sh[4];
  const int b = blockIdx.y;
  const int64_t o = (int64_t)b * a.cells;
  const T kk = a.ep[b].gpe_k;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.cells; i += (int64_t)gridDim.x * 256) {
    const int ix = (int)(i / a.ny), iy = (int)(i - (int64_t)ix * a.ny);
    const T x = a.spots.x_first + T(ix) * a.spots.hx, y = a.spots.y_first + T(iy) * a.spots.hy;
    const Cx<T> c = cmul(a.work[o + i], rsadj_phase<T>(a, b, i, x, y, a.psi0[o + i], kk));
    a.work[o + i] = c;
    a.cbuf[o + i] = c;
    acc += (double)c.re * (double)c.re + (double)c.im * (double)c.im;
  }
  const double s = radj_block_sum(acc, sh);
  if (threadIdx.x == 0) a.part[((int64_t)b * kBlocks + blockIdx.x) * kSlots + kNorm] = s;
}

// lam: lambda_d -> lambda_a;  cbuf: c -> 2 k g_w psi0;  part[b][block][kGradK, kGradE] = sum g_w |psi0|^2,
// g_w (x^2 - y^2) / 2;  part[b][block][kSpot0 + 4 s + q] = sum g_w x partial q of spot s
template <typename T>
__global__ __launch_bounds__(256) void rsadj_pointwise_kernel(const RsadjArgs<T> a) {
  __shared__ double sh[4];
  __shared__ double tot[2];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t o = (int64_t)b * a.cells;
  if (tid < 64) {  // the two sums of this environment, every workgroup in the same order
    const double sn = rsadj_total(a.part, b, kNorm, tid), ss = rsadj_total(a.part, b, kSigma, tid);
    if (tid == 0) {
      tot[0] = sn;
      tot[1] = ss;
    }
  }
  __syncthreads();
  const double nrm = sqrt(tot[0] * a.h2);
  const T inv_n = (T)(1.0 / nrm);
  const T s_over_n = (T)(a.h2 * tot[1] / (nrm * nrm));  // sigma / n, sigma = h^2 sum Re(conj(c) lambda_d) / n
  const T kk = a.ep[b].gpe_k;
  const int ns = a.spots.n;
  double acc_k = 0.0, acc_e = 0.0;
  double acc[kSpotSums];
#pragma unroll
  for (int q = 0; q < kSpotSums; ++q) acc[q] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < a.cells; i += (int64_t)gridDim.x * 256) {
    const int ix = (int)(i / a.ny), iy = (int)(i - (int64_t)ix * a.ny);
    const T xs = a.spots.x_first + T(ix) * a.spots.hx, ys = a.spots.y_first + T(iy) * a.spots.hy;
    const Cx<T> p0 = a.psi0[o + i];
    const Cx<T> e = rsadj_phase<T>(a, b, i, xs, ys, p0, kk);
    const Cx<T> c = a.cbuf[o + i], ld = a.lam[o + i];
    // lambda_c = (lambda_d - sigma d) / n, d = c / n
    const Cx<T> lc{(ld.re - s_over_n * c.re) * inv_n, (ld.im - s_over_n * c.im) * inv_n};
    // lambda_a = lambda_c conj(e)
    a.lam[o + i] = cmul(lc, Cx<T>{e.re, -e.im});
    // g_w = Re(conj(-i tau c) lambda_c), -i tau = ti - i tr
    const T zr = a.ti * c.re + a.tr * c.im, zi = a.ti * c.im - a.tr * c.re;
    const T gw = zr * lc.re + zi * lc.im;
    const T f = T(2) * kk * gw;
    a.cbuf[o + i] = Cx<T>{f * p0.re, f * p0.im};
    const T x = a.x_first + T(ix) * a.hx, y = a.y_first + T(iy) * a.hy;
    acc_k += (double)gw * (double)(p0.re * p0.re + p0.im * p0.im);
    acc_e += (double)gw * (double)(T(0.5) * (x * x - y * y));
#pragma unroll
    for (int s = 0; s < PDEOPT_MAX_SPOTS; ++s) {
      if (s < ns) {
        T d[4];
        spot_partials<T>(a.spots, b, s, xs, ys, d);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[4 * s + q] += (double)gw * (double)d[q];
      }
    }
  }
  double* out = a.part + ((int64_t)b * kBlocks + blockIdx.x) * kSlots;
  const double sk = radj_block_sum(acc_k, sh);
  if (tid == 0) out[kGradK] = sk;
  const double se = radj_block_sum(acc_e, sh);
  if (tid == 0) out[kGradE] = se;
#pragma unroll
  for (int q = 0; q < kSpotSums; ++q) {
    if (q < 4 * ns) {  // uniform over the workgroup
      const double v = radj_block_sum(acc[q], sh);
      if (tid == 0) out[kSpot0 + q] = v;
    }
  }
}

// lam += direct;  workgroup 0 of every environment: grad[b][0 .. 3] += (k, e, S_Omega, t0 S_Omega) and
// spot_grad[b][s][0 .. 6] += the spot sums (rates: t0 x their value's sum), the sums over the fixed partition
template <typename T>
__global__ __launch_bounds__(256) void rsadj_finish_kernel(Cx<T>* __restrict__ lam, const Cx<T>* __restrict__ direct,
                                                           int64_t cells, const double* __restrict__ part,
                                                           double* __restrict__ grad, double* __restrict__ spot_grad,
                                                           int n_spots, double h2, double t0) {
  const int b = blockIdx.y;
  const int64_t o = (int64_t)b * cells;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (int64_t)gridDim.x * 256) {
    const Cx<T> d = direct[o + i];
    Cx<T> l = lam[o + i];
    l.re += d.re;
    l.im += d.im;
    lam[o + i] = l;
  }
  if (blockIdx.x == 0 && threadIdx.x < 64) {  // one wave, uniform control flow around the shuffles
    const int lane = threadIdx.x;
    const double sn = rsadj_total(part, b, kNorm, lane);
    const double gk = rsadj_total(part, b, kGradK, lane), ge = rsadj_total(part, b, kGradE, lane);
    const double o1 = rsadj_total(part, b, kOmega1, lane), o2 = rsadj_total(part, b, kOmega2, lane);
    const double o3 = rsadj_total(part, b, kOmega3, lane), o4 = rsadj_total(part, b, kOmega4, lane);
    if (lane == 0) {
      double* g = grad + (int64_t)b * 4;
      const double s_omega = (o1 + o2) + (o3 + o4) / sqrt(sn * h2);  // S3, S4 are the spectra of c = n d
      g[0] += gk;
      g[1] += ge;
      g[2] += s_omega;
      g[3] += t0 * s_omega;
    }
    for (int sq = 0; sq < 4 * n_spots; ++sq) {  // uniform over the wave
      const double v = rsadj_total(part, b, kSpot0 + sq, lane);
      if (lane == 0) {
        const int s = sq >> 2, q = sq & 3;
        double* g = spot_grad + ((int64_t)b * n_spots + s) * 7;  // amp0, amp_rate, x0, x_rate, y0, y_rate, inv_two_w2
        if (q == 3) {
          g[6] += v;
        } else {
          g[2 * q] += v;
          g[2 * q + 1] += t0 * v;
        }
      }
    }
  }
}

template <typename T>
int ensure_tables(pdeopt_ctx* ctx, GpeRotStirAdjoint& ra, double dt) {
  const pdeopt_problem& p = ctx->prob;
  if (ra.valid && ra.key_dt == dt && ra.key_tr == ctx->ts_re && ra.key_ti == ctx->ts_im && ra.key_hx == p.hx && ra.key_hy == p.hy)
    return PDEOPT_OK;
  const std::complex<double> half_tau = 0.5 * dt * std::complex<double>(ctx->ts_re, ctx->ts_im);
  int rc;
  if ((rc = upload_kinetic<T>(ctx, &ra.kin_x, p.nx, p.hx, half_tau))) return rc;
  if ((rc = upload_kinetic<T>(ctx, &ra.kin_y, p.ny, p.hy, half_tau))) return rc;
  ra.valid = true;
  ra.key_dt = dt;
  ra.key_tr = ctx->ts_re;
  ra.key_ti = ctx->ts_im;
  ra.key_hx = p.hx;
  ra.key_hy = p.hy;
  return PDEOPT_OK;
}

template <typename T>
int rot_stir_adjoint_step_t(pdeopt_ctx* ctx, double t0, double dt, const void* psi0, void* lam_dev, double* grad_dev,
                            double* spot_grad_dev) {
  GpeRotStirAdjoint& ra = *ctx->gpe_rot_stir_adjoint;
  const pdeopt_problem& p = ctx->prob;
  const int64_t cells = (int64_t)p.nx * p.ny;
  int rc = ensure_tables<T>(ctx, ra, dt);
  if (rc) return rc;
  const std::complex<double> tau = dt * std::complex<double>(ctx->ts_re, ctx->ts_im);
  const dim3 mgrid((unsigned)std::min<int64_t>(4096, (cells + 255) / 256), p.batch), rgrid(kBlocks, p.batch), blk(256);
  const EnvParams<T>* ep = env_params<T>(ctx, 0);
  const RotAxis<T> axes[2] = {rot_axis<T>(ctx, 0, 0.5 * tau), rot_axis<T>(ctx, 1, 0.5 * tau)};
  const Cx<T>* const kin[2] = {(const Cx<T>*)ra.kin_x, (const Cx<T>*)ra.kin_y};
  const AuxField& pot = ctx->aux[PDEOPT_AUX_GPE_POTENTIAL];
  Cx<T>* const work = (Cx<T>*)ra.work;
  Cx<T>* const lam = (Cx<T>*)lam_dev;
  const T t = (T)t0;
  RsadjArgs<T> a{};
  a.work = work;
  a.cbuf = (Cx<T>*)ra.cbuf;
  a.psi0 = (const Cx<T>*)psi0;
  a.lam = lam;
  a.pot = (const T*)pot.dev;
  a.pot_stride = pot.per_env ? cells : 0;
  a.ep = ep;
  a.tr = (T)tau.real();
  a.ti = (T)tau.imag();
  a.x_first = (T)ctx->rot_x_first;
  a.y_first = (T)ctx->rot_y_first;
  a.hx = (T)p.hx;
  a.hy = (T)p.hy;
  a.cells = cells;
  a.ny = p.ny;
  a.h2 = ctx->strang_dx * ctx->strang_dx;
  a.part = ra.part;
  a.spots = make_spot_args<T>(ctx, 0, t0);
  // primal: transform along `axis`, multiply (the spectrum kept in `save`), and back unless it is the last one
  auto primal_op = [&](int axis, Cx<T>* save, bool back) -> int {
    int r = spectral_c2c_axis(ctx, axis, true, work);
    if (r) return r;
    if (axis == 0)
      hipLaunchKernelGGL((rsadj_mul_kernel<T, 0>), mgrid, blk, 0, ctx->stream, work, save, kin[0], ep, axes[0], p.nx, p.ny, t);
    else
      hipLaunchKernelGGL((rsadj_mul_kernel<T, 1>), mgrid, blk, 0, ctx->stream, work, save, kin[1], ep, axes[1], p.nx, p.ny, t);
    return back ? spectral_c2c_axis(ctx, axis, false, work) : PDEOPT_OK;
  };
  // cotangent: lam <- L^H lam of the operator whose multiplied primal spectrum is `prim`, its Omega sum into `slot`
  auto cotangent_op = [&](int axis, const Cx<T>* prim, int slot) -> int {
    int r = spectral_c2c_axis(ctx, axis, true, lam);
    if (r) return r;
    if (axis == 0)
      hipLaunchKernelGGL((rsadj_conj_mul_kernel<T, 0, false>), rgrid, blk, 0, ctx->stream, lam, prim, kin[0], ep, axes[0],
                         p.nx, p.ny, ra.part, slot, t);
    else if (slot == kOmega3)
      hipLaunchKernelGGL((rsadj_conj_mul_kernel<T, 1, true>), rgrid, blk, 0, ctx->stream, lam, prim, kin[1], ep, axes[1],
                         p.nx, p.ny, ra.part, slot, t);
    else
      hipLaunchKernelGGL((rsadj_conj_mul_kernel<T, 1, false>), rgrid, blk, 0, ctx->stream, lam, prim, kin[1], ep, axes[1],
                         p.nx, p.ny, ra.part, slot, t);
    return spectral_c2c_axis(ctx, axis, false, lam);
  };
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(work, psi0, ctx->total_bytes, hipMemcpyDeviceToDevice, ctx->stream));
  if ((rc = primal_op(0, (Cx<T>*)ra.spec[0], true))) return rc;   // u1
  if ((rc = primal_op(1, (Cx<T>*)ra.spec[1], true))) return rc;   // a
  hipLaunchKernelGGL(rsadj_recompute_kernel<T>, rgrid, blk, 0, ctx->stream, a);
  if ((rc = primal_op(1, (Cx<T>*)ra.spec[2], true))) return rc;   // n e1
  if ((rc = primal_op(0, nullptr, false))) return rc;             // work = S4
  if ((rc = cotangent_op(0, work, kOmega4))) return rc;                        // mu1
  if ((rc = cotangent_op(1, (const Cx<T>*)ra.spec[2], kOmega3))) return rc;    // lambda_d, the raw sigma
  hipLaunchKernelGGL(rsadj_pointwise_kernel<T>, rgrid, blk, 0, ctx->stream, a);
  if ((rc = cotangent_op(1, (const Cx<T>*)ra.spec[1], kOmega2))) return rc;    // nu
  if ((rc = cotangent_op(0, (const Cx<T>*)ra.spec[0], kOmega1))) return rc;    // Lx^H nu
  hipLaunchKernelGGL(rsadj_finish_kernel<T>, rgrid, blk, 0, ctx->stream, lam, (const Cx<T>*)ra.cbuf, cells,
                     (const double*)ra.part, grad_dev, spot_grad_dev, ctx->n_spots, a.h2, t0);
  ctx->n_stage_launches += 26;  // 15 transforms, 8 multiplies, 3 passes
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  return PDEOPT_OK;
}

}  // namespace

void gpe_rot_stir_adjoint_invalidate(pdeopt_ctx* ctx) {
  if (ctx->gpe_rot_stir_adjoint) ctx->gpe_rot_stir_adjoint->valid = false;
}

void gpe_rot_stir_adjoint_destroy(pdeopt_ctx* ctx) {
  GpeRotStirAdjoint* ra = ctx->gpe_rot_stir_adjoint;
  if (!ra) return;
  void* bufs[] = {ra->work, ra->cbuf, ra->spec[0], ra->spec[1], ra->spec[2], ra->kin_x, ra->kin_y, ra->part, ra->gacc, ra->sacc};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  delete ra;
  ctx->gpe_rot_stir_adjoint = nullptr;
}

}  // namespace pdeopt

using namespace pdeopt;

extern "C" {

int pdeopt_gpe_rot_stir_adjoint_step(pdeopt_ctx* ctx, double t0, double dt, const void* psi0_dev, void* lam_dev, double* grad,
                                     double* spot_grad) {
  if (!ctx) return PDEOPT_EINVAL;
  if (!ctx->configured) return fail(ctx, PDEOPT_ESTATE, "pdeopt_configure has not been called");
  const pdeopt_problem& p = ctx->prob;
  if (p.equation != PDEOPT_EQ_GPE)
    return fail(ctx, PDEOPT_EINVAL, "the adjoint of the stirred rotating-frame split step needs the GPE");
  if (!ctx->rot_set)
    return fail(ctx, PDEOPT_ESTATE, "the adjoint of the stirred rotating-frame split step needs pdeopt_set_gpe_rotation (Omega "
                                    "and the mesh origin)");
  if (has_time_aux(ctx, PDEOPT_AUX_GPE_POTENTIAL))
    return fail(ctx, PDEOPT_EINVAL, "a potential registered through pdeopt_set_aux_time_fn is a host callable: the "
                                    "rotating-frame split step takes a static potential and Gaussian spots");
  if (ctx->n_spots && !spot_grad)
    return fail(ctx, PDEOPT_EINVAL, "%d light spots are set: spot_grad is their gradient block [batch][n_spots][7], not NULL",
                ctx->n_spots);
  if (!ctx->n_spots && spot_grad)
    return fail(ctx, PDEOPT_EINVAL, "no light spots are set (pdeopt_set_gpe_spots): spot_grad must be NULL");
  if (!(dt > 0)) return fail(ctx, PDEOPT_EINVAL, "dt = %g", dt);
  if (!std::isfinite(t0)) return fail(ctx, PDEOPT_EINVAL, "t0 = %g", t0);
  if (!psi0_dev || !lam_dev || !grad || (uintptr_t)psi0_dev % ctx->esize || (uintptr_t)lam_dev % ctx->esize ||
      (uintptr_t)grad % 8 || (uintptr_t)spot_grad % 8)
    return fail(ctx, PDEOPT_EINVAL, "psi0_dev / lam_dev are device fields [batch][nx][ny][2] in the problem dtype, grad is "
                                    "[batch][4] doubles, spot_grad [batch][n_spots][7] doubles, all aligned to their type");
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  // grad, spot_grad: device memory is added into by the kernel; anything else is host memory, staged through a device block
  const auto on_device = [](const void* ptr) {
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, ptr) == hipSuccess) return attr.type == hipMemoryTypeDevice;
    (void)hipGetLastError();  // an unregistered host pointer: not an error of the ctx
    return false;
  };
  const bool grad_on_device = on_device(grad);
  if (spot_grad && on_device(spot_grad) != grad_on_device)
    return fail(ctx, PDEOPT_EINVAL, "grad and spot_grad are both device memory or both host memory");
  const size_t gbytes = sizeof(double) * (size_t)p.batch * 4;
  const size_t sbytes = sizeof(double) * (size_t)p.batch * ctx->n_spots * 7;
  const auto overlap = [](const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
  };
  bool bad = overlap(lam_dev, ctx->total_bytes, psi0_dev, ctx->total_bytes);
  if (spot_grad) bad = bad || overlap(grad, gbytes, spot_grad, sbytes);
  if (grad_on_device) {
    bad = bad || overlap(grad, gbytes, lam_dev, ctx->total_bytes) || overlap(grad, gbytes, psi0_dev, ctx->total_bytes);
    if (spot_grad)
      bad = bad || overlap(spot_grad, sbytes, lam_dev, ctx->total_bytes) || overlap(spot_grad, sbytes, psi0_dev, ctx->total_bytes);
  }
  if (bad)
    return fail(ctx, PDEOPT_EINVAL, "lam_dev, grad and spot_grad are written: they must not overlap each other or psi0_dev");
  if (!ctx->gpe_rot_stir_adjoint) ctx->gpe_rot_stir_adjoint = new GpeRotStirAdjoint();
  GpeRotStirAdjoint& ra = *ctx->gpe_rot_stir_adjoint;
  int rc;
  if ((rc = ensure_buffer(ctx, &ra.work, ctx->total_bytes))) return rc;
  if ((rc = ensure_buffer(ctx, &ra.cbuf, ctx->total_bytes))) return rc;
  for (void*& s : ra.spec)
    if ((rc = ensure_buffer(ctx, &s, ctx->total_bytes))) return rc;
  if ((rc = ensure_buffer(ctx, (void**)&ra.part, sizeof(double) * (size_t)p.batch * kBlocks * kSlots))) return rc;
  if ((rc = ensure_buffer(ctx, (void**)&ra.gacc, gbytes))) return rc;
  if ((rc = ensure_buffer(ctx, (void**)&ra.sacc, sizeof(double) * (size_t)p.batch * PDEOPT_MAX_SPOTS * 7))) return rc;
  double *gdev = grad, *sdev = spot_grad;
  if (!grad_on_device) {
    gdev = ra.gacc;
    PDEOPT_HIP_CHECK(ctx, hipMemsetAsync(gdev, 0, gbytes, ctx->stream));
    if (spot_grad) {
      sdev = ra.sacc;
      PDEOPT_HIP_CHECK(ctx, hipMemsetAsync(sdev, 0, sbytes, ctx->stream));
    }
  }
  rc = with_dtype(ctx, [&](auto t) { return rot_stir_adjoint_step_t<decltype(t)>(ctx, t0, dt, psi0_dev, lam_dev, gdev, sdev); });
  if (rc) return rc;
  if (!grad_on_device) {
    std::vector<double> hg(gbytes / sizeof(double)), hs(sbytes / sizeof(double));
    PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(hg.data(), gdev, gbytes, hipMemcpyDeviceToHost, ctx->stream));
    if (spot_grad) PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(hs.data(), sdev, sbytes, hipMemcpyDeviceToHost, ctx->stream));
    PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < hg.size(); ++i) grad[i] += hg[i];
    if (spot_grad)
      for (size_t i = 0; i < hs.size(); ++i) spot_grad[i] += hs[i];
  }
  ctx->last_kernel = "strang_rot_stir_adjoint_rocfft_1d";
  return PDEOPT_OK;
}

}  // extern "C"
