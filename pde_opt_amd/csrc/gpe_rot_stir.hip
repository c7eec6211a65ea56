// The rotating-frame split step (gpe_rot.hip) with a potential and a rotation frequency that
// change from step to step: Gaussian light spots (pdeopt_set_gpe_spots) evaluated in the row
// pass, and Omega(t) = Omega + rate t (pdeopt_set_env_gpe_omega_rate) in the line operators.
//
// The step starting at local time t_s = t0 + s dt uses Omega(t_s) in all four of its line operators and
// V(t_s) = potential + spots(t_s, x, y) in b (the convention of the non-rotating Strang step: b at the substep's start):
//   col FIRST : |psi0|^2 -> Lx(tau/2; Omega(t_s))
//   row       : Ly(tau/2; Omega(t_s)) -> * exp(b tau) with the spots at t_s, partial sums -> Ly(tau/2; Omega(t_s))
//   col JOIN  : Lx(tau/2; Omega(t_s)) * scale -> |psi|^2 -> Lx(tau/2; Omega(t_s+1))     (col LAST: the first half only)
// The JOIN pass is the one place where two steps meet: its two halves take their own local time and form their own
// line coefficient.  Nothing is added to the passes over the field; the kernels are launched only when there are spots
// or some environment has a nonzero rate (advance_strang_rot), so a frozen problem keeps the kernels of gpe_rot.hip
// and their bits.
#include <algorithm>
#include <cmath>
#include <complex>

#include "common.hpp"
#include "groups.hpp"
#include "fft_lds.hpp"
#include "fft_reg.hpp"
#include "split_step_util.hpp"
#include "gpe_rot_line.hpp"
#include "gpe_rot_step.hpp"

namespace pdeopt {

namespace {

// Omega(t) of an environment: rot_omega_at (gpe_rot_line.hpp), shared with the adjoint

// The row pass of gpe_rot.hip with Omega(t) and the spots at t (sa.t) in b.
template <typename T, int N>
__global__ __launch_bounds__(256) void rstir_row_kernel(Cx<T>* __restrict__ psi, const T* __restrict__ dens,
                                                        const T* __restrict__ pot, int64_t pot_env_stride,
                                                        const EnvParams<T>* __restrict__ ep,
                                                        const Cx<T>* __restrict__ tw, const Cx<T>* __restrict__ kin,
                                                        T tr, T ti, const RotAxis<T> ax, int nx,
                                                        double* __restrict__ partial, const SpotArgs<T> sa) {
  using E = RegFft<T, N>;
  constexpr int PTS = E::kPts, TT = E::TT, F = 256 / TT, NP = E::NP;
  static_assert(E::kWaveLocal, "a line lives in one wave");
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int tid = threadIdx.x;
  const int f = tid / TT, j = tid - f * TT;
  Cx<T>* const seq = reinterpret_cast<Cx<T>*>(smem_raw) + f * NP;
  const int64_t row = (int64_t)blockIdx.x * F + f;
  const int env = (int)(row / nx);
  const int ix = (int)(row - (int64_t)env * nx);
  Cx<T>* const g = psi + row * N;
  const T a = ax.w * rot_omega_at(ep[env], sa.t) * (ax.c_first + T(ix) * ax.c_step);
  Cx<T> v[PTS];
#pragma unroll
  for (int m = 0; m < PTS; ++m) v[m] = g[E::natural(j, m)];
  E::template dif<-1>(v, seq, tw, j);
#pragma unroll
  for (int sl = 0; sl < PTS; ++sl) {
    const int fr = E::freq(j, sl);
    v[sl] = cmul(v[sl], rot_mult<T>(kin[fr], a, fr, N, ax.sr, ax.si));
    if constexpr (kOneFactorAtATime<T, PTS>) __builtin_amdgcn_sched_barrier(0);
  }
  E::template dit<+1>(v, seq, tw, j);
  // psi2 = psi1 exp(b tau), b = -i (V + spots(t) + k |psi0|^2)
  const T kk = ep[env].gpe_k;
  const T* const vrow = pot ? pot + (int64_t)env * pot_env_stride + (int64_t)ix * N : nullptr;
  const T xs = sa.x_first + T(ix) * sa.hx;
  T accp = T(0);
#pragma unroll
  for (int m = 0; m < PTS; ++m) {
    const int n = E::natural(j, m);
    T w = vrow ? vrow[n] : T(0);
    if (sa.n) w += spots_value<T>(sa, env, xs, sa.y_first + T(n) * sa.hy);
    w += kk * dens[row * N + n];
    T sn, cs;
    sincos_t<T>(w * tr, &sn, &cs);
    const T mag = (ti == T(0)) ? T(1) : exp_t<T>(w * ti);
    v[m] = cmul(v[m], Cx<T>{mag * cs, -mag * sn});
    accp += v[m].re * v[m].re + v[m].im * v[m].im;
    if constexpr (kOneFactorAtATime<T, PTS>) __builtin_amdgcn_sched_barrier(0);
  }
  double acc = (double)accp;
  __shared__ double red[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
  E::template dif<-1>(v, seq, tw, j);
#pragma unroll
  for (int sl = 0; sl < PTS; ++sl) {
    const int fr = E::freq(j, sl);
    v[sl] = cmul(v[sl], rot_mult<T>(kin[fr], a, fr, N, ax.sr, ax.si));
    if constexpr (kOneFactorAtATime<T, PTS>) __builtin_amdgcn_sched_barrier(0);
  }
  E::template dit<+1>(v, seq, tw, j);
#pragma unroll
  for (int m = 0; m < PTS; ++m) g[E::natural(j, m)] = v[m];
}

// The column pass of gpe_rot.hip with a local time per half: PRE (the second half of the step that started at t_pre)
// uses Omega(t_pre), POST (the first half of the step that starts at t_post) Omega(t_post).
template <typename T, int N, int C, bool PRE, bool POST>
__global__ __launch_bounds__(C* N / reg_default_pts<N>()) void rstir_col_kernel(
    Cx<T>* __restrict__ psi, T* __restrict__ dens, const EnvParams<T>* __restrict__ ep, const Cx<T>* __restrict__ tw,
    const Cx<T>* __restrict__ kin, const RotAxis<T> ax, int ny, const double* __restrict__ partial, int blocks_per_env,
    double dx2, T t_pre, T t_post) {
  using E = RegFft<T, N>;
  constexpr int PTS = E::kPts, NP = E::NP;
  constexpr bool WL = rot_col_wave_local(N);
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int tid = threadIdx.x;
  const int j = tid / C, c = tid - j * C;
  Cx<T>* const seq = reinterpret_cast<Cx<T>*>(smem_raw) + c * NP;
  const int env = blockIdx.y;
  const int col0 = blockIdx.x * C;
  Cx<T>* const gb = psi + (int64_t)env * N * ny + col0;
  T* const db = dens + (int64_t)env * N * ny + col0;
  Cx<T> v[PTS];
#pragma unroll
  for (int m = 0; m < PTS; ++m) v[m] = gb[E::natural(j, m) * ny + c];
  __shared__ double scale_sh;  // published by the barrier(s) of the first transform
  if constexpr (PRE) {
    if (tid < 64) {
      double sum = 0.0;
      for (int q = tid; q < blocks_per_env; q += 64) sum += partial[(int64_t)env * blocks_per_env + q];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o, 64);
      if (tid == 0) scale_sh = 1.0 / sqrt(sum * dx2);
    }
  }
  const int ji = WL ? tid % E::TT : j;
  const int cs = WL ? tid / E::TT : c;
  Cx<T>* const seqi = reinterpret_cast<Cx<T>*>(smem_raw) + cs * NP;
  const T wy = ax.w * (ax.c_first + T(col0 + cs) * ax.c_step);  // the line's coefficient is Omega(t) times this
  // one line operator with the coefficient a (gpe_rot.hip: two in a row need no barrier in between)
  auto line_op = [&](auto scaled, const T a) {
    if constexpr (WL)
      E::template dif_split<-1>(v, seq, j, seqi, ji, tw);
    else
      E::template dif<-1, false>(v, seq, tw, j);
    T scale = T(1);
    if constexpr (decltype(scaled)::value) scale = (T)scale_sh;  // read behind the transform's barrier
#pragma unroll
    for (int sl = 0; sl < PTS; ++sl) {
      const int fr = E::freq(ji, sl);
      Cx<T> m = rot_mult<T>(kin[fr], a, fr, N, ax.sr, ax.si);
      if constexpr (decltype(scaled)::value) {
        m.re *= scale;
        m.im *= scale;
      }
      v[sl] = cmul(v[sl], m);
      if constexpr (kOneFactorAtATime<T, PTS>) __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (WL)
      E::template dit_split<+1>(v, seqi, ji, seq, j, tw);
    else
      E::template dit<+1, false>(v, seq, tw, j);
  };
  if constexpr (PRE) line_op(std::true_type{}, rot_omega_at(ep[env], t_pre) * wy);
  if constexpr (POST) {
#pragma unroll
    for (int m = 0; m < PTS; ++m) db[E::natural(j, m) * ny + c] = v[m].re * v[m].re + v[m].im * v[m].im;
    line_op(std::false_type{}, rot_omega_at(ep[env], t_post) * wy);
  }
#pragma unroll
  for (int m = 0; m < PTS; ++m) gb[E::natural(j, m) * ny + c] = v[m];
}

// ---- pointwise kernels of the library path (any grid) ------------------------------------------------------------

// rot_mul_kernel of gpe_rot.hip with Omega(t)
template <typename T, int AXIS, bool SCALED>
__global__ __launch_bounds__(256) void rstir_mul_kernel(Cx<T>* __restrict__ psi, const Cx<T>* __restrict__ kin,
                                                        const EnvParams<T>* __restrict__ ep, const RotAxis<T> ax, int nx,
                                                        int ny, const double* __restrict__ partial, int nblocks, double dx2,
                                                        T t) {
  const int b = blockIdx.y;
  const int64_t cells = (int64_t)nx * ny;
  Cx<T>* const pb = psi + (int64_t)b * cells;
  T scale = T(1);
  if constexpr (SCALED) {
    double s = 0.0;
    for (int q = 0; q < nblocks; ++q) s += partial[(int64_t)b * nblocks + q];
    scale = (T)(1.0 / sqrt(s * dx2));
  }
  const T om = rot_omega_at(ep[b], t);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (int64_t)gridDim.x * 256) {
    const int ix = (int)(i / ny), iy = (int)(i - (int64_t)ix * ny);
    const int k = AXIS == 0 ? ix : iy, n = AXIS == 0 ? nx : ny, line = AXIS == 0 ? iy : ix;
    Cx<T> m = rot_mult<T>(kin[k], om * (ax.w * (ax.c_first + T(line) * ax.c_step)), k, n, ax.sr, ax.si);
    m.re *= scale;
    m.im *= scale;
    pb[i] = cmul(pb[i], m);
  }
}

// rot_b_kernel of gpe_rot.hip with the spots at sa.t in b
template <typename T>
__global__ __launch_bounds__(256) void rstir_b_kernel(Cx<T>* __restrict__ psi, const T* __restrict__ dens,
                                                      const T* __restrict__ pot, int64_t pot_stride,
                                                      const EnvParams<T>* __restrict__ ep, T tr, T ti, int64_t cells, int ny,
                                                      double* __restrict__ partial, const SpotArgs<T> sa) {
  const int b = blockIdx.y;
  Cx<T>* const pb = psi + (int64_t)b * cells;
  const T* const db = dens + (int64_t)b * cells;
  const T* const vb = pot ? pot + (int64_t)b * pot_stride : nullptr;
  const T kk = ep[b].gpe_k;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (int64_t)gridDim.x * 256) {
    T w = vb ? vb[i] : T(0);
    if (sa.n) {
      const int ix = (int)(i / ny), iy = (int)(i - (int64_t)ix * ny);
      w += spots_value<T>(sa, b, sa.x_first + T(ix) * sa.hx, sa.y_first + T(iy) * sa.hy);
    }
    w += kk * db[i];
    T sn, cs;
    sincos_t<T>(w * tr, &sn, &cs);
    const T mag = (ti == T(0)) ? T(1) : exp_t<T>(w * ti);
    const Cx<T> r = cmul(pb[i], Cx<T>{mag * cs, -mag * sn});
    pb[i] = r;
    acc += (double)(r.re * r.re + r.im * r.im);
  }
  __shared__ double sh[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[(int64_t)b * gridDim.x + blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// ---- host ----------------------------------------------------------------------------------------------------------

template <typename T, int N>
int launch_rstir_row(pdeopt_ctx* ctx, const Window& w, GpeRot& gr, std::complex<double> tau, double t) {
  const pdeopt_problem& p = ctx->prob;
  const AuxField& pot = ctx->aux[PDEOPT_AUX_GPE_POTENTIAL];
  constexpr int F = rot_row_lines<T, N>();
  const size_t lds = (size_t)F * RegFft<T, N>::NP * sizeof(Cx<T>);
  auto kern = rstir_row_kernel<T, N>;
  int rc = allow_lds(ctx, kern, lds);
  if (rc) return rc;
  const int64_t cells = (int64_t)p.nx * p.ny, w0 = w.lo;
  const int blocks = (int)((int64_t)w.n * p.nx / F);
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), lds, w.stream, (Cx<T>*)ctx->Y + w0 * cells,
                     (const T*)gr.dens + w0 * cells, pot.dev ? (const T*)pot.dev + (pot.per_env ? w0 * cells : 0) : nullptr,
                     pot.per_env ? cells : (int64_t)0, env_params<T>(ctx, w.lo), (const Cx<T>*)gr.tw_y,
                     (const Cx<T>*)gr.kin_y, (T)tau.real(), (T)tau.imag(), rot_axis<T>(ctx, 1, 0.5 * tau), p.nx,
                     gr.partial + w0 * gr.partial_per_env, make_spot_args<T>(ctx, w.lo, t));
  ctx->n_stage_launches++;
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  return PDEOPT_OK;
}

// JOIN instantiations that do not fit the register file run as LAST + FIRST (3 passes per step), as in gpe_rot.hip:
// fp64 at N = 1024 there and here; the second line coefficient costs no further instantiation
template <typename T, int N>
constexpr bool rstir_join_fits() { return !(sizeof(T) == 8 && N == 1024); }

template <typename T, int N, bool PRE, bool POST>
int launch_rstir_col(pdeopt_ctx* ctx, const Window& w, GpeRot& gr, std::complex<double> tau, double t_pre, double t_post) {
  if constexpr (PRE && POST && !rstir_join_fits<T, N>()) {
    const int rc = launch_rstir_col<T, N, true, false>(ctx, w, gr, tau, t_pre, t_post);
    return rc ? rc : launch_rstir_col<T, N, false, true>(ctx, w, gr, tau, t_pre, t_post);
  }
  const pdeopt_problem& p = ctx->prob;
  constexpr int C = rot_cols<T, N>();
  const int64_t cells = (int64_t)p.nx * p.ny, w0 = w.lo;
  const size_t lds = (size_t)C * RegFft<T, N>::NP * sizeof(Cx<T>);
  if constexpr (!(PRE && POST) || rstir_join_fits<T, N>()) {
    auto kern = rstir_col_kernel<T, N, C, PRE, POST>;
    int rc = allow_lds(ctx, kern, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(kern, dim3(p.ny / C, w.n), dim3(C * N / reg_default_pts<N>()), lds, w.stream,
                       (Cx<T>*)ctx->Y + w0 * cells, (T*)gr.dens + w0 * cells, env_params<T>(ctx, w.lo),
                       (const Cx<T>*)gr.tw_x, (const Cx<T>*)gr.kin_x, rot_axis<T>(ctx, 0, 0.5 * tau), p.ny,
                       (const double*)gr.partial + w0 * gr.partial_per_env, gr.partial_per_env,
                       ctx->strang_dx * ctx->strang_dx, (T)t_pre, (T)t_post);
    ctx->n_stage_launches++;
    PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  }
  return PDEOPT_OK;
}

template <typename T>
int rstir_row_dispatch(pdeopt_ctx* ctx, const Window& w, GpeRot& gr, std::complex<double> tau, double t) {
  switch (ctx->prob.ny) {
#define X(NN) case NN: return launch_rstir_row<T, NN>(ctx, w, gr, tau, t);
    PDEOPT_ROT_SIZES(X)
#undef X
    default: return fail(ctx, PDEOPT_EINVAL, "rotating split step: ny=%d is not covered", ctx->prob.ny);
  }
}
template <typename T, bool PRE, bool POST>
int rstir_col_dispatch(pdeopt_ctx* ctx, const Window& w, GpeRot& gr, std::complex<double> tau, double t_pre, double t_post) {
  switch (ctx->prob.nx) {
#define X(NN) case NN: return launch_rstir_col<T, NN, PRE, POST>(ctx, w, gr, tau, t_pre, t_post);
    PDEOPT_ROT_SIZES(X)
#undef X
    default: return fail(ctx, PDEOPT_EINVAL, "rotating split step: nx=%d is not covered", ctx->prob.nx);
  }
}

// one substep from local time t on rocFFT's 1-D plans, whole batch
template <typename T>
int rstir_library_step(pdeopt_ctx* ctx, GpeRot& gr, std::complex<double> tau, double t) {
  const pdeopt_problem& p = ctx->prob;
  const int64_t cells = (int64_t)p.nx * p.ny, total = cells * p.batch;
  const AuxField& pot = ctx->aux[PDEOPT_AUX_GPE_POTENTIAL];
  const int g1 = (int)std::min<int64_t>(4096, (cells + 255) / 256);
  const dim3 mgrid(g1, p.batch);
  const EnvParams<T>* ep = env_params<T>(ctx, 0);
  const RotAxis<T> ax = rot_axis<T>(ctx, 0, 0.5 * tau), ay = rot_axis<T>(ctx, 1, 0.5 * tau);
  const double dx2 = ctx->strang_dx * ctx->strang_dx;
  Cx<T>* const y = (Cx<T>*)ctx->Y;
  int rc;
  auto lx = [&](bool scaled) -> int {
    int r = spectral_c2c_axis(ctx, 0, true, y);
    if (r) return r;
    if (scaled)
      hipLaunchKernelGGL((rstir_mul_kernel<T, 0, true>), mgrid, dim3(256), 0, ctx->stream, y, (const Cx<T>*)gr.kin_x, ep, ax,
                         p.nx, p.ny, (const double*)gr.partial, kLibNormBlocks, dx2, (T)t);
    else
      hipLaunchKernelGGL((rstir_mul_kernel<T, 0, false>), mgrid, dim3(256), 0, ctx->stream, y, (const Cx<T>*)gr.kin_x, ep,
                         ax, p.nx, p.ny, (const double*)nullptr, 0, dx2, (T)t);
    return spectral_c2c_axis(ctx, 0, false, y);
  };
  auto ly = [&]() -> int {
    int r = spectral_c2c_axis(ctx, 1, true, y);
    if (r) return r;
    hipLaunchKernelGGL((rstir_mul_kernel<T, 1, false>), mgrid, dim3(256), 0, ctx->stream, y, (const Cx<T>*)gr.kin_y, ep, ay,
                       p.nx, p.ny, (const double*)nullptr, 0, dx2, (T)t);
    return spectral_c2c_axis(ctx, 1, false, y);
  };
  hipLaunchKernelGGL(rot_density_kernel<T>, dim3((int)std::min<int64_t>(4096, (total + 255) / 256)), dim3(256), 0,
                     ctx->stream, (const Cx<T>*)y, (T*)gr.dens, total);
  if ((rc = lx(false))) return rc;
  if ((rc = ly())) return rc;
  hipLaunchKernelGGL(rstir_b_kernel<T>, dim3(kLibNormBlocks, p.batch), dim3(256), 0, ctx->stream, y, (const T*)gr.dens,
                     (const T*)pot.dev, pot.per_env ? cells : (int64_t)0, ep, (T)tau.real(), (T)tau.imag(), cells, p.ny,
                     gr.partial, make_spot_args<T>(ctx, 0, t));
  if ((rc = ly())) return rc;
  if ((rc = lx(true))) return rc;
  ctx->n_stage_launches += 6;
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  return PDEOPT_OK;
}

template <typename T>
int strang_rot_stir_t(pdeopt_ctx* ctx, bool fused, double t0, double dt, int64_t n) {
  GpeRot& gr = *ctx->gpe_rot;
  const pdeopt_problem& p = ctx->prob;
  const int64_t cells = (int64_t)p.nx * p.ny;
  const std::complex<double> tau = dt * std::complex<double>(ctx->ts_re, ctx->ts_im);
  const auto t_of = [&](int64_t s) { return t0 + (double)s * dt; };  // the local time of pdeopt_advance's substep s
  int rc;
  if (!fused) {
    for (int64_t s = 0; s < n; ++s)
      if ((rc = rstir_library_step<T>(ctx, gr, tau, t_of(s)))) return rc;
    ctx->last_kernel = "strang_rot_stir_rocfft_1d";
    return PDEOPT_OK;
  }
  // the group schedule of gpe_rot.hip; a window's spot table and parameters start at its first environment
  int group = p.batch;
  if (ctx->opt_group_envs > 0)
    group = (int)std::min<int64_t>(ctx->opt_group_envs, p.batch);
  else if (ctx->opt_group_envs == 0 && n > 1)
    group = cache_group(p.batch, (size_t)cells * (sizeof(Cx<T>) + sizeof(T)), 192ull << 20, false);
  auto first = [&](const Window& w) -> int { return rstir_col_dispatch<T, false, true>(ctx, w, gr, tau, t_of(0), t_of(0)); };
  auto substep = [&](const Window& w, int64_t s, int&) -> int {
    int r;
    if ((r = rstir_row_dispatch<T>(ctx, w, gr, tau, t_of(s)))) return r;
    return s + 1 < n ? rstir_col_dispatch<T, true, true>(ctx, w, gr, tau, t_of(s), t_of(s + 1))
                     : rstir_col_dispatch<T, true, false>(ctx, w, gr, tau, t_of(s), t_of(s));
  };
  if ((rc = run_groups(ctx, group, false, 0, n, first, substep))) return rc;
  ctx->last_kernel = "strang_rot_stir_fused_lds_fft";
  return PDEOPT_OK;
}

}  // namespace

int advance_strang_rot_stir(pdeopt_ctx* ctx, double t0, double dt, int64_t n) {
  bool fused = false;
  const int rc = gpe_rot_prepare(ctx, dt, &fused);
  if (rc) return rc;
  return with_dtype(ctx, [&](auto t) { return strang_rot_stir_t<decltype(t)>(ctx, fused, t0, dt, n); });
}

}  // namespace pdeopt
