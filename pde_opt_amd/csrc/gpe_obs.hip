// Observables of the resident GPE wavefunction (pdeopt_gpe_observables): norm, kinetic,
// potential and interaction energy, angular momentum and the second moments, per environment, in two read-only
// passes with the geometry of the rotating split step (gpe_rot.hip).
//
// With psi^x = fft(psi, axis 0), psi^y = fft(psi, axis 1) (unnormalised), Px = |psi^x|^2 / nx, Py = |psi^y|^2 / ny
// (Parseval per line), kx / ky the signed fftfreq values and h^2 = hx hy:
//   norm  = h^2 sum |psi|^2                         e_pot = h^2 sum V |psi|^2      e_int = h^2 sum k/2 |psi|^4
//   e_kin = h^2 [sum 1/2 (2 pi kx)^2 Px + sum 1/2 (2 pi ky)^2 Py]
//   l_z   = h^2 [sum x (2 pi ky) Py - sum y (2 pi kx) Px]            x2, y2 = h^2 sum x^2 |psi|^2, h^2 sum y^2 |psi|^2
// V is what a substep starting at t would use: the resident potential (shared or per environment; a source registered
// through pdeopt_set_aux_time_fn is sampled at t) plus the in-kernel spots at t.
//
//   row pass : a line along y per N/PTS threads of one wave (rot_row_kernel's layout): the five pointwise sums, one
//              forward transform in registers / LDS, the two Py-weighted sums
//   col pass : a line along x (rot_col_kernel's layout): one forward transform, the two Px-weighted sums
//   finish   : the workgroups' partial sums of an environment, added in a fixed order, times h^2
// Every lane accumulates in fp64 (the products are formed in fp64 from the stored values), the partial sums travel as
// plain stores, there are no atomics: a repeat gives identical bits.  The weights come from the signed frequency index
// and the line's coordinate: no N^2 table.  The state is not modified and no inverse transform is needed.
//
// An axis whose length is outside {64 .. 1024}, or whose pass would not divide the other axis into whole workgroups
// (gpe_observables_t), is transformed by rocFFT's batched 1-D plan (spectral_c2c_axis) on a copy of the state, and a
// pointwise kernel forms the weighted sums; the two axes choose independently.  The plans are whole-batch: the library
// path copies and transforms every environment once per library axis even when a sub-range is asked for.
#include <algorithm>
#include <cmath>

#include "block_sums.hpp"
#include "common.hpp"
#include "fft_lds.hpp"
#include "fft_reg.hpp"
#include "split_step_util.hpp"

namespace pdeopt {

struct GpeObs : Feature {
  DeviceBuffer tw_x;  // twiddle tables exp(-2 pi i n / N) in the problem dtype
  DeviceBuffer tw_y;
  DeviceBuffer work;  // library path: the copy of the state rocFFT transforms in place
  // doubles:
  DeviceBuffer part8;   // [batch][n8][8]: pointwise sums (+ the Py-weighted ones of the hand-written row pass)
  DeviceBuffer part_y;  // [batch][kLibBlocks][2]: (e_kin, l_z) share of the y transform, library path
  DeviceBuffer part_x;  // [batch][nx_blocks][2]: (e_kin, l_z) share of the x transform
  DeviceBuffer out;     // [batch][8]
};

namespace {

constexpr int kObs = PDEOPT_GPE_OBS_COUNT;
constexpr int kLibBlocks = 64;

// where cell (0, 0) sits and what a frequency index is worth: coordinates and weights are formed in fp64
struct ObsGeom {
  double x_first, y_first, hx, hy;
  double wx, wy;  // 2 pi / (nx hx), 2 pi / (ny hy): 2 pi k = w * signed index
};

__device__ __forceinline__ int signed_index(int f, int n) { return f < (n + 1) / 2 ? f : f - n; }

template <typename T>
__device__ __forceinline__ double abs2(const Cx<T> v) {
  return (double)v.re * (double)v.re + (double)v.im * (double)v.im;
}

// the five pointwise terms of one cell, added into a[0] norm, a[2] e_pot, a[3] e_int, a[5] x2, a[6] y2
template <typename T>
__device__ __forceinline__ void point_terms(double (&a)[7], const Cx<T> v, double pot, double half_k, double x, double y) {
  const double d = abs2(v);
  a[0] += d;
  a[2] += pot * d;
  a[3] += half_k * d * d;
  a[5] += x * x * d;
  a[6] += y * y * d;
}

// The row pass: lines along y (contiguous), N/PTS threads per line, 256/(N/PTS) lines per workgroup, every line in one
// wave.  partial[blockIdx.x][8]
template <typename T, int N>
__global__ __launch_bounds__(256) void gobs_row_kernel(const Cx<T>* __restrict__ psi, const T* __restrict__ pot,
                                                       int64_t pot_env_stride, const EnvParams<T>* __restrict__ ep,
                                                       const SpotArgs<T> sa, const Cx<T>* __restrict__ tw, int nx,
                                                       const ObsGeom gm, double* __restrict__ partial) {
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
  const Cx<T>* const g = psi + row * N;
  Cx<T> v[PTS];
#pragma unroll
  for (int m = 0; m < PTS; ++m) v[m] = g[E::natural(j, m)];
  const double x = gm.x_first + (double)ix * gm.hx;
  const double half_k = 0.5 * (double)ep[env].gpe_k;
  const T* const vrow = pot ? pot + (int64_t)env * pot_env_stride + (int64_t)ix * N : nullptr;
  const T xs = sa.x_first + T(ix) * sa.hx;  // the spots' coordinates as a substep forms them
  double a[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int m = 0; m < PTS; ++m) {
    const int n = E::natural(j, m);
    T w = vrow ? vrow[n] : T(0);
    if (sa.n) w += spots_value<T>(sa, env, xs, sa.y_first + T(n) * sa.hy);
    point_terms<T>(a, v[m], (double)w, half_k, x, gm.y_first + (double)n * gm.hy);
  }
  E::template dif<-1>(v, seq, tw, j);
  double s1 = 0.0, s2 = 0.0;  // sum (2 pi ky)^2 |psi^y|^2, sum (2 pi ky) |psi^y|^2
#pragma unroll
  for (int sl = 0; sl < PTS; ++sl) {
    const double kv = gm.wy * (double)signed_index(E::freq(j, sl), N);
    const double p = abs2(v[sl]);
    s1 += kv * kv * p;
    s2 += kv * p;
  }
  a[1] = 0.5 * s1 * (1.0 / N);
  a[4] = x * s2 * (1.0 / N);
  block_sums<7, 4>(a, partial + (int64_t)blockIdx.x * kObs);
}

// column-pass geometry of the rotating step (rot_cols in gpe_rot.hip): C adjacent columns x N/PTS threads, the column
// index fastest across lanes on the global side; up to N = 512 stages 1.. run with a column per wave
constexpr bool gobs_col_wave_local(int n) { return n <= 512; }
template <typename T, int N>
constexpr int gobs_cols() {
  constexpr int c = sizeof(T) == 4 ? 16 : 8, cap = sizeof(T) == 4 ? 512 : 256, tt = N / reg_default_pts<N>();
  return c * tt > cap ? cap / tt : c;
}

// The column pass: lines along x (stride ny).  partial[env][blockIdx.x][2] = (e_kin, l_z) share of the x transform
template <typename T, int N, int C>
__global__ __launch_bounds__(C* N / reg_default_pts<N>()) void gobs_col_kernel(const Cx<T>* __restrict__ psi,
                                                                               const Cx<T>* __restrict__ tw, int ny,
                                                                               const ObsGeom gm,
                                                                               double* __restrict__ partial) {
  using E = RegFft<T, N>;
  constexpr int PTS = E::kPts, NP = E::NP, THREADS = C * N / reg_default_pts<N>();
  constexpr bool WL = gobs_col_wave_local(N);
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int tid = threadIdx.x;
  const int j = tid / C, c = tid - j * C;
  Cx<T>* const seq = reinterpret_cast<Cx<T>*>(smem_raw) + c * NP;
  const int env = blockIdx.y;
  const int col0 = blockIdx.x * C;
  const Cx<T>* const gb = psi + (int64_t)env * N * ny + col0;
  Cx<T> v[PTS];
#pragma unroll
  for (int m = 0; m < PTS; ++m) v[m] = gb[E::natural(j, m) * ny + c];
  // spectrum side: with WL the thread serves column tid / TT as its thread ji, else column c as thread j
  const int ji = WL ? tid % E::TT : j;
  const int cs = WL ? tid / E::TT : c;
  Cx<T>* const seqi = reinterpret_cast<Cx<T>*>(smem_raw) + cs * NP;
  if constexpr (WL)
    E::template dif_split<-1>(v, seq, j, seqi, ji, tw);
  else
    E::template dif<-1, false>(v, seq, tw, j);
  const double y = gm.y_first + (double)(col0 + cs) * gm.hy;
  double s1 = 0.0, s2 = 0.0;
#pragma unroll
  for (int sl = 0; sl < PTS; ++sl) {
    const double kv = gm.wx * (double)signed_index(E::freq(ji, sl), N);
    const double p = abs2(v[sl]);
    s1 += kv * kv * p;
    s2 += kv * p;
  }
  double a[2] = {0.5 * s1 * (1.0 / N), -y * s2 * (1.0 / N)};
  block_sums<2, (THREADS + 63) / 64>(a, partial + ((int64_t)env * gridDim.x + blockIdx.x) * 2);
}

// ---- pointwise kernels of the library path (any grid) ------------------------------------------------------------

// the five pointwise sums: partial[env][blockIdx.x][8] (entries 1 and 4 are zero)
template <typename T>
__global__ __launch_bounds__(256) void gobs_point_kernel(const Cx<T>* __restrict__ psi, const T* __restrict__ pot,
                                                         int64_t pot_env_stride, const EnvParams<T>* __restrict__ ep,
                                                         const SpotArgs<T> sa, int nx, int ny, const ObsGeom gm,
                                                         double* __restrict__ partial) {
  const int b = blockIdx.y;
  const int64_t cells = (int64_t)nx * ny;
  const Cx<T>* const pb = psi + (int64_t)b * cells;
  const T* const vb = pot ? pot + (int64_t)b * pot_env_stride : nullptr;
  const double half_k = 0.5 * (double)ep[b].gpe_k;
  double a[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (int64_t)gridDim.x * 256) {
    const int ix = (int)(i / ny), iy = (int)(i - (int64_t)ix * ny);
    T w = vb ? vb[i] : T(0);
    if (sa.n) w += spots_value<T>(sa, b, sa.x_first + T(ix) * sa.hx, sa.y_first + T(iy) * sa.hy);
    point_terms<T>(a, pb[i], (double)w, half_k, gm.x_first + (double)ix * gm.hx, gm.y_first + (double)iy * gm.hy);
  }
  block_sums<7, 4>(a, partial + ((int64_t)b * gridDim.x + blockIdx.x) * kObs);
}

// spec = the state transformed along `axis` (0: x, frequency index ix, the line's coordinate is y of iy; 1: y,
// frequency index iy, coordinate x of ix): partial[env][blockIdx.x][2] = (e_kin, l_z) share of that transform
template <typename T>
__global__ __launch_bounds__(256) void gobs_spec_kernel(const Cx<T>* __restrict__ spec, int axis, int nx, int ny,
                                                        const ObsGeom gm, double* __restrict__ partial) {
  const int b = blockIdx.y;
  const int64_t cells = (int64_t)nx * ny;
  const Cx<T>* const pb = spec + (int64_t)b * cells;
  const int n = axis == 0 ? nx : ny;
  const double w = axis == 0 ? gm.wx : gm.wy, rn = 1.0 / (double)n;
  double a[2] = {0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (int64_t)gridDim.x * 256) {
    const int ix = (int)(i / ny), iy = (int)(i - (int64_t)ix * ny);
    const double kv = w * (double)signed_index(axis == 0 ? ix : iy, n);
    const double coord = axis == 0 ? -(gm.y_first + (double)iy * gm.hy) : gm.x_first + (double)ix * gm.hx;
    const double p = abs2(pb[i]) * rn;
    a[0] += 0.5 * kv * kv * p;
    a[1] += coord * kv * p;
  }
  block_sums<2, 4>(a, partial + ((int64_t)b * gridDim.x + blockIdx.x) * 2);
}

// one wave per environment: the partial sums in a fixed order, times h^2
__global__ __launch_bounds__(64) void gobs_finish_kernel(const double* __restrict__ p8, int n8,
                                                         const double* __restrict__ py, int npy,
                                                         const double* __restrict__ px, int npx, double h2,
                                                         double* __restrict__ out) {
  const int env = blockIdx.x, lane = threadIdx.x;
  double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  rows_total<7, kObs>(p8 + (int64_t)env * n8 * kObs, n8, lane, s);
  for (int q = lane; q < npy; q += 64) {
    s[1] += py[((int64_t)env * npy + q) * 2];
    s[4] += py[((int64_t)env * npy + q) * 2 + 1];
  }
  for (int q = lane; q < npx; q += 64) {
    s[1] += px[((int64_t)env * npx + q) * 2];
    s[4] += px[((int64_t)env * npx + q) * 2 + 1];
  }
#pragma unroll
  for (int c = 0; c < 7; ++c) s[c] = wave_sum(s[c]);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 7; ++c) out[(int64_t)env * kObs + c] = s[c] * h2;
    out[(int64_t)env * kObs + 7] = 0.0;
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------

bool gobs_size_ok(int n) { return n == 64 || n == 128 || n == 256 || n == 512 || n == 1024; }
int gobs_row_lines(int ny) { return 256 / (ny / (ny > 512 ? 16 : 8)); }
template <typename T>
int gobs_cols_rt(int nx) {  // gobs_cols<T, nx>() of a covered size
  const int c = sizeof(T) == 4 ? 16 : 8, cap = sizeof(T) == 4 ? 512 : 256, tt = nx / (nx > 512 ? 16 : 8);
  return c * tt > cap ? cap / tt : c;
}

#define PDEOPT_GOBS_SIZES(X) X(64) X(128) X(256) X(512) X(1024)

template <typename T, int N>
int launch_gobs_row(pdeopt_ctx* ctx, GpeObs& go, int env_first, int env_count, const SpotArgs<T>& sa, const ObsGeom& gm) {
  const pdeopt_problem& p = ctx->prob;
  const AuxField& pot = ctx->aux[PDEOPT_AUX_GPE_POTENTIAL];
  constexpr int F = 256 / RegFft<T, N>::TT;
  const size_t lds = (size_t)F * RegFft<T, N>::NP * sizeof(Cx<T>);
  auto kern = gobs_row_kernel<T, N>;
  int rc = allow_lds(ctx, kern, lds);
  if (rc) return rc;
  const int64_t cells = (int64_t)p.nx * p.ny, w0 = env_first;
  const int blocks = (int)((int64_t)env_count * p.nx / F);
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), lds, ctx->stream, ctx->Y.as<const Cx<T>>() + w0 * cells,
                     pot.dev ? pot.dev.as<const T>() + (pot.per_env ? w0 * cells : 0) : nullptr,
                     pot.per_env ? cells : (int64_t)0, env_params<T>(ctx, env_first), sa, go.tw_y.as<const Cx<T>>(), p.nx, gm,
                     go.part8.as<double>());
  return PDEOPT_OK;
}

template <typename T, int N>
int launch_gobs_col(pdeopt_ctx* ctx, GpeObs& go, int env_first, int env_count, const ObsGeom& gm) {
  const pdeopt_problem& p = ctx->prob;
  constexpr int C = gobs_cols<T, N>();
  const size_t lds = (size_t)C * RegFft<T, N>::NP * sizeof(Cx<T>);
  auto kern = gobs_col_kernel<T, N, C>;
  int rc = allow_lds(ctx, kern, lds);
  if (rc) return rc;
  const int64_t cells = (int64_t)p.nx * p.ny;
  hipLaunchKernelGGL(kern, dim3(p.ny / C, env_count), dim3(C * N / reg_default_pts<N>()), lds, ctx->stream,
                     ctx->Y.as<const Cx<T>>() + (int64_t)env_first * cells, go.tw_x.as<const Cx<T>>(), p.ny, gm, go.part_x.as<double>());
  return PDEOPT_OK;
}

template <typename T>
int gobs_row_dispatch(pdeopt_ctx* ctx, GpeObs& go, int env_first, int env_count, const SpotArgs<T>& sa, const ObsGeom& gm) {
  switch (ctx->prob.ny) {
#define X(NN) case NN: return launch_gobs_row<T, NN>(ctx, go, env_first, env_count, sa, gm);
    PDEOPT_GOBS_SIZES(X)
#undef X
    default: return fail(ctx, PDEOPT_EINVAL, "GPE observables: ny=%d has no hand-written row pass", ctx->prob.ny);
  }
}
template <typename T>
int gobs_col_dispatch(pdeopt_ctx* ctx, GpeObs& go, int env_first, int env_count, const ObsGeom& gm) {
  switch (ctx->prob.nx) {
#define X(NN) case NN: return launch_gobs_col<T, NN>(ctx, go, env_first, env_count, gm);
    PDEOPT_GOBS_SIZES(X)
#undef X
    default: return fail(ctx, PDEOPT_EINVAL, "GPE observables: nx=%d has no hand-written column pass", ctx->prob.nx);
  }
}

// the (e_kin, l_z) share of the transform along `axis` through rocFFT: the whole batch is copied and transformed
// (the plans are whole-batch), the sums are formed for the environments asked for
template <typename T>
int gobs_library_axis(pdeopt_ctx* ctx, GpeObs& go, int axis, int env_first, int env_count, const ObsGeom& gm, double* part) {
  const pdeopt_problem& p = ctx->prob;
  const int64_t cells = (int64_t)p.nx * p.ny;
  const size_t bytes = (size_t)cells * p.batch * sizeof(Cx<T>);
  int rc = ensure_buffer(ctx, go.work, bytes);
  if (rc) return rc;
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(go.work.get(), ctx->Y.get(), bytes, hipMemcpyDeviceToDevice, ctx->stream));
  if ((rc = spectral_c2c_axis(ctx, axis, true, go.work.get()))) return rc;
  hipLaunchKernelGGL(gobs_spec_kernel<T>, dim3(kLibBlocks, env_count), dim3(256), 0, ctx->stream,
                     go.work.as<const Cx<T>>() + (int64_t)env_first * cells, axis, p.nx, p.ny, gm, part);
  return PDEOPT_OK;
}

template <typename T>
int gpe_observables_t(pdeopt_ctx* ctx, double t, int env_first, int env_count, double x_first, double y_first,
                      double* host_out) {
  GpeObs& go = ctx->features.ensure<GpeObs>(FS_GPE_OBS);
  const pdeopt_problem& p = ctx->prob;
  const int64_t cells = (int64_t)p.nx * p.ny;
  // The two axes choose independently, so unlike the rotating step a hand-written pass may meet an uncovered length on
  // the OTHER axis: the row pass takes whole workgroups of lines that must not straddle environments (nx a multiple of
  // its lines per workgroup), the column pass whole groups of C columns (ny a multiple of C); otherwise that axis
  // goes through the library too
  const bool row_fused = ctx->opt_kernel_path != 1 && gobs_size_ok(p.ny) && p.nx % gobs_row_lines(p.ny) == 0;
  const bool col_fused = ctx->opt_kernel_path != 1 && gobs_size_ok(p.nx) && p.ny % gobs_cols_rt<T>(p.nx) == 0;
  int rc;
  // sized for either path of either axis: at most nx row workgroups and ny column workgroups per environment
  if ((rc = ensure_buffer(ctx, go.part8, sizeof(double) * kObs * (size_t)p.batch * std::max(p.nx, kLibBlocks)))) return rc;
  if ((rc = ensure_buffer(ctx, go.part_y, sizeof(double) * 2 * (size_t)p.batch * kLibBlocks))) return rc;
  if ((rc = ensure_buffer(ctx, go.part_x, sizeof(double) * 2 * (size_t)p.batch * std::max(p.ny, kLibBlocks)))) return rc;
  if ((rc = ensure_buffer(ctx, go.out, sizeof(double) * kObs * (size_t)p.batch))) return rc;
  if (row_fused && !go.tw_y && (rc = upload_table<T>(ctx, go.tw_y, p.ny))) return rc;
  if (col_fused && !go.tw_x && (rc = upload_table<T>(ctx, go.tw_x, p.nx))) return rc;
  if ((rc = refresh_time_aux(ctx, PDEOPT_AUX_GPE_POTENTIAL, t))) return rc;
  const AuxField& pot = ctx->aux[PDEOPT_AUX_GPE_POTENTIAL];
  const SpotArgs<T> sa = make_spot_args<T>(ctx, env_first, t);
  ObsGeom gm;
  gm.x_first = x_first;
  gm.y_first = y_first;
  gm.hx = p.hx;
  gm.hy = p.hy;
  gm.wx = 2.0 * M_PI / ((double)p.nx * p.hx);
  gm.wy = 2.0 * M_PI / ((double)p.ny * p.hy);
  int n8, npy, npx;
  if (row_fused) {
    if ((rc = gobs_row_dispatch<T>(ctx, go, env_first, env_count, sa, gm))) return rc;
    n8 = p.nx / gobs_row_lines(p.ny);
    npy = 0;
  } else {
    hipLaunchKernelGGL(gobs_point_kernel<T>, dim3(kLibBlocks, env_count), dim3(256), 0, ctx->stream,
                       ctx->Y.as<const Cx<T>>() + (int64_t)env_first * cells,
                       pot.dev ? pot.dev.as<const T>() + (pot.per_env ? (int64_t)env_first * cells : 0) : nullptr,
                       pot.per_env ? cells : (int64_t)0, env_params<T>(ctx, env_first), sa, p.nx, p.ny, gm, go.part8.as<double>());
    if ((rc = gobs_library_axis<T>(ctx, go, 1, env_first, env_count, gm, go.part_y.as<double>()))) return rc;
    n8 = kLibBlocks;
    npy = kLibBlocks;
  }
  if (col_fused) {
    if ((rc = gobs_col_dispatch<T>(ctx, go, env_first, env_count, gm))) return rc;
    npx = p.ny / gobs_cols_rt<T>(p.nx);
  } else {
    if ((rc = gobs_library_axis<T>(ctx, go, 0, env_first, env_count, gm, go.part_x.as<double>()))) return rc;
    npx = kLibBlocks;
  }
  hipLaunchKernelGGL(gobs_finish_kernel, dim3(env_count), dim3(64), 0, ctx->stream, go.part8.as<const double>(), n8,
                     go.part_y.as<const double>(), npy, go.part_x.as<const double>(), npx, p.hx * p.hy, go.out.as<double>());
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(host_out, go.out.as<double>(), sizeof(double) * kObs * (size_t)env_count, hipMemcpyDeviceToHost,
                                       ctx->stream));
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->last_kernel = row_fused && col_fused ? "gpe_obs_fused_lds_fft" : row_fused || col_fused ? "gpe_obs_mixed" : "gpe_obs_rocfft_1d";
  return PDEOPT_OK;
}

}  // namespace

int gpe_observables(pdeopt_ctx* ctx, double t, int env_first, int env_count, double x_first, double y_first,
                    double* host_out) {
  return with_dtype(ctx, [&](auto tag) {
    return gpe_observables_t<decltype(tag)>(ctx, t, env_first, env_count, x_first, y_first, host_out);
  });
}

}  // namespace pdeopt
