// Alternating-direction split step of the rotating-frame GPE (PDEOPT_INT_STRANG_ROT).
//
// The two operators GPE2DTSRot.A_terms publishes (gross_pitaevskii.py:122-126),
//   Ax(kx, y) = 0.5j (2 pi i kx)^2 - Omega y (2 pi i kx),     Ay(x, ky) = 0.5j (2 pi i ky)^2 + Omega x (2 pi i ky),
// are diagonal under a transform along ONE axis at a fixed coordinate of the other (Bao & Wang 2006):
//   Lx(s) v = ifft_x[exp(s Ax) fft_x v],   Ly(s) v = ifft_y[exp(s Ay) fft_y v].
// Step, tau = dt * time_scale, h^2 = strang_dx^2 (the two quirks of StrangSplitting.step kept: b from the state
// BEFORE the half step, renormalisation every step):
//   psi1 = Ly(tau/2) Lx(tau/2) psi0;   b = -i (V + k |psi0|^2);   psi2 = psi1 exp(b tau)
//   psi3 = psi2 / sqrt(h^2 sum |psi2|^2);   psi4 = Lx(tau/2) Ly(tau/2) psi3
//
// Every line is independent, so a pass loads a line, transforms it, multiplies, transforms back -- in registers / LDS
// (fft_reg.hpp) -- and two line operators of neighbouring half steps along the same axis share a pass:
//   col FIRST :                               |psi0|^2 -> Lx(tau/2)
//   row       : Ly(tau/2) -> * exp(b tau), partial sums of |psi2|^2 -> Ly(tau/2)
//   col JOIN  : Lx(tau/2) * scale -> |psi|^2 of the next step -> Lx(tau/2)          (col LAST: the first half only)
// = 2 passes per step in steady state.  The norm of psi2 is not known inside the row pass; the transforms are
// linear, so the scale is applied by the column pass that follows (fixed-order fp64 partial sums, no atomics).
//
// The multiplier of a line is a 1-D kinetic table per axis, exp(tau/2 0.5j (2 pi i k)^2) / N, times the rotation
// factor exp(-/+ Omega coord (2 pi i k) tau/2), evaluated in-kernel from Omega (EnvParams: one per environment),
// the line's coordinate and k: no N^2 table.
//
// Grids outside nx, ny in {64 .. 1024} run the same step on rocFFT's batched 1-D plans (spectral_c2c_axis) with the
// pointwise kernels below.
//
// Stirring and spinning up: Gaussian light spots (pdeopt_set_gpe_spots) in b and
// Omega(t) = Omega + rate t (pdeopt_set_env_gpe_omega_rate) in the line operators.  The step starting at local time
// t_s = t0 + s dt uses Omega(t_s) in all four of its line operators and V(t_s) = potential + spots(t_s, x, y) in b (the
// convention of the non-rotating Strang step: b at the substep's start); the JOIN pass is the one place where two steps
// meet, and its two halves take their own local time.  Every pass has two kernels: rot_ for a frozen problem, rstir_
// launched only when there are spots or some environment has a nonzero rate (advance_strang_rot), so a frozen problem
// keeps its instructions and its bits.  The host code is one copy.  The kernels stand side by side and are NOT one
// template body.  Tried (hipcc of ROCm's clang, -O3, the flags of build.py): the row, column, mul and b bodies as
// __device__ __forceinline__ templates on a clock type (frozen: no state; stirred: the spots and the local times) with
// `if constexpr` for the differences, each called from two thin __global__ wrappers of the present names; with and
// without __restrict__ on the body, structs by value and by reference.  Every kernel but rot_b_kernel<float> then
// compiled to other instructions than written out, the frozen ones included: rot_b_kernel<double> 2 of 451 (commuted
// operands), rot_mul_kernel 2 to 89 of about 300, the row and column passes most of theirs with up to 7 % fewer or
// more instructions (the optimised IR differs in operand and block order; presumably the body is simplified on its own
// before it is inlined).  The frozen kernels' instructions are not to move, so no pair is shared; a change to a pass
// is made in both kernels of its pair.  (The adjoint's multiplies, gpe_rot_adjoint.hip, came out identical and ARE shared.)
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

// RotAxis, rot_mult, rot_omega_at, rot_axis, upload_kinetic: gpe_rot_line.hpp (shared with the adjoint,
// gpe_rot_adjoint.hip); GpeRot, the pass geometry and rot_density_kernel: gpe_rot_step.hpp

// The row pass: lines along y (contiguous), N/PTS threads per line, 256/(N/PTS) lines per workgroup, every line in
// one wave (the exchanges need no s_barrier).  Ly(tau/2) -> exp(b tau) + norm partial -> Ly(tau/2).
template <typename T, int N>
__global__ __launch_bounds__(256) void rot_row_kernel(Cx<T>* __restrict__ psi, const T* __restrict__ dens,
                                                      const T* __restrict__ pot, int64_t pot_env_stride,
                                                      const EnvParams<T>* __restrict__ ep,
                                                      const Cx<T>* __restrict__ tw, const Cx<T>* __restrict__ kin,
                                                      T tr, T ti, const RotAxis<T> ax, int nx,
                                                      double* __restrict__ partial) {
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
  const T a = ax.w * ep[env].gpe_omega * (ax.c_first + T(ix) * ax.c_step);
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
  // psi2 = psi1 exp(b tau), b = -i (V + k |psi0|^2): exp(-i w (tr + i ti)) = exp(w ti) (cos(w tr) - i sin(w tr)).
  // |psi2|^2 of the thread's points in the working precision, the sums across threads / workgroups in fp64
  const T kk = ep[env].gpe_k;
  const T* const vrow = pot ? pot + (int64_t)env * pot_env_stride + (int64_t)ix * N : nullptr;
  T accp = T(0);
#pragma unroll
  for (int m = 0; m < PTS; ++m) {
    const int n = E::natural(j, m);
    const T w = (vrow ? vrow[n] : T(0)) + kk * dens[row * N + n];
    T sn, cs;
    sincos_t<T>(w * tr, &sn, &cs);
    const T mag = (ti == T(0)) ? T(1) : exp_t<T>(w * ti);
    v[m] = cmul(v[m], Cx<T>{mag * cs, -mag * sn});
    accp += v[m].re * v[m].re + v[m].im * v[m].im;
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

// The column pass: lines along x (stride ny).  PRE: Lx(tau/2) * scale, the second half of a step (scale =
// 1 / sqrt(h^2 sum |psi2|^2) from the row pass's partial sums).  POST: |psi|^2 of the state, then Lx(tau/2), the
// first half of a step.  FIRST = POST, JOIN = PRE + POST, LAST = PRE.
template <typename T, int N, int C, bool PRE, bool POST>
__global__ __launch_bounds__(C* N / reg_default_pts<N>()) void rot_col_kernel(
    Cx<T>* __restrict__ psi, T* __restrict__ dens, const EnvParams<T>* __restrict__ ep, const Cx<T>* __restrict__ tw,
    const Cx<T>* __restrict__ kin, const RotAxis<T> ax, int ny, const double* __restrict__ partial, int blocks_per_env,
    double dx2) {
  using E = RegFft<T, N>;
  constexpr int PTS = E::kPts, NP = E::NP;
  constexpr bool WL = rot_col_wave_local(N);
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int tid = threadIdx.x;
  const int j = tid / C, c = tid - j * C;
  Cx<T>* const seq = reinterpret_cast<Cx<T>*>(smem_raw) + c * NP;
  const int env = blockIdx.y;
  const int col0 = blockIdx.x * C;
  // uniform base pointers + 32-bit per-thread offsets
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
  // spectrum side: with WL the thread serves column tid / TT as its thread ji, else column c as thread j
  const int ji = WL ? tid % E::TT : j;
  const int cs = WL ? tid / E::TT : c;
  Cx<T>* const seqi = reinterpret_cast<Cx<T>*>(smem_raw) + cs * NP;
  const T a = ax.w * ep[env].gpe_omega * (ax.c_first + T(col0 + cs) * ax.c_step);
  // One line operator.  Two in a row need no barrier in between: the last exchange of the inverse reads, and the
  // first exchange of the next forward transform writes, only the thread's OWN stage-0 positions of the image.
  auto line_op = [&](auto scaled) {
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
  if constexpr (PRE) line_op(std::true_type{});
  if constexpr (POST) {
#pragma unroll
    for (int m = 0; m < PTS; ++m) db[E::natural(j, m) * ny + c] = v[m].re * v[m].re + v[m].im * v[m].im;
    line_op(std::false_type{});
  }
#pragma unroll
  for (int m = 0; m < PTS; ++m) gb[E::natural(j, m) * ny + c] = v[m];
}

// ---- pointwise kernels of the library path (any grid) ------------------------------------------------------------

// psi[b][ix][iy] *= kin[k] * rotation factor (* the norm scale of environment b).  AXIS 0: the field is transformed
// along x, k = ix, the line's coordinate is y of iy; AXIS 1: transformed along y, k = iy, coordinate x of ix.
template <typename T, int AXIS, bool SCALED>
__global__ __launch_bounds__(256) void rot_mul_kernel(Cx<T>* __restrict__ psi, const Cx<T>* __restrict__ kin,
                                                      const EnvParams<T>* __restrict__ ep, const RotAxis<T> ax, int nx,
                                                      int ny, const double* __restrict__ partial, int nblocks, double dx2) {
  const int b = blockIdx.y;
  const int64_t cells = (int64_t)nx * ny;
  Cx<T>* const pb = psi + (int64_t)b * cells;
  T scale = T(1);
  if constexpr (SCALED) {
    double s = 0.0;
    for (int q = 0; q < nblocks; ++q) s += partial[(int64_t)b * nblocks + q];
    scale = (T)(1.0 / sqrt(s * dx2));
  }
  const T om = ax.w * ep[b].gpe_omega;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (int64_t)gridDim.x * 256) {
    const int ix = (int)(i / ny), iy = (int)(i - (int64_t)ix * ny);
    const int k = AXIS == 0 ? ix : iy, n = AXIS == 0 ? nx : ny, line = AXIS == 0 ? iy : ix;
    Cx<T> m = rot_mult<T>(kin[k], om * (ax.c_first + T(line) * ax.c_step), k, n, ax.sr, ax.si);
    m.re *= scale;
    m.im *= scale;
    pb[i] = cmul(pb[i], m);
  }
}

// psi *= exp(b tau);  partial[b][block] = sum |psi|^2 (fixed partition, fixed order)
template <typename T>
__global__ __launch_bounds__(256) void rot_b_kernel(Cx<T>* __restrict__ psi, const T* __restrict__ dens,
                                                    const T* __restrict__ pot, int64_t pot_stride,
                                                    const EnvParams<T>* __restrict__ ep, T tr, T ti, int64_t cells,
                                                    double* __restrict__ partial) {
  const int b = blockIdx.y;
  Cx<T>* const pb = psi + (int64_t)b * cells;
  const T* const db = dens + (int64_t)b * cells;
  const T* const vb = pot ? pot + (int64_t)b * pot_stride : nullptr;
  const T kk = ep[b].gpe_k;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (int64_t)gridDim.x * 256) {
    const T w = (vb ? vb[i] : T(0)) + kk * db[i];
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

// ---- the stirred kernels: Omega(t) in the line coefficient, the spots at t in b ---------------------------------------

// rot_row_kernel with Omega(t) and the spots at t (sa.t) in b.
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

// rot_col_kernel with a local time per half: PRE (the second half of the step that started at t_pre)
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
  // one line operator with the coefficient a (as in rot_col_kernel, two in a row need no barrier in between)
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

// rot_mul_kernel with Omega(t)
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

// rot_b_kernel with the spots at sa.t in b
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

// ---- host: one copy, STIRRED picks the kernels and appends their arguments; t, t_pre and t_post are the local times a
// stirred launch passes on and a frozen one ignores ------------------------------------------------------------------

template <typename T, bool STIRRED, int N>
int launch_rot_row(pdeopt_ctx* ctx, const Window& w, GpeRot& gr, std::complex<double> tau, double t) {
  const pdeopt_problem& p = ctx->prob;
  const AuxField& pot = ctx->aux[PDEOPT_AUX_GPE_POTENTIAL];
  constexpr int F = rot_row_lines<T, N>();
  const size_t lds = (size_t)F * RegFft<T, N>::NP * sizeof(Cx<T>);
  const int64_t cells = (int64_t)p.nx * p.ny, w0 = w.lo;
  const int blocks = (int)((int64_t)w.n * p.nx / F);
  auto launch = [&](auto kern, auto... clock_args) -> int {
    int rc = allow_lds(ctx, kern, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), lds, w.stream, ctx->Y.as<Cx<T>>() + w0 * cells,
                       gr.dens.as<const T>() + w0 * cells,
                       pot.dev ? pot.dev.as<const T>() + (pot.per_env ? w0 * cells : 0) : nullptr,
                       pot.per_env ? cells : (int64_t)0, env_params<T>(ctx, w.lo), gr.tw_y.as<const Cx<T>>(),
                       gr.kin_y.as<const Cx<T>>(), (T)tau.real(), (T)tau.imag(), rot_axis<T>(ctx, 1, 0.5 * tau), p.nx,
                       gr.partial.as<double>() + w0 * gr.partial_per_env, clock_args...);
    ctx->n_stage_launches++;
    PDEOPT_HIP_CHECK(ctx, hipGetLastError());
    return PDEOPT_OK;
  };
  // a window's spot table and parameters start at its first environment
  if constexpr (STIRRED) return launch(rstir_row_kernel<T, N>, make_spot_args<T>(ctx, w.lo, t));
  else return launch(rot_row_kernel<T, N>);
}

// fp64 at N = 1024 runs JOIN as LAST + FIRST (3 passes per step): that one JOIN instantiation does not fit the
// register file (28 bytes of scratch per lane at 256 threads), every other one does; the stirred pass's second line
// coefficient costs no further instantiation
template <typename T, int N>
constexpr bool rot_join_fits() { return !(sizeof(T) == 8 && N == 1024); }

template <typename T, bool STIRRED, int N, bool PRE, bool POST>
int launch_rot_col(pdeopt_ctx* ctx, const Window& w, GpeRot& gr, std::complex<double> tau, double t_pre, double t_post) {
  if constexpr (PRE && POST && !rot_join_fits<T, N>()) {
    const int rc = launch_rot_col<T, STIRRED, N, true, false>(ctx, w, gr, tau, t_pre, t_post);
    return rc ? rc : launch_rot_col<T, STIRRED, N, false, true>(ctx, w, gr, tau, t_pre, t_post);
  } else {
    const pdeopt_problem& p = ctx->prob;
    constexpr int C = rot_cols<T, N>();
    const int64_t cells = (int64_t)p.nx * p.ny, w0 = w.lo;
    const size_t lds = (size_t)C * RegFft<T, N>::NP * sizeof(Cx<T>);
    auto launch = [&](auto kern, auto... clock_args) -> int {
      int rc = allow_lds(ctx, kern, lds);
      if (rc) return rc;
      hipLaunchKernelGGL(kern, dim3(p.ny / C, w.n), dim3(C * N / reg_default_pts<N>()), lds, w.stream,
                         ctx->Y.as<Cx<T>>() + w0 * cells, gr.dens.as<T>() + w0 * cells, env_params<T>(ctx, w.lo),
                         gr.tw_x.as<const Cx<T>>(), gr.kin_x.as<const Cx<T>>(), rot_axis<T>(ctx, 0, 0.5 * tau), p.ny,
                         gr.partial.as<const double>() + w0 * gr.partial_per_env, gr.partial_per_env,
                         ctx->strang_dx * ctx->strang_dx, clock_args...);
      ctx->n_stage_launches++;
      PDEOPT_HIP_CHECK(ctx, hipGetLastError());
      return PDEOPT_OK;
    };
    if constexpr (STIRRED) return launch(rstir_col_kernel<T, N, C, PRE, POST>, (T)t_pre, (T)t_post);
    else return launch(rot_col_kernel<T, N, C, PRE, POST>);
  }
}

template <typename T, bool STIRRED>
int rot_row_dispatch(pdeopt_ctx* ctx, const Window& w, GpeRot& gr, std::complex<double> tau, double t) {
  switch (ctx->prob.ny) {
#define X(NN) case NN: return launch_rot_row<T, STIRRED, NN>(ctx, w, gr, tau, t);
    PDEOPT_ROT_SIZES(X)
#undef X
    default: return fail(ctx, PDEOPT_EINVAL, "rotating split step: ny=%d is not covered", ctx->prob.ny);
  }
}
template <typename T, bool STIRRED, bool PRE, bool POST>
int rot_col_dispatch(pdeopt_ctx* ctx, const Window& w, GpeRot& gr, std::complex<double> tau, double t_pre, double t_post) {
  switch (ctx->prob.nx) {
#define X(NN) case NN: return launch_rot_col<T, STIRRED, NN, PRE, POST>(ctx, w, gr, tau, t_pre, t_post);
    PDEOPT_ROT_SIZES(X)
#undef X
    default: return fail(ctx, PDEOPT_EINVAL, "rotating split step: nx=%d is not covered", ctx->prob.nx);
  }
}

// one substep from local time t on rocFFT's 1-D plans, whole batch
template <typename T, bool STIRRED>
int rot_library_step(pdeopt_ctx* ctx, GpeRot& gr, std::complex<double> tau, double t) {
  const pdeopt_problem& p = ctx->prob;
  const int64_t cells = (int64_t)p.nx * p.ny, total = cells * p.batch;
  const AuxField& pot = ctx->aux[PDEOPT_AUX_GPE_POTENTIAL];
  const int g1 = (int)std::min<int64_t>(4096, (cells + 255) / 256);
  const dim3 mgrid(g1, p.batch);
  const EnvParams<T>* ep = env_params<T>(ctx, 0);
  const double dx2 = ctx->strang_dx * ctx->strang_dx;
  Cx<T>* const y = ctx->Y.as<Cx<T>>();
  int rc;
  // one line operator along `axis`: transform, multiply (scaled: by the norm's scale too), transform back
  auto line = [&](auto axis, auto scaled) -> int {
    constexpr int A = decltype(axis)::value;
    constexpr bool S = decltype(scaled)::value;
    int r = spectral_c2c_axis(ctx, A, true, y);
    if (r) return r;
    auto launch = [&](auto kern, auto... clock_args) {
      hipLaunchKernelGGL(kern, mgrid, dim3(256), 0, ctx->stream, y, (const Cx<T>*)(A == 0 ? gr.kin_x.get() : gr.kin_y.get()), ep,
                         rot_axis<T>(ctx, A, 0.5 * tau), p.nx, p.ny, S ? gr.partial.as<const double>() : nullptr,
                         S ? kLibNormBlocks : 0, dx2, clock_args...);
    };
    if constexpr (STIRRED) launch(rstir_mul_kernel<T, A, S>, (T)t);
    else launch(rot_mul_kernel<T, A, S>);
    return spectral_c2c_axis(ctx, A, false, y);
  };
  constexpr std::integral_constant<int, 0> along_x{};
  constexpr std::integral_constant<int, 1> along_y{};
  hipLaunchKernelGGL(rot_density_kernel<T>, dim3((int)std::min<int64_t>(4096, (total + 255) / 256)), dim3(256), 0,
                     ctx->stream, (const Cx<T>*)y, gr.dens.as<T>(), total);
  if ((rc = line(along_x, std::false_type{}))) return rc;
  if ((rc = line(along_y, std::false_type{}))) return rc;
  auto launch_b = [&](auto kern, auto... clock_args) {
    hipLaunchKernelGGL(kern, dim3(kLibNormBlocks, p.batch), dim3(256), 0, ctx->stream, y, gr.dens.as<const T>(),
                       pot.dev.as<const T>(), pot.per_env ? cells : (int64_t)0, ep, (T)tau.real(), (T)tau.imag(), cells,
                       clock_args...);
  };
  if constexpr (STIRRED) launch_b(rstir_b_kernel<T>, p.ny, gr.partial.as<double>(), make_spot_args<T>(ctx, 0, t));
  else launch_b(rot_b_kernel<T>, gr.partial.as<double>());
  if ((rc = line(along_y, std::false_type{}))) return rc;
  if ((rc = line(along_x, std::true_type{}))) return rc;
  ctx->n_stage_launches += 6;
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  return PDEOPT_OK;
}

// buffers, twiddles and the kinetic tables of a step of dt (rebuilt when dt, time_scale or the mesh changed)
template <typename T>
int rot_prepare_t(pdeopt_ctx* ctx, double dt, bool* fused_out) {
  GpeRot& gr = ctx->features.ensure<GpeRot>(FS_GPE_ROT);
  const pdeopt_problem& p = ctx->prob;
  const int64_t cells = (int64_t)p.nx * p.ny;
  const bool fused = ctx->opt_kernel_path != 1 && rot_size_ok(p.nx) && rot_size_ok(p.ny);
  *fused_out = fused;
  int rc;
  if (!gr.dens) {
    if (fused) {
      if ((rc = upload_table<T>(ctx, gr.tw_x, p.nx))) return rc;
      if ((rc = upload_table<T>(ctx, gr.tw_y, p.ny))) return rc;
    }
    if ((rc = ensure_buffer(ctx, gr.dens, (size_t)cells * p.batch * sizeof(T)))) return rc;
    const size_t np = (size_t)std::max(p.nx, kLibNormBlocks);
    if ((rc = ensure_buffer(ctx, gr.partial, sizeof(double) * (size_t)p.batch * np))) return rc;
  }
  if (fused && !gr.tw_x) {  // the library path ran first (PDEOPT_OPT_KERNEL_PATH changed in between)
    if ((rc = upload_table<T>(ctx, gr.tw_x, p.nx))) return rc;
    if ((rc = upload_table<T>(ctx, gr.tw_y, p.ny))) return rc;
  }
  gr.partial_per_env = fused ? p.nx / rot_row_lines_rt(p.ny) : kLibNormBlocks;
  const std::complex<double> tau = dt * std::complex<double>(ctx->ts_re, ctx->ts_im);
  if (!gr.valid || gr.key_dt != dt || gr.key_tr != ctx->ts_re || gr.key_ti != ctx->ts_im || gr.key_hx != p.hx ||
      gr.key_hy != p.hy) {
    if ((rc = upload_kinetic<T>(ctx, gr.kin_x, p.nx, p.hx, 0.5 * tau))) return rc;
    if ((rc = upload_kinetic<T>(ctx, gr.kin_y, p.ny, p.hy, 0.5 * tau))) return rc;
    gr.valid = true;
    gr.key_dt = dt;
    gr.key_tr = ctx->ts_re;
    gr.key_ti = ctx->ts_im;
    gr.key_hx = p.hx;
    gr.key_hy = p.hy;
  }
  return PDEOPT_OK;
}

// n steps from local time t0
template <typename T, bool STIRRED>
int strang_rot_t(pdeopt_ctx* ctx, double t0, double dt, int64_t n) {
  bool fused;
  int rc = rot_prepare_t<T>(ctx, dt, &fused);
  if (rc) return rc;
  GpeRot& gr = *ctx->features.get<GpeRot>(FS_GPE_ROT);
  const pdeopt_problem& p = ctx->prob;
  const int64_t cells = (int64_t)p.nx * p.ny;
  const std::complex<double> tau = dt * std::complex<double>(ctx->ts_re, ctx->ts_im);
  const auto t_of = [&](int64_t s) { return t0 + (double)s * dt; };  // the local time of pdeopt_advance's substep s
  if (!fused) {
    for (int64_t s = 0; s < n; ++s)
      if ((rc = rot_library_step<T, STIRRED>(ctx, gr, tau, t_of(s)))) return rc;
    ctx->last_kernel = STIRRED ? "strang_rot_stir_rocfft_1d" : "strang_rot_rocfft_1d";
    return PDEOPT_OK;
  }
  // environments are independent: the n-step pipeline group by group, a group's wavefunction + density sized to
  // stay in the Infinity Cache between its passes (as the non-rotating fused step)
  int group = p.batch;
  if (ctx->opt_group_envs > 0)
    group = (int)std::min<int64_t>(ctx->opt_group_envs, p.batch);
  else if (ctx->opt_group_envs == 0 && n > 1)
    group = cache_group(p.batch, (size_t)cells * (sizeof(Cx<T>) + sizeof(T)), 192ull << 20, false);
  auto first = [&](const Window& w) -> int { return rot_col_dispatch<T, STIRRED, false, true>(ctx, w, gr, tau, t_of(0), t_of(0)); };
  auto substep = [&](const Window& w, int64_t s, int&) -> int {
    int r;
    if ((r = rot_row_dispatch<T, STIRRED>(ctx, w, gr, tau, t_of(s)))) return r;
    return s + 1 < n ? rot_col_dispatch<T, STIRRED, true, true>(ctx, w, gr, tau, t_of(s), t_of(s + 1))
                     : rot_col_dispatch<T, STIRRED, true, false>(ctx, w, gr, tau, t_of(s), t_of(s));
  };
  if ((rc = run_groups(ctx, group, false, 0, n, first, substep))) return rc;
  ctx->last_kernel = STIRRED ? "strang_rot_stir_fused_lds_fft" : "strang_rot_fused_lds_fft";
  return PDEOPT_OK;
}

}  // namespace

int advance_strang_rot(pdeopt_ctx* ctx, double t0, double dt, int64_t n) {
  if (!ctx->rot_set)
    return fail(ctx, PDEOPT_ESTATE, "the rotating-frame split step needs pdeopt_set_gpe_rotation (Omega and the mesh origin)");
  if (has_time_aux(ctx, PDEOPT_AUX_GPE_POTENTIAL))
    return fail(ctx, PDEOPT_EINVAL, "the rotating-frame split step takes a static potential plus Gaussian light spots "
                                    "(pdeopt_set_gpe_spots), no host-sampled potential");
  // light spots or a rotation ramp: the stirred kernels; without either, the frozen ones, whose results do not change
  const bool stirred = ctx->n_spots || ctx->rot_any_rate;
  return with_dtype(ctx, [&](auto t) {
    using T = decltype(t);
    return stirred ? strang_rot_t<T, true>(ctx, t0, dt, n) : strang_rot_t<T, false>(ctx, t0, dt, n);
  });
}

}  // namespace pdeopt
