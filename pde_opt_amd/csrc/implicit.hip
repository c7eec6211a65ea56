// Implicit Euler by matrix-free Newton-GMRES (PDEOPT_INT_IMPLICIT_EULER): the counterpart of
// diffrax.ImplicitEuler with a Newton root-find and lineax.GMRES inside (upstream's notebooks/test_implicit.ipynb), for
// the periodic 2-D Cahn-Hilliard and Allen-Cahn equations with finite differences.
//
// One step solves G(y) = y - y0 - dt f(y) = 0 per environment.
//   Newton   first iterate y0; G and the fp64 partials of |G|^2, |y|^2 in one pass over f = the forward right-hand side
//            (launch_rhs); one wave per environment adds the partials and decides: rms(G) <= atol + rtol rms(y) freezes
//            the environment, otherwise it sets up the linear solve (beta = |G|, the scale -1 / beta of the first
//            basis vector, the tolerance krylov_rtol beta).
//   GMRES    (I - dt J_f(y)) delta = -G, restarted every m iterations.  Iteration j:
//              op        w = v - dt J v, v = scale x (the previous iteration's w, or -G / the restart residual): the
//                        normalisation of v_j is folded into the read, the kernel stores v_j as it goes by
//              dots      all j + 1 products <w, v_i> in one launch that reads w once; fp64 partials per workgroup
//              update    every workgroup adds the partials in one fixed order, w -= sum h_i v_i, partials of |w|^2
//              dots, update again: classical Gram-Schmidt with one re-orthogonalisation (CGS2)
//              small     one wave per environment: h_{j+1,j} = |w|, Givens rotations, residual estimate, the flag
//                        LIN_CONV, 1 / |w| for the next op; the triangular solve when the environment's cycle ends
//            cycle end  delta (+)= V y_k and, where the linear solve has converged, y += delta, in one launch;
//            restart    r = -G - (I - dt J) delta for the environments that have not converged (one op on delta).
// With the spectral preconditioner (pdeopt_implicit_set_precond; off by default) the solve is right-preconditioned:
// iteration j forms z_j = M^-1 v_j (r2c, one multiply that also carries the normalisation and the 1 / N, c2r) and
// w = A z_j, the operator storing v_j from the raw field; a cycle ends with delta (+)= M^-1 (V y_k).  The residual
// estimate is still that of the original system.  Off, the launches and the bits are those of the lines above.
// The host reads the B flags back once per iteration (4 B bytes) to know when every environment is done.  Environments
// run in lockstep but converge independently: every kernel returns at once for a frozen environment (flags != 0), whose
// vectors are then neither normalised nor updated; an environment's arithmetic does not depend on the batch it is in.
// No atomics, nothing waits on another workgroup; flags and small systems are written by the one-wave kernels only,
// which run as launches of their own, so no field kernel reads a word another workgroup of the same launch writes.
#include <algorithm>
#include <cmath>

#include "block_sums.hpp"
#include "closures.hpp"
#include "common.hpp"
#include "sens_tile.hpp"

namespace pdeopt {

constexpr int kImpMaxRestart = 64;
constexpr int kImpCellsPerThread = 8, kImpChunk = 256 * kImpCellsPerThread;  // cells per workgroup of the vector kernels
constexpr int kImpDotCols = 8;                                                // products per sweep over w's registers
enum : int { IMP_NEWTON_DONE = 1, IMP_LIN_CONV = 2, IMP_FAIL = 4 };

// per-environment words and small systems on the device, m = restart
struct ImpSmall {
  double* part_dot;  // [B][m][nblk]  workgroup partials of <w, v_i>
  double* part_nrm;  // [B][2][nblk]  workgroup partials of |w|^2 (row 0; Newton: |G|^2) and |y|^2 (row 1)
  double* hcol;      // [B][m]        the column being built: h_i of pass 1 + pass 2
  double* R;         // [B][m][m]     the rotated upper triangle, column j at [j][i]
  double* cs;        // [B][m]
  double* sn;        // [B][m]
  double* g;         // [B][m + 1]    the rotated right-hand side
  double* ycoef;     // [B][m]        solution of the triangular system
  double* gnorm;     // [B]           |G|_2 of the Newton iterate
  double* tol;       // [B]           krylov_rtol |G|_2
  double* vscale;    // [B]           factor the next op applies to its source
  double* res;       // [B]           last residual: rms(G) after a Newton check, the GMRES estimate inside a linear solve
  int* flags;        // [B]
  int* kcols;        // [B]           columns of this cycle's triangular system
  int* conv_cycle;   // [B]           cycle in which LIN_CONV was set (the cycle-end launch applies delta once)
  int m, nblk;
};

// coefficients and tables of the spectral preconditioner
struct ImpPrecond {
  double* part;   // [B][2][nblk]  workgroup partials of sum D mu_h' (row 0) and sum D (row 1)
  double* coef;   // [B][2]        a_b (clamped), c_b
  double* sin2x;  // [nx]          sin^2(pi kx / nx)
  double* sin2y;  // [ny / 2 + 1]  sin^2(pi ky / ny)
};

struct Implicit : Feature {
  double rtol = 0, atol = 0, krylov_rtol = 0;
  int restart = 0, max_newton = 0, max_krylov = 0;
  int B = 0, nblk = 0;
  int64_t cells = 0;
  DeviceBuffer fields;  // Y0 | G | DELTA | W0 | W1 | V[restart], each [B][cells] in the problem dtype
  size_t field_bytes = 0;  // one of them
  DeviceBuffer small_blk;
  ImpSmall sm{};
  PinnedBuffer flags_host;  // ints
  PinnedBuffer res_host;    // doubles
  // pdeopt_implicit_set_precond: 0 none, 1 spectral.  The workspace of the preconditioner is one more field of the batch
  // and the small block below; the hermitian work field and the plans are spectral.hip's
  int precond = 0;
  DeviceBuffer zfield;  // [B][cells]: z_j = M^-1 v_j of an iteration, V y_k at a cycle's end
  DeviceBuffer pc_blk;
  ImpPrecond pc{};
  void* hbuf = nullptr;    // borrowed (spectral_real_prepare)
  int64_t half_cells = 0;
  std::vector<int64_t> pc_count;   // [B] applications of M^-1 inside the steps since configure
  std::vector<char> lin_applied;   // [B] this linear solve's delta has been added to y
};
// nullptr until pdeopt_implicit_configure
inline Implicit* implicit_of(const pdeopt_ctx* ctx) { return ctx->features.get<Implicit>(FS_IMPLICIT); }

namespace {

// ---- operator application: w = v - dt J_f(y) v, v = scale[b] x src ------------------------------------------------------
template <typename T>
struct ImpOpArgs {
  const T* y;
  const T* src;
  const T* raw;         // preconditioned operator only: the field v_j = scale x raw is formed from (src is then z_j = M^-1 v_j)
  T* vout;              // v as formed (the basis vector v_j); nullptr: not stored
  T* wout;
  const double* scale;  // [B] or nullptr (1)
  const int* flags;     // [B] or nullptr: environments with flags != 0 are skipped
  const EnvParams<T>* ep;
  ClosureSpec mu, mob;
  int nx, ny;
  T rhx, rhy, rhx2, rhy2;
  T dt;
};

// Cahn-Hilliard: J v = div( avg(D'(u) v) grad(mu) + avg(D(u)) grad(mu_h'(u) v - kappa lap v) ), mu = mu_h(u) - kappa lap u:
// the tangent kernel of sens.hip with one tangent and no coefficient term.  u and v on the tile + 2-cell ring, the four
// face quantities on the tile + 1-cell ring; mu_h' and D' live in the registers of the thread that forms dmu and dD
// PRE (right preconditioning): the source is z_j, read as it is, and the basis vector stored for the tile is scale x raw
template <typename T, bool PRE>
__device__ __forceinline__ void imp_op_ch_body(const ImpOpArgs<T>& a) {
  __shared__ T su[kR2 * kC2], sv[kR2 * kC2];
  __shared__ T smu[kR1 * kC1], sD[kR1 * kC1], sdmu[kR1 * kC1], sdD[kR1 * kC1];
  const int b = blockIdx.z;
  if (a.flags && a.flags[b]) return;
  const int tid = threadIdx.x;
  const int i0 = blockIdx.y * kTR, j0 = blockIdx.x * kTC;
  const int nx = a.nx, ny = a.ny;
  const int64_t cells = (int64_t)nx * ny;
  const EnvParams<T>& ep = a.ep[b];
  const T kappa = ep.kappa;
  const T sc = a.scale ? T(a.scale[b]) : T(1);
  const T* __restrict__ u = a.y + (int64_t)b * cells;
  const T* __restrict__ s = a.src + (int64_t)b * cells;
  for (int q = tid; q < kR2 * kC2; q += 256) {
    const int r = q / kC2, c = q - r * kC2;
    const int64_t g = (int64_t)wrap_idx(i0 + r - 2, nx) * ny + wrap_idx(j0 + c - 2, ny);
    su[q] = u[g];
    sv[q] = PRE ? s[g] : sc * s[g];
  }
  __syncthreads();
  for (int q = tid; q < kR1 * kC1; q += 256) {
    const int r = q / kC1, c = q - r * kC1;
    const int o = (r + 1) * kC2 + (c + 1);
    const T uc = su[o], vc = sv[o];
    const T muh = closure_generic<T>(a.mu, ep.mu, uc);
    const T D = closure_generic<T>(a.mob, ep.mob, uc);
    smu[q] = muh - kappa * tile_lap5<T>(su, o, kC2, a.rhx2, a.rhy2);
    sD[q] = D;
    sdmu[q] = closure_dc<T>(a.mu, ep.mu, uc, muh) * vc - kappa * tile_lap5<T>(sv, o, kC2, a.rhx2, a.rhy2);
    sdD[q] = closure_dc<T>(a.mob, ep.mob, uc, D) * vc;
  }
  __syncthreads();
  T* __restrict__ vout = a.vout ? a.vout + (int64_t)b * cells : nullptr;
  T* __restrict__ wout = a.wout + (int64_t)b * cells;
  for (int q = tid; q < kTR * kTC; q += 256) {
    const int r = q / kTC, c = q - r * kTC;
    const int gi = i0 + r, gj = j0 + c;
    if (gi >= nx || gj >= ny) continue;
    const int o = (r + 1) * kC1 + (c + 1);
    const T fxp = tile_tangent_flux<T>(smu, sD, sdmu, sdD, o, o + kC1, a.rhx);
    const T fxm = tile_tangent_flux<T>(smu, sD, sdmu, sdD, o - kC1, o, a.rhx);
    const T fyp = tile_tangent_flux<T>(smu, sD, sdmu, sdD, o, o + 1, a.rhy);
    const T fym = tile_tangent_flux<T>(smu, sD, sdmu, sdD, o - 1, o, a.rhy);
    const T jv = (fxp - fxm) * a.rhx + (fyp - fym) * a.rhy;
    const T v = sv[(r + 2) * kC2 + (c + 2)];
    const int64_t g = (int64_t)gi * ny + gj;
    if (vout) vout[g] = PRE ? sc * a.raw[(int64_t)b * cells + g] : v;
    wout[g] = v - a.dt * jv;
  }
}
template <typename T>
__global__ __launch_bounds__(256) void imp_op_ch_kernel(ImpOpArgs<T> a) {
  imp_op_ch_body<T, false>(a);
}
template <typename T>
__global__ __launch_bounds__(256) void precond_op_ch_kernel(ImpOpArgs<T> a) {
  imp_op_ch_body<T, true>(a);
}

// Allen-Cahn: J v = -R'(u) v m - R(u) (mu_h'(u) v - kappa lap v), m = mu_h(u) - kappa lap u.  Radius 1: u and v on the
// tile + 1-cell ring, everything else in registers
template <typename T, bool PRE>
__device__ __forceinline__ void imp_op_ac_body(const ImpOpArgs<T>& a) {
  __shared__ T su[kR1 * kC1], sv[kR1 * kC1];
  const int b = blockIdx.z;
  if (a.flags && a.flags[b]) return;
  const int tid = threadIdx.x;
  const int i0 = blockIdx.y * kTR, j0 = blockIdx.x * kTC;
  const int nx = a.nx, ny = a.ny;
  const int64_t cells = (int64_t)nx * ny;
  const EnvParams<T>& ep = a.ep[b];
  const T kappa = ep.kappa;
  const T sc = a.scale ? T(a.scale[b]) : T(1);
  const T* __restrict__ u = a.y + (int64_t)b * cells;
  const T* __restrict__ s = a.src + (int64_t)b * cells;
  for (int q = tid; q < kR1 * kC1; q += 256) {
    const int r = q / kC1, c = q - r * kC1;
    const int64_t g = (int64_t)wrap_idx(i0 + r - 1, nx) * ny + wrap_idx(j0 + c - 1, ny);
    su[q] = u[g];
    sv[q] = PRE ? s[g] : sc * s[g];
  }
  __syncthreads();
  T* __restrict__ vout = a.vout ? a.vout + (int64_t)b * cells : nullptr;
  T* __restrict__ wout = a.wout + (int64_t)b * cells;
  for (int q = tid; q < kTR * kTC; q += 256) {
    const int r = q / kTC, c = q - r * kTC;
    const int gi = i0 + r, gj = j0 + c;
    if (gi >= nx || gj >= ny) continue;
    const int o = (r + 1) * kC1 + (c + 1);
    const T uc = su[o], vc = sv[o];
    const T muh = closure_generic<T>(a.mu, ep.mu, uc);
    const T R = closure_generic<T>(a.mob, ep.mob, uc);
    const T m = muh - kappa * tile_lap5<T>(su, o, kC1, a.rhx2, a.rhy2);
    const T dmu = closure_dc<T>(a.mu, ep.mu, uc, muh) * vc - kappa * tile_lap5<T>(sv, o, kC1, a.rhx2, a.rhy2);
    const T dR = closure_dc<T>(a.mob, ep.mob, uc, R) * vc;
    const T jv = -(dR * m) - R * dmu;
    const int64_t g = (int64_t)gi * ny + gj;
    if (vout) vout[g] = PRE ? sc * a.raw[(int64_t)b * cells + g] : vc;
    wout[g] = vc - a.dt * jv;
  }
}
template <typename T>
__global__ __launch_bounds__(256) void imp_op_ac_kernel(ImpOpArgs<T> a) {
  imp_op_ac_body<T, false>(a);
}
template <typename T>
__global__ __launch_bounds__(256) void precond_op_ac_kernel(ImpOpArgs<T> a) {
  imp_op_ac_body<T, true>(a);
}

// ---- vector kernels: grid (nblk, B), 256 threads, workgroup blk owns the cells [blk kImpChunk, (blk + 1) kImpChunk) ----

// this thread's cell m of the workgroup's chunk
__device__ __forceinline__ int64_t imp_cell(int m) {
  return (int64_t)blockIdx.x * kImpChunk + m * 256 + threadIdx.x;
}

// Newton residual G = y - y0 - dt f and the partials of |G|^2 and |y|^2
template <typename T>
__global__ __launch_bounds__(256) void imp_residual_kernel(const T* __restrict__ y, const T* __restrict__ y0, const T* __restrict__ f,
                                                         T* __restrict__ G, T dt, int64_t cells, ImpSmall sm) {
  __shared__ double sh[4];
  const int b = blockIdx.y;
  if (sm.flags[b] & (IMP_NEWTON_DONE | IMP_FAIL)) return;
  const int64_t base = (int64_t)b * cells;
  double g2 = 0.0, y2 = 0.0;
#pragma unroll
  for (int m = 0; m < kImpCellsPerThread; ++m) {
    const int64_t c = imp_cell(m);
    if (c < cells) {
      const T yv = y[base + c];
      const T gv = (yv - y0[base + c]) - dt * f[base + c];
      G[base + c] = gv;
      g2 += (double)gv * (double)gv;
      y2 += (double)yv * (double)yv;
    }
  }
  g2 = block_sum(g2, sh);
  y2 = block_sum(y2, sh);
  if (threadIdx.x == 0) {
    sm.part_nrm[((int64_t)b * 2 + 0) * sm.nblk + blockIdx.x] = g2;
    sm.part_nrm[((int64_t)b * 2 + 1) * sm.nblk + blockIdx.x] = y2;
  }
}

// one wave: the sum of row `row` of an environment's norm partials, in lane 0
__device__ __forceinline__ double imp_norm_total(const ImpSmall& sm, int b, int row) {
  const double* p = sm.part_nrm + ((int64_t)b * 2 + row) * sm.nblk;
  double s = 0.0;
  for (int q = threadIdx.x; q < sm.nblk; q += 64) s += p[q];
  return wave_sum(s);
}

// grid B, one wave: the Newton decision of an environment
__global__ __launch_bounds__(64) void imp_newton_small_kernel(ImpSmall sm, double cells, double rtol, double atol, double krylov_rtol,
                                                            int newton_it, int max_newton) {
  const int b = blockIdx.x;
  if (sm.flags[b] & (IMP_NEWTON_DONE | IMP_FAIL)) return;
  const double g2 = imp_norm_total(sm, b, 0), y2 = imp_norm_total(sm, b, 1);
  if (threadIdx.x != 0) return;
  const double rms_g = sqrt(g2 / cells), thr = atol + rtol * sqrt(y2 / cells);
  sm.res[b] = rms_g;
  sm.tol[b] = thr;  // the host's message quotes it when the budget runs out
  if (rms_g <= thr) {
    sm.flags[b] = IMP_NEWTON_DONE;
  } else if (!(g2 > 0.0) || !isfinite(g2) || newton_it >= max_newton) {
    sm.flags[b] = IMP_FAIL;  // a residual that is not a number, or the budget of linear solves is spent
  } else {
    const double beta = sqrt(g2);
    sm.gnorm[b] = beta;
    sm.tol[b] = krylov_rtol * beta;
    sm.vscale[b] = -1.0 / beta;  // v_0 = -G / |G|
    sm.g[(int64_t)b * (sm.m + 1)] = beta;
    sm.kcols[b] = 0;
    sm.conv_cycle[b] = -1;
    sm.flags[b] = 0;
  }
}

template <typename T>
struct ImpVecArgs {
  T* w;          // [B][cells]
  const T* V;    // [m][B][cells]
  T* y;          // solution launch
  T* delta;
  const T* G;    // restart launch
  int64_t cells;
  int B, ncols;  // products of this launch: <w, v_i>, i < ncols
  int pass;      // update: 0 first Gram-Schmidt pass, 1 the re-orthogonalisation
  int cycle;
  ImpSmall sm;
};

// <w, v_i> for i < ncols: w's cells stay in registers, the basis vectors stream past them kImpDotCols at a time
template <typename T>
__global__ __launch_bounds__(256) void imp_dots_kernel(ImpVecArgs<T> a) {
  __shared__ double red[4][kImpDotCols];
  const int b = blockIdx.y;
  if (a.sm.flags[b]) return;
  const int tid = threadIdx.x;
  const int64_t cells = a.cells;
  const T* __restrict__ w = a.w + (int64_t)b * cells;
  double wv[kImpCellsPerThread];
#pragma unroll
  for (int m = 0; m < kImpCellsPerThread; ++m) {
    const int64_t c = imp_cell(m);
    wv[m] = c < cells ? (double)w[c] : 0.0;
  }
  for (int i0 = 0; i0 < a.ncols; i0 += kImpDotCols) {
    double acc[kImpDotCols];
#pragma unroll
    for (int q = 0; q < kImpDotCols; ++q) {
      acc[q] = 0.0;
      if (i0 + q < a.ncols) {
        const T* __restrict__ v = a.V + ((int64_t)(i0 + q) * a.B + b) * cells;
#pragma unroll
        for (int m = 0; m < kImpCellsPerThread; ++m) {
          const int64_t c = imp_cell(m);
          if (c < cells) acc[q] += wv[m] * (double)v[c];
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) acc[q] += __shfl_down(acc[q], o, 64);
    }
    if ((tid & 63) == 0) {
#pragma unroll
      for (int q = 0; q < kImpDotCols; ++q) red[tid >> 6][q] = acc[q];
    }
    __syncthreads();
    if (tid < kImpDotCols && i0 + tid < a.ncols)
      a.sm.part_dot[((int64_t)b * a.sm.m + i0 + tid) * a.sm.nblk + blockIdx.x] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
    __syncthreads();  // red is written again by the next sweep
  }
}

// h_i = the partials of <w, v_i> added in one fixed order (every workgroup forms the same bits); w -= sum h_i v_i; the
// partial of |w|^2.  Workgroup 0 of the environment records the column for the small system
template <typename T>
__global__ __launch_bounds__(256) void imp_update_kernel(ImpVecArgs<T> a) {
  __shared__ double sh_h[kImpMaxRestart];
  __shared__ double sh[4];
  const int b = blockIdx.y;
  if (a.sm.flags[b]) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nblk = a.sm.nblk;
  for (int i = wave; i < a.ncols; i += 4) {
    const double* p = a.sm.part_dot + ((int64_t)b * a.sm.m + i) * nblk;
    double s = 0.0;
    for (int q = lane; q < nblk; q += 64) s += p[q];
    s = wave_sum(s);
    if (lane == 0) sh_h[i] = s;
  }
  __syncthreads();
  if (blockIdx.x == 0 && tid < a.ncols) {
    double* h = a.sm.hcol + (int64_t)b * a.sm.m + tid;
    *h = a.pass ? *h + sh_h[tid] : sh_h[tid];
  }
  const int64_t cells = a.cells;
  T* __restrict__ w = a.w + (int64_t)b * cells;
  double wv[kImpCellsPerThread];
#pragma unroll
  for (int m = 0; m < kImpCellsPerThread; ++m) {
    const int64_t c = imp_cell(m);
    wv[m] = c < cells ? (double)w[c] : 0.0;
  }
  for (int i = 0; i < a.ncols; ++i) {
    const T* __restrict__ v = a.V + ((int64_t)i * a.B + b) * cells;
    const double h = sh_h[i];
#pragma unroll
    for (int m = 0; m < kImpCellsPerThread; ++m) {
      const int64_t c = imp_cell(m);
      if (c < cells) wv[m] -= h * (double)v[c];
    }
  }
  double n2 = 0.0;
#pragma unroll
  for (int m = 0; m < kImpCellsPerThread; ++m) {
    const int64_t c = imp_cell(m);
    if (c < cells) {
      const T r = (T)wv[m];
      w[c] = r;
      n2 += (double)r * (double)r;
    }
  }
  n2 = block_sum(n2, sh);
  if (tid == 0) a.sm.part_nrm[(int64_t)b * 2 * nblk + blockIdx.x] = n2;
}

// grid B, one wave: column j of the small system of an environment.  `last`: the cycle ends after this iteration
// whatever the estimate says (j + 1 = m, or the budget max_krylov is spent)
__global__ __launch_bounds__(64) void imp_gmres_small_kernel(ImpSmall sm, int j, int cycle, int last) {
  __shared__ double h[kImpMaxRestart + 1];
  const int b = blockIdx.x;
  if (sm.flags[b]) return;
  const int m = sm.m;
  const double n2 = imp_norm_total(sm, b, 0);
  if (threadIdx.x != 0) return;
  const double hn = sqrt(n2);
  for (int i = 0; i <= j; ++i) h[i] = sm.hcol[(int64_t)b * m + i];
  double* const cs = sm.cs + (int64_t)b * m;
  double* const sn = sm.sn + (int64_t)b * m;
  double* const g = sm.g + (int64_t)b * (m + 1);
  double* const Rj = sm.R + ((int64_t)b * m + j) * m;
  for (int i = 0; i < j; ++i) {
    const double t = cs[i] * h[i] + sn[i] * h[i + 1];
    h[i + 1] = -sn[i] * h[i] + cs[i] * h[i + 1];
    h[i] = t;
    Rj[i] = t;
  }
  // a zero h_{j+1,j} (the Krylov space is exhausted: the estimate below becomes 0) divides nothing
  const double den = sqrt(h[j] * h[j] + hn * hn);
  const double c = den > 0.0 ? h[j] / den : 1.0, s = den > 0.0 ? hn / den : 0.0;
  Rj[j] = den;
  cs[j] = c;
  sn[j] = s;
  const double gj = g[j];
  g[j] = c * gj;
  g[j + 1] = -s * gj;
  const double est = fabs(s * gj);
  sm.res[b] = est;
  sm.kcols[b] = j + 1;
  const bool conv = est <= sm.tol[b];
  if (conv) {
    sm.flags[b] = IMP_LIN_CONV;
    sm.conv_cycle[b] = cycle;
  } else {
    sm.vscale[b] = hn > 0.0 ? 1.0 / hn : 0.0;
  }
  if (conv || last) {
    double* const yk = sm.ycoef + (int64_t)b * m;
    for (int i = j; i >= 0; --i) {
      double t = g[i];
      for (int k = i + 1; k <= j; ++k) t -= sm.R[((int64_t)b * m + k) * m + i] * yk[k];
      const double d = sm.R[((int64_t)b * m + i) * m + i];
      yk[i] = d != 0.0 ? t / d : 0.0;
    }
  }
}

// end of a cycle: delta (+)= V y_k; where the environment's linear solve converged in this cycle, y += delta
template <typename T>
__global__ __launch_bounds__(256) void imp_solution_kernel(ImpVecArgs<T> a) {
  __shared__ double sh_y[kImpMaxRestart];
  const int b = blockIdx.y;
  const int fl = a.sm.flags[b];
  if (fl & (IMP_NEWTON_DONE | IMP_FAIL)) return;
  if ((fl & IMP_LIN_CONV) && a.sm.conv_cycle[b] < a.cycle) return;  // applied when it converged
  const int k = a.sm.kcols[b];
  if (threadIdx.x < k) sh_y[threadIdx.x] = a.sm.ycoef[(int64_t)b * a.sm.m + threadIdx.x];
  __syncthreads();
  const int64_t cells = a.cells;
  T* __restrict__ delta = a.delta + (int64_t)b * cells;
  double d[kImpCellsPerThread];
#pragma unroll
  for (int m = 0; m < kImpCellsPerThread; ++m) {
    const int64_t c = imp_cell(m);
    d[m] = (a.cycle > 0 && c < cells) ? (double)delta[c] : 0.0;
  }
  for (int i = 0; i < k; ++i) {
    const T* __restrict__ v = a.V + ((int64_t)i * a.B + b) * cells;
    const double yi = sh_y[i];
#pragma unroll
    for (int m = 0; m < kImpCellsPerThread; ++m) {
      const int64_t c = imp_cell(m);
      if (c < cells) d[m] += yi * (double)v[c];
    }
  }
  T* __restrict__ y = a.y + (int64_t)b * cells;
#pragma unroll
  for (int m = 0; m < kImpCellsPerThread; ++m) {
    const int64_t c = imp_cell(m);
    if (c < cells) {
      const T dv = (T)d[m];
      delta[c] = dv;
      if (fl & IMP_LIN_CONV) y[c] += dv;
    }
  }
}

// restart: w holds (I - dt J) delta; w = -G - w is the residual of the linear system, with the partial of its norm
template <typename T>
__global__ __launch_bounds__(256) void imp_restart_kernel(ImpVecArgs<T> a) {
  __shared__ double sh[4];
  const int b = blockIdx.y;
  if (a.sm.flags[b]) return;
  const int64_t cells = a.cells, base = (int64_t)b * cells;
  double n2 = 0.0;
#pragma unroll
  for (int m = 0; m < kImpCellsPerThread; ++m) {
    const int64_t c = imp_cell(m);
    if (c < cells) {
      const T r = -a.G[base + c] - a.w[base + c];
      a.w[base + c] = r;
      n2 += (double)r * (double)r;
    }
  }
  n2 = block_sum(n2, sh);
  if (threadIdx.x == 0) a.sm.part_nrm[(int64_t)b * 2 * a.sm.nblk + blockIdx.x] = n2;
}

__global__ __launch_bounds__(64) void imp_restart_small_kernel(ImpSmall sm, int cycle) {
  const int b = blockIdx.x;
  if (sm.flags[b]) return;
  const double n2 = imp_norm_total(sm, b, 0);
  if (threadIdx.x != 0) return;
  const double beta = sqrt(n2);
  sm.g[(int64_t)b * (sm.m + 1)] = beta;
  sm.kcols[b] = 0;
  sm.res[b] = beta;
  if (beta <= sm.tol[b]) {
    sm.flags[b] = IMP_LIN_CONV;
    sm.conv_cycle[b] = cycle;
  } else {
    sm.vscale[b] = 1.0 / beta;
  }
}

// ---- spectral preconditioner (pdeopt_implicit_set_precond) ------------------------------------------------------------
// M = the symbol of the constant-coefficient part of the finite-difference operator I - dt J at the Newton iterate:
//   s(kx, ky) = (4 / hx^2) sin^2(pi kx / nx) + (4 / hy^2) sin^2(pi ky / ny)   (the 5-point Laplacian is -s)
//   Cahn-Hilliard  M = 1 + dt s (a + c kappa s),  c = mean D(y),  a = max(mean(D(y) mu_h'(y)), 0)
//   Allen-Cahn     M = 1 + dt   (a + c kappa s),  c = mean R(y),  a = max(mean(R(y) mu_h'(y)), 0)
// M >= 1 and M(0) = 1 (Cahn-Hilliard), so M^-1 keeps the mean of what it is applied to.  M^-1 v = c2r( r2c(v) / (N M) )
// with the batched rocFFT plans of spectral.hip.  (These kernels' names do not start with imp_: the list of
// tests/test_kernel_budgets_implicit.py is the unpreconditioned solver's; theirs is tests/test_kernel_budgets_implicit_precond.py.)
template <typename T>
struct PrecondCoefArgs {
  const T* y;
  const int* flags;  // [B] or nullptr: environments with flags != 0 are skipped
  const EnvParams<T>* ep;
  ClosureSpec mu, mob;
  int64_t cells;
  int nblk;
  ImpPrecond pc;
};

// the two sums of an environment's coefficients, one fp64 partial per workgroup each (the layout of imp_residual_kernel)
template <typename T>
__global__ __launch_bounds__(256) void precond_coef_kernel(PrecondCoefArgs<T> a) {
  __shared__ double sh[4];
  const int b = blockIdx.y;
  if (a.flags && a.flags[b]) return;
  const EnvParams<T>& ep = a.ep[b];
  const T* __restrict__ y = a.y + (int64_t)b * a.cells;
  double sa = 0.0, sc = 0.0;
#pragma unroll
  for (int m = 0; m < kImpCellsPerThread; ++m) {
    const int64_t c = imp_cell(m);
    if (c < a.cells) {
      const T uc = y[c];
      const T muh = closure_generic<T>(a.mu, ep.mu, uc);
      const T D = closure_generic<T>(a.mob, ep.mob, uc);
      sa += (double)D * (double)closure_dc<T>(a.mu, ep.mu, uc, muh);
      sc += (double)D;
    }
  }
  sa = block_sum(sa, sh);
  sc = block_sum(sc, sh);
  if (threadIdx.x == 0) {
    a.pc.part[((int64_t)b * 2 + 0) * a.nblk + blockIdx.x] = sa;
    a.pc.part[((int64_t)b * 2 + 1) * a.nblk + blockIdx.x] = sc;
  }
}

// grid B, one wave: the partials added in the order of imp_norm_total, the means, the clamp
__global__ __launch_bounds__(64) void precond_coef_finish_kernel(ImpPrecond pc, const int* flags, int nblk, double cells) {
  const int b = blockIdx.x;
  if (flags && flags[b]) return;
  double t[2];
  for (int row = 0; row < 2; ++row) {
    const double* p = pc.part + ((int64_t)b * 2 + row) * nblk;
    double s = 0.0;
    for (int q = threadIdx.x; q < nblk; q += 64) s += p[q];
    t[row] = wave_sum(s);
  }
  if (threadIdx.x != 0) return;
  const double a = t[0] / cells;
  pc.coef[2 * b] = a > 0.0 ? a : 0.0;  // inside the spinodal region mu_h' < 0: M stays >= 1
  pc.coef[2 * b + 1] = t[1] / cells;
}

template <typename T>
struct PrecondMulArgs {
  T* h;                 // [B][nx][nyh] interleaved complex
  const double* scale;  // [B] or nullptr (1): the GMRES normalisation of the field that was transformed
  const int* flags;     // [B] or nullptr: every environment
  const int* conv_cycle;
  int cycle;            // < 0: an iteration (flags != 0 skips); >= 0: the end of this cycle (the rule of imp_solution_kernel)
  const EnvParams<T>* ep;
  ImpPrecond pc;
  int nx, nyh, ch;
  double dt, fx, fy, rn;  // fx = 4 / hx^2, fy = 4 / hy^2, rn = 1 / (nx ny): the transforms are unnormalised
};

// the environments the launches of a cycle's end work on
__device__ __forceinline__ bool imp_cycle_end_skips(int fl, const int* conv_cycle, int b, int cycle) {
  if (fl & (IMP_NEWTON_DONE | IMP_FAIL)) return true;
  return (fl & IMP_LIN_CONV) && conv_cycle[b] < cycle;  // applied when it converged
}

// half spectrum *= scale / (N M_b), the factor formed in fp64: grid (cells of the half spectrum / 256, B)
template <typename T>
__global__ __launch_bounds__(256) void precond_mul_kernel(PrecondMulArgs<T> a) {
  const int b = blockIdx.y;
  if (a.flags) {
    const int fl = a.flags[b];
    if (a.cycle < 0 ? fl != 0 : imp_cycle_end_skips(fl, a.conv_cycle, b, a.cycle)) return;
  }
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t hc = (int64_t)a.nx * a.nyh;
  if (q >= hc) return;
  const int kx = (int)(q / a.nyh), ky = (int)(q - (int64_t)kx * a.nyh);
  const double s = a.fx * a.pc.sin2x[kx] + a.fy * a.pc.sin2y[ky];
  const double ab = a.pc.coef[2 * b], cb = a.pc.coef[2 * b + 1];
  const double lin = ab + cb * (double)a.ep[b].kappa * s;
  const double M = 1.0 + a.dt * (a.ch ? s * lin : lin);
  const T f = (T)((a.scale ? a.scale[b] : 1.0) * a.rn / M);
  T* __restrict__ h = a.h + ((int64_t)b * hc + q) * 2;
  h[0] *= f;
  h[1] *= f;
}

// end of a cycle, preconditioned: z = V y_k (precond_combine_kernel), z <- M^-1 z, then delta (+)= z and, where the
// linear solve converged in this cycle, y += delta (precond_add_kernel): imp_solution_kernel cut in two
template <typename T>
__global__ __launch_bounds__(256) void precond_combine_kernel(ImpVecArgs<T> a) {
  __shared__ double sh_y[kImpMaxRestart];
  const int b = blockIdx.y;
  if (imp_cycle_end_skips(a.sm.flags[b], a.sm.conv_cycle, b, a.cycle)) return;
  const int k = a.sm.kcols[b];
  if (threadIdx.x < k) sh_y[threadIdx.x] = a.sm.ycoef[(int64_t)b * a.sm.m + threadIdx.x];
  __syncthreads();
  const int64_t cells = a.cells;
  double d[kImpCellsPerThread];
#pragma unroll
  for (int m = 0; m < kImpCellsPerThread; ++m) d[m] = 0.0;
  for (int i = 0; i < k; ++i) {
    const T* __restrict__ v = a.V + ((int64_t)i * a.B + b) * cells;
    const double yi = sh_y[i];
#pragma unroll
    for (int m = 0; m < kImpCellsPerThread; ++m) {
      const int64_t c = imp_cell(m);
      if (c < cells) d[m] += yi * (double)v[c];
    }
  }
  T* __restrict__ z = a.w + (int64_t)b * cells;
#pragma unroll
  for (int m = 0; m < kImpCellsPerThread; ++m) {
    const int64_t c = imp_cell(m);
    if (c < cells) z[c] = (T)d[m];
  }
}

template <typename T>
__global__ __launch_bounds__(256) void precond_add_kernel(ImpVecArgs<T> a) {
  const int b = blockIdx.y;
  const int fl = a.sm.flags[b];
  if (imp_cycle_end_skips(fl, a.sm.conv_cycle, b, a.cycle)) return;
  const int64_t cells = a.cells;
  const T* __restrict__ z = a.w + (int64_t)b * cells;
  T* __restrict__ delta = a.delta + (int64_t)b * cells;
  T* __restrict__ y = a.y + (int64_t)b * cells;
#pragma unroll
  for (int m = 0; m < kImpCellsPerThread; ++m) {
    const int64_t c = imp_cell(m);
    if (c < cells) {
      const T dv = a.cycle > 0 ? (T)((double)delta[c] + (double)z[c]) : z[c];
      delta[c] = dv;
      if (fl & IMP_LIN_CONV) y[c] += dv;
    }
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------

template <typename T>
T* imp_field(const Implicit& s, int which) {
  return reinterpret_cast<T*>(s.fields.as<char>() + (size_t)which * s.field_bytes);
}
enum { F_Y0 = 0, F_G = 1, F_DELTA = 2, F_W0 = 3, F_W1 = 4, F_V = 5 };

bool implicit_equation(const pdeopt_problem& p) {
  return (p.equation == PDEOPT_EQ_CAHN_HILLIARD || p.equation == PDEOPT_EQ_ALLEN_CAHN) && p.nz <= 1;
}

// what the implicit step covers, asked before any launch
int implicit_check_problem(pdeopt_ctx* ctx) {
  const pdeopt_problem& p = ctx->prob;
  if (!implicit_equation(p))
    return fail(ctx, PDEOPT_EINVAL, "implicit Euler covers the periodic 2-D Cahn-Hilliard and Allen-Cahn equations: the 3-D, "
                                    "smoothed-boundary, Butler-Volmer, advection-diffusion and GPE kernels have no Jacobian action "
                                    "(equation %d)", p.equation);
  if (p.derivs != PDEOPT_DERIVS_FD)
    return fail(ctx, PDEOPT_EINVAL, "implicit Euler linearises the finite-difference right-hand side: derivs=\"fd\", not \"fourier\"");
  if (ctx->halo)
    return fail(ctx, PDEOPT_EINVAL, "implicit Euler needs the periodic layout: its sums run over whole environments, the padded "
                                    "(decomposed) layout holds a tile of one");
  if (p.mu.kind == PDEOPT_CL_JIT || p.mob.kind == PDEOPT_CL_JIT)
    return fail(ctx, PDEOPT_EINVAL, "implicit Euler needs closures of the in-kernel family (POLY / LEGENDRE): a run-time-compiled "
                                    "closure has no derivative to linearise with");
  return PDEOPT_OK;
}

int check_implicit(pdeopt_ctx* ctx) {
  if (!ctx->configured) return fail(ctx, PDEOPT_ESTATE, "pdeopt_configure has not been called");
  const Implicit* s = implicit_of(ctx);
  if (!s) return fail(ctx, PDEOPT_ESTATE, "pdeopt_implicit_configure has not been called");
  const int rc = implicit_check_problem(ctx);
  if (rc) return rc;
  if (s->B != ctx->prob.batch || s->cells != (int64_t)ctx->prob.nx * ctx->prob.ny)
    return fail(ctx, PDEOPT_ESTATE, "the problem changed shape after pdeopt_implicit_configure: configure the implicit step again");
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return PDEOPT_OK;
}

// raw != nullptr: the preconditioned operator, w = A src with src = z_j as it is, and v_j = scale x raw stored in vout
template <typename T>
int launch_op(pdeopt_ctx* ctx, const T* src, T* vout, T* wout, const double* scale, const int* flags, double dt,
              const T* raw = nullptr) {
  const pdeopt_problem& p = ctx->prob;
  ImpOpArgs<T> a{};
  a.y = ctx->Y.as<const T>();
  a.src = src;
  a.raw = raw;
  a.vout = vout;
  a.wout = wout;
  a.scale = scale;
  a.flags = flags;
  set_closures<T>(a, ctx, 0);
  a.nx = p.nx;
  a.ny = p.ny;
  set_recip_plain(a, grid_recip(p));
  a.dt = T(dt);
  const dim3 grid((p.ny + kTC - 1) / kTC, (p.nx + kTR - 1) / kTR, p.batch);
  const bool ac = p.equation == PDEOPT_EQ_ALLEN_CAHN;
  if (raw) {
    if (ac) hipLaunchKernelGGL(precond_op_ac_kernel<T>, grid, dim3(256), 0, ctx->stream, a);
    else hipLaunchKernelGGL(precond_op_ch_kernel<T>, grid, dim3(256), 0, ctx->stream, a);
  } else if (ac) {
    hipLaunchKernelGGL(imp_op_ac_kernel<T>, grid, dim3(256), 0, ctx->stream, a);
  } else {
    hipLaunchKernelGGL(imp_op_ch_kernel<T>, grid, dim3(256), 0, ctx->stream, a);
  }
  ctx->n_stage_launches++;
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  return PDEOPT_OK;
}

// a_b, c_b of the resident state for the environments with flags == 0 (flags == nullptr: all)
template <typename T>
int launch_precond_coefs(pdeopt_ctx* ctx, const int* flags) {
  Implicit& s = *implicit_of(ctx);
  PrecondCoefArgs<T> a{};
  a.y = ctx->Y.as<const T>();
  a.flags = flags;
  set_closures<T>(a, ctx, 0);
  a.cells = s.cells;
  a.nblk = s.nblk;
  a.pc = s.pc;
  hipLaunchKernelGGL(precond_coef_kernel<T>, dim3(s.nblk, s.B), dim3(256), 0, ctx->stream, a);
  hipLaunchKernelGGL(precond_coef_finish_kernel, dim3(s.B), dim3(64), 0, ctx->stream, s.pc, flags, s.nblk, (double)s.cells);
  ctx->n_stage_launches += 2;
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  return PDEOPT_OK;
}

// out = M^-1 (scale x in) over the whole batch: r2c, multiply, c2r.  cycle < 0: an iteration's rule for which environments
// the multiply touches, otherwise a cycle end's; the transforms run over every environment.  A frozen one's vectors are
// not written while it is frozen and the multiply with the 1 / N skips it, so its z is N x its stale source after an
// iteration and N^2 x after a cycle end, which the next iteration replaces: finite, bounded, nothing accumulates, and
// nobody reads it
template <typename T>
int launch_precond(pdeopt_ctx* ctx, const T* in, T* out, const double* scale, const int* flags, int cycle, double dt) {
  Implicit& s = *implicit_of(ctx);
  const pdeopt_problem& p = ctx->prob;
  int rc;
  if ((rc = spectral_real_exec(ctx, true, const_cast<T*>(in), s.hbuf))) return rc;
  PrecondMulArgs<T> a{};
  a.h = static_cast<T*>(s.hbuf);
  a.scale = scale;
  a.flags = flags;
  a.conv_cycle = s.sm.conv_cycle;
  a.cycle = cycle;
  a.ep = env_params<T>(ctx, 0);
  a.pc = s.pc;
  a.nx = p.nx;
  a.nyh = p.ny / 2 + 1;
  a.ch = p.equation == PDEOPT_EQ_CAHN_HILLIARD;
  a.dt = dt;
  a.fx = 4.0 / (p.hx * p.hx);
  a.fy = 4.0 / (p.hy * p.hy);
  a.rn = 1.0 / ((double)p.nx * (double)p.ny);
  const int64_t hc = (int64_t)a.nx * a.nyh;
  hipLaunchKernelGGL(precond_mul_kernel<T>, dim3((unsigned)((hc + 255) / 256), s.B), dim3(256), 0, ctx->stream, a);
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  if ((rc = spectral_real_exec(ctx, false, s.hbuf, out))) return rc;
  ctx->n_stage_launches += 3;  // the two transforms count as one each
  return PDEOPT_OK;
}

int read_flags(pdeopt_ctx* ctx) {
  Implicit& s = *implicit_of(ctx);
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(s.flags_host.as<int>(), s.sm.flags, (size_t)s.B * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PDEOPT_OK;
}

// the budget ran out: put the step's start back, say which environment and how far it got
int implicit_fail(pdeopt_ctx* ctx, int64_t step, const char* what, int iters) {
  Implicit& s = *implicit_of(ctx);
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(ctx->Y.get(), s.fields.get(), ctx->total_bytes, hipMemcpyDeviceToDevice, ctx->stream));
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(s.res_host.as<double>(), s.sm.res, (size_t)s.B * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(s.res_host.as<double>() + s.B, s.sm.tol, (size_t)s.B * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  int env = 0;
  for (int b = 0; b < s.B; ++b)
    if (!(s.flags_host.as<int>()[b] & (IMP_NEWTON_DONE | IMP_LIN_CONV))) { env = b; break; }
  return fail(ctx, PDEOPT_ENOCONVERGE, "implicit Euler did not converge: environment %d, step %lld: %s after %d iteration(s), last "
                                       "residual %.6g (threshold %.6g); the state is the one the step started from",
              env, (long long)step, what, iters, s.res_host.as<double>()[env], s.res_host.as<double>()[s.B + env]);
}

// one step y <- the solution of y - y0 - dt f(y) = 0; st: [B][4] counters or nullptr
template <typename T>
int implicit_step(pdeopt_ctx* ctx, double t1, double dt, int64_t step, int64_t* st) {
  Implicit& s = *implicit_of(ctx);
  const int B = s.B, m = s.restart;
  const int64_t cells = s.cells;
  T* const y = ctx->Y.as<T>();
  T* const W[2] = {imp_field<T>(s, F_W0), imp_field<T>(s, F_W1)};
  T* const V = imp_field<T>(s, F_V);
  const dim3 vgrid(s.nblk, B), sgrid(B);
  ImpVecArgs<T> va{};
  va.V = V;
  va.y = y;
  va.delta = imp_field<T>(s, F_DELTA);
  va.G = imp_field<T>(s, F_G);
  va.cells = cells;
  va.B = B;
  va.sm = s.sm;
  const bool pre = s.precond != 0;
  T* const Z = s.zfield.as<T>();
  int rc;
  auto count = [&](int which) {  // the environments the next launch works on
    if (st)
      for (int b = 0; b < B; ++b)
        if (!s.flags_host.as<int>()[b]) st[4 * b + which]++;
  };
  auto any_active = [&] {
    for (int b = 0; b < B; ++b)
      if (!s.flags_host.as<int>()[b]) return true;
    return false;
  };
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(s.fields.get(), y, ctx->total_bytes, hipMemcpyDeviceToDevice, ctx->stream));
  PDEOPT_HIP_CHECK(ctx, hipMemsetAsync(s.sm.flags, 0, (size_t)B * sizeof(int), ctx->stream));
  std::fill(s.flags_host.as<int>(), s.flags_host.as<int>() + B, 0);
  for (int newton_it = 0;; ++newton_it) {
    // the environments that are not frozen at the Newton level: LIN_CONV is the only other flag alive here
    for (int b = 0; b < B; ++b) s.flags_host.as<int>()[b] &= IMP_NEWTON_DONE;
    count(3);
    if ((rc = launch_rhs(ctx, whole_batch(ctx), y, ctx->TA.get(), t1))) return rc;
    hipLaunchKernelGGL(imp_residual_kernel<T>, vgrid, dim3(256), 0, ctx->stream, static_cast<const T*>(y),
                       static_cast<const T*>(imp_field<T>(s, F_Y0)), ctx->TA.as<const T>(), imp_field<T>(s, F_G), (T)dt, cells, s.sm);
    hipLaunchKernelGGL(imp_newton_small_kernel, sgrid, dim3(64), 0, ctx->stream, s.sm, (double)cells, s.rtol, s.atol, s.krylov_rtol,
                       newton_it, s.max_newton);
    ctx->n_stage_launches += 2;
    PDEOPT_HIP_CHECK(ctx, hipGetLastError());
    if ((rc = read_flags(ctx))) return rc;
    for (int b = 0; b < B; ++b)
      if (s.flags_host.as<int>()[b] & IMP_FAIL) return implicit_fail(ctx, step, "Newton: rms(G) above atol + rtol rms(y)", newton_it);
    if (!any_active()) return PDEOPT_OK;
    count(0);
    if (pre) {  // the symbol's coefficients at this Newton iterate
      if ((rc = launch_precond_coefs<T>(ctx, s.sm.flags))) return rc;
      std::fill(s.lin_applied.begin(), s.lin_applied.end(), (char)0);
    }
    int kit = 0;
    bool spent = false;
    for (int cycle = 0;; ++cycle) {
      if (cycle > 0) {  // the residual of the linear system at the delta so far
        count(2);
        if ((rc = launch_op<T>(ctx, va.delta, nullptr, W[1], nullptr, s.sm.flags, dt))) return rc;
        va.w = W[1];
        va.cycle = cycle;
        hipLaunchKernelGGL(imp_restart_kernel<T>, vgrid, dim3(256), 0, ctx->stream, va);
        hipLaunchKernelGGL(imp_restart_small_kernel, sgrid, dim3(64), 0, ctx->stream, s.sm, cycle);
        ctx->n_stage_launches += 2;
        PDEOPT_HIP_CHECK(ctx, hipGetLastError());
        if ((rc = read_flags(ctx))) return rc;
      }
      for (int j = 0; j < m && any_active(); ++j) {
        const T* src = j == 0 ? (cycle == 0 ? va.G : W[1]) : W[(j - 1) & 1];
        T* const w = W[j & 1];
        count(1);
        count(2);
        if (pre) {  // z_j = M^-1 v_j, w = A z_j; the operator stores v_j = scale x src as it goes by
          for (int b = 0; b < B; ++b)
            if (!s.flags_host.as<int>()[b]) s.pc_count[b]++;
          if ((rc = launch_precond<T>(ctx, src, Z, s.sm.vscale, s.sm.flags, -1, dt))) return rc;
          if ((rc = launch_op<T>(ctx, Z, V + (int64_t)j * B * cells, w, s.sm.vscale, s.sm.flags, dt, src))) return rc;
        } else if ((rc = launch_op<T>(ctx, src, V + (int64_t)j * B * cells, w, s.sm.vscale, s.sm.flags, dt))) {
          return rc;
        }
        va.w = w;
        va.ncols = j + 1;
        for (int pass = 0; pass < 2; ++pass) {
          va.pass = pass;
          hipLaunchKernelGGL(imp_dots_kernel<T>, vgrid, dim3(256), 0, ctx->stream, va);
          hipLaunchKernelGGL(imp_update_kernel<T>, vgrid, dim3(256), 0, ctx->stream, va);
        }
        ++kit;
        const bool last = j + 1 == m || kit >= s.max_krylov;
        hipLaunchKernelGGL(imp_gmres_small_kernel, sgrid, dim3(64), 0, ctx->stream, s.sm, j, cycle, (int)last);
        ctx->n_stage_launches += 5;
        PDEOPT_HIP_CHECK(ctx, hipGetLastError());
        if ((rc = read_flags(ctx))) return rc;
        if (kit >= s.max_krylov && any_active()) {
          spent = true;
          break;
        }
      }
      if (spent) return implicit_fail(ctx, step, "GMRES: residual estimate above krylov_rtol |G|", kit);
      va.cycle = cycle;
      if (pre) {  // delta (+)= M^-1 (V y_k): one application per cycle
        for (int b = 0; b < B; ++b) {
          const int fl = s.flags_host.as<int>()[b];
          if ((fl & (IMP_NEWTON_DONE | IMP_FAIL)) || ((fl & IMP_LIN_CONV) && s.lin_applied[b])) continue;
          s.pc_count[b]++;
          if (fl & IMP_LIN_CONV) s.lin_applied[b] = 1;
        }
        va.w = Z;
        hipLaunchKernelGGL(precond_combine_kernel<T>, vgrid, dim3(256), 0, ctx->stream, va);
        PDEOPT_HIP_CHECK(ctx, hipGetLastError());
        if ((rc = launch_precond<T>(ctx, Z, Z, nullptr, s.sm.flags, cycle, dt))) return rc;
        hipLaunchKernelGGL(precond_add_kernel<T>, vgrid, dim3(256), 0, ctx->stream, va);
        PDEOPT_HIP_CHECK(ctx, hipGetLastError());
        ctx->n_stage_launches += 2;
      } else {
        hipLaunchKernelGGL(imp_solution_kernel<T>, vgrid, dim3(256), 0, ctx->stream, va);
        ctx->n_stage_launches++;
      }
      PDEOPT_HIP_CHECK(ctx, hipGetLastError());
      if (!any_active()) break;
    }
  }
}

}  // namespace

int implicit_advance(pdeopt_ctx* ctx, double t0, double dt, int64_t n, int64_t* stats) {
  int rc;
  if ((rc = check_implicit(ctx))) return rc;
  if (!(dt > 0.0) || !std::isfinite(dt)) return fail(ctx, PDEOPT_EINVAL, "implicit Euler: dt = %g", dt);
  if ((rc = ensure_buffer(ctx, ctx->TA, ctx->total_bytes))) return rc;
  const int B = ctx->prob.batch;
  if (stats) std::fill(stats, stats + 4 * (int64_t)B, (int64_t)0);
  for (int64_t s = 0; s < n; ++s) {
    const double t1 = t0 + (double)(s + 1) * dt;
    rc = with_dtype(ctx, [&](auto t) { return implicit_step<decltype(t)>(ctx, t1, dt, s, stats); });
    if (rc) return rc;
  }
  char buf[96];
  snprintf(buf, sizeof(buf), "implicit_euler_%s_%s_gmres%d", equation_short_name(ctx->prob.equation),
           ctx->prob.dtype == PDEOPT_F32 ? "f32" : "f64", implicit_of(ctx)->restart);
  ctx->last_kernel = buf;
  return PDEOPT_OK;
}

}  // namespace pdeopt

using namespace pdeopt;

extern "C" {

int pdeopt_implicit_configure(pdeopt_ctx* ctx, double rtol, double atol, double krylov_rtol, int restart, int max_newton,
                              int max_krylov) {
  if (!ctx) return PDEOPT_EINVAL;
  if (!ctx->configured) return fail(ctx, PDEOPT_ESTATE, "pdeopt_configure has not been called");
  int rc;
  if ((rc = implicit_check_problem(ctx))) return rc;
  if (!(rtol >= 0.0) || !(atol >= 0.0) || !std::isfinite(rtol) || !std::isfinite(atol) || !(rtol + atol > 0.0))
    return fail(ctx, PDEOPT_EINVAL, "implicit Euler: rtol = %g, atol = %g (non-negative, not both zero)", rtol, atol);
  if (!(krylov_rtol > 0.0) || !(krylov_rtol < 1.0))
    return fail(ctx, PDEOPT_EINVAL, "implicit Euler: krylov_rtol = %g (0 < krylov_rtol < 1)", krylov_rtol);
  if (restart < 1 || restart > kImpMaxRestart)
    return fail(ctx, PDEOPT_EINVAL, "implicit Euler: restart = %d (1 .. %d: the small systems live in one workgroup's LDS)", restart,
                kImpMaxRestart);
  if (max_newton < 1 || max_krylov < 1)
    return fail(ctx, PDEOPT_EINVAL, "implicit Euler: max_newton = %d, max_krylov = %d (at least 1 each)", max_newton, max_krylov);
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const pdeopt_problem& p = ctx->prob;
  const int B = p.batch, m = restart;
  const int64_t cells = (int64_t)p.nx * p.ny;
  const int nblk = (int)((cells + kImpChunk - 1) / kImpChunk);
  const size_t field_bytes = (size_t)B * cells * ctx->esize;
  const size_t fields_bytes = (size_t)(F_V + m) * field_bytes;
  // doubles of the small block, in the order of ImpSmall; then the three int arrays
  const size_t nd = (size_t)B * ((size_t)m * nblk + 2 * (size_t)nblk + m + (size_t)m * m + m + m + (m + 1) + m + 4);
  const size_t small_bytes = nd * sizeof(double) + 3 * (size_t)B * sizeof(int);
  Implicit* s = implicit_of(ctx);
  if (s && (s->fields.bytes() != fields_bytes || s->small_blk.bytes() != small_bytes || s->B != B || s->restart != m)) {
    PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->features.drop(FS_IMPLICIT);
    s = nullptr;
  }
  if (!s) {
    size_t free_b = 0, total_b = 0;
    PDEOPT_HIP_CHECK(ctx, hipMemGetInfo(&free_b, &total_b));
    const size_t want = fields_bytes + small_bytes + (ctx->TA ? 0 : ctx->total_bytes);
    if (want > free_b)
      return fail(ctx, PDEOPT_ENOMEM, "implicit Euler: the workspace of restart = %d needs %zu bytes ((restart + 5) fields of the "
                                      "batch and the partial sums), %zu are free on the device", m, want, free_b);
    s = &ctx->features.ensure<Implicit>(FS_IMPLICIT);
    if ((rc = ensure_buffer(ctx, s->fields, fields_bytes)) || (rc = ensure_buffer(ctx, s->small_blk, small_bytes)) ||
        (rc = ensure_buffer(ctx, s->flags_host, (size_t)B * sizeof(int))) ||
        (rc = ensure_buffer(ctx, s->res_host, 2 * (size_t)B * sizeof(double)))) {
      ctx->features.drop(FS_IMPLICIT);
      return rc;
    }
    s->B = B;
    s->cells = cells;
    s->nblk = nblk;
    s->restart = m;
    s->field_bytes = field_bytes;
    double* d = s->small_blk.as<double>();
    ImpSmall& sm = s->sm;
    auto take = [&](size_t per_env) { double* q = d; d += (size_t)B * per_env; return q; };
    sm.part_dot = take((size_t)m * nblk);
    sm.part_nrm = take(2 * (size_t)nblk);
    sm.hcol = take(m);
    sm.R = take((size_t)m * m);
    sm.cs = take(m);
    sm.sn = take(m);
    sm.g = take(m + 1);
    sm.ycoef = take(m);
    sm.gnorm = take(1);
    sm.tol = take(1);
    sm.vscale = take(1);
    sm.res = take(1);
    sm.flags = reinterpret_cast<int*>(d);
    sm.kcols = sm.flags + B;
    sm.conv_cycle = sm.kcols + B;
    sm.m = m;
    sm.nblk = nblk;
    PDEOPT_HIP_CHECK(ctx, hipMemsetAsync(s->small_blk.get(), 0, small_bytes, ctx->stream));
  }
  s->precond = 0;  // pdeopt_implicit_set_precond comes after this call; its buffers stay with the workspace
  s->pc_count.assign((size_t)B, 0);
  s->lin_applied.assign((size_t)B, 0);
  s->rtol = rtol;
  s->atol = atol;
  s->krylov_rtol = krylov_rtol;
  s->max_newton = max_newton;
  s->max_krylov = max_krylov;
  return PDEOPT_OK;
}

int pdeopt_implicit_advance(pdeopt_ctx* ctx, double t0, double dt, int64_t n_steps, int64_t* stats_out) {
  if (!ctx) return PDEOPT_EINVAL;
  if (n_steps < 0) return fail(ctx, PDEOPT_EINVAL, "n_steps < 0");
  ctx->tsit5_fsal_valid = false;
  ctx->tsit5_pending = false;
  return implicit_advance(ctx, t0, dt, n_steps, stats_out);
}

int pdeopt_implicit_apply(pdeopt_ctx* ctx, double dt, const void* v_host, void* out_host) {
  if (!ctx || !v_host || !out_host) return PDEOPT_EINVAL;
  int rc;
  if ((rc = check_implicit(ctx))) return rc;
  Implicit& s = *implicit_of(ctx);
  return with_dtype(ctx, [&](auto t) {
    using T = decltype(t);
    T* const v = imp_field<T>(s, F_W0);
    T* const w = imp_field<T>(s, F_W1);
    PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(v, v_host, ctx->total_bytes, hipMemcpyHostToDevice, ctx->stream));
    int r;
    if ((r = launch_op<T>(ctx, v, nullptr, w, nullptr, nullptr, dt))) return r;
    PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(out_host, w, ctx->total_bytes, hipMemcpyDeviceToHost, ctx->stream));
    PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return (int)PDEOPT_OK;
  });
}

int pdeopt_implicit_set_precond(pdeopt_ctx* ctx, int kind) {
  if (!ctx) return PDEOPT_EINVAL;
  if (!ctx->configured) return fail(ctx, PDEOPT_ESTATE, "pdeopt_configure has not been called");
  int rc;
  if ((rc = implicit_check_problem(ctx))) return rc;  // another equation, another layout, 3-D: PDEOPT_EINVAL
  if ((rc = check_implicit(ctx))) return rc;
  if (kind != PDEOPT_IMPLICIT_PRECOND_NONE && kind != PDEOPT_IMPLICIT_PRECOND_SPECTRAL)
    return fail(ctx, PDEOPT_EINVAL, "implicit Euler: preconditioner %d (0 none, 1 spectral)", kind);
  Implicit& s = *implicit_of(ctx);
  std::fill(s.pc_count.begin(), s.pc_count.end(), (int64_t)0);
  if (kind == PDEOPT_IMPLICIT_PRECOND_NONE) {
    s.precond = 0;
    return PDEOPT_OK;
  }
  const pdeopt_problem& p = ctx->prob;
  const int nyh = p.ny / 2 + 1;
  const size_t nd = (size_t)s.B * (2 * (size_t)s.nblk + 2) + (size_t)p.nx + (size_t)nyh;
  // Set up once per workspace.  The tables and the size of pc_blk belong to one (nx, ny, batch, dtype), and so does this
  // workspace: pdeopt_configure frees it (features.clear(), with the field buffers) on any change of shape or dtype, and
  // pdeopt_implicit_configure, whose own reuse test compares byte sizes only, cannot see another grid without that.  A
  // reuse rule that lets a workspace outlive its grid has to rebuild these too.
  if (!s.zfield || !s.pc_blk) {
    size_t free_b = 0, total_b = 0;
    PDEOPT_HIP_CHECK(ctx, hipMemGetInfo(&free_b, &total_b));
    const size_t half_bytes = (size_t)s.B * p.nx * nyh * 2 * ctx->esize;
    const size_t want = s.field_bytes + half_bytes + nd * sizeof(double);
    if (want > free_b)
      return fail(ctx, PDEOPT_ENOMEM, "implicit Euler: the spectral preconditioner needs %zu bytes (one more field of the batch, "
                                      "the half-spectrum field of the transforms and the coefficient sums), %zu are free on the "
                                      "device", want, free_b);
    if ((rc = ensure_buffer(ctx, s.zfield, s.field_bytes)) || (rc = ensure_buffer(ctx, s.pc_blk, nd * sizeof(double)))) return rc;
    // the transforms run over every environment, a frozen one's included: what they read there is stale, never garbage
    PDEOPT_HIP_CHECK(ctx, hipMemsetAsync(s.zfield.get(), 0, s.field_bytes, ctx->stream));
    PDEOPT_HIP_CHECK(ctx, hipMemsetAsync(s.fields.as<char>() + (size_t)F_W0 * s.field_bytes, 0, 2 * s.field_bytes, ctx->stream));
    PDEOPT_HIP_CHECK(ctx, hipMemsetAsync(s.pc_blk.get(), 0, nd * sizeof(double), ctx->stream));
    double* d = s.pc_blk.as<double>();
    s.pc.part = d;
    s.pc.coef = s.pc.part + (size_t)s.B * 2 * s.nblk;
    s.pc.sin2x = s.pc.coef + (size_t)s.B * 2;
    s.pc.sin2y = s.pc.sin2x + p.nx;
    std::vector<double> tab((size_t)p.nx + nyh);
    const double pi = 3.14159265358979323846;
    for (int k = 0; k < p.nx; ++k) tab[k] = std::pow(std::sin(pi * k / p.nx), 2);
    for (int k = 0; k < nyh; ++k) tab[(size_t)p.nx + k] = std::pow(std::sin(pi * k / p.ny), 2);
    PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(s.pc.sin2x, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  }
  if ((rc = spectral_real_prepare(ctx, &s.hbuf, &s.half_cells))) return rc;
  if (s.half_cells != (int64_t)p.nx * nyh)
    return fail(ctx, PDEOPT_ESTATE, "implicit Euler: the half spectrum holds %lld cells, %lld expected", (long long)s.half_cells,
                (long long)p.nx * nyh);
  s.precond = kind;
  return PDEOPT_OK;
}

// the preconditioner entry points need one that is switched on
static int check_precond(pdeopt_ctx* ctx) {
  int rc;
  if ((rc = check_implicit(ctx))) return rc;
  if (!implicit_of(ctx)->precond)
    return fail(ctx, PDEOPT_ESTATE, "pdeopt_implicit_set_precond(ctx, PDEOPT_IMPLICIT_PRECOND_SPECTRAL) has not been called");
  return PDEOPT_OK;
}

int pdeopt_implicit_precond_coefs(pdeopt_ctx* ctx, double* out) {
  if (!ctx || !out) return PDEOPT_EINVAL;
  int rc;
  if ((rc = check_precond(ctx))) return rc;
  Implicit& s = *implicit_of(ctx);
  if ((rc = with_dtype(ctx, [&](auto t) { return launch_precond_coefs<decltype(t)>(ctx, nullptr); }))) return rc;
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(out, s.pc.coef, 2 * (size_t)s.B * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PDEOPT_OK;
}

int pdeopt_implicit_precond_apply(pdeopt_ctx* ctx, double dt, const void* v_host, void* out_host) {
  if (!ctx || !v_host || !out_host) return PDEOPT_EINVAL;
  int rc;
  if ((rc = check_precond(ctx))) return rc;
  if (!(dt > 0.0) || !std::isfinite(dt)) return fail(ctx, PDEOPT_EINVAL, "implicit Euler: dt = %g", dt);
  Implicit& s = *implicit_of(ctx);
  return with_dtype(ctx, [&](auto t) {
    using T = decltype(t);
    T* const v = imp_field<T>(s, F_W0);
    T* const z = s.zfield.as<T>();
    PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(v, v_host, ctx->total_bytes, hipMemcpyHostToDevice, ctx->stream));
    int r;
    if ((r = launch_precond_coefs<T>(ctx, nullptr))) return r;
    if ((r = launch_precond<T>(ctx, v, z, nullptr, nullptr, -1, dt))) return r;
    PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(out_host, z, ctx->total_bytes, hipMemcpyDeviceToHost, ctx->stream));
    PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return (int)PDEOPT_OK;
  });
}

int pdeopt_implicit_precond_count(pdeopt_ctx* ctx, int64_t* out) {
  if (!ctx || !out) return PDEOPT_EINVAL;
  int rc;
  if ((rc = check_implicit(ctx))) return rc;
  const Implicit& s = *implicit_of(ctx);
  std::copy(s.pc_count.begin(), s.pc_count.end(), out);
  return PDEOPT_OK;
}

}  // extern "C"
