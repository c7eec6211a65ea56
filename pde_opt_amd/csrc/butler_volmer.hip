// Allen-Cahn with Butler-Volmer kinetics, at a given voltage or at constant current, as a stage right-hand side.
//
// Replaces rhs_fd / get_voltage of pde_opt/numerics/equations/allen_cahn.py:162-395
// (AllenCahn2DPeriodicButlerVolmer, ...ConstantCurrent, AllenCahn2DSmoothedBoundaryButlerVolmerConstantCurrent):
//
//   mu  = mu_h(u) - kappa lap(u)                                        periodic            (w = 1)
//   mu  = mu_h(u) - kappa/psi [divx(avgx(psi) gradx u) + divy(...)]     smoothed boundary   (w = psi; no wall term)
//   I+- = hx hy sum w j0(u) exp(+- mu / 2),   y = (-C + sqrt(C^2 + 4 I+ I-)) / (2 I+),   v = 2 log y     constant current
//   du/dt = j0(u) (exp(-alpha eta) - exp((1 - alpha) eta)),   eta = mu + v
//
// The constant-current right-hand side is not local: v needs two sums over the whole environment.  Two launches:
//   pass 1  bv_mu_sums_kernel   mu of every cell into a work field, and the workgroup's two weighted sums -- per thread in
//                               fp64, reduced over the workgroup in a fixed order -- into partials[env][workgroup][2]
//   pass 2  bv_rate_kernel      EVERY workgroup adds its environment's partials itself, in one fixed order in fp64
//                               (bv_sum_partials), so all of them hold the same bits of v; then the rate and the stage
//                               launcher's output modes (stage_update).  Workgroup 0 of an environment records v in bv_v.
// No atomics, no finish kernel between the passes, nothing waits for another workgroup.  At a given voltage pass 2 is
// the only launch and evaluates the stencil itself.  pdeopt_bv_voltage runs pass 1 on the resident state and a
// one-wave-per-environment finish that calls the same bv_sum_partials / bv_voltage_of: bitwise the v of a right-hand side.
#include <cmath>

#include "stencil_generic.hpp"

namespace pdeopt {

namespace {

constexpr int kBvRows = 16, kBvCols = 64;      // cells per workgroup tile; 256 threads as (64, 4), four rows each
constexpr int kBvPitch = kBvCols + 2;          // LDS row pitch: the tile and its one-cell ring
constexpr int kBvLdsRows = kBvRows + 2;
constexpr int kBvRpt = kBvRows / 4;

template <typename T>
struct BvArgs {
  StageArgs<T> s;
  T* mu;              // work field [env][nx][ny] (constant current)
  double* partials;   // [env][nwg][2]
  double* bv_v;       // [env]
  const double* par;  // [env][2]: column 0 = v (mode 0) or C (mode 1)
  double alpha, h2, v_shift;
  int nwg, mode;
};

// a closure of the in-kernel family, then sqrt(.) if SQRT_WRAP: the exchange current sqrt(c (1 - c))
template <typename T>
__device__ __forceinline__ T bv_closure(const ClosureSpec& s, const T* __restrict__ coef, T c) {
  const T r = closure_generic<T>(s, coef, c);
  return (s.flags & PDEOPT_CL_SQRT_WRAP) ? t_sqrt<T>(r) : r;
}

// tile of `f` with its periodic ring -> LDS: LDS (r, c) holds cell (wrap(i0 - 1 + r), wrap(j0 - 1 + c)); any nx, ny
template <typename T>
__device__ __forceinline__ void bv_load_tile(T* __restrict__ lds, const T* __restrict__ f, int nx, int ny, int i0, int j0, int tid) {
  for (int e = tid; e < kBvLdsRows * kBvPitch; e += 256) {
    const int r = e / kBvPitch, c = e - r * kBvPitch;
    lds[e] = f[(int64_t)wrap_idx(i0 - 1 + r, nx) * ny + wrap_idx(j0 - 1 + c, ny)];
  }
}

// mu of the cell at LDS position (r, c), from the tile(s)
template <typename T, bool SBM>
__device__ __forceinline__ T bv_mu_at(const StageArgs<T>& a, const EnvParams<T>& p, const T* __restrict__ su, const T* __restrict__ sp,
                                      int r, int c) {
  const int o = r * kBvPitch + c;
  const T u0 = su[o], xp = su[o + kBvPitch], xm = su[o - kBvPitch], yp = su[o + 1], ym = su[o - 1];
  if constexpr (SBM) {
    // the expression of INNER in rhs_generic_point without its wall term (allen_cahn.py:323-339 has it commented out)
    const T pc = sp[o], pxp = sp[o + kBvPitch], pxm = sp[o - kBvPitch], pyp = sp[o + 1], pym = sp[o - 1];
    const T dx_hi = (T(0.5) * (pc + pxp)) * ((xp - u0) * a.rhx), dx_lo = (T(0.5) * (pxm + pc)) * ((u0 - xm) * a.rhx);
    const T dy_hi = (T(0.5) * (pc + pyp)) * ((yp - u0) * a.rhy), dy_lo = (T(0.5) * (pym + pc)) * ((u0 - ym) * a.rhy);
    const T lap = (dx_hi - dx_lo) * a.rhx + (dy_hi - dy_lo) * a.rhy;
    return closure_generic<T>(a.mu, p.mu, u0) - (p.kappa / pc) * lap;
  } else {
    return closure_generic<T>(a.mu, p.mu, u0) - p.kappa * lap_at<T>(u0, xp, xm, yp, ym, a.rhx2, a.rhy2);
  }
}

// The sum of an environment's n partial pairs by ONE wave, in one fixed order: lane l adds pairs l, l + 64, ... in index
// order, then the shuffle tree.  Every caller -- each workgroup of pass 2, the finish kernel -- gets the same bits.
__device__ __forceinline__ void bv_sum_partials(const double* __restrict__ part, int n, int lane, double* sp, double* sm) {
  double a = 0.0, b = 0.0;
  for (int q = lane; q < n; q += 64) {
    a += part[2 * q];
    b += part[2 * q + 1];
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    a += __shfl_down(a, s, 64);
    b += __shfl_down(b, s, 64);
  }
  *sp = a;  // lane 0 holds the sums
  *sm = b;
}

// v = 2 log y of the constant-current constraint (the 1/2 in I+- is fixed upstream, it is not alpha)
__device__ __forceinline__ double bv_voltage_of(double sp, double sm, double h2, double C) {
  const double ip = h2 * sp, im = h2 * sm;
  const double y = (-C + sqrt(C * C + 4.0 * ip * im)) / (2.0 * ip);
  return 2.0 * log(y);
}

template <typename T>
__device__ __forceinline__ T bv_rate(T j0, T eta, T alpha) {
  return j0 * (t_exp<T>(-alpha * eta) - t_exp<T>((T(1) - alpha) * eta));
}

}  // namespace

// pass 1 (constant current): mu -> work field, the workgroup's two weighted sums -> partials
template <typename T, bool SBM>
__global__ __launch_bounds__(256) void bv_mu_sums_kernel(const BvArgs<T> a) {
  __shared__ T su[kBvLdsRows * kBvPitch];
  __shared__ T sp[SBM ? kBvLdsRows * kBvPitch : 1];
  __shared__ double red[8];
  const int nx = a.s.g.nx, ny = a.s.g.ny;
  const int b = blockIdx.z, i0 = blockIdx.y * kBvRows, j0 = blockIdx.x * kBvCols;
  const int tid = threadIdx.y * 64 + threadIdx.x;
  const EnvParams<T>& p = a.s.ep[b];
  const int64_t base = (int64_t)b * a.s.g.bstride;
  bv_load_tile<T>(su, a.s.in + base, nx, ny, i0, j0, tid);
  if constexpr (SBM) bv_load_tile<T>(sp, a.s.psi, nx, ny, i0, j0, tid);
  __syncthreads();
  double accp = 0.0, accm = 0.0;
  const int j = j0 + threadIdx.x;
#pragma unroll
  for (int q = 0; q < kBvRpt; ++q) {
    const int ri = threadIdx.y + 4 * q, i = i0 + ri;
    if (i < nx && j < ny) {
      const int r = ri + 1, c = threadIdx.x + 1;
      const T mu = bv_mu_at<T, SBM>(a.s, p, su, sp, r, c);
      a.mu[base + (int64_t)i * ny + j] = mu;
      const T j0v = bv_closure<T>(a.s.mob, p.mob, su[r * kBvPitch + c]);
      const T ep = t_exp<T>(T(0.5) * mu), em = t_exp<T>(T(-0.5) * mu);
      double wj = (double)j0v;  // products in fp64 from the T values
      if constexpr (SBM) wj *= (double)sp[r * kBvPitch + c];
      accp += wj * (double)ep;
      accm += wj * (double)em;
    }
  }
  // fixed order: the shuffle tree of each wave, then the four waves in index order
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    accp += __shfl_down(accp, s, 64);
    accm += __shfl_down(accm, s, 64);
  }
  if (threadIdx.x == 0) {
    red[2 * threadIdx.y] = accp;
    red[2 * threadIdx.y + 1] = accm;
  }
  __syncthreads();
  if (tid < 2) {  // lane 0: I+, lane 1: I-; one plain store each
    const double v = ((red[tid] + red[2 + tid]) + red[4 + tid]) + red[6 + tid];
    const int wg = blockIdx.y * gridDim.x + blockIdx.x;
    a.partials[((int64_t)b * a.nwg + wg) * 2 + tid] = v;
  }
}

// pass 2 (STENCIL 0: constant current, mu from the work field), or the only launch at a given voltage (STENCIL 1: the
// periodic stencil, 2: the smoothed-boundary one)
template <typename T, int STENCIL>
__global__ __launch_bounds__(256) void bv_rate_kernel(const BvArgs<T> a) {
  __shared__ T su[STENCIL ? kBvLdsRows * kBvPitch : 1];
  __shared__ T sp[STENCIL == 2 ? kBvLdsRows * kBvPitch : 1];
  __shared__ double sv;
  const int nx = a.s.g.nx, ny = a.s.g.ny;
  const int b = blockIdx.z, i0 = blockIdx.y * kBvRows, j0 = blockIdx.x * kBvCols;
  const int tid = threadIdx.y * 64 + threadIdx.x;
  const EnvParams<T>& p = a.s.ep[b];
  const int64_t base = (int64_t)b * a.s.g.bstride;
  double vd;
  if constexpr (STENCIL == 0) {
    if (threadIdx.y == 0) {  // wave 0 adds the environment's partials; the other waves wait at the barrier
      double s_p, s_m;
      bv_sum_partials(a.partials + (int64_t)b * a.nwg * 2, a.nwg, threadIdx.x, &s_p, &s_m);
      if (threadIdx.x == 0) {
        const double v = bv_voltage_of(s_p, s_m, a.h2, a.par[2 * b]);
        sv = v;
        if (blockIdx.x == 0 && blockIdx.y == 0) a.bv_v[b] = v;
      }
    }
    __syncthreads();
    vd = sv;
  } else {
    vd = a.par[2 * b] + a.v_shift;
    bv_load_tile<T>(su, a.s.in + base, nx, ny, i0, j0, tid);
    if constexpr (STENCIL == 2) bv_load_tile<T>(sp, a.s.psi, nx, ny, i0, j0, tid);
    __syncthreads();
    if (tid == 0 && blockIdx.x == 0 && blockIdx.y == 0) a.bv_v[b] = vd;
  }
  const T v = T(vd), alpha = T(a.alpha);
  const int j = j0 + threadIdx.x;
#pragma unroll
  for (int q = 0; q < kBvRpt; ++q) {
    const int ri = threadIdx.y + 4 * q, i = i0 + ri;
    if (i < nx && j < ny) {
      const int64_t idx = base + (int64_t)i * ny + j;
      T mu, u0;
      if constexpr (STENCIL == 0) {
        mu = a.mu[idx];
        u0 = a.s.in[idx];
      } else {
        mu = bv_mu_at<T, STENCIL == 2>(a.s, p, su, sp, ri + 1, threadIdx.x + 1);
        u0 = su[(ri + 1) * kBvPitch + threadIdx.x + 1];
      }
      T k = bv_rate<T>(bv_closure<T>(a.s.mob, p.mob, u0), mu + v, alpha);
      if (a.s.scaled) k *= p.kscale;
      stage_update<T>(a.s, idx, k);
    }
  }
}

// pdeopt_bv_voltage: one wave per environment, the summation of pass 2
__global__ __launch_bounds__(64) void bv_finish_kernel(const double* __restrict__ partials, const double* __restrict__ par, int nwg,
                                                       double h2, double* __restrict__ bv_v) {
  const int b = blockIdx.x;
  double s_p, s_m;
  bv_sum_partials(partials + (int64_t)b * nwg * 2, nwg, threadIdx.x, &s_p, &s_m);
  if (threadIdx.x == 0) bv_v[b] = bv_voltage_of(s_p, s_m, h2, par[2 * b]);
}

// ---------------------------------------------------------------------------------------------------------------------
// Tangent-linear right-hand side (forward-mode sensitivities: sens.hip; PDEModel.train on the Butler-Volmer classes).
// The batch is [(1 + P) B][nx][ny]: tangent j of trajectory b is environment B + j B + b.  For the state tangent du of
// parameter p_j (a coefficient of mu_h, or of the exchange current j0):
//   dmu   = mu_h'(u) du - kappa L(du) + [role_j = MU] dmu_h/dp_j          L: the forward stencil (bv_stencil_lap)
//   dj0   = j0'(u) du + [role_j = MOB] dj0/dp_j                            (SQRT_WRAP: j0 = sqrt(r), dj0 = dr / (2 sqrt r))
//   dS+-  = sum w (dj0 exp(+-mu/2) +- 1/2 j0 exp(+-mu/2) dmu)              fp64, the order of the forward sums
//   dy    = (dI+ I- + I+ dI-) / (s I+) - y dI+ / I+,   dv = 2 dy / y       s = sqrt(C^2 + 4 I+ I-), I+- = h2 S+-
//   drate = dj0 (e^{-alpha eta} - e^{(1-alpha) eta}) - j0 (alpha e^{-alpha eta} + (1-alpha) e^{(1-alpha) eta}) (dmu + dv)
// Constant current, two launches over the tangent block whatever P is (the base block's slope, mu and partials come from
// launch_bv_stage over the window [0, B), so the base trajectory keeps the bits of a plain solve):
//   pass 1  bvsens_tile_kernel<.., 1>  grid (tiles, B): the base tile once, then per tangent the du tile -> dmu_j into the
//                                      work field at the tangent environment, the workgroup's two sums -> dpart[b][j][wg][2]
//   pass 2  bvsens_rate_kernel         every workgroup adds the base partials and its trajectory's tangent partials itself
//                                      (bv_sum_partials), forms v and dv_j, writes drate_j
// Given voltage (dv = 0): bvsens_tile_kernel<.., 0> alone, drate_j straight from the tiles.  Each tangent is reduced
// inside the tangent loop: P is a run-time value and no per-thread array is indexed by j.
// ---------------------------------------------------------------------------------------------------------------------
template <typename T>
struct BvSensArgs {
  BvArgs<T> f;     // window [0, B) of the forward arguments; f.s.in is the whole batch (the state or a stage value)
  T* out;          // slopes of the whole batch: the kernels write the tangent block
  double* dpart;   // [B][P][nwg][2]
  double* dv;      // [B][1 + P]: v and dv_j (bvsens_finish_kernel)
  int B, P;
  int role[kMaxSens], index[kMaxSens];
};

namespace {

// the basis function of coefficient k at c: c^k or P_k(2c - 1) (the recurrence of series_generic)
template <typename T>
__device__ __forceinline__ T bv_basis(const ClosureSpec& s, int k, T c) {
  T b = T(1);
  if (s.kind == PDEOPT_CL_POLY) {
    for (int q = 0; q < k; ++q) b *= c;
  } else if (k > 0) {
    const T x = T(2) * c - T(1);
    T pm = T(1);
    b = x;
    for (int q = 2; q <= k; ++q) {
      const T pn = (T(2 * q - 1) * x * b - T(q - 1) * pm) / T(q);
      pm = b;
      b = pn;
    }
  }
  return b;
}

// what a cell keeps of a closure for the tangent loop: the value f, df/dc, and g with df/dcoef[k] = g B_k(c)
template <typename T>
struct BvClosureJet {
  T f, dc, g;
};
template <typename T>
__device__ __forceinline__ BvClosureJet<T> bv_closure_jet(const ClosureSpec& s, const T* __restrict__ coef, T c) {
  const T r = closure_generic<T>(s, coef, c);  // before the square root
  BvClosureJet<T> o;
  o.dc = closure_dc<T>(s, coef, c, r);
  o.g = (s.flags & PDEOPT_CL_EXP_WRAP) ? r : T(1);
  o.f = r;
  if (s.flags & PDEOPT_CL_SQRT_WRAP) {
    o.f = t_sqrt<T>(r);
    const T h = T(0.5) / o.f;
    o.dc *= h;
    o.g *= h;
  }
  return o;
}

// L(du) at LDS position o: lap5, or (1/psi) div(psi_face grad) with the expressions of bv_mu_at
template <typename T, bool SBM>
__device__ __forceinline__ T bv_stencil_lap(const StageArgs<T>& a, const T* __restrict__ sd, const T* __restrict__ sp, int o) {
  const T u0 = sd[o], xp = sd[o + kBvPitch], xm = sd[o - kBvPitch], yp = sd[o + 1], ym = sd[o - 1];
  if constexpr (SBM) {
    const T pc = sp[o], pxp = sp[o + kBvPitch], pxm = sp[o - kBvPitch], pyp = sp[o + 1], pym = sp[o - 1];
    const T dx_hi = (T(0.5) * (pc + pxp)) * ((xp - u0) * a.rhx), dx_lo = (T(0.5) * (pxm + pc)) * ((u0 - xm) * a.rhx);
    const T dy_hi = (T(0.5) * (pc + pyp)) * ((yp - u0) * a.rhy), dy_lo = (T(0.5) * (pym + pc)) * ((u0 - ym) * a.rhy);
    return ((dx_hi - dx_lo) * a.rhx + (dy_hi - dy_lo) * a.rhy) / pc;
  } else {
    return lap_at<T>(u0, xp, xm, yp, ym, a.rhx2, a.rhy2);
  }
}

// dv = 2 dy / y of the constant-current constraint, from the sums and their tangents
__device__ __forceinline__ double bv_dvoltage_of(double sp, double sm, double dsp, double dsm, double h2, double C) {
  const double ip = h2 * sp, im = h2 * sm, dip = h2 * dsp, dim = h2 * dsm;
  const double s = sqrt(C * C + 4.0 * ip * im);
  const double y = (s - C) / (2.0 * ip);
  const double dy = (dip * im + ip * dim) / (s * ip) - y * dip / ip;
  return 2.0 * dy / y;
}

}  // namespace

// CURRENT 1: pass 1 of the constant-current tangents; CURRENT 0: the only launch at a given voltage.  grid (tiles, B)
template <typename T, bool SBM, int CURRENT>
__global__ __launch_bounds__(256) void bvsens_tile_kernel(const BvSensArgs<T> a) {
  __shared__ T su[kBvLdsRows * kBvPitch];
  __shared__ T sdu[kBvLdsRows * kBvPitch];
  __shared__ T sp[SBM ? kBvLdsRows * kBvPitch : 1];
  __shared__ double red[8];
  const StageArgs<T>& s = a.f.s;
  const int nx = s.g.nx, ny = s.g.ny;
  const int b = blockIdx.z, i0 = blockIdx.y * kBvRows, j0 = blockIdx.x * kBvCols;
  const int tid = threadIdx.y * 64 + threadIdx.x;
  const EnvParams<T>& p = s.ep[b];
  const T kappa = p.kappa;
  bv_load_tile<T>(su, s.in + (int64_t)b * s.g.bstride, nx, ny, i0, j0, tid);
  if constexpr (SBM) bv_load_tile<T>(sp, s.psi, nx, ny, i0, j0, tid);
  __syncthreads();
  const int j = j0 + threadIdx.x, c = threadIdx.x + 1;
  // this thread's four cells: what the tangent loop needs of the base state
  T u0[kBvRpt], mu1[kBvRpt], mug[kBvRpt], j0f[kBvRpt], j0dc[kBvRpt], j0g[kBvRpt];
  T ca[kBvRpt], cb[kBvRpt];  // CURRENT: w exp(+mu/2), w exp(-mu/2); else the two factors of drate
  const T alpha = T(a.f.alpha);
  const T v = CURRENT ? T(0) : T(a.f.par[2 * b] + a.f.v_shift);
#pragma unroll
  for (int q = 0; q < kBvRpt; ++q) {
    const int ri = threadIdx.y + 4 * q, i = i0 + ri;
    u0[q] = T(0.5);
    if (i < nx && j < ny) u0[q] = su[(ri + 1) * kBvPitch + c];
    const BvClosureJet<T> jm = bv_closure_jet<T>(s.mu, p.mu, u0[q]), jj = bv_closure_jet<T>(s.mob, p.mob, u0[q]);
    mu1[q] = jm.dc;
    mug[q] = jm.g;
    j0f[q] = jj.f;
    j0dc[q] = jj.dc;
    j0g[q] = jj.g;
    T mu = T(0);
    if (i < nx && j < ny) mu = bv_mu_at<T, SBM>(s, p, su, sp, ri + 1, c);
    if constexpr (CURRENT) {
      T w = T(1);
      if constexpr (SBM) w = sp[(ri + 1) * kBvPitch + c];
      ca[q] = w * t_exp<T>(T(0.5) * mu);
      cb[q] = w * t_exp<T>(T(-0.5) * mu);
    } else {
      const T eta = mu + v;
      const T e1 = t_exp<T>(-alpha * eta), e2 = t_exp<T>((T(1) - alpha) * eta);
      ca[q] = e1 - e2;
      cb[q] = -(j0f[q] * (alpha * e1 + (T(1) - alpha) * e2));
    }
  }
  for (int t = 0; t < a.P; ++t) {
    if (t) __syncthreads();  // the previous tangent's readers are done with sdu (and with red)
    const int64_t ebase = ((int64_t)a.B + (int64_t)t * a.B + b) * s.g.bstride;
    bv_load_tile<T>(sdu, s.in + ebase, nx, ny, i0, j0, tid);
    __syncthreads();
    const bool on_mu = a.role[t] == PDEOPT_SENS_MU;
    const int kc = a.index[t];
    double accp = 0.0, accm = 0.0;
#pragma unroll
    for (int q = 0; q < kBvRpt; ++q) {
      const int ri = threadIdx.y + 4 * q, i = i0 + ri;
      if (i < nx && j < ny) {
        const int o = (ri + 1) * kBvPitch + c;
        const T d = sdu[o];
        T dmu = mu1[q] * d - kappa * bv_stencil_lap<T, SBM>(s, sdu, sp, o);
        T dj0 = j0dc[q] * d;
        if (on_mu) dmu += mug[q] * bv_basis<T>(s.mu, kc, u0[q]);
        else dj0 += j0g[q] * bv_basis<T>(s.mob, kc, u0[q]);
        const int64_t idx = ebase + (int64_t)i * ny + j;
        if constexpr (CURRENT) {
          a.f.mu[idx] = dmu;
          const double hp = 0.5 * (double)j0f[q] * (double)dmu;  // products in fp64 from the T values
          accp += (double)ca[q] * ((double)dj0 + hp);
          accm += (double)cb[q] * ((double)dj0 - hp);
        } else {
          a.out[idx] = dj0 * ca[q] + cb[q] * dmu;
        }
      }
    }
    if constexpr (CURRENT) {
      // the fixed order of bv_mu_sums_kernel: the shuffle tree of each wave, then the four waves in index order
#pragma unroll
      for (int sh = 32; sh > 0; sh >>= 1) {
        accp += __shfl_down(accp, sh, 64);
        accm += __shfl_down(accm, sh, 64);
      }
      if (threadIdx.x == 0) {
        red[2 * threadIdx.y] = accp;
        red[2 * threadIdx.y + 1] = accm;
      }
      __syncthreads();
      if (tid < 2) {
        const double tot = ((red[tid] + red[2 + tid]) + red[4 + tid]) + red[6 + tid];
        const int wg = blockIdx.y * gridDim.x + blockIdx.x;
        a.dpart[(((int64_t)b * a.P + t) * a.f.nwg + wg) * 2 + tid] = tot;
      }
    }
  }
}

// pass 2 of the constant-current tangents, grid (tiles, B): base mu from the work field, dmu_j from its tangent environments
template <typename T>
__global__ __launch_bounds__(256) void bvsens_rate_kernel(const BvSensArgs<T> a) {
  __shared__ double ssum[2];
  __shared__ double sdv[kMaxSens + 1];  // v, then dv_j
  const StageArgs<T>& s = a.f.s;
  const int nx = s.g.nx, ny = s.g.ny;
  const int b = blockIdx.z, i0 = blockIdx.y * kBvRows, j0 = blockIdx.x * kBvCols;
  const EnvParams<T>& p = s.ep[b];
  const double C = a.f.par[2 * b];
  if (threadIdx.y == 0) {  // wave 0 adds the base partials, as in bv_rate_kernel
    double s_p, s_m;
    bv_sum_partials(a.f.partials + (int64_t)b * a.f.nwg * 2, a.f.nwg, threadIdx.x, &s_p, &s_m);
    if (threadIdx.x == 0) {
      ssum[0] = s_p;
      ssum[1] = s_m;
      sdv[0] = a.f.bv_v[b];  // the v the base block's bv_rate_kernel used and recorded: the same bits, whatever the compiler
                             // makes of bv_voltage_of next to bv_dvoltage_of here
    }
  }
  __syncthreads();
  for (int t = threadIdx.y; t < a.P; t += 4) {  // wave w adds the partials of tangents w, w + 4, ...
    double d_p, d_m;
    bv_sum_partials(a.dpart + ((int64_t)b * a.P + t) * a.f.nwg * 2, a.f.nwg, threadIdx.x, &d_p, &d_m);
    if (threadIdx.x == 0) sdv[1 + t] = bv_dvoltage_of(ssum[0], ssum[1], d_p, d_m, a.f.h2, C);
  }
  __syncthreads();
  const T v = T(sdv[0]), alpha = T(a.f.alpha);
  const int j = j0 + threadIdx.x;
  int64_t cell[kBvRpt];
  T u0[kBvRpt], j0dc[kBvRpt], j0g[kBvRpt], ca[kBvRpt], cb[kBvRpt];
#pragma unroll
  for (int q = 0; q < kBvRpt; ++q) {
    const int i = i0 + threadIdx.y + 4 * q;
    cell[q] = (i < nx && j < ny) ? (int64_t)i * ny + j : -1;
    T mu = T(0);
    u0[q] = T(0.5);
    if (cell[q] >= 0) {
      const int64_t idx = (int64_t)b * s.g.bstride + cell[q];
      mu = a.f.mu[idx];
      u0[q] = s.in[idx];
    }
    const BvClosureJet<T> jj = bv_closure_jet<T>(s.mob, p.mob, u0[q]);
    j0dc[q] = jj.dc;
    j0g[q] = jj.g;
    const T eta = mu + v;
    const T e1 = t_exp<T>(-alpha * eta), e2 = t_exp<T>((T(1) - alpha) * eta);
    ca[q] = e1 - e2;
    cb[q] = -(jj.f * (alpha * e1 + (T(1) - alpha) * e2));
  }
  for (int t = 0; t < a.P; ++t) {
    const int64_t ebase = ((int64_t)a.B + (int64_t)t * a.B + b) * s.g.bstride;
    const bool on_mob = a.role[t] != PDEOPT_SENS_MU;
    const int kc = a.index[t];
    const T dv = T(sdv[1 + t]);
#pragma unroll
    for (int q = 0; q < kBvRpt; ++q) {
      if (cell[q] >= 0) {
        const int64_t idx = ebase + cell[q];
        T dj0 = j0dc[q] * s.in[idx];
        if (on_mob) dj0 += j0g[q] * bv_basis<T>(s.mob, kc, u0[q]);
        a.out[idx] = dj0 * ca[q] + cb[q] * (a.f.mu[idx] + dv);
      }
    }
  }
}

// pdeopt_sens_bv_voltage: one wave per trajectory, the summation of pass 2 -> dv[b][0] = v, dv[b][1 + j] = dv/dp_j.  v itself
// is bv_finish_kernel's (launched before this one): pdeopt_bv_voltage's bits by construction
__global__ __launch_bounds__(64) void bvsens_finish_kernel(const double* __restrict__ partials, const double* __restrict__ dpart,
                                                           const double* __restrict__ par, int nwg, int P, double h2,
                                                           const double* __restrict__ bv_v, double* __restrict__ dv) {
  const int b = blockIdx.x;
  double s_p, s_m;
  bv_sum_partials(partials + (int64_t)b * nwg * 2, nwg, threadIdx.x, &s_p, &s_m);  // lane 0 holds the sums
  const double C = par[2 * b];
  if (threadIdx.x == 0) dv[(int64_t)b * (1 + P)] = bv_v[b];
  for (int t = 0; t < P; ++t) {
    double d_p, d_m;
    bv_sum_partials(dpart + ((int64_t)b * P + t) * nwg * 2, nwg, threadIdx.x, &d_p, &d_m);
    if (threadIdx.x == 0) dv[(int64_t)b * (1 + P) + 1 + t] = bv_dvoltage_of(s_p, s_m, d_p, d_m, h2, C);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
struct BvState : Feature {
  double alpha = 0.5;
  int mode = 0;
  bool set = false;
  DeviceBuffer par;       // [batch][2] doubles
  DeviceBuffer partials;  // [batch][nwg][2] doubles
  DeviceBuffer v;         // [batch] doubles
  int nwg = 0, batch = 0;
  // tangents (bv_sens_slopes / bv_sens_voltage): [B][P][nwg][2] partial sums and [B][1 + P] voltages, grown on demand
  DeviceBuffer dpart;
  DeviceBuffer dv;
};
// nullptr until pdeopt_set_bv_params
inline BvState* bv_of(const pdeopt_ctx* ctx) { return ctx->features.get<BvState>(FS_BV); }

namespace {

int bv_ensure(pdeopt_ctx* ctx) {
  BvState* st = &ctx->features.ensure<BvState>(FS_BV);
  const pdeopt_problem& p = ctx->prob;
  const int nwg = ((p.nx + kBvRows - 1) / kBvRows) * ((p.ny + kBvCols - 1) / kBvCols);
  if (st->par && st->nwg == nwg && st->batch == p.batch) return PDEOPT_OK;
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  st->par.reset();
  st->partials.reset();
  st->v.reset();
  st->nwg = nwg;
  st->batch = p.batch;
  st->set = false;
  int rc;
  if ((rc = ensure_buffer(ctx, st->par, sizeof(double) * 2 * (size_t)p.batch))) return rc;
  if ((rc = ensure_buffer(ctx, st->partials, sizeof(double) * 2 * (size_t)nwg * p.batch))) return rc;
  if ((rc = ensure_buffer(ctx, st->v, sizeof(double) * (size_t)p.batch))) return rc;
  PDEOPT_HIP_CHECK(ctx, hipMemsetAsync(st->par.get(), 0, sizeof(double) * 2 * (size_t)p.batch, ctx->stream));
  PDEOPT_HIP_CHECK(ctx, hipMemsetAsync(st->v.get(), 0, sizeof(double) * (size_t)p.batch, ctx->stream));
  return PDEOPT_OK;
}

int bv_check(pdeopt_ctx* ctx) {
  const pdeopt_problem& p = ctx->prob;
  if (!bv_equation(p.equation)) return fail(ctx, PDEOPT_EINVAL, "equation %d is not a Butler-Volmer equation", p.equation);
  if (!bv_of(ctx) || !bv_of(ctx)->set || bv_of(ctx)->batch != p.batch)
    return fail(ctx, PDEOPT_ESTATE, "the Butler-Volmer equations need pdeopt_set_bv_params after pdeopt_configure");
  if (p.equation == PDEOPT_EQ_ALLEN_CAHN_SBM_BV && !ctx->aux[PDEOPT_AUX_SBM_PSI].dev)
    return fail(ctx, PDEOPT_ESTATE, "the smoothed-boundary Butler-Volmer equation needs the SBM_PSI aux field");
  if (p.batch > 65535 || (p.nx + kBvRows - 1) / kBvRows > 65535)
    return fail(ctx, PDEOPT_EINVAL, "grid too large for the Butler-Volmer kernels (nx=%d batch=%d)", p.nx, p.batch);
  return PDEOPT_OK;
}

template <typename T>
BvArgs<T> bv_args(pdeopt_ctx* ctx, const Window& w, const StageArgs<T>& s) {
  BvState* st = bv_of(ctx);
  BvArgs<T> a{};
  a.s = s;
  a.mu = ctx->KS.as<T>() + (int64_t)w.lo * s.g.bstride;
  a.partials = st->partials.as<double>() + (int64_t)w.lo * st->nwg * 2;
  a.bv_v = st->v.as<double>() + w.lo;
  a.par = st->par.as<const double>() + 2 * (int64_t)w.lo;
  a.alpha = st->alpha;
  a.h2 = ctx->prob.hx * ctx->prob.hy;
  a.v_shift = (double)s.tw_a;
  a.nwg = st->nwg;
  a.mode = st->mode;
  return a;
}

dim3 bv_grid(const pdeopt_ctx* ctx, int n_env) {
  return dim3((ctx->prob.ny + kBvCols - 1) / kBvCols, (ctx->prob.nx + kBvRows - 1) / kBvRows, n_env);
}

template <typename T>
void bv_launch_pass1(pdeopt_ctx* ctx, const Window& w, const BvArgs<T>& a) {
  const dim3 grid = bv_grid(ctx, w.n), block(64, 4, 1);
  if (ctx->prob.equation == PDEOPT_EQ_ALLEN_CAHN_SBM_BV)
    hipLaunchKernelGGL((bv_mu_sums_kernel<T, true>), grid, block, 0, w.stream, a);
  else
    hipLaunchKernelGGL((bv_mu_sums_kernel<T, false>), grid, block, 0, w.stream, a);
}

}  // namespace

template <typename T>
int launch_bv_stage(pdeopt_ctx* ctx, const Window& w, const StageArgs<T>& s) {
  int rc;
  if ((rc = bv_check(ctx))) return rc;
  const bool sbm = ctx->prob.equation == PDEOPT_EQ_ALLEN_CAHN_SBM_BV;
  const dim3 grid = bv_grid(ctx, w.n), block(64, 4, 1);
  if (bv_of(ctx)->mode == 1) {
    if ((rc = ensure_buffer(ctx, ctx->KS, ctx->total_bytes))) return rc;
    const BvArgs<T> a = bv_args<T>(ctx, w, s);
    bv_launch_pass1<T>(ctx, w, a);
    hipLaunchKernelGGL((bv_rate_kernel<T, 0>), grid, block, 0, w.stream, a);
    ctx->last_kernel = sbm ? "bv_mu_sums<SBM>+bv_rate" : "bv_mu_sums+bv_rate";
  } else {
    const BvArgs<T> a = bv_args<T>(ctx, w, s);
    if (sbm)
      hipLaunchKernelGGL((bv_rate_kernel<T, 2>), grid, block, 0, w.stream, a);
    else
      hipLaunchKernelGGL((bv_rate_kernel<T, 1>), grid, block, 0, w.stream, a);
    ctx->last_kernel = sbm ? "bv_rate<SBM,voltage>" : "bv_rate<voltage>";
  }
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  return PDEOPT_OK;
}
template int launch_bv_stage<float>(pdeopt_ctx*, const Window&, const StageArgs<float>&);
template int launch_bv_stage<double>(pdeopt_ctx*, const Window&, const StageArgs<double>&);

int bv_set_params(pdeopt_ctx* ctx, double alpha, int mode, const double* per_env) {
  if (!bv_equation(ctx->prob.equation)) return fail(ctx, PDEOPT_EINVAL, "pdeopt_set_bv_params belongs to the Butler-Volmer equations");
  if (mode != 0 && mode != 1) return fail(ctx, PDEOPT_EINVAL, "Butler-Volmer mode %d: 0 = voltage given, 1 = constant current", mode);
  if (!std::isfinite(alpha)) return fail(ctx, PDEOPT_EINVAL, "Butler-Volmer symmetry factor alpha must be finite");
  int rc;
  const void* const par_before = bv_of(ctx) ? bv_of(ctx)->par.get() : nullptr;
  if ((rc = bv_ensure(ctx))) return rc;
  BvState* st = bv_of(ctx);
  // alpha, the mode and the buffers are kernel arguments of a captured substep graph (the per-environment values are not)
  if (st->par.get() != par_before || st->alpha != alpha || st->mode != mode) graph_destroy(ctx);
  st->alpha = alpha;
  st->mode = mode;
  const size_t bytes = sizeof(double) * 2 * (size_t)ctx->prob.batch;
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(st->par.get(), per_env, bytes, hipMemcpyHostToDevice, ctx->stream));
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // `per_env` is the caller's again
  st->set = true;
  ctx->tsit5_fsal_valid = false;
  return PDEOPT_OK;
}

int bv_voltage(pdeopt_ctx* ctx, int env_first, int env_count, double* host_out, bool recompute) {
  int rc;
  if ((rc = bv_check(ctx))) return rc;
  BvState* st = bv_of(ctx);
  if (recompute) {
    if (st->mode != 1) return fail(ctx, PDEOPT_EINVAL, "pdeopt_bv_voltage solves the constant-current constraint: set mode 1");
    if ((rc = ensure_buffer(ctx, ctx->KS, ctx->total_bytes))) return rc;
    const Window w{env_first, env_count, ctx->stream};
    rc = with_dtype(ctx, [&](auto tag) -> int {
      using T = decltype(tag);
      StageArgs<T> s{};
      s.g = make_geo(ctx);
      s.in = ctx->Y.as<const T>() + (int64_t)w.lo * s.g.bstride;
      set_recip_plain(s, grid_recip(ctx->prob));
      set_closures<T>(s, ctx, w.lo);
      s.psi = ctx->aux[PDEOPT_AUX_SBM_PSI].dev.as<const T>();
      const BvArgs<T> a = bv_args<T>(ctx, w, s);
      bv_launch_pass1<T>(ctx, w, a);
      hipLaunchKernelGGL(bv_finish_kernel, dim3(w.n), dim3(64), 0, w.stream, a.partials, a.par, a.nwg, a.h2, a.bv_v);
      return PDEOPT_OK;
    });
    if (rc) return rc;
    PDEOPT_HIP_CHECK(ctx, hipGetLastError());
    ctx->last_kernel = "bv_mu_sums+bv_finish";
  }
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(host_out, st->v.as<const double>() + env_first, sizeof(double) * (size_t)env_count,
                                       hipMemcpyDeviceToHost, ctx->stream));
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PDEOPT_OK;
}

// ---- tangents --------------------------------------------------------------------------------------------------------
namespace {

int bv_sens_check(pdeopt_ctx* ctx, const BvSensSpec& sp) {
  int rc;
  if ((rc = bv_check(ctx))) return rc;
  if (sp.B < 1 || sp.P < 1 || sp.P > kMaxSens || (int64_t)(1 + sp.P) * sp.B != ctx->prob.batch)
    return fail(ctx, PDEOPT_EINVAL, "Butler-Volmer tangents: batch %d is not (1 + %d) %d", ctx->prob.batch, sp.P, sp.B);
  if (bv_time_dependent(ctx))
    return fail(ctx, PDEOPT_EINVAL, "Butler-Volmer sensitivities are autonomous: a voltage protocol v(t) is not supported");
  return PDEOPT_OK;
}

template <typename T>
int bv_sens_args(pdeopt_ctx* ctx, const BvSensSpec& sp, const void* in, void* out, BvSensArgs<T>* a) {
  BvState* st = bv_of(ctx);
  int rc;
  if ((rc = ensure_buffer(ctx, ctx->KS, ctx->total_bytes))) return rc;
  // a block that is too small is freed after the stream's work, which may still use it -- and so may a captured graph
  const size_t dpart_bytes = sizeof(double) * 2 * (size_t)st->nwg * sp.B * sp.P, dv_bytes = sizeof(double) * (size_t)sp.B * (1 + sp.P);
  const bool regrow = (st->dpart && st->dpart.bytes() < dpart_bytes) || (st->dv && st->dv.bytes() < dv_bytes);
  if ((rc = grow_device_buffer(ctx, st->dpart, dpart_bytes, /*sync_first=*/true))) return rc;
  if ((rc = grow_device_buffer(ctx, st->dv, dv_bytes, /*sync_first=*/true))) return rc;
  if (regrow) graph_destroy(ctx);
  StageArgs<T> s{};
  s.g = make_geo(ctx);
  s.in = static_cast<const T*>(in);
  set_recip_plain(s, grid_recip(ctx->prob));
  set_closures<T>(s, ctx, 0);
  s.psi = ctx->aux[PDEOPT_AUX_SBM_PSI].dev.as<const T>();
  *a = BvSensArgs<T>{};
  a->f = bv_args<T>(ctx, Window{0, sp.B, ctx->stream}, s);
  a->out = static_cast<T*>(out);
  a->dpart = st->dpart.as<double>();
  a->dv = st->dv.as<double>();
  a->B = sp.B;
  a->P = sp.P;
  for (int j = 0; j < sp.P; ++j) {
    a->role[j] = sp.role[j];
    a->index[j] = sp.index[j];
  }
  return PDEOPT_OK;
}

template <typename T, int CURRENT>
void bv_sens_launch_tiles(pdeopt_ctx* ctx, const BvSensArgs<T>& a) {
  const dim3 grid = bv_grid(ctx, a.B), block(64, 4, 1);
  if (ctx->prob.equation == PDEOPT_EQ_ALLEN_CAHN_SBM_BV)
    hipLaunchKernelGGL((bvsens_tile_kernel<T, true, CURRENT>), grid, block, 0, ctx->stream, a);
  else
    hipLaunchKernelGGL((bvsens_tile_kernel<T, false, CURRENT>), grid, block, 0, ctx->stream, a);
}

}  // namespace

// the tangent block of `out` = J_f(in) du_j + df/dp_j.  Constant current: the base block's launch_bv_stage of the same
// `in` has left mu in KS[0, B) and the base partials (sens_slopes runs it first)
int bv_sens_slopes(pdeopt_ctx* ctx, const BvSensSpec& sp, const void* in, void* out) {
  int rc;
  if ((rc = bv_sens_check(ctx, sp))) return rc;
  const bool current = bv_of(ctx)->mode == 1;
  rc = with_dtype(ctx, [&](auto tag) -> int {
    using T = decltype(tag);
    BvSensArgs<T> a;
    const int r = bv_sens_args<T>(ctx, sp, in, out, &a);
    if (r) return r;
    if (current) {
      bv_sens_launch_tiles<T, 1>(ctx, a);
      hipLaunchKernelGGL(bvsens_rate_kernel<T>, bv_grid(ctx, a.B), dim3(64, 4, 1), 0, ctx->stream, a);
    } else {
      bv_sens_launch_tiles<T, 0>(ctx, a);
    }
    return PDEOPT_OK;
  });
  if (rc) return rc;
  ctx->n_stage_launches += current ? 2 : 1;
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  return PDEOPT_OK;
}

// v and dv/dp_j of the resident state, host_out [B][1 + P]: forward pass 1 on the base block, tangent pass 1, one wave per
// trajectory (bv_finish_kernel for v, bvsens_finish_kernel for dv_j).  The work field KS is overwritten; the state is not
int bv_sens_voltage(pdeopt_ctx* ctx, const BvSensSpec& sp, double* host_out) {
  int rc;
  if ((rc = bv_sens_check(ctx, sp))) return rc;
  BvState* st = bv_of(ctx);
  if (st->mode != 1) return fail(ctx, PDEOPT_EINVAL, "pdeopt_sens_bv_voltage differentiates the constant-current constraint: set mode 1");
  rc = with_dtype(ctx, [&](auto tag) -> int {
    using T = decltype(tag);
    BvSensArgs<T> a;
    const int r = bv_sens_args<T>(ctx, sp, ctx->Y.get(), nullptr, &a);
    if (r) return r;
    bv_launch_pass1<T>(ctx, Window{0, sp.B, ctx->stream}, a.f);
    bv_sens_launch_tiles<T, 1>(ctx, a);
    hipLaunchKernelGGL(bv_finish_kernel, dim3(sp.B), dim3(64), 0, ctx->stream, a.f.partials, a.f.par, a.f.nwg, a.f.h2, a.f.bv_v);
    hipLaunchKernelGGL(bvsens_finish_kernel, dim3(sp.B), dim3(64), 0, ctx->stream, a.f.partials, a.dpart, a.f.par, a.f.nwg, a.P, a.f.h2,
                       a.f.bv_v, a.dv);
    return PDEOPT_OK;
  });
  if (rc) return rc;
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  ctx->last_kernel = "bv_mu_sums+bvsens_tile+bv_finish+bvsens_finish";
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(host_out, st->dv.get(), sizeof(double) * (size_t)sp.B * (1 + sp.P), hipMemcpyDeviceToHost, ctx->stream));
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PDEOPT_OK;
}

bool bv_params_set(const pdeopt_ctx* ctx) { return bv_of(ctx) && bv_of(ctx)->set && bv_of(ctx)->batch == ctx->prob.batch; }

bool bv_time_dependent(const pdeopt_ctx* ctx) {
  return bv_equation(ctx->prob.equation) && bv_of(ctx) && bv_of(ctx)->mode == 0 && (ctx->time_fn != nullptr || !ctx->tt_times.empty());
}

}  // namespace pdeopt
