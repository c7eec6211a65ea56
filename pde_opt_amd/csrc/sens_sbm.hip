// Tangent-linear right-hand sides of the smoothed-boundary equations (AllenCahn2DSmoothedBoundary, allen_cahn.py:142-159;
// CahnHilliard2DSmoothedBoundary, cahn_hilliard.py:260-289) for the forward-mode sensitivities of sens.hip, in its layout:
// environments [0, B) are the trajectories, environment B + j B + b holds the tangent du/dp_j of trajectory b.
//
//   inner     = mu_h(u) - (kappa / psi) div(psi_f grad u) - sqrt(kappa) g sqrt(2 f(u)) w(t)
//   d inner_j = c1 du_j + [role_j = MU] dmu_h/dp_j - (kappa / psi) div(psi_f grad du_j),
//               c1 = mu_h'(u) - sqrt(kappa) g w(t) f'(u) / sqrt(2 f(u))     (the wall term's part is 0 where f(u) <= 0)
//   AC:  df_j = -(R'(u) du_j + [role_j = MOB] dR/dp_j) inner - R(u) d inner_j
//   CH:  df_j = div( psi_f avg(dD_j) grad(inner) + psi_f avg(D) grad(d inner_j) ) / psi,   dD_j = D'(u) du_j + [MOB] dD/dp_j
// with g = |grad psi| / psi (the NORM_GRAD aux field), w(t) = tw_a mask + tw_b (1 - mask) -- the two cosines the base
// block's own slope launch resolved for the same stage time (ctx->time_last) -- and the forward kernels' primitives in
// their order: face averages of psi, face gradients, face divergence.  The source term g flux(t) depends on neither u nor
// the parameters: its tangent is 0.  f is the free-energy closure `fe` (fixed data, per-environment coefficients).
//
// One workgroup per (16 x 32 tile, trajectory), as the kernels of sens.hip: the base quantities are formed once per tile,
// then the P tangents are streamed through LDS -- each tangent field read once, each tangent slope written once, one
// launch whatever P is.
#include "closures.hpp"
#include "common.hpp"
#include "sens_tile.hpp"

namespace pdeopt {

namespace {

template <typename T>
struct SbmSensArgs {
  const T* y;  // state [(1 + P) B][nx][ny]
  T* k;        // slopes, same layout; the kernels write the tangent block
  const EnvParams<T>* ep;
  ClosureSpec mu, mob, fe;
  const T *psi, *ngp, *mask;  // [nx][ny], shared by the batch
  int nx, ny, B, P;
  T rhx, rhy, rhx2, rhy2;
  T tw_a, tw_b;  // cos(theta(t)) on / off the mask at this evaluation's time
  int role[kMaxSens];
  int index[kMaxSens];
};

// s[(r, c)] = f[wrap(i0 - RING + r), wrap(j0 - RING + c)] for r < kTR + 2 RING, c < kTC + 2 RING
template <typename T, int RING>
__device__ __forceinline__ void sbm_stage(T* __restrict__ s, const T* __restrict__ f, int i0, int j0, int nx, int ny, int tid) {
  constexpr int kRows = kTR + 2 * RING, kCols = kTC + 2 * RING;
  for (int q = tid; q < kRows * kCols; q += 256) {
    const int r = q / kCols, c = q - r * kCols;
    s[q] = f[(int64_t)wrap_idx(i0 + r - RING, nx) * ny + wrap_idx(j0 + c - RING, ny)];
  }
}

// div(psi_f grad v) at position o of two LDS arrays of row pitch LD (the expression of `inner` in the forward kernels)
template <typename T, int LD>
__device__ __forceinline__ T sbm_div(const T* __restrict__ v, const T* __restrict__ p, int o, T rhx, T rhy) {
  const T c = v[o], pc = p[o];
  const T dx_hi = (T(0.5) * (pc + p[o + LD])) * ((v[o + LD] - c) * rhx), dx_lo = (T(0.5) * (p[o - LD] + pc)) * ((c - v[o - LD]) * rhx);
  const T dy_hi = (T(0.5) * (pc + p[o + 1])) * ((v[o + 1] - c) * rhy), dy_lo = (T(0.5) * (p[o - 1] + pc)) * ((c - v[o - 1]) * rhy);
  return (dx_hi - dx_lo) * rhx + (dy_hi - dy_lo) * rhy;
}

// what a cell keeps of the base state for the tangent loop
template <typename T>
struct SbmCell {
  T muh, mob, mob1, c1, inner;
};
// u = the cell's value, lap = div(psi_f grad u) there, pc = psi, wall = sqrt(kappa) g w(t)
template <typename T>
__device__ __forceinline__ SbmCell<T> sbm_cell(const SbmSensArgs<T>& a, const EnvParams<T>& ep, T u, T lap, T pc, T wall) {
  SbmCell<T> o;
  o.muh = closure_generic<T>(a.mu, ep.mu, u);
  o.mob = closure_generic<T>(a.mob, ep.mob, u);
  o.mob1 = closure_dc<T>(a.mob, ep.mob, u, o.mob);
  const T fe = closure_generic<T>(a.fe, ep.fe, u);
  const T sq = t_sqrt<T>(T(2) * fe);
  o.inner = o.muh - (ep.kappa * t_rcp<T>(pc)) * lap - wall * sq;
  // d sqrt(2 f) / du = f' / sqrt(2 f); where f <= 0 (the forward value is 0 or NaN there) the wall term has no tangent
  const T dsq = fe > T(0) ? closure_dc<T>(a.fe, ep.fe, u, fe) * t_rcp<T>(sq) : T(0);
  o.c1 = closure_dc<T>(a.mu, ep.mu, u, o.muh) - wall * dsq;
  return o;
}

// ---- Allen-Cahn: radius-1 stencil in u.  u, psi and du_j are staged in LDS (tile + 1-cell ring); everything else a cell
// needs stays in the registers of the thread that owns it.  A thread owns the cells (r, c) and (r + 8, c) of the tile.
template <typename T>
__global__ __launch_bounds__(256) void sens_sbm_ac_tangent_rhs_kernel(SbmSensArgs<T> a) {
  __shared__ T su[kR1 * kC1], sp[kR1 * kC1], sdu[kR1 * kC1];
  const int tid = threadIdx.x;
  const int b = blockIdx.z;
  const int i0 = blockIdx.y * kTR, j0 = blockIdx.x * kTC;
  const int nx = a.nx, ny = a.ny;
  const int64_t cells = (int64_t)nx * ny;
  const EnvParams<T>& ep = a.ep[b];
  const T sqk = sqrt(ep.kappa);
  sbm_stage<T, 1>(su, a.y + (int64_t)b * cells, i0, j0, nx, ny, tid);
  sbm_stage<T, 1>(sp, a.psi, i0, j0, nx, ny, tid);
  __syncthreads();
  const int c = tid & 31;
  const int gj = j0 + c;
  int o[2], gi[2];
  T uc[2], kpsi[2];
  SbmCell<T> q[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int r = (tid >> 5) + 8 * e;
    gi[e] = i0 + r;
    o[e] = (r + 1) * kC1 + (c + 1);
    const int64_t at = (int64_t)wrap_idx(gi[e], nx) * ny + wrap_idx(gj, ny);
    const T m = a.mask[at];
    const T wall = sqk * a.ngp[at] * (a.tw_a * m + a.tw_b * (T(1) - m));
    uc[e] = su[o[e]];
    kpsi[e] = ep.kappa * t_rcp<T>(sp[o[e]]);
    q[e] = sbm_cell<T>(a, ep, uc[e], sbm_div<T, kC1>(su, sp, o[e], a.rhx, a.rhy), sp[o[e]], wall);
  }
  for (int j = 0; j < a.P; ++j) {
    if (j) __syncthreads();  // the previous tangent's readers are done with sdu
    const int64_t env = (int64_t)a.B + (int64_t)j * a.B + b;
    sbm_stage<T, 1>(sdu, a.y + env * cells, i0, j0, nx, ny, tid);
    __syncthreads();
    const bool on_mu = a.role[j] == PDEOPT_SENS_MU;
    const int kc = a.index[j];
    T* __restrict__ out = a.k + env * cells;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const T d = sdu[o[e]];
      T dinner = q[e].c1 * d - kpsi[e] * sbm_div<T, kC1>(sdu, sp, o[e], a.rhx, a.rhy);
      T dR = q[e].mob1 * d;
      if (on_mu) dinner += closure_dcoef<T>(a.mu, kc, uc[e], q[e].muh);
      else dR += closure_dcoef<T>(a.mob, kc, uc[e], q[e].mob);
      if (gi[e] < nx && gj < ny) out[(int64_t)gi[e] * ny + gj] = -(dR * q[e].inner) - q[e].mob * dinner;
    }
  }
}

// ---- Cahn-Hilliard: radius-2 stencil in u and psi.  u, psi and du_j on the tile + 2-cell ring; inner, D, D', c1 and mu_h
// (the factor of an exp-wrapped mu's coefficient derivative) of the base state on the tile + 1-cell ring, formed once;
// per tangent d inner_j and dD_j on the same ring, then the psi-weighted flux divergence on the tile.
template <typename T>
__global__ __launch_bounds__(256) void sens_sbm_ch_tangent_rhs_kernel(SbmSensArgs<T> a) {
  __shared__ T su[kR2 * kC2], sp[kR2 * kC2], sdu[kR2 * kC2];
  __shared__ T sin[kR1 * kC1], sD[kR1 * kC1], sD1[kR1 * kC1], sc1[kR1 * kC1], smuh[kR1 * kC1];
  __shared__ T sdin[kR1 * kC1], sdD[kR1 * kC1];
  const int tid = threadIdx.x;
  const int b = blockIdx.z;
  const int i0 = blockIdx.y * kTR, j0 = blockIdx.x * kTC;
  const int nx = a.nx, ny = a.ny;
  const int64_t cells = (int64_t)nx * ny;
  const EnvParams<T>& ep = a.ep[b];
  const T kappa = ep.kappa;
  const T sqk = sqrt(kappa);
  sbm_stage<T, 2>(su, a.y + (int64_t)b * cells, i0, j0, nx, ny, tid);
  sbm_stage<T, 2>(sp, a.psi, i0, j0, nx, ny, tid);
  __syncthreads();
  for (int q = tid; q < kR1 * kC1; q += 256) {
    const int r = q / kC1, c = q - r * kC1;
    const int o = (r + 1) * kC2 + (c + 1);
    const int64_t at = (int64_t)wrap_idx(i0 + r - 1, nx) * ny + wrap_idx(j0 + c - 1, ny);
    const T m = a.mask[at];
    const T wall = sqk * a.ngp[at] * (a.tw_a * m + a.tw_b * (T(1) - m));
    const SbmCell<T> cell = sbm_cell<T>(a, ep, su[o], sbm_div<T, kC2>(su, sp, o, a.rhx, a.rhy), sp[o], wall);
    sin[q] = cell.inner;
    sD[q] = cell.mob;
    sD1[q] = cell.mob1;
    sc1[q] = cell.c1;
    smuh[q] = cell.muh;
  }
  for (int j = 0; j < a.P; ++j) {
    __syncthreads();  // the previous tangent's readers are done with sdu / sdin / sdD (and the base arrays are written)
    const int64_t env = (int64_t)a.B + (int64_t)j * a.B + b;
    sbm_stage<T, 2>(sdu, a.y + env * cells, i0, j0, nx, ny, tid);
    __syncthreads();
    const bool on_mu = a.role[j] == PDEOPT_SENS_MU;
    const int kc = a.index[j];
    for (int q = tid; q < kR1 * kC1; q += 256) {
      const int r = q / kC1, c = q - r * kC1;
      const int o = (r + 1) * kC2 + (c + 1);
      const T uc = su[o], d = sdu[o];
      T dinner = sc1[q] * d - (kappa * t_rcp<T>(sp[o])) * sbm_div<T, kC2>(sdu, sp, o, a.rhx, a.rhy);
      T dD = sD1[q] * d;
      if (on_mu) dinner += closure_dcoef<T>(a.mu, kc, uc, smuh[q]);
      else dD += closure_dcoef<T>(a.mob, kc, uc, sD[q]);
      sdin[q] = dinner;
      sdD[q] = dD;
    }
    __syncthreads();
    T* __restrict__ out = a.k + env * cells;
    for (int q = tid; q < kTR * kTC; q += 256) {
      const int r = q / kTC, c = q - r * kTC;
      const int gi = i0 + r, gj = j0 + c;
      if (gi >= nx || gj >= ny) continue;
      const int o = (r + 1) * kC1 + (c + 1);
      const int xp = o + kC1, xm = o - kC1, yp = o + 1, ym = o - 1;
      const int w = (r + 2) * kC2 + (c + 2);
      const T pc = sp[w];
      // faces +-1/2 along x (axis 0) and y (axis 1): psi_f (avg(dD) grad(inner) + avg(D) grad(d inner))
      const T fxp = (T(0.5) * (pc + sp[w + kC2])) * (T(0.5) * (sdD[o] + sdD[xp]) * ((sin[xp] - sin[o]) * a.rhx) +
                                                     T(0.5) * (sD[o] + sD[xp]) * ((sdin[xp] - sdin[o]) * a.rhx));
      const T fxm = (T(0.5) * (sp[w - kC2] + pc)) * (T(0.5) * (sdD[xm] + sdD[o]) * ((sin[o] - sin[xm]) * a.rhx) +
                                                     T(0.5) * (sD[xm] + sD[o]) * ((sdin[o] - sdin[xm]) * a.rhx));
      const T fyp = (T(0.5) * (pc + sp[w + 1])) * (T(0.5) * (sdD[o] + sdD[yp]) * ((sin[yp] - sin[o]) * a.rhy) +
                                                   T(0.5) * (sD[o] + sD[yp]) * ((sdin[yp] - sdin[o]) * a.rhy));
      const T fym = (T(0.5) * (sp[w - 1] + pc)) * (T(0.5) * (sdD[ym] + sdD[o]) * ((sin[o] - sin[ym]) * a.rhy) +
                                                   T(0.5) * (sD[ym] + sD[o]) * ((sdin[o] - sdin[ym]) * a.rhy));
      out[(int64_t)gi * ny + gj] = ((fxp - fxm) * a.rhx + (fyp - fym) * a.rhy) * t_rcp<T>(pc);
    }
  }
}

template <typename T>
int launch_sbm_tangent_rhs(pdeopt_ctx* ctx, const BvSensSpec& sp, const void* in, void* out) {
  const pdeopt_problem& p = ctx->prob;
  SbmSensArgs<T> a{};
  a.y = static_cast<const T*>(in);
  a.k = static_cast<T*>(out);
  set_closures<T>(a, ctx, 0);
  a.fe = closure_spec(p.fe);
  a.psi = ctx->aux[PDEOPT_AUX_SBM_PSI].dev.as<const T>();
  a.ngp = ctx->aux[PDEOPT_AUX_SBM_NORM_GRAD].dev.as<const T>();
  a.mask = ctx->aux[PDEOPT_AUX_SBM_MASK].dev.as<const T>();
  a.nx = p.nx;
  a.ny = p.ny;
  a.B = sp.B;
  a.P = sp.P;
  set_recip_plain(a, grid_recip(p));
  a.tw_a = T(ctx->time_last[0]);
  a.tw_b = T(ctx->time_last[1]);
  for (int j = 0; j < sp.P; ++j) {
    a.role[j] = sp.role[j];
    a.index[j] = sp.index[j];
  }
  const dim3 grid((p.ny + kTC - 1) / kTC, (p.nx + kTR - 1) / kTR, sp.B);
  if (p.equation == PDEOPT_EQ_ALLEN_CAHN_SBM) hipLaunchKernelGGL(sens_sbm_ac_tangent_rhs_kernel<T>, grid, dim3(256), 0, ctx->stream, a);
  else hipLaunchKernelGGL(sens_sbm_ch_tangent_rhs_kernel<T>, grid, dim3(256), 0, ctx->stream, a);
  ctx->n_stage_launches++;
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  return PDEOPT_OK;
}

}  // namespace

int sbm_sens_slopes(pdeopt_ctx* ctx, const BvSensSpec& sp, const void* in, void* out) {
  if (!sbm_equation(ctx->prob.equation)) return fail(ctx, PDEOPT_EINVAL, "sbm_sens_slopes belongs to the smoothed-boundary equations");
  if (!ctx->aux[PDEOPT_AUX_SBM_PSI].dev || !ctx->aux[PDEOPT_AUX_SBM_NORM_GRAD].dev || !ctx->aux[PDEOPT_AUX_SBM_MASK].dev)
    return fail(ctx, PDEOPT_ESTATE, "smoothed-boundary sensitivities need the SBM_PSI, SBM_NORM_GRAD and SBM_MASK aux fields");
  if ((int64_t)(1 + sp.P) * sp.B != ctx->prob.batch || sp.P > kMaxSens || sp.B > 65535 || (ctx->prob.nx + kTR - 1) / kTR > 65535)
    return fail(ctx, PDEOPT_EINVAL, "smoothed-boundary sensitivities: batch %d, B = %d, P = %d, nx = %d (grid too large)",
                ctx->prob.batch, sp.B, sp.P, ctx->prob.nx);
  return with_dtype(ctx, [&](auto t) { return launch_sbm_tangent_rhs<decltype(t)>(ctx, sp, in, out); });
}

}  // namespace pdeopt
