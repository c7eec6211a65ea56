// Cahn-Hilliard with the homogeneous chemical potential mu_h given as a FIELD: the forward slope and step, and one
// substep of their discrete adjoint (the reference's train(method="mse") with a neural-network mu,
// docs/notebooks/optimization_neural_network.ipynb: pde_opt/numerics/functions/cnn.py as mu, the solve differentiated in
// reverse mode by RecursiveCheckpointAdjoint, pde_model.py:429-460).
//
// The network lives in torch on the same device and stream.  It hands a field mu_h = N(u) in and takes a cotangent
// field dJ/dmu_h out; no kernel here sees the network.  With m = mu_h - kappa lap5(u) the right-hand side is
//   f = div( avg(D(u)) grad(m) )                                                        (cahn_hilliard.py:89-109)
// and for a cotangent lambda of f, J = <lambda, f> = -sum over faces of avg(D) grad(m) grad(lambda), so
//   g_mu = dJ/dmu_h = div( avg(D) grad(lambda) )               (the operator is symmetric in m)
//   g_D(o)          = -1/2 sum over the 4 faces of o of grad(lambda)_face grad(m)_face
//   g_u  = dJ/du at fixed mu_h = -kappa lap5(g_mu) + D'(u) g_D
// The caller adds the network's own vector-Jacobian product N'(u)^T g_mu.
//
// One substep is Y += dt S f(Y, mu_h) with S = I (Euler) or S = Re ifft(fft(.) / (1 + A dt symbol)) (IMEX,
// solvers.py:56-70; rocFFT's real transforms on every grid).  Its adjoint takes the cotangent lambda of the new state to
// lambda + J_f^T (dt S lambda): S is real-symmetric for a real even symbol (Cahn-Hilliard's kappa k^4), so the same
// transforms serve.
#include "closures.hpp"
#include "common.hpp"
#include "sens_tile.hpp"

namespace pdeopt {
namespace {

template <typename T>
struct FieldMuArgs {
  const T* u;    // state [B][nx][ny]
  const T* muh;  // mu_h, same layout
  const T* lam;  // adjoint: S lambda of the new state, same layout (the kernel scales its staged copy by `scale`)
  T* out;        // forward: the slope f; adjoint: g_mu
  T* lam_io;     // adjoint: lambda itself, += g_u
  const EnvParams<T>* ep;
  ClosureSpec mob;
  int nx, ny;
  T rhx, rhy, rhx2, rhy2;
  T scale;  // adjoint: dt
};

// s[(r, c)] = f[wrap(i0 - 2 + r), wrap(j0 - 2 + c)] on the tile + 2-cell ring
template <typename T>
__device__ __forceinline__ void stage_ring2(T* __restrict__ s, const T* __restrict__ f, int i0, int j0, int nx, int ny, int tid) {
  for (int q = tid; q < kR2 * kC2; q += 256) {
    const int r = q / kC2, c = q - r * kC2;
    s[q] = f[(int64_t)wrap_idx(i0 + r - 2, nx) * ny + wrap_idx(j0 + c - 2, ny)];
  }
}

// m = mu_h - kappa lap5(u) on the tile + 1-cell ring: mu_h from the field, u from its LDS tile
template <typename T>
__device__ __forceinline__ void form_m(T* __restrict__ sm, const T* __restrict__ su, const T* __restrict__ muh, T kappa,
                                       const FieldMuArgs<T>& a, int i0, int j0, int tid) {
  for (int q = tid; q < kR1 * kC1; q += 256) {
    const int r = q / kC1, c = q - r * kC1;
    const int o = (r + 1) * kC2 + (c + 1);
    const T uc = su[o];
    const T lap = (su[o + kC2] - T(2) * uc + su[o - kC2]) * a.rhx2 + (su[o + 1] - T(2) * uc + su[o - 1]) * a.rhy2;
    sm[q] = muh[(int64_t)wrap_idx(i0 + r - 1, a.nx) * a.ny + wrap_idx(j0 + c - 1, a.ny)] - kappa * lap;
  }
}

// div( avg(D) grad(v) ) at cell o of arrays with row pitch ld: the forward kernels' face expressions in their order
template <typename T>
__device__ __forceinline__ T div_flux(const T* __restrict__ sD, const T* __restrict__ sv, int o, int ld, T rhx, T rhy) {
  const int xp = o + ld, xm = o - ld, yp = o + 1, ym = o - 1;
  const T fxp = (T(0.5) * (sD[o] + sD[xp])) * ((sv[xp] - sv[o]) * rhx);
  const T fxm = (T(0.5) * (sD[xm] + sD[o])) * ((sv[o] - sv[xm]) * rhx);
  const T fyp = (T(0.5) * (sD[o] + sD[yp])) * ((sv[yp] - sv[o]) * rhy);
  const T fym = (T(0.5) * (sD[ym] + sD[o])) * ((sv[o] - sv[ym]) * rhy);
  return (fxp - fxm) * rhx + (fyp - fym) * rhy;
}

// f = div( avg(D(u)) grad(mu_h - kappa lap5(u)) ).  One workgroup per (tile, trajectory): the geometry of
// sens_tangent_rhs_kernel (16 x 32 outputs, u on the 2-cell ring, m and D on the 1-cell ring).
template <typename T>
__global__ __launch_bounds__(256) void fieldmu_rhs_kernel(FieldMuArgs<T> a) {
  __shared__ T su[kR2 * kC2];
  __shared__ T sm[kR1 * kC1], sD[kR1 * kC1];
  const int tid = threadIdx.x;
  const int b = blockIdx.z;
  const int i0 = blockIdx.y * kTR, j0 = blockIdx.x * kTC;
  const int nx = a.nx, ny = a.ny;
  const int64_t cells = (int64_t)nx * ny;
  const EnvParams<T>& ep = a.ep[b];
  stage_ring2<T>(su, a.u + (int64_t)b * cells, i0, j0, nx, ny, tid);
  __syncthreads();
  form_m<T>(sm, su, a.muh + (int64_t)b * cells, ep.kappa, a, i0, j0, tid);
  for (int q = tid; q < kR1 * kC1; q += 256) {
    const int r = q / kC1, c = q - r * kC1;
    sD[q] = closure_generic<T>(a.mob, ep.mob, su[(r + 1) * kC2 + (c + 1)]);
  }
  __syncthreads();
  T* __restrict__ out = a.out + (int64_t)b * cells;
  for (int q = tid; q < kTR * kTC; q += 256) {
    const int r = q / kTC, c = q - r * kTC;
    const int gi = i0 + r, gj = j0 + c;
    if (gi >= nx || gj >= ny) continue;
    out[(int64_t)gi * ny + gj] = div_flux<T>(sD, sm, (r + 1) * kC1 + (c + 1), kC1, a.rhx, a.rhy);
  }
}

// The transpose of the kernel above at fixed mu_h, in gather form: every output cell collects its own contributions, no
// atomics.  lambda and u are staged on the 2-cell ring, D is formed there too, so g_mu = div( avg(D) grad(lambda) ) is
// available on the 1-cell ring in LDS for the Laplacian of g_u without a trip through memory.
template <typename T>
__global__ __launch_bounds__(256) void fieldmu_adjoint_kernel(FieldMuArgs<T> a) {
  __shared__ T su[kR2 * kC2], sl[kR2 * kC2], sD[kR2 * kC2];
  __shared__ T sm[kR1 * kC1], sg[kR1 * kC1];
  const int tid = threadIdx.x;
  const int b = blockIdx.z;
  const int i0 = blockIdx.y * kTR, j0 = blockIdx.x * kTC;
  const int nx = a.nx, ny = a.ny;
  const int64_t cells = (int64_t)nx * ny;
  const EnvParams<T>& ep = a.ep[b];
  const T kappa = ep.kappa;
  stage_ring2<T>(su, a.u + (int64_t)b * cells, i0, j0, nx, ny, tid);
  stage_ring2<T>(sl, a.lam + (int64_t)b * cells, i0, j0, nx, ny, tid);
  for (int q = tid; q < kR2 * kC2; q += 256) {  // each thread reads back the cells it staged itself
    sD[q] = closure_generic<T>(a.mob, ep.mob, su[q]);
    sl[q] *= a.scale;
  }
  __syncthreads();
  form_m<T>(sm, su, a.muh + (int64_t)b * cells, kappa, a, i0, j0, tid);
  for (int q = tid; q < kR1 * kC1; q += 256) {
    const int r = q / kC1, c = q - r * kC1;
    sg[q] = div_flux<T>(sD, sl, (r + 1) * kC2 + (c + 1), kC2, a.rhx, a.rhy);
  }
  __syncthreads();
  T* __restrict__ gmu = a.out + (int64_t)b * cells;
  T* __restrict__ lam = a.lam_io + (int64_t)b * cells;
  for (int q = tid; q < kTR * kTC; q += 256) {
    const int r = q / kTC, c = q - r * kTC;
    const int gi = i0 + r, gj = j0 + c;
    if (gi >= nx || gj >= ny) continue;
    const int o = (r + 1) * kC1 + (c + 1);   // in the 1-ring arrays
    const int p = (r + 2) * kC2 + (c + 2);   // in the 2-ring arrays
    // grad(lambda) grad(m) on the four faces of the cell
    const T gxp = ((sl[p + kC2] - sl[p]) * a.rhx) * ((sm[o + kC1] - sm[o]) * a.rhx);
    const T gxm = ((sl[p] - sl[p - kC2]) * a.rhx) * ((sm[o] - sm[o - kC1]) * a.rhx);
    const T gyp = ((sl[p + 1] - sl[p]) * a.rhy) * ((sm[o + 1] - sm[o]) * a.rhy);
    const T gym = ((sl[p] - sl[p - 1]) * a.rhy) * ((sm[o] - sm[o - 1]) * a.rhy);
    const T gD = T(-0.5) * ((gxp + gxm) + (gyp + gym));
    const T g = sg[o];
    const T lap = (sg[o + kC1] - T(2) * g + sg[o - kC1]) * a.rhx2 + (sg[o + 1] - T(2) * g + sg[o - 1]) * a.rhy2;
    const int64_t at = (int64_t)gi * ny + gj;
    gmu[at] = g;
    lam[at] += closure_dc<T>(a.mob, ep.mob, su[p], sD[p]) * gD - kappa * lap;
  }
}

// The kernel above, line for line (the same bits in lambda and g_mu), and on top the tile's share of the gradient over
// the mobility's coefficients: the sum over its owned cells of g_D(o) dD/dcoef_k(u(o)) for k < mob.n (closure_dcoef's
// B_k, the basis run upward once per cell), in fp64 whatever T is -- the two cells of a thread, then across the wave, then
// the four waves through LDS in a fixed order.  Thread k adds the result to slot (trajectory, tile, k) of
// slots[batch][tiles][kMaxCoef] with a plain load-add-store: a slot has one owner and the substeps of a sweep are ordered
// on the stream, so there is no race and no atomic, and the bits do not depend on the run.  (A kernel of its own, not a
// template flag of the one above: that one's code stays what it was.)
template <typename T>
__global__ __launch_bounds__(256) void fieldmu_adjoint_coef_kernel(FieldMuArgs<T> a, double* __restrict__ slots) {
  __shared__ T su[kR2 * kC2], sl[kR2 * kC2], sD[kR2 * kC2];
  __shared__ T sm[kR1 * kC1], sg[kR1 * kC1];
  __shared__ double sw[kTR * kTC];     // g_D, times D(u) under EXP_WRAP, per owned cell
  __shared__ double sred[4][kMaxCoef];  // per wave and coefficient
  __shared__ double* sslot;
  const int tid = threadIdx.x;
  const int b = blockIdx.z;
  const int i0 = blockIdx.y * kTR, j0 = blockIdx.x * kTC;
  const int nx = a.nx, ny = a.ny;
  const int64_t cells = (int64_t)nx * ny;
  const EnvParams<T>& ep = a.ep[b];
  const T kappa = ep.kappa;
  // this workgroup's slots, parked in LDS until the end (the barriers below publish it): the fp64 stencil leaves no
  // scalar registers to carry the pieces of the address that far
  if (tid == 0) sslot = slots + (((int64_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * kMaxCoef;
  stage_ring2<T>(su, a.u + (int64_t)b * cells, i0, j0, nx, ny, tid);
  stage_ring2<T>(sl, a.lam + (int64_t)b * cells, i0, j0, nx, ny, tid);
  for (int q = tid; q < kR2 * kC2; q += 256) {
    sD[q] = closure_generic<T>(a.mob, ep.mob, su[q]);
    sl[q] *= a.scale;
  }
  __syncthreads();
  form_m<T>(sm, su, a.muh + (int64_t)b * cells, kappa, a, i0, j0, tid);
  for (int q = tid; q < kR1 * kC1; q += 256) {
    const int r = q / kC1, c = q - r * kC1;
    sg[q] = div_flux<T>(sD, sl, (r + 1) * kC2 + (c + 1), kC2, a.rhx, a.rhy);
  }
  __syncthreads();
  T* __restrict__ gmu = a.out + (int64_t)b * cells;
  T* __restrict__ lam = a.lam_io + (int64_t)b * cells;
  const bool exp_wrap = a.mob.flags & PDEOPT_CL_EXP_WRAP;
  for (int q = tid; q < kTR * kTC; q += 256) {
    const int r = q / kTC, c = q - r * kTC;
    const int gi = i0 + r, gj = j0 + c;
    sw[q] = 0.0;  // cells outside the grid contribute nothing
    if (gi >= nx || gj >= ny) continue;
    const int o = (r + 1) * kC1 + (c + 1);
    const int p = (r + 2) * kC2 + (c + 2);
    const T gxp = ((sl[p + kC2] - sl[p]) * a.rhx) * ((sm[o + kC1] - sm[o]) * a.rhx);
    const T gxm = ((sl[p] - sl[p - kC2]) * a.rhx) * ((sm[o] - sm[o - kC1]) * a.rhx);
    const T gyp = ((sl[p + 1] - sl[p]) * a.rhy) * ((sm[o + 1] - sm[o]) * a.rhy);
    const T gym = ((sl[p] - sl[p - 1]) * a.rhy) * ((sm[o] - sm[o - 1]) * a.rhy);
    const T gD = T(-0.5) * ((gxp + gxm) + (gyp + gym));
    const T g = sg[o];
    const T lap = (sg[o + kC1] - T(2) * g + sg[o - kC1]) * a.rhx2 + (sg[o + 1] - T(2) * g + sg[o - 1]) * a.rhy2;
    const int64_t at = (int64_t)gi * ny + gj;
    gmu[at] = g;
    lam[at] += closure_dc<T>(a.mob, ep.mob, su[p], sD[p]) * gD - kappa * lap;
    sw[q] = exp_wrap ? (double)gD * (double)sD[p] : (double)gD;  // read back below by this thread alone
  }
  // A pass of its own, after the stencil's registers are free.  The tile is 2 x 256 cells: a thread runs the basis of its
  // two cells upward side by side, so coefficient k is summed, reduced across the wave and put down before k + 1 is
  // formed, and one sum is live at a time.
  static_assert(kTR * kTC == 2 * 256, "two cells per thread");
  const int lane = tid & 63, wave = tid >> 6;
  const int n = a.mob.n;
  const bool poly = a.mob.kind == PDEOPT_CL_POLY;
  double w[2];
  T u[2], x[2], bk[2], pm[2];  // B_k and B_(k-1) without the exp factor, by closure_dcoef's recurrences
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int q = tid + 256 * h, r = q / kTC, c = q - r * kTC;
    w[h] = sw[q];
    u[h] = su[(r + 2) * kC2 + (c + 2)];
    x[h] = T(2) * u[h] - T(1);
    bk[h] = pm[h] = T(1);
  }
#pragma unroll
  for (int k = 0; k < kMaxCoef; ++k) {
    if (k < n) {
      double v = w[0] * (double)bk[0] + w[1] * (double)bk[1];
      for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s, 64);
      if (lane == 0) sred[wave][k] = v;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (poly) {
          bk[h] *= u[h];
        } else if (k == 0) {
          bk[h] = x[h];
        } else if (k + 1 < kMaxCoef) {
          const T pn = (T(2 * k + 1) * x[h] * bk[h] - T(k) * pm[h]) * T(kRecip[k + 1]);
          pm[h] = bk[h];
          bk[h] = pn;
        }
      }
    }
  }
  __syncthreads();
  if (tid < n) sslot[tid] += ((sred[0][tid] + sred[1][tid]) + sred[2][tid]) + sred[3][tid];
}

// what every entry point asks of the configured problem (the rules of pdeopt_sens_configure) and of its pointers
int check_fieldmu(pdeopt_ctx* ctx, std::initializer_list<const void*> fields) {
  if (!ctx->configured) return fail(ctx, PDEOPT_ESTATE, "pdeopt_configure has not been called");
  const pdeopt_problem& p = ctx->prob;
  if (p.equation != PDEOPT_EQ_CAHN_HILLIARD || p.nz > 1 || p.derivs != PDEOPT_DERIVS_FD || ctx->halo)
    return fail(ctx, PDEOPT_EINVAL, "a field mu_h needs the periodic 2-D Cahn-Hilliard equation with derivs=\"fd\"");
  if (p.mob.kind == PDEOPT_CL_JIT)
    return fail(ctx, PDEOPT_EINVAL, "a field mu_h needs a mobility of the in-kernel family (POLY / LEGENDRE), not a run-time-compiled one");
  for (const void* f : fields)
    if (!f || (uintptr_t)f % ctx->esize)
      return fail(ctx, PDEOPT_EINVAL, "field pointer %p: device fields are [batch][nx][ny] in the problem dtype, aligned to it", f);
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return ensure_buffer(ctx, ctx->TA, ctx->total_bytes);
}

// the integrators of a field-mu step; IMEX also prepares the multiplier of step dt
int check_step(pdeopt_ctx* ctx, int integrator, double dt) {
  if (!(dt > 0)) return fail(ctx, PDEOPT_EINVAL, "dt = %g", dt);
  if (integrator == PDEOPT_INT_EULER) return PDEOPT_OK;
  if (integrator != PDEOPT_INT_IMEX)
    return fail(ctx, PDEOPT_EINVAL, "a field mu_h supports the IMEX and Euler integrators (got %d)", integrator);
  if (!ctx->aux[PDEOPT_AUX_IMEX_SYMBOL].dev)
    return fail(ctx, PDEOPT_ESTATE, "IMEX needs the IMEX_SYMBOL aux field (fourier_symbol)");
  if (ctx->imex_per_env)
    return fail(ctx, PDEOPT_EINVAL, "a field mu_h needs one implicit operator shared by the batch (no per-environment IMEX scales)");
  return imex_rocfft_prepare(ctx, dt);
}

template <typename T>
FieldMuArgs<T> fieldmu_args(const pdeopt_ctx* ctx, const void* u, const void* muh, void* out) {
  FieldMuArgs<T> a{};
  a.u = static_cast<const T*>(u);
  a.muh = static_cast<const T*>(muh);
  a.out = static_cast<T*>(out);
  a.ep = env_params<T>(ctx, 0);
  a.mob = closure_spec(ctx->prob.mob);
  a.nx = ctx->prob.nx;
  a.ny = ctx->prob.ny;
  set_recip_plain(a, grid_recip(ctx->prob));
  return a;
}

inline dim3 tile_grid(const pdeopt_ctx* ctx) {
  return dim3((ctx->prob.ny + kTC - 1) / kTC, (ctx->prob.nx + kTR - 1) / kTR, ctx->prob.batch);
}

// out = f(Y, mu_h)
int launch_fieldmu_rhs(pdeopt_ctx* ctx, const void* muh, void* out) {
  return with_dtype(ctx, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(fieldmu_rhs_kernel<T>, tile_grid(ctx), dim3(256), 0, ctx->stream, fieldmu_args<T>(ctx, ctx->Y.get(), muh, out));
    ctx->n_stage_launches++;
    PDEOPT_HIP_CHECK(ctx, hipGetLastError());
    return (int)PDEOPT_OK;
  });
}

// what the coefficient gradient asks on top: a mobility whose coefficients it can name, one and the same for the whole
// batch (the gradient is of one shared D), and the zeroed slots
int check_coef(pdeopt_ctx* ctx) {
  const pdeopt_problem& p = ctx->prob;
  if (p.mob.kind != PDEOPT_CL_POLY && p.mob.kind != PDEOPT_CL_LEGENDRE)
    return fail(ctx, PDEOPT_EINVAL, "the coefficient gradient needs a mobility of the POLY / LEGENDRE family (kind %d)", p.mob.kind);
  const bool shared = with_dtype(ctx, [&](auto t) {
    using T = decltype(t);
    const auto* e = reinterpret_cast<const EnvParams<T>*>(ctx->env_params_host.data());
    for (int b = 1; b < p.batch; ++b)
      for (int k = 0; k < p.mob.n; ++k)
        if (e[b].mob[k] != e[0].mob[k]) return false;
    return true;
  });
  if (!shared)
    return fail(ctx, PDEOPT_EINVAL, "the coefficient gradient is of one mobility shared by the batch: the environments' mobility coefficients differ");
  if (ctx->fieldmu_coef) return PDEOPT_OK;
  const dim3 g = tile_grid(ctx);
  ctx->fieldmu_coef_slots = (size_t)g.x * g.y * g.z * kMaxCoef;
  if (const int rc = ensure_buffer(ctx, ctx->fieldmu_coef, ctx->fieldmu_coef_slots * sizeof(double))) return rc;
  PDEOPT_HIP_CHECK(ctx, hipMemsetAsync(ctx->fieldmu_coef.as<double>(), 0, ctx->fieldmu_coef_slots * sizeof(double), ctx->stream));
  return PDEOPT_OK;
}

// one adjoint substep; `coef`: the kernel that also adds the mobility's coefficient gradient to ctx->fieldmu_coef
int adjoint_step(pdeopt_ctx* ctx, int integrator, double dt, const void* u_dev, const void* mu_dev, void* lam_dev,
                 void* gmu_dev, bool coef) {
  if (!ctx) return PDEOPT_EINVAL;
  int rc = check_fieldmu(ctx, {u_dev, mu_dev, lam_dev, gmu_dev});
  if (rc || (rc = check_step(ctx, integrator, dt))) return rc;
  if (coef && (rc = check_coef(ctx))) return rc;
  // the fields are [p, p + total_bytes): the two that are written must not overlap each other or an input
  const auto overlap = [&](const void* a, const void* b) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + ctx->total_bytes && y < x + ctx->total_bytes;
  };
  if (overlap(gmu_dev, lam_dev) || overlap(gmu_dev, u_dev) || overlap(gmu_dev, mu_dev) || overlap(lam_dev, u_dev) ||
      overlap(lam_dev, mu_dev))
    return fail(ctx, PDEOPT_EINVAL, "lam_dev and gmu_dev are written: they must not overlap each other or the inputs");
  // TA = S lambda: the kernel reads lambda on a ring while it updates lambda itself, so it reads the copy
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(ctx->TA.get(), lam_dev, ctx->total_bytes, hipMemcpyDeviceToDevice, ctx->stream));
  if (integrator == PDEOPT_INT_IMEX) {
    if ((rc = imex_rocfft_apply(ctx))) return rc;
    ctx->n_stage_launches += 3;
  }
  rc = with_dtype(ctx, [&](auto t) {
    using T = decltype(t);
    FieldMuArgs<T> a = fieldmu_args<T>(ctx, u_dev, mu_dev, gmu_dev);
    a.lam = ctx->TA.as<const T>();
    a.lam_io = static_cast<T*>(lam_dev);
    a.scale = (T)dt;
    if (coef)
      hipLaunchKernelGGL(fieldmu_adjoint_coef_kernel<T>, tile_grid(ctx), dim3(256), 0, ctx->stream, a, ctx->fieldmu_coef.as<double>());
    else
      hipLaunchKernelGGL(fieldmu_adjoint_kernel<T>, tile_grid(ctx), dim3(256), 0, ctx->stream, a);
    ctx->n_stage_launches++;
    PDEOPT_HIP_CHECK(ctx, hipGetLastError());
    return (int)PDEOPT_OK;
  });
  if (rc) return rc;
  ctx->last_kernel = integrator == PDEOPT_INT_IMEX ? "imex_rocfft_r2c+fieldmu_adjoint" : "fieldmu_adjoint";
  if (coef) ctx->last_kernel += "_coef";
  return PDEOPT_OK;
}

}  // namespace
}  // namespace pdeopt

using namespace pdeopt;

extern "C" {

int pdeopt_fieldmu_rhs(pdeopt_ctx* ctx, const void* mu_dev, void* out_dev) {
  if (!ctx) return PDEOPT_EINVAL;
  const int rc = check_fieldmu(ctx, {mu_dev, out_dev});
  if (rc) return rc;
  ctx->last_kernel = "fieldmu_rhs";
  return launch_fieldmu_rhs(ctx, mu_dev, out_dev);
}

int pdeopt_fieldmu_step(pdeopt_ctx* ctx, int integrator, double dt, const void* mu_dev) {
  if (!ctx) return PDEOPT_EINVAL;
  int rc = check_fieldmu(ctx, {mu_dev});
  if (rc || (rc = check_step(ctx, integrator, dt))) return rc;
  ctx->tsit5_pending = false;
  ctx->tsit5_fsal_valid = false;
  if ((rc = launch_fieldmu_rhs(ctx, mu_dev, ctx->TA.get()))) return rc;
  if (integrator == PDEOPT_INT_IMEX) {
    rc = imex_rocfft_solve(ctx, dt);
    ctx->n_stage_launches += 4;  // r2c, multiply, c2r, axpy (host calls, as pdeopt_sens_advance counts them)
  } else {
    rc = axpy_state(ctx, dt);
    ctx->n_stage_launches++;
  }
  if (rc) return rc;
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  ctx->last_kernel = integrator == PDEOPT_INT_IMEX ? "fieldmu_rhs+imex_rocfft_r2c" : "fieldmu_rhs+euler";
  return PDEOPT_OK;
}

int pdeopt_fieldmu_adjoint_step(pdeopt_ctx* ctx, int integrator, double dt, const void* u_dev, const void* mu_dev,
                                void* lam_dev, void* gmu_dev) {
  return adjoint_step(ctx, integrator, dt, u_dev, mu_dev, lam_dev, gmu_dev, false);
}

int pdeopt_fieldmu_adjoint_step_coef(pdeopt_ctx* ctx, int integrator, double dt, const void* u_dev, const void* mu_dev,
                                     void* lam_dev, void* gmu_dev) {
  return adjoint_step(ctx, integrator, dt, u_dev, mu_dev, lam_dev, gmu_dev, true);
}

int pdeopt_fieldmu_coef_grad_read(pdeopt_ctx* ctx, double* out_host, int n, int reset) {
  if (!ctx) return PDEOPT_EINVAL;
  if (!ctx->configured) return fail(ctx, PDEOPT_ESTATE, "pdeopt_configure has not been called");
  if (!out_host || n != ctx->prob.mob.n)
    return fail(ctx, PDEOPT_EINVAL, "the mobility has %d coefficients (got %d)", ctx->prob.mob.n, n);
  for (int k = 0; k < n; ++k) out_host[k] = 0.0;
  if (!ctx->fieldmu_coef) return PDEOPT_OK;  // no pdeopt_fieldmu_adjoint_step_coef since the buffers were made
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  std::vector<double> slots(ctx->fieldmu_coef_slots);
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(slots.data(), ctx->fieldmu_coef.as<double>(), slots.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (reset) PDEOPT_HIP_CHECK(ctx, hipMemsetAsync(ctx->fieldmu_coef.as<double>(), 0, slots.size() * sizeof(double), ctx->stream));
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t s = 0; s < slots.size(); s += kMaxCoef)  // trajectories, then tiles: one fixed order
    for (int k = 0; k < n; ++k) out_host[k] += slots[s + k];
  return PDEOPT_OK;
}

}  // extern "C"
