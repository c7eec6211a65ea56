// Free energy, dissipation and mass of the resident phase-field state (pdeopt_pf_observables):
// eight fp64 sums per environment, discretised so that they are consistent with the finite-difference right-hand
// sides the stage kernels integrate (stencil_generic.hpp: CH, AC, CH-3D).  With h = hx hy (hz), mu = mu_h(u) -
// kappa lap(u) the 5- / 7-point chemical potential, grad_f the forward difference to the face and D_f the face average
// of D(u):
//   MASS   = h sum u                 U2  = h sum u^2          F_BULK = h sum f_h(u),  f_h' = mu_h, f_h(0) = 0
//   F_GRAD = h sum kappa/2 sum_axes (grad_f u)^2              MU = h sum mu           MU2 = h sum mu^2
//   DISS   = h sum_faces D_f (grad_f mu)^2  (Cahn-Hilliard)   h sum R(u) mu^2  (Allen-Cahn)
//   NONFINITE = number of cells whose u or mu is not finite
// so that d(F_BULK + F_GRAD)/du_ij = h mu_ij and, along u_t = rhs_fd(u), d(F_BULK + F_GRAD)/dt = -DISS (summation by
// parts on the periodic grid).
//
//   2-D   : one pass, one workgroup per 16 x 64 tile and environment.  u on the tile + ring in LDS (2 cells for CH: DISS
//           needs mu at the two forward neighbours; 1 for AC), every row / column index wrapped, so partial tiles and grids
//           smaller than a tile see the periodic field.  mu and D once per cell of the tile (+ its forward row and column
//           for CH) into registers / LDS, then the per-cell terms.
//   3-D   : two passes like the stage kernels -- mu into a work field, then the sums from the forward
//           neighbours of u and mu (a one-pass LDS brick was slower for the stage kernels: stencil_generic.hpp).
//   finish: the workgroups' partial rows of an environment, added in a fixed order, times h.
// Every term is formed in fp64 from the stored values, whatever the state's dtype (as gpe_obs.hip forms its products):
// an fp32 state is read as it is and its mu, D and f_h are evaluated by the fp64 closure classes with the (fp32-rounded)
// parameters the engine carries, so the sums are those of the stored state to fp64 rounding -- with fp32 terms the
// per-cell rounding of mu alone (1e-7 of a value that nearly cancels in MU and DISS) would be the size of the answer's
// own fp32 error.  Partial rows travel as plain stores to a slot only their workgroup owns, there are
// no atomics: a repeat gives identical bits, and an environment's row does not depend on which range was asked for.
#include <algorithm>

#include "block_sums.hpp"
#include "stencil_generic.hpp"

namespace pdeopt {

namespace {

constexpr int kObs = PDEOPT_PF_OBS_COUNT;
constexpr int kTI = 16, kTJ = 64;  // tile of the 2-D kernel: rows x columns (a column per lane)

template <typename T>
struct PfObsArgs {
  const T* u;         // first environment of the range, in the state's dtype
  const double* mu3;  // 3-D: the chemical potential of the first pass
  const EnvParams<double>* ep;  // the range's parameters in fp64 (an fp32 engine's table, converted)
  ClosureSpec mu, mob;
  double rhx, rhy, rhz, rhx2, rhy2, rhz2;
  int nx, ny, nz;
  int64_t bstride;
  double* partial;  // [env][slot][kObs]
};

template <typename T>
__device__ __forceinline__ T xlogx(T c) {
  return c == T(0) ? T(0) : c * t_log<T>(c);
}

// f_h(c) = int_0^c series: a polynomial term by term; a Legendre series on x = 2c - 1 through
// int P_k(2c - 1) dc = (P_{k+1}(x) - P_{k-1}(x)) / (2 (2k + 1)), which vanishes at c = 0, by series_generic's recurrence
template <typename T>
__device__ __forceinline__ T antiderivative_generic(const ClosureSpec& s, const T* __restrict__ coef, T c) {
  T r;
  if (s.kind == PDEOPT_CL_POLY) {
    r = coef[s.n - 1] / T(s.n);
    for (int k = s.n - 2; k >= 0; --k) r = r * c + coef[k] / T(k + 1);
    r *= c;
  } else {
    const T x = T(2) * c - T(1);
    r = coef[0] * c;
    T pm = T(1), pc = x;
    for (int k = 1; k < s.n; ++k) {
      const T pn = (T(2 * k + 1) * x * pc - T(k) * pm) / T(k + 1);
      r += coef[k] * (pn - pm) / T(2 * (2 * k + 1));
      pm = pc;
      pc = pn;
    }
  }
  if (s.flags & PDEOPT_CL_LOGIT_PRIOR) r += xlogx<T>(c) + xlogx<T>(T(1) - c);
  return r;
}

// f_h(c) of the closure class CL (eval_mu's classes)
template <typename T, int CL>
__device__ __forceinline__ T eval_fbulk(const ClosureSpec& s, const T* __restrict__ coef, T c) {
  if constexpr (CL == CL_GENERIC) {
    return antiderivative_generic<T>(s, coef, c);
  } else {
    T r = (((coef[3] * T(0.25) * c + coef[2] * (T(1) / T(3))) * c + coef[1] * T(0.5)) * c + coef[0]) * c;
    if constexpr (CL == CL_LOGIT) r += xlogx<T>(c) + xlogx<T>(T(1) - c);
    return r;
  }
}

// the pointwise terms of one cell
__device__ __forceinline__ void point_terms(double (&acc)[kObs], double c0, double fb, double m) {
  acc[PDEOPT_PF_OBS_MASS] += c0;
  acc[PDEOPT_PF_OBS_U2] += c0 * c0;
  acc[PDEOPT_PF_OBS_F_BULK] += fb;
  acc[PDEOPT_PF_OBS_MU] += m;
  acc[PDEOPT_PF_OBS_MU2] += m * m;
  if (!isfinite(c0) || !isfinite(m)) acc[PDEOPT_PF_OBS_NONFINITE] += 1.0;
}
// D_f (grad_f mu)^2 of one face, the factors of the stage kernels' flux
__device__ __forceinline__ double face_diss(double d0, double dn, double m0, double mn, double rh) {
  const double df = 0.5 * (d0 + dn), g = (mn - m0) * rh;
  return df * g * g;
}
__device__ __forceinline__ double face_grad2(double c0, double cn, double rh) {
  const double g = (cn - c0) * rh;
  return g * g;
}

// grid (tiles_j, tiles_i, envs), 256 threads: wave w owns rows w, w + 4, w + 8, w + 12 of the tile, lane l column l
template <typename T, int EQ, int CL>
__global__ __launch_bounds__(256) void pfobs_tile_kernel(const PfObsArgs<T> a) {
  constexpr bool CH = EQ == PDEOPT_EQ_CAHN_HILLIARD;
  constexpr int HU = CH ? 2 : 1, HM = CH ? 1 : 0;  // rings of u and of mu around the tile
  constexpr int UR = kTI + 2 * HU, UC = kTJ + 2 * HU;
  static_assert(kTJ == 64 && kTI % 4 == 0, "a column per lane, whole trips of the four waves");
  __shared__ T su[UR][UC];  // the state as stored
  __shared__ double sm[kTI + HM][kTJ + HM];
  __shared__ double sd[kTI + HM][kTJ + HM];
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int b = blockIdx.z, i0 = blockIdx.y * kTI, j0 = blockIdx.x * kTJ;
  const int nx = a.nx, ny = a.ny;
  const T* __restrict__ u = a.u + (int64_t)b * a.bstride;
  const EnvParams<double>& p = a.ep[b];

  // tile + ring -> LDS: a row per wave and trip (its wrap is wave-uniform), the column wraps once per thread
  const int jc0 = wrap_idx(j0 - HU + lane, ny), jc1 = wrap_idx(j0 - HU + kTJ + lane, ny);
  for (int r = wave; r < UR; r += 4) {
    const T* __restrict__ row = u + (int64_t)wrap_idx(i0 - HU + r, nx) * ny;
    su[r][lane] = row[jc0];
    if (lane < 2 * HU) su[r][kTJ + lane] = row[jc1];
  }
  __syncthreads();
  auto U = [&](int rr, int cc) -> double { return (double)su[rr][cc]; };

  // mu and D at cell (r, c) of the tile (+ forward ring), the expression of rhs_generic_point
  auto mu_at = [&](int r, int c, double& d) -> double {
    const int rr = r + HU, cc = c + HU;
    const double c0 = U(rr, cc);
    d = eval_mob<double, CL>(a.mob, p.mob, c0);
    return eval_mu<double, CL>(a.mu, p.mu, c0) -
           p.kappa * lap_at<double>(c0, U(rr + 1, cc), U(rr - 1, cc), U(rr, cc + 1), U(rr, cc - 1), a.rhx2, a.rhy2);
  };
  double mr[kTI / 4], dr[kTI / 4];
#pragma unroll
  for (int q = 0; q < kTI / 4; ++q) {
    const int r = wave + 4 * q;
    mr[q] = mu_at(r, lane, dr[q]);
    if constexpr (CH) {
      sm[r][lane] = mr[q];
      sd[r][lane] = dr[q];
    }
  }
  if constexpr (CH) {
    // the forward row (kTJ + 1 cells) and column (kTI cells), dealt over the four waves
    constexpr int NB = kTJ + 1 + kTI;
    const int qb = lane * 4 + wave;
    if (qb < NB) {
      const int r = qb <= kTJ ? kTI : qb - (kTJ + 1), c = qb <= kTJ ? qb : kTJ;
      double d;
      sm[r][c] = mu_at(r, c, d);
      sd[r][c] = d;
    }
    __syncthreads();
  }

  double acc[kObs] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const bool col_ok = j0 + lane < ny;
#pragma unroll
  for (int q = 0; q < kTI / 4; ++q) {
    const int r = wave + 4 * q;
    if (col_ok && i0 + r < nx) {
      const double c0 = U(r + HU, lane + HU);
      point_terms(acc, c0, eval_fbulk<double, CL>(a.mu, p.mu, c0), mr[q]);
      acc[PDEOPT_PF_OBS_F_GRAD] += 0.5 * p.kappa * (face_grad2(c0, U(r + HU + 1, lane + HU), a.rhx) +
                                                    face_grad2(c0, U(r + HU, lane + HU + 1), a.rhy));
      if constexpr (CH) {
        acc[PDEOPT_PF_OBS_DISS] += face_diss(dr[q], sd[r + 1][lane], mr[q], sm[r + 1][lane], a.rhx) +
                                   face_diss(dr[q], sd[r][lane + 1], mr[q], sm[r][lane + 1], a.rhy);
      } else {
        acc[PDEOPT_PF_OBS_DISS] += dr[q] * mr[q] * mr[q];
      }
    }
  }
  const int64_t slot = ((int64_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  block_sums<kObs, 4>(acc, a.partial + slot * kObs);
}

// 3-D, first pass: ch3d_mu_kernel's expression into the work field.  grid (ceil(nz / 64), ceil(ny / 4), nx * envs)
template <typename T, int CL>
__global__ __launch_bounds__(256) void pfobs_mu3_kernel(const PfObsArgs<T> a, double* __restrict__ mu_out) {
  const int nx = a.nx, ny = a.ny, nz = a.nz;
  const int k = blockIdx.x * 64 + (threadIdx.x & 63);
  const int j = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int i = blockIdx.z % nx, b = blockIdx.z / nx;
  if (k >= nz || j >= ny) return;
  const T* __restrict__ u = a.u + (int64_t)b * a.bstride;
  const EnvParams<double>& p = a.ep[b];
  auto U = [&](int ii, int jj, int kk) -> double { return (double)u[((int64_t)ii * ny + jj) * nz + kk]; };
  const int ip = (i + 1 == nx) ? 0 : i + 1, im = (i == 0) ? nx - 1 : i - 1;
  const int jp = (j + 1 == ny) ? 0 : j + 1, jm = (j == 0) ? ny - 1 : j - 1;
  const int kp = (k + 1 == nz) ? 0 : k + 1, km = (k == 0) ? nz - 1 : k - 1;
  const double c = U(i, j, k);
  const double lap = (U(ip, j, k) - 2.0 * c + U(im, j, k)) * a.rhx2 + (U(i, jp, k) - 2.0 * c + U(i, jm, k)) * a.rhy2 +
                     (U(i, j, kp) - 2.0 * c + U(i, j, km)) * a.rhz2;
  mu_out[(int64_t)b * a.bstride + ((int64_t)i * ny + j) * nz + k] = eval_mu<double, CL>(a.mu, p.mu, c) - p.kappa * lap;
}

// 3-D, second pass: the terms of a cell from u and mu at the cell and its three forward neighbours (same grid)
template <typename T, int CL>
__global__ __launch_bounds__(256) void pfobs_sum3_kernel(const PfObsArgs<T> a) {
  const int nx = a.nx, ny = a.ny, nz = a.nz;
  const int k = blockIdx.x * 64 + (threadIdx.x & 63);
  const int j = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int i = blockIdx.z % nx, b = blockIdx.z / nx;
  double acc[kObs] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (k < nz && j < ny) {
    const int64_t base = (int64_t)b * a.bstride;
    const T* __restrict__ u = a.u + base;
    const double* __restrict__ m = a.mu3 + base;
    const EnvParams<double>& p = a.ep[b];
    auto at = [&](int ii, int jj, int kk) -> int64_t { return ((int64_t)ii * ny + jj) * nz + kk; };
    const int ip = (i + 1 == nx) ? 0 : i + 1, jp = (j + 1 == ny) ? 0 : j + 1, kp = (k + 1 == nz) ? 0 : k + 1;
    const int64_t c = at(i, j, k), cx = at(ip, j, k), cy = at(i, jp, k), cz = at(i, j, kp);
    const double c0 = (double)u[c], m0 = m[c], d0 = eval_mob<double, CL>(a.mob, p.mob, c0);
    const double ux = (double)u[cx], uy = (double)u[cy], uz = (double)u[cz];
    point_terms(acc, c0, eval_fbulk<double, CL>(a.mu, p.mu, c0), m0);
    acc[PDEOPT_PF_OBS_F_GRAD] += 0.5 * p.kappa * (face_grad2(c0, ux, a.rhx) + face_grad2(c0, uy, a.rhy) + face_grad2(c0, uz, a.rhz));
    acc[PDEOPT_PF_OBS_DISS] += face_diss(d0, eval_mob<double, CL>(a.mob, p.mob, ux), m0, m[cx], a.rhx) +
                               face_diss(d0, eval_mob<double, CL>(a.mob, p.mob, uy), m0, m[cy], a.rhy) +
                               face_diss(d0, eval_mob<double, CL>(a.mob, p.mob, uz), m0, m[cz], a.rhz);
  }
  const int64_t slot = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;  // blockIdx.z = b nx + i
  block_sums<kObs, 4>(acc, a.partial + slot * kObs);
}

// one wave per environment: its partial rows in a fixed order, the sums times h (the count as it is)
__global__ __launch_bounds__(64) void pfobs_finish_kernel(const double* __restrict__ partial, int slots, double h,
                                                          double* __restrict__ out) {
  const int env = blockIdx.x, lane = threadIdx.x;
  double s[kObs] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  rows_total<kObs>(partial + (int64_t)env * slots * kObs, slots, lane, s);
#pragma unroll
  for (int c = 0; c < kObs; ++c) s[c] = wave_sum(s[c]);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < kObs; ++c) out[(int64_t)env * kObs + c] = c == PDEOPT_PF_OBS_NONFINITE ? s[c] : s[c] * h;
  }
}

// the parameters of the environments [first, first + count) in fp64: an fp64 engine's own table, else the fp32 table's
// values widened (kappa and the coefficients are what the engine carries) and uploaded to `dev`
template <typename T>
int params_fp64(pdeopt_ctx* ctx, int first, int count, EnvParams<double>* dev, std::vector<EnvParams<double>>& host,
                const EnvParams<double>** out) {
  if constexpr (sizeof(T) == 8) {
    *out = env_params<double>(ctx, first);
  } else {
    const auto* e = reinterpret_cast<const EnvParams<float>*>(ctx->env_params_host.data()) + first;
    host.assign((size_t)count, EnvParams<double>{});
    for (int b = 0; b < count; ++b) {
      host[b].kappa = (double)e[b].kappa;
      for (int k = 0; k < kMaxCoef; ++k) {
        host[b].mu[k] = (double)e[b].mu[k];
        host[b].mob[k] = (double)e[b].mob[k];
      }
    }
    PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(dev, host.data(), sizeof(EnvParams<double>) * (size_t)count, hipMemcpyHostToDevice, ctx->stream));
    *out = dev;
  }
  return PDEOPT_OK;
}

template <typename T>
int pf_observables_t(pdeopt_ctx* ctx, int env_first, int env_count, double* host_out) {
  const pdeopt_problem& p = ctx->prob;
  const bool is3d = p.equation == PDEOPT_EQ_CAHN_HILLIARD_3D;
  const int nz = is3d ? p.nz : 1;
  const dim3 grid = is3d ? dim3((nz + 63) / 64, (p.ny + 3) / 4, (unsigned)(p.nx * env_count))
                         : dim3((p.ny + kTJ - 1) / kTJ, (p.nx + kTI - 1) / kTI, env_count);
  if (grid.y > 65535u || grid.z > 65535u)
    return fail(ctx, PDEOPT_EINVAL, "pf_observables: grid too large (nx=%d ny=%d environments=%d)", p.nx, p.ny, env_count);
  const int64_t slots = (int64_t)grid.x * grid.y * (is3d ? p.nx : 1);  // per environment
  const int64_t cells = (int64_t)p.nx * p.ny * nz;
  // one block: the rows [envs][8], the partial rows [envs][slots][8], 3-D: mu [envs][cells], fp32: the fp64 parameters
  const size_t n_out = (size_t)kObs * env_count, n_part = n_out * (size_t)slots, n_mu = is3d ? (size_t)cells * env_count : 0;
  const size_t need = sizeof(double) * (n_out + n_part + n_mu) + sizeof(EnvParams<double>) * (size_t)env_count;
  if (const int rc = grow_device_buffer(ctx, ctx->pf_obs_dev, need, /*sync_first=*/true)) return rc;
  double* const out = ctx->pf_obs_dev.as<double>();
  double* const mu3 = out + n_out + n_part;
  PfObsArgs<T> a{};
  std::vector<EnvParams<double>> widened;
  int rc = params_fp64<T>(ctx, env_first, env_count, reinterpret_cast<EnvParams<double>*>(mu3 + n_mu), widened, &a.ep);
  if (rc) return rc;
  a.bstride = cells;
  a.u = ctx->Y.as<const T>() + (int64_t)env_first * cells;
  a.mu3 = mu3;
  a.mu = closure_spec(p.mu);
  a.mob = closure_spec(p.mob);
  const GridRecip r = grid_recip(p);
  set_recip_plain(a, r);
  a.rhz = is3d ? r.rz : 0.0;
  a.rhz2 = is3d ? r.rz2 : 0.0;
  a.nx = p.nx;
  a.ny = p.ny;
  a.nz = nz;
  a.partial = out + n_out;
  const int cl = classify_closures(p.mu, p.mob);
  rc = with_closure_class<CL_GENERIC, CL_POLY, CL_LOGIT>(cl, [&](auto c) -> int {
    constexpr int CL = decltype(c)::value;
    if (is3d) {
      hipLaunchKernelGGL((pfobs_mu3_kernel<T, CL>), grid, dim3(256), 0, ctx->stream, a, mu3);
      hipLaunchKernelGGL((pfobs_sum3_kernel<T, CL>), grid, dim3(256), 0, ctx->stream, a);
    } else if (p.equation == PDEOPT_EQ_CAHN_HILLIARD) {
      hipLaunchKernelGGL((pfobs_tile_kernel<T, PDEOPT_EQ_CAHN_HILLIARD, CL>), grid, dim3(256), 0, ctx->stream, a);
    } else {
      hipLaunchKernelGGL((pfobs_tile_kernel<T, PDEOPT_EQ_ALLEN_CAHN, CL>), grid, dim3(256), 0, ctx->stream, a);
    }
    return PDEOPT_OK;
  });
  if (rc) return rc;
  const double h = p.hx * p.hy * (is3d ? p.hz : 1.0);
  hipLaunchKernelGGL(pfobs_finish_kernel, dim3(env_count), dim3(64), 0, ctx->stream, (const double*)a.partial, (int)slots, h, out);
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(host_out, out, sizeof(double) * n_out, hipMemcpyDeviceToHost, ctx->stream));
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->last_kernel = std::string("pf_obs<") + (is3d ? "CH-3D" : equation_short_name(p.equation)) + "," + dtype_name<T>() + "," +
                     closure_class_name(cl) + ">";
  return PDEOPT_OK;
}

}  // namespace

int pf_observables(pdeopt_ctx* ctx, int env_first, int env_count, double* host_out) {
  const pdeopt_problem& p = ctx->prob;
  if (p.equation != PDEOPT_EQ_CAHN_HILLIARD && p.equation != PDEOPT_EQ_ALLEN_CAHN && p.equation != PDEOPT_EQ_CAHN_HILLIARD_3D)
    return fail(ctx, PDEOPT_EINVAL, "pf_observables covers the periodic Cahn-Hilliard (2-D, 3-D) and Allen-Cahn equations; the "
                "smoothed-boundary, Butler-Volmer, advection-diffusion and GPE classes have no free energy here (equation %d)", p.equation);
  if (ctx->halo) return fail(ctx, PDEOPT_EINVAL, "pf_observables is not available in the padded (domain-decomposition) layout");
  if (p.derivs != PDEOPT_DERIVS_FD)
    return fail(ctx, PDEOPT_EINVAL, "pf_observables is discretised with the finite-difference right-hand side (derivs = \"fd\")");
  if (p.mu.kind == PDEOPT_CL_JIT || p.mob.kind == PDEOPT_CL_JIT)
    return fail(ctx, PDEOPT_EINVAL, "pf_observables needs mu in the in-kernel family: a run-time-compiled closure has no antiderivative here");
  if (p.mu.flags & (PDEOPT_CL_MIX_ENTROPY | PDEOPT_CL_EXP_WRAP))
    return fail(ctx, PDEOPT_EINVAL, "pf_observables: mu with the %s flag has no closed-form antiderivative",
                (p.mu.flags & PDEOPT_CL_MIX_ENTROPY) ? "mixing-entropy" : "exp-wrap");
  if (!env_count) return PDEOPT_OK;
  return with_dtype(ctx, [&](auto tag) { return pf_observables_t<decltype(tag)>(ctx, env_first, env_count, host_out); });
}

}  // namespace pdeopt
