// Host-side dispatch of the fused stencil + integrator-stage kernels (explicit integrators).
//
// Replaces the body of diffrax.diffeqsolve's while-loop for explicit solvers at the call sites
// pde_opt/pde_env.py:293-303 and pde_opt/pde_model.py:120-134: one kernel per Runge-Kutta stage,
// each evaluating equation.rhs on the stage input and applying the stage's axpy updates in the
// same pass.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "stencil_generic.hpp"
#include "stencil_tiled.hpp"
#include "stencil_fused.hpp"
#include "stencil_fused_ac.hpp"
#include "stencil_fused_ac4.hpp"
#include "stencil_fused_ch4.hpp"
#include "stencil_fused_launch.hpp"
#include "stencil_small.hpp"
#include "stencil_small_adaptive.hpp"
#include "stencil_coop_adaptive.hpp"
#include "stencil_sbm_tiled.hpp"
#include "groups.hpp"

namespace pdeopt {

namespace {

template <typename T>
StageArgs<T> make_args(pdeopt_ctx* ctx, const Window& w, double t, const void* in, const void* y, void* out, void* acc,
                       double a, double b, int out_mode, int acc_mode) {
  const pdeopt_problem& p = ctx->prob;
  StageArgs<T> s{};
  // environment window [w.lo, w.lo + w.n): pointers are pre-offset, kernels see a batch of w.n
  s.g = make_geo(ctx);
  const int64_t woff = (int64_t)w.lo * s.g.bstride;
  s.in = static_cast<const T*>(in) + woff;
  s.y = static_cast<const T*>(y) + woff;
  s.out = out ? static_cast<T*>(out) + woff : nullptr;
  s.acc = acc ? static_cast<T*>(acc) + woff : nullptr;
  s.a = T(a);
  s.b = T(b);
  const GridRecip r = grid_recip(p);
  set_recip_plain(s, r);
  s.rhz = p.nz > 1 ? T(r.rz) : T(0);
  s.rhz2 = p.nz > 1 ? T(r.rz2) : T(0);
  s.mu3 = nullptr;
  set_closures<T>(s, ctx, w.lo);
  s.vstride = ctx->aux[PDEOPT_AUX_VX_FACE].per_env ? (int64_t)p.nx * p.ny : 0;
  s.vx = ctx->aux[PDEOPT_AUX_VX_FACE].dev.as<const T>();
  s.vy = ctx->aux[PDEOPT_AUX_VY_FACE].dev.as<const T>();
  if (s.vx) s.vx += w.lo * s.vstride;
  if (s.vy) s.vy += w.lo * s.vstride;
  s.psi = ctx->aux[PDEOPT_AUX_SBM_PSI].dev.as<const T>();
  s.ngp = ctx->aux[PDEOPT_AUX_SBM_NORM_GRAD].dev.as<const T>();
  s.mask = ctx->aux[PDEOPT_AUX_SBM_MASK].dev.as<const T>();
  s.fe = closure_spec(p.fe);
  // (Butler-Volmer at a given voltage: tv[0] is the voltage protocol's v(t), added to the per-environment v)
  if (p.equation == PDEOPT_EQ_ALLEN_CAHN_SBM || p.equation == PDEOPT_EQ_CAHN_HILLIARD_SBM || bv_equation(p.equation)) {
    double tv[3] = {ctx->time_const[0], ctx->time_const[1], ctx->time_const[2]};
    // the table of pdeopt_set_time_table first (stage times arrive in order: resume at the cursor), the host callback
    // for times it does not hold
    bool found = false;
    const size_t nt = ctx->tt_times.size();
    for (size_t q = 0; q < nt && !found; ++q) {
      const size_t i = (ctx->tt_cursor + q) % nt;
      if (ctx->tt_times[i] == t) {
        for (int c = 0; c < 3; ++c) tv[c] = ctx->tt_terms[3 * i + c];
        ctx->tt_cursor = i;
        found = true;
      }
    }
    if (!found && ctx->time_fn) ctx->time_fn(t, tv, ctx->time_user);
    // a table that does not hold this stage time and no callback to ask: the constant terms would be used silently
    // (a caller whose times differ from the library's t0 + s dt, + dt/2 arithmetic by an ulp) -- pdeopt_advance reports it
    if (!found && !ctx->time_fn && nt) ctx->tt_misses++;
    s.tw_a = T(tv[0]);
    s.tw_b = T(tv[1]);
    s.tsrc = T(tv[2]);
    for (int c = 0; c < 3; ++c) ctx->time_last[c] = tv[c];
  }
  s.out_mode = out_mode;
  s.acc_mode = acc_mode;
  s.scaled = ctx->slope_scaled ? 1 : 0;
  s.dbg = (int)ctx->opt_debug_ablate;
  return s;
}

template <typename T>
int launch_generic(pdeopt_ctx* ctx, const Window& w, const StageArgs<T>& s) {
  const pdeopt_problem& p = ctx->prob;
  dim3 block(64, 4, 1);
  dim3 grid((p.ny + 63) / 64, (p.nx + 3) / 4, w.n);
  if (grid.y > 65535u || grid.z > 65535u)
    return fail(ctx, PDEOPT_EINVAL, "grid too large for the generic kernel (nx=%d batch=%d)", p.nx,
                p.batch);
  if (jit_closures_active(ctx)) return launch_jit_stage<T>(ctx, w, s);  // closures compiled at run time (jit.hip)
  if (p.equation == PDEOPT_EQ_CAHN_HILLIARD_3D) {
    // two passes: chemical potential into the work field, then the flux divergence + stage update
    const int nz = s.g.nz;
    dim3 g3((nz + 63) / 64, (p.ny + 3) / 4, (unsigned)(p.nx * w.n));
    if (g3.y > 65535u || g3.z > 65535u) return fail(ctx, PDEOPT_EINVAL, "grid too large for the 3-D kernels");
    int rc = ensure_buffer(ctx, ctx->KS, ctx->total_bytes);
    if (rc) return rc;
    StageArgs<T> s3 = s;
    s3.mu3 = ctx->KS.as<const T>() + (int64_t)w.lo * s.g.bstride;
    const int cl = classify_closures(p.mu, p.mob);
    ctx->last_kernel = cl == CL_GENERIC ? "stage_generic<CH-3D>" : std::string("stage_generic<CH-3D,") + closure_class_name(cl) + ">";
    return with_closure_class<CL_GENERIC, CL_POLY, CL_LOGIT>(cl, [&](auto c) -> int {
      constexpr int CL = decltype(c)::value;
      hipLaunchKernelGGL((ch3d_mu_kernel<T, CL>), g3, block, 0, w.stream, s3, const_cast<T*>(s3.mu3));
      hipLaunchKernelGGL((ch3d_stage_kernel<T, CL>), g3, block, 0, w.stream, s3);
      PDEOPT_HIP_CHECK(ctx, hipGetLastError());
      return PDEOPT_OK;
    });
  }
  // the one-pass generic kernel of equation EQ; named "stage_generic<short name>"
  auto generic = [&](auto eq_c, const char* short_name) {
    hipLaunchKernelGGL((stage_generic_kernel<T, decltype(eq_c)::value>), grid, block, 0, w.stream, s);
    ctx->last_kernel = std::string("stage_generic<") + short_name + ">";
  };
  switch (p.equation) {
    case PDEOPT_EQ_CAHN_HILLIARD:
      generic(int_c<PDEOPT_EQ_CAHN_HILLIARD>{}, "CH");
      break;
    case PDEOPT_EQ_ALLEN_CAHN:
      generic(int_c<PDEOPT_EQ_ALLEN_CAHN>{}, "AC");
      break;
    case PDEOPT_EQ_ADVECTION_DIFFUSION:
      if (!s.vx || !s.vy)
        return fail(ctx, PDEOPT_ESTATE, "advection-diffusion needs VX_FACE and VY_FACE aux fields");
      generic(int_c<PDEOPT_EQ_ADVECTION_DIFFUSION>{}, "AD");
      break;
    case PDEOPT_EQ_SHAPE_SMOOTH:
      if (ctx->halo) return fail(ctx, PDEOPT_EINVAL, "shape smoothing needs the periodic layout");
      generic(int_c<PDEOPT_EQ_SHAPE_SMOOTH>{}, "shape-smooth");
      break;
    case PDEOPT_EQ_ALLEN_CAHN_SBM:
    case PDEOPT_EQ_CAHN_HILLIARD_SBM:
      if (!s.psi || !s.ngp || !s.mask)
        return fail(ctx, PDEOPT_ESTATE, "smoothed-boundary equations need the SBM_PSI, SBM_NORM_GRAD and SBM_MASK aux fields");
      if (ctx->halo) return fail(ctx, PDEOPT_EINVAL, "smoothed-boundary equations need the periodic layout");
      if (sbm_tiled_supported<T>(ctx)) {
        const int rc_t = launch_sbm_tiled<T>(ctx, w, s);
        if (rc_t) return rc_t;
        break;
      }
      if (p.equation == PDEOPT_EQ_ALLEN_CAHN_SBM) {
        generic(int_c<PDEOPT_EQ_ALLEN_CAHN_SBM>{}, "AC-SBM");
      } else if (ctx->opt_fuse_stages < 0 ||
                 (ctx->opt_fuse_stages == 0 && (int64_t)p.nx * p.ny * w.n < (1 << 18))) {
        // the literal one-pass form (inner re-evaluated at 5 points per cell): one launch instead of two, faster
        // on the notebook-sized grids (128^2: 7.0 vs 7.7 us per evaluation); PDEOPT_OPT_FUSE_STAGES = 1 / -1
        // force the two-pass / the literal form
        generic(int_c<PDEOPT_EQ_CAHN_HILLIARD_SBM>{}, "CH-SBM");
      } else {
        // two passes: inner once per cell into the work field, then the psi-weighted flux divergence
        // (1024^2 fp32: 24.8 vs 30.6 us per evaluation; both forms are L2-bound one-thread-per-cell kernels)
        int rc = ensure_buffer(ctx, ctx->KS, ctx->total_bytes);
        if (rc) return rc;
        StageArgs<T> s2 = s;
        s2.mu3 = ctx->KS.as<const T>() + (int64_t)w.lo * s.g.bstride;
        hipLaunchKernelGGL(sbm_inner_kernel<T>, grid, block, 0, w.stream, s2, const_cast<T*>(s2.mu3));
        hipLaunchKernelGGL(sbm_ch_stage_kernel<T>, grid, block, 0, w.stream, s2);
        ctx->last_kernel = "stage_two_pass<CH-SBM>";
      }
      break;
    default:
      return fail(ctx, PDEOPT_EINVAL, "equation %d has no explicit RHS kernel", p.equation);
  }
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  return PDEOPT_OK;
}

// pointwise stage update for RHS evaluations that are not fused into a stencil kernel
template <typename T>
__global__ void stage_update_kernel(const StageArgs<T> a, const T* __restrict__ k, int64_t total, int64_t env_elems) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t st = (int64_t)gridDim.x * blockDim.x;
  for (; i < total; i += st) stage_update<T>(a, i, a.scaled ? k[i] * a.ep[i / env_elems].kscale : k[i]);
}

// field of environment b *= ratio[b]
template <typename T>
__global__ void env_scale_kernel(T* __restrict__ f, const double* __restrict__ ratio, int64_t env_elems) {
  const int b = blockIdx.y;
  const T r = (T)ratio[b];
  T* p = f + (int64_t)b * env_elems;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < env_elems; i += (int64_t)gridDim.x * blockDim.x) p[i] *= r;
}

template <typename T>
int launch_stage_fourier(pdeopt_ctx* ctx, const Window& w, const StageArgs<T>& s, const void* in, void* out) {
  if (w.lo != 0 || w.n != ctx->prob.batch)
    return fail(ctx, PDEOPT_EINVAL, "spectral RHS works on the whole batch");
  int rc;
  if (s.out_mode == OUT_K && s.acc_mode == ACC_NONE && !s.scaled) return rhs_fourier(ctx, in, out);
  if ((rc = ensure_buffer(ctx, ctx->KS, ctx->total_bytes))) return rc;
  if ((rc = rhs_fourier(ctx, in, ctx->KS.get()))) return rc;
  const int64_t total = (int64_t)(ctx->env_elems * ctx->prob.batch);
  const int blocks = (int)std::min<int64_t>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(stage_update_kernel<T>, dim3(blocks), dim3(256), 0, ctx->stream, s, ctx->KS.as<const T>(), total,
                     (int64_t)ctx->env_elems);
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  return PDEOPT_OK;
}

// What every per-stage launch does: bring the advection velocities to the stage time, fill the arguments (`extra`
// adds what only one caller sets), count the launch and take the fourier, tiled or generic path.
// refuse_forced_tiled: PDEOPT_OPT_KERNEL_PATH = 2 on a shape the tiled kernel does not cover is an error (the plain stage launch) or falls through to the generic kernel (the linear-combination launch)
template <typename T, typename Extra>
int launch_stage_path(pdeopt_ctx* ctx, const Window& w, double t, const void* in, const void* y, void* out, void* acc, double a,
                      double b, int out_mode, int acc_mode, bool refuse_forced_tiled, Extra&& extra) {
  if (ctx->prob.equation == PDEOPT_EQ_ADVECTION_DIFFUSION) {
    // velocity_fn(t, x, y): face velocities at the time of THIS right-hand side (t = stage time)
    int rc;
    if ((rc = refresh_time_aux(ctx, PDEOPT_AUX_VX_FACE, t))) return rc;
    if ((rc = refresh_time_aux(ctx, PDEOPT_AUX_VY_FACE, t))) return rc;
  }
  StageArgs<T> s = make_args<T>(ctx, w, t, in, y, out, acc, a, b, out_mode, acc_mode);
  extra(s);
  ctx->n_stage_launches++;
  if (bv_equation(ctx->prob.equation)) {
    if (ctx->prob.derivs != PDEOPT_DERIVS_FD || ctx->halo)
      return fail(ctx, PDEOPT_EINVAL, "the Butler-Volmer equations run finite differences on the periodic layout only");
    return launch_bv_stage<T>(ctx, w, s);
  }
  if (ctx->prob.derivs == PDEOPT_DERIVS_FOURIER) return launch_stage_fourier<T>(ctx, w, s, in, out);
  if (ctx->opt_kernel_path != 1 && tiled_supported<T>(ctx)) return launch_tiled<T>(ctx, w, s);
  if (refuse_forced_tiled && ctx->opt_kernel_path == 2)
    return fail(ctx, PDEOPT_EINVAL, "LDS-tiled kernel forced but shape %dx%d / equation %d is not covered",
                ctx->prob.nx, ctx->prob.ny, ctx->prob.equation);
  return launch_generic<T>(ctx, w, s);
}

// One fused stage: k = rhs(in); out/acc updated per (out_mode, acc_mode).
int launch_stage(pdeopt_ctx* ctx, const Window& w, double t, const void* in, const void* y, void* out, void* acc, double a,
                 double b, int out_mode, int acc_mode) {
  return with_dtype(ctx, [&](auto tag) {
    using T = decltype(tag);
    return launch_stage_path<T>(ctx, w, t, in, y, out, acc, a, b, out_mode, acc_mode, /*refuse_forced_tiled=*/true, [](StageArgs<T>&) {});
  });
}

// k = rhs(in) -> kout, and  next = y + sum_{j<n} c[j] K[j] + c[n] k  in the same pass (OUT_K_LC)
template <typename T>
int launch_stage_lc(pdeopt_ctx* ctx, const Window& w, double t, const void* in, const void* y, void* kout, const DeviceBuffer* ks, const double* c,
                    int n, void* next) {
  return launch_stage_path<T>(ctx, w, t, in, y, kout, nullptr, 0.0, 0.0, OUT_K_LC, ACC_NONE, /*refuse_forced_tiled=*/false, [&](StageArgs<T>& s) {
    const int64_t woff = (int64_t)w.lo * s.g.bstride;
    for (int j = 0; j < n; ++j) {
      s.lc.k[j] = ks[j].as<const T>() + woff;
      s.lc.c[j] = T(c[j]);
    }
    s.lc.c[n] = T(c[n]);
    s.lc.n = n;
    s.lc.next = static_cast<T*>(next) + woff;
  });
}

int launch_pair_dt(pdeopt_ctx* ctx, const Window& w, const HaloIo& io, int pair, const void* in, const void* y, const void* acc, void* out,
                   void* acc_out, double aA, double bA, double aB, double bB) {
  return with_dtype(ctx, [&](auto t) { return launch_pair<decltype(t)>(ctx, w, io, pair, in, y, acc, out, acc_out, aA, bA, aB, bB); });
}

template <typename T>
__global__ void lerp_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ out,
                            T theta, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) out[i] = a[i] + theta * (b[i] - a[i]);
}

}  // namespace

int launch_rhs(pdeopt_ctx* ctx, const Window& w, const void* in, void* out, double t) {
  return launch_stage(ctx, w, t, in, in, out, nullptr, 0.0, 0.0, OUT_K, ACC_NONE);
}

#ifndef PDEOPT_IMEX_SLOPE_PAIR
#define PDEOPT_IMEX_SLOPE_PAIR 1
#endif
int launch_rhs_slope(pdeopt_ctx* ctx, const Window& w, const void* in, void* out, double t) {
#if PDEOPT_IMEX_SLOPE_PAIR
  if (ctx->prob.derivs == PDEOPT_DERIVS_FD && ctx->prob.nz <= 1 && !ctx->time_fn) {
    return with_dtype(ctx, [&](auto tag) {
      using T = decltype(tag);
      return slope_pair_supported<T>(ctx) ? launch_slope_pair<T>(ctx, w, in, out) : launch_rhs(ctx, w, in, out, t);
    });
  }
#endif
  return launch_rhs(ctx, w, in, out, t);
}

namespace {
constexpr int kGraphUnit = 16;  // substeps per captured graph (even: ping-pong buffers return)

// The kernel families of the explicit fixed-step path: what runs a substep.
enum ExplicitKernel {
  EK_COOP_FIXED, EK_SMALL_STEP,  // all substeps in one launch: several compute units per environment (stencil_coop_adaptive.hpp, MODE 1) / one (stencil_small.hpp)
  EK_EULER_STAGE, EK_EULER_PAIR,  // one launch per Euler substep / per two of them (the stage-pair kernel), an odd last one on its own
  EK_RK4_STAGE, EK_RK4_PAIRS,  // one launch per RK4 stage / stages 1+2 and 3+4 as two temporally fused launches (7 words/cell instead of 16)
  EK_AC_SINGLE,  // Allen-Cahn fp32: the whole RK4 substep in one pass (2 words per cell instead of 7)
  EK_CH_SINGLE,  // Cahn-Hilliard fp32, periodic divisible grids: the same (stencil_fused_ch4.hpp)
};
inline bool is_rk4(ExplicitKernel k) { return k >= EK_RK4_STAGE; }
// launches of one RK4 substep = the points at which a phase-wise caller may do work of its own
inline int rk4_phases(ExplicitKernel k) { return k == EK_RK4_STAGE ? 4 : k == EK_RK4_PAIRS ? 2 : 1; }

// do the fused stage-pair kernels (stencil_fused.hpp, stencil_fused_ac.hpp) cover the configured problem?
bool stage_pairs_available(const pdeopt_ctx* ctx) {
  return ctx->opt_kernel_path != 1 && ctx->prob.derivs == PDEOPT_DERIVS_FD &&
         with_dtype(ctx, [&](auto t) { return fused_supported<decltype(t)>(ctx); });
}

// Which family runs an RK4 substep of the configured problem.  phased: the substep is driven phase by phase (pdeopt_rk4_phase,
// the decomposed drivers) -- a single-pass kernel exists there for the halo-8 layout only, whose 8-cell halo is that kernel's
// tile + 8 input, and that layout has stage pairs for Cahn-Hilliard only.  PDEOPT_OPT_FUSE_STAGES = 1 keeps the stage pairs.
ExplicitKernel rk4_family(const pdeopt_ctx* ctx, bool phased) {
  if (!phased && ac_quad_supported(ctx)) return EK_AC_SINGLE;
  if ((!phased || ctx->halo == 8) && ch_quad_chosen(ctx)) return EK_CH_SINGLE;
  if (stage_pairs_available(ctx) && (ctx->halo != 8 || ctx->prob.equation == PDEOPT_EQ_CAHN_HILLIARD)) return EK_RK4_PAIRS;
  return EK_RK4_STAGE;
}

// Does the whole-environment-step kernel (stencil_small.hpp) take this advance?  PDEOPT_OPT_SMALL_PERSIST: 1 = wherever
// it can run, -1 = never, 0 = auto: grids of at most 64^2-class size (<= 4096 cells: one launch instead of 2 n
// dependent ones, measured 2.7-4.8 x faster per environment step), and larger LDS-resident grids once enough
// environments run side by side to fill the chip's compute units (>= 192) -- a single 128^2 environment is faster on
// the tiled kernels, which spread it over 8+ CUs, than on one CU.
bool small_chosen(const pdeopt_ctx* ctx, int integrator, int64_t n) {
  if (ctx->opt_small_persist < 0 || ctx->opt_kernel_path == 1 || ctx->opt_debug_ablate) return false;
  if (integrator != PDEOPT_INT_EULER && integrator != PDEOPT_INT_RK4) return false;
  if (!with_dtype(ctx, [&](auto t) { return small_supported<decltype(t)>(ctx); })) return false;
  if (ctx->opt_small_persist > 0) return true;
  if (!tiled_knobs_untouched(ctx)) return false;
  const int64_t cells = (int64_t)ctx->prob.nx * ctx->prob.ny;
  if (n < 2) return false;
  return cells <= kSmallAutoCells || ctx->prob.batch >= kSmallAutoBatch;
}

// Everything advance_explicit decides before it launches: the kernel family and the schedule.  plan_explicit fills it;
// it allocates nothing, launches nothing and writes nothing into the ctx.
struct ExplicitPlan {
  ExplicitKernel kernel;
  int fuse_stages;    // PDEOPT_OPT_FUSE_STAGES the stage pairs were chosen under (part of a captured graph's key), else 0
  int group;          // environments per group (groups.hpp); the batch: one sweep
  bool side_by_side;  // two groups in flight on two streams
  bool graph;         // capture kGraphUnit substeps into a hipGraph and replay it
  bool timed;         // time-dependent terms evaluated by the host per stage (smoothed-boundary scalars, advection velocities)
};
ExplicitPlan plan_explicit(const pdeopt_ctx* ctx, int integrator, int64_t n) {
  const int batch = ctx->prob.batch;
  ExplicitPlan p{};
  p.group = batch;
  // one environment (or a few) of a mid-sized grid: several compute units per environment, all substeps in one launch
  const bool coop = with_dtype(ctx, [&](auto t) { return coop_fixed_chosen<decltype(t)>(ctx, integrator, n); });
  const bool small = small_chosen(ctx, integrator, n);
  const bool f64 = ctx->prob.dtype == PDEOPT_F64;  // (64^2 fp64: 0.70 ms against the one-CU kernel's 1.14, which small_chosen would pick)
  // Euler: two substeps per launch through the stage-pair kernels where they exist
  //   PAIR_12 with aA = bA = bB = dt:  w = y + dt f(y),  ACC = y + dt f(y) + dt f(w) = two Euler steps
  if (coop && (ctx->opt_small_persist == 2 || f64 || !small)) p.kernel = EK_COOP_FIXED;
  else if (small) p.kernel = EK_SMALL_STEP;
  else if (integrator == PDEOPT_INT_EULER) p.kernel = n >= 2 && stage_pairs_available(ctx) ? EK_EULER_PAIR : EK_EULER_STAGE;
  else p.kernel = rk4_family(ctx, /*phased=*/false);
  if (p.kernel <= EK_SMALL_STEP) return p;  // one launch holds every environment and every substep
  if (p.kernel == EK_RK4_PAIRS) p.fuse_stages = (int)ctx->opt_fuse_stages;

  // Environments are independent, so the substep loop may run group by group: a group whose working set (4 fields x
  // group x nx x ny) fits the 256 MiB Infinity Cache keeps every stage's reads and writes on-die for all n substeps
  // instead of streaming the whole batch through HBM once per stage.
  p.timed = ctx->prob.equation == PDEOPT_EQ_ALLEN_CAHN_SBM || ctx->prob.equation == PDEOPT_EQ_CAHN_HILLIARD_SBM ||
            has_time_aux(ctx, PDEOPT_AUX_VX_FACE) || has_time_aux(ctx, PDEOPT_AUX_VY_FACE) ||
            bv_time_dependent(ctx);  // (a voltage protocol v(t): the whole batch per sweep, no graph)
  const bool fd = ctx->prob.derivs == PDEOPT_DERIVS_FD;
  const bool ch3d = ctx->prob.equation == PDEOPT_EQ_CAHN_HILLIARD_3D;
  if (!fd || p.timed) p.group = batch;  // batched rocFFT plans cover the whole batch; host callbacks run once per stage time
  else if (ctx->opt_group_envs > 0) p.group = (int)std::min<int64_t>(ctx->opt_group_envs, batch);
  else if (ctx->opt_group_envs == 0) {
    // auto: largest balanced group whose 4 fields fit the Infinity Cache (measured on MI355X: 32 x 1024^2 fp32 runs
    // 13-16 % faster as 2 groups of 16 = 256 MiB than as one 512 MiB sweep; smaller groups lose more to per-launch
    // ramp/tail than they gain)
    if (n > 1) p.group = cache_group(batch, 4 * ctx->env_elems * ctx->esize, 256ull << 20, false);
    // Two groups side by side on two streams, each half the size (the same resident working set): a launch of the
    // stage kernels is 3-6 rounds of resident workgroups, its ramp and its tail leave compute units idle, and the
    // next launch of the SAME group depends on it -- the other group's does not.
    if (p.group < batch && ctx->opt_group_streams != 1 && p.group >= 2 && !ch3d) {
      p.group = (p.group + 1) / 2;
      p.side_by_side = true;
    }
  }
  const bool can_pair = !p.timed && fd && !ch3d;
  if (ctx->opt_group_streams == 2 && can_pair && p.group < batch) p.side_by_side = true;
  // ... and a batch that fits the cache as one group runs as two halves side by side for the same reason (measured
  // 512^2 x 64 Allen-Cahn: 20.1 k env-steps/s against 18.9 k), unless it is small enough for the hipGraph replay below
  if (ctx->opt_group_streams == 0 && ctx->opt_group_envs == 0 && can_pair && p.group >= batch && batch >= 2 && n > 1 &&
      ctx->opt_graph <= 0 && (int64_t)ctx->prob.nx * ctx->prob.ny * batch > (1 << 21)) {
    p.group = (batch + 1) / 2;
    p.side_by_side = true;
  }
  // launch-bound regime (small grids / few environments: a stage kernel runs for a few microseconds, the host needs ~3.5 us to issue one): replay_graph
  const int64_t cells_per_launch = (int64_t)ctx->prob.nx * ctx->prob.ny * p.group;
  p.graph = !p.timed && ctx->opt_graph >= 0 && p.group >= batch && fd && n >= 2 * kGraphUnit &&
            (ctx->opt_graph > 0 || cells_per_launch <= (1 << 20));
  return p;
}

// The work fields the launches of a family use, allocated before the first of them.
int ensure_work_fields(pdeopt_ctx* ctx, ExplicitKernel k) {
  int rc;
  if ((rc = ensure_buffer(ctx, ctx->TA, ctx->total_bytes))) return rc;
  if ((is_rk4(k) || k == EK_EULER_PAIR) && (rc = ensure_buffer(ctx, ctx->TB, ctx->total_bytes))) return rc;
  if (is_rk4(k) && (rc = ensure_buffer(ctx, ctx->ACC, ctx->total_bytes))) return rc;
  // work field of the two-pass 3-D right-hand side: allocated here, never inside a stream capture
  const bool ks = ctx->prob.equation == PDEOPT_EQ_CAHN_HILLIARD_3D || bv_equation(ctx->prob.equation);
  return ks ? ensure_buffer(ctx, ctx->KS, ctx->total_bytes) : PDEOPT_OK;
}

// Launch `ph` of an RK4 substep of family k on the window: Y holds the state, TA takes the new one (one launch per stage: TA
// is a stage input and stage 4 puts the new state into Y in place -- y is only touched pointwise); TB and ACC are the ctx's.
// t is the time of the stage launched; it only matters to time-dependent equations, which run one launch per stage.
int launch_rk4_phase(pdeopt_ctx* ctx, ExplicitKernel k, int ph, const Window& w, const HaloIo& io, void* Y, void* TA, double t, double dt) {
  void *const TB = ctx->TB.get(), *const ACC = ctx->ACC.get();
  if (k == EK_AC_SINGLE) return launch_ac_quad(ctx, w, Y, TA, dt);
  if (k == EK_CH_SINGLE) return launch_ch_quad(ctx, w, io, Y, TA, dt);
  if (k == EK_RK4_PAIRS) {
    if (ph == 0) return launch_pair_dt(ctx, w, io, PAIR_12, Y, nullptr, nullptr, TB, ACC, dt / 2, dt / 6, dt / 2, dt / 3);
    return launch_pair_dt(ctx, w, io, PAIR_34, TB, Y, ACC, TA, nullptr, dt, dt / 3, 0.0, dt / 6);
  }
  switch (ph) {
    case 0: return launch_stage(ctx, w, t, Y, Y, TA, ACC, dt / 2, dt / 6, OUT_Y_PLUS_AK, ACC_INIT);   // k1 = f(y);   TA = y + dt/2 k1;  ACC = y + dt/6 k1
    case 1: return launch_stage(ctx, w, t, TA, Y, TB, ACC, dt / 2, dt / 3, OUT_Y_PLUS_AK, ACC_ADD);   // k2 = f(TA);  TB = y + dt/2 k2;  ACC += dt/3 k2
    case 2: return launch_stage(ctx, w, t, TB, Y, TA, ACC, dt, dt / 3, OUT_Y_PLUS_AK, ACC_ADD);       // k3 = f(TB);  TA = y + dt k3;    ACC += dt/3 k3
    default: return launch_stage(ctx, w, t, TA, Y, Y, ACC, 0.0, dt / 6, OUT_ACC_PLUS_BK, ACC_NONE);  // k4 = f(TA);  y = ACC + dt/6 k4
  }
}

// Capture kGraphUnit substeps of the whole batch once into a hipGraph and replay it while n has that many left;
// *done = the substeps replayed.  Kernel arguments baked into the graph are the field pointers, dt and the problem
// structure; per-environment parameter VALUES live in device memory and may change between replays.
template <typename Step>
int replay_graph(pdeopt_ctx* ctx, const ExplicitPlan& plan, double dt, int64_t n, Step&& step, int64_t* done) {
  GraphKey key;
  memset(&key, 0, sizeof(key));  // padding bytes take part in the memcmp below
  key.kernel = plan.kernel; key.fuse_stages = plan.fuse_stages; key.dt = dt;
  key.Y = ctx->Y.get(); key.TA = ctx->TA.get(); key.TB = ctx->TB.get(); key.ACC = ctx->ACC.get(); key.KS = ctx->KS.get();
  key.ep = ctx->env_params_dev.get();
  key.vx = ctx->aux[PDEOPT_AUX_VX_FACE].dev.get(); key.vy = ctx->aux[PDEOPT_AUX_VY_FACE].dev.get();
  key.kernel_path = ctx->opt_kernel_path; key.tile_rows = ctx->opt_tile_rows; key.ablate = ctx->opt_debug_ablate;
  // the part of a problem that is baked into kernel arguments (not the per-env parameter values)
  const pdeopt_problem& p = ctx->prob;
  GraphStructure& g = key.structure;
  g.equation = p.equation; g.dtype = p.dtype; g.nx = p.nx; g.ny = p.ny; g.batch = p.batch; g.derivs = p.derivs;
  g.nz = p.nz; g.hx = p.hx; g.hy = p.hy; g.hz = p.hz;
  g.mu_kind = p.mu.kind; g.mu_flags = p.mu.flags; g.mu_n = p.mu.n;
  g.mob_kind = p.mob.kind; g.mob_flags = p.mob.flags; g.mob_n = p.mob.n;
  if (!ctx->graph_exec || memcmp(&key, &ctx->graph_key, sizeof(key)) != 0) {
    graph_destroy(ctx);
    const int64_t launches_before = ctx->n_stage_launches;
    hipGraph_t graph = nullptr;
    int rc = PDEOPT_OK;
    PDEOPT_HIP_CHECK(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
    for (int u = 0; u < kGraphUnit && !rc;) {
      int took = 1;
      rc = step(whole_batch(ctx), u, 0, took);
      u += took;
    }
    const hipError_t e_end = hipStreamEndCapture(ctx->stream, &graph);
    ctx->graph_launches_per_replay = ctx->n_stage_launches - launches_before;
    ctx->n_stage_launches = launches_before;
    if (rc) {
      if (graph) (void)hipGraphDestroy(graph);
      return rc;
    }
    PDEOPT_HIP_CHECK(ctx, e_end);
    const hipError_t e_inst = hipGraphInstantiate(&ctx->graph_exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    PDEOPT_HIP_CHECK(ctx, e_inst);
    ctx->graph_key = key;
    ctx->graph_name = ctx->last_kernel + "+hipGraph";
    // kGraphUnit is even: the ping-pong buffers are back in place after one replay
  }
  for (; *done + kGraphUnit <= n; *done += kGraphUnit) {
    PDEOPT_HIP_CHECK(ctx, hipGraphLaunch(ctx->graph_exec, ctx->stream));
    ctx->n_stage_launches += ctx->graph_launches_per_replay;
  }
  ctx->last_kernel = ctx->graph_name;
  return PDEOPT_OK;
}

}  // namespace

int advance_explicit(pdeopt_ctx* ctx, int integrator, double t0, double dt, int64_t n) {
  if (integrator != PDEOPT_INT_EULER && integrator != PDEOPT_INT_RK4)
    return fail(ctx, PDEOPT_EINVAL, "integrator %d is not an explicit fixed-step integrator", integrator);
  const ExplicitPlan plan = plan_explicit(ctx, integrator, n);
  const ExplicitKernel kernel = plan.kernel;
  ctx->last_groups = 1;  // (run_groups sets it for the families that come to it)
  if (kernel == EK_COOP_FIXED) return with_dtype(ctx, [&](auto t) { return coop_fixed_advance<decltype(t)>(ctx, integrator, t0, dt, n); });
  if (kernel == EK_SMALL_STEP) return with_dtype(ctx, [&](auto t) { return launch_small<decltype(t)>(ctx, whole_batch(ctx), integrator, dt, n); });
  int rc;
  if ((rc = ensure_work_fields(ctx, kernel))) return rc;

  // The state ping-pongs between Y and TA: every launch that advances it (an Euler step or pair, a fused RK4 substep)
  // writes the other buffer; the per-stage RK4 updates y in place.  Every group performs the same launches, so which
  // buffer holds the state before substep s depends on s alone: `base` is where the buffers were as the ctx has them.
  void *const Y0 = ctx->Y.get(), *const TA0 = ctx->TA.get();
  auto rotations = [&](int64_t s, int64_t base) -> int64_t { return kernel == EK_RK4_STAGE ? 0 : kernel == EK_EULER_PAIR ? (s - base + 1) / 2 : s - base; };
  const HaloIo none{};

  // substep s (and s + 1, where two Euler substeps go into one launch: took = 2) of the window
  auto step = [&](const Window& w, int64_t s, int64_t base, int& took) -> int {
    const bool odd = rotations(s, base) & 1;
    void* const Y = odd ? TA0 : Y0;
    void* const TA = odd ? Y0 : TA0;
    const double ts = t0 + (double)s * dt;  // stage times only matter to time-dependent equations
    if (kernel == EK_EULER_PAIR && s + 1 < n) {
      // result into TA, TB takes the kernel's unused y + dt k2 output
      took = 2;
      return launch_pair_dt(ctx, w, none, PAIR_12, Y, nullptr, nullptr, ctx->TB.get(), TA, dt, dt, dt, dt);
    }
    if (!is_rk4(kernel)) return launch_stage(ctx, w, ts, Y, Y, TA, nullptr, dt, 0.0, OUT_Y_PLUS_AK, ACC_NONE);
    int r = PDEOPT_OK;
    for (int ph = 0; ph < rk4_phases(kernel) && !r; ++ph)  // stage times: ts, ts + dt/2 twice, ts + dt
      r = launch_rk4_phase(ctx, kernel, ph, w, none, Y, TA, ph == 0 ? ts : ph == 3 ? ts + dt : ts + dt / 2, dt);
    return r;
  };

  int64_t done = 0;
  if (plan.graph && (rc = replay_graph(ctx, plan, dt, n, step, &done))) return rc;
  // the substeps the graph did not take, group by group
  rc = run_groups(ctx, plan.group, plan.side_by_side, done, n, [](const Window&) { return PDEOPT_OK; },
                  [&](const Window& w, int64_t s, int& took) { return step(w, s, done, took); });
  if (!rc && (rotations(n, done) & 1)) std::swap(ctx->Y, ctx->TA);
  return rc;
}

void graph_destroy(pdeopt_ctx* ctx) {
  if (ctx->graph_exec) (void)hipGraphExecDestroy(ctx->graph_exec);
  ctx->graph_exec = nullptr;
}

// One phase of an RK4 substep for callers that interleave their own work between phases (the
// domain-decomposed driver exchanges halos of `fields[phase]` before `rk4_phase(phase)`).
int rk4_phase_plan(pdeopt_ctx* ctx, int* fields, int* nphases) {
  const ExplicitKernel k = rk4_family(ctx, /*phased=*/true);
  *nphases = rk4_phases(k);
  // one launch per stage: Y, TA, TB, TA.  The single-pass kernel (halo-8 layout: its tile + 8 input is the halo): Y
  fields[0] = 0; fields[1] = 1; fields[2] = 2; fields[3] = 1;
  // Stage pairs: Y (pair 1+2 differentiates y), then TB (pair 3+4 differentiates y + dt/2 k2) -- but the halo-8 layout
  // has ONE exchange per substep: pair 1+2 runs on the tile + 4 ring (it reads y on tile + 8), so pair 3+4 finds TB on
  // its tile + 4 input region without an exchange of TB (-1: no exchange before phase 1)
  if (k == EK_RK4_PAIRS) fields[1] = ctx->halo == 8 ? -1 : 2;
  return PDEOPT_OK;
}

// part: 0 = the whole tile; 1 = interior tiles only, 2 = edge tiles only (fused stage pairs; the caller runs
// part 1 while the halo exchange of this phase is in flight and part 2 after pdeopt_halo_unpack).  The
// substep's buffer rotation happens with the LAST launch of the last phase (part 0 or 2).
// io: where the halo-8 launches find the state's halo and put the new state's strip (rk4_substep_h8)
static int rk4_phase_io(pdeopt_ctx* ctx, int phase, double dt, int part, HaloIo io) {
  if (ctx->prob.equation == PDEOPT_EQ_GPE) return fail(ctx, PDEOPT_EINVAL, "no explicit RHS for the GPE");
  if (part < 0 || part > 2) return fail(ctx, PDEOPT_EINVAL, "part %d outside 0..2", part);
  const ExplicitKernel k = rk4_family(ctx, /*phased=*/true);
  const int n = rk4_phases(k);
  if (const int rc = ensure_work_fields(ctx, k)) return rc;
  if (phase < 0 || phase >= n) return fail(ctx, PDEOPT_EINVAL, "phase %d outside 0..%d", phase, n - 1);
  if (ctx->halo == 8 && k == EK_RK4_STAGE)
    return fail(ctx, PDEOPT_EINVAL, "the halo-8 layout needs the fused Cahn-Hilliard kernels (closure class / tile shape / "
                                    "PDEOPT_OPT_FUSE_STAGES rule them out here): use halo layout 4");
  if (ctx->halo == 8 && part != 0)
    return fail(ctx, PDEOPT_EINVAL, "interior / edge launches belong to the halo-4 layout (two exchanges per substep)");
  if (k == EK_RK4_STAGE && part != 0)
    return fail(ctx, PDEOPT_EINVAL, "interior / edge launches exist for the fused stage pairs only (this problem runs one kernel per stage)");
  if (k == EK_RK4_PAIRS) {
    io.part = part;
    if (phase == 0) io.ext = ctx->halo == 8 ? 4 : 0;
  }
  // a phase call carries no time: the decomposed driver runs autonomous equations, t = 0 for any time-dependent term
  const int rc = launch_rk4_phase(ctx, k, phase, whole_batch(ctx), io, ctx->Y.get(), ctx->TA.get(), 0.0, dt);
  if (k != EK_RK4_STAGE && phase == n - 1 && part != 1) std::swap(ctx->Y, ctx->TA);
  return rc;
}

int rk4_phase(pdeopt_ctx* ctx, int phase, double dt, int part) { return rk4_phase_io(ctx, phase, dt, part, HaloIo{}); }

// n RK4 substeps of a single-rank padded tile with the loop-back halo exchange, entirely in the library: the
// per-substep pack -> unpack -> phase sequence of the decomposed driver without a host round trip per call
// (what one rank of pde_opt_amd/decomp.py executes, minus the collective).
int rk4_loopback_advance(pdeopt_ctx* ctx, double dt, int64_t n) {
  int fields[4], np_ = 0;
  rk4_phase_plan(ctx, fields, &np_);
  const int nbr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int rc = PDEOPT_OK;
  if (ctx->halo == 8) {
    // one exchange per substep; after the first one the strip comes out of PAIR_34's epilogue (fused pack) and the
    // loop-back "collective" is the strip buffer itself
    if (n <= 0) return PDEOPT_OK;
    if ((rc = halo_pack(ctx, 0, nullptr))) return rc;
    // the strip written by substep s (fused pack) is read by substep s + 1 (fused unpack): two buffers
    const size_t bytes = halo_strip_elems(ctx) * ctx->esize;
    if ((rc = grow_device_buffer(ctx, ctx->halo_scratch2, bytes, /*sync_first=*/true))) return rc;
    void* cur = ctx->halo_scratch.get();
    void* nxt = ctx->halo_scratch2.get();
    for (int64_t s = 0; s < n && !rc; ++s) {
      rc = rk4_substep_h8(ctx, dt, s + 1 < n ? nxt : nullptr, cur, nbr);
      std::swap(cur, nxt);
    }
    return rc;
  }
  for (int64_t s = 0; s < n && !rc; ++s)
    for (int ph = 0; ph < np_ && !rc; ++ph) {
      if ((rc = halo_pack(ctx, fields[ph], nullptr))) break;
      if ((rc = halo_unpack(ctx, fields[ph], nullptr, nbr))) break;
      rc = rk4_phase(ctx, ph, dt, 0);
    }
  return rc;
}

// halo-8 layout: both stage pairs of one substep (or the single-pass kernel).  The first launch reads the state's
// halo as io says (in the field already, from gathered strips, from the neighbours' own buffers); the last writes the
// NEW state's halo strip into io.strip (nullptr: not wanted)
static int rk4_substep_h8_io(pdeopt_ctx* ctx, double dt, const HaloIo& io) {
  if (rk4_family(ctx, /*phased=*/true) == EK_CH_SINGLE) return rk4_phase_io(ctx, 0, dt, 0, io);  // one kernel: halo in, the new strip out
  HaloIo in = io, out{};
  in.strip = nullptr;
  out.strip = io.strip;
  const int rc = rk4_phase_io(ctx, 0, dt, 0, in);
  return rc ? rc : rk4_phase_io(ctx, 1, dt, 0, out);
}

int rk4_substep_h8(pdeopt_ctx* ctx, double dt, void* strip, const void* recv, const int* nbr) {
  HaloIo io{};
  io.strip = strip;
  io.recv = recv;
  if (recv) std::copy(nbr, nbr + 8, io.nbr);
  return rk4_substep_h8_io(ctx, dt, io);
}

int rk4_substep_h8_peer(pdeopt_ctx* ctx, double dt, void* strip, const void* const* peer) {
  HaloIo io{};
  io.strip = strip;
  std::copy(peer, peer + 8, io.peer);
  return rk4_substep_h8_io(ctx, dt, io);
}

// ------------------------------------------------------------------------------------------
// Tsit5 (diffrax.Tsit5; call sites tests/test_solvers.py:81,263 and most notebooks).  Tableau:
// Ch. Tsitouras, Comput. Math. Appl. 62 (2011) 770-775 -- the published coefficients diffrax
// ships.  Row f1 of SURVEY section 8: one trial step + scaled error norm per environment; the
// PID step-size logic stays on the host (pde_opt_amd/pde_model.py).
// ------------------------------------------------------------------------------------------
namespace {

template <typename T>
struct LinComb {
  const T* y;
  const T* k[7];
  T c[7];
  int n;
  T* out;
};

template <typename T>
__global__ void lincomb_kernel(const LinComb<T> a, int64_t total) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t st = (int64_t)gridDim.x * blockDim.x;
  for (; i < total; i += st) {
    T r = a.y[i];
    for (int j = 0; j < a.n; ++j) r += a.c[j] * a.k[j][i];
    a.out[i] = r;
  }
}

constexpr int kErrBlocks = 64;

// partial[b][blk] = sum ((dt sum_j e_j k_j) / (atol + rtol max(|y0|,|y1|)))^2
template <typename T>
__global__ __launch_bounds__(256) void tsit5_err_kernel(const LinComb<T> a, const T* __restrict__ y1,
                                                        T rtol, T atol, int64_t env_elems,
                                                        double* __restrict__ partial) {
  const int b = blockIdx.y;
  const int64_t o = (int64_t)b * env_elems;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < env_elems; i += (int64_t)gridDim.x * 256) {
    T e = T(0);
    for (int j = 0; j < 7; ++j) e += a.c[j] * a.k[j][o + i];
    const T sc = atol + rtol * fmax(fabs(a.y[o + i]), fabs(y1[o + i]));
    const double q = (double)(e / sc);
    acc += q * q;
  }
  __shared__ double sh[4];
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) acc += __shfl_down(acc, s, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[(int64_t)b * gridDim.x + blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

template <typename T>
int tsit5_trial_t(pdeopt_ctx* ctx, double t, double dt, double rtol, double atol, double* err) {
  int rc;
  for (DeviceBuffer& k : ctx->K)
    if ((rc = ensure_buffer(ctx, k, ctx->total_bytes))) return rc;
  if ((rc = ensure_buffer(ctx, ctx->TA, ctx->total_bytes))) return rc;
  if ((rc = ensure_buffer(ctx, ctx->TB, ctx->total_bytes))) return rc;
  const int64_t total = (int64_t)(ctx->env_elems * ctx->prob.batch);
  const int blocks = (int)std::min<int64_t>((total + 255) / 256, 4096);
  const Window w = whole_batch(ctx);
  if (!ctx->tsit5_fsal_valid && (rc = launch_stage(ctx, w, t, ctx->Y.get(), ctx->Y.get(), ctx->K[0].get(), nullptr, 0, 0, OUT_K, ACC_NONE))) return rc;
  // stage 2 input from k1 alone (k1 is the previous step's k7 under FSAL, so nothing could form it earlier)
  {
    LinComb<T> lc{};
    lc.y = ctx->Y.as<const T>();
    lc.n = 1;
    lc.k[0] = ctx->K[0].as<const T>();
    lc.c[0] = T(dt * kTsA[0][0]);
    lc.out = ctx->TA.as<T>();
    hipLaunchKernelGGL(lincomb_kernel<T>, dim3(blocks), dim3(256), 0, ctx->stream, lc, total);
  }
  // stages 2..6: k_s = f(in_s) and, in the same pass, in_{s+1} = y + dt sum_j a_{s+1,j} k_j  (ping-pong
  // TA / TB; in_7 -- the 5th-order solution -- lands in TB).  Stage 7 evaluates k7 = f(in_7) for the
  // error estimate and the next step's FSAL.  8 launches per step instead of 13.
  for (int s = 1; s <= 5; ++s) {
    void* in_s = (s & 1) ? ctx->TA.get() : ctx->TB.get();
    void* in_next = (s & 1) ? ctx->TB.get() : ctx->TA.get();
    double c[kMaxLc + 1];
    for (int j = 0; j <= s; ++j) c[j] = dt * kTsA[s][j];
    if ((rc = launch_stage_lc<T>(ctx, w, t + kTsC[s - 1] * dt, in_s, ctx->Y.get(), ctx->K[s].get(), ctx->K, c, s, in_next))) return rc;
  }
  if ((rc = launch_stage(ctx, w, t + kTsC[5] * dt, ctx->TB.get(), ctx->TB.get(), ctx->K[6].get(), nullptr, 0, 0, OUT_K, ACC_NONE))) return rc;
  ctx->tsit5_pending = true;
  if (err) {
    double* part = nullptr;
    const size_t need = sizeof(double) * kErrBlocks * ctx->prob.batch;
    if ((rc = grow_device_buffer(ctx, ctx->red_dev, need, /*sync_first=*/false))) return rc;
    part = ctx->red_dev.as<double>();
    LinComb<T> lc{};
    lc.y = ctx->Y.as<const T>();
    lc.n = 7;
    for (int j = 0; j < 7; ++j) {
      lc.k[j] = ctx->K[j].as<const T>();
      lc.c[j] = T(dt * kTsE[j]);
    }
    hipLaunchKernelGGL(tsit5_err_kernel<T>, dim3(kErrBlocks, ctx->prob.batch), dim3(256), 0,
                       ctx->stream, lc, ctx->TB.as<const T>(), (T)rtol, (T)atol,
                       (int64_t)ctx->env_elems, part);
    PDEOPT_HIP_CHECK(ctx, hipGetLastError());
    std::vector<double> h((size_t)kErrBlocks * ctx->prob.batch);
    PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(h.data(), part, need, hipMemcpyDeviceToHost, ctx->stream));
    PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    for (int b = 0; b < ctx->prob.batch; ++b) {
      double s = 0;
      for (int c = 0; c < kErrBlocks; ++c) s += h[(size_t)b * kErrBlocks + c];
      err[b] = std::sqrt(s / (double)ctx->env_elems);  // diffrax rms_norm
    }
  }
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  return PDEOPT_OK;
}

}  // namespace

int tsit5_trial(pdeopt_ctx* ctx, double t, double dt, double rtol, double atol, double* err) {
  return with_dtype(ctx, [&](auto tag) { return tsit5_trial_t<decltype(tag)>(ctx, t, dt, rtol, atol, err); });
}

template <typename T>
static int tsit5_dense_t(pdeopt_ctx* ctx, double theta, double dt, int env_first, int env_count, void* dev_out) {
  double b[7];
  tsit5_dense_weights(theta, b);
  const int64_t o = (int64_t)env_first * (int64_t)ctx->env_elems;
  LinComb<T> lc{};
  lc.y = ctx->Y.as<const T>() + o;
  lc.n = 7;
  for (int j = 0; j < 7; ++j) {
    lc.k[j] = ctx->K[j].as<const T>() + o;
    lc.c[j] = T(dt * b[j]);
  }
  lc.out = (T*)dev_out + o;
  const int64_t total = (int64_t)ctx->env_elems * env_count;
  const int blocks = (int)std::min<int64_t>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(lincomb_kernel<T>, dim3(blocks), dim3(256), 0, ctx->stream, lc, total);
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  return PDEOPT_OK;
}

int tsit5_dense(pdeopt_ctx* ctx, double theta, double dt, int env_first, int env_count, void* dev_out) {
  if (!ctx->tsit5_pending) return fail(ctx, PDEOPT_ESTATE, "dense output needs a pending Tsit5 trial step");
  return with_dtype(ctx, [&](auto t) { return tsit5_dense_t<decltype(t)>(ctx, theta, dt, env_first, env_count, dev_out); });
}

// FSAL slope of environment b *= ratio[b] (its step size changed between two per-environment trials)
int tsit5_rescale_fsal(pdeopt_ctx* ctx, const double* ratio) {
  const size_t need = sizeof(double) * (size_t)ctx->prob.batch;
  if (const int rc = grow_device_buffer(ctx, ctx->red_dev, need, /*sync_first=*/false)) return rc;
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(ctx->red_dev.as<double>(), ratio, need, hipMemcpyHostToDevice, ctx->stream));
  const int64_t ee = (int64_t)ctx->env_elems;
  const dim3 grid((unsigned)std::min<int64_t>((ee + 255) / 256, 1024), ctx->prob.batch);
  with_dtype(ctx, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(env_scale_kernel<T>, grid, dim3(256), 0, ctx->stream, ctx->K[0].as<T>(), ctx->red_dev.as<const double>(), ee);
  });
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // `ratio` is the caller's again
  return PDEOPT_OK;
}

// per-environment commit: accepted environments take the candidate and its FSAL slope, the others keep theirs
int tsit5_commit_env(pdeopt_ctx* ctx, const uint8_t* accept) {
  if (!ctx->tsit5_pending) return fail(ctx, PDEOPT_ESTATE, "no Tsit5 trial step is pending");
  ctx->tsit5_pending = false;
  const int batch = ctx->prob.batch;
  std::swap(ctx->Y, ctx->TB);
  std::swap(ctx->K[0], ctx->K[6]);
  const size_t eb = ctx->env_elems * ctx->esize;
  for (int b = 0; b < batch; ++b) {
    if (accept[b]) continue;
    // rejected: the old state / slope (now in TB / K[6]) go back
    PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(ctx->Y.as<char>() + eb * b, ctx->TB.as<const char>() + eb * b, eb, hipMemcpyDeviceToDevice, ctx->stream));
    PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(ctx->K[0].as<char>() + eb * b, ctx->K[6].as<const char>() + eb * b, eb, hipMemcpyDeviceToDevice, ctx->stream));
  }
  ctx->tsit5_fsal_valid = true;
  return PDEOPT_OK;
}

int tsit5_commit(pdeopt_ctx* ctx, int accept) {
  if (!ctx->tsit5_pending) return fail(ctx, PDEOPT_ESTATE, "no Tsit5 trial step is pending");
  ctx->tsit5_pending = false;
  if (accept) {
    std::swap(ctx->Y, ctx->TB);         // y <- 5th-order candidate
    std::swap(ctx->K[0], ctx->K[6]);    // FSAL: k7 = f(t+dt, y1) is the next k1
  }
  ctx->tsit5_fsal_valid = true;         // on rejection K[0] = f(t, y) is still valid
  return PDEOPT_OK;
}

// the in-kernel adaptive solve: one workgroup per environment (LDS-resident periodic Cahn-Hilliard / Allen-Cahn grids,
// stencil_small_adaptive.hpp) or several cooperating workgroups per environment (larger grids, the smoothed-boundary
// forms, advection-diffusion: stencil_coop_adaptive.hpp)
static bool tsit5_single_wg(const pdeopt_ctx* ctx) {
  return with_dtype(ctx, [&](auto t) { return small_tsit5_supported<decltype(t)>(ctx); });
}
static bool tsit5_coop(const pdeopt_ctx* ctx) {
  return with_dtype(ctx, [&](auto t) { return coop_tsit5_supported<decltype(t)>(ctx); });
}
bool tsit5_solve_small_supported(const pdeopt_ctx* ctx) { return tsit5_single_wg(ctx) || tsit5_coop(ctx); }

int tsit5_solve_small(pdeopt_ctx* ctx, double t0, double t1, double dt0, const pdeopt_pid* pid, int64_t max_steps, int n_save,
                      const double* save_ts, void* save_host, pdeopt_tsit5_stats* stats) {
  const bool single = tsit5_single_wg(ctx), coop = tsit5_coop(ctx);
  if (!single && !coop)
    return fail(ctx, PDEOPT_EINVAL, "the in-kernel adaptive solve takes periodic / smoothed-boundary Cahn-Hilliard and Allen-Cahn FD problems and "
                                    "advection-diffusion with a steady velocity, on grids its tiles cover (pdeopt_tsit5_solve_small_supported)");
  // both apply: one workgroup up to two vectors per thread (64^2 fp32: 18 us per trial step against 21 on 32 workgroups);
  // from three vectors per thread on (its state then lives in LDS: 64^2 fp64 33 us) the multi-workgroup kernel (25 us)
  constexpr int kV32 = 4, kV64 = 2;
  const int64_t nvec = (int64_t)ctx->prob.nx * ctx->prob.ny / (ctx->prob.dtype == PDEOPT_F32 ? kV32 : kV64);
  const bool prefer_coop = ctx->opt_small_persist == 2 || (ctx->opt_small_persist == 0 && nvec > 1024);
  return with_dtype(ctx, [&](auto t) {
    using T = decltype(t);
    if (coop && (!single || prefer_coop)) return coop_tsit5_solve<T>(ctx, t0, t1, dt0, pid, max_steps, n_save, save_ts, save_host, stats);
    return small_tsit5_solve<T>(ctx, t0, t1, dt0, pid, max_steps, n_save, save_ts, save_host, stats);
  });
}

int launch_lerp(pdeopt_ctx* ctx, const void* a, const void* b, void* out, double theta,
                size_t env_first, size_t env_count) {
  const size_t off = env_first * ctx->env_elems;
  const int64_t n = (int64_t)(env_count * ctx->env_elems);
  const int threads = 256;
  const int blocks = (int)std::min<int64_t>((n + threads - 1) / threads, 2048);
  with_dtype(ctx, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(lerp_kernel<T>, dim3(blocks), dim3(threads), 0, ctx->stream, (const T*)a + off, (const T*)b + off, (T*)out, (T)theta, n);
  });
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  return PDEOPT_OK;
}

}  // namespace pdeopt
