// extern "C" entry points of libpdeopt_hip.so (declared in include/pdeopt_hip.h).
#include <cstdarg>
#include <cstring>
#include <mutex>

#include "closures.hpp"
#include "common.hpp"

namespace pdeopt {

static std::string g_create_error;

int fail(pdeopt_ctx* ctx, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (ctx)
    ctx->err = buf;
  else
    g_create_error = buf;
  return code;
}

namespace {
template <typename Buffer>
int ensure_any(pdeopt_ctx* ctx, Buffer& b, size_t bytes, const char* what) {
  if (b && b.bytes() < bytes)
    return fail(ctx, PDEOPT_ESTATE, "a buffer of %zu bytes was asked to hold %zu: its owner did not release or grow it", b.bytes(), bytes);
  const hipError_t e = b.ensure(bytes);
  if (e != hipSuccess) return fail(ctx, PDEOPT_ENOMEM, "%s(%zu bytes) failed: %s", what, bytes, hipGetErrorString(e));
  return PDEOPT_OK;
}
}  // namespace

int ensure_buffer(pdeopt_ctx* ctx, DeviceBuffer& b, size_t bytes) { return ensure_any(ctx, b, bytes, "hipMalloc"); }
int ensure_buffer(pdeopt_ctx* ctx, PinnedBuffer& b, size_t bytes) { return ensure_any(ctx, b, bytes, "hipHostMalloc"); }

int grow_device_buffer(pdeopt_ctx* ctx, DeviceBuffer& b, size_t need_bytes, bool sync_first) {
  if (sync_first && b && b.bytes() < need_bytes) PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  const hipError_t e = b.reserve(need_bytes);
  if (e != hipSuccess) return fail(ctx, PDEOPT_ENOMEM, "hipMalloc(%zu bytes) failed: %s", need_bytes, hipGetErrorString(e));
  return PDEOPT_OK;
}

int ensure_stream2(pdeopt_ctx* ctx) {
  if (ctx->stream2) return PDEOPT_OK;
  PDEOPT_HIP_CHECK(ctx, hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking));
  PDEOPT_HIP_CHECK(ctx, hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
  PDEOPT_HIP_CHECK(ctx, hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
  return PDEOPT_OK;
}

namespace {

void free_fields(pdeopt_ctx* ctx) {
  // the members that die with a configuration
  ctx->n_spots = 0;
  ctx->spots_host.clear();
  for (DeviceBuffer* b : {&ctx->Y, &ctx->TA, &ctx->TB, &ctx->ACC, &ctx->SNAP, &ctx->KS, &ctx->obs_dev, &ctx->vort_dev,
                          &ctx->env_params_dev, &ctx->spots_dev})
    b->reset();
  for (DeviceBuffer& k : ctx->K) k.reset();
  ctx->fieldmu_coef.reset();
  ctx->fieldmu_coef_slots = 0;
  for (auto& a : ctx->aux) a = AuxField{};
  ctx->features.clear();
  sk_drop(ctx);  // the shell tables belong to one grid
  graph_destroy(ctx);
  ctx->tsit5_pending = false;
  ctx->tsit5_fsal_valid = false;
  ctx->configured = false;
}

int check_closure(pdeopt_ctx* ctx, const pdeopt_closure& c, const char* name, const std::string* jit_body = nullptr, int more_flags = 0) {
  if (c.kind == PDEOPT_CL_JIT) {  // compiled at run time from the body handed over by pdeopt_set_jit_closures
    if (!jit_body || jit_body->empty())
      return fail(ctx, PDEOPT_EINVAL, "closure %s has kind PDEOPT_CL_JIT but pdeopt_set_jit_closures gave no body for it", name);
    return PDEOPT_OK;
  }
  if (c.kind != PDEOPT_CL_POLY && c.kind != PDEOPT_CL_LEGENDRE)
    return fail(ctx, PDEOPT_EINVAL, "closure %s: unknown kind %d", name, c.kind);
  if (c.n < 1 || c.n > kMaxCoef)
    return fail(ctx, PDEOPT_EINVAL, "closure %s: n=%d outside 1..%d", name, c.n, kMaxCoef);
  if ((c.flags & PDEOPT_CL_SQRT_WRAP) && !(more_flags & PDEOPT_CL_SQRT_WRAP))
    return fail(ctx, PDEOPT_EINVAL, "closure %s: PDEOPT_CL_SQRT_WRAP is evaluated by the Butler-Volmer kernels only", name);
  if (c.flags & ~(PDEOPT_CL_LOGIT_PRIOR | PDEOPT_CL_EXP_WRAP | PDEOPT_CL_MIX_ENTROPY | more_flags))
    return fail(ctx, PDEOPT_EINVAL, "closure %s: unknown flags 0x%x", name, c.flags);
  return PDEOPT_OK;
}

template <typename T>
void fill_env_params(pdeopt_ctx* ctx) {
  const pdeopt_problem& p = ctx->prob;
  ctx->env_params_host.assign(sizeof(EnvParams<T>) * (size_t)p.batch, 0);
  auto* e = reinterpret_cast<EnvParams<T>*>(ctx->env_params_host.data());
  for (int b = 0; b < p.batch; ++b) {
    e[b].kappa = T(p.kappa);
    e[b].gpe_k = T(p.gpe_k);
    e[b].kscale = T(1);
    e[b].imex_scale = T(1);
    e[b].gpe_omega = T(0);
    e[b].gpe_omega_rate = T(0);
    for (int k = 0; k < kMaxCoef; ++k) {
      e[b].mu[k] = k < p.mu.n ? T(p.mu.coef[k]) : T(0);
      e[b].mob[k] = k < p.mob.n ? T(p.mob.coef[k]) : T(0);
      e[b].fe[k] = k < p.fe.n ? T(p.fe.coef[k]) : T(0);
    }
  }
}

template <typename T>
void patch_env_params(pdeopt_ctx* ctx, int first, int count, const double* kappa, const double* mu,
                      const double* mob) {
  auto* e = reinterpret_cast<EnvParams<T>*>(ctx->env_params_host.data());
  for (int i = 0; i < count; ++i) {
    EnvParams<T>& d = e[first + i];
    if (kappa) d.kappa = T(kappa[i]);
    for (int k = 0; k < kMaxCoef; ++k) {
      if (mu) d.mu[k] = k < ctx->prob.mu.n ? T(mu[(size_t)i * kMaxCoef + k]) : T(0);
      if (mob) d.mob[k] = k < ctx->prob.mob.n ? T(mob[(size_t)i * kMaxCoef + k]) : T(0);
    }
  }
}

template <typename T>
void patch_env_gpe_k(pdeopt_ctx* ctx, int first, int count, const double* k) {
  auto* e = reinterpret_cast<EnvParams<T>*>(ctx->env_params_host.data());
  for (int i = 0; i < count; ++i) e[first + i].gpe_k = T(k[i]);
}

template <typename T>
void patch_env_gpe_omega(pdeopt_ctx* ctx, int first, int count, const double* omega, double all) {
  auto* e = reinterpret_cast<EnvParams<T>*>(ctx->env_params_host.data());
  for (int i = 0; i < count; ++i) e[first + i].gpe_omega = T(omega ? omega[i] : all);
}

// returns whether any environment of the batch has a nonzero rate afterwards
template <typename T>
bool patch_env_gpe_omega_rate(pdeopt_ctx* ctx, int first, int count, const double* rate) {
  auto* e = reinterpret_cast<EnvParams<T>*>(ctx->env_params_host.data());
  for (int i = 0; i < count; ++i) e[first + i].gpe_omega_rate = T(rate ? rate[i] : 0.0);
  bool any = false;
  for (int b = 0; b < ctx->prob.batch; ++b) any = any || e[b].gpe_omega_rate != T(0);
  return any;
}

template <typename T>
bool patch_imex_scale(pdeopt_ctx* ctx, int first, int count, const double* sigma) {
  auto* e = reinterpret_cast<EnvParams<T>*>(ctx->env_params_host.data());
  for (int i = 0; i < count; ++i) e[first + i].imex_scale = T(sigma[i]);
  bool any = false;
  for (int b = 0; b < ctx->prob.batch; ++b) any = any || e[b].imex_scale != T(1);
  return any;
}

template <typename T>
void patch_kscale(pdeopt_ctx* ctx, const std::vector<double>& sc) {
  auto* e = reinterpret_cast<EnvParams<T>*>(ctx->env_params_host.data());
  for (size_t b = 0; b < sc.size(); ++b) e[b].kscale = T(sc[b]);
}

int upload_env_params(pdeopt_ctx* ctx) {
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(ctx->env_params_dev.get(), ctx->env_params_host.data(),
                                       ctx->env_params_host.size(), hipMemcpyHostToDevice,
                                       ctx->stream));
  // the host vector may be edited right after this call returns
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PDEOPT_OK;
}

int check_envs(pdeopt_ctx* ctx, int first, int count) {
  if (!ctx->configured) return fail(ctx, PDEOPT_ESTATE, "pdeopt_configure has not been called");
  if (first < 0 || count < 0 || (int64_t)first + count > ctx->prob.batch)
    return fail(ctx, PDEOPT_EINVAL, "environment range [%d, %d) outside batch %d", first,
                first + count, ctx->prob.batch);
  return PDEOPT_OK;
}

size_t aux_bytes(const pdeopt_ctx* ctx, int which, int per_env) {
  const bool cplx = which == PDEOPT_AUX_IMEX_SYMBOL || which == PDEOPT_AUX_GPE_A_TERM;
  return (size_t)ctx->prob.nx * ctx->prob.ny * (ctx->prob.nz > 1 ? ctx->prob.nz : 1) * (cplx ? 2 : 1) * ctx->esize *
         (per_env ? (size_t)ctx->prob.batch : 1);
}

// (re)allocate the device buffer of an auxiliary field for the given sharing mode
int aux_alloc(pdeopt_ctx* ctx, int which, int per_env) {
  const size_t bytes = aux_bytes(ctx, which, per_env);
  AuxField& a = ctx->aux[which];
  if (a.dev && a.dev.bytes() != bytes) {
    PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    a.dev.reset();
    a.stage.reset();
  }
  int rc = ensure_buffer(ctx, a.dev, bytes);
  if (rc) return rc;
  a.per_env = per_env ? 1 : 0;
  return PDEOPT_OK;
}

}  // namespace

int refresh_time_aux(pdeopt_ctx* ctx, int which, double t) {
  AuxField& a = ctx->aux[which];
  if (!a.fn || (a.loaded && a.t_loaded == t)) return PDEOPT_OK;
  // the staging buffer is reused: the previous upload must have left it
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (a.fn(t, which, a.stage.get(), a.user) != 0)
    return fail(ctx, PDEOPT_EINVAL, "time-dependent source of aux field %d failed at t = %g", which, t);
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(a.dev.get(), a.stage.get(), a.dev.bytes(), hipMemcpyHostToDevice, ctx->stream));
  a.t_loaded = t;
  a.loaded = true;
  return PDEOPT_OK;
}

}  // namespace pdeopt

using namespace pdeopt;

extern "C" {

int pdeopt_abi_version(void) { return 1; }

int pdeopt_device_count(int* count) {
  if (!count) return PDEOPT_EINVAL;
  hipError_t e = hipGetDeviceCount(count);
  if (e != hipSuccess) {
    *count = 0;
    return fail(nullptr, PDEOPT_EHIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
  }
  return PDEOPT_OK;
}

int pdeopt_ctx_create(int device, pdeopt_ctx** out) {
  if (!out) return fail(nullptr, PDEOPT_EINVAL, "out is NULL");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return fail(nullptr, PDEOPT_EHIP, "no HIP device available (%s)", hipGetErrorString(e));
  if (device < 0 || device >= n)
    return fail(nullptr, PDEOPT_EINVAL, "device %d outside 0..%d", device, n - 1);
  e = hipSetDevice(device);
  if (e != hipSuccess) return fail(nullptr, PDEOPT_EHIP, "hipSetDevice: %s", hipGetErrorString(e));
  auto* ctx = new pdeopt_ctx();
  ctx->device = device;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
    ctx->num_cus = cus;
  if ((e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipEventCreate(&ctx->ev0)) != hipSuccess || (e = hipEventCreate(&ctx->ev1)) != hipSuccess) {
    fail(nullptr, PDEOPT_EHIP, "stream/event creation: %s", hipGetErrorString(e));
    delete ctx;
    return PDEOPT_EHIP;
  }
  *out = ctx;
  return PDEOPT_OK;
}

int pdeopt_ctx_destroy(pdeopt_ctx* ctx) {
  if (!ctx) return PDEOPT_OK;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  comm_destroy(ctx);
  free_fields(ctx);  // the feature states and their plans, graphs
  if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
  if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
  if (ctx->stream2) (void)hipStreamDestroy(ctx->stream2);
  if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
  if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
  if (ctx->stream && !ctx->stream_borrowed) (void)hipStreamDestroy(ctx->stream);
  delete ctx;  // the buffers that live with the ctx free themselves here, on ctx->device
  return PDEOPT_OK;
}

const char* pdeopt_last_error(const pdeopt_ctx* ctx) {
  return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

const char* pdeopt_last_kernel(const pdeopt_ctx* ctx) { return ctx ? ctx->last_kernel.c_str() : ""; }

int pdeopt_set_option(pdeopt_ctx* ctx, int option, int64_t value) {
  if (!ctx) return PDEOPT_EINVAL;
  switch (option) {
    case PDEOPT_OPT_KERNEL_PATH:
      if (value < 0 || value > 2) return fail(ctx, PDEOPT_EINVAL, "kernel path %lld", (long long)value);
      ctx->opt_kernel_path = value;
      return PDEOPT_OK;
    case PDEOPT_OPT_TILE_ROWS:
      if (value != 0 && value != 16 && value != 32 && value != 64)
        return fail(ctx, PDEOPT_EINVAL, "tile rows must be 0 (auto), 16, 32 or 64");
      ctx->opt_tile_rows = value;
      return PDEOPT_OK;
    case PDEOPT_OPT_IMEX_LDS_FFT:
      ctx->opt_imex_lds_fft = value;
      return PDEOPT_OK;
    case PDEOPT_OPT_GRAPH:
      if (value < -1 || value > 1) return fail(ctx, PDEOPT_EINVAL, "graph option must be -1, 0 or 1");
      ctx->opt_graph = value;
      return PDEOPT_OK;
    case PDEOPT_OPT_HALO_LAYOUT:
      if (value != 0 && value != 4 && value != 8)
        return fail(ctx, PDEOPT_EINVAL, "halo layout must be 0 (periodic), 4 or 8 (padded tiles)");
      ctx->opt_halo = value;
      return PDEOPT_OK;
    case PDEOPT_OPT_FUSE_STAGES:
      ctx->opt_fuse_stages = value;
      return PDEOPT_OK;
    case PDEOPT_OPT_DEBUG_ABLATE:
      ctx->opt_debug_ablate = value;
      return PDEOPT_OK;
    case PDEOPT_OPT_GROUP_ENVS:
      ctx->opt_group_envs = value;
      return PDEOPT_OK;
    case PDEOPT_OPT_GROUP_STREAMS:
      if (value < 0 || value > 2) return fail(ctx, PDEOPT_EINVAL, "group-streams option must be 0, 1 or 2");
      ctx->opt_group_streams = value;
      return PDEOPT_OK;
    case PDEOPT_OPT_SMALL_PERSIST:
      if (value < -1 || value > 2) return fail(ctx, PDEOPT_EINVAL, "small-persist option must be -1, 0, 1 or 2");
      ctx->opt_small_persist = value;
      return PDEOPT_OK;
    default:
      return fail(ctx, PDEOPT_EINVAL, "unknown option %d", option);
  }
}

int pdeopt_configure(pdeopt_ctx* ctx, const pdeopt_problem* pr) {
  if (!ctx || !pr) return PDEOPT_EINVAL;
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  // Re-configuring with the same shape (the per-step "rebuild the equation" of PDEEnv.step,
  // pde_env.py:286) keeps every device buffer, rocFFT plan and the resident state: only the
  // parameters change.
  const bool same_shape = ctx->configured && pr->equation == ctx->prob.equation &&
                          pr->dtype == ctx->prob.dtype && pr->nx == ctx->prob.nx &&
                          pr->ny == ctx->prob.ny && pr->nz == ctx->prob.nz && pr->batch == ctx->prob.batch &&
                          (int)ctx->opt_halo == ctx->halo;
  if (!same_shape) free_fields(ctx);
  ctx->configured = false;
  if (pr->dtype != PDEOPT_F32 && pr->dtype != PDEOPT_F64)
    return fail(ctx, PDEOPT_EINVAL, "unknown dtype %d", pr->dtype);
  if (pr->equation < PDEOPT_EQ_CAHN_HILLIARD || pr->equation > PDEOPT_EQ_ALLEN_CAHN_SBM_BV)
    return fail(ctx, PDEOPT_EINVAL, "unknown equation %d", pr->equation);
  if (pr->nx < 1 || pr->ny < 1 || pr->batch < 1)
    return fail(ctx, PDEOPT_EINVAL, "bad extents nx=%d ny=%d batch=%d", pr->nx, pr->ny, pr->batch);
  if (!(pr->hx > 0) || !(pr->hy > 0)) return fail(ctx, PDEOPT_EINVAL, "grid spacing must be > 0");
  const bool sbm = pr->equation == PDEOPT_EQ_ALLEN_CAHN_SBM || pr->equation == PDEOPT_EQ_CAHN_HILLIARD_SBM;
  const bool is3d = pr->equation == PDEOPT_EQ_CAHN_HILLIARD_3D;
  if (is3d) {
    if (pr->nz < 1 || !(pr->hz > 0)) return fail(ctx, PDEOPT_EINVAL, "3-D problem needs nz >= 1 and hz > 0");
    if (ctx->halo) return fail(ctx, PDEOPT_EINVAL, "the padded layout is 2-D only");
  } else if (pr->nz > 1) {
    return fail(ctx, PDEOPT_EINVAL, "nz=%d with a 2-D equation", pr->nz);
  }
  if (pr->equation == PDEOPT_EQ_CAHN_HILLIARD || pr->equation == PDEOPT_EQ_ALLEN_CAHN || sbm || is3d) {
    int rc;
    const bool plain2d = pr->equation == PDEOPT_EQ_CAHN_HILLIARD || pr->equation == PDEOPT_EQ_ALLEN_CAHN;
    if ((rc = check_closure(ctx, pr->mu, "mu", plain2d ? &ctx->jit_src[0] : nullptr))) return rc;
    if ((rc = check_closure(ctx, pr->mob, "mob", plain2d ? &ctx->jit_src[1] : nullptr))) return rc;
    if (sbm && (rc = check_closure(ctx, pr->fe, "f"))) return rc;
    if ((pr->mu.kind == PDEOPT_CL_JIT || pr->mob.kind == PDEOPT_CL_JIT) && pr->derivs != PDEOPT_DERIVS_FD)
      return fail(ctx, PDEOPT_EINVAL, "run-time-compiled closures run the finite-difference kernels only (derivs = \"fd\")");
    // a role that is NOT compiled at run time while the other is: its family member is evaluated by ... the same
    // compiled kernel, which has no closure_generic: the host emits a body for both roles whenever one needs it
    if ((pr->mu.kind == PDEOPT_CL_JIT) != (pr->mob.kind == PDEOPT_CL_JIT))
      return fail(ctx, PDEOPT_EINVAL, "run-time-compiled closures: hand over bodies for mu AND the mobility (kind PDEOPT_CL_JIT for both)");
  }
  if (bv_equation(pr->equation)) {
    int rc;
    if (pr->mu.kind == PDEOPT_CL_JIT || pr->mob.kind == PDEOPT_CL_JIT)
      return fail(ctx, PDEOPT_EINVAL, "the Butler-Volmer kernels evaluate closures of the in-kernel family only (no run-time-compiled closures)");
    if ((rc = check_closure(ctx, pr->mu, "mu"))) return rc;  // (SQRT_WRAP is the exchange current's: the kernels evaluate mu_h without it)
    if ((rc = check_closure(ctx, pr->mob, "j0", nullptr, PDEOPT_CL_SQRT_WRAP))) return rc;
    if (pr->derivs != PDEOPT_DERIVS_FD)
      return fail(ctx, PDEOPT_EINVAL, "the Butler-Volmer equations have a finite-difference right-hand side only (derivs = \"fd\")");
    if (ctx->opt_halo)
      return fail(ctx, PDEOPT_EINVAL, "the Butler-Volmer equations need the periodic layout (their sums run over the whole environment)");
  }
  if (pr->equation == PDEOPT_EQ_SHAPE_SMOOTH && !(pr->gpe_k > 0))
    return fail(ctx, PDEOPT_EINVAL, "shape smoothing needs smooth_epsilon (gpe_k) > 0");
  if (sbm && pr->derivs != PDEOPT_DERIVS_FD)
    return fail(ctx, PDEOPT_EINVAL, "Invalid derivative type: %d", pr->derivs);
  if (pr->derivs != PDEOPT_DERIVS_FD && pr->derivs != PDEOPT_DERIVS_FOURIER)
    return fail(ctx, PDEOPT_EINVAL, "Invalid derivative type: %d", pr->derivs);
  if (pr->derivs == PDEOPT_DERIVS_FOURIER && pr->equation != PDEOPT_EQ_CAHN_HILLIARD &&
      pr->equation != PDEOPT_EQ_ALLEN_CAHN && pr->equation != PDEOPT_EQ_CAHN_HILLIARD_3D)
    return fail(ctx, PDEOPT_EINVAL, "the pseudo-spectral RHS exists for Cahn-Hilliard / Allen-Cahn only");
  ctx->prob = *pr;
  if (ctx->prob.mu.n < 1) ctx->prob.mu.n = 1;
  if (ctx->prob.mob.n < 1) ctx->prob.mob.n = 1;
  if (ctx->prob.fe.n < 1) ctx->prob.fe.n = 1;
  ctx->esize = pr->dtype == PDEOPT_F32 ? 4 : 8;
  ctx->comps = pr->equation == PDEOPT_EQ_GPE ? 2 : 1;
  ctx->halo = (int)ctx->opt_halo;
  if (ctx->halo && pr->equation != PDEOPT_EQ_CAHN_HILLIARD && pr->equation != PDEOPT_EQ_ALLEN_CAHN)
    return fail(ctx, PDEOPT_EINVAL, "the padded (domain-decomposition) layout covers CH / AC only");
  ctx->env_elems = (size_t)pad_rows(pr->nx, ctx->halo) * pad_ld(pr->ny, ctx->halo) * ctx->comps;
  if (pr->equation == PDEOPT_EQ_CAHN_HILLIARD_3D) ctx->env_elems *= (size_t)pr->nz;
  ctx->total_bytes = ctx->env_elems * pr->batch * ctx->esize;
  int rc;
  if (!same_shape) {
    if ((rc = ensure_buffer(ctx, ctx->Y, ctx->total_bytes))) return rc;
    PDEOPT_HIP_CHECK(ctx, hipMemsetAsync(ctx->Y.get(), 0, ctx->total_bytes, ctx->stream));
  }
  ctx->tsit5_pending = false;
  ctx->tsit5_fsal_valid = false;
  if (ctx->fieldmu_coef)  // a coefficient gradient belongs to one problem: a new one starts from zero
    PDEOPT_HIP_CHECK(ctx, hipMemsetAsync(ctx->fieldmu_coef.as<double>(), 0, ctx->fieldmu_coef_slots * sizeof(double), ctx->stream));
  with_dtype(ctx, [&](auto t) { fill_env_params<decltype(t)>(ctx); });
  if ((rc = ensure_buffer(ctx, ctx->env_params_dev, ctx->env_params_host.size()))) return rc;
  ctx->imex_per_env = false;
  ctx->rot_set = false;
  ctx->rot_any_rate = false;
  ctx->configured = true;
  return upload_env_params(ctx);
}

int pdeopt_set_env_params(pdeopt_ctx* ctx, int env_first, int env_count, const double* kappa,
                          const double* mu_coef, const double* mob_coef) {
  if (!ctx) return PDEOPT_EINVAL;
  int rc = check_envs(ctx, env_first, env_count);
  if (rc) return rc;
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  with_dtype(ctx, [&](auto t) { patch_env_params<decltype(t)>(ctx, env_first, env_count, kappa, mu_coef, mob_coef); });
  return upload_env_params(ctx);
}

int pdeopt_set_bv_params(pdeopt_ctx* ctx, double alpha, int mode, const double* per_env) {
  if (!ctx || !per_env) return PDEOPT_EINVAL;
  if (!ctx->configured) return fail(ctx, PDEOPT_ESTATE, "pdeopt_configure has not been called");
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return bv_set_params(ctx, alpha, mode, per_env);
}

int pdeopt_bv_voltage(pdeopt_ctx* ctx, int env_first, int env_count, double* host_out) {
  if (!ctx || !host_out) return PDEOPT_EINVAL;
  int rc = check_envs(ctx, env_first, env_count);
  if (rc) return rc;
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return env_count ? bv_voltage(ctx, env_first, env_count, host_out, true) : PDEOPT_OK;
}

int pdeopt_bv_last_voltage(pdeopt_ctx* ctx, int env_first, int env_count, double* host_out) {
  if (!ctx || !host_out) return PDEOPT_EINVAL;
  int rc = check_envs(ctx, env_first, env_count);
  if (rc) return rc;
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return env_count ? bv_voltage(ctx, env_first, env_count, host_out, false) : PDEOPT_OK;
}

int pdeopt_set_aux(pdeopt_ctx* ctx, int which, const void* host, int per_env) {
  if (!ctx || !host) return PDEOPT_EINVAL;
  if (!ctx->configured) return fail(ctx, PDEOPT_ESTATE, "pdeopt_configure has not been called");
  if (which < 0 || which >= kNumAux) return fail(ctx, PDEOPT_EINVAL, "unknown aux field %d", which);
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int rc = aux_alloc(ctx, which, per_env);
  if (rc) return rc;
  AuxField& a = ctx->aux[which];
  const size_t bytes = a.dev.bytes();
  a.fn = nullptr;  // a static upload replaces a time-dependent source
  a.loaded = false;
  ctx->features.invalidate_all();  // multipliers derived from the old aux field are stale
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(a.dev.get(), host, bytes, hipMemcpyHostToDevice, ctx->stream));
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PDEOPT_OK;
}

int pdeopt_set_aux_time_fn(pdeopt_ctx* ctx, int which, pdeopt_aux_fn fn, void* user, int per_env) {
  if (!ctx) return PDEOPT_EINVAL;
  if (!ctx->configured) return fail(ctx, PDEOPT_ESTATE, "pdeopt_configure has not been called");
  if (which != PDEOPT_AUX_GPE_POTENTIAL && which != PDEOPT_AUX_VX_FACE && which != PDEOPT_AUX_VY_FACE)
    return fail(ctx, PDEOPT_EINVAL, "aux field %d cannot be time-dependent (GPE_POTENTIAL, VX_FACE, VY_FACE can)", which);
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  AuxField& a = ctx->aux[which];
  if (!fn) {
    a.fn = nullptr;
    a.user = nullptr;
    return PDEOPT_OK;
  }
  int rc = aux_alloc(ctx, which, per_env);
  if (rc) return rc;
  if ((rc = ensure_buffer(ctx, a.stage, a.dev.bytes()))) return rc;
  a.fn = fn;
  a.user = user;
  a.loaded = false;
  ctx->tsit5_fsal_valid = false;
  graph_destroy(ctx);
  return PDEOPT_OK;
}

int pdeopt_set_gpe_spots(pdeopt_ctx* ctx, int env_first, int env_count, int n_spots, const pdeopt_light_spot* spots,
                         double x_first, double y_first) {
  if (!ctx) return PDEOPT_EINVAL;
  int rc = check_envs(ctx, env_first, env_count);
  if (rc) return rc;
  if (ctx->prob.equation != PDEOPT_EQ_GPE) return fail(ctx, PDEOPT_EINVAL, "light spots belong to the GPE");
  if (n_spots < 0 || n_spots > PDEOPT_MAX_SPOTS)
    return fail(ctx, PDEOPT_EINVAL, "n_spots = %d outside 0..%d", n_spots, PDEOPT_MAX_SPOTS);
  if (n_spots > 0 && !spots) return PDEOPT_EINVAL;
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int batch = ctx->prob.batch;
  if (n_spots != ctx->n_spots && !(env_first == 0 && env_count == batch))
    return fail(ctx, PDEOPT_EINVAL, "changing the number of spots (%d -> %d) needs the whole batch in one call",
                ctx->n_spots, n_spots);
  ctx->n_spots = n_spots;
  ctx->spots_x_first = x_first;
  ctx->spots_y_first = y_first;
  if (n_spots == 0) return PDEOPT_OK;
  ctx->spots_host.resize((size_t)batch * PDEOPT_MAX_SPOTS, pdeopt_light_spot{});
  for (int e = 0; e < env_count; ++e)
    for (int s = 0; s < PDEOPT_MAX_SPOTS; ++s)
      ctx->spots_host[(size_t)(env_first + e) * PDEOPT_MAX_SPOTS + s] =
          s < n_spots ? spots[(size_t)e * n_spots + s] : pdeopt_light_spot{};
  const size_t n = ctx->spots_host.size();
  const bool f32 = ctx->prob.dtype == PDEOPT_F32;
  const size_t bytes = n * 7 * (f32 ? sizeof(float) : sizeof(double));
  if ((rc = ensure_buffer(ctx, ctx->spots_dev, bytes))) return rc;
  std::vector<char> packed(bytes);
  for (size_t i = 0; i < n; ++i) {
    const pdeopt_light_spot& q = ctx->spots_host[i];
    const double v[7] = {q.amp0, q.amp_rate, q.x0, q.x_rate, q.y0, q.y_rate, q.inv_two_w2};
    for (int c = 0; c < 7; ++c) {
      if (f32)
        reinterpret_cast<float*>(packed.data())[i * 7 + c] = (float)v[c];
      else
        reinterpret_cast<double*>(packed.data())[i * 7 + c] = v[c];
    }
  }
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(ctx->spots_dev.get(), packed.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PDEOPT_OK;
}

int pdeopt_set_env_imex_scale(pdeopt_ctx* ctx, int env_first, int env_count, const double* sigma) {
  if (!ctx || !sigma) return PDEOPT_EINVAL;
  int rc = check_envs(ctx, env_first, env_count);
  if (rc) return rc;
  for (int i = 0; i < env_count; ++i)
    if (!(sigma[i] > 0.0)) return fail(ctx, PDEOPT_EINVAL, "imex scale %g of environment %d must be positive", sigma[i], env_first + i);
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  ctx->imex_per_env = with_dtype(ctx, [&](auto t) { return patch_imex_scale<decltype(t)>(ctx, env_first, env_count, sigma); });
  return upload_env_params(ctx);
}

int pdeopt_set_env_gpe_k(pdeopt_ctx* ctx, int env_first, int env_count, const double* k) {
  if (!ctx || !k) return PDEOPT_EINVAL;
  int rc = check_envs(ctx, env_first, env_count);
  if (rc) return rc;
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  with_dtype(ctx, [&](auto t) { patch_env_gpe_k<decltype(t)>(ctx, env_first, env_count, k); });
  return upload_env_params(ctx);
}

int pdeopt_set_gpe_rotation(pdeopt_ctx* ctx, double omega, double x_first, double y_first) {
  if (!ctx) return PDEOPT_EINVAL;
  if (!ctx->configured) return fail(ctx, PDEOPT_ESTATE, "pdeopt_configure has not been called");
  if (ctx->prob.equation != PDEOPT_EQ_GPE) return fail(ctx, PDEOPT_EINVAL, "the rotation frequency belongs to the GPE");
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  ctx->rot_set = true;
  ctx->rot_x_first = x_first;
  ctx->rot_y_first = y_first;
  with_dtype(ctx, [&](auto t) { patch_env_gpe_omega<decltype(t)>(ctx, 0, ctx->prob.batch, nullptr, omega); });
  ctx->rot_any_rate = with_dtype(ctx, [&](auto t) { return patch_env_gpe_omega_rate<decltype(t)>(ctx, 0, ctx->prob.batch, nullptr); });
  return upload_env_params(ctx);
}

int pdeopt_set_env_gpe_omega(pdeopt_ctx* ctx, int env_first, int env_count, const double* omega) {
  if (!ctx || !omega) return PDEOPT_EINVAL;
  int rc = check_envs(ctx, env_first, env_count);
  if (rc) return rc;
  if (ctx->prob.equation != PDEOPT_EQ_GPE) return fail(ctx, PDEOPT_EINVAL, "the rotation frequency belongs to the GPE");
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  with_dtype(ctx, [&](auto t) { patch_env_gpe_omega<decltype(t)>(ctx, env_first, env_count, omega, 0.0); });
  return upload_env_params(ctx);
}

int pdeopt_set_env_gpe_omega_rate(pdeopt_ctx* ctx, int env_first, int env_count, const double* rate) {
  if (!ctx || !rate) return PDEOPT_EINVAL;
  int rc = check_envs(ctx, env_first, env_count);
  if (rc) return rc;
  if (ctx->prob.equation != PDEOPT_EQ_GPE) return fail(ctx, PDEOPT_EINVAL, "the rotation frequency belongs to the GPE");
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  ctx->rot_any_rate = with_dtype(ctx, [&](auto t) { return patch_env_gpe_omega_rate<decltype(t)>(ctx, env_first, env_count, rate); });
  return upload_env_params(ctx);
}

int pdeopt_set_state(pdeopt_ctx* ctx, int env_first, int env_count, const void* host) {
  if (!ctx || !host) return PDEOPT_EINVAL;
  int rc = check_envs(ctx, env_first, env_count);
  if (rc) return rc;
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const size_t eb = ctx->env_elems * ctx->esize;
  if (ctx->halo) {
    // interior of each padded tile; halo cells are filled by pdeopt_halo_unpack
    const size_t h = ctx->halo, pny = pad_ld(ctx->prob.ny, ctx->halo), row = (size_t)ctx->prob.ny * ctx->esize;
    for (int e = 0; e < env_count; ++e)
      PDEOPT_HIP_CHECK(ctx, hipMemcpy2DAsync(ctx->Y.as<char>() + eb * (env_first + e) + (h * pny + h) * ctx->esize,
                                             pny * ctx->esize, (const char*)host + (size_t)e * row * ctx->prob.nx,
                                             row, row, ctx->prob.nx, hipMemcpyHostToDevice, ctx->stream));
  } else {
    PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(ctx->Y.as<char>() + eb * env_first, host, eb * env_count,
                                         hipMemcpyHostToDevice, ctx->stream));
  }
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->tsit5_fsal_valid = false;
  ctx->tsit5_pending = false;
  return PDEOPT_OK;
}

int pdeopt_get_state(pdeopt_ctx* ctx, int env_first, int env_count, void* host) {
  if (!ctx || !host) return PDEOPT_EINVAL;
  int rc = check_envs(ctx, env_first, env_count);
  if (rc) return rc;
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const size_t eb = ctx->env_elems * ctx->esize;
  if (ctx->halo) {
    const size_t h = ctx->halo, pny = pad_ld(ctx->prob.ny, ctx->halo), row = (size_t)ctx->prob.ny * ctx->esize;
    for (int e = 0; e < env_count; ++e)
      PDEOPT_HIP_CHECK(ctx, hipMemcpy2DAsync((char*)host + (size_t)e * row * ctx->prob.nx, row,
                                             ctx->Y.as<const char>() + eb * (env_first + e) + (h * pny + h) * ctx->esize,
                                             pny * ctx->esize, row, ctx->prob.nx, hipMemcpyDeviceToHost,
                                             ctx->stream));
  } else {
    PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(host, ctx->Y.as<char>() + eb * env_first, eb * env_count,
                                         hipMemcpyDeviceToHost, ctx->stream));
  }
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PDEOPT_OK;
}

int pdeopt_state_device_ptr(pdeopt_ctx* ctx, void** dev_ptr, int64_t* bytes) {
  if (!ctx || !dev_ptr) return PDEOPT_EINVAL;
  if (!ctx->configured) return fail(ctx, PDEOPT_ESTATE, "pdeopt_configure has not been called");
  *dev_ptr = ctx->Y.get();
  if (bytes) *bytes = (int64_t)ctx->total_bytes;
  return PDEOPT_OK;
}

int pdeopt_rhs(pdeopt_ctx* ctx, double t, void* host_out) {
  if (!ctx) return PDEOPT_EINVAL;
  if (!ctx->configured) return fail(ctx, PDEOPT_ESTATE, "pdeopt_configure has not been called");
  if (ctx->prob.equation == PDEOPT_EQ_GPE)
    return fail(ctx, PDEOPT_EINVAL, "the GPE has no explicit RHS kernel (use the Strang integrator)");
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int rc = ensure_buffer(ctx, ctx->TA, ctx->total_bytes);
  if (rc) return rc;
  if ((rc = launch_rhs(ctx, whole_batch(ctx), ctx->Y.get(), ctx->TA.get(), t))) return rc;
  if (host_out) {
    PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(host_out, ctx->TA.get(), ctx->total_bytes, hipMemcpyDeviceToHost,
                                         ctx->stream));
    PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  }
  return PDEOPT_OK;
}

int pdeopt_set_jit_closures(pdeopt_ctx* ctx, const char* mu_body, const char* mob_body) {
  if (!ctx) return PDEOPT_EINVAL;
  for (const char* b : {mu_body, mob_body})
    if (b && (strchr(b, '\n') || strlen(b) > 16000 || !strstr(b, "return")))
      return fail(ctx, PDEOPT_EINVAL, "a closure body is one line of statements ending in `return ...;`");
  ctx->jit_src[0] = mu_body ? mu_body : "";
  ctx->jit_src[1] = mob_body ? mob_body : "";
  return PDEOPT_OK;
}

int pdeopt_jit_check(int dtype, const char* mu_body, const char* mob_body, char* log, int log_cap) {
  if (!mu_body || !mob_body || (dtype != PDEOPT_F32 && dtype != PDEOPT_F64)) return PDEOPT_EINVAL;
  return pdeopt::jit_check(dtype, mu_body, mob_body, log, log_cap);
}

int pdeopt_set_time_terms(pdeopt_ctx* ctx, pdeopt_time_fn fn, void* user, const double constant[3]) {
  if (!ctx) return PDEOPT_EINVAL;
  ctx->time_fn = fn;
  ctx->time_user = user;
  for (int i = 0; i < 3; ++i) ctx->time_const[i] = constant ? constant[i] : 0.0;
  ctx->tt_times.clear();  // a table belongs to the source it was sampled from
  ctx->tt_terms.clear();
  ctx->time_poly_valid = false;  // ... and so do polynomials: the caller states them again (pdeopt_set_time_terms_poly)
  ctx->tsit5_fsal_valid = false;
  return PDEOPT_OK;
}

int pdeopt_set_time_terms_poly(pdeopt_ctx* ctx, int n_theta, const double* theta, int n_flux, const double* flux) {
  if (!ctx) return PDEOPT_EINVAL;
  if (n_theta < 0 || n_theta > 4 || n_flux < 0 || n_flux > 4 || (n_theta > 0 && !theta) || (n_flux > 0 && !flux))
    return fail(ctx, PDEOPT_EINVAL, "pdeopt_set_time_terms_poly: 0..4 coefficients each (cubic polynomials in t)");
  ctx->time_poly_valid = n_theta > 0;  // n_theta == 0 withdraws the polynomials
  for (int i = 0; i < 4; ++i) {
    ctx->time_theta[i] = i < n_theta ? theta[i] : 0.0;
    ctx->time_flux[i] = i < n_flux ? flux[i] : 0.0;
  }
  return PDEOPT_OK;
}

int pdeopt_set_time_table(pdeopt_ctx* ctx, int n, const double* times, const double* terms) {
  if (!ctx || n < 0 || (n > 0 && (!times || !terms))) return PDEOPT_EINVAL;
  ctx->tt_times.assign(times, times + n);
  ctx->tt_terms.assign(terms, terms + 3 * (size_t)n);
  ctx->tt_cursor = 0;
  ctx->tsit5_fsal_valid = false;
  return PDEOPT_OK;
}

int pdeopt_set_integrator_params(pdeopt_ctx* ctx, double imex_A, double time_scale_re,
                                 double time_scale_im, double strang_dx) {
  if (!ctx) return PDEOPT_EINVAL;
  ctx->imex_A = imex_A;
  ctx->ts_re = time_scale_re;
  ctx->ts_im = time_scale_im;
  ctx->strang_dx = strang_dx;
  return PDEOPT_OK;
}

int pdeopt_advance(pdeopt_ctx* ctx, int integrator, double t0, double dt, int64_t n_substeps) {
  if (!ctx) return PDEOPT_EINVAL;
  if (!ctx->configured) return fail(ctx, PDEOPT_ESTATE, "pdeopt_configure has not been called");
  if (n_substeps < 0) return fail(ctx, PDEOPT_EINVAL, "n_substeps < 0");
  if (n_substeps == 0) return PDEOPT_OK;
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  ctx->tsit5_fsal_valid = false;
  ctx->tsit5_pending = false;
  ctx->last_groups = 1;
  ctx->last_group_streams = 1;
  if (ctx->halo)
    return fail(ctx, PDEOPT_EINVAL, "padded layout: drive the substep with pdeopt_rk4_phase + halo exchange");
  // a table sampled for a fixed-step advance is stale here: the scope drops it before the advance
  if (integrator != PDEOPT_INT_EULER && integrator != PDEOPT_INT_RK4) { TimeTableScope stale(ctx); }
  const int eq = ctx->prob.equation;
  switch (integrator) {
    case PDEOPT_INT_EULER:
    case PDEOPT_INT_RK4:
      if (eq == PDEOPT_EQ_GPE)
        return fail(ctx, PDEOPT_EINVAL, "the GPE is integrated by Strang splitting only");
    {
      TimeTableScope table(ctx);
      const int rc = advance_explicit(ctx, integrator, t0, dt, n_substeps);
      return rc ? rc : table.missed();
    }
    case PDEOPT_INT_IMEX:
      if (eq != PDEOPT_EQ_CAHN_HILLIARD && eq != PDEOPT_EQ_ALLEN_CAHN && eq != PDEOPT_EQ_CAHN_HILLIARD_3D)
        return fail(ctx, PDEOPT_EINVAL, "IMEX needs a periodic Cahn-Hilliard/Allen-Cahn equation");
      return advance_imex(ctx, t0, dt, n_substeps);
    case PDEOPT_INT_STRANG:
      if (eq != PDEOPT_EQ_GPE) return fail(ctx, PDEOPT_EINVAL, "Strang splitting needs the GPE");
      return advance_strang(ctx, t0, dt, n_substeps);
    case PDEOPT_INT_STRANG_ROT:
      if (eq != PDEOPT_EQ_GPE) return fail(ctx, PDEOPT_EINVAL, "the rotating-frame split step needs the GPE");
      return advance_strang_rot(ctx, t0, dt, n_substeps);
    case PDEOPT_INT_TSIT5: {
      if (eq == PDEOPT_EQ_GPE)
        return fail(ctx, PDEOPT_EINVAL, "the GPE is integrated by Strang splitting only");
      std::vector<double> err((size_t)ctx->prob.batch);
      for (int64_t s = 0; s < n_substeps; ++s) {
        int rc = tsit5_trial(ctx, t0 + s * dt, dt, 1.0, 1.0, nullptr);
        if (rc) return rc;
        if ((rc = tsit5_commit(ctx, 1))) return rc;
      }
      return PDEOPT_OK;
    }
    case PDEOPT_INT_IMPLICIT_EULER:
      return implicit_advance(ctx, t0, dt, n_substeps, nullptr);
    default:
      return fail(ctx, PDEOPT_EINVAL, "unknown integrator %d", integrator);
  }
}

int pdeopt_snapshot(pdeopt_ctx* ctx) {
  if (!ctx) return PDEOPT_EINVAL;
  if (!ctx->configured) return fail(ctx, PDEOPT_ESTATE, "pdeopt_configure has not been called");
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int rc = ensure_buffer(ctx, ctx->SNAP, ctx->total_bytes);
  if (rc) return rc;
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(ctx->SNAP.get(), ctx->Y.get(), ctx->total_bytes, hipMemcpyDeviceToDevice,
                                       ctx->stream));
  return PDEOPT_OK;
}

int pdeopt_get_interpolated(pdeopt_ctx* ctx, double theta, int env_first, int env_count,
                            void* host_out) {
  if (!ctx || !host_out) return PDEOPT_EINVAL;
  int rc = check_envs(ctx, env_first, env_count);
  if (rc) return rc;
  if (!ctx->SNAP) return fail(ctx, PDEOPT_ESTATE, "pdeopt_snapshot has not been called");
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if ((rc = ensure_buffer(ctx, ctx->TA, ctx->total_bytes))) return rc;
  if ((rc = launch_lerp(ctx, ctx->SNAP.get(), ctx->Y.get(), ctx->TA.get(), theta, env_first, env_count))) return rc;
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(host_out, ctx->TA.get(), ctx->env_elems * ctx->esize * env_count,
                                       hipMemcpyDeviceToHost, ctx->stream));
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PDEOPT_OK;
}

int pdeopt_reduce(pdeopt_ctx* ctx, int op, double* out_per_env) {
  if (!ctx || !out_per_env) return PDEOPT_EINVAL;
  if (!ctx->configured) return fail(ctx, PDEOPT_ESTATE, "pdeopt_configure has not been called");
  if (ctx->halo) return fail(ctx, PDEOPT_EINVAL, "reductions are not available in the padded layout");
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return reduce_state(ctx, op, out_per_env);
}

int pdeopt_probe(pdeopt_ctx* ctx, const int32_t* cells, int n_probes, int env_first, int env_count,
                 double* host_out) {
  if (!ctx || !cells || !host_out) return PDEOPT_EINVAL;
  int rc = check_envs(ctx, env_first, env_count);
  if (rc) return rc;
  if (n_probes < 1) return fail(ctx, PDEOPT_EINVAL, "n_probes = %d", n_probes);
  if (ctx->halo) return fail(ctx, PDEOPT_EINVAL, "probes are not available in the padded layout");
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return env_count ? probe_state(ctx, cells, n_probes, env_first, env_count, host_out) : PDEOPT_OK;
}

int pdeopt_observe_u8(pdeopt_ctx* ctx, double lo, double hi, int env_first, int env_count,
                      uint8_t* host_out) {
  if (!ctx || !host_out) return PDEOPT_EINVAL;
  int rc = check_envs(ctx, env_first, env_count);
  if (rc) return rc;
  if (ctx->prob.equation == PDEOPT_EQ_GPE) return fail(ctx, PDEOPT_EINVAL, "observe_u8 needs a real field");
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return observe_u8(ctx, lo, hi, env_first, env_count, host_out);
}

int pdeopt_observe_u8_device(pdeopt_ctx* ctx, double lo, double hi, int env_first, int env_count, void** dev_out,
                             int64_t* nbytes) {
  if (!ctx || !dev_out) return PDEOPT_EINVAL;
  int rc = check_envs(ctx, env_first, env_count);
  if (rc) return rc;
  if (ctx->prob.equation == PDEOPT_EQ_GPE) return fail(ctx, PDEOPT_EINVAL, "observe_u8 needs a real field");
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if ((rc = observe_u8(ctx, lo, hi, env_first, env_count, nullptr))) return rc;
  *dev_out = ctx->obs_dev.get();
  if (nbytes) *nbytes = (int64_t)ctx->env_elems * env_count;
  return PDEOPT_OK;
}

int pdeopt_detect_vortices(pdeopt_ctx* ctx, double amp_thresh, double tol, int env_first, int env_count,
                           int32_t* host_winding, int64_t* host_counts) {
  if (!ctx || !host_counts) return PDEOPT_EINVAL;
  int rc = check_envs(ctx, env_first, env_count);
  if (rc) return rc;
  if (ctx->prob.equation != PDEOPT_EQ_GPE)
    return fail(ctx, PDEOPT_EINVAL, "detect_vortices needs a complex (GPE) state");
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return detect_vortices(ctx, amp_thresh, tol, env_first, env_count, host_winding, host_counts);
}

int pdeopt_gpe_observables(pdeopt_ctx* ctx, double t, int env_first, int env_count, double x_first, double y_first,
                           double* host_out) {
  if (!ctx || !host_out) return PDEOPT_EINVAL;
  int rc = check_envs(ctx, env_first, env_count);
  if (rc) return rc;
  if (ctx->prob.equation != PDEOPT_EQ_GPE)
    return fail(ctx, PDEOPT_EINVAL, "gpe_observables needs a complex (GPE) state");
  if (ctx->halo) return fail(ctx, PDEOPT_EINVAL, "gpe_observables is not available in the padded layout");
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return env_count ? gpe_observables(ctx, t, env_first, env_count, x_first, y_first, host_out) : PDEOPT_OK;
}

int pdeopt_pf_observables(pdeopt_ctx* ctx, int env_first, int env_count, double* host_out) {
  if (!ctx || !host_out) return PDEOPT_EINVAL;
  int rc = check_envs(ctx, env_first, env_count);
  if (rc) return rc;
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return pf_observables(ctx, env_first, env_count, host_out);  // (its refusals hold for an empty range too)
}

int pdeopt_sk_configure(pdeopt_ctx* ctx, const double* t0, const double* t1, const double* t2, int n_bins) {
  if (!ctx || !t0 || !t1) return PDEOPT_EINVAL;
  if (!ctx->configured) return fail(ctx, PDEOPT_ESTATE, "pdeopt_configure has not been called");
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return sk_configure(ctx, t0, t1, t2, n_bins);
}

int pdeopt_structure_factor(pdeopt_ctx* ctx, int env_first, int env_count, double* host_out) {
  if (!ctx || !host_out) return PDEOPT_EINVAL;
  int rc = check_envs(ctx, env_first, env_count);
  if (rc) return rc;
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return structure_factor(ctx, env_first, env_count, host_out);  // (its refusals hold for an empty range too)
}

int pdeopt_tsit5_trial(pdeopt_ctx* ctx, double t, double dt, double rtol, double atol,
                       double* err_norm) {
  if (!ctx) return PDEOPT_EINVAL;
  if (!ctx->configured) return fail(ctx, PDEOPT_ESTATE, "pdeopt_configure has not been called");
  if (ctx->prob.equation == PDEOPT_EQ_GPE)
    return fail(ctx, PDEOPT_EINVAL, "the GPE is integrated by Strang splitting only");
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (!ctx->kscale_prev.empty()) {
    // the FSAL slope may carry per-environment scales from pdeopt_tsit5_trial_env: recompute it
    bool ones = true;
    for (double v : ctx->kscale_prev) ones = ones && v == 1.0;
    if (!ones) ctx->tsit5_fsal_valid = false;
    ctx->kscale_prev.clear();
  }
  return tsit5_trial(ctx, t, dt, rtol, atol, err_norm);
}

int pdeopt_tsit5_solve_small_supported(pdeopt_ctx* ctx) {
  return ctx && ctx->configured && ctx->prob.equation != PDEOPT_EQ_GPE && tsit5_solve_small_supported(ctx) ? 1 : 0;
}

int pdeopt_tsit5_solve_small(pdeopt_ctx* ctx, double t0, double t1, double dt0, const pdeopt_pid* pid, int64_t max_steps,
                             int n_save, const double* save_ts, void* host_save, pdeopt_tsit5_stats* stats) {
  if (!ctx) return PDEOPT_EINVAL;
  if (!ctx->configured) return fail(ctx, PDEOPT_ESTATE, "pdeopt_configure has not been called");
  if (!pid || !stats || n_save < 0 || (n_save > 0 && (!save_ts || !host_save)))
    return fail(ctx, PDEOPT_EINVAL, "pdeopt_tsit5_solve_small: null argument");
  if (!(max_steps > 0)) return fail(ctx, PDEOPT_EINVAL, "max_steps must be positive");
  if (!(dt0 > 0) || !(t1 >= t0)) return fail(ctx, PDEOPT_EINVAL, "need dt0 > 0 and t1 >= t0");
  if (!(pid->rtol >= 0) || !(pid->atol >= 0) || !(pid->rtol + pid->atol > 0))
    return fail(ctx, PDEOPT_EINVAL, "need rtol, atol >= 0, not both zero");
  if (!(pid->factormin > 0) || !(pid->factormax >= pid->factormin) || !(pid->safety > 0))
    return fail(ctx, PDEOPT_EINVAL, "need 0 < factormin <= factormax and safety > 0");
  for (int q = 0; q < n_save; ++q)
    if (!(save_ts[q] > t0) || (q && !(save_ts[q] >= save_ts[q - 1])))
      return fail(ctx, PDEOPT_EINVAL, "save_ts must be ascending and > t0");
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  ctx->kscale_prev.clear();
  return tsit5_solve_small(ctx, t0, t1, dt0, pid, max_steps, n_save, save_ts, host_save, stats);
}

int pdeopt_tsit5_trial_env(pdeopt_ctx* ctx, double t, const double* dt, double rtol, double atol, double* dt_ref,
                           double* err_norm) {
  if (!ctx || !dt || !dt_ref) return PDEOPT_EINVAL;
  if (!ctx->configured) return fail(ctx, PDEOPT_ESTATE, "pdeopt_configure has not been called");
  if (ctx->prob.equation == PDEOPT_EQ_GPE)
    return fail(ctx, PDEOPT_EINVAL, "the GPE is integrated by Strang splitting only");
  if (ctx->time_fn || has_time_aux(ctx, PDEOPT_AUX_VX_FACE) || has_time_aux(ctx, PDEOPT_AUX_VY_FACE) ||
      ctx->prob.equation == PDEOPT_EQ_ALLEN_CAHN_SBM || ctx->prob.equation == PDEOPT_EQ_CAHN_HILLIARD_SBM)
    return fail(ctx, PDEOPT_EINVAL, "per-environment step sizes need an autonomous right-hand side (environments sit at different times)");
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int batch = ctx->prob.batch;
  double ref = 0.0;
  for (int b = 0; b < batch; ++b) {
    if (!(dt[b] >= 0.0)) return fail(ctx, PDEOPT_EINVAL, "dt[%d] = %g", b, dt[b]);
    ref = dt[b] > ref ? dt[b] : ref;
  }
  if (!(ref > 0.0)) return fail(ctx, PDEOPT_EINVAL, "every per-environment step size is zero");
  std::vector<double> sc((size_t)batch), ratio((size_t)batch, 1.0);
  if (ctx->kscale_prev.size() != (size_t)batch) ctx->kscale_prev.assign((size_t)batch, 1.0);
  bool rescale = false;
  for (int b = 0; b < batch; ++b) {
    sc[b] = dt[b] / ref;
    ratio[b] = ctx->kscale_prev[b] > 0.0 ? sc[b] / ctx->kscale_prev[b] : 0.0;
    rescale = rescale || ratio[b] != 1.0;
  }
  int rc;
  // the FSAL slope K[0] of environment b carries the scale of its previous trial
  if (ctx->tsit5_fsal_valid && rescale && (rc = tsit5_rescale_fsal(ctx, ratio.data()))) return rc;
  with_dtype(ctx, [&](auto t) { patch_kscale<decltype(t)>(ctx, sc); });
  if ((rc = upload_env_params(ctx))) return rc;
  ctx->slope_scaled = true;
  rc = tsit5_trial(ctx, t, ref, rtol, atol, err_norm);
  ctx->slope_scaled = false;
  ctx->kscale_prev = sc;
  *dt_ref = ref;
  return rc;
}

int pdeopt_tsit5_commit_env(pdeopt_ctx* ctx, const uint8_t* accept) {
  if (!ctx || !accept) return PDEOPT_EINVAL;
  if (!ctx->configured) return fail(ctx, PDEOPT_ESTATE, "pdeopt_configure has not been called");
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return tsit5_commit_env(ctx, accept);
}

int pdeopt_tsit5_commit(pdeopt_ctx* ctx, int accept) {
  if (!ctx) return PDEOPT_EINVAL;
  if (!ctx->configured) return fail(ctx, PDEOPT_ESTATE, "pdeopt_configure has not been called");
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return tsit5_commit(ctx, accept);
}

int pdeopt_tsit5_dense(pdeopt_ctx* ctx, double theta, double dt, int env_first, int env_count, void* host_out) {
  if (!ctx || !host_out) return PDEOPT_EINVAL;
  int rc = check_envs(ctx, env_first, env_count);
  if (rc) return rc;
  if (!(theta >= 0.0 && theta <= 1.0)) return fail(ctx, PDEOPT_EINVAL, "theta = %g outside [0, 1]", theta);
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  // TA is free between a trial and its commit (the candidate sits in TB)
  if ((rc = tsit5_dense(ctx, theta, dt, env_first, env_count, ctx->TA.get()))) return rc;
  const size_t eb = ctx->env_elems * ctx->esize;
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(host_out, ctx->TA.as<const char>() + eb * env_first, eb * env_count,
                                       hipMemcpyDeviceToHost, ctx->stream));
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PDEOPT_OK;
}

int pdeopt_get_counter(pdeopt_ctx* ctx, int which, int64_t* value) {
  if (!ctx || !value) return PDEOPT_EINVAL;
  switch (which) {
    case PDEOPT_CNT_STAGE_LAUNCHES:
      *value = ctx->n_stage_launches;
      return PDEOPT_OK;
    case PDEOPT_CNT_LAST_GROUPS:
      *value = ctx->last_groups;
      return PDEOPT_OK;
    case PDEOPT_CNT_GROUP_STREAMS:
      *value = ctx->last_group_streams;
      return PDEOPT_OK;
    case PDEOPT_CNT_DEVICE_BYTES:
      *value = g_device_bytes.load();
      return PDEOPT_OK;
    default:
      return fail(ctx, PDEOPT_EINVAL, "unknown counter %d", which);
  }
}

int pdeopt_halo_strip_elems(pdeopt_ctx* ctx, int64_t* elems) {
  if (!ctx || !elems) return PDEOPT_EINVAL;
  if (!ctx->configured || !ctx->halo) return fail(ctx, PDEOPT_ESTATE, "no padded layout is configured");
  *elems = (int64_t)halo_strip_elems(ctx);
  return PDEOPT_OK;
}

int pdeopt_halo_pack(pdeopt_ctx* ctx, int field, void* dev_send) {
  if (!ctx) return PDEOPT_EINVAL;
  if (!ctx->configured || !ctx->halo) return fail(ctx, PDEOPT_ESTATE, "no padded layout is configured");
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return halo_pack(ctx, field, dev_send);
}

int pdeopt_halo_unpack(pdeopt_ctx* ctx, int field, const void* dev_recv, const int* neighbours) {
  if (!ctx || !neighbours) return PDEOPT_EINVAL;
  if (!ctx->configured || !ctx->halo) return fail(ctx, PDEOPT_ESTATE, "no padded layout is configured");
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return halo_unpack(ctx, field, dev_recv, neighbours);
}

int pdeopt_rk4_phase_plan(pdeopt_ctx* ctx, int* fields, int* nphases) {
  if (!ctx || !fields || !nphases) return PDEOPT_EINVAL;
  if (!ctx->configured) return fail(ctx, PDEOPT_ESTATE, "pdeopt_configure has not been called");
  return rk4_phase_plan(ctx, fields, nphases);
}

int pdeopt_rk4_phase(pdeopt_ctx* ctx, int phase, double dt) {
  if (!ctx) return PDEOPT_EINVAL;
  if (!ctx->configured) return fail(ctx, PDEOPT_ESTATE, "pdeopt_configure has not been called");
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return rk4_phase(ctx, phase, dt, 0);
}

int pdeopt_rk4_phase_part(pdeopt_ctx* ctx, int phase, double dt, int part) {
  if (!ctx) return PDEOPT_EINVAL;
  if (!ctx->configured) return fail(ctx, PDEOPT_ESTATE, "pdeopt_configure has not been called");
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return rk4_phase(ctx, phase, dt, part);
}

int pdeopt_comm_unique_id(char out[128]) {
  if (!out) return PDEOPT_EINVAL;
  return comm_unique_id(nullptr, out);
}

int pdeopt_comm_init(pdeopt_ctx* ctx, int world, int rank, const char id[128]) {
  if (!ctx || !id) return PDEOPT_EINVAL;
  if (world < 1 || rank < 0 || rank >= world) return fail(ctx, PDEOPT_EINVAL, "rank %d of %d", rank, world);
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return comm_init(ctx, world, rank, id);
}

int pdeopt_local_group_create(int world, pdeopt_local_group** out) {
  if (!out) return PDEOPT_EINVAL;
  *out = nullptr;
  if (world < 1 || world > 1024) return fail(nullptr, PDEOPT_EINVAL, "local group of %d ranks", world);
  *out = local_group_new(world);
  return PDEOPT_OK;
}

int pdeopt_local_group_destroy(pdeopt_local_group* g) {
  if (g) local_group_delete(g);
  return PDEOPT_OK;
}

int pdeopt_comm_init_local(pdeopt_ctx* ctx, pdeopt_local_group* g, int rank) {
  if (!ctx || !g) return PDEOPT_EINVAL;
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return comm_init_local(ctx, g, rank);
}

int pdeopt_comm_ipc_export(pdeopt_ctx* ctx, int world, int rank, void* handle64) {
  if (!ctx || !handle64) return PDEOPT_EINVAL;
  if (!ctx->configured || !ctx->halo) return fail(ctx, PDEOPT_ESTATE, "configure the tile in the padded layout first (the strip size is the problem's)");
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return comm_ipc_export(ctx, world, rank, handle64);
}

int pdeopt_comm_ipc_attach(pdeopt_ctx* ctx, const void* handles) {
  if (!ctx || !handles) return PDEOPT_EINVAL;
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return comm_ipc_attach(ctx, handles);
}

int pdeopt_comm_destroy(pdeopt_ctx* ctx) {
  if (!ctx) return PDEOPT_EINVAL;
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  comm_destroy(ctx);
  return PDEOPT_OK;
}

int pdeopt_rk4_decomposed_advance(pdeopt_ctx* ctx, double dt, int64_t n_substeps, const int* neighbours, int overlap) {
  if (!ctx || !neighbours) return PDEOPT_EINVAL;
  if (!ctx->configured || !ctx->halo) return fail(ctx, PDEOPT_ESTATE, "no padded layout is configured");
  if (n_substeps < 0) return fail(ctx, PDEOPT_EINVAL, "n_substeps < 0");
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return rk4_decomposed_advance(ctx, dt, n_substeps, neighbours, overlap);
}

int pdeopt_rk4_loopback_advance(pdeopt_ctx* ctx, double dt, int64_t n_substeps) {
  if (!ctx) return PDEOPT_EINVAL;
  if (!ctx->configured || !ctx->halo) return fail(ctx, PDEOPT_ESTATE, "no padded layout is configured");
  if (n_substeps < 0) return fail(ctx, PDEOPT_EINVAL, "n_substeps < 0");
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return rk4_loopback_advance(ctx, dt, n_substeps);
}

int pdeopt_ctx_create_on_stream(int device, void* hip_stream, pdeopt_ctx** out) {
  int rc = pdeopt_ctx_create(device, out);
  if (rc) return rc;
  if (hip_stream) {
    (void)hipStreamDestroy((*out)->stream);
    (*out)->stream = static_cast<hipStream_t>(hip_stream);
    (*out)->stream_borrowed = true;
  }
  return PDEOPT_OK;
}

int pdeopt_host_alloc(pdeopt_ctx* ctx, int64_t bytes, void** host) {
  if (!ctx || !host || bytes <= 0) return PDEOPT_EINVAL;
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  *host = nullptr;
  PinnedBuffer b;
  if (const int rc = ensure_buffer(ctx, b, (size_t)bytes)) return rc;
  *host = b.get();
  ctx->host_allocs.push_back(std::move(b));
  return PDEOPT_OK;
}

int pdeopt_host_free(pdeopt_ctx* ctx, void* host) {
  if (!ctx) return PDEOPT_EINVAL;
  for (size_t i = 0; i < ctx->host_allocs.size(); ++i)
    if (ctx->host_allocs[i].get() == host) {
      PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
      ctx->host_allocs.erase(ctx->host_allocs.begin() + (long)i);
      return PDEOPT_OK;
    }
  return fail(ctx, PDEOPT_EINVAL, "pointer was not returned by pdeopt_host_alloc on this ctx");
}

int pdeopt_buffer_alloc(pdeopt_ctx* ctx, int64_t bytes, void** dev) {
  if (!ctx || !dev || bytes <= 0) return PDEOPT_EINVAL;
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  *dev = nullptr;
  const hipError_t e = hipMalloc(dev, (size_t)bytes);  // the caller's from here on (pdeopt_buffer_free)
  if (e != hipSuccess) {
    *dev = nullptr;
    return fail(ctx, PDEOPT_ENOMEM, "hipMalloc(%zu bytes) failed: %s", (size_t)bytes, hipGetErrorString(e));
  }
  return PDEOPT_OK;
}

int pdeopt_buffer_free(pdeopt_ctx* ctx, void* dev) {
  if (!ctx) return PDEOPT_EINVAL;
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (dev) PDEOPT_HIP_CHECK(ctx, hipFree(dev));
  return PDEOPT_OK;
}

int pdeopt_buffer_copy(pdeopt_ctx* ctx, void* dst, const void* src, int64_t bytes, int kind) {
  if (!ctx || !dst || !src || bytes < 0) return PDEOPT_EINVAL;
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipMemcpyKind k;
  switch (kind) {
    case PDEOPT_COPY_H2D: k = hipMemcpyHostToDevice; break;
    case PDEOPT_COPY_D2H: k = hipMemcpyDeviceToHost; break;
    case PDEOPT_COPY_D2D: k = hipMemcpyDeviceToDevice; break;
    default: return fail(ctx, PDEOPT_EINVAL, "unknown copy kind %d", kind);
  }
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(dst, src, (size_t)bytes, k, ctx->stream));
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PDEOPT_OK;
}

int pdeopt_sync(pdeopt_ctx* ctx) {
  if (!ctx) return PDEOPT_EINVAL;
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PDEOPT_OK;
}

// the clock the chip holds over a timed region: one lane stamps s_memtime (shader-clock ticks) and s_memrealtime
// (constant 100 MHz) on the ctx stream next to each timer event (tools/valubench.hip measures the issue rate the same way)
__global__ void clock_stamp_kernel(unsigned long long* out) {
  out[0] = __builtin_amdgcn_s_memtime();
  out[1] = __builtin_amdgcn_s_memrealtime();
}

int pdeopt_timer_start(pdeopt_ctx* ctx) {
  if (!ctx) return PDEOPT_EINVAL;
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (const int rc = ensure_buffer(ctx, ctx->clock_stamps, 4 * sizeof(unsigned long long))) return rc;
  PDEOPT_HIP_CHECK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  hipLaunchKernelGGL(clock_stamp_kernel, dim3(1), dim3(1), 0, ctx->stream, ctx->clock_stamps.as<unsigned long long>());
  return PDEOPT_OK;
}

int pdeopt_timer_clock(pdeopt_ctx* ctx, double* shader_hz) {
  if (!ctx || !shader_hz) return PDEOPT_EINVAL;
  if (ctx->timer_shader_hz < 0.0 && ctx->clock_stamps) {
    // (not in pdeopt_timer_stop: the first device-to-host copy of a process costs ~8 ms of staging set-up, which a caller
    // timing a few milliseconds on the wall clock around timer_stop would have booked as run time)
    PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    unsigned long long h[4] = {0, 0, 0, 0};
    PDEOPT_HIP_CHECK(ctx, hipMemcpy(h, ctx->clock_stamps.get(), sizeof(h), hipMemcpyDeviceToHost));
    ctx->timer_shader_hz = (h[3] > h[1] && h[2] > h[0]) ? (double)(h[2] - h[0]) / (double)(h[3] - h[1]) * 100.0e6 : 0.0;
  }
  *shader_hz = ctx->timer_shader_hz > 0.0 ? ctx->timer_shader_hz : 0.0;
  return PDEOPT_OK;
}

int pdeopt_timer_stop(pdeopt_ctx* ctx, double* ms) {
  if (!ctx || !ms) return PDEOPT_EINVAL;
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  unsigned long long* const st = ctx->clock_stamps.as<unsigned long long>();
  if (st) hipLaunchKernelGGL(clock_stamp_kernel, dim3(1), dim3(1), 0, ctx->stream, st + 2);
  PDEOPT_HIP_CHECK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  PDEOPT_HIP_CHECK(ctx, hipEventSynchronize(ctx->ev1));
  float f = 0.f;
  PDEOPT_HIP_CHECK(ctx, hipEventElapsedTime(&f, ctx->ev0, ctx->ev1));
  *ms = (double)f;
  ctx->timer_shader_hz = -1.0;  // the stamps are fetched by pdeopt_timer_clock, outside the caller's timed region
  return PDEOPT_OK;
}

}  // extern "C"
