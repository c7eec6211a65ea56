// Internal declarations shared by the translation units of libpdeopt_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <rocfft/rocfft.h>

#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/pdeopt_hip.h"
#include "device_buffer.hpp"
#include "feature_slot.hpp"

namespace pdeopt {

constexpr int kMaxCoef = PDEOPT_CLOSURE_MAX_COEF;
constexpr int kNumAux = 8;

// Per-environment scalar parameters, stored in the arithmetic type of the path.  One struct per
// environment in device memory; kernels index it with the (wave-uniform) batch index so the
// loads are scalar.
template <typename T>
struct EnvParams {
  T kappa;
  T gpe_k;
  T kscale;  // slope scale dt_b / dt_ref of per-environment step sizes (pdeopt_tsit5_trial_env); 1 otherwise
  T imex_scale;  // sigma_b: this environment's fourier_symbol = sigma_b x the uploaded one (pdeopt_set_env_imex_scale)
  T mu[kMaxCoef];
  T mob[kMaxCoef];
  T fe[kMaxCoef];  // free-energy density closure (smoothed-boundary equations)
  T gpe_omega;     // rotation frequency of the rotating-frame GPE (pdeopt_set_gpe_rotation / pdeopt_set_env_gpe_omega)
  T gpe_omega_rate;  // its rate of change: Omega(t) = gpe_omega + gpe_omega_rate t (pdeopt_set_env_gpe_omega_rate)
};

// Gaussian light spots of the GPE control field (pdeopt_set_gpe_spots), in the arithmetic type of the path;
// device table [batch][PDEOPT_MAX_SPOTS]
template <typename T>
struct LightSpot {
  T amp0, amp_rate, x0, x_rate, y0, y_rate, c;  // c = 1 / (2 width^2)
};
// what a Strang kernel needs to evaluate lights(t, x, y) of its environment at cell (ix, iy)
template <typename T>
struct SpotArgs {
  const LightSpot<T>* table;  // nullptr / n == 0: no spots
  int n;
  T t, x_first, y_first, hx, hy;
};
template <typename T>
__device__ __forceinline__ T t_exp_neg(T x);  // exp(-x)
template <>
__device__ __forceinline__ float t_exp_neg<float>(float x) { return __expf(-x); }
template <>
__device__ __forceinline__ double t_exp_neg<double>(double x) { return exp(-x); }
template <typename T>
__device__ __forceinline__ T spots_value(const SpotArgs<T>& a, int env, T x, T y) {
  T w = T(0);
  for (int s = 0; s < a.n; ++s) {
    const LightSpot<T> q = a.table[(size_t)env * PDEOPT_MAX_SPOTS + s];
    const T dx = x - (q.x0 + q.x_rate * a.t), dy = y - (q.y0 + q.y_rate * a.t);
    w += (q.amp0 + q.amp_rate * a.t) * t_exp_neg<T>((dx * dx + dy * dy) * q.c);
  }
  return w;
}
// The sibling of spots_value for the adjoint of the Strang step (gpe_adjoint.hip): the four independent partial
// derivatives of spot s of lights(t, x, y) at one cell,
//   d[0] = d/d amp0 = G;  d[1] = d/d x0 = amp G dx 2c;  d[2] = d/d y0 = amp G dy 2c;  d[3] = d/d c = -amp G (dx^2 + dy^2)
// (amp, dx, dy and G as spots_value forms them).  The rates' partials are t times those of amp0, x0, y0.
template <typename T>
__device__ __forceinline__ void spot_partials(const SpotArgs<T>& a, int env, int s, T x, T y, T* d) {
  const LightSpot<T> q = a.table[(size_t)env * PDEOPT_MAX_SPOTS + s];
  const T dx = x - (q.x0 + q.x_rate * a.t), dy = y - (q.y0 + q.y_rate * a.t);
  const T r2 = dx * dx + dy * dy;
  const T g = t_exp_neg<T>(r2 * q.c);
  const T ag = (q.amp0 + q.amp_rate * a.t) * g;
  d[0] = g;
  d[1] = ag * dx * (T(2) * q.c);
  d[2] = ag * dy * (T(2) * q.c);
  d[3] = -ag * r2;
}

// structure of a closure (shared by the whole batch; only coefficient VALUES vary per env)
struct ClosureSpec {
  int kind;
  int flags;
  int n;
};

// Closure specialisation classes (template parameter CL of the kernels):
//   CL_GENERIC : any kind / flags / n, decided at run time (wave-uniform branches)
//   CL_POLY    : mu = cubic polynomial, mobility = quadratic polynomial, fully unrolled
//   CL_LOGIT   : as CL_POLY with the log(c/(1-c)) prior added to mu (regular-solution model)
//   CL_LOGIT1  : CL_LOGIT whose polynomial part is linear (the regular-solution model 3 (1 - 2c) of the
//                headline workload): two FMAs less per evaluation in the VALU-bound fused CH kernel
//                (coefficients past n are stored as zeros), and the fused fp32/fp64 pair kernel folds
//                -kappa lap into the same expression (stencil_fused.hpp, FOLD_MU)
//   CL_POLY_M0 : CL_POLY with a constant mobility (Allen-Cahn's R = 1, BASELINE config 2): two FMAs less
//                per evaluation in the VALU-bound single-pass RK4 kernel, bitwise equal on finite states
enum { CL_GENERIC = 0, CL_POLY = 1, CL_LOGIT = 2, CL_LOGIT1 = 3, CL_POLY_M0 = 4 };

// Where a field lives in memory.  Periodic fields: ld == ny, off == 0, wrap by index.
// Halo-padded tiles (domain decomposition): neighbours exist in memory, no wrap.
struct Geo {
  int nx, ny;       // extent of the computed region
  int ld;           // row pitch in elements
  int64_t off;      // element offset of cell (0,0) inside one environment's array
  int64_t bstride;  // elements between environments
  int periodic;     // 1: wrap indices; 0: read halo cells at i in [-2, nx+1], j in [-2, ny+1]
  int nz;           // 3-D equations: extent of the contiguous axis (1 otherwise)
};

struct AuxField {
  DeviceBuffer dev;  // its bytes() is the size of the field in the sharing mode of per_env
  int per_env = 0;
  // time-dependent source (pdeopt_set_aux_time_fn): host callback, pinned staging buffer, time last uploaded
  pdeopt_aux_fn fn = nullptr;
  void* user = nullptr;
  PinnedBuffer stage;
  double t_loaded = 0.0;
  bool loaded = false;
};

struct CommState;    // RCCL / in-process communicator + strip buffers of the decomposed driver (comm.hip)

// what a captured substep graph depends on (explicit integrators, stencil.hip)
struct GraphStructure {
  int equation, dtype, nx, ny, nz, batch, derivs;
  double hx, hy, hz;
  int mu_kind, mu_flags, mu_n, mob_kind, mob_flags, mob_n;
};
struct GraphKey {
  int kernel, fuse_stages;  // the plan's kernel family (ExplicitPlan, stencil.hip: it implies the integrator) and the fusion option it ran under
  double dt;
  void *Y, *TA, *TB, *ACC, *KS, *ep, *vx, *vy;
  int64_t kernel_path, tile_rows, ablate;
  GraphStructure structure;
};

}  // namespace pdeopt

struct pdeopt_ctx {
  int device = 0;
  int num_cus = 256;  // compute units of the device (sizes persistent launches)
  hipStream_t stream = nullptr;
  bool stream_borrowed = false;  // stream belongs to the caller (pdeopt_ctx_create_on_stream)
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  pdeopt::DeviceBuffer clock_stamps;  // [start, stop] x (s_memtime, s_memrealtime) of the timer pair
  double timer_shader_hz = 0.0;   // shader clock held between the last pdeopt_timer_start / _stop (0: not measured)
  std::string err;
  std::string last_kernel;
  bool configured = false;
  pdeopt_problem prob{};
  size_t esize = 4;        // bytes per real element
  int comps = 1;           // 2 for the GPE (re, im)
  size_t env_elems = 0;    // real elements per environment
  size_t total_bytes = 0;  // one field, whole batch
  // field buffers (device).  Y always holds the current state.
  // Every DeviceBuffer / PinnedBuffer member frees itself with the ctx; free_fields (api.hip) resets the ones that die
  // with a configuration, the others are grow-only and live as long as the ctx.
  pdeopt::DeviceBuffer Y, TA, TB, ACC, SNAP;
  pdeopt::DeviceBuffer obs_dev;   // uint8 observation frames
  pdeopt::DeviceBuffer vort_dev;  // vortex counters + winding map; grow-only
  pdeopt::DeviceBuffer KS;        // slope scratch of the spectral-RHS stage path
  pdeopt::DeviceBuffer K[7];      // Tsit5 slopes
  bool tsit5_pending = false;
  bool tsit5_fsal_valid = false;
  bool slope_scaled = false;           // stage launches multiply k by EnvParams::kscale (per-environment dt)
  std::vector<double> kscale_prev;     // scale the FSAL slope K[0] of each environment carries
  // smoothed-boundary equations: scalar terms of the right-hand side at the time it is evaluated
  pdeopt_time_fn time_fn = nullptr;
  void* time_user = nullptr;
  double time_const[3] = {0.0, 0.0, 0.0};
  // pdeopt_set_time_terms_poly: theta(t), flux(t) of the smoothed-boundary forms as cubic polynomials in t -- what the
  // in-kernel adaptive solve (stencil_coop_adaptive.hpp) evaluates at its own stage times
  bool time_poly_valid = false;
  double time_theta[4] = {0.0, 0.0, 0.0, 0.0}, time_flux[4] = {0.0, 0.0, 0.0, 0.0};
  // pdeopt_set_time_table: the three scalars at a list of evaluation times, looked up before the callback is asked
  std::vector<double> tt_times, tt_terms;
  size_t tt_cursor = 0;
  int64_t tt_misses = 0;  // stage times a non-empty table did not hold while no callback was registered
  // the three scalars the last right-hand-side launch of a time-dependent equation resolved (make_args): the tangent
  // kernels of the smoothed-boundary equations take theirs from here, so tangent and base see identical numbers
  double time_last[3] = {0.0, 0.0, 0.0};
  pdeopt::DeviceBuffer env_params_dev;
  std::vector<char> env_params_host;
  pdeopt::AuxField aux[pdeopt::kNumAux];
  std::string jit_src[2];  // pdeopt_set_jit_closures: C function bodies of mu / mobility (closure kind PDEOPT_CL_JIT)
  int64_t opt_kernel_path = 0;
  int64_t opt_tile_rows = 0;  // 0 auto, 16 or 32
  int64_t opt_group_envs = 0; // explicit integrators: envs per cache-resident group (0 auto, <0 whole batch)
  int64_t n_stage_launches = 0;  // fused stencil+update launches issued so far
  int64_t opt_halo = 0;          // requested halo width of the NEXT configure (0 periodic, 4 or 8 padded)
  int halo = 0;                  // halo width of the configured layout
  pdeopt::DeviceBuffer halo_scratch;   // single-rank loop-back buffer for pack/unpack; grow-only
  pdeopt::DeviceBuffer halo_scratch2;  // second loop-back strip (halo-8 loop: fused pack writes one while the next is read)
  int64_t opt_imex_lds_fft = 0;  // IMEX transforms: 0 auto (hand-written passes where the size is covered), -1 rocFFT
  int64_t opt_graph = 0;         // hipGraph replay of the substep loop: 0 auto (launch-bound sizes), 1 always, -1 never
  hipGraphExec_t graph_exec = nullptr;
  pdeopt::GraphKey graph_key{};
  int64_t graph_launches_per_replay = 0;
  std::string graph_name;
  int64_t opt_fuse_stages = 0;   // RK4 stage-pair fusion: 0 auto, -1 off (one launch per stage), 1 stage pairs (AC: no single-pass kernel)
  int64_t opt_debug_ablate = 0;  // timing-only ablations, results are wrong when set
  // device work block of the one-launch solves: the adaptive solves' save times, statistics and save slots
  // (small_tsit5_solve, coop_tsit5_solve; the latter also its barrier words and partial sums), the multi-workgroup fixed
  // step's tags (coop_fixed_advance).  Grow-only: a solve of a 64^2 grid is a few hundred microseconds, a hipMalloc /
  // hipFree pair is not free
  pdeopt::DeviceBuffer adaptive_blk;
  int64_t opt_group_streams = 0;  // PDEOPT_OPT_GROUP_STREAMS
  // second stream of the two-groups-side-by-side schedule and its fork / join events (created on first use); only
  // run_groups (groups.hpp) names them, launch helpers see the stream as part of a Window
  hipStream_t stream2 = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  int64_t opt_small_persist = 0; // whole-environment-step kernel for LDS-resident grids: 0 auto, 1 wherever it can, -1 never
  // Gaussian light spots of the GPE (pdeopt_set_gpe_spots)
  int n_spots = 0;
  pdeopt::DeviceBuffer spots_dev;
  std::vector<pdeopt_light_spot> spots_host;  // [batch][PDEOPT_MAX_SPOTS]
  double spots_x_first = 0.0, spots_y_first = 0.0;
  bool imex_per_env = false;  // some environment has imex_scale != 1: one environment per complex field
  int64_t last_group_streams = 1;  // PDEOPT_CNT_GROUP_STREAMS
  int64_t last_groups = 1;    // environment groups of the last advance (PDEOPT_CNT_LAST_GROUPS)
  double imex_A = 0.5, ts_re = 1.0, ts_im = 0.0, strang_dx = 1.0;
  pdeopt::DeviceBuffer red_dev;  // reduction scratch (doubles); grow-only
  pdeopt::DeviceBuffer red_mean_dev;
  pdeopt::DeviceBuffer pf_obs_dev;  // pdeopt_pf_observables: the rows [envs][8], then the workgroups' partial rows; grow-only
  // pdeopt_structure_factor: the axis tables t_0 | t_1 (| t_2) of pdeopt_sk_configure (reset by free_fields through sk_drop;
  // sk_bins = 0: none), and the call's work block -- the rows [envs][n_bins], then the workgroups' rows; grow-only
  pdeopt::DeviceBuffer sk_tab_dev;
  int sk_bins = 0;
  pdeopt::DeviceBuffer sk_dev;
  std::vector<pdeopt::PinnedBuffer> host_allocs;  // pdeopt_host_alloc
  pdeopt::CommState* comm = nullptr;
  // The feature states (feature_slot.hpp names them; each is defined in the file that uses it and owns its buffers).  A
  // state lives from its first use to the next shape-changing pdeopt_configure or to pdeopt_ctx_destroy (free_fields,
  // api.hip); a same-shape configure keeps it, and pdeopt_set_aux invalidates the multipliers the states cache.
  pdeopt::FeatureTable features;
  // rotating-frame GPE (pdeopt_set_gpe_rotation): coordinates of cell (0, 0); Omega itself lives in EnvParams
  bool rot_set = false;
  bool rot_any_rate = false;  // some environment's gpe_omega_rate is not 0: the step runs the stirred kernels of gpe_rot.hip
  double rot_x_first = 0.0, rot_y_first = 0.0;
  // pdeopt_fieldmu_adjoint_step_coef: fp64 partial sums of the mobility's coefficient gradient, one slot per
  // (trajectory, tile, coefficient); reset by free_fields, zeroed by pdeopt_configure
  pdeopt::DeviceBuffer fieldmu_coef;
  size_t fieldmu_coef_slots = 0;
};

namespace pdeopt {

// Padded (domain-decomposition) layouts.  halo 4: the tile with 4 halo cells on every side.  halo 8: 8 halo cells
// in front of the tile and 8 + a tail margin behind it -- the first stage pair of a substep runs on the tile + 4
// ring in whole workgroup tiles (32 rows x 32 16-byte vectors) that start at cell (-4, -4), so its last tile row /
// column over-runs the ring by up to a tile; the over-run cells are computed from whatever the margin holds and
// written back into it, nobody reads them.  Rows: 8 + nx + 8 + 32; row pitch: 8 + ny + 8 + 128.
constexpr int kTailRows = 32, kTailCols = 128;
inline int pad_rows(int nx, int h) { return h == 8 ? nx + 2 * h + kTailRows : nx + 2 * h; }
inline int pad_ld(int ny, int h) { return h == 8 ? ny + 2 * h + kTailCols : ny + 2 * h; }

// field geometry of the configured layout: periodic, or padded by ctx->halo cells on every side
inline Geo make_geo(const pdeopt_ctx* ctx) {
  Geo g;
  const int h = ctx->halo;
  g.nx = ctx->prob.nx;
  g.ny = ctx->prob.ny;
  g.ld = pad_ld(ctx->prob.ny, h);
  g.off = (int64_t)h * g.ld + h;
  g.bstride = (int64_t)pad_rows(ctx->prob.nx, h) * g.ld;
  g.periodic = h == 0 ? 1 : 0;
  g.nz = ctx->prob.nz > 1 ? ctx->prob.nz : 1;
  if (g.nz > 1) g.bstride *= g.nz;  // [nx][ny][nz], no halo layout in 3-D
  return g;
}

int fail(pdeopt_ctx* ctx, int code, const char* fmt, ...);

// the 2-D stencil equations' short names in the one-launch solves' last_kernel strings
inline const char* equation_short_name(int eq) {
  return eq == PDEOPT_EQ_CAHN_HILLIARD ? "CH" : eq == PDEOPT_EQ_ALLEN_CAHN ? "AC" : eq == PDEOPT_EQ_CAHN_HILLIARD_SBM ? "CH-SBM"
         : eq == PDEOPT_EQ_ALLEN_CAHN_SBM ? "AC-SBM" : eq == PDEOPT_EQ_ALLEN_CAHN_BV ? "AC-BV" : eq == PDEOPT_EQ_ALLEN_CAHN_SBM_BV ? "AC-SBM-BV" : "AD";
}
// the Butler-Volmer equations run their own two kernels (butler_volmer.hip) behind the stage launcher and nothing else
inline bool bv_equation(int eq) { return eq == PDEOPT_EQ_ALLEN_CAHN_BV || eq == PDEOPT_EQ_ALLEN_CAHN_SBM_BV; }

#define PDEOPT_HIP_CHECK(ctx, expr)                                                        \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return pdeopt::fail((ctx), PDEOPT_EHIP, "%s failed: %s (%s:%d)", #expr,              \
                          hipGetErrorString(e_), __FILE__, __LINE__);                      \
  } while (0)

// b holds `bytes` afterwards: allocated when empty; an existing block that is too small is PDEOPT_ESTATE (its owner
// should have reset it, or the site should grow)
int ensure_buffer(pdeopt_ctx* ctx, DeviceBuffer& b, size_t bytes);
int ensure_buffer(pdeopt_ctx* ctx, PinnedBuffer& b, size_t bytes);
// b holds at least need_bytes afterwards, grow-only: a block that is too small is freed first (sync_first: after the
// stream's work, which may still use it)
int grow_device_buffer(pdeopt_ctx* ctx, DeviceBuffer& b, size_t need_bytes, bool sync_first);
int ensure_stream2(pdeopt_ctx* ctx);  // the ctx's second stream + fork / join events, created on first use
// api.hip: bring a time-dependent auxiliary field to local time t (no-op for static fields)
int refresh_time_aux(pdeopt_ctx* ctx, int which, double t);
inline bool has_time_aux(const pdeopt_ctx* ctx, int which) { return ctx->aux[which].fn != nullptr; }
// a caller who turned one of the tiled path's knobs is asking for that path (the automatic choice of the one-launch kernels)
inline bool tiled_knobs_untouched(const pdeopt_ctx* ctx) {
  return ctx->opt_fuse_stages == 0 && ctx->opt_kernel_path == 0 && ctx->opt_graph == 0 && ctx->opt_group_envs == 0 && ctx->opt_tile_rows == 0;
}

// The table of pdeopt_set_time_table belongs to the advance it was sampled for: it is gone when that call returns,
// however it returns (a table left behind would override the constants of a later right-hand side).  on = false: this
// advance evaluates no time-dependent terms and leaves the table alone.
struct TimeTableScope {
  pdeopt_ctx* ctx;
  bool on;
  explicit TimeTableScope(pdeopt_ctx* c, bool on_ = true) : ctx(c), on(on_) { if (on) ctx->tt_misses = 0; }
  TimeTableScope(const TimeTableScope&) = delete;
  ~TimeTableScope() {
    if (!on) return;
    ctx->tt_times.clear();
    ctx->tt_terms.clear();
    ctx->tt_cursor = 0;
  }
  // rc of an advance that succeeded, unless stage times were missing from a table it was given (make_args counts them)
  int missed() const {
    if (!on || ctx->tt_times.empty() || !ctx->tt_misses) return PDEOPT_OK;
    return fail(ctx, PDEOPT_EINVAL, "pdeopt_set_time_table: %lld stage time(s) of this advance are not in the table and no "
                "pdeopt_set_time_terms callback is registered (times must be formed as t0 + (double) s * dt, + dt / 2, + dt)",
                (long long)ctx->tt_misses);
  }
};

// What a launch operates on: the environments [lo, lo + n) of the batch, on this stream.  Launch helpers pre-offset
// their pointers by lo and size their grid by n; kernels see a batch of n.
struct Window {
  int lo, n;
  hipStream_t stream;
};
inline Window whole_batch(const pdeopt_ctx* ctx) { return Window{0, ctx->prob.batch, ctx->stream}; }

// What only the launches on a decomposed field's tile need (stage pairs, the single-pass Cahn-Hilliard RK4 kernel).
// All zero: periodic field, or the halo is already in place and no strip is wanted.
struct HaloIo {
  int part = 0;                // tiles: 0 all, 1 interior, 2 edge (pdeopt_rk4_phase_part)
  int ext = 0;                 // PAIR_12 covers the tile + this many ring cells (halo-8 layout: 4)
  void* strip = nullptr;       // fused pack: the new state's halo strip goes here
  const void* recv = nullptr;  // fused unpack: the halo comes from these gathered strips (of neighbour ranks nbr[8])
  int nbr[8] = {};
  const void* peer[8] = {};    // ... or from the neighbours' own strip buffers (peer-mapped exchange)
};

// where a fused-unpack launch finds the strips of its 8 neighbours: slices of the gathered buffer (recv + rank * strip
// elements), or the neighbours' own buffers (peer); all nullptr: no fused unpack
template <typename T>
inline void fill_neighbour_strips(const HaloIo& io, int64_t strip_rank_elems, const T** nbase) {
  for (int q = 0; q < 8; ++q) {
    if (io.peer[0]) nbase[q] = static_cast<const T*>(io.peer[q]);
    else if (io.recv) nbase[q] = static_cast<const T*>(io.recv) + (int64_t)io.nbr[q] * strip_rank_elems;
    else nbase[q] = nullptr;
  }
}
// light spots of the environments from first_env on, at local time t
template <typename T>
inline SpotArgs<T> make_spot_args(const pdeopt_ctx* ctx, int first_env, double t) {
  SpotArgs<T> a{};
  a.n = ctx->n_spots;
  a.table = a.n ? ctx->spots_dev.as<const LightSpot<T>>() + (size_t)first_env * PDEOPT_MAX_SPOTS : nullptr;
  a.t = T(t);
  a.x_first = T(ctx->spots_x_first);
  a.y_first = T(ctx->spots_y_first);
  a.hx = T(ctx->prob.hx);
  a.hy = T(ctx->prob.hy);
  return a;
}

// stencil.hip: out = f(t, in) for the environments of the window
int launch_rhs(pdeopt_ctx* ctx, const Window& w, const void* in, void* out, double t);
// the same slope for the IMEX step: the stage-B half of the fused pair kernel where it applies (CH, periodic
// layout, polynomial / logit closures), launch_rhs otherwise; equal to launch_rhs up to rounding
int launch_rhs_slope(pdeopt_ctx* ctx, const Window& w, const void* in, void* out, double t);
int advance_explicit(pdeopt_ctx* ctx, int integrator, double t0, double dt, int64_t n);
int tsit5_trial(pdeopt_ctx* ctx, double t, double dt, double rtol, double atol, double* err);
int tsit5_commit(pdeopt_ctx* ctx, int accept);
int tsit5_dense(pdeopt_ctx* ctx, double theta, double dt, int env_first, int env_count, void* dev_out);
int tsit5_commit_env(pdeopt_ctx* ctx, const uint8_t* accept);
int tsit5_rescale_fsal(pdeopt_ctx* ctx, const double* ratio);  // K[0] of environment b *= ratio[b]
bool tsit5_solve_small_supported(const pdeopt_ctx* ctx);
int tsit5_solve_small(pdeopt_ctx* ctx, double t0, double t1, double dt0, const pdeopt_pid* pid, int64_t max_steps, int n_save,
                      const double* save_ts, void* save_host, pdeopt_tsit5_stats* stats);
void graph_destroy(pdeopt_ctx* ctx);
int launch_lerp(pdeopt_ctx* ctx, const void* a, const void* b, void* out, double theta,
                size_t env_first, size_t env_count);
// halo.hip (domain decomposition: padded, non-periodic layout)
int halo_pack(pdeopt_ctx* ctx, int field, void* dev_send);
int halo_unpack(pdeopt_ctx* ctx, int field, const void* dev_recv, const int* nbr);
size_t halo_strip_elems(const pdeopt_ctx* ctx);
int rk4_phase(pdeopt_ctx* ctx, int phase, double dt, int part = 0);
int rk4_loopback_advance(pdeopt_ctx* ctx, double dt, int64_t n);
// halo-8 layout: one substep = [unpack(Y), or fused into the first pair] -> PAIR_12 on the tile + 4 ring -> PAIR_34 (+ the new state's halo strip
// written into `strip` by the edge tiles' epilogue when strip != nullptr); Y / TA are swapped
// recv != nullptr: the halo of the state is NOT in the field yet -- the first pair's edge tiles read it from the
// gathered strips `recv` (neighbour ranks nbr[8]) and write the frame cells back (fused unpack)
int rk4_substep_h8(pdeopt_ctx* ctx, double dt, void* strip, const void* recv = nullptr, const int* nbr = nullptr);
// the same with the halo taken from the 8 neighbours' OWN strip buffers (peer-mapped exchange: comm.hip)
int rk4_substep_h8_peer(pdeopt_ctx* ctx, double dt, void* strip, const void* const* peer);
int rk4_phase_plan(pdeopt_ctx* ctx, int* fields, int* nphases);
void* field_ptr(pdeopt_ctx* ctx, int field);
// comm.hip
int comm_unique_id(pdeopt_ctx* ctx, char* out128);
int comm_init(pdeopt_ctx* ctx, int world, int rank, const char* id128);
int comm_init_local(pdeopt_ctx* ctx, pdeopt_local_group* g, int rank);
pdeopt_local_group* local_group_new(int world);
void local_group_delete(pdeopt_local_group* g);
void comm_destroy(pdeopt_ctx* ctx);
int rk4_decomposed_advance(pdeopt_ctx* ctx, double dt, int64_t n, const int* nbr, int overlap);
int comm_ipc_export(pdeopt_ctx* ctx, int world, int rank, void* handle64);
int comm_ipc_attach(pdeopt_ctx* ctx, const void* handles);
// reduce.hip
int reduce_state(pdeopt_ctx* ctx, int op, double* out);
int probe_state(pdeopt_ctx* ctx, const int32_t* cells, int n_probes, int env_first, int env_count, double* host_out);
int observe_u8(pdeopt_ctx* ctx, double lo, double hi, int env_first, int env_count, void* host_out);
int detect_vortices(pdeopt_ctx* ctx, double amp_thresh, double tol, int env_first, int env_count,
                    int32_t* host_winding, int64_t* host_counts);
// spectral.hip
int advance_imex(pdeopt_ctx* ctx, double t0, double dt, int64_t n);
int rhs_fourier(pdeopt_ctx* ctx, const void* in, void* out);
int advance_strang(pdeopt_ctx* ctx, double t0, double dt, int64_t n);
// jit.hip: do these closure bodies compile (hiprtc, gfx950)?
int jit_check(int dtype, const char* mu_body, const char* mob_body, char* log_out, int log_cap);
// strang_fused.hip
bool strang_fused_supported(const pdeopt_ctx* ctx);
int advance_strang_fused(pdeopt_ctx* ctx, double t0, double dt, int64_t n);
bool imex_fused_supported(const pdeopt_ctx* ctx);
int advance_imex_fused(pdeopt_ctx* ctx, double dt, int64_t n);
// the IMEX step's transforms alone, for callers that form the slope TA themselves (sens.hip): prepare the multiplier
// of step dt, then y += dt L^-1 TA over the environments of the window
int imex_fused_prepare(pdeopt_ctx* ctx, double dt);
int imex_fused_passes(pdeopt_ctx* ctx, const Window& w, double dt);
// the same split of the rocFFT IMEX step (spectral.hip; any grid, 3-D included): plans, work fields and the
// half-spectrum multiplier of step dt, then y += dt L^-1 TA over the whole batch (r2c, multiply, c2r, axpy)
int imex_rocfft_prepare(pdeopt_ctx* ctx, double dt);
int imex_rocfft_solve(pdeopt_ctx* ctx, double dt);
// the two halves of imex_rocfft_solve for callers that need them apart (fieldmu.hip): TA = L^-1 TA (r2c, multiply,
// c2r; the multiplier of the last imex_rocfft_prepare), and y += dt TA
int imex_rocfft_apply(pdeopt_ctx* ctx);
int axpy_state(pdeopt_ctx* ctx, double dt);
// The rocFFT IMEX step of a sensitivity batch (B trajectories, then tangent j of trajectory b at B + j B + b) with a
// kappa tangent among its P roles (sens.hip).  prepare_kappa, after imex_rocfft_prepare: the derivative of the
// half-spectrum multiplier, m' = -(1/n) A dt (s / kappa) / (1 + A dt s)^2, built in double and symmetrised like m; the
// symbol s is taken to be LINEAR in kappa (the equation classes publish kappa K2^2), so ds/dkappa = s / kappa.
// solve_kappa: r2c, sens_imex_mul_kappa_kernel (c_j m, plus c_base m' for the kappa tangent), c2r, axpy
int imex_rocfft_prepare_kappa(pdeopt_ctx* ctx, double dt, double kappa);
int imex_rocfft_solve_kappa(pdeopt_ctx* ctx, double dt, int B, int P, const int* role);
// one unnormalised complex transform of a whole-batch field [batch][nx][ny], in place, on the ctx's stream (the C2C
// plans of the library Strang path: any grid); host copy of a shared complex aux field
int spectral_c2c(pdeopt_ctx* ctx, bool forward, void* buf);
// one unnormalised real-to-hermitian transform of the resident state, whole batch (the plans of the rocFFT IMEX step:
// any 2-D / 3-D grid), into the hermitian work field, which is scratch between steps: *half is [batch][*half_cells]
// interleaved complex in the state's dtype, the last axis halved.  The state is not modified
int spectral_r2c_state(pdeopt_ctx* ctx, void** half, int64_t* half_cells);
// the pieces of that call for a caller that transforms fields of its own (implicit.hip): the plans and the hermitian work
// field, then one unnormalised transform of a whole-batch field, real `in` to hermitian `out` (forward) or hermitian `in`
// to real `out`, out of place; the inverse may overwrite its input
int spectral_real_prepare(pdeopt_ctx* ctx, void** half, int64_t* half_cells);
int spectral_real_exec(pdeopt_ctx* ctx, bool forward, void* in, void* out);
int spectral_fetch_complex_aux(pdeopt_ctx* ctx, int which, std::vector<std::complex<double>>& out);
// one unnormalised complex transform along ONE axis (0: x, lines of stride ny; 1: y, contiguous lines) of a
// whole-batch field [batch][nx][ny], in place, on the ctx's stream: rocFFT batched 1-D plans, any grid
int spectral_c2c_axis(pdeopt_ctx* ctx, int axis, bool forward, void* buf);
// gpe_rot.hip: the rotating-frame ADI split step (PDEOPT_INT_STRANG_ROT)
int advance_strang_rot(pdeopt_ctx* ctx, double t0, double dt, int64_t n);
// gpe_obs.hip: energy terms, angular momentum and moments of the resident GPE state, [env_count][PDEOPT_GPE_OBS_COUNT]
// doubles
int gpe_observables(pdeopt_ctx* ctx, double t, int env_first, int env_count, double x_first, double y_first,
                    double* host_out);
// pf_obs.hip: mass, free energy, chemical-potential moments and dissipation of the resident phase-field state (periodic
// CH, AC, CH-3D with finite differences), [env_count][PDEOPT_PF_OBS_COUNT] doubles; refuses what it does not cover
int pf_observables(pdeopt_ctx* ctx, int env_first, int env_count, double* host_out);
// structure_factor.hip: the shell sums P_b of the resident real state's power spectrum, [env_count][n_bins] doubles, from
// the axis tables of sk_configure; sk_drop forgets the tables (a new grid), the work block lives with the ctx
int sk_configure(pdeopt_ctx* ctx, const double* t0, const double* t1, const double* t2, int n_bins);
int structure_factor(pdeopt_ctx* ctx, int env_first, int env_count, double* host_out);
void sk_drop(pdeopt_ctx* ctx);
// butler_volmer.hip: parameters of the Butler-Volmer equations; the voltage of the resident state (recompute) or the one
// the last right-hand side used
int bv_set_params(pdeopt_ctx* ctx, double alpha, int mode, const double* per_env);
int bv_voltage(pdeopt_ctx* ctx, int env_first, int env_count, double* host_out, bool recompute);
// does the right-hand side depend on t?  (a voltage protocol v(t) registered for the given-voltage mode)
bool bv_time_dependent(const pdeopt_ctx* ctx);
// the tangent-linear right-hand side of those equations (sens.hip drives it): the P parameters of B trajectories in the
// layout of pdeopt_sens_configure.  bv_sens_slopes writes the tangent block of `out` for the whole-batch field `in` (at
// constant current after the base block's own slope launch of the same `in`); bv_sens_voltage returns v and dv/dp_j of the
// resident state, [B][1 + P]
constexpr int kMaxSens = 2 * PDEOPT_CLOSURE_MAX_COEF;
struct BvSensSpec {
  int B, P;
  const int* role;
  const int* index;
};
int bv_sens_slopes(pdeopt_ctx* ctx, const BvSensSpec& sp, const void* in, void* out);
int bv_sens_voltage(pdeopt_ctx* ctx, const BvSensSpec& sp, double* host_out);
bool bv_params_set(const pdeopt_ctx* ctx);  // has pdeopt_set_bv_params been called for this batch?
// sens_sbm.hip: the tangent-linear right-hand side of the smoothed-boundary equations (PDEOPT_EQ_ALLEN_CAHN_SBM /
// _CAHN_HILLIARD_SBM), same layout: writes the tangent block of `out` for the whole-batch field `in`, with the time terms
// ctx->time_last of the base block's own slope launch of the same `in` (which sens.hip issues first)
int sbm_sens_slopes(pdeopt_ctx* ctx, const BvSensSpec& sp, const void* in, void* out);
inline bool sbm_equation(int eq) { return eq == PDEOPT_EQ_ALLEN_CAHN_SBM || eq == PDEOPT_EQ_CAHN_HILLIARD_SBM; }
// implicit.hip: n implicit Euler steps (stats: [batch][4] totals or nullptr)
int implicit_advance(pdeopt_ctx* ctx, double t0, double dt, int64_t n, int64_t* stats);

}  // namespace pdeopt

#include "launch_util.hpp"
