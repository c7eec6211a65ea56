// Spectral integrators on rocFFT: SemiImplicitFourierSpectral.step and StrangSplitting.step
// (pde_opt/numerics/solvers.py:56-70 and :99-122), batched over environments.
//
//   IMEX    y1 = y0 + dt Re ifftn( fftn(rhs(y0)) / (1 + A dt fourier_symbol) )        solvers.py:58-63
//   Strang  tau = dt * time_scale;  E = exp(A_term tau / 2)
//           psi1 = ifft(fft(psi0) E);  b = B(t0, psi0)  (PRE-half-step state, :109)
//           psi2 = psi1 exp(b tau);    psi3 = psi2 / sqrt(sum |psi2|^2 dx^2)  (:111, every step)
//           psi4 = ifft(fft(psi3) E)
//   with b = -i (V + k |psi0|^2)  (gross_pitaevskii.py:67-75; V = trap + lights, an aux field).
//
// rocFFT transforms are unnormalised; the 1/N of ifft is folded into the spectral multipliers,
// and the per-environment normalisation scalar of psi3 is folded into the second spectral
// multiply (the FFT is linear), which saves one pass over the field.
#include <algorithm>
#include <cmath>
#include <complex>
#include <mutex>

#include "closures.hpp"
#include "common.hpp"

namespace pdeopt {

struct Spectral : Feature {
  bool setup = false;
  rocfft_plan fwd = nullptr, inv = nullptr;
  rocfft_execution_info info = nullptr;
  DeviceBuffer work;
  size_t work_bytes = 0;   // what the two plans ask for
  DeviceBuffer cbuf;       // complex work field (IMEX, rhs_fourier)
  DeviceBuffer cbuf2;      // rhs_fourier work fields
  DeviceBuffer cbuf3;
  DeviceBuffer mult;       // complex spectral multiplier, shared [nx][ny]
  DeviceBuffer dens;       // real |psi0|^2 (Strang)
  DeviceBuffer partial;    // doubles [batch][kNormBlocks]
  DeviceBuffer scale;      // doubles [batch]
  // real <-> hermitian transforms of the IMEX step (half the bytes of C2C)
  rocfft_plan r2c = nullptr, c2r = nullptr;
  rocfft_execution_info rinfo = nullptr;
  DeviceBuffer rwork;
  DeviceBuffer hbuf;       // hermitian half-spectrum work field
  DeviceBuffer hmult;      // multiplier on the half-spectrum
  DeviceBuffer hmultk;     // d hmult / d kappa (sensitivities of kappa), cached on (dt, A, kappa)
  double multk_dt = NAN, multk_A = NAN, multk_kappa = NAN;
  int64_t half_cells = 0;  // complex elements of one half-spectrum
  // batched 1-D complex plans along one axis of a [batch][nx][ny] field (the rotating-frame split step on grids the
  // hand-written passes do not cover): [0] along x (stride ny, one environment per execution), [1] along y
  rocfft_plan ax_fwd[2] = {nullptr, nullptr}, ax_inv[2] = {nullptr, nullptr};
  rocfft_execution_info ax_info = nullptr;
  DeviceBuffer ax_work;
  // cache key of `mult` / `hmult`
  int mult_kind = -1;
  double mult_dt = NAN, mult_A = NAN, mult_tr = NAN, mult_ti = NAN;

  void invalidate() override {
    mult_kind = -1;
    multk_dt = NAN;
  }
  // the body runs before the members go: the work fields are freed after the plans that were given them
  ~Spectral() override {
    for (int a = 0; a < 2; ++a) {
      if (ax_fwd[a]) rocfft_plan_destroy(ax_fwd[a]);
      if (ax_inv[a]) rocfft_plan_destroy(ax_inv[a]);
    }
    if (ax_info) rocfft_execution_info_destroy(ax_info);
    if (r2c) rocfft_plan_destroy(r2c);
    if (c2r) rocfft_plan_destroy(c2r);
    if (rinfo) rocfft_execution_info_destroy(rinfo);
    if (fwd) rocfft_plan_destroy(fwd);
    if (inv) rocfft_plan_destroy(inv);
    if (info) rocfft_execution_info_destroy(info);
  }
};

namespace {

constexpr int kNormBlocks = 128;

#define PDEOPT_FFT_CHECK(ctx, expr)                                                         \
  do {                                                                                      \
    rocfft_status s_ = (expr);                                                              \
    if (s_ != rocfft_status_success)                                                        \
      return fail((ctx), PDEOPT_EFFT, "%s failed with rocfft_status %d (%s:%d)", #expr,    \
                  (int)s_, __FILE__, __LINE__);                                            \
  } while (0)

std::once_flag g_rocfft_once;

int ensure_plans(pdeopt_ctx* ctx) {
  Spectral& sp = ctx->features.ensure<Spectral>(FS_SPECTRAL);
  if (sp.setup) return PDEOPT_OK;
  std::call_once(g_rocfft_once, [] { rocfft_setup(); });
  const pdeopt_problem& p = ctx->prob;
  // rocFFT lengths are fastest-first; a dimension of length 1 is dropped (256 x 1 "1-D" runs
  // of tests/test_solvers.py:21-61)
  size_t lengths[3];
  size_t dims = 0;
  if (p.nz > 1) lengths[dims++] = (size_t)p.nz;  // 3-D equations: z is the contiguous axis
  if (p.ny > 1) lengths[dims++] = (size_t)p.ny;
  if (p.nx > 1) lengths[dims++] = (size_t)p.nx;
  if (dims == 0) lengths[dims++] = 1;
  const rocfft_precision prec =
      p.dtype == PDEOPT_F32 ? rocfft_precision_single : rocfft_precision_double;
  PDEOPT_FFT_CHECK(ctx, rocfft_plan_create(&sp.fwd, rocfft_placement_inplace,
                                           rocfft_transform_type_complex_forward, prec, dims,
                                           lengths, (size_t)p.batch, nullptr));
  PDEOPT_FFT_CHECK(ctx, rocfft_plan_create(&sp.inv, rocfft_placement_inplace,
                                           rocfft_transform_type_complex_inverse, prec, dims,
                                           lengths, (size_t)p.batch, nullptr));
  size_t w1 = 0, w2 = 0;
  PDEOPT_FFT_CHECK(ctx, rocfft_plan_get_work_buffer_size(sp.fwd, &w1));
  PDEOPT_FFT_CHECK(ctx, rocfft_plan_get_work_buffer_size(sp.inv, &w2));
  sp.work_bytes = w1 > w2 ? w1 : w2;
  PDEOPT_FFT_CHECK(ctx, rocfft_execution_info_create(&sp.info));
  if (sp.work_bytes) {
    int rc = ensure_buffer(ctx, sp.work, sp.work_bytes);
    if (rc) return rc;
    PDEOPT_FFT_CHECK(ctx, rocfft_execution_info_set_work_buffer(sp.info, sp.work.get(), sp.work_bytes));
  }
  PDEOPT_FFT_CHECK(ctx, rocfft_execution_info_set_stream(sp.info, ctx->stream));
  sp.setup = true;
  return PDEOPT_OK;
}

// real-to-hermitian plans.  The fastest non-trivial dimension is the one rocFFT halves.
int ensure_real_plans(pdeopt_ctx* ctx) {
  Spectral& sp = *ctx->features.get<Spectral>(FS_SPECTRAL);
  if (sp.r2c) return PDEOPT_OK;
  const pdeopt_problem& p = ctx->prob;
  size_t lengths[3];
  size_t dims = 0;
  if (p.nz > 1) lengths[dims++] = (size_t)p.nz;  // 3-D equations: z is the contiguous axis
  if (p.ny > 1) lengths[dims++] = (size_t)p.ny;
  if (p.nx > 1) lengths[dims++] = (size_t)p.nx;
  if (dims == 0) lengths[dims++] = 1;
  sp.half_cells = (int64_t)(lengths[0] / 2 + 1);
  for (size_t d = 1; d < dims; ++d) sp.half_cells *= (int64_t)lengths[d];
  const rocfft_precision prec =
      p.dtype == PDEOPT_F32 ? rocfft_precision_single : rocfft_precision_double;
  PDEOPT_FFT_CHECK(ctx, rocfft_plan_create(&sp.r2c, rocfft_placement_notinplace,
                                           rocfft_transform_type_real_forward, prec, dims, lengths,
                                           (size_t)p.batch, nullptr));
  PDEOPT_FFT_CHECK(ctx, rocfft_plan_create(&sp.c2r, rocfft_placement_notinplace,
                                           rocfft_transform_type_real_inverse, prec, dims, lengths,
                                           (size_t)p.batch, nullptr));
  size_t w1 = 0, w2 = 0;
  PDEOPT_FFT_CHECK(ctx, rocfft_plan_get_work_buffer_size(sp.r2c, &w1));
  PDEOPT_FFT_CHECK(ctx, rocfft_plan_get_work_buffer_size(sp.c2r, &w2));
  const size_t wb = w1 > w2 ? w1 : w2;
  PDEOPT_FFT_CHECK(ctx, rocfft_execution_info_create(&sp.rinfo));
  if (wb) {
    int rc = ensure_buffer(ctx, sp.rwork, wb);
    if (rc) return rc;
    PDEOPT_FFT_CHECK(ctx, rocfft_execution_info_set_work_buffer(sp.rinfo, sp.rwork.get(), wb));
  }
  PDEOPT_FFT_CHECK(ctx, rocfft_execution_info_set_stream(sp.rinfo, ctx->stream));
  return PDEOPT_OK;
}

int real_fft_exec(pdeopt_ctx* ctx, bool forward, void* in, void* out) {
  Spectral& sp = *ctx->features.get<Spectral>(FS_SPECTRAL);
  void* ib[1] = {in};
  void* ob[1] = {out};
  PDEOPT_FFT_CHECK(ctx, rocfft_execute(forward ? sp.r2c : sp.c2r, ib, ob, sp.rinfo));
  return PDEOPT_OK;
}

// 1-D plans of spectral_c2c_axis.  Along y the lines are contiguous: one plan over all nx * batch of them.  Along x a
// line has stride ny and the ny lines of an environment start one element apart; the next environment's do not
// continue that pattern, so the plan covers one environment and is executed once per environment.
int ensure_axis_plans(pdeopt_ctx* ctx) {
  Spectral& sp = ctx->features.ensure<Spectral>(FS_SPECTRAL);
  if (sp.ax_info) return PDEOPT_OK;
  std::call_once(g_rocfft_once, [] { rocfft_setup(); });
  const pdeopt_problem& p = ctx->prob;
  const rocfft_precision prec = p.dtype == PDEOPT_F32 ? rocfft_precision_single : rocfft_precision_double;
  size_t wmax = 0;
  for (int axis = 0; axis < 2; ++axis) {
    size_t len[1] = {(size_t)(axis == 0 ? p.nx : p.ny)};
    size_t stride[1] = {(size_t)(axis == 0 ? p.ny : 1)};
    const size_t dist = axis == 0 ? 1 : (size_t)p.ny;
    const size_t count = axis == 0 ? (size_t)p.ny : (size_t)p.nx * p.batch;
    rocfft_plan_description desc = nullptr;
    PDEOPT_FFT_CHECK(ctx, rocfft_plan_description_create(&desc));
    PDEOPT_FFT_CHECK(ctx, rocfft_plan_description_set_data_layout(desc, rocfft_array_type_complex_interleaved,
                                                                  rocfft_array_type_complex_interleaved, nullptr, nullptr,
                                                                  1, stride, dist, 1, stride, dist));
    PDEOPT_FFT_CHECK(ctx, rocfft_plan_create(&sp.ax_fwd[axis], rocfft_placement_inplace,
                                             rocfft_transform_type_complex_forward, prec, 1, len, count, desc));
    PDEOPT_FFT_CHECK(ctx, rocfft_plan_create(&sp.ax_inv[axis], rocfft_placement_inplace,
                                             rocfft_transform_type_complex_inverse, prec, 1, len, count, desc));
    PDEOPT_FFT_CHECK(ctx, rocfft_plan_description_destroy(desc));
    size_t w1 = 0, w2 = 0;
    PDEOPT_FFT_CHECK(ctx, rocfft_plan_get_work_buffer_size(sp.ax_fwd[axis], &w1));
    PDEOPT_FFT_CHECK(ctx, rocfft_plan_get_work_buffer_size(sp.ax_inv[axis], &w2));
    wmax = std::max(wmax, std::max(w1, w2));
  }
  PDEOPT_FFT_CHECK(ctx, rocfft_execution_info_create(&sp.ax_info));
  if (wmax) {
    int rc = ensure_buffer(ctx, sp.ax_work, wmax);
    if (rc) return rc;
    PDEOPT_FFT_CHECK(ctx, rocfft_execution_info_set_work_buffer(sp.ax_info, sp.ax_work.get(), wmax));
  }
  PDEOPT_FFT_CHECK(ctx, rocfft_execution_info_set_stream(sp.ax_info, ctx->stream));
  return PDEOPT_OK;
}

int fft_exec(pdeopt_ctx* ctx, bool forward, void* buf) {
  Spectral& sp = *ctx->features.get<Spectral>(FS_SPECTRAL);
  void* in[1] = {buf};
  PDEOPT_FFT_CHECK(ctx, rocfft_execute(forward ? sp.fwd : sp.inv, in, nullptr, sp.info));
  return PDEOPT_OK;
}

// ---------------------------------------------------------------------------------- kernels

template <typename T>
struct C2 {
  T re, im;
};

template <typename T>
__device__ __forceinline__ void t_sincos(T x, T* s, T* c);
template <>
__device__ __forceinline__ void t_sincos<float>(float x, float* s, float* c) {
  sincosf(x, s, c);
}
template <>
__device__ __forceinline__ void t_sincos<double>(double x, double* s, double* c) {
  sincos(x, s, c);
}
template <typename T>
__device__ __forceinline__ T t_expr(T x);
template <>
__device__ __forceinline__ float t_expr<float>(float x) {
  return expf(x);
}
template <>
__device__ __forceinline__ double t_expr<double>(double x) {
  return exp(x);
}

// cbuf = (k, 0)
template <typename T>
__global__ void embed_real_kernel(const T* __restrict__ k, C2<T>* __restrict__ c, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t st = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += st) c[i] = C2<T>{k[i], T(0)};
}

// c[b][cell] *= m[cell] (* scale[b])
template <typename T, bool SCALED>
__global__ void spectral_mul_kernel(C2<T>* __restrict__ c, const C2<T>* __restrict__ m,
                                    const double* __restrict__ scale, int64_t cells) {
  const int b = blockIdx.y;
  C2<T>* cb = c + (int64_t)b * cells;
  const T s = SCALED ? (T)scale[b] : T(1);
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t st = (int64_t)gridDim.x * blockDim.x;
  for (; i < cells; i += st) {
    const C2<T> v = cb[i], w = m[i];
    C2<T> r;
    r.re = (v.re * w.re - v.im * w.im) * s;
    r.im = (v.re * w.im + v.im * w.re) * s;
    cb[i] = r;
  }
}

// y += dt * Re(c)
template <typename T>
__global__ void imex_update_kernel(T* __restrict__ y, const C2<T>* __restrict__ c, T dt, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t st = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += st) y[i] += dt * c[i].re;
}

// dens = |psi|^2
template <typename T>
__global__ void density_kernel(const C2<T>* __restrict__ psi, T* __restrict__ d, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t st = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += st) {
    const C2<T> v = psi[i];
    d[i] = v.re * v.re + v.im * v.im;
  }
}

// psi *= exp(b tau), b = -i (V + k dens);  partial[b][block] = sum |psi|^2   (deterministic)
template <typename T>
__global__ __launch_bounds__(256) void strang_b_kernel(C2<T>* __restrict__ psi,
                                                       const T* __restrict__ dens,
                                                       const T* __restrict__ pot, int64_t pot_stride,
                                                       const EnvParams<T>* __restrict__ ep, T tr,
                                                       T ti, int64_t cells,
                                                       double* __restrict__ partial, const SpotArgs<T> spots, int ny) {
  const int b = blockIdx.y;
  C2<T>* pb = psi + (int64_t)b * cells;
  const T* db = dens + (int64_t)b * cells;
  const T* vb = pot ? pot + (int64_t)b * pot_stride : nullptr;
  const T kk = ep[b].gpe_k;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (int64_t)gridDim.x * 256) {
    T w = (vb ? vb[i] : T(0)) + kk * db[i];
    if (spots.n)  // lights(t0, x, y) as Gaussian spots (pdeopt_set_gpe_spots)
      w += spots_value<T>(spots, b, spots.x_first + T(i / ny) * spots.hx, spots.y_first + T(i % ny) * spots.hy);
    // exp(-i w (tr + i ti)) = exp(w ti) (cos(w tr) - i sin(w tr))
    T sn, cs;
    t_sincos<T>(w * tr, &sn, &cs);
    const T mag = (ti == T(0)) ? T(1) : t_expr<T>(w * ti);
    const T er = mag * cs, ei = -mag * sn;
    const C2<T> v = pb[i];
    C2<T> r;
    r.re = v.re * er - v.im * ei;
    r.im = v.re * ei + v.im * er;
    pb[i] = r;
    acc += (double)r.re * (double)r.re + (double)r.im * (double)r.im;
  }
  __shared__ double sh[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[(int64_t)b * gridDim.x + blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// scale[b] = 1 / sqrt(sum_b dx^2)
__global__ void norm_finalize_kernel(const double* __restrict__ partial, int nblocks, double dx2,
                                     double* __restrict__ scale, int batch) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  double s = 0.0;
  for (int i = 0; i < nblocks; ++i) s += partial[(int64_t)b * nblocks + i];
  scale[b] = 1.0 / sqrt(s * dx2);
}

inline int grid_for(int64_t n) {
  int64_t g = (n + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

template <typename T>
int upload_mult(pdeopt_ctx* ctx, const std::vector<std::complex<double>>& m) {
  Spectral& sp = *ctx->features.get<Spectral>(FS_SPECTRAL);
  const size_t cells = m.size();
  int rc = ensure_buffer(ctx, sp.mult, cells * 2 * sizeof(T));
  if (rc) return rc;
  std::vector<C2<T>> h(cells);
  for (size_t i = 0; i < cells; ++i) h[i] = C2<T>{(T)m[i].real(), (T)m[i].imag()};
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(sp.mult.get(), h.data(), cells * sizeof(C2<T>),
                                       hipMemcpyHostToDevice, ctx->stream));
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PDEOPT_OK;
}

// host copy of a complex aux field as complex<double>
int fetch_complex_aux(pdeopt_ctx* ctx, int which, std::vector<std::complex<double>>& out) {
  const AuxField& a = ctx->aux[which];
  const size_t cells = (size_t)ctx->prob.nx * ctx->prob.ny * (ctx->prob.nz > 1 ? ctx->prob.nz : 1);
  out.resize(cells);
  if (a.per_env) return fail(ctx, PDEOPT_EINVAL, "spectral aux fields must be shared across the batch");
  if (ctx->prob.dtype == PDEOPT_F32) {
    std::vector<float> h(cells * 2);
    PDEOPT_HIP_CHECK(ctx, hipMemcpy(h.data(), a.dev.get(), cells * 8, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < cells; ++i) out[i] = {h[2 * i], h[2 * i + 1]};
  } else {
    PDEOPT_HIP_CHECK(ctx, hipMemcpy(out.data(), a.dev.get(), cells * 16, hipMemcpyDeviceToHost));
  }
  return PDEOPT_OK;
}

// y += dt * r
template <typename T>
__global__ void axpy_real_kernel(T* __restrict__ y, const T* __restrict__ r, T dt, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t st = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += st) y[i] += dt * r[i];
}

// A full-spectrum multiplier m(cell q of [nx][ny][nz]) in double, symmetrised onto the half spectrum of the real
// transforms: h(k) = (m(k) + conj m(-k)) / 2 (see imex_t).  Half-spectrum layout [slow ...][fast/2+1]: the halved axis is
// the fastest non-trivial one (z for the 3-D equations, else y, else x for the ny == 1 "1-D" runs)
template <typename T, typename F>
std::vector<C2<T>> half_spectrum(const pdeopt_problem& p, int64_t hc, F m) {
  const int nzz = p.nz > 1 ? p.nz : 1;
  const int n3[3] = {p.nx, p.ny, nzz};
  auto at = [&](int i, int j, int k) -> std::complex<double> { return m(((size_t)i * p.ny + j) * nzz + k); };
  std::vector<C2<T>> h((size_t)hc);
  const int fast = nzz > 1 ? 2 : (p.ny > 1 ? 1 : 0);
  const int nh = n3[fast] / 2 + 1;
  int64_t o = 0;
  for (int i = 0; i < (fast == 0 ? nh : p.nx); ++i)
    for (int j = 0; j < (fast == 1 ? nh : (fast == 0 ? 1 : p.ny)); ++j)
      for (int k = 0; k < (fast == 2 ? nh : 1); ++k) {
        const std::complex<double> v =
            0.5 * (at(i, j, k) + std::conj(at((p.nx - i) % p.nx, (p.ny - j) % p.ny, (nzz - k) % nzz)));
        h[(size_t)o++] = C2<T>{(T)v.real(), (T)v.imag()};
      }
  return h;
}

// plans, work fields and the half-spectrum multiplier of step dt (kept while dt and A hold)
template <typename T>
int imex_rocfft_prepare_t(pdeopt_ctx* ctx, double dt) {
  Spectral& sp = ctx->features.ensure<Spectral>(FS_SPECTRAL);
  const pdeopt_problem& p = ctx->prob;
  const int nzz = p.nz > 1 ? p.nz : 1;
  const int64_t cells = (int64_t)p.nx * p.ny * nzz;
  int rc;
  if ((rc = ensure_real_plans(ctx))) return rc;
  const int64_t hc = sp.half_cells;
  if ((rc = ensure_buffer(ctx, ctx->TA, ctx->total_bytes))) return rc;
  if ((rc = ensure_buffer(ctx, sp.hbuf, (size_t)hc * p.batch * 2 * sizeof(T)))) return rc;
  if (sp.mult_kind != 2 || sp.mult_dt != dt || sp.mult_A != ctx->imex_A) {
    std::vector<std::complex<double>> sym;
    if ((rc = fetch_complex_aux(ctx, PDEOPT_AUX_IMEX_SYMBOL, sym))) return rc;
    const double inv_n = 1.0 / (double)cells;
    const std::vector<C2<T>> h = half_spectrum<T>(p, hc, [&](size_t q) { return inv_n / (1.0 + ctx->imex_A * dt * sym[q]); });
    if ((rc = ensure_buffer(ctx, sp.hmult, (size_t)hc * sizeof(C2<T>)))) return rc;
    PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(sp.hmult.get(), h.data(), (size_t)hc * sizeof(C2<T>), hipMemcpyHostToDevice, ctx->stream));
    PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    sp.mult_kind = 2;
    sp.mult_dt = dt;
    sp.mult_A = ctx->imex_A;
  }
  return PDEOPT_OK;
}

// TA = Re ifftn(fftn(TA) m) over the whole batch: r2c, multiply, c2r
template <typename T>
int imex_rocfft_apply_t(pdeopt_ctx* ctx) {
  Spectral& sp = *ctx->features.get<Spectral>(FS_SPECTRAL);
  const int64_t hc = sp.half_cells;
  int rc;
  if ((rc = real_fft_exec(ctx, true, ctx->TA.get(), sp.hbuf.get()))) return rc;
  hipLaunchKernelGGL((spectral_mul_kernel<T, false>), dim3(grid_for(hc), ctx->prob.batch), dim3(256), 0,
                     ctx->stream, sp.hbuf.as<C2<T>>(), sp.hmult.as<const C2<T>>(), nullptr, hc);
  return real_fft_exec(ctx, false, sp.hbuf.get(), ctx->TA.get());
}

// y += dt TA over the whole batch
template <typename T>
int axpy_state_t(pdeopt_ctx* ctx, double dt) {
  const pdeopt_problem& p = ctx->prob;
  const int64_t total = (int64_t)p.nx * p.ny * (p.nz > 1 ? p.nz : 1) * p.batch;
  hipLaunchKernelGGL(axpy_real_kernel<T>, dim3(grid_for(total)), dim3(256), 0, ctx->stream,
                     ctx->Y.as<T>(), ctx->TA.as<const T>(), (T)dt, total);
  return PDEOPT_OK;
}

// y += dt Re ifftn(fftn(TA) m) over the whole batch: r2c, multiply, c2r, axpy
template <typename T>
int imex_rocfft_solve_t(pdeopt_ctx* ctx, double dt) {
  const int rc = imex_rocfft_apply_t<T>(ctx);
  return rc ? rc : axpy_state_t<T>(ctx, dt);
}

// ---- the IMEX multiply of a sensitivity batch whose operator moves with a parameter (kappa) -------------------------
//   dy1 = dy0 + dt Re F^-1[ F[df] m + F[f_base] m' ]
// grid (cells of the half spectrum, B): one thread takes spectrum cell i of trajectory b.  It reads the base value v0
// once, writes c[env_j][i] m[i] for every tangent j (plus v0 m'[i] where role[j] is kappa) and, last, v0 m[i] into the
// base: no other thread reads that base value, nothing is overwritten before it is used, no atomics, no extra launch.
// The products by m are spectral_mul_kernel<T, false>'s expression in its order: the bits of the base and of the other
// tangents do not depend on a kappa tangent being there.
template <typename T>
struct KappaMulArgs {
  C2<T>* c;             // [(1 + P) B][cells] half spectra
  const C2<T>* m;       // [cells]
  const C2<T>* mk;      // [cells] dm / dkappa
  int64_t cells;
  int B, P;
  int role[kMaxSens];
};

template <typename T>
__device__ __forceinline__ C2<T> spectral_mul1(const C2<T> v, const C2<T> w) {
  C2<T> r;
  r.re = (v.re * w.re - v.im * w.im) * T(1);
  r.im = (v.re * w.im + v.im * w.re) * T(1);
  return r;
}

template <typename T>
__global__ __launch_bounds__(256) void sens_imex_mul_kappa_kernel(KappaMulArgs<T> a) {
  const int b = blockIdx.y;
  const int64_t st = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.cells; i += st) {
    const C2<T> w = a.m[i];
    C2<T>* base = a.c + (int64_t)b * a.cells + i;
    const C2<T> v0 = *base;
    for (int j = 0; j < a.P; ++j) {
      C2<T>* cj = a.c + ((int64_t)a.B + (int64_t)j * a.B + b) * a.cells + i;
      C2<T> r = spectral_mul1<T>(*cj, w);
      if (a.role[j] == PDEOPT_SENS_KAPPA) {
        const C2<T> wk = a.mk[i];
        r.re += v0.re * wk.re - v0.im * wk.im;
        r.im += v0.re * wk.im + v0.im * wk.re;
      }
      *cj = r;
    }
    *base = spectral_mul1<T>(v0, w);
  }
}

template <typename T>
int imex_rocfft_prepare_kappa_t(pdeopt_ctx* ctx, double dt, double kappa) {
  Spectral& sp = *ctx->features.get<Spectral>(FS_SPECTRAL);  // (imex_rocfft_prepare has run: plans, hbuf, hmult)
  const pdeopt_problem& p = ctx->prob;
  const int64_t hc = sp.half_cells;
  if (sp.hmultk && sp.multk_dt == dt && sp.multk_A == ctx->imex_A && sp.multk_kappa == kappa) return PDEOPT_OK;
  int rc;
  std::vector<std::complex<double>> sym;
  if ((rc = fetch_complex_aux(ctx, PDEOPT_AUX_IMEX_SYMBOL, sym))) return rc;
  const double inv_n = 1.0 / (double)sym.size(), adt = ctx->imex_A * dt;
  const std::vector<C2<T>> h = half_spectrum<T>(p, hc, [&](size_t q) {
    const std::complex<double> L = 1.0 + adt * sym[q];
    return -inv_n * adt * (sym[q] / kappa) / (L * L);
  });
  if ((rc = ensure_buffer(ctx, sp.hmultk, (size_t)hc * sizeof(C2<T>)))) return rc;
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(sp.hmultk.get(), h.data(), (size_t)hc * sizeof(C2<T>), hipMemcpyHostToDevice, ctx->stream));
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  sp.multk_dt = dt;
  sp.multk_A = ctx->imex_A;
  sp.multk_kappa = kappa;
  return PDEOPT_OK;
}

template <typename T>
int imex_rocfft_solve_kappa_t(pdeopt_ctx* ctx, double dt, int B, int P, const int* role) {
  Spectral& sp = *ctx->features.get<Spectral>(FS_SPECTRAL);
  const int64_t hc = sp.half_cells;
  if (P < 1 || P > kMaxSens || (int64_t)(1 + P) * B != ctx->prob.batch)
    return fail(ctx, PDEOPT_ESTATE, "IMEX kappa multiply: batch %d is not (1 + %d) %d", ctx->prob.batch, P, B);
  int rc;
  if ((rc = real_fft_exec(ctx, true, ctx->TA.get(), sp.hbuf.get()))) return rc;
  KappaMulArgs<T> a{};
  a.c = sp.hbuf.as<C2<T>>();
  a.m = sp.hmult.as<const C2<T>>();
  a.mk = sp.hmultk.as<const C2<T>>();
  a.cells = hc;
  a.B = B;
  a.P = P;
  for (int j = 0; j < P; ++j) a.role[j] = role[j];
  hipLaunchKernelGGL(sens_imex_mul_kappa_kernel<T>, dim3(grid_for(hc), B), dim3(256), 0, ctx->stream, a);
  if ((rc = real_fft_exec(ctx, false, sp.hbuf.get(), ctx->TA.get()))) return rc;
  return axpy_state_t<T>(ctx, dt);
}

// IMEX on real <-> hermitian transforms.  The reference runs full complex transforms on the real
// field (cahn_hilliard.py:72-73) and keeps `.real` of the result (solvers.py:63).  For a real input F
// is hermitian, so  Re ifft(F m) = ifft(F m_h)  with  m_h(k) = (m(k) + conj(m(-k))) / 2 : the
// symmetrised multiplier on the half-spectrum reproduces the reference for ANY (also non-even,
// complex) fourier_symbol while moving half the bytes through rocFFT.
template <typename T>
int imex_t(pdeopt_ctx* ctx, double dt, int64_t n) {
  int rc;
  if ((rc = imex_rocfft_prepare_t<T>(ctx, dt))) return rc;
  for (int64_t s = 0; s < n; ++s) {
    if ((rc = launch_rhs(ctx, whole_batch(ctx), ctx->Y.get(), ctx->TA.get(), 0.0))) return rc;
    if ((rc = imex_rocfft_solve_t<T>(ctx, dt))) return rc;
  }
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  ctx->last_kernel += "+imex_rocfft_r2c";
  return PDEOPT_OK;
}

template <typename T>
int strang_t(pdeopt_ctx* ctx, double t0, double dt, int64_t n) {
  Spectral& sp = *ctx->features.get<Spectral>(FS_SPECTRAL);
  const pdeopt_problem& p = ctx->prob;
  const int64_t cells = (int64_t)p.nx * p.ny;
  const int64_t total = cells * p.batch;
  int rc;
  if ((rc = ensure_buffer(ctx, sp.dens, (size_t)total * sizeof(T)))) return rc;
  if ((rc = ensure_buffer(ctx, sp.partial, sizeof(double) * kNormBlocks * p.batch))) return rc;
  if ((rc = ensure_buffer(ctx, sp.scale, sizeof(double) * p.batch))) return rc;
  const std::complex<double> tau = dt * std::complex<double>(ctx->ts_re, ctx->ts_im);
  if (sp.mult_kind != 1 || sp.mult_dt != dt || sp.mult_tr != ctx->ts_re || sp.mult_ti != ctx->ts_im) {
    // E / N,  E = exp(A_term tau / 2)   (solvers.py:105)
    std::vector<std::complex<double>> a;
    if ((rc = fetch_complex_aux(ctx, PDEOPT_AUX_GPE_A_TERM, a))) return rc;
    const double inv_n = 1.0 / (double)cells;
    for (auto& v : a) v = std::exp(v * 0.5 * tau) * inv_n;
    if ((rc = upload_mult<T>(ctx, a))) return rc;
    sp.mult_kind = 1;
    sp.mult_dt = dt;
    sp.mult_tr = ctx->ts_re;
    sp.mult_ti = ctx->ts_im;
  }
  const AuxField& pot = ctx->aux[PDEOPT_AUX_GPE_POTENTIAL];
  const int64_t pot_stride = pot.per_env ? cells : 0;
  const dim3 mgrid(grid_for(cells), p.batch);
  for (int64_t s = 0; s < n; ++s) {
    hipLaunchKernelGGL(density_kernel<T>, dim3(grid_for(total)), dim3(256), 0, ctx->stream,
                       ctx->Y.as<const C2<T>>(), sp.dens.as<T>(), total);
    if ((rc = fft_exec(ctx, true, ctx->Y.get()))) return rc;
    hipLaunchKernelGGL((spectral_mul_kernel<T, false>), mgrid, dim3(256), 0, ctx->stream,
                       ctx->Y.as<C2<T>>(), sp.mult.as<const C2<T>>(), nullptr, cells);
    if ((rc = fft_exec(ctx, false, ctx->Y.get()))) return rc;
    // b = terms.vf(t0, y0): a time-dependent potential is evaluated at this substep's start time (solvers.py:109)
    if ((rc = refresh_time_aux(ctx, PDEOPT_AUX_GPE_POTENTIAL, t0 + (double)s * dt))) return rc;
    hipLaunchKernelGGL(strang_b_kernel<T>, dim3(kNormBlocks, p.batch), dim3(256), 0, ctx->stream,
                       ctx->Y.as<C2<T>>(), sp.dens.as<const T>(), pot.dev.as<const T>(), pot_stride,
                       ctx->env_params_dev.as<const EnvParams<T>>(), (T)tau.real(), (T)tau.imag(), cells,
                       sp.partial.as<double>(), make_spot_args<T>(ctx, 0, t0 + (double)s * dt), p.ny);
    hipLaunchKernelGGL(norm_finalize_kernel, dim3((p.batch + 63) / 64), dim3(64), 0, ctx->stream,
                       sp.partial.as<const double>(), kNormBlocks, ctx->strang_dx * ctx->strang_dx,
                       sp.scale.as<double>(), p.batch);
    if ((rc = fft_exec(ctx, true, ctx->Y.get()))) return rc;
    hipLaunchKernelGGL((spectral_mul_kernel<T, true>), mgrid, dim3(256), 0, ctx->stream,
                       ctx->Y.as<C2<T>>(), sp.mult.as<const C2<T>>(), sp.scale.as<const double>(), cells);
    if ((rc = fft_exec(ctx, false, ctx->Y.get()))) return rc;
  }
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  ctx->last_kernel = "strang_rocfft_c2c";
  return PDEOPT_OK;
}

// ---------------------------------------------------------------------------------------------
// pseudo-spectral right-hand sides (cahn_hilliard.py:82-87, allen_cahn.py:74-79)
//   t_hat = F[mu_h(u)] - kappa K2 F[u],   K2 = (2 pi i kx)^2 + (2 pi i ky)^2
//   CH:  rhs = Re F^-1[ ikx F[D(u) F^-1[ikx t_hat]] + iky F[D(u) F^-1[iky t_hat]] ]     (7 FFTs)
//   AC:  rhs = -R(u) Re F^-1[t_hat]                                                     (3 FFTs)
// wave numbers are formed in-kernel from the index (fftfreq(n, h), domains.py:44-47).
// ---------------------------------------------------------------------------------------------

template <typename T>
__device__ __forceinline__ T wavenumber_2pi(int idx, int n, T inv_len) {
  // 2 pi * fftfreq(n, h)[idx], inv_len = 1 / (n h)
  const int k = (idx < (n + 1) / 2) ? idx : idx - n;
  return T(6.283185307179586476925286766559) * T(k) * inv_len;
}

// a = (u, 0), b = (mu_h(u), 0)
template <typename T>
__global__ void fourier_embed_kernel(const T* __restrict__ u, C2<T>* __restrict__ a, C2<T>* __restrict__ b,
                                     const EnvParams<T>* __restrict__ ep, ClosureSpec mu, int64_t cells) {
  const int env = blockIdx.y;
  const EnvParams<T>& p = ep[env];
  const int64_t o = (int64_t)env * cells;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += (int64_t)gridDim.x * blockDim.x) {
    const T c = u[o + i];
    a[o + i] = C2<T>{c, T(0)};
    b[o + i] = C2<T>{closure_generic<T>(mu, p.mu, c), T(0)};
  }
}

// t_hat = b - kappa K2 a ;  CH: a <- ikx t_hat, b <- iky t_hat ;  AC: b <- t_hat
template <typename T, bool CH>
__global__ void fourier_that_kernel(C2<T>* __restrict__ a, C2<T>* __restrict__ b,
                                    const EnvParams<T>* __restrict__ ep, int nx, int ny, T inv_lx, T inv_ly) {
  const int env = blockIdx.y;
  const T kap = ep[env].kappa;
  const int64_t cells = (int64_t)nx * ny, o = (int64_t)env * cells;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += (int64_t)gridDim.x * blockDim.x) {
    const int ix = (int)(i / ny), iy = (int)(i % ny);
    const T kx = wavenumber_2pi<T>(ix, nx, inv_lx), ky = wavenumber_2pi<T>(iy, ny, inv_ly);
    const T k2 = -(kx * kx + ky * ky);  // (i kx)^2 + (i ky)^2
    const C2<T> ua = a[o + i], mb = b[o + i];
    const C2<T> t{mb.re - kap * k2 * ua.re, mb.im - kap * k2 * ua.im};
    if (CH) {
      a[o + i] = C2<T>{-kx * t.im, kx * t.re};  // i kx t
      b[o + i] = C2<T>{-ky * t.im, ky * t.re};
    } else {
      b[o + i] = t;
    }
  }
}

// a *= D(u)/N, b *= D(u)/N   (the 1/N of the preceding inverse transform folded in)
template <typename T>
__global__ void fourier_mob_kernel(const T* __restrict__ u, C2<T>* __restrict__ a, C2<T>* __restrict__ b,
                                   const EnvParams<T>* __restrict__ ep, ClosureSpec mob, int64_t cells, T inv_n) {
  const int env = blockIdx.y;
  const EnvParams<T>& p = ep[env];
  const int64_t o = (int64_t)env * cells;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += (int64_t)gridDim.x * blockDim.x) {
    const T d = closure_generic<T>(mob, p.mob, u[o + i]) * inv_n;
    C2<T> va = a[o + i], vb = b[o + i];
    a[o + i] = C2<T>{va.re * d, va.im * d};
    b[o + i] = C2<T>{vb.re * d, vb.im * d};
  }
}

// a <- ikx a + iky b
template <typename T>
__global__ void fourier_div_kernel(C2<T>* __restrict__ a, const C2<T>* __restrict__ b, int nx, int ny,
                                   T inv_lx, T inv_ly) {
  const int env = blockIdx.y;
  const int64_t cells = (int64_t)nx * ny, o = (int64_t)env * cells;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += (int64_t)gridDim.x * blockDim.x) {
    const int ix = (int)(i / ny), iy = (int)(i % ny);
    const T kx = wavenumber_2pi<T>(ix, nx, inv_lx), ky = wavenumber_2pi<T>(iy, ny, inv_ly);
    const C2<T> va = a[o + i], vb = b[o + i];
    a[o + i] = C2<T>{-kx * va.im - ky * vb.im, kx * va.re + ky * vb.re};
  }
}

// CH: out = Re(a)/N ;  AC: out = -R(u) Re(b)/N
template <typename T, bool CH>
__global__ void fourier_out_kernel(const T* __restrict__ u, const C2<T>* __restrict__ c, T* __restrict__ out,
                                   const EnvParams<T>* __restrict__ ep, ClosureSpec mob, int64_t cells, T inv_n) {
  const int env = blockIdx.y;
  const EnvParams<T>& p = ep[env];
  const int64_t o = (int64_t)env * cells;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += (int64_t)gridDim.x * blockDim.x) {
    const T r = c[o + i].re * inv_n;
    out[o + i] = CH ? r : -closure_generic<T>(mob, p.mob, u[o + i]) * r;
  }
}

template <typename T>
int rhs_fourier_t(pdeopt_ctx* ctx, const void* in, void* out) {
  Spectral& sp = *ctx->features.get<Spectral>(FS_SPECTRAL);
  const pdeopt_problem& p = ctx->prob;
  const int64_t cells = (int64_t)p.nx * p.ny, total = cells * p.batch;
  int rc;
  if ((rc = ensure_buffer(ctx, sp.cbuf2, (size_t)total * 2 * sizeof(T)))) return rc;
  if ((rc = ensure_buffer(ctx, sp.cbuf3, (size_t)total * 2 * sizeof(T)))) return rc;
  C2<T>* a = sp.cbuf2.as<C2<T>>();
  C2<T>* b = sp.cbuf3.as<C2<T>>();
  const T* u = (const T*)in;
  const auto* ep = ctx->env_params_dev.as<const EnvParams<T>>();
  const ClosureSpec mu{p.mu.kind, p.mu.flags, p.mu.n}, mob{p.mob.kind, p.mob.flags, p.mob.n};
  const dim3 grid(grid_for(cells), p.batch), blk(256);
  const T inv_lx = T(1.0 / (p.nx * p.hx)), inv_ly = T(1.0 / (p.ny * p.hy)), inv_n = T(1.0 / (double)cells);
  const bool ch = p.equation == PDEOPT_EQ_CAHN_HILLIARD;
  hipLaunchKernelGGL(fourier_embed_kernel<T>, grid, blk, 0, ctx->stream, u, a, b, ep, mu, cells);
  if ((rc = fft_exec(ctx, true, a))) return rc;
  if ((rc = fft_exec(ctx, true, b))) return rc;
  if (ch) {
    hipLaunchKernelGGL((fourier_that_kernel<T, true>), grid, blk, 0, ctx->stream, a, b, ep, p.nx, p.ny, inv_lx, inv_ly);
    if ((rc = fft_exec(ctx, false, a))) return rc;
    if ((rc = fft_exec(ctx, false, b))) return rc;
    hipLaunchKernelGGL(fourier_mob_kernel<T>, grid, blk, 0, ctx->stream, u, a, b, ep, mob, cells, inv_n);
    if ((rc = fft_exec(ctx, true, a))) return rc;
    if ((rc = fft_exec(ctx, true, b))) return rc;
    hipLaunchKernelGGL(fourier_div_kernel<T>, grid, blk, 0, ctx->stream, a, (const C2<T>*)b, p.nx, p.ny, inv_lx, inv_ly);
    if ((rc = fft_exec(ctx, false, a))) return rc;
    hipLaunchKernelGGL((fourier_out_kernel<T, true>), grid, blk, 0, ctx->stream, u, (const C2<T>*)a, (T*)out, ep, mob, cells, inv_n);
  } else {
    hipLaunchKernelGGL((fourier_that_kernel<T, false>), grid, blk, 0, ctx->stream, a, b, ep, p.nx, p.ny, inv_lx, inv_ly);
    if ((rc = fft_exec(ctx, false, b))) return rc;
    hipLaunchKernelGGL((fourier_out_kernel<T, false>), grid, blk, 0, ctx->stream, u, (const C2<T>*)b, (T*)out, ep, mob, cells, inv_n);
  }
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  ctx->last_kernel = ch ? "rhs_fourier<CH>(rocfft x7)" : "rhs_fourier<AC>(rocfft x3)";
  return PDEOPT_OK;
}

// ---------------------------------------------------------------------------------------------
// CahnHilliard3DPeriodic.rhs_fourier (cahn_hilliard.py:167-175), fields [b][nx][ny][nz]:
//   t_hat = F[mu_h(u)] - kappa K2 F[u];   rhs = Re F^-1[ sum_d i k_d F[ D(u) F^-1[ i k_d t_hat ] ] ]   (9 FFTs)
// one axis at a time through a single work field, the divergence accumulated in spectral space.
// ---------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void wave3(int64_t i, int nx, int ny, int nz, T ilx, T ily, T ilz, T* k) {
  const int iz = (int)(i % nz), iy = (int)((i / nz) % ny), ix = (int)(i / ((int64_t)nz * ny));
  k[0] = wavenumber_2pi<T>(ix, nx, ilx);
  k[1] = wavenumber_2pi<T>(iy, ny, ily);
  k[2] = wavenumber_2pi<T>(iz, nz, ilz);
}

// b <- t_hat = b - kappa K2 a
template <typename T>
__global__ void fourier3_that_kernel(const C2<T>* __restrict__ a, C2<T>* __restrict__ b, const EnvParams<T>* __restrict__ ep,
                                     int nx, int ny, int nz, T ilx, T ily, T ilz) {
  const int env = blockIdx.y;
  const T kap = ep[env].kappa;
  const int64_t cells = (int64_t)nx * ny * nz, o = (int64_t)env * cells;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += (int64_t)gridDim.x * blockDim.x) {
    T k[3];
    wave3<T>(i, nx, ny, nz, ilx, ily, ilz, k);
    const T k2 = -(k[0] * k[0] + k[1] * k[1] + k[2] * k[2]);
    const C2<T> ua = a[o + i], mb = b[o + i];
    b[o + i] = C2<T>{mb.re - kap * k2 * ua.re, mb.im - kap * k2 * ua.im};
  }
}

// w <- i k_axis t_hat
template <typename T>
__global__ void fourier3_grad_kernel(const C2<T>* __restrict__ that, C2<T>* __restrict__ w, int axis, int nx, int ny,
                                     int nz, T ilx, T ily, T ilz) {
  const int env = blockIdx.y;
  const int64_t cells = (int64_t)nx * ny * nz, o = (int64_t)env * cells;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += (int64_t)gridDim.x * blockDim.x) {
    T k[3];
    wave3<T>(i, nx, ny, nz, ilx, ily, ilz, k);
    const C2<T> t = that[o + i];
    w[o + i] = C2<T>{-k[axis] * t.im, k[axis] * t.re};
  }
}

// w *= D(u) / N
template <typename T>
__global__ void fourier3_mob_kernel(const T* __restrict__ u, C2<T>* __restrict__ w, const EnvParams<T>* __restrict__ ep,
                                    ClosureSpec mob, int64_t cells, T inv_n) {
  const int env = blockIdx.y;
  const EnvParams<T>& p = ep[env];
  const int64_t o = (int64_t)env * cells;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += (int64_t)gridDim.x * blockDim.x) {
    const T d = closure_generic<T>(mob, p.mob, u[o + i]) * inv_n;
    const C2<T> v = w[o + i];
    w[o + i] = C2<T>{v.re * d, v.im * d};
  }
}

// acc (+)= i k_axis w
template <typename T>
__global__ void fourier3_div_kernel(C2<T>* __restrict__ acc, const C2<T>* __restrict__ w, int axis, int first, int nx,
                                    int ny, int nz, T ilx, T ily, T ilz) {
  const int env = blockIdx.y;
  const int64_t cells = (int64_t)nx * ny * nz, o = (int64_t)env * cells;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += (int64_t)gridDim.x * blockDim.x) {
    T k[3];
    wave3<T>(i, nx, ny, nz, ilx, ily, ilz, k);
    const C2<T> v = w[o + i];
    C2<T> r{-k[axis] * v.im, k[axis] * v.re};
    if (!first) {
      const C2<T> old = acc[o + i];
      r.re += old.re;
      r.im += old.im;
    }
    acc[o + i] = r;
  }
}

template <typename T>
int rhs_fourier3_t(pdeopt_ctx* ctx, const void* in, void* out) {
  Spectral& sp = *ctx->features.get<Spectral>(FS_SPECTRAL);
  const pdeopt_problem& p = ctx->prob;
  const int64_t cells = (int64_t)p.nx * p.ny * p.nz, total = cells * p.batch;
  int rc;
  if ((rc = ensure_buffer(ctx, sp.cbuf, (size_t)total * 2 * sizeof(T)))) return rc;
  if ((rc = ensure_buffer(ctx, sp.cbuf2, (size_t)total * 2 * sizeof(T)))) return rc;
  if ((rc = ensure_buffer(ctx, sp.cbuf3, (size_t)total * 2 * sizeof(T)))) return rc;
  C2<T>* a = sp.cbuf2.as<C2<T>>();   // F[u], later the accumulated divergence
  C2<T>* b = sp.cbuf3.as<C2<T>>();   // F[mu_h(u)], then t_hat
  C2<T>* w = sp.cbuf.as<C2<T>>();    // one axis at a time
  const T* u = (const T*)in;
  const auto* ep = ctx->env_params_dev.as<const EnvParams<T>>();
  const ClosureSpec mu{p.mu.kind, p.mu.flags, p.mu.n}, mob{p.mob.kind, p.mob.flags, p.mob.n};
  const dim3 grid(grid_for(cells), p.batch), blk(256);
  const T ilx = T(1.0 / (p.nx * p.hx)), ily = T(1.0 / (p.ny * p.hy)), ilz = T(1.0 / (p.nz * p.hz));
  const T inv_n = T(1.0 / (double)cells);
  hipLaunchKernelGGL(fourier_embed_kernel<T>, grid, blk, 0, ctx->stream, u, a, b, ep, mu, cells);
  if ((rc = fft_exec(ctx, true, a))) return rc;
  if ((rc = fft_exec(ctx, true, b))) return rc;
  hipLaunchKernelGGL(fourier3_that_kernel<T>, grid, blk, 0, ctx->stream, (const C2<T>*)a, b, ep, p.nx, p.ny, p.nz, ilx, ily, ilz);
  for (int axis = 0; axis < 3; ++axis) {
    hipLaunchKernelGGL(fourier3_grad_kernel<T>, grid, blk, 0, ctx->stream, (const C2<T>*)b, w, axis, p.nx, p.ny, p.nz, ilx, ily, ilz);
    if ((rc = fft_exec(ctx, false, w))) return rc;
    hipLaunchKernelGGL(fourier3_mob_kernel<T>, grid, blk, 0, ctx->stream, u, w, ep, mob, cells, inv_n);
    if ((rc = fft_exec(ctx, true, w))) return rc;
    hipLaunchKernelGGL(fourier3_div_kernel<T>, grid, blk, 0, ctx->stream, a, (const C2<T>*)w, axis, axis == 0 ? 1 : 0, p.nx,
                       p.ny, p.nz, ilx, ily, ilz);
  }
  if ((rc = fft_exec(ctx, false, a))) return rc;
  hipLaunchKernelGGL((fourier_out_kernel<T, true>), grid, blk, 0, ctx->stream, u, (const C2<T>*)a, (T*)out, ep, mob, cells, inv_n);
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  ctx->last_kernel = "rhs_fourier<CH-3D>(rocfft x9)";
  return PDEOPT_OK;
}

}  // namespace

int rhs_fourier(pdeopt_ctx* ctx, const void* in, void* out) {
  if (ctx->halo) return fail(ctx, PDEOPT_EINVAL, "the pseudo-spectral RHS needs the periodic layout");
  int rc = ensure_plans(ctx);
  if (rc) return rc;
  return with_dtype(ctx, [&](auto t) {
    using T = decltype(t);
    return ctx->prob.equation == PDEOPT_EQ_CAHN_HILLIARD_3D ? rhs_fourier3_t<T>(ctx, in, out) : rhs_fourier_t<T>(ctx, in, out);
  });
}

int advance_imex(pdeopt_ctx* ctx, double, double dt, int64_t n) {
  if (!ctx->aux[PDEOPT_AUX_IMEX_SYMBOL].dev)
    return fail(ctx, PDEOPT_ESTATE, "IMEX needs the IMEX_SYMBOL aux field (fourier_symbol)");
  if (imex_fused_supported(ctx)) return advance_imex_fused(ctx, dt, n);  // FFTs in LDS, 4 kernels per substep
  if (ctx->imex_per_env)
    return fail(ctx, PDEOPT_EINVAL, "per-environment IMEX scales need the hand-written FFT passes (power-of-two grids 64..1024)");
  int rc = ensure_plans(ctx);
  if (rc) return rc;
  return with_dtype(ctx, [&](auto t) { return imex_t<decltype(t)>(ctx, dt, n); });
}

int imex_rocfft_prepare(pdeopt_ctx* ctx, double dt) {
  return with_dtype(ctx, [&](auto t) { return imex_rocfft_prepare_t<decltype(t)>(ctx, dt); });
}

int imex_rocfft_solve(pdeopt_ctx* ctx, double dt) {
  return with_dtype(ctx, [&](auto t) { return imex_rocfft_solve_t<decltype(t)>(ctx, dt); });
}

int imex_rocfft_prepare_kappa(pdeopt_ctx* ctx, double dt, double kappa) {
  return with_dtype(ctx, [&](auto t) { return imex_rocfft_prepare_kappa_t<decltype(t)>(ctx, dt, kappa); });
}

int imex_rocfft_solve_kappa(pdeopt_ctx* ctx, double dt, int B, int P, const int* role) {
  return with_dtype(ctx, [&](auto t) { return imex_rocfft_solve_kappa_t<decltype(t)>(ctx, dt, B, P, role); });
}

int imex_rocfft_apply(pdeopt_ctx* ctx) {
  return with_dtype(ctx, [&](auto t) { return imex_rocfft_apply_t<decltype(t)>(ctx); });
}

int axpy_state(pdeopt_ctx* ctx, double dt) {
  return with_dtype(ctx, [&](auto t) { return axpy_state_t<decltype(t)>(ctx, dt); });
}

int spectral_c2c(pdeopt_ctx* ctx, bool forward, void* buf) {
  const int rc = ensure_plans(ctx);
  return rc ? rc : fft_exec(ctx, forward, buf);
}

int spectral_real_prepare(pdeopt_ctx* ctx, void** half, int64_t* half_cells) {
  Spectral& sp = ctx->features.ensure<Spectral>(FS_SPECTRAL);
  std::call_once(g_rocfft_once, [] { rocfft_setup(); });
  int rc = ensure_real_plans(ctx);
  if (rc) return rc;
  if ((rc = ensure_buffer(ctx, sp.hbuf, (size_t)sp.half_cells * ctx->prob.batch * 2 * ctx->esize))) return rc;
  *half = sp.hbuf.get();
  *half_cells = sp.half_cells;
  return PDEOPT_OK;
}

int spectral_real_exec(pdeopt_ctx* ctx, bool forward, void* in, void* out) { return real_fft_exec(ctx, forward, in, out); }

int spectral_r2c_state(pdeopt_ctx* ctx, void** half, int64_t* half_cells) {
  const int rc = spectral_real_prepare(ctx, half, half_cells);
  return rc ? rc : real_fft_exec(ctx, true, ctx->Y.get(), *half);
}

int spectral_c2c_axis(pdeopt_ctx* ctx, int axis, bool forward, void* buf) {
  int rc = ensure_axis_plans(ctx);
  if (rc) return rc;
  Spectral& sp = *ctx->features.get<Spectral>(FS_SPECTRAL);
  const pdeopt_problem& p = ctx->prob;
  rocfft_plan plan = forward ? sp.ax_fwd[axis] : sp.ax_inv[axis];
  const size_t env_bytes = (size_t)p.nx * p.ny * 2 * ctx->esize;
  for (int b = 0; b < (axis == 0 ? p.batch : 1); ++b) {
    void* in[1] = {static_cast<char*>(buf) + (size_t)b * env_bytes};
    PDEOPT_FFT_CHECK(ctx, rocfft_execute(plan, in, nullptr, sp.ax_info));
  }
  return PDEOPT_OK;
}

int spectral_fetch_complex_aux(pdeopt_ctx* ctx, int which, std::vector<std::complex<double>>& out) {
  return fetch_complex_aux(ctx, which, out);
}

int advance_strang(pdeopt_ctx* ctx, double t0, double dt, int64_t n) {
  if (!ctx->aux[PDEOPT_AUX_GPE_A_TERM].dev)
    return fail(ctx, PDEOPT_ESTATE, "Strang splitting needs the GPE_A_TERM aux field");
  if (strang_fused_supported(ctx)) return advance_strang_fused(ctx, t0, dt, n);  // LDS FFTs, fused passes
  int rc = ensure_plans(ctx);
  if (rc) return rc;
  return with_dtype(ctx, [&](auto t) { return strang_t<decltype(t)>(ctx, t0, dt, n); });
}

}  // namespace pdeopt
