// Shell sums of the power spectrum of the resident real state (pdeopt_structure_factor): with
// u^ = rfftn(u), unnormalised, the last axis halved (m = 0 .. nh - 1, nh = n_last / 2 + 1),
//   P_b = sum over the modes of shell b of w |u^|^2,   b = (int)floor(sqrt(q) + 0.5),
//   q = t_0[i] + t_1[m] (2-D),  (t_0[i] + t_1[j]) + t_2[m] (3-D)   -- fp64 additions in that order, a correctly rounded root,
// t_a the fp64 axis tables of pdeopt_sk_configure ((2 pi fftfreq / dk)^2, built on the host), w the hermitian weight: 1 on
// the columns m = 0 and, for an even last axis, m = n_last / 2, else 2; 0 for the zero mode.  The host and the device form
// b from the same table entries by the same three IEEE operations, so they agree on every mode's shell bit for bit.
//
//   transform : one real-to-hermitian rocFFT transform of the state into the hermitian work field (spectral_r2c_state)
//   sk_bin    : a "row" is a fixed i (2-D) or (i, j) (3-D).  A workgroup of four waves takes 32 consecutive rows of an
//               environment, wave w the rows w, w + 4, ..; it walks a row in chunks of 64 modes, a mode per lane.  Along a
//               row t_last[m] does not decrease, so the shells of a chunk are sorted across the lanes: a segmented
//               inclusive scan by __shfl_up (a lane adds its lower neighbour's running sum where both have the same
//               shell) leaves each shell's sum of the chunk in the last lane of its segment, and that lane adds it to the
//               wave's own array of n_bins doubles in LDS -- the tails of a chunk have distinct shells, so no two lanes
//               of the instruction meet, and nothing is atomic.  After a barrier the four arrays are added in wave order
//               into the slot [env][row_block][n_bins], which only this workgroup writes.
//   sk_finish : a lane per shell; wave w of four adds its quarter of the environment's row blocks in block order, the
//               four sums meet in LDS in wave order.
// |u^|^2 is formed in fp64 from the converted components whatever the state's dtype.  No atomics, nothing waits between
// workgroups: a repeat gives identical bits, and an environment's row does not depend on which range was asked for.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.hpp"
#include "launch_util.hpp"

namespace pdeopt {

namespace {

constexpr int kRows = 32;        // rows of a workgroup of sk_bin_kernel
constexpr int kMaxBins = 4096;   // 4 arrays of n_bins doubles: 128 KiB of the CU's 160 KiB of LDS
constexpr int64_t kAblateBinning = 0x10000;  // PDEOPT_OPT_DEBUG_ABLATE, timing only: the transform, the copy and the synchronise alone

template <typename T>
struct C2 {
  T re, im;
};

template <typename T>
struct SkArgs {
  const C2<T>* c;    // the half spectra of the range's first environment: [env][rows][nh]
  const double* ta;  // 2-D: t_0[rows].  3-D: t_0[n_0]
  const double* tb;  // 3-D: t_1[n_1]
  const double* tl;  // the halved axis: t_last[0 .. nh)
  int rows, n1;      // n1: rows per i in 3-D, 0 in 2-D
  int nh, n_last, n_bins;
  int64_t estride;   // rows * nh
  double* partial;   // [env][row_block][n_bins]
};

// grid (row blocks, environments), 256 threads, 4 * n_bins doubles of dynamic LDS
template <typename T>
__global__ __launch_bounds__(256) void sk_bin_kernel(const SkArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  double* const bins = reinterpret_cast<double*>(smem_raw);  // [4][n_bins]
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int nb = a.n_bins, nh = a.nh;
  for (int q = tid; q < 4 * nb; q += 256) bins[q] = 0.0;
  __syncthreads();
  double* const mine = bins + wave * nb;
  const int r0 = blockIdx.x * kRows;
  const C2<T>* __restrict__ c = a.c + (int64_t)blockIdx.y * a.estride;
  for (int rr = wave; rr < kRows && r0 + rr < a.rows; rr += 4) {  // (wave-uniform)
    const int r = r0 + rr;
    double qrow;
    if (a.n1) {
      const int i = r / a.n1;
      qrow = a.ta[i] + a.tb[r - i * a.n1];
    } else {
      qrow = a.ta[r];
    }
    const C2<T>* __restrict__ row = c + (int64_t)r * nh;
    for (int m0 = 0; m0 < nh; m0 += 64) {
      const int m = m0 + lane;
      int b = 0x7fffffff;  // lanes past the row's end: a shell of their own behind every other, nothing to add
      double v = 0.0;
      if (m < nh) {
        b = (int)floor(__dsqrt_rn(qrow + a.tl[m]) + 0.5);
        const C2<T> z = row[m];
        const double re = (double)z.re, im = (double)z.im;
        const double p = re * re + im * im;
        v = (m == 0 || 2 * m == a.n_last) ? ((r | m) == 0 ? 0.0 : p) : 2.0 * p;
      }
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const double vu = __shfl_up(v, o, 64);
        const int bu = __shfl_up(b, o, 64);
        if (lane >= o && bu == b) v += vu;
      }
      const int bn = __shfl_down(b, 1, 64);
      if ((lane == 63 || bn != b) && b < nb) mine[b] += v;
    }
  }
  __syncthreads();
  double* __restrict__ dst = a.partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * nb;
  for (int q = tid; q < nb; q += 256) dst[q] = ((bins[q] + bins[nb + q]) + bins[2 * nb + q]) + bins[3 * nb + q];
}

// grid (ceil(n_bins / 64), environments), 256 threads: lane l of every wave takes shell 64 blockIdx.x + l
__global__ __launch_bounds__(256) void sk_finish_kernel(const double* __restrict__ partial, int blocks, int n_bins,
                                                        double* __restrict__ out) {
  __shared__ double red[4][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x * 64 + lane, env = blockIdx.y;
  const int per = (blocks + 3) / 4, k0 = wave * per, k1 = min(blocks, k0 + per);
  double s = 0.0;
  if (b < n_bins) {
    const double* __restrict__ p = partial + (int64_t)env * blocks * n_bins + b;
#pragma unroll 8
    for (int k = k0; k < k1; ++k) s += p[(int64_t)k * n_bins];
  }
  red[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && b < n_bins) out[(int64_t)env * n_bins + b] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

struct SkGrid {
  int dims, n[3];
  int rows, nh;
};

// the transformed grid as the real plans of spectral.hip see it; false where the halved axis would not be the last one
bool sk_grid(const pdeopt_problem& p, SkGrid* g) {
  const bool is3d = p.equation == PDEOPT_EQ_CAHN_HILLIARD_3D;
  g->dims = is3d ? 3 : 2;
  g->n[0] = p.nx;
  g->n[1] = p.ny;
  g->n[2] = is3d ? p.nz : 1;
  for (int a = 0; a < g->dims; ++a)
    if (g->n[a] < 2) return false;
  g->rows = is3d ? p.nx * p.ny : p.nx;
  g->nh = g->n[g->dims - 1] / 2 + 1;
  return true;
}

int refuse_layout(pdeopt_ctx* ctx, SkGrid* g) {
  const pdeopt_problem& p = ctx->prob;
  if (ctx->comps != 1)
    return fail(ctx, PDEOPT_EINVAL, "the structure factor is that of a real scalar state; the GPE's state is complex");
  if (ctx->halo) return fail(ctx, PDEOPT_EINVAL, "the structure factor is not available in the padded (domain-decomposition) layout");
  if (!sk_grid(p, g))
    return fail(ctx, PDEOPT_EINVAL, "the structure factor needs at least 2 points along every axis (nx=%d ny=%d nz=%d)", p.nx, p.ny, p.nz);
  return PDEOPT_OK;
}

template <typename T>
int structure_factor_t(pdeopt_ctx* ctx, const SkGrid& g, int env_first, int env_count, double* host_out) {
  const int nb = ctx->sk_bins;
  const int blocks = (g.rows + kRows - 1) / kRows;
  if (env_count > 65535) return fail(ctx, PDEOPT_EINVAL, "structure_factor: %d environments in one call (at most 65535)", env_count);
  void* half = nullptr;
  int64_t hc = 0;
  int rc = spectral_r2c_state(ctx, &half, &hc);  // the plans cover the batch: all of it is transformed
  if (rc) return rc;
  if (hc != (int64_t)g.rows * g.nh)
    return fail(ctx, PDEOPT_ESTATE, "structure_factor: the transform's half spectrum has %lld cells, expected %lld", (long long)hc,
                (long long)g.rows * g.nh);
  const size_t n_out = (size_t)nb * env_count, need = sizeof(double) * n_out * (size_t)(1 + blocks);
  if ((rc = grow_device_buffer(ctx, ctx->sk_dev, need, /*sync_first=*/true))) return rc;
  SkArgs<T> a{};
  a.c = static_cast<const C2<T>*>(half) + (int64_t)env_first * hc;
  a.ta = ctx->sk_tab_dev.as<double>();
  a.tb = g.dims == 3 ? ctx->sk_tab_dev.as<double>() + g.n[0] : nullptr;
  a.tl = ctx->sk_tab_dev.as<double>() + (g.dims == 3 ? g.n[0] + g.n[1] : g.n[0]);
  a.rows = g.rows;
  a.n1 = g.dims == 3 ? g.n[1] : 0;
  a.nh = g.nh;
  a.n_last = g.n[g.dims - 1];
  a.n_bins = nb;
  a.estride = hc;
  a.partial = ctx->sk_dev.as<double>() + n_out;
  const size_t lds = sizeof(double) * 4 * (size_t)nb;
  if (lds > 32768)
    PDEOPT_HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(sk_bin_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  if (!(ctx->opt_debug_ablate & kAblateBinning)) {
    hipLaunchKernelGGL(sk_bin_kernel<T>, dim3(blocks, env_count), dim3(256), lds, ctx->stream, a);
    hipLaunchKernelGGL(sk_finish_kernel, dim3((nb + 63) / 64, env_count), dim3(256), 0, ctx->stream, (const double*)a.partial, blocks, nb,
                       ctx->sk_dev.as<double>());
  }
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(host_out, ctx->sk_dev.as<double>(), sizeof(double) * n_out, hipMemcpyDeviceToHost, ctx->stream));
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->last_kernel = std::string("structure_factor<") + (g.dims == 3 ? "3-D," : "2-D,") + dtype_name<T>() + ">";
  return PDEOPT_OK;
}

}  // namespace

void sk_drop(pdeopt_ctx* ctx) {
  ctx->sk_tab_dev.reset();
  ctx->sk_bins = 0;
}

int sk_configure(pdeopt_ctx* ctx, const double* t0, const double* t1, const double* t2, int n_bins) {
  SkGrid g;
  int rc = refuse_layout(ctx, &g);
  if (rc) return rc;
  if ((g.dims == 3) != (t2 != nullptr))
    return fail(ctx, PDEOPT_EINVAL, "sk_configure: %s", g.dims == 3 ? "a 3-D grid needs the table t2" : "a 2-D grid takes no table t2 (pass NULL)");
  const double* const t[3] = {t0, t1, t2};
  std::vector<double> tab;
  double qmax = 0.0;
  for (int a = 0; a < g.dims; ++a) {
    double tmax = 0.0;
    for (int i = 0; i < g.n[a]; ++i) {
      if (!(t[a][i] >= 0.0) || !std::isfinite(t[a][i]))
        return fail(ctx, PDEOPT_EINVAL, "sk_configure: t%d[%d] = %g is not a finite number >= 0", a, i, t[a][i]);
      tmax = std::max(tmax, t[a][i]);
    }
    qmax = a == 0 ? tmax : qmax + tmax;
    tab.insert(tab.end(), t[a], t[a] + g.n[a]);
  }
  // the kernel's scan relies on shells that do not decrease along the halved axis
  for (int m = 1; m < g.nh; ++m)
    if (t[g.dims - 1][m] < t[g.dims - 1][m - 1])
      return fail(ctx, PDEOPT_EINVAL, "sk_configure: the last axis' table decreases at index %d of its half range [0, %d)", m, g.nh);
  const double implied = 1.0 + std::floor(std::sqrt(qmax) + 0.5);
  if ((double)n_bins != implied)
    return fail(ctx, PDEOPT_EINVAL, "sk_configure: n_bins = %d, but the tables imply 1 + floor(sqrt(sum of the axes' maxima) + 0.5) = %.0f", n_bins,
                implied);
  if (n_bins > kMaxBins)
    return fail(ctx, PDEOPT_EINVAL, "sk_configure: n_bins = %d exceeds %d: the four waves' shell arrays (4 x n_bins x 8 bytes) must fit in 128 KiB "
                "of the 160 KiB of LDS of a compute unit", n_bins, kMaxBins);
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  sk_drop(ctx);
  if (const int rc = ensure_buffer(ctx, ctx->sk_tab_dev, sizeof(double) * tab.size())) return rc;
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(ctx->sk_tab_dev.as<double>(), tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice, ctx->stream));
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->sk_bins = n_bins;
  return PDEOPT_OK;
}

int structure_factor(pdeopt_ctx* ctx, int env_first, int env_count, double* host_out) {
  SkGrid g;
  int rc = refuse_layout(ctx, &g);
  if (rc) return rc;
  if (!ctx->sk_bins)
    return fail(ctx, PDEOPT_ESTATE, "pdeopt_sk_configure has not been called for this grid (configuring another grid drops the tables)");
  if (!env_count) return PDEOPT_OK;
  return with_dtype(ctx, [&](auto tag) { return structure_factor_t<decltype(tag)>(ctx, g, env_first, env_count, host_out); });
}

}  // namespace pdeopt
