// An MLP-mixer evaluated and differentiated inside the library (the reference's pde_opt/numerics/functions/mixer_mlp.py
// as mu of Cahn-Hilliard; pde_opt_amd/numerics/functions/mixer.py is the torch module with the same parameters).
// For one field u (nx, ny), patch size p, C = hidden_size, P = (nx / p)(ny / p) patches, Q = p^2 pixels per patch:
//
//   y_0 = conv_in(u)                      (C, P)   a p x p convolution of stride p, patches row-major over the patch grid
//   y_a = y   + MLP_patch(LN_1(y))                 P -> mix_patch -> P on every channel row
//   y_b = y_a + MLP_hidden(LN_2(y_a^T))^T          C -> mix_hidden -> C on every patch row
//   mu  = conv_out(LN(y_last))            (nx, ny) a transposed p x p convolution of stride p
//
// LN is a layer norm over the whole (C, P) array of a field: one mean and one biased variance, eps = 1e-5, a weight and
// a bias per entry.  Every product is D[m][n] = sum_k A[m][k] W[k][n] on the 16 x 16 x 4 matrix instruction:
//   A  an activation, addressed by two strides (a transpose is a choice of strides; a field is read and written as
//      its (patch, pixel-of-patch) matrix), with the layer norm applied as it is loaded;
//   W  a weight, packed [K padded to 16][N padded to 16] with zeros in the padding, once for the forward product
//      (W^T of torch's (out, in)) and once for the backward-data product (W itself);
//   the epilogue adds the bias, applies the activation (keeping z for the backward pass), multiplies by act'(z), adds
//      the residual, or adds into a field.
// Activations live unpadded in the handle's workspace and every load and store is bounds-checked against the real
// sizes, so no sum ever sees padding.  Weight gradients dW[o][i] = sum_{b, k} delta[k][o] x[k][i] are the same instruction
// with both operands activations; a column of ones appended to x gives the bias gradient.  The four waves of a workgroup
// split k, move their fp32 / fp64 accumulators into fp64 sums every 64 instructions, and are added in wave order into
// the fp64 gradient buffer, which lives on the device across the substeps of a sweep.  Layer-norm statistics and the two
// sums of its backward pass are fp64 tree sums of fixed shape.  Nothing is atomic: a repeat gives identical bits.
//
// Launches: 6 per block + 3 forward (conv_in; per block statistics, two products, statistics, two products; the final
// statistics and conv_out); 18 per block + 9 for the vector-Jacobian product (the forward pass without conv_out, then
// per product one weight gradient and one backward-data product, per layer norm two kernels, and the output bias).
//
// Flat parameter order (torch's parameters() of the mirror): conv_in.weight (C, 1, p, p), conv_in.bias (C),
// conv_out.weight (C, 1, p, p), conv_out.bias (1), per block patch_mixer W1 (Mp, P), b1, W2 (P, Mp), b2, hidden_mixer
// W3 (Mh, C), b3, W4 (C, Mh), b4, norm1 weight and bias (C, P), norm2 weight and bias (P, C); the final norm's (C, P).
#include <algorithm>

#include "common.hpp"
#include "nn_device.hpp"
#include "nn_host.hpp"

constexpr int kMixMaxBlocks = 8;

struct pdeopt_mixer : pdeopt::NativeNet {
  int nx = 0, ny = 0, ps = 0, C = 0, Mp = 0, Mh = 0, K = 0, act = 0;
  int pw = 0, P = 0, Q = 0;  // patches per row of the patch grid, patches, pixels per patch
  // offsets in the flat parameter vector
  int64_t win = 0, bin = 0, wout = 0, bout = 0, gf = 0, bef = 0;
  struct Block {
    int64_t w1, b1, w2, b2, w3, b3, w4, b4, g1, be1, g2, be2;
    int64_t f1, r1, f2, r2, f3, r3, f4, r4;  // packed weights: forward and backward-data (reverse) products
  } blk[kMixMaxBlocks] = {};
  int64_t f_in = 0, r_in = 0, f_out = 0, r_out = 0;
  int64_t packed_elems = 0;  // the packed block: the flat vector as it is, then the packed weights
  // workspace of the configured dtype and batch
  int s_batch = 0;
  pdeopt::DeviceBuffer Y[2 * kMixMaxBlocks + 1];
  pdeopt::DeviceBuffer H1[kMixMaxBlocks], Z1[kMixMaxBlocks], H2[kMixMaxBlocks], Z2[kMixMaxBlocks];
  pdeopt::DeviceBuffer DY, DN, DZ;
  pdeopt::DeviceBuffer stats;  // doubles [2 K + 1 norms][batch][mean, rstd], then [batch][2] sums of a layer norm's backward pass
};

namespace pdeopt {
namespace {

constexpr double kLnEps = 1e-5;

// An activation as a matrix (i0, i1) of n0 x n1 real entries per field: two strides, or the (patch, pixel-of-patch)
// view of a field [nx][ny]; gamma != nullptr: the layer norm of its field is applied to what is loaded
template <typename T>
struct Operand {
  const T* ptr;
  int64_t sb, s0, s1;
  int n0, n1;
  int patch, ps, pw, ld;
  const T* gamma;
  const T* beta;
  int64_t g0, g1;
  const double* stats;  // [batch][mean, rstd]
};

__device__ __forceinline__ int64_t patch_offset(int p, int q, int ps, int pw, int ld) {
  const int pi = p / pw, pj = p - pi * pw, qi = q / ps, qj = q - qi * ps;
  return (int64_t)(pi * ps + qi) * ld + pj * ps + qj;
}

template <typename T>
__device__ __forceinline__ T load_op(const Operand<T>& a, int b, int i0, int i1, T mean, T rstd) {
  if (i0 >= a.n0 || i1 >= a.n1) return T(0);
  const int64_t off = a.patch ? patch_offset(i0, i1, a.ps, a.pw, a.ld) : i0 * a.s0 + i1 * a.s1;
  T v = a.ptr[b * a.sb + off];
  if (a.gamma) {
    const int64_t g = i0 * a.g0 + i1 * a.g1;
    v = (v - mean) * rstd * a.gamma[g] + a.beta[g];
  }
  return v;
}

enum { EPI_ACT = 1, EPI_DACT = 2, EPI_RES = 4, EPI_ADD = 8 };

template <typename T>
struct GemmArgs {
  Operand<T> A;   // (m, k)
  const T* w;     // [Kp][Np]
  int Kp, Np, M, N;
  const T* bias;  // nullptr: none; entry n * bias_stride
  int bias_stride;
  int epi;
  T* out;         // entry (m, n) of field b at b ob + m o0 + n o1, or the patch view of a field
  T* zout;        // EPI_ACT: the pre-activation is kept here when not nullptr (addressed as out)
  const T* zaux;  // EPI_DACT: the pre-activation (addressed as out)
  const T* res;   // EPI_RES: the residual (addressed as out)
  int64_t ob, o0, o1;
  int out_patch, ps, pw, ld;
};

// grid (N tiles, M tiles / 4, batch): every wave one 16 x 16 tile of D = A W with its epilogue
template <typename T, int ACT>
__global__ __launch_bounds__(256) void mixer_gemm_kernel(GemmArgs<T> a) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lp = lane & 15, lk = lane >> 4;
  const int b = blockIdx.z;
  const int m0 = (blockIdx.y * 4 + wave) * 16, n0 = blockIdx.x * 16;
  if (m0 >= a.M) return;
  T mean = T(0), rstd = T(1);
  if (a.A.gamma) mean = (T)a.A.stats[2 * b], rstd = (T)a.A.stats[2 * b + 1];
  vec4<T> acc = vec4<T>{T(0), T(0), T(0), T(0)};
  const T* __restrict__ wp = a.w + (int64_t)lk * a.Np + n0 + lp;
  for (int k = 0; k < a.Kp; k += 16) {  // Kp is a multiple of 16: the loads of four instructions are issued together
    T av[4], bv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      av[j] = load_op<T>(a.A, b, m0 + lp, k + 4 * j + lk, mean, rstd);
      bv[j] = wp[(int64_t)(k + 4 * j) * a.Np];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = mfma16(av[j], bv[j], acc);
  }
  const int n = n0 + lp;
  if (n >= a.N) return;
  const T bias = a.bias ? a.bias[(int64_t)n * a.bias_stride] : T(0);
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int m = m0 + acc_row<T>(lk, reg);
    if (m >= a.M) continue;
    const int64_t o = b * a.ob + (a.out_patch ? patch_offset(m, n, a.ps, a.pw, a.ld) : m * a.o0 + n * a.o1);
    T v = acc[reg] + bias;
    if (a.epi & EPI_ACT) {
      if (a.zout) a.zout[o] = v;
      v = act_value<T, ACT>(v);
    }
    if (a.epi & EPI_DACT) v *= act_deriv<T, ACT>(a.zaux[o]);
    if (a.epi & EPI_RES) v = a.res[o] + v;
    if (a.epi & EPI_ADD) v = a.out[o] + v;
    a.out[o] = v;
  }
}

template <typename T>
struct WgradArgs {
  Operand<T> D;  // delta (k, o)
  Operand<T> X;  // x (k, i)
  int B, K, O, I, ones;  // ones: x has a column I of ones, whose product is the bias gradient
  double* gw;    // entry (o, i) at o gw_o + i
  int64_t gw_o;
  double* gb;    // [O]
};

// grid (tiles of I + ones, tiles of O): gw[o][i] += sum over the fields in order and over k of delta[k][o] x[k][i]
template <typename T>
__global__ __launch_bounds__(256) void mixer_wgrad_kernel(WgradArgs<T> a) {
  __shared__ double red[4 * 256];
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63, lp = lane & 15, lk = lane >> 4;
  const int o = blockIdx.y * 16 + lp, i = blockIdx.x * 16 + lp;
  const bool one = a.ones && i == a.I;
  const int steps = (a.K + 3) / 4;
  double sum[4] = {0.0, 0.0, 0.0, 0.0};
  for (int b = 0; b < a.B; ++b) {
    T dm = T(0), dr = T(1), xm = T(0), xr = T(1);
    if (a.D.gamma) dm = (T)a.D.stats[2 * b], dr = (T)a.D.stats[2 * b + 1];
    if (a.X.gamma) xm = (T)a.X.stats[2 * b], xr = (T)a.X.stats[2 * b + 1];
    vec4<T> acc = vec4<T>{T(0), T(0), T(0), T(0)};
    int held = 0;
    for (int s = wave; s < steps; s += 4) {
      const int k = s * 4 + lk;
      const T dv = load_op<T>(a.D, b, k, o, dm, dr);
      const T xv = one ? (k < a.K ? T(1) : T(0)) : load_op<T>(a.X, b, k, i, xm, xr);
      acc = mfma16(dv, xv, acc);
      if (++held == 64) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) sum[reg] += (double)acc[reg], acc[reg] = T(0);
        held = 0;
      }
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) sum[reg] += (double)acc[reg];
  }
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) red[wave * 256 + acc_row<T>(lk, reg) * 16 + lp] = sum[reg];
  __syncthreads();
  const double total = ((red[tid] + red[256 + tid]) + red[512 + tid]) + red[768 + tid];
  const int ro = blockIdx.y * 16 + (tid >> 4), ci = blockIdx.x * 16 + (tid & 15);
  if (ro >= a.O) return;
  if (ci < a.I) a.gw[ro * a.gw_o + ci] += total;
  else if (a.ones && ci == a.I) a.gb[ro] += total;
}

// the sum of v over the 256 threads of the workgroup, in a tree of fixed shape, returned to every thread
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  return red[0];
}

// grid (batch): mean and 1 / sqrt(biased variance + eps) of the n entries of every field, in fp64
template <typename T>
__global__ __launch_bounds__(256) void mixer_stats_kernel(const T* __restrict__ y, int64_t n, double* __restrict__ stats) {
  __shared__ double red[256];
  const int tid = threadIdx.x, b = blockIdx.x;
  const T* __restrict__ p = y + (int64_t)b * n;
  double s = 0.0;
  for (int64_t e = tid; e < n; e += 256) s += (double)p[e];
  const double mean = block_sum(s, red) / (double)n;
  double v = 0.0;
  for (int64_t e = tid; e < n; e += 256) {
    const double d = (double)p[e] - mean;
    v += d * d;
  }
  const double var = block_sum(v, red) / (double)n;
  if (tid == 0) stats[2 * b] = mean, stats[2 * b + 1] = 1.0 / sqrt(var + kLnEps);
}

template <typename T>
struct LnBwdArgs {
  const T* y;        // [batch][C][P], the layer norm's input
  const T* dn;       // [batch][C][P], the cotangent of its output
  T* dy;             // [batch][C][P]: the cotangent of its input is added (residual) or stored
  const T* gamma;    // entry (c, p) at c gc + p gp
  int64_t gc, gp;
  const double* stats;
  double* sums;      // [batch][sum dn gamma, sum dn gamma xhat]
  double* ggamma;    // the gradients of gamma and beta, addressed as gamma
  double* gbeta;
  int B, C, P, residual;
};

// grid (batch): the two sums of the layer norm's backward pass over the C P entries of every field, in fp64
template <typename T>
__global__ __launch_bounds__(256) void mixer_ln_bwd_sums_kernel(LnBwdArgs<T> a) {
  __shared__ double red[256];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int64_t n = (int64_t)a.C * a.P;
  const double mean = a.stats[2 * b], rstd = a.stats[2 * b + 1];
  double s1 = 0.0, s2 = 0.0;
  for (int64_t e = tid; e < n; e += 256) {
    const int c = (int)(e / a.P), p = (int)(e - (int64_t)c * a.P);
    const double dx = (double)a.dn[b * n + e] * (double)a.gamma[c * a.gc + p * a.gp];
    s1 += dx;
    s2 += dx * (((double)a.y[b * n + e] - mean) * rstd);
  }
  s1 = block_sum(s1, red);
  s2 = block_sum(s2, red);
  if (tid == 0) a.sums[2 * b] = s1, a.sums[2 * b + 1] = s2;
}

// one thread per entry (c, p): dy = rstd (dn gamma - mean(dn gamma) - xhat mean(dn gamma xhat)) of every field, and the
// gradients of gamma and beta summed over the fields in order
template <typename T>
__global__ __launch_bounds__(256) void mixer_ln_bwd_apply_kernel(LnBwdArgs<T> a) {
  const int64_t n = (int64_t)a.C * a.P;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const int c = (int)(e / a.P), p = (int)(e - (int64_t)c * a.P);
  const int64_t gi = c * a.gc + p * a.gp;
  const T g = a.gamma[gi];
  double gg = 0.0, gb = 0.0;
  for (int b = 0; b < a.B; ++b) {
    const T mean = (T)a.stats[2 * b], rstd = (T)a.stats[2 * b + 1];
    const T m1 = (T)(a.sums[2 * b] / (double)n), m2 = (T)(a.sums[2 * b + 1] / (double)n);
    const T xh = (a.y[b * n + e] - mean) * rstd;
    const T dn = a.dn[b * n + e];
    const T d = rstd * (dn * g - m1 - xh * m2);
    a.dy[b * n + e] = a.residual ? a.dy[b * n + e] + d : d;
    gg += (double)(dn * xh);
    gb += (double)dn;
  }
  a.ggamma[gi] += gg;
  a.gbeta[gi] += gb;
}

// one workgroup: out[0] += the sum of all n entries, in fp64 (the gradient of conv_out's bias)
template <typename T>
__global__ __launch_bounds__(256) void mixer_sum_kernel(const T* __restrict__ g, int64_t n, double* __restrict__ out) {
  __shared__ double red[256];
  double s = 0.0;
  for (int64_t e = threadIdx.x; e < n; e += 256) s += (double)g[e];
  s = block_sum(s, red);
  if (threadIdx.x == 0) out[0] += s;
}

// ---- host ---------------------------------------------------------------------------------------------------------------

// offsets of the flat vector and of the packed weights behind it
void lay_out(pdeopt_mixer* n) {
  const int64_t C = n->C, P = n->P, Q = n->Q, Mp = n->Mp, Mh = n->Mh;
  int64_t o = 0;
  const auto take = [&](int64_t count) {
    const int64_t at = o;
    o += count;
    return at;
  };
  n->win = take(C * Q), n->bin = take(C), n->wout = take(C * Q), n->bout = take(1);
  for (int k = 0; k < n->K; ++k) {
    pdeopt_mixer::Block& b = n->blk[k];
    b.w1 = take(Mp * P), b.b1 = take(Mp), b.w2 = take(P * Mp), b.b2 = take(P);
    b.w3 = take(Mh * C), b.b3 = take(Mh), b.w4 = take(C * Mh), b.b4 = take(C);
    b.g1 = take(C * P), b.be1 = take(C * P), b.g2 = take(P * C), b.be2 = take(P * C);
  }
  n->gf = take(C * P), n->bef = take(C * P);
  n->n_params = o;
  const int64_t Cp = pad16(n->C), Pp = pad16(n->P), Qp = pad16(n->Q), Mpp = pad16(n->Mp), Mhp = pad16(n->Mh);
  n->f_in = take(Qp * Cp), n->r_in = take(Cp * Qp), n->f_out = take(Cp * Qp), n->r_out = take(Qp * Cp);
  for (int k = 0; k < n->K; ++k) {
    pdeopt_mixer::Block& b = n->blk[k];
    b.f1 = take(Pp * Mpp), b.r1 = take(Mpp * Pp), b.f2 = take(Mpp * Pp), b.r2 = take(Pp * Mpp);
    b.f3 = take(Cp * Mhp), b.r3 = take(Mhp * Cp), b.f4 = take(Mhp * Cp), b.r4 = take(Cp * Mhp);
  }
  n->packed_elems = o;
}

// a weight of a map from I inputs to O outputs, stored (O, I) (or (I, O) when stored_io), into its two packed blocks:
// forward [pad16(I)][pad16(O)], backward-data [pad16(O)][pad16(I)]
template <typename T>
void pack_pair(std::vector<T>& h, const double* w, int O, int I, bool stored_io, int64_t fwd, int64_t rev) {
  const int Op = pad16(O), Ip = pad16(I);
  for (int o = 0; o < O; ++o)
    for (int i = 0; i < I; ++i) {
      const T v = (T)(stored_io ? w[(int64_t)i * O + o] : w[(int64_t)o * I + i]);
      h[fwd + (int64_t)i * Op + o] = v;
      h[rev + (int64_t)o * Ip + i] = v;
    }
}

template <typename T>
int upload_packed(pdeopt_mixer* n) {
  std::vector<T> h((size_t)n->packed_elems, T(0));
  for (int64_t q = 0; q < n->n_params; ++q) h[q] = (T)n->params[q];
  const double* p = n->params.data();
  pack_pair<T>(h, p + n->win, n->C, n->Q, false, n->f_in, n->r_in);
  pack_pair<T>(h, p + n->wout, n->Q, n->C, true, n->f_out, n->r_out);
  for (int k = 0; k < n->K; ++k) {
    const pdeopt_mixer::Block& b = n->blk[k];
    pack_pair<T>(h, p + b.w1, n->Mp, n->P, false, b.f1, b.r1);
    pack_pair<T>(h, p + b.w2, n->P, n->Mp, false, b.f2, b.r2);
    pack_pair<T>(h, p + b.w3, n->Mh, n->C, false, b.f3, b.r3);
    pack_pair<T>(h, p + b.w4, n->C, n->Mh, false, b.f4, b.r4);
  }
  return net_upload(n, h);
}

// the workspace of the batch in the handle's key: what a forward pass writes, and for the backward pass z and the cotangents
int size_workspace(pdeopt_mixer* n, bool backward) {
  pdeopt_ctx* ctx = n->ctx;
  const pdeopt_problem& p = ctx->prob;
  const size_t B = p.batch, cp = (size_t)n->C * n->P, cm = (size_t)n->C * n->Mp, pm = (size_t)n->P * n->Mh, es = ctx->esize;
  int rc = 0;
  for (int j = 0; j <= 2 * n->K; ++j)
    if ((rc = ensure_buffer(ctx, n->Y[j], B * cp * es))) return rc;
  for (int k = 0; k < n->K; ++k) {
    if ((rc = ensure_buffer(ctx, n->H1[k], B * cm * es)) || (rc = ensure_buffer(ctx, n->H2[k], B * pm * es))) return rc;
    if (backward && ((rc = ensure_buffer(ctx, n->Z1[k], B * cm * es)) || (rc = ensure_buffer(ctx, n->Z2[k], B * pm * es)))) return rc;
  }
  if ((rc = ensure_buffer(ctx, n->stats, (size_t)(2 * n->K + 2) * B * 2 * sizeof(double)))) return rc;
  if (backward) {
    if ((rc = ensure_buffer(ctx, n->DY, B * cp * es)) || (rc = ensure_buffer(ctx, n->DN, B * cp * es)) ||
        (rc = ensure_buffer(ctx, n->DZ, B * std::max(cm, pm) * es)))
      return rc;
  }
  return PDEOPT_OK;
}

template <typename T>
Operand<T> plain(const void* ptr, int64_t sb, int n0, int n1, int64_t s0, int64_t s1) {
  Operand<T> a{};
  a.ptr = static_cast<const T*>(ptr), a.sb = sb, a.n0 = n0, a.n1 = n1, a.s0 = s0, a.s1 = s1;
  return a;
}
// a field [nx][ny] as its (patch, pixel-of-patch) matrix
template <typename T>
Operand<T> patches(const pdeopt_mixer* n, const void* field) {
  Operand<T> a{};
  a.ptr = static_cast<const T*>(field), a.sb = (int64_t)n->nx * n->ny, a.n0 = n->P, a.n1 = n->Q;
  a.patch = 1, a.ps = n->ps, a.pw = n->pw, a.ld = n->ny;
  return a;
}
template <typename T>
Operand<T> normed(Operand<T> a, const pdeopt_mixer* n, int64_t gamma, int64_t beta, int64_t g0, int64_t g1, int which) {
  const T* P = n->packed.as<const T>();
  a.gamma = P + gamma, a.beta = P + beta, a.g0 = g0, a.g1 = g1;
  a.stats = n->stats.as<double>() + (size_t)which * n->s_batch * 2;
  return a;
}

template <typename T, int ACT>
void launch_gemm_act(pdeopt_ctx* ctx, const GemmArgs<T>& a) {
  const dim3 grid((a.N + 15) / 16, ((a.M + 15) / 16 + 3) / 4, ctx->prob.batch);
  hipLaunchKernelGGL((mixer_gemm_kernel<T, ACT>), grid, dim3(256), 0, ctx->stream, a);
}
template <typename T>
int launch_gemm(pdeopt_mixer* n, const GemmArgs<T>& a) {
  pdeopt_ctx* ctx = n->ctx;
  if (!(a.epi & (EPI_ACT | EPI_DACT))) launch_gemm_act<T, NN_ACT_NONE>(ctx, a);
  else if (n->act == PDEOPT_MIXER_RELU) launch_gemm_act<T, NN_ACT_RELU>(ctx, a);
  else if (n->act == PDEOPT_MIXER_GELU) launch_gemm_act<T, NN_ACT_GELU>(ctx, a);
  else if (n->act == PDEOPT_MIXER_GELU_TANH) launch_gemm_act<T, NN_ACT_GELU_TANH>(ctx, a);
  else launch_gemm_act<T, NN_ACT_TANH>(ctx, a);
  ctx->n_stage_launches++;
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  return PDEOPT_OK;
}
// D = A W (+ bias) into out (m, n) at b ob + m o0 + n o1
template <typename T>
GemmArgs<T> gemm(const pdeopt_mixer* n, const Operand<T>& A, int64_t w, int N, void* out, int64_t ob, int64_t o0, int64_t o1) {
  GemmArgs<T> a{};
  a.A = A, a.w = n->packed.as<const T>() + w, a.Kp = pad16(A.n1), a.Np = pad16(N), a.M = A.n0, a.N = N;
  a.out = static_cast<T*>(out), a.ob = ob, a.o0 = o0, a.o1 = o1;
  return a;
}
template <typename T>
void with_bias(GemmArgs<T>& a, const pdeopt_mixer* n, int64_t bias, int stride = 1) {
  a.bias = n->packed.as<const T>() + bias, a.bias_stride = stride;
}
template <typename T>
void into_field(GemmArgs<T>& a, const pdeopt_mixer* n) {
  a.ob = (int64_t)n->nx * n->ny, a.out_patch = 1, a.ps = n->ps, a.pw = n->pw, a.ld = n->ny;
}

template <typename T>
int launch_stats(pdeopt_mixer* n, int which) {
  pdeopt_ctx* ctx = n->ctx;
  hipLaunchKernelGGL(mixer_stats_kernel<T>, dim3(ctx->prob.batch), dim3(256), 0, ctx->stream, n->Y[which].as<const T>(),
                     (int64_t)n->C * n->P, n->stats.as<double>() + (size_t)which * n->s_batch * 2);
  ctx->n_stage_launches++;
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  return PDEOPT_OK;
}

// mu = N(u), or everything below conv_out when mu == nullptr; keep_z: the pre-activations stay for the backward pass
template <typename T>
int forward(pdeopt_mixer* n, const void* u, void* mu, bool keep_z) {
  const int C = n->C, P = n->P, Mp = n->Mp, Mh = n->Mh;
  const int64_t cp = (int64_t)C * P, cm = (int64_t)C * Mp, pm = (int64_t)P * Mh;
  int rc = 0;
  {
    GemmArgs<T> a = gemm<T>(n, patches<T>(n, u), n->f_in, C, n->Y[0].get(), cp, 1, P);
    with_bias(a, n, n->bin);
    if ((rc = launch_gemm(n, a))) return rc;
  }
  for (int k = 0; k < n->K; ++k) {
    const pdeopt_mixer::Block& b = n->blk[k];
    void *y = n->Y[2 * k].get(), *ya = n->Y[2 * k + 1].get(), *yb = n->Y[2 * k + 2].get();
    if ((rc = launch_stats<T>(n, 2 * k))) return rc;
    GemmArgs<T> g1 = gemm<T>(n, normed(plain<T>(y, cp, C, P, P, 1), n, b.g1, b.be1, P, 1, 2 * k), b.f1, Mp, n->H1[k].get(), cm, Mp, 1);
    with_bias(g1, n, b.b1);
    g1.epi = EPI_ACT, g1.zout = keep_z ? n->Z1[k].as<T>() : nullptr;
    if ((rc = launch_gemm(n, g1))) return rc;
    GemmArgs<T> g2 = gemm<T>(n, plain<T>(n->H1[k].get(), cm, C, Mp, Mp, 1), b.f2, P, ya, cp, P, 1);
    with_bias(g2, n, b.b2);
    g2.epi = EPI_RES, g2.res = static_cast<const T*>(y);
    if ((rc = launch_gemm(n, g2))) return rc;
    if ((rc = launch_stats<T>(n, 2 * k + 1))) return rc;
    GemmArgs<T> g3 = gemm<T>(n, normed(plain<T>(ya, cp, P, C, 1, P), n, b.g2, b.be2, C, 1, 2 * k + 1), b.f3, Mh, n->H2[k].get(), pm, Mh, 1);
    with_bias(g3, n, b.b3);
    g3.epi = EPI_ACT, g3.zout = keep_z ? n->Z2[k].as<T>() : nullptr;
    if ((rc = launch_gemm(n, g3))) return rc;
    GemmArgs<T> g4 = gemm<T>(n, plain<T>(n->H2[k].get(), pm, P, Mh, Mh, 1), b.f4, C, yb, cp, 1, P);
    with_bias(g4, n, b.b4);
    g4.epi = EPI_RES, g4.res = static_cast<const T*>(ya);
    if ((rc = launch_gemm(n, g4))) return rc;
  }
  if ((rc = launch_stats<T>(n, 2 * n->K))) return rc;
  if (mu) {
    GemmArgs<T> a = gemm<T>(n, normed(plain<T>(n->Y[2 * n->K].get(), cp, P, C, 1, P), n, n->gf, n->bef, 1, P, 2 * n->K), n->f_out, n->Q, mu, 0, 0, 0);
    with_bias(a, n, n->bout, 0);
    into_field(a, n);
    if ((rc = launch_gemm(n, a))) return rc;
  }
  return PDEOPT_OK;
}

// gw (o, i) at o gw_o + i += sum delta[k][o] x[k][i]; bias >= 0: its gradient from a column of ones
template <typename T>
int launch_wgrad(pdeopt_mixer* n, const Operand<T>& D, const Operand<T>& X, int64_t weight, int64_t bias) {
  pdeopt_ctx* ctx = n->ctx;
  WgradArgs<T> a{};
  a.D = D, a.X = X, a.B = ctx->prob.batch, a.K = D.n0, a.O = D.n1, a.I = X.n1, a.ones = bias >= 0;
  a.gw = n->grad.as<double>() + weight, a.gw_o = X.n1, a.gb = bias >= 0 ? n->grad.as<double>() + bias : nullptr;
  hipLaunchKernelGGL(mixer_wgrad_kernel<T>, dim3((a.I + a.ones + 15) / 16, (a.O + 15) / 16), dim3(256), 0, ctx->stream, a);
  ctx->n_stage_launches++;
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  return PDEOPT_OK;
}

// the layer norm `which` backwards: DN is the cotangent of its output, DY receives (residual: is added) that of its input
template <typename T>
int launch_ln_bwd(pdeopt_mixer* n, int which, int64_t gamma, int64_t beta, int64_t gc, int64_t gp, bool residual) {
  pdeopt_ctx* ctx = n->ctx;
  LnBwdArgs<T> a{};
  a.y = n->Y[which].as<const T>(), a.dn = n->DN.as<const T>(), a.dy = n->DY.as<T>();
  a.gamma = n->packed.as<const T>() + gamma, a.gc = gc, a.gp = gp;
  a.stats = n->stats.as<double>() + (size_t)which * n->s_batch * 2;
  a.sums = n->stats.as<double>() + (size_t)(2 * n->K + 1) * n->s_batch * 2;
  a.ggamma = n->grad.as<double>() + gamma, a.gbeta = n->grad.as<double>() + beta;
  a.B = ctx->prob.batch, a.C = n->C, a.P = n->P, a.residual = residual;
  const int64_t cp = (int64_t)n->C * n->P;
  hipLaunchKernelGGL(mixer_ln_bwd_sums_kernel<T>, dim3(a.B), dim3(256), 0, ctx->stream, a);
  hipLaunchKernelGGL(mixer_ln_bwd_apply_kernel<T>, dim3((unsigned)((cp + 255) / 256)), dim3(256), 0, ctx->stream, a);
  ctx->n_stage_launches += 2;
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  return PDEOPT_OK;
}

template <typename T>
int backward(pdeopt_mixer* n, const void* u, const void* gmu, void* lam) {
  pdeopt_ctx* ctx = n->ctx;
  const int C = n->C, P = n->P, Mp = n->Mp, Mh = n->Mh, Q = n->Q, last = 2 * n->K;
  const int64_t cp = (int64_t)C * P, cm = (int64_t)C * Mp, pm = (int64_t)P * Mh;
  int rc = 0;
  // conv_out and the final norm
  hipLaunchKernelGGL(mixer_sum_kernel<T>, dim3(1), dim3(256), 0, ctx->stream, static_cast<const T*>(gmu),
                     (int64_t)ctx->prob.batch * n->nx * n->ny, n->grad.as<double>() + n->bout);
  ctx->n_stage_launches++;
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  if ((rc = launch_wgrad<T>(n, normed(plain<T>(n->Y[last].get(), cp, P, C, 1, P), n, n->gf, n->bef, 1, P, last), patches<T>(n, gmu), n->wout, -1)))
    return rc;
  if ((rc = launch_gemm(n, gemm<T>(n, patches<T>(n, gmu), n->r_out, C, n->DN.get(), cp, 1, P)))) return rc;
  if ((rc = launch_ln_bwd<T>(n, last, n->gf, n->bef, P, 1, false))) return rc;
  for (int k = n->K - 1; k >= 0; --k) {
    const pdeopt_mixer::Block& b = n->blk[k];
    // the hidden mixer: DY is the cotangent of y_b, as (patch, channel) rows
    const Operand<T> dyt = plain<T>(n->DY.get(), cp, P, C, 1, P);
    if ((rc = launch_wgrad<T>(n, dyt, plain<T>(n->H2[k].get(), pm, P, Mh, Mh, 1), b.w4, b.b4))) return rc;
    GemmArgs<T> g4 = gemm<T>(n, dyt, b.r4, Mh, n->DZ.get(), pm, Mh, 1);
    g4.epi = EPI_DACT, g4.zaux = n->Z2[k].as<const T>();
    if ((rc = launch_gemm(n, g4))) return rc;
    const Operand<T> dz2 = plain<T>(n->DZ.get(), pm, P, Mh, Mh, 1);
    if ((rc = launch_wgrad<T>(n, dz2, normed(plain<T>(n->Y[2 * k + 1].get(), cp, P, C, 1, P), n, b.g2, b.be2, C, 1, 2 * k + 1), b.w3, b.b3)))
      return rc;
    if ((rc = launch_gemm(n, gemm<T>(n, dz2, b.r3, C, n->DN.get(), cp, 1, P)))) return rc;
    if ((rc = launch_ln_bwd<T>(n, 2 * k + 1, b.g2, b.be2, 1, C, true))) return rc;
    // the patch mixer: DY is the cotangent of y_a, as (channel, patch) rows
    const Operand<T> dy = plain<T>(n->DY.get(), cp, C, P, P, 1);
    if ((rc = launch_wgrad<T>(n, dy, plain<T>(n->H1[k].get(), cm, C, Mp, Mp, 1), b.w2, b.b2))) return rc;
    GemmArgs<T> g2 = gemm<T>(n, dy, b.r2, Mp, n->DZ.get(), cm, Mp, 1);
    g2.epi = EPI_DACT, g2.zaux = n->Z1[k].as<const T>();
    if ((rc = launch_gemm(n, g2))) return rc;
    const Operand<T> dz1 = plain<T>(n->DZ.get(), cm, C, Mp, Mp, 1);
    if ((rc = launch_wgrad<T>(n, dz1, normed(plain<T>(n->Y[2 * k].get(), cp, C, P, P, 1), n, b.g1, b.be1, P, 1, 2 * k), b.w1, b.b1))) return rc;
    if ((rc = launch_gemm(n, gemm<T>(n, dz1, b.r1, P, n->DN.get(), cp, P, 1)))) return rc;
    if ((rc = launch_ln_bwd<T>(n, 2 * k, b.g1, b.be1, P, 1, true))) return rc;
  }
  // conv_in: DY is the cotangent of y_0
  const Operand<T> dy0 = plain<T>(n->DY.get(), cp, P, C, 1, P);
  if ((rc = launch_wgrad<T>(n, dy0, patches<T>(n, u), n->win, n->bin))) return rc;
  GemmArgs<T> a = gemm<T>(n, dy0, n->r_in, Q, lam, 0, 0, 0);
  a.epi = EPI_ADD;
  into_field(a, n);
  return launch_gemm(n, a);
}

// the mixer as the shared steps of nn_host.hpp see it
struct MixerFamily {
  static constexpr const char *forward_kernels = "mixer_gemm+mixer_stats", *vjp_kernels = "mixer_gemm+mixer_wgrad";
  static int refuse(pdeopt_mixer* n, const pdeopt_problem& p) {
    if (p.nx == n->nx && p.ny == n->ny) return PDEOPT_OK;
    return fail(n->ctx, PDEOPT_EINVAL, "the mixer was created for a %d x %d grid, the problem is now %d x %d: its parameter shapes "
                "depend on the grid", n->nx, n->ny, p.nx, p.ny);
  }
  static bool keyed_for(const pdeopt_mixer* n, const pdeopt_problem& p) { return n->s_dtype == p.dtype && n->s_batch == p.batch; }
  static void rekey(pdeopt_mixer* n, const pdeopt_problem& p) {
    for (DeviceBuffer& y : n->Y) y.reset();
    for (int k = 0; k < kMixMaxBlocks; ++k) n->H1[k].reset(), n->Z1[k].reset(), n->H2[k].reset(), n->Z2[k].reset();
    n->DY.reset(), n->DN.reset(), n->DZ.reset();
    n->stats.reset();
    n->s_dtype = p.dtype, n->s_batch = p.batch;
  }
  static int size_workspace(pdeopt_mixer* n, bool backward) { return pdeopt::size_workspace(n, backward); }
  // in the problem dtype, t = T(): pack(t, n), forward(t, n, u, mu, keep_z), backward(t, n, u, gmu, lam)
  static constexpr auto pack = [](auto t, auto... a) { return upload_packed<decltype(t)>(a...); };
  static constexpr auto forward = [](auto t, auto... a) { return pdeopt::forward<decltype(t)>(a...); };
  static constexpr auto backward = [](auto t, auto... a) { return pdeopt::backward<decltype(t)>(a...); };
};

}  // namespace
}  // namespace pdeopt

using namespace pdeopt;

extern "C" {

int pdeopt_mixer_create(pdeopt_ctx* ctx, int patch, int hidden, int mix_patch, int mix_hidden, int blocks, int activation,
                        pdeopt_mixer** out) {
  if (!ctx || !out) return PDEOPT_EINVAL;
  *out = nullptr;
  if (!ctx->configured) return fail(ctx, PDEOPT_ESTATE, "pdeopt_configure has not been called: the mixer takes its grid from the problem");
  const pdeopt_problem& p = ctx->prob;
  if (p.nz > 1 || ctx->comps != 1 || ctx->halo)
    return fail(ctx, PDEOPT_EINVAL, "the mixer runs on periodic 2-D real fields [batch][nx][ny]");
  if (patch < 1 || patch > 16) return fail(ctx, PDEOPT_EINVAL, "patch size %d: supported are 1 to 16", patch);
  if (p.nx % patch || p.ny % patch)
    return fail(ctx, PDEOPT_EINVAL, "patch size %d does not divide the %d x %d grid", patch, p.nx, p.ny);
  if (hidden < 1 || hidden > 64) return fail(ctx, PDEOPT_EINVAL, "hidden size %d: supported are 1 to 64", hidden);
  if (mix_patch < 1 || mix_patch > 256 || mix_hidden < 1 || mix_hidden > 256)
    return fail(ctx, PDEOPT_EINVAL, "mix sizes %d and %d: supported are 1 to 256", mix_patch, mix_hidden);
  const int64_t patches = (int64_t)(p.nx / patch) * (p.ny / patch);
  if (patches < 1 || patches > 4096)
    return fail(ctx, PDEOPT_EINVAL, "%lld patches: supported are 1 to 4096", (long long)patches);
  if (blocks < 1 || blocks > kMixMaxBlocks) return fail(ctx, PDEOPT_EINVAL, "%d blocks: supported are 1 to %d", blocks, kMixMaxBlocks);
  if (activation != PDEOPT_MIXER_RELU && activation != PDEOPT_MIXER_GELU && activation != PDEOPT_MIXER_GELU_TANH &&
      activation != PDEOPT_MIXER_TANH)
    return fail(ctx, PDEOPT_EINVAL, "activation %d: supported are relu, gelu (erf form), gelu (tanh form) and tanh", activation);
  pdeopt_mixer* n = new pdeopt_mixer();
  n->what = "mixer";
  n->nx = p.nx, n->ny = p.ny, n->ps = patch, n->C = hidden, n->Mp = mix_patch, n->Mh = mix_hidden, n->K = blocks, n->act = activation;
  n->pw = p.ny / patch, n->P = (int)patches, n->Q = patch * patch;
  lay_out(n);
  return net_open(ctx, n, out);
}

int pdeopt_mixer_set_params(pdeopt_mixer* n, const double* params, int64_t count) { return net_set_params(n, params, count); }

int pdeopt_mixer_forward(pdeopt_mixer* n, const void* u_dev, void* mu_dev) { return net_forward<MixerFamily>(n, u_dev, mu_dev); }

int pdeopt_mixer_vjp(pdeopt_mixer* n, const void* u_dev, const void* gmu_dev, void* lam_dev) {
  return net_vjp<MixerFamily>(n, u_dev, gmu_dev, lam_dev);
}

int pdeopt_mixer_grad_read(pdeopt_mixer* n, double* out, int64_t count, int reset) { return net_grad_read(n, out, count, reset); }

int pdeopt_mixer_destroy(pdeopt_mixer* n) { return net_close(n); }

}  // extern "C"
