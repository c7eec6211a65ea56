// A periodic CNN evaluated and differentiated inside the library (the reference's pde_opt/numerics/functions/cnn.py as
// mu of Cahn-Hilliard; pde_opt_amd/numerics/functions/cnn.py is the torch module with the same parameters): a stack of
// 3 x 3 convolutions with circular "same" padding, stride 1, one input and one output channel, 1 to 6 hidden layers of
// width 1 ... 64 with one activation (gelu in its erf form, gelu in its tanh form, tanh), fp32 and fp64.
//
//   z_l = W_l * a_{l-1} + b_l,   a_l = act(z_l)  (l < L),   mu = z_L,   a_0 = u            (cross-correlation, as torch)
//
// Layout.  Activations are channels-last, [B][nx][ny][Cp] with the width padded to a multiple of 16 by zeros (zero
// weights and biases keep the padding zero through every activation of the family: act(0) = 0).  The input u and the
// output mu are plain fields [B][nx][ny]; the first and the last layer read / write them as channel 0 of 16.
// Packed weights: [tap = 3 ky + kx][c_in padded][c_out padded], so that a 16 x 16 x 4 matrix instruction takes
//   A[pixel][k]  = the LDS tile of the input, 16 pixels of one row at the tap's offset, 4 input channels
//   B[k][c_out]  = 4 x 16 packed weights, 64 contiguous bytes (fp32) per k
// and accumulates D[pixel][c_out] over 9 taps x C_in / 4 steps.  The backward-data pass is the same kernel on the
// transposed, flipped weights W'[tap'][o][i] = W[o][i][2 - ky'][2 - kx'] with the act'(z) epilogue.
//
// Tile plan.  One workgroup of 4 waves computes 8 x 16 pixels x all output channels: wave w owns rows 2 w and 2 w + 1
// (two M tiles) and every N tile, so an A operand read from LDS serves C_out / 16 instructions and a B operand read
// from memory serves two.  The input is staged 16 channels at a time on the tile + 1-cell periodic ring:
// 10 x 18 pixels x 16 channels at a pixel pitch of 18 elements (the 16 pixels x 2 k of a half wave then fall on
// distinct banks), 13 KB in fp32 and 26 KB in fp64.
//
// Weight gradient.  dW_l[o][i][tap] = sum over pixels of delta_l[o][p] a_{l-1}[i][p + tap] is the product
// A[o][k = pixel] B[k = pixel][i]: workgroup (g, i-block, o-block) walks the pixel tiles g, g + G, ... with both
// operands staged in LDS, every wave sums the 32 pixels of its two rows into nine 16 x 16 accumulators (one per tap),
// the four waves' accumulators are added in wave order, and cnn_wgrad_reduce_kernel sums the G partials in the order
// of g in fp64 and adds the result to the fp64 gradient buffer, which lives on the device across the substeps of a
// sweep.  Every sum has a fixed order and nothing is atomic: a repeat gives identical bits.
#include <algorithm>

#include "common.hpp"
#include "nn_device.hpp"
#include "nn_host.hpp"

constexpr int kCnnMaxLayers = 7;  // convolutions: 1 to 6 hidden layers + the output layer

struct pdeopt_cnn : pdeopt::NativeNet {
  int L = 0;                        // convolutions
  int C[kCnnMaxLayers + 1] = {};    // channels: C[0] = C[L] = 1
  int Cp[kCnnMaxLayers + 1] = {};   // padded to 16
  int act = 0;
  int64_t w_off[kCnnMaxLayers + 1] = {}, b_off[kCnnMaxLayers + 1] = {};  // torch order, layer l = 1 ... L
  // the packed block, per layer: forward weights, backward weights, bias
  int64_t wf_off[kCnnMaxLayers + 1] = {}, wb_off[kCnnMaxLayers + 1] = {}, pb_off[kCnnMaxLayers + 1] = {};  // elements
  // scratch of the configured shape: a_l and z_l of the hidden layers, two delta fields, the wgrad partials
  int s_nx = 0, s_ny = 0, s_batch = 0;
  pdeopt::DeviceBuffer a[kCnnMaxLayers];
  pdeopt::DeviceBuffer z[kCnnMaxLayers];
  pdeopt::DeviceBuffer delta[2];
  pdeopt::DeviceBuffer partial;
};

namespace pdeopt {
namespace {

constexpr int kPR = 8, kPC = 16;          // pixels of a workgroup tile
constexpr int kKC = 16;                   // channels staged per pass
constexpr int kLd = kKC + 2;              // LDS pixel pitch in elements
constexpr int kRR = kPR + 2, kRC = kPC + 2;  // the tile + its 1-cell ring

__device__ __forceinline__ int pmod(int i, int n) {
  const int m = i % n;
  return m < 0 ? m + n : m;
}

// s[pixel of the tile + ring][16 channels from kc on] of a channels-last field with C channels (scalar: a plain field
// as channel 0, zeros above), periodic in both axes
template <typename T>
__device__ __forceinline__ void stage_ring(T* __restrict__ s, const T* __restrict__ in, int b, int i0, int j0, int nx, int ny, int C,
                                           int kc, int scalar, int tid) {
  for (int q = tid; q < kRR * kRC * kKC; q += 256) {
    const int pix = q >> 4, ch = q & 15;
    const int r = pix / kRC, c = pix - r * kRC;
    const int64_t cell = ((int64_t)b * nx + pmod(i0 + r - 1, nx)) * ny + pmod(j0 + c - 1, ny);
    s[pix * kLd + ch] = scalar ? (ch == 0 ? in[cell] : T(0)) : in[cell * C + kc + ch];
  }
}
// the tile itself without ring, zeros outside the grid (the weight gradient sums over what is staged)
template <typename T>
__device__ __forceinline__ void stage_tile0(T* __restrict__ s, const T* __restrict__ in, int b, int i0, int j0, int nx, int ny, int C,
                                            int kc, int scalar, int tid) {
  for (int q = tid; q < kPR * kPC * kKC; q += 256) {
    const int pix = q >> 4, ch = q & 15;
    const int gi = i0 + (pix >> 4), gj = j0 + (pix & 15);
    T v = T(0);
    if (gi < nx && gj < ny) {
      const int64_t cell = ((int64_t)b * nx + gi) * ny + gj;
      v = scalar ? (ch == 0 ? in[cell] : T(0)) : in[cell * C + kc + ch];
    }
    s[pix * kLd + ch] = v;
  }
}

enum { EPI_ACT = 0, EPI_SCALAR = 1, EPI_DACT = 2, EPI_SCALAR_ADD = 3 };

template <typename T>
struct ConvArgs {
  const T* in;    // [B][nx][ny][Cip], or a plain field when in_scalar
  const T* w;     // [9][Cip][Cop]
  const T* bias;  // [Cop]; nullptr: none
  const T* zaux;  // EPI_DACT: z of the layer the result belongs to, [B][nx][ny][Cop]
  T* z_out;       // EPI_ACT: z is kept here when not nullptr
  T* out;         // [B][nx][ny][Cop]; EPI_SCALAR / EPI_SCALAR_ADD: a plain field, channel 0 stored / added
  int nx, ny, Cip, Cop, in_scalar, epi;
};

// One 3 x 3 periodic convolution layer with its epilogue; NT = Cop / 16.  ACT == NN_ACT_NONE: the scalar epilogues.
template <typename T, int ACT, int NT>
__global__ __launch_bounds__(256) void cnn_conv3x3_kernel(ConvArgs<T> a) {
  __shared__ T s[kRR * kRC * kLd];
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63, lp = lane & 15, lk = lane >> 4;
  const int b = blockIdx.z;
  const int i0 = blockIdx.y * kPR, j0 = blockIdx.x * kPC;
  const int nx = a.nx, ny = a.ny, Cip = a.Cip, Cop = a.Cop;
  vec4<T> acc[2][NT];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[m][nt] = vec4<T>{T(0), T(0), T(0), T(0)};
  const int ksteps = a.in_scalar ? 1 : kKC / 4;  // a plain field fills channel 0 alone
  for (int kc = 0; kc < Cip; kc += kKC) {
    if (kc) __syncthreads();
    stage_ring<T>(s, a.in, b, i0, j0, nx, ny, Cip, kc, a.in_scalar, tid);
    __syncthreads();
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int ky = tap / 3, kx = tap - 3 * ky;
      const T* __restrict__ sa = s + ((2 * wave + ky) * kRC + lp + kx) * kLd + lk;
      const T* __restrict__ wp = a.w + ((int64_t)tap * Cip + kc + lk) * Cop + lp;
#pragma unroll
      for (int k4 = 0; k4 < kKC / 4; ++k4) {
        if (k4 < ksteps) {
          const T a0 = sa[k4 * 4], a1 = sa[kRC * kLd + k4 * 4];
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            const T bv = wp[(int64_t)k4 * 4 * Cop + nt * 16];
            acc[0][nt] = mfma16(a0, bv, acc[0][nt]);
            acc[1][nt] = mfma16(a1, bv, acc[1][nt]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int gi = i0 + 2 * wave + m;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int co = nt * 16 + lp;
      const T bias = a.bias ? a.bias[co] : T(0);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int gj = j0 + acc_row<T>(lk, reg);
        if (gi >= nx || gj >= ny) continue;
        const int64_t cell = ((int64_t)b * nx + gi) * ny + gj;
        const T v = acc[m][nt][reg] + bias;
        if (ACT == NN_ACT_NONE) {
          if (co == 0) {
            if (a.epi == EPI_SCALAR) a.out[cell] = v;
            else a.out[cell] += v;
          }
        } else if (a.epi == EPI_ACT) {
          if (a.z_out) a.z_out[cell * Cop + co] = v;
          a.out[cell * Cop + co] = act_value<T, ACT>(v);
        } else {
          a.out[cell * Cop + co] = v * act_deriv<T, ACT>(a.zaux[cell * Cop + co]);
        }
      }
    }
  }
}

template <typename T>
struct WgradArgs {
  const T* act;  // a_{l-1}: [B][nx][ny][Cip], or a plain field (act_scalar)
  const T* del;  // delta_l: [B][nx][ny][Cop], or a plain field (del_scalar)
  T* partial;    // [G][o-block][i-block][9][16 o][16 i], then the bias partials [G][o-block][16]
  int nx, ny, Cip, Cop, act_scalar, del_scalar;
  int G, tiles_x, tiles_y, ntiles;  // ntiles = B tiles_y tiles_x
};

// grid (G, Cip / 16, Cop / 16): partial sums of dW over the pixel tiles g, g + G, ... for one 16 x 16 block of (o, i)
// and all nine taps; the i-block 0 also sums delta itself (the bias gradient)
template <typename T>
__global__ __launch_bounds__(256) void cnn_wgrad_kernel(WgradArgs<T> a) {
  __shared__ T sa[kRR * kRC * kLd];
  __shared__ T sd[kPR * kPC * kLd];
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63, lp = lane & 15, lk = lane >> 4;
  const int g = blockIdx.x, yi = blockIdx.y, zo = blockIdx.z;
  const int nti = gridDim.y, nto = gridDim.z;
  vec4<T> acc[9];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) acc[tap] = vec4<T>{T(0), T(0), T(0), T(0)};
  T bacc = T(0);
  for (int t = g; t < a.ntiles; t += a.G) {
    const int b = t / (a.tiles_x * a.tiles_y), rem = t - b * (a.tiles_x * a.tiles_y);
    const int ti = rem / a.tiles_x, tj = rem - ti * a.tiles_x;
    const int i0 = ti * kPR, j0 = tj * kPC;
    if (t != g) __syncthreads();
    stage_ring<T>(sa, a.act, b, i0, j0, a.nx, a.ny, a.Cip, yi * kKC, a.act_scalar, tid);
    stage_tile0<T>(sd, a.del, b, i0, j0, a.nx, a.ny, a.Cop, zo * kKC, a.del_scalar, tid);
    __syncthreads();
#pragma unroll
    for (int st = 0; st < 8; ++st) {  // 4 pixels per step: the wave's two rows of 16
      const int r = 2 * wave + (st >> 2), c = (st & 3) * 4 + lk;
      const T dv = sd[(r * kPC + c) * kLd + lp];
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int ky = tap / 3, kx = tap - 3 * ky;
        acc[tap] = mfma16(dv, sa[((r + ky) * kRC + c + kx) * kLd + lp], acc[tap]);
      }
    }
    if (yi == 0) {  // thread (p, ch): pixels p, p + 16, ... of channel ch
#pragma unroll
      for (int j = 0; j < kPR * kPC / 16; ++j) bacc += sd[((tid >> 4) + 16 * j) * kLd + (tid & 15)];
    }
  }
  // the four waves' accumulators, added in wave order
  T* __restrict__ red = sa;  // 4 x 256
  T* __restrict__ out = a.partial + (((int64_t)g * nto + zo) * nti + yi) * (9 * 256);
  for (int tap = 0; tap < 9; ++tap) {
    __syncthreads();
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) red[wave * 256 + acc_row<T>(lk, reg) * 16 + lp] = acc[tap][reg];
    __syncthreads();
    out[tap * 256 + tid] = ((red[tid] + red[256 + tid]) + red[512 + tid]) + red[768 + tid];
  }
  if (yi == 0) {
    __syncthreads();
    red[tid] = bacc;
    __syncthreads();
    if (tid < 16) {
      T sum = T(0);
      for (int p = 0; p < 16; ++p) sum += red[p * 16 + tid];
      a.partial[(int64_t)a.G * nto * nti * (9 * 256) + ((int64_t)g * nto + zo) * 16 + tid] = sum;
    }
  }
}

// grad[torch offset] += the partials summed over g in order, in fp64; one thread per packed entry of the layer
template <typename T>
__global__ __launch_bounds__(256) void cnn_wgrad_reduce_kernel(const T* __restrict__ partial, double* __restrict__ gw,
                                                               double* __restrict__ gb, int G, int nto, int nti, int Co, int Ci) {
  const int64_t block = (int64_t)nto * nti * (9 * 256);
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q < block) {
    const int i16 = q & 15, o16 = (q >> 4) & 15;
    const int tap = (int)((q >> 8) % 9);
    const int pair = (int)(q / (9 * 256));
    const int zo = pair / nti, yi = pair - zo * nti;
    const int o = zo * 16 + o16, i = yi * 16 + i16;
    if (o >= Co || i >= Ci) return;
    double sum = 0.0;
    for (int g = 0; g < G; ++g) sum += (double)partial[g * block + q];
    gw[((int64_t)o * Ci + i) * 9 + tap] += sum;
  } else if (q < block + nto * 16) {
    const int o = (int)(q - block);
    if (o >= Co) return;
    const T* __restrict__ bp = partial + (int64_t)G * block;
    double sum = 0.0;
    for (int g = 0; g < G; ++g) sum += (double)bp[(int64_t)g * nto * 16 + o];
    gb[o] += sum;
  }
}

inline int tiles_x(const pdeopt_ctx* ctx) { return (ctx->prob.ny + kPC - 1) / kPC; }
inline int tiles_y(const pdeopt_ctx* ctx) { return (ctx->prob.nx + kPR - 1) / kPR; }
// pixel-tile groups of the weight gradient of a layer with `pairs` 16 x 16 blocks: about 512 workgroups in all
inline int wgrad_groups(int ntiles, int pairs) { return std::min(ntiles, std::max(1, 512 / pairs)); }

// parameters in torch order -> the packed device block, in the problem dtype
template <typename T>
int upload_packed(pdeopt_cnn* n) {
  int64_t total = 0;
  for (int l = 1; l <= n->L; ++l) {
    const int64_t m = 9 * (int64_t)n->Cp[l - 1] * n->Cp[l];
    n->wf_off[l] = total;
    n->wb_off[l] = total + m;
    n->pb_off[l] = total + 2 * m;
    total += 2 * m + n->Cp[l];
  }
  std::vector<T> h((size_t)total, T(0));
  for (int l = 1; l <= n->L; ++l) {
    const int Ci = n->C[l - 1], Co = n->C[l], Cip = n->Cp[l - 1], Cop = n->Cp[l];
    const double* w = n->params.data() + n->w_off[l];
    for (int o = 0; o < Co; ++o)
      for (int i = 0; i < Ci; ++i)
        for (int tap = 0; tap < 9; ++tap) {
          const T v = (T)w[((int64_t)o * Ci + i) * 9 + tap];
          h[n->wf_off[l] + ((int64_t)tap * Cip + i) * Cop + o] = v;
          h[n->wb_off[l] + ((int64_t)(8 - tap) * Cop + o) * Cip + i] = v;  // (2 - ky, 2 - kx) is tap 8 - tap
        }
    for (int o = 0; o < Co; ++o) h[n->pb_off[l] + o] = (T)n->params[n->b_off[l] + o];
  }
  return net_upload(n, h);
}

// the scratch of the shape in the handle's key: what a forward pass writes, and for the backward pass z, delta, the partials
int size_scratch(pdeopt_cnn* n, bool backward) {
  pdeopt_ctx* ctx = n->ctx;
  const pdeopt_problem& p = ctx->prob;
  const size_t cells = (size_t)p.batch * p.nx * p.ny;
  int rc = 0;
  int cmax = 16;
  for (int l = 1; l < n->L; ++l) {
    cmax = std::max(cmax, n->Cp[l]);
    if ((rc = ensure_buffer(ctx, n->a[l], cells * n->Cp[l] * ctx->esize))) return rc;
    if (backward && (rc = ensure_buffer(ctx, n->z[l], cells * n->Cp[l] * ctx->esize))) return rc;
  }
  if (backward) {
    for (DeviceBuffer& d : n->delta)
      if ((rc = ensure_buffer(ctx, d, cells * cmax * ctx->esize))) return rc;
    const int ntiles = p.batch * tiles_x(ctx) * tiles_y(ctx);
    size_t most = 0;
    for (int l = 1; l <= n->L; ++l) {
      const int pairs = (n->Cp[l - 1] / 16) * (n->Cp[l] / 16);
      const size_t G = wgrad_groups(ntiles, pairs);
      most = std::max(most, G * pairs * (9 * 256) + G * (n->Cp[l] / 16) * 16);
    }
    if ((rc = ensure_buffer(ctx, n->partial, most * ctx->esize))) return rc;
  }
  return PDEOPT_OK;
}

template <typename T, int ACT>
int launch_conv_nt(pdeopt_ctx* ctx, const ConvArgs<T>& a) {
  const dim3 grid(tiles_x(ctx), tiles_y(ctx), ctx->prob.batch);
  switch (a.Cop / 16) {
    case 1: hipLaunchKernelGGL((cnn_conv3x3_kernel<T, ACT, 1>), grid, dim3(256), 0, ctx->stream, a); break;
    case 2: hipLaunchKernelGGL((cnn_conv3x3_kernel<T, ACT, 2>), grid, dim3(256), 0, ctx->stream, a); break;
    case 3: hipLaunchKernelGGL((cnn_conv3x3_kernel<T, ACT, 3>), grid, dim3(256), 0, ctx->stream, a); break;
    default: hipLaunchKernelGGL((cnn_conv3x3_kernel<T, ACT, 4>), grid, dim3(256), 0, ctx->stream, a); break;
  }
  ctx->n_stage_launches++;
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  return PDEOPT_OK;
}
template <typename T>
int launch_conv(pdeopt_ctx* ctx, int act, const ConvArgs<T>& a) {
  if (a.epi == EPI_SCALAR || a.epi == EPI_SCALAR_ADD) {
    hipLaunchKernelGGL((cnn_conv3x3_kernel<T, NN_ACT_NONE, 1>), dim3(tiles_x(ctx), tiles_y(ctx), ctx->prob.batch), dim3(256), 0,
                       ctx->stream, a);
    ctx->n_stage_launches++;
    PDEOPT_HIP_CHECK(ctx, hipGetLastError());
    return PDEOPT_OK;
  }
  if (act == PDEOPT_CNN_GELU) return launch_conv_nt<T, NN_ACT_GELU>(ctx, a);
  if (act == PDEOPT_CNN_GELU_TANH) return launch_conv_nt<T, NN_ACT_GELU_TANH>(ctx, a);
  return launch_conv_nt<T, NN_ACT_TANH>(ctx, a);
}

// mu = N(u), or the hidden layers alone when mu == nullptr; keep_z: their z_l stay in the handle's scratch for the
// backward pass
template <typename T>
int forward(pdeopt_cnn* n, const void* u, void* mu, bool keep_z) {
  pdeopt_ctx* ctx = n->ctx;
  const T* P = n->packed.as<const T>();
  for (int l = 1; l <= n->L; ++l) {
    if (l == n->L && !mu) break;
    ConvArgs<T> a{};
    a.in = l == 1 ? static_cast<const T*>(u) : n->a[l - 1].as<const T>();
    a.in_scalar = l == 1;
    a.w = P + n->wf_off[l];
    a.bias = P + n->pb_off[l];
    a.nx = ctx->prob.nx, a.ny = ctx->prob.ny, a.Cip = n->Cp[l - 1], a.Cop = n->Cp[l];
    if (l == n->L) {
      a.epi = EPI_SCALAR;
      a.out = static_cast<T*>(mu);
    } else {
      a.epi = EPI_ACT;
      a.out = n->a[l].as<T>();
      a.z_out = keep_z ? n->z[l].as<T>() : nullptr;
    }
    if (const int rc = launch_conv<T>(ctx, n->act, a)) return rc;
  }
  return PDEOPT_OK;
}

template <typename T>
int backward(pdeopt_cnn* n, const void* u, const void* gmu, void* lam) {
  pdeopt_ctx* ctx = n->ctx;
  const pdeopt_problem& p = ctx->prob;
  const T* P = n->packed.as<const T>();
  const int ntiles = p.batch * tiles_x(ctx) * tiles_y(ctx);
  const T* del = static_cast<const T*>(gmu);  // delta_L
  for (int l = n->L; l >= 1; --l) {
    const int Cip = n->Cp[l - 1], Cop = n->Cp[l];
    const int nti = Cip / 16, nto = Cop / 16;
    WgradArgs<T> w{};
    w.act = l == 1 ? static_cast<const T*>(u) : n->a[l - 1].as<const T>();
    w.act_scalar = l == 1;
    w.del = del;
    w.del_scalar = l == n->L;
    w.partial = n->partial.as<T>();
    w.nx = p.nx, w.ny = p.ny, w.Cip = Cip, w.Cop = Cop;
    w.G = wgrad_groups(ntiles, nti * nto);
    w.tiles_x = tiles_x(ctx), w.tiles_y = tiles_y(ctx), w.ntiles = ntiles;
    hipLaunchKernelGGL(cnn_wgrad_kernel<T>, dim3(w.G, nti, nto), dim3(256), 0, ctx->stream, w);
    const int64_t entries = (int64_t)nto * nti * (9 * 256) + nto * 16;
    hipLaunchKernelGGL(cnn_wgrad_reduce_kernel<T>, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, ctx->stream,
                       n->partial.as<const T>(), n->grad.as<double>() + n->w_off[l], n->grad.as<double>() + n->b_off[l], w.G, nto, nti, n->C[l],
                       n->C[l - 1]);
    ctx->n_stage_launches += 2;
    PDEOPT_HIP_CHECK(ctx, hipGetLastError());
    // delta_{l-1} = (W_l^T flipped * delta_l) act'(z_{l-1}); below the first layer it is the cotangent of u
    ConvArgs<T> a{};
    a.in = del;
    a.in_scalar = l == n->L;
    a.w = P + n->wb_off[l];
    a.nx = p.nx, a.ny = p.ny, a.Cip = Cop, a.Cop = Cip;
    if (l == 1) {
      a.epi = EPI_SCALAR_ADD;
      a.out = static_cast<T*>(lam);
    } else {
      a.epi = EPI_DACT;
      a.zaux = n->z[l - 1].as<const T>();
      a.out = n->delta[l & 1].as<T>();
    }
    if (const int rc = launch_conv<T>(ctx, n->act, a)) return rc;
    del = a.out;
  }
  return PDEOPT_OK;
}

// the CNN as the shared steps of nn_host.hpp see it
struct CnnFamily {
  static constexpr const char *forward_kernels = "cnn_conv3x3", *vjp_kernels = "cnn_conv3x3+cnn_wgrad";
  static int refuse(pdeopt_cnn* n, const pdeopt_problem& p) {
    return p.nx >= 4 && p.ny >= 4 ? PDEOPT_OK : fail(n->ctx, PDEOPT_EINVAL, "the CNN needs a grid of at least 4 x 4 (got %d x %d)", p.nx, p.ny);
  }
  static bool keyed_for(const pdeopt_cnn* n, const pdeopt_problem& p) {
    return n->s_dtype == p.dtype && n->s_nx == p.nx && n->s_ny == p.ny && n->s_batch == p.batch;
  }
  static void rekey(pdeopt_cnn* n, const pdeopt_problem& p) {
    for (int l = 0; l < kCnnMaxLayers; ++l) n->a[l].reset(), n->z[l].reset();
    for (DeviceBuffer& d : n->delta) d.reset();
    n->partial.reset();
    n->s_dtype = p.dtype, n->s_nx = p.nx, n->s_ny = p.ny, n->s_batch = p.batch;
  }
  static int size_workspace(pdeopt_cnn* n, bool backward) { return size_scratch(n, backward); }
  // in the problem dtype, t = T(): pack(t, n), forward(t, n, u, mu, keep_z), backward(t, n, u, gmu, lam)
  static constexpr auto pack = [](auto t, auto... a) { return upload_packed<decltype(t)>(a...); };
  static constexpr auto forward = [](auto t, auto... a) { return pdeopt::forward<decltype(t)>(a...); };
  static constexpr auto backward = [](auto t, auto... a) { return pdeopt::backward<decltype(t)>(a...); };
};

}  // namespace
}  // namespace pdeopt

using namespace pdeopt;

extern "C" {

int pdeopt_cnn_create(pdeopt_ctx* ctx, int n_layers, const int* channels, int activation, pdeopt_cnn** out) {
  if (!ctx || !out) return PDEOPT_EINVAL;
  *out = nullptr;
  if (!channels) return fail(ctx, PDEOPT_EINVAL, "channels is NULL");
  if (n_layers < 2 || n_layers > kCnnMaxLayers)
    return fail(ctx, PDEOPT_EINVAL, "the CNN has 1 to 6 hidden layers, that is 2 to 7 convolutions (got %d)", n_layers);
  if (channels[0] != 1 || channels[n_layers] != 1)
    return fail(ctx, PDEOPT_EINVAL, "the CNN maps one channel to one channel (got %d -> %d)", channels[0], channels[n_layers]);
  for (int l = 1; l < n_layers; ++l)
    if (channels[l] < 1 || channels[l] > 64)
      return fail(ctx, PDEOPT_EINVAL, "hidden layer %d has width %d: supported are 1 to 64", l, channels[l]);
  if (activation != PDEOPT_CNN_GELU && activation != PDEOPT_CNN_GELU_TANH && activation != PDEOPT_CNN_TANH)
    return fail(ctx, PDEOPT_EINVAL, "activation %d: supported are gelu (erf form), gelu (tanh form) and tanh", activation);
  pdeopt_cnn* n = new pdeopt_cnn();
  n->what = "CNN";
  n->L = n_layers;
  n->act = activation;
  for (int l = 0; l <= n_layers; ++l) n->C[l] = channels[l], n->Cp[l] = pad16(channels[l]);
  for (int l = 1; l <= n_layers; ++l) {
    n->w_off[l] = n->n_params;
    n->b_off[l] = n->n_params + 9 * (int64_t)n->C[l] * n->C[l - 1];
    n->n_params = n->b_off[l] + n->C[l];
  }
  return net_open(ctx, n, out);
}

int pdeopt_cnn_set_params(pdeopt_cnn* n, const double* params, int64_t count) { return net_set_params(n, params, count); }

int pdeopt_cnn_forward(pdeopt_cnn* n, const void* u_dev, void* mu_dev) { return net_forward<CnnFamily>(n, u_dev, mu_dev); }

int pdeopt_cnn_vjp(pdeopt_cnn* n, const void* u_dev, const void* gmu_dev, void* lam_dev) {
  return net_vjp<CnnFamily>(n, u_dev, gmu_dev, lam_dev);
}

int pdeopt_cnn_grad_read(pdeopt_cnn* n, double* out, int64_t count, int reset) { return net_grad_read(n, out, count, reset); }

int pdeopt_cnn_destroy(pdeopt_cnn* n) { return net_close(n); }

}  // extern "C"
