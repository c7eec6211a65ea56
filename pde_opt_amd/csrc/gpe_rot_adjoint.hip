// One substep of the discrete adjoint of the rotating-frame alternating-direction split step (PDEOPT_INT_STRANG_ROT,
// gpe_rot.hip): the reverse-mode gradient of a scalar objective of the solution over the interaction strength k, the
// trap anisotropy e and the rotation frequency Omega of every environment, and the cotangent of the start state
// (DESIGN.md section 4.12).
//
// Forward substep (gpe_rot.hip:1-10), s = tau / 2, tau = dt * time_scale, h^2 = strang_dx^2:
//   u1 = Lx(s) psi0;  a = Ly(s) u1;  w = V + k |psi0|^2;  c = a exp(-i w tau)
//   n = sqrt(h^2 sum |c|^2);  d = c / n;  e1 = Ly(s) d;  psi1 = Lx(s) e1
// Cotangents are complex fields dJ/dRe + i dJ/dIm in the state's (re, im) storage, the inner product is the real one;
// L^H multiplies by conj(exp(s A)) in the line's Fourier space.  With lambda1 the cotangent of psi1:
//   mu1 = Lx^H lambda1;  lambda_d = Ly^H mu1
//   sigma = h^2 sum Re(conj(d) lambda_d);  lambda_c = (lambda_d - sigma d) / n
//   lambda_a = lambda_c conj(exp(-i w tau));  g_w = Re(conj(-i tau c) lambda_c)
//   nu = Ly^H lambda_a;  lambda0 = Lx^H nu + 2 k g_w psi0
//   dJ/dk += sum g_w |psi0|^2;  dJ/de += sum g_w (x^2 - y^2) / 2   (V = ((1 + e) x^2 + (1 - e) y^2) / 2)
// Omega enters the four line operators only.  On a line the kinetic and the rotation part commute, so
// dL/dOmega = s R L with R = -y (2 pi i kx) for Lx and +x (2 pi i ky) for Ly.  With v an operator's output and
// lambda_v its cotangent, both transformed along the operator's axis (length N, unnormalised):
//   dJ/dOmega += (1 / N) sum Re(conj(lambda_v^) s R v^)      for each of the four operators, any complex s.
//
// Order of a call.  The cotangent chain needs nothing of the primal except in these sums, and every sum pairs a
// cotangent spectrum with the primal spectrum of the same operator, so the primal runs first and leaves its four
// spectra behind:
//   primal    : work = psi0 -> [x] S1 -> u1 -> [y] S2 -> a -> recompute: c, partial sums of |c|^2 -> [y] S3 -> [x] S4
//               ([axis] Sj: transform, multiply, keep the multiplied spectrum; the kinetic table carries the 1 / N of
//               the round trip, so Sj = v^ / N and the 1 / N of the Omega sum is already in it.  S3 and S4 are those
//               of c, not d: their sums are divided by n at the end.)
//   cotangent : lam [x] conj-multiply against S4 -> mu1 -> [y] against S3 -> lambda_d -> pointwise ->
//               lambda_a [y] against S2 -> nu -> [x] against S1 -> finish: + direct term, the sums
// sum Re(conj(c) lambda_d), the raw sigma, is taken in Fourier space by the conjugate multiply against S3 (Parseval
// along y: it equals sum Re(conj(S3) mu1^) line by line), which saves a pass over c and lambda_d.
//
// Per substep: 15 batched 1-D transforms on the library's rocFFT plans (spectral_c2c_axis: every grid the forward step
// takes), 1 copy, and 11 launches of the kernels below (4 multiplies, 4 conjugate multiplies, recompute, pointwise,
// finish), each one pass over the field = 27 launches.  Work buffers: FIVE field-sized arrays (work, c / the direct term,
// S1, S2, S3; S4 is work itself), allocated on first use and freed with the ctx, plus the two 1-D kinetic tables and
// the partial sums.
//
// Every reduction is in gather form, no atomics: a fixed partition (kBlocks workgroups per environment), fp64
// partials summed in a fixed order -- the scheme of gpe_adjoint.hip.  A repeat gives the same bits.
//
// The stirred, ramped step (DESIGN.md sections 4.13, 4.14; pdeopt_gpe_rot_stir_adjoint_step): Gaussian light spots in
// the potential and Omega(t) = omega + rate t in the line operators, and with them the gradient over the rate and over
// the seven numbers of every spot.  Forward substep starting at local time t0:
//   Omega0 = omega + rate t0 (one fused multiply-add, rot_omega_at: the forward step's number) in all four operators
//   w = V + spots(t0, x, y) + k |psi0|^2
// The cotangent chain is the one above with Omega0 in the factors and the spots in w.  With S_Omega the four operator
// sums (S3, S4 divided by n):
//   dJ/domega += S_Omega;  dJ/drate += t0 S_Omega
//   dJ/d(amp0, x0, y0, inv_two_w2) of spot s += sum over cells of g_w spot_partials(s)[0 .. 3]   (w enters, sign +)
//   dJ/d(amp_rate, x_rate, y_rate) of spot s += t0 x (the sums of amp0, x0, y0);  dJ/dk, dJ/de as before.
// The partial block of a workgroup has 8 + 4 PDEOPT_MAX_SPOTS slots.
//
// Both entry points run ONE schedule, tables and buffers (rot_adjoint_step_t).  The kernels come in pairs, radj_ for
// the frozen step and rsadj_ for the stirred one, and a frozen problem keeps its instructions and bits.  The multiply,
// the conjugate multiply and the phase expression are one __device__ __forceinline__ body each, a template on STIRRED
// under two thin __global__ wrappers: all their kernels compile to the instructions of the written-out ones.  The
// recompute pair is written out (as one inlined body both kernels changed: the frozen one 39 of 205 instructions fp32,
// 72 of 444 fp64), and so are pointwise and finish, which differ by the spot sums and the rate gradient.
#include <algorithm>
#include <cmath>
#include <complex>

#include "common.hpp"
#include "gpe_rot_adjoint_sums.hpp"
#include "gpe_rot_line.hpp"

namespace pdeopt {

// one per entry point (slots FS_GPE_ROT_ADJOINT, FS_GPE_ROT_STIR_ADJOINT): their partial blocks differ in size
struct GpeRotAdjoint : Feature {
  DeviceBuffer work;     // the running primal field, at the end S4     [batch][nx][ny] complex
  DeviceBuffer cbuf;     // c, then the direct term 2 k g_w psi0         same
  DeviceBuffer spec[3];  // S1, S2, S3                                   same
  DeviceBuffer kin_x;    // exp(tau/2 0.5j (2 pi i kx)^2) / nx, complex [nx]
  DeviceBuffer kin_y;
  DeviceBuffer part;     // doubles [batch][kBlocks][kSlots or kStirSlots]
  DeviceBuffer gacc;     // doubles [batch][3 or 4]: staging of a host gradient block
  DeviceBuffer sacc;     // doubles, stirred only: [batch][PDEOPT_MAX_SPOTS][7], staging of a host spot block
  double key_dt = NAN, key_tr = NAN, key_ti = NAN, key_hx = NAN, key_hy = NAN;
  bool valid = false;

  void invalidate() override { valid = false; }
};

namespace {

constexpr int kBlocks = kRadjBlocks;  // the fixed partition of every reduction (gpe_rot_adjoint_sums.hpp)
// the sums of one environment
enum { kNorm = 0, kSigma = 1, kGradK = 2, kGradE = 3, kOmega1 = 4, kOmega2 = 5, kOmega3 = 6, kOmega4 = 7, kSlots = 8 };
// the stirred step: the same, then 4 independent sums per spot (spot_partials)
constexpr int kSpotSums = 4 * PDEOPT_MAX_SPOTS, kSpot0 = kSlots, kStirSlots = kSpot0 + kSpotSums;

// block_sum: block_sums.hpp; radj_slot_total: gpe_rot_adjoint_sums.hpp
__device__ __forceinline__ double radj_slot_total(const double* part, int b, int slot, int lane) {
  return pdeopt::radj_slot_total(part, kSlots, b, slot, lane);
}
__device__ __forceinline__ double rsadj_total(const double* part, int b, int slot, int lane) {
  return pdeopt::radj_slot_total(part, kStirSlots, b, slot, lane);
}

// ---- the bodies both variants share: STIRRED chooses at compile time, a frozen kernel holds nothing of the other -----

// Omega of the environment and the line coefficient, each with its variant's own association (the stirred adjoint must
// form the number rstir_mul_kernel forms, Omega0 * (w * coord); the frozen one rot_mul_kernel's, (w * Omega) * coord)
template <bool STIRRED, typename T>
__device__ __forceinline__ T radj_omega(const RotAxis<T>& ax, const EnvParams<T>& e, T t0) {
  if constexpr (STIRRED) return rot_omega_at(e, t0);
  else return ax.w * e.gpe_omega;
}
template <bool STIRRED, typename T>
__device__ __forceinline__ T radj_coef(const RotAxis<T>& ax, T om, T coord) {
  if constexpr (STIRRED) return om * (ax.w * coord);
  else return om * coord;
}

// The primal's multiply: buf[b][ix][iy] *= kin[k] * rotation factor, the product kept in `save` too (nullptr: not).
// AXIS 0: the field is transformed along x, k = ix, the line's coordinate is y of iy; AXIS 1: along y, k = iy, x of ix.
// Stirred: at Omega0 = Omega(t0); frozen: t0 is not read.
template <typename T, int AXIS, bool STIRRED>
__device__ __forceinline__ void radj_mul_body(Cx<T>* __restrict__ buf, Cx<T>* __restrict__ save,
                                              const Cx<T>* __restrict__ kin, const EnvParams<T>* __restrict__ ep,
                                              const RotAxis<T>& ax, int nx, int ny, T t0) {
  const int b = blockIdx.y;
  const int64_t cells = (int64_t)nx * ny, o = (int64_t)b * cells;
  const T om = radj_omega<STIRRED>(ax, ep[b], t0);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (int64_t)gridDim.x * 256) {
    const int ix = (int)(i / ny), iy = (int)(i - (int64_t)ix * ny);
    const int k = AXIS == 0 ? ix : iy, n = AXIS == 0 ? nx : ny, line = AXIS == 0 ? iy : ix;
    const Cx<T> m = rot_mult<T>(kin[k], radj_coef<STIRRED>(ax, om, ax.c_first + T(line) * ax.c_step), k, n, ax.sr, ax.si);
    const Cx<T> r = cmul(buf[o + i], m);
    buf[o + i] = r;
    if (save) save[o + i] = r;
  }
}
template <typename T, int AXIS>
__global__ __launch_bounds__(256) void radj_mul_kernel(Cx<T>* __restrict__ buf, Cx<T>* __restrict__ save,
                                                       const Cx<T>* __restrict__ kin, const EnvParams<T>* __restrict__ ep,
                                                       const RotAxis<T> ax, int nx, int ny) {
  radj_mul_body<T, AXIS, false>(buf, save, kin, ep, ax, nx, ny, T(0));
}
template <typename T, int AXIS>
__global__ __launch_bounds__(256) void rsadj_mul_kernel(Cx<T>* __restrict__ buf, Cx<T>* __restrict__ save,
                                                        const Cx<T>* __restrict__ kin, const EnvParams<T>* __restrict__ ep,
                                                        const RotAxis<T> ax, int nx, int ny, T t0) {
  radj_mul_body<T, AXIS, true>(buf, save, kin, ep, ax, nx, ny, t0);
}

// The cotangent's multiply: lam^ *= conj(kin[k] * rotation factor), and beside it the Omega sum of this operator,
//   part[b][block][slot] = sum Re(conj(lam^) s R prim),   s R = (sr + i si) i r,   r = w coord k_signed
// (prim = the operator's multiplied primal spectrum / N).  SIGMA: part[b][block][kSigma] = sum Re(conj(prim) lam^).
// The partial block of a workgroup has kSlots (frozen) or kStirSlots slots.
template <typename T, int AXIS, bool SIGMA, bool STIRRED>
__device__ __forceinline__ void radj_conj_mul_body(Cx<T>* __restrict__ lam, const Cx<T>* __restrict__ prim,
                                                   const Cx<T>* __restrict__ kin, const EnvParams<T>* __restrict__ ep,
                                                   const RotAxis<T>& ax, int nx, int ny, double* __restrict__ part,
                                                   int slot, T t0) {
  __shared__ double sh[4];
  const int b = blockIdx.y;
  const int64_t cells = (int64_t)nx * ny, o = (int64_t)b * cells;
  const T om = radj_omega<STIRRED>(ax, ep[b], t0);
  double acc_o = 0.0, acc_s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (int64_t)gridDim.x * 256) {
    const int ix = (int)(i / ny), iy = (int)(i - (int64_t)ix * ny);
    const int k = AXIS == 0 ? ix : iy, n = AXIS == 0 ? nx : ny, line = AXIS == 0 ? iy : ix;
    const T coord = ax.c_first + T(line) * ax.c_step, wc = ax.w * coord;
    const Cx<T> m = rot_mult<T>(kin[k], radj_coef<STIRRED>(ax, om, coord), k, n, ax.sr, ax.si);  // the primal's factor, bit for bit
    const Cx<T> l = lam[o + i], v = prim[o + i];
    const int ks = k < (n + 1) / 2 ? k : k - n;
    // (sr + i si) i v = (-si v.re - sr v.im) + i (sr v.re - si v.im)
    const T zr = -ax.si * v.re - ax.sr * v.im, zi = ax.sr * v.re - ax.si * v.im;
    acc_o += (double)(wc * T(ks)) * ((double)l.re * (double)zr + (double)l.im * (double)zi);
    if (SIGMA) acc_s += (double)v.re * (double)l.re + (double)v.im * (double)l.im;
    lam[o + i] = cmul(l, Cx<T>{m.re, -m.im});
  }
  double* out = part + ((int64_t)b * kBlocks + blockIdx.x) * (STIRRED ? kStirSlots : kSlots);
  const double so = block_sum(acc_o, sh);
  if (threadIdx.x == 0) out[slot] = so;
  if (SIGMA) {
    const double ss = block_sum(acc_s, sh);
    if (threadIdx.x == 0) out[kSigma] = ss;
  }
}
template <typename T, int AXIS, bool SIGMA>
__global__ __launch_bounds__(256) void radj_conj_mul_kernel(Cx<T>* __restrict__ lam, const Cx<T>* __restrict__ prim,
                                                            const Cx<T>* __restrict__ kin,
                                                            const EnvParams<T>* __restrict__ ep, const RotAxis<T> ax,
                                                            int nx, int ny, double* __restrict__ part, int slot) {
  radj_conj_mul_body<T, AXIS, SIGMA, false>(lam, prim, kin, ep, ax, nx, ny, part, slot, T(0));
}
template <typename T, int AXIS, bool SIGMA>
__global__ __launch_bounds__(256) void rsadj_conj_mul_kernel(Cx<T>* __restrict__ lam, const Cx<T>* __restrict__ prim,
                                                             const Cx<T>* __restrict__ kin,
                                                             const EnvParams<T>* __restrict__ ep, const RotAxis<T> ax,
                                                             int nx, int ny, double* __restrict__ part, int slot, T t0) {
  radj_conj_mul_body<T, AXIS, SIGMA, true>(lam, prim, kin, ep, ax, nx, ny, part, slot, t0);
}

template <typename T>
struct RadjArgs {
  Cx<T>* work;            // recompute: a in, c out
  Cx<T>* cbuf;            // recompute: c out; pointwise: c in, the direct term out
  const Cx<T>* psi0;
  Cx<T>* lam;             // pointwise: lambda_d in, lambda_a out
  const T* pot;           // trap potential, nullptr: none
  int64_t pot_stride;     // elements between environments (0: shared)
  const EnvParams<T>* ep;
  T tr, ti;               // tau
  T x_first, y_first, hx, hy;
  int64_t cells;
  int ny;
  double h2;
  double* part;
};
template <typename T>
struct RsadjArgs : RadjArgs<T> {
  SpotArgs<T> spots;      // the spots at t0 (spots.n == 0: none)
};

// exp(-i w tau), w = V + k |psi0|^2 (the expression of rot_b_kernel); stirred, A = RsadjArgs: w = V + spots(t0) + k |psi0|^2
// at cell (ix, iy) (the expression of rstir_b_kernel)
template <bool STIRRED, typename T, typename A>
__device__ __forceinline__ Cx<T> radj_phase(const A& a, int env, int64_t i, int ix, int iy, Cx<T> p0, T kk) {
  T w = a.pot ? a.pot[(int64_t)env * a.pot_stride + i] : T(0);
  if constexpr (STIRRED) {
    if (a.spots.n)
      w += spots_value<T>(a.spots, env, a.spots.x_first + T(ix) * a.spots.hx, a.spots.y_first + T(iy) * a.spots.hy);
  }
  w += kk * (p0.re * p0.re + p0.im * p0.im);
  T sn, cs;
  sincos_t<T>(w * a.tr, &sn, &cs);
  const T mag = (a.ti == T(0)) ? T(1) : exp_t<T>(w * a.ti);
  return Cx<T>{mag * cs, -mag * sn};
}

// work: a -> c = a exp(-i w tau), cbuf = c;  part[b][block][kNorm] = sum |c|^2.  The pair is written out: as one inlined
// body both kernels compiled to other instructions (the frozen ones 39 of 205 fp32, 72 of 444 fp64).
template <typename T>
__global__ __launch_bounds__(256) void radj_recompute_kernel(const RadjArgs<T> a) {
  __shared__ double sh[4];
  const int b = blockIdx.y;
  const int64_t o = (int64_t)b * a.cells;
  const T kk = a.ep[b].gpe_k;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.cells; i += (int64_t)gridDim.x * 256) {
    const Cx<T> c = cmul(a.work[o + i], radj_phase<false, T>(a, b, i, 0, 0, a.psi0[o + i], kk));
    a.work[o + i] = c;
    a.cbuf[o + i] = c;
    acc += (double)c.re * (double)c.re + (double)c.im * (double)c.im;
  }
  const double s = block_sum(acc, sh);
  if (threadIdx.x == 0) a.part[((int64_t)b * kBlocks + blockIdx.x) * kSlots + kNorm] = s;
}
template <typename T>
__global__ __launch_bounds__(256) void rsadj_recompute_kernel(const RsadjArgs<T> a) {
  __shared__ double sh[4];
  const int b = blockIdx.y;
  const int64_t o = (int64_t)b * a.cells;
  const T kk = a.ep[b].gpe_k;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.cells; i += (int64_t)gridDim.x * 256) {
    const int ix = (int)(i / a.ny), iy = (int)(i - (int64_t)ix * a.ny);
    const Cx<T> c = cmul(a.work[o + i], radj_phase<true, T>(a, b, i, ix, iy, a.psi0[o + i], kk));
    a.work[o + i] = c;
    a.cbuf[o + i] = c;
    acc += (double)c.re * (double)c.re + (double)c.im * (double)c.im;
  }
  const double s = block_sum(acc, sh);
  if (threadIdx.x == 0) a.part[((int64_t)b * kBlocks + blockIdx.x) * kStirSlots + kNorm] = s;
}

// ---- pointwise and finish: side by side (the stirred ones carry the spot sums and the rate gradient; shared through
// `if constexpr` they would not read better than the two copies) -------------------------------------------------------

// lam: lambda_d -> lambda_a;  cbuf: c -> 2 k g_w psi0;  part[b][block][kGradK, kGradE] = sum g_w |psi0|^2, g_w (x^2 - y^2) / 2
template <typename T>
__global__ __launch_bounds__(256) void radj_pointwise_kernel(const RadjArgs<T> a) {
  __shared__ double sh[4];
  __shared__ double tot[2];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t o = (int64_t)b * a.cells;
  if (tid < 64) {  // the two sums of this environment, every workgroup in the same order
    const double sn = radj_slot_total(a.part, b, kNorm, tid), ss = radj_slot_total(a.part, b, kSigma, tid);
    if (tid == 0) {
      tot[0] = sn;
      tot[1] = ss;
    }
  }
  __syncthreads();
  const double nrm = sqrt(tot[0] * a.h2);
  const T inv_n = (T)(1.0 / nrm);
  const T s_over_n = (T)(a.h2 * tot[1] / (nrm * nrm));  // sigma / n, sigma = h^2 sum Re(conj(c) lambda_d) / n
  const T kk = a.ep[b].gpe_k;
  double acc_k = 0.0, acc_e = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < a.cells; i += (int64_t)gridDim.x * 256) {
    const Cx<T> p0 = a.psi0[o + i];
    const Cx<T> e = radj_phase<false, T>(a, b, i, 0, 0, p0, kk);
    const Cx<T> c = a.cbuf[o + i], ld = a.lam[o + i];
    // lambda_c = (lambda_d - sigma d) / n, d = c / n
    const Cx<T> lc{(ld.re - s_over_n * c.re) * inv_n, (ld.im - s_over_n * c.im) * inv_n};
    // lambda_a = lambda_c conj(e)
    a.lam[o + i] = cmul(lc, Cx<T>{e.re, -e.im});
    // g_w = Re(conj(-i tau c) lambda_c), -i tau = ti - i tr
    const T zr = a.ti * c.re + a.tr * c.im, zi = a.ti * c.im - a.tr * c.re;
    const T gw = zr * lc.re + zi * lc.im;
    const T f = T(2) * kk * gw;
    a.cbuf[o + i] = Cx<T>{f * p0.re, f * p0.im};
    const int ix = (int)(i / a.ny), iy = (int)(i - (int64_t)ix * a.ny);
    const T x = a.x_first + T(ix) * a.hx, y = a.y_first + T(iy) * a.hy;
    acc_k += (double)gw * (double)(p0.re * p0.re + p0.im * p0.im);
    acc_e += (double)gw * (double)(T(0.5) * (x * x - y * y));
  }
  double* out = a.part + ((int64_t)b * kBlocks + blockIdx.x) * kSlots;
  const double sk = block_sum(acc_k, sh);
  if (tid == 0) out[kGradK] = sk;
  const double se = block_sum(acc_e, sh);
  if (tid == 0) out[kGradE] = se;
}

// lam += direct;  workgroup 0 of every environment: grad[b][0 .. 2] += (k, e, Omega), the sums over the fixed partition
template <typename T>
__global__ __launch_bounds__(256) void radj_finish_kernel(Cx<T>* __restrict__ lam, const Cx<T>* __restrict__ direct,
                                                          int64_t cells, const double* __restrict__ part,
                                                          double* __restrict__ grad, double h2) {
  const int b = blockIdx.y;
  const int64_t o = (int64_t)b * cells;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (int64_t)gridDim.x * 256) {
    const Cx<T> d = direct[o + i];
    Cx<T> l = lam[o + i];
    l.re += d.re;
    l.im += d.im;
    lam[o + i] = l;
  }
  if (blockIdx.x == 0 && threadIdx.x < 64) {  // one wave, uniform control flow around the shuffles
    const int lane = threadIdx.x;
    const double sn = radj_slot_total(part, b, kNorm, lane);
    const double gk = radj_slot_total(part, b, kGradK, lane), ge = radj_slot_total(part, b, kGradE, lane);
    const double o1 = radj_slot_total(part, b, kOmega1, lane), o2 = radj_slot_total(part, b, kOmega2, lane);
    const double o3 = radj_slot_total(part, b, kOmega3, lane), o4 = radj_slot_total(part, b, kOmega4, lane);
    if (lane == 0) {
      double* g = grad + (int64_t)b * 3;
      g[0] += gk;
      g[1] += ge;
      g[2] += (o1 + o2) + (o3 + o4) / sqrt(sn * h2);  // S3, S4 are the spectra of c = n d
    }
  }
}

// ---- the stirred kernels ------------------------------------------------------------------------------------------

// lam: lambda_d -> lambda_a;  cbuf: c -> 2 k g_w psi0;  part[b][block][kGradK, kGradE] = sum g_w |psi0|^2,
// g_w (x^2 - y^2) / 2;  part[b][block][kSpot0 + 4 s + q] = sum g_w x partial q of spot s
template <typename T>
__global__ __launch_bounds__(256) void rsadj_pointwise_kernel(const RsadjArgs<T> a) {
  __shared__ double sh[4];
  __shared__ double tot[2];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t o = (int64_t)b * a.cells;
  if (tid < 64) {  // the two sums of this environment, every workgroup in the same order
    const double sn = rsadj_total(a.part, b, kNorm, tid), ss = rsadj_total(a.part, b, kSigma, tid);
    if (tid == 0) {
      tot[0] = sn;
      tot[1] = ss;
    }
  }
  __syncthreads();
  const double nrm = sqrt(tot[0] * a.h2);
  const T inv_n = (T)(1.0 / nrm);
  const T s_over_n = (T)(a.h2 * tot[1] / (nrm * nrm));  // sigma / n, sigma = h^2 sum Re(conj(c) lambda_d) / n
  const T kk = a.ep[b].gpe_k;
  const int ns = a.spots.n;
  double acc_k = 0.0, acc_e = 0.0;
  double acc[kSpotSums];
#pragma unroll
  for (int q = 0; q < kSpotSums; ++q) acc[q] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < a.cells; i += (int64_t)gridDim.x * 256) {
    const int ix = (int)(i / a.ny), iy = (int)(i - (int64_t)ix * a.ny);
    const T xs = a.spots.x_first + T(ix) * a.spots.hx, ys = a.spots.y_first + T(iy) * a.spots.hy;
    const Cx<T> p0 = a.psi0[o + i];
    const Cx<T> e = radj_phase<true, T>(a, b, i, ix, iy, p0, kk);
    const Cx<T> c = a.cbuf[o + i], ld = a.lam[o + i];
    // lambda_c = (lambda_d - sigma d) / n, d = c / n
    const Cx<T> lc{(ld.re - s_over_n * c.re) * inv_n, (ld.im - s_over_n * c.im) * inv_n};
    // lambda_a = lambda_c conj(e)
    a.lam[o + i] = cmul(lc, Cx<T>{e.re, -e.im});
    // g_w = Re(conj(-i tau c) lambda_c), -i tau = ti - i tr
    const T zr = a.ti * c.re + a.tr * c.im, zi = a.ti * c.im - a.tr * c.re;
    const T gw = zr * lc.re + zi * lc.im;
    const T f = T(2) * kk * gw;
    a.cbuf[o + i] = Cx<T>{f * p0.re, f * p0.im};
    const T x = a.x_first + T(ix) * a.hx, y = a.y_first + T(iy) * a.hy;
    acc_k += (double)gw * (double)(p0.re * p0.re + p0.im * p0.im);
    acc_e += (double)gw * (double)(T(0.5) * (x * x - y * y));
#pragma unroll
    for (int s = 0; s < PDEOPT_MAX_SPOTS; ++s) {
      if (s < ns) {
        T d[4];
        spot_partials<T>(a.spots, b, s, xs, ys, d);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[4 * s + q] += (double)gw * (double)d[q];
      }
    }
  }
  double* out = a.part + ((int64_t)b * kBlocks + blockIdx.x) * kStirSlots;
  const double sk = block_sum(acc_k, sh);
  if (tid == 0) out[kGradK] = sk;
  const double se = block_sum(acc_e, sh);
  if (tid == 0) out[kGradE] = se;
#pragma unroll
  for (int q = 0; q < kSpotSums; ++q) {
    if (q < 4 * ns) {  // uniform over the workgroup
      const double v = block_sum(acc[q], sh);
      if (tid == 0) out[kSpot0 + q] = v;
    }
  }
}

// lam += direct;  workgroup 0 of every environment: grad[b][0 .. 3] += (k, e, S_Omega, t0 S_Omega) and
// spot_grad[b][s][0 .. 6] += the spot sums (rates: t0 x their value's sum), the sums over the fixed partition
template <typename T>
__global__ __launch_bounds__(256) void rsadj_finish_kernel(Cx<T>* __restrict__ lam, const Cx<T>* __restrict__ direct,
                                                           int64_t cells, const double* __restrict__ part,
                                                           double* __restrict__ grad, double* __restrict__ spot_grad,
                                                           int n_spots, double h2, double t0) {
  const int b = blockIdx.y;
  const int64_t o = (int64_t)b * cells;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (int64_t)gridDim.x * 256) {
    const Cx<T> d = direct[o + i];
    Cx<T> l = lam[o + i];
    l.re += d.re;
    l.im += d.im;
    lam[o + i] = l;
  }
  if (blockIdx.x == 0 && threadIdx.x < 64) {  // one wave, uniform control flow around the shuffles
    const int lane = threadIdx.x;
    const double sn = rsadj_total(part, b, kNorm, lane);
    const double gk = rsadj_total(part, b, kGradK, lane), ge = rsadj_total(part, b, kGradE, lane);
    const double o1 = rsadj_total(part, b, kOmega1, lane), o2 = rsadj_total(part, b, kOmega2, lane);
    const double o3 = rsadj_total(part, b, kOmega3, lane), o4 = rsadj_total(part, b, kOmega4, lane);
    if (lane == 0) {
      double* g = grad + (int64_t)b * 4;
      const double s_omega = (o1 + o2) + (o3 + o4) / sqrt(sn * h2);  // S3, S4 are the spectra of c = n d
      g[0] += gk;
      g[1] += ge;
      g[2] += s_omega;
      g[3] += t0 * s_omega;
    }
    for (int sq = 0; sq < 4 * n_spots; ++sq) {  // uniform over the wave
      const double v = rsadj_total(part, b, kSpot0 + sq, lane);
      if (lane == 0) {
        const int s = sq >> 2, q = sq & 3;
        double* g = spot_grad + ((int64_t)b * n_spots + s) * 7;  // amp0, amp_rate, x0, x_rate, y0, y_rate, inv_two_w2
        if (q == 3) {
          g[6] += v;
        } else {
          g[2 * q] += v;
          g[2 * q + 1] += t0 * v;
        }
      }
    }
  }
}

// ---- host: one copy, STIRRED picks the kernels and appends their arguments ------------------------------------------

template <typename T>
int ensure_tables(pdeopt_ctx* ctx, GpeRotAdjoint& ra, double dt) {
  const pdeopt_problem& p = ctx->prob;
  if (ra.valid && ra.key_dt == dt && ra.key_tr == ctx->ts_re && ra.key_ti == ctx->ts_im && ra.key_hx == p.hx && ra.key_hy == p.hy)
    return PDEOPT_OK;
  const std::complex<double> half_tau = 0.5 * dt * std::complex<double>(ctx->ts_re, ctx->ts_im);
  int rc;
  if ((rc = upload_kinetic<T>(ctx, ra.kin_x, p.nx, p.hx, half_tau))) return rc;
  if ((rc = upload_kinetic<T>(ctx, ra.kin_y, p.ny, p.hy, half_tau))) return rc;
  ra.valid = true;
  ra.key_dt = dt;
  ra.key_tr = ctx->ts_re;
  ra.key_ti = ctx->ts_im;
  ra.key_hx = p.hx;
  ra.key_hy = p.hy;
  return PDEOPT_OK;
}

// the work fields, the partial sums and the staging blocks of a substep, allocated on first use
template <bool STIRRED>
int ensure_work(pdeopt_ctx* ctx, GpeRotAdjoint& ra) {
  const size_t batch = (size_t)ctx->prob.batch;
  int rc;
  if ((rc = ensure_buffer(ctx, ra.work, ctx->total_bytes))) return rc;
  if ((rc = ensure_buffer(ctx, ra.cbuf, ctx->total_bytes))) return rc;
  for (DeviceBuffer& s : ra.spec)
    if ((rc = ensure_buffer(ctx, s, ctx->total_bytes))) return rc;
  if ((rc = ensure_buffer(ctx, ra.part, sizeof(double) * batch * kBlocks * (STIRRED ? kStirSlots : kSlots)))) return rc;
  if ((rc = ensure_buffer(ctx, ra.gacc, sizeof(double) * batch * (STIRRED ? 4 : 3)))) return rc;
  if (STIRRED && (rc = ensure_buffer(ctx, ra.sacc, sizeof(double) * batch * PDEOPT_MAX_SPOTS * 7))) return rc;
  return PDEOPT_OK;
}

// One backward substep (the order of a call, above).  Frozen: t0 and spot_grad_dev are not used.
template <typename T, bool STIRRED>
int rot_adjoint_step_t(pdeopt_ctx* ctx, GpeRotAdjoint& ra, double t0, double dt, const void* psi0, void* lam_dev,
                       double* grad_dev, double* spot_grad_dev) {
  const pdeopt_problem& p = ctx->prob;
  const int64_t cells = (int64_t)p.nx * p.ny;
  int rc = ensure_tables<T>(ctx, ra, dt);
  if (rc) return rc;
  const std::complex<double> tau = dt * std::complex<double>(ctx->ts_re, ctx->ts_im);
  const dim3 mgrid((unsigned)std::min<int64_t>(4096, (cells + 255) / 256), p.batch), rgrid(kBlocks, p.batch), blk(256);
  const EnvParams<T>* ep = env_params<T>(ctx, 0);
  const RotAxis<T> axes[2] = {rot_axis<T>(ctx, 0, 0.5 * tau), rot_axis<T>(ctx, 1, 0.5 * tau)};
  const Cx<T>* const kin[2] = {ra.kin_x.as<const Cx<T>>(), ra.kin_y.as<const Cx<T>>()};
  const AuxField& pot = ctx->aux[PDEOPT_AUX_GPE_POTENTIAL];
  Cx<T>* const work = ra.work.as<Cx<T>>();
  Cx<T>* const lam = (Cx<T>*)lam_dev;
  const T t = (T)t0;
  std::conditional_t<STIRRED, RsadjArgs<T>, RadjArgs<T>> a{};
  a.work = work;
  a.cbuf = ra.cbuf.as<Cx<T>>();
  a.psi0 = (const Cx<T>*)psi0;
  a.lam = lam;
  a.pot = pot.dev.as<const T>();
  a.pot_stride = pot.per_env ? cells : 0;
  a.ep = ep;
  a.tr = (T)tau.real();
  a.ti = (T)tau.imag();
  a.x_first = (T)ctx->rot_x_first;
  a.y_first = (T)ctx->rot_y_first;
  a.hx = (T)p.hx;
  a.hy = (T)p.hy;
  a.cells = cells;
  a.ny = p.ny;
  a.h2 = ctx->strang_dx * ctx->strang_dx;
  a.part = ra.part.as<double>();
  if constexpr (STIRRED) a.spots = make_spot_args<T>(ctx, 0, t0);
  // primal: transform along `axis`, multiply (the spectrum kept in `save`), and back unless it is the last one
  auto primal_op = [&](auto axis, Cx<T>* save, bool back) -> int {
    constexpr int A = decltype(axis)::value;
    int r = spectral_c2c_axis(ctx, A, true, work);
    if (r) return r;
    if constexpr (STIRRED)
      hipLaunchKernelGGL((rsadj_mul_kernel<T, A>), mgrid, blk, 0, ctx->stream, work, save, kin[A], ep, axes[A], p.nx, p.ny, t);
    else
      hipLaunchKernelGGL((radj_mul_kernel<T, A>), mgrid, blk, 0, ctx->stream, work, save, kin[A], ep, axes[A], p.nx, p.ny);
    return back ? spectral_c2c_axis(ctx, A, false, work) : PDEOPT_OK;
  };
  // cotangent: lam <- L^H lam of the operator whose multiplied primal spectrum is `prim`, its Omega sum into `slot`
  // (sigma: the raw sigma beside it)
  auto cotangent_op = [&](auto axis, auto sigma, const Cx<T>* prim, int slot) -> int {
    constexpr int A = decltype(axis)::value;
    constexpr bool S = decltype(sigma)::value;
    int r = spectral_c2c_axis(ctx, A, true, lam);
    if (r) return r;
    if constexpr (STIRRED)
      hipLaunchKernelGGL((rsadj_conj_mul_kernel<T, A, S>), rgrid, blk, 0, ctx->stream, lam, prim, kin[A], ep, axes[A], p.nx,
                         p.ny, ra.part.as<double>(), slot, t);
    else
      hipLaunchKernelGGL((radj_conj_mul_kernel<T, A, S>), rgrid, blk, 0, ctx->stream, lam, prim, kin[A], ep, axes[A], p.nx,
                         p.ny, ra.part.as<double>(), slot);
    return spectral_c2c_axis(ctx, A, false, lam);
  };
  constexpr std::integral_constant<int, 0> along_x{};
  constexpr std::integral_constant<int, 1> along_y{};
  constexpr std::false_type plain{};
  constexpr std::true_type with_sigma{};
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(work, psi0, ctx->total_bytes, hipMemcpyDeviceToDevice, ctx->stream));
  if ((rc = primal_op(along_x, ra.spec[0].as<Cx<T>>(), true))) return rc;   // u1
  if ((rc = primal_op(along_y, ra.spec[1].as<Cx<T>>(), true))) return rc;   // a
  if constexpr (STIRRED) hipLaunchKernelGGL(rsadj_recompute_kernel<T>, rgrid, blk, 0, ctx->stream, a);
  else hipLaunchKernelGGL(radj_recompute_kernel<T>, rgrid, blk, 0, ctx->stream, a);
  if ((rc = primal_op(along_y, ra.spec[2].as<Cx<T>>(), true))) return rc;   // n e1
  if ((rc = primal_op(along_x, nullptr, false))) return rc;             // work = S4
  if ((rc = cotangent_op(along_x, plain, work, kOmega4))) return rc;                             // mu1
  if ((rc = cotangent_op(along_y, with_sigma, ra.spec[2].as<const Cx<T>>(), kOmega3))) return rc;    // lambda_d, the raw sigma
  if constexpr (STIRRED) hipLaunchKernelGGL(rsadj_pointwise_kernel<T>, rgrid, blk, 0, ctx->stream, a);
  else hipLaunchKernelGGL(radj_pointwise_kernel<T>, rgrid, blk, 0, ctx->stream, a);
  if ((rc = cotangent_op(along_y, plain, ra.spec[1].as<const Cx<T>>(), kOmega2))) return rc;         // nu
  if ((rc = cotangent_op(along_x, plain, ra.spec[0].as<const Cx<T>>(), kOmega1))) return rc;         // Lx^H nu
  if constexpr (STIRRED)
    hipLaunchKernelGGL(rsadj_finish_kernel<T>, rgrid, blk, 0, ctx->stream, lam, ra.cbuf.as<const Cx<T>>(), cells,
                       ra.part.as<const double>(), grad_dev, spot_grad_dev, ctx->n_spots, a.h2, t0);
  else
    hipLaunchKernelGGL(radj_finish_kernel<T>, rgrid, blk, 0, ctx->stream, lam, ra.cbuf.as<const Cx<T>>(), cells,
                       ra.part.as<const double>(), grad_dev, a.h2);
  ctx->n_stage_launches += 26;  // 15 transforms, 8 multiplies, 3 passes
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  return PDEOPT_OK;
}

}  // namespace

}  // namespace pdeopt

using namespace pdeopt;

extern "C" {

int pdeopt_gpe_rot_adjoint_step(pdeopt_ctx* ctx, double dt, const void* psi0_dev, void* lam_dev, double* grad) {
  if (!ctx) return PDEOPT_EINVAL;
  if (!ctx->configured) return fail(ctx, PDEOPT_ESTATE, "pdeopt_configure has not been called");
  const pdeopt_problem& p = ctx->prob;
  if (p.equation != PDEOPT_EQ_GPE) return fail(ctx, PDEOPT_EINVAL, "the adjoint of the rotating-frame split step needs the GPE");
  if (!ctx->rot_set)
    return fail(ctx, PDEOPT_ESTATE, "the adjoint of the rotating-frame split step needs pdeopt_set_gpe_rotation (Omega and the "
                                    "mesh origin)");
  if (ctx->n_spots)
    return fail(ctx, PDEOPT_EINVAL, "the rotating-frame split step has no light spots: their gradient is "
                                    "pdeopt_gpe_adjoint_step's");
  if (ctx->rot_any_rate)
    return fail(ctx, PDEOPT_EINVAL, "the adjoint of the rotating-frame split step takes a constant Omega: an environment has "
                                    "a nonzero rate (pdeopt_set_env_gpe_omega_rate)");
  if (has_time_aux(ctx, PDEOPT_AUX_GPE_POTENTIAL))
    return fail(ctx, PDEOPT_EINVAL, "a potential registered through pdeopt_set_aux_time_fn is a host callable: the "
                                    "rotating-frame split step takes a static potential");
  if (!(dt > 0)) return fail(ctx, PDEOPT_EINVAL, "dt = %g", dt);
  if (!psi0_dev || !lam_dev || !grad || (uintptr_t)psi0_dev % ctx->esize || (uintptr_t)lam_dev % ctx->esize || (uintptr_t)grad % 8)
    return fail(ctx, PDEOPT_EINVAL, "psi0_dev / lam_dev are device fields [batch][nx][ny][2] in the problem dtype, grad is "
                                    "[batch][3] doubles, all aligned to their type");
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  // grad: device memory is added into by the kernel; anything else is host memory, staged through a device block
  hipPointerAttribute_t attr{};
  bool grad_on_device = false;
  if (hipPointerGetAttributes(&attr, grad) == hipSuccess) grad_on_device = attr.type == hipMemoryTypeDevice;
  else (void)hipGetLastError();  // an unregistered host pointer: not an error of the ctx
  const size_t gbytes = sizeof(double) * (size_t)p.batch * 3;
  const auto overlap = [](const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
  };
  if (overlap(lam_dev, ctx->total_bytes, psi0_dev, ctx->total_bytes) ||
      (grad_on_device && (overlap(grad, gbytes, lam_dev, ctx->total_bytes) || overlap(grad, gbytes, psi0_dev, ctx->total_bytes))))
    return fail(ctx, PDEOPT_EINVAL, "lam_dev and grad are written: they must not overlap each other or psi0_dev");
  GpeRotAdjoint& ra = ctx->features.ensure<GpeRotAdjoint>(FS_GPE_ROT_ADJOINT);
  int rc = ensure_work<false>(ctx, ra);
  if (rc) return rc;
  double* gdev = grad;
  if (!grad_on_device) {
    gdev = ra.gacc.as<double>();
    PDEOPT_HIP_CHECK(ctx, hipMemsetAsync(gdev, 0, gbytes, ctx->stream));
  }
  rc = with_dtype(ctx, [&](auto t) { return rot_adjoint_step_t<decltype(t), false>(ctx, ra, 0.0, dt, psi0_dev, lam_dev, gdev, nullptr); });
  if (rc) return rc;
  if (!grad_on_device) {
    std::vector<double> h(gbytes / sizeof(double));
    PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(h.data(), gdev, gbytes, hipMemcpyDeviceToHost, ctx->stream));
    PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < h.size(); ++i) grad[i] += h[i];
  }
  ctx->last_kernel = "strang_rot_adjoint_rocfft_1d";
  return PDEOPT_OK;
}


int pdeopt_gpe_rot_stir_adjoint_step(pdeopt_ctx* ctx, double t0, double dt, const void* psi0_dev, void* lam_dev, double* grad,
                                     double* spot_grad) {
  if (!ctx) return PDEOPT_EINVAL;
  if (!ctx->configured) return fail(ctx, PDEOPT_ESTATE, "pdeopt_configure has not been called");
  const pdeopt_problem& p = ctx->prob;
  if (p.equation != PDEOPT_EQ_GPE)
    return fail(ctx, PDEOPT_EINVAL, "the adjoint of the stirred rotating-frame split step needs the GPE");
  if (!ctx->rot_set)
    return fail(ctx, PDEOPT_ESTATE, "the adjoint of the stirred rotating-frame split step needs pdeopt_set_gpe_rotation (Omega "
                                    "and the mesh origin)");
  if (has_time_aux(ctx, PDEOPT_AUX_GPE_POTENTIAL))
    return fail(ctx, PDEOPT_EINVAL, "a potential registered through pdeopt_set_aux_time_fn is a host callable: the "
                                    "rotating-frame split step takes a static potential and Gaussian spots");
  if (ctx->n_spots && !spot_grad)
    return fail(ctx, PDEOPT_EINVAL, "%d light spots are set: spot_grad is their gradient block [batch][n_spots][7], not NULL",
                ctx->n_spots);
  if (!ctx->n_spots && spot_grad)
    return fail(ctx, PDEOPT_EINVAL, "no light spots are set (pdeopt_set_gpe_spots): spot_grad must be NULL");
  if (!(dt > 0)) return fail(ctx, PDEOPT_EINVAL, "dt = %g", dt);
  if (!std::isfinite(t0)) return fail(ctx, PDEOPT_EINVAL, "t0 = %g", t0);
  if (!psi0_dev || !lam_dev || !grad || (uintptr_t)psi0_dev % ctx->esize || (uintptr_t)lam_dev % ctx->esize ||
      (uintptr_t)grad % 8 || (uintptr_t)spot_grad % 8)
    return fail(ctx, PDEOPT_EINVAL, "psi0_dev / lam_dev are device fields [batch][nx][ny][2] in the problem dtype, grad is "
                                    "[batch][4] doubles, spot_grad [batch][n_spots][7] doubles, all aligned to their type");
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  // grad, spot_grad: device memory is added into by the kernel; anything else is host memory, staged through a device block
  const auto on_device = [](const void* ptr) {
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, ptr) == hipSuccess) return attr.type == hipMemoryTypeDevice;
    (void)hipGetLastError();  // an unregistered host pointer: not an error of the ctx
    return false;
  };
  const bool grad_on_device = on_device(grad);
  if (spot_grad && on_device(spot_grad) != grad_on_device)
    return fail(ctx, PDEOPT_EINVAL, "grad and spot_grad are both device memory or both host memory");
  const size_t gbytes = sizeof(double) * (size_t)p.batch * 4;
  const size_t sbytes = sizeof(double) * (size_t)p.batch * ctx->n_spots * 7;
  const auto overlap = [](const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
  };
  bool bad = overlap(lam_dev, ctx->total_bytes, psi0_dev, ctx->total_bytes);
  if (spot_grad) bad = bad || overlap(grad, gbytes, spot_grad, sbytes);
  if (grad_on_device) {
    bad = bad || overlap(grad, gbytes, lam_dev, ctx->total_bytes) || overlap(grad, gbytes, psi0_dev, ctx->total_bytes);
    if (spot_grad)
      bad = bad || overlap(spot_grad, sbytes, lam_dev, ctx->total_bytes) || overlap(spot_grad, sbytes, psi0_dev, ctx->total_bytes);
  }
  if (bad)
    return fail(ctx, PDEOPT_EINVAL, "lam_dev, grad and spot_grad are written: they must not overlap each other or psi0_dev");
  GpeRotAdjoint& ra = ctx->features.ensure<GpeRotAdjoint>(FS_GPE_ROT_STIR_ADJOINT);
  int rc = ensure_work<true>(ctx, ra);
  if (rc) return rc;
  double *gdev = grad, *sdev = spot_grad;
  if (!grad_on_device) {
    gdev = ra.gacc.as<double>();
    PDEOPT_HIP_CHECK(ctx, hipMemsetAsync(gdev, 0, gbytes, ctx->stream));
    if (spot_grad) {
      sdev = ra.sacc.as<double>();
      PDEOPT_HIP_CHECK(ctx, hipMemsetAsync(sdev, 0, sbytes, ctx->stream));
    }
  }
  rc = with_dtype(ctx, [&](auto t) { return rot_adjoint_step_t<decltype(t), true>(ctx, ra, t0, dt, psi0_dev, lam_dev, gdev, sdev); });
  if (rc) return rc;
  if (!grad_on_device) {
    std::vector<double> hg(gbytes / sizeof(double)), hs(sbytes / sizeof(double));
    PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(hg.data(), gdev, gbytes, hipMemcpyDeviceToHost, ctx->stream));
    if (spot_grad) PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(hs.data(), sdev, sbytes, hipMemcpyDeviceToHost, ctx->stream));
    PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < hg.size(); ++i) grad[i] += hg[i];
    if (spot_grad)
      for (size_t i = 0; i < hs.size(); ++i) spot_grad[i] += hs[i];
  }
  ctx->last_kernel = "strang_rot_stir_adjoint_rocfft_1d";
  return PDEOPT_OK;
}

}  // extern "C"
