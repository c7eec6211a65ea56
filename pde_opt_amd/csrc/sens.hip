// Forward-mode sensitivities of the Cahn-Hilliard and Allen-Cahn solves with respect to closure coefficients, and the
// Gauss-Newton sums of a least-squares fit (the reference's PDEModel.train / residuals, pde_opt/pde_model.py:138-460, which
// differentiates diffeqsolve with diffrax's ForwardMode adjoint at :410-423).
//
// Layout: the ctx is configured with batch (1 + P) B.  Environments [0, B) are the B trajectories; environment
// B + j B + b holds the tangent du/dp_j of trajectory b.  Per substep
//   IMEX   k = f(y) for the base block (launch_rhs_slope, the forward solve's own slope kernels),
//          dk_j = J_f(y) du_j + df/dp_j for the tangent block (2-D Cahn-Hilliard: sens_tangent_rhs_kernel; 3-D:
//          sens3d_dmu_kernel and sens3d_flux_kernel; Allen-Cahn: sens_ac_tangent_rhs_kernel),
//          y += dt L^-1 k over the whole (1 + P) B batch (the forward IMEX transforms): L = 1 + A dt fourier_symbol is
//          linear and independent of the closure coefficients, so their tangent of the step is the same implicit
//          solve applied to the linearised slope.  2-D power-of-two grids 64..1024 run the hand-written
//          FFT passes (4 launches + 1); other 2-D grids and the 3-D equation run the rocFFT real transforms, multiply
//          and axpy of the forward rocFFT IMEX loop.  None of the launch counts depends on P.
//          kappa (PDEOPT_SENS_KAPPA, the three periodic equations) moves L: with m = (1/n) / (1 + A dt s) and
//          s = fourier_symbol = kappa K2^2 (taken to be linear in kappa: the equation classes publish nothing else),
//            dy1 = dy0 + dt Re F^-1[ F[df] m + F[f_base] m' ],   m' = -(1/n) A dt (s / kappa) / (1 + A dt s)^2.
//          The second term couples a tangent environment to its trajectory's spectrum, which the hand-written passes
//          (two real environments packed into one complex field, multiply inside the column pass) cannot hold: with a
//          kappa role configured every grid takes the rocFFT loop, whose multiply becomes sens_imex_mul_kappa_kernel
//          (spectral.hip).  The slope kernels add d m / d kappa = -lap(u) to dmu of that tangent (template parameter
//          KAPPA; the false instantiations are the kernels of a configuration without kappa, instruction for instruction).
//   Euler  the same slope launches, then y += dt k over the whole batch.
//   RK4    (Allen-Cahn) the classical tableau over the whole batch: per stage the slope launches at the stage's base and
//          tangent values, then one pointwise update of the stage input and the accumulator -- the exact derivative of
//          the discrete step.  3 launches per stage, 12 per substep, whatever P is.
// IMEX is Cahn-Hilliard only: Allen-Cahn publishes no fourier_symbol.
// The Butler-Volmer Allen-Cahn equations (PDEOPT_EQ_ALLEN_CAHN_BV / _SBM_BV; Euler and RK4 like Allen-Cahn) take their
// tangent slopes from butler_volmer.hip (bv_sens_slopes): at constant current the voltage couples every cell of a
// trajectory, so the tangent of a slope needs 2 P more global sums -- two launches over the tangent block, whatever P is.
// The smoothed-boundary equations (PDEOPT_EQ_ALLEN_CAHN_SBM / _CAHN_HILLIARD_SBM; Euler and RK4, both of them) take theirs
// from sens_sbm.hip (sbm_sens_slopes).  They are the one time-dependent case: every slope is evaluated at its stage time
// t0 + s dt + c_i dt, the base launch resolves theta(t) and flux(t) and the tangent kernel is handed the same numbers.
//
// At a save point the tangents are reduced on the device: to the Gauss-Newton sums of a least-squares fit
// (pdeopt_sens_accumulate) or, for the gradient of a general objective J(ys) (PDEModel.optimize, pde_model.py:462-551),
// to the P contractions <dJ/dys[q], du/dp_j> (pdeopt_sens_contract).
#include <vector>

#include "closures.hpp"
#include "common.hpp"
#include "sens_tile.hpp"

namespace pdeopt {

struct Sens : Feature {
  int B = 0, P = 0;
  int role[kMaxSens] = {};   // PDEOPT_SENS_MU / PDEOPT_SENS_MOB / PDEOPT_SENS_KAPPA
  int index[kMaxSens] = {};  // coefficient k of that closure
  DeviceBuffer data;         // [n_frames][B][*spatial] observed frames or cotangents, problem dtype; grow-only
  int n_frames = 0;
  DeviceBuffer partial;      // doubles [B][K][nblk] per-block sums of the accumulation (K = P for the contraction); grow-only
  DeviceBuffer sums;         // doubles [B][K]; grow-only
  bool has_kappa = false;  // some role is PDEOPT_SENS_KAPPA: the KAPPA kernels, and IMEX through the rocFFT loop
};
// nullptr until pdeopt_sens_configure
inline Sens* sens_of(const pdeopt_ctx* ctx) { return ctx->features.get<Sens>(FS_SENS); }

namespace {

// (closure derivatives: closure_dc in closures.hpp, closure_dcoef in sens_tile.hpp)

template <typename T>
struct SensArgs {
  const T* y;  // state [(1 + P) B][nx][ny] (2-D)
  T* k;        // slopes, same layout; the kernel writes the tangent block
  const EnvParams<T>* ep;
  ClosureSpec mu, mob;
  int nx, ny, B, P;
  T rhx, rhy, rhx2, rhy2;
  int role[kMaxSens];
  int index[kMaxSens];
};

// Tangent-linear right-hand side of Cahn-Hilliard with FD derivatives (cahn_hilliard.py:89-109):
//   f       = div( avg(D(u)) grad(mu) ),                 mu = mu_h(u) - kappa lap u
//   dmu_j   = mu_h'(u) du_j + dmu_h/dp_j - kappa lap du_j
//   dD_j    = D'(u) du_j + dD/dp_j
//   df_j    = div( avg(dD_j) grad(mu) + avg(D) grad(dmu_j) )
// with the forward kernel's primitives: 5-point Laplacian, face gradients, face averages, face divergence.
// One workgroup per (tile, trajectory): u, mu, D and their derivatives are formed once, then the P tangents are
// streamed through the same LDS tile (each tangent field read once, each tangent slope written once).
// KAPPA: some role is PDEOPT_SENS_KAPPA; that tangent's direct term is dmu += d(mu_h - kappa lap u)/dkappa = -lap5(u),
// recomputed from su, which is still resident (one more LDS array would take the fp64 kernel from 45.8 to 50.7 KB).
template <typename T, bool KAPPA>
__global__ __launch_bounds__(256) void sens_tangent_rhs_kernel(SensArgs<T> a) {
  __shared__ T su[kR2 * kC2], sdu[kR2 * kC2];
  __shared__ T smu[kR1 * kC1], smuh[kR1 * kC1], sD[kR1 * kC1], smu1[kR1 * kC1], sD1[kR1 * kC1];
  __shared__ T sdmu[kR1 * kC1], sdD[kR1 * kC1];
  const int tid = threadIdx.x;
  const int b = blockIdx.z;
  const int i0 = blockIdx.y * kTR, j0 = blockIdx.x * kTC;
  const int nx = a.nx, ny = a.ny;
  const int64_t cells = (int64_t)nx * ny;
  const EnvParams<T>& ep = a.ep[b];
  const T kappa = ep.kappa;
  const T* __restrict__ u = a.y + (int64_t)b * cells;
  for (int q = tid; q < kR2 * kC2; q += 256) {
    const int r = q / kC2, c = q - r * kC2;
    su[q] = u[(int64_t)wrap_idx(i0 + r - 2, nx) * ny + wrap_idx(j0 + c - 2, ny)];
  }
  __syncthreads();
  for (int q = tid; q < kR1 * kC1; q += 256) {
    const int r = q / kC1, c = q - r * kC1;
    const int o = (r + 1) * kC2 + (c + 1);
    const T uc = su[o];
    const T lap = (su[o + kC2] - T(2) * uc + su[o - kC2]) * a.rhx2 + (su[o + 1] - T(2) * uc + su[o - 1]) * a.rhy2;
    const T muh = closure_generic<T>(a.mu, ep.mu, uc);
    const T D = closure_generic<T>(a.mob, ep.mob, uc);
    smuh[q] = muh;
    smu[q] = muh - kappa * lap;
    sD[q] = D;
    smu1[q] = closure_dc<T>(a.mu, ep.mu, uc, muh);
    sD1[q] = closure_dc<T>(a.mob, ep.mob, uc, D);
  }
  for (int j = 0; j < a.P; ++j) {
    __syncthreads();  // the previous tangent's readers are done with sdu / sdmu / sdD (and the base arrays are written)
    const int64_t env = (int64_t)a.B + (int64_t)j * a.B + b;
    const T* __restrict__ du = a.y + env * cells;
    for (int q = tid; q < kR2 * kC2; q += 256) {
      const int r = q / kC2, c = q - r * kC2;
      sdu[q] = du[(int64_t)wrap_idx(i0 + r - 2, nx) * ny + wrap_idx(j0 + c - 2, ny)];
    }
    __syncthreads();
    const bool on_mu = a.role[j] == PDEOPT_SENS_MU;
    const bool on_kappa = KAPPA && a.role[j] == PDEOPT_SENS_KAPPA;
    const int kc = a.index[j];
    for (int q = tid; q < kR1 * kC1; q += 256) {
      const int r = q / kC1, c = q - r * kC1;
      const int o = (r + 1) * kC2 + (c + 1);
      const T uc = su[o], d = sdu[o];
      const T lap = (sdu[o + kC2] - T(2) * d + sdu[o - kC2]) * a.rhx2 + (sdu[o + 1] - T(2) * d + sdu[o - 1]) * a.rhy2;
      T dmu = smu1[q] * d - kappa * lap;
      T dD = sD1[q] * d;
      if (on_mu) dmu += closure_dcoef<T>(a.mu, kc, uc, smuh[q]);
      else if (on_kappa) dmu -= (su[o + kC2] - T(2) * uc + su[o - kC2]) * a.rhx2 + (su[o + 1] - T(2) * uc + su[o - 1]) * a.rhy2;
      else dD += closure_dcoef<T>(a.mob, kc, uc, sD[q]);
      sdmu[q] = dmu;
      sdD[q] = dD;
    }
    __syncthreads();
    T* __restrict__ out = a.k + env * cells;
    for (int q = tid; q < kTR * kTC; q += 256) {
      const int r = q / kTC, c = q - r * kTC;
      const int gi = i0 + r, gj = j0 + c;
      if (gi >= nx || gj >= ny) continue;
      const int o = (r + 1) * kC1 + (c + 1);
      const int xp = o + kC1, xm = o - kC1, yp = o + 1, ym = o - 1;
      // faces +-1/2 along x (axis 0) and y (axis 1): avg(dD) grad(mu) + avg(D) grad(dmu)
      const T fxp = T(0.5) * (sdD[o] + sdD[xp]) * ((smu[xp] - smu[o]) * a.rhx) +
                    T(0.5) * (sD[o] + sD[xp]) * ((sdmu[xp] - sdmu[o]) * a.rhx);
      const T fxm = T(0.5) * (sdD[xm] + sdD[o]) * ((smu[o] - smu[xm]) * a.rhx) +
                    T(0.5) * (sD[xm] + sD[o]) * ((sdmu[o] - sdmu[xm]) * a.rhx);
      const T fyp = T(0.5) * (sdD[o] + sdD[yp]) * ((smu[yp] - smu[o]) * a.rhy) +
                    T(0.5) * (sD[o] + sD[yp]) * ((sdmu[yp] - sdmu[o]) * a.rhy);
      const T fym = T(0.5) * (sdD[ym] + sdD[o]) * ((smu[o] - smu[ym]) * a.rhy) +
                    T(0.5) * (sD[ym] + sD[o]) * ((sdmu[o] - sdmu[ym]) * a.rhy);
      out[(int64_t)gi * ny + gj] = (fxp - fxm) * a.rhx + (fyp - fym) * a.rhy;
    }
  }
}

// ---- Allen-Cahn (allen_cahn.py:81-84; the forward kernels' EQ_ALLEN_CAHN with derivs = "fd") ----------------------
//   f     = -R(u) m,                                     m = mu_h(u) - kappa lap5(u)
//   df_j  = -(R'(u) du_j + dR/dp_j) m - R(u) (mu_h'(u) du_j + dmu_h/dp_j - kappa lap5(du_j))
// One workgroup per (tile, trajectory), as the Cahn-Hilliard kernel above; the stencil has radius 1, so only u and du_j
// are staged in LDS (tile + 1-cell ring) and everything else a cell needs -- u, mu_h, m, R, R', mu_h' -- stays in the
// registers of the thread that owns it.  A thread owns two neighbouring cells of a row.  Each tangent field is read
// from HBM once and each tangent slope written once; per tangent only the basis function of closure_dcoef is evaluated.
// KAPPA: the base Laplacian of the thread's two cells stays in registers too; the kappa tangent's dmu += -lap5(u).
template <typename T>
struct AcTile {
  static constexpr int V = 16 / (int)sizeof(T);  // cells per 16-byte vector
  static constexpr int kRows = kTR + 2;
  static constexpr int kLd = kTC + 2 * V;        // the tile's first column sits at V: 16-byte aligned rows in LDS
  static constexpr int kSize = kRows * kLd;
};
template <typename T> struct AcVec;
template <> struct AcVec<float> { using type = float4; };
template <> struct AcVec<double> { using type = double2; };

// s[(r, V - 1 + c)] = f[wrap(i0 - 1 + r), wrap(j0 - 1 + c)] for r < kTR + 2, c < kTC + 2.  Tiles whose kTC columns lie
// inside an aligned row (`wide`) take them as 16-byte row loads and only the two ring columns as single cells.
template <typename T>
__device__ __forceinline__ void ac_stage(T* __restrict__ s, const T* __restrict__ f, int i0, int j0, int nx, int ny,
                                         bool wide, int tid) {
  using A = AcTile<T>;
  using Vec = typename AcVec<T>::type;
  if (wide) {
    constexpr int kVecRow = kTC / A::V;
    for (int q = tid; q < A::kRows * kVecRow; q += 256) {
      const int r = q / kVecRow, c = (q - r * kVecRow) * A::V;
      const int64_t row = (int64_t)wrap_idx(i0 + r - 1, nx) * ny;
      *reinterpret_cast<Vec*>(s + r * A::kLd + A::V + c) = *reinterpret_cast<const Vec*>(f + row + j0 + c);
    }
    for (int q = tid; q < 2 * A::kRows; q += 256) {
      const int r = q >> 1, right = q & 1;
      const int64_t row = (int64_t)wrap_idx(i0 + r - 1, nx) * ny;
      s[r * A::kLd + (right ? A::V + kTC : A::V - 1)] = f[row + wrap_idx(right ? j0 + kTC : j0 - 1, ny)];
    }
  } else {
    for (int q = tid; q < A::kRows * kC1; q += 256) {
      const int r = q / kC1, c = q - r * kC1;
      s[r * A::kLd + A::V - 1 + c] = f[(int64_t)wrap_idx(i0 + r - 1, nx) * ny + wrap_idx(j0 + c - 1, ny)];
    }
  }
}

template <typename T, bool KAPPA>
__global__ __launch_bounds__(256) void sens_ac_tangent_rhs_kernel(SensArgs<T> a) {
  using A = AcTile<T>;
  __shared__ __attribute__((aligned(16))) T su[A::kSize];
  __shared__ __attribute__((aligned(16))) T sdu[A::kSize];
  const int tid = threadIdx.x;
  const int b = blockIdx.z;
  const int i0 = blockIdx.y * kTR, j0 = blockIdx.x * kTC;
  const int nx = a.nx, ny = a.ny;
  const int64_t cells = (int64_t)nx * ny;
  const EnvParams<T>& ep = a.ep[b];
  const T kappa = ep.kappa;
  const bool wide = ny % A::V == 0 && j0 + kTC <= ny;
  // this thread's cells: row r, columns c and c + 1 of the tile
  const int r = tid >> 4, c = (tid & 15) * 2;
  const int gi = i0 + r, gj = j0 + c;
  const int o = (r + 1) * A::kLd + A::V + c;
  ac_stage<T>(su, a.y + (int64_t)b * cells, i0, j0, nx, ny, wide, tid);
  __syncthreads();
  T uc[2], muh[2], m[2], R[2], R1[2], mu1[2];
  T lapu[2];  // KAPPA only
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int q = o + e;
    uc[e] = su[q];
    const T lap = (su[q + A::kLd] - T(2) * uc[e] + su[q - A::kLd]) * a.rhx2 + (su[q + 1] - T(2) * uc[e] + su[q - 1]) * a.rhy2;
    if constexpr (KAPPA) lapu[e] = lap;
    muh[e] = closure_generic<T>(a.mu, ep.mu, uc[e]);
    m[e] = muh[e] - kappa * lap;
    R[e] = closure_generic<T>(a.mob, ep.mob, uc[e]);
    mu1[e] = closure_dc<T>(a.mu, ep.mu, uc[e], muh[e]);
    R1[e] = closure_dc<T>(a.mob, ep.mob, uc[e], R[e]);
  }
  for (int j = 0; j < a.P; ++j) {
    if (j) __syncthreads();  // the previous tangent's readers are done with sdu
    const int64_t env = (int64_t)a.B + (int64_t)j * a.B + b;
    ac_stage<T>(sdu, a.y + env * cells, i0, j0, nx, ny, wide, tid);
    __syncthreads();
    const bool on_mu = a.role[j] == PDEOPT_SENS_MU;
    const bool on_kappa = KAPPA && a.role[j] == PDEOPT_SENS_KAPPA;
    const int kc = a.index[j];
    T df[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int q = o + e;
      const T d = sdu[q];
      const T lap = (sdu[q + A::kLd] - T(2) * d + sdu[q - A::kLd]) * a.rhx2 + (sdu[q + 1] - T(2) * d + sdu[q - 1]) * a.rhy2;
      T dmu = mu1[e] * d - kappa * lap;
      T dR = R1[e] * d;
      if (on_mu) dmu += closure_dcoef<T>(a.mu, kc, uc[e], muh[e]);
      else if constexpr (KAPPA) {
        if (on_kappa) dmu -= lapu[e];
        else dR += closure_dcoef<T>(a.mob, kc, uc[e], R[e]);
      } else dR += closure_dcoef<T>(a.mob, kc, uc[e], R[e]);
      df[e] = -(dR * m[e]) - R[e] * dmu;
    }
    T* __restrict__ out = a.k + env * cells + (int64_t)gi * ny + gj;
    if (gi < nx) {
      if (ny % 2 == 0 && gj + 1 < ny) {
        if constexpr (sizeof(T) == 4) *reinterpret_cast<float2*>(out) = make_float2(df[0], df[1]);
        else *reinterpret_cast<double2*>(out) = make_double2(df[0], df[1]);
      } else {
        if (gj < ny) out[0] = df[0];
        if (gj + 1 < ny) out[1] = df[1];
      }
    }
  }
}

// ---- 3-D: CahnHilliard3DPeriodic.rhs_fd (cahn_hilliard.py:180-200), fields [env][nx][ny][nz] with z contiguous ----
// Two passes, as the forward ch3d_mu_kernel / ch3d_stage_kernel (stencil_generic.hpp), with their primitives in their
// order: 7-point Laplacian, face gradients, face averages, face divergence.
//   pass 1  dmu_j = mu_h'(u) du_j + [role_j == MU] dmu_h/dp_j - [role_j == KAPPA] lap7(u) - kappa lap7(du_j)  -> the work
//           field KS at the tangent environments (the base slope launch has left the base mu in KS[0, B)); lap7(u), six
//           more reads, is formed once before the loop and only in the KAPPA instantiation
//   pass 2  df_j = div( avg_face(dD_j) grad_face(mu) + avg_face(D) grad_face(dmu_j) ),  dD_j = D'(u) du_j + [MOB] dD/dp_j
// One thread per cell and trajectory, flat over the cells (a 32^3 field fills every lane); the values of u at the
// stencil points (mu_h', or D and D' at the 7 points) are formed once and the thread then walks the P tangents.
template <typename T>
struct Sens3Args {
  const T* y;  // state [(1 + P) B][nx][ny][nz]
  T* w;        // work field KS, same layout: base mu in [0, B), pass 1 writes dmu_j at the tangent environments
  T* k;        // slopes TA, same layout; pass 2 writes the tangent block
  const EnvParams<T>* ep;
  ClosureSpec mu, mob;
  int nx, ny, nz, B, P;
  T rhx, rhy, rhz, rhx2, rhy2, rhz2;
  int role[kMaxSens];
  int index[kMaxSens];
};

// offsets (within one environment) of cell c and its 6 periodic neighbours: 0 = c, then +x, -x, +y, -y, +z, -z
template <typename T>
__device__ __forceinline__ void nb7(const Sens3Args<T>& a, int c, int o[7]) {
  const int nz = a.nz, ny = a.ny, nx = a.nx;
  const int k = c % nz, q = c / nz;
  const int j = q % ny, i = q / ny;
  const int syz = ny * nz;
  o[0] = c;
  o[1] = c + (i + 1 == nx ? -(nx - 1) * syz : syz);
  o[2] = c + (i == 0 ? (nx - 1) * syz : -syz);
  o[3] = c + (j + 1 == ny ? -(ny - 1) * nz : nz);
  o[4] = c + (j == 0 ? (ny - 1) * nz : -nz);
  o[5] = c + (k + 1 == nz ? -(nz - 1) : 1);
  o[6] = c + (k == 0 ? nz - 1 : -1);
}

// grid (cells / 256, B)
template <typename T, bool KAPPA>
__global__ __launch_bounds__(256) void sens3d_dmu_kernel(Sens3Args<T> a) {
  const int cells = a.nx * a.ny * a.nz;
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (c >= cells) return;
  int o[7];
  nb7<T>(a, c, o);
  const EnvParams<T>& ep = a.ep[b];
  const T kappa = ep.kappa;
  const T uc = a.y[(int64_t)b * cells + c];
  const T muh = closure_generic<T>(a.mu, ep.mu, uc);
  const T mu1 = closure_dc<T>(a.mu, ep.mu, uc, muh);
  T lapu = T(0);
  if constexpr (KAPPA) {
    const T* __restrict__ u = a.y + (int64_t)b * cells;
    lapu = (u[o[1]] - T(2) * uc + u[o[2]]) * a.rhx2 + (u[o[3]] - T(2) * uc + u[o[4]]) * a.rhy2 +
           (u[o[5]] - T(2) * uc + u[o[6]]) * a.rhz2;
  }
  for (int j = 0; j < a.P; ++j) {
    const int64_t env = (int64_t)a.B + (int64_t)j * a.B + b;
    const T* __restrict__ du = a.y + env * cells;
    const T d = du[o[0]];
    const T lap = (du[o[1]] - T(2) * d + du[o[2]]) * a.rhx2 + (du[o[3]] - T(2) * d + du[o[4]]) * a.rhy2 +
                  (du[o[5]] - T(2) * d + du[o[6]]) * a.rhz2;
    T dmu = mu1 * d - kappa * lap;
    if (a.role[j] == PDEOPT_SENS_MU) dmu += closure_dcoef<T>(a.mu, a.index[j], uc, muh);
    else if (KAPPA && a.role[j] == PDEOPT_SENS_KAPPA) dmu -= lapu;
    a.w[env * cells + c] = dmu;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void sens3d_flux_kernel(Sens3Args<T> a) {
  const int cells = a.nx * a.ny * a.nz;
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (c >= cells) return;
  int o[7];
  nb7<T>(a, c, o);
  const EnvParams<T>& ep = a.ep[b];
  const T* __restrict__ u = a.y + (int64_t)b * cells;
  const T* __restrict__ m = a.w + (int64_t)b * cells;
  T uu[7], D[7], D1[7], mm[7];
#pragma unroll
  for (int q = 0; q < 7; ++q) {
    uu[q] = u[o[q]];
    mm[q] = m[o[q]];
    D[q] = closure_generic<T>(a.mob, ep.mob, uu[q]);
    D1[q] = closure_dc<T>(a.mob, ep.mob, uu[q], D[q]);
  }
  const T rh[3] = {a.rhx, a.rhy, a.rhz};
  for (int j = 0; j < a.P; ++j) {
    const int64_t env = (int64_t)a.B + (int64_t)j * a.B + b;
    const T* __restrict__ du = a.y + env * cells;
    const T* __restrict__ dm = a.w + env * cells;
    const bool on_mob = a.role[j] == PDEOPT_SENS_MOB;
    const int kc = a.index[j];
    T dD[7], dmu[7];
#pragma unroll
    for (int q = 0; q < 7; ++q) {
      dmu[q] = dm[o[q]];
      dD[q] = D1[q] * du[o[q]];
      if (on_mob) dD[q] += closure_dcoef<T>(a.mob, kc, uu[q], D[q]);
    }
    // faces +-1/2 along x, y, z: avg(dD) grad(mu) + avg(D) grad(dmu), then the face divergence
    T kk = T(0);
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      const int p = 1 + 2 * ax, n = 2 + 2 * ax;
      const T fp = T(0.5) * (dD[0] + dD[p]) * ((mm[p] - mm[0]) * rh[ax]) +
                   T(0.5) * (D[0] + D[p]) * ((dmu[p] - dmu[0]) * rh[ax]);
      const T fm = T(0.5) * (dD[n] + dD[0]) * ((mm[0] - mm[n]) * rh[ax]) +
                   T(0.5) * (D[n] + D[0]) * ((dmu[0] - dmu[n]) * rh[ax]);
      kk += (fp - fm) * rh[ax];
    }
    a.k[env * cells + c] = kk;
  }
}

template <typename T>
__global__ void sens_axpy_kernel(T* __restrict__ y, const T* __restrict__ k, T dt, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    y[i] += dt * k[i];
}

// One RK4 stage update of the whole batch, with the forward stage kernels' expressions (stage_update):
//   mode 0 (stage 1)     next = y + a k,  acc = y + b k
//   mode 1 (stages 2, 3) next = y + a k,  acc += b k
//   mode 2 (stage 4)     y = acc + b k
template <typename T>
__global__ void sens_rk4_update_kernel(T* __restrict__ y, const T* __restrict__ k, T* __restrict__ next, T* __restrict__ acc,
                                       T a, T b, int mode, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const T ki = k[i];
    if (mode == 2) {
      y[i] = acc[i] + b * ki;
    } else {
      const T yi = y[i];
      acc[i] = (mode == 0 ? yi : acc[i]) + b * ki;
      next[i] = yi + a * ki;
    }
  }
}

// ---- Gauss-Newton sums at one save point ------------------------------------------------------------------------
// Rows: 0 = the residual r = v - pred, 1..P = the tangent dpred_j; pred = snap + theta (y - snap) (the lerp of
// pdeopt_get_interpolated) or y.  Output index of the product of rows i <= j:
//   i = 0:  j (0 = sum r^2, j = sum r dpred_j);   i >= 1: 1 + P + the upper-triangle index of (i - 1, j - 1).
constexpr int kGnThreads = 256, kGnCellsPerThread = 8, kGnCellsPerBlock = kGnThreads * kGnCellsPerThread;

__host__ __device__ __forceinline__ int gn_index(int i, int j, int P) {
  if (i == 0) return j;
  const int a = i - 1, c = j - 1;
  return 1 + P + a * P - a * (a - 1) / 2 + (c - a);
}

template <typename T>
__device__ __forceinline__ double gn_row(const T* __restrict__ y, const T* __restrict__ snap, const T* __restrict__ v,
                                         int row, int b, int B, int64_t cells, int64_t c, T theta, int interp) {
  const int64_t env = row == 0 ? b : (int64_t)B + (int64_t)(row - 1) * B + b;
  const int64_t o = env * cells + c;
  const T p = interp ? snap[o] + theta * (y[o] - snap[o]) : y[o];
  return row == 0 ? (double)v[(int64_t)b * cells + c] - (double)p : (double)p;
}

// grid (blocks per field, B, 1 + P): block (x, b, i) sums row i times rows j >= i over its 2048 cells of trajectory
// b; the block total (fixed-order tree in LDS) goes to partial[b][index][x].  No atomics: repeated calls give the
// same bits.
template <typename T>
__global__ __launch_bounds__(kGnThreads) void sens_gn_partial_kernel(const T* __restrict__ y, const T* __restrict__ snap,
                                                                   const T* __restrict__ v, double* __restrict__ partial,
                                                                   int B, int P, int64_t cells, T theta, int interp) {
  __shared__ double red[kGnThreads];
  const int tid = threadIdx.x, blk = blockIdx.x, b = blockIdx.y, i = blockIdx.z;
  const int nblk = gridDim.x, K = 1 + P + P * (P + 1) / 2;
  const int64_t c0 = (int64_t)blk * kGnCellsPerBlock + tid;
  double av[kGnCellsPerThread];
#pragma unroll
  for (int m = 0; m < kGnCellsPerThread; ++m) {
    const int64_t c = c0 + (int64_t)m * kGnThreads;
    av[m] = c < cells ? gn_row<T>(y, snap, v, i, b, B, cells, c, theta, interp) : 0.0;
  }
  for (int j = i; j <= P; ++j) {
    double acc = 0.0;
#pragma unroll
    for (int m = 0; m < kGnCellsPerThread; ++m) {
      const int64_t c = c0 + (int64_t)m * kGnThreads;
      if (c < cells) acc += av[m] * (j == i ? av[m] : gn_row<T>(y, snap, v, j, b, B, cells, c, theta, interp));
    }
    red[tid] = acc;
    __syncthreads();
    for (int s = kGnThreads / 2; s > 0; s >>= 1) {
      if (tid < s) red[tid] += red[tid + s];
      __syncthreads();
    }
    if (tid == 0) partial[((int64_t)b * K + gn_index(i, j, P)) * nblk + blk] = red[0];
    __syncthreads();
  }
}

// sums[b][k] = sum over blocks of partial[b][k][.], in block order
__global__ void sens_gn_final_kernel(const double* __restrict__ partial, double* __restrict__ sums, int n, int nblk) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  const double* p = partial + (int64_t)q * nblk;
  double s = 0.0;
  for (int x = 0; x < nblk; ++x) s += p[x];
  sums[q] = s;
}

// ---- contraction of a cotangent field with the tangents at one save point (PDEModel.optimize) ---------------------
// grid (blocks per field, B): block (x, b) reads its 2048 cells of g[b] once, keeps them in registers and streams the
// P tangent fields dpred_j past them (gn_row, rows 1..P: the state or the lerp of pdeopt_get_interpolated); the block
// total of g dpred_j (the same fixed-order tree in LDS) goes to partial[b][j][x].  O(P) reads per cell, no atomics.
template <typename T>
__global__ __launch_bounds__(kGnThreads) void sens_contract_partial_kernel(const T* __restrict__ y, const T* __restrict__ snap,
                                                                         const T* __restrict__ g, double* __restrict__ partial,
                                                                         int B, int P, int64_t cells, T theta, int interp) {
  __shared__ double red[kGnThreads];
  const int tid = threadIdx.x, blk = blockIdx.x, b = blockIdx.y;
  const int nblk = gridDim.x;
  const int64_t c0 = (int64_t)blk * kGnCellsPerBlock + tid;
  double gv[kGnCellsPerThread];
#pragma unroll
  for (int m = 0; m < kGnCellsPerThread; ++m) {
    const int64_t c = c0 + (int64_t)m * kGnThreads;
    gv[m] = c < cells ? (double)g[(int64_t)b * cells + c] : 0.0;
  }
  for (int j = 1; j <= P; ++j) {
    double acc = 0.0;
#pragma unroll
    for (int m = 0; m < kGnCellsPerThread; ++m) {
      const int64_t c = c0 + (int64_t)m * kGnThreads;
      if (c < cells) acc += gv[m] * gn_row<T>(y, snap, g, j, b, B, cells, c, theta, interp);
    }
    red[tid] = acc;
    __syncthreads();
    for (int s = kGnThreads / 2; s > 0; s >>= 1) {
      if (tid < s) red[tid] += red[tid + s];
      __syncthreads();
    }
    if (tid == 0) partial[((int64_t)b * P + (j - 1)) * nblk + blk] = red[0];
    __syncthreads();
  }
}

// cells of one environment: nx ny, or nx ny nz for the 3-D equation
inline int64_t sens_cells(const pdeopt_ctx* ctx) {
  const pdeopt_problem& p = ctx->prob;
  return (int64_t)p.nx * p.ny * (p.nz > 1 ? p.nz : 1);
}

// the equations whose tangent kernels have the kappa term
inline bool sens_kappa_equation(const pdeopt_problem& p) {
  return (p.equation == PDEOPT_EQ_CAHN_HILLIARD && p.nz <= 1) || p.equation == PDEOPT_EQ_CAHN_HILLIARD_3D ||
         (p.equation == PDEOPT_EQ_ALLEN_CAHN && p.nz <= 1);
}

// A kappa role differentiates with respect to ONE scalar: the B trajectories must share it (as mobility coefficients
// that differ between environments are refused).  *kappa: that value in double -- the problem's own when the
// environments still hold it, else what pdeopt_set_env_params gave them
int sens_kappa_check(pdeopt_ctx* ctx, int B, double* kappa) {
  const pdeopt_problem& p = ctx->prob;
  if (!sens_kappa_equation(p))
    return fail(ctx, PDEOPT_EINVAL, "PDEOPT_SENS_KAPPA belongs to the periodic 2-D / 3-D Cahn-Hilliard and the periodic 2-D "
                                    "Allen-Cahn equations: the smoothed-boundary and Butler-Volmer tangent kernels have no kappa "
                                    "term (equation %d)", p.equation);
  return with_dtype(ctx, [&](auto t) {
    using T = decltype(t);
    const auto* e = reinterpret_cast<const EnvParams<T>*>(ctx->env_params_host.data());
    for (int b = 1; b < B; ++b)
      if (e[b].kappa != e[0].kappa)
        return fail(ctx, PDEOPT_EINVAL, "PDEOPT_SENS_KAPPA: trajectory %d has kappa = %g, trajectory 0 has %g; the derivative is "
                                        "of one scalar shared by the trajectories", b, (double)e[b].kappa, (double)e[0].kappa);
    if (!(e[0].kappa != T(0)))
      return fail(ctx, PDEOPT_EINVAL, "PDEOPT_SENS_KAPPA: kappa = %g (the implicit operator's derivative divides the symbol by it)",
                  (double)e[0].kappa);
    if (kappa) *kappa = T(p.kappa) == e[0].kappa ? p.kappa : (double)e[0].kappa;
    return (int)PDEOPT_OK;
  });
}

int check_sens(pdeopt_ctx* ctx) {
  if (!ctx->configured) return fail(ctx, PDEOPT_ESTATE, "pdeopt_configure has not been called");
  const Sens* s = sens_of(ctx);
  if (!s) return fail(ctx, PDEOPT_ESTATE, "pdeopt_sens_configure has not been called");
  if ((int64_t)(1 + s->P) * s->B != ctx->prob.batch)
    return fail(ctx, PDEOPT_ESTATE, "batch %d is not (1 + P) B = %d: configure again before pdeopt_sens_configure",
                ctx->prob.batch, (1 + s->P) * s->B);
  for (int j = 0; j < s->P; ++j) {
    if (s->role[j] == PDEOPT_SENS_KAPPA) continue;  // a scalar: no closure behind it (sens_kappa_check below)
    const pdeopt_closure& cl = s->role[j] == PDEOPT_SENS_MU ? ctx->prob.mu : ctx->prob.mob;
    if (s->index[j] >= cl.n)
      return fail(ctx, PDEOPT_EINVAL, "sensitivity %d: coefficient %d of a closure with %d coefficients", j, s->index[j], cl.n);
  }
  return s->has_kappa ? sens_kappa_check(ctx, s->B, nullptr) : PDEOPT_OK;
}

// the members SensArgs and Sens3Args share
template <typename T, typename Args>
void fill_tangent_args(Args& a, const pdeopt_ctx* ctx, const void* in, void* out) {
  const pdeopt_problem& p = ctx->prob;
  const Sens& s = *sens_of(ctx);
  a.y = static_cast<const T*>(in);
  a.k = static_cast<T*>(out);
  set_closures<T>(a, ctx, 0);
  a.nx = p.nx;
  a.ny = p.ny;
  a.B = s.B;
  a.P = s.P;
  set_recip_plain(a, grid_recip(p));
  for (int j = 0; j < s.P; ++j) {
    a.role[j] = s.role[j];
    a.index[j] = s.index[j];
  }
}

template <typename T>
int launch_tangent_rhs(pdeopt_ctx* ctx, const void* in, void* out) {
  const pdeopt_problem& p = ctx->prob;
  SensArgs<T> a{};
  fill_tangent_args<T>(a, ctx, in, out);
  const dim3 grid((p.ny + kTC - 1) / kTC, (p.nx + kTR - 1) / kTR, a.B);
  // the KAPPA instantiations only when a kappa role is configured: every other fit runs the kernels it always ran
  const bool kap = sens_of(ctx)->has_kappa;
  if (p.equation == PDEOPT_EQ_ALLEN_CAHN) {
    if (kap) hipLaunchKernelGGL((sens_ac_tangent_rhs_kernel<T, true>), grid, dim3(256), 0, ctx->stream, a);
    else hipLaunchKernelGGL((sens_ac_tangent_rhs_kernel<T, false>), grid, dim3(256), 0, ctx->stream, a);
  } else {
    if (kap) hipLaunchKernelGGL((sens_tangent_rhs_kernel<T, true>), grid, dim3(256), 0, ctx->stream, a);
    else hipLaunchKernelGGL((sens_tangent_rhs_kernel<T, false>), grid, dim3(256), 0, ctx->stream, a);
  }
  ctx->n_stage_launches++;
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  return PDEOPT_OK;
}

// the two 3-D passes over the tangent block; the base slope launch has left the base mu in KS[0, B)
template <typename T>
int launch_tangent_rhs3d(pdeopt_ctx* ctx, const void* in, void* out) {
  int rc;
  if ((rc = ensure_buffer(ctx, ctx->KS, ctx->total_bytes))) return rc;
  const GridRecip r = grid_recip(ctx->prob);
  Sens3Args<T> a{};
  fill_tangent_args<T>(a, ctx, in, out);
  a.w = ctx->KS.as<T>();
  a.nz = ctx->prob.nz;
  a.rhz = T(r.rz);
  a.rhz2 = T(r.rz2);
  const dim3 grid((unsigned)((sens_cells(ctx) + 255) / 256), a.B);
  if (sens_of(ctx)->has_kappa) hipLaunchKernelGGL((sens3d_dmu_kernel<T, true>), grid, dim3(256), 0, ctx->stream, a);
  else hipLaunchKernelGGL((sens3d_dmu_kernel<T, false>), grid, dim3(256), 0, ctx->stream, a);
  hipLaunchKernelGGL(sens3d_flux_kernel<T>, grid, dim3(256), 0, ctx->stream, a);
  ctx->n_stage_launches += 2;
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  return PDEOPT_OK;
}

// out = (f(t, y_base), J_f du_j + df/dp_j) of the whole batch `in` (the state, or an RK4 stage value).  t matters to the
// smoothed-boundary equations only (theta(t), flux(t)); callers pass 0.0 for the autonomous ones
int sens_slopes(pdeopt_ctx* ctx, const void* in, void* out, double t) {
  int rc;
  // the base block's slope; the tangent blocks' slopes come from the kernels below
  if ((rc = launch_rhs_slope(ctx, Window{0, sens_of(ctx)->B, ctx->stream}, in, out, t))) return rc;
  if (sbm_equation(ctx->prob.equation)) {
    // the tangent kernel reads the time terms that launch resolved (ctx->time_last): the same numbers, whatever their source
    const Sens& s = *sens_of(ctx);
    return sbm_sens_slopes(ctx, BvSensSpec{s.B, s.P, s.role, s.index}, in, out);
  }
  if (bv_equation(ctx->prob.equation)) {
    const Sens& s = *sens_of(ctx);
    return bv_sens_slopes(ctx, BvSensSpec{s.B, s.P, s.role, s.index}, in, out);
  }
  return with_dtype(ctx, [&](auto t) {
    using T = decltype(t);
    return ctx->prob.equation == PDEOPT_EQ_CAHN_HILLIARD_3D ? launch_tangent_rhs3d<T>(ctx, in, out) : launch_tangent_rhs<T>(ctx, in, out);
  });
}

template <typename T>
int euler_update(pdeopt_ctx* ctx, double dt) {
  const int64_t n = (int64_t)ctx->env_elems * ctx->prob.batch;
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(sens_axpy_kernel<T>, dim3(blocks), dim3(256), 0, ctx->stream, ctx->Y.as<T>(),
                     ctx->TA.as<const T>(), (T)dt, n);
  ctx->n_stage_launches++;
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  return PDEOPT_OK;
}

// One classical RK4 substep of the whole (1 + P) B batch: K = TA, stage input TB, accumulator ACC.  ts: the substep's
// start time for the time-dependent equations (stage times ts, ts + dt / 2, ts + dt / 2, ts + dt, formed as
// advance_explicit forms them), `timed` false: every stage passes 0.0
template <typename T>
int rk4_substep(pdeopt_ctx* ctx, double dt, double ts, bool timed) {
  const int64_t n = (int64_t)ctx->env_elems * ctx->prob.batch;
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
  T* const y = ctx->Y.as<T>();
  T* const k = ctx->TA.as<T>();
  T* const in = ctx->TB.as<T>();
  T* const acc = ctx->ACC.as<T>();
  const double a[4] = {dt / 2, dt / 2, dt, 0.0}, b[4] = {dt / 6, dt / 3, dt / 3, dt / 6};
  const double tst[4] = {ts, ts + dt / 2, ts + dt / 2, ts + dt};
  for (int st = 0; st < 4; ++st) {
    int rc;
    if ((rc = sens_slopes(ctx, st == 0 ? y : in, k, timed ? tst[st] : 0.0))) return rc;
    hipLaunchKernelGGL(sens_rk4_update_kernel<T>, dim3(blocks), dim3(256), 0, ctx->stream, y, static_cast<const T*>(k), in, acc,
                       (T)a[st], (T)b[st], st == 0 ? 0 : (st == 3 ? 2 : 1), n);
    ctx->n_stage_launches++;
  }
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  return PDEOPT_OK;
}

// the buffers of the two-stage reductions below: partial[B][K][nblk] and sums[B][K]
int ensure_sums(pdeopt_ctx* ctx, int K, int nblk) {
  Sens& s = *sens_of(ctx);
  const size_t pbytes = (size_t)s.B * K * nblk * sizeof(double), sbytes = (size_t)s.B * K * sizeof(double);
  const int rc = grow_device_buffer(ctx, s.partial, pbytes, /*sync_first=*/true);
  return rc ? rc : grow_device_buffer(ctx, s.sums, sbytes, /*sync_first=*/true);
}

// sums[b][k] = the block totals of partial[b][k][.] in block order, copied to the host
int finish_sums(pdeopt_ctx* ctx, int K, int nblk, double* host_out) {
  Sens& s = *sens_of(ctx);
  const int n = s.B * K;
  hipLaunchKernelGGL(sens_gn_final_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, s.partial.as<double>(), s.sums.as<double>(), n, nblk);
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(host_out, s.sums.as<double>(), (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PDEOPT_OK;
}

// One two-stage reduction over frame `frame` of the uploaded data at the current save point: `kernel` on a grid
// (blocks per field, B, grid_z) leaves K block totals per trajectory, finish_sums adds them up for the host
template <typename T, typename Kernel>
int reduce_frame(pdeopt_ctx* ctx, Kernel kernel, int K, int grid_z, int frame, double theta, int interp, double* host_out) {
  Sens& s = *sens_of(ctx);
  const int64_t cells = sens_cells(ctx);
  const int nblk = (int)((cells + kGnCellsPerBlock - 1) / kGnCellsPerBlock);
  int rc;
  if ((rc = ensure_sums(ctx, K, nblk))) return rc;
  const T* v = s.data.as<const T>() + (int64_t)frame * s.B * cells;
  hipLaunchKernelGGL(kernel, dim3(nblk, s.B, grid_z), dim3(kGnThreads), 0, ctx->stream, ctx->Y.as<const T>(),
                     ctx->SNAP.as<const T>(), v, s.partial.as<double>(), s.B, s.P, cells, (T)theta, interp);
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  return finish_sums(ctx, K, nblk, host_out);
}

// what pdeopt_sens_accumulate and pdeopt_sens_contract ask of their frame and of the snapshot before they launch
int check_frame(pdeopt_ctx* ctx, int frame, int interp) {
  const int rc = check_sens(ctx);
  if (rc) return rc;
  const Sens& s = *sens_of(ctx);
  if (!s.data || frame < 0 || frame >= s.n_frames)
    return fail(ctx, PDEOPT_EINVAL, "frame %d of %d uploaded (pdeopt_sens_set_data)", frame, s.n_frames);
  if (interp && !ctx->SNAP) return fail(ctx, PDEOPT_ESTATE, "pdeopt_snapshot has not been called");
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return PDEOPT_OK;
}

}  // namespace

}  // namespace pdeopt

using namespace pdeopt;

extern "C" {

int pdeopt_sens_configure(pdeopt_ctx* ctx, int n_traj, int n_params, const int32_t* roles, const int32_t* coef_index) {
  if (!ctx || (n_params > 0 && (!roles || !coef_index))) return PDEOPT_EINVAL;
  if (!ctx->configured) return fail(ctx, PDEOPT_ESTATE, "pdeopt_configure has not been called");
  const pdeopt_problem& p = ctx->prob;
  const bool ch2d = p.equation == PDEOPT_EQ_CAHN_HILLIARD && p.nz <= 1, ch3d = p.equation == PDEOPT_EQ_CAHN_HILLIARD_3D;
  const bool ac2d = p.equation == PDEOPT_EQ_ALLEN_CAHN && p.nz <= 1;
  const bool bv = bv_equation(p.equation) && p.nz <= 1;
  const bool sbm = sbm_equation(p.equation) && p.nz <= 1;
  if (!(ch2d || ch3d || ac2d || bv || sbm) || p.derivs != PDEOPT_DERIVS_FD || ctx->halo)
    return fail(ctx, PDEOPT_EINVAL, "sensitivities need the periodic 2-D or 3-D Cahn-Hilliard equation, the periodic 2-D Allen-Cahn "
                                    "equation or a Butler-Volmer Allen-Cahn equation, with derivs=\"fd\" (or a 2-D smoothed-boundary "
                                    "Allen-Cahn / Cahn-Hilliard equation)");
  if (sbm && (!ctx->aux[PDEOPT_AUX_SBM_PSI].dev || !ctx->aux[PDEOPT_AUX_SBM_NORM_GRAD].dev || !ctx->aux[PDEOPT_AUX_SBM_MASK].dev))
    return fail(ctx, PDEOPT_ESTATE, "smoothed-boundary sensitivities need the SBM_PSI, SBM_NORM_GRAD and SBM_MASK aux fields before "
                                    "pdeopt_sens_configure");
  if (bv && !bv_params_set(ctx))
    return fail(ctx, PDEOPT_ESTATE, "Butler-Volmer sensitivities need pdeopt_set_bv_params before pdeopt_sens_configure");
  if (ch3d && sens_cells(ctx) > (int64_t)INT32_MAX / 2)
    return fail(ctx, PDEOPT_EINVAL, "3-D sensitivities index cells in 32 bits (%dx%dx%d)", p.nx, p.ny, p.nz);
  if (p.mu.kind == PDEOPT_CL_JIT || p.mob.kind == PDEOPT_CL_JIT || (sbm && p.fe.kind == PDEOPT_CL_JIT))
    return fail(ctx, PDEOPT_EINVAL, "sensitivities need closures of the in-kernel family (POLY / LEGENDRE), not run-time-compiled ones");
  if (n_traj < 1 || n_params < 1 || n_params > kMaxSens)
    return fail(ctx, PDEOPT_EINVAL, "n_traj = %d, n_params = %d (1 .. %d)", n_traj, n_params, kMaxSens);
  if ((int64_t)(1 + n_params) * n_traj != p.batch)
    return fail(ctx, PDEOPT_EINVAL, "batch %d is not (1 + n_params) n_traj = %d", p.batch, (1 + n_params) * n_traj);
  bool has_kappa = false;
  for (int j = 0; j < n_params; ++j) {
    if (roles[j] == PDEOPT_SENS_KAPPA) {
      if (coef_index[j] != 0)
        return fail(ctx, PDEOPT_EINVAL, "sensitivity %d: PDEOPT_SENS_KAPPA is a scalar, its coef_index must be 0 (got %d)", j, coef_index[j]);
      if (has_kappa) return fail(ctx, PDEOPT_EINVAL, "sensitivity %d: PDEOPT_SENS_KAPPA given twice", j);
      int rc;
      if ((rc = sens_kappa_check(ctx, n_traj, nullptr))) return rc;
      has_kappa = true;
      continue;
    }
    if (roles[j] != PDEOPT_SENS_MU && roles[j] != PDEOPT_SENS_MOB)
      return fail(ctx, PDEOPT_EINVAL, "sensitivity %d: unknown role %d", j, roles[j]);
    const pdeopt_closure& cl = roles[j] == PDEOPT_SENS_MU ? p.mu : p.mob;
    if (coef_index[j] < 0 || coef_index[j] >= cl.n)
      return fail(ctx, PDEOPT_EINVAL, "sensitivity %d: coefficient %d of a closure with %d coefficients", j, coef_index[j], cl.n);
  }
  Sens& s = ctx->features.ensure<Sens>(FS_SENS);
  s.B = n_traj;
  s.P = n_params;
  s.has_kappa = has_kappa;
  for (int j = 0; j < n_params; ++j) {
    s.role[j] = roles[j];
    s.index[j] = coef_index[j];
  }
  return PDEOPT_OK;
}

int pdeopt_sens_rhs(pdeopt_ctx* ctx, void* host_out) {
  if (!ctx) return PDEOPT_EINVAL;
  int rc = check_sens(ctx);
  if (rc) return rc;
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if ((rc = ensure_buffer(ctx, ctx->TA, ctx->total_bytes))) return rc;
  if ((rc = sens_slopes(ctx, ctx->Y.get(), ctx->TA.get(), 0.0))) return rc;
  if (host_out)
    PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(host_out, ctx->TA.get(), ctx->total_bytes, hipMemcpyDeviceToHost, ctx->stream));
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PDEOPT_OK;
}

int pdeopt_sens_advance(pdeopt_ctx* ctx, int integrator, double t0, double dt, int64_t n_substeps) {
  if (!ctx) return PDEOPT_EINVAL;
  int rc = check_sens(ctx);
  if (rc) return rc;
  if (n_substeps < 0 || !(dt > 0)) return fail(ctx, PDEOPT_EINVAL, "n_substeps = %lld, dt = %g", (long long)n_substeps, dt);
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  ctx->tsit5_pending = false;
  ctx->tsit5_fsal_valid = false;
  const bool bv = bv_equation(ctx->prob.equation);
  // the smoothed-boundary equations: theta(t) and flux(t) at every stage time t0 + s dt (+ dt / 2, + dt); all others
  // are autonomous and keep passing 0.0
  const bool sbm = sbm_equation(ctx->prob.equation);
  TimeTableScope table(ctx, sbm);  // as in pdeopt_advance (a table left behind would override the constants of a later pdeopt_sens_rhs)
  const bool ac = ctx->prob.equation == PDEOPT_EQ_ALLEN_CAHN || bv || sbm;  // Euler and RK4, no fourier_symbol
  bool fused = false, kap = false;
  if (integrator == PDEOPT_INT_IMEX) {
    if (sbm)
      return fail(ctx, PDEOPT_EINVAL, "AllenCahn2DSmoothedBoundary / CahnHilliard2DSmoothedBoundary sensitivities support the Euler "
                                      "and RK4 integrators (the psi-weighted operator has no fourier_symbol)");
    if (ac) return fail(ctx, PDEOPT_EINVAL, "Allen-Cahn sensitivities support the Euler and RK4 integrators (it has no fourier_symbol)");
    if (!ctx->aux[PDEOPT_AUX_IMEX_SYMBOL].dev)
      return fail(ctx, PDEOPT_ESTATE, "IMEX needs the IMEX_SYMBOL aux field (fourier_symbol)");
    if (ctx->imex_per_env)
      return fail(ctx, PDEOPT_EINVAL, "IMEX sensitivities need one implicit operator shared by the batch (no per-environment "
                                      "IMEX scales)");
    // the hand-written FFT passes where they exist (power-of-two 2-D grids 64..1024), rocFFT's real transforms elsewhere;
    // a kappa tangent needs the base spectrum next to its own (m'), which only the rocFFT loop's multiply can give it
    kap = sens_of(ctx)->has_kappa;
    fused = !kap && imex_fused_supported(ctx);
    if ((rc = fused ? imex_fused_prepare(ctx, dt) : imex_rocfft_prepare(ctx, dt))) return rc;
    if (kap) {
      double kappa = 0.0;
      if ((rc = sens_kappa_check(ctx, sens_of(ctx)->B, &kappa))) return rc;
      if ((rc = imex_rocfft_prepare_kappa(ctx, dt, kappa))) return rc;
    }
  } else if (integrator == PDEOPT_INT_RK4 && ac) {
    if ((rc = ensure_buffer(ctx, ctx->TB, ctx->total_bytes))) return rc;
    if ((rc = ensure_buffer(ctx, ctx->ACC, ctx->total_bytes))) return rc;
  } else if (integrator != PDEOPT_INT_EULER) {
    return fail(ctx, PDEOPT_EINVAL, "sensitivities support the IMEX and Euler integrators for Cahn-Hilliard, Euler and RK4 for "
                                    "Allen-Cahn (got %d)", integrator);
  }
  if ((rc = ensure_buffer(ctx, ctx->TA, ctx->total_bytes))) return rc;
  for (int64_t s = 0; s < n_substeps; ++s) {
    const double ts = t0 + (double)s * dt;
    if (integrator == PDEOPT_INT_RK4) {
      if ((rc = with_dtype(ctx, [&](auto t) { return rk4_substep<decltype(t)>(ctx, dt, ts, sbm); }))) return rc;
      continue;
    }
    if ((rc = sens_slopes(ctx, ctx->Y.get(), ctx->TA.get(), sbm ? ts : 0.0))) return rc;
    if (integrator == PDEOPT_INT_IMEX && fused) {
      rc = imex_fused_passes(ctx, whole_batch(ctx), dt);
    } else if (integrator == PDEOPT_INT_IMEX) {
      rc = kap ? imex_rocfft_solve_kappa(ctx, dt, sens_of(ctx)->B, sens_of(ctx)->P, sens_of(ctx)->role) : imex_rocfft_solve(ctx, dt);
      ctx->n_stage_launches += 4;  // r2c, multiply, c2r, axpy (host calls; rocFFT may run more than one kernel per transform)
    } else {
      rc = with_dtype(ctx, [&](auto t) { return euler_update<decltype(t)>(ctx, dt); });
    }
    if (rc) return rc;
  }
  PDEOPT_HIP_CHECK(ctx, hipGetLastError());
  if ((rc = table.missed())) return rc;
  // after the loop: the base slope launches name their own kernel
  const int eq = ctx->prob.equation;
  ctx->last_kernel = eq == PDEOPT_EQ_CAHN_HILLIARD_3D ? "sens3d_dmu+sens3d_flux" : eq == PDEOPT_EQ_ALLEN_CAHN_SBM ? "sens_sbm_ac_tangent_rhs"
                     : eq == PDEOPT_EQ_CAHN_HILLIARD_SBM ? "sens_sbm_ch_tangent_rhs" : (bv ? "bvsens_tangent_rhs" : (ac ? "sens_ac_tangent_rhs" : "sens_tangent_rhs"));
  ctx->last_kernel += integrator == PDEOPT_INT_RK4 ? "+rk4" : (integrator != PDEOPT_INT_IMEX ? "+euler" : (fused ? "+imex_fused_lds_fft" : (kap ? "+imex_rocfft_r2c_kappa" : "+imex_rocfft_r2c")));
  return PDEOPT_OK;
}

int pdeopt_sens_bv_voltage(pdeopt_ctx* ctx, double* out) {
  if (!ctx || !out) return PDEOPT_EINVAL;
  const int rc = check_sens(ctx);
  if (rc) return rc;
  if (!bv_equation(ctx->prob.equation)) return fail(ctx, PDEOPT_EINVAL, "pdeopt_sens_bv_voltage belongs to the Butler-Volmer equations");
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const Sens& s = *sens_of(ctx);
  return bv_sens_voltage(ctx, BvSensSpec{s.B, s.P, s.role, s.index}, out);
}

int pdeopt_sens_set_data(pdeopt_ctx* ctx, int n_frames, const void* host) {
  if (!ctx || n_frames < 1 || !host) return PDEOPT_EINVAL;
  int rc = check_sens(ctx);
  if (rc) return rc;
  PDEOPT_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  Sens& s = *sens_of(ctx);
  const size_t bytes = (size_t)n_frames * s.B * sens_cells(ctx) * ctx->esize;
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  if ((rc = grow_device_buffer(ctx, s.data, bytes, /*sync_first=*/false))) return rc;  // (synchronised above)
  s.n_frames = n_frames;
  PDEOPT_HIP_CHECK(ctx, hipMemcpyAsync(s.data.get(), host, bytes, hipMemcpyHostToDevice, ctx->stream));
  PDEOPT_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PDEOPT_OK;
}

int pdeopt_sens_accumulate(pdeopt_ctx* ctx, int frame, double theta, int interp, double* out) {
  if (!ctx || !out) return PDEOPT_EINVAL;
  const int rc = check_frame(ctx, frame, interp);
  if (rc) return rc;
  const int P = sens_of(ctx)->P;
  return with_dtype(ctx, [&](auto t) {
    using T = decltype(t);
    return reduce_frame<T>(ctx, sens_gn_partial_kernel<T>, 1 + P + P * (P + 1) / 2, 1 + P, frame, theta, interp, out);
  });
}

int pdeopt_sens_contract(pdeopt_ctx* ctx, int frame, double theta, int interp, double* out) {
  if (!ctx || !out) return PDEOPT_EINVAL;
  const int rc = check_frame(ctx, frame, interp);
  if (rc) return rc;
  return with_dtype(ctx, [&](auto t) {
    using T = decltype(t);
    return reduce_frame<T>(ctx, sens_contract_partial_kernel<T>, sens_of(ctx)->P, 1, frame, theta, interp, out);
  });
}

}  // extern "C"
