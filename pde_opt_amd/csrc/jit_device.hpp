// DEVICE SOURCE of the run-time-compiled closure kernels (csrc/jit.hip hands this text to hiprtc; csrc/build.py embeds
// it into the library as a string).  NOT included by any translation unit of the library.
//
// The reference accepts ANY pointwise callable as mu, D, R (dataclass fields cahn_hilliard.py:51-54, allen_cahn.py:47-50)
// and as the prior of a Legendre chemical potential (functions/legendre.py:56-74): jax.jit traces it into the
// right-hand side.  The in-kernel closure family (closures.hpp) covers what the reference's own tests and notebooks pass;
// for a callable outside it (tanh(3 c), sqrt(c) (1 - c), a Legendre series + an arbitrary prior ...) the host side turns
// the traced sympy expression into three function BODIES (pde_opt_amd/numerics/closures.py: jit_body) and this file is
// compiled once per distinct (bodies, dtype) with them pasted in:
//
//     PDEOPT_JIT_T          float / double
//     PDEOPT_JIT_MU_BODY    statements ending in `return ...;`, the argument is `c`   (likewise _MOB_BODY)
//     PDEOPT_JIT_STAGEARGS_SIZE, _OFF_*   sizeof / offsetof of the host's StageArgs<T>: the struct copies below are
//                           checked against them, so a layout drift fails the compilation instead of reading garbage
//
// The kernel is stage_generic_kernel (stencil_generic.hpp) for Cahn-Hilliard / Allen-Cahn with the two closure calls
// replaced: one thread per cell, every layout (periodic / padded), every stage mode (Euler, RK4, Tsit5's OUT_K_LC).
typedef PDEOPT_JIT_T T;
typedef long long i64;

struct Geo {
  int nx, ny, ld;
  i64 off, bstride;
  int periodic, nz;
};
struct EnvParams {
  T kappa, gpe_k, kscale, imex_scale;
  T mu[16], mob[16], fe[16];
  T gpe_omega, gpe_omega_rate;
};
struct ClosureSpec {
  int kind, flags, n;
};
struct LcArgs {
  const T* k[6];
  T c[7];
  int n;
  T* next;
};
struct StageArgs {
  const T* in;
  const T* y;
  T* out;
  T* acc;
  T a, b;
  T rhx, rhy, rhx2, rhy2;
  T rhz, rhz2;
  const T* mu3;
  Geo g;
  const EnvParams* ep;
  ClosureSpec mu, mob;
  const T* vx;
  const T* vy;
  i64 vstride;
  const T* psi;
  const T* ngp;
  const T* mask;
  T tw_a, tw_b, tsrc;
  ClosureSpec fe;
  LcArgs lc;
  int out_mode, acc_mode;
  int scaled;
  int dbg;
};
static_assert(sizeof(StageArgs) == PDEOPT_JIT_STAGEARGS_SIZE, "StageArgs layout differs from the library's");
static_assert(__builtin_offsetof(StageArgs, g) == PDEOPT_JIT_OFF_G, "StageArgs::g");
static_assert(__builtin_offsetof(StageArgs, ep) == PDEOPT_JIT_OFF_EP, "StageArgs::ep");
static_assert(__builtin_offsetof(StageArgs, lc) == PDEOPT_JIT_OFF_LC, "StageArgs::lc");
static_assert(__builtin_offsetof(StageArgs, out_mode) == PDEOPT_JIT_OFF_OUT_MODE, "StageArgs::out_mode");
static_assert(sizeof(EnvParams) == PDEOPT_JIT_ENVPARAMS_SIZE, "EnvParams layout differs from the library's");

enum { OUT_NONE = 0, OUT_K = 1, OUT_Y_PLUS_AK = 2, OUT_ACC_PLUS_BK = 3, OUT_K_LC = 4 };
enum { ACC_NONE = 0, ACC_INIT = 1, ACC_ADD = 2 };

// x^n for a small integer n (the tracer emits these for c**2, c**3 ...: no pow() call)
__device__ __forceinline__ T jit_powi(T x, int n) {
  T r = T(1);
  for (int i = 0; i < n; ++i) r *= x;
  return r;
}

__device__ __forceinline__ T jit_mu(T c) {
  PDEOPT_JIT_MU_BODY
}
__device__ __forceinline__ T jit_mob(T c) {
  PDEOPT_JIT_MOB_BODY
}

__device__ __forceinline__ int wrap_idx(int i, int n) {
  i %= n;
  return i < 0 ? i + n : i;
}
__device__ __forceinline__ T lap_at(T c, T xp, T xm, T yp, T ym, T rhx2, T rhy2) {
  return (xp - T(2) * c + xm) * rhx2 + (yp - T(2) * c + ym) * rhy2;
}

// rhs_generic_point (stencil_generic.hpp) for EQ = Cahn-Hilliard (0) / Allen-Cahn (1): cahn_hilliard.py:89-109, allen_cahn.py:81-84
template <int EQ>
__device__ __forceinline__ T rhs_point(const StageArgs& a, const T* __restrict__ u, const EnvParams& p, int i, int j) {
  const Geo& g = a.g;
  int i1 = i + 1, i2 = i + 2, im1 = i - 1, im2 = i - 2;
  int j1 = j + 1, j2 = j + 2, jm1 = j - 1, jm2 = j - 2;
  if (g.periodic) {
    i1 = wrap_idx(i1, g.nx); i2 = wrap_idx(i2, g.nx);
    im1 = wrap_idx(im1, g.nx); im2 = wrap_idx(im2, g.nx);
    j1 = wrap_idx(j1, g.ny); j2 = wrap_idx(j2, g.ny);
    jm1 = wrap_idx(jm1, g.ny); jm2 = wrap_idx(jm2, g.ny);
  }
  const i64 ld = g.ld;
  auto U = [&](int ii, int jj) -> T { return u[(i64)ii * ld + jj]; };
  const T u00 = U(i, j), uxp = U(i1, j), uxm = U(im1, j), uyp = U(i, j1), uym = U(i, jm1);
  const T kap = p.kappa;
  if (EQ == 1) {
    const T mu = jit_mu(u00) - kap * lap_at(u00, uxp, uxm, uyp, uym, a.rhx2, a.rhy2);
    return -jit_mob(u00) * mu;
  }
  const T ux2 = U(i2, j), uxm2 = U(im2, j), uy2 = U(i, j2), uym2 = U(i, jm2);
  const T upp = U(i1, j1), upm = U(i1, jm1), ump = U(im1, j1), umm = U(im1, jm1);
  auto MU = [&](T c, T xp, T xm, T yp, T ym) -> T { return jit_mu(c) - kap * lap_at(c, xp, xm, yp, ym, a.rhx2, a.rhy2); };
  const T m00 = MU(u00, uxp, uxm, uyp, uym);
  const T mxp = MU(uxp, ux2, u00, upp, upm);
  const T mxm = MU(uxm, u00, uxm2, ump, umm);
  const T myp = MU(uyp, upp, ump, uy2, u00);
  const T mym = MU(uym, upm, umm, u00, uym2);
  const T d00 = jit_mob(u00), dxp = jit_mob(uxp), dxm = jit_mob(uxm), dyp = jit_mob(uyp), dym = jit_mob(uym);
  const T fx0 = (T(0.5) * (d00 + dxp)) * ((mxp - m00) * a.rhx);
  const T fxm = (T(0.5) * (dxm + d00)) * ((m00 - mxm) * a.rhx);
  const T fy0 = (T(0.5) * (d00 + dyp)) * ((myp - m00) * a.rhy);
  const T fym = (T(0.5) * (dym + d00)) * ((m00 - mym) * a.rhy);
  return (fx0 - fxm) * a.rhx + (fy0 - fym) * a.rhy;
}

__device__ __forceinline__ void stage_update(const StageArgs& a, i64 idx, T k) {
  if (a.acc_mode == ACC_INIT) a.acc[idx] = a.y[idx] + a.b * k;
  if (a.out_mode == OUT_K) {
    a.out[idx] = k;
  } else if (a.out_mode == OUT_Y_PLUS_AK) {
    a.out[idx] = a.y[idx] + a.a * k;
  } else if (a.out_mode == OUT_ACC_PLUS_BK) {
    a.out[idx] = a.acc[idx] + a.b * k;
  } else if (a.out_mode == OUT_K_LC) {
    a.out[idx] = k;
    T r = a.y[idx];
    for (int j = 0; j < a.lc.n; ++j) r += a.lc.c[j] * a.lc.k[j][idx];
    a.lc.next[idx] = r + a.lc.c[a.lc.n] * k;
  }
  if (a.acc_mode == ACC_ADD) a.acc[idx] += a.b * k;
}

template <int EQ>
__device__ __forceinline__ void stage_body(const StageArgs& a) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  const int i = blockIdx.y * 4 + threadIdx.y;
  const int b = blockIdx.z;
  if (i >= a.g.nx || j >= a.g.ny) return;
  const i64 base = (i64)b * a.g.bstride + a.g.off;
  const EnvParams& p = a.ep[b];
  T k = rhs_point<EQ>(a, a.in + base, p, i, j);
  if (a.scaled) k *= p.kscale;
  stage_update(a, base + (i64)i * a.g.ld + j, k);
}

extern "C" __global__ __launch_bounds__(256) void pdeopt_jit_stage_ch(const StageArgs a) { stage_body<0>(a); }
extern "C" __global__ __launch_bounds__(256) void pdeopt_jit_stage_ac(const StageArgs a) { stage_body<1>(a); }
