// What the frozen and the stirred kernels of the rotating-frame split step (gpe_rot.hip) share: the step's buffers, the
// geometry of its passes and the one kernel both variants run.  The line operator itself is gpe_rot_line.hpp.
#pragma once

#include <cmath>
#include <complex>

#include "common.hpp"
#include "fft_lds.hpp"
#include "fft_reg.hpp"
#include "gpe_rot_line.hpp"

namespace pdeopt {

struct GpeRot : Feature {
  DeviceBuffer tw_x;   // twiddle tables exp(-2 pi i n / N) in the problem dtype
  DeviceBuffer tw_y;
  DeviceBuffer kin_x;  // exp(tau/2 0.5j (2 pi i kx)^2) / nx, complex [nx]
  DeviceBuffer kin_y;
  DeviceBuffer dens;   // |psi0|^2, real [batch][nx][ny]
  DeviceBuffer partial;  // doubles
  int partial_per_env = 0;
  double key_dt = NAN, key_tr = NAN, key_ti = NAN, key_hx = NAN, key_hy = NAN;
  bool valid = false;

  void invalidate() override { valid = false; }
};

// fp64 and 16-point threads: one factor's sincos at a time (interleaved, their temporaries cost more registers than
// the line itself)
template <typename T, int PTS>
constexpr bool kOneFactorAtATime = sizeof(T) == 8 || PTS > 8;

// Column-pass geometry: C adjacent columns x N/PTS threads per workgroup, the column index fastest across lanes on
// the global side (strang_fused.hip has the measurements behind 128-byte segments).  Up to N = 512 stages 1.. of a
// transform run with a column per wave (RegFft::dif_split / dit_split: one workgroup barrier per transform); at
// N = 1024 the barrier form.  Workgroups of at most 512 (fp32) / 256 (fp64) threads: the JOIN form holds a line's
// points, the twiddles of a butterfly and a sincos in flight, and at more threads the compiler's register cap
// (128 VGPRs at 1024 threads) spills the fp64 instantiations to scratch.
constexpr bool rot_col_wave_local(int n) { return n <= 512; }
template <typename T, int N>
constexpr int rot_cols() {
  constexpr int c = sizeof(T) == 4 ? 16 : 8, cap = sizeof(T) == 4 ? 512 : 256, tt = N / reg_default_pts<N>();
  return c * tt > cap ? cap / tt : c;
}

constexpr int kLibNormBlocks = 64;

inline bool rot_size_ok(int n) { return n == 64 || n == 128 || n == 256 || n == 512 || n == 1024; }

template <typename T, int N>
constexpr int rot_row_lines() { return 256 / RegFft<T, N>::TT; }
inline int rot_row_lines_rt(int ny) { return 256 / (ny / (ny > 512 ? 16 : 8)); }

#define PDEOPT_ROT_SIZES(X) X(64) X(128) X(256) X(512) X(1024)

template <typename T>
__global__ __launch_bounds__(256) void rot_density_kernel(const Cx<T>* __restrict__ psi, T* __restrict__ d, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const Cx<T> v = psi[i];
    d[i] = v.re * v.re + v.im * v.im;
  }
}

}  // namespace pdeopt
