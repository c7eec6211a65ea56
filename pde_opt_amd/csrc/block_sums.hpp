// Deterministic sums over a wave, a workgroup and a row of workgroup partials: no atomics, fixed order.  Users: the
// observable kernels (gpe_obs.hip, pf_obs.hip: block_sums in the tile kernels, rows_total + wave_sum in the finish
// kernels) and the adjoints of the split steps (gpe_adjoint.hip, gpe_rot_adjoint.hip through gpe_rot_adjoint_sums.hpp:
// block_sum per workgroup, wave_sum in the totals over the partition).
#pragma once

#include <cstdint>

#include "common.hpp"

namespace pdeopt {

// sum over the 64 lanes of a wave, valid in lane 0
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// sum over the workgroup (256 threads), valid in thread 0; sh: 4 doubles of LDS.  (Here and in block_sums the shuffle
// loop is written out: called through wave_sum, the callers' kernels come out in another instruction order.)
__device__ __forceinline__ double block_sum(double v, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  __syncthreads();  // sh may still be read from the previous sum
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}

// sum of NV values per lane over the workgroup's NW waves, in a fixed order; the first NV threads store one each at dst
template <int NV, int NW>
__device__ __forceinline__ void block_sums(double (&a)[NV], double* __restrict__ dst) {
  __shared__ double red[NW][NV];
#pragma unroll
  for (int c = 0; c < NV; ++c) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a[c] += __shfl_down(a[c], o, 64);
  }
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) {
#pragma unroll
    for (int c = 0; c < NV; ++c) red[tid >> 6][c] = a[c];
  }
  __syncthreads();
  if (tid < NV) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) s += red[w][tid];
    dst[tid] = s;
  }
}

// one wave: s[c] += column c of the rows lane, lane + 64, .. below n (rows: n rows of STRIDE doubles, the first NV added)
template <int NV, int STRIDE = NV>
__device__ __forceinline__ void rows_total(const double* __restrict__ rows, int n, int lane, double (&s)[NV]) {
  for (int q = lane; q < n; q += 64) {
    const double* const r = rows + (int64_t)q * STRIDE;
#pragma unroll
    for (int c = 0; c < NV; ++c) s[c] += r[c];
  }
}

}  // namespace pdeopt
