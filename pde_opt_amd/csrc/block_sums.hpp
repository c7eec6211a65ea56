// Deterministic workgroup reduction of the observable kernels (gpe_obs.hip, pf_obs.hip): no atomics, fixed order.
#pragma once

#include "common.hpp"

namespace pdeopt {

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

}  // namespace pdeopt
