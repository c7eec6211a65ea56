// Device helpers the library's own networks share (cnn.hip, mixer.hip): the 16 x 16 x 4 matrix instruction in fp32 and
// fp64 with the row map of its result, and the activations with their derivatives.
#pragma once

#include "common.hpp"

namespace pdeopt {

// template values of the activations: the hidden activations are numbered as pdeopt_cnn_activation and
// pdeopt_mixer_activation number them
enum { NN_ACT_NONE = -1, NN_ACT_GELU = 0, NN_ACT_GELU_TANH = 1, NN_ACT_TANH = 2, NN_ACT_RELU = 3 };

template <typename T>
using vec4 = T __attribute__((ext_vector_type(4)));

__device__ __forceinline__ vec4<float> mfma16(float a, float b, vec4<float> c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ vec4<double> mfma16(double a, double b, vec4<double> c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}
// row of accumulator register `reg` of lane group lk = lane >> 4 in the 16 x 16 result (its column is lane & 15): the
// fp64 instruction interleaves the rows of the four lane groups, the fp32 one gives each group four consecutive rows
template <typename T>
__device__ __forceinline__ int acc_row(int lk, int reg) {
  return sizeof(T) == 8 ? lk + 4 * reg : lk * 4 + reg;
}

__device__ __forceinline__ float t_tanh(float x) { return tanhf(x); }
__device__ __forceinline__ double t_tanh(double x) { return tanh(x); }
__device__ __forceinline__ float t_erf(float x) { return erff(x); }
__device__ __forceinline__ double t_erf(double x) { return erf(x); }
__device__ __forceinline__ float t_exp(float x) { return expf(x); }
__device__ __forceinline__ double t_exp(double x) { return exp(x); }

template <typename T, int ACT>
__device__ __forceinline__ T act_value(T z) {
  if (ACT == NN_ACT_GELU) return T(0.5) * z * (T(1) + t_erf(z * T(0.70710678118654752440)));
  if (ACT == NN_ACT_GELU_TANH) {
    const T t = t_tanh(T(0.79788456080286535588) * (z + T(0.044715) * z * z * z));
    return T(0.5) * z * (T(1) + t);
  }
  if (ACT == NN_ACT_TANH) return t_tanh(z);
  if (ACT == NN_ACT_RELU) return z > T(0) ? z : T(0);
  return z;
}
template <typename T, int ACT>
__device__ __forceinline__ T act_deriv(T z) {
  if (ACT == NN_ACT_GELU)
    return T(0.5) * (T(1) + t_erf(z * T(0.70710678118654752440))) + z * T(0.39894228040143267794) * t_exp(T(-0.5) * z * z);
  if (ACT == NN_ACT_GELU_TANH) {
    const T k = T(0.79788456080286535588);
    const T t = t_tanh(k * (z + T(0.044715) * z * z * z));
    return T(0.5) * (T(1) + t) + T(0.5) * z * (T(1) - t * t) * k * (T(1) + T(3 * 0.044715) * z * z);
  }
  if (ACT == NN_ACT_TANH) {
    const T t = t_tanh(z);
    return T(1) - t * t;
  }
  if (ACT == NN_ACT_RELU) return z > T(0) ? T(1) : T(0);
  return T(1);
}

}  // namespace pdeopt
