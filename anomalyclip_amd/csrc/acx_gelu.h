// Exact GELU (nn.GELU, approximate="none"): gelu(x) = x Phi(x) = 0.5 x (1 + erf(x / sqrt 2)), and its derivative
// Phi(x) + x phi(x), phi(x) = exp(-x^2 / 2) / sqrt(2 pi).  The activation of every CLIP checkpoint that was not trained with
// QuickGELU (open_clip's LAION-2B / DataComp ViT-B/32, B/16, L/14: configs without `quick_gelu: true`).
// f32-accurate: erff is the device library's (not a tanh / sigmoid form, which is off by ~5e-4).  tests/test_gpu_gelu.py holds
// the forward and the derivative to twice the fp64 error of torch's own float32 CPU F.gelu ("Exact GELU").
//   * x -> -inf: erff saturates at -1, 1 + erf = +0 and the result is -0.0 (never a NaN: no inf * 0, x is finite)
//   * x -> +inf: 1 + erf = 2, the result is x exactly
//   * |gelu(x)| <= |x| (Phi in [0, 1]): what ACX_PREC_F32X6_R16's fp16 planes of s_hid * hidden rest on, as for QuickGELU
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ float acx_gelu_erf(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f)); }

// d gelu / dx from the pre-activation
__device__ __forceinline__ float acx_gelu_erf_grad(float v) {
  const float cdf = 0.5f * (1.f + erff(v * 0.70710678118654752440f));
  const float pdf = 0.39894228040143267794f * expf(-0.5f * v * v);
  return fmaf(v, pdf, cdf);
}
