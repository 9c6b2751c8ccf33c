// kd_loss_common.h -- what the loss kernels share.  The hard-label files (kd_loss.hip, kd_loss_region.hip, kd_loss_lovasz.hip,
// kd_loss_ohem.hip): the per-pixel softmax, the kept-pixel predicate and the choice of the class bucket; the KL term of the
// region and OHEM calls keeps the bits of kd_seg_loss_fwd_bwd because all of them run this one softmax.  The feature-term files
// (kd_loss_cwd.hip, kd_loss_pair.hip, kd_loss_ifv.hip): the row helpers at the end.
#pragma once

#include "kd_common.h"

// K: the class bucket.  Every per-class loop runs j = 0 .. K-1 in ascending order, fully unrolled, guarded by j < NC: the
// per-pixel arrays stay in registers and the operation order is that of the K = 4 instance for every bucket.
template <int K>
__device__ __forceinline__ void softmax_c(const float* z, int NC, float invT, float* p, float* logp) {
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < K; ++j) if (j < NC) mx = fmaxf(mx, z[j] * invT);
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < K; ++j) if (j < NC) { p[j] = expf(z[j] * invT - mx); s += p[j]; }
  const float ls = logf(s);
#pragma unroll
  for (int j = 0; j < K; ++j) if (j < NC) { logp[j] = z[j] * invT - mx - ls; p[j] = p[j] / s; }
}

// the pixels the hard-label terms keep: a label that is not ignore_index and names one of the NC classes.  A macro: as an inline
// function the same expression compiles to another instruction order in the kernels that use it (profiles/loss_header_codegen.txt)
#define KD_KEPT_LABEL(y, ignore_index, NC) ((y) != (ignore_index) && (y) >= 0 && (y) < (NC))

// launches the smallest of the instances kernel<4>, kernel<8>, kernel<16> that holds NC classes (NC <= 16 is the caller's check)
#define KD_LAUNCH_CLASS_BUCKET(kernel, NC, grid, block, stream, ...)                         \
  do {                                                                                       \
    if ((NC) <= 4) hipLaunchKernelGGL(kernel<4>, grid, block, 0, stream, __VA_ARGS__);       \
    else if ((NC) <= 8) hipLaunchKernelGGL(kernel<8>, grid, block, 0, stream, __VA_ARGS__);  \
    else hipLaunchKernelGGL(kernel<16>, grid, block, 0, stream, __VA_ARGS__);                \
  } while (0)

// ---- rows of a feature map, four channels to a float4 (kd_loss_cwd.hip, kd_loss_pair.hip, kd_loss_ifv.hip) ----
// 1 / |x| correctly rounded (sqrt, then a true division); 0 for a norm of at most 1e-12
__device__ __forceinline__ float inv_norm(float ss) {
  const float r = __fsqrt_rn(ss);
  return r > 1e-12f ? __fdiv_rn(1.f, r) : 0.f;
}
__device__ __forceinline__ float sumsq4(float4 v, float acc) { return fmaf(v.w, v.w, fmaf(v.z, v.z, fmaf(v.y, v.y, fmaf(v.x, v.x, acc)))); }
__device__ __forceinline__ float4 scale4(float4 v, float k) {
  return make_float4(__fmul_rn(v.x, k), __fmul_rn(v.y, k), __fmul_rn(v.z, k), __fmul_rn(v.w, k));
}
// the sum over the 8 lanes that share a row: a butterfly, so every lane holds the same bits
__device__ __forceinline__ float row8_sum(float v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  return v;
}
