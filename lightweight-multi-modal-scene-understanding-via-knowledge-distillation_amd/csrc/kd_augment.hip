// kd_augment.hip -- opt-in training augmentation of a whole batch on the device, in place (no reference counterpart:
// neither the reference nor its loaders augment).  Two kernels, both specified to the bit in include/kd_hip.h and
// mirrored in numpy by tests/_augment_ref.py:
//   * kd_points_augment_batch: joint flip, yaw, isotropic scale, translation, per-point jitter and an intensity gain over
//     the packed columns x | y | z | i of B ragged frames, BEFORE the rasteriser and the point stacker read them, so BEV
//     labels and points agree by construction;
//   * kd_image_augment_batch: per-channel gain + offset, clamp to [0, 1] and the left-right mirror of the joint flip over
//     the float32 [B,3,H,W] batch, AFTER the convert or the resize launch.
// The 16 per-frame parameters are drawn on the host (kdrt/augment.py, frame_params).  Row layout (float32 words):
//    0 c   1 s   2 scale   3 tx   4 ty   5 sx   6 sy   7 gi   8 a_r   9 a_g   10 a_b   11 b   12 mirror   13..15 padding
// Host draw: the 12 words w0..w11 of Philox-4x32-10 at counters (0, 1, key lo, key hi), (1, 1, ..), (2, 1, ..) under
// the key (seed lo, seed hi), u_k = (w_k >> 8) * 2^-24:  w0 yaw, w1 scale, w2 tx, w3 ty, w4 flip, w5 intensity gain,
// w6 brightness, w7 contrast, w8 / w9 / w10 channel gain r / g / b, w11 camera drop.  Counter word 1 separates the
// streams: 0 is the subset sampler of kd_points_prepare_batch, 1 the frame parameters, 2 the per-point jitter below.
// Both kernels are HBM streams (32 B per point, 8 B per pixel value): the frame index rides in blockIdx.y, so a
// frame's parameters, offsets and key are wave-uniform loads and no thread searches the offsets; every product and sum
// is a separately rounded float32 operation (__f*_rn: the library is built with -ffp-contract=on and nothing here may
// fuse).  No atomics, no workspace, no LDS.
#include "kd_common.h"

namespace {

constexpr int kAugThreads = 256;

struct FrameAug { float c, s, scale, tx, ty, sx, sy, gi; };

// (w >> 8) * 2^-23 - 1: 24 bits in [-1, 1), exact; one rounding in the product with `jitter`
__device__ __forceinline__ float jitter_of(uint32_t w, float jitter) {
  return __fmul_rn(jitter, __fsub_rn(__fmul_rn((float)(w >> 8), 1.1920928955078125e-07f), 1.f));
}

template <bool JIT>
__device__ __forceinline__ void aug_point(float& x, float& y, float& z, float& w, const FrameAug& p, float jitter, uint32_t j,
                                          uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  const float xf = __fmul_rn(p.sx, x), yf = __fmul_rn(p.sy, y);
  const float xr = __fsub_rn(__fmul_rn(p.c, xf), __fmul_rn(p.s, yf));
  const float yr = __fadd_rn(__fmul_rn(p.s, xf), __fmul_rn(p.c, yf));
  x = __fadd_rn(__fmul_rn(p.scale, xr), p.tx);
  y = __fadd_rn(__fmul_rn(p.scale, yr), p.ty);
  z = __fmul_rn(p.scale, z);
  w = __fmul_rn(p.gi, w);
  if (JIT) {
    const uint4 r = kd_philox4(j, 2u, c2, c3, k0, k1);
    x = __fadd_rn(x, jitter_of(r.x, jitter));
    y = __fadd_rn(y, jitter_of(r.y, jitter));
    z = __fadd_rn(z, jitter_of(r.z, jitter));
  }
}

__device__ __forceinline__ uint32_t line_slot(const float* p) { return (uint32_t)(reinterpret_cast<uintptr_t>(p) >> 2) & 3u; }

template <bool JIT>
__global__ __launch_bounds__(kAugThreads) void points_augment_kernel(float* __restrict__ x, float* __restrict__ y,
                                                                     float* __restrict__ z, float* __restrict__ w,
                                                                     const int64_t* __restrict__ off,
                                                                     const uint64_t* __restrict__ frame_key,
                                                                     const float* __restrict__ params, uint64_t seed,
                                                                     float jitter) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t base = off[b];
  const uint32_t n = (uint32_t)(off[b + 1] - base);                      // the host checked n_total < 2^31
  if (n == 0) return;
  const float* q = params + (int64_t)b * 16;
  const FrameAug p{q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7]};
  const uint64_t fk = JIT ? frame_key[b] : 0;
  const uint32_t c2 = (uint32_t)fk, c3 = (uint32_t)(fk >> 32), k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  x += base; y += base; z += base; w += base;
  const uint32_t first = blockIdx.x * kAugThreads + tid, step = gridDim.x * kAugThreads;

  // 16-byte accesses need the four columns of this frame at the same place within a 16-byte line
  const uint32_t slot = line_slot(x);
  if (line_slot(y) != slot || line_slot(z) != slot || line_slot(w) != slot) {
    for (uint32_t j = first; j < n; j += step) {
      float vx = x[j], vy = y[j], vz = z[j], vw = w[j];
      aug_point<JIT>(vx, vy, vz, vw, p, jitter, j, c2, c3, k0, k1);
      x[j] = vx; y[j] = vy; z[j] = vz; w[j] = vw;
    }
    return;
  }
  const uint32_t to_line = (4u - slot) & 3u;
  const uint32_t head = to_line < n ? to_line : n;                        // scalar points before the first whole line
  const uint32_t nvec = (n - head) >> 2;
  const uint32_t tail = head + 4u * nvec;                                 // scalar points [tail, n): at most 3
  if (blockIdx.x == 0 && tid < 8) {
    const uint32_t j = tid < 4 ? (uint32_t)tid : tail + (uint32_t)tid - 4u;
    if (tid < 4 ? j < head : j < n) {
      float vx = x[j], vy = y[j], vz = z[j], vw = w[j];
      aug_point<JIT>(vx, vy, vz, vw, p, jitter, j, c2, c3, k0, k1);
      x[j] = vx; y[j] = vy; z[j] = vz; w[j] = vw;
    }
  }
  for (uint32_t v = first; v < nvec; v += step) {
    const uint32_t j = head + 4u * v;
    float4 vx = kd_ld4(x + j), vy = kd_ld4(y + j), vz = kd_ld4(z + j), vw = kd_ld4(w + j);
    aug_point<JIT>(vx.x, vy.x, vz.x, vw.x, p, jitter, j, c2, c3, k0, k1);
    aug_point<JIT>(vx.y, vy.y, vz.y, vw.y, p, jitter, j + 1u, c2, c3, k0, k1);
    aug_point<JIT>(vx.z, vy.z, vz.z, vw.z, p, jitter, j + 2u, c2, c3, k0, k1);
    aug_point<JIT>(vx.w, vy.w, vz.w, vw.w, p, jitter, j + 3u, c2, c3, k0, k1);
    kd_st4(x + j, vx); kd_st4(y + j, vy); kd_st4(z + j, vz); kd_st4(w + j, vw);
  }
}

// min(max(v * a + b, 0), 1), product and sum rounded separately
__device__ __forceinline__ float img_val(float v, float a, float o) {
  return __builtin_fminf(__builtin_fmaxf(__fadd_rn(__fmul_rn(v, a), o), 0.f), 1.f);
}
__device__ __forceinline__ float4 img_val4(float4 v, float a, float o) {
  return make_float4(img_val(v.x, a, o), img_val(v.y, a, o), img_val(v.z, a, o), img_val(v.w, a, o));
}
__device__ __forceinline__ float4 rev4(float4 v) { return make_float4(v.w, v.z, v.y, v.x); }

// One thread owns the pair (w, W-1-w) of a row -- four such pairs on the vector path -- so the mirror swaps in place
// without a race; without the mirror the same pair is only scaled.  blockIdx.y = plane b*3 + c.
template <bool VEC>
__global__ __launch_bounds__(kAugThreads) void image_augment_kernel(float* __restrict__ img, const float* __restrict__ params,
                                                                    int H, int W) {
  const int plane = blockIdx.y, b = plane / 3, c = plane - 3 * b;
  const float* q = params + (int64_t)b * 16;
  const float a = q[8 + c], o = q[11];
  const bool mirror = q[12] != 0.f;
  float* p = img + (int64_t)plane * H * W;
  const int half = VEC ? W / 8 : (W + 1) / 2;                             // owners per row
  const uint32_t units = (uint32_t)H * (uint32_t)half;                    // the host checked H * W < 2^31
  for (uint32_t u = blockIdx.x * kAugThreads + threadIdx.x; u < units; u += gridDim.x * kAugThreads) {
    const int h = (int)(u / (uint32_t)half), k = (int)(u - (uint32_t)h * (uint32_t)half);
    float* row = p + (int64_t)h * W;
    if (VEC) {
      float* lp = row + 4 * k;
      float* rp = row + W - 4 - 4 * k;                                    // W % 8 == 0: lp < rp, never the same line
      const float4 l = img_val4(kd_ld4(lp), a, o), r = img_val4(kd_ld4(rp), a, o);
      kd_st4(lp, mirror ? rev4(r) : l);
      kd_st4(rp, mirror ? rev4(l) : r);
    } else {
      const int rk = W - 1 - k;
      const float l = img_val(row[k], a, o);
      if (rk == k) {                                                      // the middle column of an odd W
        row[k] = l;
      } else {
        const float r = img_val(row[rk], a, o);
        row[k] = mirror ? r : l;
        row[rk] = mirror ? l : r;
      }
    }
  }
}

}  // namespace

extern "C" {

int kd_points_augment_batch(float* x, float* y, float* z, float* intensity, const int64_t* offsets, const uint64_t* frame_keys,
                            const float* params, int B, int64_t n_total, uint64_t seed, float jitter, void* stream) {
  KD_REQUIRE(offsets && frame_keys && params && B > 0 && B <= 65535 && n_total >= 0, KD_ERR_ARG, "kd_points_augment_batch: bad args");
  KD_REQUIRE(n_total == 0 || (x && y && z && intensity), KD_ERR_ARG, "kd_points_augment_batch: null coordinate arrays");
  KD_REQUIRE(n_total < (int64_t)1 << 31, KD_ERR_SHAPE, "kd_points_augment_batch: too many points");
  KD_REQUIRE(jitter >= 0.f && jitter < INFINITY, KD_ERR_ARG, "kd_points_augment_batch: jitter must be finite and >= 0");
  if (n_total == 0) return KD_OK;
  // a frame may hold every point of the batch: blocks of 1024 points each, capped so that B frames give a few thousand
  // blocks; the rest is a grid-stride loop, and blocks past a short frame's end leave at once
  const int64_t need = (n_total + 4 * kAugThreads - 1) / (4 * kAugThreads);
  const int64_t cap = 8192 / B > 8 ? 8192 / B : 8;
  const dim3 grid((unsigned)(need < cap ? need : cap), (unsigned)B);
  hipStream_t st = (hipStream_t)stream;
  if (jitter > 0.f)
    hipLaunchKernelGGL(points_augment_kernel<true>, grid, dim3(kAugThreads), 0, st, x, y, z, intensity, offsets, frame_keys,
                       params, seed, jitter);
  else
    hipLaunchKernelGGL(points_augment_kernel<false>, grid, dim3(kAugThreads), 0, st, x, y, z, intensity, offsets, frame_keys,
                       params, seed, jitter);
  return kd_check_launch("kd_points_augment_batch");
}

int kd_image_augment_batch(float* img, const float* params, int B, int H, int W, void* stream) {
  KD_REQUIRE(img && params && B > 0 && H > 0 && W > 0, KD_ERR_ARG, "kd_image_augment_batch: bad args");
  KD_REQUIRE(B <= 21845 && (int64_t)H * W < (int64_t)1 << 31, KD_ERR_SHAPE, "kd_image_augment_batch: batch or image too large");
  const bool vec = W % 8 == 0 && kd_aligned16(img);
  const int64_t units = (int64_t)H * (vec ? W / 8 : (W + 1) / 2);
  const int64_t need = (units + kAugThreads - 1) / kAugThreads;
  const dim3 grid((unsigned)(need < 64 ? need : 64), (unsigned)(B * 3));
  hipStream_t st = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL(image_augment_kernel<true>, grid, dim3(kAugThreads), 0, st, img, params, H, W);
  else
    hipLaunchKernelGGL(image_augment_kernel<false>, grid, dim3(kAugThreads), 0, st, img, params, H, W);
  return kd_check_launch("kd_image_augment_batch");
}

}  // extern "C"
