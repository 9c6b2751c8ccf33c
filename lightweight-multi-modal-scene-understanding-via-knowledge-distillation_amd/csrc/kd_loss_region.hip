// kd_loss_region.hip -- the opt-in region-based hard-label loss of the KD step:
//   L_hard = wf * Focal + wt * Tversky, optionally with the temperature-softmax KL term of kd_loss.hip riding along,
//   value and dL/dlogits from one call of three launches, like kd_seg_loss_fwd_bwd which it can replace.
//   Focal   = sum_K w[y] (1 - p_y)^gamma (-log p_y) / sum_K w[y]          (K: the kept pixels, p = softmax(z) at T = 1)
//   Tversky = 1 - (1/NC) sum_c (TP_c + s) / (TP_c + a FP_c + b FN_c + s)   (one set of sums over the whole batch)
// Launch layout (mirrored by tests/_fp64_region_loss_ref.py): 256 threads, at most 1024 blocks, a thread adds its pixels in fp32,
// a wave its 64 lanes (6 butterfly steps), a block its 4 waves; the slab rows and everything after them are summed in double.
// No atomics and a fixed order everywhere: the same input gives the same bits on every call and every graph replay.
#include "kd_loss_common.h"

#include <cmath>

namespace {

constexpr int MAXC = 4;
constexpr int ROW = 16;                   // floats per slab row: 0 focal numerator, 1 sum w, 2 KL, 3.. TP_c, 7.. A_c, 11.. N_c
constexpr int V_TI = 5, V_QS = 9, V_QO = 13;                  // layout of the 17 `vals` past (L_hard, KL, sum w, Focal, Tversky)

struct RegionArgs {
  const float* zs; const float* zt; const int64_t* target; const float* cw;
  int ignore_index; float T; float alpha; float gscale; const float* gdev;
  float gamma, wf, wt, a, b, s;
  float* slab; float* vals; float* dzs;
  int64_t npix; int HW; int NC;
};

// om^e for om in [0, 1]: the exponents 0, 1 and 2 (gamma = 2 is the default) without powf
__device__ __forceinline__ float pow_om(float om, float e) {
  if (e == 0.f) return 1.f;
  if (e == 1.f) return om;
  if (e == 2.f) return om * om;
  return powf(om, e);
}

// p_y, log p_y and 1 - p_y as the sum of the other classes' probabilities (never a subtraction from 1)
__device__ __forceinline__ void pick(const float* p, const float* lp, int NC, int y, float& py, float& lpy, float& om) {
  py = 0.f; lpy = 0.f; om = 0.f;
#pragma unroll
  for (int j = 0; j < MAXC; ++j) if (j < NC) { if (j == y) { py = p[j]; lpy = lp[j]; } else om += p[j]; }
}

__global__ __launch_bounds__(256) void region_partial_kernel(RegionArgs a) {
  float v[ROW];
#pragma unroll
  for (int k = 0; k < ROW; ++k) v[k] = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.npix; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / a.HW, hw = i % a.HW;
    float z[MAXC], p[MAXC], lp[MAXC];
#pragma unroll
    for (int j = 0; j < MAXC; ++j) if (j < a.NC) z[j] = a.zs[(b * a.NC + j) * a.HW + hw];
    const int64_t y = a.target[i];
    if (KD_KEPT_LABEL(y, a.ignore_index, a.NC)) {
      softmax_c<MAXC>(z, a.NC, 1.f, p, lp);
      float py, lpy, om;
      pick(p, lp, a.NC, (int)y, py, lpy, om);
      const float w = a.cw ? a.cw[y] : 1.f;
      v[0] = fmaf(w * pow_om(om, a.gamma), -lpy, v[0]);
      v[1] += w;
#pragma unroll
      for (int j = 0; j < MAXC; ++j) if (j < a.NC) {
        v[7 + j] += p[j];
        if (j == (int)y) { v[3 + j] += p[j]; v[11 + j] += 1.f; }
      }
    }
    if (a.zt) {
      float zt[MAXC], pt[MAXC], lpt[MAXC];
#pragma unroll
      for (int j = 0; j < MAXC; ++j) if (j < a.NC) zt[j] = a.zt[(b * a.NC + j) * a.HW + hw];
      softmax_c<MAXC>(z, a.NC, 1.f / a.T, p, lp);
      softmax_c<MAXC>(zt, a.NC, 1.f / a.T, pt, lpt);
#pragma unroll
      for (int j = 0; j < MAXC; ++j) if (j < a.NC) v[2] += pt[j] > 0.f ? pt[j] * (lpt[j] - lp[j]) : 0.f;
    }
  }
  __shared__ float red[ROW][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < ROW; ++k) {
    const float s = kd_wave_sum(v[k]);
    if (lane == 0) red[k][wave] = s;
  }
  __syncthreads();
  if (threadIdx.x < ROW)
    a.slab[(int64_t)blockIdx.x * ROW + threadIdx.x] = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
}

// One block.  vals: [0] L_hard  [1] KL (per-pixel mean)  [2] sum of weights  [3] Focal  [4] Tversky  [5..8] TI_c
//   [9..12]  qs_c = -(wt/NC) dTI_c/dp_c at a pixel with y == c     [13..16] qo_c = the same at a pixel with y != c
// With D = TP + a FP + b FN + s and U = TP + s:  dTI/dp = (D - U (1 - b)) / D^2 = (a FP + b (N + s)) / D^2  (FN + TP = N: the
// form without a cancellation) where y == c, and -U a / D^2 elsewhere.  A term whose weight is 0 is not evaluated (its values are 0).
__global__ __launch_bounds__(256) void region_final_kernel(const float* slab, int nblk, double npix, int NC, float wf, float wt,
                                                           float ta, float tb, float ts, float* vals) {
  __shared__ double red[ROW - 1][256];
  double s[ROW - 1];
#pragma unroll
  for (int k = 0; k < ROW - 1; ++k) s[k] = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 256) {
#pragma unroll
    for (int k = 0; k < ROW - 1; ++k) s[k] += (double)slab[(int64_t)i * ROW + k];
  }
#pragma unroll
  for (int k = 0; k < ROW - 1; ++k) red[k][threadIdx.x] = s[k];
  __syncthreads();
  if (threadIdx.x == 0) {
    double t[ROW - 1];
#pragma unroll
    for (int k = 0; k < ROW - 1; ++k) t[k] = 0.0;
    for (int i = 0; i < 256; ++i) {
#pragma unroll
      for (int k = 0; k < ROW - 1; ++k) t[k] += red[k][i];
    }
    double hard = 0.0, focal = 0.0, tv = 0.0;
    if (wf > 0.f) { focal = t[0] / t[1]; hard += (double)wf * focal; }
    for (int c = 0; c < MAXC; ++c) vals[V_TI + c] = vals[V_QS + c] = vals[V_QO + c] = 0.f;
    if (wt > 0.f) {
      const double al = ta, be = tb, sm = ts, coef = (double)wt / NC;
      double sti = 0.0;
      for (int c = 0; c < NC; ++c) {
        const double TP = t[3 + c], FP = t[7 + c] - TP, N = t[11 + c], FN = N - TP;
        const double U = TP + sm, D = TP + al * FP + be * FN + sm;
        const double ti = U / D;
        sti += ti;
        vals[V_TI + c] = (float)ti;
        vals[V_QS + c] = (float)(-coef * (al * FP + be * (N + sm)) / (D * D));
        vals[V_QO + c] = (float)(coef * U * al / (D * D));
      }
      tv = 1.0 - sti / NC;
      hard += (double)wt * tv;
    }
    vals[0] = (float)hard;
    vals[1] = (float)(t[2] / npix);
    vals[2] = (float)t[1];
    vals[3] = (float)focal;
    vals[4] = (float)tv;
  }
}

__global__ __launch_bounds__(256) void region_grad_kernel(RegionArgs a) {
  const float sumw = a.vals[2];
  const float gs = a.gscale * (a.gdev ? a.gdev[0] : 1.f);      // upstream gradient as a device scalar
  const float klc = a.zt ? gs * a.alpha * a.T / (float)a.npix : 0.f;
  float qs[MAXC], qo[MAXC];
#pragma unroll
  for (int j = 0; j < MAXC; ++j) { qs[j] = a.vals[V_QS + j]; qo[j] = a.vals[V_QO + j]; }
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.npix; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / a.HW, hw = i % a.HW;
    float z[MAXC], p[MAXC], lp[MAXC], g[MAXC];
#pragma unroll
    for (int j = 0; j < MAXC; ++j) { g[j] = 0.f; if (j < a.NC) z[j] = a.zs[(b * a.NC + j) * a.HW + hw]; }
    const int64_t y = a.target[i];
    if (KD_KEPT_LABEL(y, a.ignore_index, a.NC)) {
      softmax_c<MAXC>(z, a.NC, 1.f, p, lp);
      if (a.wf > 0.f) {
        float py, lpy, om;
        pick(p, lp, a.NC, (int)y, py, lpy, om);
        // d/dz_j of w (1 - p_y)^gamma (-log p_y) = w [gamma p_y (1 - p_y)^(gamma-1) log p_y - (1 - p_y)^gamma] ([j == y] - p_j);
        // both terms of the bracket are <= 0, gamma = 0 leaves -1 (the cross-entropy's gradient)
        const float f = a.gamma == 0.f ? -1.f : fmaf(a.gamma * py * pow_om(om, a.gamma - 1.f), lpy, -pow_om(om, a.gamma));
        const float c = a.wf * (a.cw ? a.cw[y] : 1.f) * gs / sumw * f;
#pragma unroll
        for (int j = 0; j < MAXC; ++j) if (j < a.NC) g[j] = c * (j == (int)y ? om : -p[j]);
      }
      if (a.wt > 0.f) {
        float q[MAXC], dot = 0.f;
#pragma unroll
        for (int j = 0; j < MAXC; ++j) if (j < a.NC) { q[j] = j == (int)y ? qs[j] : qo[j]; dot = fmaf(p[j], q[j], dot); }
#pragma unroll
        for (int j = 0; j < MAXC; ++j) if (j < a.NC) g[j] = fmaf(gs * p[j], q[j] - dot, g[j]);
      }
    }
    if (a.zt) {
      float zt[MAXC], pt[MAXC], lpt[MAXC];
#pragma unroll
      for (int j = 0; j < MAXC; ++j) if (j < a.NC) zt[j] = a.zt[(b * a.NC + j) * a.HW + hw];
      softmax_c<MAXC>(z, a.NC, 1.f / a.T, p, lp);
      softmax_c<MAXC>(zt, a.NC, 1.f / a.T, pt, lpt);
#pragma unroll
      for (int j = 0; j < MAXC; ++j) if (j < a.NC) g[j] = fmaf(klc, p[j] - pt[j], g[j]);
    }
#pragma unroll
    for (int j = 0; j < MAXC; ++j) if (j < a.NC) a.dzs[(b * a.NC + j) * a.HW + hw] = g[j];
  }
}

inline int64_t region_blocks(int64_t npix) {
  const int64_t g = (npix + 255) / 256;
  return g > 1024 ? 1024 : (g < 1 ? 1 : g);
}

}  // namespace

extern "C" {

size_t kd_seg_region_loss_ws_bytes(int64_t npix) { return (size_t)region_blocks(npix) * ROW * sizeof(float); }

// vals (17 floats, layout at region_final_kernel): vals[0] = wf * Focal + wt * Tversky, vals[1] = the KL of kd_seg_loss_fwd_bwd (0 if
// zt null), vals[2] = sum of class weights over kept pixels.   dzs = gscale * gscale_dev[0] * d/dzs (vals[0] + alpha*T^2*KL);
// dzs == null: forward only.  No kept pixel: Focal is 0/0 = NaN when wf > 0 (as the cross-entropy); with wf == 0 the focal
// term is never formed and the Tversky value stands with an all-zero hard-label gradient.
int kd_seg_region_loss_fwd_bwd(const float* zs, const float* zt, const int64_t* target, const float* class_w, int ignore_index,
                               float T, float alpha, float gscale, const float* gscale_dev, float gamma, float wf, float wt,
                               float a, float b, float s, float* vals, float* dzs, int B, int NC, int HW, void* ws,
                               size_t ws_bytes, void* stream) {
  KD_REQUIRE(zs && target && vals && ws && B > 0 && HW > 0, KD_ERR_ARG, "kd_seg_region_loss_fwd_bwd: bad args");
  KD_REQUIRE(NC >= 2 && NC <= MAXC, KD_ERR_SHAPE, "kd_seg_region_loss_fwd_bwd: num_classes=%d unsupported (2..4)", NC);
  KD_REQUIRE(std::isfinite(gamma) && (gamma == 0.f || gamma >= 1.f), KD_ERR_ARG,
             "kd_seg_region_loss_fwd_bwd: gamma must be 0 or >= 1 (got %g: the derivative is unbounded at p_y -> 1 in between)", (double)gamma);
  KD_REQUIRE(std::isfinite(a) && std::isfinite(b) && std::isfinite(s) && a >= 0.f && b >= 0.f && s > 0.f, KD_ERR_ARG,
             "kd_seg_region_loss_fwd_bwd: need a >= 0, b >= 0, s > 0 (got %g, %g, %g)", (double)a, (double)b, (double)s);
  KD_REQUIRE(std::isfinite(wf) && std::isfinite(wt) && wf >= 0.f && wt >= 0.f && (wf > 0.f || wt > 0.f), KD_ERR_ARG,
             "kd_seg_region_loss_fwd_bwd: need wf >= 0, wt >= 0 and not both 0 (got %g, %g)", (double)wf, (double)wt);
  const int64_t npix = (int64_t)B * HW;
  const int64_t grid = region_blocks(npix);
  KD_REQUIRE(ws_bytes >= (size_t)grid * ROW * sizeof(float), KD_ERR_WORKSPACE, "kd_seg_region_loss_fwd_bwd: workspace too small");
  RegionArgs r{zs, zt, target, class_w, ignore_index, T, alpha, gscale, gscale_dev, gamma, wf, wt, a, b, s,
               (float*)ws, vals, dzs, npix, HW, NC};
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(region_partial_kernel, dim3((unsigned)grid), dim3(256), 0, st, r);
  hipLaunchKernelGGL(region_final_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, (int)grid, (double)npix, NC, wf, wt, a, b, s, vals);
  if (dzs) hipLaunchKernelGGL(region_grad_kernel, dim3((unsigned)grid), dim3(256), 0, st, r);
  return kd_check_launch("kd_seg_region_loss_fwd_bwd");
}

}  // extern "C"
