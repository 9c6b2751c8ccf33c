// kd_loss.hip -- loss, metric and optimiser kernels of the KD step.
//   * weighted cross-entropy with ignore_index (trainer.py:55,88) fused with the temperature-softmax
//     KL term of the KD objective (build-defined) -- forward value and
//     dL/dlogits in one call;
//   * feature MSE forward + gradient;
//   * argmax + confusion matrix (SegmentationMetrics.update, trainer.py:18-26) -- integer exact;
//   * AdamW over flat parameter / gradient / moment buffers (trainer.py:56, torch.optim.AdamW math).
#include "kd_loss_common.h"

namespace {

constexpr int MAXC = 4;                           // the class bucket of the default path and the width of kd_argmax_confusion
constexpr int SEG_MAXC = 16;                      // kd_seg_loss_fwd_bwd: class buckets 4, 8, 16 (the launcher takes the smallest that holds NC)

struct SegArgs {
  const float* zs; const float* zt; const int64_t* target; const float* cw;
  int ignore_index; float T; float alpha; float gscale; const float* gdev;
  float* slab; float* losses; float* dzs;
  int64_t npix; int HW; int NC;
};

__device__ __forceinline__ void block_sum3(float a, float b, float c, float* out3) {
  __shared__ float red[3][4];
  a = kd_wave_sum(a); b = kd_wave_sum(b); c = kd_wave_sum(c);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { red[0][wave] = a; red[1][wave] = b; red[2][wave] = c; }
  __syncthreads();
  if (threadIdx.x < 3) out3[threadIdx.x] = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
}

template <int K>
__global__ __launch_bounds__(256) void seg_loss_partial_kernel(SegArgs a) {
  float swn = 0.f, sw = 0.f, skl = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.npix; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / a.HW, hw = i % a.HW;
    float z[K], p[K], lp[K];
#pragma unroll
    for (int j = 0; j < K; ++j) if (j < a.NC) z[j] = a.zs[(b * a.NC + j) * a.HW + hw];
    const int64_t y = a.target[i];
    if (KD_KEPT_LABEL(y, a.ignore_index, a.NC)) {
      softmax_c<K>(z, a.NC, 1.f, p, lp);
      float nll = 0.f;
#pragma unroll
      for (int j = 0; j < K; ++j) if (j == (int)y) nll = -lp[j];
      const float w = a.cw ? a.cw[y] : 1.f;
      swn = fmaf(w, nll, swn);
      sw += w;
    }
    if (a.zt) {
      float zt[K], pt[K], lpt[K];
#pragma unroll
      for (int j = 0; j < K; ++j) if (j < a.NC) zt[j] = a.zt[(b * a.NC + j) * a.HW + hw];
      softmax_c<K>(z, a.NC, 1.f / a.T, p, lp);
      softmax_c<K>(zt, a.NC, 1.f / a.T, pt, lpt);
#pragma unroll
      for (int j = 0; j < K; ++j) if (j < a.NC) skl += pt[j] > 0.f ? pt[j] * (lpt[j] - lp[j]) : 0.f;
    }
  }
  block_sum3(swn, sw, skl, a.slab + (int64_t)blockIdx.x * 4);
}

__global__ void seg_loss_final_kernel(const float* slab, int nblk, double npix, float* losses) {
  // losses: [0] CE (weighted mean), [1] KL (per-pixel mean), [2] sum of weights
  __shared__ double red[3][256];
  double s[3] = {0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < nblk; i += 256)
    for (int k = 0; k < 3; ++k) s[k] += (double)slab[(int64_t)i * 4 + k];
  for (int k = 0; k < 3; ++k) red[k][threadIdx.x] = s[k];
  __syncthreads();
  if (threadIdx.x == 0) {
    double t[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < 256; ++i) for (int k = 0; k < 3; ++k) t[k] += red[k][i];
    losses[0] = (float)(t[0] / t[1]);
    losses[1] = (float)(t[2] / npix);
    losses[2] = (float)t[1];
  }
}

template <int K>
__global__ __launch_bounds__(256) void seg_loss_grad_kernel(SegArgs a) {
  const float sumw = a.losses[2];
  const float gs = a.gscale * (a.gdev ? a.gdev[0] : 1.f);      // upstream gradient as a device scalar
  const float klc = a.zt ? gs * a.alpha * a.T / (float)a.npix : 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.npix; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / a.HW, hw = i % a.HW;
    float z[K], p[K], lp[K], g[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { g[j] = 0.f; if (j < a.NC) z[j] = a.zs[(b * a.NC + j) * a.HW + hw]; }
    const int64_t y = a.target[i];
    if (KD_KEPT_LABEL(y, a.ignore_index, a.NC)) {
      softmax_c<K>(z, a.NC, 1.f, p, lp);
      const float w = (a.cw ? a.cw[y] : 1.f) * gs / sumw;
#pragma unroll
      for (int j = 0; j < K; ++j) if (j < a.NC) g[j] = w * (p[j] - (j == (int)y ? 1.f : 0.f));
    }
    if (a.zt) {
      float zt[K], pt[K], lpt[K];
#pragma unroll
      for (int j = 0; j < K; ++j) if (j < a.NC) zt[j] = a.zt[(b * a.NC + j) * a.HW + hw];
      softmax_c<K>(z, a.NC, 1.f / a.T, p, lp);
      softmax_c<K>(zt, a.NC, 1.f / a.T, pt, lpt);
#pragma unroll
      for (int j = 0; j < K; ++j) if (j < a.NC) g[j] = fmaf(klc, p[j] - pt[j], g[j]);
    }
#pragma unroll
    for (int j = 0; j < K; ++j) if (j < a.NC) a.dzs[(b * a.NC + j) * a.HW + hw] = g[j];
  }
}

__global__ __launch_bounds__(256) void mse_kernel(const float* a, const float* b, int64_t n4, float gcoef,
                                                  const float* gdev, float* da, float* slab) {
  float s = 0.f;
  if (gdev) gcoef *= gdev[0];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const float4 x = kd_ld4(a + i * 4), y = kd_ld4(b + i * 4);
    const float4 d = make_float4(x.x - y.x, x.y - y.y, x.z - y.z, x.w - y.w);
    s = fmaf(d.x, d.x, fmaf(d.y, d.y, fmaf(d.z, d.z, fmaf(d.w, d.w, s))));
    if (da) kd_st4(da + i * 4, make_float4(gcoef * d.x, gcoef * d.y, gcoef * d.z, gcoef * d.w));
  }
  __shared__ float sh3[3];
  block_sum3(s, 0.f, 0.f, sh3);
  __syncthreads();
  if (threadIdx.x == 0 && slab) slab[blockIdx.x] = sh3[0];
}

// total = ce + ckl * kl + beta * (mse_c + mse_l), rounded after every operation like the fp32 tensor expression it replaces
__global__ void kd_total_kernel(const float* ce_kl, const float* mse_c, const float* mse_l, float ckl, float beta, float* total) {
  if (threadIdx.x == 0) {
    const float t = __fadd_rn(ce_kl[0], __fmul_rn(ckl, ce_kl[1]));
    const float m = __fadd_rn(mse_c ? mse_c[0] : 0.f, mse_l ? mse_l[0] : 0.f);
    total[0] = __fadd_rn(t, __fmul_rn(beta, m));
  }
}

// the two feature-MSE values from their per-block partial sums (the reduction of mse_final_kernel, same order) and the KD objective's
// total in one launch: out[0] = mse_c, out[1] = mse_l, out[2] = ce_kl[0] + ckl * ce_kl[1] + beta * (mse_c + mse_l)
__global__ void kd_objective_final_kernel(const float* ce_kl, const float* slab_c, int nblk_c, double n_c, const float* slab_l, int nblk_l,
                                          double n_l, float ckl, float beta, float* out) {
  __shared__ double red[2][256];
  double sc = 0.0, sl = 0.0;
  for (int i = threadIdx.x; i < nblk_c; i += 256) sc += (double)slab_c[i];
  for (int i = threadIdx.x; i < nblk_l; i += 256) sl += (double)slab_l[i];
  red[0][threadIdx.x] = sc;
  red[1][threadIdx.x] = sl;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tc = 0.0, tl = 0.0;
    for (int i = 0; i < 256; ++i) { tc += red[0][i]; tl += red[1][i]; }
    const float mc = (float)(tc / n_c), ml = (float)(tl / n_l);
    out[0] = mc;
    out[1] = ml;
    out[2] = __fadd_rn(__fadd_rn(ce_kl[0], __fmul_rn(ckl, ce_kl[1])), __fmul_rn(beta, __fadd_rn(mc, ml)));
  }
}

__global__ void mse_final_kernel(const float* slab, int nblk, double n, float* loss) {
  __shared__ double red[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 256) s += (double)slab[i];
  red[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < 256; ++i) t += red[i];
    *loss = (float)(t / n);
  }
}

__global__ __launch_bounds__(256) void confusion_kernel(const float* z, const int64_t* target, int ignore_index,
                                                        int64_t npix, int HW, int NC, int M, unsigned long long* conf,
                                                        int64_t* pred) {
  __shared__ unsigned int loc[MAXC * MAXC];
  if (threadIdx.x < MAXC * MAXC) loc[threadIdx.x] = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / HW, hw = i % HW;
    int best = 0;
    float bv = z[(b * NC) * HW + hw];
    for (int j = 1; j < NC; ++j) {
      const float v = z[(b * NC + j) * HW + hw];
      if (v > bv) { bv = v; best = j; }           // first maximum wins, like torch.argmax
    }
    if (pred) pred[i] = best;
    const int64_t t = target ? target[i] : ignore_index;
    if (target && t != ignore_index && t >= 0 && t < M && best < M) atomicAdd(&loc[t * M + best], 1u);
  }
  __syncthreads();
  if (conf && threadIdx.x < M * M && loc[threadIdx.x]) atomicAdd(&conf[threadIdx.x], (unsigned long long)loc[threadIdx.x]);
}

// confusion_kernel for up to 16 classes and a matrix of up to 16 x 16: one LDS counter per thread of the block.  The argmax
// loop is confusion_kernel's (first maximum wins; a NaN never beats the running maximum, a NaN in class 0 keeps index 0).
constexpr int CONF16 = 16;

__global__ __launch_bounds__(256) void confusion16_kernel(const float* z, const int64_t* target, int ignore_index,
                                                          int64_t npix, int HW, int NC, int M, unsigned long long* conf,
                                                          int64_t* pred) {
  __shared__ unsigned int loc[CONF16 * CONF16];
  loc[threadIdx.x] = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / HW, hw = i % HW;
    int best = 0;
    float bv = z[(b * NC) * HW + hw];
    for (int j = 1; j < NC; ++j) {
      const float v = z[(b * NC + j) * HW + hw];
      if (v > bv) { bv = v; best = j; }
    }
    if (pred) pred[i] = best;
    const int64_t t = target ? target[i] : ignore_index;
    if (target && t != ignore_index && t >= 0 && t < M && best < M) atomicAdd(&loc[t * M + best], 1u);
  }
  __syncthreads();
  if (conf && threadIdx.x < M * M && loc[threadIdx.x]) atomicAdd(&conf[threadIdx.x], (unsigned long long)loc[threadIdx.x]);
}

__global__ __launch_bounds__(256) void adamw_kernel(float* p, const float* g, float* m, float* v, int64_t n, float lr,
                                                    float b1, float b2, float eps, float wd, float bc1, float bc2sqrt,
                                                    float ginv) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float gi = g[i] * ginv;
    float pi = p[i] * (1.f - lr * wd);
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    const float denom = sqrtf(vi) / bc2sqrt + eps;
    pi -= (lr / bc1) * (mi / denom);
    p[i] = pi; m[i] = mi; v[i] = vi;
  }
}

}  // namespace

extern "C" {

size_t kd_seg_loss_ws_bytes(int64_t npix) {
  int64_t g = (npix + 255) / 256;
  if (g > 1024) g = 1024;
  return (size_t)g * 4 * sizeof(float);
}

// losses[0] = CE_w(zs, target), losses[1] = mean-per-pixel KL(softmax(zt/T) || softmax(zs/T)) (0 if zt null),
// losses[2] = sum of class weights over kept pixels.
// dzs = gscale * d/dzs ( CE + alpha*T^2*KL ).   zt == null: CE only.   dzs == null: forward only.
int kd_seg_loss_fwd_bwd(const float* zs, const float* zt, const int64_t* target, const float* class_w,
                        int ignore_index, float T, float alpha, float gscale, const float* gscale_dev, float* losses,
                        float* dzs, int B, int NC, int HW, void* ws, size_t ws_bytes, void* stream) {
  KD_REQUIRE(zs && target && losses && ws && B > 0 && HW > 0, KD_ERR_ARG, "kd_seg_loss_fwd_bwd: bad args");
  KD_REQUIRE(NC >= 2 && NC <= SEG_MAXC, KD_ERR_SHAPE, "kd_seg_loss_fwd_bwd: num_classes=%d unsupported (2..16)", NC);
  const int64_t npix = (int64_t)B * HW;
  int64_t grid = (npix + 255) / 256;
  if (grid > 1024) grid = 1024;
  KD_REQUIRE(ws_bytes >= (size_t)grid * 4 * sizeof(float), KD_ERR_WORKSPACE, "kd_seg_loss_fwd_bwd: workspace too small");
  SegArgs a{zs, zt, target, class_w, ignore_index, T, alpha, gscale, gscale_dev, (float*)ws, losses, dzs, npix, HW, NC};
  hipStream_t st = (hipStream_t)stream;
  const dim3 g((unsigned)grid), blk(256);
  KD_LAUNCH_CLASS_BUCKET(seg_loss_partial_kernel, NC, g, blk, st, a);
  hipLaunchKernelGGL(seg_loss_final_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, (int)grid, (double)npix, losses);
  if (dzs) KD_LAUNCH_CLASS_BUCKET(seg_loss_grad_kernel, NC, g, blk, st, a);
  return kd_check_launch("kd_seg_loss_fwd_bwd");
}

size_t kd_mse_ws_bytes(int64_t n) {
  int64_t g = (n / 4 + 255) / 256;
  if (g > 2048) g = 2048;
  if (g < 1) g = 1;
  return (size_t)g * sizeof(float);
}

// loss = mean((a-b)^2) (skipped when loss == null); da = gcoef * gscale_dev[0] * (a-b) (skipped when
// da == null; gscale_dev may be null).  Pass gcoef = 2*beta/n.
int kd_mse_fwd_bwd(const float* a, const float* b, int64_t n, float gcoef, const float* gscale_dev, float* loss,
                   float* da, void* ws, size_t ws_bytes, void* stream) {
  KD_REQUIRE(a && b && (loss || da) && ws && n > 0 && n % 4 == 0, KD_ERR_ARG, "kd_mse_fwd_bwd: bad args (n must be a multiple of 4)");
  int64_t grid = (n / 4 + 255) / 256;
  if (grid > 2048) grid = 2048;
  KD_REQUIRE(ws_bytes >= (size_t)grid * sizeof(float), KD_ERR_WORKSPACE, "kd_mse_fwd_bwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mse_kernel, dim3((unsigned)grid), dim3(256), 0, st, a, b, n / 4, gcoef, gscale_dev, da,
                     loss ? (float*)ws : nullptr);
  if (loss) hipLaunchKernelGGL(mse_final_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, (int)grid, (double)n, loss);
  return kd_check_launch("kd_mse_fwd_bwd");
}

// The KD objective's value from its parts: total = ce_kl[0] + ckl * ce_kl[1] + beta * (mse_c + mse_l),
// each operation rounded to fp32 in this order (what `ce + (alpha*T*T) * kl + beta * (mse_c + mse_l)` on fp32 scalars gives).
int kd_kd_total(const float* ce_kl, const float* mse_c, const float* mse_l, float ckl, float beta, float* total, void* stream) {
  KD_REQUIRE(ce_kl && total, KD_ERR_ARG, "kd_kd_total: bad args");
  hipLaunchKernelGGL(kd_total_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, ce_kl, mse_c, mse_l, ckl, beta, total);
  return kd_check_launch("kd_kd_total");
}

// kd_mse_fwd_bwd without its one-block final reduction: the per-block sums of (a-b)^2 go to `slab` (kd_mse_slab_blocks(n) floats) for
// kd_kd_objective_final, da = gcoef * (a-b) as in kd_mse_fwd_bwd (skipped when NULL).
int64_t kd_mse_slab_blocks(int64_t n) { int64_t g = (n / 4 + 255) / 256; return g > 2048 ? 2048 : (g < 1 ? 1 : g); }
int kd_mse_partial(const float* a, const float* b, int64_t n, float gcoef, float* da, float* slab, void* stream) {
  KD_REQUIRE(a && b && slab && n > 0 && n % 4 == 0, KD_ERR_ARG, "kd_mse_partial: bad args (n must be a multiple of 4)");
  hipLaunchKernelGGL(mse_kernel, dim3((unsigned)kd_mse_slab_blocks(n)), dim3(256), 0, (hipStream_t)stream, a, b, n / 4, gcoef, (const float*)nullptr, da, slab);
  return kd_check_launch("kd_mse_partial");
}

// out[0] = mean((a_c-b_c)^2), out[1] = mean((a_l-b_l)^2) from the slabs of two kd_mse_partial calls over n_c / n_l elements, and
// out[2] = ce_kl[0] + ckl * ce_kl[1] + beta * (out[0] + out[1]) (the rounding order of kd_kd_total): three tiny launches in one.
int kd_kd_objective_final(const float* ce_kl, const float* slab_c, int64_t n_c, const float* slab_l, int64_t n_l, float ckl, float beta,
                          float* out, void* stream) {
  KD_REQUIRE(ce_kl && slab_c && slab_l && out && n_c > 0 && n_l > 0, KD_ERR_ARG, "kd_kd_objective_final: bad args");
  hipLaunchKernelGGL(kd_objective_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, ce_kl, slab_c, (int)kd_mse_slab_blocks(n_c), (double)n_c,
                     slab_l, (int)kd_mse_slab_blocks(n_l), (double)n_l, ckl, beta, out);
  return kd_check_launch("kd_kd_objective_final");
}

// conf[M*M] (uint64, ACCUMULATED into) and/or pred[B*HW] (int64 argmax over all NC classes).  M is the width of the matrix
// (SegmentationMetrics.num_classes), independent of NC: a pixel counts at [t, argmax] only when both are below M (trainer.py:18-26).
int kd_argmax_confusion(const float* logits, const int64_t* target, int ignore_index, uint64_t* conf, int64_t* pred,
                        int B, int NC, int M, int HW, void* stream) {
  KD_REQUIRE(logits && (conf || pred) && B > 0 && HW > 0 && NC >= 1 && NC <= MAXC, KD_ERR_ARG, "kd_argmax_confusion: bad args");
  KD_REQUIRE(M >= 1 && M <= MAXC, KD_ERR_SHAPE, "kd_argmax_confusion: confusion matrix width %d unsupported (1..4)", M);
  const int64_t npix = (int64_t)B * HW;
  int64_t grid = (npix + 255) / 256;
  if (grid > 1024) grid = 1024;
  hipLaunchKernelGGL(confusion_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, logits, target,
                     ignore_index, npix, HW, NC, M, (unsigned long long*)conf, pred);
  return kd_check_launch("kd_argmax_confusion");
}

// kd_argmax_confusion for 1 <= NC <= 16 classes and a matrix width 1 <= M <= 16: same arguments, same counting rule, same ties
// (the lowest class index) and the same NaN behaviour; 256 LDS counters per block, int64 accumulation.
int kd_argmax_confusion16(const float* logits, const int64_t* target, int ignore_index, uint64_t* conf, int64_t* pred,
                          int B, int NC, int M, int HW, void* stream) {
  KD_REQUIRE(logits && (conf || pred) && B > 0 && HW > 0, KD_ERR_ARG, "kd_argmax_confusion16: bad args");
  KD_REQUIRE(NC >= 1 && NC <= CONF16, KD_ERR_SHAPE, "kd_argmax_confusion16: num_classes=%d unsupported (1..16)", NC);
  KD_REQUIRE(M >= 1 && M <= CONF16, KD_ERR_SHAPE, "kd_argmax_confusion16: confusion matrix width %d unsupported (1..16)", M);
  const int64_t npix = (int64_t)B * HW;
  int64_t grid = (npix + 255) / 256;
  if (grid > 1024) grid = 1024;
  hipLaunchKernelGGL(confusion16_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, logits, target,
                     ignore_index, npix, HW, NC, M, (unsigned long long*)conf, pred);
  return kd_check_launch("kd_argmax_confusion16");
}

// One AdamW step over flat buffers; `step` is the 1-based step count; grads are scaled by ginv first
// (1/world_size after a sum all-reduce).
int kd_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                  float eps, float weight_decay, int step, float ginv, void* stream) {
  KD_REQUIRE(p && g && m && v && n > 0 && step >= 1, KD_ERR_ARG, "kd_adamw_step: bad args");
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  int64_t grid = (n + 255) / 256;
  if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, lr, beta1,
                     beta2, eps, weight_decay, (float)bc1, (float)sqrt(bc2), ginv);
  return kd_check_launch("kd_adamw_step");
}

// Graph-replay-safe AdamW: everything that changes from step to step lives in a device array
//   state[0] = lr   state[1] = step count (as float)   state[2] = 1 - beta1^step   state[3] = sqrt(1 - beta2^step)
// The tick kernel advances the step and refreshes the bias corrections; the update kernel reads them.
// A captured hipGraph of the training step therefore stays correct on every replay (a host-side
// `step` argument would be frozen at capture time).  lr is changed by writing state[0] between replays.
__global__ void adamw_tick_kernel(float* state, float b1, float b2) {
  const float t = state[1] + 1.f;
  state[1] = t;
  state[2] = (float)(1.0 - pow((double)b1, (double)t));
  state[3] = (float)sqrt(1.0 - pow((double)b2, (double)t));
}
__global__ __launch_bounds__(256) void adamw_dev_kernel(float* p, const float* g, float* m, float* v, int64_t n,
                                                        const float* state, float b1, float b2, float eps, float wd,
                                                        float ginv) {
  const float lr = state[0], bc1 = state[2], bc2sqrt = state[3];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float gi = g[i] * ginv;
    float pi = p[i] * (1.f - lr * wd);
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    const float denom = sqrtf(vi) / bc2sqrt + eps;
    pi -= (lr / bc1) * (mi / denom);
    p[i] = pi; m[i] = mi; v[i] = vi;
  }
}
int kd_adamw_step_dev(float* p, const float* g, float* m, float* v, int64_t n, float* state, float beta1, float beta2,
                      float eps, float weight_decay, float ginv, void* stream) {
  KD_REQUIRE(p && g && m && v && state && n > 0, KD_ERR_ARG, "kd_adamw_step_dev: bad args");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(adamw_tick_kernel, dim3(1), dim3(1), 0, st, state, beta1, beta2);
  int64_t grid = (n + 255) / 256;
  if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL(adamw_dev_kernel, dim3((unsigned)grid), dim3(256), 0, st, p, g, m, v, n, (const float*)state, beta1,
                     beta2, eps, weight_decay, ginv);
  return kd_check_launch("kd_adamw_step_dev");
}

}  // extern "C"

// ---- global-norm gradient clipping folded into the device-state AdamW step ------------------------------------------------
// Launch layout of the sum of squares (mirrored by tests/_fp64_clip_ref.py): 256 threads, one float4 per thread and iteration,
// at most GSQ_CAP blocks.  A thread adds its squares in fp32 (one fused multiply-add per element), a wave adds its 64 lanes in
// fp32 (6 butterfly steps), everything after that is double: the 4 waves of a block, the per-block partials, the final sum.
// No atomics and a fixed order everywhere, so the same input gives the same bits on every run and every graph replay.
namespace {

constexpr int GSQ_CAP = 2048;

inline int64_t gsq_blocks(int64_t n) {
  int64_t g = (n / 4 + 255) / 256;
  return g > GSQ_CAP ? GSQ_CAP : (g < 1 ? 1 : g);
}

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* g, int64_t n4, double* partial) {
  float s = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const float4 x = kd_ld4(g + i * 4);
    s = fmaf(x.x, x.x, fmaf(x.y, x.y, fmaf(x.z, x.z, fmaf(x.w, x.w, s))));
  }
  __shared__ float red[4];
  s = kd_wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (((double)red[0] + (double)red[1]) + (double)red[2]) + (double)red[3];
}

// One block.  Sums the partials (thread t takes t, t + 256, ...; then a halving tree over the 256 threads), forms the norm, the
// clip coefficient and the gradient scale, and advances the AdamW state only when the norm is finite.
//   clip[0] = grad_norm = ginv * sqrt(sum)  (evaluated in double, rounded once)
//   clip[1] = gscale = ginv * min(1, max_norm / (grad_norm + 1e-6))  (fp32 operations, torch.nn.utils.clip_grad_norm_'s formula)
//   clip[2] = skipped steps (counts up on a non-finite norm)      clip[3] = 1 if this step is applied, 0 if it is skipped
__global__ __launch_bounds__(256) void adamw_clip_tick_kernel(const double* partial, int nblk, float* state, float* clip, float b1,
                                                              float b2, float ginv, float max_norm) {
  __shared__ double red[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 256) s += partial[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float norm = (float)((double)ginv * sqrt(red[0]));
    clip[0] = norm;
    if (isfinite(norm)) {
      const float coef = fminf(1.f, __fdiv_rn(max_norm, __fadd_rn(norm, 1e-6f)));
      clip[1] = __fmul_rn(ginv, coef);
      clip[3] = 1.f;
      const float t = state[1] + 1.f;              // adamw_tick_kernel
      state[1] = t;
      state[2] = (float)(1.0 - pow((double)b1, (double)t));
      state[3] = (float)sqrt(1.0 - pow((double)b2, (double)t));
    } else {
      clip[1] = 0.f;
      clip[2] = clip[2] + 1.f;
      clip[3] = 0.f;
    }
  }
}

// adamw_dev_kernel's arithmetic, expression for expression, on one element with the gradient scale read from the device
__device__ __forceinline__ void adamw_clip_elem(float& p, float g, float& m, float& v, float lr, float bc1, float bc2sqrt, float b1,
                                                float b2, float eps, float wd, float gs) {
  const float gi = g * gs;
  float pi = p * (1.f - lr * wd);
  const float mi = b1 * m + (1.f - b1) * gi;
  const float vi = b2 * v + (1.f - b2) * gi * gi;
  const float denom = sqrtf(vi) / bc2sqrt + eps;
  pi -= (lr / bc1) * (mi / denom);
  p = pi; m = mi; v = vi;
}

__global__ __launch_bounds__(256) void adamw_clip_kernel(float* p, const float* g, float* m, float* v, int64_t n4, const float* state,
                                                         const float* clip, float b1, float b2, float eps, float wd) {
  if (clip[3] == 0.f) return;                      // non-finite gradient norm: the step is skipped, nothing is written
  const float lr = state[0], bc1 = state[2], bc2sqrt = state[3], gs = clip[1];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    float4 pv = kd_ld4(p + i * 4), mv = kd_ld4(m + i * 4), vv = kd_ld4(v + i * 4);
    const float4 gv = kd_ld4(g + i * 4);
    adamw_clip_elem(pv.x, gv.x, mv.x, vv.x, lr, bc1, bc2sqrt, b1, b2, eps, wd, gs);
    adamw_clip_elem(pv.y, gv.y, mv.y, vv.y, lr, bc1, bc2sqrt, b1, b2, eps, wd, gs);
    adamw_clip_elem(pv.z, gv.z, mv.z, vv.z, lr, bc1, bc2sqrt, b1, b2, eps, wd, gs);
    adamw_clip_elem(pv.w, gv.w, mv.w, vv.w, lr, bc1, bc2sqrt, b1, b2, eps, wd, gs);
    kd_st4(p + i * 4, pv); kd_st4(m + i * 4, mv); kd_st4(v + i * 4, vv);
  }
}

}  // namespace

extern "C" {

size_t kd_grad_sumsq_ws_bytes(int64_t n) { return (size_t)gsq_blocks(n) * sizeof(double); }

// ws[b] (double) = the sum of g[i]^2 over the float4s block b owns, b < kd_grad_sumsq_ws_bytes(n) / 8
int kd_grad_sumsq_partials(const float* g, int64_t n, void* ws, size_t ws_bytes, void* stream) {
  KD_REQUIRE(g && ws && n > 0 && n % 4 == 0, KD_ERR_ARG, "kd_grad_sumsq_partials: bad args (n must be a positive multiple of 4)");
  KD_REQUIRE(kd_aligned16(g) && (reinterpret_cast<uintptr_t>(ws) & 7u) == 0, KD_ERR_ALIGN,
             "kd_grad_sumsq_partials: g must be 16-byte aligned, ws 8-byte aligned");
  const int64_t grid = gsq_blocks(n);
  KD_REQUIRE(ws_bytes >= (size_t)grid * sizeof(double), KD_ERR_WORKSPACE, "kd_grad_sumsq_partials: workspace too small");
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, g, n / 4, (double*)ws);
  return kd_check_launch("kd_grad_sumsq_partials");
}

// kd_adamw_step_dev with the gradients clipped to a global L2 norm of max_norm (see include/kd_hip.h).  Three launches: the
// partial sums of squares, the one-block tick, the update.  A non-finite norm skips the step on the device.
int kd_adamw_step_clip_dev(float* p, const float* g, float* m, float* v, int64_t n, float* state, float* clip_state, void* ws,
                           size_t ws_bytes, float beta1, float beta2, float eps, float weight_decay, float ginv, float max_norm,
                           void* stream) {
  KD_REQUIRE(p && g && m && v && state && clip_state && ws && n > 0 && n % 4 == 0, KD_ERR_ARG,
             "kd_adamw_step_clip_dev: bad args (n must be a positive multiple of 4)");
  KD_REQUIRE(std::isfinite(max_norm) && max_norm > 0.f, KD_ERR_ARG, "kd_adamw_step_clip_dev: max_norm must be finite and > 0 (got %g)",
             (double)max_norm);
  KD_REQUIRE(kd_aligned16(p) && kd_aligned16(g) && kd_aligned16(m) && kd_aligned16(v) && (reinterpret_cast<uintptr_t>(ws) & 7u) == 0,
             KD_ERR_ALIGN, "kd_adamw_step_clip_dev: p, g, m, v must be 16-byte aligned, ws 8-byte aligned");
  const int64_t nblk = gsq_blocks(n);
  KD_REQUIRE(ws_bytes >= (size_t)nblk * sizeof(double), KD_ERR_WORKSPACE, "kd_adamw_step_clip_dev: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)nblk), dim3(256), 0, st, g, n / 4, (double*)ws);
  hipLaunchKernelGGL(adamw_clip_tick_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, (int)nblk, state, clip_state, beta1, beta2,
                     ginv, max_norm);
  int64_t grid = (n / 4 + 255) / 256;
  if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL(adamw_clip_kernel, dim3((unsigned)grid), dim3(256), 0, st, p, g, m, v, n / 4, (const float*)state,
                     (const float*)clip_state, beta1, beta2, eps, weight_decay);
  return kd_check_launch("kd_adamw_step_clip_dev");
}

}  // extern "C"

// ---- parameter groups and an EMA weight copy in the device-state AdamW step ---------------------------------------------------
// The flat buffer is cut into segments (ascending ends in float4 units, one group index each); a float4 never straddles two
// tensors, so one lookup per float4 gives its group's (lr, weight_decay).  Every workgroup copies the table into LDS once and a
// thread searches it only when its float4 leaves the segment of its previous iteration.  The EMA copy is one more 16-byte load
// and store per float4 of parameters that are in registers anyway.
namespace {

constexpr int GROUPS_MAX_SEG = 4096;               // 32 KiB of LDS for the table

// One block.  With `clip`: adamw_clip_tick_kernel, expression for expression (the same reduction, the same bits).  Without:
// adamw_tick_kernel.  An applied step then refreshes ema[0] = d_t and ema[1] = 1 - d_t from the step count after the tick.
__global__ __launch_bounds__(256) void adamw_groups_tick_kernel(const double* partial, int nblk, float* state, float* clip, float* ema,
                                                                float b1, float b2, float ginv, float max_norm, float decay,
                                                                int warmup) {
  __shared__ double red[256];
  bool apply = true;
  if (clip) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 256) s += partial[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
      if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      const float norm = (float)((double)ginv * sqrt(red[0]));
      clip[0] = norm;
      apply = isfinite(norm);
      if (apply) {
        const float coef = fminf(1.f, __fdiv_rn(max_norm, __fadd_rn(norm, 1e-6f)));
        clip[1] = __fmul_rn(ginv, coef);
        clip[3] = 1.f;
      } else {
        clip[1] = 0.f;
        clip[2] = clip[2] + 1.f;
        clip[3] = 0.f;
      }
    }
  }
  if (threadIdx.x == 0 && apply) {
    const float t = state[1] + 1.f;                // adamw_tick_kernel
    state[1] = t;
    state[2] = (float)(1.0 - pow((double)b1, (double)t));
    state[3] = (float)sqrt(1.0 - pow((double)b2, (double)t));
    if (ema) {
      const float d = warmup ? fminf(decay, __fdiv_rn(__fadd_rn(1.f, t), __fadd_rn(10.f, t))) : decay;
      ema[0] = d;
      ema[1] = __fsub_rn(1.f, d);
    }
  }
}

__global__ __launch_bounds__(256) void adamw_groups_kernel(float* p, const float* g, float* m, float* v, float* e, int64_t n4,
                                                           const float* state, const int* seg_end, const int* seg_group, int n_seg,
                                                           const float* group_state, const float* clip, const float* ema, float b1,
                                                           float b2, float eps, float ginv) {
  if (clip && clip[3] == 0.f) return;              // non-finite gradient norm: the step is skipped, nothing is written
  extern __shared__ int tab[];
  int* ends = tab;
  int* grps = tab + n_seg;
  for (int i = threadIdx.x; i < n_seg; i += 256) { ends[i] = seg_end[i]; grps[i] = seg_group[i]; }
  __syncthreads();
  const float bc1 = state[2], bc2sqrt = state[3], gs = clip ? clip[1] : ginv;
  const float d = e ? ema[0] : 1.f, omd = e ? ema[1] : 0.f;
  int64_t lo = 0, hi = 0;                          // the float4 range of the segment whose lr, wd are loaded (none yet)
  float lr = 0.f, wd = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    if (i >= hi || i < lo) {                       // the first segment whose end lies beyond i
      int a = 0, b = n_seg - 1;
      while (a < b) {
        const int c = (a + b) >> 1;
        if ((int64_t)ends[c] > i) b = c; else a = c + 1;
      }
      lo = a ? ends[a - 1] : 0;
      hi = ends[a];
      const int gi = grps[a];
      lr = group_state[2 * gi];
      wd = group_state[2 * gi + 1];
    }
    float4 pv = kd_ld4(p + i * 4), mv = kd_ld4(m + i * 4), vv = kd_ld4(v + i * 4);
    const float4 gv = kd_ld4(g + i * 4);
    adamw_clip_elem(pv.x, gv.x, mv.x, vv.x, lr, bc1, bc2sqrt, b1, b2, eps, wd, gs);
    adamw_clip_elem(pv.y, gv.y, mv.y, vv.y, lr, bc1, bc2sqrt, b1, b2, eps, wd, gs);
    adamw_clip_elem(pv.z, gv.z, mv.z, vv.z, lr, bc1, bc2sqrt, b1, b2, eps, wd, gs);
    adamw_clip_elem(pv.w, gv.w, mv.w, vv.w, lr, bc1, bc2sqrt, b1, b2, eps, wd, gs);
    kd_st4(p + i * 4, pv); kd_st4(m + i * 4, mv); kd_st4(v + i * 4, vv);
    if (omd != 0.f) {                              // d == 1: the average keeps its bits, no traffic
      float4 ev = pv;                              // d == 0: the average is the parameter, bit for bit, no load
      if (d != 0.f) {
        ev = kd_ld4(e + i * 4);
        ev.x = fmaf(d, ev.x, omd * pv.x);
        ev.y = fmaf(d, ev.y, omd * pv.y);
        ev.z = fmaf(d, ev.z, omd * pv.z);
        ev.w = fmaf(d, ev.w, omd * pv.w);
      }
      kd_st4(e + i * 4, ev);
    }
  }
}

}  // namespace

extern "C" {

// kd_adamw_step_dev / kd_adamw_step_clip_dev with per-segment (lr, weight_decay) and an optional EMA copy (see include/kd_hip.h).
// Two launches (the tick, the update), three with clipping.  The table is validated here from the caller's host copy.
int kd_adamw_step_groups_dev(float* p, const float* g, float* m, float* v, int64_t n, float* state, const int* seg_end,
                             const int* seg_group, const int* seg_end_host, const int* seg_group_host, int n_seg,
                             const float* group_state, int n_groups, float* ema, float* ema_state, float ema_decay, int ema_warmup,
                             float* clip_state, void* ws, size_t ws_bytes, float beta1, float beta2, float eps, float ginv,
                             float max_norm, void* stream) {
  KD_REQUIRE(p && g && m && v && state && seg_end && seg_group && seg_end_host && seg_group_host && group_state && n > 0 && n % 4 == 0 &&
                 n / 4 <= (int64_t)INT32_MAX && n_seg > 0 && n_groups > 0,
             KD_ERR_ARG, "kd_adamw_step_groups_dev: bad args (n must be a positive multiple of 4)");
  KD_REQUIRE((ema == nullptr) == (ema_state == nullptr), KD_ERR_ARG, "kd_adamw_step_groups_dev: ema and ema_state go together");
  KD_REQUIRE(!ema || (ema_decay >= 0.f && ema_decay <= 1.f), KD_ERR_ARG, "kd_adamw_step_groups_dev: ema_decay must lie in [0, 1] (got %g)",
             (double)ema_decay);
  KD_REQUIRE((clip_state == nullptr) == (ws == nullptr), KD_ERR_ARG, "kd_adamw_step_groups_dev: clip_state and ws go together");
  KD_REQUIRE(!clip_state || (std::isfinite(max_norm) && max_norm > 0.f), KD_ERR_ARG,
             "kd_adamw_step_groups_dev: max_norm must be finite and > 0 (got %g)", (double)max_norm);
  KD_REQUIRE(n_seg <= GROUPS_MAX_SEG, KD_ERR_SHAPE, "kd_adamw_step_groups_dev: %d segments, at most %d (merge neighbours of one group)",
             n_seg, GROUPS_MAX_SEG);
  int prev = 0;
  for (int i = 0; i < n_seg; ++i) {
    KD_REQUIRE(seg_end_host[i] > prev, KD_ERR_ARG, "kd_adamw_step_groups_dev: segment ends must ascend (end[%d] = %d after %d)", i,
               seg_end_host[i], prev);
    KD_REQUIRE(seg_group_host[i] >= 0 && seg_group_host[i] < n_groups, KD_ERR_ARG,
               "kd_adamw_step_groups_dev: segment %d names group %d of %d", i, seg_group_host[i], n_groups);
    prev = seg_end_host[i];
  }
  KD_REQUIRE((int64_t)prev == n / 4, KD_ERR_ARG, "kd_adamw_step_groups_dev: the last segment ends at float4 %d, the buffer at %lld", prev,
             (long long)(n / 4));
  KD_REQUIRE(kd_aligned16(p) && kd_aligned16(g) && kd_aligned16(m) && kd_aligned16(v) && kd_aligned16(ema) &&
                 (reinterpret_cast<uintptr_t>(ws) & 7u) == 0,
             KD_ERR_ALIGN, "kd_adamw_step_groups_dev: p, g, m, v, ema must be 16-byte aligned, ws 8-byte aligned");
  const int64_t nblk = gsq_blocks(n);
  KD_REQUIRE(!clip_state || ws_bytes >= (size_t)nblk * sizeof(double), KD_ERR_WORKSPACE, "kd_adamw_step_groups_dev: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  if (clip_state) hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)nblk), dim3(256), 0, st, g, n / 4, (double*)ws);
  hipLaunchKernelGGL(adamw_groups_tick_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, (int)nblk, state, clip_state, ema_state, beta1,
                     beta2, ginv, max_norm, ema_decay, ema_warmup);
  int64_t grid = (n / 4 + 255) / 256;
  if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL(adamw_groups_kernel, dim3((unsigned)grid), dim3(256), (size_t)n_seg * 2 * sizeof(int), st, p, g, m, v, ema, n / 4,
                     (const float*)state, seg_end, seg_group, n_seg, group_state, (const float*)clip_state, (const float*)ema_state, beta1,
                     beta2, eps, ginv);
  return kd_check_launch("kd_adamw_step_groups_dev");
}

}  // extern "C"

// ---- gradient accumulation over micro-batches ------------------------------------------------------------------------------
// Backward kernels overwrite their slot of the flat gradient buffer, so the sum over k micro-batches lives in a second flat
// buffer.  FOLD = false: accum += grad (micro-batches 1 .. k-1).  FOLD = true: grad = accum + grad and accum = +0 in the same
// pass (micro-batch k: the optimiser step then reads the sum where it reads the gradient today, and the next cycle -- or the
// next replay of a captured graph -- starts from zeros without a memset).  One fp32 add per element, accum the left operand:
// nothing to contract, the bits of torch's `accum + grad`.
namespace {

constexpr int GACC_CAP = 2048;

template <bool FOLD>
__global__ __launch_bounds__(256) void grad_accumulate_kernel(float* accum, float* grad, int64_t n) {
  const int64_t n4 = n / 4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const float4 a = kd_ld4(accum + i * 4), g = kd_ld4(grad + i * 4);
    const float4 s = make_float4(a.x + g.x, a.y + g.y, a.z + g.z, a.w + g.w);
    if (FOLD) {
      kd_st4(grad + i * 4, s);
      kd_st4(accum + i * 4, kd_zero4());
    } else {
      kd_st4(accum + i * 4, s);
    }
  }
  const int64_t t = n4 * 4 + threadIdx.x;          // the scalar tail: at most three elements, block 0
  if (blockIdx.x == 0 && t < n) {
    const float s = accum[t] + grad[t];
    if (FOLD) {
      grad[t] = s;
      accum[t] = 0.f;
    } else {
      accum[t] = s;
    }
  }
}

}  // namespace

extern "C" {

int kd_grad_accumulate(float* accum, float* grad, int64_t n, int fold, void* stream) {
  KD_REQUIRE(n >= 0 && (fold == 0 || fold == 1), KD_ERR_ARG, "kd_grad_accumulate: bad args (n = %lld, fold = %d)", (long long)n, fold);
  if (n == 0) return KD_OK;
  KD_REQUIRE(accum && grad && accum != grad, KD_ERR_ARG, "kd_grad_accumulate: accum and grad must be two non-null buffers");
  KD_REQUIRE(kd_aligned16(accum) && kd_aligned16(grad), KD_ERR_ALIGN, "kd_grad_accumulate: accum and grad must be 16-byte aligned");
  int64_t grid = (n / 4 + 255) / 256;
  if (grid > GACC_CAP) grid = GACC_CAP;
  if (grid < 1) grid = 1;
  if (fold)
    hipLaunchKernelGGL(grad_accumulate_kernel<true>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, accum, grad, n);
  else
    hipLaunchKernelGGL(grad_accumulate_kernel<false>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, accum, grad, n);
  return kd_check_launch("kd_grad_accumulate");
}

}  // extern "C"
