// kd_loss_lovasz.hip -- the opt-in Lovasz-Softmax hard-label term of the KD step (Berman et al., CVPR 2018),
//   classes = "present", per_image = True:   L = (1/B) sum_b (1/|P_b|) sum_{c in P_b} L_{b,c},   L_{b,c} = sum_k e_k g_k
//   e: the per-pixel error of class c (p_c off the class, the sum of the other probabilities on it), sorted descending with
//   equal fp32 bits in ascending pixel order; g: the increments of the Jaccard loss along that order, in closed form.
// Three launches: one workgroup per (image, class) builds 64-bit keys, sorts them in LDS (bitonic), scans the foreground
// bits, forms g_k, sums e_k g_k and scatters dL/dp_{i,c} into the workspace; one block sums the L_{b,c} in double; a point-wise
// pass recomputes the softmax, joins a pixel's NC coefficients and stores or adds dzs.
// No atomics and a fixed order everywhere: the same input gives the same bits on every call and every graph replay.
#include "kd_loss_common.h"

#include <cmath>

namespace {

constexpr int MAXC = 4;
constexpr int MAX_HW = 16384;             // 8-byte keys: 128 KiB of the CU's 160 KiB of LDS
constexpr int MAX_T = 1024;
constexpr unsigned long long PAD = ~0ull; // dropped pixels and the padding to a power of two: sorts last

struct LovaszArgs {
  const float* zs; const int64_t* target; int ignore_index;
  float* lbc; int* pbc; float* coef; int32_t* order;
  int B, NC, HW, NPAD;
};

// the probabilities of softmax_c at T = 1; the log-probabilities are not used
__device__ __forceinline__ void softmax_p(const float* z, int NC, float* p) {
  float lp[MAXC];
  softmax_c<MAXC>(z, NC, 1.f, p, lp);
}

inline int lovasz_npad(int HW) {
  int n = 64;
  while (n < HW) n <<= 1;
  return n;
}
inline int lovasz_threads(int npad) {
  const int t = npad / 8;
  return t < 64 ? 64 : (t > MAX_T ? MAX_T : t);
}

// One workgroup per (image b, class c).  Key = ~bits(e) : (pixel << 1 | fg), sorted ascending: e descending (e >= 0, so its
// bits order as unsigned integers), then pixel ascending.  A thread owns NPAD / blockDim consecutive sorted positions.
__global__ __launch_bounds__(MAX_T) void lovasz_sort_kernel(LovaszArgs a) {
  extern __shared__ unsigned long long keys[];
  __shared__ int s_present[MAXC];
  __shared__ int s_fg[MAX_T / 64];
  __shared__ float s_sum[MAX_T / 64];
  const int b = blockIdx.x / a.NC, c = blockIdx.x % a.NC;
  const int T = blockDim.x, t = threadIdx.x;
  const float* z0 = a.zs + (int64_t)b * a.NC * a.HW;
  const int64_t* y0 = a.target + (int64_t)b * a.HW;
  float* coef = a.coef ? a.coef + ((int64_t)b * a.NC + c) * a.HW : nullptr;
  int32_t* order = a.order ? a.order + ((int64_t)b * a.NC + c) * a.HW : nullptr;
  if (t < MAXC) s_present[t] = 0;
  __syncthreads();
  for (int i = t; i < a.NPAD; i += T) {
    unsigned long long key = PAD;
    if (i < a.HW) {
      const int64_t y = y0[i];
      if (KD_KEPT_LABEL(y, a.ignore_index, a.NC)) {
        float z[MAXC], p[MAXC];
#pragma unroll
        for (int j = 0; j < MAXC; ++j) if (j < a.NC) z[j] = z0[(int64_t)j * a.HW + i];
        softmax_p(z, a.NC, p);
        float pc = 0.f, om = 0.f;          // the class's probability and the sum of the others (never a subtraction from 1)
#pragma unroll
        for (int j = 0; j < MAXC; ++j) if (j < a.NC) { if (j == c) pc = p[j]; else om += p[j]; }
        const unsigned fg = (int)y == c;
        const float e = fg ? om : pc;
        key = ((unsigned long long)(~__float_as_uint(e)) << 32) | (unsigned)((i << 1) | fg);
        s_present[(int)y] = 1;             // every writer stores the same value
      } else if (coef) {
        coef[i] = 0.f;
      }
    }
    keys[i] = key;
  }
  __syncthreads();
  int np = 0;
#pragma unroll
  for (int j = 0; j < MAXC; ++j) np += s_present[j];
  if (!s_present[c]) {                     // absent class (the whole workgroup agrees): no loss, a zero gradient, no order
    for (int i = t; i < a.HW; i += T) {
      if (coef) coef[i] = 0.f;
      if (order) order[i] = -1;
    }
    if (t == 0) { a.lbc[b * a.NC + c] = 0.f; a.pbc[b * a.NC + c] = 0; }
    return;
  }

  const int half = a.NPAD >> 1;
  for (int k = 2; k <= a.NPAD; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int q = t; q < half; q += T) {
        const int lo = ((q & ~(j - 1)) << 1) | (q & (j - 1)), hi = lo | j;
        const unsigned long long x = keys[lo], y = keys[hi];
        if ((x > y) == ((lo & k) == 0)) { keys[lo] = y; keys[hi] = x; }
      }
      kd_lds_barrier();
    }
  }

  // block scan of the foreground bits over the sorted positions
  const int E = a.NPAD / T, k0 = t * E;
  const int lane = t & 63, wave = t >> 6, nwave = T >> 6;
  int mine = 0;
  for (int u = 0; u < E; ++u) {
    const unsigned long long key = keys[k0 + u];
    if (key != PAD) mine += (int)(key & 1u);
  }
  int incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  if (lane == 63) s_fg[wave] = incl;
  __syncthreads();
  int F = incl - mine, G = 0;
  for (int w = 0; w < nwave; ++w) {
    if (w < wave) F += s_fg[w];
    G += s_fg[w];
  }
  const float denom = (float)(a.B * np);
  float acc = 0.f;
  for (int u = 0; u < E; ++u) {
    const int k = k0 + u;
    const unsigned long long key = keys[k];
    if (key == PAD) {
      if (order && k < a.HW) order[k] = -1;
      continue;
    }
    const unsigned low = (unsigned)key;
    const int fg = low & 1u, idx = low >> 1;
    const float e = __uint_as_float(~(unsigned)(key >> 32));
    F += fg;
    const int I = G - F, U = G + (k + 1) - F;
    // J_k - J_{k-1} without the cancellation: 1 / U_k on the class, I_k / (U_{k-1} U_k) off it, where U_{k-1} = U_k - 1
    const float g = fg ? 1.f / (float)U : (float)I / ((float)(U - 1) * (float)U);
    acc = fmaf(e, g, acc);
    if (coef) coef[idx] = (fg ? -g : g) / denom;
    if (order) order[k] = idx;
  }
  const float ws = kd_wave_sum(acc);
  if (lane == 0) s_sum[wave] = ws;
  __syncthreads();
  if (t == 0) {
    float s = 0.f;
    for (int w = 0; w < nwave; ++w) s += s_sum[w];
    a.lbc[b * a.NC + c] = s;
    a.pbc[b * a.NC + c] = 1;
  }
}

// One block.  vals: [0] L  [1..4] per class the mean of L_{b,c} over the images where the class is present (0 if never)
__global__ __launch_bounds__(256) void lovasz_final_kernel(const float* lbc, const int* pbc, int B, int NC, float weight, float* vals,
                                                           float* hard_inout) {
  constexpr int NR = 1 + 2 * MAXC;
  __shared__ double red[NR][256];
  double s[NR];
#pragma unroll
  for (int k = 0; k < NR; ++k) s[k] = 0.0;
  for (int b = threadIdx.x; b < B; b += 256) {
    int np = 0;
    double sb = 0.0;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) if (c < NC && pbc[b * NC + c]) {
      const double l = (double)lbc[b * NC + c];
      ++np;
      sb += l;
      s[1 + c] += l;
      s[1 + MAXC + c] += 1.0;
    }
    if (np) s[0] += sb / np;
  }
#pragma unroll
  for (int k = 0; k < NR; ++k) red[k][threadIdx.x] = s[k];
  __syncthreads();
  if (threadIdx.x == 0) {
    double t[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) t[k] = 0.0;
    for (int i = 0; i < 256; ++i) {
#pragma unroll
      for (int k = 0; k < NR; ++k) t[k] += red[k][i];
    }
    const double L = t[0] / B;
    vals[0] = (float)L;
    for (int c = 0; c < MAXC; ++c) vals[1 + c] = t[1 + MAXC + c] > 0.0 ? (float)(t[1 + c] / t[1 + MAXC + c]) : 0.f;
    if (hard_inout) hard_inout[0] = (float)((double)hard_inout[0] + (double)weight * L);
  }
}

struct LovaszGradArgs {
  const float* zs; const int64_t* target; int ignore_index; const float* coef;
  float weight, gscale; const float* gdev; float* dzs; int accumulate;
  int64_t npix; int HW; int NC;
};

// dL/dz_j = p_j (q_j - sum_c p_c q_c) with q_c = dL/dp_c from the workspace; a dropped pixel stores 0 / adds nothing
__global__ __launch_bounds__(256) void lovasz_grad_kernel(LovaszGradArgs a) {
  const float sc = a.weight * (a.gscale * (a.gdev ? a.gdev[0] : 1.f));
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.npix; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / a.HW, hw = i % a.HW;
    const int64_t y = a.target[i];
    float g[MAXC];
#pragma unroll
    for (int j = 0; j < MAXC; ++j) g[j] = 0.f;
    const bool kept = KD_KEPT_LABEL(y, a.ignore_index, a.NC);
    if (kept) {
      float z[MAXC], p[MAXC], q[MAXC], dot = 0.f;
#pragma unroll
      for (int j = 0; j < MAXC; ++j) if (j < a.NC) { z[j] = a.zs[(b * a.NC + j) * a.HW + hw]; q[j] = a.coef[(b * a.NC + j) * a.HW + hw]; }
      softmax_p(z, a.NC, p);
#pragma unroll
      for (int j = 0; j < MAXC; ++j) if (j < a.NC) dot = fmaf(p[j], q[j], dot);
#pragma unroll
      for (int j = 0; j < MAXC; ++j) if (j < a.NC) g[j] = (sc * p[j]) * (q[j] - dot);
    }
    if (a.accumulate) {
      if (kept) {
#pragma unroll
        for (int j = 0; j < MAXC; ++j) if (j < a.NC) {
          float* d = a.dzs + (b * a.NC + j) * a.HW + hw;
          *d = __fadd_rn(*d, g[j]);          // the rounded sum of what was there and the accumulate = 0 result: no contraction
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < MAXC; ++j) if (j < a.NC) a.dzs[(b * a.NC + j) * a.HW + hw] = g[j];
    }
  }
}

inline size_t lovasz_ws(int64_t B, int64_t NC, int64_t HW) {
  if (B < 1 || NC < 1 || HW < 1) return 0;
  return (size_t)(2 * B * NC + B * NC * HW) * sizeof(float);
}

}  // namespace

extern "C" {

size_t kd_seg_lovasz_ws_bytes(int B, int NC, int HW) { return lovasz_ws(B, NC, HW); }

// ws: [B*NC] L_{b,c}, [B*NC] presence flags, [B*NC*HW] dL/dp_{i,c}
int kd_seg_lovasz_fwd_bwd(const float* zs, const int64_t* target, int ignore_index, float weight, float gscale, const float* gscale_dev,
                          float* vals, float* hard_inout, float* dzs, int accumulate, int32_t* order_out, int B, int NC, int HW,
                          void* ws, size_t ws_bytes, void* stream) {
  KD_REQUIRE(zs && target && vals, KD_ERR_ARG, "kd_seg_lovasz_fwd_bwd: null zs, target or vals");
  KD_REQUIRE(std::isfinite(weight) && weight > 0.f, KD_ERR_ARG, "kd_seg_lovasz_fwd_bwd: weight must be finite and > 0 (got %g)", (double)weight);
  KD_REQUIRE(NC >= 2 && NC <= MAXC, KD_ERR_SHAPE, "kd_seg_lovasz_fwd_bwd: num_classes=%d unsupported (2..4)", NC);
  KD_REQUIRE(B >= 1 && B <= (1 << 20) && HW >= 1, KD_ERR_SHAPE, "kd_seg_lovasz_fwd_bwd: B=%d, HW=%d unsupported", B, HW);
  KD_REQUIRE(HW <= MAX_HW, KD_ERR_SHAPE, "kd_seg_lovasz_fwd_bwd: HW=%d exceeds %d (128 x 128): an image's keys must fit the LDS of one CU",
             HW, MAX_HW);
  KD_REQUIRE(ws && ws_bytes >= lovasz_ws(B, NC, HW), KD_ERR_WORKSPACE, "kd_seg_lovasz_fwd_bwd: workspace too small");
  const int npad = lovasz_npad(HW), threads = lovasz_threads(npad);
  static std::atomic<uint64_t> raised{0};
  const hipError_t e = kd_raise_dynamic_lds((const void*)lovasz_sort_kernel, (size_t)MAX_HW * 8, raised);
  KD_REQUIRE(e == hipSuccess, (int)e, "kd_seg_lovasz_fwd_bwd: cannot raise the dynamic LDS limit to %d B: %s", MAX_HW * 8, hipGetErrorString(e));
  float* lbc = (float*)ws;
  int* pbc = (int*)(lbc + (size_t)B * NC);
  float* coef = lbc + (size_t)2 * B * NC;
  hipStream_t st = (hipStream_t)stream;
  LovaszArgs s{zs, target, ignore_index, lbc, pbc, dzs ? coef : nullptr, order_out, B, NC, HW, npad};
  hipLaunchKernelGGL(lovasz_sort_kernel, dim3((unsigned)(B * NC)), dim3(threads), (size_t)npad * 8, st, s);
  hipLaunchKernelGGL(lovasz_final_kernel, dim3(1), dim3(256), 0, st, (const float*)lbc, (const int*)pbc, B, NC, weight, vals, hard_inout);
  if (dzs) {
    const int64_t npix = (int64_t)B * HW;
    int64_t grid = (npix + 255) / 256;
    if (grid > 1024) grid = 1024;
    LovaszGradArgs g{zs, target, ignore_index, coef, weight, gscale, gscale_dev, dzs, accumulate, npix, HW, NC};
    hipLaunchKernelGGL(lovasz_grad_kernel, dim3((unsigned)grid), dim3(256), 0, st, g);
  }
  return kd_check_launch("kd_seg_lovasz_fwd_bwd");
}

}  // extern "C"
