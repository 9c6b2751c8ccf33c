// kd_loss_ifv.hip -- the opt-in intra-class feature variation distillation feature term of the KD step (DESIGN.md section 3;
// Wang et al., "Intra-class Feature Variation Distillation for Semantic Segmentation", ECCV 2020) on the NHWC matrices
// S [B*HW, Cs], T [B*HW, Ct] and the label map y [B*HW] (int64).  Pixel i of image b is kept when y != ignore_index and 0 <= y < NC;
// K_b kept pixels, N_bc of class c.  For X in {S, T}, per image:
//   r_i = |x_i|,  xh_i = x_i / r_i (0 for r_i <= 1e-12),  m_c = 1/N_bc sum_{i in c} x_i,  mh_c = m_c / |m_c| (0 for |m_c| <= 1e-12),
//   s_i = xh_i . mh_{y_i},   L_b = 1/K_b sum_kept (sS_i - sT_i)^2,   IFV = 1/B sum_b L_b,
//   w_i = (sS_i - sT_i) / K_b,   E_c = (sum_{i in c} w_i xh_i - (sum_{i in c} w_i s_i) mh_c) / (|m_c| N_bc)      (all from S),
//   ds_j = k (w_j (mh_c - s_j xh_j) / r_j + E_c), c = y_j, for kept j and 0 otherwise: k * (B/2) * dIFV/dS.
// Launches.  (1) class sums: a workgroup per (image, row slice, map); a thread owns one float4 column group and every RL-th row of the
// slice and adds rows into ITS OWN per-class accumulators in LDS (NC float4 per thread: no register array under a runtime class index,
// no bank conflict, no atomics), the row lanes are joined in lane order and the per-slice sums and counts go to the workspace.
// (2) join: slices in slice order in double -> m, |m|, mh, N_bc, K_b.  (3) similarity: 8 lanes per row as in kd_loss_pair.hip, S and T
// through ONE device function; {1/r, sS, w, sS - sT} per pixel to the workspace.  (4) with ds: the class sums again over S, each row
// weighted by w_i / r_i.  (5) join: L_b, sum w_i s_i per class and the slices of (4) in double -> E_c; (5b) the mean over images in
// one block.  (6) gradient: point-wise, mh and E of the image in LDS, 16-byte stores.
// That is 4 sweeps of S (2 forward only), 2 of T and one store: sum w_i xh_i per class needs w, which needs the prototypes, and a
// thread of the 8-lanes-per-row pass cannot hold NC accumulators per column, so it is a sweep of its own in the class-sum layout.
// No floating-point atomics, a fixed order everywhere; S and T go
// through the same instruction sequence: identical bits in both give sS - sT == 0 for every pixel, the value 0 and ds = +-0.
#include "kd_loss_common.h"

#include <cmath>

namespace {

constexpr int THREADS = 256;
constexpr int MIN_C = 4, MAX_C = 256, MIN_NC = 2, MAX_NC = 16;
constexpr int SR = 32;                    // rows of a step of the similarity pass (8 lanes per row); a slice is a multiple of it
constexpr int WANT_WGS = 1024;            // workgroups the sweeps aim for: 4 per CU

inline bool ifv_shape_ok(int B, int HW, int Cs, int Ct, int NC) {
  return B >= 1 && HW >= 1 && HW <= (1 << 30) && Cs >= MIN_C && Cs <= MAX_C && Cs % 4 == 0 && Ct >= MIN_C && Ct <= MAX_C && Ct % 4 == 0 &&
         NC >= MIN_NC && NC <= MAX_NC;
}
// rows per slice: a multiple of SR, at least 64 rows; a function of (B, HW) alone
inline int ifv_slice_rows(int B, int HW) {
  const int64_t want = B >= WANT_WGS ? 1 : (WANT_WGS + B - 1) / B;
  const int64_t cap = ((int64_t)HW + 63) / 64;
  const int64_t s = want < cap ? want : cap;
  const int64_t rows = ((int64_t)HW + s - 1) / s;
  return (int)((rows + SR - 1) / SR * SR);
}
inline int ifv_slices(int B, int HW) {
  const int rows = ifv_slice_rows(B, HW);
  return (int)(((int64_t)HW + rows - 1) / rows);
}
inline size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

// workspace: per pixel {1/r, sS, w, d} | per-slice class sums of S, of T, of the weighted S | per-slice counts | N_bc | K_b | mh of S, of T
// | 1/|m| of S | E | L_b in double
struct IfvWs { size_t pix, partS, partT, partV, cnt, N, K, mhS, mhT, invn, E, L, total; };
inline IfvWs ifv_ws(int B, int HW, int Cs, int Ct, int NC) {
  const size_t sl = (size_t)ifv_slices(B, HW);
  IfvWs w;
  size_t o = 0;
  w.pix = o; o += (size_t)B * HW * sizeof(float4);
  w.partS = o; o += (size_t)B * sl * NC * Cs * sizeof(float);
  w.partT = o; o += (size_t)B * sl * NC * Ct * sizeof(float);
  w.partV = o; o += (size_t)B * sl * NC * Cs * sizeof(float);
  w.cnt = o; o += up16((size_t)B * sl * NC * sizeof(int));
  w.N = o; o += up16((size_t)B * NC * sizeof(int));
  w.K = o; o += up16((size_t)B * sizeof(int));
  w.mhS = o; o += (size_t)B * NC * Cs * sizeof(float);
  w.mhT = o; o += (size_t)B * NC * Ct * sizeof(float);
  w.invn = o; o += up16((size_t)B * NC * sizeof(float));
  w.E = o; o += (size_t)B * NC * Cs * sizeof(float);
  w.L = o; o += up16((size_t)B * sizeof(double));
  w.total = o;
  return w;
}

__device__ __forceinline__ float dot4(float4 a, float4 b, float acc) { return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, fmaf(a.x, b.x, acc)))); }
// the class of a pixel, or -1 when it is not kept
__device__ __forceinline__ int kept_class(int64_t y, int ignore_index, int NC) {
  return (y != (int64_t)ignore_index && y >= 0 && y < (int64_t)NC) ? (int)y : -1;
}
// the sum of red[0 .. THREADS) in a fixed tree order; every thread returns it.  Ends with a barrier: red may be rewritten at once.
__device__ __forceinline__ double block_sum(double* red, double v) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int o = THREADS / 2; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  const double s = red[0];
  __syncthreads();
  return s;
}

struct SumArgs {
  const float* x[2]; float* part[2]; int C[2];
  const float4* pix;                  // non-NULL: row i enters with the weight pix[i].z * pix[i].x (w_i / r_i); NULL: 1
  const int64_t* y; int* cnt;         // cnt non-NULL: the per-slice class counts are written (by the workgroups of map 0)
  int ignore_index, NC, HW, slices, slice_rows;
};

// Launches 1 and 4.  grid = (B * slices, maps).  LDS: [NC][THREADS] float4, thread t owns column t of every class row.
__global__ __launch_bounds__(THREADS) void ifv_class_sum_kernel(SumArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ int cntl[MAX_NC];
  float4* acc = reinterpret_cast<float4*>(lds);
  const int t = threadIdx.x, map = blockIdx.y;
  const int b = blockIdx.x / a.slices, sl = blockIdx.x % a.slices;
  const int C = a.C[map], qn = C / 4, RL = THREADS / qn;
  const int q = t % qn, rl = t / qn;
  const bool active = rl < RL;
  for (int c = 0; c < a.NC; ++c) acc[c * THREADS + t] = kd_zero4();
  if (t < MAX_NC) cntl[t] = 0;
  __syncthreads();
  const int64_t row_lo = (int64_t)sl * a.slice_rows;
  const int64_t row_end = min((int64_t)a.HW, row_lo + a.slice_rows);
  const float* xb = a.x[map] + (int64_t)b * a.HW * C + 4 * q;
  const int64_t* yb = a.y + (int64_t)b * a.HW;
  const float4* pb = a.pix ? a.pix + (int64_t)b * a.HW : nullptr;
  const bool count = a.cnt != nullptr && map == 0 && q == 0;
  if (active) {
#pragma unroll 1
    for (int64_t r0 = row_lo + rl; r0 < row_end; r0 += 4 * RL) {
      float4 v[4];
      float wt[4];
      int cls[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {                             // four rows in flight per thread
        const int64_t r = r0 + (int64_t)u * RL;
        const bool ok = r < row_end;
        v[u] = ok ? kd_ld4(xb + r * C) : kd_zero4();
        cls[u] = ok ? kept_class(yb[r], a.ignore_index, a.NC) : -1;
        wt[u] = 1.f;
        if (pb && ok) { const float4 p = pb[r]; wt[u] = __fmul_rn(p.z, p.x); }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (cls[u] >= 0) {
          float4 s = acc[cls[u] * THREADS + t];
          s.x = fmaf(wt[u], v[u].x, s.x); s.y = fmaf(wt[u], v[u].y, s.y); s.z = fmaf(wt[u], v[u].z, s.z); s.w = fmaf(wt[u], v[u].w, s.w);
          acc[cls[u] * THREADS + t] = s;
          if (count) atomicAdd(&cntl[cls[u]], 1);               // an integer count: any order gives the same bits
        }
      }
    }
  }
  __syncthreads();
  float* out = a.part[map] + ((int64_t)b * a.slices + sl) * a.NC * C;
  for (int idx = t; idx < a.NC * qn; idx += THREADS) {          // the row lanes in lane order
    const int c = idx / qn, qq = idx % qn;
    float4 s = acc[c * THREADS + qq];
    for (int l = 1; l < RL; ++l) {
      const float4 o = acc[c * THREADS + l * qn + qq];
      s.x += o.x; s.y += o.y; s.z += o.z; s.w += o.w;
    }
    kd_st4(out + (int64_t)c * C + 4 * qq, s);
  }
  if (a.cnt != nullptr && map == 0 && t < a.NC) a.cnt[((int64_t)b * a.slices + sl) * a.NC + t] = cntl[t];
}

struct JoinArgs {
  const float* part[2]; float* mh[2]; int C[2];
  const int* cnt; int* N; int* K; float* invn;
  int NC, slices;
};

// Launch 2.  grid = (B, 2): image b, map blockIdx.y; thread k is channel k.  m = (slices in order, in double) / N_bc, |m| from a tree
// sum of m^2 in double, mh = m / |m|.
__global__ __launch_bounds__(THREADS) void ifv_proto_kernel(JoinArgs a) {
  __shared__ double red[THREADS];
  __shared__ int Nl[MAX_NC];
  const int t = threadIdx.x, b = blockIdx.x, map = blockIdx.y, C = a.C[map];
  if (t < a.NC) {
    int n = 0;
    for (int sl = 0; sl < a.slices; ++sl) n += a.cnt[((int64_t)b * a.slices + sl) * a.NC + t];
    Nl[t] = n;
    if (map == 0) a.N[b * a.NC + t] = n;
  }
  __syncthreads();
  if (map == 0 && t == 0) {
    int k = 0;
    for (int c = 0; c < a.NC; ++c) k += Nl[c];
    a.K[b] = k;
  }
  for (int c = 0; c < a.NC; ++c) {
    const int n = Nl[c];
    float m = 0.f;
    if (t < C && n > 0) {
      double s = 0.0;
      for (int sl = 0; sl < a.slices; ++sl) s += (double)a.part[map][(((int64_t)b * a.slices + sl) * a.NC + c) * C + t];
      m = (float)(s / (double)n);
    }
    const float nrm = (float)sqrt(block_sum(red, (double)m * (double)m));
    const bool live = nrm > 1e-12f;
    if (t < C) a.mh[map][((int64_t)b * a.NC + c) * C + t] = live ? __fdiv_rn(m, nrm) : 0.f;
    if (map == 0 && t == 0) a.invn[b * a.NC + c] = live ? __fdiv_rn(1.f, nrm) : 0.f;
  }
}

// one map's side of a row of the similarity pass: thread (row, sub) holds float4 columns sub, sub + 8, ...; -> (1 / r, xh . mh_c) with
// every lane of the row holding the same bits.  mhc: the class row of this map's prototypes in LDS, NULL for a pixel that is not kept.
template <int GQ>
__device__ __forceinline__ float2 row_sim(const float* xrow, int C, const float* mhc, int sub) {
  float4 p[GQ];
#pragma unroll
  for (int m = 0; m < GQ; ++m) {
    const int q = sub + 8 * m;
    p[m] = (xrow && 4 * q < C) ? kd_ld4(xrow + 4 * q) : kd_zero4();
  }
  float ss = 0.f;
#pragma unroll
  for (int m = 0; m < GQ; ++m) ss = sumsq4(p[m], ss);
  const float rinv = inv_norm(row8_sum(ss));
  float dot = 0.f;
#pragma unroll
  for (int m = 0; m < GQ; ++m) {
    const int q = sub + 8 * m;
    if (mhc && 4 * q < C) dot = dot4(scale4(p[m], rinv), kd_ld4(mhc + 4 * q), dot);
  }
  return make_float2(rinv, row8_sum(dot));
}

struct SimArgs {
  const float* s; const float* t; const int64_t* y; const float* mhS; const float* mhT; const int* K; float4* pix;
  int ignore_index, NC, HW, Cs, Ct, slices, slice_rows;
};

// Launch 3.  grid = B * slices.  LDS: mh of S [NC][Cs], then of T [NC][Ct].
template <int GQ>
__global__ __launch_bounds__(THREADS) void ifv_sim_kernel(SimArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int t = threadIdx.x, row = t >> 3, sub = t & 7;
  const int b = blockIdx.x / a.slices, sl = blockIdx.x % a.slices;
  float* mS = lds;
  float* mT = lds + a.NC * a.Cs;
  for (int i = 4 * t; i < a.NC * a.Cs; i += 4 * THREADS) kd_st4(mS + i, kd_ld4(a.mhS + (int64_t)b * a.NC * a.Cs + i));
  for (int i = 4 * t; i < a.NC * a.Ct; i += 4 * THREADS) kd_st4(mT + i, kd_ld4(a.mhT + (int64_t)b * a.NC * a.Ct + i));
  __syncthreads();
  const float Kf = (float)a.K[b];
  const int64_t row_lo = (int64_t)sl * a.slice_rows;
  const int64_t row_end = min((int64_t)a.HW, row_lo + a.slice_rows);
  const float* sb = a.s + (int64_t)b * a.HW * a.Cs;
  const float* tb = a.t + (int64_t)b * a.HW * a.Ct;
#pragma unroll 1
  for (int64_t r0 = row_lo; r0 < row_end; r0 += SR) {
    const int64_t r = r0 + row;
    const bool ok = r < row_end;
    const int c = ok ? kept_class(a.y[(int64_t)b * a.HW + r], a.ignore_index, a.NC) : -1;
    const float2 fs = row_sim<GQ>(ok ? sb + r * a.Cs : nullptr, a.Cs, c >= 0 ? mS + c * a.Cs : nullptr, sub);
    const float2 ft = row_sim<GQ>(ok ? tb + r * a.Ct : nullptr, a.Ct, c >= 0 ? mT + c * a.Ct : nullptr, sub);
    if (ok && sub == 0) {
      const float d = c >= 0 ? fs.y - ft.y : 0.f;
      const float w = c >= 0 ? __fdiv_rn(d, Kf) : 0.f;          // kept: K_b >= 1
      a.pix[(int64_t)b * a.HW + r] = make_float4(fs.x, c >= 0 ? fs.y : 0.f, w, d);
    }
  }
}

struct ImgArgs {
  const float4* pix; const int64_t* y; const float* partV; const float* mhS; const float* invn; const int* N; const int* K;
  float* E; double* L;
  int ignore_index, NC, HW, Cs, slices, grad;
};

// Launch 5.  grid = B.  L_b = (sum d^2 in double) / K_b; with grad, A_c = sum_{i in c} w_i s_i in double (a thread's pixels into its own
// column of [NC][THREADS], then a tree per class) and E_c = (V_c - A_c mh_c) / (|m_c| N_bc), V_c the slices of launch 4 in order.
__global__ __launch_bounds__(THREADS) void ifv_image_kernel(ImgArgs a) {
  __shared__ double red[THREADS];
  __shared__ double accA[MAX_NC * THREADS];
  __shared__ double A[MAX_NC];
  const int t = threadIdx.x, b = blockIdx.x;
  const float4* pb = a.pix + (int64_t)b * a.HW;
  const int64_t* yb = a.y + (int64_t)b * a.HW;
  if (a.grad)
    for (int c = 0; c < a.NC; ++c) accA[c * THREADS + t] = 0.0;
  double l = 0.0;
  for (int64_t i = t; i < a.HW; i += THREADS) {
    const float4 p = pb[i];
    l += (double)p.w * (double)p.w;
    if (a.grad) {
      const int c = kept_class(yb[i], a.ignore_index, a.NC);
      if (c >= 0) accA[c * THREADS + t] += (double)p.z * (double)p.y;
    }
  }
  const double tot = block_sum(red, l);
  const int K = a.K[b];
  if (t == 0) a.L[b] = K > 0 ? tot / (double)K : 0.0;
  if (!a.grad) return;
  for (int c = 0; c < a.NC; ++c) {
    const double s = block_sum(red, accA[c * THREADS + t]);
    if (t == 0) A[c] = s;
  }
  __syncthreads();
  if (t < a.Cs) {
    for (int c = 0; c < a.NC; ++c) {
      const int n = a.N[b * a.NC + c];
      const float inv = a.invn[b * a.NC + c];
      float e = 0.f;
      if (n > 0 && inv > 0.f) {
        double v = 0.0;
        for (int sl = 0; sl < a.slices; ++sl) v += (double)a.partV[(((int64_t)b * a.slices + sl) * a.NC + c) * a.Cs + t];
        e = (float)((v - A[c] * (double)a.mhS[((int64_t)b * a.NC + c) * a.Cs + t]) * (double)inv / (double)n);
      }
      a.E[((int64_t)b * a.NC + c) * a.Cs + t] = e;
    }
  }
}

// Launch 5b.  One block: the mean over images in a fixed order.
__global__ __launch_bounds__(THREADS) void ifv_final_kernel(const double* L, int B, float* img_out, float* val) {
  __shared__ double red[THREADS];
  double s = 0.0;
  for (int b = threadIdx.x; b < B; b += THREADS) {
    s += L[b];
    if (img_out) img_out[b] = (float)L[b];
  }
  const double tot = block_sum(red, s);
  if (threadIdx.x == 0) val[0] = (float)(tot / (double)B);
}

struct GradArgs {
  const float* s; const int64_t* y; const float4* pix; const float* mhS; const float* E; float* ds; const float* gdev; float gcoef;
  int ignore_index, NC, HW, Cs, slices, slice_rows;
};

// Launch 6.  grid = B * slices.  LDS: mh of S [NC][Cs], then E [NC][Cs].  The class-sum pass's thread layout: a column group and every
// RL-th row.
__global__ __launch_bounds__(THREADS) void ifv_grad_kernel(GradArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int t = threadIdx.x;
  const int b = blockIdx.x / a.slices, sl = blockIdx.x % a.slices;
  const int C = a.Cs, qn = C / 4, RL = THREADS / qn, q = t % qn, rl = t / qn;
  float* mS = lds;
  float* El = lds + a.NC * C;
  for (int i = 4 * t; i < a.NC * C; i += 4 * THREADS) {
    kd_st4(mS + i, kd_ld4(a.mhS + (int64_t)b * a.NC * C + i));
    kd_st4(El + i, kd_ld4(a.E + (int64_t)b * a.NC * C + i));
  }
  __syncthreads();
  if (rl >= RL) return;
  const float k = a.gdev ? __fmul_rn(a.gcoef, a.gdev[0]) : a.gcoef;
  const int64_t row_lo = (int64_t)sl * a.slice_rows;
  const int64_t row_end = min((int64_t)a.HW, row_lo + a.slice_rows);
  const float* xb = a.s + (int64_t)b * a.HW * C + 4 * q;
  float* db = a.ds + (int64_t)b * a.HW * C + 4 * q;
  const int64_t* yb = a.y + (int64_t)b * a.HW;
  const float4* pb = a.pix + (int64_t)b * a.HW;
#pragma unroll 2
  for (int64_t r = row_lo + rl; r < row_end; r += RL) {
    const int c = kept_class(yb[r], a.ignore_index, a.NC);
    float4 d = kd_zero4();
    if (c >= 0) {
      const float4 p = pb[r];                                   // {1 / r, sS, w, .}
      const float4 xh = scale4(kd_ld4(xb + r * C), p.x);
      const float4 mh = kd_ld4(mS + c * C + 4 * q), e = kd_ld4(El + c * C + 4 * q);
      const float wr = __fmul_rn(p.z, p.x);
      d.x = __fmul_rn(k, fmaf(wr, fmaf(-p.y, xh.x, mh.x), e.x));
      d.y = __fmul_rn(k, fmaf(wr, fmaf(-p.y, xh.y, mh.y), e.y));
      d.z = __fmul_rn(k, fmaf(wr, fmaf(-p.y, xh.z, mh.z), e.z));
      d.w = __fmul_rn(k, fmaf(wr, fmaf(-p.y, xh.w, mh.w), e.w));
    }
    kd_st4(db + r * C, d);
  }
}

}  // namespace

extern "C" {

size_t kd_feat_ifv_ws_bytes(int B, int HW, int Cs, int Ct, int NC) {
  if (!ifv_shape_ok(B, HW, Cs, Ct, NC)) return 0;
  return ifv_ws(B, HW, Cs, Ct, NC).total;
}

int kd_feat_ifv_slices(int B, int HW) { return (B < 1 || HW < 1 || HW > (1 << 30)) ? 0 : ifv_slices(B, HW); }

int kd_feat_ifv_fwd_bwd(const float* s, const float* t, const int64_t* target, int ignore_index, int B, int HW, int Cs, int Ct, int NC,
                        float gcoef, const float* gscale_dev, float* val, float* ds, float* img_vals_out, void* ws, size_t ws_bytes,
                        void* stream) {
  KD_REQUIRE(s && t && target && val, KD_ERR_ARG, "kd_feat_ifv_fwd_bwd: null s, t, target or val");
  KD_REQUIRE(std::isfinite(gcoef), KD_ERR_ARG, "kd_feat_ifv_fwd_bwd: gcoef must be finite (got %g)", (double)gcoef);
  KD_REQUIRE(ifv_shape_ok(B, HW, Cs, Ct, NC), KD_ERR_SHAPE,
             "kd_feat_ifv_fwd_bwd: B=%d, HW=%d, Cs=%d, Ct=%d, NC=%d unsupported (B >= 1, 1 <= HW <= 2^30; widths multiples of 4 from %d to %d; "
             "%d to %d classes)", B, HW, Cs, Ct, NC, MIN_C, MAX_C, MIN_NC, MAX_NC);
  const int slices = ifv_slices(B, HW), slice_rows = ifv_slice_rows(B, HW);
  KD_REQUIRE((int64_t)B * slices <= 0x7fffffff, KD_ERR_SHAPE, "kd_feat_ifv_fwd_bwd: B=%d x %d row slices exceeds the grid", B, slices);
  KD_REQUIRE(ws, KD_ERR_ARG, "kd_feat_ifv_fwd_bwd: null workspace");
  const IfvWs l = ifv_ws(B, HW, Cs, Ct, NC);
  KD_REQUIRE(ws_bytes >= l.total, KD_ERR_WORKSPACE, "kd_feat_ifv_fwd_bwd: workspace too small (%zu < %zu bytes)", ws_bytes, l.total);
  KD_REQUIRE(kd_aligned16(s) && kd_aligned16(t) && kd_aligned16(ws) && (!ds || kd_aligned16(ds)), KD_ERR_ALIGN,
             "kd_feat_ifv_fwd_bwd: s, t, ds and ws must be 16-byte aligned");
  KD_REQUIRE((reinterpret_cast<uintptr_t>(target) & 7u) == 0, KD_ERR_ALIGN, "kd_feat_ifv_fwd_bwd: target must be 8-byte aligned");
  char* base = (char*)ws;
  float4* pix = (float4*)(base + l.pix);
  float* partS = (float*)(base + l.partS);
  float* partT = (float*)(base + l.partT);
  float* partV = (float*)(base + l.partV);
  int* cnt = (int*)(base + l.cnt);
  int* N = (int*)(base + l.N);
  int* K = (int*)(base + l.K);
  float* mhS = (float*)(base + l.mhS);
  float* mhT = (float*)(base + l.mhT);
  float* invn = (float*)(base + l.invn);
  float* E = (float*)(base + l.E);
  double* L = (double*)(base + l.L);
  hipStream_t st = (hipStream_t)stream;
  const unsigned nwg = (unsigned)(B * slices);
  const size_t acc_lds = (size_t)NC * THREADS * sizeof(float4);   // 64 KiB at 16 classes, next to the static counters: above the default limit
  {                                                               // before any launch: a refused call writes nothing
    static std::atomic<uint64_t> raised;
    const hipError_t le = kd_raise_dynamic_lds((const void*)ifv_class_sum_kernel, (size_t)MAX_NC * THREADS * sizeof(float4), raised);
    KD_REQUIRE(le == hipSuccess, (int)le, "kd_feat_ifv_fwd_bwd: cannot raise the dynamic LDS limit: %s", hipGetErrorString(le));
  }

  SumArgs sa{{s, t}, {partS, partT}, {Cs, Ct}, nullptr, target, cnt, ignore_index, NC, HW, slices, slice_rows};
  hipLaunchKernelGGL(ifv_class_sum_kernel, dim3(nwg, 2), dim3(THREADS), acc_lds, st, sa);
  JoinArgs ja{{partS, partT}, {mhS, mhT}, {Cs, Ct}, cnt, N, K, invn, NC, slices};
  hipLaunchKernelGGL(ifv_proto_kernel, dim3((unsigned)B, 2), dim3(THREADS), 0, st, ja);
  SimArgs ma{s, t, target, mhS, mhT, K, pix, ignore_index, NC, HW, Cs, Ct, slices, slice_rows};
  const size_t sim_lds = (size_t)NC * (Cs + Ct) * sizeof(float);
  if (Cs <= 128 && Ct <= 128) hipLaunchKernelGGL(ifv_sim_kernel<4>, dim3(nwg), dim3(THREADS), sim_lds, st, ma);
  else hipLaunchKernelGGL(ifv_sim_kernel<8>, dim3(nwg), dim3(THREADS), sim_lds, st, ma);
  if (ds) {
    SumArgs va{{s, nullptr}, {partV, nullptr}, {Cs, 0}, pix, target, nullptr, ignore_index, NC, HW, slices, slice_rows};
    hipLaunchKernelGGL(ifv_class_sum_kernel, dim3(nwg, 1), dim3(THREADS), acc_lds, st, va);
  }
  ImgArgs ia{pix, target, partV, mhS, invn, N, K, E, L, ignore_index, NC, HW, Cs, slices, ds ? 1 : 0};
  hipLaunchKernelGGL(ifv_image_kernel, dim3((unsigned)B), dim3(THREADS), 0, st, ia);
  hipLaunchKernelGGL(ifv_final_kernel, dim3(1), dim3(THREADS), 0, st, (const double*)L, B, img_vals_out, val);
  if (ds) {
    GradArgs ga{s, target, pix, mhS, E, ds, gscale_dev, gcoef, ignore_index, NC, HW, Cs, slices, slice_rows};
    hipLaunchKernelGGL(ifv_grad_kernel, dim3(nwg), dim3(THREADS), (size_t)2 * NC * Cs * sizeof(float), st, ga);
  }
  return kd_check_launch("kd_feat_ifv_fwd_bwd");
}

}  // extern "C"
