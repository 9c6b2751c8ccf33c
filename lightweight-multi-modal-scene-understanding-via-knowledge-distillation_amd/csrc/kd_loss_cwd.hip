// kd_loss_cwd.hip -- the opt-in channel-wise distillation feature term of the KD step (Shu et al., ICCV 2021):
//   phi(X)[b,c,i] = softmax over the HW positions i of X[b,c,:] / tau
//   CWD(S, T)     = tau^2 / (B*C) * sum_{b,c} sum_i phi(T) (log phi(T) - log phi(S)),   dCWD/dS = tau / (B*C) * (phi(S) - phi(T))
// on the NHWC matrices [B*HW, C]: a COLUMN-wise log-sum-exp over the HW rows of each image, then a point-wise pass.
// Three launches.  (1) statistics: a workgroup per (image, chunk of rows); a thread owns 4 consecutive channels (one float4 of
// a row, so a wave reads whole rows: 1 KiB contiguous) and walks every `slots`-th row of its chunk in register batches of 8
// rows with an online (max, sum); the slots of a channel are joined through LDS in slot order and the chunk's (max, sum) of
// s / tau and of t / tau go to the workspace.  (2) point-wise: the same grid; the prologue re-reduces the image's chunk partials
// in chunk order to (max, log-sum-exp, 1 / sum) per channel, then one sweep forms both log-probabilities and probabilities,
// sums phi(t) (log phi(t) - log phi(s)) and stores ds.  (3) one block sums the per-workgroup values in double.
// 5 sweeps of a map per call with the gradient (s and t twice, ds once), 4 forward only.
// No atomics, a fixed order everywhere, and s and t go through the same device functions operation for operation (every product
// that could contract with a neighbouring sum is an explicit __fmul_rn / fmaf): identical bits in s and t give val == 0 and
// ds == +-0, and an image's statistics and gradient depend on that image's rows alone.
#include "kd_loss_common.h"

#include <cmath>

namespace {

constexpr int THREADS = 256;
constexpr int BATCH = 8;                  // rows a thread holds in registers per online-softmax step
constexpr int NBATCH = 8;                 // steps per chunk: a thread walks BATCH * NBATCH rows of its chunk
constexpr int ROWS_PER_THREAD = BATCH * NBATCH;
constexpr int MAX_C = 512;

struct CwdLayout {
  int groups;        // C / 4: float4 columns
  int slots;         // row slots of a workgroup = 256 / groups
  int chunk_rows;    // slots * ROWS_PER_THREAD
  int nchunk;        // chunks per image
};

inline CwdLayout cwd_layout(int HW, int C) {
  CwdLayout l;
  l.groups = C / 4;
  l.slots = THREADS / l.groups;
  l.chunk_rows = l.slots * ROWS_PER_THREAD;
  l.nchunk = (int)(((int64_t)HW + l.chunk_rows - 1) / l.chunk_rows);
  return l;
}

inline size_t cwd_ws(int64_t B, int64_t HW, int64_t C) {
  if (B < 1 || HW < 1 || C < 4 || C % 4 != 0 || C > MAX_C) return 0;
  const CwdLayout l = cwd_layout((int)HW, (int)C);
  return (size_t)(B * l.nchunk * (4 * C + 1)) * sizeof(float);      // (max, sum) of s and of t per channel, one value partial
}

struct CwdArgs {
  const float* s; const float* t;
  float* part;       // [B][nchunk][4][C]: max s, sum s, max t, sum t
  float* vpart;      // [B][nchunk]
  float* ds; float* stats_out;
  const float* gdev;
  float invtau, gcoef;
  int HW, C, groups, slots, chunk_rows, nchunk;
};

struct MS4 { float4 m, s; };

__device__ __forceinline__ float4 max4(float4 a, float4 b) {
  return make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w));
}
// sum * exp(m_old - m_new): the running sum moved to a new maximum (m_old = -inf: the sum is 0 and stays 0)
__device__ __forceinline__ float rescale(float sum, float m_old, float m_new) { return __fmul_rn(sum, expf(m_old - m_new)); }

// one thread's (max, sum exp(x - max)) over the rows row0, row0 + slots, ... < row_end of one map, x = v * invtau
__device__ __forceinline__ MS4 column_stats(const float* base, int64_t row0, int64_t row_end, int slots, int C, float invtau) {
  MS4 a;
  a.m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
  a.s = kd_zero4();
#pragma unroll 1
  for (int nb = 0; nb < NBATCH; ++nb) {
    const int64_t r0 = row0 + (int64_t)nb * BATCH * slots;
    if (r0 >= row_end) break;              // the first row of a step is the thread's lowest: a step is never empty
    float4 x[BATCH];
    float4 bm = a.m;
#pragma unroll
    for (int k = 0; k < BATCH; ++k) {
      const int64_t r = r0 + (int64_t)k * slots;
      if (r < row_end) {
        x[k] = scale4(kd_ld4(base + r * C), invtau);
        bm = max4(bm, x[k]);
      } else {
        x[k] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);      // expf(-inf) = 0: adds nothing
      }
    }
    a.s.x = rescale(a.s.x, a.m.x, bm.x); a.s.y = rescale(a.s.y, a.m.y, bm.y);
    a.s.z = rescale(a.s.z, a.m.z, bm.z); a.s.w = rescale(a.s.w, a.m.w, bm.w);
    a.m = bm;
#pragma unroll
    for (int k = 0; k < BATCH; ++k) {
      a.s.x += expf(x[k].x - bm.x); a.s.y += expf(x[k].y - bm.y);
      a.s.z += expf(x[k].z - bm.z); a.s.w += expf(x[k].w - bm.w);
    }
  }
  return a;
}

// (M, S) += a partial (m, s) whose maximum is already in M: S = s * exp(m - M) + S
__device__ __forceinline__ float join(float S, float s, float m, float M) { return fmaf(s, expf(m - M), S); }

// Launch 1.  grid = B * nchunk workgroups.
__global__ __launch_bounds__(THREADS) void cwd_stats_kernel(CwdArgs a) {
  __shared__ float4 sh[4][THREADS];        // [max s, sum s, max t, sum t][thread]
  const int b = blockIdx.x / a.nchunk, ch = blockIdx.x % a.nchunk;
  const int t = threadIdx.x, g = t % a.groups, slot = t / a.groups;
  const bool live = slot < a.slots;
  const int64_t row_lo = (int64_t)ch * a.chunk_rows;
  const int64_t row_end = min((int64_t)a.HW, row_lo + a.chunk_rows);
  const int64_t off = (int64_t)b * a.HW * a.C + 4 * g;
  if (live) {
    const MS4 ss = column_stats(a.s + off, row_lo + slot, row_end, a.slots, a.C, a.invtau);
    const MS4 tt = column_stats(a.t + off, row_lo + slot, row_end, a.slots, a.C, a.invtau);
    sh[0][t] = ss.m; sh[1][t] = ss.s; sh[2][t] = tt.m; sh[3][t] = tt.s;
  }
  __syncthreads();
  if (t < a.groups) {                      // slot 0 of each float4 column joins the slots in order
    float* out = a.part + ((int64_t)b * a.nchunk + ch) * 4 * a.C + 4 * t;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      float4 M = sh[2 * q][t];
      for (int j = 1; j < a.slots; ++j) M = max4(M, sh[2 * q][j * a.groups + t]);
      float4 S = kd_zero4();
      for (int j = 0; j < a.slots; ++j) {
        const float4 m = sh[2 * q][j * a.groups + t], s = sh[2 * q + 1][j * a.groups + t];
        S.x = join(S.x, s.x, m.x, M.x); S.y = join(S.y, s.y, m.y, M.y);
        S.z = join(S.z, s.z, m.z, M.z); S.w = join(S.w, s.w, m.w, M.w);
      }
      kd_st4(out + (2 * q) * a.C, M);
      kd_st4(out + (2 * q + 1) * a.C, S);
    }
  }
}

struct LP { float lp, p; };
// log phi = (x - M) - L with L = log S, and phi = exp(x - M) * (1 / S): the probability is never exponentiated from the rounded log
__device__ __forceinline__ LP logprob(float v, float invtau, float M, float L, float R) {
  const float d = __fmul_rn(v, invtau) - M;
  LP r;
  r.lp = d - L;
  r.p = __fmul_rn(expf(d), R);
  return r;
}
__device__ __forceinline__ float point(float vs, float vt, float invtau, float Ms, float Ls, float Rs, float Mt, float Lt, float Rt, float k,
                                       float& acc) {
  const LP s = logprob(vs, invtau, Ms, Ls, Rs);
  const LP t = logprob(vt, invtau, Mt, Lt, Rt);
  const float d = t.lp - s.lp;
  acc = fmaf(t.p, d, acc);                 // phi(t) = 0 (underflow): 0 * finite = 0
  return __fmul_rn(k, s.p - t.p);
}

// Launch 2.  The same grid and the same thread-to-row map as launch 1.
__global__ __launch_bounds__(THREADS) void cwd_point_kernel(CwdArgs a) {
  __shared__ __attribute__((aligned(16))) float st[6 * MAX_C];          // [M_s, L_s, 1/S_s, M_t, L_t, 1/S_t][C]
  __shared__ float wsum[THREADS / 64];
  const int b = blockIdx.x / a.nchunk, ch = blockIdx.x % a.nchunk;
  const int t = threadIdx.x;
  const float* part = a.part + (int64_t)b * a.nchunk * 4 * a.C;
  for (int c = t; c < a.C; c += THREADS) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      float M = part[(2 * q) * a.C + c];
      for (int k = 1; k < a.nchunk; ++k) M = fmaxf(M, part[((int64_t)k * 4 + 2 * q) * a.C + c]);
      float S = 0.f;
      for (int k = 0; k < a.nchunk; ++k) S = join(S, part[((int64_t)k * 4 + 2 * q + 1) * a.C + c], part[((int64_t)k * 4 + 2 * q) * a.C + c], M);
      const float L = logf(S);
      st[(3 * q) * a.C + c] = M;
      st[(3 * q + 1) * a.C + c] = L;
      st[(3 * q + 2) * a.C + c] = 1.f / S;
      if (a.stats_out && ch == 0) {
        float* o = a.stats_out + ((int64_t)b * a.C + c) * 4 + 2 * q;
        o[0] = M;
        o[1] = L;
      }
    }
  }
  __syncthreads();
  const int g = t % a.groups, slot = t / a.groups;
  const float k = a.gdev ? __fmul_rn(a.gcoef, a.gdev[0]) : a.gcoef;
  float acc = 0.f;
  if (slot < a.slots) {
    const int64_t row_lo = (int64_t)ch * a.chunk_rows;
    const int64_t row_end = min((int64_t)a.HW, row_lo + a.chunk_rows);
    const int64_t off = (int64_t)b * a.HW * a.C + 4 * g;
    const float4 Ms = kd_ld4(st + 4 * g), Ls = kd_ld4(st + a.C + 4 * g), Rs = kd_ld4(st + 2 * a.C + 4 * g);
    const float4 Mt = kd_ld4(st + 3 * a.C + 4 * g), Lt = kd_ld4(st + 4 * a.C + 4 * g), Rt = kd_ld4(st + 5 * a.C + 4 * g);
#pragma unroll 4
    for (int64_t r = row_lo + slot; r < row_end; r += a.slots) {
      const int64_t o = off + r * a.C;
      const float4 vs = kd_ld4(a.s + o), vt = kd_ld4(a.t + o);
      float4 d;
      d.x = point(vs.x, vt.x, a.invtau, Ms.x, Ls.x, Rs.x, Mt.x, Lt.x, Rt.x, k, acc);
      d.y = point(vs.y, vt.y, a.invtau, Ms.y, Ls.y, Rs.y, Mt.y, Lt.y, Rt.y, k, acc);
      d.z = point(vs.z, vt.z, a.invtau, Ms.z, Ls.z, Rs.z, Mt.z, Lt.z, Rt.z, k, acc);
      d.w = point(vs.w, vt.w, a.invtau, Ms.w, Ls.w, Rs.w, Mt.w, Lt.w, Rt.w, k, acc);
      if (a.ds) kd_st4(a.ds + o, d);
    }
  }
  const float w = kd_wave_sum(acc);
  if ((t & 63) == 0) wsum[t >> 6] = w;
  __syncthreads();
  if (t == 0) a.vpart[(int64_t)b * a.nchunk + ch] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// Launch 3.  One block: val = coef * sum of the workgroup values, summed in double in a fixed order.
__global__ __launch_bounds__(THREADS) void cwd_final_kernel(const float* vpart, int64_t n, double coef, float* val) {
  __shared__ double red[THREADS];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += THREADS) s += (double)vpart[i];
  red[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < THREADS; ++i) t += red[i];
    val[0] = (float)(t * coef);
  }
}

}  // namespace

extern "C" {

size_t kd_feat_cwd_ws_bytes(int B, int HW, int C) { return cwd_ws(B, HW, C); }

// ws: [B][nchunk][4][C] chunk partials, then [B][nchunk] value partials
int kd_feat_cwd_fwd_bwd(const float* s, const float* t, int B, int HW, int C, float tau, float gcoef, const float* gscale_dev, float* val,
                        float* ds, float* stats_out, void* ws, size_t ws_bytes, void* stream) {
  KD_REQUIRE(s && t && val, KD_ERR_ARG, "kd_feat_cwd_fwd_bwd: null s, t or val");
  KD_REQUIRE(std::isfinite(tau) && tau > 0.f, KD_ERR_ARG, "kd_feat_cwd_fwd_bwd: tau must be finite and > 0 (got %g)", (double)tau);
  KD_REQUIRE(C >= 4 && C % 4 == 0 && C <= MAX_C, KD_ERR_SHAPE, "kd_feat_cwd_fwd_bwd: C=%d unsupported (a multiple of 4 up to %d)", C, MAX_C);
  KD_REQUIRE(B >= 1 && HW >= 1, KD_ERR_SHAPE, "kd_feat_cwd_fwd_bwd: B=%d, HW=%d unsupported", B, HW);
  const CwdLayout l = cwd_layout(HW, C);
  const int64_t nblk = (int64_t)B * l.nchunk;
  KD_REQUIRE(nblk <= 0x7fffffff, KD_ERR_SHAPE, "kd_feat_cwd_fwd_bwd: B=%d x %d row chunks exceeds the grid", B, l.nchunk);
  KD_REQUIRE(ws, KD_ERR_ARG, "kd_feat_cwd_fwd_bwd: null workspace");
  KD_REQUIRE(ws_bytes >= cwd_ws(B, HW, C), KD_ERR_WORKSPACE, "kd_feat_cwd_fwd_bwd: workspace too small (%zu < %zu bytes)", ws_bytes,
             cwd_ws(B, HW, C));
  KD_REQUIRE(kd_aligned16(s) && kd_aligned16(t) && kd_aligned16(ws) && (!ds || kd_aligned16(ds)), KD_ERR_ALIGN,
             "kd_feat_cwd_fwd_bwd: s, t, ds and ws must be 16-byte aligned");
  float* part = (float*)ws;
  float* vpart = part + nblk * 4 * C;
  hipStream_t st = (hipStream_t)stream;
  // one launch pair over the whole batch: splitting it into groups of images whose second read would come from the Infinity
  // Cache was measured and lost (profiles/cwd_feature_ab.txt): a group small enough to stay resident does not fill the CUs
  CwdArgs a{s, t, part, vpart, ds, stats_out, gscale_dev, 1.f / tau, gcoef, HW, C, l.groups, l.slots, l.chunk_rows, l.nchunk};
  hipLaunchKernelGGL(cwd_stats_kernel, dim3((unsigned)nblk), dim3(THREADS), 0, st, a);
  hipLaunchKernelGGL(cwd_point_kernel, dim3((unsigned)nblk), dim3(THREADS), 0, st, a);
  const double coef = (double)tau * (double)tau / ((double)B * (double)C);
  hipLaunchKernelGGL(cwd_final_kernel, dim3(1), dim3(THREADS), 0, st, (const float*)vpart, nblk, coef, val);
  return kd_check_launch("kd_feat_cwd_fwd_bwd");
}

}  // extern "C"
