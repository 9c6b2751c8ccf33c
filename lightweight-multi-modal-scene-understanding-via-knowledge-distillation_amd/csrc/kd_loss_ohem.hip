// kd_loss_ohem.hip -- the opt-in online-hard-example-mining (OHEM) cross-entropy of the KD step, 2 to 16 classes:
//   l_i = -log p_{y_i} over the pixels K the weighted CE keeps (n of them),   m = min(n, max(min_kept, ceil(n / min_divisor))),
//   theta = min(m-th largest l, lambda),   S = { i in K : l_i >= theta },   L = sum_S w[y] l / sum_S w[y],
//   dL/dz_ij = w[y_i] (p_ij - [j == y_i]) / sum_S w on S and 0 off it; the temperature KL rides along over all pixels, value and
//   gradient as in kd_seg_loss_fwd_bwd (kd_loss.hip), bit for bit.
// l >= 0, so its fp32 bits order as unsigned integers: the m-th largest is an exact radix select over the 31 value bits in three
// digits of 11 + 10 + 10 bits.  Seven launches with a gradient, six without:
//   1 fill     zeroes the three digit histograms and the selection state
//   2 score    key_i = bits(l_i) (SENT off K) into the workspace, the KL partial sums, the histogram of the top digit
//   3 digit 2  every block finds the top digit's bucket from histogram 1 (block 0 records n, m and the rank left inside the bucket),
//              then counts the middle digit of the keys in that bucket
//   4 digit 3  the same one digit down
//   5 sum      every block finds the last digit -> theta; masked partial sums of w l and w over S and over K, |S|, keep_out
//   6 final    one block: the slab in double -> vals, counts_out
//   7 grad     dzs; a pixel is in S when its stored key is >= the bits of theta
// The bucket choice is folded into the pass that needs it (a block scans at most 2048 counters), which saves three one-block
// launches.  Histograms are privatised in LDS and flushed with integer atomics; there is no floating-point atomic and no host read:
// the same input gives the same bytes on every call and every graph replay, and S is a function of the values alone.
#include "kd_loss_common.h"

#include <cmath>
#include <cstring>

namespace {

constexpr int SEG_MAXC = 16;                      // class buckets 4, 8, 16 as in kd_seg_loss_fwd_bwd
constexpr unsigned SENT = 0xFFFFFFFFu;            // a pixel outside K: the sign bit no kept key carries
constexpr int D1_BITS = 11, D2_BITS = 10, D3_BITS = 10;
constexpr int D1_BINS = 1 << D1_BITS, D2_BINS = 1 << D2_BITS, D3_BINS = 1 << D3_BITS;
constexpr int HIST_WORDS = D1_BINS + D2_BINS + D3_BINS;
constexpr int SLAB_COLS = 8;                      // doubles per block: swn_S, sw_S, swn_K, sw_K, |S|, skl, 2 spare
// selection state, 32-bit words behind the histograms
enum { ST_N = 0, ST_M, ST_D1, ST_R1, ST_D2, ST_R2, ST_THETA, ST_WORDS = 16 };

struct OhemArgs {
  const float* zs; const float* zt; const int64_t* target; const float* cw;
  int ignore_index; float T; float alpha; float gscale; const float* gdev;
  unsigned lambda_bits; int64_t min_kept; int64_t min_divisor;
  double* slab; unsigned* hist; unsigned* state; unsigned* keys;
  float* vals; int64_t* counts; float* dzs; float* nll_out; unsigned char* keep_out;
  int64_t npix; int HW; int NC;
};

__device__ __forceinline__ int kd_wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The bucket of the rank-th largest key among the `nbins` counters of one digit (rank counts from 1 at the largest), by all 256
// threads of the block: thread t owns nbins / 256 consecutive counters, walked from the top digit down.  -> digit, the rank left
// inside its bucket, and the sum of all counters.  rank == 0 or rank > total: digit = rest = 0 (the caller never uses them then).
// `rank_from_total`: the rank is m(total) of the first digit, formed here once the total is known.
__device__ __forceinline__ void find_bucket(const unsigned* hist, int nbins, unsigned rank, bool rank_from_total, int64_t min_kept,
                                            int64_t min_divisor, unsigned* digit, unsigned* rest, unsigned* total, unsigned* m_out) {
  __shared__ unsigned s_wave[4];
  __shared__ unsigned s_res[2];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int E = nbins >> 8;                        // 8 or 4 counters per thread
  unsigned c[D1_BINS / 256];
  unsigned mine = 0;
#pragma unroll
  for (int u = 0; u < D1_BINS / 256; ++u) {
    c[u] = 0;
    if (u < E) { c[u] = hist[nbins - 1 - (t * E + u)]; mine += c[u]; }
  }
  unsigned incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  if (t < 2) s_res[t] = 0;
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  unsigned above = incl - mine, tot = 0;
  for (int w = 0; w < 4; ++w) {
    if (w < wave) above += s_wave[w];
    tot += s_wave[w];
  }
  if (rank_from_total) {
    const int64_t n = (int64_t)tot;
    int64_t m = (n + min_divisor - 1) / min_divisor;             // n < 2^31 and min_divisor >= 1: no overflow
    if (m < min_kept) m = min_kept;
    if (m > n) m = n;
    rank = (unsigned)m;
  }
#pragma unroll
  for (int u = 0; u < D1_BINS / 256; ++u) {
    if (u < E) {
      if (above < rank && rank <= above + c[u]) {  // exactly one counter of one thread when 1 <= rank <= total
        s_res[0] = (unsigned)(nbins - 1 - (t * E + u));
        s_res[1] = rank - above;
      }
      above += c[u];
    }
  }
  __syncthreads();
  *digit = s_res[0];
  *rest = s_res[1];
  *total = tot;
  *m_out = rank;
  __syncthreads();                                  // s_wave / s_res may be reused by the next call in the same kernel
}

__device__ __forceinline__ void hist_clear(unsigned* loc, int nbins) {
  for (int i = threadIdx.x; i < nbins; i += 256) loc[i] = 0;
  __syncthreads();
}
__device__ __forceinline__ void hist_flush(const unsigned* loc, unsigned* glob, int nbins) {
  __syncthreads();
  for (int i = threadIdx.x; i < nbins; i += 256) {
    const unsigned v = loc[i];
    if (v) atomicAdd(&glob[i], v);
  }
}

// Launch 2.  The KL partial sum is seg_loss_partial_kernel's, expression for expression and in its order (thread, wave, the four
// waves in fp32), so the KL value keeps the bits of kd_seg_loss_fwd_bwd.
template <int K>
__global__ __launch_bounds__(256) void ohem_score_kernel(OhemArgs a) {
  __shared__ unsigned loc[D1_BINS];
  __shared__ float red[4];
  hist_clear(loc, D1_BINS);
  float skl = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.npix; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / a.HW, hw = i % a.HW;
    float z[K], p[K], lp[K];
#pragma unroll
    for (int j = 0; j < K; ++j) if (j < a.NC) z[j] = a.zs[(b * a.NC + j) * a.HW + hw];
    const int64_t y = a.target[i];
    unsigned key = SENT;
    if (KD_KEPT_LABEL(y, a.ignore_index, a.NC)) {
      softmax_c<K>(z, a.NC, 1.f, p, lp);
      float nll = 0.f;
#pragma unroll
      for (int j = 0; j < K; ++j) if (j == (int)y) nll = -lp[j];
      key = __float_as_uint(nll) & 0x7FFFFFFFu;    // l >= 0; -0 and a NaN's sign are cleared, a NaN sorts above every number
      atomicAdd(&loc[key >> (D2_BITS + D3_BITS)], 1u);
    }
    a.keys[i] = key;
    if (a.nll_out) a.nll_out[i] = key == SENT ? -1.f : __uint_as_float(key);
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
  hist_flush(loc, a.hist, D1_BINS);
  skl = kd_wave_sum(skl);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = skl;
  __syncthreads();
  if (threadIdx.x == 0) a.slab[(int64_t)blockIdx.x * SLAB_COLS + 5] = (double)(red[0] + red[1] + red[2] + red[3]);
}

// Launches 3 and 4.  PASS 2: the bucket of digit 1 from histogram 1, then the histogram of digit 2 inside it; PASS 3: one digit down.
template <int PASS>
__global__ __launch_bounds__(256) void ohem_digit_kernel(OhemArgs a) {
  __shared__ unsigned loc[D2_BINS];
  unsigned digit, rest, total, m;
  unsigned prefix;                                  // the key's bits above the digit this pass counts
  int shift;
  unsigned* out;
  if (PASS == 2) {
    find_bucket(a.hist, D1_BINS, 0, true, a.min_kept, a.min_divisor, &digit, &rest, &total, &m);
    if (blockIdx.x == 0 && threadIdx.x == 0) { a.state[ST_N] = total; a.state[ST_M] = m; a.state[ST_D1] = digit; a.state[ST_R1] = rest; }
    if (total == 0) return;                         // no kept pixel (every block agrees): nothing to select
    prefix = digit; shift = D3_BITS; out = a.hist + D1_BINS;
  } else {
    if (a.state[ST_N] == 0) return;
    find_bucket(a.hist + D1_BINS, D2_BINS, a.state[ST_R1], false, 0, 1, &digit, &rest, &total, &m);
    if (blockIdx.x == 0 && threadIdx.x == 0) { a.state[ST_D2] = digit; a.state[ST_R2] = rest; }
    prefix = (a.state[ST_D1] << D2_BITS) | digit; shift = 0; out = a.hist + D1_BINS + D2_BINS;
  }
  hist_clear(loc, D2_BINS);
  const int pshift = PASS == 2 ? D2_BITS + D3_BITS : D3_BITS;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.npix; i += (int64_t)gridDim.x * 256) {
    const unsigned key = a.keys[i];
    if (key != SENT && (key >> pshift) == prefix) atomicAdd(&loc[(key >> shift) & (D2_BINS - 1)], 1u);
  }
  hist_flush(loc, out, D2_BINS);
}

// Launch 5.  theta, then the masked sums in seg_loss_partial_kernel's order per thread and wave; the four waves and the slab in double.
__global__ __launch_bounds__(256) void ohem_sum_kernel(OhemArgs a) {
  __shared__ double red[5][4];
  const unsigned n = a.state[ST_N];
  unsigned theta = a.lambda_bits;                   // no kept pixel: nothing is compared against it
  if (n) {
    unsigned digit, rest, total, m;
    find_bucket(a.hist + D1_BINS + D2_BINS, D3_BINS, a.state[ST_R2], false, 0, 1, &digit, &rest, &total, &m);
    const unsigned tau = (a.state[ST_D1] << (D2_BITS + D3_BITS)) | (a.state[ST_D2] << D3_BITS) | digit;
    theta = tau < a.lambda_bits ? tau : a.lambda_bits;           // both >= 0: the order of the bits is the order of the values
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) a.state[ST_THETA] = theta;
  float swn = 0.f, sw = 0.f, awn = 0.f, aw = 0.f;
  int cnt = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.npix; i += (int64_t)gridDim.x * 256) {
    const unsigned key = a.keys[i];
    const bool kept = key != SENT && key >= theta;
    if (key != SENT) {
      const float nll = __uint_as_float(key);
      const float w = a.cw ? a.cw[a.target[i]] : 1.f;
      awn = fmaf(w, nll, awn);
      aw += w;
      if (kept) {
        swn = fmaf(w, nll, swn);
        sw += w;
        ++cnt;
      }
    }
    if (a.keep_out) a.keep_out[i] = kept ? 1 : 0;
  }
  swn = kd_wave_sum(swn); sw = kd_wave_sum(sw); awn = kd_wave_sum(awn); aw = kd_wave_sum(aw);
  cnt = kd_wave_sum_int(cnt);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { red[0][wave] = swn; red[1][wave] = sw; red[2][wave] = awn; red[3][wave] = aw; red[4][wave] = (double)cnt; }
  __syncthreads();
  if (threadIdx.x < 5)
    a.slab[(int64_t)blockIdx.x * SLAB_COLS + threadIdx.x] = ((red[threadIdx.x][0] + red[threadIdx.x][1]) + red[threadIdx.x][2]) + red[threadIdx.x][3];
}

// Launch 6.  One block; the reduction order of seg_loss_final_kernel.
__global__ __launch_bounds__(256) void ohem_final_kernel(const double* slab, int nblk, double npix, const unsigned* state, float* vals,
                                                         int64_t* counts) {
  constexpr int NR = 6;
  __shared__ double red[NR][256];
  double s[NR];
#pragma unroll
  for (int k = 0; k < NR; ++k) s[k] = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 256) {
#pragma unroll
    for (int k = 0; k < NR; ++k) s[k] += slab[(int64_t)i * SLAB_COLS + k];
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
    const double n = (double)state[ST_N];
    vals[0] = (float)(t[0] / t[1]);
    vals[1] = (float)(t[5] / npix);
    vals[2] = (float)t[1];
    vals[3] = (float)(t[2] / t[3]);
    vals[4] = __uint_as_float(state[ST_THETA]);
    vals[5] = (float)(t[4] / n);
    vals[6] = 0.f;
    vals[7] = 0.f;
    if (counts) { counts[0] = (int64_t)state[ST_N]; counts[1] = (int64_t)state[ST_M]; counts[2] = (int64_t)t[4]; }
  }
}

// Launch 7.  seg_loss_grad_kernel with the hard-label part restricted to S, decided from the stored key.
template <int K>
__global__ __launch_bounds__(256) void ohem_grad_kernel(OhemArgs a) {
  const float sumw = a.vals[2];
  const unsigned theta = a.state[ST_THETA];
  const float gs = a.gscale * (a.gdev ? a.gdev[0] : 1.f);      // upstream gradient as a device scalar
  const float klc = a.zt ? gs * a.alpha * a.T / (float)a.npix : 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.npix; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / a.HW, hw = i % a.HW;
    float z[K], p[K], lp[K], g[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { g[j] = 0.f; if (j < a.NC) z[j] = a.zs[(b * a.NC + j) * a.HW + hw]; }
    const unsigned key = a.keys[i];
    if (key != SENT && key >= theta) {
      const int64_t y = a.target[i];
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

inline int64_t ohem_grid(int64_t npix) {
  int64_t g = (npix + 255) / 256;
  return g > 1024 ? 1024 : (g < 1 ? 1 : g);
}
// ws: [grid * 8] doubles (the slab), [HIST_WORDS] histograms, [ST_WORDS] state, [npix] keys
inline size_t ohem_ws(int64_t npix) {
  if (npix < 1) return 0;
  return (size_t)ohem_grid(npix) * SLAB_COLS * sizeof(double) + (size_t)(HIST_WORDS + ST_WORDS) * sizeof(unsigned) + (size_t)npix * sizeof(unsigned);
}

}  // namespace

extern "C" {

size_t kd_seg_ohem_ws_bytes(int64_t npix) { return ohem_ws(npix); }

int kd_seg_ohem_fwd_bwd(const float* zs, const float* zt, const int64_t* target, const float* class_w, int ignore_index, float T,
                        float alpha, float gscale, const float* gscale_dev, float lambda, int64_t min_kept, int64_t min_divisor,
                        float* vals, int64_t* counts_out, float* dzs, float* nll_out, uint8_t* keep_out, int B, int NC, int HW,
                        void* ws, size_t ws_bytes, void* stream) {
  KD_REQUIRE(zs && target && vals, KD_ERR_ARG, "kd_seg_ohem_fwd_bwd: null zs, target or vals");
  KD_REQUIRE(std::isfinite(lambda) && lambda >= 0.f, KD_ERR_ARG, "kd_seg_ohem_fwd_bwd: lambda = -log(thresh) must be finite and >= 0 (got %g)",
             (double)lambda);
  KD_REQUIRE(min_kept >= 1 && min_divisor >= 1, KD_ERR_ARG, "kd_seg_ohem_fwd_bwd: min_kept and min_divisor must be >= 1 (got %lld, %lld)",
             (long long)min_kept, (long long)min_divisor);
  KD_REQUIRE(NC >= 2 && NC <= SEG_MAXC, KD_ERR_SHAPE, "kd_seg_ohem_fwd_bwd: num_classes=%d unsupported (2..16)", NC);
  KD_REQUIRE(B >= 1 && HW >= 1 && (int64_t)B * HW <= (int64_t)INT32_MAX, KD_ERR_SHAPE,
             "kd_seg_ohem_fwd_bwd: B=%d, HW=%d unsupported (1 <= B * HW < 2^31: the counters are 32 bits wide)", B, HW);
  const int64_t npix = (int64_t)B * HW;
  KD_REQUIRE(ws && ws_bytes >= ohem_ws(npix), KD_ERR_WORKSPACE, "kd_seg_ohem_fwd_bwd: workspace too small");
  KD_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7u) == 0, KD_ERR_ALIGN, "kd_seg_ohem_fwd_bwd: ws must be 8-byte aligned");
  const int64_t grid = ohem_grid(npix);
  double* slab = (double*)ws;
  unsigned* hist = (unsigned*)(slab + (size_t)grid * SLAB_COLS);
  unsigned* state = hist + HIST_WORDS;
  unsigned* keys = state + ST_WORDS;
  unsigned lambda_bits;
  lambda = lambda + 0.f;                            // -0 -> +0
  std::memcpy(&lambda_bits, &lambda, sizeof(lambda_bits));
  hipStream_t st = (hipStream_t)stream;
  const hipError_t e = kd_fill_async(hist, 0, (size_t)(HIST_WORDS + ST_WORDS) * sizeof(unsigned), st);
  KD_REQUIRE(e == hipSuccess, (int)e, "kd_seg_ohem_fwd_bwd: zeroing the histograms failed: %s", hipGetErrorString(e));
  OhemArgs a{zs, zt, target, class_w, ignore_index, T, alpha, gscale, gscale_dev, lambda_bits, min_kept, min_divisor,
             slab, hist, state, keys, vals, counts_out, dzs, nll_out, keep_out, npix, HW, NC};
  const dim3 g((unsigned)grid), blk(256);
  KD_LAUNCH_CLASS_BUCKET(ohem_score_kernel, NC, g, blk, st, a);
  hipLaunchKernelGGL(ohem_digit_kernel<2>, g, blk, 0, st, a);
  hipLaunchKernelGGL(ohem_digit_kernel<3>, g, blk, 0, st, a);
  hipLaunchKernelGGL(ohem_sum_kernel, g, blk, 0, st, a);
  hipLaunchKernelGGL(ohem_final_kernel, dim3(1), dim3(256), 0, st, (const double*)slab, (int)grid, (double)npix, (const unsigned*)state, vals,
                     counts_out);
  if (dzs) KD_LAUNCH_CLASS_BUCKET(ohem_grad_kernel, NC, g, blk, st, a);
  return kd_check_launch("kd_seg_ohem_fwd_bwd");
}

}  // extern "C"
