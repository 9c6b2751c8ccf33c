// kd_loss_pair.hip -- the opt-in pair-wise (pairwise-similarity) distillation feature term of the KD step (DESIGN.md section 3;
// Liu et al., "Structured Knowledge Distillation for Semantic Segmentation", CVPR 2019), in Gram form:
//   xh_i = x_i / |x_i| (0 for |x_i| <= 1e-12),  a_ij = xh_i . xh_j over the n = HW positions of an image,
//   L_b  = 1/n^2 sum_ij (a^S_ij - a^T_ij)^2 = 1/n^2 (|Gss|_F^2 - 2 |Gts|_F^2 + |Gtt|_F^2),  Gss = Sh^T Sh, Gts = Th^T Sh, Gtt = Th^T Th,
//   PAIR = 1/B sum_b L_b,  dPAIR/dSh = 4/(B n^2) (Sh Gss - Th Gts),  dPAIR/dS_i = (gh_i - xh_i (xh_i . gh_i)) / |x_i|
// on the NHWC matrices [B*HW, C]: the n x n affinity matrix is never formed.  Every product runs on the exact fp32 MFMA
// (v_mfma_f32_32x32x2_f32: a k-ordered fp32 fma chain), so there is no bf16 split and no conversion work.
// Launches.  (1) Gram: a workgroup per (image, row slice, group of 4 x 4 tiles per matrix) stages 32-row chunks of S and T through
// LDS, normalised (the reciprocal norms go to the workspace), and accumulates its 32 x 32 tiles of the three matrices over the rows,
// a wave owning one row tile of each so that 10 operand reads feed 12 products; the tiles go to a slab.  (2) join: the slices are
// summed in slice order and sum(gss^2) - 2 sum(gts^2) + sum(gtt^2) is formed in double, term by term; (2b) one block forms L_b and
// the mean over images in a fixed order.  (3) gradient: [Gss; Gts] resident in LDS (streamed in 32-row pieces when they do not fit),
// a wave owns 32 rows and forms Sh Gss and Th Gts in two accumulator sets, then the normalisation backward, the coefficient and
// 16-byte stores.
// No atomics, a fixed order everywhere, and S and T go through the same instruction sequence: with identical bits in both the three
// Gram matrices are identical bit for bit, the value is exactly 0 and ds is +-0.
#include "kd_loss_common.h"

#include <cmath>

namespace {

constexpr int THREADS = 256;
constexpr int MIN_C = 4, MAX_C = 256;
constexpr int GR = 32;                    // rows of a staged chunk of the Gram pass
constexpr int GC = 4;                     // a workgroup takes 4 row tiles (one per wave) x 4 column tiles of each of Gss, Gts, Gtt:
                                          // 12 accumulator tiles per wave, all 48 tiles of C = 128 in one workgroup
constexpr int TILE = 32 * 32;
constexpr int JB = 16;                    // join workgroups per image
constexpr int DR = 128;                   // rows of a workgroup step of the gradient pass (32 per wave)
constexpr int DK = 32;                    // columns of X staged per step of the gradient pass
constexpr int DLD = DK + 4;               // row pitch of that stage
constexpr int G_RESIDENT_BYTES = 128 * 1024;
constexpr int CUS = 256;

inline int pad32(int c) { return (c + 31) & ~31; }

struct PairGeom {
  int Csp, Ctp, nsc, ntc;       // padded widths, 32-column tiles per side
  int nss, nts, ntt, ntiles;    // tiles of Gss [Cs x Cs], Gts [Ct x Cs], Gtt [Ct x Ct]
  int cgroups, tgroups;         // groups of GC tiles per side; workgroups an image slice's tiles are spread over (cgroups^2)
  int slice_rows, slices;
  bool resident;                // [Gss; Gts] fit in LDS next to the row stage
};

// rows per slice: a multiple of the Gram chunk; a function of (B, HW) alone
inline int pair_slice_rows(int B, int HW) {
  const int64_t want = B >= CUS ? 1 : (CUS + B - 1) / B;
  const int64_t cap = ((int64_t)HW + 63) / 64;              // a slice has at least 64 rows
  const int64_t s = want < cap ? want : cap;
  const int64_t rows = ((int64_t)HW + s - 1) / s;
  return (int)((rows + GR - 1) / GR * GR);
}
inline int pair_slices(int B, int HW) {
  const int rows = pair_slice_rows(B, HW);
  return (int)(((int64_t)HW + rows - 1) / rows);
}

inline bool pair_shape_ok(int B, int HW, int Cs, int Ct) {
  return B >= 1 && HW >= 1 && HW <= (1 << 30) && Cs >= MIN_C && Cs <= MAX_C && Cs % 4 == 0 && Ct >= MIN_C && Ct <= MAX_C && Ct % 4 == 0;
}

inline PairGeom pair_geom(int B, int HW, int Cs, int Ct) {
  PairGeom g;
  g.Csp = pad32(Cs); g.Ctp = pad32(Ct);
  g.nsc = g.Csp / 32; g.ntc = g.Ctp / 32;
  g.nss = g.nsc * g.nsc; g.nts = g.ntc * g.nsc; g.ntt = g.ntc * g.ntc;
  g.ntiles = g.nss + g.nts + g.ntt;
  g.cgroups = ((g.nsc > g.ntc ? g.nsc : g.ntc) + GC - 1) / GC;
  g.tgroups = g.cgroups * g.cgroups;
  g.slice_rows = pair_slice_rows(B, HW);
  g.slices = pair_slices(B, HW);
  g.resident = (size_t)(g.Csp + g.Ctp) * g.Csp * sizeof(float) <= (size_t)G_RESIDENT_BYTES;
  return g;
}

inline size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

// workspace: [2][B*HW] reciprocal norms | [B][slices][ntiles][32][32] slab | (slices > 1) [B][ntiles][32][32] joined | [B][JB] double
// | [B] per-image values
struct PairWs { size_t rinv, slab, joined, part, img, total; };
inline PairWs pair_ws(int B, int HW, const PairGeom& g) {
  PairWs w;
  size_t o = 0;
  w.rinv = o; o += up16((size_t)2 * B * HW * sizeof(float));
  w.slab = o; o += (size_t)B * g.slices * g.ntiles * TILE * sizeof(float);
  w.joined = o; if (g.slices > 1) o += (size_t)B * g.ntiles * TILE * sizeof(float);
  w.part = o; o += up16((size_t)B * JB * sizeof(double));
  w.img = o; o += up16((size_t)B * sizeof(float));
  w.total = o;
  return w;
}

struct PairArgs {
  const float* s; const float* t;
  float* rinv_s; float* rinv_t;       // [B*HW]
  float* slab;                        // [B][slices][ntiles][32][32]
  const float* G;                     // [B][ntiles][32][32]: the joined matrices (the slab itself with one slice)
  float* ds; const float* gdev; float gcoef;
  int HW, Cs, Ct, Csp, Ctp, nsc, ntc, nss, nts, ntiles, slices, slice_rows, resident, cgroups;
};

// GQ: the float4 columns a thread holds of a row of the Gram chunk (8 threads per row): 4 up to 128 channels, 8 above

// one map's rows r0 .. r0 + 31 of a slice into registers: thread (row = t / 8, sub = t % 8) holds float4 columns sub, sub + 8, ...
template <int GQ>
__device__ __forceinline__ void gram_fetch(float4 (&p)[GQ], const float* base, int64_t r, int64_t row_end, int C, int sub) {
#pragma unroll
  for (int m = 0; m < GQ; ++m) {
    const int q = sub + 8 * m;
    p[m] = (r < row_end && 4 * q < C) ? kd_ld4(base + r * C + 4 * q) : kd_zero4();
  }
}
// normalise the fetched row, store it to the LDS stage [GR][Cp] and return 1 / |x|
template <int GQ>
__device__ __forceinline__ float gram_stage(const float4 (&p)[GQ], float* stage, int row, int sub, int C, int Cp) {
  float ss = 0.f;
#pragma unroll
  for (int m = 0; m < GQ; ++m) ss = sumsq4(p[m], ss);          // columns past C hold zeros
  const float rinv = inv_norm(row8_sum(ss));
#pragma unroll
  for (int m = 0; m < GQ; ++m) {
    const int q = sub + 8 * m;
    if (4 * q < C) kd_st4(stage + row * Cp + 4 * q, scale4(p[m], rinv));
  }
  return rinv;
}

// The products of one staged chunk for one wave: row tile `ri` of both sides against the column tiles c0 .. c0 + 3 of both sides.
// ss = (S row tile)^T (S column tiles), ts = (T row tile)^T (S column tiles), tt = (T row tile)^T (T column tiles): 10 operand reads
// feed 12 products per k step.  FULL: every tile exists (the whole of C = 128 on both sides); otherwise each is guarded, wave-uniformly.
template <bool FULL>
__device__ __forceinline__ void gram_chunk(f32x16 (&ss)[GC], f32x16 (&ts)[GC], f32x16 (&tt)[GC], const float* pS, const float* pT, int Csp,
                                           int Ctp, int ri, int c0, int nsc, int ntc) {
  const bool rowS = FULL || ri < nsc, rowT = FULL || ri < ntc;
#pragma unroll 4
  for (int kk = 0; kk < GR / 2; ++kk) {
    const float* qS = pS + 2 * kk * Csp;
    const float* qT = pT + 2 * kk * Ctp;
    const float as = rowS ? qS[32 * ri] : 0.f, at = rowT ? qT[32 * ri] : 0.f;
    float bs[GC], bt[GC];
#pragma unroll
    for (int j = 0; j < GC; ++j) {
      bs[j] = (FULL || c0 + j < nsc) ? qS[32 * (c0 + j)] : 0.f;
      bt[j] = (FULL || c0 + j < ntc) ? qT[32 * (c0 + j)] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < GC; ++j) {
      if (FULL || (rowS && c0 + j < nsc)) ss[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(as, bs[j], ss[j], 0, 0, 0);
      if (FULL || (rowT && c0 + j < nsc)) ts[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(at, bs[j], ts[j], 0, 0, 0);
      if (FULL || (rowT && c0 + j < ntc)) tt[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(at, bt[j], tt[j], 0, 0, 0);
    }
  }
}

__device__ __forceinline__ void tile_store(float* out, const f32x16& acc, int lane) {
#pragma unroll
  for (int r = 0; r < 16; ++r) out[((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * 32 + (lane & 31)] = acc[r];
}

// Launch 1.  grid = (B * slices, tgroups).  LDS: [GR][Csp] of Sh, then [GR][Ctp] of Th; the columns past C stay 0.
// blockIdx.y = (group of 4 row tiles, group of 4 column tiles): one group at widths up to 128, four above.
template <int GQ>
__global__ __launch_bounds__(THREADS) void pair_gram_kernel(PairArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int t = threadIdx.x, lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int b = blockIdx.x / a.slices, sl = blockIdx.x % a.slices, z = blockIdx.y;
  const int ri = GC * (z / a.cgroups) + w, c0 = GC * (z % a.cgroups);
  const bool full = GC * (z / a.cgroups) + GC <= min(a.nsc, a.ntc) && c0 + GC <= min(a.nsc, a.ntc);
  const int toff = GR * a.Csp;                                  // Th's stage
  for (int i = t; i < GR * (a.Csp + a.Ctp); i += THREADS) lds[i] = 0.f;
  f32x16 ss[GC], ts[GC], tt[GC];
#pragma unroll
  for (int i = 0; i < GC; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) { ss[i][r] = 0.f; ts[i][r] = 0.f; tt[i][r] = 0.f; }

  const int row = t >> 3, sub = t & 7;
  const int64_t row_lo = (int64_t)sl * a.slice_rows;
  const int64_t row_end = min((int64_t)a.HW, row_lo + a.slice_rows);
  const float* sb = a.s + (int64_t)b * a.HW * a.Cs;
  const float* tb = a.t + (int64_t)b * a.HW * a.Ct;
  const float* pS = lds + (lane >> 5) * a.Csp + (lane & 31);    // row = the MFMA's k, column = the tile's i / j
  const float* pT = lds + toff + (lane >> 5) * a.Ctp + (lane & 31);
  float4 ps[GQ], pt[GQ];
  gram_fetch(ps, sb, row_lo + row, row_end, a.Cs, sub);
  gram_fetch(pt, tb, row_lo + row, row_end, a.Ct, sub);
  __syncthreads();                                              // the zero fill
#pragma unroll 1
  for (int64_t r0 = row_lo; r0 < row_end; r0 += GR) {
    const float ris = gram_stage(ps, lds, row, sub, a.Cs, a.Csp);
    const float rit = gram_stage(pt, lds + toff, row, sub, a.Ct, a.Ctp);
    if (sub == 0 && z == 0 && r0 + row < row_end) {
      a.rinv_s[(int64_t)b * a.HW + r0 + row] = ris;
      a.rinv_t[(int64_t)b * a.HW + r0 + row] = rit;
    }
    __syncthreads();
    if (r0 + GR < row_end) {                                    // the next chunk's loads fly under this chunk's products
      gram_fetch(ps, sb, r0 + GR + row, row_end, a.Cs, sub);
      gram_fetch(pt, tb, r0 + GR + row, row_end, a.Ct, sub);
    }
    if (full) gram_chunk<true>(ss, ts, tt, pS, pT, a.Csp, a.Ctp, ri, c0, a.nsc, a.ntc);
    else gram_chunk<false>(ss, ts, tt, pS, pT, a.Csp, a.Ctp, ri, c0, a.nsc, a.ntc);
    __syncthreads();
  }
  float* out = a.slab + ((int64_t)b * a.slices + sl) * a.ntiles * TILE;
#pragma unroll
  for (int j = 0; j < GC; ++j) {
    const int cj = c0 + j;
    if (ri < a.nsc && cj < a.nsc) tile_store(out + (int64_t)(ri * a.nsc + cj) * TILE, ss[j], lane);
    if (ri < a.ntc && cj < a.nsc) tile_store(out + (int64_t)(a.nss + ri * a.nsc + cj) * TILE, ts[j], lane);
    if (ri < a.ntc && cj < a.ntc) tile_store(out + (int64_t)(a.nss + a.nts + ri * a.ntc + cj) * TILE, tt[j], lane);
  }
}

// Launch 2.  grid = (JB, B): workgroup jb sums the slices of its share of the padded elements in slice order (and stores the joined
// matrices when there is more than one slice) and forms its share of sum gss^2 - 2 gts^2 + gtt^2 in double.  The three matrices are
// walked with ONE index: with equal widths element e is the same entry of all three.
__global__ __launch_bounds__(THREADS) void pair_join_kernel(const float* slab, float* joined, double* part, int slices, int nss, int nts,
                                                            int ntt) {
  __shared__ double red[THREADS];
  const int b = blockIdx.y, jb = blockIdx.x, t = threadIdx.x;
  const int64_t Nss = (int64_t)nss * TILE, Nts = (int64_t)nts * TILE, Ntt = (int64_t)ntt * TILE, N = Nss + Nts + Ntt;
  const int64_t nmax = max(Nss, max(Nts, Ntt));
  const int64_t seg = (nmax + JB - 1) / JB;
  const int64_t lo = jb * seg, hi = min(nmax, lo + seg);
  const float* sl0 = slab + (int64_t)b * slices * N;
  float* jo = joined ? joined + (int64_t)b * N : nullptr;
  double acc = 0.0;
  for (int64_t e = lo + t; e < hi; e += THREADS) {
    float g[3] = {0.f, 0.f, 0.f};
    const int64_t off[3] = {0, Nss, Nss + Nts}, cnt[3] = {Nss, Nts, Ntt};
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      if (e < cnt[m]) {
        float v = sl0[off[m] + e];
        for (int k = 1; k < slices; ++k) v += sl0[(int64_t)k * N + off[m] + e];
        if (jo) jo[off[m] + e] = v;
        g[m] = v;
      }
    }
    acc += ((double)g[0] * (double)g[0] - 2.0 * ((double)g[1] * (double)g[1])) + (double)g[2] * (double)g[2];
  }
  red[t] = acc;
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int i = 0; i < THREADS; ++i) s += red[i];
    part[(int64_t)b * JB + jb] = s;
  }
}

// Launch 2b.  One block: L_b = (the image's JB partials in order) / n^2, then the mean over images in a fixed order.
__global__ __launch_bounds__(THREADS) void pair_final_kernel(const double* part, int B, double inv_n2, float* img_ws, float* img_out, float* val) {
  __shared__ double red[THREADS];
  double s = 0.0;
  for (int b = threadIdx.x; b < B; b += THREADS) {
    double l = 0.0;
    for (int j = 0; j < JB; ++j) l += part[(int64_t)b * JB + j];
    l *= inv_n2;
    img_ws[b] = (float)l;
    if (img_out) img_out[b] = (float)l;
    s += l;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int i = 0; i < THREADS; ++i) tot += red[i];
    val[0] = (float)(tot / (double)B);
  }
}

// element (c, j) of a joined matrix whose tiles are [c / 32][j / 32] with `ncol` column tiles, first tile `tau0`
__device__ __forceinline__ const float* tile_elem(const float* G, int tau0, int ncol, int c, int j) {
  return G + (int64_t)(tau0 + (c >> 5) * ncol + (j >> 5)) * TILE + (c & 31) * 32 + (j & 31);
}

// One side of the gradient pass: acc[jt] += Xh[rows of this wave][0 .. Cp) . Gm[0 .. Cp)[32 jt .. 32 jt + 32), Xh = x * rinv formed on the
// way into the LDS stage, DK columns per step.  Gm: rows [grow0, grow0 + Cp) of the resident image, or streamed per step.
template <int NTJ>
__device__ __forceinline__ void grad_side(f32x16 (&acc)[NTJ], const PairArgs& a, const float* xb, int C, int Cp, int64_t r0, int64_t row_end,
                                          const float* rinv, const float* Gb, int tau0, int grow0, float* xs, float* gl) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int q = t & 7, rr = t >> 3;
  float ri[4];
  float4 pre[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t r = r0 + rr + 32 * i;
    ri[i] = r < row_end ? rinv[r] : 0.f;
    pre[i] = (r < row_end && 4 * q < C) ? kd_ld4(xb + r * C + 4 * q) : kd_zero4();
  }
  const int steps = Cp / DK;
#pragma unroll 1
  for (int st = 0; st < steps; ++st) {
#pragma unroll
    for (int i = 0; i < 4; ++i) kd_st4(xs + (rr + 32 * i) * DLD + 4 * q, scale4(pre[i], ri[i]));
    if (!a.resident) {                                          // rows DK * st .. of this side's matrix, [DK][Csp]
      const int n4 = a.Csp / 4;
      for (int idx = t; idx < DK * n4; idx += THREADS) {
        const int c = idx / n4, j = 4 * (idx % n4);
        kd_st4(gl + c * a.Csp + j, kd_ld4(tile_elem(Gb, tau0, a.nsc, DK * st + c, j)));
      }
    }
    __syncthreads();
    if (st + 1 < steps) {
      const int col = DK * (st + 1) + 4 * q;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t r = r0 + rr + 32 * i;
        pre[i] = (r < row_end && col < C) ? kd_ld4(xb + r * C + col) : kd_zero4();
      }
    }
    const float* gm = a.resident ? gl + (grow0 + DK * st) * a.Csp : gl;
    const float* xa = xs + (32 * w + (lane & 31)) * DLD + (lane >> 5);
    const float* gb = gm + (lane >> 5) * a.Csp + (lane & 31);
#pragma unroll
    for (int kk = 0; kk < DK / 2; ++kk) {
      const float av = xa[2 * kk];
#pragma unroll
      for (int jt = 0; jt < NTJ; ++jt)
        if (jt < a.nsc) acc[jt] = __builtin_amdgcn_mfma_f32_32x32x2f32(gb[2 * kk * a.Csp + 32 * jt], av, acc[jt], 0, 0, 0);
    }
    __syncthreads();
  }
}

// Launch 3.  grid = B * slices.  LDS: the row stage [DR][DLD], then [Gss; Gts] as [Csp + Ctp][Csp] (resident) or one [DK][Csp] piece.
template <int NTJ>
__global__ __launch_bounds__(THREADS) void pair_grad_kernel(PairArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xs = lds;
  float* gl = lds + DR * DLD;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int b = blockIdx.x / a.slices, sl = blockIdx.x % a.slices;
  const float* Gb = a.G + (int64_t)b * a.ntiles * TILE;
  if (a.resident) {
    const int n4 = a.Csp / 4;
    for (int idx = t; idx < (a.Csp + a.Ctp) * n4; idx += THREADS) {
      const int c = idx / n4, j = 4 * (idx % n4);
      const float* src = c < a.Csp ? tile_elem(Gb, 0, a.nsc, c, j) : tile_elem(Gb, a.nss, a.nsc, c - a.Csp, j);
      kd_st4(gl + c * a.Csp + j, kd_ld4(src));
    }
  }
  const float k = a.gdev ? __fmul_rn(a.gcoef, a.gdev[0]) : a.gcoef;
  const int64_t row_lo = (int64_t)sl * a.slice_rows;
  const int64_t row_end = min((int64_t)a.HW, row_lo + a.slice_rows);
  const float* sb = a.s + (int64_t)b * a.HW * a.Cs;
  const float* tb = a.t + (int64_t)b * a.HW * a.Ct;
  const float* rs = a.rinv_s + (int64_t)b * a.HW;
  const float* rt = a.rinv_t + (int64_t)b * a.HW;
  float* db = a.ds + (int64_t)b * a.HW * a.Cs;
#pragma unroll 1
  for (int64_t r0 = row_lo; r0 < row_end; r0 += DR) {
    f32x16 accS[NTJ], accT[NTJ];
#pragma unroll
    for (int jt = 0; jt < NTJ; ++jt)
#pragma unroll
      for (int r = 0; r < 16; ++r) { accS[jt][r] = 0.f; accT[jt][r] = 0.f; }
    grad_side<NTJ>(accS, a, sb, a.Cs, a.Csp, r0, row_end, rs, Gb, 0, 0, xs, gl);
    grad_side<NTJ>(accT, a, tb, a.Ct, a.Ctp, r0, row_end, rt, Gb, a.nss, a.Csp, xs, gl);
    // the matrix is the A operand and the rows are the B operand, so a tile is [j][row]: the row on lane & 31 and four consecutive
    // columns j = 32 jt + 8 g + 4 (lane >> 5) + 0..3 in registers 4 g .. 4 g + 3: a float4 of x and of ds
    const int64_t rw = r0 + 32 * w + (lane & 31);
    const int h = lane >> 5;
    const bool rok = rw < row_end;
    const float ri = rok ? rs[rw] : 0.f;
    const float* xrow = sb + rw * a.Cs;
    float dot = 0.f;                                             // xh_i . gh_i: this lane's columns, then the other half-wave's
#pragma unroll
    for (int jt = 0; jt < NTJ; ++jt) {
      if (jt < a.nsc) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int j = 32 * jt + 8 * g + 4 * h;
          const float4 xh = scale4((rok && j < a.Cs) ? kd_ld4(xrow + j) : kd_zero4(), ri);
          const float g0 = accS[jt][4 * g] - accT[jt][4 * g], g1 = accS[jt][4 * g + 1] - accT[jt][4 * g + 1];
          const float g2 = accS[jt][4 * g + 2] - accT[jt][4 * g + 2], g3 = accS[jt][4 * g + 3] - accT[jt][4 * g + 3];
          accS[jt][4 * g] = g0; accS[jt][4 * g + 1] = g1; accS[jt][4 * g + 2] = g2; accS[jt][4 * g + 3] = g3;
          dot = fmaf(xh.w, g3, fmaf(xh.z, g2, fmaf(xh.y, g1, fmaf(xh.x, g0, dot))));
        }
      }
    }
    dot += __shfl_xor(dot, 32, 64);
#pragma unroll
    for (int jt = 0; jt < NTJ; ++jt) {
      if (jt < a.nsc) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int j = 32 * jt + 8 * g + 4 * h;
          if (rok && j < a.Cs) {
            const float4 xh = scale4(kd_ld4(xrow + j), ri);
            float4 d;
            d.x = __fmul_rn(k, __fmul_rn(fmaf(-xh.x, dot, accS[jt][4 * g]), ri));
            d.y = __fmul_rn(k, __fmul_rn(fmaf(-xh.y, dot, accS[jt][4 * g + 1]), ri));
            d.z = __fmul_rn(k, __fmul_rn(fmaf(-xh.z, dot, accS[jt][4 * g + 2]), ri));
            d.w = __fmul_rn(k, __fmul_rn(fmaf(-xh.w, dot, accS[jt][4 * g + 3]), ri));
            kd_st4(db + rw * a.Cs + j, d);
          }
        }
      }
    }
  }
}

}  // namespace

extern "C" {

size_t kd_feat_pair_ws_bytes(int B, int HW, int Cs, int Ct) {
  if (!pair_shape_ok(B, HW, Cs, Ct)) return 0;
  return pair_ws(B, HW, pair_geom(B, HW, Cs, Ct)).total;
}

int kd_feat_pair_slices(int B, int HW) { return (B < 1 || HW < 1 || HW > (1 << 30)) ? 0 : pair_slices(B, HW); }

int kd_feat_pair_fwd_bwd(const float* s, const float* t, int B, int HW, int Cs, int Ct, float gcoef, const float* gscale_dev, float* val,
                         float* ds, float* img_vals_out, void* ws, size_t ws_bytes, void* stream) {
  KD_REQUIRE(s && t && val, KD_ERR_ARG, "kd_feat_pair_fwd_bwd: null s, t or val");
  KD_REQUIRE(std::isfinite(gcoef), KD_ERR_ARG, "kd_feat_pair_fwd_bwd: gcoef must be finite (got %g)", (double)gcoef);
  KD_REQUIRE(pair_shape_ok(B, HW, Cs, Ct), KD_ERR_SHAPE,
             "kd_feat_pair_fwd_bwd: B=%d, HW=%d, Cs=%d, Ct=%d unsupported (B >= 1, 1 <= HW <= 2^30; widths multiples of 4 from %d to %d)", B, HW, Cs, Ct,
             MIN_C, MAX_C);
  const PairGeom g = pair_geom(B, HW, Cs, Ct);
  KD_REQUIRE((int64_t)B * g.slices <= 0x7fffffff && B <= 65535, KD_ERR_SHAPE, "kd_feat_pair_fwd_bwd: B=%d x %d row slices exceeds the grid", B,
             g.slices);
  KD_REQUIRE(ws, KD_ERR_ARG, "kd_feat_pair_fwd_bwd: null workspace");
  const PairWs l = pair_ws(B, HW, g);
  KD_REQUIRE(ws_bytes >= l.total, KD_ERR_WORKSPACE, "kd_feat_pair_fwd_bwd: workspace too small (%zu < %zu bytes)", ws_bytes, l.total);
  KD_REQUIRE(kd_aligned16(s) && kd_aligned16(t) && kd_aligned16(ws) && (!ds || kd_aligned16(ds)), KD_ERR_ALIGN,
             "kd_feat_pair_fwd_bwd: s, t, ds and ws must be 16-byte aligned");
  char* base = (char*)ws;
  float* rinv = (float*)(base + l.rinv);
  float* slab = (float*)(base + l.slab);
  float* joined = g.slices > 1 ? (float*)(base + l.joined) : nullptr;
  double* part = (double*)(base + l.part);
  float* img = (float*)(base + l.img);
  hipStream_t st = (hipStream_t)stream;
  PairArgs a{s, t, rinv, rinv + (int64_t)B * HW, slab, joined ? joined : slab, ds, gscale_dev, gcoef, HW, Cs, Ct, g.Csp, g.Ctp, g.nsc, g.ntc,
             g.nss, g.nts, g.ntiles, g.slices, g.slice_rows, g.resident ? 1 : 0, g.cgroups};
  const size_t grad_lds = (size_t)DR * DLD * sizeof(float) + (g.resident ? (size_t)(g.Csp + g.Ctp) * g.Csp : (size_t)DK * g.Csp) * sizeof(float);
  const void* grad_fn = g.nsc <= 4 ? (const void*)pair_grad_kernel<4> : (const void*)pair_grad_kernel<8>;
  if (ds) {                                                     // before any launch: a refused call writes nothing
    static std::atomic<uint64_t> raised[2];
    const hipError_t le = kd_raise_dynamic_lds(grad_fn, G_RESIDENT_BYTES + DR * DLD * sizeof(float), raised[g.nsc <= 4 ? 0 : 1]);
    KD_REQUIRE(le == hipSuccess, (int)le, "kd_feat_pair_fwd_bwd: cannot raise the dynamic LDS limit: %s", hipGetErrorString(le));
  }
  const size_t gram_lds = (size_t)GR * (g.Csp + g.Ctp) * sizeof(float);
  const dim3 gram_grid((unsigned)(B * g.slices), (unsigned)g.tgroups);
  if (g.cgroups == 1) hipLaunchKernelGGL(pair_gram_kernel<4>, gram_grid, dim3(THREADS), gram_lds, st, a);
  else hipLaunchKernelGGL(pair_gram_kernel<8>, gram_grid, dim3(THREADS), gram_lds, st, a);
  hipLaunchKernelGGL(pair_join_kernel, dim3(JB, (unsigned)B), dim3(THREADS), 0, st, (const float*)slab, joined, part, g.slices, g.nss, g.nts,
                     g.ntt);
  hipLaunchKernelGGL(pair_final_kernel, dim3(1), dim3(THREADS), 0, st, (const double*)part, B, 1.0 / ((double)HW * (double)HW), img,
                     img_vals_out, val);
  if (ds) {
    if (g.nsc <= 4) hipLaunchKernelGGL(pair_grad_kernel<4>, dim3((unsigned)(B * g.slices)), dim3(THREADS), grad_lds, st, a);
    else hipLaunchKernelGGL(pair_grad_kernel<8>, dim3((unsigned)(B * g.slices)), dim3(THREADS), grad_lds, st, a);
  }
  return kd_check_launch("kd_feat_pair_fwd_bwd");
}

}  // extern "C"
