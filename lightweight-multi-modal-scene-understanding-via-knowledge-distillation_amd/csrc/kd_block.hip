// kd_block.hip -- inference-mode fusion of a depthwise-separable tail:
//     depthwise 3x3 (input BatchNorm + activation applied on load) -> BatchNorm -> activation -> 1x1 conv -> BatchNorm
//     -> activation (+ residual)
// in ONE kernel, for the eval-mode / no-grad forward (frozen KD teacher, validation): the last two units of an
// InvertedResidual (camera_encoder.py:30-42: dw 3x3 + BN + ReLU6, project 1x1 + BN, + x) and every DWSeparableConv
// (fusion_module.py:25-34: dw 3x3 + BN + ReLU, 1x1 + BN + ReLU).  In eval mode all BatchNorm coefficients are known before
// the kernel starts, so the depthwise output -- the widest tensor of the block (6x the block's channels) -- never goes to
// HBM: the separate kernels write it once and read it once.
//
// A workgroup owns a tile of TH x TW output pixels of one image (8 x 16 at stride 1, 8 x 8 at stride 2 = the M-tile of the
// GEMM: 128 / 64 rows) and ALL output channels (32, 64 or 128), and walks the hidden channels in chunks of 32:
//   1. the chunk's input halo tile ((TH-1)*S+3) x ((TW-1)*S+3) pixels x 32 channels is loaded (registers, one chunk ahead),
//      activated (deferred BatchNorm + activation of the producer, zero outside the image) and staged in LDS as fp32;
//      the chunk of the 1x1 weight is cut into its three bf16 planes and staged too;
//   2. thread (pixel, channel quad) computes the depthwise output from LDS (same fma order as dw_fwd_sw_kernel), applies
//      BatchNorm + activation, cuts the four values into three bf16 pieces and writes them where the MFMA A operand wants them;
//   3. the four waves accumulate the 32-wide K-chunk on v_mfma_f32_32x32x16_bf16 (six piece products per product, fp32
//      accumulate) -- the same arithmetic in the same order as pw_gemm_kernel<.., SPLIT> / pw_stream_kernel.
// Epilogue: BatchNorm + activation (+ residual) straight from the accumulators, dword stores (EPI5 of the GEMM kernels).
// The result is bit-identical to kd_dwconv3x3_fwd followed by kd_pwconv_gemm(pro 1, epi 5) in the split arithmetic
// (tests/test_gpu_units.py::test_dw_pw_inference_fusion_same_bits).
// block_infer_kernel (below) puts the expand 1x1 of an InvertedResidual in front of the same phases: the whole block in one kernel.
#include "kd_gemm_args.h"

namespace {

struct DwPwArgs {
  const float* x; const float* isc; const float* ish; int iact;     // depthwise input [B,H,W,Ch]: raw + deferred BN (isc null: as is)
  const float* wd;                                                  // depthwise taps [Ch][9]
  const float* dsc; const float* dsh; int dact;                     // BatchNorm (eval affine) + activation behind the depthwise conv
  const float* wp; const float* pbias;                              // 1x1 weight [Cout][Ch], bias [Cout] or null
  const float* psc; const float* psh; int pact;                     // BatchNorm + activation behind the 1x1 conv
  const float* res; int64_t ldres;                                  // optional residual [B*Ho*Wo][ldres], added last
  float* out; int64_t ldo;                                          // [B*Ho*Wo][ldo]
  int B, H, W, Ch, Ho, Wo;
  int tiles_x, tiles_y;
};

// 256 threads and 32 hidden channels per chunk: two workgroups per CU, so one's barriers and load waits overlap the other's
// phases.  (512 threads with 64-channel chunks -- half the barriers, one workgroup per CU -- measured 0-35 % SLOWER.)
constexpr int NTHR = 256, KC = 32, CQN = KC / 4;                    // threads per workgroup; hidden channels per chunk; channel quads per chunk
constexpr int XLD = KC + 4;                                         // floats per staged pixel (pad: rows stay 16-byte aligned)
// bf16 offset of 16-byte chunk `chunk` in a 64-byte row, XOR-swizzled by (row >> 2) & 3 (the LDS image of pw_gemm_kernel<.., SPLIT>:
// conflict-free for the ds_read_b128 lane groups and for the 8-byte stores)
__device__ __forceinline__ int sw_off(int row, int chunk) { return (chunk ^ ((row >> 2) & 3)) * 8; }

// ---- phases shared by dw_pw_infer_kernel and block_infer_kernel (thread (pl, cq) = (pixel / weight-row lane, channel quad)) ---------
// the chunk of the 1x1 weight, rows pl + 32 i, cut into its three bf16 planes
template <int NCB>
__device__ __forceinline__ void stage_wp(unsigned short* Wp, const float4 (&wr)[NCB], int pl, int cq) {
  constexpr int COUT = 32 * NCB;
#pragma unroll
  for (int i = 0; i < NCB; ++i) {
    const int n = pl + 32 * i;
    uint2 hi, mid, lo;
    kd_split3(wr[i], hi, mid, lo);
    unsigned short* d = Wp + n * KC + sw_off(n, cq >> 1) + (cq & 1) * 4;
    *reinterpret_cast<uint2*>(d) = hi;
    *reinterpret_cast<uint2*>(d + COUT * KC) = mid;
    *reinterpret_cast<uint2*>(d + 2 * COUT * KC) = lo;
  }
}

// 4 channels x 9 taps as loaded (contiguous) -> per-channel tap rows
__device__ __forceinline__ void taps_of(const float4 (&wt)[9], float (&w9)[4][9]) {
  const float flat[36] = {wt[0].x, wt[0].y, wt[0].z, wt[0].w, wt[1].x, wt[1].y, wt[1].z, wt[1].w, wt[2].x, wt[2].y, wt[2].z, wt[2].w,
                          wt[3].x, wt[3].y, wt[3].z, wt[3].w, wt[4].x, wt[4].y, wt[4].z, wt[4].w, wt[5].x, wt[5].y, wt[5].z, wt[5].w,
                          wt[6].x, wt[6].y, wt[6].z, wt[6].w, wt[7].x, wt[7].y, wt[7].z, wt[7].w, wt[8].x, wt[8].y, wt[8].z, wt[8].w};
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int tp = 0; tp < 9; ++tp) w9[j][tp] = flat[j * 9 + tp];
}

// depthwise 3x3 on the staged tile -> BatchNorm + activation -> three bf16 planes of the A tile
template <int STRIDE>
__device__ __forceinline__ void dw_phase(const float* Xs, unsigned short* Ap, const float (&w9)[4][9], float4 csc, float4 csh, int dact,
                                         int pl, int cq) {
  constexpr int TH = 8, TW = STRIDE == 1 ? 16 : 8, MT = TH * TW, WT = (TW - 1) * STRIDE + 3;
#pragma unroll
  for (int p = 0; p < MT / 32; ++p) {
    const int px = p * 32 + pl;
    const int ty = px / TW, tx = px % TW;
    const float* xp = Xs + ((ty * STRIDE) * WT + tx * STRIDE) * XLD + 4 * cq;
    float4 v = kd_zero4();
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const float4 l = kd_ld4(xp + (kh * WT + 0) * XLD), c = kd_ld4(xp + (kh * WT + 1) * XLD), rr = kd_ld4(xp + (kh * WT + 2) * XLD);
      v.x = fmaf(l.x, w9[0][kh * 3], fmaf(c.x, w9[0][kh * 3 + 1], fmaf(rr.x, w9[0][kh * 3 + 2], v.x)));
      v.y = fmaf(l.y, w9[1][kh * 3], fmaf(c.y, w9[1][kh * 3 + 1], fmaf(rr.y, w9[1][kh * 3 + 2], v.y)));
      v.z = fmaf(l.z, w9[2][kh * 3], fmaf(c.z, w9[2][kh * 3 + 1], fmaf(rr.z, w9[2][kh * 3 + 2], v.z)));
      v.w = fmaf(l.w, w9[3][kh * 3], fmaf(c.w, w9[3][kh * 3 + 1], fmaf(rr.w, w9[3][kh * 3 + 2], v.w)));
    }
    v = kd_affine_act4(v, csc, csh, dact);
    uint2 hi, mid, lo;
    kd_split3(v, hi, mid, lo);
    unsigned short* d = Ap + px * KC + sw_off(px, cq >> 1) + (cq & 1) * 4;
    *reinterpret_cast<uint2*>(d) = hi;
    *reinterpret_cast<uint2*>(d + MT * KC) = mid;
    *reinterpret_cast<uint2*>(d + 2 * MT * KC) = lo;
  }
}

constexpr int TSN = KC * 9 + 2 * KC;                               // floats of a chunk's depthwise record: taps [KC][9], scale [KC], shift [KC]
constexpr int PA[6] = {0, 2, 1, 0, 1, 0}, PB[6] = {2, 0, 1, 1, 0, 0};    // six piece products, smallest terms first (as pw_gemm_kernel)

// one K-chunk of the project GEMM in 16-wide steps: row block rb, column blocks jb0 .. jb0 + NBW - 1
template <int MT, int COUT, int NBW>
__device__ __forceinline__ void project_chunk(const unsigned short* Ap, const unsigned short* Wp, f32x16 (&acc)[NBW], int rb, int jb0, int r, int h) {
#pragma unroll
  for (int ks = 0; ks < KC / 16; ++ks) {
    const int ko = sw_off(r, ks * 2 + h);                             // swizzle bits of a block row == those of its lane: block offsets are multiples of 32
    bf16x8 fa[3], fb[NBW][3];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      fa[p] = *reinterpret_cast<const bf16x8*>(Ap + (p * MT + rb * 32 + r) * KC + ko);
#pragma unroll
      for (int j = 0; j < NBW; ++j) fb[j][p] = *reinterpret_cast<const bf16x8*>(Wp + (p * COUT + (jb0 + j) * 32 + r) * KC + ko);
    }
#pragma unroll
    for (int tt = 0; tt < 6; ++tt)
#pragma unroll
      for (int j = 0; j < NBW; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[PA[tt]], fb[j][PB[tt]], acc[j], 0, 0, 0);
  }
}

// epilogue: BatchNorm + activation (+ residual), register q of a block = tile row (q & 3) + 8 (q >> 2) + 4 h
template <int TW, int NBW>
__device__ __forceinline__ void tail_epilogue(const DwPwArgs& a, const f32x16 (&acc)[NBW], int b, int ty0, int tx0, int rb, int jb0, int r, int h) {
#pragma unroll
  for (int j = 0; j < NBW; ++j) {
    const int col = (jb0 + j) * 32 + r;
    const float bias = a.pbias ? a.pbias[col] : 0.f, esc = a.psc[col], esh = a.psh[col];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int px = rb * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
      const int oy = ty0 + px / TW, ox = tx0 + px % TW;
      if (oy < a.Ho && ox < a.Wo) {
        const int64_t m = ((int64_t)b * a.Ho + oy) * a.Wo + ox;
        float v = kd_act(kd_affine(acc[j][q] + bias, esc, esh), a.pact);
        if (a.res) v += a.res[m * a.ldres + col];
        a.out[m * a.ldo + col] = v;
      }
    }
  }
}

template <int STRIDE, int NCB>                                       // NCB = Cout / 32
__global__ __launch_bounds__(NTHR, 2) void dw_pw_infer_kernel(DwPwArgs a) {
  constexpr int TH = 8, TW = STRIDE == 1 ? 16 : 8, MT = TH * TW, NRB = MT / 32;
  constexpr int HT = (TH - 1) * STRIDE + 3, WT = (TW - 1) * STRIDE + 3, HP = HT * WT;
  constexpr int COUT = 32 * NCB;
  constexpr int NH = (HP * CQN + NTHR - 1) / NTHR;                   // halo float4 per thread per chunk
  constexpr int NJG = (NTHR / 64) / NRB;                             // groups of column blocks the waves split into
  constexpr int NBW = NCB >= NJG ? NCB / NJG : 1;                    // 32x32 accumulator blocks per (working) wave
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float* Xs = reinterpret_cast<float*>(smem_raw);                                          // [HP][XLD] activated input, fp32
  unsigned short* Ap = reinterpret_cast<unsigned short*>(smem_raw + (size_t)HP * XLD * 4); // [3][MT][KC] bf16 planes of the A tile
  unsigned short* Wp = Ap + 3 * MT * KC;                                                   // [3][COUT][KC] bf16 planes of the W chunk
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;

  int t = blockIdx.x;
  const int tx0 = (t % a.tiles_x) * TW; t /= a.tiles_x;
  const int ty0 = (t % a.tiles_y) * TH;
  const int b = t / a.tiles_y;
  const int iy0 = ty0 * STRIDE - 1, ix0 = tx0 * STRIDE - 1;          // input coordinates of halo pixel (0, 0)
  const int cq = tid & (CQN - 1);                                     // this thread's channel quad of the chunk, in every phase
  const int pl = tid / CQN;                                           // ... and its pixel / weight-row lane (0..31)
  const bool deferred = a.isc != nullptr;

  // accumulator blocks of this wave: row block rb, column blocks jb0 .. jb0 + NBW - 1 (waves beyond the block count only stage)
  const int rb = wave % NRB;
  const int jb0 = (wave / NRB) * NBW;
  const bool mma = jb0 < NCB;
  f32x16 acc[NBW];
#pragma unroll
  for (int j = 0; j < NBW; ++j)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[j][q] = 0.f;

  // ---- per-chunk global loads, one chunk ahead -------------------------------------------------------------------------------
  float4 xh[NH], wr[NCB], wt[9], isc = make_float4(1.f, 1.f, 1.f, 1.f), ish = kd_zero4(), dsc, dsh;
  auto issue = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NH; ++i) {
      int e = tid + NTHR * i;
      e = e < HP * CQN ? e : HP * CQN - 1;
      const int hp = e / CQN;
      int iy = iy0 + hp / WT, ix = ix0 + hp % WT;
      iy = iy < 0 ? 0 : (iy >= a.H ? a.H - 1 : iy);
      ix = ix < 0 ? 0 : (ix >= a.W ? a.W - 1 : ix);
      xh[i] = kd_ld4(a.x + (((int64_t)b * a.H + iy) * a.W + ix) * a.Ch + k0 + 4 * cq);
    }
#pragma unroll
    for (int i = 0; i < NCB; ++i) wr[i] = kd_ld4(a.wp + (int64_t)(pl + 32 * i) * a.Ch + k0 + 4 * cq);
#pragma unroll
    for (int i = 0; i < 9; ++i) wt[i] = kd_ld4(a.wd + (int64_t)(k0 + 4 * cq) * 9 + 4 * i);     // 4 channels x 9 taps, contiguous
    if (deferred) { isc = kd_ld4(a.isc + k0 + 4 * cq); ish = kd_ld4(a.ish + k0 + 4 * cq); }
    dsc = kd_ld4(a.dsc + k0 + 4 * cq); dsh = kd_ld4(a.dsh + k0 + 4 * cq);
  };

  issue(0);
  for (int k0 = 0; k0 < a.Ch; k0 += KC) {
    // ---- 1. stage the activated halo tile and the split W chunk ------------------------------------------------------------
#pragma unroll
    for (int i = 0; i < NH; ++i) {
      const int e = tid + NTHR * i;
      const int hp = (e < HP * CQN ? e : HP * CQN - 1) / CQN;
      const int iy = iy0 + hp / WT, ix = ix0 + hp % WT;
      const bool ok = iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
      float4 v = xh[i];
      if (deferred) v = kd_affine_act4(v, isc, ish, a.iact);
      v = make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f);
      if (e < HP * CQN) kd_st4(Xs + hp * XLD + 4 * cq, v);
    }
    stage_wp<NCB>(Wp, wr, pl, cq);
    // the depthwise taps / coefficients of THIS chunk move to their own registers: the prefetch below overwrites wt, dsc, dsh
    float w9[4][9];
    taps_of(wt, w9);
    const float4 csc = dsc, csh = dsh;
    kd_lds_barrier();
    if (k0 + KC < a.Ch) issue(k0 + KC);                               // flies during the depthwise phase and the MFMAs

    // ---- 2. depthwise 3x3 on the staged tile -> BatchNorm + activation -> three bf16 planes of the A tile -------------------
    dw_phase<STRIDE>(Xs, Ap, w9, csc, csh, a.dact, pl, cq);
    kd_lds_barrier();

    // ---- 3. one K-chunk of the GEMM in 16-wide steps -------------------------------------------------------------------------
    if (mma) project_chunk<MT, COUT, NBW>(Ap, Wp, acc, rb, jb0, r, h);
    kd_lds_barrier();                                                 // the next chunk overwrites Xs / Wp / Ap
  }

  if (mma) tail_epilogue<TW, NBW>(a, acc, b, ty0, tx0, rb, jb0, r, h);
}

template <int STRIDE, int NCB>
int launch(const DwPwArgs& a, hipStream_t st) {
  constexpr int TH = 8, TW = STRIDE == 1 ? 16 : 8, MT = TH * TW;
  constexpr int HP = ((TH - 1) * STRIDE + 3) * ((TW - 1) * STRIDE + 3);
  constexpr size_t lds = (size_t)HP * XLD * 4 + (size_t)3 * MT * KC * 2 + (size_t)3 * NCB * 32 * KC * 2;
  static_assert(lds <= 160 * 1024, "the staged tiles must fit the LDS of one CU");
  static std::atomic<uint64_t> lds_raised{0};
  const hipError_t e = kd_raise_dynamic_lds((const void*)dw_pw_infer_kernel<STRIDE, NCB>, lds, lds_raised);
  KD_REQUIRE(e == hipSuccess, (int)e, "kd_dw_pw_infer: cannot raise the dynamic LDS limit to %zu B: %s", lds, hipGetErrorString(e));
  const int64_t grid = (int64_t)a.B * a.tiles_y * a.tiles_x;
  hipLaunchKernelGGL((dw_pw_infer_kernel<STRIDE, NCB>), dim3((unsigned)grid), dim3(NTHR), lds, st, a);
  return kd_check_launch("kd_dw_pw_infer");
}

// ---- the whole InvertedResidual: expand 1x1 + BN + act -> depthwise 3x3 + BN + act -> project 1x1 + BN + act (+ residual) -----------
// Same tile ownership and chunk walk as dw_pw_infer_kernel, but the chunk's activated hidden halo tile is COMPUTED, not loaded:
//   * the block-input halo tile (HP pixels x Cin, clamped coordinates) is read from HBM once per tile, cut into its three bf16
//     planes and kept in REGISTERS as MFMA A fragments for the whole chunk loop: wave w owns the 32-row blocks w, w + 4, ... of
//     the halo tile (lane (r, h) holds row r, k = 16 u + 8 h .. + 7 of k-step u, the operand layout of pw_stream_kernel).  LDS
//     stays at the footprint of dw_pw_infer_kernel plus one expand-weight chunk, so two workgroups still share a CU;
//   * per chunk the [32 hidden x Cin] slice of the expand weight is cut into its planes (LDS, rows XOR-swizzled) and
//     hidden_raw[halo px x 32] = X . We^T runs on v_mfma_f32_32x32x16_bf16: K ascending in 16-wide steps, the six piece products
//     of pw_gemm_kernel<.., SPLIT> / pw_stream_kernel in their order, fp32 accumulate from zero -- the bits of kd_pwconv_gemm;
//   * the accumulators get the bias, the expand BatchNorm + activation (kd_affine_act4, as the deferred-input load of
//     dw_pw_infer_kernel), zero outside the image, and go to Xs as fp32.
// The chunk loop is two phases with one barrier each: [matrix] project MFMAs of chunk c - 1 and expand MFMAs of chunk c (no
// dependence between them), [vector] depthwise of chunk c, staging of the project-weight chunk c and the expand-weight chunk c + 1.
struct BlockArgs {
  DwPwArgs d;                                                       // d.x: block input [B,H,W,Cin]; d.isc / d.ish / d.iact: the expand BatchNorm + activation
  const float* we; const float* ebias;                              // expand weight [Ch][Cin], bias [Ch] or null
};

// bf16 offset of 16-byte chunk `chunk` of expand-weight row n (CIN bf16 per row): conflict-free ds_read_b128 (sw_key of pw_stream_kernel)
template <int CIN>
__device__ __forceinline__ int we_off(int n, int chunk) {
  static_assert(CIN == 32 || CIN == 64, "expand-weight rows of 64 or 128 bytes");
  return (chunk ^ (CIN == 32 ? (n >> 2) & 3 : (n >> 1) & 7)) * 8;
}

template <int STRIDE, int CKB, int NCB>                              // CKB = Cin / 32, NCB = Cout / 32
__global__ __launch_bounds__(NTHR, 2) void block_infer_kernel(BlockArgs g) {
  constexpr int TH = 8, TW = STRIDE == 1 ? 16 : 8, MT = TH * TW, NRB = MT / 32;
  constexpr int HT = (TH - 1) * STRIDE + 3, WT = (TW - 1) * STRIDE + 3, HP = HT * WT;
  constexpr int CIN = 32 * CKB, COUT = 32 * NCB;
  constexpr int NJG = (NTHR / 64) / NRB;
  constexpr int NBW = NCB >= NJG ? NCB / NJG : 1;
  constexpr int NXB = (HP + 31) / 32, XBW = (NXB + 3) / 4;           // 32-row blocks of the halo tile; blocks per wave
  constexpr int NKS = CIN / 16;                                      // k-steps of the expand GEMM
  const DwPwArgs& a = g.d;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float* Xs = reinterpret_cast<float*>(smem_raw);                                          // [32 NXB][XLD] activated hidden tile, fp32 (rows >= HP: padding)
  unsigned short* Ap = reinterpret_cast<unsigned short*>(smem_raw + (size_t)NXB * 32 * XLD * 4); // [3][MT][KC]
  unsigned short* Wp = Ap + 3 * MT * KC;                                                   // [3][COUT][KC]
  unsigned short* We = Wp + 3 * COUT * KC;                                                 // [3][KC][CIN] planes of the expand-weight chunk
  float* Ts = reinterpret_cast<float*>(We + 3 * KC * CIN);                                 // [2][TSN] depthwise taps [32][9], scale [32], shift [32] of a chunk
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;

  int t = blockIdx.x;
  const int tx0 = (t % a.tiles_x) * TW; t /= a.tiles_x;
  const int ty0 = (t % a.tiles_y) * TH;
  const int b = t / a.tiles_y;
  const int iy0 = ty0 * STRIDE - 1, ix0 = tx0 * STRIDE - 1;
  const int cq = tid & (CQN - 1);
  const int pl = tid / CQN;
  const int rb = wave % NRB;
  const int jb0 = (wave / NRB) * NBW;
  const bool mma = jb0 < NCB;
  f32x16 acc[NBW];
#pragma unroll
  for (int j = 0; j < NBW; ++j)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[j][q] = 0.f;

  // ---- per-chunk global loads (weights and coefficients only: L2-resident), issued at the start of the matrix phase ----------
  // The depthwise taps and coefficients of a chunk travel as ONE float4 per thread (threads 0..TSN/4-1) and are staged in LDS a
  // chunk ahead, double-buffered: 36 tap registers per thread would not fit beside the input fragments.
  float4 wr[NCB], wx[CKB], tp = kd_zero4();
  float ebn = 0.f, escn, eshn;                                       // bias / scale / shift of hidden channel r of the NEXT chunk
  auto issue_e = [&](int k0) {                                       // what the matrix phase of chunk k0 and the vector phase before it need
#pragma unroll
    for (int i = 0; i < CKB; ++i) wx[i] = kd_ld4(g.we + (int64_t)(k0 + pl) * CIN + 32 * i + 4 * cq);
    if (g.ebias) ebn = g.ebias[k0 + r];
    escn = a.isc[k0 + r]; eshn = a.ish[k0 + r];
    if (tid < TSN / 4) {
      const float* src = tid < 72 ? a.wd + (int64_t)k0 * 9 + 4 * tid : (tid < 80 ? a.dsc + k0 + 4 * (tid - 72) : a.dsh + k0 + 4 * (tid - 80));
      tp = kd_ld4(src);
    }
  };
  auto issue = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NCB; ++i) wr[i] = kd_ld4(a.wp + (int64_t)(pl + 32 * i) * a.Ch + k0 + 4 * cq);
    issue_e(k0 + KC < a.Ch ? k0 + KC : k0);                          // (last chunk: a valid address, staged and never read)
  };
  auto stage_ts = [&](int buf) { if (tid < TSN / 4) kd_st4(Ts + buf * TSN + 4 * tid, tp); };
  auto stage_we = [&]() {
#pragma unroll
    for (int i = 0; i < CKB; ++i) {
      const int k4 = 8 * i + cq;
      uint2 hi, mid, lo;
      kd_split3(wx[i], hi, mid, lo);
      unsigned short* d = We + pl * CIN + we_off<CIN>(pl, k4 >> 1) + (k4 & 1) * 4;
      *reinterpret_cast<uint2*>(d) = hi;
      *reinterpret_cast<uint2*>(d + KC * CIN) = mid;
      *reinterpret_cast<uint2*>(d + 2 * KC * CIN) = lo;
    }
  };

  // ---- once per tile: this wave's rows of the block-input halo tile -> bf16x3 A fragments; which of their pixels are inside the
  // image (bit q of inm: row of accumulator register q) and inside the tile (vld: rows >= HP are padding and never stored) ------
  issue_e(0);
  bf16x8 xf[XBW][NKS][3];
  unsigned inm[XBW];
  {
    float4 xr[XBW][NKS][2];
#pragma unroll
    for (int i = 0; i < XBW; ++i) {
      int hp = (wave + 4 * i) * 32 + r;
      hp = hp < HP ? hp : HP - 1;
      int iy = iy0 + hp / WT, ix = ix0 + hp % WT;
      iy = iy < 0 ? 0 : (iy >= a.H ? a.H - 1 : iy);
      ix = ix < 0 ? 0 : (ix >= a.W ? a.W - 1 : ix);
      const float* xp = a.x + (((int64_t)b * a.H + iy) * a.W + ix) * CIN + 8 * h;
#pragma unroll
      for (int u = 0; u < NKS; ++u) { xr[i][u][0] = kd_ld4(xp + 16 * u); xr[i][u][1] = kd_ld4(xp + 16 * u + 4); }
      inm[i] = 0;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int row = (wave + 4 * i) * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
        const int y = iy0 + row / WT, x = ix0 + row % WT;
        inm[i] |= ((y >= 0 && y < a.H && x >= 0 && x < a.W) ? 1u : 0u) << q;
      }
    }
    stage_we();
    stage_ts(0);
#pragma unroll
    for (int i = 0; i < XBW; ++i)
#pragma unroll
      for (int u = 0; u < NKS; ++u) {
        typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
        uint2 h0, m0, l0, h1, m1, l1;
        kd_split3(xr[i][u][0], h0, m0, l0);
        kd_split3(xr[i][u][1], h1, m1, l1);
        const u32x4 ph = {h0.x, h0.y, h1.x, h1.y}, pm = {m0.x, m0.y, m1.x, m1.y}, pq = {l0.x, l0.y, l1.x, l1.y};
        xf[i][u][0] = __builtin_bit_cast(bf16x8, ph);
        xf[i][u][1] = __builtin_bit_cast(bf16x8, pm);
        xf[i][u][2] = __builtin_bit_cast(bf16x8, pq);
      }
  }
  kd_lds_barrier();

  for (int k0 = 0;; k0 += KC) {
    // ---- matrix phase: project chunk k0 - KC (Ap, Wp), expand chunk k0 (We) -> Xs ------------------------------------------------
    const bool more = k0 < a.Ch;
    const float eb = ebn, esc = escn, esh = eshn;                     // the prefetch below overwrites them
    if (k0 > 0 && mma) project_chunk<MT, COUT, NBW>(Ap, Wp, acc, rb, jb0, r, h);
    if (!more) break;
    issue(k0);                                                        // flies during the expand MFMAs (after the project fragments: registers)
    const float4 eb4 = make_float4(eb, eb, eb, eb), esc4 = make_float4(esc, esc, esc, esc), esh4 = make_float4(esh, esh, esh, esh);
#pragma unroll
    for (int i = 0; i < XBW; ++i) {
      if (wave + 4 * i < NXB) {                                       // wave-uniform
        f32x16 e;
#pragma unroll
        for (int q = 0; q < 16; ++q) e[q] = 0.f;
#pragma unroll
        for (int u = 0; u < NKS; ++u) {
          bf16x8 fb[3];
#pragma unroll
          for (int p = 0; p < 3; ++p) fb[p] = *reinterpret_cast<const bf16x8*>(We + (p * KC + r) * CIN + we_off<CIN>(r, 2 * u + h));
#pragma unroll
          for (int tt = 0; tt < 6; ++tt) e = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xf[i][u][PA[tt]], fb[PB[tt]], e, 0, 0, 0);
        }
        float* xd = Xs + ((wave + 4 * i) * 32 + 4 * h) * XLD + r;
#pragma unroll
        for (int qg = 0; qg < 4; ++qg) {
          float4 v = make_float4(e[4 * qg] + eb4.x, e[4 * qg + 1] + eb4.y, e[4 * qg + 2] + eb4.z, e[4 * qg + 3] + eb4.w);
          v = kd_affine_act4(v, esc4, esh4, a.iact);
          const float o[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) {
            const int q = 4 * qg + qq;
            xd[((q & 3) + 8 * (q >> 2)) * XLD] = ((inm[i] >> q) & 1u) ? o[qq] : 0.f;
          }
        }
      }
    }
    kd_lds_barrier();

    // ---- vector phase: depthwise of chunk k0 (Xs -> Ap), project-weight chunk k0 -> Wp, expand-weight chunk and taps k0 + KC ----
    const int cb = (k0 / KC) & 1;
    stage_wp<NCB>(Wp, wr, pl, cq);                                    // (first: their registers are free before the depthwise temporaries)
    stage_we();
    stage_ts(cb ^ 1);
    {
      const float* tq = Ts + cb * TSN;
      float4 wt[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) wt[i] = kd_ld4(tq + 36 * cq + 4 * i);
      float w9[4][9];
      taps_of(wt, w9);
      dw_phase<STRIDE>(Xs, Ap, w9, kd_ld4(tq + 288 + 4 * cq), kd_ld4(tq + 320 + 4 * cq), a.dact, pl, cq);
    }
    kd_lds_barrier();
  }

  if (mma) tail_epilogue<TW, NBW>(a, acc, b, ty0, tx0, rb, jb0, r, h);
}

template <int STRIDE, int CKB, int NCB>
int launch_block(const BlockArgs& g, hipStream_t st) {
  constexpr int TH = 8, TW = STRIDE == 1 ? 16 : 8, MT = TH * TW;
  constexpr int HP = ((TH - 1) * STRIDE + 3) * ((TW - 1) * STRIDE + 3);
  constexpr size_t lds = (size_t)((HP + 31) / 32 * 32) * XLD * 4 + (size_t)3 * MT * KC * 2 + (size_t)3 * NCB * 32 * KC * 2 +
                         (size_t)3 * KC * CKB * 32 * 2 + (size_t)2 * TSN * 4;
  static_assert(2 * lds <= 160 * 1024, "two workgroups share the LDS of one CU");
  static std::atomic<uint64_t> lds_raised{0};
  const hipError_t e = kd_raise_dynamic_lds((const void*)block_infer_kernel<STRIDE, CKB, NCB>, lds, lds_raised);
  KD_REQUIRE(e == hipSuccess, (int)e, "kd_block_infer: cannot raise the dynamic LDS limit to %zu B: %s", lds, hipGetErrorString(e));
  const int64_t grid = (int64_t)g.d.B * g.d.tiles_y * g.d.tiles_x;
  hipLaunchKernelGGL((block_infer_kernel<STRIDE, CKB, NCB>), dim3((unsigned)grid), dim3(NTHR), lds, st, g);
  return kd_check_launch("kd_block_infer");
}

}  // namespace

extern "C" {

// 1 if kd_dw_pw_infer has an instance for this shape
int kd_dw_pw_infer_supported(int Ch, int Cout, int stride) {
  if (Ch < 32 || Ch % 32 != 0) return 0;               // hidden channels are walked in chunks of 32
  // (the 128-output-column instances needed 48-52 bytes of scratch per lane and lost to the two separate kernels on every shape they
  // covered -- profiles/r02_dw_pw_fusion.txt: not built since round 3)
  if (stride == 1) return Cout == 32 || Cout == 64;
  if (stride == 2) return Cout == 64;
  return 0;
}

// out[B*Ho*Wo, Cout] = pact(bn_p(conv1x1(dact(bn_d(dwconv3x3_stride(iact(bn_i(x)))))))) (+ res), all BatchNorms as eval-mode
// affine (scale, shift) pairs; split bf16x3 GEMM arithmetic.  isc == NULL: x is used as it is.  See the file header.
int kd_dw_pw_infer(const float* x, const float* isc, const float* ish, int iact, const float* wd, const float* dsc, const float* dsh,
                   int dact, const float* wp, const float* pbias, const float* psc, const float* psh, int pact, const float* res,
                   int64_t ldres, float* out, int64_t ldo, int B, int H, int W, int Ch, int stride, int Cout, void* stream) {
  KD_REQUIRE(x && wd && dsc && dsh && wp && psc && psh && out && B > 0 && H > 0 && W > 0, KD_ERR_ARG, "kd_dw_pw_infer: bad args");
  KD_REQUIRE(!isc || ish, KD_ERR_ARG, "kd_dw_pw_infer: isc needs ish");
  KD_REQUIRE(kd_dw_pw_infer_supported(Ch, Cout, stride), KD_ERR_SHAPE, "kd_dw_pw_infer: no instance for Ch=%d Cout=%d stride=%d", Ch, Cout, stride);
  KD_REQUIRE(ldo >= Cout && (!res || ldres >= Cout), KD_ERR_SHAPE, "kd_dw_pw_infer: row strides smaller than Cout");
  KD_REQUIRE(kd_aligned16(x) && kd_aligned16(wd) && kd_aligned16(wp) && kd_aligned16(dsc) && kd_aligned16(dsh) && kd_aligned16(isc) &&
             kd_aligned16(ish), KD_ERR_ALIGN, "kd_dw_pw_infer: 16-byte alignment");
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  KD_REQUIRE((int64_t)B * Ho * Wo < ((int64_t)1 << 31), KD_ERR_SHAPE, "kd_dw_pw_infer: too many output pixels");
  const int TH = 8, TW = stride == 1 ? 16 : 8;
  DwPwArgs a{x, isc, ish, iact, wd, dsc, dsh, dact, wp, pbias, psc, psh, pact, res, ldres, out, ldo, B, H, W, Ch, Ho, Wo,
             (Wo + TW - 1) / TW, (Ho + TH - 1) / TH};
  hipStream_t st = (hipStream_t)stream;
  if (stride == 1) {
    if (Cout == 32) return launch<1, 1>(a, st);
    return launch<1, 2>(a, st);
  }
  return launch<2, 2>(a, st);
}

// 1 if kd_block_infer has an instance for this shape
int kd_block_infer_supported(int Cin, int Ch, int Cout, int stride) {
  if (Ch < 32 || Ch % 32 != 0) return 0;               // hidden channels are walked in chunks of 32
  if (stride == 1) return Cin == 64 && Cout == 64;
  if (stride == 2) return Cin == 32 && Cout == 64;
  return 0;
}

// out[B*Ho*Wo, Cout] = pact(bn_p(conv1x1(dact(bn_d(dwconv3x3_stride(eact(bn_e(conv1x1(x) + ebias))))))) + pbias)) (+ res): a whole
// InvertedResidual in eval mode, the hidden tensor never written.  x: dense [B,H,W,Cin], finished values.  See block_infer_kernel.
int kd_block_infer(const float* x, const float* we, const float* ebias, const float* esc, const float* esh, int eact, const float* wd,
                   const float* dsc, const float* dsh, int dact, const float* wp, const float* pbias, const float* psc, const float* psh,
                   int pact, const float* res, int64_t ldres, float* out, int64_t ldo, int B, int H, int W, int Cin, int Ch, int stride,
                   int Cout, void* stream) {
  KD_REQUIRE(x && we && esc && esh && wd && dsc && dsh && wp && psc && psh && out && B > 0 && H > 0 && W > 0, KD_ERR_ARG,
             "kd_block_infer: bad args");
  KD_REQUIRE(kd_block_infer_supported(Cin, Ch, Cout, stride), KD_ERR_SHAPE, "kd_block_infer: no instance for Cin=%d Ch=%d Cout=%d stride=%d",
             Cin, Ch, Cout, stride);
  KD_REQUIRE(ldo >= Cout && (!res || ldres >= Cout), KD_ERR_SHAPE, "kd_block_infer: row strides smaller than Cout");
  KD_REQUIRE(kd_aligned16(x) && kd_aligned16(we) && kd_aligned16(wd) && kd_aligned16(wp) && kd_aligned16(dsc) && kd_aligned16(dsh),
             KD_ERR_ALIGN, "kd_block_infer: 16-byte alignment");
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  KD_REQUIRE((int64_t)B * Ho * Wo < ((int64_t)1 << 31), KD_ERR_SHAPE, "kd_block_infer: too many output pixels");
  const int TH = 8, TW = stride == 1 ? 16 : 8;
  BlockArgs g{{x, esc, esh, eact, wd, dsc, dsh, dact, wp, pbias, psc, psh, pact, res, ldres, out, ldo, B, H, W, Ch, Ho, Wo,
               (Wo + TW - 1) / TW, (Ho + TH - 1) / TH}, we, ebias};
  hipStream_t st = (hipStream_t)stream;
  if (stride == 1) return launch_block<1, 2, 2>(g, st);
  return launch_block<2, 1, 2>(g, st);
}

}  // extern "C"
