// kd_resize.hip -- Pillow-exact 8-bit bilinear image resize on the device (reference: pandaset_dataset.py:105-111,
// `Image.open(jpg).convert("RGB").resize(image_size, Image.BILINEAR)` then uint8 HWC -> float32 CHW / 255).
//
// Pillow's ImagingResample for 8-bit images is integer arithmetic over two coefficient tables: per output index a first
// source index `xmin`, a tap count `n` and n coefficients k = (int)(0.5 + w * 2^22); an output sample is
// min(255, (2^21 + sum pixel[xmin + t] * k[t]) >> 22).  The horizontal pass runs first and rounds to uint8, the vertical
// pass runs over those bytes.  The host builds the tables in double (kdrt/resample.py) and uploads them once per
// (in, out) pair; the kernel does integer work only, so its bits cannot depend on device floating point.  The float
// output is __fdiv_rn((float)u8, 255.f), the bits of kd_image_u8hwc_to_f32chw_batch.
//
// Shape: one 256-thread workgroup owns a band of R (<= 8) output rows x a tile of TW (<= 256) output columns of one
// frame.  It copies the bounds and coefficients of its tile into LDS (horizontal coefficients transposed, [tap][column]:
// a wave reads consecutive dwords), then walks the source rows the band needs, G rows per round: 16-byte loads of the
// row window into an LDS staging buffer -> barrier -> horizontal resample of G x TW pixels out of the staging buffer
// into the uint8 LDS tile [rows][TW][3] -> barrier.  The vertical pass then reads the tile, a thread per output pixel,
// and writes three coalesced float rows (one per plane) and, when asked, the byte image.  The uint8 intermediate never
// reaches HBM; adjacent bands re-read about 2 * support source rows.  No scratch, no atomics, no workspace.
//
// Supported: sources up to 4096 x 4096, any upscale, downscale up to a factor of 16 per axis (at most 33 taps).
// R, TW and G are chosen on the host so that the LDS image fits 64 KiB at every supported shape
// (1080 x 1920 -> 256 x 256: R = 8, TW = 256, G = 3, 62 KiB).  Every table entry is clamped to the source and to the
// LDS windows on the device: a wrong table gives wrong pixels, never an access outside the buffers.
#include "kd_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxSrc = 4096;
constexpr int kMaxFactor = 16;
constexpr int kMaxTaps = 2 * kMaxFactor + 1;
constexpr int kMaxBand = 8;
constexpr int kMaxTile = 256;
constexpr int kMaxRound = 8;
constexpr size_t kLdsBudget = 64 * 1024;
constexpr uint32_t kHalf = 1u << 21;             // Pillow: PRECISION_BITS = 32 - 8 - 2 = 22

struct ResizeArgs {
  const uint8_t* in; const int32_t* hb; const int32_t* hk; const int32_t* vb; const int32_t* vk;
  float* outf; uint8_t* outb;
  int B, Hs, Ws, H, W, hks, vks;
  int TW, R, G, NR, SW, rowbytes;                // tile columns, band rows, source rows per round, tile rows, window columns
  int ntx, nby;
  int o_tile, o_hk, o_vk, o_hb, o_vb;            // LDS byte offsets (the staging buffer is at 0)
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// 16 source bytes at the 16-byte aligned address p; bytes outside [lo, hi) (the first / last chunk of the buffer) read as 0
__device__ __forceinline__ uint4 load_chunk(uintptr_t p, uintptr_t lo, uintptr_t hi) {
  if (p >= lo && p + 16 <= hi) return *reinterpret_cast<const uint4*>(p);
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uintptr_t q = p + i;
    const uint32_t v = (q >= lo && q < hi) ? (uint32_t)*reinterpret_cast<const uint8_t*>(q) : 0u;
    w[i >> 2] |= v << (8 * (i & 3));
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ uint32_t clip8(uint32_t acc) {
  const uint32_t v = acc >> 22;
  return v > 255u ? 255u : v;
}

__global__ __launch_bounds__(kThreads) void resize_bilinear_kernel(ResizeArgs a) {
  extern __shared__ __align__(16) uint8_t smem[];
  uint8_t* stage = smem;
  uint8_t* tile = smem + a.o_tile;
  int32_t* hkl = reinterpret_cast<int32_t*>(smem + a.o_hk);      // [hks][TW]
  int32_t* vkl = reinterpret_cast<int32_t*>(smem + a.o_vk);      // [R][vks]
  int32_t* hbl = reinterpret_cast<int32_t*>(smem + a.o_hb);      // [TW][2]: xmin, n
  int32_t* vbl = reinterpret_cast<int32_t*>(smem + a.o_vb);      // [R][2]
  const int tid = threadIdx.x;
  int blk = blockIdx.x;
  const int tx = blk % a.ntx; blk /= a.ntx;
  const int by = blk % a.nby;
  const int b = blk / a.nby;
  const int c0 = tx * a.TW, cw = min(a.TW, a.W - c0);
  const int r0 = by * a.R, rh = min(a.R, a.H - r0);
  const int TW = a.TW, pitch = a.TW * 3;

  for (int i = tid; i < cw; i += kThreads) {
    const int xmin = clampi(a.hb[2 * (c0 + i)], 0, a.Ws);
    hbl[2 * i] = xmin;
    hbl[2 * i + 1] = clampi(a.hb[2 * (c0 + i) + 1], 0, min(a.hks, a.Ws - xmin));
  }
  for (int i = tid; i < cw * a.hks; i += kThreads) {
    const int x = i / a.hks, t = i - x * a.hks;
    hkl[t * TW + x] = a.hk[(int64_t)c0 * a.hks + i];
  }
  for (int i = tid; i < rh; i += kThreads) {
    const int ymin = clampi(a.vb[2 * (r0 + i)], 0, a.Hs);
    vbl[2 * i] = ymin;
    vbl[2 * i + 1] = clampi(a.vb[2 * (r0 + i) + 1], 0, min(a.vks, a.Hs - ymin));
  }
  for (int i = tid; i < rh * a.vks; i += kThreads) vkl[i] = a.vk[(int64_t)r0 * a.vks + i];
  __syncthreads();

  // source window of this band x tile: Pillow's xmin and xmin + n are non-decreasing in the output index
  const int sx0 = hbl[0], sx1 = min(hbl[2 * (cw - 1)] + hbl[2 * (cw - 1) + 1], sx0 + a.SW);
  const int sy0 = vbl[0], sy1 = min(vbl[2 * (rh - 1)] + vbl[2 * (rh - 1) + 1], sy0 + a.NR);
  const int nrows = sy1 - sy0, wbytes = (sx1 - sx0) * 3;
  const uintptr_t lo = reinterpret_cast<uintptr_t>(a.in);
  const uintptr_t hi = lo + (uintptr_t)a.B * a.Hs * a.Ws * 3;
  const uintptr_t win = lo + (((uintptr_t)b * a.Hs + sy0) * a.Ws + sx0) * 3;     // first byte of the window
  const uintptr_t rstride = (uintptr_t)a.Ws * 3;
  const int cpr = a.rowbytes >> 4;

  for (int g0 = 0; g0 < nrows; g0 += a.G) {
    const int gc = min(a.G, nrows - g0);
    for (int i = tid; i < gc * cpr; i += kThreads) {
      const int g = i / cpr, ch = i - g * cpr;
      const uintptr_t p = win + (uintptr_t)(g0 + g) * rstride;
      const int shift = (int)(p & 15u);
      if (ch * 16 < shift + wbytes)
        *reinterpret_cast<uint4*>(stage + g * a.rowbytes + ch * 16) = load_chunk(p - shift + (uintptr_t)ch * 16, lo, hi);
    }
    __syncthreads();
    for (int i = tid; i < gc * cw; i += kThreads) {
      const int g = i / cw, x = i - g * cw;
      const int xmin = hbl[2 * x];
      int n = hbl[2 * x + 1];
      if (xmin < sx0 || xmin + n > sx1) n = 0;
      const int shift = (int)((win + (uintptr_t)(g0 + g) * rstride) & 15u);
      const uint8_t* s = stage + g * a.rowbytes + shift + (xmin - sx0) * 3;
      const int32_t* k = hkl + x;
      uint32_t a0 = kHalf, a1 = kHalf, a2 = kHalf;
      for (int t = 0; t < n; ++t) {
        const uint32_t kk = (uint32_t)k[t * TW];
        a0 += __umul24(s[3 * t], kk);
        a1 += __umul24(s[3 * t + 1], kk);
        a2 += __umul24(s[3 * t + 2], kk);
      }
      uint8_t* d = tile + (g0 + g) * pitch + x * 3;
      d[0] = (uint8_t)clip8(a0);
      d[1] = (uint8_t)clip8(a1);
      d[2] = (uint8_t)clip8(a2);
    }
    __syncthreads();
  }

  const int64_t HW = (int64_t)a.H * a.W;
  for (int i = tid; i < rh * cw; i += kThreads) {
    const int r = i / cw, x = i - r * cw;
    const int ymin = vbl[2 * r];
    int n = vbl[2 * r + 1];
    if (ymin < sy0 || ymin + n > sy1) n = 0;
    const uint8_t* s = tile + (ymin - sy0) * pitch + x * 3;
    const int32_t* k = vkl + r * a.vks;
    uint32_t a0 = kHalf, a1 = kHalf, a2 = kHalf;
    for (int t = 0; t < n; ++t) {
      const uint32_t kk = (uint32_t)k[t];
      a0 += __umul24(s[t * pitch], kk);
      a1 += __umul24(s[t * pitch + 1], kk);
      a2 += __umul24(s[t * pitch + 2], kk);
    }
    const uint32_t v0 = clip8(a0), v1 = clip8(a1), v2 = clip8(a2);
    const int64_t q = (int64_t)(r0 + r) * a.W + c0 + x;
    if (a.outf) {
      float* d = a.outf + (int64_t)b * 3 * HW + q;
      d[0] = __fdiv_rn((float)v0, 255.f);
      d[HW] = __fdiv_rn((float)v1, 255.f);
      d[2 * HW] = __fdiv_rn((float)v2, 255.f);
    }
    if (a.outb) {
      uint8_t* d = a.outb + ((int64_t)b * HW + q) * 3;
      d[0] = (uint8_t)v0;
      d[1] = (uint8_t)v1;
      d[2] = (uint8_t)v2;
    }
  }
}

// most source samples that `cnt` consecutive outputs of an `in` -> `out` axis can span: the first output's xmin is
// above center - support - 0.5, the last one's xmax at most center + support + 0.5 (+ 1 for the double arithmetic)
int span_cap(int in, int out, int cnt) {
  const double scale = (double)in / out, fs = scale < 1.0 ? 1.0 : scale;
  const int v = (int)((cnt - 1) * scale + 2.0 * fs + 1.0) + 1;
  return v < in ? v : in;
}

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// largest column tile, then band, whose LDS image fits the budget with at least one staged source row per round
bool resize_plan(int Hs, int Ws, int H, int W, int hks, int vks, ResizeArgs& a, size_t& lds) {
  for (int TW = W < kMaxTile ? W : kMaxTile; TW >= 1; TW = TW > 32 ? (TW + 1) / 2 : 0) {
    for (int R = H < kMaxBand ? H : kMaxBand; R >= 1; R /= 2) {
      const int NR = span_cap(Hs, H, R), SW = span_cap(Ws, W, TW);
      const size_t rowbytes = align16((size_t)SW * 3) + 32;              // + the 16-byte alignment shift at both ends
      const size_t s_tile = align16((size_t)NR * TW * 3), s_hk = align16((size_t)hks * TW * 4), s_vk = align16((size_t)R * vks * 4);
      const size_t s_hb = align16((size_t)TW * 8), s_vb = align16((size_t)R * 8);
      const size_t fixed = s_tile + s_hk + s_vk + s_hb + s_vb;
      if (fixed + rowbytes > kLdsBudget) continue;
      int G = (int)((kLdsBudget - fixed) / rowbytes);
      G = G > kMaxRound ? kMaxRound : G;
      G = G > NR ? NR : G;
      a.TW = TW; a.R = R; a.G = G; a.NR = NR; a.SW = SW; a.rowbytes = (int)rowbytes;
      a.o_tile = (int)(G * rowbytes);
      a.o_hk = a.o_tile + (int)s_tile;
      a.o_vk = a.o_hk + (int)s_hk;
      a.o_hb = a.o_vk + (int)s_vk;
      a.o_vb = a.o_hb + (int)s_hb;
      lds = (size_t)a.o_vb + s_vb;
      return true;
    }
  }
  return false;
}

}  // namespace

extern "C" {

int kd_image_resize_bilinear_supported(int Hs, int Ws, int H, int W) {
  return Hs >= 1 && Ws >= 1 && H >= 1 && W >= 1 && Hs <= kMaxSrc && Ws <= kMaxSrc && H <= kMaxFactor * kMaxSrc &&
         W <= kMaxFactor * kMaxSrc && (int64_t)Hs <= (int64_t)kMaxFactor * H && (int64_t)Ws <= (int64_t)kMaxFactor * W;
}

int kd_image_resize_bilinear_batch(const uint8_t* in, const int32_t* hbounds, const int32_t* hk, int hks, const int32_t* vbounds,
                                   const int32_t* vk, int vks, float* out_f32chw, uint8_t* out_u8hwc, int B, int Hs, int Ws,
                                   int H, int W, void* stream) {
  KD_REQUIRE(in && hbounds && hk && vbounds && vk && (out_f32chw || out_u8hwc) && B > 0, KD_ERR_ARG,
             "kd_image_resize_bilinear_batch: bad args");
  KD_REQUIRE(kd_image_resize_bilinear_supported(Hs, Ws, H, W), KD_ERR_SHAPE,
             "kd_image_resize_bilinear_batch: %dx%d -> %dx%d (height x width) is outside the supported range: sources up to "
             "%dx%d, downscale up to a factor of %d per axis", Hs, Ws, H, W, kMaxSrc, kMaxSrc, kMaxFactor);
  KD_REQUIRE(hks >= 1 && hks <= kMaxTaps && vks >= 1 && vks <= kMaxTaps, KD_ERR_SHAPE,
             "kd_image_resize_bilinear_batch: %d / %d taps per output, at most %d", hks, vks, kMaxTaps);
  ResizeArgs a{};
  size_t lds = 0;
  KD_REQUIRE(resize_plan(Hs, Ws, H, W, hks, vks, a, lds), KD_ERR_SHAPE, "kd_image_resize_bilinear_batch: no LDS plan for %dx%d -> %dx%d",
             Hs, Ws, H, W);
  a.in = in; a.hb = hbounds; a.hk = hk; a.vb = vbounds; a.vk = vk; a.outf = out_f32chw; a.outb = out_u8hwc;
  a.B = B; a.Hs = Hs; a.Ws = Ws; a.H = H; a.W = W; a.hks = hks; a.vks = vks;
  a.ntx = (W + a.TW - 1) / a.TW;
  a.nby = (H + a.R - 1) / a.R;
  const int64_t grid = (int64_t)B * a.ntx * a.nby;
  KD_REQUIRE(grid < (int64_t)1 << 31, KD_ERR_SHAPE, "kd_image_resize_bilinear_batch: too many tiles (%lld)", (long long)grid);
  hipLaunchKernelGGL(resize_bilinear_kernel, dim3((unsigned)grid), dim3(kThreads), lds, (hipStream_t)stream, a);
  return kd_check_launch("kd_image_resize_bilinear_batch");
}

}  // extern "C"
