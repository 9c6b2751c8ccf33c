// kd_input.hip -- per-frame input preparation on the device (reference: src/data_loading/pandaset_dataset.py).
//   * remap_semantic (:13-20) + rasterize_bev (:23-45): raw PandaSet class ids -> {0,1}, then a BEV mask where
//     each cell takes the label of the FIRST point (input order) whose label is non-zero.  The reference walks
//     the points in a Python loop; here every labelled point does an atomicMin of its in-frame index on its
//     cell and a second kernel reads the winner's label: order-independent, bit-exact, one pass over the points.
//   * the voting rasteriser for class maps (no reference counterpart): majority or priority per cell from per-(cell, class)
//     integer counters, and the class histogram of a label mask
//   * point stacking + zero padding / subsample gather (:113-127)
//   * uint8 HWC image -> float32 CHW / 255 (:108-111)
//   * the same two for a whole ragged batch in one launch each; a frame longer than max_points is cut to a uniform
//     subset ON THE DEVICE: a counter-based key per point index (Philox-4x32-10), radix-select of the max_points-th
//     smallest (key, index) pair over an LDS histogram, ordered compaction of the kept rows -- no permutation of the
//     sweep, no sort, nothing stored per point.
// All HBM-bound byte/integer work: coalesced streams; LDS only for the select's histogram and block scans.
#include "kd_common.h"

namespace {

constexpr int32_t kEmpty = 0x7f7f7f7f;          // hipMemsetAsync(0x7f) sentinel: "no labelled point yet"

__device__ __forceinline__ int64_t label_of(int64_t id, int remap, uint64_t bits) {
  if (!remap) return id;
  return (id >= 0 && id < 64) ? (int64_t)((bits >> id) & 1ull) : 0;
}

// numpy float32 order of operations, no contraction, IEEE division: ((v - lo) / span * (n - 1)) -> trunc -> clip
__device__ __forceinline__ int axis_cell(float v, float lo, float span, int n) {
  const float t = __fmul_rn(__fdiv_rn(__fsub_rn(v, lo), span), (float)(n - 1));
  int c = (int)t;
  c = c < 0 ? 0 : c;
  return c > n - 1 ? n - 1 : c;
}

__device__ __forceinline__ int frame_of(const int64_t* __restrict__ off, int B, int64_t i) {
  int lo = 0, hi = B;                             // largest b with off[b] <= i
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

struct RastArgs {
  const float* x; const float* y; const int64_t* cls; const int64_t* off; int B; int64_t n;
  uint64_t bits; int remap; int H, W; float x0, xs, x1, y0, ys, y1; int32_t* first; int64_t* mask;
};

__global__ __launch_bounds__(256) void raster_claim_kernel(RastArgs a) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * 256) {
    const float x = a.x[i], y = a.y[i];
    const bool keep = x >= a.x0 && x <= a.x1 && y >= a.y0 && y <= a.y1;      // NaN fails every comparison
    if (!keep || label_of(a.cls[i], a.remap, a.bits) == 0) continue;
    const int b = frame_of(a.off, a.B, i);
    const int cell = axis_cell(y, a.y0, a.ys, a.H) * a.W + axis_cell(x, a.x0, a.xs, a.W);
    atomicMin(a.first + (int64_t)b * a.H * a.W + cell, (int32_t)(i - a.off[b]));
  }
}

__global__ __launch_bounds__(256) void raster_resolve_kernel(RastArgs a) {
  const int64_t ncell = (int64_t)a.B * a.H * a.W;
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < ncell; k += (int64_t)gridDim.x * 256) {
    const int32_t f = a.first[k];
    const int b = (int)(k / ((int64_t)a.H * a.W));
    a.mask[k] = f == kEmpty ? 0 : label_of(a.cls[a.off[b] + f], a.remap, a.bits);
  }
}

// ---- voting rasteriser: majority / priority per cell ---------------------------------------------------------------
// Count pass: every point that passes the range test and has a class in 1 .. NC-1 adds to the uint32 counter
// ws[(b * H * W + cell) * K + class], K = the class bucket 4 / 8 / 16 that holds NC, so a cell's counters are one aligned
// 16 / 32 / 64 byte group.  Real sweeps put thousands of consecutive points into the cells round the sensor: a run of
// consecutive lanes with the same counter is merged, its first lane adds the run length (one atomic per run).  The slot
// carries frame, cell and class, so a run ends at a frame boundary; a point that counts nowhere has no slot and ends it too.
// Against one atomic per point (profiles/label_rule_ab.txt): the same time on a uniform scene, 13 times faster on a concentrated
// scene in scan order.
// Resolve pass: one thread per cell reads its K counters with 16-byte loads and picks the winner.  Integer atomics only:
// the counters, and so every output bit, do not depend on the execution order.
struct VoteArgs {
  const float* x; const float* y; const int64_t* cls; const int64_t* off; int B; int64_t n;
  int NC, rule, min_points, H, W; float x0, xs, x1, y0, ys, y1;
  const int32_t* rank; uint32_t* cnt; int64_t* mask; int32_t* votes;
};

constexpr int kRuleMajority = 1, kRulePriority = 2;

template <int K>
__global__ __launch_bounds__(256) void vote_count_kernel(VoteArgs a) {
  const int lane = threadIdx.x & 63;
  // the trip count is the same for the whole block: the shuffle and the ballot below run with all 64 lanes
  for (int64_t base = (int64_t)blockIdx.x * 256; base < a.n; base += (int64_t)gridDim.x * 256) {
    const int64_t i = base + threadIdx.x;
    int slot = -1;                                // no counter: out of range, class 0 / negative / >= NC, or past the end
    if (i < a.n) {
      const float x = a.x[i], y = a.y[i];
      const int64_t c = a.cls[i];
      const bool keep = x >= a.x0 && x <= a.x1 && y >= a.y0 && y <= a.y1;    // NaN fails every comparison
      if (keep && c >= 1 && c < a.NC) {
        const int b = frame_of(a.off, a.B, i);
        const int cell = axis_cell(y, a.y0, a.ys, a.H) * a.W + axis_cell(x, a.x0, a.xs, a.W);
        slot = (b * a.H * a.W + cell) * K + (int)c;                          // the host checked B * H * W * K < 2^31
      }
    }
    const int prev = __shfl_up(slot, 1, 64);
    const bool starts = lane == 0 || prev != slot;
    const unsigned long long heads = __ballot(starts);
    if (starts && slot >= 0) {
      const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
      const unsigned int len = above ? (unsigned int)__ffsll((long long)above) : (unsigned int)(64 - lane);
      atomicAdd(a.cnt + slot, len);
    }
  }
}

template <int K>
__global__ __launch_bounds__(256) void vote_resolve_kernel(VoteArgs a) {
  int rk[K];
#pragma unroll
  for (int c = 0; c < K; ++c) rk[c] = (a.rank && c >= 1 && c < a.NC) ? a.rank[c] : 0;
  const int64_t ncell = (int64_t)a.B * a.H * a.W;
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < ncell; k += (int64_t)gridDim.x * 256) {
    uint32_t n[K];
    const uint4* src = reinterpret_cast<const uint4*>(a.cnt + k * K);
#pragma unroll
    for (int q = 0; q < K / 4; ++q) {
      const uint4 v = src[q];
      n[4 * q] = v.x; n[4 * q + 1] = v.y; n[4 * q + 2] = v.z; n[4 * q + 3] = v.w;
    }
    int best = 0, brk = 0;
    uint32_t bn = 0;
#pragma unroll
    for (int c = 1; c < K; ++c) {                 // ascending: on a full tie the smaller class stays
      const bool eligible = c < a.NC && n[c] >= (uint32_t)a.min_points;
      const bool better = a.rule == kRuleMajority ? (n[c] > bn || (n[c] == bn && rk[c] > brk))
                                                  : (rk[c] > brk || (rk[c] == brk && n[c] > bn));
      if (eligible && (best == 0 || better)) { best = c; bn = n[c]; brk = rk[c]; }
    }
    a.mask[k] = best;
    if (a.votes) a.votes[k] = (int32_t)bn;
  }
}

// counts[c] += #{mask == c} for 0 <= c < NC, counts[NC] += every other value: 17 LDS counters per block, one 64-bit atomic per
// non-zero counter (the pattern of confusion16_kernel in kd_loss.hip)
__global__ __launch_bounds__(256) void label_histogram_kernel(const int64_t* __restrict__ mask, int64_t n, int NC,
                                                              unsigned long long* counts) {
  __shared__ unsigned int loc[17];
  if (threadIdx.x < 17) loc[threadIdx.x] = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t v = mask[i];
    atomicAdd(&loc[(v >= 0 && v < NC) ? (int)v : NC], 1u);
  }
  __syncthreads();
  if (threadIdx.x <= NC && loc[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)loc[threadIdx.x]);
}

__global__ __launch_bounds__(256) void remap_kernel(const int64_t* __restrict__ raw, int64_t n, uint64_t bits,
                                                    int64_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    out[i] = label_of(raw[i], 1, bits);
}

// out = table[raw], ids outside 0 .. ntab-1 -> 0 (background)
__global__ __launch_bounds__(256) void remap_table_kernel(const int64_t* __restrict__ raw, int64_t n,
                                                          const int64_t* __restrict__ table, int ntab,
                                                          int64_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t id = raw[i];
    out[i] = (id >= 0 && id < ntab) ? table[id] : 0;
  }
}

__global__ __launch_bounds__(256) void points_prepare_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                             const float* __restrict__ z, const float* __restrict__ w,
                                                             const int64_t* __restrict__ choice, int64_t n_take,
                                                             int64_t max_points, float* __restrict__ out) {
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < max_points; j += (int64_t)gridDim.x * 256) {
    float4 v = kd_zero4();
    if (j < n_take) {
      const int64_t s = choice ? choice[j] : j;
      v = make_float4(x[s], y[s], z[s], w[s]);
    }
    kd_st4(out + j * 4, v);
  }
}

__global__ __launch_bounds__(256) void image_chw_kernel(const uint8_t* __restrict__ in, float* __restrict__ out, int HW) {
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
    const uint8_t* s = in + (int64_t)p * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[(int64_t)c * HW + p] = __fdiv_rn((float)s[c], 255.f);
  }
}

// ---- batched forms ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void image_chw_batch_kernel(const uint8_t* __restrict__ in, float* __restrict__ out,
                                                              int64_t HW, int64_t total) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < total; p += (int64_t)gridDim.x * 256) {
    const int64_t b = p / HW, q = p - b * HW;
    const uint8_t* s = in + p * 3;
    float* d = out + b * 3 * HW + q;
#pragma unroll
    for (int c = 0; c < 3; ++c) d[(int64_t)c * HW] = __fdiv_rn((float)s[c], 255.f);
  }
}

// Philox-4x32-10 (Salmon et al., SC'11), word 0 of the output block
__device__ __forceinline__ uint32_t philox_word0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return c0;
}

constexpr int kSelThreads = 1024;                // one workgroup per frame
constexpr int kSelWaves = kSelThreads / 64;
constexpr int kSelItems = 4;                     // consecutive point indices per thread and compaction chunk

struct SelShared {
  uint32_t hist[256];
  uint32_t wave_tot[kSelWaves];
  uint32_t prefix, remaining;
};

// exclusive prefix sum of `v` over the workgroup in thread order (+ the workgroup total); all threads must call it
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* wave_tot, uint32_t& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __syncthreads();                               // the previous call's readers are done with wave_tot
  if (lane == 63) wave_tot[wave] = inc;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kSelWaves; ++w) {
    const uint32_t t = wave_tot[w];
    before += w < wave ? t : 0u;
    all += t;
  }
  total = all;
  return before + inc - v;
}

__global__ __launch_bounds__(kSelThreads) void points_prepare_batch_kernel(
    const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, const float* __restrict__ w,
    const int64_t* __restrict__ off, const uint64_t* __restrict__ frame_key, uint64_t seed, int64_t max_points,
    float* __restrict__ out) {
  __shared__ SelShared sh;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t base = off[b];
  const int64_t n = off[b + 1] - base;
  x += base; y += base; z += base; w += base;
  out += (int64_t)b * max_points * 4;
  if (n <= max_points) {                         // stack + zero padding: the bits of kd_points_prepare(choice = NULL)
    for (int64_t j = tid; j < max_points; j += kSelThreads)
      kd_st4(out + j * 4, j < n ? make_float4(x[j], y[j], z[j], w[j]) : kd_zero4());
    return;
  }
  const uint64_t fk = frame_key[b];
  const uint32_t c2 = (uint32_t)fk, c3 = (uint32_t)(fk >> 32), k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const uint32_t nn = (uint32_t)n;               // the host checked n_total < 2^31

  // radix select, most significant byte first: after the four passes `prefix` is the key T of the max_points-th
  // smallest (key, index) pair and `remaining` how many points with key == T are kept (those of lowest index)
  uint32_t prefix = 0, remaining = (uint32_t)max_points;
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 256) sh.hist[tid] = 0;
    __syncthreads();
    const uint32_t hi_mask = shift == 24 ? 0u : ~0u << (shift + 8);
    for (uint32_t j = tid; j < nn; j += kSelThreads) {
      const uint32_t k = philox_word0(j, 0u, c2, c3, k0, k1);
      if ((k & hi_mask) == prefix) atomicAdd(&sh.hist[(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    const uint32_t h = tid < 256 ? sh.hist[tid] : 0u;
    uint32_t total;
    const uint32_t below = block_excl_scan(h, sh.wave_tot, total);
    if (tid < 256 && below < remaining && remaining <= below + h) {          // exactly one bin
      sh.prefix = prefix | ((uint32_t)tid << shift);
      sh.remaining = remaining - below;
    }
    __syncthreads();
    prefix = sh.prefix;
    remaining = sh.remaining;
  }

  // ordered compaction over index chunks: a kept row's slot = (# keys < T before it) + min(# keys == T before it, remaining)
  uint32_t less_before = 0, tie_before = 0;
  constexpr uint32_t kChunk = kSelThreads * kSelItems;
  for (uint32_t c0 = 0; c0 < nn; c0 += kChunk) {
    const uint32_t j0 = c0 + (uint32_t)tid * kSelItems;
    uint32_t less[kSelItems], tie[kSelItems], packed = 0;                    // chunk counts <= 4096: 16 bits each
#pragma unroll
    for (int i = 0; i < kSelItems; ++i) {
      const uint32_t j = j0 + i;
      const uint32_t k = philox_word0(j, 0u, c2, c3, k0, k1);
      less[i] = (j < nn && k < prefix) ? 1u : 0u;
      tie[i] = (j < nn && k == prefix) ? 1u : 0u;
      packed += less[i] | (tie[i] << 16);
    }
    uint32_t total;
    const uint32_t ex = block_excl_scan(packed, sh.wave_tot, total);
    uint32_t nl = less_before + (ex & 0xffffu), nt = tie_before + (ex >> 16);
#pragma unroll
    for (int i = 0; i < kSelItems; ++i) {
      const uint32_t j = j0 + i;
      if (less[i] || (tie[i] && nt < remaining)) {
        const uint32_t slot = nl + (nt < remaining ? nt : remaining);
        kd_st4(out + (int64_t)slot * 4, make_float4(x[j], y[j], z[j], w[j]));
      }
      nl += less[i];
      nt += tie[i];
    }
    less_before += total & 0xffffu;
    tie_before += total >> 16;
  }
}

int grid_for(int64_t n) {
  int64_t g = (n + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

int vote_bucket(int NC) { return NC <= 4 ? 4 : (NC <= 8 ? 8 : 16); }

}  // namespace

extern "C" {

size_t kd_bev_rasterize_ws_bytes(int B, int H, int W) { return (size_t)B * H * W * sizeof(int32_t); }

int kd_bev_rasterize(const float* x, const float* y, const int64_t* cls, const int64_t* offsets, int B, int64_t n_total,
                     int remap, uint64_t remap_bits, int H, int W, float x_min, float x_span, float x_max, float y_min,
                     float y_span, float y_max, void* ws, size_t ws_bytes, int64_t* mask, void* stream) {
  KD_REQUIRE(offsets && mask && ws && B > 0 && H > 0 && W > 0 && n_total >= 0, KD_ERR_ARG, "kd_bev_rasterize: bad args");
  KD_REQUIRE(n_total == 0 || (x && y && cls), KD_ERR_ARG, "kd_bev_rasterize: null point arrays with n_total=%lld", (long long)n_total);
  KD_REQUIRE(n_total < (int64_t)kEmpty, KD_ERR_SHAPE, "kd_bev_rasterize: too many points");
  KD_REQUIRE(x_span > 0.f && y_span > 0.f, KD_ERR_ARG, "kd_bev_rasterize: empty range");
  KD_REQUIRE(ws_bytes >= kd_bev_rasterize_ws_bytes(B, H, W), KD_ERR_WORKSPACE, "kd_bev_rasterize: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(ws, 0x7f, kd_bev_rasterize_ws_bytes(B, H, W), st);
  KD_REQUIRE(e == hipSuccess, (int)e, "kd_bev_rasterize: memset failed");
  RastArgs a{x, y, cls, offsets, B, n_total, remap_bits, remap, H, W, x_min, x_span, x_max, y_min, y_span, y_max,
             (int32_t*)ws, mask};
  if (n_total > 0) hipLaunchKernelGGL(raster_claim_kernel, dim3(grid_for(n_total)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(raster_resolve_kernel, dim3(grid_for((int64_t)B * H * W)), dim3(256), 0, st, a);
  return kd_check_launch("kd_bev_rasterize");
}

size_t kd_bev_rasterize_vote_ws_bytes(int B, int H, int W, int NC) {
  if (B <= 0 || H <= 0 || W <= 0 || NC < 2 || NC > 16) return 0;
  return (size_t)B * H * W * vote_bucket(NC) * sizeof(uint32_t);
}

// The majority / priority rule per cell (include/kd_hip.h carries the specification): memset of the counters, count pass, resolve.
int kd_bev_rasterize_vote(const float* x, const float* y, const int64_t* cls, const int64_t* offsets, int B, int64_t n_total,
                          int NC, int rule, const int32_t* rank, int min_points, int H, int W, float x_min, float x_span,
                          float x_max, float y_min, float y_span, float y_max, void* ws, size_t ws_bytes, int64_t* mask,
                          int32_t* votes, void* stream) {
  KD_REQUIRE(NC >= 2 && NC <= 16, KD_ERR_SHAPE, "kd_bev_rasterize_vote: num_classes=%d unsupported (2..16)", NC);
  KD_REQUIRE(rule == kRuleMajority || rule == kRulePriority, KD_ERR_ARG,
             "kd_bev_rasterize_vote: rule=%d is neither 1 (majority) nor 2 (priority); the first-point rule is kd_bev_rasterize", rule);
  KD_REQUIRE(min_points >= 1, KD_ERR_ARG, "kd_bev_rasterize_vote: min_points=%d must be at least 1", min_points);
  KD_REQUIRE(offsets && mask && ws && B > 0 && H > 0 && W > 0 && n_total >= 0, KD_ERR_ARG, "kd_bev_rasterize_vote: bad args");
  KD_REQUIRE(n_total == 0 || (x && y && cls), KD_ERR_ARG, "kd_bev_rasterize_vote: null point arrays with n_total=%lld", (long long)n_total);
  KD_REQUIRE(n_total < (int64_t)1 << 31, KD_ERR_SHAPE, "kd_bev_rasterize_vote: too many points");          // uint32 counters
  const int K = vote_bucket(NC);
  KD_REQUIRE((int64_t)B * H * W * K < (int64_t)1 << 31, KD_ERR_SHAPE, "kd_bev_rasterize_vote: B * H * W * %d counters exceed 2^31", K);
  KD_REQUIRE(x_span > 0.f && y_span > 0.f, KD_ERR_ARG, "kd_bev_rasterize_vote: empty range");
  KD_REQUIRE(kd_aligned16(ws), KD_ERR_ALIGN, "kd_bev_rasterize_vote: the workspace must be 16-byte aligned");
  const size_t need = kd_bev_rasterize_vote_ws_bytes(B, H, W, NC);
  KD_REQUIRE(ws_bytes >= need, KD_ERR_WORKSPACE, "kd_bev_rasterize_vote: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(ws, 0, need, st);
  KD_REQUIRE(e == hipSuccess, (int)e, "kd_bev_rasterize_vote: memset failed");
  VoteArgs a{x, y, cls, offsets, B, n_total, NC, rule, min_points, H, W, x_min, x_span, x_max, y_min, y_span, y_max,
             rank, (uint32_t*)ws, mask, votes};
  const dim3 gc(grid_for(n_total)), gr(grid_for((int64_t)B * H * W)), blk(256);
  if (K == 4) {
    if (n_total > 0) hipLaunchKernelGGL(vote_count_kernel<4>, gc, blk, 0, st, a);
    hipLaunchKernelGGL(vote_resolve_kernel<4>, gr, blk, 0, st, a);
  } else if (K == 8) {
    if (n_total > 0) hipLaunchKernelGGL(vote_count_kernel<8>, gc, blk, 0, st, a);
    hipLaunchKernelGGL(vote_resolve_kernel<8>, gr, blk, 0, st, a);
  } else {
    if (n_total > 0) hipLaunchKernelGGL(vote_count_kernel<16>, gc, blk, 0, st, a);
    hipLaunchKernelGGL(vote_resolve_kernel<16>, gr, blk, 0, st, a);
  }
  return kd_check_launch("kd_bev_rasterize_vote");
}

// counts[NC + 1] (int64, ACCUMULATED into): the class histogram of a label mask; values outside 0 .. NC-1 (the ignore index) -> counts[NC]
int kd_label_histogram(const int64_t* mask, int64_t n, int NC, int64_t* counts, void* stream) {
  KD_REQUIRE(NC >= 1 && NC <= 16, KD_ERR_SHAPE, "kd_label_histogram: num_classes=%d unsupported (1..16)", NC);
  KD_REQUIRE(counts && n >= 0 && (n == 0 || mask), KD_ERR_ARG, "kd_label_histogram: bad args");
  KD_REQUIRE(n < (int64_t)1 << 40, KD_ERR_SHAPE, "kd_label_histogram: too many labels");                  // uint32 counters per block
  if (n == 0) return KD_OK;
  int64_t grid = (n + 255) / 256;
  if (grid > 1024) grid = 1024;
  hipLaunchKernelGGL(label_histogram_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, mask, n, NC,
                     (unsigned long long*)counts);
  return kd_check_launch("kd_label_histogram");
}

int kd_semantic_remap(const int64_t* raw, int64_t n, uint64_t remap_bits, int64_t* out, void* stream) {
  KD_REQUIRE(n >= 0 && (n == 0 || (raw && out)), KD_ERR_ARG, "kd_semantic_remap: bad args");
  if (n == 0) return KD_OK;
  hipLaunchKernelGGL(remap_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, raw, n, remap_bits, out);
  return kd_check_launch("kd_semantic_remap");
}

// The multi-class form of kd_semantic_remap: out[i] = table[raw[i]] for 0 <= raw[i] < ntab, else 0 (raw and out: two buffers).
int kd_semantic_remap_table(const int64_t* raw, int64_t n, const int64_t* table, int ntab, int64_t* out, void* stream) {
  KD_REQUIRE(n >= 0 && (n == 0 || (raw && out)) && table && ntab >= 1, KD_ERR_ARG, "kd_semantic_remap_table: bad args");
  if (n == 0) return KD_OK;
  hipLaunchKernelGGL(remap_table_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, raw, n, table, ntab, out);
  return kd_check_launch("kd_semantic_remap_table");
}

int kd_points_prepare(const float* x, const float* y, const float* z, const float* intensity, const int64_t* choice,
                      int64_t n, int64_t max_points, float* out, void* stream) {
  KD_REQUIRE(out && max_points > 0 && n >= 0, KD_ERR_ARG, "kd_points_prepare: bad args");
  KD_REQUIRE(n == 0 || (x && y && z && intensity), KD_ERR_ARG, "kd_points_prepare: null coordinate arrays");
  KD_REQUIRE(kd_aligned16(out), KD_ERR_ALIGN, "kd_points_prepare: out must be 16-byte aligned");
  KD_REQUIRE(!choice || n >= max_points, KD_ERR_ARG, "kd_points_prepare: a subsample needs n >= max_points");
  const int64_t take = choice ? max_points : (n < max_points ? n : max_points);
  hipLaunchKernelGGL(points_prepare_kernel, dim3(grid_for(max_points)), dim3(256), 0, (hipStream_t)stream, x, y, z,
                     intensity, choice, take, max_points, out);
  return kd_check_launch("kd_points_prepare");
}

int kd_image_u8hwc_to_f32chw(const uint8_t* in, float* out, int H, int W, void* stream) {
  KD_REQUIRE(in && out && H > 0 && W > 0, KD_ERR_ARG, "kd_image_u8hwc_to_f32chw: bad args");
  hipLaunchKernelGGL(image_chw_kernel, dim3(grid_for((int64_t)H * W)), dim3(256), 0, (hipStream_t)stream, in, out, H * W);
  return kd_check_launch("kd_image_u8hwc_to_f32chw");
}

int kd_image_u8hwc_to_f32chw_batch(const uint8_t* in, float* out, int B, int H, int W, void* stream) {
  KD_REQUIRE(in && out && B > 0 && H > 0 && W > 0, KD_ERR_ARG, "kd_image_u8hwc_to_f32chw_batch: bad args");
  const int64_t HW = (int64_t)H * W;
  hipLaunchKernelGGL(image_chw_batch_kernel, dim3(grid_for(B * HW)), dim3(256), 0, (hipStream_t)stream, in, out, HW, B * HW);
  return kd_check_launch("kd_image_u8hwc_to_f32chw_batch");
}

int kd_points_prepare_batch(const float* x, const float* y, const float* z, const float* intensity, const int64_t* offsets,
                            const uint64_t* frame_keys, int B, int64_t n_total, int64_t max_points, uint64_t seed, float* out,
                            void* stream) {
  KD_REQUIRE(offsets && frame_keys && out && B > 0 && max_points > 0 && n_total >= 0, KD_ERR_ARG, "kd_points_prepare_batch: bad args");
  KD_REQUIRE(n_total == 0 || (x && y && z && intensity), KD_ERR_ARG, "kd_points_prepare_batch: null coordinate arrays");
  KD_REQUIRE(n_total < (int64_t)1 << 31 && max_points < (int64_t)1 << 31, KD_ERR_SHAPE, "kd_points_prepare_batch: too many points");
  KD_REQUIRE(kd_aligned16(out), KD_ERR_ALIGN, "kd_points_prepare_batch: out must be 16-byte aligned");
  hipLaunchKernelGGL(points_prepare_batch_kernel, dim3(B), dim3(kSelThreads), 0, (hipStream_t)stream, x, y, z, intensity,
                     offsets, frame_keys, seed, max_points, out);
  return kd_check_launch("kd_points_prepare_batch");
}

}  // extern "C"
