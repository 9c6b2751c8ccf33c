/* kd_hip.h -- C ABI of libkd_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * camera+LiDAR knowledge-distillation training step.
 *
 * The reference (KELVIN-ASU/Lightweight-Multi-Modal-Scene-Understanding-via-Knowledge-Distillation)
 * has no native layer: its hot path is Python nn.Modules dispatching to ATen.  Each entry point
 * below therefore replaces the ATen op sequence issued by the cited reference lines (paths are
 * relative to the reference root).  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless stated; the caller (PyTorch's caching allocator)
 *     owns all memory including workspaces; the library never allocates and keeps no pointer;
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*); no host synchronisation,
 *     so every call is legal inside hipStreamBeginCapture / hipGraph replay;
 *   - return 0 on success, < 0 for argument / shape / alignment / workspace errors, > 0 for a
 *     hipError_t; kd_last_error_string() describes the last failure on the calling thread;
 *   - activations are fp32 NHWC: a row-major matrix [M = B*H*W, C] with a row stride `ld` (floats);
 *   - a "deferred" operand (x, sc, sh, act) means value = act(x*sc[c] + sh[c]); sc == NULL means
 *     the tensor is already materialised; act: 0 none, 1 ReLU, 2 ReLU6;
 *   - BatchNorm batch statistics travel as a slab `partial[rows][2][C]` of per-workgroup sums whose
 *     row count is given by the matching kd_*_stat_rows() query (host function, no GPU work);
 *     `pstride` is the slab's channel stride (== C unless the BN covers a slice of a wider slab).
 */
#ifndef KD_HIP_H
#define KD_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KD_ACT_NONE 0
#define KD_ACT_RELU 1
#define KD_ACT_RELU6 2

int kd_version(void);
const char* kd_arch(void);
const char* kd_last_error_string(void);

/* ---- 1x1 convolution = fp32-MFMA GEMM ------------------------------------------------------
 * Replaces nn.Conv2d(k=1) / nn.Conv1d(k=1) forward and its data gradient:
 * camera_encoder.py:24,39  fusion_module.py:12,29,116  lidar_encoder.py:29,32.
 *   C[M,N] = Aeff[M,K] . W[N,K]^T (+ bias[N]) (+ addend[M,N])
 *   pro 0: Aeff = A                      pro 1: Aeff = act(A*p0 + p1)         (p0/p1 = sc/sh [K])
 *   pro 2: Aeff = p0*(A*mask(A2*p3+p4)) + p1*A2 + p2   (BN backward folded in: A = G, A2 = X raw,
 *          p0/p1/p2 = al/be/ga from kd_bn_bwd_finalize, p3/p4 = sc/sh of the mask or NULL)
 *   epi 0: store     epi 1: store + partial (sum, sum^2)      [forward, feeds kd_bn_finalize_train]
 *   epi 2: C *= act'(X*esc+esh); partial (sum C, sum C*xhat)  [dgrad, feeds kd_bn_bwd_finalize]
 *   epi 5: C = epi_act((raw + bias)*esc + esh) (+ addend)      [inference: eval BatchNorm + activation in the epilogue]
 *          pro 0 / 1 only; needs esc / esh [N] (16-byte aligned; kd_bn_eval_coeffs), no X, no partial.  Here the addend is
 *          the block's residual and is added AFTER the activation (the bits of kd_bn_act_apply with `res`); with epi 0 / 1 / 2
 *          it joins the raw result, before the bias, the statistics and the epi 2 mask.
 * The dgrad call passes W = transposed weight [K_out=Cin][N_red=Cout] (kd_transpose).
 * m_dev (optional device int): data-dependent row count <= M read by the kernel itself (no host sync). */
/* Arithmetic of the GEMM family: 0 = exact-fp32 MFMA (v_mfma_f32_32x32x2_f32), 1 = every fp32 operand split
 * exactly into three bf16 pieces and the six leading piece products accumulated in fp32 on the bf16 matrix pipe
 * (fp32-grade: error <= 3.97 * 2^-24 |x||y| per product.  That is 1.5 x the worst single-product error measured on an MI355X,
 * 2.65 * 2^-24 |x||y| over 1 M products per kernel form (tests/test_gpu_gemm_fp64.py); six sequentially nearest-rounded adds would
 * give 1.67 * 2^-24, the matrix pipe's own accumulation rounds less tightly.  The exact-fp32 form meets 2^-24 |x||y|).
 * Process-wide; returns the previous setting. */
int kd_set_gemm_split(int on);
int64_t kd_pwconv_stat_rows(int64_t M);
int64_t kd_pwconv_stat_rows_for(int64_t M, int K, int N, int pro, int epi, int with_addend);
/* Rows of the statistics slab the launch for (K, N, pro, epi, addend given or not) will write in the current arithmetic (one per workgroup for the
 * weight-resident streaming kernels of kd_gemm_stream.hip, one per 128 matrix rows for the tiled kernels): size the slab and
 * drive kd_bn_finalize_train / kd_bn_bwd_finalize with it.  kd_set_gemm_stream: 0 = tiled kernels only, 1 = streaming
 * kernels only for the shapes that win in isolation, 2 = every covered shape (default; env KD_GEMM_STREAM=0|1|all), 3 = every covered forward shape, tiled data gradients;
 * returns the previous mode. */
int kd_set_gemm_stream(int mode);
int kd_pwconv_gemm(const float* A, int64_t lda, const float* A2, int64_t lda2, int pro, int pro_act,
                   const float* p0, const float* p1, const float* p2, const float* p3, const float* p4,
                   const float* W, const float* bias, float* C, int64_t ldc, const float* addend,
                   int64_t ldadd, int epi, const float* X, int64_t ldx, const float* esc, const float* esh,
                   const float* emean, const float* einv, int epi_act, float* partial, int64_t partial_rows, int64_t M,
                   int K, int N, const int* m_dev, void* stream);
/* partial_rows (here and in kd_lidar_l1_fwd / _l1_dgrad / _l2_dgrad): the row count the caller sized `partial` for --
 * the value kd_pwconv_stat_rows_for() / kd_lidar_l*_dgrad_stat_rows() returned -- and will pass to kd_bn_finalize_train /
 * kd_bn_bwd_finalize.  The launch is REFUSED (status < 0) when it differs from what the kernel form selected now would
 * write (the streaming and tiled forms write different row counts and the choice depends on process-wide switches):
 * a slab sized for the other form is an error, never a silently wrong reduction.  Ignored when partial == NULL. */
/* weight gradient dW[N,K] = Deff[M,N]^T . Aeff[M,K] (split-M partial tiles in `ws`, fixed-order sum).
 * d_mode 0: Deff = D; d_mode 2: Deff = al*(D*mask(X*msc+msh)) + be*X + ga.  a_mode 0/1 like pro 0/1. */
size_t kd_pwconv_wgrad_ws_bytes(int64_t M, int N, int K);
/* Weight-gradient kernel form (split arithmetic only).  1 (default): layers where the role-specialised kernel (csrc/kd_wgrad_rs.hip: one
 * workgroup per CU owns a whole block of dW, vector waves load / convert, matrix waves multiply) measured faster use it; 2 (env
 * KD_WGRAD_RS=all): every layer that has an instance; 0 (KD_WGRAD_RS=0): the tiled kernel everywhere.  Returns the previous mode.
 * kd_pwconv_wgrad_ws_bytes answers for the larger of the two forms whatever the mode. */
int kd_set_wgrad_rs(int mode);
int kd_pwconv_wgrad(const float* D, int64_t ldd, const float* X, int64_t ldx, int d_mode, int d_act,
                    const float* al, const float* be, const float* ga, const float* msc, const float* msh,
                    const float* A, int64_t lda, int a_mode, int a_act, const float* asc, const float* ash,
                    float* dW, int64_t M, int N, int K, void* ws, size_t ws_bytes, void* stream);
/* Data gradient and weight gradient of one 1x1 layer in ONE launch (csrc/kd_wgrad_rs.hip): the role-specialised weight-gradient
 * kernel with the data gradient dX[M,K] = Deff[M,N] . Wt[K,N]^T on a matrix wave that plan leaves idle, from the D planes already
 * in LDS -- D and X are read and converted once instead of twice.  One instance: N = 192, K = 32 (the stage-2 expand layer),
 * split arithmetic, d_mode 0 / 2, a_mode 0, epi 0, no addend, kd_set_wgrad_rs != 0; kd_pwconv_bwd_supported answers 0 for everything
 * else and the caller keeps kd_pwconv_wgrad + kd_pwconv_gemm.  dW has the bits of kd_pwconv_wgrad (default mode), dX those of
 * kd_pwconv_gemm(pro = d_mode, epi 0) with W = Wt.  D, X, A, dX dense (ldd == ldx == N, lda == lddx == K);
 * ws >= kd_pwconv_bwd_ws_bytes (the weight-gradient slab + a 256-byte line that absorbs the stores of rows beyond M).
 * Any unsupported call is refused with a status < 0 and no launch. */
int kd_pwconv_bwd_supported(int N, int K, int d_mode, int a_mode, int epi);
size_t kd_pwconv_bwd_ws_bytes(int64_t M, int N, int K);
int kd_pwconv_bwd(const float* D, int64_t ldd, const float* X, int64_t ldx, int d_mode, int d_act,
                  const float* al, const float* be, const float* ga, const float* msc, const float* msh,
                  const float* A, int64_t lda, int a_mode, int a_act, const float* asc, const float* ash,
                  const float* Wt, float* dX, int64_t lddx, const float* addend, int64_t ldadd, int epi,
                  float* dW, int64_t M, int N, int K, void* ws, size_t ws_bytes, void* stream);
int kd_transpose(const float* in, float* out, int R, int C, void* stream);
/* the same for n weights in one launch: table = device int64 [n][5] {in pointer, out pointer, R, C, first 256-element block of
 * this matrix}, first blocks ascending from 0, nblocks = sum of ceil(R*C/256) */
int kd_transpose_batch(const int64_t* table, int n, int nblocks, void* stream);
/* up to four small device-to-device float copies in one launch (unused segments: n = 0): packed parameter gradients -> their
 * slots in a flat gradient buffer */
int kd_copy_segments(const float* s0, float* d0, int64_t n0, const float* s1, float* d1, int64_t n1, const float* s2, float* d2,
                     int64_t n2, const float* s3, float* d3, int64_t n3, void* stream);

/* ---- stem 3x3/s2 conv (camera_encoder.py:63-67), NCHW image in, NHWC raw out, Cout in {8, 16, 24, 32, 40}
 * (TwinLiteEncoder base_channels; any other Cout: KD_ERR_SHAPE), Cin 1..4; the statistics slab is [rows][2][Cout] ---- */
int64_t kd_stem_stat_rows(int64_t npix_out);
int kd_stem_conv_fwd(const float* x_nchw, const float* w, float* y_nhwc, float* partial, int B, int Cin, int H,
                     int W, int Cout, void* stream);
/* inference (eval mode, no autograd): y = act(conv(x) * sc + sh) in one kernel, Cin == 3; the bits of kd_stem_conv_fwd + kd_bn_act_apply */
int kd_stem_conv_fwd_infer(const float* x_nchw, const float* w, const float* sc, const float* sh, int act, float* y_nhwc,
                           int B, int Cin, int H, int W, int Cout, void* stream);
/* im2col (K padded to Kp, zeros) so that the stem weight gradient is kd_pwconv_wgrad with K = Kp. */
int kd_stem_im2col(const float* x_nchw, float* col, int B, int Cin, int H, int W, int Kp, void* stream);

/* ---- depthwise 3x3, pad 1, stride 1|2 (camera_encoder.py:30-35, fusion_module.py:25-27,78) ---- */
int64_t kd_dwconv_stat_rows(int64_t npix_out, int C);
int kd_dwconv3x3_fwd(const float* x, const float* sc, const float* sh, int act, const float* w, float* y,
                     float* partial, int B, int H, int W, int C, int stride, void* stream);
int64_t kd_dwconv_bwd_stat_rows(int64_t npix_in, int C);
/* form of the stride-1 backward when both gradients are requested: 0 separate data / weight kernels, 1 one fused
 * column-walk kernel, 2 one fused tile kernel (operands staged once through LDS), 3 (default) chosen by shape */
int kd_set_dw_bwd_mode(int mode);
size_t kd_dwconv_bwd_ws_bytes(int64_t npix_out, int C);
int kd_dwconv3x3_bwd(const float* D, const float* Y, const float* al, const float* be, const float* ga,
                     const float* dsc, const float* dsh, int d_act, const float* x, const float* sc,
                     const float* sh, int act, const float* mean, const float* invstd, const float* w, float* gx,
                     float* partial, float* dw, int B, int H, int W, int C, int stride, void* ws, size_t ws_bytes,
                     void* stream);
/* the same with a second gradient path into the conv's input (the residual of an inverted-residual block whose first
 * convolution is this one, camera_encoder.py:46-51 at expansion_ratio 1): gx = (conv^T dy + addend) * act'(.), sums included.
 * Needs both gradients and a shape kd_dwconv3x3_bwd_add_supported() accepts (the stride-1 column-walk form). */
int kd_dwconv3x3_bwd_add_supported(int C, int W, int stride);
int kd_dwconv3x3_bwd_add(const float* D, const float* Y, const float* al, const float* be, const float* ga,
                         const float* dsc, const float* dsh, int d_act, const float* x, const float* sc,
                         const float* sh, int act, const float* mean, const float* invstd, const float* w,
                         const float* addend, float* gx, float* partial, float* dw, int B, int H, int W, int C, int stride,
                         void* ws, size_t ws_bytes, void* stream);

/* ---- BatchNorm coefficient kernels (nn.BatchNorm1d/2d: eps 1e-5, momentum 0.1) ---------------- */
int kd_bn_finalize_train(float* partial, int rows, int C, int pstride, int64_t count, const float* gamma,
                         const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                         int64_t* num_batches_tracked, float* mean, float* invstd, float* scale, float* shift,
                         void* stream);
int kd_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                      float eps, int C, float* mean, float* invstd, float* scale, float* shift, void* stream);
int64_t kd_rowwise_stat_rows(int64_t M, int C);
int kd_bn_act_apply(const float* x, int64_t ldx, const float* sc, const float* sh, int act, const float* res,
                    int64_t ldr, float* out, int64_t ldo, int64_t M, int C, void* stream);
/* the same with a residual that is itself deferred: out = act(x*sc+sh) + ract(res*rsc+rsh) */
int kd_bn_act_apply_res(const float* x, int64_t ldx, const float* sc, const float* sh, int act, const float* res, int64_t ldr,
                        const float* rsc, const float* rsh, int ract, float* out, int64_t ldo, int64_t M, int C, void* stream);
int kd_bn_bwd_reduce(const float* D, int64_t ldd, const float* X, int64_t ldx, const float* sc, const float* sh,
                     int act, const float* mean, const float* invstd, float* partial, int64_t M, int C,
                     void* stream);
int kd_bn_bwd_finalize(float* partial, int rows, int C, int pstride, int64_t count, const float* gamma, const float* mean,
                       const float* invstd, int training, float* dgamma, float* dbeta, float* al, float* be,
                       float* ga, float* dbias, void* stream);

/* ---- LiDAR branch (lidar_encoder.py:25-35,42-99) ----------------------------------------------- */
/* layer 0 (Conv1d 4 -> C, bias): y == NULL runs the BatchNorm-statistics pass only -- the consumers below recompute
 * the layer from the 16-byte point, so its [P, C] output never exists in HBM */
int kd_lidar_l0_fwd(const float* pts, const float* w, const float* b, float* y, float* partial, int64_t P, int C,
                    const int* p_dev, void* stream);
/* layer 1 (Conv1d C0 -> N, lidar_encoder.py:29) over act0(bn0(layer0(pts))) recomputed on load: forward (epi 0 store,
 * 1 store + BN statistics), data gradient (writes G0 = d/d(layer-0 output) * act0' with the BN0-backward sums; Wt = W1
 * transposed to [K0][N1]) and weight gradient.  Same kernels and coefficient conventions as kd_pwconv_gemm / _wgrad. */
int kd_lidar_l1_fwd(const float* pts, const float* w0, const float* b0, const float* sc0, const float* sh0, int act0,
                    const float* W1, const float* bias1, float* C, int64_t ldc, int epi, float* partial,
                    int64_t partial_rows, int64_t M, int K, int N, const int* m_dev, void* stream);
int kd_lidar_l1_dgrad(const float* G, int64_t ldg, const float* Y1, int64_t ldy, const float* al, const float* be,
                      const float* ga, const float* msc, const float* msh, int mact, const float* Wt, float* G0,
                      int64_t ldg0, const float* pts, const float* w0, const float* b0, const float* sc0,
                      const float* sh0, const float* mean0, const float* invstd0, int act0, float* partial,
                      int64_t partial_rows, float* m1_out, void* m1_ws, size_t m1_ws_bytes, int64_t M, int N1, int K0,
                      void* stream);
/* m1_out (optional, [4][K0]) = sum_m G0[m][c] * pts[m][j]: the only way the layer-0 weight gradient depends on G0
 * (dW0 = al0 * m1 + sum_m (be0*y0 + ga0) * pts, the second term from kd_lidar_l0_bwd with D = NULL).  With m1_out set,
 * G0 may be NULL and the [points, K0] gradient is never written.  m1_ws: kd_lidar_l1_dgrad_ws_bytes. */
size_t kd_lidar_l1_dgrad_ws_bytes(int64_t M, int K0);
/* rows of the BatchNorm-backward slab (`partial`) kd_lidar_l1_dgrad / kd_lidar_l2_dgrad write for a shape in the current
 * arithmetic (one per workgroup when a streaming kernel takes the launch, one per 128 matrix rows otherwise) */
int64_t kd_lidar_l1_dgrad_stat_rows(int64_t M, int N1, int K0);
int64_t kd_lidar_l2_dgrad_stat_rows(int64_t M, int N2, int K1);
int kd_lidar_l1_wgrad(const float* D, int64_t ldd, const float* X, int64_t ldx, int d_act, const float* al,
                      const float* be, const float* ga, const float* msc, const float* msh, const float* pts,
                      const float* w0, const float* b0, const float* sc0, const float* sh0, int act0, float* dW,
                      int64_t M, int N, int K, void* ws, size_t ws_bytes, void* stream);
size_t kd_lidar_l0_bwd_ws_bytes(int64_t P, int C);
/* Y == NULL: the layer output is recomputed from (w, b) and the point (it was never written, see kd_lidar_l1_*) */
int kd_lidar_l0_bwd(const float* D, const float* Y, const float* w, const float* b, const float* al, const float* be, const float* ga,
                    const float* pts, float* dwb, int64_t P, int C, void* ws, size_t ws_bytes, void* stream);
/* eval mode: last point-MLP layer + BatchNorm + ReLU + BEV scatter-max in one kernel (zeroes `grid` first); rows are the
 * compacted in-range points, cell_idx[p] their flat (frame, cell) grid row; the layer output is never written */
int kd_lidar_l2_fwd_scatter(const float* A, int64_t lda, const float* sc1, const float* sh1, int act1, const float* W2,
                            const float* bias2, const float* sc2, const float* sh2, int act2, const int* cell_idx,
                            float* grid, int64_t ncells, int64_t M, int K, int N, const int* m_dev, void* stream);
/* The WHOLE eval-mode encoder in one kernel (csrc/kd_lidar_infer.hip): point MLP 4 -> 64 -> 128 -> 128 (Conv1d + eval BatchNorm +
 * ReLU each, lidar_encoder.py:25-35) + scatter-max (:85-96); no activation leaves the CU (layer 1 is computed transposed so
 * that its accumulators are layer 2's operand fragments).  Split arithmetic; zeroes `grid`; sc / sh = kd_bn_eval_coeffs. */
int kd_lidar_mlp_scatter_infer_supported(int C0, int C1, int C2);
int kd_lidar_mlp_scatter_infer(const float* pts, const int* cell, const int* p_dev, const float* w0, const float* b0,
                               const float* sc0, const float* sh0, const float* W1, const float* bias1, const float* sc1,
                               const float* sh1, const float* W2, const float* bias2, const float* sc2, const float* sh2,
                               float* grid, int64_t ncells, int64_t P, int C0, int C1, int C2, void* stream);
/* the same encoder in the bf16-storage inference mode (operands rounded to bf16 once, one MFMA product, fp32 accumulate, fp32
 * grid): replaces kd_bf16_pwconv(a_kind 3) + kd_bf16_pwconv(epi 4) and the bf16 [P, 128] tensor between them */
int kd_bf16_lidar_mlp_scatter_supported(int C0, int C1, int C2);
int kd_bf16_lidar_mlp_scatter(const float* pts, const int* cell, const int* p_dev, const float* w0, const float* b0,
                               const float* sc0, const float* sh0, const float* W1, const float* bias1, const float* sc1,
                               const float* sh1, const float* W2, const float* bias2, const float* sc2, const float* sh2,
                               float* grid, int64_t ncells, int64_t P, int C0, int C1, int C2, void* stream);
/* Activation contract of every scatter-max entry point: the FORWARD forms (kd_lidar_scatter_max_fwd, _scatter_max_idx_fwd,
 * _seg_max_fwd, _seg_hold_fwd, _l2_fwd_scatter) take KD_ACT_RELU or KD_ACT_RELU6 (anything else: KD_ERR_ARG -- the zeroed grid
 * is the maximum's identity only for non-negative values).  The BACKWARD forms (kd_lidar_scatter_max_bwd, _seg_max_bwd,
 * _seg_share_bwd, _seg_hold_bwd, _l2_dgrad, _l2_wgrad, _l2_bwd) split dout evenly among the holders v > 0 && v == max, which is
 * the derivative under ReLU only: under ReLU6 a maximum saturated at 6.0 has derivative 0 (ATen: the amax split, then
 * hardtanh_backward zeroes z >= 6), so they refuse KD_ACT_RELU6 with KD_ERR_ARG instead of returning a wrong gradient. */
int kd_lidar_scatter_max_fwd(const float* pts, const float* y, const float* sc, const float* sh, int act,
                             float* grid, int B, int64_t N, int C, int H, int W, float x0, float x1, float y0,
                             float y1, void* stream);
int64_t kd_lidar_scatter_stat_rows(int64_t P, int C);
size_t kd_lidar_scatter_bwd_ws_bytes(int B, int H, int W, int C);
int kd_lidar_scatter_max_bwd(const float* pts, const float* y, const float* sc, const float* sh, int act,
                             const float* grid, const float* dout, const float* mean, const float* invstd,
                             float* G, float* partial, int B, int64_t N, int C, int H, int W, float x0, float x1,
                             float y0, float y1, void* ws, size_t ws_bytes, void* stream);
int kd_lidar_bev_index(const float* pts, int* cell, int64_t P, int H, int W, float x0, float x1, float y0,
                       float y1, void* stream);
/* training path of the same scatter-max (lidar_encoder.py:57-99), atomic-free: bin the point ids by grid row
 * once (counting sort), then one wave per row takes the max / counts the ties / splits the gradient.
 * row_of_point[B*N] = b*H*W + cell or -1; seg_start[B*H*W + 1]; perm[B*N] (first seg_start[B*H*W] entries used).
 * Same results as kd_lidar_scatter_max_fwd / _bwd (bit-identical grid and G).  C must be 64, 128 or 256. */
size_t kd_lidar_cell_sort_ws_bytes(int B, int64_t N, int H, int W);
int kd_lidar_cell_sort(const float* pts, int B, int64_t N, int H, int W, float x0, float x1, float y0, float y1,
                       int* row_of_point, int* seg_start, int* perm, void* ws, size_t ws_bytes, void* stream);
/* the same bins with a deterministic in-cell order (ascending point id), applied to the POINTS: the point MLP then runs
 * on pts_sorted, every grid row owns a contiguous row range (pass perm = NULL to kd_lidar_seg_max_*), the out-of-range
 * points are the tail, and the eval path's compacted list is the first seg_start[B*H*W] rows.  perm may be NULL.
 * KD_ERR_SHAPE (-4) when H*W + 1 > 36865 (144 KB LDS histogram): call kd_lidar_sort_points_wide (below) instead. */
size_t kd_lidar_sort_points_ws_bytes(int B, int64_t N, int H, int W);
int kd_lidar_sort_points(const float* pts, int B, int64_t N, int H, int W, float x0, float x1, float y0, float y1,
                         float* pts_sorted, int* row_sorted, int* seg_start, int* perm, void* ws, size_t ws_bytes,
                         void* stream);
/* kd_lidar_sort_points for larger grids: same arguments, same outputs (the unique stable sort by (frame, cell); out-of-range
 * and NaN points after all in-range points, frame by frame in original order; point bits unchanged; perm may be NULL), for
 * any 1 <= H, W <= 4096 (KD_ERR_SHAPE beyond; B*N and B*H*W + 1 below 2^31 as above).  A two-digit counting sort inside each
 * frame (by column, then by row): LDS holds max(H, W) + 1 ints and the workspace blocks x (W + H + 1) table entries instead of
 * blocks x (H*W + 1) -- about 0.37 GB at B = 256, N = 80000, 256 x 256.  Small grids are accepted too (same bits as
 * kd_lidar_sort_points; kdrt keeps that one for grids up to 192 x 192).  No floating-point atomics; the per-cell counts
 * are integer atomic adds of ones, the same in every order. */
size_t kd_lidar_sort_points_wide_ws_bytes(int B, int64_t N, int H, int W);
int kd_lidar_sort_points_wide(const float* pts, int B, int64_t N, int H, int W, float x0, float x1, float y0, float y1,
                              float* pts_sorted, int* row_sorted, int* seg_start, int* perm, void* ws, size_t ws_bytes,
                              void* stream);
/* Training backward of the last point-MLP layer WITHOUT the [points, C] scatter-max gradient (rows sorted by
 * kd_lidar_sort_points).  kd_lidar_seg_share_bwd leaves share[cells, C] = dout / holders and the BatchNorm-backward sums;
 * the two GEMMs rebuild G[m][c] = (rows[m] >= 0 && v > 0 && v == grid[rows[m]][c]) ? share[rows[m]][c] : 0 on load
 * (v = act2(Y2*sc2 + sh2)) -- bit-identical to kd_lidar_seg_max_bwd + kd_pwconv_gemm(pro 2, epi 2) / kd_pwconv_wgrad
 * (d_mode 2), minus 2.5 passes over a [points, C] tensor. */
int64_t kd_lidar_seg_share_stat_rows(int64_t ncells, int64_t P);
int kd_lidar_seg_share_bwd(const float* y, const float* sc, const float* sh, int act, const float* grid,
                           const float* dout, const float* mean, const float* invstd, const int* seg_start,
                           const int* row_sorted, float* share, float* cnt_ws, float* partial, int64_t P,
                           int64_t ncells, int C, void* stream);
/* The same pair without the second read of y: kd_lidar_seg_hold_fwd is kd_lidar_seg_max_fwd (row_sorted form, same grid bits)
 * that also records, per (cell, channel), rawmax = the raw value of the maximum's first holder and holders = their number
 * (one byte; 255 = "sweep the cell's rows": holders with different raw values, more than 254 of them, a row of more than
 * 256 points).  kd_lidar_seg_hold_bwd derives share and partial from (dout, rawmax, holders) -- bit-identical to
 * kd_lidar_seg_share_bwd for finite features -- and reads y and grid only for the cells marked 255.  rawmax [ncells, C]
 * (rows of empty and >256-point cells are not written), holders [ncells, C] bytes, 4-byte aligned, every row written. */
int kd_lidar_seg_hold_fwd(const float* y, const float* sc, const float* sh, int act, const int* seg_start,
                          const int* row_sorted, float* grid, float* rawmax, uint8_t* holders, int64_t P, int64_t ncells,
                          int C, void* stream);
int kd_lidar_seg_hold_bwd(const float* y, const float* sc, const float* sh, int act, const float* grid,
                          const float* rawmax, const uint8_t* holders, const float* dout, const float* mean,
                          const float* invstd, const int* seg_start, const int* row_sorted, float* share, float* cnt_ws,
                          float* partial, int64_t P, int64_t ncells, int C, void* stream);
int kd_lidar_l2_dgrad(const float* Y2, int64_t ldy2, const int* rows, const float* grid, const float* share,
                      const float* al, const float* be, const float* ga, const float* sc2, const float* sh2, int act2,
                      const float* Wt, float* G1, int64_t ldg1, const float* Y1, int64_t ldy1, const float* sc1,
                      const float* sh1, const float* mean1, const float* invstd1, int act1, float* partial,
                      int64_t partial_rows, int64_t M, int N2, int K1, void* stream);
int kd_lidar_l2_wgrad(const float* Y2, int64_t ldy2, const int* rows, const float* grid, const float* share,
                      const float* al, const float* be, const float* ga, const float* sc2, const float* sh2, int act2,
                      const float* Y1, int64_t ldy1, const float* sc1, const float* sh1, int act1, float* dW,
                      int64_t M, int N2, int K1, void* ws, size_t ws_bytes, void* stream);
/* The same backward in ONE kernel (csrc/kd_lidar_bwd.hip): G1 + BatchNorm-1 backward sums (== kd_lidar_l2_dgrad, bit for bit)
 * and dW2 (== kd_lidar_l2_wgrad up to summation order) from one read and one bf16x3 split of Y2 and Y1 -- 31 GB instead of
 * 52 GB of HBM traffic at 256 frames x 80 000 points.  Split arithmetic, N2 = K1 = 128 (kd_lidar_l2_bwd_supported); `partial`
 * has kd_lidar_l2_bwd_stat_rows(M) rows (passed back as partial_rows and checked), ws >= kd_lidar_l2_bwd_ws_bytes. */
int kd_lidar_l2_bwd_supported(int N2, int K1);
int64_t kd_lidar_l2_bwd_stat_rows(int64_t M);
size_t kd_lidar_l2_bwd_ws_bytes(int64_t M, int N2, int K1);
int kd_lidar_l2_bwd(const float* Y2, int64_t ldy2, const int* rows, const float* grid, const float* share, const float* al,
                    const float* be, const float* ga, const float* sc2, const float* sh2, int act2, const float* Wt,
                    float* G1, int64_t ldg1, const float* Y1, int64_t ldy1, const float* sc1, const float* sh1,
                    const float* mean1, const float* invstd1, int act1, float* partial, int64_t partial_rows, float* dW,
                    int64_t M, int N2, int K1, void* ws, size_t ws_bytes, void* stream);
/* Layer 1 in the same one-kernel form: dW1, the BatchNorm-0 backward sums of G0 = (dy1 . W1) * relu'(bn0(l0(point))) and the
 * moments m1_out[4][K0] = sum_m G0 * point (== kd_lidar_l1_dgrad(G0 = NULL, m1_out) + kd_lidar_l1_wgrad with an unmasked G:
 * dy1 = al*G + be*Y1 + ga).  Split arithmetic, N1 = 128, K0 = 64, ReLU; G and Y1 dense. */
int kd_lidar_l1_bwd_supported(int N1, int K0);
int64_t kd_lidar_l1_bwd_stat_rows(int64_t M);
size_t kd_lidar_l1_bwd_ws_bytes(int64_t M, int N1, int K0);
int kd_lidar_l1_bwd(const float* G, int64_t ldg, const float* Y1, int64_t ldy, const float* al, const float* be, const float* ga,
                    const float* Wt, const float* pts, const float* w0, const float* b0, const float* sc0, const float* sh0,
                    const float* mean0, const float* invstd0, int act0, float* partial, int64_t partial_rows, float* m1_out,
                    float* dW, int64_t M, int N1, int K0, void* ws, size_t ws_bytes, void* stream);
int kd_lidar_gather_sorted(const float* pts, const int* perm, const int* row_of_point, const int* nvalid_dev,
                           float* out_pts, int* out_row, int64_t P, void* stream);
/* row_sorted (optional, rows sorted by kd_lidar_sort_points, perm == NULL): grid rows holding more than 256 points are
 * then processed 64 points per wave, so a scene concentrated in a few cells costs what a uniform one costs. */
int kd_lidar_seg_max_fwd(const float* y, const float* sc, const float* sh, int act, const int* seg_start,
                         const int* perm, const int* row_sorted, float* grid, int64_t P, int64_t ncells, int C,
                         void* stream);
int64_t kd_lidar_seg_stat_rows(int64_t ncells);
int kd_lidar_seg_max_bwd(const float* y, const float* sc, const float* sh, int act, const float* grid,
                         const float* dout, const float* mean, const float* invstd, const int* seg_start,
                         const int* perm, const int* row_of_point, float* G, float* partial, int64_t P,
                         int64_t ncells, int C, void* stream);
/* inference-only: compact the in-range points (arbitrary order) with their flat (batch, cell) row; `counter`
 * (one device int, zeroed here) receives the count.  Then scatter-max over the pre-binned rows. */
int kd_lidar_compact(const float* pts, float* out_pts, int* out_cell, int* counter, int B, int64_t N, int H, int W,
                     float x0, float x1, float y0, float y1, void* stream);
int kd_lidar_scatter_max_idx_fwd(const float* y, const float* sc, const float* sh, int act, const int* cell_idx,
                                 float* grid, int64_t P, int C, int64_t ncells, const int* p_dev, void* stream);

/* ---- FPN resize, weighted-fusion tail, classifier (fusion_module.py:58-63,115-120,170-173) ----- */
int kd_bilinear_accum_fwd(const float* in, const float* sc, const float* sh, int act, float* out, int accumulate,
                          int B, int Hi, int Wi, int Ho, int Wo, int C, void* stream);
/* the whole FPN sum in one pass: up to three deferred laterals (in_i == NULL: absent, no gaps), bit-identical to
 * accumulating them one by one with kd_bilinear_accum_fwd */
int kd_bilinear_sum_fwd(const float* in0, const float* sc0, const float* sh0, int act0, int H0, int W0, const float* in1,
                        const float* sc1, const float* sh1, int act1, int H1, int W1, const float* in2, const float* sc2,
                        const float* sh2, int act2, int H2, int W2, float* out, int B, int Ho, int Wo, int C, void* stream);
int kd_bilinear_bwd(const float* dout, const float* in, const float* sc, const float* sh, int act,
                    const float* mean, const float* invstd, float* gin, float* partial, int B, int Hi, int Wi,
                    int Ho, int Wo, int C, void* stream);
/* Inference: the FPN lateral at the output size writes the FPN sum itself.  out[B*Ho*Wo, N] = (act0((A . W^T + bias) * esc + esh)
 * + 0.f) + resize(act1(in1 * sc1 + sh1)) (+ resize(act2(in2 * sc2 + sh2)); in2 == NULL: absent), in_t = [B, H_t, W_t, N]: the bits
 * of kd_pwconv_gemm (pro 0, epi 0) followed by kd_bilinear_sum_fwd; the raw lateral map is never written.  A = [B*Ho*Wo, K] with
 * row stride lda.  Covered (kd_pwconv_gemm_fpn_sum_supported, else KD_ERR_SHAPE and nothing is written): K = 64, N = 128, one
 * or two smaller laterals of any size, split arithmetic with the streaming kernels on. */
int kd_pwconv_gemm_fpn_sum_supported(int64_t M, int K, int N, int nlat);
int kd_pwconv_gemm_fpn_sum(const float* A, int64_t lda, const float* W, const float* bias, const float* esc, const float* esh,
                           int act0, const float* in1, const float* sc1, const float* sh1, int act1, int H1, int W1,
                           const float* in2, const float* sc2, const float* sh2, int act2, int H2, int W2, float* out, int B,
                           int Ho, int Wo, int K, int N, void* stream);
/* 1 (default): a lateral of exactly half the output size takes the quad body of kd_bilinear_sum_fwd and the 4 x 4 window form
 * of kd_bilinear_bwd / kd_bilinear_bwd2; 0: the general per-pixel bodies for every geometry.  The same bits either way.
 * Returns the previous mode. */
int kd_set_bilinear_2x_mode(int mode);
/* kd_bilinear_bwd for two laterals of one geometry [B,Hi,Wi,C] under the same dout: dout is read once; gin_i and partial_i
 * are bit-identical to two kd_bilinear_bwd launches */
int kd_bilinear_bwd2(const float* dout, const float* in0, const float* sc0, const float* sh0, int act0, const float* mean0,
                     const float* invstd0, float* gin0, float* partial0, const float* in1, const float* sc1, const float* sh1,
                     int act1, const float* mean1, const float* invstd1, float* gin1, float* partial1, int B, int Hi, int Wi,
                     int Ho, int Wo, int C, void* stream);
int kd_weighted_fuse_fwd(const float* cat, const float* sc, const float* sh, const float* hraw, const float* w2,
                         const float* b2, float* out, float* wts, int64_t M, int C, void* stream);
size_t kd_weighted_fuse_bwd_ws_bytes(int64_t M, int C);
int kd_weighted_fuse_bwd(const float* dout, const float* cat, const float* sc, const float* sh, const float* hraw,
                         const float* w2, const float* wts, float* dcat, float* gh, float* dparams, int64_t M,
                         int C, void* ws, size_t ws_bytes, void* stream);
/* Classifier 1x1 conv (Cin a multiple of 4 up to 64; 1 <= NC <= 16 classes, else KD_ERR_SHAPE) over a deferred NHWC input, NCHW
 * logits.  The kernels are compiled per class bucket (4, 8, 16) and the call takes the smallest bucket that holds NC; every
 * per-class operation runs in ascending class order in every bucket.  Backward: gx [M, Cin], partial = the fused BatchNorm-backward
 * sums (kd_cls_conv_bwd_stat_rows(M, Cin) rows of 2 * Cin), dwb = dW [NC*Cin] | db [NC] with db padded by zeros to a multiple of
 * 4: kd_cls_conv_dwb_floats(Cin, NC) floats (NC <= 4: NC*Cin + 4), which is also the row of the workspace. */
int kd_cls_conv_fwd(const float* x, const float* sc, const float* sh, int act, const float* w, const float* b,
                    float* logits_nchw, int64_t M, int HW, int Cin, int NC, void* stream);
int64_t kd_cls_conv_dwb_floats(int Cin, int NC);
size_t kd_cls_conv_bwd_ws_bytes(int64_t M, int Cin, int NC);
int64_t kd_cls_conv_bwd_stat_rows(int64_t M, int Cin);
int kd_cls_conv_bwd(const float* dlog_nchw, const float* x, const float* sc, const float* sh, int act,
                    const float* mean, const float* invstd, const float* w, float* gx, float* partial, float* dwb,
                    int64_t M, int HW, int Cin, int NC, void* ws, size_t ws_bytes, void* stream);

/* ---- "x4" decoder head: LightweightSegmentationHead (fusion_module.py:142-159) ------------------
 * ConvTranspose2d(k=4, s=2, p=1, bias=False) = kd_pwconv_gemm with W.view(Cin, Cout*16)^T (columns ordered
 * co*16 + kh*4 + kw, the weight's own layout) followed by col2im; backward = im2col of the folded dy
 * (al/be/ga of kd_bn_bwd_finalize, mask of the stage's own BN+ReLU) followed by the wgrad / dgrad GEMMs.
 * cls3x3 = Conv2d(Cin<=32, NC<=4, 3, padding=1) over a deferred NHWC input, NCHW logits. */
int64_t kd_deconv_stat_rows(int64_t npix_out, int Cout);
int kd_deconv4x4s2_col2im_fwd(const float* col, float* out, float* partial, int B, int H, int W, int Cout,
                             void* stream);
int kd_deconv4x4s2_im2col_bwd(const float* D, const float* Y, const float* al, const float* be, const float* ga,
                             const float* msc, const float* msh, int act, float* dcol, int B, int H, int W,
                             int Cout, void* stream);
int kd_cls3x3_fwd(const float* x, const float* sc, const float* sh, int act, const float* w, const float* b,
                  float* logits_nchw, int B, int H, int W, int Cin, int NC, void* stream);
int64_t kd_cls3x3_bwd_stat_rows(int64_t npix, int Cin);
size_t kd_cls3x3_bwd_ws_bytes(int64_t npix, int Cin, int NC);
int kd_cls3x3_bwd(const float* dlog_nchw, const float* x, const float* sc, const float* sh, int act,
                  const float* mean, const float* invstd, const float* w, float* gx, float* partial, float* dwb,
                  int B, int H, int W, int Cin, int NC, void* ws, size_t ws_bytes, void* stream);

/* ---- per-frame input preparation (src/data_loading/pandaset_dataset.py:13-45,108-127) ------------------
 * kd_bev_rasterize = remap_semantic (remap != 0: label = bit `id` of remap_bits, ids outside 0..63 -> 0) +
 * rasterize_bev over B ragged frames (offsets: device int64 [B+1], points of frame b are [offsets[b], offsets[b+1])):
 * mask[b,r,c] = label of the first point in input order of that cell with a non-zero label, else 0.  Range test is
 * inclusive (x_min <= x <= x_max); cell = trunc((v - min) / span * (n-1)) in float32, span = max - min as the
 * reference's float32 arithmetic sees it.  ws: kd_bev_rasterize_ws_bytes(B, H, W). */
size_t kd_bev_rasterize_ws_bytes(int B, int H, int W);
int kd_bev_rasterize(const float* x, const float* y, const int64_t* cls, const int64_t* offsets, int B, int64_t n_total,
                     int remap, uint64_t remap_bits, int H, int W, float x_min, float x_span, float x_max, float y_min,
                     float y_span, float y_max, void* ws, size_t ws_bytes, int64_t* mask, void* stream);
int kd_semantic_remap(const int64_t* raw, int64_t n, uint64_t remap_bits, int64_t* out, void* stream);
/* The multi-class remap: out[i] = table[raw[i]] for 0 <= raw[i] < ntab, else 0 (background); table: device int64 [ntab], ntab >= 1;
 * raw and out are two buffers.  Followed by kd_bev_rasterize with remap = 0 it gives a BEV mask of class indices. */
int kd_semantic_remap_table(const int64_t* raw, int64_t n, const int64_t* table, int ntab, int64_t* out, void* stream);
/* The voting rasteriser for class maps: kd_bev_rasterize decides a cell by the sweep's point order, this one by counts.  Points,
 * offsets, range test and cell arithmetic are those of kd_bev_rasterize (the same device functions: a point's cell is the same bit
 * for bit).  cls: class indices as kd_semantic_remap_table writes them; NC in 2..16, else KD_ERR_SHAPE and nothing is written.
 * rule: 1 = majority, 2 = priority, anything else KD_ERR_ARG (the first-point rule is kd_bev_rasterize).  rank: device int32 [NC],
 * or NULL for all zero; rank[0] is ignored.  min_points >= 1.  votes: optional int32 [B, H, W].
 * For every cell, n_c = the number of points of the frame that pass the inclusive range test, fall into the cell and have class c,
 * 1 <= c < NC.  A point of class 0, of a negative class or of a class >= NC counts nowhere; a NaN coordinate fails the range test.
 * A class is eligible in a cell when n_c >= min_points.
 *   majority: the eligible class with the largest n_c; equal counts go to the larger rank[c], then to the smaller c.
 *   priority: the eligible class with the largest rank[c]; equal ranks go to the larger n_c, then to the smaller c.
 *   no eligible class: mask = 0.      votes = the winner's n_c, 0 in a background cell.
 * ws: kd_bev_rasterize_vote_ws_bytes(B, H, W, NC) bytes (0 for arguments the call refuses), 16-byte aligned: uint32 counters
 * [B][H * W][K], K = 4 / 8 / 16, the class bucket that holds NC; cleared inside the call.  B * H * W * K < 2^31, n_total < 2^31.
 * Integer atomics only: the same input gives the same bits on every call, whatever the order of the points inside a frame.
 * tests/_label_rule_ref.py is the numpy mirror of the rule. */
size_t kd_bev_rasterize_vote_ws_bytes(int B, int H, int W, int NC);
int kd_bev_rasterize_vote(const float* x, const float* y, const int64_t* cls, const int64_t* offsets, int B, int64_t n_total,
                          int NC, int rule, const int32_t* rank, int min_points, int H, int W,
                          float x_min, float x_span, float x_max, float y_min, float y_span, float y_max,
                          void* ws, size_t ws_bytes, int64_t* mask, int32_t* votes, void* stream);
/* Class histogram of a label mask: counts is int64 [NC + 1] and is ACCUMULATED into: counts[c] += #{mask == c} for 0 <= c < NC,
 * counts[NC] += every other value (the ignore index -1 lands there).  NC in 1..16, n >= 0 (n = 0: nothing is launched). */
int kd_label_histogram(const int64_t* mask, int64_t n, int NC, int64_t* counts, void* stream);
/* out[max_points,4] = stack(x,y,z,i) zero-padded, or (choice != NULL, n >= max_points) the rows choice[0..max_points) */
int kd_points_prepare(const float* x, const float* y, const float* z, const float* intensity, const int64_t* choice,
                      int64_t n, int64_t max_points, float* out, void* stream);
int kd_image_u8hwc_to_f32chw(const uint8_t* in, float* out, int H, int W, void* stream);
/* Whole-batch forms, one launch each.  in[B,H,W,3] -> out[B,3,H,W], every frame with the bits of the per-frame call. */
int kd_image_u8hwc_to_f32chw_batch(const uint8_t* in, float* out, int B, int H, int W, void* stream);
/* out[B,max_points,4] from B ragged frames (offsets as in kd_bev_rasterize; x, y, z, intensity concatenated).  A frame
 * of n <= max_points points is stacked and zero-padded (the bits of kd_points_prepare with choice = NULL).  A longer
 * frame is cut to a uniform subset of exactly max_points rows without replacement, chosen on the device: point index
 * j gets the 32-bit key  Philox-4x32-10(counter = (j, 0, frame_keys[b] low word, high word), key = (seed low word,
 * high word))[word 0]  (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85); the kept rows are
 * the max_points smallest (key, j) pairs in lexicographic order and are written in ascending j.  A frame's rows so
 * depend on (seed, frame_keys[b], n, max_points) and its own points only -- not on the batch around it, the launch
 * shape or any atomics order.  frame_keys: device uint64 [B].  One workgroup per frame; no workspace.
 * tests/_input_batch_ref.py is the numpy mirror of the rule. */
int kd_points_prepare_batch(const float* x, const float* y, const float* z, const float* intensity, const int64_t* offsets,
                            const uint64_t* frame_keys, int B, int64_t n_total, int64_t max_points, uint64_t seed, float* out,
                            void* stream);
/* Pillow-exact 8-bit bilinear resize of a batch (pandaset_dataset.py:105-111): in[B,Hs,Ws,3] uint8 -> the bytes of
 * Image.fromarray(frame).resize((W, H), Image.BILINEAR), written as out_f32chw[B,3,H,W] = byte / 255 (the bits of
 * kd_image_u8hwc_to_f32chw_batch over the resized bytes) and / or out_u8hwc[B,H,W,3]; either output may be NULL, not both.
 * Pillow's ImagingResample in integers: horizontal pass first, rounded to uint8, then the vertical pass over those bytes
 * (kept in LDS); a sample is min(255, (2^21 + sum_t pixel[xmin + t] * k[t]) >> 22).  The tables are device pointers
 * built by the host in double (kdrt/resample.py, mirrored by tests/_pil_resample_ref.py): hbounds int32 [W,2] =
 * (xmin, n) per output column over the Ws axis, hk int32 [W,hks] its coefficients (n <= hks, tail ignored); vbounds
 * [H,2] / vk [H,vks] the same over the Hs axis.  An axis whose size does not change takes the table of (in, in), which is
 * the identity.  Supported (kd_image_resize_bilinear_supported, else KD_ERR_SHAPE and nothing is written): sources up
 * to 4096 x 4096, any upscale, downscale up to a factor of 16 per axis (hks, vks <= 33).  No workspace, no atomics. */
int kd_image_resize_bilinear_supported(int Hs, int Ws, int H, int W);
int kd_image_resize_bilinear_batch(const uint8_t* in, const int32_t* hbounds, const int32_t* hk, int hks, const int32_t* vbounds,
                                   const int32_t* vk, int vks, float* out_f32chw, uint8_t* out_u8hwc, int B, int Hs, int Ws,
                                   int H, int W, void* stream);

/* ---- opt-in training augmentation of a batch, in place (csrc/kd_augment.hip; no reference counterpart) ----------
 * params: device float32 [B,16], one row per frame, drawn on the host by kdrt/augment.py frame_params as a pure function
 * of (settings, seed, frame key).  Row layout (word: field):
 *    0 c   1 s   2 scale   3 tx   4 ty   5 sx   6 sy   7 gi   8 a_r   9 a_g   10 a_b   11 b   12 mirror   13..15 padding
 * (c, s: cosine and sine of the yaw; sx, sy: +1 / -1 flip signs; gi: intensity gain; a_*, b: image gains and offset;
 * mirror: 0 or 1).  The draw: w0..w11 = the output words of Philox-4x32-10 at counters (0, 1, key lo, key hi),
 * (1, 1, ..), (2, 1, ..) under the key (seed lo, seed hi), u_k = (w_k >> 8) * 2^-24, d(r, u) = r * (2u - 1) in double:
 *    w0  yaw = d(rot_deg, u0) degrees; c, s = its cosine and sine (reduced to a multiple of 90 degrees plus a rest in
 *        [-45, 45] first, so that 0, +-90 and +-180 degrees give exact 0 and +-1)
 *    w1  scale = 1 + d(scale, u1)          w2  tx = d(translate, u2)          w3  ty = d(translate, u3)
 *    w4  flipped = u4 < flip: the sign of flip_axis is -1 and mirror = 1
 *    w5  gi = 1 + d(intensity, u5)         w6  brightness = d(brightness, u6)  w7  contrast = 1 + d(contrast, u7)
 *    w8, w9, w10  channel gain r, g, b = 1 + d(channel_gain, u)
 *    w11 dropped = u11 < camera_drop: a_r = a_g = a_b = b = 0
 *    a_c = gain_c * contrast,  b = 0.5 * (1 - contrast) + brightness;  every field computed in double, rounded once.
 * Counter word 1 keeps the streams apart: 0 is the subset sampler of kd_points_prepare_batch, 1 these parameters, 2 the
 * per-point jitter.  tests/_augment_ref.py is the numpy mirror of both kernels and of the draw.
 *
 * kd_points_augment_batch: x, y, z, intensity are the packed columns of B ragged frames (offsets, frame_keys as in
 * kd_points_prepare_batch), rewritten in place.  Point j of frame b, every operation a separately rounded float32 one:
 *    xf = sx*x;  yf = sy*y;  xr = c*xf - s*yf;  yr = s*xf + c*yf;
 *    x' = (scale*xr + tx) + jx;  y' = (scale*yr + ty) + jy;  z' = scale*z + jz;  i' = gi*i
 * with j? = jitter * ((word? >> 8) * 2^-23 - 1) from words 0, 1, 2 of Philox-4x32-10(counter = (j, 2, frame_keys[b] low
 * word, high word), key = (seed low word, high word)).  jitter == 0: no jitter term is added and no Philox block is
 * computed.  NaN rows stay NaN.  Run it before kd_bev_rasterize and kd_points_prepare_batch: labels and points then see
 * the same coordinates.  A frame's result depends on its own points, row, key, seed and jitter only.  16-byte accesses
 * where the four columns of a frame sit alike within a 16-byte line (a column stride that is a multiple of 4 floats
 * gives that), 4-byte accesses otherwise.  No workspace, no atomics.
 *
 * kd_image_augment_batch: img[B,3,H,W] float32 in place, v' = min(max(v*a_c + b, 0), 1) (product and sum rounded
 * separately); with mirror != 0 the columns w and W-1-w of every row swap.  Any W >= 1; 16-byte accesses when W is a
 * multiple of 8 and img is 16-byte aligned. */
int kd_points_augment_batch(float* x, float* y, float* z, float* intensity, const int64_t* offsets, const uint64_t* frame_keys,
                            const float* params, int B, int64_t n_total, uint64_t seed, float jitter, void* stream);
int kd_image_augment_batch(float* img, const float* params, int B, int H, int W, void* stream);

/* ---- losses, metric, optimiser (trainer.py:18-37,55-56,86-90; KD terms are build-defined) ------ */
/* Weighted CE with ignore_index + temperature KL to a teacher, value and dL/dzs in one call, 2 <= NC <= 16 classes (else
 * KD_ERR_SHAPE, nothing written).  losses[0] = CE (weighted mean), [1] = KL (per-pixel mean; 0 if zt NULL), [2] = sum of class
 * weights over the kept pixels, [3] unused.  dzs (NULL: forward only) = gscale * gscale_dev[0] * d/dzs (CE + alpha*T^2*KL).  The
 * kernels are compiled per class bucket (4, 8, 16) and the call takes the smallest bucket that holds NC; every per-class operation
 * runs in ascending class order in every bucket, and NC <= 4 runs the bucket-4 code.  ws = kd_seg_loss_ws_bytes(B * HW) bytes. */
size_t kd_seg_loss_ws_bytes(int64_t npix);
int kd_seg_loss_fwd_bwd(const float* zs, const float* zt, const int64_t* target, const float* class_w,
                        int ignore_index, float T, float alpha, float gscale, const float* gscale_dev, float* losses,
                        float* dzs, int B, int NC, int HW, void* ws, size_t ws_bytes, void* stream);
/* The opt-in region-based hard-label loss: vals[0] = wf * Focal + wt * Tversky in place of the weighted CE,
 *   Focal   = sum_K w[y] (1 - p_y)^gamma (-log p_y) / sum_K w[y],   K = the pixels kd_seg_loss_fwd_bwd keeps, p = softmax(zs),
 *   Tversky = 1 - (1/NC) sum_c (TP_c + s) / (TP_c + a FP_c + b FN_c + s) over the kept pixels of the whole call (no class weights).
 * Arguments as kd_seg_loss_fwd_bwd (zt NULL: no KL; dzs NULL: forward only; dzs = gscale * gscale_dev[0] * d/dzs (vals[0] +
 * alpha*T^2*KL)) plus gamma (0 or >= 1), wf, wt (>= 0, not both 0), a, b (>= 0), s (> 0); anything else is KD_ERR_ARG.  vals holds
 * 17 floats: [0] L_hard [1] KL [2] sum of weights [3] Focal [4] Tversky [5..8] TI_c [9..16] the per-class gradient coefficients the
 * gradient pass reads.  A term whose weight is 0 is not evaluated (reported as 0); no kept pixel and wf > 0: vals[0] is NaN like the
 * CE.  Three launches, no atomics, no host reads, ws = kd_seg_region_loss_ws_bytes(B * HW) bytes: bit-identical from call to call. */
size_t kd_seg_region_loss_ws_bytes(int64_t npix);
int kd_seg_region_loss_fwd_bwd(const float* zs, const float* zt, const int64_t* target, const float* class_w, int ignore_index,
                               float T, float alpha, float gscale, const float* gscale_dev, float gamma, float wf, float wt,
                               float a, float b, float s, float* vals, float* dzs, int B, int NC, int HW, void* ws,
                               size_t ws_bytes, void* stream);
/* The opt-in Lovasz-Softmax hard-label term (csrc/kd_loss_lovasz.hip), classes = "present", per image:
 *   L = (1/B) sum_b (1/|P_b|) sum_{c in P_b} L_{b,c},  L_{b,c} = sum_k e_k g_k over the kept pixels of image b (the pixels
 *   kd_seg_loss_fwd_bwd keeps) sorted by the error e descending, equal fp32 bits in ascending pixel order; e = p_c off the class and
 *   the sum of the other probabilities on it (p = softmax(zs)), g_k the increment of the Jaccard loss at sorted position k, P_b the
 *   classes with a pixel in image b.  An image without a kept pixel adds 0 and still counts in B.  No class weights.
 * vals holds 1 + 4 floats: L, then per class the mean of L_{b,c} over the images where it is present (0 if never).
 * hard_inout (may be NULL): hard_inout[0] += weight * L.   dzs (may be NULL: forward only) = weight * gscale * gscale_dev[0] * dL/dzs,
 * stored (accumulate = 0) or added to what dzs holds (accumulate = 1: the CE / region call wrote it before, on the same stream).
 * order_out (may be NULL; for tests): [B][NC][HW] int32, the pixel at sorted position k, -1 past the kept count and for absent classes.
 * One workgroup per (image, class) sorts 64-bit keys in LDS, so HW <= 16384 (128 x 128) and 2 <= NC <= 4, else KD_ERR_SHAPE; a
 * weight that is not finite and > 0 or a NULL zs / target / vals is KD_ERR_ARG; ws = kd_seg_lovasz_ws_bytes(B, NC, HW) bytes, else
 * KD_ERR_WORKSPACE.  Three launches, no atomics, no host reads: bit-identical from call to call. */
size_t kd_seg_lovasz_ws_bytes(int B, int NC, int HW);
int kd_seg_lovasz_fwd_bwd(const float* zs, const int64_t* target, int ignore_index, float weight, float gscale,
                          const float* gscale_dev, float* vals, float* hard_inout, float* dzs, int accumulate, int32_t* order_out,
                          int B, int NC, int HW, void* ws, size_t ws_bytes, void* stream);
/* The opt-in online-hard-example-mining (OHEM) cross-entropy (csrc/kd_loss_ohem.hip), 2 <= NC <= 16 classes on the
 * class buckets of kd_seg_loss_fwd_bwd.  K = the pixels kd_seg_loss_fwd_bwd keeps, n = |K|, l_i = -log p_{y_i} in fp32 from the same
 * softmax at T = 1 (>= 0, stored with the sign bit clear, so its bits order as unsigned integers):
 *   m = min(n, max(min_kept, ceil(n / min_divisor))) in integers,   tau_m = the m-th largest l over K (an exact order statistic),
 *   theta = min(tau_m, lambda) with lambda = fl32(-log(thresh)) formed by the caller,   S = { i in K : l_i >= theta },
 *   vals[0] = L = sum_S w[y] l / sum_S w[y],   dzs = gscale * gscale_dev[0] * (dL/dzs + alpha*T^2 dKL/dzs) with S held constant:
 *   w[y_i] (p_ij - [j == y_i]) / sum_S w on S, 0 on the rest of K; the KL value and gradient run over all pixels and keep the bits
 *   of kd_seg_loss_fwd_bwd.  At least m pixels above the threshold: all of them are kept; otherwise the m hardest with every tie at
 *   tau_m: S is a function of the values alone.  min_divisor = 1 or lambda = 0 keeps all of K (the weighted CE).  n = 0: vals[0] is NaN
 *   like the CE, no hard-label gradient.  A NaN l sorts above every number and is kept.
 * vals holds 8 floats: [0] L  [1] KL (per-pixel mean; 0 if zt NULL)  [2] sum_S w  [3] the weighted CE over all of K  [4] theta
 * [5] |S| / n  [6..7] 0.  counts_out (may be NULL): int64[3] = n, m, |S|.  nll_out (may be NULL; for tests): float [B*HW], l or -1
 * outside K.  keep_out (may be NULL; for tests): uint8 [B*HW], 1 on S.  zt NULL: no KL; dzs NULL: forward only.
 * Selection: a radix select over the 31 value bits in digits of 11 + 10 + 10 bits, histograms privatised in LDS and flushed with
 * integer atomics, m, the running rank and theta on the device.  Seven launches with dzs, six without; no floating-point atomics,
 * no host reads: capturable, bit-identical from call to call.  NC outside 2..16, B < 1, HW < 1 or B * HW >= 2^31 is KD_ERR_SHAPE; a
 * lambda that is not finite and >= 0, min_kept < 1, min_divisor < 1 or a NULL zs / target / vals is KD_ERR_ARG; ws =
 * kd_seg_ohem_ws_bytes(B * HW) bytes, 8-byte aligned, else KD_ERR_WORKSPACE / KD_ERR_ALIGN.  A refused call writes nothing. */
size_t kd_seg_ohem_ws_bytes(int64_t npix);
int kd_seg_ohem_fwd_bwd(const float* zs, const float* zt, const int64_t* target, const float* class_w, int ignore_index, float T,
                        float alpha, float gscale, const float* gscale_dev, float lambda, int64_t min_kept, int64_t min_divisor,
                        float* vals, int64_t* counts_out, float* dzs, float* nll_out, uint8_t* keep_out, int B, int NC, int HW,
                        void* ws, size_t ws_bytes, void* stream);
size_t kd_mse_ws_bytes(int64_t n);
int kd_mse_fwd_bwd(const float* a, const float* b, int64_t n, float gcoef, const float* gscale_dev, float* loss,
                   float* da, void* ws, size_t ws_bytes, void* stream);
/* value of the KD objective from its parts: total = ce_kl[0] + ckl * ce_kl[1] + beta * (mse_c[0] + mse_l[0]) (either MSE may be
 * NULL = 0), every operation rounded to fp32 in that order */
int kd_kd_total(const float* ce_kl, const float* mse_c, const float* mse_l, float ckl, float beta, float* total, void* stream);
/* the same objective with fewer launches: kd_mse_partial leaves the per-block sums of (a-b)^2 in a slab of kd_mse_slab_blocks(n)
 * floats (and writes da = gcoef * (a-b) when da != NULL); kd_kd_objective_final reduces two such slabs to out[0], out[1] = the two
 * feature MSEs and out[2] = the total (rounding order of kd_kd_total) */
int64_t kd_mse_slab_blocks(int64_t n);
int kd_mse_partial(const float* a, const float* b, int64_t n, float gcoef, float* da, float* slab, void* stream);
int kd_kd_objective_final(const float* ce_kl, const float* slab_c, int64_t n_c, const float* slab_l, int64_t n_l, float ckl, float beta,
                          float* out, void* stream);
/* The opt-in channel-wise distillation feature term (csrc/kd_loss_cwd.hip; Shu et al., ICCV 2021) of two NHWC
 * feature matrices s, t [B*HW, C] (row-major, what ops.nhwc_view yields), temperature tau:
 *   phi(X)[b,c,i] = exp(X[b,i,c]/tau) / sum_j exp(X[b,j,c]/tau)   over the HW rows i, j of image b: a softmax down each COLUMN,
 *   val[0] = tau^2 / (B*C) * sum_{b,c} sum_i phi(t) (log phi(t) - log phi(s))     (not scaled by gcoef),
 *   ds     = k * (phi(s) - phi(t)),  k = gcoef * (gscale_dev ? gscale_dev[0] : 1) formed once in fp32 (ds NULL: forward only); the
 *   caller passes gcoef = tau / (B*C) times whatever it folds in.
 * Log-probabilities are x/tau - max - log(sum exp(x/tau - max)), never the logarithm of a probability; a position whose phi(t)
 * underflows adds exactly 0.  stats_out (may be NULL; for tests): [B][C][4] = the column maximum M of s/tau and log(sum exp(s/tau - M)) (the
 * log-sum-exp of the column is their sum, which the kernel never forms), then the same two of t/tau.  s and t go through the same instruction sequence: identical bits in both give val[0] == 0 and ds == +-0 exactly (s == t as
 * pointers is allowed).  An image's statistics and ds rows depend on that image's rows and k alone (a B = 1 call on image b
 * reproduces their bits).  C % 4 != 0, C > 512, HW < 1 or B < 1 is KD_ERR_SHAPE; a tau that is not finite and > 0 or a NULL s / t /
 * val / ws is KD_ERR_ARG; s, t, ds or ws not 16-byte aligned is KD_ERR_ALIGN; ws = kd_feat_cwd_ws_bytes(B, HW, C) bytes, else
 * KD_ERR_WORKSPACE.  Three launches (column statistics per row chunk; chunk join + the point-wise pass; the value's final sum in
 * double), 5 sweeps of a map with the gradient and 4 without, no atomics, no host reads: bit-identical from call to call. */
size_t kd_feat_cwd_ws_bytes(int B, int HW, int C);
int kd_feat_cwd_fwd_bwd(const float* s, const float* t, int B, int HW, int C, float tau, float gcoef, const float* gscale_dev,
                        float* val, float* ds, float* stats_out, void* ws, size_t ws_bytes, void* stream);
/* The opt-in pair-wise distillation feature term in Gram form (csrc/kd_loss_pair.hip; Liu et al., CVPR 2019) of two
 * NHWC feature matrices s [B*HW, Cs] and t [B*HW, Ct] (row-major, what ops.nhwc_view yields), n = HW positions per image:
 *   r_i = sqrt(sum_c x_ic^2), xh_i = x_i / r_i if r_i > 1e-12 else 0 (such a row also receives no gradient),  a_ij = xh_i . xh_j,
 *   L_b = 1/n^2 sum_ij (a^S_ij - a^T_ij)^2 = 1/n^2 (|Gss|_F^2 - 2 |Gts|_F^2 + |Gtt|_F^2),  Gss = Sh^T Sh, Gts = Th^T Sh, Gtt = Th^T Th,
 *   val[0] = PAIR = 1/B sum_b L_b                       (not scaled by gcoef),
 *   ds     = k * (gh_i - xh_i (xh_i . gh_i)) / r_i,  gh = Sh Gss - Th Gts,  k = gcoef * (gscale_dev ? gscale_dev[0] : 1) formed once in
 *   fp32 (ds NULL: forward only); the caller passes gcoef = 4 / (B n^2) times whatever it folds in.
 * img_vals_out (may be NULL; for tests): the B per-image values L_b.  The n x n affinities are never formed: O(n C^2) work on the exact
 * fp32 MFMA (a k-ordered fp32 fma chain), sqrtf and a true division for the norms.  kd_feat_pair_slices(B, HW): the row slices an image
 * is cut into for the Gram pass (1 once B fills the device; a function of B and HW alone; 0 for an unsupported B or HW).  Launches: Gram
 * partials per (image, slice) to a slab; the slice join with sum gss^2 - 2 gts^2 + gtt^2 in double; the per-image values and their
 * mean in double in one block; with ds the gradient pass ([Gss; Gts] resident in LDS when (Csp + Ctp) * Csp * 4 <= 128 KiB, widths
 * padded to 32; streamed otherwise).  No atomics, no host reads: capturable, bit-identical from call to call.  s and t go through
 * the same instruction sequence: identical bits in both (s == t as pointers is allowed) give val[0] == 0 and ds == +-0 exactly.
 * The value and the gradient are differences of quantities of order 1 (the cancellation note).
 * A width that is no multiple of 4 or outside 4..256, HW < 1, HW > 2^30 or B < 1 is KD_ERR_SHAPE; a NULL s / t / val / ws or a gcoef that is not
 * finite is KD_ERR_ARG; s, t, ds or ws not 16-byte aligned is KD_ERR_ALIGN; ws = kd_feat_pair_ws_bytes(B, HW, Cs, Ct) bytes (0 for an
 * unsupported shape), else KD_ERR_WORKSPACE.  A refused call launches and writes nothing. */
size_t kd_feat_pair_ws_bytes(int B, int HW, int Cs, int Ct);
int kd_feat_pair_slices(int B, int HW);
int kd_feat_pair_fwd_bwd(const float* s, const float* t, int B, int HW, int Cs, int Ct, float gcoef, const float* gscale_dev,
                         float* val, float* ds, float* img_vals_out, void* ws, size_t ws_bytes, void* stream);
/* The opt-in intra-class feature variation distillation feature term (csrc/kd_loss_ifv.hip; Wang et al., ECCV 2020)
 * of two NHWC feature matrices s [B*HW, Cs] and t [B*HW, Ct] under the label map target [B*HW] (int64, the maps' resolution).  Pixel i of
 * image b is kept when target != ignore_index and 0 <= target < NC; K_b kept pixels, N_bc of class c.  For X in {s, t}, per image:
 *   r_i = sqrt(sum_k x_ik^2), xh_i = x_i / r_i if r_i > 1e-12 else 0,  m_c = 1/N_bc sum_{i kept, y_i = c} x_i,
 *   mh_c = m_c / |m_c| if |m_c| > 1e-12 else 0,  s_i = xh_i . mh_{y_i},
 *   L_b = 1/K_b sum_{i kept} (sS_i - sT_i)^2 (0 for K_b = 0; the image still counts in B),  val[0] = IFV = 1/B sum_b L_b (not scaled),
 *   ds_j = k * (w_j (mh_c - s_j xh_j) / r_j [0 for r_j <= 1e-12] + D_c / N_bc), c = y_j, w_i = (sS_i - sT_i) / K_b,
 *          D_c = sum_{i kept, y_i = c} w_i (xh_i - s_i mh_c) / |m_c| (0 for |m_c| <= 1e-12), everything from s; 0 for a row that is not
 *          kept; k = gcoef * (gscale_dev ? gscale_dev[0] : 1) formed once in fp32 (ds NULL: forward only).  That is k * (B/2) * dIFV/ds:
 *          the caller passes gcoef = 2 / B times whatever it folds in.  A kept all-zero row still receives D_c / N_bc.
 * img_vals_out (may be NULL; for tests): the B per-image values L_b.  kd_feat_ifv_slices(B, HW): the row slices an image is cut into
 * (a function of B and HW alone; 0 for an unsupported B or HW).  Launches: per-class channel sums per (image, slice, map) in per-thread
 * LDS accumulators; the slice join in double to m, |m|, mh, N_bc; the similarity pass (8 lanes per row, {1/r, sS, w} per pixel to the
 * workspace); with ds the class sums of w_i xh_i; the per-image join in double (L_b, D_c / N_bc); the mean over images in one block;
 * with ds the point-wise gradient pass.  No floating-point atomics, no host reads: capturable, bit-identical from call to call.  s and t
 * go through the same instruction sequence: identical bits in both (s == t as pointers is allowed) give val[0] == 0 and ds == +-0.
 * A width that is no multiple of 4 or outside 4..256, NC outside 2..16, HW < 1, HW > 2^30 or B < 1 is KD_ERR_SHAPE; a NULL s / t /
 * target / val / ws or a gcoef that is not finite is KD_ERR_ARG; s, t, ds or ws not 16-byte aligned (target: 8) is KD_ERR_ALIGN;
 * ws = kd_feat_ifv_ws_bytes(B, HW, Cs, Ct, NC) bytes (0 for an unsupported shape), else KD_ERR_WORKSPACE.  A refused call launches and
 * writes nothing. */
size_t kd_feat_ifv_ws_bytes(int B, int HW, int Cs, int Ct, int NC);
int kd_feat_ifv_slices(int B, int HW);
int kd_feat_ifv_fwd_bwd(const float* s, const float* t, const int64_t* target, int ignore_index, int B, int HW, int Cs, int Ct, int NC,
                        float gcoef, const float* gscale_dev, float* val, float* ds, float* img_vals_out, void* ws, size_t ws_bytes,
                        void* stream);
/* pred[B*HW] = argmax over the NC (1..4) classes, first maximum wins; conf[M*M] (ACCUMULATED into) counts a pixel at [t, argmax]
 * when t != ignore_index and 0 <= t < M and argmax < M: M (1..4) is the width of the matrix, independent of NC.  Either of conf
 * and pred may be NULL; target NULL: no counting. */
int kd_argmax_confusion(const float* logits, const int64_t* target, int ignore_index, uint64_t* conf,
                        int64_t* pred, int B, int NC, int M, int HW, void* stream);
/* kd_argmax_confusion for 1 <= NC <= 16 classes and a matrix width 1 <= M <= 16 (else KD_ERR_SHAPE, nothing written): the same
 * arguments, counting rule, ties (the lowest class index wins) and NaN behaviour (a NaN never beats the running maximum); 256 LDS
 * counters per block, accumulated into conf as 64-bit integers.  kd_argmax_confusion keeps its own limits of 4. */
int kd_argmax_confusion16(const float* logits, const int64_t* target, int ignore_index, uint64_t* conf,
                          int64_t* pred, int B, int NC, int M, int HW, void* stream);
int kd_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                  float eps, float weight_decay, int step, float ginv, void* stream);
/* hipGraph-replay-safe form: state = device float[4] {lr, step, 1-beta1^step, sqrt(1-beta2^step)}; the call
 * advances state[1] on the device and refreshes the bias corrections before the update. */
int kd_adamw_step_dev(float* p, const float* g, float* m, float* v, int64_t n, float* state, float beta1,
                      float beta2, float eps, float weight_decay, float ginv, void* stream);
/* Global-norm gradient clipping on the device.
 * kd_grad_sumsq_partials: ws[b] (double) = the sum of g[i]^2 over the elements block b of the launch owns, for
 * b < kd_grad_sumsq_ws_bytes(n) / 8.  256 threads, one float4 per thread and iteration, at most 2048 blocks; fp32 inside a thread
 * and a wave, double from there on; fixed summation order, no atomics: the same input gives the same bits on every run and on
 * every replay of a captured graph.  n must be a positive multiple of 4 (KD_ERR_ARG; pad with zeros, as the flat gradient buffer
 * of kdrt.optim.FlatParams is), g 16-byte and ws 8-byte aligned (KD_ERR_ALIGN), ws_bytes >= kd_grad_sumsq_ws_bytes(n)
 * (KD_ERR_WORKSPACE).  A refused call launches nothing.
 *
 * kd_adamw_step_clip_dev: kd_adamw_step_dev with the gradient clipped to a global L2 norm of max_norm.  `state` is the same
 * float[4]; `clip_state` is a second device float[4] {grad_norm, gscale, skipped_steps, last_step_finite}, of which the caller
 * zeroes skipped_steps once.  Three launches (partials, a one-block tick, the update), no host synchronisation:
 *   grad_norm = ginv * sqrt(sum g^2)         the norm of the gradient the optimiser applies (the rank average when ginv = 1/world)
 *   clip_coef = min(1, max_norm / (grad_norm + 1e-6))                       torch.nn.utils.clip_grad_norm_'s formula, in fp32
 *   gscale    = ginv * clip_coef             one fp32 product: bit-equal to ginv when nothing is clipped, and the update is then
 *                                            bit-identical to kd_adamw_step_dev's
 * and the update uses g[i] * gscale where kd_adamw_step_dev uses g[i] * ginv.  g itself is only read: after the call it still
 * holds the unclipped gradients (under data parallelism the summed ones).
 * A non-finite grad_norm (an inf or NaN anywhere in g, or a sum of squares beyond the fp32 range) SKIPS the step: p, m, v and
 * state keep their bits -- the step count does not advance --, skipped_steps goes up by one, last_step_finite is 0, gscale is 0
 * and grad_norm holds the non-finite value.  This departs on purpose from clip_grad_norm_(error_if_nonfinite=False), which would
 * scale by NaN and leave NaN in every parameter.
 * max_norm must be finite and > 0, n a positive multiple of 4 (KD_ERR_ARG); p, g, m, v 16-byte and ws 8-byte aligned
 * (KD_ERR_ALIGN); ws_bytes >= kd_grad_sumsq_ws_bytes(n) (KD_ERR_WORKSPACE).  A refused call launches nothing. */
size_t kd_grad_sumsq_ws_bytes(int64_t n);
int kd_grad_sumsq_partials(const float* g, int64_t n, void* ws, size_t ws_bytes, void* stream);
int kd_adamw_step_clip_dev(float* p, const float* g, float* m, float* v, int64_t n, float* state, float* clip_state, void* ws,
                           size_t ws_bytes, float beta1, float beta2, float eps, float weight_decay, float ginv, float max_norm,
                           void* stream);
/* Parameter groups and an EMA weight copy in the same device step.
 * kd_adamw_step_groups_dev: kd_adamw_step_dev (clip_state == NULL and ws == NULL) or kd_adamw_step_clip_dev (both given, same
 * clip_state, workspace, norm, skip rule and bits) where every float4 of the buffer takes lr and weight_decay from its segment:
 *   seg_end[n_seg]   ascending segment ends in float4 units, the last = n / 4 (a padding element belongs to the tensor before it)
 *   seg_group[n_seg] the group of each segment, < n_groups
 *   group_state      device float[n_groups][2] = (lr, weight_decay) per group; rewrite the lr entries between graph replays
 * seg_end / seg_group are device int32 arrays; seg_end_host / seg_group_host are the caller's host copies of the same values, which
 * this call validates (it never reads device memory on the host).  Every workgroup copies the table into LDS and a thread searches
 * it when its float4 leaves the segment of its previous iteration; at most 4096 segments (KD_ERR_SHAPE beyond: merge neighbouring
 * tensors of one group).  Cost of the copy: workgroups x n_seg x 8 bytes of (mostly L2) reads per step, 1 MB at the 64 segments of
 * the published models with 2048 workgroups, 64 MB at 4096 segments -- more than the update's own traffic there, so keep tables
 * short.  `state` is the same float[4]; state[0] (the single learning rate) is neither read nor written.
 * beta1, beta2, eps are shared by all groups.  Per-element arithmetic is kd_adamw_step_clip_dev's, expression for expression: with
 * one segment the results are bit-identical to kd_adamw_step_dev / kd_adamw_step_clip_dev at that lr and weight_decay.
 * EMA (ema == NULL and ema_state == NULL: off): ema is a float[n] copy of the weights, ema_state a device float[2] that the tick
 * kernel writes on every applied step:
 *   ema_state[0] = d_t = ema_warmup ? min(ema_decay, (1 + t) / (10 + t)) : ema_decay     t = the step count after the tick; fp32
 *   ema_state[1] = 1 - d_t                                                               operations, each rounded once
 *   ema[i] = fmaf(d_t, ema[i], ema_state[1] * p_new[i])      the product rounded to fp32, then one fused multiply-add
 * When ema_state[1] == 0 (d_t = 1) ema is not touched; when d_t == 0 p_new is stored as it is: both exact, bit for bit.
 * A skipped step (non-finite gradient norm with clipping on) leaves p, m, v, ema, ema_state and the step count unchanged.
 * n a positive multiple of 4 with n / 4 < 2^31, ema_decay in [0, 1], max_norm finite and > 0 when clipping, ends ascending from
 * above 0 to n / 4, group indices in range, ema with ema_state and clip_state with ws (KD_ERR_ARG); p, g, m, v, ema 16-byte and
 * ws 8-byte aligned (KD_ERR_ALIGN); ws_bytes >= kd_grad_sumsq_ws_bytes(n) when clipping (KD_ERR_WORKSPACE).  A refused call
 * launches nothing. */
int kd_adamw_step_groups_dev(float* p, const float* g, float* m, float* v, int64_t n, float* state, const int* seg_end,
                             const int* seg_group, const int* seg_end_host, const int* seg_group_host, int n_seg,
                             const float* group_state, int n_groups, float* ema, float* ema_state, float ema_decay, int ema_warmup,
                             float* clip_state, void* ws, size_t ws_bytes, float beta1, float beta2, float eps, float ginv,
                             float max_norm, void* stream);
/* Gradient accumulation over micro-batches: the backward kernels overwrite the flat gradient buffer, the running sum lives in
 * `accum`, a second buffer of the same length.
 *   fold 0: accum[i] = accum[i] + grad[i]; grad is only read                       (micro-batches 1 .. k-1 of a cycle)
 *   fold 1: grad[i] = accum[i] + grad[i] and accum[i] = +0.0f in the same pass     (micro-batch k: the AdamW entry points above
 *           then step on the summed gradient with ginv / k, and the next cycle -- or the next replay of a captured graph --
 *           starts from zeros without a memset)
 * One fp32 add per element with accum as the left operand: the bits of torch's `accum + grad`.  One launch: 256 threads, one
 * float4 per thread and iteration, at most 2048 blocks, the last n % 4 elements one by one; any n >= 0, n == 0 returns 0 without
 * a launch.  accum == grad, a null pointer with n > 0, n < 0 or fold outside {0, 1}: KD_ERR_ARG; accum and grad 16-byte aligned
 * (KD_ERR_ALIGN; every tensor, and so every gradient bucket, of kdrt.optim.FlatParams starts on such a boundary).  A refused call
 * launches nothing. */
int kd_grad_accumulate(float* accum, float* grad, int64_t n, int fold, void* stream);

/* ---- inference-mode block fusion (csrc/kd_block.hip) ------------------------------------------------------------------
 * The tail of an InvertedResidual (reference camera_encoder.py:30-42: depthwise 3x3 + BN + ReLU6, project 1x1 + BN, + x) or a
 * whole DWSeparableConv (fusion_module.py:25-34) in ONE kernel for the eval-mode / no-grad forward: every BatchNorm is an
 * (scale, shift) pair known before the launch, so the depthwise output -- the widest tensor of the block -- never goes to HBM.
 *   out[B*Ho*Wo, Cout] = pact(bn_p(conv1x1(dact(bn_d(dwconv3x3_stride(iact(bn_i(x)))))))) (+ res)
 * x: [B,H,W,Ch] NHWC (isc == NULL: used as it is), wd: [Ch][9], wp: [Cout][Ch]; split bf16x3 GEMM arithmetic; bit-identical to
 * kd_dwconv3x3_fwd followed by kd_pwconv_gemm(pro 1, epi 5).  Shapes: Ch a multiple of 32; stride 1 with Cout 32 / 64 / 128,
 * stride 2 with Cout 64 / 128 (kd_dw_pw_infer_supported); anything else returns KD_ERR_SHAPE. */
int kd_dw_pw_infer_supported(int Ch, int Cout, int stride);
int kd_dw_pw_infer(const float* x, const float* isc, const float* ish, int iact, const float* wd, const float* dsc, const float* dsh,
                   int dact, const float* wp, const float* pbias, const float* psc, const float* psh, int pact, const float* res,
                   int64_t ldres, float* out, int64_t ldo, int B, int H, int W, int Ch, int stride, int Cout, void* stream);

/* The WHOLE InvertedResidual (expand 1x1 + BN + act, depthwise 3x3 + BN + act, project 1x1 + BN + act, + res) in one kernel: the 6x
 * hidden tensor is neither written nor read.  The block-input halo tile of a workgroup is read once and kept as bf16x3 MFMA
 * fragments; per 32 hidden channels the expand GEMM is recomputed over the 3x3 halo on the matrix pipe.
 *   out[B*Ho*Wo, Cout] = pact(bn_p(conv1x1_p(dact(bn_d(dwconv3x3_stride(eact(bn_e(conv1x1_e(x) + ebias))))) + pbias)) (+ res)
 * x: dense [B,H,W,Cin] NHWC of finished values, we: [Ch][Cin], ebias: [Ch] or NULL, esc / esh: [Ch] (required), the rest as
 * kd_dw_pw_infer.  Split bf16x3 GEMM arithmetic; bit-identical to kd_pwconv_gemm(pro 0, epi 0) followed by kd_dw_pw_infer.
 * Shapes (kd_block_infer_supported): Ch a multiple of 32 with (Cin 32, stride 2, Cout 64) or (Cin 64, stride 1, Cout 64);
 * anything else returns KD_ERR_SHAPE. */
int kd_block_infer_supported(int Cin, int Ch, int Cout, int stride);
int kd_block_infer(const float* x, const float* we, const float* ebias, const float* esc, const float* esh, int eact, const float* wd,
                   const float* dsc, const float* dsh, int dact, const float* wp, const float* pbias, const float* psc, const float* psh,
                   int pact, const float* res, int64_t ldres, float* out, int64_t ldo, int B, int H, int W, int Cin, int Ch, int stride,
                   int Cout, void* stream);

/* ---- bf16-storage INFERENCE path (csrc/kd_bf16.hip; BASELINE.json configs[1]) -----------------------------------------
 * A second mode beside the fp32 contract: eval forward only.  Activations are bf16 NHWC matrices [M][C], already
 * normalised + activated; every entry point is one whole unit conv -> fma(raw, sc, sh) -> act (+ residual) -> bf16, with
 * fp32 accumulation; weights / coefficient vectors are fp32.  Replaces, in eval mode: the stem (camera_encoder.py:63-67),
 * depthwise 3x3 (:30-35, fusion_module.py:25-27,78), every 1x1 conv / Conv1d(k=1) (camera_encoder.py:24,39,
 * fusion_module.py:12,29, lidar_encoder.py:26-34 incl. the scatter-max of :85-96), the FPN resize + sum (:58-63) and the
 * classifier (:170).  kd_bf16_pwconv: a_kind 0 = A bf16, 1 = A fp32 (rounded on load), 3 = A are LiDAR points [M][4] and
 * layer 0 (l0w [K][4], l0b, sc0, sh0, act0) is recomputed; epi 0 = C bf16 (+ res bf16), 4 = scatter-max of the
 * non-negative result into the zero-filled fp32 grid [cells][ldgrid] by cell[m] (< 0: skipped).  K and N are multiples of 8,
 * K <= 1024 (multiples of 32 run the full-tile kernels; others a zero-padded, column-masked tile).  kd_bf16_stem: Cout in
 * {8, 16, 24, 32, 40}.  kd_bf16_dwconv3x3: C a multiple of 8, C <= 1024. */
int kd_bf16_stem(const float* x_nchw, const float* w, const float* sc, const float* sh, int act, void* y, int B, int Cin, int H,
                 int W, int Cout, void* stream);
int kd_bf16_dwconv3x3(const void* x, const float* w, const float* sc, const float* sh, int act, void* y, int B, int H, int W,
                      int C, int stride, void* stream);
int kd_bf16_pwconv(const void* A, int64_t lda, int a_kind, const float* W, const float* bias, const float* esc, const float* esh,
                   int act, void* C, int64_t ldc, const void* res, int64_t ldres, int epi, int64_t M, int K, int N,
                   const int* m_dev, const float* l0w, const float* l0b, const float* sc0, const float* sh0, int act0,
                   const int* cell, float* grid, int64_t ldgrid, void* stream);
int kd_bf16_bilinear_sum(const void* in0, int H0, int W0, const void* in1, int H1, int W1, const void* in2, int H2, int W2,
                         void* out, int B, int Ho, int Wo, int C, void* stream);
int kd_bf16_cls_conv(const void* x, const float* w, const float* b, float* logits_nchw, int64_t M, int HW, int Cin, int NC,
                     void* stream);
/* weighted-fusion tail (fusion_module.py:115-120): h [M][C] bf16 = relu(attention.0(cat)); out [M][C] bf16 =
 * w_0 * cat[:, :C] + w_1 * cat[:, C:], (w_0, w_1) = softmax(h . w2^T + b2); w2 [2][C], b2 [2] fp32. */
int kd_bf16_weighted_tail(const void* h, const void* cat, const float* w2, const float* b2, void* out, int64_t M, int C,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KD_HIP_H */
