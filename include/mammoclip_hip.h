/*
 * mammoclip_hip.h -- C ABI of libmammoclip_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * Mammo-CLIP image<->text contrastive pre-training hot path.
 *
 * The reference (batmanlab/Mammo-CLIP) has no FFI of its own: its hot path bottoms out in torch
 * operators (conv2d / batch_norm / linear / matmul / cross_entropy ...).  Every entry point below
 * replaces one such operator call-site (or a fused group of them) and cites it as
 *   [ref: <file>:<lines>]  relative to  src/codebase/breastclip/ .
 * The host-side mirror of the reference's Python API (build_model / build_loss / BreastClip ...) lives in
 * mammo_clip_amd/breastclip/ and binds these symbols with ctypes.
 *
 * Conventions
 *   - plain pointers and sizes only; all pointers are DEVICE pointers unless stated otherwise
 *   - bf16 tensors are raw uint16 bit patterns; activations are row-major [rows, channels] (NHWC),
 *     channels % 8 == 0, base pointers 16-byte aligned
 *   - the 16-bit storage / MFMA operand type is a property of the library BUILD: libmammoclip_hip.so holds bf16
 *     (default), libmammoclip_hip_f16.so (compiled from the same sources with -DMC_F16) holds IEEE f16 -- the
 *     reference's AMP dtype [ref: trainer.py:271-278] -- behind the SAME symbols: wherever this header says "bf16" /
 *     mc_bf16, the f16 build reads and writes f16 bit patterns.  mc_storage_is_f16() tells which one a process loaded.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous
 *   - return 0 on success, non-zero on error; mc_last_error() gives the message (thread-local)
 *   - no hidden allocation: workspaces / partial buffers are caller-provided
 */
#ifndef MAMMOCLIP_HIP_H
#define MAMMOCLIP_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef uint16_t mc_bf16;

const char* mc_last_error(void);
int mc_version(void);
int mc_storage_is_f16(void);   /* 0: bf16 build, 1: f16 build (see Conventions) */

/* ------------------------------------------------------------------------------------------------
 * bf16 MFMA GEMM:  C[M,N] (+)= alpha * op(A)[M,K] . op(B)[K,N] + bias[N]  -> act -> + R
 * [ref: model/modules/efficientnet_custom.py:104,122,283 (1x1 convs _expand_conv/_project_conv/_conv_head),
 *       model/modules/text_encoder.py:48 (BertModel linears and attention matmuls),
 *       and their autograd backward (dgrad: b_kmajor, wgrad: a_kmajor+b_kmajor+split-K atomics)]
 * a_kmajor = 0: A[m*lda + k]   1: A[k*lda + m]        b_kmajor = 0: B[n*ldb + k]   1: B[k*ldb + n]
 * batch index z -> (b1, b2) = (z / nb2, z % nb2); operand offsets b1*s?1 + b2*s?2 (elements).
 * Prologue (fused BN + SiLU (+ SE gate) on the streamed operand, [ref: efficientnet_custom.py:110-119]):
 *   pro_operand 1 = A (k-contiguous: row = pixel, k = channel), 2 = B (k-major: k = pixel, n = channel)
 *   v' = silu(v*pro_scale[c] + pro_shift[c]) * pro_gate[(pixel / pro_rows_per_img) * pro_nch + c]
 * stat_partials (optional, bf16 output only): float[rows][2][N] with rows = mc_gemm_stat_rows();
 *   row r holds the column sums / sums of squares of the C rows handled by workgroup-row r.
 */
typedef struct mc_gemm_args {
    const mc_bf16* A;
    const mc_bf16* B;
    void* C;
    long long M, K;
    int N;
    long long lda, ldb, ldc;
    int a_kmajor, b_kmajor;
    int c_f32, c_atomic;
    int splits;
    int batch, nb2;
    long long sA1, sA2, sB1, sB2, sC1, sC2;
    const float* bias;
    long long bias_stride1;
    int act;                 /* 0 none, 1 erf-GELU */
    const mc_bf16* R;
    long long ldr;
    float alpha;             /* 0 is read as 1 */
    int pro_operand;
    const float* pro_scale;
    const float* pro_shift;
    const float* pro_gate;
    long long pro_rows_per_img;
    int pro_nch;
    float* stat_partials;
    int max_grid_m;          /* 0 = default */
    float* splitk_ws;        /* optional float[splits*M*N]: split-K partial tiles are combined by a second kernel
                                (C = sum, or C += sum when c_atomic) instead of per-element atomics */
    /* grouped split-K (weight gradient of a conv whose input carries a per-image, per-channel factor, e.g. the SE gate):
     * the reduction index is cut at multiples of split_group_rows (rows per image), split_sub splits per group
     * (splits = groups * split_sub), and partial s is multiplied by split_scale[s / split_sub][column] when the
     * partials are combined:  dW[n][k] = sum_img gate[img][k] * sum_{m in img} dY[m][n] * A[m][k]  -- no prologue needed */
    long long split_group_rows;
    int split_sub;
    const float* split_scale;
    /* fp8 operands (BASELINE config #5: fp8 weights / activations for the pointwise convolutions,
     * efficientnet_custom.py:104,122,283): A and B hold OCP e4m3 bytes (gfx950's fp8, NOT the fnuz form), lda / ldb /
     * strides in elements (= bytes), K, lda, ldb multiples of 16; plain NT layout, bf16 output, fp32 accumulation
     * (v_mfma_f32_16x16x32_fp8_fp8).  The product of the two per-tensor dequantisation scales is passed in alpha and/or
     * alpha_dev (device scalar, multiplied onto alpha; produced by mc_quant_fp8_bf16 without a host round trip).
     * alpha_dev is read by the 256 x 256 NT kernel of gemm256.hip only (with or without ab_fp8): a problem that carries it
     * and is not served by that kernel -- any other layout, fp32 output, the TN weight-gradient kernel -- is an error. */
    int ab_fp8;
    const float* alpha_dev;
} mc_gemm_args;
int mc_gemm_bf16(const mc_gemm_args* args, void* stream);
/* rows of the stat_partials buffer the launch described by `args` (the COMPLETE argument block) will write */
int mc_gemm_stat_rows(const mc_gemm_args* args);
/* which tile kernel serves `args`: 256 = the 256 x 256 x 64 direct-to-LDS kernel (gemm256.hip: plain NT operands, bf16
 * output, enough well-filled tiles for the 256 CUs), 128 = the 128-row tile family (gemm.hip) */
int mc_gemm_tile_config(const mc_gemm_args* args);
/* Weight-gradient (TN) problems -- a_kmajor = b_kmajor = 1, fp32 output, plain operands, K = the long pixel / token
 * reduction [ref: autograd backward of efficientnet_custom.py:104,122,283, text_encoder.py:47-49] -- run on the
 * 256 x 256 x 64 transpose-read kernel of gemm256_tn.hip when mc_gemm256_tn_eligible() says so (mc_gemm_bf16 routes them
 * itself).  mc_gemm256_tn_splits: the number of K splits that kernel wants (splitk_ws = float[splits*M*N]); with
 * group_rows > 0 (grouped form, split_group_rows) the number of sub-splits per group (split_sub). */
int mc_gemm256_tn_eligible(const mc_gemm_args* args);
int mc_gemm256_tn_splits(long long m, long long n, long long k, long long group_rows);

/* fp8 operand preparation (BASELINE config #5; OCP e4m3 as implemented by gfx950).
 * mc_amax_bf16:       amax[0] = max(amax[0], max |x|)   (caller zero-fills amax; integer atomic, deterministic)
 * mc_quant_fp8_bf16:  y = e4m3(clamp(x * 448 / amax_in[0], +-448));  scale_out[0] = amax_in[0] / 448 (the dequantisation
 *                     scale, optional);  amax_next[0] = max(amax_next[0], max |x|) (optional: delayed scaling measures the
 *                     tensor it converts);  n % 8 == 0, contiguous.
 *                     The scale is finite for every finite amax_in > 0 (below 2^-100 amax and x are both multiplied by 2^64
 *                     before the division, which changes no rounding): finite x never gives a NaN code, +-amax gives +-448.
 *                     amax_in = 0 -> scale 1 and scale_out 1;  NaN amax_in or NaN x -> NaN code (0x7f / 0xff). */
int mc_amax_bf16(const mc_bf16* x, long long n, float* amax, void* stream);
int mc_quant_fp8_bf16(const mc_bf16* x, long long n, const float* amax_in, unsigned char* y, float* scale_out,
                      float* amax_next, void* stream);

/* Row-streaming variant for the HBM-bound 1x1 convolutions (small weight matrix, millions of pixels):
 *   C[M,N] = pro(X)[M,K] . W[N,K]^T (+ R);  N <= 256, K <= 384 (mc_gemm_rows_supported), bf16 in/out.
 * Weights live in LDS for the whole launch, each workgroup writes complete, contiguous output rows.
 * The data gradient of a 1x1 conv is the same call with the transposed weight (mc_cast_transpose_f32_bf16).
 * stat_partials (optional): float[mc_gemm_rows_blocks(args)][2][N] column sums / sums of squares of C. */
typedef struct mc_gemm_rows_args {
    const mc_bf16* X;
    long long M;
    int K;
    long long ldx;
    const mc_bf16* W;
    int N;
    long long ldw;
    mc_bf16* C;
    long long ldc;
    const mc_bf16* R;
    long long ldr;
    const float* pro_scale;
    const float* pro_shift;
    const float* pro_gate;
    long long pro_rows_per_img;
    float* stat_partials;
    const float* bias;       /* optional float[N], added to every output row (after the statistics, with the residual) */
    /* Fused elementwise epilogues for the DATA GRADIENT of an MBConv projection conv (round 3).  G = X.W^T is d loss / d (gated
     * activation) [ref: efficientnet_custom.py:117-122 backwards]; it is rounded to bf16 like the stored tensor would be but never
     * goes to memory (N <= 256, K <= 128, no residual / bias / statistics / prologue):
     *   epi_mode 1: the five per-image sums of mc_bnact_se_sums over (epi_x, G) -> epi_sums [5][n_img][N]; C is not written;
     *   epi_mode 2: mc_bnact_bwd_apply on (epi_x, G): C = coef0*dz + coef1*epi_x + coef2,
     *               dz = (G * epi_mul[img] + epi_add[img] * epi_add_scale) * silu'(epi_x * epi_scale + epi_shift).
     * epi_x [M,N] (leading dimension epi_ldx) = the depthwise conv output in front of BatchNorm1; epi_rows_per_img % 16 == 0. */
    int epi_mode;
    const mc_bf16* epi_x;
    long long epi_ldx;
    long long epi_rows_per_img;
    const float* epi_scale;
    const float* epi_shift;
    const float* epi_mean;
    const float* epi_invstd;
    const float* epi_coef;   /* [3][N] (mc_bn_bwd_finalize) */
    const float* epi_mul;    /* [n_img][N] */
    const float* epi_add;    /* [n_img][N] */
    float epi_add_scale;
    float* epi_sums;         /* epi_mode 1: [5][n_img][N] */
    float* epi_ws;           /* epi_mode 1: float[mc_gemm_rows_epi_ws_floats(args)] */
} mc_gemm_rows_args;
int mc_gemm_rows_supported(int n, int k);
long long mc_gemm_rows_epi_ws_floats(const mc_gemm_rows_args* args);
/* can mc_gemm_rows_bf16 run the epilogue form epi_mode (1 / 2) of an [M, K] x [N, K]^T data gradient with rows_per_img rows per
 * image?  (N <= 256, K <= 128, whole 16-row groups per image, at most one image boundary per wave range) */
int mc_gemm_rows_epi_supported(long long M, int N, int K, long long rows_per_img, int epi_mode);
int mc_gemm_rows_blocks(const mc_gemm_rows_args* args);     /* persistent workgroups of the launch = rows of stat_partials */
int mc_gemm_rows_bf16(const mc_gemm_rows_args* args, void* stream);

/* Streaming weight gradient of the same layers: dW[N,K] (fp32) (+)= dY[M,N]^T . pro(X)[M,K]; both operands are
 * staged row-major and read with gfx950's LDS transpose-read (ds_read_b64_tr_b16); no atomics.
 * ws: float[mc_wgrad_rows_blocks(M) * N * K] scratch (per-workgroup partials, reduced by a second kernel). */
typedef struct mc_wgrad_rows_args {
    const mc_bf16* dY;
    int N;
    long long lddy;
    const mc_bf16* X;
    int K;
    long long ldx;
    long long M;
    float* dW;               /* [N, K] contiguous */
    float* ws;
    int accumulate;
    const float* pro_scale;  /* prologue on X: silu(x*scale[k] + shift[k]) * gate[(m / rows_per_img) * K + k] */
    const float* pro_shift;
    const float* pro_gate;
    long long pro_rows_per_img;
} mc_wgrad_rows_args;
int mc_wgrad_rows_supported(int n, int k);
int mc_wgrad_rows_blocks(long long m);
int mc_wgrad_rows_bf16(const mc_wgrad_rows_args* args, void* stream);
/* Round 5 -- BOTH gradients of such a 1x1 convolution e = x W^T from ONE pass over the upstream gradient dY [M, N] (the expand
 * conv of an MBConv block: dY is the widest tensor of the block, 6x its input) [ref: autograd backward of
 * efficientnet_custom.py:104]:   dW[N, K] (fp32) (+)= dY^T x   (args as for mc_wgrad_rows_bf16, no prologue; ws with
 * mc_xbwd_rows_blocks(M) * N * K floats)   and   dX[M, K] (bf16) = dY . wt[K, N]^T (+ r[M, K])   -- what
 * mc_gemm_rows_bf16(dY, wt, residual r) returns.  Shapes: mc_xbwd_rows_supported(N, K) (K <= 64 and the expand geometries
 * of EfficientNet-B2 / -B5: (96,16) (144,24) (240,40) (288,48) (384,64)). */
int mc_xbwd_rows_supported(int n, int k);
int mc_xbwd_rows_blocks(long long m);
int mc_xbwd_rows_bf16(const mc_wgrad_rows_args* args, const mc_bf16* wt, long long ldwt, mc_bf16* dx, long long lddx,
                      const mc_bf16* r, long long ldr, void* stream);

/* ------------------------------------------------------------------------------------------------
 * small helpers */
int mc_cast_f32_bf16(const float* src, mc_bf16* dst, long long n, void* stream);
/* low term of the two-term bf16 split of fp32 weights, dst = bf16(src - float(bf16(src))): with mc_cast_f32_bf16's image as
 * the high term, x . (hi + lo)^T carries the weights to 2^-17 instead of 2^-9 (the opt-in "hi + lo" operand mode of the BERT
 * linears -- the eval-mode parity configuration of DESIGN.md (c); the reference's own path is fp32 / fp16 autocast,
 * trainer.py:271-278) */
int mc_cast_f32_bf16_lo(const float* src, mc_bf16* dst, long long n, void* stream);
int mc_cast_bf16_f32(const mc_bf16* src, float* dst, long long n, void* stream);
int mc_transpose_f32(const float* src, float* dst, int rows, int cols, void* stream); /* dst[c][r] = src[r][c] */
int mc_cast_transpose_f32_bf16(const float* src, mc_bf16* dst, int rows, int cols, void* stream); /* dst[c][r] = bf16(src[r][c]) */
/* stem weight [C0,3,3,3] fp32 (OIHW) -> bf16 [C0,32], k = cin*9 + kh*3 + kw, zero padded 27..31 */
int mc_stem_weight_prep(const float* w, mc_bf16* out, int c0, void* stream);

/* ------------------------------------------------------------------------------------------------
 * stem im2col: fp32 image batch with arbitrary element strides (NCHW or the trainer's permuted NHWC
 * view, [ref: trainer_ddp.py:288-291]) -> bf16 patches [n*oh*ow, 32] for the 3x3 stride-2 stem conv
 * with static padding (pad_l, pad_t) [ref: efficientnet_custom.py:273, efficient_net_custom_utils.py:248-276] */
int mc_stem_im2col(const float* x, long long sn, long long sc, long long sh, long long sw,
                   int n, int h, int w, int pad_l, int pad_t, int oh, int ow, mc_bf16* out, void* stream);
/* out[img][n][k] = bf16(w[n][k] * gate[img][k]) (w dense [n,k] bf16, k % 8 == 0): per-image SE-gated copies of the
 * projection weight [ref: efficientnet_custom.py:119,122  x = sigmoid(se) * x; _project_conv(x)] -- scaling the small
 * operand instead of the activation tensor lets the projection run as a plain batched GEMM */
int mc_gate_weights_bf16(const mc_bf16* w, const float* gate, int n_img, int n, int k, mc_bf16* out, void* stream);

/* input pipeline in front of the stem: raw 8-bit pixels instead of a normalised fp32
 * batch.  [ref: data/datasets/imagetext.py:131-135]  x = float32(u8); x -= x.min(); x /= x.max(); (x - mean) / std
 * per image, every step rounded to float32 in that order -- reproduced bit for bit, then the same patches as above.
 * minmax: unsigned[2][n] workspace = per-image min, then per-image max (filled by mc_image_minmax_u8 from a DENSE
 * per-image block of elems_per_image bytes at stride sn; the [b,1,H,W,3] -> [b,3,H,W] permute of
 * trainer_ddp.py:288-291 is again just the (sc, sh, sw) element strides). */
int mc_image_minmax_u8(const unsigned char* x, long long sn, long long elems_per_image, int n,
                       unsigned int* minmax, void* stream);
int mc_stem_im2col_u8(const unsigned char* x, long long sn, long long sc, long long sh, long long sw,
                      const unsigned int* minmax, float mean, float std, int n, int h, int w, int pad_l,
                      int pad_t, int oh, int ow, mc_bf16* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * direct stem convolution (csrc/stem.hip): the same 3x3 stride-2 conv without the patch matrix, for a CHANNELS-LAST
 * image (element (img, y, x, c) at img*sn + y*sh + x*3 + c; fp32, or raw uint8 with the normalisation above).
 *   fwd:   e[n*oh*ow, c0] bf16 = patches . wb[c0,32]^T (wb from mc_stem_weight_prep; 32 <= c0 <= 64, c0 % 8 == 0) -- the bits of
 *          mc_stem_im2col + mc_gemm_rows_bf16; stat_partials (optional): [mc_stem_conv_blocks(n, oh, ow, 1)][2][c0] column sum /
 *          sum of squares of e, the layout mc_bn_finalize reduces
 *   wgrad: dw[c0,32] fp32 = de[n*oh*ow, c0]^T . patches (columns 27..31 zero); ws: [mc_stem_conv_blocks(n, oh, ow, 0 or 2)][c0][32]
 *          floats of per-workgroup partials, summed in workgroup order (no atomics: the same bits every run).
 *          bn_e / bn_coef (both or neither): `de` is dZ0 = dL/d bn0(e) and the kernel forms the BatchNorm0 backward apply
 *          de = coef[0]*dZ0 + coef[1]*e + coef[2] (coef [3][c0] from mc_bn_bwd_finalize; rounded to 16 bits like the output of
 *          mc_bnact_bwd_apply) while it stages dZ0: that pass and its tensor are not needed */
int mc_stem_conv_blocks(int n, int oh, int ow, int kind);     /* kind: 0 wgrad, 1 fwd, 2 wgrad with bn_e / bn_coef */
int mc_stem_conv_fwd(const float* x, long long sn, long long sh, int n, int h, int w, int pad_l, int pad_t, int oh,
                     int ow, const mc_bf16* wb, int c0, mc_bf16* e, float* stat_partials, void* stream);
int mc_stem_conv_fwd_u8(const unsigned char* x, long long sn, long long sh, const unsigned int* minmax, float mean,
                        float std, int n, int h, int w, int pad_l, int pad_t, int oh, int ow, const mc_bf16* wb, int c0,
                        mc_bf16* e, float* stat_partials, void* stream);
int mc_stem_conv_wgrad(const void* x, int is_u8, long long sn, long long sh, const unsigned int* minmax, float mean,
                       float std, int n, int h, int w, int pad_l, int pad_t, int oh, int ow, const mc_bf16* de, int c0,
                       const mc_bf16* bn_e, const float* bn_coef, float* ws, float* dw, void* stream);

/* ------------------------------------------------------------------------------------------------
 * depthwise k x k convolution, NHWC bf16, static asymmetric zero padding
 * [ref: efficientnet_custom.py:109 (_depthwise_conv) + :110-111 (_bn1 statistics), :105-107 fused as
 *  prologue: x' = silu(x*pro_scale[c] + pro_shift[c]) applied to in-range inputs only]
 * w_kkc: fp32 [k*k][C] (tap-major).  stat_partials: float[mc_dwconv_stat_rows()][2][C] (optional). */
typedef struct mc_dwconv_args {
    const mc_bf16* x;        /* [n,h,w,c] */
    const mc_bf16* dy;       /* [n,oh,ow,c]  (backward only) */
    void* out;               /* fwd: y bf16 [n,oh,ow,c]; bwd_data: dx bf16 [n,h,w,c]; bwd_weight: dw f32 [k*k][c] (+=) */
    const float* w_kkc;
    int n, h, w, c;
    int k, stride, pad_l, pad_t, oh, ow;
    const float* pro_scale;
    const float* pro_shift;
    float* stat_partials;
    /* BatchNorm(+SiLU)-backward epilogue of the DATA GRADIENT launch: mc_dwconv_fwd on flipped taps for a stride-1 conv,
     * mc_dwconv_bwd_data for a stride-2 conv (stat_partials then has mc_dwconv_bwd_data_stat_rows() rows and epi_x is
     * [n,h,w,c], the shape of the gradient).  epi_x = the conv output e [n,oh,ow,c] that fed
     * silu(bn(e)); the kernel then writes dZ = y * silu'(e*epi_scale + epi_shift) instead of y and stat_partials receives
     * [rows][2][c] = (sum dZ, sum dZ * (e - epi_mean) * epi_invstd), the input of mc_bn_bwd_finalize.  NULL = plain conv. */
    const mc_bf16* epi_x;
    const float* epi_scale;
    const float* epi_shift;
    const float* epi_mean;
    const float* epi_invstd;
    /* round 5 -- fused backward of a stride-1 depthwise conv (mc_dwconv_bwd_fused): weight gradient f32 [k*k][c] (+=) */
    float* dw_out;
    /* rows the caller allocated in stat_partials (what mc_dwconv_stat_rows / mc_dwconv_bwd_*_stat_rows returned for THIS
     * argument block); 0 = not checked.  A launch whose kernel form would write a different number of rows is refused --
     * the form can change between the two calls through mc_dwconv_set_lane_mode / MC_DW_LANE. */
    int stat_rows;
    /* round 6 -- mc_mbconv_xdw_fwd: the expand 1x1 conv in front of the depthwise conv, run inside its staging.  xw = the
     * expand weight [c][cin] (16-bit, row-major, c = the depthwise conv's channels); x is then the BLOCK INPUT [n,h,w,cin].
     * mc_dwconv_bwd_fused with xw != NULL: epi_x is the block input [n,oh,ow,cin] (the launch's output geometry = the conv's
     * input geometry) and the e rows the epilogue / weight gradient need are formed from it in the staging (cin <= 64). */
    const mc_bf16* xw;
    int cin;
    /* The store-and-sum ending of the WEIGHT GRADIENT (mc_dwconv_bwd_weight, mc_dwconv_bwd_fused, mc_dwconv_bwd_data with xw +
     * dw_out): with dw_partials != NULL no float atomic is issued -- the unit that adds its partial sums to the gradient with
     * atomicAdd otherwise (the wave's y slot of the lane = column kernel, the persistent workgroup of the marching kernels)
     * stores them to its own row of dw_partials: float[dw_rows][k*k][c], rows in the conv's own tap order, every element of every
     * row written by the launch (no fill needed).  A second launch on the same stream then finishes
     * dw[t][c] += (float) sum_r (double) dw_partials[r][t][c], r ascending (mc_ordered_sum): bit-reproducible, and still +=.
     * dw_rows = what mc_dwconv_bwd_weight_dw_rows / _bwd_fused_dw_rows / _bwd_data_dw_rows returned for THIS argument block;
     * 0 = not checked, and a launch whose kernel form would write another row count is refused (the stat_rows rule).
     * NULL = the atomic ending, unchanged. */
    float* dw_partials;
    int dw_rows;
} mc_dwconv_args;
int mc_dwconv_stat_rows(const mc_dwconv_args* args);
int mc_dwconv_bwd_data_stat_rows(const mc_dwconv_args* args);
int mc_dwconv_fwd(const mc_dwconv_args* args, void* stream);
int mc_dwconv_bwd_data(const mc_dwconv_args* args, void* stream);
int mc_dwconv_bwd_weight(const mc_dwconv_args* args, void* stream);
/* rows of args->dw_partials that the launch writes for THIS argument block under the current lane mode (pure functions of the
 * geometry fields; pointers are only tested for NULL): mc_dwconv_bwd_weight (its form follows mc_dwconv_set_lane_mode),
 * mc_dwconv_bwd_data with xw + dw_out (= mc_dwconv_bwd_data_stat_rows), mc_dwconv_bwd_fused (= its stat rows). */
int mc_dwconv_bwd_weight_dw_rows(const mc_dwconv_args* args);
int mc_dwconv_bwd_data_dw_rows(const mc_dwconv_args* args);
int mc_dwconv_bwd_fused_dw_rows(const mc_dwconv_args* args);
/* The E-free form of mc_dwconv_bwd_data for a STRIDE-2 3x3 conv whose input was silu(bn0(e))
 * [ref: efficientnet_custom.py:104-111 backwards: _depthwise_conv, _bn0 + swish, with e = _expand_conv(x)]: with args->xw
 * (+ cin <= 64, cin % 8 == 0) the launch does not READ e: epi_x is the block input x [n,h,w,cin] and e = x . xw^T is formed on
 * the MFMA unit for the pixels the launch completes (raw e rounded once to 16 bits like the tensor the expand GEMM stores, the
 * rule of mc_dwconv_bwd_fused below).  out = dZ0 and stat_partials (mc_dwconv_bwd_data_stat_rows() rows, the same count with
 * and without xw) are what the e-reading launch leaves.  With args->dw_out the same launch is also the conv's weight gradient:
 * f32 [k*k][c], accumulated into (+=) in the conv's own tap order, dW[kh,kw,c] += dD[o,j,c] * a0[2o-pt+kh, 2j-pl+kw, c] with
 * a0 = silu(bn0(e)) (dw_out without xw is refused).  Together with mc_mbconv_xdw_fwd and the folded BatchNorm0 backward the
 * expanded tensor of such a block is then neither rebuilt nor read in the backward.
 * _supported: 3x3, stride 2, c % 8 == 0, epi_x and xw given, cin % 8 == 0, cin <= 64 (pointers are only tested for NULL).
 * _preferred: the shapes on which the launch measured faster than the three it replaces. */
int mc_dwconv_bwd_data_xw_supported(const mc_dwconv_args* args);
/* how the stride-2 epilogue launch (with or without xw) splits its work: plan[4] = column strips per row, row segments per
 * image, super-rows (2 input rows) per segment, channel tiles; returns mc_dwconv_bwd_data_stat_rows().  For tests that must
 * know a shape spans several strips / segments. */
int mc_dwconv_bwd_data_plan(const mc_dwconv_args* args, int* plan);
/* Two more host-only queries for tests that must know which tile seams a shape reaches (pure functions of the geometry fields;
 * neither launches anything nor looks at the lane mode).
 * mc_dwconv_march_plan: the marching forward (weight_grad == 0; with epi_x its stride-1 data-gradient form) or weight gradient:
 * plan[6] = output columns per strip, channels per tile, column strips per row, row segments per image, output rows per
 * segment, persistent workgroups per channel tile (= the return value: the rows of stat_partials / dw_partials of that form).
 * mc_dwconv_lane_plan: the lane = column configuration for mode 0 (forward), 1 (stride-1 data gradient with the epilogue; the
 * argument block of that launch), 2 (weight gradient), 3 (fused backward; the argument block of mc_dwconv_bwd_fused):
 * plan[8] = images per wave, output columns per lane, output columns per strip, column strips per row, channel tiles, tile
 * pairs, work units, y slots (= the return value: the rows of stat_partials / dw_partials of that form).
 * Both return 0 for an argument block the form does not take. */
int mc_dwconv_march_plan(const mc_dwconv_args* args, int weight_grad, int* plan);
int mc_dwconv_lane_plan(const mc_dwconv_args* args, int mode, int* plan);
int mc_dwconv_bwd_data_xw_preferred(const mc_dwconv_args* args);
/* Two device forms of the forward / stride-1 data gradient exist: the "marching" kernels (a lane owns 2-4 channels, taps
 * in VGPRs) and the "lane = column" kernels of round 4 (a wave owns one channel pair, taps in SGPRs, 16-wave workgroups;
 * conv_lane.hip).  mc_dwconv_fwd picks by shape (5x5 from 50 output columns up); this switch overrides the choice for
 * tests and A/B timing: -1 policy, 0 marching only, 1 lane = column wherever supported.  Returns the previous mode.
 * (Environment variable MC_DW_LANE sets the initial mode.)  Both forms produce bit-identical outputs. */
int mc_dwconv_set_lane_mode(int mode);
int mc_dwconv_lane_supported(const mc_dwconv_args* args);
/* Round 5 -- the whole backward of a STRIDE-1 3x3 / 5x5 depthwise conv whose input was silu(bn0(e)) in ONE launch
 * [ref: efficientnet_custom.py:104-111 backwards: _depthwise_conv, _bn0 + swish]: the data gradient with the BatchNorm0
 * epilogue of mc_dwconv_fwd(epi_x) AND the weight gradient of mc_dwconv_bwd_weight from one staging of (dd, e) -- dd and e
 * are read once, dZ0 is written once (3 passes over the expanded tensor instead of 5).  The argument block is the one of
 * the data-gradient launch (x = dd [n, h, w, c] on the conv's OUTPUT geometry, w_kkc = the taps rotated by 180 degrees,
 * pad = k-1-pad, (oh, ow) = the conv's input geometry, epi_* = e and its BatchNorm statistics, out = dZ0, stat_partials
 * with mc_dwconv_bwd_fused_stat_rows() rows) plus dw_out: f32 [k*k][c], accumulated into (+=) in the conv's OWN tap order.
 * The launch and its sizing helpers take 3x3 and 5x5.  The 5x5 launch runs 12-wave workgroups on 24-channel tiles (its 50 tap
 * accumulators and the windows do not fit the 128 registers of a 16-wave workgroup: see conv_lane.hip); both weight-gradient
 * endings (atomic, dw_partials) exist for it; the xw form below is 3x3 only.
 * mc_dwconv_bwd_fused_supported: 3x3, stride 1, c % 8 == 0, epi_x given (it answers for the 3x3 instances only, as before).
 * mc_dwconv_bwd_fused5_supported: the same for 5x5 (no xw).
 * _preferred / fused5_preferred: the shapes on which the launch measured faster than the two it replaces. */
/* Round 6: with args->xw (+ cin <= 64) the launch does not READ e: epi_x is the block input x and e = x . xw^T is formed per
 * 16-pixel group on the MFMA unit while the rows are staged (the staging of mc_mbconv_xdw_fwd, raw e rounded once to 16 bits
 * like the tensor the expand GEMM stores).  Together with mc_mbconv_xdw_fwd and the folded BatchNorm0 backward
 * (mc_bn_fold_*) the expanded tensor of a stride-1 3x3 block then never exists in HBM, forward or backward. */
int mc_dwconv_bwd_fused_supported(const mc_dwconv_args* args);
int mc_dwconv_bwd_fused_preferred(const mc_dwconv_args* args);
int mc_dwconv_bwd_fused5_supported(const mc_dwconv_args* args);
int mc_dwconv_bwd_fused5_preferred(const mc_dwconv_args* args);
int mc_dwconv_bwd_fused_stat_rows(const mc_dwconv_args* args);
int mc_dwconv_bwd_fused(const mc_dwconv_args* args, void* stream);
/* Round 6 -- expand 1x1 conv -> BatchNorm0 + swish -> depthwise k x k conv of an MBConv block in ONE launch
 * [ref: efficientnet_custom.py:104-111: _expand_conv, _bn0, _swish, _depthwise_conv]: the expanded tensor e = x . xw^T never
 * exists in HBM.  The lane = column depthwise kernel (conv_lane.hip) stages the block input x (cin channels per pixel) instead
 * of e: every wave turns 16-pixel groups of the staged rows into its workgroup's 32 expanded channels with
 * v_mfma_f32_16x16x32 (weight slice resident in LDS as operand fragments), applies z = e*pro_scale + pro_shift and
 * silu(z) to the fp32 accumulators (e is NOT rounded to 16 bits on the way, unlike the two-launch form), zeroes the static
 * padding and writes the 16-bit activations into the LDS tile the stencil reads.  Everything behind the staging -- stencil,
 * output tile, BatchNorm1 statistics partials of the output (stat_partials, mc_mbconv_xdw_stat_rows() rows) -- is the plain
 * forward launch.  Arguments: the mc_dwconv_fwd block with x = block input [n,h,w,cin], xw, cin, pro_scale / pro_shift =
 * BatchNorm0's scale / shift over the c expanded channels (required: training mode takes them from mc_bn_gram_partials +
 * mc_bn_finalize or from a statistics tape, eval mode from the running statistics); epi_* must be NULL.
 * _supported: k in {3,5}, stride in {1,2}, c % 8 == 0, cin % 8 == 0, cin <= 128. */
int mc_mbconv_xdw_supported(const mc_dwconv_args* args);
int mc_mbconv_xdw_stat_rows(const mc_dwconv_args* args);
int mc_mbconv_xdw_fwd(const mc_dwconv_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * training-mode BatchNorm pieces [ref: efficientnet_custom.py:64,74,88,177,205; momentum 0.01, eps 1e-3]
 * finalize: partials float[rows][2][C] (sum, sum of squares) -> mean, invstd, scale = gamma*invstd,
 * shift = beta - mean*scale; running stats updated with the unbiased variance when update_running. */
int mc_bn_finalize(const float* partials, int rows, int c, double count, const float* gamma,
                   const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                   int update_running, float* mean, float* invstd, float* scale, float* shift, void* stream);
/* eval mode: scale/shift from running statistics */
int mc_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean,
                      const float* running_var, float eps, int c, float* scale, float* shift, void* stream);
/* the same, with the two rows a BACKWARD through a BatchNorm on running statistics needs as well (frozen BatchNorm:
 * model.eval() with autograd on, or EfficientNet.freeze_bn): mean = running_mean, invstd = 1/sqrt(running_var + eps);
 * scale / shift by the very fp32 expressions of mc_bn_eval_coeffs (bit-identical).  All outputs float[c]. */
int mc_bn_eval_stats(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                     float eps, int c, float* mean, float* invstd, float* scale, float* shift, void* stream);

/* elementwise family on x[n_img * hw, c] (bf16):  z = x*scale[c] + shift[c];  y = act(z)  (act 0 none, 1 SiLU)
 * apply:  out = y * rowscale[img] + res            (rowscale = drop_connect keep/keep_prob, res = skip input)
 *         [ref: efficientnet_custom.py:123-131, efficient_net_custom_utils.py:129-154]
 * pool:   pooled[img, c] = mean_hw y               [ref: efficientnet_custom.py:115 (SE squeeze), :307 (_avg_pooling)]
 *         with args->out != NULL the pass also stores y (bf16) there and pools the stored values: the late-stage project
 *         convolutions then read the activated tensor with a gate-only GEMM prologue instead of re-evaluating
 *         BN+SiLU once per column tile (forward) and once per row tile (weight gradient) */
typedef struct mc_bnact_args {
    const mc_bf16* x;
    long long n_img, hw;
    int c;
    const float* scale;
    const float* shift;
    int act;
    /* apply */
    const float* rowscale;   /* [n_img] or NULL */
    const mc_bf16* res;      /* or NULL */
    mc_bf16* out;
    /* pool */
    float* pooled;           /* [n_img, c] */
    /* backward: upstream gradient of y is  g*mul[img,c] + add[img,c]  (any of the three may be NULL;
     * g NULL = 0, mul NULL = 1, add NULL = 0), then dz = that * act'(z) * rowscale[img] */
    const mc_bf16* g;
    const float* mul;
    const float* add;
    float add_scale;         /* add is multiplied by this (0 is read as 1), e.g. 1/hw for pooled gradients */
    const float* mean;
    const float* invstd;
    float* partials;         /* bwd_reduce: float[mc_bnact_rows()][2][c] = (sum dz, sum dz*xhat) */
    const float* coef;       /* bwd_apply: float[3][c] from mc_bn_bwd_finalize: dx = A*dz + B*x + C */
    mc_bf16* dx;
    float* dgate;            /* se_dgate: [n_img, c] = sum_hw g * act(z) */
    /* pool / se_dgate / se_sums split the rows of an image over mc_bnact_img_splits() workgroups; when that is > 1
     * they need float[splits * n_img * c] (se_sums: * 5) of scratch here and combine it in split order, so results are
     * bit-reproducible run to run (no float atomics) */
    float* split_ws;
} mc_bnact_args;
int mc_bnact_rows(const mc_bnact_args* args);
int mc_bnact_img_splits(const mc_bnact_args* args);
int mc_bnact_apply(const mc_bnact_args* args, void* stream);
int mc_bnact_pool(const mc_bnact_args* args, void* stream);
int mc_bnact_bwd_reduce(const mc_bnact_args* args, void* stream);
int mc_bnact_bwd_apply(const mc_bnact_args* args, void* stream);
/* Backward through a FROZEN BatchNorm (running statistics) in ONE pass: the reduce pass (same optional g / mul / add /
 * add_scale / rowscale, act 0 / 1, same grid, same partials layout with mc_bnact_rows() rows, same reduction order: no atomics)
 * that also stores dx = scale[c] * dz (16 bit; required) -- frozen, dx does not depend on the reduction.  mean / invstd are the
 * running statistics (mc_bn_eval_stats); partials go to mc_bn_bwd_finalize_frozen for dgamma / dbeta. */
int mc_bnact_bwd_frozen(const mc_bnact_args* args, void* stream);
int mc_bnact_se_dgate(const mc_bnact_args* args, void* stream);
/* one pass over (x, g): args->dgate = float[5][n_img][c]: {sum g*y, sum g*y', sum g*y'*xhat, sum y', sum y'*xhat}
 * (y = act(z)); [0] is d loss / d gate, [1..4] let the BatchNorm-backward sums be formed without another pass: */
int mc_bnact_se_sums(const mc_bnact_args* args, void* stream);
/* partials[n_img][2][c] (the mc_bn_bwd_finalize input) for upstream gradient g*gate + dpooled*add_scale */
int mc_bn_partials_from_se_sums(const float* sums, const float* gate, const float* dpooled, float add_scale,
                                long long n_img, int c, float* partials, void* stream);
/* dgamma = sum dz*xhat, dbeta = sum dz; coef[0..2][c] for bwd_apply */
int mc_bn_bwd_finalize(const float* partials, int rows, int c, double count, const float* gamma,
                       const float* mean, const float* invstd, float* dgamma, float* dbeta, float* coef,
                       void* stream);
/* frozen BatchNorm: the same fp64 reduction of partials[rows][2][c] (xhat from the running statistics) -> dgamma, dbeta;
 * coef[3][c] = (scale, 0, 0) exactly, so every apply-type consumer (mc_bnact_bwd_apply, gemm_rows epi_mode 2) computes the
 * frozen dx = scale*dz unchanged */
int mc_bn_bwd_finalize_frozen(const float* partials, int rows, int c, const float* scale, float* dgamma, float* dbeta,
                              float* coef, void* stream);
/* frozen BatchNorm in front of a 1x1 conv e = x W^T (W = src [n, k] fp32): de = diag(scale) dz, hence dx = dz (diag(scale) W)
 * and dW = diag(scale) (dz^T x).  Row i of src times scale[i], written as w_t [k, n] (16 bit, TRANSPOSED: the data-gradient
 * GEMM's operand) and / or as out [n, k] fp32 (may alias src); either output may be NULL, not both. */
int mc_bn_frozen_rows(const float* src, const float* scale, int n, int k, mc_bf16* w_t, float* out, void* stream);

/* Training-mode BatchNorm backward folded into the 1x1 convolution in front of it (bnfold.hip; MBConv expand conv +
 * _bn0 [ref: efficientnet_custom.py:104-107]): with e = x We^T (We [n, k] fp32), coef = (A, B, C) from
 * mc_bn_bwd_finalize, dbeta = sum dz and rows = pixels,
 *     dx  = dz (A.We) + x G + cvec        dWe = A.(dz^T x - mean(dz) (x) colsum(x)) + (B.We) Sxx
 * so the consumers of de read dz and x only.  prepare: w1t [k, n] = bf16((A.We)^T), wb [n, k] = bf16(B.We),
 * sxx [k, k] = bf16(x^T x - colsum(x) (x) colsum(x) / rows);  cvec: gt [k, k] = (We^T wb)^T fp32 -> gtb bf16 and
 * cvec [k];  wgrad: dwe = A.(t1 - mean(dz) (x) colsum(x)) + wx  with t1 = dz^T x and wx = wb . sxx */
int mc_bn_fold_prepare(const float* we, const float* coef, const float* xtx, const float* colsum_x, double rows, int n,
                       int k, mc_bf16* w1t, mc_bf16* wb, mc_bf16* sxx, void* stream);
int mc_bn_fold_cvec(const float* gt, const float* we, const float* coef, const float* dbeta, const float* colsum_x,
                    double rows, int n, int k, mc_bf16* gtb, float* cvec, void* stream);
int mc_bn_fold_wgrad(const float* t1, const float* wx, const float* coef, const float* dbeta, const float* colsum_x,
                     double rows, int n, int k, float* dwe, void* stream);
/* Round 6 -- training-mode BatchNorm statistics of e = x . W^T (W [n, k] 16-bit, the MFMA operand image) WITHOUT e
 * [ref: efficientnet_custom.py:104-105: _expand_conv -> _bn0]: column sums and sums of squares of e follow from the k x k Gram
 * matrix of the (6 x narrower) input: sum_e[c] = w_c . colsum(x), and with the centred Gram S = x^T x - colsum (x) colsum / rows
 * the centred second moment is w_c^T S w_c (evaluated in fp64).  Writes TWO partials rows [2][2][n] = (sum, sum of squares) rounded to fp32 + the rounding
 * remainders (mc_bn_finalize adds its rows in fp64) in the layout mc_bn_finalize reads, so finalize / running statistics / the statistics tape are the code every other BatchNorm
 * uses.  xtx [k, k] fp32 (mc_wgrad_rows_bf16(x, x) / the tile TN GEMM), colsum_x [k] fp32 (mc_colsum_bf16). */
int mc_bn_gram_partials(const mc_bf16* w, int ldw, const float* xtx, const float* colsum_x, double rows, int n, int k,
                        float* partials, void* stream);

/* column sums of a bf16 matrix: out[c] = sum_m x[m, c]  (bias gradients).  partials: float[rows][c] */
int mc_colsum_rows(long long m, int c);
int mc_colsum_bf16(const mc_bf16* x, long long m, int c, long long ld, float* partials, float* out,
                   int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------
 * squeeze-excite MLP on pooled features [ref: efficientnet_custom.py:114-119]
 *   r = silu(w1 . pooled + b1);  gate = sigmoid(w2 . r + b2);  w1 [cs, c], w2 [c, cs] fp32 */
int mc_se_fwd(const float* pooled, const float* w1, const float* b1, const float* w2, const float* b2,
              int n, int c, int cs, float* gate, float* ws /* float[n*cs] scratch */, void* stream);
/* ws: float[n * (c + 2*cs)] scratch; dw*, db* are WRITTEN (every element by exactly one thread: no zero-fill needed) */
int mc_se_bwd(const float* pooled, const float* gate, const float* dgate, const float* w1, const float* b1,
              const float* w2, const float* b2, int n, int c, int cs, float* dpooled, float* dw1, float* db1,
              float* dw2, float* db2, float* ws, void* stream);

/* dropout on fp32 vectors (pooled image features [ref: efficientnet_custom.py:310-312]); y = x * mask/(1-p),
 * mask = philox(seed, stream_id, index): calling it on the gradient with the same ids is the backward. */
int mc_dropout_f32(const float* x, float* y, long long n, float p, unsigned long long seed,
                   unsigned int stream_id, void* stream);

/* ------------------------------------------------------------------------------------------------
 * BERT pieces [ref: model/modules/text_encoder.py:47-49 -> transformers BertModel] */
/* embeddings: y = dropout(LN(word[ids] + pos[t] + type[tt]))  -> bf16 [b*t, h]; saves mean/rstd */
int mc_bert_embed_fwd(const long long* ids, const long long* tt, const float* word, const float* pos,
                      const float* type, const float* gamma, const float* beta, float eps, int b, int t,
                      int h, float p, unsigned long long seed, unsigned int stream_id, mc_bf16* y,
                      float* mean, float* rstd, void* stream);
int mc_bert_embed_bwd(const mc_bf16* dy, const long long* ids, const long long* tt, const float* word,
                      const float* pos, const float* type, const float* gamma, const float* mean,
                      const float* rstd, int b, int t, int h, float p, unsigned long long seed,
                      unsigned int stream_id, float* dword, float* dpos, float* dtype, float* dgamma,
                      float* dbeta, void* stream);    /* all outputs accumulated (+=) */
/* y = LN(dropout(x) + res) ; rows x h */
int mc_add_ln_fwd(const mc_bf16* x, const mc_bf16* res, const float* gamma, const float* beta, float eps,
                  long long rows, int h, float p, unsigned long long seed, unsigned int stream_id,
                  mc_bf16* y, float* mean, float* rstd, void* stream);
/* dx = dropout-masked grad wrt x, dres = grad wrt res (pre-LN sum grad); dgamma/dbeta accumulated (+=) */
int mc_add_ln_bwd(const mc_bf16* dy, const mc_bf16* x, const mc_bf16* res, const float* gamma,
                  const float* mean, const float* rstd, long long rows, int h, float p,
                  unsigned long long seed, unsigned int stream_id, mc_bf16* dx, mc_bf16* dres,
                  float* dgamma, float* dbeta, void* stream);
/* mc_add_ln_bwd without float atomics: every workgroup stores its 2*h sums to its row of ws: float[ws_rows][2][h] with
 * ws_rows = mc_add_ln_bwd_ws_rows(rows) (the capped grid; another count is refused), every element written, then
 * dgamma / dbeta += the rows summed in row order (mc_ordered_sum).  dx / dres are the bits of mc_add_ln_bwd. */
int mc_add_ln_bwd_ws_rows(long long rows);
int mc_add_ln_bwd_ws(const mc_bf16* dy, const mc_bf16* x, const mc_bf16* res, const float* gamma,
                     const float* mean, const float* rstd, long long rows, int h, float p,
                     unsigned long long seed, unsigned int stream_id, mc_bf16* dx, mc_bf16* dres,
                     float* dgamma, float* dbeta, float* ws, int ws_rows, void* stream);
/* mc_bert_embed_bwd without float atomics (store-and-sum).  ws: float[mc_bert_embed_bwd_ws_floats(b, t, h, b * t, plan)] =
 * dx of every token row [b*t][h] | position sums per batch group [plan[0]][t][h] | gamma / beta / type-0 / type-1 sums per
 * workgroup [plan[1]][4][h]; every element is written by the launch.  Then dword[id] += the dx rows of the tokens that name id,
 * summed in ascending token-row order by one wave per vocabulary row (rows no token names are not touched), dpos += the groups
 * in group order, dtype / dgamma / dbeta += the workgroups in order (mc_ordered_sum): all outputs accumulated (+=), fp64
 * accumulators, one rounding.  sorted_ids / order: int64 [b*t], the token ids sorted ascending by a STABLE sort and the token
 * row (index into the flattened ids) of each sorted entry.  plan (optional): int[2] = batch groups, workgroups. */
long long mc_bert_embed_bwd_ws_floats(int b, int t, int h, long long rows, int* plan);
int mc_bert_embed_bwd_ws(const mc_bf16* dy, const long long* ids, const long long* tt, const float* word, const float* pos,
                         const float* type, const float* gamma, const float* mean, const float* rstd, int b, int t, int h,
                         float p, unsigned long long seed, unsigned int stream_id, float* dword, float* dpos, float* dtype,
                         float* dgamma, float* dbeta, const long long* sorted_ids, const long long* order, float* ws,
                         long long ws_floats, void* stream);
/* out[i] = (accumulate ? out[i] : 0) + (float) sum_r (double) ws[r * ld + i], 0 <= i < n <= ld, r = 0 .. rows-1 ascending:
 * one fp64 accumulator per element and one rounding -- the finish step of every store-and-sum reduction above and below. */
int mc_ordered_sum(const float* ws, int rows, long long ld, long long n, float* out, int accumulate, void* stream);
/* row softmax of fp32 scores [rows, t] -> probs (bf16) and dropped probs (bf16; may alias probs when p == 0) */
int mc_softmax_fwd(const float* scores, long long rows, int t, float p, unsigned long long seed,
                   unsigned int stream_id, mc_bf16* probs, mc_bf16* probs_drop, void* stream);
/* dscores = probs * (dp - sum(probs*dp)) * alpha with dp = dprobs_drop * mask/(1-p); bf16 out */
int mc_softmax_bwd(const mc_bf16* probs, const float* dprobs_drop, long long rows, int t, float p,
                   unsigned long long seed, unsigned int stream_id, float alpha, mc_bf16* dscores, void* stream);
/* Fused self-attention core (attn.hip), head size 64, 32 <= t <= 256, t % 32 == 0 (mc_attn_supported):
 *   ctx[b*t, nh*64] = dropout(softmax(alpha * Q K^T + mask_bias[b, key])) V   per (sequence, head),
 * qkv = [b*t, 3*nh*64] (Q | K | V column blocks).  The [b, nh, t, t] scores / probabilities are never stored: the
 * forward keeps lse[b*nh*t][2] = (row max, 1 / row sum) and the backward recomputes them.  Dropout masks are the
 * same function of (seed, stream_id, element) as mc_softmax_fwd's.
 * Replaces transformers BertSelfAttention.forward as called from the reference's text encoder
 * [ref: model/modules/text_encoder.py:47-49]. */
int mc_attn_supported(int t, int head_dim);
int mc_attn_fwd(const mc_bf16* qkv, const float* mask_bias, int b, int t, int nh, float alpha, float p,
                unsigned long long seed, unsigned int stream_id, mc_bf16* ctx, float* lse, void* stream);
/* dqkv [b*t, 3*nh*64] (every element written) from dctx [b*t, nh*64] */
int mc_attn_bwd(const mc_bf16* qkv, const float* mask_bias, const mc_bf16* dctx, const float* lse, int b, int t,
                int nh, float alpha, float p, unsigned long long seed, unsigned int stream_id, mc_bf16* dqkv,
                void* stream);
/* The same contract and arguments for 32 <= t <= 512, t % 32 == 0 (mc_attn_long_supported; attn.hip, long kernels): K / V
 * whole in LDS in the forward, 256-row tiles restaged per chunk in the backward.  Same lse layout and dropout masks as
 * mc_attn_fwd / mc_attn_bwd; the text encoder sends only t > 256 here. */
int mc_attn_long_supported(int t, int head_dim);
int mc_attn_long_fwd(const mc_bf16* qkv, const float* mask_bias, int b, int t, int nh, float alpha, float p,
                     unsigned long long seed, unsigned int stream_id, mc_bf16* ctx, float* lse, void* stream);
int mc_attn_long_bwd(const mc_bf16* qkv, const float* mask_bias, const mc_bf16* dctx, const float* lse, int b, int t,
                     int nh, float alpha, float p, unsigned long long seed, unsigned int stream_id, mc_bf16* dqkv,
                     void* stream);
int mc_gelu_fwd(const mc_bf16* x, mc_bf16* y, long long n, void* stream);
int mc_gelu_bwd(const mc_bf16* dy, const mc_bf16* x, mc_bf16* dx, long long n, void* stream);
/* mask bias for attention: out[b, t] = (1 - mask[b,t]) * -3.0e38-ish (finfo.min)  */
int mc_mask_bias(const long long* mask, float* out, long long n, void* stream);
/* eos pooling [ref: model/clip.py:65-68]: out[b, :] = h[b, sum(mask[b]) - 1, :]  (bf16 -> fp32) */
int mc_eos_gather(const mc_bf16* hid, const long long* mask, int b, int t, int h, float* out, void* stream);
int mc_eos_scatter(const float* dout, const long long* mask, int b, int t, int h, mc_bf16* dhid, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Packed (variable-length) text encoder: the b reports of a call as ONE [rows, h] matrix that holds only their real
 * tokens.  Sequence i owns rows cu_seqlens[i] .. cu_seqlens[i+1]-1 (int32 [b+1], cu_seqlens[0] = 0); rows
 * cu_seqlens[b] .. rows-1 are alignment rows that belong to no sequence; row_map[rows] (int32) is the row i*t_pad + position
 * of each packed row in the padded [b, t_pad] layout (-1 for alignment rows).  The reference pads every report to
 * max_length 256 and runs BertModel on all of them [ref: data/datasets/imagetext.py:217-222;
 * model/modules/text_encoder.py:47-49]; the padded rows are never read by a real token, so leaving them out changes
 * no result.  Every dropout mask below is the one the padded entry point draws for the same (seed, stream_id):
 * the element index is formed from the padded row. */
/* Fused self-attention on packed rows (attn.hip, packed view), head size 64, 1 <= len_i <= max_len <= 256:
 *   ctx[rows, nh*64] = dropout(softmax(alpha * Q K^T)) V   per (sequence, head) over the sequence's own tokens
 * -- mc_attn_fwd on the padded batch with a 1..10..0 mask, without the padded rows
 * [ref: model/modules/text_encoder.py:47-49 -> transformers BertSelfAttention.forward].  qkv = [rows, 3*nh*64];
 * lse = [rows, nh, 2]; order = int32 [b] sequence indices in launch order (longest first) or NULL; t_pad = T of the padded
 * layout (multiple of 8, >= max_len).  Alignment rows of ctx / dqkv are written with zeros. */
int mc_attn_varlen_supported(int max_len, int head_dim);
int mc_attn_varlen_fwd(const mc_bf16* qkv, const int* cu_seqlens, const int* order, int b, int max_len, int t_pad,
                       long long rows, int nh, float alpha, float p, unsigned long long seed, unsigned int stream_id,
                       mc_bf16* ctx, float* lse, void* stream);
int mc_attn_varlen_bwd(const mc_bf16* qkv, const int* cu_seqlens, const int* order, const mc_bf16* dctx, const float* lse,
                       int b, int max_len, int t_pad, long long rows, int nh, float alpha, float p,
                       unsigned long long seed, unsigned int stream_id, mc_bf16* dqkv, void* stream);
/* mc_attn_varlen_* for 1 <= len_i <= max_len <= 512 (mc_attn_varlen_long_supported; attn.hip, long kernels), same arguments */
int mc_attn_varlen_long_supported(int max_len, int head_dim);
int mc_attn_varlen_long_fwd(const mc_bf16* qkv, const int* cu_seqlens, const int* order, int b, int max_len, int t_pad,
                            long long rows, int nh, float alpha, float p, unsigned long long seed, unsigned int stream_id,
                            mc_bf16* ctx, float* lse, void* stream);
int mc_attn_varlen_long_bwd(const mc_bf16* qkv, const int* cu_seqlens, const int* order, const mc_bf16* dctx, const float* lse,
                            int b, int max_len, int t_pad, long long rows, int nh, float alpha, float p,
                            unsigned long long seed, unsigned int stream_id, mc_bf16* dqkv, void* stream);
/* mc_bert_embed_fwd / _bwd on packed rows [ref: transformers BertEmbeddings via text_encoder.py:47-49]: ids / tt in packed
 * order, pos_ids[r] = r - cu_seqlens[i]; alignment rows of y are zeros.  The backward accumulates (+=) like the padded one. */
int mc_bert_embed_rows_fwd(const long long* ids, const long long* tt, const int* pos_ids, const int* row_map,
                           const float* word, const float* pos, const float* type, const float* gamma,
                           const float* beta, float eps, long long rows, int h, float p, unsigned long long seed,
                           unsigned int stream_id, mc_bf16* y, float* mean, float* rstd, void* stream);
int mc_bert_embed_rows_bwd(const mc_bf16* dy, const long long* ids, const long long* tt, const int* cu_seqlens,
                           const float* word, const float* pos, const float* type, const float* gamma,
                           const float* mean, const float* rstd, int b, int max_len, int t_pad, int h, float p,
                           unsigned long long seed, unsigned int stream_id, float* dword, float* dpos, float* dtype,
                           float* dgamma, float* dbeta, void* stream);
/* mc_bert_embed_bwd_ws on packed rows: real_rows = cu_seqlens[b] token rows (the alignment rows behind them are not looked
 * at), ws: float[mc_bert_embed_bwd_ws_floats(b, max_len, h, real_rows, plan)], sorted_ids / order over the first real_rows ids. */
int mc_bert_embed_rows_bwd_ws(const mc_bf16* dy, const long long* ids, const long long* tt, const int* cu_seqlens,
                              const float* word, const float* pos, const float* type, const float* gamma,
                              const float* mean, const float* rstd, int b, int max_len, int t_pad, int h,
                              long long real_rows, float p, unsigned long long seed, unsigned int stream_id, float* dword,
                              float* dpos, float* dtype, float* dgamma, float* dbeta, const long long* sorted_ids,
                              const long long* order, float* ws, long long ws_floats, void* stream);
/* mc_add_ln_fwd / _bwd on packed rows [ref: transformers BertSelfOutput / BertOutput via text_encoder.py:47-49]; alignment
 * rows are normalised without dropout (finite in, finite out). */
int mc_add_ln_rows_fwd(const mc_bf16* x, const mc_bf16* res, const int* row_map, const float* gamma, const float* beta,
                       float eps, long long rows, int h, float p, unsigned long long seed, unsigned int stream_id,
                       mc_bf16* y, float* mean, float* rstd, void* stream);
int mc_add_ln_rows_bwd(const mc_bf16* dy, const mc_bf16* x, const mc_bf16* res, const int* row_map, const float* gamma,
                       const float* mean, const float* rstd, long long rows, int h, float p, unsigned long long seed,
                       unsigned int stream_id, mc_bf16* dx, mc_bf16* dres, float* dgamma, float* dbeta, void* stream);
/* ... and its store-and-sum form, see mc_add_ln_bwd_ws */
int mc_add_ln_rows_bwd_ws(const mc_bf16* dy, const mc_bf16* x, const mc_bf16* res, const int* row_map, const float* gamma,
                          const float* mean, const float* rstd, long long rows, int h, float p, unsigned long long seed,
                          unsigned int stream_id, mc_bf16* dx, mc_bf16* dres, float* dgamma, float* dbeta, float* ws,
                          int ws_rows, void* stream);
/* Pooling from packed rows [ref: model/clip.py:65-75]: eos = gather of rows cu_seqlens[i+1]-1, bos = rows cu_seqlens[i]
 * (out[i] = float(src[idx[i]]); the backward scatters into a zero-filled dsrc), mean = per-sequence mean. */
int mc_rows_gather(const mc_bf16* src, const int* idx, int n, int h, float* out, void* stream);
int mc_rows_scatter(const float* dout, const int* idx, int n, int h, mc_bf16* dsrc, void* stream);
int mc_segment_mean_fwd(const mc_bf16* src, const int* cu_seqlens, int b, int h, float* out, void* stream);
/* every row of dsrc written (alignment rows: zeros); t = t_pad of row_map */
int mc_segment_mean_bwd(const float* dout, const int* cu_seqlens, const int* row_map, long long rows, int t, int h,
                        mc_bf16* dsrc, void* stream);
/* last_hidden_state [b, t, h] from packed rows, zeros at the padded positions [ref: text_encoder.py:49], and its backward
 * (gather of the real rows, zeros in the alignment rows); h % 8 == 0 */
int mc_unpack_rows(const mc_bf16* src, const int* cu_seqlens, int b, int t, int h, mc_bf16* dst, void* stream);
int mc_pack_rows(const mc_bf16* src, const int* row_map, long long rows, int h, mc_bf16* dst, void* stream);

/* ------------------------------------------------------------------------------------------------
 * fp32 small GEMM with arbitrary strides: C[m,n] = alpha * sum_k A[m*ars + k*acs] * B[k*brs + n*bcs] + beta*C + bias[n]
 * [ref: model/modules/projection.py:23-29 (LinearProjectionHead); loss/breast_clip.py:46-100 (logits)] */
/* alpha_dev (optional): device scalar multiplied into alpha (e.g. the learnable logit scale).
 * ws (optional): float[mc_sgemm_ws_floats(m, n, k)] scratch; lets few-tile / long-k products (projection heads, their
 * weight gradients) spread over the chip by split-K, partials combined in split order (deterministic) */
long long mc_sgemm_ws_floats(int m, int n, int k);
int mc_sgemm(const float* a, long long ars, long long acs, const float* b, long long brs, long long bcs,
             float* c, long long ldc, int m, int n, int k, float alpha, float beta, const float* bias,
             const float* alpha_dev, float* ws, void* stream);
/* y[i] = x[i] * (*scalar_dev) * alpha */
int mc_scale_f32(const float* x, const float* scalar_dev, float alpha, float* y, long long n, void* stream);
/* y = x / ||x||_2 per row (no epsilon) [ref: model/clip.py:90-91]; bwd: dx = (dy - y*(y.dy)) / ||x|| */
int mc_l2norm_fwd(const float* x, int rows, int d, float* y, float* norm, void* stream);
int mc_l2norm_bwd(const float* dy, const float* y, const float* norm, int rows, int d, float* dx, void* stream);
/* MLP projection head [ref: model/modules/projection.py:4-20]: p = x W1^T + b1; g = GELU(p); f = g W2^T + b2;
 * y = LayerNorm(dropout(f) + p).  The GEMMs and their gradients are mc_sgemm calls; the entry points below are the rest, fp32
 * in both storage builds.  n = projection_dim must satisfy mc_mlp_head_supported(n): n % 8 == 0 (one Philox draw covers 8
 * consecutive elements of a row) and 8 <= n <= mc_mlp_head_max_n() = 2048 (a wave holds a row in registers: at most four
 * 8-float vectors per lane).  Row pointers must be 16-byte aligned. */
int mc_mlp_head_max_n(void);
int mc_mlp_head_supported(int n);
/* y = x * 0.5 * (1 + erf(x / sqrt 2))  (nn.GELU's default, exact form) */
int mc_gelu_f32_fwd(const float* x, float* y, long long count, void* stream);
/* dx = dg * GELU'(x) + add: joins the fc branch and the residual branch into the gradient of p (dx may alias dg or add) */
int mc_gelu_f32_bwd_add(const float* dg, const float* x, const float* add, float* dx, long long count, void* stream);
/* one wave per row of [rows, n]: z = f * keep_scale + res, mean and (two-pass, biased) variance of z over the row,
 * xhat = (z - mean) * rstd, y = xhat * gamma + beta; rstd = 1 / sqrt(var + eps), one float per row.  keep_scale is the
 * factor mc_dropout_f32 applies to element row * n + col for the same (seed, stream_id): 0 or 1 / (1 - p); at p == 0 no
 * random numbers are drawn and z = f + res.  0 <= p < 1. */
int mc_mlp_head_ln_fwd(const float* f, const float* res, const float* gamma, const float* beta, float eps, int rows, int n,
                       float p, unsigned long long seed, unsigned int stream_id, float* y, float* xhat, float* rstd,
                       void* stream);
/* LayerNorm backward per row: dz = rstd * (dy gamma - mean(dy gamma) - xhat mean(dy gamma xhat)), also the gradient of the
 * residual; df = dz * keep_scale (the forward's mask, regenerated).  Every workgroup stores its partial column sums of
 * dy * xhat (dgamma), dy (dbeta) and df (the fc bias gradient) to its row of ws: float[ws_rows][3][n] with
 * ws_rows = mc_mlp_head_ln_bwd_ws_rows(rows) (the capped grid; another count is refused), every element written;
 * mc_ordered_sum(ws, ws_rows, 3 n, 3 n, out, ...) finishes them.  No float atomics: bit-reproducible as it stands. */
int mc_mlp_head_ln_bwd_ws_rows(int rows);
int mc_mlp_head_ln_bwd(const float* dy, const float* xhat, const float* rstd, const float* gamma, int rows, int n, float p,
                       unsigned long long seed, unsigned int stream_id, float* df, float* dz, float* ws, int ws_rows,
                       void* stream);
/* mean cross-entropy over rows of logits [rows, n], weight w; the target of row r is labels[r] + label_offset
 * (labels: int64 device array or NULL = r):
 * loss_out[0] += w * mean_r CE_r (label smoothing `smoothing`);  dlogits = w/rows * (softmax - target)  (in place)
 * row_ws: `rows` floats of scratch -- per-row terms, summed in a fixed order (bit-reproducible, no float atomics)
 * [ref: loss/breast_clip.py:43-100 (labels = labels + rank*batch; F.cross_entropy)] */
int mc_ce_fwd_bwd(float* logits, int rows, int n, const long long* labels, int label_offset, float w, float smoothing,
                  float* loss_out, float* row_ws, void* stream);

/* ------------------------------------------------------------------------------------------------
 * evaluation metrics (retrieval.hip), fp32 in both storage builds.  a[N,D] image embeddings, b[M,D] text embeddings, both
 * row-major; similarities <a_i, b_j> are exact-f32 products (f32-input MFMA, k ascending) and the N x M matrix is never
 * written to memory: a workgroup owns 64 rows of a and a chunk of b and keeps only counts / short lists. */
/* rank[i] = 1 + #{ j : <a_i,b_j> > <a_i,b_label[i]> }: the rank of the paired report, ties not counted (the paired
 * similarity comes out of the same arithmetic, so a text never outranks itself); label[i] outside [0, M) gives rank[i] = -1
 * [ref: evaluator.py:226-240 (cosine_similarity + one argsort per image)] */
int mc_sim_rank(const float* a, const float* b, const int* label, int* rank, int N, int M, int D, void* stream);
/* per row the k largest similarities and their text indices, score descending then index ascending; 1 <= k <= 32, k <= M.
 * ws: mc_sim_topk_ws_bytes(N, M, k) bytes (O(N * k * splits)); the result does not depend on the split of M
 * [ref: evaluator.py:226-232 (the head of the per-image argsort)] */
long long mc_sim_topk_ws_bytes(int N, int M, int k);
int mc_sim_topk(const float* a, const float* b, float* vals, int* idx, int N, int M, int D, int k, void* ws, void* stream);
/* number of chunks M is split into by mc_sim_rank / mc_sim_topk: 0 = chosen per call (enough workgroups to fill the device
 * when N is small), 1..64 = fixed (capped at the number of 128-text tiles).  Process-wide developer / test switch. */
int mc_sim_set_splits(int splits);
/* p[i,:] = softmax_j <a_i, b_j> over the M prompts, any M >= 1 [ref: evaluator.py:173] */
int mc_sim_softmax(const float* a, const float* b, float* p, int N, int M, int D, void* stream);
/* counts[0] = #{(p,n): score_p > score_n}, counts[1] = #{score_p == score_n} over all (positive, negative) pairs,
 * counts[2] = positives (label != 0), counts[3] = negatives (label == 0); 64-bit integer atomics.  The host finishes
 * AUROC = (counts[0] + 0.5 counts[1]) / (counts[2] counts[3]), the Mann-Whitney form of roc_curve + auc
 * [ref: evaluator.py:176-177,180-181,188-189] */
int mc_auroc_counts(const float* score, const int* label, long long* counts, int N, void* stream);
/* Binary-classification metrics of one finding without a sort.  score fp32 [N], label int32 [N]
 * (0 or 1; the kernels take label != 0 as positive and COUNT the others in the record), 1 <= N <= 2^24: counts fit 32 bits and
 * count products fit 64-bit integers and fp64 exactly.  No float atomics anywhere: integer atomics for the counts, fp64 sums
 * as per-workgroup partials added in a fixed order (the mc_ordered_sum pattern), so two calls return the same bits.
 *
 * counts [N][5], per sample i: positives / negatives j with s_j >= s_i (i included) = (TP, FP) at threshold s_i; the same
 * with s_j > s_i = (TP, FP) at the next higher distinct threshold, (0, 0) at the curve's start; #{j < i : s_j == s_i}, which
 * is 0 for exactly one sample per distinct score (the representative of that threshold).  All pairs are compared from LDS
 * tiles of 2048 partners, like mc_auroc_counts.
 * [ref: evaluator.py:301-309 (pfbeta_binarized: one pass over the samples per positive), 340-346 (precision_recall_curve)] */
int mc_rank_counts(const float* score, const int* label, unsigned int* counts, int N, void* stream);
/* record: 20 eight-byte slots.  Integers [0..16): n_pos, n_neg; the AUROC pair counts gt = sum_pos (n_neg - neg_ge) and
 * eq = sum_pos (neg_ge - neg_gt); tp, fp and the score (fp32 bits in the low word) of the best-pF1 threshold among the
 * positives' scores -- 2 tp / (tp + fp + n_pos) compared exactly as a cross product, the higher threshold on equal value,
 * (0, 0, -inf) without a positive; tp, fp, tn, fn at `threshold` with (double) score >= threshold predicted positive; the
 * number K of distinct scores; the number of NaN scores; the number of labels outside {0, 1}; two spare slots (0).
 * fp64 [16..20): PR-AUC = sum over representatives of (R1 - R0)(P1 + P0)/2 and average precision = sum of (R1 - R0) P1
 * (P = tp/(tp+fp), R = tp/n_pos, P0 = 1 at the start point; NaN without a positive); sum of clip(s, 0, 1) over the positives
 * and over the negatives.  counts == NULL: only the fields that need no counts (n_pos, n_neg, the threshold's four, NaN and
 * label counts, clip sums); the others are 0 / NaN.  ws: mc_cls_record_ws_bytes(N) bytes (0 for N out of range).
 * [ref: evaluator.py:301-346 (pfbeta_binarized, auroc, pfbeta, pr_auc); Classifiers/experiments.py:58,66-69 (pred >= 0.5)] */
long long mc_cls_record_ws_bytes(int N);
int mc_cls_record(const float* score, const int* label, const unsigned int* counts, int N, double threshold, long long* record,
                  void* ws, void* stream);
/* the integer PR / ROC curve: tp[k], fp[k], threshold[k] of the k-th distinct score in ascending order, K = the record's
 * number of distinct scores (an entry whose position is >= K is not written); pos_ws: N words of scratch
 * [ref: evaluator.py:341-344 (pr_auc(get_all=True): precision = tp/(tp+fp), recall = tp/n_pos, finished by the caller)] */
int mc_cls_curve(const float* score, const unsigned int* counts, int N, int K, unsigned int* pos_ws, int* tp, int* fp,
                 float* threshold, void* stream);
/* B bootstrap replicates of the record: records [B][20], replicate r = mc_cls_record's 20 slots on the
 * multiset of N samples drawn with replacement (NaN and label counters 0; K = the distinct scores present; a score absent
 * from a replicate is no threshold of it).  Draw t of replicate r takes sample (u N) >> 32 with u = word t & 3 of
 * philox4x32(t >> 2, r, 0x626f6f74, 0x5bd1e995; key seed low, seed high) -- a function of (seed, r, t, N) only, never of
 * the scores.  stratified != 0: draws t < n_pos take the ((u n_pos) >> 32)-th positive in index order, the others the
 * ((u n_neg) >> 32)-th negative, so every replicate keeps the class counts.  counts: what mc_rank_counts wrote for these
 * scores and labels; bin = N - pos_ge - neg_ge orders the thresholds, so no sort runs (a sample the counts do not place, e.g.
 * a NaN score, is folded into the highest bin: check the point record's counters first).  A replicate is a histogram
 * [bin][class] filled by integer atomics, then one workgroup scans it from the highest bin down: gt, eq and the threshold's
 * four in integers, the best-pF1 candidate by mc_cls_record's exact order, the fp64 sums per thread in scan order and over
 * the threads in a fixed tree.  No float atomics; the same bits on every call, on any stream and for any chunk size.
 * 1 <= N <= 2^24, 1 <= B <= 2^20.  ws: ws_bytes >= mc_boot_ws_bytes(N, B) bytes (0 for arguments out of range), 16-byte
 * aligned: the tables (16 N bytes) plus the histograms of one chunk of replicates (8 N bytes each, about 64 MiB per chunk). */
long long mc_boot_ws_bytes(int N, int B);
int mc_boot_records(const float* score, const int* label, const unsigned int* counts, int N, int B, double threshold,
                    unsigned long long seed, int stratified, long long* records, void* ws, long long ws_bytes, void* stream);
/* replicates per chunk of mc_boot_records: 0 = chosen per call (64 MiB of histograms), 1..65535 = fixed (capped at B);
 * mc_boot_ws_bytes follows it and the records do not depend on it.  Process-wide developer / test switch. */
int mc_boot_set_chunk(int chunk);
/* which stages mc_boot_records launches: bit 0 the tables and the histograms, bit 1 the record scan; 3 (the default) is the
 * op, 1 and 2 exist to time each kernel on its own (scripts/boot_metrics_bench.py).  Process-wide developer switch. */
int mc_boot_set_stages(int mask);

/* ------------------------------------------------------------------------------------------------
 * training augmentation (augment.hip): flips, affine and elastic warp of the reference's train transform as one gather per
 * output pixel, all integer; the specification is the docstring of mammo_clip_amd/augment.py and the
 * result equals its numpy path byte for byte [ref: data/data_utils.py:25-62; data/datasets/imagetext.py:126-160].
 * src: one uint8 plane per source image, element (i, y, x) at src[i*sn + y*sh + x*sw] (any strides, e.g. a channel of an HWC
 * array); params: device int32 [n_out][16] rows (source index, flags, Q16 inverse affine, alpha_q8, seed; a row whose source
 * index is outside [0, n_src) reads nothing and writes zeros); taps: device int32 [2*radius + 1], sum 32768;
 * dst: dense uint8 [n_out][3][h][w].  1 <= h, w <= 16384; 1 <= radius <= min(128, min(h, w) - 1).
 * ws: ws_bytes >= mc_augment_ws_bytes(1, h, w) bytes; the images are worked through in chunks of as many as fit, and the
 * result does not depend on the chunking.  mc_augment_ws_bytes returns 0 for extents outside the range. */
long long mc_augment_ws_bytes(int n_out, int h, int w);
int mc_augment_u8(const unsigned char* src, long long sn, long long sh, long long sw, int n_src, const int* params, int n_out,
                  const int* taps, int radius, int h, int w, unsigned char* dst, void* ws, long long ws_bytes, void* stream);
/* which of the two kernels mc_augment_u8 launches: bit 0 the noise + horizontal pass, bit 1 the vertical pass + warp; 3 (the
 * default) is the op, 1 and 2 exist to time each kernel on its own (scripts/augment_bench.py).  Process-wide developer switch. */
int mc_augment_set_stages(int mask);

/* ------------------------------------------------------------------------------------------------
 * optimizer step of the hot loop [ref: breastclip/optimizer/__init__.py:28-29 ->
 * torch.optim.AdamW(model.parameters(), lr, weight_decay); trainer_ddp.py:300-303].  Multi-tensor, in place, fp32:
 *   p -= lr*wd*p;  m += (1-b1)(g-m);  v = b2*v + (1-b2) g*g;  p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
 * `tensors` is a HOST array of device pointers (one entry per parameter); `step` = t >= 1 (after increment).
 * The LR schedule [ref: breastclip/scheduler/warmup_cosine.py:41-50] is a host scalar: pass the scheduled lr.
 * Hyper-parameters are doubles: the derived scalars (1-b2, bias corrections) are formed in double as torch does. */
typedef struct {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    long long numel;
    mc_bf16* bf16_image;   /* optional: bf16 copy of the updated parameter (same element order), or NULL */
} mc_adamw_tensor;
int mc_adamw_step(const mc_adamw_tensor* tensors, int n_tensors, double lr, double beta1, double beta2, double eps,
                  double weight_decay, long long step, void* stream);
/* Loss-scaled step of the f16 storage build [ref: trainer.py:271-278: the reference's backward runs under
 * torch.cuda.amp.GradScaler; scaler.step() unscales the gradients and skips the update when one of them is inf / nan]:
 * grad[i] *= inv_scale in place for every tensor of the list (only .grad and .numel are read), *found_inf (a device
 * float, zeroed by the caller) is set to 1 if any unscaled value is not finite. */
int mc_grads_unscale(const mc_adamw_tensor* tensors, int n_tensors, float inv_scale, float* found_inf, void* stream);
/* The same step with NO host synchronisation (round 5): the dynamic scale, the non-finite flag and the skip decision stay on
 * the device, like torch's own GradScaler keeps them [ref: trainer_ddp.py:296-303 scaler.scale / step / update].
 *   state = float[8] on the device: {scale, clean steps in a row, found_inf of the step in flight, steps skipped, outcome of
 *           the last step (1 = skipped), -, -, -}
 *   mc_grads_unscale_dev : grad *= 1 / *scale_dev, sets *found_inf (= &state[2]) on a non-finite value
 *   mc_adamw_step_ls     : mc_adamw_step that does nothing when *found_inf != 0 and takes its bias corrections from the number
 *                          of APPLIED steps, step - *skipped (skipped = the optimizer's own device counter)
 *   mc_loss_scale_update : GradScaler.update(): consumes and clears the flag; scale *= backoff on a bad step, *= growth after
 *                          growth_interval clean ones (dynamic != 0); counts the skip in state[3] and in *opt_skipped.
 *                          The scale does not grow past the fp32 range: a grown value that is not finite is dropped (the
 *                          clean-step counter still returns to 0).  The factors are doubles and the product is rounded to
 *                          fp32 once, which is torch's arithmetic bit for bit. */
int mc_grads_unscale_dev(const mc_adamw_tensor* tensors, int n_tensors, const float* scale_dev, float* found_inf, void* stream);
int mc_adamw_step_ls(const mc_adamw_tensor* tensors, int n_tensors, double lr, double beta1, double beta2, double eps,
                     double weight_decay, long long step, const float* found_inf, const float* skipped, void* stream);
int mc_loss_scale_update(float* state, float* opt_skipped, double growth_factor, double backoff_factor, int growth_interval,
                         int dynamic, void* stream);
/* Global L2 norm of the gradients and clipping by it, on the device with no host read [ref: the downstream loops call
 * torch.nn.utils.clip_grad_norm_, Detectors/experiments.py:103].  Only .grad and .numel of the list are read; one workgroup
 * owns one 16384-element chunk of one tensor and writes that chunk's fp64 sum of squares to partials[chunk index of the
 * call]; a last one-workgroup launch adds the partials in a fixed order.  No floating-point atomics: the result is the same
 * bit for bit on every run and stream.
 *   out2[0] = (float)sqrt(sum g^2), the sum and its terms in fp64 (gradients of 1e-25 or 1e25 neither vanish nor overflow)
 *   out2[1] = min(1, max_norm / (out2[0] + 1e-6)), formed in fp32 from the ROUNDED norm the way torch forms the python
 *             expression `max_norm / tensor`: the correctly rounded reciprocal times max_norm.  A nan norm gives a nan
 *             coefficient (torch.clamp(nan, max=1)), max_norm = inf gives exactly 1, an empty list gives norm 0.
 * max_norm must be > 0 (inf allowed; nan is refused).  Every argument is checked before the first launch.
 *   mc_grad_norm_partials     : host arithmetic only: the doubles of workspace the list needs, sum of ceil(numel / 16384);
 *                               -1 on a bad list (negative n_tensors or numel, NULL list with n_tensors > 0)
 *   mc_grad_norm              : norm and coefficient of the gradients as they are; n_partials = capacity of `partials`
 *   mc_grads_unscale_norm_dev : mc_grads_unscale_dev whose workgroups also sum the squares of the values they STORE (the
 *                               fp32-rounded unscaled gradients) with the same per-chunk code as mc_grad_norm: gradients and
 *                               out2 are bit-equal to mc_grads_unscale_dev followed by mc_grad_norm, in one pass
 *   mc_grads_scale_dev        : grad *= *coef in place (one fp32 product per element, no reciprocal): the clip for optimizers
 *                               other than the HIP AdamW
 *   mc_adamw_step_clip        : mc_adamw_step (found_inf = skipped = NULL) or mc_adamw_step_ls (both set) that multiplies
 *                               every gradient by *grad_coef as it loads it -- one fp32 rounding, the product Tensor.mul_
 *                               would have stored.  The gradients in memory are NOT rewritten.  grad_coef is required. */
long long mc_grad_norm_partials(const mc_adamw_tensor* tensors, int n_tensors);
int mc_grad_norm(const mc_adamw_tensor* tensors, int n_tensors, double* partials, long long n_partials, float max_norm,
                 float* out2, void* stream);
int mc_grads_unscale_norm_dev(const mc_adamw_tensor* tensors, int n_tensors, const float* scale_dev, float* found_inf,
                              double* partials, long long n_partials, float max_norm, float* out2, void* stream);
int mc_grads_scale_dev(const mc_adamw_tensor* tensors, int n_tensors, const float* coef, void* stream);
int mc_adamw_step_clip(const mc_adamw_tensor* tensors, int n_tensors, double lr, double beta1, double beta2, double eps,
                       double weight_decay, long long step, const float* grad_coef, const float* found_inf,
                       const float* skipped, void* stream);
/* Exponential moving average of the weights (a shadow model), kept by the optimizer step with no host read.
 * CONTRACT.  For a tensor value p after the optimizer step and its fp32 shadow e, one applied update is three separately
 * rounded fp32 operations, never fused:  s = p - e;  t = w * s;  e = e + t  -- what three tensor operations of torch give on
 * any IEEE host.  w = (float)(1.0 - d_k) with d_k = min(decay, (1.0 + k) / (10.0 + k)) when warmup != 0 and d_k = decay
 * otherwise, in double; k = *count + 1, where *count (a device int64 the caller owns) is the number of updates applied so
 * far.  0 < decay < 1.  Every launch of one update reads *count; mc_ema_tick advances it once, last.  When found_inf is given
 * and *found_inf != 0 (the step the loss scaler skips) no shadow changes and the count stays -- so the tick has to run before
 * mc_loss_scale_update clears the flag.  The count is independent of the optimizer's own `skipped` counter.
 *   mc_adamw_step_ema : the AdamW pass with the shadow update of the same element folded in: `shadows` is a HOST array of
 *                       device pointers parallel to `tensors` (shadows[i] belongs to tensors[i].param; vector path when it is
 *                       16-byte aligned like the others).  grad_coef is optional (NULL: no clip); found_inf / skipped are both
 *                       NULL or both set, as in mc_adamw_step_clip.  Parameters, moments and bf16 images come out bit-equal to
 *                       mc_adamw_step / _ls / _clip with the same arguments.
 *   mc_ema_update     : the stand-alone form over HOST arrays of shadow pointers, source pointers and element counts (buffers,
 *                       parameters the optimizer pass did not cover, other optimizers); found_inf is optional.  Same packing,
 *                       vector path when both pointers of a tensor are 16-byte aligned.
 *   mc_ema_tick       : *count += 1 unless *found_inf != 0 (found_inf optional); one thread.
 * Every argument is checked before the first launch: NULL lists with n_tensors > 0, a decay outside (0, 1) or nan, a NULL
 * count, negative sizes, NULL pointers of non-empty tensors. */
int mc_adamw_step_ema(const mc_adamw_tensor* tensors, float* const* shadows, int n_tensors, double lr, double beta1, double beta2,
                      double eps, double weight_decay, long long step, double decay, int warmup, const long long* count,
                      const float* grad_coef, const float* found_inf, const float* skipped, void* stream);
int mc_ema_update(float* const* shadows, const float* const* sources, const long long* numel, int n_tensors, double decay,
                  int warmup, const long long* count, const float* found_inf, void* stream);
int mc_ema_tick(long long* count, const float* found_inf, void* stream);
/* SGD with momentum, the other optimizer of the reference's factory [ref: breastclip/optimizer/__init__.py:26-27 ->
 * torch.optim.SGD(model.parameters(), **config)].  Multi-tensor, in place, fp32, packed like mc_adamw_step; `tensors` is the same
 * HOST table: exp_avg carries the momentum buffer (NULL allowed when momentum == 0), exp_avg_sq is not read, bf16_image keeps
 * its meaning.  RULE, per element, every operation rounded to fp32 on its own and never fused (what separate tensor operations
 * of torch give on any IEEE host):
 *   g' = maximize ? -g : g
 *   g' = g' * c                                   only with grad_coef (c = *grad_coef, a device scalar; grad is not rewritten)
 *   g' = g' + wd * p                              only if weight_decay != 0
 *   momentum != 0:  buf = g'                                          on the first APPLIED step of the launch set
 *                   buf = mu * buf + (1 - dampening) * g'             otherwise
 *                   d = nesterov ? g' + mu * buf : buf
 *   momentum == 0:  d = g'                        (no buffer is read or written)
 *   p = p - lr * d
 * lr, mu, 1 - dampening (formed in double) and wd are rounded to fp32 once, on the host.  `step` >= 1 is the host's count for
 * the launch set: without a loss scale the first applied step is step == 1; with one (found_inf / skipped both set) it is
 * step - *skipped <= 1, read on the device, and *found_inf != 0 makes the whole call a no-op -- a skipped first step leaves the
 * buffer unwritten and the next applied step sets buf = g'.  `shadows` (optional, a HOST array parallel to `tensors`) folds the
 * weight EMA of mc_ema_update into the pass, applied to the updated p with w from *count exactly as there; decay, warmup and
 * count are ignored when shadows is NULL.  Every argument is checked before the first launch: NULL list, negative size, NULL
 * pointers of non-empty tensors, NULL shadow, half-set loss-scale pair, nesterov without momentum or with dampening, negative
 * lr / momentum / weight_decay, step < 1, decay outside (0, 1), NULL count. */
int mc_sgd_step(const mc_adamw_tensor* tensors, float* const* shadows, int n_tensors, double lr, double momentum, double dampening,
                double weight_decay, int nesterov, int maximize, long long step, double decay, int warmup, const long long* count,
                const float* grad_coef, const float* found_inf, const float* skipped, void* stream);

#ifdef __cplusplus
}
#endif
#endif
