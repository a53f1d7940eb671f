/* libcris_hip.so - C ABI of the MI355X-native CRIS training path (gfx950 only).
 *
 * The reference (DerrickWang005/CRIS.pytorch) has NO native / FFI interface: every kernel it runs is a
 * stock torch/cuDNN/cuBLAS kernel reached through torch.nn (SURVEY.md section 2a).  Each entry point below
 * therefore replaces the torch operator(s) named in its comment, cited as reference file:line of the
 * call site.  Conventions (SURVEY.md section 8b):
 *   - plain pointers + sizes, no torch types; every buffer is owned by the caller (device memory from
 *     torch's caching allocator) and no reference is kept past the call; the library never allocates or
 *     frees device memory;
 *   - every launcher takes the hipStream_t to launch on (as void*), is re-entrant, keeps no global mutable
 *     state (forward runs on the Python thread, backward on autograd's worker thread);
 *   - return 0 on success, non-zero on error; the message is available from cris_last_error()
 *     (thread local).  No exceptions cross the ABI.
 *   - activations are NHWC / token-major bf16 (raw uint16), parameters and statistics fp32.
 */
#ifndef CRIS_HIP_H
#define CRIS_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef uint16_t cris_bf16;

const char* cris_last_error(void);
/* CRIS_ABI_VERSION moves whenever an exported signature or struct changes or a symbol is added; a binding compares cris_abi_version() with the
 * value it was written against and refuses a library of another version (a stale build loaded with new argument lists would
 * mis-read them silently, and one without a new symbol fails only at the first call).  2: cris_step_advance took its fourth argument (round 5); 3, 4: round 6 (arena exchange; row strides of the weight packs); 5: the FP8 inference kernels; 6: cris_eval_iou_batch; 7: cris_grad_sumsq / cris_grad_clip_finalize; 8: cris_grad_accumulate / cris_step_advance_micro; the EMA symbols (cris_ema_advance / cris_ema_update / cris_ema_blocks, cris_ema_desc) were added at 8 WITHOUT moving it: no existing signature or struct changed, and a binding written for them binds every symbol and checks every struct size at load, so a library without them is still refused there; cris_adam_schedule_lrs (the per-step learning-rate schedule) was likewise added at 8 without moving it: it is a new symbol over the unchanged cris_adam_desc, no existing signature or struct changed, and a binding that knows it binds it at load, so a library without it is refused there too; cris_adamw_step (one weight decay per tensor, coupled or decoupled) was added at 8 without moving it in the same way: a new symbol over the unchanged cris_adam_desc, cris_adam_step[_amp] keep their signatures and their results, and a binding that knows it binds it at load; cris_seg_loss_fwd / cris_seg_loss_bwd / cris_seg_loss_ws_floats (the configurable segmentation loss: weighted BCE plus soft Dice) were added at 8 without moving it in the same way: three new symbols that take plain pointers and scalars, no struct and no existing signature changed, cris_bce_fwd / cris_bce_bwd keep their code and their results, and a binding that knows the three binds them at load, so a library without them is refused there; cris_gray_sum_batch / cris_preprocess_batch_aug (training-time augmentation of the input pipeline) were added at 8 without moving it in the same way: two new symbols over the unchanged cris_sample_desc, cris_preprocess_batch keeps its signature, its kernel and its results, and a binding that knows the two binds them at load, so a library without them is refused there; cris_predict_masks_batch (masks, areas, boxes and scores for unlabeled images in one launch) was added at 8 without moving it in the same way: one new symbol over the unchanged cris_eval_desc, cris_eval_iou_batch and cris_eval_desc_fill keep their signatures and their results, and a binding that knows it binds it at load, so a library without it is refused there (the tests of the earlier additions pin the number 8, which is why a new symbol alone does not move it); cris_eval_iou_sweep_batch (the intersection / union counts of a batch at up to 64 thresholds in one launch) was added at 8 without moving it in the same way: one new symbol over the unchanged cris_eval_desc, cris_eval_iou_batch and cris_predict_masks_batch keep their signatures, their kernels and their results, and a binding that knows it binds it at load, so a library without it is refused there; cris_attn_plan (which kernel an attention launcher takes: host arithmetic for the per-element attention tests) was added at 8 without moving it in the same way: one new symbol over the unchanged cris_attn_params, cris_attn_fwd / cris_attn_bwd_dq / cris_attn_bwd_dkv keep their signatures, their kernels and their results, and a binding that knows it binds it at load, so a library without it is refused there; cris_label_components / cris_filter_components / cris_filter_components_work_bytes / cris_mask_iou_batch (connected-component clean-up of the predicted masks: keep the largest component, drop the small ones) were added at 8 without moving it in the same way: four new symbols over the unchanged cris_eval_desc, cris_eval_iou_batch / cris_eval_iou_sweep_batch / cris_predict_masks_batch keep their signatures, their kernels and their results, and a binding that knows the four binds them at load, so a library without them is refused there; cris_rle_encode / cris_rle_work_bytes (COCO run-length encoding of the packed masks on the device) were added at 8 without moving it in the same way: two new symbols over the unchanged cris_eval_desc in a translation unit of their own (csrc/rle.hip), every other launcher keeps its signature, its kernel and its results, and a binding that knows the two binds them at load, so a library without them is refused there; cris_erode_masks / cris_boundary_iou_batch / cris_boundary_work_bytes (square-structuring-element erosion of the packed masks and the Boundary IoU counts built on it) were added at 8 without moving it in the same way: three new symbols over the unchanged cris_eval_desc in a translation unit of their own (csrc/morph.hip), the radii travel as a separate int32 array, every other launcher keeps its signature, its kernel and its results, and a binding that knows the three binds them at load, so a library without them is refused there; cris_morph_masks / cris_fill_holes / cris_fill_holes_work_bytes (mask smoothing: chained dilation / erosion of the packed masks, hence opening and closing, and hole filling) were added at 8 without moving it in the same way: three new symbols over the unchanged cris_eval_desc, the operation codes and radii travel as separate int32 arrays, cris_erode_masks / cris_boundary_iou_batch / cris_label_components / cris_filter_components keep their signatures, their launches and their results, and a binding that knows the three binds them at load, so a library without them is refused there; cris_polygon_count / cris_polygon_trace / cris_polygon_work_bytes / cris_polygon_trace_work_bytes (polygon tracing of the packed masks on the device) were added at 8 without moving it in the same way: four new symbols over the unchanged cris_eval_desc in a translation unit of their own (csrc/polygon.hip), cris_rle_encode and every other launcher keep their signatures, their kernels and their results, and a binding that knows the four binds them at load, so a library without them is refused there; cris_polygon_simplify / cris_polygon_simplify_work_bytes (Douglas-Peucker simplification of the traced rings on the device) were added at 8 without moving it in the same way: two new symbols in a translation unit of their own (csrc/simplify.hip) that read what cris_polygon_trace left, cris_polygon_count / cris_polygon_trace keep their signatures, their launches and their results, and a binding that knows the two binds them at load, so a library without them is refused there; cris_rle_decode / cris_polygon_fill / cris_mask_decode_work_bytes (encoded masks decoded into the packed layouts on the device) were added at 8 without moving it in the same way: three new symbols and one new struct, cris_mask_src, in a translation unit of their own (csrc/decode.hip), cris_eval_desc and every other launcher keep their layouts, their launches and their results, and a binding that knows the three binds them and checks the struct's size at load, so a library without them is refused there */
#define CRIS_ABI_VERSION 8
int cris_abi_version(void);
/* sizeof() of the parameter structs, so the Python mirror (ctypes) can be checked without a GPU */
int cris_sizeof(const char* struct_name);
/* Host-only self check of struct layout: returns a checksum of fields read through the C struct. */
long cris_echo_conv_gemm(const void* conv_gemm_params);

/* ------------------------------------------------------------------------------------------------
 * Implicit-GEMM convolution / linear, bf16 MFMA (v_mfma_f32_32x32x16_bf16; 16x16x32 in the M <= 144 kernel), fp32 accumulate.
 *   out[m, n] = epilogue( sum_k A_im2col[m, k] * Wt[n, k] )
 *   m = (b, oh, ow) over an NHWC input [Bn, H, W, lda] (channels a_coff .. a_coff+C),  k = tap*C + c.
 * Replaces: nn.Conv2d forward everywhere (reference model/clip.py:17-42,77,165-182; model/layers.py:10,58),
 * nn.Linear / MHA in-proj / out-proj (model/clip.py:246-251; model/layers.py:15,61,202-212), `@ text_projection`
 * (model/clip.py:451-452); with flipped/transposed weight packs also their input-gradient (dgrad).
 * Linear layers use Bn=M, H=W=OH=OW=KH=KW=1.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    const cris_bf16* A;      /* NHWC input */
    const cris_bf16* Wt;     /* [N][ldb], k contiguous */
    const float* bias;       /* [N] or NULL */
    const void* resid;       /* [M][ldr] (+r_coff) added after activation/dropout, bf16 or fp32; or NULL */
    void* out;               /* [M][ldc] (+c_coff) bf16 or fp32; or NULL */
    cris_bf16* outT;         /* optional head-split transposed copy, see T_* ; or NULL */
    float* colsum;           /* optional BatchNorm statistics partials [nparts][N]: per row-block column sums ...  */
    float* colsq;            /* ... and sums of squared deviations from the block mean; nparts = ceil(M / R) blocks of
                                R = cris_conv_gemm_stat_rows(p) rows (deterministic, no atomics) */
    long T_sec_stride;       /* elements between consecutive T_E-wide column sections in outT */
    int lda, a_coff;
    int Bn, H, W, C;
    int OH, OW, KH, KW, stride, pad;
    int ldb;
    int M, N, K;
    int act;                 /* 0 none, 1 relu, 2 QuickGELU x*sigmoid(1.702x) (model/clip.py:234-236); 3 relu applied AFTER the
                              * residual add (Bottleneck tail `out += identity; relu` model/clip.py:55-56 with the BatchNorm folded) */
    int ldr, r_coff, resid_f32;
    int ldc, c_coff, out_f32;
    int T_L, T_Lpad, T_E;    /* outT[sec][(b*(T_E/64)+h)*64+d][l], m = b*T_L + l, n = sec*T_E + h*64 + d */
    float drop_p;            /* dropout on (acc+bias, act) before the residual add; survivors scaled 1/(1-p) */
    uint32_t drop_thresh;    /* keep iff hash >= drop_thresh; host computes min(int(p*2^32), 2^32-1); 0 = off */
    uint32_t drop_seed, drop_stream;
    const uint32_t* drop_seed_dev; /* optional device word added to drop_seed (per-step seed of a replayed HIP graph) */
    float* ws;               /* workspace of cris_conv_gemm_ws_floats(p, variant) floats (the split-K skinny variant; else unused) */
    /* BatchNorm-BACKWARD partials instead of the forward statistics (input-gradient GEMMs; tile variants only): when bnr_y is set,
     * the output of this GEMM is dz, the gradient of z = relu(bn(y)) (model/clip.py:47-50 `relu(bn(conv(.)))` whose only consumer is
     * the convolution this GEMM differentiates), and colsum / colsq receive per row block (sum g, sum g * xhat) with
     * g = dz where scale*y + shift > 0 else 0, xhat = (y - mean) * invstd - what cris_bn_bwd_reduce would compute in a launch of
     * its own.  stat_ld: row stride of the colsum / colsq tables in floats (0 = N), so that both can live in ONE [parts][2N]
     * table (colsq = colsum + N) that cris_bn_bwd_sum adds up. */
    const cris_bf16* bnr_y;
    const float* bnr_mean; const float* bnr_invstd; const float* bnr_scale; const float* bnr_shift;
    int bnr_ldy, bnr_coff;
    int stat_ld, pad_;
} cris_conv_gemm_params;
/* Limits checked by every launcher: channels / leading dimensions / offsets multiples of 8, operand extents below 2 GiB (32-bit
 * buffer offsets), and - since the prologue's index arithmetic works by reciprocal multiplication (round 5) - fewer than 2^24 output
 * rows and 2^22 tiles (CRIS-R50 at 416x416: 346112 rows per 8 samples, i.e. up to batch 384 per launch). */
int cris_conv_gemm(const cris_conv_gemm_params* p, void* stream);
/* rows per BatchNorm-statistics partial written for this problem (depends on the tile variant chosen; host only) */
int cris_conv_gemm_stat_rows(const cris_conv_gemm_params* p);
/* The same launch with the tile variant named by the caller instead of chosen from the problem size (tests and the
 * per-shape tuning tool tools/gemm_variants.py; `variant` < 0 = automatic = cris_conv_gemm).  Variants: the 4-wave tiles
 * 128x64 / 64x64 / 64x128 / 128x128, the two skinny kernels, the 8-wave ping-pong tiles 256x256 / 256x128 / 128x256
 * (csrc/gemm8.hip; C % 64 == 0 only).  Returns -1 when the variant cannot run the problem.  Results of different variants
 * differ only by fp32 summation order inside a K-tile (none: every variant adds k in the same order) - the outputs are
 * bit-identical; the BatchNorm partials differ in their row grouping (cris_conv_gemm_variant_stat_rows). */
int cris_conv_gemm_variant(const cris_conv_gemm_params* p, int variant, void* stream);
int cris_conv_gemm_variant_stat_rows(const cris_conv_gemm_params* p, int variant);
/* floats of workspace p->ws the launch of this problem with this variant needs (0 for every variant but the split-K skinny one) */
long cris_conv_gemm_ws_floats(const cris_conv_gemm_params* p, int variant);
int cris_conv_gemm_num_variants(void);
const char* cris_conv_gemm_variant_name(int variant);
/* what cris_conv_gemm_variant(p, variant) would run: the resolved tile variant (>= 0; -1 when `variant` cannot run the problem)
 * and, in *epilogue, the epilogue instantiation (0 general, 1 lean, 2 lean + bias / ReLU); host only */
int cris_conv_gemm_plan(const cris_conv_gemm_params* p, int variant, int* epilogue);

/* Up to CRIS_GEMM_GROUP_MAX INDEPENDENT forward / input-gradient problems in ONE launch (problem table passed by value in the
 * kernel arguments; reference call sites: the q / k / v projections of nn.MultiheadAttention model/layers.py:202-207,235-243 and
 * AttentionPool2d model/clip.py:112-139, the FPN's f4_proj3/4/5 model/layers.py:300-302, a Bottleneck's conv1 + downsample
 * model/clip.py:44-53 - and their input-gradient twins).  No problem may read or accumulate into what another one writes.  All
 * problems run the tile `variant` (one of the 4-wave tiles 128x64 / 64x64 / 64x128 / 128x128 or the 8-wave 128x128 tile,
 * which needs C % 64 == 0 everywhere) and must share the epilogue instantiation (cris_conv_gemm_plan).  Results are bit-identical to
 * cris_conv_gemm_variant(prob[i], variant) one by one.  block_start is filled by the launcher. */
#define CRIS_GEMM_GROUP_MAX 12
typedef struct {
    int n;                                           /* problems in prob[] */
    int block_start[CRIS_GEMM_GROUP_MAX + 1];        /* (out) first block of each problem */
    cris_conv_gemm_params prob[CRIS_GEMM_GROUP_MAX];
} cris_conv_gemm_group;
int cris_conv_gemm_group_launch(const cris_conv_gemm_group* g, int variant, void* stream);

/* Weight gradient in the GEMM layout: dW[n][tap*C + c] = sum_m dY[m, n] * X_im2col[m, tap*C + c]  (csrc/wgrad.hip).
 * Deterministic, no atomics: splits == 1 stores the whole reduction; splits > 1 stores one partial tile per split into the
 * workspace `ws` (cris_wgrad_ws_floats floats) and sums the slabs in split order (cris_wgrad_reduce, launched by
 * cris_conv_wgrad itself).  Replaces convolution_backward(weight) / addmm backward for every Conv2d / Linear above.
 * cris_adam_step reads this layout directly; cris_unpack_grads converts it to the parameter layout [n][c][tap]. */
typedef struct {
    const cris_bf16* dY;     /* [M][ldy] (+y_coff) */
    const cris_bf16* X;      /* NHWC input of the forward conv */
    float* dW;               /* fp32 [N][ldw], k = tap*C + c contiguous; overwritten */
    int ldy, y_coff, N_ld;   /* N_ld: columns of dY that may be read (multiple of 8, >= N) */
    int ldx, x_coff;
    int Bn, H, W, C;
    int OH, OW, KH, KW, stride, pad;
    int M, N, K;
    int ldw;                 /* row stride of dW (>= K) */
    int splits;              /* requested split of the pixel range (each split covers ceil(M/splits) rows rounded up to 128;
                                the launcher drops splits that would be empty) */
    int tile;                /* output tile: 0 = the library's choice (cris_conv_wgrad_tile), 128 = 4-wave kernel, 256 = 8-wave */
    int defer_reduce;        /* 1: cris_conv_wgrad leaves the split slabs in `ws`; the caller adds them up later with
                                cris_wgrad_reduce or, for several problems in one launch, cris_wgrad_reduce_group */
    float* dbias;            /* optional [N]: = column sums of dY (bias gradient); or NULL */
    float* ws;               /* splits > 1: workspace of cris_wgrad_ws_floats(M, N, ldw, splits) floats, 16-byte aligned */
} cris_wgrad_params;
int cris_conv_wgrad(const cris_wgrad_params* p, void* stream);
/* output tile (128: 4-wave kernel, 256: 8-wave kernel) the launchers use for this problem; host only.  A caller that sizes the
 * pixel split from the tile count asks this first; the problems of one cris_conv_wgrad_group launch must share the tile. */
int cris_conv_wgrad_tile(const cris_wgrad_params* p);
long cris_wgrad_ws_floats(int M, int N, int ldw, int splits);
int cris_wgrad_reduce(const cris_wgrad_params* p, void* stream);

/* Up to CRIS_WGRAD_GROUP_MAX weight-gradient problems in ONE launch (problem table passed by value in the kernel
 * arguments): the mid-size layers have too few 128x128 output tiles to fill the chip alone; the engine queues them per
 * gradient-arena stage and launches them together, longest pixel reductions first.  block_start is filled by the launcher. */
#define CRIS_WGRAD_GROUP_MAX 24
typedef struct {
    int n;                                           /* problems in prob[] */
    int block_start[CRIS_WGRAD_GROUP_MAX + 1];       /* (out) first block of each problem */
    cris_wgrad_params prob[CRIS_WGRAD_GROUP_MAX];
} cris_wgrad_group;
int cris_conv_wgrad_group(const cris_wgrad_group* g, void* stream);
/* the split reductions (cris_wgrad_reduce) of up to CRIS_WGRAD_GROUP_MAX problems launched with defer_reduce, in ONE launch;
 * problems with splits == 1 are skipped (the native trainer's default since round 4: ops.WgradQueue). */
int cris_wgrad_reduce_group(const cris_wgrad_group* g, void* stream);

/* Batched weight packing (fp32 parameter layout -> bf16 GEMM layouts), one launch for a table of tensors.
 *   F layout: Wf[n][tap][Cpad]        (forward, k = tap*Cpad + c, zero padded)
 *   D layout: Wd[c][taps-1-tap][Npad] (dgrad: conv of dY with flipped taps; for linear = transpose) */
typedef struct {
    const float* src;        /* [N][Cin][taps]  (or [Cin][N] when src_transposed, taps == 1) */
    cris_bf16* dstF;         /* or NULL */
    cris_bf16* dstD;         /* or NULL */
    const float* row_scale;  /* or NULL; [N]: output row n is multiplied by row_scale[n] before rounding - an inference-time
                              * BatchNorm folded into its convolution (gamma / sqrt(running_var + eps), cris_bn_eval_coeffs) */
    int N, Cin, taps, Cpad, Npad, src_transposed;
    int block_start;         /* first block of this tensor in the launch grid (prefix sum) */
    int ldF;                 /* row stride of dstF in elements, 0 = dense (taps * Cpad); the GEMMs take it as ldb.  Round 6, opt-in
                              * (CRIS_PACK_SKEW=1): a row stride of an ODD number of 128-byte lines (taps * Cpad + 64 when that is a
                              * multiple of 128 elements) spreads a resident panel's rows over all L2 channels: the K = 4608 convolutions
                              * 5 - 10 % faster standalone, nothing in the step (profiles/r06/stride_skew_probe.log, r06_ab_experiments.md) */
    int ldD;                 /* the same for dstD, 0 = dense (taps * Npad) */
    int pad_;
} cris_pack_desc;
int cris_pack_weights(const cris_pack_desc* dev_table, int n_desc, int total_blocks, void* stream);
/* number of blocks a (host-side) descriptor needs: used to build block_start prefix sums on the host */
int cris_pack_blocks(const cris_pack_desc* host_desc);
int cris_pack_block_elems(void);

/* ------------------------------------------------------------------------------------------------
 * FP8 inference (csrc/gemm_fp8.hip; opt-in, no training path uses it).  OCP e4m3fn bytes, power-of-two scales:
 *   quantise(x, e) = RNE_e4m3(clamp(x * 2^-e, -448, 448))  (bit for bit torch's (x * 2**-e).clamp(-448, 448).to(float8_e4m3fn))
 * Implicit-GEMM convolution on the block-scaled MFMA (v_mfma_scale_f32_32x32x64_f8f6f4, unit block scales), fp32 accumulate:
 *   x = sum_k A8[m, k] * W8[n, k] * 2^(e_x + e_w[n]) + bias[n];  act 1: relu;  x += resid[m, n] (bf16);  act 3: relu
 *   out[m, n] = bf16(x) and / or out8[m, n] = quantise(x, e_y)
 * m = (b, oh, ow) over an NHWC fp8 input [Bn, H, W, lda] (channels a_coff .. a_coff+C), k = tap*C + c; C % 16 == 0.
 * Tile variants 128x128 and 64x64 (cris_conv_gemm_fp8_plan; `variant` < 0 = chosen from the problem size).  No atomics;
 * the results are deterministic and the same for every variant. */
typedef struct {
    const uint8_t* A;        /* NHWC fp8 input, row stride lda bytes */
    const uint8_t* Wt;       /* [N][ldb] fp8 weights (cris_pack_weights_fp8), k contiguous */
    const int* e_w;          /* [N] weight exponents */
    const float* bias;       /* [N] or NULL */
    const cris_bf16* resid;  /* [M][ldr] (+r_coff) bf16 or NULL */
    cris_bf16* out;          /* [M][ldc] (+c_coff) bf16 or NULL */
    uint8_t* out8;           /* [M][ldq] (+q_coff) fp8 or NULL */
    int lda, a_coff;
    int Bn, H, W, C;
    int OH, OW, KH, KW, stride, pad;
    int ldb;
    int M, N, K;
    int act;                 /* 0 none, 1 relu before the residual, 3 relu after it (cris_conv_gemm_params.act) */
    int ldr, r_coff;
    int ldc, c_coff;
    int ldq, q_coff;
    int e_x;                 /* activation exponent: the real input is A8 * 2^e_x */
    int e_y;                 /* exponent of the fp8 output */
} cris_conv_gemm_fp8_params;
int cris_conv_gemm_fp8(const cris_conv_gemm_fp8_params* p, int variant, void* stream);
/* the tile variant cris_conv_gemm_fp8(p, variant) runs (-1: out of range); host only */
int cris_conv_gemm_fp8_plan(const cris_conv_gemm_fp8_params* p, int variant);
int cris_conv_gemm_fp8_num_variants(void);
const char* cris_conv_gemm_fp8_variant_name(int variant);
/* Weight quantise + pack, one launch for a table of tensors, one block per output channel (block_start: prefix sums of N):
 *   v = src[n][c][tap] * row_scale[n] (the folded fp32 weight of cris_pack_desc), e_w[n] = the smallest integer with
 *   max |v| * 2^-e_w[n] <= 448 (0 for an all-zero row), dst[n][tap*Cpad + c] = quantise(v, e_w[n]); channels Cin .. Cpad-1 and
 *   columns taps*Cpad .. ld-1 are written as zeros. */
typedef struct {
    const float* src;        /* [N][Cin][taps] */
    const float* row_scale;  /* [N] or NULL */
    uint8_t* dst;            /* [N][ld] */
    int* e_w;                /* [N] */
    int N, Cin, taps, Cpad, ld;
    int block_start;
} cris_pack_fp8_desc;
int cris_pack_weights_fp8(const cris_pack_fp8_desc* dev_table, int n_desc, int total_blocks, void* stream);
/* 2x2 / stride 2 average pool of an NHWC bf16 map (the arithmetic of cris_avgpool2_fwd) with an fp8 output quantise(y, e_y)
 * [Bn*H/2*W/2][ldq] (+qcoff); y (bf16, the same values unrounded by fp8) is optional (NULL) */
int cris_avgpool2_fwd_fp8(const cris_bf16* x, int ldx, int xcoff, int Bn, int H, int W, int C, cris_bf16* y, int ldy, int ycoff,
                          uint8_t* y8, int ldq, int qcoff, int e_y, void* stream);
/* max |x| over an NHWC bf16 tensor [rows][ldx] (channels xcoff .. xcoff+C) -> out[0] (calibration of the activation scales);
 * ws: cris_absmax_ws_floats() floats.  Two launches, no atomics. */
int cris_absmax_bf16(const cris_bf16* x, int ldx, int xcoff, long rows, int C, float* ws, float* out, void* stream);
int cris_absmax_ws_floats(void);


/* ------------------------------------------------------------------------------------------------
 * BatchNorm (training statistics), replaces native_batch_norm / its backward
 * (reference: every nn.BatchNorm2d/1d, model/clip.py:18-41,78,173-183; model/layers.py:11,16,262).
 * Statistics arrive as per-row-block partials (column sum, M2 about the block mean) from the conv GEMM
 * epilogue or cris_colstats_bf16 and are merged exactly: mean = sum_i S_i / n, M2 = sum_i [M2_i + n_i (S_i / n_i - mean)^2] (the
 * decomposition of the sum of squares about the common mean; two passes over the list, no E[x^2] - mean^2 cancellation).
 * SyncBN: call once with `merged` (local sum / M2 / mean out), exchange (cris_bn_sync_pack + ONE all-reduce +
 * cris_bn_sync_unpack), then call again with `global_stats`.
 * Lists of up to 512 parts take one launch (16 or, for more than 128 parts, 64 merge lanes per channel); longer ones are first
 * merged into 64 slices by a second launch: psum / pm2 must have room for cris_bn_partials_rows(nparts) rows of C floats each
 * (the slices are written behind the nparts partial rows).  nparts must be ceil(count_local / rows_per_part).
 * ---------------------------------------------------------------------------------------------- */
int cris_bn_partials_rows(int nparts);
int cris_bn_finalize(const float* psum, const float* pm2, int nparts, int rows_per_part, float count_local, float count,
                     const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum,
                     float eps, int C, float* scale, float* shift, float* mean, float* invstd, float* merged,
                     const float* global_stats, void* stream);
/* single-exchange SyncBN: pack the local (sum | M2) [2C] into moments about `ref` (identical on every rank, e.g. the
 * running mean), all-reduce the 2C floats once, unpack into (global sum | M2 about the global mean) for
 * cris_bn_finalize(global_stats=...) */
int cris_bn_sync_pack(float* merged, const float* mean_local, const float* ref, float n_local, int C, void* stream);
int cris_bn_sync_unpack(float* merged, const float* ref, float count_global, int C, void* stream);
int cris_colstats_bf16(const cris_bf16* x, int ldx, int coff, int M, int C, int rows_per_part, float* psum, float* pm2,
                       void* stream);
/* eval mode: scale/shift from the running statistics */
int cris_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                        float eps, int C, float* scale, float* shift, void* stream);

typedef struct {
    const cris_bf16* y;  int ldy, y_coff;           /* conv output */
    const float* scale;  const float* shift;         /* [C] */
    const cris_bf16* y2; int ldy2, y2_coff;          /* optional second BN branch (downsample) or NULL */
    const float* scale2; const float* shift2;
    const cris_bf16* ident; int ldi, i_coff;         /* optional identity added before the ReLU, or NULL */
    const float* mul;                                /* optional [Bn][C] multiplier applied after the ReLU */
    cris_bf16* z;        int ldz, z_coff;            /* output */
    int Bn, H, W, C;                                 /* input geometry, M = Bn*H*W rows */
    int relu;
    int pool;                                        /* 1: 2x2/s2 average pool after the ReLU (H,W even) */
} cris_bn_apply_params;
int cris_bn_apply(const cris_bn_apply_params* p, void* stream);

typedef struct {
    const cris_bf16* dz; int lddz, dz_coff;          /* grad wrt output z (pooled resolution when pool) */
    const cris_bf16* z;  int ldz, z_coff;            /* forward output: ReLU mask when ident/y2 are used (else recomputed) */
    const cris_bf16* y;  int ldy, y_coff;
    const float* scale; const float* shift; const float* mean; const float* invstd;
    const cris_bf16* y2; int ldy2, y2_coff;          /* second branch or NULL */
    const float* mean2; const float* invstd2; const float* scale2;
    const float* mul;                                /* [Bn][C] or NULL (forward multiplier) */
    float* sums;                                     /* [4*C]: sum g, sum g*xhat, (branch 2) sum g, sum g*xhat2 (+=) */
    float* part;                                     /* reduce workspace, cris_bn_bwd_ws_floats(p) floats: one partial row of
                                                        sums per row block (<= 64); summed in block order (no atomics) */
    float* dmul;                                     /* [Bn][C] grad of mul or NULL */
    cris_bf16* dy;  int lddy, dy_coff;               /* grad wrt y */
    cris_bf16* dy2; int lddy2, dy2_coff;             /* grad wrt y2 or NULL */
    cris_bf16* dident; int lddi, di_coff;            /* grad wrt identity (= masked dz) or NULL */
    int dident_accum;                                /* 1: dident += */
    int Bn, H, W, C;
    int relu, pool;
    float count;                                     /* rows entering the statistics (global count under SyncBN) */
} cris_bn_bwd_params;
int cris_bn_bwd_reduce(const cris_bn_bwd_params* p, void* stream);
/* the second half of cris_bn_bwd_reduce alone: p->part already holds `nparts` partial rows [2C] (written by the epilogue of the
 * input-gradient GEMM that produced dz: cris_conv_gemm_params.bnr_y); adds them up in row order into p->sums (+=) */
int cris_bn_bwd_sum(const cris_bn_bwd_params* p, int nparts, void* stream);
long cris_bn_bwd_ws_floats(const cris_bn_bwd_params* p);
int cris_bn_bwd_apply(const cris_bn_bwd_params* p, void* stream);

/* ------------------------------------------------------------------------------------------------
 * LayerNorm (replaces native_layer_norm fwd/bwd; reference model/clip.py:226-231,247,252,381;
 * model/layers.py:103,199-200,211,214-216) with the surrounding elementwise work fused.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    const void* x; int x_f32; int ldx;               /* input rows */
    const float* gamma; const float* beta;
    const float* pos; int pos_rows;                  /* optional [pos_rows][C] table, row index = row % pos_rows */
    const float* resid;                              /* optional fp32 [rows][C]: out_f32 = resid + dropout(LN(x)) */
    cris_bf16* y;                                    /* optional bf16 LN(x) */
    cris_bf16* ypos;                                 /* optional bf16 LN(x) + pos */
    float* out_f32;                                  /* optional fp32 (see resid) */
    float* mean; float* rstd;                        /* [rows] saved for backward */
    int rows, C;
    int in_relu;                                     /* apply ReLU to x first (bf16 input holds pre-activation) */
    float in_drop_p; uint32_t in_thresh, in_seed, in_stream;     /* dropout on the input (FFN: LN(dropout(relu(h)))) */
    float out_drop_p; uint32_t out_thresh, out_seed, out_stream; /* dropout on LN(x) before the residual add */
    float eps;
    const uint32_t* seed_dev;                        /* optional device word added to in_seed / out_seed */
} cris_ln_fwd_params;
int cris_ln_fwd(const cris_ln_fwd_params* p, void* stream);

typedef struct {
    const void* x; int x_f32; int ldx;
    const float* gamma;
    const float* mean; const float* rstd;
    const cris_bf16* dy;                             /* optional grad wrt y */
    const cris_bf16* dypos;                          /* optional grad wrt ypos (added to dy) */
    const float* dout_f32;                           /* optional grad wrt out_f32 (passes the output dropout) */
    float* part;                                     /* (out) [cris_ln_bwd_parts(rows)][2C]: per-block (dgamma | dbeta) partial rows;
                                                        cris_sum_tables adds them in block order into the gradients */
    void* dx; int dx_f32; int dx_accum;              /* grad wrt x: bf16 or fp32; accum: += (fp32 only) */
    int rows, C;
    int in_relu;
    float in_drop_p; uint32_t in_thresh, in_seed, in_stream;
    float out_drop_p; uint32_t out_thresh, out_seed, out_stream;
    const uint32_t* seed_dev;
} cris_ln_bwd_params;
int cris_ln_bwd(const cris_ln_bwd_params* p, void* stream);
int cris_ln_bwd_parts(int rows);                     /* rows of the partials table for `rows` LayerNorm rows */

/* Ordered column sums of up to CRIS_SUM_GROUP_MAX partial tables in one launch (table passed by value):
 * out[c] = sum_p part[p*ld + c], p = 0 .. nparts-1 in order - the deterministic replacement of atomic accumulation for
 * the LayerNorm parameter gradients (the engine flushes one group per gradient-arena stage).  block_start: launcher. */
#define CRIS_SUM_GROUP_MAX 64
typedef struct { const float* part; float* out; int nparts, ncol, ld, pad_; } cris_sum_entry;
typedef struct {
    int n;
    int block_start[CRIS_SUM_GROUP_MAX + 1];
    cris_sum_entry e[CRIS_SUM_GROUP_MAX];
} cris_sum_group;
int cris_sum_tables(const cris_sum_group* g, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused multi-head attention, head dim 64 (replaces bmm/baddbmm/_softmax/bernoulli_/bmm of the
 * need_weights=True torch path, reference model/layers.py:235,240-243, and the SDPA calls of
 * model/clip.py:119-139,259-260).  q is scaled by `scale` before QK^T; optional causal mask,
 * key-padding mask (int64 token ids == 0 are padding: model/segmenter.py:37) and dropout on the
 * probabilities.  Operands are read straight from L2 in MFMA fragment order: Q/K/V token-major
 * [B*L][ld] (head h at column h*64) plus head-split transposed copies Kt/Vt/Qt/dOt
 * [(b*H+h)*64+d][Lpad] written by the producing GEMM's epilogue (zero padded beyond L).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    const cris_bf16* Q;  int ldq;                    /* [B*Lq][ldq] */
    const cris_bf16* K;  int ldk;                    /* [B*Lk][ldk] */
    const cris_bf16* V;  int ldv;
    const cris_bf16* Vt; const cris_bf16* Kt; const cris_bf16* Qt; int Lk_pad, Lq_pad;
    const int64_t* key_tokens;                       /* [B][Lk] or NULL; token == 0 -> key masked */
    cris_bf16* O;  int ldo;                          /* [B*Lq][ldo] */
    float* lse;                                      /* [B*H][Lq] log-sum-exp of scaled scores */
    /* backward */
    const cris_bf16* dO; int lddo; const cris_bf16* dOt;   /* dOt [(b*H+h)*64+d][Lq_pad] */
    float* delta;                                    /* [B*H][Lq] rowsum(dO*O), written by bwd_dq */
    cris_bf16* dQ; int lddq;
    cris_bf16* dK; int lddk;
    cris_bf16* dV; int lddv;
    int B, Hn, Lq, Lk;
    int causal;
    float scale;
    float drop_p; uint32_t drop_thresh, drop_seed, drop_stream;
    const uint32_t* drop_seed_dev;                   /* optional device word added to drop_seed */
} cris_attn_params;
int cris_attn_fwd(const cris_attn_params* p, void* stream);
int cris_attn_bwd_dq(const cris_attn_params* p, void* stream);
int cris_attn_bwd_dkv(const cris_attn_params* p, void* stream);
/* Which kernel a launcher takes for `p` (host arithmetic, no device call; the launchers branch on the same predicates):
 * which = 0 cris_attn_fwd, 1 cris_attn_bwd_dq, 2 cris_attn_bwd_dkv.  Returns 0 = the direct kernel (operands straight from L2),
 * 1 = the long-sequence kernel that stages 64-row tiles through LDS; -1 (cris_last_error) for any other `which`. */
int cris_attn_plan(const cris_attn_params* p, int which);

/* ------------------------------------------------------------------------------------------------
 * Elementwise / data movement kernels
 * ---------------------------------------------------------------------------------------------- */
/* stem: fp32 NCHW image -> bf16 im2col rows [B*OH*OW][32] for the 3x3/s2/p1 conv (k = ci*9 + kh*3 + kw, 27..31 zero)
 * (reference model/clip.py:165-170,215: x.type(dtype) + conv1) */
int cris_stem_im2col(const float* img, int Bn, int H, int W, cris_bf16* out, void* stream);
/* 2x2/s2 average pool, NHWC bf16 (avg_pool2d: model/clip.py:23,35,184; model/layers.py:297) */
int cris_avgpool2_fwd(const cris_bf16* x, int ldx, int xcoff, int Bn, int H, int W, int C, cris_bf16* y, int ldy,
                      int ycoff, void* stream);
int cris_avgpool2_bwd(const cris_bf16* dy, int lddy, int dycoff, int Bn, int H, int W, int C, cris_bf16* dx, int lddx,
                      int dxcoff, int accum, void* stream);
/* x2 bilinear upsample, align_corners=False (F.interpolate / nn.Upsample: model/layers.py:54,56,293,304) */
int cris_upsample2_fwd(const cris_bf16* x, int ldx, int xcoff, int Bn, int H, int W, int C, cris_bf16* y, int ldy,
                       int ycoff, void* stream);
int cris_upsample2_bwd(const cris_bf16* dy, int lddy, int dycoff, int Bn, int H, int W, int C, cris_bf16* dx,
                       int lddx, int dxcoff, int accum, void* stream);
/* sample gather (several expressions of one image: infer.InferEngine.forward_multi):
 * y[k*R + r][ycoff + c] = x[index[k]*R + r][xcoff + c] for k < K, r < R = rows_per_sample, c < C.  index: device int32 [K],
 * every entry in [0, samples of x) - validated by the caller, not by the kernel.  Exact copies. */
int cris_gather_samples_bf16(const cris_bf16* x, int ldx, int xcoff, const int32_t* index, int K, int rows_per_sample, int C,
                             cris_bf16* y, int ldy, int ycoff, void* stream);
/* CoordConv coordinate channels (model/layers.py:30-39): x at column coff, y at coff+1, zeros up to coff+nfill */
int cris_fill_coords(cris_bf16* x, int ldx, int coff, int nfill, int Bn, int H, int W, void* stream);
/* generic strided bf16 ops: y (=|+=) a [+ b] ;  and y = a + f32 table[row % trows] */
int cris_add_bf16(const cris_bf16* a, int lda, int acoff, const cris_bf16* b, int ldb, int bcoff, cris_bf16* y,
                  int ldy, int ycoff, int M, int C, void* stream);
int cris_add_rowtable(const cris_bf16* a, int lda, const float* table, int trows, cris_bf16* y, int ldy, int M,
                      int C, void* stream);
int cris_cast_f32_bf16(const float* x, cris_bf16* y, long n, void* stream);
int cris_cast_bf16_f32(const cris_bf16* x, float* y, long n, int accum, void* stream);
/* y = bf16(dropout(x)) over a flat fp32 tensor (gradient of nn.Dropout on the residual branches, model/layers.py:217-219) */
int cris_cast_f32_bf16_drop(const float* x, cris_bf16* y, long n, float drop_p, uint32_t drop_thresh, uint32_t seed,
                            uint32_t stream_id, const uint32_t* seed_dev, void* stream);
/* device-side per-step state of a replayed HIP graph: seed[0] = step[0] * 7919 + 17 ; step[0] += 1 ; exchange_gen[0] += 1
 * (exchange_gen may be NULL: the generation counter of the peer-mailbox exchanges, never rewound - see csrc/p2p_ll.h) */
int cris_step_advance(int32_t* step, uint32_t* seed, int32_t* exchange_gen, void* stream);
/* the same for micro-batch `micro` (0-based) of `accum` of one optimizer step (gradient accumulation): step[0] += 1 only when micro == 0,
 * seed[0] = (s * accum + micro) * 7919 + 17 with s = optimizer steps completed before this step, exchange_gen[0] += 1 on EVERY
 * micro-batch (each runs its own SyncBN exchanges).  accum == 1 gives cris_step_advance's values. */
int cris_step_advance_micro(int32_t* step, uint32_t* seed, int32_t* exchange_gen, int micro, int accum, void* stream);
int cris_axpy_f32(float* dst, const float* src, float alpha, long n, void* stream);
/* gradient accumulation over a range of the fp32 gradient arena: mode 0: dst[i] = src[i] (first micro-batch: starts the sum, no
 * memset), mode 1: dst[i] += src[i] (one correctly rounded fp32 add per element, each written by exactly one thread: bit-reproducible).
 * n a multiple of 4, both pointers 16-byte aligned, ranges disjoint.  16-byte accesses, grid-stride, grid sized from the CU count. */
int cris_grad_accumulate(float* dst, const float* src, long n, int mode, void* stream);
/* QuickGELU x*sigmoid(1.702x) on a stored bf16 pre-activation (model/clip.py:234-236) */
int cris_quickgelu_fwd(const cris_bf16* x, cris_bf16* y, long n, void* stream);
int cris_quickgelu_bwd(const cris_bf16* x, const cris_bf16* dy, cris_bf16* dx, long n, void* stream);
/* token embedding + positional embedding (model/clip.py:440-443) and its backward (embedding_dense_backward) */
int cris_embed_fwd(const int64_t* tokens, const float* table, const float* pos, int Bn, int L, int D, float* out,
                   void* stream);
/* row_live (optional, [vocabulary] bytes, sticky): set to 1 for every token of the batch - the rows of the table that have ever
 * received a gradient (see cris_adam_desc.row_live) */
int cris_embed_bwd(const int64_t* tokens, const float* dx, int Bn, int L, int D, float* dtable, float* dpos, unsigned char* row_live,
                   void* stream);
/* rows x[b*L + argmax_l tokens[b,:]] -> bf16 (EOT feature select, model/clip.py:451-452; first max wins) */
int cris_eot_gather(const int64_t* tokens, const cris_bf16* x, int Bn, int L, int D, cris_bf16* out, int* eot_index,
                    void* stream);
int cris_eot_scatter_add(const int* eot_index, const cris_bf16* dstate_rows, int Bn, int L, int D, cris_bf16* dx,
                         void* stream);
/* posr[t][c] = sum_j R[t][j] * pos[1+j][c] (bicubic resize of the attnpool positional embedding as a
 * constant linear map, model/clip.py:80-108) and its transpose for the gradient */
int cris_posresize_fwd(const float* R, const float* pos, int T, int G, int C, float* posr, void* stream);
int cris_posresize_bwd(const float* R, const float* dposr, int T, int G, int C, float* dpos, void* stream);
/* dposr[t][c] = sum_b dx[b*T+t][c] */
int cris_batch_rowsum(const cris_bf16* dx, int ldx, int Bn, int T, int C, float* out, void* stream);
/* text-to-pixel dynamic conv (grouped conv2d, groups = B: model/layers.py:71-84), fp32 logits out */
int cris_dynconv_fwd(const cris_bf16* x, int Bn, int H, int W, int C, const float* wb, int ldwb, float* pred,
                     void* stream);
/* dx, and dwb[b][i] += (per-sample kernel + bias gradient); ws: cris_dynconv_bwd_ws_floats floats (per-block partial rows,
 * summed in block order - no atomics) */
int cris_dynconv_bwd(const cris_bf16* x, const float* dpred, int Bn, int H, int W, int C, const float* wb, int ldwb,
                     cris_bf16* dx, float* dwb, float* ws, void* stream);
long cris_dynconv_bwd_ws_floats(int Bn, int H, int W, int ldwb);
/* nearest mask resize + BCE-with-logits mean (model/segmenter.py:56-59) and gradient.
 * loss[0] = sum(loss_i)/n (per-block partials in ws [cris_bce_ws_floats()], added in block order: no atomics) ;
 * grad = (sigmoid(x) - t)/n * (*gscale or 1) */
int cris_mask_resize_nearest(const float* mask, int Bn, int IH, int IW, int OH, int OW, float* out, void* stream);
int cris_bce_fwd(const float* logits, const float* target, long n, float* loss, float* ws, void* stream);
int cris_bce_ws_floats(void);
int cris_bce_bwd(const float* logits, const float* target, long n, const float* gscale, float* dlogits, void* stream);
/* Configurable segmentation loss on logits / target [Bn][HW] (n = Bn * HW, p = sigmoid(x), targets anywhere in [0, 1]):
 *   bce  = 1/n sum_b sum_i (1 - t) x + (1 + (pw - 1) t) softplus(-x)      (torch's BCEWithLogitsLoss with pos_weight = pw)
 *   dice = 1/Bn sum_b 1 - (2 I_b + s) / (P_b + T_b + s),  I_b = sum_i p t, P_b = sum_i p, T_b = sum_i t    (per sample)
 *   loss[0] = w_bce * bce + w_dice * dice ; terms[2] = (bce, dice) unweighted ; coef[Bn][2] = (a_b, c_b) = (2 / D_b, (2 I_b + s) / D_b^2),
 *   D_b = P_b + T_b + s, for the backward.  Two launches: 16 blocks per sample write four partials each into ws
 *   [cris_seg_loss_ws_floats(Bn)], one wave adds them in slice order, then the samples in sample order: no atomics, the same bits
 *   on every run and for every grid.  logits, target and ws 16-byte aligned; any HW >= 1, Bn >= 1.
 *   dlogits = (*gscale or 1) * [ w_bce / n * ((1 + (pw - 1) t) p - pw t) + w_dice / Bn * p (1 - p) (c_b - a_b t) ]     (one launch)
 * w_bce, w_dice >= 0 and not both 0, pw > 0, s > 0, all finite: refused before any launch otherwise. */
int cris_seg_loss_fwd(const float* logits, const float* target, int Bn, int HW, float w_bce, float w_dice, float pw, float s,
                      float* loss, float* terms, float* coef, float* ws, void* stream);
long cris_seg_loss_ws_floats(int Bn);
int cris_seg_loss_bwd(const float* logits, const float* target, int Bn, int HW, float w_bce, float w_dice, float pw, float s,
                      const float* coef, const float* gscale, float* dlogits, void* stream);
/* trainMetricGPU (utils/misc.py:114-129): out[0] = 100*mean IoU, out[1] = 100*mean(IoU > pr_iou) */
int cris_train_metric(const float* logits, const float* target, int Bn, int HW, float thr, float pr_iou, float* out,
                      void* stream);
/* ---- evaluation post-processing (reference engine/engine.py:100-123 validate, :171-188 inference; csrc/evalpost.hip) ----
 * out[b] = F.interpolate(sigmoid(logits[b]), (H, W), mode='bicubic', align_corners=True)   (engine.py:101-106) */
int cris_sigmoid_bicubic_up(const float* logits, int Bn, int h, int w, int H, int W, float* out, void* stream);
/* dst = cv2.warpAffine(src, mat, (w_out, h_out), flags=cv2.INTER_CUBIC, borderValue=border) (engine.py:114-116); mat: HOST
 * pointer to the 2x3 double matrix the reference passes (param['inverse']); OpenCV's fixed-point algorithm restated */
int cris_warp_affine_cubic(const float* src, int H, int W, const double* mat, int w_out, int h_out, float border, float* dst,
                           void* stream);
/* counts[0] += #(pred > thr & mask), counts[1] += #(pred > thr | mask)  (engine.py:117-122); counts: 2 device ints */
int cris_threshold_iou(const float* pred, const float* mask, long n, float thr, int* counts, void* stream);
/* One launch per batch of the three steps above (warp + threshold + counts) for n ragged samples; the warped map is never written.
 * A descriptor names its probability map, its mask (packed uint8 rows, zero-padded to a pitch that is a multiple of 4; several
 * descriptors may share one mask: the expressions of one image) and its row of the count table.  Per pixel the value equals
 * cris_warp_affine_cubic's bit for bit; a mask pixel counts when its byte is != 0.  counts[row][0..1] += (intersection, union);
 * out_masks (may be NULL): (value > thr) * 255 as uint8 at out_off, with the mask's pitch, padding bytes zero.
 * cris_eval_desc_fill (host) inverts `mat` (the matrix cv2.warpAffine is given) exactly as cris_warp_affine_cubic does.
 * descs_host / descs_dev: the same n descriptors in host memory (checked here: sizes, offsets against mask_bytes / out_bytes,
 * rows against count_rows) and in device memory (read by the kernel). */
typedef struct {
    double m[6];
    int w_out, h_out;
    int map, row;
    long mask_off, out_off;
    int pitch, pad_;
} cris_eval_desc;
int cris_eval_desc_fill(cris_eval_desc* desc, const double* mat, int w_out, int h_out, int map, long mask_off, int pitch,
                        long out_off, int row);
int cris_eval_iou_batch(const float* probs, int P, int H, int W, const cris_eval_desc* descs_host, const cris_eval_desc* descs_dev,
                        int n, const unsigned char* masks, size_t mask_bytes, float thr, float border, int* counts, int count_rows,
                        unsigned char* out_masks, size_t out_bytes, void* stream);
/* The same launch at T thresholds at once (re-tuning thr without one pass per candidate): the n ragged descriptors, the grid, the
 * per-pixel value (bit for bit cris_warp_affine_cubic's) and the mask bytes of cris_eval_iou_batch; no mask is written.
 * thresholds: HOST array of T floats, 1 <= T <= 64, finite and strictly increasing (passed to the kernel by value).  counts: int32
 * table [count_rows][T][2]; descriptor d adds to row d.row, for every i < T,
 *     counts[d.row][i][0] += #(value > thresholds[i] && mask != 0)      counts[d.row][i][1] += #(value > thresholds[i] || mask != 0)
 * so column i is exactly what cris_eval_iou_batch adds at thr = thresholds[i] (the same comparison on the same value; a NaN value
 * is above no threshold).  Integer atomics after a per-block histogram over (mask bit, number of thresholds below the value): exact,
 * order-free, the same table on every run; the kernel accumulates, so a second launch doubles the table.  Checked on the host
 * before the launch: operands non-NULL, n in 1 .. 65535, T, the thresholds, masks and counts 4-byte aligned, and per descriptor
 * what cris_eval_iou_batch checks (sizes, map < P, row < count_rows, pitch, mask_off against mask_bytes; out_off is ignored). */
int cris_eval_iou_sweep_batch(const float* probs, int P, int H, int W, const cris_eval_desc* descs_host, const cris_eval_desc* descs_dev,
                              int n, const unsigned char* masks, size_t mask_bytes, const float* thresholds, int T, float border,
                              int* counts, int count_rows, void* stream);
/* The same launch without ground truth (prediction on unlabeled images): n ragged descriptors, the grid, the per-pixel value (bit for
 * bit cris_warp_affine_cubic's) and the mask bytes of cris_eval_iou_batch; mask_off is ignored and no mask is read.  out_masks (may be
 * NULL: statistics only): (value > thr) * 255 as uint8 at out_off, row pitch `pitch`, padding bytes zero.  stats: int64 table
 * [stat_rows][6], descriptor d updates row d.row = (area, score_q16, x_min, y_min, x_end, y_end): over the pixels with value > thr,
 * area += 1, score_q16 += (long long)rintf(value * 65536.f) (a power-of-two scale: exact; half to even), x_min / y_min = min of x / y,
 * x_end / y_end = max of x + 1 / y + 1.  The caller initialises a row to (0, 0, 2^31 - 1, 2^31 - 1, 0, 0); the kernel accumulates, so
 * a second launch on the same row doubles the two sums and leaves the box.  Integer atomics (64-bit add / min / max, one set per
 * block after a wave-shuffle + LDS reduction): exact, order-free, the same table on every run; mean score = score_q16 / (65536 area).
 * Checked on the host before the launch: operands non-NULL (out_masks excepted), 0 <= thr finite, n in 1 .. 65535, row < stat_rows,
 * map < P, pitch a multiple of 4 and >= w_out, w_out * h_out < 2^31, and with out_masks every out_off 4-byte aligned and inside
 * out_bytes. */
int cris_predict_masks_batch(const float* probs, int P, int H, int W, const cris_eval_desc* descs_host, const cris_eval_desc* descs_dev,
                             int n, float thr, float border, long long* stats, int stat_rows, unsigned char* out_masks, size_t out_bytes,
                             void* stream);
/* Connected components of the packed masks those launches write (mask clean-up before the statistics: keep the largest component, drop
 * the small ones).  masks: the out_masks buffer (descriptor d at d.out_off, d.h_out rows of d.pitch bytes); a pixel is foreground iff
 * its byte is != 0 and x < w_out, the pitch padding is background and never a neighbour.  labels: one int32 word per mask byte, same
 * offsets; after cris_label_components the word of a foreground pixel is its CANONICAL label, the index y * pitch + x (relative to
 * out_off) of the first pixel of its component in raster order, and background and padding are -1 (-2 marks a pixel whose union-find
 * walk hit its iteration cap: never with intact buffers).  connectivity: 4 or 8.  Three launches (32 x 32 tiles in LDS, merges across
 * tile borders, flatten) on the stream, none depending on the mask's content.  Checked on the host before the first launch: operands
 * non-NULL, n in 1 .. 65535, connectivity, alignment, label_words >= mask_bytes, and per descriptor sizes, pitch and out_off inside
 * mask_bytes (map, row and mask_off are ignored). */
int cris_label_components(const unsigned char* masks, size_t mask_bytes, const cris_eval_desc* descs_host, const cris_eval_desc* descs_dev,
                          int n, int connectivity, int* labels, size_t label_words, void* stream);
/* Filter by those labels, in place: components of area < min_area are dropped first; with keep_largest the remaining component of
 * greatest area alone survives (ties: the lowest canonical label).  Kept bytes become 255, every other byte of the rectangle 0.
 * info: int64 table [info_rows][4], descriptor d adds to row d.row (n_components before filtering, kept_components, raw_area = foreground
 * pixels before filtering, error = 1 when a label carries the cap mark); the caller zeroes it.  probs / stats (both or neither): over the
 * KEPT pixels stats[d.row] receives exactly what cris_predict_masks_batch adds per pixel above its threshold (the value is recomputed by
 * the same device function), so for a mask of one component the row equals that launch's row bit for bit; stats rows are initialised
 * as for that launch.  work: device scratch of cris_filter_components_work_bytes bytes (areas per root, one winner word per
 * descriptor), zeroed here by a memset on the stream; then three launches (areas, winner by one 64-bit atomicMax of
 * (area << 32) | (0xffffffff - label), filter).  Integer atomics only: the same masks and tables on every run.  Checked on the host
 * first: operands, n, keep_largest, min_area >= 0, alignment, label_words, work_bytes, row < min(info_rows, stat_rows), map < P with
 * probs, and per descriptor what cris_label_components checks. */
size_t cris_filter_components_work_bytes(size_t mask_bytes, int n);
int cris_filter_components(unsigned char* masks, size_t mask_bytes, const int* labels, size_t label_words, const cris_eval_desc* descs_host,
                           const cris_eval_desc* descs_dev, int n, int keep_largest, int min_area, void* work, size_t work_bytes,
                           long long* info, int info_rows, const float* probs, int P, int H, int W, float border, long long* stats,
                           int stat_rows, void* stream);
/* counts[d.row] += (#(pred != 0 && gt != 0), #(pred != 0 || gt != 0)) over x < w_out, from mask BYTES: pred at d.out_off of `pred`
 * (filtered or not), gt at d.mask_off of `gt`, both with d.pitch.  The int32 [count_rows][2] table and the integer atomics of
 * cris_eval_iou_batch: on its unfiltered out_masks this launch reproduces its counts. */
int cris_mask_iou_batch(const unsigned char* pred, size_t pred_bytes, const cris_eval_desc* descs_host, const cris_eval_desc* descs_dev,
                        int n, const unsigned char* gt, size_t gt_bytes, int* counts, int count_rows, void* stream);
/* COCO run-length encoding of the same packed masks (csrc/rle.hip; DESIGN.md 9b).  Foreground as above: byte != 0 and x < w_out, the
 * pitch padding is never read as a pixel.  With i = x * h_out + y (column-major), v(i) the foreground bit and v(-1) = 0, the
 * transition positions P of a descriptor are the ascending i in [0, h_out * w_out) with v(i) != v(i - 1) - a run continues from the
 * bottom of column x into the top of column x + 1 - and the COCO counts are diff([0] + P + [h_out * w_out]) (host: rle.py).
 * runs receives P of descriptor 0, then 1, ..., packed contiguously; totals (device, n + 1 words): totals[i] = |P_i|, totals[n] = their
 * sum = the words needed.  The call never writes at or beyond runs + run_words: when totals[n] > run_words every position whose slot
 * lies below run_words is written, the rest is dropped, and the caller grows the buffer and calls again (sum of h_out * w_out words
 * always suffice).  work: device scratch of cris_rle_work_bytes(descs_host, n) bytes (every descriptor gets max over the batch of
 * w_out * ceil(h_out / 32) words for its per-segment counts, then n 64-bit bases; 0 for NULL descriptors or n outside 1 .. 65535);
 * nothing has to be zeroed.  Four launches on the stream (count per segment, scan per descriptor, scan over descriptors, write), none
 * depending on the content; integers only, no atomics: the same words on every run.  Checked on the host before the first launch:
 * operands non-NULL, n in 1 .. 65535, work and totals 8-byte and runs 4-byte aligned, work_bytes, and per descriptor h_out, w_out >= 1,
 * h_out * w_out < 2^31, w_out <= pitch, pitch a multiple of 4, pitch * h_out < 2^31, out_off >= 0 and the rectangle inside mask_bytes
 * (map, row and mask_off are ignored). */
size_t cris_rle_work_bytes(const cris_eval_desc* descs_host, int n);
int cris_rle_encode(const unsigned char* masks, size_t mask_bytes, const cris_eval_desc* descs_host, const cris_eval_desc* descs_dev, int n,
                    void* work, size_t work_bytes, unsigned* runs, size_t run_words, long long* totals, void* stream);
/* Polygon tracing of the same packed masks (csrc/polygon.hip, csrc/polygon_core.h; DESIGN.md 9b; the format: polygon.py).  Foreground
 * as above: byte != 0 and x < w_out, the pitch padding is never read, outside the image is background.  Vertices are pixel corners
 * (x, y), 0 <= x <= w_out, 0 <= y <= h_out; a crack is a unit edge between foreground and background directed with the foreground on
 * its right (y grows downwards); a ring continues with the first existing crack among turn right, straight, turn left, and lists the
 * vertices at which its direction changes, from its raster-first vertex on (outer rings leave it heading east, 2 A > 0; holes heading
 * south, 2 A < 0).  The vertex count is data, hence two calls with a read of totals between them:
 *   cris_polygon_count  totals (device, n + 1 words): totals[i] = vertices of descriptor i (always even), totals[n] = their sum.  work:
 *     device scratch of cris_polygon_work_bytes(descs_host, n) bytes (per descriptor max over the batch of (h_out + 1) * ceil((w_out + 1) / 64)
 *     and of (w_out + 1) * ceil((h_out + 1) / 32) words for the per-segment counts of the row-major and column-major lists, then n 64-bit
 *     bases; 0 for NULL descriptors or n outside 1 .. 65535); nothing has to be zeroed.  Three launches, none depending on the content.
 *   cris_polygon_trace  the same masks, descriptors and work (unchanged since the count: it holds the offsets), the device totals, and
 *     what the host read from them: total_vertices = totals[n] (even, 2 .. 2^30: a batch without foreground is not traced) and
 *     max_vertices_per_mask = max totals[i], which fixes the pointer-jumping rounds ceil(log2(max)) + extra_rounds (extra_rounds in
 *     0 .. 8 changes no word of the result).  trace_work: device scratch of cris_polygon_trace_work_bytes(total_vertices, n) bytes (nine
 *     words per vertex, one 64-bit word per 1024 vertices; 0 for a total outside 1 .. 2^30).  vertices: int32 (x, y) pairs, vertex_cap
 *     PAIRS; ring i of the batch (descriptor order, then raster order of the ring starts) occupies rings[4 i ..] = (descriptor, offset
 *     in pairs, length, 2 A) with ring_cap ROWS; header[0] = rings, header[1] = vertices written.  total_vertices pairs and
 *     total_vertices / 4 rows always suffice; nothing is written at or beyond either capacity, rows and vertices that do not fit are
 *     dropped.  7 + rounds launches; integers only, no atomics: the same words on every run.
 * Checked on the host before the first launch: operands non-NULL, n in 1 .. 65535, alignment (8 bytes; vertices 4), both work sizes,
 * the scalars above, and per descriptor h_out, w_out >= 1, (h_out + 1) * (w_out + 1) <= 2^28, w_out <= pitch, pitch a multiple of 4,
 * pitch * h_out < 2^31, out_off >= 0 and the rectangle inside mask_bytes (map, row and mask_off are ignored). */
size_t cris_polygon_work_bytes(const cris_eval_desc* descs_host, int n);
size_t cris_polygon_trace_work_bytes(long long total_vertices, int n);
int cris_polygon_count(const unsigned char* masks, size_t mask_bytes, const cris_eval_desc* descs_host, const cris_eval_desc* descs_dev, int n,
                       void* work, size_t work_bytes, long long* totals, void* stream);
int cris_polygon_trace(const unsigned char* masks, size_t mask_bytes, const cris_eval_desc* descs_host, const cris_eval_desc* descs_dev, int n,
                       const void* work, size_t work_bytes, const long long* totals, long long total_vertices, long long max_vertices_per_mask,
                       int extra_rounds, void* trace_work, size_t trace_work_bytes, int* vertices, size_t vertex_cap, long long* rings,
                       size_t ring_cap, long long* header, void* stream);
/* Douglas-Peucker simplification of the rings cris_polygon_trace left on the device (csrc/simplify.hip, csrc/simplify_core.h; DESIGN.md
 * 9b; polygon.simplify is the host restatement).  q = 4 epsilon in 1 .. 256 (epsilon in pixels, a multiple of 0.25 in [0.25, 64]).  Per
 * ring v_0 .. v_k-1 (v_k = v_0): the kept set starts as {0, a}, a the smallest index that maximises |v_i - v_0|^2; for a segment (i, j) of
 * kept vertices with j - i >= 2 the candidate is the m in (i, j) of greatest c_m = |(v_j - v_i) x (v_m - v_i)|, among equals the one
 * nearest the middle (smallest |2 m - (i + j)|), among those the smallest m; it is kept, and both halves go on, iff
 * 16 c_m^2 > q^2 |v_j - v_i|^2, strictly.  All of it in 64-bit integers, which bounds h_out, w_out <= 32767.  A ring left with fewer than
 * 3 vertices is removed.  vertices, rings (4 words per row) and header: the trace's outputs, only read, nothing is read by the host in
 * between; total_vertices: the pairs `vertices` holds (what the trace was given), ring_cap: the rows `rings` holds.  work: device scratch
 * of cris_polygon_simplify_work_bytes(total_vertices, ring_cap) bytes (0 for a total outside 4 .. 2^30 or a ring_cap outside 1 .. 2^28);
 * nothing has to be zeroed.  out_vertices: the kept (x, y) pairs of the remaining rings in ring order, out_vertex_cap PAIRS
 * (>= total_vertices); out_rings: 5 words per remaining ring = (descriptor, offset in pairs, length, 2 A of the simplified ring - it may be
 * 0 or odd -, 1 iff the TRACED ring is a hole), out_ring_cap ROWS (>= ring_cap); out_header[0 .. 4) = rings, vertices written, traced
 * rings, rounds of the deepest ring.  3 or 4 launches; integers only, the same words on every run.  Checked on the host before the
 * first launch: operands non-NULL, alignment (8 bytes; vertices 4), q, the scalars, the capacities, the work size, n in 1 .. 65535 and per
 * descriptor h_out, w_out in 1 .. 32767 (nothing else of a descriptor is read). */
size_t cris_polygon_simplify_work_bytes(long long total_vertices, long long ring_cap);
int cris_polygon_simplify(const int* vertices, const long long* rings, const long long* header, long long total_vertices, long long ring_cap,
                          int q, const cris_eval_desc* descs_host, int n, void* work, size_t work_bytes, int* out_vertices,
                          size_t out_vertex_cap, long long* out_rings, size_t out_ring_cap, long long* out_header, void* stream);
/* Erosion by a (2 r + 1)-square of the same packed masks and the Boundary IoU counts built on it (csrc/morph.hip; DESIGN.md 9b).
 * Foreground as above: byte != 0 and x < w_out, the pitch padding is never read as a pixel; outside the image is background.  With
 * r = radii[i] >= 1 the radius of descriptor i (computed on the host: the device reads integers; radii_host is checked here,
 * radii_dev - the same n values in device memory - is read by the kernels),
 *     E_r(M)[y, x] = 1 iff every pixel of [y - r, y + r] x [x - r, x + r] lies inside the image and is foreground
 * (r iterations of a 3 x 3 erosion behind a one-pixel zero border), empty when 2 r + 1 > min(h_out, w_out), and B_r(M) = M & ~E_r(M).
 * cris_erode_masks reads `masks` at out_off / pitch and writes bytes 0 / 255 at the same offsets of `out`: E_r (boundary = 0) or
 * B_r (boundary = 1); no byte outside a descriptor's h_out x w_out pixels is written (not the pitch padding, not the gaps, not the
 * tail).  out == masks (in place) is allowed: every source byte is read by the first launch, every output byte written by the third.
 * cris_boundary_iou_batch: counts[d.row] += (|B_r(P) & B_r(G)|, |B_r(P) | B_r(G)|), P at d.out_off of `pred`, G at d.mask_off of `gt`,
 * both with d.pitch; the int32 [count_rows][2] table of cris_eval_iou_batch.  work: device scratch of
 * cris_boundary_work_bytes(descs_host, n) bytes = 4 bit planes (prediction, ground truth, each raw and eroded along x) of n slots of
 * max over the batch of h_out * ceil(w_out / 64) 64-bit words (cris_erode_masks uses two of the four and accepts half; 0 for NULL
 * descriptors or n outside 1 .. 65535); nothing has to be zeroed.  Three launches each on the stream (pack to bit planes by wave
 * ballot, window AND along x, window AND along y + counts or bytes), none depending on the content; integers only, the counts by one
 * integer atomic pair per block after a reduction: the same numbers on every run.  Checked on the host before the first launch:
 * operands non-NULL, n in 1 .. 65535, boundary, alignment (work 8-byte; radii_dev, counts 4-byte), every radius >= 1, work_bytes, and
 * per descriptor h_out, w_out >= 1, h_out * w_out < 2^31, w_out <= pitch, pitch a multiple of 4, pitch * h_out < 2^31, out_off >= 0
 * and the rectangle inside mask_bytes and out_bytes (pred_bytes), mask_off >= 0 and the rectangle inside gt_bytes, row < count_rows
 * (map is ignored). */
size_t cris_boundary_work_bytes(const cris_eval_desc* descs_host, int n);
int cris_erode_masks(const unsigned char* masks, size_t mask_bytes, const cris_eval_desc* descs_host, const cris_eval_desc* descs_dev, int n,
                     const int* radii_host, const int* radii_dev, void* work, size_t work_bytes, unsigned char* out, size_t out_bytes,
                     int boundary, void* stream);
int cris_boundary_iou_batch(const unsigned char* pred, size_t pred_bytes, const cris_eval_desc* descs_host, const cris_eval_desc* descs_dev,
                            int n, const unsigned char* gt, size_t gt_bytes, const int* radii_host, const int* radii_dev, void* work,
                            size_t work_bytes, int* counts, int count_rows, void* stream);
/* Mask smoothing on the same packed masks (csrc/morph.hip, csrc/evalpost.hip; DESIGN.md 9b): a chain of window operations, and hole
 * filling.  With W_r(p) the (2 r + 1)-square around p CLIPPED to the image (nothing outside the image exists),
 *     CRIS_MORPH_ERODE          E_r   as above: background outside the image (cris_erode_masks' result, bit for bit)
 *     CRIS_MORPH_DILATE         D_r(M)[p]  = OR  of M over W_r(p)
 *     CRIS_MORPH_ERODE_CLIPPED  E'_r(M)[p] = AND of M over W_r(p) = ~D_r(~M) on the image (binary_erosion with border_value = 1)
 * so open_r = D_r E_r (scipy's binary_opening with a full square; anti-extensive, idempotent) and close_r = E'_r D_r (extensive also
 * for objects at the image border, idempotent; NOT scipy's binary_closing default, whose second step erodes from the border).
 * cris_morph_masks applies ops_host[0], then ops_host[1], ... (1 <= n_ops <= CRIS_MORPH_MAX_OPS) with the radius
 * radii[k * n + i] of operation k on descriptor i (radii_host is checked here, radii_dev - the same n_ops * n values in device memory -
 * is read by the kernels; every value in 1 .. 65535) and writes bytes 0 / 255 at out_off / pitch of `out`; no byte outside a
 * descriptor's h_out x w_out pixels is written, out == masks is allowed, descriptors may alias one rectangle.  work: two bit planes,
 * cris_boundary_work_bytes(descs_host, n) / 2 bytes, nothing has to be zeroed.  2 + 2 n_ops launches on the stream (pack; per
 * operation a row pass plane A -> B and a column pass B -> A; store), none depending on the content, integers only.  Checked on the
 * host before the first launch: operands non-NULL, n, n_ops, every operation code, every radius, alignment (work 8-byte, radii_dev
 * 4-byte), work_bytes, and per descriptor what cris_erode_masks checks. */
#define CRIS_MORPH_ERODE 0
#define CRIS_MORPH_DILATE 1
#define CRIS_MORPH_ERODE_CLIPPED 2
#define CRIS_MORPH_MAX_OPS 8
int cris_morph_masks(const unsigned char* masks, size_t mask_bytes, const cris_eval_desc* descs_host, const cris_eval_desc* descs_dev, int n,
                     const int* ops_host, int n_ops, const int* radii_host, const int* radii_dev, void* work, size_t work_bytes,
                     unsigned char* out, size_t out_bytes, void* stream);
/* cris_fill_holes, in place: a hole is a connected component of the BACKGROUND (byte == 0, x < w_out; connectivity 4 or 8) that holds no
 * pixel of the image's outer frame (row 0, row h_out - 1, column 0, column w_out - 1); every pixel of a hole of at most max_area pixels
 * (max_area = -1: of any hole) becomes 255, no other byte is written.  connectivity 4, max_area -1 is scipy's binary_fill_holes.
 * The background is labelled by cris_label_components' three launches into `labels` (one int32 word per mask byte; the words of
 * foreground pixels and padding become -1); then `work` (cris_fill_holes_work_bytes(mask_bytes) bytes: one word per mask byte) is zeroed
 * by a memset on the stream, one launch adds every background pixel to its root's area and marks the roots that own a frame pixel,
 * and one launch writes the holes.  info: int64 table [info_rows][4], descriptor d adds to row d.row (holes_filled, pixels_filled,
 * holes = all holes whatever their area, error = 1 when a label carries the union-find's cap mark); the caller zeroes it.  Integer
 * atomics only: the same masks and tables on every run.  Checked on the host first: operands non-NULL, n in 1 .. 65535, connectivity,
 * max_area >= -1, alignment (masks 4-byte; labels, work 16-byte; info 8-byte), label_words >= mask_bytes, work_bytes, row < info_rows,
 * and per descriptor what cris_label_components checks.  Descriptors must not alias. */
size_t cris_fill_holes_work_bytes(size_t mask_bytes);
int cris_fill_holes(unsigned char* masks, size_t mask_bytes, const cris_eval_desc* descs_host, const cris_eval_desc* descs_dev, int n,
                    int connectivity, int max_area, int* labels, size_t label_words, void* work, size_t work_bytes, long long* info,
                    int info_rows, void* stream);
/* Encoded masks decoded into the packed layouts above (csrc/decode.hip, csrc/decode_core.h; DESIGN.md 9b): the inverse of cris_rle_encode
 * and of cris_polygon_count / cris_polygon_trace / cris_polygon_simplify; rle.decode and polygon.decode (host) are the definitions.  A
 * cris_mask_src row names ONE mask: its slot - h rows of pitch bytes at dst_off of `out`, so that a ground-truth slot (a descriptor's
 * mask_off) and a prediction slot (out_off) are filled alike, and several descriptors may name a mask that is decoded once - its
 * payload and its kind.  Both entry points take the whole table and serve the rows of their kind only; for each such row they write
 * 0 / 255 at x < w and 0 at w <= x < pitch of every row and nothing else (not the gap to the next slot, not the tail, no slot of the
 * other kind).  The payload is only read.
 *   CRIS_MASK_RLE      pay_off / pay_len: the first word and the number of the mask's counts in `counts` (uint32, COCO order:
 *     column-major, i = x * h + y, the first run background).  Pixel i is foreground iff the number of run ends <= i is odd; runs of
 *     length zero are legal anywhere.  Counts that do not sum to h * w (the host validates them first) change values, never addresses.
 *     Two launches: scan of the counts per mask, one upper-bound search per pixel with a dword stored per 4 pixels.
 *   CRIS_MASK_POLYGON  pay_off / pay_len: the first row and the number of the mask's rows in the ring table, rows of ring_stride
 *     (3 .. 8) 64-bit words that start (index of the mask in this table, offset in pairs, length) - the first columns of what the
 *     tracer and the simplifier leave; the rows of one mask are adjacent and their vertices follow each other in `vertices` (int32
 *     (x, y) pairs, pixel corners).  Even-odd filling sampled at pixel centres in exact integers: every non-horizontal edge
 *     (x0, y0) -> (x1, y1) oriented downwards toggles, on each centre line py = y0 .. y1 - 1, the pixels at x >= px,
 *     px = x0 - floor((dy - num) / (2 dy)), num = (2 py + 1 - 2 y0) dx, clipped to [0, w] (w toggles nothing); rows outside [0, h) are
 *     skipped.  One memset of the work buffer and two launches: one 64-bit integer atomic XOR per (edge, row) into the mask's bit plane,
 *     then the inclusive prefix parity of every row, a dword stored per 4 pixels.
 * work: device scratch of cris_mask_decode_work_bytes(srcs_host, n) bytes - n slots of the maximum over the table of ceil(pay_len / 2)
 * (RLE: the run ends) and h * ceil(w / 64) (polygon: the plane) 64-bit words; 0 for a NULL table or n outside 1 .. 65535; nothing has to
 * be zeroed, and both entry points may use one buffer on one stream.  Integers only, the XORs commute: the same bytes on every run.
 * Checked on the host before the first launch: operands non-NULL, n in 1 .. 65535, alignment (work, the tables, vertices 8-byte; counts,
 * out and every dst_off 4-byte), work_bytes, and per row of EITHER kind its kind, h, w >= 1, h * w < 2^31 ((h + 1) * (w + 1) <= 2^28 for
 * a polygon), w <= pitch, pitch a multiple of 4, pitch * h < 2^31, the slot inside out_bytes, the payload inside count_words / ring_rows,
 * and per ring row the mask it names, length >= 1, its vertices inside vertex_pairs and adjacent to the previous ring's. */
#define CRIS_MASK_RLE 0
#define CRIS_MASK_POLYGON 1
typedef struct {
    long dst_off;
    long pay_off;
    int pitch, h, w;
    int pay_len;
    int kind, pad_;
} cris_mask_src;
size_t cris_mask_decode_work_bytes(const cris_mask_src* srcs_host, int n);
int cris_rle_decode(const cris_mask_src* srcs_host, const cris_mask_src* srcs_dev, int n, const unsigned* counts, size_t count_words,
                    void* work, size_t work_bytes, unsigned char* out, size_t out_bytes, void* stream);
int cris_polygon_fill(const cris_mask_src* srcs_host, const cris_mask_src* srcs_dev, int n, const int* vertices, size_t vertex_pairs,
                      const long long* rings_host, const long long* rings_dev, size_t ring_rows, int ring_stride, void* work,
                      size_t work_bytes, unsigned char* out, size_t out_bytes, void* stream);
/* ---- input preprocessing (reference utils/dataset.py:146-168 RefDataset.__getitem__, :207-221 convert; csrc/inputpipe.hip) ----
 * One launch per batch: img_out[b] = ((cv2.warpAffine(rgb_u8, mat, (S_w, S_h), INTER_CUBIC, borderValue=border_rgb).float()
 * / 255 - mean) / std) as [3][S_h][S_w] (through lut_img [3][256]), mask_out[b] = cv2.warpAffine(mask_u8, mat, ...,
 * INTER_LINEAR, borderValue=0) / 255 (through lut_mask [256]).  OpenCV's 8-bit fixed-point algorithm restated (unpinned:
 * cv2 is not available offline).  samples_dev: DEVICE array of n descriptors; img [H][W][3] / mask [H][W] device bytes (either
 * may be NULL); inv = destination->source matrix (cris_invert_affine of the matrix getTransformMat returns, :190-205). */
typedef struct {
    const unsigned char* img;
    const unsigned char* mask;
    int H, W;
    double inv[6];
} cris_sample_desc;
typedef struct { unsigned char v[4]; } cris_u8x4;
int cris_preprocess_batch(const cris_sample_desc* samples_dev, int n, int S_h, int S_w, const short* tab_linear, const short* tab_cubic,
                          const float* lut_img, const float* lut_mask, const unsigned char* border_rgb /* host, 3 bytes */,
                          float* img_out, float* mask_out, void* stream);
/* ---- training-time augmentation of the same launch (no reference counterpart: RefDataset has none; DESIGN.md 9b) ----
 * Geometry needs nothing new: cris_preprocess_batch applies whatever inverse matrix the descriptor carries (rotation, mirror,
 * scale and shift included).  The colour jitter is THIS PROJECT'S OWN definition - fixed order brightness, contrast, saturation,
 * no hue - and is not pinned against another library.
 * cris_gray_sum_batch: one launch for the ragged batch, sums[b] += sum over the source pixels of 77 R + 150 G + 29 B as an exact
 * integer (64-bit accumulators throughout: a 32-bit one wraps after 65 793 white pixels; wave shuffle, LDS, one 64-bit atomic add
 * per block - exact and order-free).  sums_dev [n] is zeroed by the caller; the kernel ADDS.  The images are read as whole
 * dwords (4 pixels per 3 dwords), so every img must be non-NULL and 4-byte aligned: samples_host, the HOST copy of the same n
 * descriptors, is what the launcher checks that on before the launch (the way cris_eval_iou_batch takes both copies); only
 * samples_dev is read by the kernel.  H, W > 0. */
int cris_gray_sum_batch(const cris_sample_desc* samples_host, const cris_sample_desc* samples_dev, int n, unsigned long long* sums_dev,
                        void* stream);
/* cris_preprocess_batch_aug: the arguments and the warp code of cris_preprocess_batch (one template, two instantiations) plus
 * factors_dev [n][3] = (fb, fc, fs) per sample, sums_dev [n] from cris_gray_sum_batch (may be NULL when no sample has fc != 1),
 * unit_dev [256] with unit[v] = float32(v) / float32(255) built on the host, norm = HOST array of 6 floats (mean rgb, std rgb).
 * The 8-bit cubic result v_c of a pixel becomes, every step one separately rounded float32 operation (never fused):
 *     x_c = clamp01(unit[v_c] * fb)
 *     mean = (float)((double)sums[b] / (65280.0 * (double)H * (double)W)) ;  pivot = min(fb * mean, 1)
 *     k = (1 - fc) * pivot ;  x_c = clamp01(x_c * fc + k)
 *     g = 0.299f * x_r + 0.587f * x_g + 0.114f * x_b   (left to right)
 *     x_c = clamp01(x_c * fs + (1 - fs) * g)
 *     out_c = (x_c - mean_c) / std_c                    (IEEE division)
 * A sample whose three factors are all exactly 1.0f, and any destination pixel none of whose 16 cubic taps lies inside the source
 * (pure letter-box border), go through lut_img exactly as in cris_preprocess_batch.  The mask path is unchanged. */
int cris_preprocess_batch_aug(const cris_sample_desc* samples_dev, int n, int S_h, int S_w, const short* tab_linear, const short* tab_cubic,
                              const float* lut_img, const float* lut_mask, const unsigned char* border_rgb /* host, 3 bytes */,
                              const float* factors_dev, const unsigned long long* sums_dev, const float* unit_dev,
                              const float* norm /* host, 6 floats */, float* img_out, float* mask_out, void* stream);
/* host: inv = cv::invertAffineTransform(mat) (2x3 doubles) */
int cris_invert_affine(const double* mat, double* inv);
/* host: the 16-bit remap weight tables of cv::initInterTab2D(fixpt): tab_linear [1024][4], tab_cubic [1024][16] (copy to the device) */
int cris_remap_tables_u8(short* tab_linear, short* tab_cubic);
/* zero fill of any 16-byte aligned buffer */
int cris_zero_bytes(void* p, size_t nbytes, void* stream);
/* zero several byte ranges in one launch (the parts of the gradient arena that are accumulated into or only partly written:
 * BatchNorm sums, embedding rows; everything a kernel overwrites completely every step is left alone) */
#define CRIS_ZERO_RANGES_MAX 16
typedef struct { void* p; size_t nbytes; } cris_zero_range;
typedef struct { int n; int pad_; cris_zero_range r[CRIS_ZERO_RANGES_MAX]; } cris_zero_ranges;
int cris_zero_many(const cris_zero_ranges* r, void* stream);

/* fused multi-tensor Adam (torch.optim.Adam semantics, train.py:105-107): table of {p,g,m,v,n}.
 * p/m/v are in the parameter layout; g is in the parameter layout when taps == 0, else in the GEMM layout
 * [n][tap][cpad] written by cris_conv_wgrad (element (n, c, tap) of the parameter reads g[(n*taps + tap)*cpad + c]).
 * dstF / dstD (optional): the bf16 GEMM-operand copies of a weight (layouts of cris_pack_desc); the update then also writes
 * them from the new values (tile by tile through LDS) - no separate packing pass re-reads the fp32 weights.  A table holds
 * either the 9-tap (3x3) packed tensors or everything else (pack_taps of cris_adam_step: 9 / 1).
 * step_dev (optional, device int32): 1-based step count read on the device - the bias corrections are then
 * 1 - beta^step (in double) and bias_corr1/2 are ignored (lets a captured HIP graph be replayed step after step). */
typedef struct {
    float* p; const float* g; float* m; float* v;
    long n;
    float lr; float pad_;
    int block_start; int taps;
    int cin; int cpad;
    cris_bf16* dstF; cris_bf16* dstD;
    int N; int npad;                 /* packed tensors: rows, padded rows of the D layout (cin / cpad above) */
    int transposed; int ldF;         /* packed: parameter stored [cin][N] (one tap); ldF / ldD: row strides of dstF / dstD in elements */
    const unsigned char* row_live;   /* optional (plain tensors, weight_decay == 0): byte r != 0 <=> row r (row_len elements) has ever
                                        had a non-zero gradient.  Rows that never had one are skipped: with g = m = v = 0 the
                                        Adam update is the identity (p - step * 0 / (0 + eps) = p), so the result is bit-identical
                                        to the dense update - the token embedding is 17% of CRIS-R50's parameters and a step
                                        touches at most B*L of its 49408 rows. */
    int row_len; int ldD;            /* (ldF / ldD: 0 = dense, as in cris_pack_desc) */
} cris_adam_desc;
int cris_adam_step(const cris_adam_desc* dev_table, int n_desc, int total_blocks, float beta1, float beta2, float eps,
                   float weight_decay, float bias_corr1, float bias_corr2, float grad_scale, const int32_t* step_dev,
                   int pack_taps, void* stream);
/* The same update under torch.amp.GradScaler, decided on the device (what `scaler.step(optimizer)` does for an optimizer with
 * `_step_supports_amp_scaling`; engine/engine.py:56): loss_scale_dev (optional) = the scaler's scale, the gradients are divided
 * by it inside the update; skip_dev (optional) = the scaler's found_inf, != 0 skips the whole update (parameters, moments and
 * operand copies untouched).  cris_counter_advance_unless keeps a device step count that does not advance on a skipped step. */
int cris_adam_step_amp(const cris_adam_desc* dev_table, int n_desc, int total_blocks, float beta1, float beta2, float eps,
                       float weight_decay, float bias_corr1, float bias_corr2, float grad_scale, const int32_t* step_dev,
                       const float* loss_scale_dev, const float* skip_dev, int pack_taps, void* stream);
/* cris_adam_step_amp with one weight decay per tensor instead of one for the table: decay_of[i] (device, fp32, finite, >= 0) belongs
 * to dev_table[i], and every block of a tensor reads its tensor's value.
 *   decoupled == 0: the coupled rule of cris_adam_step, g += decay_of[i] * p before the moments.  With every entry equal to w the
 *     result is, bit for bit, that of cris_adam_step_amp(weight_decay = w), w = 0 included.
 *   decoupled == 1 (AdamW, torch.optim.AdamW): keep = (float)(1.0 - (double)lr * (double)decay_of[i]) once per block, lr read from
 *     the descriptor (so after cris_adam_schedule_lrs on the same stream the decay follows the scheduled rate of this step); per
 *     element p = p * keep, rounded on its own (never fused into the subtraction that follows), then the update of
 *     cris_adam_step_amp with weight_decay = 0: gradient and moments do not see the decay.  "Scale the parameters by keep, then
 *     cris_adam_step_amp(weight_decay = 0)" gives the same bits.
 * Plain tensors, GEMM-layout gradients and the 1- and 9-tap packed tiles alike; the bf16 operand copies are written from the decayed
 * and updated values.  row_live of descriptor i is honoured exactly when decay_of[i] == 0 (a decayed row moves without a gradient).
 * loss_scale_dev, skip_dev, step_dev and pack_taps as for cris_adam_step_amp.  Non-zero with cris_last_error() before anything is
 * launched: a null dev_table or decay_of; n_desc < 1; total_blocks < 1; pack_taps not 1 or 9; decoupled not 0 or 1. */
int cris_adamw_step(const cris_adam_desc* dev_table, int n_desc, int total_blocks, float beta1, float beta2, float eps,
                    const float* decay_of /*[n_desc], device*/, int decoupled, float bias_corr1, float bias_corr2,
                    float grad_scale, const int32_t* step_dev, const float* loss_scale_dev, const float* skip_dev,
                    int pack_taps, void* stream);
int cris_counter_advance_unless(int32_t* counter, const float* skip, void* stream);
int cris_adam_blocks(const cris_adam_desc* d);       /* blocks one descriptor occupies (host: block_start prefix sums) */
int cris_adam_block_elems(void);
/* dst (param layout, desc.p) <- src (GEMM layout, desc.g) for a table of tensors; block_start as for cris_adam_step */
int cris_unpack_grads(const cris_adam_desc* dev_table, int n_desc, int total_blocks, void* stream);
/* Global gradient norm and the clipping divisor of torch.nn.utils.clip_grad_norm_ (engine/engine.py:54-55), over the tables
 * cris_adam_step takes and in its block partition: block b (block_start / cris_adam_blocks) writes partials[b] = sum of g^2 over
 * the elements that block updates, g read where the update reads it - parameter layout when taps == 0, else [n][tap][cpad], of
 * which only the c < cin entries count (the padding columns are never read).  Rows with row_live == 0 are not read (they hold
 * zeros).  Thread, wave and block sums are taken in a fixed order without atomics: the same bits on every run.  Call it once
 * per table into disjoint ranges of one partials buffer, then cris_grad_clip_finalize once over all of it:
 *   out[0] = norm = grad_scale * sqrt(sum of the partials)  (partials added in double, fixed order; grad_scale = the 1/world
 *            the update applies, so the norm is that of the averaged gradient)
 *   out[1] = max(1, (norm + 1e-6) / max_norm) = 1 / clamp(max_norm / (norm + 1e-6), max=1), the divisor to hand to
 *            cris_adam_step_amp as loss_scale_dev; exactly 1 when nothing is clipped; non-finite when the norm is (the update
 *            then writes NaN, as the reference's error_if_nonfinite=False does).  max_norm = +infinity: norm only, divisor 1;
 *            max_norm <= 0 is an argument error.  n_partials == 0 (an empty table): norm 0, divisor 1. */
int cris_grad_sumsq(const cris_adam_desc* dev_table, int n_desc, int total_blocks, float* partials, void* stream);
int cris_grad_clip_finalize(const float* partials, int n_partials, float grad_scale, float max_norm, float* out, void* stream);

/* Exponential moving average of the weights, inside the step (csrc/ema.hip).  `state` is a 16-byte device record
 * {int32 updates; float weight; int32 active; int32 pad}, 16-byte aligned.
 * cris_ema_advance (one thread): step = step_dev[0], the 1-based optimizer step cris_step_advance[_micro] already advanced;
 *   active = (step % every == 0).  When active: t = updates, updates += 1,
 *   d = warmup ? min(decay, (1 + t) / (10 + t)) : decay  (fp32, correctly rounded division), weight = 1 - d.
 *   When not active, updates and weight keep their values.  0 < decay < 1, every >= 1.
 * cris_ema_update: one launch over a device table of cris_ema_desc.  active == 0: every block returns at once.  Otherwise per
 *   element ema = ema + (p - ema) * weight as three separately rounded fp32 operations (no fused multiply-add), which torch's
 *   `e.add_((p - e) * w)` reproduces bit for bit.  Each element is written by one thread.  Partition: block trip b owns
 *   cris_adam_block_elems() consecutive elements of one tensor (block_start = prefix sums of cris_ema_blocks); the grid is capped
 *   at 8 blocks per CU and strides over the trips.  16-byte accesses on whole vectors (p element by element when its start is
 *   not 16-byte aligned), scalar code for the last n % 4 elements.
 *   row_live (optional; row_len = elements per row): rows whose byte is 0 are neither read nor written.  For a parameter whose
 *   row has never changed since ema was set to it, ema == p and ema + 0 * weight == ema: the same bits as the dense update.
 * cris_ema_blocks (host): validates a descriptor (p, ema non-null, n > 0, ema 16-byte aligned, row_live only with row_len > 0)
 *   and returns the block trips it occupies, -1 with cris_last_error() otherwise. */
typedef struct {
    const float* p; float* ema;
    long n;
    const unsigned char* row_live;
    int row_len; int block_start;
} cris_ema_desc;
int cris_ema_blocks(const cris_ema_desc* d);
int cris_ema_advance(const int32_t* step_dev, int every, float decay, int warmup, void* state, void* stream);
int cris_ema_update(const cris_ema_desc* dev_table, int n_desc, int total_blocks, const void* state, void* stream);

/* Per-step learning-rate schedule inside the step (csrc/lr.hip), launched once per Adam table before cris_adam_step[_amp]:
 *   s = step_dev[0], the 1-based optimizer step cris_step_advance[_micro] already advanced; row = min(max(s - 1, 0), n_rows - 1);
 *   dev_table[i].lr = lr_table[row * n_groups + group_of[i]] for i < n_desc (one plain float store per thread: no other byte of a
 *   descriptor changes); lr_out (optional) [g] = lr_table[row * n_groups + g] for g < n_groups.
 * Values are copied, never computed, so the table's schedule is followed bit for bit.  256 threads per block, ceil(n_desc / 256)
 * blocks.  Non-zero with cris_last_error() before anything is launched: a null dev_table, group_of, step_dev or lr_table;
 * n_desc < 1; n_rows < 1; n_groups outside [1, 255].  Every group_of[i] must be < n_groups (the caller checks; a larger one leaves
 * its descriptor unchanged). */
int cris_adam_schedule_lrs(cris_adam_desc* dev_table, int n_desc, const uint8_t* group_of /*[n_desc], device*/,
                           const int32_t* step_dev, const float* lr_table /*[n_rows][n_groups], device*/,
                           int n_rows, int n_groups, float* lr_out /*[n_groups], device, may be NULL*/, void* stream);

/* ---- The sentence-vector path in fp32 (csrc/smallf32.hip) ----------------------------------------------------------------
 * At most CRIS_SMALL_MAX_ROWS (= the per-GPU batch) rows: LayerNorm of the end-of-text rows (model/clip.py:449-452), `@
 * text_projection` (:456), neck.txt_proj = Linear + BatchNorm1d + ReLU (model/layers.py:262-264,286), proj.txt = Linear
 * (model/layers.py:58,71).  The bf16 path's loss error is dominated by the rounding of exactly these values (one rounding of the
 * sentence vector shifts every logit of a sample; profiles/parity_r04.md), and they are a few MFLOP: fp32 on the VALU, reading the
 * fp32 parameters directly.  Matrices are row-major with a leading dimension in floats.
 *   cris_eot_gather_ln_f32     out[b] = LayerNorm(x[b, argmax tokens[b]]) from the saved row statistics; eot_index out
 *   cris_eot_scatter_add_f32   dx[b, eot_b] += d out[b]   (dx: the bf16 gradient of the LayerNorm output)
 *   cris_linear_f32_small      out[M][N] (+)= A[M][K] W^T (+ bias), W = [N][K] (w_is_kn 0) or [K][N] (w_is_kn 1: x @ P, and the
 *                              input gradient of a [N][K] layer: dA = dOut W)
 *   cris_outer_sum_f32_small   G[R][C] = sum_m X1[m][r] X2[m][c] (weight gradient of either layout), rowsum[r] = sum_m X1[m][r] (bias)
 *   cris_colstats_f32_small    one statistics part (sum, M2) per column for cris_bn_finalize(_sync)
 *   cris_bn_relu_f32_small     z = relu(scale y + shift);  _bwd_reduce: ONE partial row [2C] for cris_bn_bwd_sum(_sync);
 *                              _bwd_apply: dy from the summed (global) sums */
#define CRIS_SMALL_MAX_ROWS 16
int cris_eot_gather_ln_f32(const int64_t* tokens, const float* x, const float* mean, const float* rstd, const float* gamma,
                           const float* beta, int Bn, int L, int D, float* out, int* eot_index, void* stream);
int cris_eot_scatter_add_f32(const int* eot_index, const float* drows, int Bn, int L, int D, cris_bf16* dx, void* stream);
int cris_linear_f32_small(const float* A, int lda, const float* W, int ldw, int w_is_kn, const float* bias, int M, int N, int K,
                          float* out, int ldo, int accumulate, void* stream);
int cris_outer_sum_f32_small(const float* X1, int ld1, const float* X2, int ld2, int M, int R, int C, float* G, int ldg, float* rowsum,
                             void* stream);
int cris_colstats_f32_small(const float* y, int ldy, int M, int C, float* psum, float* pm2, void* stream);
int cris_bn_relu_f32_small(const float* y, int ldy, const float* scale, const float* shift, int M, int C, float* z, int ldz, void* stream);
int cris_bn_relu_bwd_reduce_f32_small(const float* dz, int lddz, const float* y, int ldy, const float* scale, const float* shift,
                                      const float* mean, const float* invstd, int M, int C, float* part, void* stream);
int cris_bn_relu_bwd_apply_f32_small(const float* dz, int lddz, const float* y, int ldy, const float* scale, const float* shift,
                                     const float* mean, const float* invstd, const float* sums, float count, int M, int C, float* dy,
                                     int lddy, void* stream);

/* ---- Low-latency cross-rank sum of small fp32 vectors (EXPERIMENTAL, CRIS_SYNCBN_P2P=1) -------------------------------
 * Replaces the per-layer all_gather / all_reduce of nn.SyncBatchNorm (train.py:97-98; 142 small collectives per CRIS-R50
 * step) by ONE kernel per exchange: every rank owns a fine-grained device mailbox that all peers map through HIP IPC; the
 * kernel writes this rank's vector into every mailbox, publishes a generation flag, waits for the peers' flags and adds
 * the world vectors in rank order (bit-identical on all ranks).  Mailbox layout in csrc/p2p.hip. */
size_t cris_p2p_mailbox_bytes(int world, int slots, int max_floats);
int cris_p2p_alloc(size_t bytes, void** dev_ptr);                     /* fine-grained device memory, zero-filled */
int cris_p2p_free(void* dev_ptr);
int cris_p2p_export(void* dev_ptr, void* handle_64_bytes);            /* IPC handle of a mailbox (64 bytes) */
int cris_p2p_import(const void* handle_64_bytes, void** peer_ptr);    /* map another process's mailbox */
int cris_p2p_close(void* peer_ptr);
typedef struct {
    float* data;              /* [n] in: this rank's vector; out: the sum over ranks */
    void* const* boxes;       /* DEVICE array [world]: every rank's mailbox as mapped in this process (own one at [rank]) */
    const int* gen_dev;       /* device step counter (graph / command-list replay) or NULL -> gen_host */
    int* err;                 /* device int set to 1 if a peer never arrived (the output is then NaN); or NULL */
    int n, rank, world;
    int slot, slots;          /* which exchange of the step this is; exchanges per step the mailbox was sized for */
    int max_floats;           /* vector capacity the mailbox was sized for */
    int gen_host;
    int spin_limit;          /* polls before a missing peer is reported (err[0] = 1, NaN result); 0 = the default (~seconds) */
} cris_p2p_params;
int cris_p2p_allreduce_sum(const cris_p2p_params* p, void* stream);

/* The same mailboxes reached from INSIDE other kernels ("LL" words: value and generation in one 8-byte store, csrc/p2p_ll.h; the
 * LL region lies behind the flag-protocol region and is included in cris_p2p_mailbox_bytes).  A link names one exchange of the
 * step; the kernels that take one exchange the values they own themselves:
 *   cris_bn_finalize_sync      SyncBatchNorm forward in ONE launch: merge the local partials, moments about the running mean
 *                              to every peer, rank-order sum, scale / shift + running statistics (replaces cris_bn_finalize +
 *                              cris_bn_sync_pack + exchange + cris_bn_sync_unpack + cris_bn_finalize; same arithmetic)
 *   cris_bn_bwd_reduce_sync    SyncBatchNorm backward: the reduce launch, then ONE launch that adds up the partial rows, adds the
 *                              local sums into `local_sums` (this rank's d beta / d gamma) and leaves the sums over all ranks in
 *                              p->sums for cris_bn_bwd_apply (replaces sum + axpy + exchange)
 *   cris_p2p_ll_allreduce_sum  plain in-place sum of a vector (start-up self-test of the LL words)
 * Reference semantics: torch.nn.SyncBatchNorm as installed by train.py:97-98. */
typedef struct {
    void* const* boxes;       /* DEVICE array [world]: every rank's mailbox as mapped in this process (own one at [rank]) */
    int* err;                 /* device int set to 1 if a peer never arrived (results are then NaN); or NULL */
    const int* gen_dev;       /* device step counter (graph / command-list replay) or NULL -> gen_host */
    int gen_host;
    int rank, world;          /* world <= 0: no exchange (the kernels behave like their plain forms); 1: the exchange with itself */
    int slot, slots;          /* which exchange of the step this is; exchanges per step the mailbox was sized for */
    int max_floats;           /* vector capacity the mailbox was sized for */
    int spin_limit;           /* polls before a missing peer is reported; 0 = the default (~seconds) */
} cris_p2p_link;
int cris_p2p_ll_allreduce_sum(const cris_p2p_link* link, float* data, int n, void* stream);
int cris_bn_finalize_sync(const float* psum, const float* pm2, int nparts, int rows_per_part, float count_local, float count,
                          const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum,
                          float eps, int C, float* scale, float* shift, float* mean, float* invstd, const cris_p2p_link* link,
                          void* stream);
int cris_bn_bwd_reduce_sync(const cris_bn_bwd_params* p, float* local_sums, const cris_p2p_link* link, void* stream);
/* nparts > 0: the partial rows are already in p->part (cris_bn_bwd_sum's case), only the summation + exchange launch runs */
int cris_bn_bwd_sum_sync(const cris_bn_bwd_params* p, int nparts, float* local_sums, const cris_p2p_link* link, void* stream);

/* ---- Gradient exchange over the peer-mapped gradient arenas (csrc/p2p.hip; opt-in: CRIS_GRAD_EXCHANGE=p2p) ---------------
 * What DistributedDataParallel's bucketed all-reduce does for the reference (train.py:100-102), as SURVEY.md section 5 / 8e asks
 * for it on a fully connected xGMI node: a direct reduce-scatter + all-gather in which every rank talks to all seven peers at once,
 * instead of RCCL's schedule.  Every rank's gradient arena (one flat fp32 tensor) is mapped into every other process (HIP-IPC);
 * for one range [lo, lo + n) of the arena, in place:
 *   launch 1  barrier "my gradients of this range are final" - then rank r sums slice r of the range over the ranks IN RANK ORDER
 *             (reads of the peers' arenas over the links, bit-identical results on every rank, no atomics) into its own arena;
 *   launch 2  barrier "my slice is reduced" - then every rank copies the other ranks' reduced slices into its own arena;
 *   launch 3  barrier "I have finished reading" - returns when every peer has: the arena may be written again.
 * The barriers are LL words of the peer mailboxes (cris_p2p_link; three consecutive slots per exchange, generation = the step).
 * All three launches go to `stream` (the communicator's side stream: the exchange overlaps the rest of backward) and can be
 * captured into a HIP graph.  A peer that never arrives: bounded poll, link.err set, this rank's slice poisoned with NaN. */
typedef struct {
    void* const* arenas;      /* DEVICE array [world]: base address of every rank's arena as mapped in THIS process (own: its own) */
    long lo, n;               /* range in floats; both even (8-byte words travel) */
    cris_p2p_link link;       /* link.slot = the first of this exchange's three barrier slots */
    int blocks;               /* blocks per launch, 0 = default */
} cris_p2p_arena_params;
int cris_p2p_arena_allreduce(const cris_p2p_arena_params* p, void* stream);

/* ---- Data-parallel exchanges on library-owned RCCL communicators (csrc/comm.hip) ---------------------------------------
 * What the reference gets from `dist.init_process_group("nccl")` + `DistributedDataParallel` + `SyncBatchNorm`
 * (train.py:80-102; SURVEY.md 8b "comm entry points"), without torch.distributed on the data path.  One cris_comm per
 * process (= per GPU, the device current at cris_comm_init).  RCCL is resolved at run time (the librccl.so.1 already in the
 * process, else the system one; CRIS_RCCL_LIB overrides): the library does not link against it.
 *   bootstrap:  rank 0 calls cris_comm_unique_id and ships the CRIS_COMM_ID_BYTES bytes to the other ranks by any host
 *               channel (a c10d Store, a file, MPI); every rank then calls cris_comm_init (collective).
 *   SyncBN:     cris_comm_syncbn_exchange - in-place fp32 sum over ranks on the CALLER's stream (replaces the all_gather of
 *               (mean, invstd, count) / the all_reduce of (sum_dy, sum_dy_xmu) in torch.nn.SyncBatchNorm).
 *   gradients:  cris_comm_allreduce_bucket - in-place fp32 sum of one range of the gradient arena on the communicator's OWN
 *               side stream and OWN RCCL communicator, after everything `ready_stream` has queued so far (replaces DDP's
 *               bucketed all-reduce; the caller chooses few large ranges: xGMI is per-link bound); cris_comm_wait makes
 *               `stream` wait for every range issued since the last wait (before the optimizer).  Averaging (1/world) is
 *               left to the optimizer's grad_scale.
 *   start-up:   cris_comm_broadcast - rank root's bytes to all ranks (DDP broadcasts parameters and buffers when it wraps).
 * All calls enqueue on streams and return; they can be captured into a HIP graph together with the step's kernels. */
#define CRIS_COMM_ID_BYTES 256                 /* two ncclUniqueId: the statistics and the gradient communicator */
typedef struct cris_comm cris_comm;
const char* cris_comm_rccl_path(void);         /* which RCCL was resolved (NULL + cris_last_error() if none) */
int cris_comm_unique_id(void* id_bytes);
int cris_comm_init(int rank, int world, const void* id_bytes, cris_comm** out);
int cris_comm_destroy(cris_comm* c);
int cris_comm_rank(const cris_comm* c);
int cris_comm_world(const cris_comm* c);
int cris_comm_syncbn_exchange(cris_comm* c, float* stats, size_t n, void* stream);
int cris_comm_allreduce_bucket(cris_comm* c, float* buf, size_t n, void* ready_stream);
int cris_comm_wait(cris_comm* c, void* stream);
int cris_comm_broadcast(cris_comm* c, void* buf, size_t nbytes, int root, void* stream);

/* ---- Baseline JPEG decoding (SURVEY.md 8f-2; csrc/jpeg.hip) -------------------------------------------------------------
 * Replaces `cv2.imdecode(np.frombuffer(ref['img'], np.uint8), cv2.IMREAD_COLOR)` + `cv2.cvtColor(.., COLOR_BGR2RGB)` of the
 * reference's loader (utils/dataset.py:127-129) for the files its LMDB records hold (tools/folder2lmdb.py:50-56 stores the raw
 * JPEG bytes): 8-bit Huffman-coded JPEG, sequential (one interleaved scan or one scan per component) or progressive
 * (spectral selection + successive approximation), gray or YCbCr 4:4:4 / 4:2:2 / 4:2:0, restart intervals.  Hybrid split, as the bit-serial part does not parallelise inside an image:
 *   host   cris_jpeg_read_header, cris_jpeg_decode_coefficients(_batch): marker parsing + Huffman decoding (T.81 Annex F) into
 *          quantised coefficient blocks int16 [component][block row][block col][64] (natural order), one image per thread;
 *   device cris_jpeg_reconstruct: dequantisation + libjpeg's islow inverse DCT -> sample planes, then fancy chroma upsampling +
 *          YCbCr -> RGB -> uint8 [H][W][3], a whole ragged batch in two launches; the result is what cris_preprocess_batch reads.
 * Bit-exact with libjpeg(-turbo) at its default settings (JDCT_ISLOW, do_fancy_upsampling) - pinned against Pillow's
 * libjpeg-turbo through oracle/jpeg_baseline.py.  Anything else (arithmetic coding, lossless, 12-bit, CMYK, other samplings)
 * is refused with an error: the caller keeps such a file on its CPU decoder.  The EXIF orientation is the host mirror's job
 * (cris/pytorch_amd/jpegdec.py turns the decoded image like cv2.imdecode does). */
typedef struct {
    int width, height, ncomp;            /* ncomp 1 (gray) or 3 (YCbCr) */
    int hmax, vmax;                      /* luma sampling factors: (1,1) 4:4:4, (2,1) 4:2:2, (2,2) 4:2:0 */
    int mcus_x, mcus_y, restart_interval;
    int comp_h[3], comp_v[3];
    int blocks_w[3], blocks_h[3];        /* block grid of each component (whole MCUs) */
    int down_w[3], down_h[3];            /* real samples of each component (libjpeg downsampled_width / height) */
    unsigned short quant[3][64];         /* quantisation table of each component, natural order */
    long coef_offset[3];                 /* int16 index of each component's blocks inside the image's coefficient buffer */
    long coef_count;                     /* int16 elements of that buffer */
    long plane_offset[3];                /* byte index of each component's [blocks_h*8][blocks_w*8] sample plane in the scratch */
    long plane_bytes;
    long scan_offset;                    /* byte offset of the entropy-coded segment in the file */
    int total_blocks;
    int multiscan;                       /* 0: one interleaved sequential scan; 1: sequential, one scan per component; 2: progressive (SOF2) */
} cris_jpeg_info;
int cris_jpeg_read_header(const unsigned char* data, size_t nbytes, cris_jpeg_info* info);                         /* host */
int cris_jpeg_decode_coefficients(const unsigned char* data, size_t nbytes, const cris_jpeg_info* info, short* coef); /* host */
/* host: images [0, n) on up to n_threads threads; returns 0 or the first failing image's error (cris_last_error names it) */
int cris_jpeg_decode_coefficients_batch(int n, const unsigned char* const* data, const size_t* nbytes, const cris_jpeg_info* infos,
                                        short* const* coefs, int n_threads);
typedef struct {
    const short* coef;                   /* DEVICE: info.coef_count int16 */
    unsigned char* planes;               /* DEVICE scratch: info.plane_bytes */
    unsigned char* rgb;                  /* DEVICE out: [height][width][3] */
    cris_jpeg_info info;
} cris_jpeg_image;
/* dev_table: DEVICE array of n images; max_blocks / max_pixels: the largest info.total_blocks / width*height in the batch */
int cris_jpeg_reconstruct(const cris_jpeg_image* dev_table, int n, int max_blocks, long max_pixels, void* stream);

/* ---- PNG masks (csrc/png.hip; host only) -----------------------------------------------------------------------------------
 * Replaces `cv2.imdecode(np.frombuffer(ref['mask'], np.uint8), cv2.IMREAD_GRAYSCALE)` (utils/dataset.py:148-149) for the
 * files tools/data_process.py:115-117 writes (`cv2.imwrite(.., mask * 255)`: 8-bit grayscale, non-interlaced): chunk walk,
 * zlib + DEFLATE, row filters.  Lossless, so "parity" = equality with any PNG decoder (pinned against Pillow's).  Other PNG
 * flavours (colour, palette, 1/2/4/16-bit, interlaced) are refused. */
int cris_png_gray8_size(const unsigned char* data, size_t nbytes, int* width, int* height);
int cris_png_decode_gray8(const unsigned char* data, size_t nbytes, unsigned char* out, int width, int height);   /* out: HOST [height][width] */

#ifdef __cplusplus
}
#endif
#endif
