/*
 * xmem_hip.h - C-ABI of the MI355X (gfx950) kernels behind XMem++'s per-frame
 * space-time memory path.
 *
 * The reference (mbzuai-metaverse/XMem2) has no FFI or operator registry: its hot
 * path is a chain of stock ATen calls issued from Python.  This header is therefore
 * the boundary a maintainer would bind in place of those ATen call sites; every
 * entry point cites the reference lines it replaces (paths relative to the
 * reference checkout).  INTEGRATION.md shows the ctypes stub.
 *
 * Conventions
 *   - plain pointers + sizes, no torch types; all pointers are DEVICE pointers unless
 *     the name ends in _host;  `stream` is a hipStream_t passed as void*.
 *   - every function returns 0 on success or a negative xmem_status code; nothing
 *     throws across the ABI; no function allocates or frees caller-visible memory
 *     (scratch is passed in, sized by the matching *_workspace_bytes function).
 *   - no global mutable state: safe to call concurrently on different streams/devices.
 *   - activations are NHWC fp32: [B][H][W][C] with an explicit pixel stride `ld*`
 *     (in floats) so a tensor may live inside a wider (concatenated) buffer.
 *   - memory elements are rows: keys [N][C_k], values [N][C_v], shrinkage [N].
 */
#ifndef XMEM_HIP_H
#define XMEM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    XMEM_OK = 0,
    XMEM_ERR_BAD_ARG = -1,      /* null pointer / non-positive size / unsupported dimension */
    XMEM_ERR_UNSUPPORTED = -2,  /* shape outside what the kernels implement (message says which) */
    XMEM_ERR_WORKSPACE = -3,    /* workspace too small */
    XMEM_ERR_LAUNCH = -4,       /* hipLaunch / hipGetLastError failure */
    XMEM_ERR_TOPK = -5          /* fewer memory elements than top_k (torch.topk raises, memory_util.py:46) */
} xmem_status;

/* ABI version of this header.  2 (round 4): xmem_conv_desc grew (in_half / out_half / w_half), storage-typed `_t` entry points, plan
 * tiles 23..40.  3 (round 5): no layout change, but the MEANING of w_winograd4 / w_winograd4_split changed - the F(4x4) transforms use the
 * interpolation points (0, +-3/4, +-3/2, inf), a caller must form G g G^T with the matching G (see xmem_conv_desc.w_winograd4).  4: xmem_conv2d_plan_info added, no layout change.  5: the click-to-mask entry points added (xmem_click_*, xmem_depthwise3x3_nhwc, xmem_resize_bilinear_ac*, xmem_mask_bbox, xmem_prob_threshold), no layout change.  Still 5: the f-BRS refinement entry points added (xmem_brs_affine_nhwc, xmem_brs_loss, xmem_relu_gate_nhwc, xmem_relu_gate_outer_nhwc, xmem_brs_param_grad and their workspace sizes): new symbols only, no layout change.  Still 5: xmem_conv2d_pointwise_pair added, a new symbol only.  Still 5: xmem_affinity_plan_info added, a new symbol only.  A caller compiled against another version must not pass structs: check xmem_version() == XMEM_ABI_VERSION at load. */
#define XMEM_ABI_VERSION 5
int xmem_version(void);
const char* xmem_last_error_string(int code); /* static string for a status code */

/* Measurement aid: launches the empty kernel `xmem_trace_marker_kernel` on `stream`.  A rocprofv3 kernel trace of a
 * process that brackets a region with two markers can be cut to exactly that region (bench.py does; the reference
 * brackets the same region with perf_counter(), inference/run_on_video.py:106-113). */
int xmem_trace_marker(int tag, void* stream);

/* ------------------------------------------------------------------------------------------
 * Convolution (implicit GEMM on v_mfma_f32_32x32x2_f32) with fused epilogue.
 * Replaces nn.Conv2d (+ eval BatchNorm2d + ReLU + residual add) call sites:
 *   model/resnet.py:59-75,95-114 (BasicBlock/Bottleneck), model/modules.py:166-175,
 *   135-142, 207-211, 186-191, 229-250, model/group_modules.py:25-52 (GConv2D/GroupResBlock).
 *
 *   out[b,oh,ow,n] = act( (sum_{kh,kw,c} in'[b,oh*s-p+kh,ow*s-p+kw,c] * w[n,kh,kw,c]) * scale[n] + shift[n]
 *                         + res[b,oh,ow,n] )
 *   in' = relu(in) if relu_in.  scale/shift hold the folded BatchNorm (scale = gamma/sqrt(var+eps),
 *   shift = beta - mean*scale) or (1, bias).  res may be NULL.  Weights are [Cout][KH][KW][Cin]
 *   (Cin contiguous, Cin % 4 == 0; pad with zero channels if needed).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    const float* in;    int B, H, W, Cin, ldin;
    const float* w;     int Cout, KH, KW, stride, pad;
    const float* scale; const float* shift;
    const float* res;   int ldres;
    float* out;         int ldout;
    int relu_in, relu_out;
    int plan_tile;      /* PLAN CODE 0..40 (anything else: XMEM_ERR_BAD_ARG): algorithm, GEMM tile (rows = output pixels or Winograd tiles
                           x output channels), k-tile depth BK and kernel.  The one table behind it is kPlanCodes in csrc/conv_plan.hpp
                           (Python: xmem2_amd/conv_plan.py CODES); xmem_conv2d_plan_info() reports what a descriptor resolves to.
                             0       built-in heuristic: direct form, tile by the number of tiles (128x128, 128x64, else 64x64), BK 32
                             1..6    direct implicit GEMM, {128x128, 128x64, 64x64} x BK {32, 64}
                             7..12   Winograd F(2x2,3x3) (needs w_winograd), the same six GEMM tiles for its 16 position GEMMs
                             13..15  F(2x2) with the output transform fused into the GEMM, tiles {128x64, 64x64, 64x128}, BK 32
                             16      REDUCED PRECISION (opt-in mode 'fp16w' only, never the default): F(2x2) whose transformed operands
                                     are stored in fp16 and multiplied on v_mfma_f32_32x32x16_f16 with fp32 accumulation (needs
                                     w_winograd_f16, Cin % 64 == 0); its kernel picks 128x128 or 64x64 from the size
                             17..22  Winograd F(4x4,3x3) (needs w_winograd4), the six GEMM tiles for its 36 position GEMMs
                             23..28  F(4x4) with the position GEMMs on the streaming kernel (csrc/gemm_stream.hip):
                                     tile {64x64, 128x64, 128x128} x ring of {3, 4} LDS stages
                             29..34  F(2x2) likewise
                             35..40  a 1x1 / pad 0 convolution itself on the streaming kernel, likewise
                           FALLBACKS, applied in this order, of a code that does not apply to the layer ("Winograd-eligible": w_winograd
                           given, 3x3 / stride 1 / pad 1, Cin % 32 == 0, Cout % 4 == 0, ldout % 4 == 0, ldres % 4 == 0, out and res
                           16-byte aligned):
                             - a streaming code the streaming kernel does not take (split arithmetic, Cin % 32 != 0, not Winograd-
                               eligible or no F(4x4) operand, a 1x1 with padding) becomes 19 / 9 / 3: the 64x64 tile of its form;
                             - F(4x4) without its operand (w_winograd4, or w_winograd4_split under arith = 1) becomes code - 10: F(2x2)
                               with the same tile;
                             - 16 without w_winograd_f16, with Cin % 64 != 0, not Winograd-eligible or under arith = 1 becomes 9;
                             - 13 / 14 / 15 become 8 / 9 / 9 under arith = 1 (no split variant of the fused kernel), and 2 / 3 / 3 when
                               the layer is not Winograd-eligible;
                             - F(2x2) on a layer that is not Winograd-eligible (or, under arith = 1, without w_winograd_split) becomes
                               code - 6: the direct form with the same tile.
                           Cout = 1 ignores the code (a GEMV on the VALU).
                           HALF MODE (in_half = 1) runs the direct BK-32 tiles only: 1..3 as above, 4 = 256x128 (8 waves; split-K as for
                           128x128), 5 / 6 = the tiles of 2 / 3, 0 and everything above 6 = the heuristic.
                           The dilated entry point takes 0..6. */
    int plan_splitk;    /* 0 = heuristic; >0 = number of K splits */
    const float* w_winograd; /* optional [16][Cout][Cin]: G g G^T of the 3x3 filter (3x3 / stride 1 / pad 1 only) */
    int res_broadcast;  /* 1: res is ONE image [Ho][Wo][ldres] added to every batch element (the per-object halves of the
                           fuser convolutions share the f16 half, model/modules.py:31-41 on cat([x, g])) */
    const void* w_winograd_f16; /* optional [16][Cout][Cin] IEEE half: the same G g G^T rounded to fp16 (see plan_tile) */
    const float* w_winograd4;   /* optional [36][Cout][Cin]: G g G^T of Winograd F(4x4,3x3), fp32 (the F(4x4) plan codes, see plan_tile).
                                   INTERPOLATION POINTS
                                   p = (0, 3/4, -3/4, 3/2, -3/2, inf) since ABI version 3 (version 2: 0, +-1, +-2, inf): row i of G is
                                   (1, p_i, p_i^2) / N_i with N_i = prod_{k != i} (p_i - p_k) over the finite points, the row of
                                   infinity (0, 0, 1):  64/81 0 0 | -128/243 -32/81 -8/27 | -128/243 32/81 -8/27 | 32/243 16/81 8/27 |
                                   32/243 -16/81 8/27 | 0 0 1.  Form it in fp64 and round once (xmem2_amd.ops.winograd4_weights).
                                   Error against a fp64 convolution ~3e-6 of the output scale (the textbook points: ~1e-5). */
    /* SPLIT-OPERAND ARITHMETIC (opt-in mode 'fp32x', never the default): arith = 1 and w_split != NULL run every GEMM of the
     * call on v_mfma_f32_32x32x16_f16 with each fp32 operand carried as two halfs (x = hi + lo, relative representation error
     * <= 2^-21; the four partial products are accumulated in fp32).  The split weights have the SHAPE of their fp32
     * counterparts ([Cout][KH][KW][Cin], [16][Cout][Cin], [36][Cout][Cin]) with every group of four input channels stored as
     * eight halfs [hi0 hi1 hi2 hi3 | lo0 lo1 lo2 lo3] (16 bytes, like the four floats), pre-multiplied by a power of two
     * 2^s that the caller folds into `scale` (scale * 2^-s: exact).  Activations stay fp32 in memory; the Winograd-domain
     * intermediate V is written in the same group format.  Same call sites as above; arith = 0 ignores these fields. */
    int arith;
    const void* w_split;
    const void* w_winograd_split;
    const void* w_winograd4_split;
    /* FP16 LOOP (config['precision'] = 'fp16', opt-in, never the default; mirrors the reference's GPU mode: torch.cuda.amp.autocast
     * around the frame loop, inference/run_on_video.py:76, fp32 preload :59-66).  in_half = 1: `in` is [B][H][W][ldin] IEEE halfs
     * (Cin % 8 == 0, ldin % 8 == 0, 16-byte aligned) and w_half holds the weights [Cout][KH][KW][Cin] as halfs.  ZERO-PADDING
     * CONTRACT: the kernel reads all Cin (the layer's channel count padded to 8) halfs of every pixel; a caller whose layer has
     * fewer true channels keeps the padding channels of `in` ZERO (finite is not enough of a promise: the zero weights there would turn
     * an Inf / NaN into NaN), and a channel slice of a wider buffer holds a multiple of 8 channels and ends inside its pixel.  The contraction runs
     * on v_mfma_f32_32x32x16_f16 in the DIRECT form (no Winograd; its tiles: see plan_tile, HALF MODE) with fp32 accumulation and an fp32 epilogue.
     * out_half = 1: `out` and `res` are halfs too (ldout / ldres count halfs; the result is rounded once, to nearest even);
     * out_half = 0 stores fp32 (key projection, mask head).  arith and the Winograd operands are ignored. */
    int in_half, out_half;
    const void* w_half;
} xmem_conv_desc;

size_t xmem_conv2d_workspace_bytes(const xmem_conv_desc* d);

/* The plan xmem_conv2d_nhwc would execute for `d` (plan_tile after its fallbacks, split-K after its rule).  Host only: no GPU call,
 * no pointer of `d` is dereferenced.  Returns XMEM_OK or what xmem_conv2d_nhwc's argument validation returns. */
enum { XMEM_CONV_GEMV = 0,      /* Cout = 1: a VALU GEMV, no tile */
       XMEM_CONV_DIRECT = 1, XMEM_CONV_F2 = 2, XMEM_CONV_F2_FUSED = 3, XMEM_CONV_F2_F16 = 4, XMEM_CONV_F4 = 5 };
typedef struct {
    int form;           /* XMEM_CONV_* */
    int bm, bn, bk;     /* GEMM tile (pixels or Winograd tiles x output channels) and k-tile depth; bm = bn = 0: no tile (GEMV), or
                           chosen at launch from the size (XMEM_CONV_F2_F16) */
    int splitk;         /* slabs of the contraction (1: no workspace reduction) */
    int stream, ring;   /* stream = 1: the GEMM runs on the streaming kernel with a ring of `ring` stages; else 0, 0 */
} xmem_conv_plan_info;
int xmem_conv2d_plan_info(const xmem_conv_desc* d, xmem_conv_plan_info* out);

int xmem_conv2d_nhwc(const xmem_conv_desc* d, void* workspace, size_t workspace_bytes, void* stream);

/* SHARED WINOGRAD TRANSFORMS.  Sibling 3x3 / stride 1 convolutions of a residual block read one tensor (conv1(relu(g)) and
 * downsample(g); in the batched key pass three layers read f16), and the branch's result is only ever the residual of the block's
 * last convolution.  These entry points run the same GEMMs under the same plans as xmem_conv2d_nhwc and give the same bits; they
 * launch fewer transforms.  All of them take fp32 convolutions whose plan resolves to F(4x4) (xmem_conv2d_plan_info: form
 * XMEM_CONV_F4) with arith = 0; anything else returns XMEM_ERR_UNSUPPORTED before any GPU work (the size queries return 0) and the
 * caller issues separate xmem_conv2d_nhwc calls.
 *
 * xmem_conv2d_shared_input: descs[0..n-1], n = 2 or 3, agree in in / ldin / B / H / W / Cin.  ONE input-transform launch
 * writes one V per distinct relu_in (at most two: raw and relu; consumers with the same flag share theirs), then every
 * convolution runs its own position GEMMs and output transform, in order, as xmem_conv2d_nhwc would.  defer_m (NULL: none) names,
 * per convolution, a buffer of defer_m_bytes[i] >= xmem_conv2d_m_bytes(descs[i]) bytes, 16-byte aligned: that convolution stops
 * after its GEMMs and leaves M [36][tiles][Cout] there (its `out` is not written but must be a valid descriptor field), to be
 * finished by xmem_conv2d_nhwc_folded or xmem_conv2d_output_from_m.  The buffer is the caller's: it must not be the workspace of
 * any convolution issued in between.  workspace: xmem_conv2d_shared_input_workspace_bytes(descs, n) bytes.
 *
 * xmem_conv2d_nhwc_folded: the convolution `d` (d->res NULL) with the deferred convolution `branch` as its residual,
 *   r   = [relu_out_b](A^T M_branch A * scale_b + shift_b [+ res_b])        (res_b plain or res_broadcast, as in `branch`)
 *   out = [relu_out](A^T M A * scale + shift + r)
 * in ONE output transform: r stays in registers instead of being stored by the branch and loaded back.  Same B, Ho, Wo, Cout on
 * both sides.  workspace: xmem_conv2d_workspace_bytes(d) bytes.
 *
 * xmem_conv2d_output_from_m: the output transform + epilogue of a deferred convolution alone (when the fold does not apply). */
#define XMEM_CONV_SHARED_MAX 3
size_t xmem_conv2d_shared_input_workspace_bytes(const xmem_conv_desc* const* descs, int n);
size_t xmem_conv2d_m_bytes(const xmem_conv_desc* d);
int xmem_conv2d_shared_input(const xmem_conv_desc* const* descs, int n, void* const* defer_m, const size_t* defer_m_bytes,
                             void* workspace, size_t workspace_bytes, void* stream);
int xmem_conv2d_nhwc_folded(const xmem_conv_desc* d, const xmem_conv_desc* branch, const void* branch_m, size_t branch_m_bytes,
                            void* workspace, size_t workspace_bytes, void* stream);
int xmem_conv2d_output_from_m(const xmem_conv_desc* d, const void* m, size_t m_bytes, void* stream);

/* BOTTLENECK PAIR.  A ResNet-50 bottleneck ends in an expand 1x1 (`expand`: Cmid -> 4 Cmid, + residual, relu) and the next block opens with
 * a reduce 1x1 (`reduce`: 4 Cmid -> Cmid', relu) of that output.  This entry point runs both in ONE launch: a workgroup owns 64 pixels,
 * forms the expand output y chunk by chunk, stores it (expand->out: the next block's residual) and contracts each chunk straight from
 * LDS into the reduce accumulator; reduce->out receives z.  y is not read back from memory.
 *   reduce->in == expand->out, reduce->ldin == expand->ldout, reduce->Cin == expand->Cout, same B / H / W (else XMEM_ERR_BAD_ARG).
 * Taken: fp32 (in_half = out_half = arith = 0), 1x1 / stride 1 / pad 0, expand->Cin in {64, 128, 256}, expand->Cout = 4 Cin,
 * reduce->Cout in {Cin, 2 Cin} and <= 256, expand->res set (plain, not broadcast) and reduce->res NULL, relu_in 0 and relu_out 1 on
 * both, and BOTH plans (plan_tile / plan_splitk resolved as xmem_conv2d_nhwc resolves them) a classic direct tile with split-K 1 -
 * then y and z have the bits of the two xmem_conv2d_nhwc calls.  Anything else returns XMEM_ERR_UNSUPPORTED before any GPU work and
 * the caller issues those two calls.  No workspace. */
int xmem_conv2d_pointwise_pair(const xmem_conv_desc* expand, const xmem_conv_desc* reduce, void* stream);

/* Dilated convolution (atrous), the S2M network's DeepLabV3+ (inference/interact/s2m/s2m_resnet.py:17-20 conv3x3 with dilation, the
 * layer4 blocks 1-2 of _make_layer's replace_stride_with_dilation, :138-150; ASPPConv, s2m/_deeplab.py:113-119, rates 6 / 12 / 18).
 * Same descriptor and epilogue as xmem_conv2d_nhwc (scale / shift, res, relu_in / relu_out, ldin / ldout channel slices); tap (kh, kw)
 * reads input pixel (oh*stride - pad + kh*dilation, ow*stride - pad + kw*dilation), Ho = (H + 2 pad - dilation (KH - 1) - 1) / stride + 1.
 * The direct implicit GEMM only: plan_tile 0 (heuristic) or 1..6, plan_splitk as there; no Winograd, no half / split-operand modes,
 * no res_broadcast, Cout >= 2 (else XMEM_ERR_UNSUPPORTED).  Each workgroup skips the taps that fall outside the input for its whole
 * output tile (flags & XMEM_DILATED_NO_TAP_SKIP turns that off, for measurement: same bits either way).  With dilation 1 the result
 * is bit-identical to xmem_conv2d_nhwc under the same direct plan. */
#define XMEM_DILATED_NO_TAP_SKIP 1
size_t xmem_conv2d_dilated_workspace_bytes(const xmem_conv_desc* d, int dilation);
int xmem_conv2d_nhwc_dilated(const xmem_conv_desc* d, int dilation, int flags, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Deterministic permanent-memory augmentations on the device: every augmented uint8 frame and float mask
 * of one annotated frame in ONE launch.  Replaces the per-annotation loop of inference/run_on_video.py:231-242 over
 * get_determenistic_augmentations(subset) (inference/frame_selection/frame_selection_utils.py:50-218): ColorJitter brightness
 * (1.5 / 0.5), Grayscale(3), RandomPosterize(3), RandomAdjustSharpness(16), gaussian_blur(7) on the image with the mask kept;
 * RandomAffine rotations / scalings / shears / translations on image (PIL: nearest, zero fill) AND mask (tensor branch:
 * affine grid + grid_sample nearest).  img [H][W][3] uint8 (decoded frame at working size), mask [K][H][W] float or NULL,
 * out_img [n_aug][H][W][3], out_mask [n_aug][K][H][W] or NULL.  The arithmetic of every step is restated in the precision
 * the host libraries use (csrc/augment.hip); a load-time call (it synchronises the stream once), not for graph capture.
 * ------------------------------------------------------------------------------------------ */
enum { XMEM_AUG_BRIGHTNESS = 0, XMEM_AUG_POSTERIZE = 1, XMEM_AUG_GRAY = 2, XMEM_AUG_SHARPNESS = 3, XMEM_AUG_BLUR7 = 4, XMEM_AUG_AFFINE = 5 };
#define XMEM_AUG_MAX 32
typedef struct {
    int type;                 /* XMEM_AUG_* */
    float factor;             /* brightness / sharpness factor, posterize bits */
    double image_matrix[6];   /* AFFINE, image side: PIL's inverse matrix (output pixel centre -> input coordinate),
                                 torchvision _get_inverse_affine_matrix about the image centre */
    float mask_grid[6];       /* AFFINE, mask side: (theta^T / [W/2, H/2]) as r00 r10 r20 r01 r11 r21 of the tensor branch's
                                 _gen_affine_grid (matrix about the origin) */
} xmem_aug_desc;
size_t xmem_augment_workspace_bytes(int n_aug, int H, int W);
int xmem_augment_frames(const uint8_t* img, const float* mask, int H, int W, int K, const xmem_aug_desc* descs, int n_aug,
                        uint8_t* out_img, float* out_mask, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Pooling / resampling / gating kernels of the encoders and the decoder.
 * ------------------------------------------------------------------------------------------ */
/* nn.MaxPool2d(3, stride 2, pad 1), model/resnet.py:123; in [B][H][W][C] -> out [B][Ho][Wo][C], Ho = (H - 1) / 2 + 1 (the padding is
 * -inf).  Exact.  Refused with XMEM_ERR_UNSUPPORTED before any GPU work: C % 4 != 0, `in` or `out` off 16 bytes (8 for a half tensor). */
int xmem_maxpool3x3s2(const float* in, float* out, int B, int H, int W, int C, void* stream);

/* F.interpolate(scale 2, bilinear, align_corners=False) of g [B][h][w][C] plus the broadcast skip
 * feature [2h][2w][C] (ONE image, shared by all B): UpsampleBlock, model/modules.py:186-190 + group_modules.py:15-23.
 * Refused with XMEM_ERR_UNSUPPORTED before any GPU work: C % 4 != 0, `g`, `skip` or `out` off 16 bytes (8 for half tensors). */
int xmem_upsample2x_add(const float* g, const float* skip, float* out, int B, int h, int w, int C, void* stream);

/* F.interpolate(mode='area') by an integer ratio r (2 or 4), group_modules.py:22-23;
 * in [B][H][W][C] (pixel stride ldin) -> out [B][H/r][W/r][C] (pixel stride ldout); any r >= 1, any C, scalar accesses (no alignment
 * beyond the element's).  Refused with XMEM_ERR_UNSUPPORTED before any GPU work: H % r != 0 or W % r != 0. */
int xmem_area_downsample(const float* in, int ldin, float* out, int ldout, int B, int H, int W, int C, int r, void* stream);

/* dst[b][p][dst_off + c] = src[(b % srcB)][p][src_off + c]: builds the channel concatenations of
 * MainToGroupDistributor (group_modules.py:55-82) and torch.cat([g, h], 2) (modules.py:59,89).  Pass the addresses of the first source
 * and destination channel; a half destination is rounded once.  Refused with XMEM_ERR_UNSUPPORTED before any GPU work: C, ldsrc or
 * lddst not a multiple of 4, `src` or `dst` off 16 bytes (8 for a half tensor). */
int xmem_copy_channels(const float* src, int ldsrc, int srcB, float* dst, int lddst, int B, int P, int C, void* stream);

/* The input of HiddenUpdater's three pointwise convolutions as one concatenated tensor, in one launch (model/modules.py:49-57:
 * g16_conv(g[0]) + g8_conv(downsample_groups(g[1], 1/2)) + g4_conv(downsample_groups(g[2], 1/4)), g[2] = cat(g4, logits)):
 * out [K][h][w][ldout] <- [ g16 [K][h][w][c16] | area2(g8 [K][2h][2w][c8]) | area4(g4 [K][4h][4w][c4]) | area4(logits [K][4h][4w][1]) ];
 * channels past c16 + c8 + c4 + 1 are not written.  Same bits as xmem_copy_channels + three xmem_area_downsample calls.
 * Refused with XMEM_ERR_UNSUPPORTED before any GPU work: c16, c8, c4 or ldout not a multiple of 4, ldout < c16 + c8 + c4 + 1, a pointer
 * off 16 bytes. */
int xmem_hidden_update_gather(const float* g16, int c16, const float* g8, int c8, const float* g4, int c4, const float* logits,
                              float* out, int ldout, int K, int h, int w, void* stream);

/* The end of the decoder in one launch: the mask head (decoder.pred: 3x3, stride 1, pad 1, c4 -> 1, relu on its input; w [9][c4],
 * scale[1], shift[1]) on g4 [K][4h][4w][c4] -> logits [K][4h][4w], the tensor xmem_hidden_update_gather builds (g4d, pixel stride
 * ldg4d; channels past c16 + c8 + c4 + 1 are not written) from g16 / g8 / g4 and those logits, and hidden [K][h][w][hd] ->
 * cat[k][y][x][0..hd) (pixel stride ldcat; pass the address of the first destination channel).  g4 is read once.  c4 <= 256; every
 * channel count and stride a multiple of 4, every pointer 16-byte aligned.  Same bits as xmem_conv2d_nhwc (relu_in, no residual) +
 * xmem_hidden_update_gather + xmem_copy_channels. */
int xmem_mask_head_gather(const float* g16, int c16, const float* g8, int c8, const float* g4, int c4, const float* w,
                          const float* scale, const float* shift, const float* hidden, int hd, float* logits, float* g4d,
                          int ldg4d, float* cat, int ldcat, int K, int h, int wd, void* stream);

/* CBAM (model/cbam.py:21-77) on g [B][P=H*W][C] and the residual add of FeatureFusionBlock
 * (modules.py:36-39): out = g + CBAM(g).  mlp weights as in the checkpoint: w1 [C/16][C], b1, w2 [C][C/16], b2;
 * spatial 7x7 conv weight sw [2][7][7] (channel 0 = max, 1 = mean), bias sb[1].
 * workspace: xmem_cbam_workspace_bytes(B, H*W, C); nothing past those bytes is written.  Any H, W >= 1 (maps narrower than the gate
 * included).  Refused before any GPU work: C % 16 != 0 or `g` / `out` off 16 bytes (8 for half tensors) -> XMEM_ERR_UNSUPPORTED; a
 * workspace that is NULL or too small -> XMEM_ERR_WORKSPACE. */
size_t xmem_cbam_workspace_bytes(int B, int P, int C);
int xmem_cbam_residual(const float* g, float* out, int B, int H, int W, int C,
                       const float* w1, const float* b1, const float* w2, const float* b2,
                       const float* sw, const float* sb, void* workspace, size_t workspace_bytes, void* stream);

/* GRU-like gate shared by HiddenUpdater / HiddenReinforcer (modules.py:63-72, 93-99):
 * values [B][P][3*Ch] = (forget | update | new), h [B][P][Ch] -> new_h [B][P][Ch] */
int xmem_gru_gate(const float* values, const float* h, float* new_h, int B, int P, int Ch, void* stream);

/* y = a + b + c elementwise (n floats), HiddenUpdater sum modules.py:56-57 */
int xmem_add3(const float* a, const float* b, const float* c, float* y, size_t n, void* stream);

/* STORAGE-TYPED VARIANTS (the fp16 loop, config['precision'] = 'fp16': activations live in HBM as IEEE halfs, as the tensors of
 * the reference's autocast frame loop do, inference/run_on_video.py:76).  Same kernels, same fp32 arithmetic; `*_half` flags give
 * the storage type of each tensor (0 = float, 1 = half; leading dimensions count elements of that type); a stored value is
 * rounded once, to nearest even.  The plain functions above are the all-float instantiations and refuse what these refuse.  The GRU
 * state stays fp32. */
int xmem_maxpool3x3s2_t(const void* in, int in_half, void* out, int out_half, int B, int H, int W, int C, void* stream);
int xmem_upsample2x_add_t(const void* g, const void* skip, void* out, int half, int B, int h, int w, int C, void* stream);
int xmem_area_downsample_t(const void* in, int in_half, int ldin, void* out, int out_half, int ldout, int B, int H, int W, int C, int r, void* stream);
int xmem_copy_channels_t(const void* src, int src_half, int ldsrc, int srcB, void* dst, int dst_half, int lddst, int B, int P, int C, void* stream);
int xmem_cbam_residual_t(const void* g, void* out, int half, int B, int H, int W, int C,
                         const float* w1, const float* b1, const float* w2, const float* b2,
                         const float* sw, const float* sb, void* workspace, size_t workspace_bytes, void* stream);
int xmem_gru_gate_t(const void* values, int values_half, const float* h, float* new_h, int B, int P, int Ch, void* stream);

/* image [3][H][W] (NCHW, unpadded) -> [Hp][Wp][4] NHWC, zero padded as pad_divide_by
 * (util/tensor_util.py:47-61): left/top pads lw, lh; 4th channel zero. */
int xmem_pack_image(const float* img, float* out, int H, int W, int Hp, int Wp, int lh, int lw, void* stream);

/* Frame ingest on the device: decoded uint8 image [H][W][3] (RGB, HWC) -> the same padded NHWC4
 * tensor, after transforms.ToTensor + im_normalization (inference/data/video_reader.py:61-76,
 * dataset/range_transform.py:5-8): ((x / 255) - mean[c]) / std[c] in fp32, in that operation order.
 * mean3_host / std3_host: 3 floats each, HOST pointers. */
int xmem_pack_image_u8(const uint8_t* img, float* out, int H, int W, int Hp, int Wp, int lh, int lw,
                       const float* mean3_host, const float* std3_host, void* stream);

/* value-encoder input, model/network.py:73-81 + modules.py:126-131: per object k the 5 channels
 * (r,g,b,mask_k,sum_{j!=k} mask_j) padded to 8: image4 [Hp][Wp][4], masks [K][Hp][Wp] -> out [K][Hp][Wp][8] */
int xmem_pack_value_input(const float* image4, const float* masks, float* out, int K, int Hp, int Wp, void* stream);

/* KeyProjection activations, modules.py:207-211: proj [P][ldp] = (key C_k | d 1 | e C_k | pad) ->
 * key [P][C_k], shrinkage [P] = d^2+1, selection [P][C_k] = sigmoid(e) */
int xmem_key_post(const float* proj, int ldp, float* key, float* shrinkage, float* selection, int P, int Ck, void* stream);

/* Decoder tail + segment(): model/modules.py:247-248 (x4 bilinear), network.py:111-115 (sigmoid),
 * model/aggregate.py:6-17 (soft aggregation + softmax), util/tensor_util.py:63-77 (unpad).
 * logits [K][h4][w4] -> prob [K+1][H][W] (NCHW, crop offsets lh, lw inside the padded 4*h4 x 4*w4 frame);
 * prob_padded (nullable) receives the uncropped [K+1][4*h4][4*w4]. */
int xmem_logits_to_prob(const float* logits, float* prob, float* prob_padded, int K, int h4, int w4,
                        int H, int W, int lh, int lw, void* stream);

/* aggregate() of given masks (inference_core.py:128,163): masks [K][H][W] -> prob [K+1][H][W] */
int xmem_aggregate_masks(const float* masks, float* prob, int K, int H, int W, void* stream);

/* Given-mask / prediction merge of InferenceCore.step (inference/inference_core.py:117-127):
 * region = sum_k mask_k > 0.5 (the fp32 sum, k ascending); out_k = mask_k if bit k of valid_bits else (region ? 0 : pred_k).
 * [K][H][W] each, K <= 64. */
int xmem_merge_masks(const float* pred_no_bg, const float* mask, uint64_t valid_bits, float* out, int K, int H, int W, void* stream);

/* F.interpolate(prob, shape, mode='bilinear', align_corners=False) of _post_process (inference/run_on_video.py:166-168);
 * in [C][Hi][Wi] -> out [C][Ho][Wo] */
int xmem_resize_bilinear(const float* in, float* out, int C, int Hi, int Wi, int Ho, int Wo, void* stream);

/* torch.argmax(prob, dim=0) -> uint8, inference/run_on_video.py:170-172; prob [C][H][W], C <= 255; the first maximal index. */
int xmem_argmax_u8(const float* prob, uint8_t* out, int C, int H, int W, void* stream);

/* One pass of a test-time ensemble (eval.py --size S [--flip] --save_scores + merge_multi_scale.py), at the ORIGINAL resolution H x W:
 *   v   = bilinear(prob)[c, y, mirror ? W-1-x : x]   (identity when Hi, Wi == H, W; same arithmetic as xmem_resize_bilinear)
 *   q   = (uint16)(v * 255.f), truncated
 *   acc = first ? q : acc + q                        acc: uint16 [C][H][W]; at most 257 passes cannot overflow
 *   out (if non-NULL) = first index of max_c acc[c]   uint8 [H][W], the merged mask of the pass that closes the frame
 * prob [C][Hi][Wi], C in [1, 255]. */
int xmem_ensemble_accumulate(const float* prob, int C, int Hi, int Wi, int mirror,
                             uint16_t* acc, int H, int W, int first, uint8_t* out, void* stream);

/* DAVIS J&F counts (util/metrics.py batched_jaccard / batched_f_measure, the width=None _seg2bmap and cv2.dilate with disk(radius)):
 *   gt, pred  uint8 label maps [B][H][W]; lut (or NULL) a 256-entry uint8 map applied to pred (the MaskMapper dense -> original ids)
 *   counts    int32 [B][256][7], zeroed on `stream` first; for every frame b and label k in 1..254:
 *             gt_area, pred_area, inter, n_gt, n_pred, gt_match, pred_match  (boundary pixels; *_match: under the other map's
 *             boundary dilated by the disk dy^2 + dx^2 <= radius^2).  Labels 0 and 255 are never scored; absent labels count 0.
 * radius in [0, 63], H and W in [1, 16384] (else XMEM_ERR_UNSUPPORTED); the counts are exact and bit-reproducible. */
int xmem_jf_counts(const uint8_t* gt, const uint8_t* pred, const uint8_t* lut, int B, int H, int W, int radius,
                   int32_t* counts, void* stream);

/* ------------------------------------------------------------------------------------------
 * Scribble-to-mask (S2M) around its convolutions (inference/interact/s2m_controller.py, s2m/_deeplab.py, s2m/utils.py).
 * ------------------------------------------------------------------------------------------ */
/* Input of every object at once, s2m_controller.py:21-35 + pad_divide_by(., 16) (util/tensor_util.py:47-62): image [3][H][W]
 * (normalised), prev_mask [H][W] (float object index), scr [H][W] uint8 -> out [K][Hp][Wp][8], per object k = 1..K the channels
 * (r, g, b, prev == k, scr == k, scr != k && scr != ignore_class, 0, 0), all zero in the centred padding (top lh, left lw). */
int xmem_s2m_pack(const float* image, const float* prev_mask, const uint8_t* scr, int ignore_class, int K,
                  int H, int W, int Hp, int Wp, int lh, int lw, float* out, void* stream);

/* nn.AdaptiveAvgPool2d(1) of the ASPP pooling branch (s2m/_deeplab.py:122-133) on NHWC: in [B][P][ld] -> out [B][C], mean over the
 * P pixels in a fixed summation order (the same bits on every call).  C % 4 == 0, ld % 4 == 0, 16-byte aligned pointers. */
int xmem_channel_mean(const float* in, int ld, int B, int P, int C, float* out, void* stream);

/* The pooling branch's upsample from 1 x 1 (_deeplab.py:132): vec [B][C] written to every pixel of out [B][P][ld] (a channel slice
 * of the ASPP concat buffer; C % 4 == 0, ld % 4 == 0, 16-byte aligned). */
int xmem_broadcast_channels(const float* vec, float* out, int ld, int B, int P, int C, void* stream);

/* F.interpolate(x, size=(Ho, Wo), mode='bilinear', align_corners=False) on NHWC into a channel slice (the DeepLabV3+ decoder,
 * _deeplab.py:49-53): in [B][Hi][Wi][ldin] -> out [B][Ho][Wo][ldout], first C channels of each; source arithmetic as
 * xmem_resize_bilinear.  C, ldin, ldout multiples of 4, 16-byte aligned pointers. */
int xmem_resize_bilinear_nhwc(const float* in, int ldin, int B, int Hi, int Wi, int C, float* out, int ldout, int Ho, int Wo, void* stream);

/* S2M output (s2m/utils.py:15-20 x4 bilinear, s2m_controller.py:36 sigmoid + unpad): logits [K][h4][w4] -> prob [K][H][W] (crop
 * offsets lh, lw inside 4h4 x 4w4).  prob_wbg (nullable) [K+1][H][W] = aggregate_wbg(prob, keep_bg=True) with the logit temperature
 * `temperature` (1000 = hard=True, interaction.py:36-51, 193-196); mask (nullable) [H][W] uint8 = its first-index argmax. */
int xmem_s2m_output(const float* logits, int K, int h4, int w4, int H, int W, int lh, int lw,
                    float* prob, float* prob_wbg, uint8_t* mask, float temperature, void* stream);

/* aggregate_wbg(prob, keep_bg, hard) of interaction.py:36-51 on its own: prob [K][H][W] -> out [K+1][H][W] (keep_bg) or [K][H][W]
 * (nullable), mask (nullable) = first-index argmax over the K + 1 softmax values; temperature 1 (hard=False) or 1000 (hard=True). */
int xmem_aggregate_wbg(const float* prob, int K, int H, int W, int keep_bg, float temperature, float* out, uint8_t* mask, void* stream);

/* ------------------------------------------------------------------------------------------
 * Click-to-mask (the f-BRS click network with the NoBRS predictor: inference/interact/fbrs_controller.py, fbrs/model/
 * is_deeplab_model.py, fbrs/inference/predictors/base.py, fbrs/inference/transforms/) around its convolutions.  All fp32.
 * "align_corners" below is F.interpolate(mode='bilinear', align_corners=True): output index o of n_out reads the source
 * coordinate o (n_in - 1) / (n_out - 1), 0 when n_out == 1; the cell index and the weight come from the integer quotient and
 * remainder, so equal sizes copy bit for bit.
 * ------------------------------------------------------------------------------------------ */
/* Network input of both samples of AddHorizontalFlip in one launch (transforms/flip.py:8-21, DistMaps in cpu mode: fbrs/model/ops.py:
 * 46-53, 78 with utils/cython/_get_dist_maps.pyx, then rgb_conv: is_deeplab_model.py:36-41, 54).
 *   image   [3][H][W] at the network's working size
 *   clicks  [2][cap][2] (row, col) floats, positive clicks first; counts [2] int32 ON THE DEVICE (so that a captured graph serves any
 *           number of clicks), each clamped to [0, cap]
 *   out     [B][H][W][8] NHWC, B = with_flip ? 2 : 1, channels 3..7 zero; sample 1 is the horizontally mirrored image with the click
 *           columns (W - 1) - col
 *   features (nullable) [B][2][H][W]: the two distance features
 * Per pixel and polarity d = min_i ((r - rint(r_i)) / radius)^2 + ((c - rint(c_i)) / radius)^2 (rint: half to even), feature =
 * tanh(2 sqrt(d)), d = 1e6 (feature exactly 1) without a valid click.  A click whose rounded row is negative is ignored as in the
 * reference (its padding is (-1, -1)); a click otherwise outside the map is ignored too (the reference writes out of bounds there).
 * rgb_conv: 75 floats w1 [8][5], b1 [8], w2 [3][8], b2 [3] = Conv2d(5, 8, 1) -> LeakyReLU(0.2) -> Conv2d(8, 3, 1) with the BatchNorm
 * between them folded into w2 / b2 by the caller. */
int xmem_click_input(const float* image, const float* clicks, int cap, const int32_t* counts, float radius, const float* rgb_conv,
                     int H, int W, int with_flip, float* out, float* features, void* stream);

/* Depthwise 3x3, pad 1, stride 1, no bias (SeparableConv2d.body[0], fbrs/model/modeling/basic_blocks.py:63-64): in [B][H][W][ldin] ->
 * out [B][H][W][ldout], first C channels of each; w [9][C] (tap-major).  The pointwise convolution that follows carries BatchNorm and
 * ReLU in xmem_conv2d_nhwc's epilogue.  C, ldin, ldout multiples of 4, 16-byte aligned pointers. */
int xmem_depthwise3x3_nhwc(const float* in, int ldin, const float* w, float* out, int ldout, int B, int H, int W, int C, void* stream);

/* align_corners resize on NHWC into a channel slice (DeepLabV3Plus.forward, fbrs/model/modeling/deeplab_v3.py:77-78): shapes and
 * constraints as xmem_resize_bilinear_nhwc. */
int xmem_resize_bilinear_ac_nhwc(const float* in, int ldin, int B, int Hi, int Wi, int C, float* out, int ldout, int Ho, int Wo, void* stream);

/* align_corners resize on planar maps with a source crop and a destination paste: rows [r0, r0 + Hc) x columns [c0, c0 + Wc) of
 * in [C][Hi][Wi] resized to Hd x Wd and written at (pr0, pc0) of out [C][Ho][Wo]; zero_fill = 1 writes zeros to the rest of out, 0
 * leaves it untouched.  get_roi_image_nd and ZoomIn.inv_transform (transforms/zoom_in.py:142-160, 65-83). */
int xmem_resize_bilinear_ac(const float* in, int C, int Hi, int Wi, int r0, int c0, int Hc, int Wc,
                            float* out, int Ho, int Wo, int pr0, int pc0, int Hd, int Wd, int zero_fill, void* stream);

/* Network output: logits [B][h4][w4] (B = with_flip ? 2 : 1) -> prob [H][W] = sigmoid(mean of the align_corners upsample of sample 0
 * and the mirrored upsample of sample 1).  The flip's inverse averages LOGITS: it is the last transform, so its inverse runs before
 * SigmoidForPred's (predictors/base.py:21-26, 46-47; is_deeplab_model.py:63-64). */
int xmem_click_prob(const float* logits, int h4, int w4, int H, int W, int with_flip, float* prob, void* stream);

/* get_bbox_from_mask of prob > threshold (fbrs/utils/misc.py:19-25; prob [H][W]): out = {rmin, rmax, cmin, cmax, count} int32, the box
 * {INT_MAX, -1, INT_MAX, -1} when nothing is set.  click_pixels (nullable) [n_clicks][2] int32 (row, col) join the box but not the
 * count, as get_object_roi adds the positive clicks after its caller tested the mask's sum (transforms/zoom_in.py:41-44, 130-132).
 * ZoomIn then moves 20 bytes to the host instead of the map.  Exact and order-independent. */
int xmem_mask_bbox(const float* prob, int H, int W, float threshold, const int32_t* click_pixels, int n_clicks, int32_t* out, void* stream);

/* out[i] = prob[i] > threshold ? 1 : 0, n floats: the mask FBRSController.interact returns (inference/interact/fbrs_controller.py:46) */
int xmem_prob_threshold(const float* prob, size_t n, float threshold, float* out, void* stream);

/* ClickInteraction.predict (inference/interact/interaction.py:247-254): prev_prob [K+1][H][W] clamped to <= 0.9, row tar_obj
 * (1..K) replaced by obj_mask [H][W], then aggregate_wbg(.[1:], keep_bg=True) with `temperature` as xmem_aggregate_wbg ->
 * out [K+1][H][W] (nullable, must not alias prev_prob) and mask [H][W] uint8 (nullable) = its first-index argmax. */
int xmem_click_commit(const float* prev_prob, const float* obj_mask, int K, int H, int W, int tar_obj, float temperature,
                      float* out, uint8_t* mask, void* stream);

/* ------------------------------------------------------------------------------------------
 * f-BRS click refinement (inference/interact/fbrs/inference/predictors/brs.py:54-140, brs_functors.py, brs_losses.py): the parts of
 * the objective and of its data gradient that are not convolutions.  Everything here is bit-reproducible: the same inputs give the
 * same bits (no float atomics; fixed-order reductions), which L-BFGS and the strict `<` of the best prediction rely on.
 *
 * y = x (1 + s[c]) + b[c] on NHWC [B][h][w][C], scale_bias [2C] = the optimiser's vector (scale then bias, ScaleBiasOptimizer.
 * unpack_opt_params), the same for every batch element.  C % 4 == 0, 16-byte aligned pointers. */
int xmem_brs_affine_nhwc(const float* x, const float* scale_bias, float* y, int B, int h, int w, int C, void* stream);

/* out[i] = y[i] > 0 ? g[i] : 0 over n floats (n % 4 == 0): the adjoint of a ReLU whose OUTPUT y was kept; out may alias g. */
int xmem_relu_gate_nhwc(const float* y, const float* g, float* out, size_t n, void* stream);

/* out[p][c] = y[p][c] > 0 ? g1[p] w[c] : 0: the adjoint of a Cout = 1 pointwise layer (an outer product of its output gradient g1
 * [pixels] with its weights w [C]) followed by the ReLU gate of that layer's input y [pixels][C].  C % 4 == 0. */
int xmem_relu_gate_outer_nhwc(const float* y, const float* g1, const float* w, float* out, size_t pixels, int C, void* stream);

/* BRSMaskLoss on the align_corners upsample of logits [B][h4][w4] (B = 1 or 2: the plain and the mirrored sample, summed jointly) to
 * H x W, with the bookkeeping of BaseOptimizer.__call__ in the same launch sequence.
 *   rects     [B][cap][5] int32 per click: rows [r0, r1) x columns [c0, c1) of its square in the working image - what the numpy
 *             slice of _get_clicks_maps_nd selects, so at most 3 x 3, clipped, and EMPTY for a click whose rounded row or column is 0 -
 *             and the polarity (1 positive).  count [1] int32 ON THE DEVICE: clicks per sample, clamped to [0, cap].
 *             A pixel covered by several squares of one polarity counts once.
 *   last_mask [B][H][W] uint8 (read), mask [B][H][W] uint8 (written: upsampled logit > 0); must not alias.
 *   record    8 floats: [0] sum((1-p) pos)^2 / (sum pos + 1e-5) + sum(p neg)^2 / (sum neg + 1e-5), [1] max |(1-p) pos|, [2] max |p neg|,
 *             [3] zeroed (xmem_brs_param_grad writes the final f there), [4 + 2b], [5 + 2b] as int32: the number of pixels of sample b in
 *             mask & last_mask and in mask | last_mask.
 *   dlogit    [B][h4][w4]: d record[0] / d logits (every element written).
 * workspace: xmem_brs_loss_workspace_bytes(B, cap), 16-byte aligned. */
size_t xmem_brs_loss_workspace_bytes(int B, int cap);
int xmem_brs_loss(const float* logits, int B, int h4, int w4, int H, int W, const int32_t* rects, const int32_t* count, int cap,
                  const uint8_t* last_mask, uint8_t* mask, float* record, float* dlogit, void* workspace, size_t workspace_bytes,
                  void* stream);

/* grad[c] = sum over B h w of g x + 2 reg_weight s[c], grad[C + c] = sum g + 2 reg_weight reg_bias_weight b[c] for the feature
 * gradient g and the un-scaled features x, both NHWC [B][h][w][C] (C % 4 == 0, C <= 1024), in two fixed-order stages; and
 * record[3] = record[0] + reg_weight (sum s^2 + reg_bias_weight sum b^2).  workspace: xmem_brs_param_grad_workspace_bytes(C). */
size_t xmem_brs_param_grad_workspace_bytes(int C);
int xmem_brs_param_grad(const float* g, const float* x, int B, int h, int w, int C, const float* scale_bias, float reg_weight,
                        float reg_bias_weight, float* record, float* grad, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Robot-click evaluation (inference/interact/fbrs/inference/clicker.py:32-59, utils.py:103-110) in integer arithmetic: the same inputs
 * give the same bits.  H and W in [1, 16384] (else XMEM_ERR_UNSUPPORTED), which keeps every squared distance in int32.
 *
 * Error planes of a prediction against gt [H][W] uint8 (1 object, 255 ignore, anything else background).  The prediction is
 * prob [H][W] > threshold, or mask [H][W] != 0: exactly one of prob / mask is non-NULL.  planes [2][H][W] uint8: fn = gt & ~pred,
 * fp = ~gt & pred & not_ignore.  counts [2] int32 (zeroed on the stream first): pixels of pred & gt and of (pred | gt) & not_ignore,
 * the numerator and denominator of get_iou. */
int xmem_click_errors(const float* prob, float threshold, const uint8_t* mask, const uint8_t* gt, int H, int W, uint8_t* planes,
                      int32_t* counts, void* stream);

/* Exact squared Euclidean distance transform of planes [B][H][W] uint8 (non-zero = inside) surrounded by one ring of zeros:
 * d2 [B][H][W] int32 = min over the zero pixels of the plane and the ring pixels of dy^2 + dx^2, 0 where the plane is 0 - the square
 * of scipy's distance_transform_edt on the plane padded by one, cropped again.  A column pass and a row pass; the row pass searches
 * outwards from each pixel while dx^2 < the best so far (exact), so its cost grows with the largest distance.  B * H < 2^31. */
int xmem_edt_sq(const uint8_t* planes, int B, int H, int W, int32_t* d2, void* stream);

/* The next click of Clicker._get_click from d2 [2][H][W] (fn, fp) and not_clicked [H][W] uint8: per plane the maximum of
 * d2 * (not_clicked != 0) at its smallest linear index; is_positive = fn_max > fp_max (strict: a tie is a negative click).
 * record [8] int32 = {is_positive, row, col, fn_max_d2, fp_max_d2, counts[0], counts[1], 0} (counts nullable: zeros);
 * not_clicked[row][col] is cleared.  Two stages through workspace (xmem_next_click_workspace_bytes(H, W), 8-byte aligned). */
size_t xmem_next_click_workspace_bytes(int H, int W);
int xmem_next_click(const int32_t* d2, uint8_t* not_clicked, const int32_t* counts, int H, int W, int32_t* record, void* workspace,
                    size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Frame ingest: the working-size resize of a decoded frame (inference/data/video_reader.py:61-65, torchvision Resize on a PIL image =
 * Image.resize(size, BILINEAR), antialiased) in the host library's own integer arithmetic, so the result is the same bytes.
 *   src uint8 [Hs][Ws][3] -> dst uint8 [Hd][Wd][3] (contiguous, not aliasing src); flip != 0 writes the output columns mirrored.
 *   Per axis a tap table computed on the host (xmem2_amd/pil_resize.py: taps): bounds int32 [out][2] = (first source index, tap
 *   count), coeffs int32 [out][ksize] with 22 fractional bits, unused taps 0; any ksize >= 1.  One pass is
 *   clamp((2^21 + sum_k src[first + k] * coeffs[k]) >> 22, 0, 255) per channel in int32; the horizontal pass runs first and is rounded
 *   to uint8 into `workspace` ([Hs][Wd][3], xmem_resize_u8_workspace_bytes), the vertical pass runs on that.  A pass whose sizes are
 *   equal is skipped (its tables may be NULL); when neither axis changes one copy (or mirror) kernel runs.  Windows are clamped to the
 *   source, so a wrong table cannot read out of bounds.  Integer arithmetic only, no atomics: bit-reproducible.
 * Every side in [1, 16384] (else XMEM_ERR_UNSUPPORTED, before any GPU work; the workspace query returns 0). */
size_t xmem_resize_u8_workspace_bytes(int Hs, int Ws, int Hd, int Wd);
int xmem_resize_u8_bilinear_aa(const uint8_t* src, int Hs, int Ws, uint8_t* dst, int Hd, int Wd, int flip, const int32_t* xbounds,
                               const int32_t* xcoeffs, int xksize, const int32_t* ybounds, const int32_t* ycoeffs, int yksize,
                               void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * n device-to-device copies, src[i] -> dst[i] of bytes[i] bytes, in one launch per XMEM_COPY_MAX_SEGMENTS of them (the session's
 * feature cache: one frame's key-encoder outputs <-> its cache entry).  src / dst / bytes are HOST arrays; the triples travel by
 * value in the kernel arguments, so the call needs no device-side table and its addresses may change from call to call.
 * Byte-exact for every length (0: nothing is touched) and every alignment: 16-byte stores on the destination's aligned body, loads as
 * wide as the source's alignment relative to it allows (16, 4, 2 or 1 bytes), single bytes in front of and behind the body.
 * The ranges of one pair must not overlap (XMEM_ERR_BAD_ARG); a destination that overlaps ANOTHER pair's ranges is the caller's
 * fault.  Segments that are all empty launch nothing. */
#define XMEM_COPY_MAX_SEGMENTS 16
int xmem_copy_segments(const void* const* src, void* const* dst, const size_t* bytes, int n, void* stream);

/* ------------------------------------------------------------------------------------------
 * Run-length track export: the run boundaries, areas and boxes of uint8 label maps masks [N][H][W] (row-major), for the labels 1..K,
 * in the COCO order j = x * H + y (column-major; the bottom pixel of column x and the top pixel of column x + 1 are neighbours).
 * With b_k[j] = (masks[j] == k) and b_k[-1] = 0, an EVENT of label k is a j with b_k[j] != b_k[j - 1]; the uncompressed COCO counts of
 * k are diff([0, events..., H * W]) (the host's part: per event, never per pixel).
 *   meta    int32 [N][K][XMEM_RLE_META] per frame and label k (row k - 1): {events, area, x0, y0, x1, y1} - the TRUE number of events
 *           (also when they did not fit), the number of pixels, the inclusive box; a label without a pixel has {0, 0, 0, 0, -1, -1}.
 *   events  uint32 [N][capacity] per frame: the ascending event positions of label 1, then of label 2, ... packed back to back (label
 *           k starts at the sum of the event counts of the labels before it).  Entries at and beyond `capacity` are not written: a
 *           frame whose counts sum to more than `capacity` is to be encoded again with that sum as its capacity.
 * Three launches (count, scan, emit) and no inter-workgroup waiting; the position of every event in the output follows from the scan,
 * not from the arrival order of atomics, and the sums / minima / maxima are integer: the same input gives the same bytes.
 * Labels above K (and 0) belong to no plane.  K in [1, 254], capacity >= 1 (else XMEM_ERR_BAD_ARG); H, W in [1, 16384], N <= 65535
 * (else XMEM_ERR_UNSUPPORTED).  workspace: xmem_rle_workspace_bytes(N, W, K) bytes (0 for arguments outside those ranges), 4-byte aligned. */
#define XMEM_RLE_META 6
size_t xmem_rle_workspace_bytes(int N, int W, int K);
int xmem_rle_encode(const uint8_t* masks, int N, int H, int W, int K, int capacity, int32_t* meta, uint32_t* events, void* workspace,
                    size_t workspace_bytes, void* stream);

/* The inverse of xmem_rle_encode's record: label maps masks uint8 [N][H][W] from meta [N][K][XMEM_RLE_META] and events [N][capacity].
 * Of `meta` only field 0 is read, the number of events of row k; the rows' ascending event lists are packed back to back per frame.
 * Pixel (y, x), j = x * H + y, belongs to row k iff the number of events e of row k with e <= j is odd (a row with an odd number of
 * events runs to the last pixel, as counts = diff([0, events..., H * W]) says).  `masks` is written completely: a pixel gets
 * values[k - 1] (k when `values` is NULL) of the HIGHEST row that contains it, else 0 - rows from the encoder never overlap, rows
 * from other tools may, and the later one wins.
 *   status  int32 [N]: 0 for a good frame; 1 when the frame's counts sum to more than `capacity` (or one is negative): that frame is
 *           written all zero, and no event at or beyond `capacity` is ever read.
 * One launch, no workspace, no atomics: every thread computes and stores only pixels it owns, so no event value steers a store and the
 * same input gives the same bytes.  A NULL meta / events / masks / status is XMEM_ERR_BAD_ARG; outside H, W in [1, 16384],
 * K in [1, 254], N in [1, 65535], capacity >= 1 the call is XMEM_ERR_UNSUPPORTED. */
int xmem_rle_decode(const int32_t* meta, const uint32_t* events, int N, int H, int W, int K, int capacity, const uint8_t* values,
                    uint8_t* masks, int32_t* status, void* stream);

/* The compressed COCO string of every label of a record (the public mask API's rleToString): for the counts c[0 .. E] of a label with
 * E >= 1 events (c[0] = e[0], c[i] = e[i] - e[i - 1], c[E] = H * W - e[E - 1]) the values x[i] = c[i] for i <= 2 and c[i] - c[i - 2]
 * after that, each written as little-endian groups of 5 bits g, one character (g | (more ? 0x20 : 0)) + 48 per group, `more` until
 * the bits that remain are the sign alone - characters '0'..'o' (backslash among them), 1 to 6 per value for H, W <= 16384.
 * Input: meta [N][K][XMEM_RLE_META] and events [N][capacity] as xmem_rle_encode leaves them, on the device.
 *   str_len int32 [N][K]: the TRUE length of each label's string (also when it did not fit); 0 for a label without event; -1 for every
 *           label of a frame whose event counts sum to more than `capacity` (or hold a negative one): nothing of that frame is read,
 *           it is to be encoded again.
 *   chars   uint8 [N][char_capacity] per frame: the strings of label 1, 2, ... packed back to back.  Bytes at and beyond
 *           `char_capacity` are not written: a frame whose lengths sum to more is to be compressed again with that sum.
 * One thread owns one count (four neighbouring events); three launches (lengths, a per-frame exclusive scan in label-major order, emit),
 * no inter-workgroup waiting and no atomics: the same input gives the same bytes.  K in [1, 254], capacity >= 1, char_capacity >= 1
 * (else XMEM_ERR_BAD_ARG); H, W in [1, 16384], N <= 65535, capacity <= 2^28 (else XMEM_ERR_UNSUPPORTED).
 * workspace: xmem_rle_compress_workspace_bytes(N, K, capacity) bytes (0 outside those ranges), 4-byte aligned. */
size_t xmem_rle_compress_workspace_bytes(int N, int K, int capacity);
int xmem_rle_compress(const int32_t* meta, const uint32_t* events, int N, int H, int W, int K, int capacity, int char_capacity,
                      int32_t* str_len, uint8_t* chars, void* workspace, size_t workspace_bytes, void* stream);

/* The inverse (rleFrString): compressed strings -> the record xmem_rle_decode reads.  chars uint8 [chars_len] holds the strings of a
 * batch; str_ofs int32 [N][K + 1] per frame: row k's string is chars[str_ofs[k], str_ofs[k + 1]), an empty range is a row without
 * string (no events, status 0).
 *   meta    int32 [N][K][XMEM_RLE_META]: field 0 the row's number of events (its number of counts - 1), the other fields 0.
 *   events  uint32 [N][capacity] per frame: the rows' events (the running sums of the counts but the last) packed in row order.
 *   status  int32 [N][K]: 0 good; 1 malformed (a character outside 48..111, a value of more than 6 characters, a string that ends
 *           inside a value, offsets that are no range of chars); 2 not a plane (a negative count, a zero count after the first, a
 *           sum other than H * W); 3 the frame's events exceed `capacity` (every string of that frame).  A row with a non-zero status
 *           writes no event and has 0 events in meta; the other rows of its frame are packed as if it had no string.
 * One workgroup per string: a value is assembled at its last character from at most 5 characters before it, its index is a rank, the
 * counts two stride-2 running sums, the events the running sum of the counts, carried over chunks of the string.  Three launches
 * (check, a per-frame scan of the rows' starts, expand).  Every read stays inside the row's range, every store index is a rank checked
 * against `capacity`; no decoded value forms an address.  Argument ranges and error codes as xmem_rle_encode; chars_len >= 0.
 * workspace: xmem_rle_decompress_workspace_bytes(N, K) bytes, 4-byte aligned. */
size_t xmem_rle_decompress_workspace_bytes(int N, int K);
int xmem_rle_decompress(const uint8_t* chars, int chars_len, const int32_t* str_ofs, int N, int H, int W, int K, int capacity,
                        int32_t* meta, uint32_t* events, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* NHWC [B][P][C] (pixel stride ld) <-> NCHW [B][C][P] layout transposes for the Python surface */
int xmem_nhwc_to_nchw(const float* in, int ld, float* out, int B, int P, int C, void* stream);
int xmem_nchw_to_nhwc(const float* in, float* out, int ld, int B, int P, int C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Memory readout: fused anisotropic-L2 similarity + streaming top-k + softmax.
 * Replaces get_similarity + do_softmax (model/memory_util.py:7-65) as called from
 * MemoryManager.match_memory (inference/memory_manager.py:82-120,143-177) without ever
 * materialising the N x HW matrix, and `_readout` (memory_manager.py:57-59,185-188).
 * ------------------------------------------------------------------------------------------ */
#define XMEM_MAX_SEGMENTS 4
typedef struct {
    const float* key;        /* [n][C_k] rows */
    const float* shrinkage;  /* [n] or NULL (treated as 1, memory_util.py:36-37) */
    int n;                   /* elements in this segment (may be 0) */
    const void* rows16;      /* optional [n][XMEM_ROWS16_HALFS] IEEE halfs: the operand rows of the fp16 filter for these keys, kept
                                by the caller across calls (xmem_affinity_rows16 makes them; they depend on key and shrinkage only).
                                NULL: the call derives them into its workspace.  Never changes a result. */
} xmem_key_segment;
#define XMEM_ROWS16_HALFS 144

/* Filter operand rows of `n` memory elements (csrc/affinity_common.hpp: [ms/8 x^2 | ms/8 x | 16 augmentation terms] in fp16,
 * 288 bytes per element).  A store calls it once per appended / replaced block and hands the rows to xmem_affinity_topk_hinted
 * through xmem_key_segment.rows16 - the per-call rows kernel and its N x 288 bytes of writes disappear from the frame loop. */
int xmem_affinity_rows16(const float* key, const float* shrinkage, int n, void* rows16, void* stream);

/* segments are searched as one virtual concatenation (long | temporary | permanent in the reference's
 * order, memory_manager.py:82-83); out indices are positions in that concatenation.
 * qk [HW][C_k]; qe [HW][C_k] or NULL.  top_k in [1, 64], sum(n) >= top_k else XMEM_ERR_TOPK.
 * out_w [HW][top_k] softmax weights exp(v)/sum exp(v) (no max shift, memory_util.py:48-49), sorted by
 * descending similarity; out_idx [HW][top_k]; out_sim (nullable) [HW][top_k] raw similarities.
 * TIE RULE: equal similarities rank by ascending index, both inside the result and at its k-th place (torch.topk leaves
 *   that order open), so a query's top_k indices are distinct and fully determined by the fp32 similarities.
 * ZERO RULE: -0.0 and +0.0 are one value.  They tie (lower index first) and out_sim reports +0.0 for either.
 * NON-FINITE: a similarity of -inf (a key entry whose square overflows) is an ordinary value: it ranks last, by ascending index,
 *   with weight 0 and out_sim = -inf.  NaN inputs (and operands whose products give NaN, such as inf * 0) are outside the contract.
 * PATHS: memories of fewer than 256 tiles take one safe select; from 256 tiles on the call runs a bound pass and the wide select
 *   (xmem_affinity_plan_info reports which).  A tile is 32 rows of ONE segment, so the threshold is not an element count: a single
 *   segment reaches it at 8161 elements, segments of (1, 1, 1, 8100) elements at 8103. */
size_t xmem_affinity_topk_workspace_bytes(int n_total, int HW, int top_k);
int xmem_affinity_topk(const xmem_key_segment* segs_host, int n_seg,
                       const float* qk, const float* qe, int Ck, int HW, int top_k,
                       float* out_w, int32_t* out_idx, float* out_sim,
                       void* workspace, size_t workspace_bytes, void* stream);

/* Diagnostics for tools (not needed by a caller): byte offsets, inside a workspace sized for (n_total, HW), of the per-query
 * candidate counts [HW] int32, the per-128-query-tile flags of the two filter passes [2][ceil(HW/128)] int32 and the per-query
 * lower bounds [HW] float of the last xmem_affinity_topk_hinted call that took the fp16-filter path. */
int xmem_affinity_debug_offsets(int n_total, int HW, size_t* count_off, size_t* flag_off, size_t* bound_off);

/* Measurement aid: two HIP events (hipEvent_t, created with timing enabled) that the following xmem_affinity_topk_hinted calls
 * record on their stream right before and right after the pass-1 launch of the fp16 filter kernel - the kernel bench.py's
 * `roofline` object is about (the reference times the whole step with perf_counter, inference/run_on_video.py:106-113).
 * NULL, NULL turns it off.  The pair is held per calling host thread (thread_local): only that thread's later calls record it, so the
 * library keeps no process-wide mutable state; no effect on results. */
int xmem_affinity_profile_events(void* before_filter, void* after_filter);

/* Same function with an optional HINT: `idx` are the out_idx [HW][top_k] of an earlier call on the same list of stores (the
 * previous frame of the video), `seg_n` the segment sizes of that call, `grid_w` the width of the stride-16 query grid (0: do not
 * use grid neighbours).  The hint only bounds the k-th similarity from below (any k distinct elements give a valid bound; the
 * previous frame's matches give a tight one): results are bit-identical with and without it.  With a bound (and >= 256 tiles
 * of memory, see PATHS above) the N x HW contraction runs on the fp16 matrix pipe as a rigorously bounded filter and only the surviving
 * candidates are evaluated in fp32, with the arithmetic of the fp32 select (csrc/affinity_filter.hip).
 * hint == NULL behaves as xmem_affinity_topk.  The reference recomputes everything per frame (memory_manager.py:82-120). */
typedef struct {
    const int32_t* idx; int top_k;
    int n_seg; int seg_n[XMEM_MAX_SEGMENTS];
    int grid_w;
} xmem_affinity_hint;
int xmem_affinity_topk_hinted(const xmem_key_segment* segs_host, int n_seg,
                              const float* qk, const float* qe, int Ck, int HW, int top_k,
                              const xmem_affinity_hint* hint,
                              float* out_w, int32_t* out_idx, float* out_sim,
                              void* workspace, size_t workspace_bytes, void* stream);

/* The pipeline xmem_affinity_topk_hinted would run for segments of seg_n_host[0 .. n_seg) elements (the call launches from the same
 * numbers).  Host only: no GPU call; hint may be NULL, of a hint only the fields are read, hint->idx is compared with NULL and never
 * dereferenced.  Respects XMEM_AFFINITY_FILTER16.  Returns XMEM_OK or what the call's validation of these arguments returns. */
enum { XMEM_AFF_SMALL = 0,                    /* < 256 tiles: safe select + merge */
       XMEM_AFF_LARGE_SAMPLED = 1,            /* sampled bound pass, wide select, merge */
       XMEM_AFF_LARGE_HINTED_FP32 = 2,        /* bound from the hint, wide select, merge (XMEM_AFFINITY_FILTER16=0) */
       XMEM_AFF_LARGE_HINTED_FILTER16 = 3 };  /* bound from the hint, fp16 filter, exact refine */
typedef struct {
    int route;                      /* XMEM_AFF_* */
    int tiles;                      /* 32-row tiles, counted per segment */
    int splits, tiles_per_split;    /* of the select that runs (safe, wide, or the fp16 filter) */
    int chunk;                      /* wide select: tiles per chunk dealt round-robin to the splits; 0: contiguous ranges */
    int bound_stride, bound_splits; /* sampled route: the bound pass visits every bound_stride-th tile in bound_splits splits; else 0 */
    int list_cap, list_stride;      /* filter route: entries of a candidate list in pass 1 / its allocation (pass 2); else 0 */
} xmem_affinity_plan;
int xmem_affinity_plan_info(const int* seg_n_host, int n_seg, int HW, int top_k, const xmem_affinity_hint* hint,
                            xmem_affinity_plan* out);

/* usage = affinity.sum(dim=2) (memory_util.py:62-63) restricted to [first, first+count) of the index space,
 * accumulated order-independently (64-bit fixed point) and then folded into the store counters as
 * KeyValueMemoryStore.update_usage does (kv_memory_store.py:96-103): use_count += usage; life_count += 1.
 * fx_scratch: count uint64, zeroed by the call. */
int xmem_usage_update(const float* w, const int32_t* idx, int HW, int top_k, int first, int count,
                      float* use_count, float* life_count, uint64_t* fx_scratch, void* stream);

typedef struct {
    const float* value;  /* [n][C_v] rows of ONE object */
    int n;
} xmem_value_segment;

/* out[obj][q][c] = sum_s w[q][s] * V_obj[idx[q][s]][c]   (sparse form of v @ affinity).
 * vsegs_host: n_obj * n_seg entries, object-major; all objects share the index space of the group.
 * out [n_obj][HW][ldout] NHWC rows (pixel stride ldout >= C_v).
 * top_k in [1, 64] (what xmem_affinity_topk emits); a larger top_k returns XMEM_ERR_UNSUPPORTED and writes nothing.
 * C_v, ldout and obj_stride are multiples of 4; n_seg <= XMEM_MAX_SEGMENTS; every object has object 0's segment sizes. */
int xmem_readout_sparse(const xmem_value_segment* vsegs_host, int n_obj, int n_seg,
                        const float* w, const int32_t* idx, int HW, int top_k, int Cv,
                        float* out, int ldout, size_t obj_stride, void* stream);
/* The same readout with the output stored as IEEE halfs when out_half = 1 (ldout / obj_stride then count halfs): the fp16 loop's
 * decoder input.  Memory values stay fp32 (the permanent memory is preloaded in fp32, inference/run_on_video.py:59-66). */
int xmem_readout_sparse_t(const xmem_value_segment* vsegs_host, int n_obj, int n_seg,
                          const float* w, const int32_t* idx, int HW, int top_k, int Cv,
                          void* out, int out_half, int ldout, size_t obj_stride, void* stream);

/* Dense similarity (no top-k): sim[n][p], n over one segment, p over P queries.  Used by the long-term
 * consolidation (memory_manager.py:368) where the softmax runs over the candidate axis. out [P][n] (query-major). */
int xmem_similarity_dense(const float* key, const float* shrinkage, int n,
                          const float* qk, const float* qe, int P, int Ck, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Long-term consolidation (memory_manager.py:349-390) and eviction (kv_memory_store.py:160-181).
 * ------------------------------------------------------------------------------------------ */
/* usage[i] = use[i] / life[i] (kv_memory_store.py:183-189) */
int xmem_usage_ratio(const float* use, const float* life, float* usage, int n, void* stream);

/* torch.topk(values, k, largest, sorted=True) over a 1-D array by exact ranking (ties -> lower index first).
 * out_idx [k], out_val [k]. */
int xmem_topk_1d(const float* values, int n, int k, int largest, int32_t* out_idx, float* out_val, void* stream);

/* dst[i][0:C] = src[index[i]][0:C], i < n  (prototype gather, memory_manager.py:362-363) */
int xmem_gather_rows(const float* src, int C, const int32_t* index, int n, float* dst, void* stream);

/* in-place softmax over the last `count` entries of each row of sim [P][n] (do_softmax with top_k=None on
 * similarity[:, -count:], memory_util.py:55-60); entries before are zeroed. */
int xmem_softmax_rows_suffix(float* sim, int P, int n, int count, void* stream);

/* in-place top-k softmax of each row of sim [P][n], zeros elsewhere (do_softmax with top_k, memory_util.py:41-54: topk, exp
 * without max shift, / sum, scatter into zeros) on a materialised similarity; exact ties at the k-th value -> lowest indices. */
int xmem_softmax_rows_topk(float* sim, int P, int n, int k, void* stream);

/* out[p][c] = sum_i aff[p][n - count + i] * V[i][c], i < count: prototype values / shrinkage
 * (memory_manager.py:382-388).  V [count][C]. out [P][C]. */
int xmem_weighted_rows(const float* aff, int P, int n, int count, const float* V, int C, float* out, void* stream);

/* stream compaction for remove_obsolete_features: keep[i] = usage[i] > threshold (kv_memory_store.py:165);
 * out_index receives the kept indices in order, *out_count (device int) their number. */
int xmem_select_greater(const float* usage, int n, const float* threshold_dev, int32_t* out_index, int32_t* out_count, void* stream);

/* Eviction of a store with several object groups: every arena compacted by the same index of surviving key elements, one launch per
 * XMEM_COMPACT_MAX_ARENAS arenas (the descriptors travel by value in the kernel arguments).  The groups are suffix-aligned: an arena
 * of n rows holds the LAST n of the store's N = keep_cap elements, off = N - n (else XMEM_ERR_BAD_ARG).  With keep[0..m) ascending
 * (xmem_select_greater's out_index) and m = *m_dev read on the device (its out_count, clamped to [0, keep_cap]), arena a moves source
 * row keep[j] - off to destination row j - j0 for j >= j0, the first j with keep[j] >= off (binary search), and kept[a] (device int32
 * [n_arenas]) receives the number of rows it keeps, m - j0: all sizes reach the host in one transfer.  An arena of one object's
 * values is one entry; n = 0 is allowed (its pointers are not looked at, kept = 0).
 * src / dst: 4-byte aligned; rows whose width is a multiple of 4 floats on 16-byte-aligned bases move as 16-byte vectors.  NOT in
 * place: a destination that overlaps any source or another destination of the call is XMEM_ERR_BAD_ARG, as are null pointers, negative
 * counts, off < 0 and width < 1 - all before any GPU work.  Every source and destination row is checked against n on the device: an
 * index that is not ascending or out of range leaves rows unwritten, never an access outside an arena. */
#define XMEM_COMPACT_MAX_ARENAS 16
typedef struct {
    const float* src;   /* [n][width] rows */
    float* dst;         /* room for n rows of the same width */
    int width;          /* floats per row */
    int n;              /* rows before the compaction */
    int off;            /* N - n */
} xmem_compact_arena;
int xmem_store_compact(const xmem_compact_arena* arenas_host, int n_arenas, const int32_t* keep, const int32_t* m_dev, int keep_cap,
                       int32_t* kept, void* stream);

/* ------------------------------------------------------------------------------------------
 * Annotation-candidate selector (inference/frame_selection/frame_selection.py:99-244).
 * ------------------------------------------------------------------------------------------ */
/* Per-frame preparation (frame_selection.py:156-186): nearest-resize the C x H x W mask to h x w (as
 * torchvision Resize(NEAREST) on a tensor = F.interpolate(mode='nearest')), take the max over its channels,
 * form the composite key  c = (key * m) * alpha + key * one_minus_alpha  and expand it into the two
 * K = 2*C_k operands of the similarity: Mexp [HW][2C_k] = [c^2, c], Qexp [HW][2C_k] = [-e, 2 c e],
 * bsq [HW] = sum_c e c^2 (memory_util.py:20-27).  key / sel are [HW][C_k] rows.  mask may be NULL (c = key).
 * presence (device int32, nullable) receives #{pixels of the FULL-RES mask with max_c mask > eps}
 * (frame_selection.py:161-163). */
int xmem_selector_prepare(const float* key, const float* sel, const float* mask, int C, int H, int W,
                          int h, int w, int Ck, float alpha, float one_minus_alpha, float eps,
                          float* Mexp, float* Qexp, float* bsq, int32_t* presence, void* stream);

/* xmem_selector_prepare for a mask held as a uint8 label plane [H][W] and a 256-entry table: the mask value of a pixel is
 * lut[label] (the max over channels of the float mask the table stands for), read at the same nearest-neighbour source pixel;
 * presence receives #{pixels of the full plane with lut[label] > eps}.  Every output is bit-identical to xmem_selector_prepare
 * on that float mask.  mask and lut must not be NULL. */
int xmem_selector_prepare_u8(const float* key, const float* sel, const uint8_t* mask, const float* lut, int H, int W,
                             int h, int w, int Ck, float alpha, float one_minus_alpha, float eps,
                             float* Mexp, float* Qexp, float* bsq, int32_t* presence, void* stream);

/* Cycle dissimilarity of every frame f against frame `chosen` (frame_selection.py:218-226):
 *   out[f] = sum_{i,j} relu( S(mem=c_chosen[i], ms=s_chosen[i]; q=c_f[j], qe=e_f[j])
 *                          - S(mem=c_f[i],      ms=s_f[i];      q=c_chosen[j], qe=e_chosen[j]) ) / HW^2
 * Mexp/Qexp [n_frames][HW][2C_k], bsq/shrinkage [n_frames][HW] from xmem_selector_prepare; valid [n_frames]
 * uint8 (nullable; 0 => out[f] = 0 without computing, frame_selection.py:201-203).  out [n_frames] double
 * (deterministic fixed-order reduction).  C_k = 64. */
size_t xmem_cycle_dissimilarity_workspace_bytes(int n_frames, int HW);
int xmem_cycle_dissimilarity(const float* Mexp, const float* Qexp, const float* bsq, const float* shrinkage,
                             int n_frames, int HW, int Ck, int chosen, const uint8_t* valid, double* out,
                             void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* XMEM_HIP_H */
