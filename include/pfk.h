/*
 * pfk.h — C ABI of libpfk.so: hand-written gfx950 (MI355X / CDNA4) kernels for the RAFT-family
 * optical-flow hot path of hmorimitsu/ptlflow.
 *
 * Every entry point is `extern "C"`, takes raw *device* pointers + explicit sizes + a HIP stream,
 * allocates nothing, never synchronises, never throws; it returns 0 on success or a negative
 * pfk_status code (pfk_status_string() names it).  No torch types cross this boundary: the torch
 * extension (ptlflow_amd/csrc/pfk_torch.cpp), the ctypes tests and any other host language bind
 * exactly these symbols.
 *
 * Activation layout is *pixel-major* ("NHWC"): a feature map is a row-major matrix
 * [B*H*W pixels][ld floats] whose row p = (b*H + y)*W + x holds that pixel's channels
 * contiguously; `ld >= channels` lets several producers write channel slices of one buffer
 * (that is how the reference's torch.cat calls disappear).  All pointers must be 16-byte aligned
 * and every `ld` / channel count / channel offset a multiple of 4 floats.
 *
 * Reference interface each entry replaces (paths under hmorimitsu/ptlflow):
 *   pfk_corr_volume_f32   ptlflow/models/raft/corr.py:56-64   CorrBlock.corr (matmul / sqrt(D));
 *                         sea_raft/corr.py:109-117 (same op, per level)
 *   pfk_corr_pool2x2_f32  ptlflow/models/raft/corr.py:25-27   F.avg_pool2d(corr, 2, stride=2)
 *   pfk_corr_lookup_f32   ptlflow/models/raft/corr.py:29-54   CorrBlock.__call__ and
 *                         ptlflow/models/raft/utils.py:67-75  bilinear_sampler -> F.grid_sample
 *   pfk_conv2d_f32        ptlflow/models/raft/update.py:6-153 every nn.Conv2d of the update block
 *                         (+ the fused sigmoid/tanh/GRU-blend/relu epilogues of :58-73, :24-32,
 *                         :104-112, :144-153); torch.cat at :60,63,67,70,109,112,146 is replaced by
 *                         channel-slice addressing
 *   pfk_conv_cin2_f32     ptlflow/models/raft/update.py:100,107 (convf1: 7x7 conv on the 2-ch flow)
 *   pfk_flow_delta_f32    ptlflow/models/raft/update.py:10,14 (FlowHead.conv2) fused with
 *                         ptlflow/models/raft/raft.py:174,178 (flow = coords1-coords0; coords1 += d)
 *   pfk_convex_upsample_f32  ptlflow/models/raft/raft.py:112-123 RAFT.upsample_flow
 *   pfk_convex_upsample2_f32  ptlflow/models/ccmr/ccmr.py:128-139 CCMR.upsample_flow(scale=2) (ms_raft_plus.py:133-144 likewise)
 *   pfk_dwconv_layernorm_f32  ptlflow/models/sea_raft/layer.py:54-58,71-75 (ConvNextBlock dwconv + norm)
 *   pfk_convex_upsample_info_pm_f32  ptlflow/models/sea_raft/sea_raft.py:147-163 SEARAFT.upsample_data
 *   pfk_dwconv_layernorm_b16 / pfk_conv2d_gelu_b16 / pfk_convex_upsample_info_pm_b16  the same on the bf16 (K8b) path
 *   pfk_altcorr_forward_f32  ptlflow/utils/external/alt_cuda_corr/correlation_kernel.cu:258-285 (alt_cuda_corr.forward)
 *   pfk_corr_lookup_bwd_f32 / pfk_corr_volume_bwd_f32 / pfk_convex_upsample_bwd_f32
 *                         what torch.autograd runs for corr.py:29-64 and raft.py:112-123 in a training step (train.py;
 *                         gradients reach fmap1 / fmap2; RAFT detaches `coords` at raft.py:171, so these three give it none)
 *   pfk_corr_lookup_coords_bwd_f32  the sampling grid's gradient of the same grid_sample backward (raft/utils.py:67-75), for the
 *                         loops whose `coords1` carries one: ms_raft_plus.py:197-202 / ccmr.py:194-204 rebuild it from
 *                         `upsample_flow(..., up_mask, scale=2)` after the detach at the first iteration of a finer scale
 *   pfk_convex_upsample2_bwd_f32  what torch.autograd runs for ccmr.py:128-139 / ms_raft_plus.py:133-144 with scale = 2
 *   pfk_convex_upsample_info_bwd_pm_f32  what torch.autograd runs for sea_raft.py:147-163 in a training step (train_sea.py)
 * The native plug-in precedent in the reference is alt_cuda_corr
 * (ptlflow/utils/external/alt_cuda_corr/correlation.cpp:23-54: pybind forward/backward on raw
 * contiguous CUDA tensors); this header is the same kind of boundary, minus torch.
 */
#ifndef PFK_H
#define PFK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* pfk_stream_t; /* a hipStream_t */

enum pfk_status {
  PFK_OK = 0,
  PFK_ERR_BAD_ARG = -1,      /* null pointer, non-positive size, unsupported combination */
  PFK_ERR_ALIGNMENT = -2,    /* pointer not 16-byte aligned or ld/channels not a multiple of 4 */
  PFK_ERR_UNSUPPORTED = -3,  /* shape outside what the kernels were built for */
  PFK_ERR_LAUNCH = -4,       /* hipLaunchKernel reported an error */
  PFK_ERR_DISABLED = -5      /* a pfk_debug_set_* knob called in a process that did not opt in with PFK_DEBUG_KNOBS=1 */
};

#define PFK_MAX_LEVELS 8
#define PFK_ABI_VERSION 7

int pfk_abi_version(void);
const char* pfk_status_string(int status);
/* sha256 (first 16 hex digits) of the sources this library was built from (every file of csrc/, include/pfk.h, the compiler flags), stamped by
 * ptlflow_amd/_build.py; ptlflow_amd.load_native() refuses a library whose stamp differs from the tree it sits in. */
const char* pfk_source_hash(void);
/* The pfk_debug_set_* knobs change PROCESS-GLOBAL kernel selection (tests and tuning scripts force every tile shape / kernel
 * variant through them).  They are inert — return PFK_ERR_DISABLED and change nothing — unless the process environment has
 * PFK_DEBUG_KNOBS=1 at the first call, so a production caller cannot flip tile state by accident.  Not thread-safe.
 * tuning/debug knob: force the implicit-GEMM tile configuration (-1 = heuristic). */
int pfk_debug_set_tile(int cfg);
/* test hook: n / d through the multiplier arithmetic the persistent convolution kernel decodes its tiles with (n < 2^31, d >= 1) */
unsigned pfk_debug_fastdiv(unsigned n, unsigned d);
/* tuning knob of the pyramid lookup: source pixels per workgroup — 4 (default: 4 on the row-major layout; on the blocked layout 4
 * below 28 160 source pixels and 8 from there up), 8, 104 (always 4), 14 (4 with cross-lane tap reads, row-major only). */
int pfk_debug_set_lookup_pix(int pix);
int pfk_debug_set_altcorr(int mode);       /* on-demand correlation forward: 0 = heuristic, 1 = per-pixel kernel, 2 / 3 = window-sharing MFMA kernel on 8x4 / 8x8 patches */
int pfk_debug_set_wgrad(int variant);      /* weight-gradient tile height: 0 = by padding waste, 1 / 2 / 4 = forced 32 / 64 / 128 rows (tuning knob) */

/* ---- K1: all-pairs correlation --------------------------------------------------------------
 * out[b][i][j] = scale * sum_d f1[b][i][d] * f2[b][j][d]        (fp32 MFMA, exact fp32 products)
 * f1 [B][N1][ld1], f2 [B][N2][ld2] pixel-major, D channels used; out [B][N1][N2] row-major,
 * i.e. for source pixel i a full [h2][w2] map — the reference's [B*N,1,h2,w2] volume.
 * D % 4 == 0 and ld2 == D rounded up to a multiple of 32: the rows of f2 are read as packed weight rows, all ld2 columns of them,
 * against f1 channels that read as zero past D — so the columns [D, ld2) of f2 must hold zeros (anything finite gives the same
 * result; a NaN or inf there poisons the row's outputs).  The columns [D, ld1) of f1 are never read. */
int pfk_corr_volume_f32(const float* f1, int ld1, const float* f2, int ld2, float* out,
                        int B, int N1, int N2, int D, float scale, pfk_stream_t stream);

/* bf16 operands, bf16 volume — what the reference's matmul produces under torch.autocast(bfloat16):
 * f1_bf16 [B][N1][ld1], f2_bf16 [B][N2][ld2] bf16 rows (ld % 8 == 0, D % 8 == 0), out_bf16 [B][N1][N2] bf16; fp32 accumulate
 * on the bf16 matrix cores, scaled, rounded to nearest even.  HBM-write-bound (2 B per volume element). */
int pfk_corr_volume_bf16(const void* f1_bf16, int ld1, const void* f2_bf16, int ld2, void* out_bf16, int B, int N1, int N2, int D,
                         float scale, pfk_stream_t stream);

/* ---- K2: 2x2/stride-2 average pool over the target dims (floor) ------------------------------
 * in [M][H][W] -> out [M][H/2][W/2], value ((a00+a01)+a10)+a11) * 0.25 (torch's CPU order). */
int pfk_corr_pool2x2_f32(const float* in, float* out, int64_t M, int H, int W,
                         pfk_stream_t stream);
/* same on bf16 maps: fp32 accumulation, one rounding to bf16 (torch's avg_pool2d on bf16 tensors) */
int pfk_corr_pool2x2_bf16(const void* in, void* out, int64_t M, int H, int W, pfk_stream_t stream);
/* 2x2 average of a pixel-major FEATURE map [B][H][W][in_ld] -> [B][H/2][W/2][out_ld] (C channels): bit-identical to
 * F.interpolate(fmap2, scale_factor=0.5, mode="bilinear", align_corners=False), SEA-RAFT's pyramid step
 * (sea_raft/corr.py:81-83), and to F.avg_pool2d(fmap2, 2, 2) (AlternateCorrBlock, raft/corr.py:72-74). */
int pfk_fmap_pool2x2_f32(const float* in, int in_ld, float* out, int out_ld, int B, int H, int W, int C, pfk_stream_t stream);

/* ---- K3: radius-r bilinear lookup over all pyramid levels in one launch ----------------------
 * levels[l] is the level-l volume [B*N][lvl_h[l]][lvl_w[l]]; coords is [B][2][h][w] (x then y,
 * pixel units, fp32, NCHW as the reference passes it).  Output: out[p*out_ld + l*n*n + i*n + j]
 * with n = 2r+1, sample (i, j) taken at (x/2^l + i - r, y/2^l + j - r) — the reference's
 * x-offset-major window — through grid_sample's exact fp32 normalise/un-normalise round trip,
 * zero padding per tap, FMA accumulation order of torch's CPU kernel (bit-exact values for the
 * same pyramid).  NaN / inf coordinates and 1-pixel levels give NaN exactly like the reference. */
typedef struct {
  const void* levels[PFK_MAX_LEVELS];   /* float maps (pfk_corr_lookup_f32) or bf16 maps (pfk_corr_lookup_bf16) */
  int lvl_h[PFK_MAX_LEVELS];
  int lvl_w[PFK_MAX_LEVELS];
  int num_levels;
  int radius;      /* 1..4 */
  int B, h, w;     /* source grid: N = h*w pixels per batch element */
  const float* coords;
  void* out;       /* fp32 rows, or bf16 rows when out_bf16 != 0 */
  int out_ld;      /* in elements; >= num_levels*(2r+1)^2, multiple of 4 */
  int out_bf16;    /* ABI 7: 0 = `out` holds fp32, 1 = bf16 (each sample rounded to nearest even: what autocast hands the next
                      convolution; columns the lookup does not write — the pad up to out_ld — are left untouched) */
} pfk_lookup_desc;
int pfk_corr_lookup_f32(const pfk_lookup_desc* d, pfk_stream_t stream);
/* same with `levels` pointing to bf16 maps; arithmetic and output fp32 (grid_sample is an fp32 op under autocast) */
int pfk_corr_lookup_bf16(const pfk_lookup_desc* d, pfk_stream_t stream);

/* ---- K1-K3 on the BLOCKED volume layout (round 5; inference path) -------------------------------------------------------
 * A level's [H][W] map per source pixel stored as ceil(H/4) x ceil(W/8) tiles of 4 rows x 8 columns, 32 consecutive elements per
 * tile (one 128-byte line in fp32): element (y, x) of a map lives at ((y/4 * ceil(W/8) + x/8) * 32 + (y%4) * 8 + x%8);
 * pfk_blocked_map_elems(H, W) elements per source pixel (pad elements of edge tiles are zero).  The 12 x 12 window a lookup
 * stages covers ~9 lines instead of ~16 (raft/corr.py:29-54 reads the same taps either way).
 *   pfk_fmap_to_blocked_f32      permutes the rows of the target feature map [B][H*W][in_ld] into that order (zero rows for pad
 *                                elements): out [B][pfk_blocked_map_elems(H, W)][out_ld].  pfk_corr_volume_f32 / _bf16 run against
 *                                it (N2 = pfk_blocked_map_elems) write level 0 directly in the blocked layout (raft/corr.py:56-64).
 *   pfk_corr_pool2x2_blocked_*   K2 blocked -> blocked (raft/corr.py:25-27), the same ((a00+a01)+a10)+a11)*0.25 per element.
 *   pfk_corr_lookup_blocked_*    K3 on blocked levels: the same pfk_lookup_desc (lvl_h / lvl_w = the maps' LOGICAL sizes), the same
 *                                arithmetic, bit-identical output to pfk_corr_lookup_* on the row-major pyramid. */
int64_t pfk_blocked_map_elems(int H, int W);
int pfk_fmap_to_blocked_f32(const float* in, int in_ld, float* out, int out_ld, int B, int H, int W, int C, pfk_stream_t stream);
int pfk_corr_pool2x2_blocked_f32(const float* in, float* out, int64_t M, int H, int W, pfk_stream_t stream);
int pfk_corr_pool2x2_blocked_bf16(const void* in, void* out, int64_t M, int H, int W, pfk_stream_t stream);
int pfk_corr_lookup_blocked_f32(const pfk_lookup_desc* d, pfk_stream_t stream);
int pfk_corr_lookup_blocked_bf16(const pfk_lookup_desc* d, pfk_stream_t stream);

/* ---- backward of K3 (training): scatter d(out) through the forward's four bilinear weights --------------------
 * grad_out [B*N][grad_out_ld] (the layout of pfk_corr_lookup_f32's `out`); grad_levels[l] is the gradient of the level-l
 * volume, one [lvl_h][lvl_w] map per source pixel at row stride lvl_ld[l] floats (>= lvl_h*lvl_w; a stride padded to a
 * multiple of 4 makes the buffer a legal operand of pfk_corr_volume_bwd_f32).  ACCUMULATES (+=): the caller zeroes the
 * buffers once per training step and every recurrent iteration's lookup adds into them.  Deterministic (no atomics).
 * Taps that fell outside the map in the forward (zero padding) receive nothing.  Non-finite coordinates (NaN, +-inf), coordinates
 * too large for the map and every tap of a 1-pixel-high or -wide level (whose round trip divides by zero: the forward returns NaN
 * there) add exactly 0, as grid_sample's backward does: a finite grad_out never puts a NaN into grad_levels. */
typedef struct {
  float* grad_levels[PFK_MAX_LEVELS];
  int lvl_h[PFK_MAX_LEVELS];
  int lvl_w[PFK_MAX_LEVELS];
  long long lvl_ld[PFK_MAX_LEVELS];
  int num_levels;
  int radius;      /* 1..4 */
  int B, h, w;
  const float* coords;    /* [B][2][h][w], the coordinates the forward was called with */
  const float* grad_out;
  int grad_out_ld;
} pfk_lookup_bwd_desc;
int pfk_corr_lookup_bwd_f32(const pfk_lookup_bwd_desc* d, pfk_stream_t stream);

/* ---- coordinate gradient of K3 (training of the multi-scale loops; added within ABI 7: an addition only) -------------------
 * levels[l]: the level-l volume the forward read, ROW-MAJOR fp32, one [lvl_h][lvl_w] map per source pixel at row stride lvl_ld[l]
 * floats (>= lvl_h*lvl_w; the training path's pyramid: lvl_ld = lvl_h*lvl_w).  grad_out [B*N][grad_out_ld] as above.
 * grad_coords [B][2][h][w] (x then y) is WRITTEN, not accumulated:
 *   grad_x[p] = sum over levels l and taps (i, j) of grad_out[p][l][i][j] * 2^-l * [(v10 - v00)(1 - wy) + (v11 - v01) wy]
 *   grad_y[p] = ...                                                      * 2^-l * [(v01 - v00)(1 - wx) + (v11 - v10) wx]
 * with v.. the four values around the tap's sample point (x/2^l + i - r, y/2^l + j - r) — v10 one column to the right, v01 one row
 * down, 0 outside the map — and wx, wy its fractional parts, floor and weights taken from the forward's fp32 round trip: what
 * grid_sample's backward gives the grid, times the chain of corr.py:45-52.  Non-finite coordinates, coordinates too large for the
 * map and every tap of a 1-pixel-high or -wide level contribute exactly 0 (as to grad_levels above): a finite grad_out never yields
 * a NaN.  One wave per source pixel, one fixed-order wave sum per component: deterministic, no atomics.  Status codes as
 * pfk_corr_lookup_bwd_f32 (+ BAD_ARG for a null level or grad_coords). */
typedef struct {
  const float* levels[PFK_MAX_LEVELS];
  int lvl_h[PFK_MAX_LEVELS];
  int lvl_w[PFK_MAX_LEVELS];
  long long lvl_ld[PFK_MAX_LEVELS];
  int num_levels;
  int radius;      /* 1..4 */
  int B, h, w;
  const float* coords;    /* [B][2][h][w], the coordinates the forward was called with */
  const float* grad_out;
  int grad_out_ld;
  float* grad_coords;     /* [B][2][h][w] */
} pfk_lookup_coords_bwd_desc;
int pfk_corr_lookup_coords_bwd_f32(const pfk_lookup_coords_bwd_desc* d, pfk_stream_t stream);

/* ---- backward of K1 for one batch element and one pyramid level (training) -----------------------------------
 * The level-l volume is C = scale * F1 . F2_l^T with F2_l the (avg-pooled / bilinearly halved) target feature map, so
 *   df1[i][d]  = (accumulate_df1 ? df1[i][d] : 0) + scale * sum_j dC[i][j] * f2[j][d]         i < N1   (fp32 MFMA GEMM)
 *   df2[j][d]  =                                       scale * sum_i dC[i][j] * f1[i][d]         j < ldc  (transposed product)
 * dC [N1][ldc]: ldc % 4 == 0, columns [N2, ldc) zero.  f1 [N1][ld1] pixel-major.  f2_cm: F2_l CHANNEL-major [D][ld2cm],
 * ld2cm == round_up(ldc, 32), columns >= N2 zero (pfk_pm_to_cm_f32 into a zeroed buffer).  df1 [N1][df1_ld];
 * df2 [ldc][round_up(D, 32)] pixel-major (rows >= N2 and columns >= D come out zero).
 * workspace: pfk_corr_volume_bwd_workspace_bytes(N1, ldc, D) bytes, 16-byte aligned (may be NULL when that is 0). */
long long pfk_corr_volume_bwd_workspace_bytes(int N1, int ldc, int D);
int pfk_corr_volume_bwd_f32(const float* dC, int ldc, int N1, int N2, const float* f1, int ld1, const float* f2_cm, int ld2cm,
                            int D, float scale, float* df1, int df1_ld, int accumulate_df1, float* df2, void* workspace,
                            long long workspace_bytes, pfk_stream_t stream);

/* ---- backward of the convex upsampling (raft/raft.py:112-123) -------------------------------------------------
 * flow: NCHW [B][2][H][W] (flow_ld == 0) or pixel-major rows flow[p*flow_ld + 0..1]; mask pixel-major [M][mask_ld] as in
 * pfk_convex_upsample_f32; grad_out [B][2][8H][8W] -> grad_mask pixel-major [M][grad_mask_ld] (576 channels written),
 * grad_flow [B][2][H][W].  workspace: pfk_convex_upsample_bwd_workspace_bytes(B, H, W).  Deterministic. */
long long pfk_convex_upsample_bwd_workspace_bytes(int B, int H, int W);
int pfk_convex_upsample_bwd_f32(const float* flow, int flow_ld, const float* mask, int mask_ld, const float* grad_out,
                                float* grad_mask, int grad_mask_ld, float* grad_flow, void* workspace, long long workspace_bytes,
                                int B, int H, int W, pfk_stream_t stream);

/* ---- backward of pfk_convex_upsample2_f32 (`upsample_flow(flow, mask, scale=2)`; added within ABI 7: an addition only) -------
 * flow and mask as pfk_convex_upsample2_f32 reads them (flow_ld == 0: NCHW, else pixel-major rows; 36 logits per mask row);
 * grad_out [B][2][2H][2W] -> grad_mask pixel-major [M][grad_mask_ld] (36 columns written, grad_mask_ld >= 36) and grad_flow, NCHW
 * [B][2][H][W] (grad_flow_ld == 0) or pixel-major rows grad_flow[p*grad_flow_ld + 0..1] (grad_flow_ld >= 2).  8-byte aligned mask,
 * grad_mask and grad_out with even row strides take 8-byte accesses, anything else 4-byte ones, with the same bits.
 * workspace: pfk_convex_upsample2_bwd_workspace_bytes(B, H, W) bytes.  Deterministic (no atomics, a fixed summation order).
 * PFK_ERR_BAD_ARG: a null pointer, a non-positive size, mask_ld or grad_mask_ld < 36, a row stride of 1 or a negative one, a
 * workspace that is too small; PFK_ERR_UNSUPPORTED: more pixels than a launch grid holds. */
long long pfk_convex_upsample2_bwd_workspace_bytes(int B, int H, int W);
int pfk_convex_upsample2_bwd_f32(const float* flow, int flow_ld, const float* mask, int mask_ld, const float* grad_out,
                                 float* grad_mask, int grad_mask_ld, float* grad_flow, int grad_flow_ld, void* workspace,
                                 long long workspace_bytes, int B, int H, int W, pfk_stream_t stream);

/* ---- backward of pfk_convex_upsample_info_pm_f32 (SEARAFT.upsample_data, sea_raft/sea_raft.py:147-163), fp32, pixel-major -----
 * flow_pm / info_pm / mask as the forward reads them (columns 0..1, 0..n_info-1, 0..575 of their rows; 0 <= n_info <= 8, info_pm
 * and grad_info_pm may be NULL when n_info == 0); grad_flow_up [B][2][8H][8W], grad_info_up [B][n_info][8H][8W] or NULL (= zero)
 * -> grad_mask [M][grad_mask_ld] (576 columns written), grad_flow_pm[p*grad_flow_ld + 0..1] and grad_info_pm[p*grad_info_ld +
 * 0..n_info-1]: rows with their own ld, so both may point into one [M][8] buffer (columns 0..1 and 2..5: the gradient of
 * flow_head's output).  mask, grad_mask, grad_flow_up, grad_info_up 16-byte aligned, mask_ld % 4 == 0 and grad_mask_ld % 4 == 0
 * (PFK_ERR_ALIGNMENT otherwise).  workspace: pfk_convex_upsample_info_bwd_workspace_bytes(B, H, W, n_info) bytes
 * (B*H*W*9*(2 + n_info) floats).  Deterministic: no atomics, fixed summation order. */
long long pfk_convex_upsample_info_bwd_workspace_bytes(int B, int H, int W, int n_info);
int pfk_convex_upsample_info_bwd_pm_f32(const float* flow_pm, int flow_ld, const float* info_pm, int info_ld, int n_info,
                                        const float* mask, int mask_ld, const float* grad_flow_up, const float* grad_info_up,
                                        float* grad_mask, int grad_mask_ld, float* grad_flow_pm, int grad_flow_ld, float* grad_info_pm,
                                        int grad_info_ld, void* workspace, long long workspace_bytes, int B, int H, int W,
                                        pfk_stream_t stream);

/* ---- K4-K6: "same"-padded convolution (stride 1, or s for the encoders) as an implicit GEMM on fp32 MFMA ----
 * out[p][co] = epilogue( bias[co] + sum_{s, ky, kx, c} src[s][p + (ky-kh/2)*W + (kx-kw/2)][c]
 *                                                    * weight[co][k(s,ky,kx,c)] )
 * Input channels may come from up to 3 pixel-major sources (the reference's torch.cat operands).
 * Packed weight: row-major [cout][ktot]; k enumerates, for each source s in order, each tap
 * (ky major, kx minor), the source's channels padded up to a multiple of 32 (pad weights = 0):
 * ktot = sum_s kh*kw*round_up(channels_s, 32).  pfk_conv_ktot() returns it. */
enum pfk_epilogue {
  PFK_EPI_LINEAR = 0,  /* v = (acc+bias) ; relu? ; v *= scale ; [v = residual[p*residual_ld+co] + v] ;
                          out[p*out_ld + out_coff + co] = v */
  PFK_EPI_GRU_ZR = 1,  /* cout = 2*Ch: v = acc + bias [+ residual[p*residual_ld+co]]; co<Ch: z=sigmoid(v) -> aux_z[p*Ch+co];
                          co>=Ch: r=sigmoid(v) -> aux_rh[p*Ch + co-Ch] = r * h[p*h_ld + co-Ch] */
  PFK_EPI_GRU_Q = 2,   /* cout = Ch: q=tanh(acc + bias [+ residual]); h[p*h_ld+co] = (1-z)*h + z*q, z = aux_z[p*Ch+co] */
  PFK_EPI_LINEAR_GELU = 3  /* (added in ABI 7) LINEAR with the exact GELU in place of relu: v = (acc+bias) ;
                              v = 0.5*v*(1 + erf(v/sqrt(2))) ; v *= scale ; [v = residual + v] ; out = v.  `relu` must be 0;
                              `relu_after_residual` as LINEAR.  sea_raft/layer.py:60-62,74-75 (pwconv1 + nn.GELU()).
                              pfk_conv2d_f32 (tile grid and stream-K, no cout_active / cout_split) and pfk_conv2d_gelu_b16:
                              pfk_conv2d_group_f32, pfk_conv2d_bf16s and pfk_conv2d_b16 return PFK_ERR_UNSUPPORTED for it */
};

typedef struct {
  const float* ptr;
  int ld;        /* row stride in floats */
  int channels;  /* channels read from each row (multiple of 4) */
} pfk_conv_src;

typedef struct {
  pfk_conv_src src[3];
  int num_src;
  int B, H, W;
  int kh, kw;            /* odd; padding kh/2, kw/2 */
  const float* weight;   /* packed [cout][ktot] */
  const float* bias;     /* [cout] or NULL */
  int cout;
  int epilogue;          /* enum pfk_epilogue */
  int relu;              /* LINEAR only */
  float scale;           /* LINEAR only (1.0f for none) */
  float* out;            /* LINEAR only */
  int out_ld, out_coff;
  float* h;              /* GRU_ZR (read) / GRU_Q (read+write): hidden state slice */
  int h_ld;
  float* aux_z;          /* [M][Ch] */
  float* aux_rh;         /* [M][Ch] */
  const float* residual; /* optional [M][cout] rows.  LINEAR: added after relu/scale (GMA's `fmap + gamma*out`, gma_utils.py:111).
                            GRU_ZR / GRU_Q (ABI 5): added to the gate PRE-activation — the loop-invariant part of a gate's
                            convolution: in raft/update.py:60-71 the GRU input is cat([h, inp, motion]) and `inp` (the context
                            features, raft.py:158-160) does not change over the iterations, so conv(W[:, inp slice], inp) + bias is
                            computed once per forward and handed in here while the per-iteration convolution covers the h and
                            motion channels only (16-byte aligned, residual_ld % 4 == 0) */
  int residual_ld;
  int stride;            /* 0 or 1: "same" convolution; s > 1: output (yo, xo) reads input (yo*s + ky - kh/2, xo*s + kx - kw/2),
                            Ho = (H-1)/s + 1, Wo = (W-1)/s + 1 (= PyTorch's Conv2d(k, stride=s, padding=k/2)); H, W are the
                            INPUT dims, sources have B*H*W rows, out / h / aux / residual have B*Ho*Wo rows */
  int relu_after_residual; /* LINEAR only: relu once more after the residual add (ResidualBlock, raft/extractor.py:53-61) */
  void* workspace;       /* optional: >= pfk_conv_workspace_bytes() of device memory, 16-byte aligned, private to
                            the stream, ZERO-FILLED by the caller once after allocation (the kernels leave its flag region
                            zeroed); enables the stream-K schedule for small grids (deterministic).  NULL: tile grid */
  long long workspace_bytes;
  int cout_active;       /* ABI 6, LINEAR only: 0 or >= cout = every output channel; otherwise only output channels [0, cout_active)
                            (a multiple of 64) are computed and written, the rest of `out` is left untouched — with EXACTLY the bits
                            the full launch gives those channels: the tile schedule (tile grid or stream-K, and the stream-K split
                            points) is chosen for the full `cout` and the column tiles past cout_active are skipped.  The fused
                            flow-head | mask-head convolution (raft/update.py:13, :138-139) on the iterations whose mask nobody
                            reads (raft/raft.py:180-192 in eval). */
  int cout_split;        /* ABI 6, LINEAR only, 0 = none: the output channels form two groups [0, cout_split) and [cout_split, cout)
                            of equal width (a multiple of 64; 2 * cout_split == cout) and the stream-K schedule walks their column
                            tiles INTERLEAVED (group 0's first tile, group 1's first tile, group 0's second ...), so that a launch
                            with cout_active == cout_split still gives every block about half of its range to do.  Pass the same
                            value in the full launch and in the cout_active launch: the schedule, hence the bits, are then the
                            same.  Tile-grid schedules ignore it. */
} pfk_conv_desc;

long long pfk_conv_workspace_bytes(void);
/* Byte offset, inside a conv workspace, of a 32-bit counter of stream-K fix-ups that timed out (a partner block's partial
 * tile never became visible within the bounded spin).  The caller zero-initialises the workspace once; the kernels only
 * ever increment the word, and the affected output tile is written as NaN.  0 = every result so far is complete; after a
 * non-zero reading zero-fill the workspace again before the next launch (flags of the lost fix-up may be left set). */
long long pfk_conv_workspace_fault_offset(void);
int pfk_conv_ktot(const pfk_conv_desc* d);
int pfk_conv2d_f32(const pfk_conv_desc* d, pfk_stream_t stream);

/* Grouped launch (ABI 7): `n` (1..PFK_CONV_GROUP_MAX) INDEPENDENT convolutions — no output of one is a source, residual or weight of
 * another — in ONE grid of 64 x 64 tiles; every descriptor has the LINEAR epilogue.  Results are those of `n` calls of
 * pfk_conv2d_f32 without a workspace, bit for bit (a tile's K order does not depend on what runs beside it).  For the small-batch
 * regime, where the update block's launches leave most CUs idle: convc1 | convf2 | the previous iteration's mask conv2
 * (ptlflow/models/raft/update.py:105-108, :152 — `cor` and `flo` only meet in `conv`, the mask head reads `net` only).
 * `workspace`, `cout_active`, `cout_split` of the descriptors: ignored / unsupported (PFK_ERR_UNSUPPORTED). */
#define PFK_CONV_GROUP_MAX 4
int pfk_conv2d_group_f32(const pfk_conv_desc* descs, int n, pfk_stream_t stream);

/* Winograd F(2x2,3x3) form of pfk_conv2d_f32 for 3x3 stride-1 convolutions (fp32 MFMA, fp32 accumulate): 16 GEMMs over the
 * transformed input, 2.25x fewer products than the direct form.  Supported: one source with channels % 32 == 0, kh = kw = 3,
 * stride 0 or 1, the LINEAR epilogue without residual or relu_after_residual, `cout_active` (0, >= cout, or a multiple of 64:
 * exactly the bits the full launch gives those channels), source, output (and residual) spans below 2 GB from their pointers
 * (32-bit byte offsets).  Anything else returns PFK_ERR_UNSUPPORTED.  `workspace` and
 * `cout_split` are ignored (one schedule, no workspace: safe under graph capture).  Results differ from pfk_conv2d_f32 by fp32
 * rounding (other products, other order); the same inputs give the same bits on every run.
 * d->weight = the transformed weight, pfk_conv_wino_weight_floats(cin, cout) floats, 16-byte aligned:
 *   U = G g G^T per (co, c), G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1], rounded to fp32 once, laid out
 *   [ceil(cout/64)][cin/8][16 (xi = 4*row + col of U)][64 (nl)][8 (slot)] with co = 64*cb + nl, c = 8*ks + cc,
 *   slot = ((cc & 3)*2 + (cc >> 2)) ^ (((nl >> 2) & 3)*2), zeros for co >= cout (ptlflow_amd/packing.py, pack_wino_weight) */
long long pfk_conv_wino_weight_floats(int cin, int cout);   /* < 0 (PFK_ERR_BAD_ARG) unless cin % 32 == 0, cin, cout > 0 */
int pfk_conv2d_wino_f32(const pfk_conv_desc* d, pfk_stream_t stream);

/* The same kernel with the residual-block epilogue (sea_raft/layer.py:144-150, `relu(x + relu(bn2(conv2(y))))`):
 * v = relu?(acc + bias) * scale; v = residual[p*residual_ld + co] + v; relu_after_residual?.  `residual` is required (fp32 rows,
 * residual_ld >= cout; PFK_ERR_BAD_ARG otherwise), `cout_active` is not supported; everything else as pfk_conv2d_wino_f32, which
 * keeps refusing a residual. */
int pfk_conv2d_wino_res_f32(const pfk_conv_desc* d, pfk_stream_t stream);

/* pfk_conv2d_wino_f32 with the instance norm IN FRONT of the convolution folded into its loads: d->src[0] is the raw output of the
 * previous convolution, in_mean / in_rstd ([B][cin] fp32, e.g. of pfk_instnorm_stats_f32) its statistics, and every tap becomes
 * in_relu?((x - mean) * rstd) in registers — pfk_norm_apply_f32's arithmetic; the zero padding is applied after the norm.  The
 * output has the bits of pfk_norm_apply_f32 followed by pfk_conv2d_wino_f32.  Null statistics: PFK_ERR_BAD_ARG; everything else
 * as pfk_conv2d_wino_f32. */
int pfk_conv2d_wino_norm_f32(const pfk_conv_desc* d, const float* in_mean, const float* in_rstd, int in_relu, pfk_stream_t stream);

/* pfk_conv2d_wino_f32 that also yields the instance-norm statistics of its OUTPUT (out_mean / out_rstd, [B][cout] fp32): the
 * epilogue sums what it stores, and its square, in double per (block, column); the blocks of an image are reduced in a fixed order
 * and finished as pfk_instnorm_stats_f32 finishes (no atomics: the same bits on every run).  The output has pfk_conv2d_wino_f32's
 * bits; mean / rstd can differ from pfk_instnorm_stats_f32's by the order of a double sum, i.e. only where a double falls on an fp32
 * rounding boundary.  in_mean / in_rstd: both null, or both given as for pfk_conv2d_wino_norm_f32.  `workspace`: 8-byte aligned,
 * at least pfk_conv_wino_stats_workspace_bytes(B, H, W, cout) bytes, no need to clear it.  A residual, relu_after_residual, a null
 * out_mean / out_rstd / workspace or a short workspace: PFK_ERR_BAD_ARG; `cout_active` below cout: PFK_ERR_UNSUPPORTED. */
long long pfk_conv_wino_stats_workspace_bytes(int B, int H, int W, int cout);   /* < 0 (PFK_ERR_BAD_ARG) unless all > 0 */
int pfk_conv2d_wino_stats_f32(const pfk_conv_desc* d, const float* in_mean, const float* in_rstd, int in_relu, float eps,
                              float* out_mean, float* out_rstd, void* workspace, long long workspace_bytes, pfk_stream_t stream);

/* 1-D Winograd F(4,5) form of pfk_conv2d_f32 for the 1x5 / 5x1 stride-1 convolutions of the SepConvGRU (raft/update.py:58-73;
 * fp32 MFMA, fp32 accumulate): 8 GEMMs over the transformed input per 4 outputs along the convolution axis, 2.5x fewer products
 * than the direct form.  Supported: (kh, kw) = (1, 5) or (5, 1), stride 0 or 1, one or two sources in K order (channels % 8 == 0
 * each), the epilogues PFK_EPI_LINEAR (bias, relu, scale; no residual), PFK_EPI_GRU_ZR and PFK_EPI_GRU_Q exactly as defined above
 * (optional `residual` rows added to the pre-activation, h through h_ld, q updates h in place).  `cout_active` below cout,
 * `relu_after_residual`, any other kernel size, stride, epilogue or source count, a source, and with the gate epilogues `residual`,
 * h, aux_z or aux_rh, that spans 2 GB or more up to its last pixel's last column: PFK_ERR_UNSUPPORTED.  `workspace` and `cout_split`
 * are ignored (one schedule, no workspace).  Results differ from pfk_conv2d_f32 by fp32 rounding (pre-activation error about 6e-6 at
 * K = 256 with unit-scale operands, several times the direct form's); the same inputs give the same bits on every launch.
 * d->weight = the transformed weight, pfk_conv_wino1d_weight_floats(ktot, cout) floats, 16-byte aligned, ktot = the sources'
 * channels summed:  U = G g per (co, c) over the 5 taps (correlation order), interpolation points 0, +-1, +-2, +-1/2, inf,
 *   G = [-1 0 0 0 0; -2/9 -2/9 -2/9 -2/9 -2/9; -2/9 2/9 -2/9 2/9 -2/9; 1/90 1/45 2/45 4/45 8/45; 1/90 -1/45 2/45 -4/45 8/45;
 *        32/45 16/45 8/45 4/45 2/45; 32/45 -16/45 8/45 -4/45 2/45; 0 0 0 0 1],
 * made in float64 and rounded to fp32 once, laid out [ceil(cout/128)][ktot/8][8 (component)][128 (nl)][8 (slot)] with
 * co = 128*cb + nl, k = 8*ks + cc, slot as in pfk_conv2d_wino_f32's weight, zeros for co >= cout and for a source's pad channels
 * (ptlflow_amd/packing.py, pack_wino1d_weight). */
long long pfk_conv_wino1d_weight_floats(int ktot, int cout);   /* < 0 (PFK_ERR_BAD_ARG) unless ktot % 8 == 0, ktot, cout > 0 */
int pfk_conv1d_wino_f32(const pfk_conv_desc* d, pfk_stream_t stream);

/* Same convolution on the bf16 matrix cores with split operands (fp32 in HBM, fp32 accumulate, fp32 epilogue).
 * Every fp32 operand x is replaced by the sum of its first `nsplit` bf16 planes x0 = bf16(x), x1 = bf16(x - x0),
 * x2 = bf16(x - x0 - x1); a product keeps the terms a_i*b_j with i + j < nsplit:
 *   nsplit 1: plain bf16 operands (what the reference computes under `--fp16` autocast with bf16,
 *             model_benchmark.py:311 / base_model.py autocast), nsplit 2: ~2^-17 relative product error,
 *   nsplit 3: fp32-grade products at 6 bf16 MFMAs per 16 channels.
 * Activations are split by the kernel while staging; the caller pre-splits the weight:
 * weight_planes = bf16 [nsplit][cout][ktot], ktot = pfk_conv_ktot_bf16(d) (= pfk_conv_ktot(d): the fp32 packed
 * weight's k order and padding, split plane by plane).  d->weight, d->workspace are ignored. */
int pfk_conv_ktot_bf16(const pfk_conv_desc* d);
int pfk_conv2d_bf16s(const pfk_conv_desc* d, const void* weight_planes, int nsplit, pfk_stream_t stream);

/* ---- K8b (ABI 7): the same convolution with bf16 ACTIVATION STORAGE on the bf16 matrix cores ---------------------------
 * What the reference's convolutions compute under its reduced-precision switch (scripts/model_benchmark.py:317-319,
 * validate.py:243-244 / torch.autocast(bfloat16): every nn.Conv2d of raft/update.py:6-153 reads and writes 16-bit tensors).
 * Sources are bf16 pixel-major rows (`ld`, `channels` in ELEMENTS, multiples of 8; 16-byte aligned), the weight is bf16
 * [cout][ktot] with the K order of pfk_conv2d_f32's packed weight but 64-channel chunks: for each source, each tap (ky major), the
 * source's channels zero-padded to a multiple of 64 — ktot = pfk_conv_ktot_b16(d).  Both operands go global -> LDS by LDS-DMA
 * (no register round trip, no conversion); products on v_mfma_f32_32x32x16_bf16, fp32 accumulate, fp32 bias / residual / gate
 * arithmetic.  Outputs:
 *   LINEAR   out = bf16 (out_bf16 != 0; the next convolution's operand) or fp32 rows, `out_ld` / `out_coff` in elements of that type
 *   GRU_ZR   z -> aux_z BF16 [M][Ch];  r * h (h read from its bf16 copy h_b16) -> aux_rh BF16 [M][Ch] (the q convolution's operand)
 *   GRU_Q    h fp32 updated in place (the recurrent state keeps full precision; z read from aux_z bf16) and, when h_b16 != NULL,
 *            its bf16 rounding -> h_b16[p * h_b16_ld + co] (the next convolutions' operand)
 * `residual`: LINEAR — fp32 rows added after relu / scale (pfk_conv_desc); GRU epilogues — BF16 rows [M][cout] added to the gate
 * pre-activation (the loop-invariant context term: at batch 8 these launches are bound by the HBM bytes of their epilogues, and the
 * term is a convolution output that autocast would hold in 16 bits anyway).
 * kh * kw <= 32.  No workspace, no stream-K: tile grids only.
 * Alignment: sources / weight 16 bytes.  The GRU epilogues move their bf16 operands and results as 16-byte row pieces: Ch % 8 == 0,
 * h_b16 / aux_z / aux_rh / the bf16 `residual` 16-byte aligned with row strides that are multiples of 8 elements (h: 16 bytes, h_ld % 4).
 * LINEAR: `out` 8 bytes (bf16) / 16 bytes (fp32), out_ld / out_coff multiples of 4; bf16 rows without a residual whose pieces are 16-byte
 * aligned (out 16 bytes, out_ld and out_coff multiples of 8) are stored with 16-byte accesses. */
typedef struct {
  const void* ptr;   /* bf16 rows */
  int ld;            /* row stride in elements (multiple of 8) */
  int channels;      /* channels read from each row (multiple of 8) */
} pfk_conv_src_b16;

typedef struct {
  pfk_conv_src_b16 src[3];
  int num_src;
  int B, H, W;
  int kh, kw;
  const void* weight;    /* bf16 [cout][ktot] */
  const float* bias;     /* fp32 [cout] or NULL */
  int cout;
  int epilogue;          /* enum pfk_epilogue */
  int relu;
  float scale;
  void* out;             /* LINEAR */
  int out_ld, out_coff;
  int out_bf16;          /* LINEAR: 1 = `out` holds bf16 elements, 0 = fp32 */
  float* h;              /* GRU_Q (read + write): fp32 hidden state */
  int h_ld;
  void* h_b16;           /* GRU_ZR (read, required): bf16 copy of the hidden state; GRU_Q (write, optional): bf16 copy of the new one */
  int h_b16_ld;
  void* aux_z;           /* bf16 [M][Ch]: written by GRU_ZR, read by GRU_Q */
  void* aux_rh;          /* bf16 [M][Ch] */
  const void* residual;  /* LINEAR: fp32 [M][cout] rows; GRU_ZR / GRU_Q: bf16 [M][cout] rows (see above) */
  int residual_ld;       /* in elements of that type */
  int stride;
  int relu_after_residual;
  int residual_bf16;     /* LINEAR: 1 = `residual` holds bf16 rows (cout % 4 == 0), 0 = fp32 */
  /* batched GEMM — `batches` > 1 independent problems of one shape in one grid (LINEAR, one source, 1 x 1, B == 1: M = H*W rows
   * each): problem b reads src[0].ptr + b*src_batch_stride, weight + b*weight_batch_stride, residual + b*residual_batch_stride and
   * writes out + b*out_batch_stride (strides in ELEMENTS of the respective type).  GMA's per-pair `attn @ v`
   * (gma/gma_utils.py:100-113) on a bf16 attention map: A = attn[b] [N][N], B = v[b]^T [C][N]. */
  int batches;
  long long src_batch_stride, weight_batch_stride, out_batch_stride, residual_batch_stride;
} pfk_conv_b16_desc;
int pfk_conv_ktot_b16(const pfk_conv_b16_desc* d);
int pfk_conv2d_b16(const pfk_conv_b16_desc* d, pfk_stream_t stream);
/* pfk_conv2d_gelu_b16 (ABI 7): K8b's LINEAR epilogue with the exact GELU where relu would be applied — sea_raft/layer.py:60-62,74-75
 * (pwconv1 + nn.GELU()) on bf16 operands: v = (acc+bias) ; v = 0.5*v*(1 + erf(v/sqrt(2))) ; v *= scale ; [v = residual + v] ; out.
 * d->epilogue must be PFK_EPI_LINEAR_GELU and d->relu 0 (PFK_ERR_BAD_ARG otherwise); everything else as pfk_conv2d_b16's LINEAR
 * (bf16 or fp32 out, fp32 bias, optional residual; no batched GEMM).  pfk_conv2d_b16 itself keeps refusing PFK_EPI_LINEAR_GELU. */
int pfk_conv2d_gelu_b16(const pfk_conv_b16_desc* d, pfk_stream_t stream);
int pfk_debug_set_b16(int cfg);            /* K8b tile configuration: 0 = heuristic, 1..5 (pfk_gemm_b16.hip::launch_b16) */

/* ---- small direct kernels ------------------------------------------------------------------- */
/* k x k conv on a 2-channel map (the flow), relu optional: out[p*out_ld + out_coff + co].
 * in [M][in_ld] (channels 0,1 used); weight packed [k*k][2][cout]; bias [cout]. */
int pfk_conv_cin2_f32(const float* in, int in_ld, const float* weight, const float* bias,
                      float* out, int out_ld, int out_coff, int B, int H, int W, int k, int cout,
                      int relu, pfk_stream_t stream);

int pfk_debug_set_cin2_valu(int on);      /* 0 = by size; 1 = the tiled VALU kernel everywhere; 2 = the MFMA kernel (k = 7, cout 64 / 128) at every size */

/* same with a bf16 output (ABI 7; k = 3, 5 or 7): `out_bf16` holds bf16 elements, out_ld / out_coff in elements — the A operand of
 * convf2 on the K8b path (pfk_conv2d_b16) */
int pfk_conv_cin2_b16(const float* in, int in_ld, const float* weight, const float* bias,
                      void* out_bf16, int out_ld, int out_coff, int B, int H, int W, int k, int cout,
                      int relu, pfk_stream_t stream);

/* FlowHead.conv2 (3x3, cin -> 2) fused with the coordinate update of the RAFT loop:
 *   delta = conv(in) + bias ; coords1 += delta ; flow = coords1 - coords0
 * in [M][in_ld]; weight packed [9][2][cin]; coords0/coords1 [B][2][h][w] (NCHW, updated in place);
 * delta_out [B][2][h][w] (may be NULL); flow_out written as 2 channels at
 * flow_out[p*flow_ld + 0..1] (may be NULL). */
int pfk_flow_delta_f32(const float* in, int in_ld, int cin, const float* weight,
                       const float* bias, const float* coords0, float* coords1, float* delta_out,
                       float* flow_out, int flow_ld, int B, int H, int W, pfk_stream_t stream);

/* same with a bf16 input (ABI 7; the flow head's hidden activation as pfk_conv2d_b16 writes it: in_ld in elements, 8-byte aligned
 * rows) and an optional second, bf16 copy of the flow at flow_out_b16[p*flow_b16_ld + 0..1] (the 16-bit twin of the hx buffer that
 * the next iteration's convolutions read); weight / bias / coordinates fp32, fp32 accumulation. */
int pfk_flow_delta_b16(const void* in_bf16, int in_ld, int cin, const float* weight,
                       const float* bias, const float* coords0, float* coords1, float* delta_out,
                       float* flow_out, int flow_ld, void* flow_out_b16, int flow_b16_ld, int B, int H, int W, pfk_stream_t stream);

/* flow = coords1 - coords0 written pixel-major (2 channels) — loop prologue / drop-in mode. */
int pfk_flow_from_coords_f32(const float* coords0, const float* coords1, float* flow_out,
                             int flow_ld, int B, int H, int W, pfk_stream_t stream);

/* RAFT.upsample_flow: softmax over the 9 mask taps, convex combination of the 3x3 neighbourhood
 * of 8*flow, pixel-shuffle to 8x resolution.
 * flow [B][2][h][w] NCHW; mask pixel-major [M][mask_ld] with channel c = k*64 + sy*8 + sx
 * (already multiplied by 0.25); out [B][2][8h][8w] NCHW. */
int pfk_convex_upsample_f32(const float* flow, const float* mask, int mask_ld, float* out,
                            int B, int H, int W, pfk_stream_t stream);
/* `upsample_flow(flow, mask, scale=2)` of the multi-scale families (ccmr/ccmr.py:128-139, ms_raft_plus/ms_raft_plus.py:133-144):
 * softmax over the 9 taps, convex combination of the zero-padded 3x3 neighbourhood of 2*flow, pixel-shuffle to 2x resolution.
 * flow NCHW [B][2][H][W] (flow_ld == 0) or pixel-major rows flow[p*flow_ld + 0..1] (flow_ld >= 2); mask pixel-major fp32 logits
 * [M][mask_ld], mask_ld >= 36, channel c = k*4 + sy*2 + sx (the update block's 0.25 already applied); out [B][2][2H][2W] NCHW.
 * No alignment is required beyond the elements' own: 8-byte aligned mask and out with an even mask_ld take 8-byte accesses,
 * anything else 4-byte ones, with the same bits.  PFK_ERR_BAD_ARG: a null pointer, a non-positive size, mask_ld < 36, flow_ld == 1
 * or negative; PFK_ERR_UNSUPPORTED: more pixels than a launch grid holds.  (Added within ABI 7: an addition only.) */
int pfk_convex_upsample2_f32(const float* flow, int flow_ld, const float* mask, int mask_ld, float* out,
                             int B, int H, int W, pfk_stream_t stream);
/* upflow8 (raft/utils.py:94-96, the mask-less upsampling of raft_small): out [B][2][8H][8W] = 8 * bilinear(coords1 - coords0,
 * size 8x, align_corners = True); coords NCHW [B][2][H][W].  Index / weight arithmetic as torch's upsample_bilinear2d. */
int pfk_upflow8_f32(const float* coords0, const float* coords1, float* out, int B, int H, int W, pfk_stream_t stream);

/* ---- fused mask head conv2 + softmax + convex upsampling (round 5) ------------------------------------------------------
 * raft/update.py:138-142,152 (`0.25 * mask[2](relu(mask[0](net)))`: the 1x1 convolution to 9*64 channels) followed by
 * raft/raft.py:112-123 (`upsample_flow`) in ONE kernel: the [M][576] mask is never written.  x [M = B*H*W][x_ld] = the mask head's
 * hidden activation (cin channels, cin % 32 == 0); weight_perm [640][cin] / bias_perm [640] = the 1x1 convolution's weight and bias
 * with their ROWS in the order [quarter q (4)][tile j (5)][column c (32)]: row q*160 + j*32 + c = original channel k*64 + s with tap
 * k = 2j + (c >> 4) and sub-pixel s = q*16 + (c & 15); the rows with k == 9 (tile 4, c >= 16) are ZERO (a block's nine taps of 16
 * sub-pixels are then one contiguous range of 160 rows; ptlflow_amd/packing.py::permute_mask_head).  scale = 0.25; flow_pm
 * pixel-major (flow_pm[p*flow_ld + 0..1]); out [B][2][8H][8W] NCHW.  Bit-identical to pfk_conv2d_f32 (scale 0.25) +
 * pfk_convex_upsample_pm_f32. */
int pfk_mask_upsample_f32(const float* x, int x_ld, int cin, const float* weight_perm, const float* bias_perm, float scale,
                          const float* flow_pm, int flow_ld, float* out, int B, int H, int W, pfk_stream_t stream);

/* K13b — the same on the K8b path (ABI 7): x bf16 [M][x_ld] (cin % 64 == 0, x_ld % 8 == 0), weight_perm bf16 [640][cin] in the same
 * row order, bias / flow / out fp32.  Every logit is rounded to bf16 where pfk_conv2d_b16 (bf16 out) would store it: bit-identical
 * to that launch + pfk_convex_upsample_pm_b16. */
int pfk_mask_upsample_b16(const void* x_bf16, int x_ld, int cin, const void* weight_perm_bf16, const float* bias_perm, float scale,
                          const float* flow_pm, int flow_ld, float* out, int B, int H, int W, pfk_stream_t stream);

/* same, with the flow read pixel-major (flow_pm[p*flow_ld + 0..1], e.g. the update engine's hx slice) */
int pfk_convex_upsample_pm_f32(const float* flow_pm, int flow_ld, const float* mask, int mask_ld,
                               float* out, int B, int H, int W, pfk_stream_t stream);

/* same with a bf16 mask (ABI 7): mask_bf16 [M][mask_ld] bf16 logits (mask_ld in elements, rows 8-byte aligned) as the K8b mask head
 * writes them — what `0.25 * self.mask(net)` is under the reference's reduced-precision switch; softmax and combination in fp32 */
int pfk_convex_upsample_pm_b16(const float* flow_pm, int flow_ld, const void* mask_bf16, int mask_ld, float* out,
                               int B, int H, int W, pfk_stream_t stream);

/* ---- SEA-RAFT refinement (additions of ABI 7) ------------------------------------------------------------------------------
 * pfk_dwconv_layernorm_f32: ConvNextBlock.dwconv followed by .norm (sea_raft/layer.py:54-58, :71-75): a depthwise k x k "same"
 * convolution (zero padding k/2, bias) followed by a LayerNorm over the C channels of each pixel (biased variance, `eps`, weight
 * and bias).  in: pixel-major rows in[p*in_ld + c], p = (b*H + y)*W + x, C channels (C % 4 == 0, 4 <= C <= 512; in 16-byte
 * aligned, in_ld % 4 == 0 — e.g. the update engine's [net | context | motion | flow] rows); dw_weight [C][k*k] (tap ky*k + kx),
 * dw_bias [C] or NULL, ln_weight / ln_bias [C]; out [M][out_ld] (out_ld >= C; must not overlap the input rows).  k odd, 1 <= k <= 7.  One launch, one read of every input row from HBM (halo tiles staged in LDS), the
 * statistics finished in the kernel. */
int pfk_dwconv_layernorm_f32(const float* in, int in_ld, const float* dw_weight, const float* dw_bias, const float* ln_weight,
                             const float* ln_bias, float eps, float* out, int out_ld, int B, int H, int W, int C, int k,
                             pfk_stream_t stream);

/* pfk_dwconv_layernorm_b16: the same on bf16 rows (ABI 7): in_bf16[p*in_ld + c] -> out_bf16[p*out_ld + c]; dw_weight / dw_bias /
 * ln_weight / ln_bias fp32 as above.  fp32 accumulation, LayerNorm statistics in fp32 (mean, then the biased variance about it),
 * one rounding to bf16 at the store.  C % 8 == 0, 8 <= C <= 512, k odd <= 7; in / out 16-byte aligned, in_ld % 8 == 0,
 * out_ld % 8 == 0 (e.g. the update engine's bf16 [net | context | motion | flow] rows); out must not overlap the input rows.  No
 * workspace; one HBM read of every input row. */
int pfk_dwconv_layernorm_b16(const void* in_bf16, int in_ld, const float* dw_weight, const float* dw_bias, const float* ln_weight,
                             const float* ln_bias, float eps, void* out_bf16, int out_ld, int B, int H, int W, int C, int k,
                             pfk_stream_t stream);

/* ---- training the ConvNeXt block (K12d; additions, ABI 7) ---------------------------------------------------------------------
 * All fp32, pixel-major rows [M = B*H*W][ld] of which only the C real columns are read or written (ld may be larger), C % 4 == 0,
 * 4 <= C <= 512, rows 16-byte aligned with ld % 4 == 0, k odd <= 7.  Deterministic: no atomics, sums over pixels in an order that
 * depends on the shape only.  Arguments are validated before the device is touched: PFK_ERR_BAD_ARG / PFK_ERR_ALIGNMENT.
 *
 * pfk_dwconv_layernorm_train_f32: pfk_dwconv_layernorm_f32 with `out` bit-identical to that entry on the same inputs, and in
 * addition xhat[p*xhat_ld + c] = (u - mean) * rstd, the normalised value before weight and bias, and rstd[p].  No output may
 * overlap the input rows or another output. */
int pfk_dwconv_layernorm_train_f32(const float* in, int in_ld, const float* dw_weight, const float* dw_bias, const float* ln_weight,
                                   const float* ln_bias, float eps, float* out, int out_ld, float* xhat, int xhat_ld, float* rstd,
                                   int B, int H, int W, int C, int k, pfk_stream_t stream);

/* pfk_layernorm_bwd_f32: backward of the LayerNorm from what the train forward saved.  With g = dy * ln_weight per pixel:
 *   du[p][c] = rstd[p] * (g[c] - mean_c(g) - xhat[p][c] * mean_c(g * xhat)),  dgamma[c] = sum_p dy[p][c] * xhat[p][c],
 *   dbeta[c] = sum_p dy[p][c].
 * du must not overlap dy or xhat.  workspace: pfk_layernorm_bwd_workspace_bytes(M, C) bytes, 16-byte aligned (per-block partial
 * column sums, reduced in a fixed order). */
long long pfk_layernorm_bwd_workspace_bytes(long long M, int C);
int pfk_layernorm_bwd_f32(const float* xhat, int xhat_ld, const float* rstd, const float* ln_weight, const float* dy, int dy_ld,
                          float* du, int du_ld, float* dgamma, float* dbeta, void* workspace, long long workspace_bytes, long long M,
                          int C, pfk_stream_t stream);

/* pfk_dwconv_bwd_f32: backward of the depthwise k x k "same" convolution (R = k/2): `in` the forward's input rows, `du` the gradient
 * of its output, dw_weight [C][k*k]:
 *   dx[p][c]            = sum_{ky,kx} dw_weight[c][ky*k+kx] * du[(y-ky+R, x-kx+R)][c]    (zero outside the image, never across images)
 *   dweight[c][ky*k+kx] = sum_p du[p][c] * in[(y+ky-R, x+kx-R)][c]
 *   dbias[c]            = sum_p du[p][c]                                                  (dbias may be NULL)
 * dx must not overlap du or in.  workspace: pfk_dwconv_bwd_workspace_bytes(B, H, W, C, k) bytes, 16-byte aligned: one partial
 * [C][k*k + 1] per block slice of tiles (at most 64), summed in slice order. */
long long pfk_dwconv_bwd_workspace_bytes(int B, int H, int W, int C, int k);
int pfk_dwconv_bwd_f32(const float* in, int in_ld, const float* du, int du_ld, const float* dw_weight, float* dx, int dx_ld,
                       float* dweight, float* dbias, void* workspace, long long workspace_bytes, int B, int H, int W, int C, int k,
                       pfk_stream_t stream);

/* pfk_gelu_f32 / pfk_gelu_bwd_f32: nn.GELU() (approximate='none') on rows, PFK_EPI_LINEAR_GELU's formula, and its derivative:
 *   y = 0.5 x (1 + erf(x / sqrt 2)),   dx = dy (0.5 (1 + erf(x / sqrt 2)) + x exp(-x^2 / 2) / sqrt(2 pi))
 * (large |x|: 0 or dy, never NaN).  Any C % 4 == 0, C >= 4; out of place. */
int pfk_gelu_f32(const float* x, long long x_ld, float* y, long long y_ld, long long M, int C, pfk_stream_t stream);
int pfk_gelu_bwd_f32(const float* x, long long x_ld, const float* dy, long long dy_ld, float* dx, long long dx_ld, long long M, int C,
                     pfk_stream_t stream);

/* ---- training the ConvNeXt block on bf16 rows (K12f; additions, ABI 7) ----------------------------------------------------------
 * The five entries above with bf16 activations and activation gradients: what the block saves and moves between its bf16 GEMMs
 * (pfk_conv2d_b16 / pfk_conv_wgrad_unpacked_b16) at half the bytes.  Every `*_bf16` pointer is bf16 pixel-major rows [M][ld] of
 * which only the C real columns are read or written: C % 8 == 0, 8 <= C <= 512, 16-byte aligned with ld % 8 == 0 (ld in elements),
 * k odd <= 7.  Parameters, parameter gradients, rstd and the workspaces are fp32.  A bf16 value is widened exactly when it is read,
 * all arithmetic and all accumulation is fp32 in the order of the fp32 entry, and each bf16 output is rounded once (to nearest even)
 * at its store.  Deterministic and validated as the fp32 entries are.
 *
 * pfk_dwconv_layernorm_train_b16: pfk_dwconv_layernorm_b16 with `out_bf16` bit-identical to that entry on the same inputs, and in
 * addition xhat_bf16[p*xhat_ld + c] = bf16((u - mean) * rstd) — the fp32 normalised value rounded once, not derived from the rounded
 * output — and the fp32 rstd[p] (4-byte aligned, [M]).  No output may overlap the input rows or another output. */
int pfk_dwconv_layernorm_train_b16(const void* in_bf16, int in_ld, const float* dw_weight, const float* dw_bias, const float* ln_weight,
                                   const float* ln_bias, float eps, void* out_bf16, int out_ld, void* xhat_bf16, int xhat_ld, float* rstd,
                                   int B, int H, int W, int C, int k, pfk_stream_t stream);

/* pfk_layernorm_bwd_b16: pfk_layernorm_bwd_f32's formulas on bf16 xhat / dy -> bf16 du; rstd, ln_weight, dgamma, dbeta fp32 (the
 * column sums run over the widened dy and xhat in fp32 and are never rounded to bf16).  du must not overlap dy or xhat.  workspace:
 * pfk_layernorm_bwd_workspace_bytes(M, C) bytes, 16-byte aligned. */
int pfk_layernorm_bwd_b16(const void* xhat_bf16, int xhat_ld, const float* rstd, const float* ln_weight, const void* dy_bf16, int dy_ld,
                          void* du_bf16, int du_ld, float* dgamma, float* dbeta, void* workspace, long long workspace_bytes, long long M,
                          int C, pfk_stream_t stream);

/* pfk_dwconv_bwd_b16: pfk_dwconv_bwd_f32's formulas (never across images) on bf16 in / du -> bf16 dx; dw_weight, dweight [C][k*k] and
 * dbias [C] (may be NULL) fp32.  dx must not overlap du or in.  workspace: pfk_dwconv_bwd_workspace_bytes(B, H, W, C, k) bytes,
 * 16-byte aligned. */
int pfk_dwconv_bwd_b16(const void* in_bf16, int in_ld, const void* du_bf16, int du_ld, const float* dw_weight, void* dx_bf16, int dx_ld,
                       float* dweight, float* dbias, void* workspace, long long workspace_bytes, int B, int H, int W, int C, int k,
                       pfk_stream_t stream);

/* pfk_gelu_b16 / pfk_gelu_bwd_b16: pfk_gelu_f32's formulas evaluated in fp32 on float(x); x, y, dy, dx bf16 rows (large |x|: 0 or dy,
 * never NaN).  Any C % 8 == 0, C >= 8; out of place. */
int pfk_gelu_b16(const void* x_bf16, long long x_ld, void* y_bf16, long long y_ld, long long M, int C, pfk_stream_t stream);
int pfk_gelu_bwd_b16(const void* x_bf16, long long x_ld, const void* dy_bf16, long long dy_ld, void* dx_bf16, long long dx_ld, long long M,
                     int C, pfk_stream_t stream);

/* pfk_convex_upsample_info_pm_f32: SEARAFT.upsample_data (sea_raft/sea_raft.py:147-163).  flow_pm [M][flow_ld] (channels 0..1),
 * info_pm [M][info_ld] (channels 0..n-1, 1 <= n <= 8), mask [M][mask_ld] fp32 logits with channel c = k*64 + sy*8 + sx, already
 * multiplied by 0.25 (16-byte aligned rows, mask_ld % 4 == 0, mask_ld >= 576).  Softmax over the nine taps; convex combination of
 * the zero-padded 3x3 neighbourhood of 8*flow -> flow_out [B][2][8H][8W] and of info (no factor) -> info_out [B][n][8H][8W]
 * (both NCHW, contiguous, 16-byte aligned).  flow_out is bit-identical to pfk_convex_upsample_pm_f32 on the same flow and mask. */
int pfk_convex_upsample_info_pm_f32(const float* flow_pm, int flow_ld, const float* info_pm, int info_ld, int n_info,
                                    const float* mask, int mask_ld, float* flow_out, float* info_out, int B, int H, int W,
                                    pfk_stream_t stream);
/* same with bf16 mask logits (ABI 7): mask_bf16 [M][mask_ld] in the plain channel order, already x 0.25, 16-byte aligned rows,
 * mask_ld % 8 == 0; flow / info rows and both outputs fp32 as above.  flow_out is bit-identical to pfk_convex_upsample_pm_b16 on
 * the same flow and mask. */
int pfk_convex_upsample_info_pm_b16(const float* flow_pm, int flow_ld, const float* info_pm, int info_ld, int n_info,
                                    const void* mask_bf16, int mask_ld, float* flow_out, float* info_out, int B, int H, int W,
                                    pfk_stream_t stream);

/* ---- on-demand correlation behind the reference's alt_cuda_corr ABI --------------------------------
 * replaces corr_cuda_forward (ptlflow/utils/external/alt_cuda_corr/correlation_kernel.cu:258-285; pybind
 * `alt_cuda_corr.forward`, correlation.cpp:23-37, called from AlternateCorrBlock, raft/corr.py:76-101):
 * fmap1 [B][H1][W1][C], fmap2 [B][H2][W2][C] (NHWC fp32 contiguous), coords [B][H1][W1][2] (x, y) ->
 * out [B][(2r+1)^2][H1][W1], cell = oy + (2r+1)*ox, UNSCALED (the caller divides by sqrt(C)).
 * `workspace`: pfk_altcorr_workspace_bytes(B, H1, W1) bytes of device memory (4-byte aligned, no initialisation needed), or NULL.
 * With it the launch counts the 8x4-pixel patches whose windows share a bounding box small enough for the window-sharing MFMA
 * kernel and runs that kernel only when at least 5/8 of them qualify; otherwise (noise-like coordinate fields) every pixel
 * takes the per-pixel kernel.  NULL: the decision is per patch only. */
long long pfk_altcorr_workspace_bytes(int B, int H1, int W1);
int pfk_altcorr_forward_f32(const float* fmap1, const float* fmap2, const float* coords, float* out,
                            int B, int H1, int W1, int H2, int W2, int C, int radius,
                            void* workspace, pfk_stream_t stream);

/* The same with bf16 feature maps (NHWC bf16 contiguous; coords and out fp32): the maps are widened exactly, products and
 * accumulation are fp32 — the on-demand counterpart of the bf16 volume for bf16 / autocast callers, half the
 * gather bytes of an L2-bound kernel.  The reference's extension is float-only (correlation_kernel.cu:275) and its callers
 * up-cast half inputs (raft/corr.py:90-96); IterativeCorrBlock under autocast (ptlflow/utils/correlation.py:539-615) is the oracle. */
int pfk_altcorr_forward_bf16(const void* fmap1_bf16, const void* fmap2_bf16, const float* coords, float* out,
                             int B, int H1, int W1, int H2, int W2, int C, int radius, void* workspace, pfk_stream_t stream);

/* backward of the above w.r.t. the feature maps: corr_cuda_backward (correlation_kernel.cu:288-324, pybind
 * `alt_cuda_corr.backward`).  corr_grad [B][(2r+1)^2][H1][W1] -> fmap1_grad [B][H1][W1][C] (overwritten),
 * fmap2_grad [B][H2][W2][C] (zeroed here, then accumulated with fp32 atomics like the reference). */
int pfk_altcorr_backward_f32(const float* fmap1, const float* fmap2, const float* coords,
                             const float* corr_grad, float* fmap1_grad, float* fmap2_grad, int B, int H1,
                             int W1, int H2, int W2, int C, int radius, pfk_stream_t stream);

/* ---- weight gradient of the convolution above (torch.autograd of every nn.Conv2d in raft/update.py) ---
 * dw_packed[co][k(s,tap,c)] = sum_p dy[p][co] * src_s[p + tap][c]   — the packed [cout][ktot] layout of pfk_conv2d_f32's weight.
 * `d` describes the forward convolution (sources, B, H, W, kh, kw, cout, stride; weight/out/epilogue fields ignored);
 * dy [B*Ho*Wo][dy_ld] is the gradient w.r.t. the convolution output (Ho = (H-1)/stride + 1; stride 0 or 1: Ho = H), cout % 4 == 0;
 * with a stride the product reads src_s at (yo*stride + dy, xo*stride + dx) — no zero-upsampled gradient is needed.  The reduction runs over pixels, cut
 * into slices whose partial results go through `workspace` (pfk_conv_wgrad_workspace_bytes(d) bytes, 16-byte aligned; may
 * be NULL when that is 0) and are added in a fixed order: deterministic, no atomics.  with_bias != 0 appends 32 columns to
 * every row of dw_packed ([cout][ktot + 32]); column ktot is the bias gradient sum_p dy[p][co] (computed as one more chunk
 * whose A operand is a column of ones), the other 31 are zero.  (The data gradient needs no entry
 * point of its own: it is pfk_conv2d_f32 of dy with the spatially flipped, transposed weight.) */
long long pfk_conv_wgrad_workspace_bytes(const pfk_conv_desc* d, int with_bias);
int pfk_conv_wgrad_f32(const pfk_conv_desc* d, const float* dy, int dy_ld, float* dw_packed, int with_bias, void* workspace,
                       long long workspace_bytes, pfk_stream_t stream);

/* The same weight gradient delivered in PyTorch's layouts (what autograd accumulates): dw [cout_real][cin][kh][kw] with cin =
 * sum of real_channels[s] (the sources' real channels in order; real_channels[s] <= src[s].channels, the rest being the
 * buffers' zero padding) and db [cout_real] (NULL: no bias gradient).  d->cout is dy's channel count (a multiple of 4, >=
 * cout_real).  The slice reduction writes them directly — no packed intermediate, no un-packing copies.  accumulate != 0:
 * dw / db += the gradient (the recurrent iterations of a training step add into one buffer per parameter instead of leaving
 * eleven additions per parameter to the autograd engine); 0: overwrite.  workspace:
 * pfk_conv_wgrad_unpacked_workspace_bytes(d, db != NULL) bytes, always required. */
long long pfk_conv_wgrad_unpacked_workspace_bytes(const pfk_conv_desc* d, int with_bias);
int pfk_conv_wgrad_unpacked_f32(const pfk_conv_desc* d, const int* real_channels, const float* dy, int dy_ld, int cout_real,
                                float* dw, float* db, int accumulate, void* workspace, long long workspace_bytes, pfk_stream_t stream);

/* K12b — the same weight gradient on bf16 operands (v_mfma_f32_32x32x16_bf16, fp32 accumulation): the training form of
 * pfk_conv2d_b16.  `d` describes the forward convolution (src / num_src / B / H / W / kh / kw / cout / stride; everything else is
 * ignored): bf16 pixel-major sources as pfk_conv_src_b16 (ld and channels multiples of 8, 16-byte aligned); dy is bf16
 * [B*H*W][dy_ld], dy_ld % 8 == 0, d->cout (dy's channel count) % 8 == 0, 8 <= d->cout.  Stride 1 only (d->stride 0 or 1) and
 * kernels 1x1, 3x3, 1x5, 5x1: anything else is PFK_ERR_BAD_ARG, as are a NULL dw / workspace, a workspace that is too small and
 * a row stride that is no multiple of 8.  Outputs are FP32, in PyTorch's layouts, exactly as pfk_conv_wgrad_unpacked_f32's:
 * dw [cout_real][sum real_channels][kh][kw], db [cout_real] or NULL; `accumulate` adds into them.  The pixel range is cut into
 * slices that are added in a fixed order (deterministic, no atomics) through `workspace`
 * (pfk_conv_wgrad_unpacked_b16_workspace_bytes(d, db != NULL) bytes, 16-byte aligned, always required).  Byte offsets >= 2^31
 * are refused (PFK_ERR_UNSUPPORTED). */
long long pfk_conv_wgrad_unpacked_b16_workspace_bytes(const pfk_conv_b16_desc* d, int with_bias);
int pfk_conv_wgrad_unpacked_b16(const pfk_conv_b16_desc* d, const int* real_channels, const void* dy, int dy_ld, int cout_real,
                                float* dw, float* db, int accumulate, void* workspace, long long workspace_bytes, pfk_stream_t stream);
int pfk_debug_set_wgrad_b16(int splits);   /* pixel slices of pfk_conv_wgrad_unpacked_b16: 0 = by occupancy, n > 0 = n slices (at most one per K-step, at most 64) */

/* Gate arithmetic of one ConvGRU / SepConvGRU pass for the training path (raft/update.py:24-32, 58-73), pixel-major
 * [M][C] tensors, C % 4 == 0; z, r, rh, q, h_new, da_q, dh are contiguous [M][C], a_zr / da_zr contiguous [M][2C]
 * (z half first), h / dh_new have their own row stride.
 *   gates_zr:     z = sigmoid(a_zr[:, :C]), r = sigmoid(a_zr[:, C:]), rh = r * h
 *   gates_q:      q = tanh(a_q), h_new = (1 - z) * h + z * q
 *   backward_q:   da_q = dh_new * z * (1 - q^2);  da_zr[:, :C] = dh_new * (q - h) * z * (1 - z);  dh = dh_new * (1 - z)
 *   backward_zr:  da_zr[:, C:] = d_rh * h * r * (1 - r);  dh += d_rh * r */
int pfk_gru_gates_zr_f32(const float* a_zr, const float* h, int h_ld, float* z, float* r, float* rh, long long M, int C,
                         pfk_stream_t stream);
int pfk_gru_gates_q_f32(const float* a_q, const float* z, const float* h, int h_ld, float* q, float* h_new, long long M, int C,
                        pfk_stream_t stream);
int pfk_gru_backward_q_f32(const float* dh_new, int dh_new_ld, const float* z, const float* q, const float* h, int h_ld,
                           float* da_q, float* da_zr, float* dh, long long M, int C, pfk_stream_t stream);
int pfk_gru_backward_zr_f32(const float* d_rh, const float* h, int h_ld, const float* r, float* da_zr, float* dh, long long M,
                            int C, pfk_stream_t stream);

/* ---- warm start (second half) -------------------------------------------------------------------
 * forward_interpolate (ptlflow/utils/external/raft.py:155-185, batched by utils/utils.py:454-478): flow [B][2][H][W] ->
 * out [B][2][H][W]: every grid point takes the flow of the nearest forward-projected pixel that lands strictly inside the
 * image (float64 distances, exact ties to the lowest source index; all-invalid -> 0).  Replaces the reference's per-sample
 * host round trip through scipy.interpolate.griddata. */
int pfk_forward_interpolate_f32(const float* flow, float* out, int B, int H, int W, pfk_stream_t stream);

/* ---- encoder pieces (ptlflow/models/raft/extractor.py:122-194 BasicEncoder) -----------------
 * The residual blocks' 3x3 / 1x1 convolutions (stride 1 and 2) are pfk_conv2d_f32 / pfk_conv2d_bf16s with `stride`
 * and `relu_after_residual`; eval-mode BatchNorm is folded into their weights by the caller.  What is left:
 *
 * stem = Conv2d(3, cout, 7, stride=2, padding=3) (extractor.py:146) read from the NCHW image:
 * img [B][3][H][W]; weight packed [49][3][cout] (tap ky*7+kx major); out pixel-major [B*Ho*Wo][out_ld], Ho=(H-1)/2+1. */
int pfk_conv_stem_f32(const float* img, const float* weight, const float* bias, float* out, int out_ld, int B,
                      int H, int W, int cout, int relu, pfk_stream_t stream);

/* same with a bf16 output (ABI 7; cout = 32 or 64 only — the MFMA kernel): what the K8b convolutions (pfk_conv2d_b16) read next */
int pfk_conv_stem_b16(const float* img, const float* weight, const float* bias, void* out_bf16, int out_ld, int B,
                      int H, int W, int cout, int relu, pfk_stream_t stream);
int pfk_debug_set_stem_valu(int on);       /* 1 = pfk_conv_stem_f32 always takes the VALU kernel (A/B timing) */
/* The same stem for ONE or TWO 3-channel images summed into one output (sea_raft/extractor.py:35-37: ResNetFPN's
 * Conv2d(input_dim, 64, 7, stride=2, padding=3) with input_dim 3 (`fnet`) or 6 (`cnet`, on cat([image1, image2], 1))):
 * img_a, img_b NCHW 3-channel planes, image n of each at `img + n * bstride` floats (bstride >= 3*H*W: 6*H*W for the two halves
 * of a [B][6][H][W] tensor, img_b = img_a + 3*H*W); img_b may be NULL, then cin must be 3, else cin must be 6.  weight packed
 * [49][cin][cout] (channels 0..2 of a tap are img_a's, 3..5 img_b's), 16-byte aligned.  cout must be 64 (PFK_ERR_UNSUPPORTED
 * otherwise).  Rows of `cout` values at out_ld; nothing beyond column cout is written.  fp32 matrix cores, fp32 accumulation. */
int pfk_conv_stem2_f32(const float* img_a, long long bstride_a, const float* img_b, long long bstride_b, const float* weight,
                       const float* bias, float* out, int out_ld, int B, int H, int W, int cin, int cout, int relu, pfk_stream_t stream);
int pfk_conv_stem2_b16(const float* img_a, long long bstride_a, const float* img_b, long long bstride_b, const float* weight,
                       const float* bias, void* out_bf16, int out_ld, int B, int H, int W, int cin, int cout, int relu,
                       pfk_stream_t stream);

/* InstanceNorm2d statistics (extractor.py:136-140; affine=False, biased variance, eps inside the sqrt) over
 * pixel-major x[B*HW][ld], channels [0, C): mean[b*C+c], rstd[b*C+c].  One pass over x, deterministic chunked reduction of sum(x) and
 * sum(x*x) in double (var = E[x^2] - mean^2 evaluated in double; results rounded to fp32); needs pfk_instnorm_workspace_bytes(B, C) bytes of 32-byte-aligned device scratch.
 * Training-mode batch norm statistics are the same call with B = 1 and HW = every pixel of the batch. */
long long pfk_instnorm_workspace_bytes(int B, int C);
int pfk_instnorm_stats_f32(const float* x, int ld, int B, int HW, int C, float eps, float* mean, float* rstd,
                           void* workspace, long long workspace_bytes, pfk_stream_t stream);

/* out = relu?((x - mean) * rstd) ; if residual: out = relu?(residual + out)   — norm + relu (+ the ResidualBlock's
 * `relu(x + y)`, extractor.py:53-61) in one pass.  out may alias x. */
int pfk_norm_apply_f32(const float* x, int x_ld, const float* mean, const float* rstd, const float* residual,
                       int residual_ld, float* out, int out_ld, int B, int HW, int C, int relu,
                       int relu_after_residual, pfk_stream_t stream);

/* The same with a residual that is a raw convolution output with statistics of its own (res_mean / res_rstd, [B][C]), normalised
 * in flight: out = relu?((x - mean) * rstd); out = relu_after?(res_relu?((residual - res_mean) * res_rstd) + out).  The bits are
 * those of pfk_norm_apply_f32 on the residual (relu = res_relu) followed by pfk_norm_apply_f32 with that result as the residual.
 * Everything is required (PFK_ERR_BAD_ARG for a null pointer); out may alias x. */
int pfk_norm_apply_res_f32(const float* x, int x_ld, const float* mean, const float* rstd, const float* residual, int residual_ld,
                           const float* res_mean, const float* res_rstd, int res_relu, float* out, int out_ld, int B, int HW, int C,
                           int relu, int relu_after_residual, pfk_stream_t stream);

/* same with bf16 residual rows and a bf16 output (ABI 7; ld in elements, 8-byte aligned rows).  x = the convolution output the
 * statistics were taken from: fp32 rows (x_bf16 = 0), or bf16 rows (x_bf16 = 1; `out_bf16` may be `x` itself: in place) — what
 * F.instance_norm reads under the reference's autocast switch, where the convolution in front of it returns a 16-bit tensor
 * (the arithmetic is fp32 either way: instance_norm is on autocast's fp32 list). */
int pfk_norm_apply_b16(const void* x, int x_bf16, int x_ld, const float* mean, const float* rstd, const void* residual_bf16,
                       int residual_ld, void* out_bf16, int out_ld, int B, int HW, int C, int relu,
                       int relu_after_residual, pfk_stream_t stream);
/* the statistics of bf16 rows (pfk_instnorm_stats_f32 otherwise: one pass, double partial sums, deterministic) */
int pfk_instnorm_stats_b16(const void* x_bf16, int ld, int B, int HW, int C, float eps, float* mean, float* rstd,
                           void* workspace, long long workspace_bytes, pfk_stream_t stream);

/* In-place softmax over each row of x [rows][ld] (cols entries used) — GMA's attention map (gma/gma_utils.py:75-76:
 * `sim.softmax(dim=-1)`, once per forward; the similarity itself is pfk_corr_volume_f32 of the q / k maps). */
int pfk_softmax_rows_f32(float* x, long long rows, int cols, long long ld, pfk_stream_t stream);

/* ---- training of GMA's attention (K12c, ABI 7 additions) ----------------------------------------------------------
 * Backward of pfk_softmax_rows_f32: p fp32 [rows][ld_p] (the softmax OUTPUT, cols entries used), dp [rows][ld_dp] fp32 or bf16 ->
 *   ds[r][j] = p[r][j] * (dp[r][j] - sum_k dp[r][k] * p[r][k])    j < cols,      ds[r][j] = 0    cols <= j < ld_out
 * fp32 rows [rows][ld_out]: with ld_out % 4 == 0 a legal dC operand of pfk_corr_volume_bwd_f32.  One block per row, the row sum
 * in fp32 in a fixed order (deterministic).  _f32: ds may be dp itself (then ld_out == ld_dp).  _bf16: dp_bf16 16-byte aligned,
 * ld_dp % 8 == 0 (PFK_ERR_ALIGNMENT otherwise).  Every ld >= cols (PFK_ERR_BAD_ARG otherwise).  Aliasing: only ds == dp exactly is
 * recognised (and refused unless fp32 with ld_out == ld_dp); ds overlapping dp in any other way, or overlapping p, is the caller's
 * error and is NOT detected. */
int pfk_softmax_rows_bwd_f32(const float* p, long long ld_p, const float* dp, long long ld_dp, float* ds, long long ld_out,
                             long long rows, int cols, pfk_stream_t stream);
int pfk_softmax_rows_bwd_bf16(const float* p, long long ld_p, const void* dp_bf16, long long ld_dp, float* ds, long long ld_out,
                              long long rows, int cols, pfk_stream_t stream);
/* Batched square map in [B][N][ld_in] fp32 -> outT [B][N][ld_out] with outT[b][j][i] = in[b][i][j] and, when `out` != NULL, in the
 * same pass out[b][i][j] = in[b][i][j] at the same row stride; columns [N, ld_out) of both are written as zero.  _f32 copies the
 * bits, _b16 rounds to bf16 (nearest even; outputs 16-byte aligned, ld_out % 8 == 0, PFK_ERR_ALIGNMENT otherwise).  64 x 64 tiles
 * through LDS: reads and writes are both along rows.  The operands of GMA's aggregate in training: out = the A operand of
 * attn @ v, outT = the A operand of dV = attn^T @ dAgg (pfk_conv2d_f32 / the batched pfk_conv2d_b16). */
int pfk_transpose_pack_f32(const float* in, long long ld_in, float* outT, float* out, long long ld_out, int B, int N,
                           pfk_stream_t stream);
int pfk_transpose_pack_b16(const float* in, long long ld_in, void* outT_bf16, void* out_bf16, long long ld_out, int B, int N,
                           pfk_stream_t stream);

/* ---- encoder backward (training, BASELINE config 5) ---------------------------------------------------------------
 * Backward of y = relu?((x - mean) * rstd) with per-(image, channel) statistics (pfk_instnorm_stats_f32): instance norm,
 * and batch norm in training mode when called with B = 1 and HW = all pixels of the batch (torch.autograd of
 * nn.InstanceNorm2d / nn.BatchNorm2d + relu in raft/extractor.py:51-59, 172-181):
 *   g = dy * (y > 0);  sum_g[b*C+c] = sum_p g;  sum_gxhat[b*C+c] = sum_p g * x_hat;  dx = rstd * (g - sum_g/HW - x_hat * sum_gxhat/HW)
 * sum_g / sum_gxhat may be NULL (kept in the workspace); for an affine batch norm they are d(beta) / d(gamma) when dy is the
 * gradient w.r.t. the un-affine'd output.  The two sums and the final subtraction are carried in double (the residual of a
 * mean-dominated gradient is otherwise lost to fp32 cancellation).  workspace: pfk_norm_bwd_workspace_bytes(B, C) bytes,
 * 32-byte aligned.  Deterministic. */
long long pfk_norm_bwd_workspace_bytes(int B, int C);
int pfk_norm_bwd_f32(const float* x, int x_ld, const float* dy, int dy_ld, const float* mean, const float* rstd, float* dx,
                     int dx_ld, float* sum_g, float* sum_gxhat, int B, int HW, int C, int relu, void* workspace,
                     long long workspace_bytes, pfk_stream_t stream);
/* Weight / bias gradient of the stem (pfk_conv_stem_f32): dy pixel-major [B*Ho*Wo][dy_ld] -> dw [49][3][cout] (the packed
 * layout of the forward's weight), db [cout] (may be NULL).  cout <= 64.  workspace: pfk_conv_stem_wgrad_workspace_bytes(). */
long long pfk_conv_stem_wgrad_workspace_bytes(void);
int pfk_conv_stem_wgrad_f32(const float* img, const float* dy, int dy_ld, float* dw, float* db, int B, int H, int W, int cout,
                            void* workspace, long long workspace_bytes, pfk_stream_t stream);

/* NCHW [B][C][H][W] -> pixel-major [B*H*W][ld] (+ channel offset) and back. */
int pfk_nchw_to_pm_f32(const float* in, float* out, int out_ld, int out_coff, int B, int C,
                       int H, int W, pfk_stream_t stream);
int pfk_pm_to_nchw_f32(const float* in, int in_ld, int in_coff, float* out, int B, int C, int H,
                       int W, pfk_stream_t stream);
/* pixel-major [B*N][in_ld] -> channel-major out[b][c][n] with row stride out_ld >= N (a K-contiguous "weight"
 * operand for pfk_conv2d_f32, e.g. GMA's value matrix V^T, gma_utils.py:103-105).  The pad columns [N, out_ld) of a row are not
 * written: they keep what the caller put there (zeros, where a consumer reads them). */
int pfk_pm_to_cm_f32(const float* in, int in_ld, float* out, int out_ld, int B, int C, int N,
                     pfk_stream_t stream);

/* ---- K14: CCMR's XCiT motion aggregator (ccmr/xcit.py, XCiT(128, depth 1, 8 heads, mlp_ratio 1, separate=True); additions, ABI 7) ----
 * fp32 pixel-major rows [M][ld] of which only the C real columns are read or written; rows 16-byte aligned, ld % 4 == 0 (ld in
 * floats, 64-bit: no 2 GB limit on a span).  Deterministic: no atomics, every sum in an order fixed by the shape.  Arguments are
 * validated before the device is touched: PFK_ERR_BAD_ARG / PFK_ERR_ALIGNMENT, PFK_ERR_UNSUPPORTED for a width the kernels are not
 * built for.  The dense layers between them are pfk_conv2d_f32 / pfk_conv2d_group_f32 launches.
 *
 * pfk_layernorm_rows_f32: out[p][c] = (in[p][c] - mean_p) * rstd_p [* weight[c]] [+ bias[c]], mean over the C channels of the row,
 * then the biased variance about it, rstd = 1 / sqrt(var + eps).  weight / bias [C], 16-byte aligned, either may be NULL.
 * C % 4 == 0, 4 <= C <= 512.  out == in with the same ld is allowed, any other overlap is PFK_ERR_BAD_ARG. */
int pfk_layernorm_rows_f32(const float* in, long long in_ld, const float* weight, const float* bias, float eps, float* out,
                           long long out_ld, long long M, int C, pfk_stream_t stream);

/* pfk_xca_map_f32: XCA_separate's attention map (ccmr/xcit.py:211-229).  qk [B*N][qk_ld]: columns [0, heads*dh) are q, the next
 * heads*dh are k, column head*dh + d within each; temperature [heads]; A [B][heads][dh][dh] contiguous:
 *   A[b,h,i,j] = softmax_j( temperature[h] * (sum_n q[n,h,i] k[n,h,j]) / (max(|q_{h,i}|, 1e-12) * max(|k_{h,j}|, 1e-12)) ),
 * the norms over the N tokens of image b.  One pass over the rows forms the Gram and both norms per 256-token chunk (fp32) into
 * the workspace; the chunks are summed in order in double.  heads == 8 and dh == 16, anything else PFK_ERR_UNSUPPORTED.
 * workspace: pfk_xca_map_workspace_bytes(B, N, heads, dh) bytes (< 0: the status), 16-byte aligned, overlapping nothing. */
long long pfk_xca_map_workspace_bytes(int B, long long N, int heads, int dh);
int pfk_xca_map_f32(const float* qk, long long qk_ld, const float* temperature, float* A, void* workspace, long long workspace_bytes, int B,
                    long long N, int heads, int dh, pfk_stream_t stream);

/* The local patch interaction of XCABlock (ccmr/xcit.py:98-139, :298-299) around its GroupNorm, p = (b*H + y)*W + x, C == 128:
 *   pfk_xcit_lpi1_f32:  u = GELU(dw3x3(LN(x)) + dw_bias), LN with ln_weight / ln_bias [C] and ln_eps; the sums of u and u^2 of every
 *                       block and channel group (double) go to the workspace;
 *   pfk_xcit_lpi2_f32:  the GroupNorm statistics of each image (groups == 8 groups of C / 8 channels over H*W pixels, biased variance,
 *                       gn_eps) are finished from those partials in block order, in double; then
 *                       x2 = x + gamma * (dw3x3(GN(u)) + dw_bias),  t = LN(x2) [* ln_weight] [+ ln_bias]   (ln_weight / ln_bias may be NULL).
 * dw_weight [C][9] (tap ky*3 + kx), "same" zero padding of the NORMALISED tensor: a tap outside the image contributes exactly 0, and
 * no tap leaves its image.  Any H, W >= 1.  Per-channel vectors 16-byte aligned.  No output may overlap an input, another output or
 * the workspace.  workspace: pfk_xcit_lpi_workspace_bytes(B, H, W) bytes (< 0: the status), 16-byte aligned, the same for both
 * entries: lpi2 reads what lpi1 left there.  C != 128 or groups != 8: PFK_ERR_UNSUPPORTED. */
long long pfk_xcit_lpi_workspace_bytes(int B, int H, int W);
int pfk_xcit_lpi1_f32(const float* x, long long x_ld, const float* ln_weight, const float* ln_bias, float ln_eps, const float* dw_weight,
                      const float* dw_bias, float* u, long long u_ld, void* workspace, long long workspace_bytes, int B, int H, int W,
                      int C, pfk_stream_t stream);
int pfk_xcit_lpi2_f32(const float* u, long long u_ld, const float* gn_weight, const float* gn_bias, float gn_eps, int groups,
                      const float* dw_weight, const float* dw_bias, const float* gamma, const float* x, long long x_ld, float* x2,
                      long long x2_ld, const float* ln_weight, const float* ln_bias, float ln_eps, float* t, long long t_ld, void* workspace,
                      long long workspace_bytes, int B, int H, int W, int C, pfk_stream_t stream);

/* ---- K17: CCMR's per-scale context grouping `model.xcit[i]` (ccmr/ccmr.py:191, the same XCiT with separate=False; additions, ABI 7) ----
 * The rules of K14 hold: fp32, 16-byte aligned rows with ld % 4 == 0, no atomics, arguments validated before the device is touched.
 *
 * pfk_xcit_tokens_f32: one pass from the NCHW tensor in[b][c][y][x] (contiguous, C == 128) to the block's token rows, p = (b*H + y)*W + x:
 *   x0[p][c] = in[b][c][y][x] + pos[y*W + x][c]      (pos [H*W][C] contiguous, 16-byte aligned, may be NULL: nothing is added)
 *   xh[p][c] = (x0[p][c] - mean_p) * rstd_p           mean over the C channels, then the biased variance about it (two passes over
 *                                                     the registers, never E[x^2] - mean^2), rstd = 1 / sqrt(var + eps); no affine.
 * pfk_xcit_tokens_pm_f32: the same from pixel-major input rows in[p][in_ld] (a channels-last tensor), in_ld >= C, in_ld % 4 == 0.
 * x0_ld, xh_ld >= C.  No output may overlap the other output, `in` or `pos`.  C != 128: PFK_ERR_UNSUPPORTED. */
int pfk_xcit_tokens_f32(const float* in, const float* pos, float eps, float* x0, long long x0_ld, float* xh, long long xh_ld, int B, int C,
                        int H, int W, pfk_stream_t stream);
int pfk_xcit_tokens_pm_f32(const float* in, long long in_ld, const float* pos, float eps, float* x0, long long x0_ld, float* xh,
                           long long xh_ld, int B, int C, int H, int W, pfk_stream_t stream);

/* pfk_xca_fold_f32: everything of XCA between its value projection and `proj` is linear in the values, so behind the attention map
 * A [B][heads][dh][dh] (pfk_xca_map_f32) the branch is one affine map per image on LayerNorm(x) without affine:
 *   M[b] = wp blockdiag(A[b]) wv   [C][C],      c[b] = wp (blockdiag(A[b]) bv) + bp   [C],      C = heads * dh,
 * with wv [C][C] = W_v diag(ln.weight), bv [C] = W_v ln.bias + b_v, wp [C][C] = diag(gamma) W_proj, bp [C] = gamma * b_proj, all
 * contiguous and 16-byte aligned.  Each element is one fmaf chain in ascending index order.  heads == 8 and dh == 16, anything else
 * PFK_ERR_UNSUPPORTED.  M and c overlap nothing. */
int pfk_xca_fold_f32(const float* A, const float* wv, const float* bv, const float* wp, const float* bp, float* M, float* c, int B,
                     int heads, int dh, pfk_stream_t stream);

/* ---- K15: the multi-scale GroupNorm encoders (ccmr/extractor.py, ms_raft_plus/extractor.py: `fnet` / `cnet` of CCMR, CCMR+, MS-RAFT+;
 * additions, ABI 7) ----
 * fp32 pixel-major rows x[B*HW][ld] of which only columns [0, C) are read or written; rows 16-byte aligned, every ld % 4 == 0 (ld in
 * floats).  Memory-bound row kernels, 16-byte accesses.  Deterministic: no atomics, every sum in an order fixed by the shape.
 * Arguments are validated before the device is touched.
 *
 * pfk_groupnorm_stats_f32: nn.GroupNorm statistics (biased variance, eps inside the sqrt) over groups of `group_size` CONSECUTIVE
 * channels, per (image, group) over HW * group_size values, finished into the affine pair the apply pass reads, both [B][C] fp32:
 *   scale[b][c] = rstd_g * gamma[c],   shift[b][c] = beta[c] - mean_g * rstd_g * gamma[c]      (g = c / group_size)
 * One pass over x: sum(x) and sum(x*x) in double per 256-pixel chunk of an image, the chunks added in a fixed order, var =
 * E[x^2] - mean^2 and the pair evaluated in double and rounded to fp32 once.  gamma / beta [C] are required (PFK_ERR_BAD_ARG).
 * group_size must be 8 — the group of every GroupNorm in those encoders — with C % 8 == 0 and C <= 1024: anything else
 * PFK_ERR_UNSUPPORTED.  workspace: pfk_groupnorm_workspace_bytes(B, HW, C) bytes (< 0: the status), 8-byte aligned. */
long long pfk_groupnorm_workspace_bytes(int B, int HW, int C);
int pfk_groupnorm_stats_f32(const float* x, int ld, int B, int HW, int C, int group_size, const float* gamma, const float* beta,
                            float eps, float* scale, float* shift, void* workspace, long long workspace_bytes, pfk_stream_t stream);

/* out = relu?(x * scale[b][c] + shift[b][c]) ; if residual: out = relu_after?(residual + out)  — pfk_norm_apply_f32's contract with
 * the affine pair of pfk_groupnorm_stats_f32 in place of mean / rstd (x * scale + shift is one fused multiply-add).  scale / shift
 * [B][C], 16-byte aligned, C % 4 == 0.  x, residual and out each have their own ld; out may alias x. */
int pfk_affine_apply_f32(const float* x, int x_ld, const float* scale, const float* shift, const float* residual, int residual_ld,
                         float* out, int out_ld, int B, int HW, int C, int relu, int relu_after_residual, pfk_stream_t stream);

/* Bilinear resize of rows in[B*Hi*Wi][in_ld] to out[B*Ho*Wo][out_ld], channels [0, C), C % 4 == 0: F.interpolate(mode="bilinear",
 * align_corners=False), which for upsizing is also torchvision's TF.resize (antialias on) — the source coordinate of output o is
 * (o + 0.5) * in / out - 0.5 clamped to the image, the two taps per axis weighted linearly, edge taps replicated; no tap leaves its
 * image.  Coordinates and weights come from integer arithmetic (no rounded coordinate).  Any Ho >= Hi and Wo >= Wi (the same size: a
 * copy); downsizing needs another filter: PFK_ERR_UNSUPPORTED, as is 2 * Ho * Hi or 2 * Wo * Wi >= 2^31.  out must not overlap in. */
int pfk_resize_bilinear_pm_f32(const float* in, int in_ld, float* out, int out_ld, int B, int Hi, int Wi, int Ho, int Wo, int C,
                               pfk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PFK_H */
