// K12b — weight gradient of the convolution on bf16 operands (the training form of K8b, pfk_conv2d_b16):
//
//   dW[co][k] = sum_p dY[p][co] * A[p][k],     A[p][k = (source, tap, channel)] = src_s[p + tap][c]  (zero outside the image)
//
// on v_mfma_f32_32x32x16_bf16 with fp32 accumulation, straight from the pixel-major bf16 tensors — no im2col, no transposing
// pass.  The reduction index is the PIXEL: a K-step is 64 consecutive pixels, staged as rows exactly as they lie in memory
// (dY: 64 rows x 32 CB output channels, A: 64 rows x 32 input channels of each of the tile's (source, tap, chunk) entries, the
// tap's zero padding done by out-of-range buffer offsets as in the forward kernel and in pfk_wgrad.hip, so the zeros are IN
// LDS).  The MFMA wants 8 consecutive pixels of one channel per lane for both operands; the rows hold 8 consecutive channels
// of one pixel.  ds_read_b64_tr_b16 does the transpose on the way out of LDS: per 16-lane group it reads 4 rows x 16 columns
// and hands lane i column i, so two reads give a lane its 8 pixels.
//
// LDS image: every 32-channel piece of a tile is its own [64 pixels][32 channels] sub-image with 64-byte rows.  A 32-lane half of
// a transposed read takes 4 consecutive rows x 32 channels = 256 contiguous bytes = all 64 banks once: conflict-free (the two
// halves never conflict with each other).  The staging ds_write_b128 of four consecutive threads fill one row.
// The transposed read needs EXEC all ones and every lane's address inside the image: tiles are padded with zeros (channels
// past cout / past the source's channels, pixels past the slice), never masked; nothing branches per lane before the reads.
//
// Grid, tile shapes (CB = 32-row output-channel blocks per tile in {4, 2, 1}, one 32x32 accumulator per wave), the split of the
// pixel range into slices and their fixed-order reduction into PyTorch's layouts are those of pfk_wgrad.hip
// (pfk_wgrad_reduce.h); outputs and partial tiles are fp32.
#include "pfk_launch.h"
#include "pfk_wgrad_reduce.h"

namespace {

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
constexpr unsigned OOB = 0x80000000u;
constexpr int KS = 64;          // pixels per K-step

struct WgradB16Args {
  const void* src0; const void* src1; const void* src2;
  int ld0, ld1, ld2, ch0, ch1, ch2, nsrc;
  const void* dy; int dy_ld; int cout;
  int H, W, kh, kw;
  long long M;
  float* part;            // [splits][cout][ktot]
  int ktot, chunks, tiles_m;   // ktot / chunks include the bias chunk when with_bias
  int with_bias;               // one extra 32-column chunk whose column 0 is sum_p dY[p][co] (A = a column of ones)
  long long px_per_split; // multiple of KS
};

// 4 rows x 16 columns of 16-bit elements per 16-lane group, delivered column-major (ds_read_b64_tr_b16)
__device__ __forceinline__ s16x4 tr_read(const unsigned short* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
}

template <int CB>
__global__ __launch_bounds__(256) void conv_wgrad_b16_kernel(const WgradB16Args a) {
  constexpr int NCH = 4 / CB;
  __shared__ __attribute__((aligned(16))) unsigned short sY[2][CB][KS][32];
  __shared__ __attribute__((aligned(16))) unsigned short sX[2][NCH][KS][32];

  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int groups = (a.chunks + NCH - 1) / NCH;
  const int grp = blockIdx.x % groups;
  const int tile_m = blockIdx.x / groups;
  const int split = blockIdx.y;
  const int co0 = tile_m * 32 * CB;

  const __amdgpu_buffer_rsrc_t rsy = buffer_rsrc(a.dy);
  const long long p_begin = (long long)split * a.px_per_split;
  const long long p_end = min(a.M, p_begin + a.px_per_split);
  const int steps = p_end > p_begin ? (int)((p_end - p_begin + KS - 1) / KS) : 0;

  // this thread stages row (t >> 2) of every step: 16-byte piece q (8 channels) of each A chunk and of each dY block
  const int row = t >> 2, q = t & 3;
  long long p = p_begin + row;
  int x = (int)(p % a.W), y = (int)((p / a.W) % a.H);
  __amdgpu_buffer_rsrc_t rsx[NCH];
  int tap_off[NCH], cdy[NCH], cdx[NCH], cld[NCH];
  bool c_ok[NCH], is_bias[NCH], yok[CB];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const auto c = chunk_ref(a, grp * NCH + i);
    rsx[i] = buffer_rsrc(c.src);
    tap_off[i] = (c.dy * a.W + c.dx) * c.ld + c.c0 + q * 8;
    cdy[i] = c.dy; cdx[i] = c.dx; cld[i] = c.ld;
    c_ok[i] = c.live && !c.bias && c.c0 + q * 8 < c.cch;
    is_bias[i] = c.bias;
  }
#pragma unroll
  for (int i = 0; i < CB; ++i) yok[i] = co0 + q * 8 + 32 * i < a.cout;

  u32x4 rx[NCH], ry[CB];
  auto load = [&](void) {
    const bool in = p < p_end;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const bool ok = in && c_ok[i] && (unsigned)(y + cdy[i]) < (unsigned)a.H && (unsigned)(x + cdx[i]) < (unsigned)a.W;
      if (is_bias[i]) rx[i] = u32x4{(in && q == 0) ? 0x3f80u : 0u, 0u, 0u, 0u};        // A = [1 0 0 ...] (bf16) for every live pixel
      else rx[i] = __builtin_amdgcn_raw_buffer_load_b128(rsx[i], ok ? (unsigned)((int)p * cld[i] + tap_off[i]) * 2u : OOB, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < CB; ++i)
      ry[i] = __builtin_amdgcn_raw_buffer_load_b128(rsy, (in && yok[i]) ? (unsigned)((int)p * a.dy_ld + co0 + q * 8 + 32 * i) * 2u : OOB, 0, 0);
    p += KS;
    x += KS;
    while (x >= a.W) { x -= a.W; if (++y == a.H) y = 0; }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) *reinterpret_cast<u32x4*>(&sX[buf][i][row][q * 8]) = rx[i];
#pragma unroll
    for (int i = 0; i < CB; ++i) *reinterpret_cast<u32x4*>(&sY[buf][i][row][q * 8]) = ry[i];
  };

  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;

  if (steps > 0) {
    load();
    store(0);
  }
  __syncthreads();
  const int l31 = lane & 31, hl = lane >> 5;
  const int wcb = wid % CB, wch = wid / CB;      // this wave's co block / chunk inside the tile
  // transposed-read address of this lane inside a [64][32] sub-image: lane 4qq+pp of a 16-lane group supplies row r0 + qq,
  // columns c0 + 4pp .. +3; the group's block is columns 16 (l31 >> 4) .., rows 8 hl + 4 (second read) + 16 (MFMA of the step)
  const int trow = 8 * hl + ((lane & 15) >> 2), tcol = 16 * (l31 >> 4) + 4 * (lane & 3);
  for (int s = 0; s < steps; ++s) {
    const int buf = s & 1;
    const bool more = s + 1 < steps;
    if (more) load();
    const unsigned short* py = &sY[buf][wcb][trow][tcol];
    const unsigned short* px = &sX[buf][wch][trow][tcol];
#pragma unroll
    for (int j = 0; j < KS / 16; ++j) {
      const s16x4 a0 = tr_read(py + (16 * j) * 32), a1 = tr_read(py + (16 * j + 4) * 32);
      const s16x4 b0 = tr_read(px + (16 * j) * 32), b1 = tr_read(px + (16 * j + 4) * 32);
      const s16x8 av = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);
      const s16x8 bv = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, bv), acc, 0, 0, 0);
    }
    if (more) store(buf ^ 1);
    __syncthreads();
  }

  // D: column j = lane & 31 (input channel), rows i = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5) (output channel)
  const int chunk = grp * NCH + wch;
  if (chunk >= a.chunks) return;
  float* out = a.part + (long long)split * a.cout * a.ktot;
  const int kcol = chunk * 32 + l31;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int co = co0 + wcb * 32 + (e & 3) + 8 * (e >> 2) + 4 * hl;
    if (co < a.cout) out[(long long)co * a.ktot + kcol] = acc[e];
  }
}

int g_wgrad_b16_splits = 0;   // 0: by occupancy (pick_splits); n > 0: n slices (as far as the pixel range has K-steps) — pfk_debug_set_wgrad_b16

// The part of the plan that needs no pointers: tile height, grid and slices.
struct Plan { int cb, tiles_m, groups, splits, ktot; long long M; };

bool shape_ok(const pfk_conv_b16_desc* d) {
  if (!d || d->num_src < 1 || d->num_src > 3) return false;
  if (d->B <= 0 || d->H <= 0 || d->W <= 0 || d->cout <= 0 || (d->cout & 7)) return false;
  if (d->stride != 0 && d->stride != 1) return false;                       // the update block has no strided layer
  const bool k_ok = (d->kh == 1 && d->kw == 1) || (d->kh == 3 && d->kw == 3) || (d->kh == 1 && d->kw == 5) || (d->kh == 5 && d->kw == 1);
  if (!k_ok) return false;
  for (int i = 0; i < d->num_src; ++i)
    if (d->src[i].channels <= 0 || (d->src[i].channels & 7) || (d->src[i].ld & 7) || d->src[i].ld < d->src[i].channels) return false;
  return true;
}

Plan plan_of(const pfk_conv_b16_desc* d, int with_bias) {
  Plan pl;
  pl.ktot = pfk_conv_k(d, 32) + (with_bias ? 32 : 0);
  pl.M = (long long)d->B * d->H * d->W;
  const WgradGrid g = wgrad_grid(d->cout, pl.ktot, wgrad_pick_cb(d->cout));
  pl.cb = g.cb; pl.tiles_m = g.tiles_m; pl.groups = g.groups;
  // slices: K-steps of KS pixels (the last one partial), at least 8 (512 pixels) per slice
  pl.splits = wgrad_pick_splits((long long)g.tiles_m * g.groups, (pl.M + KS - 1) / KS, 8, g_wgrad_b16_splits);
  return pl;
}

}  // namespace

extern "C" {

int pfk_debug_set_wgrad_b16(int splits) {
  if (!pfk_debug_knobs_enabled()) return PFK_ERR_DISABLED;
  g_wgrad_b16_splits = splits;
  return PFK_OK;
}

long long pfk_conv_wgrad_unpacked_b16_workspace_bytes(const pfk_conv_b16_desc* d, int with_bias) {
  if (!shape_ok(d)) return 0;
  const Plan pl = plan_of(d, with_bias);
  return (long long)pl.splits * d->cout * pl.ktot * (long long)sizeof(float);     // the slices always go through the workspace
}

int pfk_conv_wgrad_unpacked_b16(const pfk_conv_b16_desc* d, const int* real_channels, const void* dy, int dy_ld, int cout_real,
                                float* dw, float* db, int accumulate, void* workspace, long long workspace_bytes, pfk_stream_t stream) {
  if (!d || !dw || !dy || !real_channels || !workspace || cout_real <= 0 || cout_real > d->cout) return PFK_ERR_BAD_ARG;
  if (!shape_ok(d) || dy_ld < d->cout || (dy_ld & 7)) return PFK_ERR_BAD_ARG;
  if (!pfk_aligned16(workspace) || !pfk_aligned16(dy)) return PFK_ERR_ALIGNMENT;
  const int with_bias = db != nullptr;
  const Plan pl = plan_of(d, with_bias);
  const long long n = (long long)d->cout * pl.ktot;
  if (workspace_bytes < pl.splits * n * (long long)sizeof(float)) return PFK_ERR_BAD_ARG;
  const pfk_conv_src_b16* s = d->src;
  for (int i = 0; i < d->num_src; ++i) {
    if (!s[i].ptr || real_channels[i] <= 0 || real_channels[i] > s[i].channels) return PFK_ERR_BAD_ARG;
    if (!pfk_aligned16(s[i].ptr)) return PFK_ERR_ALIGNMENT;
    if (!pfk_source_fits32(s[i], pl.M, 2)) return PFK_ERR_UNSUPPORTED;       // 32-bit byte offsets
  }
  if (!pfk_fits32(pl.M * dy_ld * 2)) return PFK_ERR_UNSUPPORTED;

  WgradB16Args a{};
  pfk_spread_sources(a, d);
  a.dy = dy; a.dy_ld = dy_ld; a.cout = d->cout;
  a.H = d->H; a.W = d->W; a.kh = d->kh; a.kw = d->kw; a.M = pl.M;
  a.with_bias = with_bias;
  a.ktot = pl.ktot; a.chunks = pl.ktot / 32; a.tiles_m = pl.tiles_m;
  a.px_per_split = ((pl.M + pl.splits - 1) / pl.splits + KS - 1) / KS * KS;
  a.part = static_cast<float*>(workspace);

  const UnpackArgs u = wgrad_unpack_args(d, real_channels, a.part, n, pl.splits, pl.ktot, cout_real, with_bias, dw, db, accumulate);

  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)(pl.tiles_m * pl.groups), (unsigned)pl.splits);
  wgrad_launch_cb<conv_wgrad_b16_kernel<4>, conv_wgrad_b16_kernel<2>, conv_wgrad_b16_kernel<1>>(pl.cb, grid, st, a);
  const long long total = (long long)cout_real * pl.ktot;
  hipLaunchKernelGGL(wgrad_reduce_unpack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, u);
  return pfk_launch_status();
}

}  // extern "C"
