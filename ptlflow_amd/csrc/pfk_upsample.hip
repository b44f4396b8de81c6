// Convex upsampling, unfused: RAFT.upsample_flow (raft/raft.py:112-123), its scale = 2 form of the multi-scale loops
// (ccmr/ccmr.py:128-139) and SEARAFT.upsample_data (sea_raft.py:147-163), forward and backward.  The arithmetic of a (coarse pixel, sub-pixel) is pfk_upsample.h's; this file is the lane layouts around it, the
// cross-lane reductions of the backward and the C entry points.  Bandwidth-bound VALU kernels, compiled with -ffp-contract=off.
// (The fused forms — mask head conv2 + softmax + upsampling, K13 / K13b — are in pfk_gemm.hip / pfk_gemm_b16.hip.)
#include "pfk_launch.h"
#include "pfk_upsample.h"

#include <initializer_list>

namespace {

// ------------------------------------------------------------------------------------------------------------------
// Forward.  A wave holds V coarse pixels, 64 / V lanes each; a lane holds V neighbouring sub-pixels s = V * idx .. + V - 1 of the 64
// (sy = s >> 3, sx = s & 7) of its pixel: the V floats of each of the nine taps' 64 mask logits, and V output floats per channel.
//   V = 1  one pixel per wave, four per block: the nine mask reads are 256-byte coalesced rows, the 3x3 neighbourhood is broadcast;
//          any mask_ld / alignment.
//   V = 4  four pixels per wave, 16 per block: a tap is ONE 1 KiB load per wave (9 per 4 pixels instead of 36 of 256 bytes) and an
//          output row piece of the group is 128 contiguous bytes.  Needs 16-byte aligned mask rows and output.
// TM = __bf16: the mask as the K8b mask head writes it (2-byte logits, widened exactly; half the bytes of this HBM-bound kernel).
// INFO: upsample_data — the same convex combination of n_info <= UP_MAX_INFO info channels (no factor 8) -> info_out
// [B][n_info][8H][8W]; flow and info are pixel-major rows.
// Every output element is up_softmax9 + up_combine (pfk_upsample.h) whatever V, TM and INFO: same logits and flow, same bits.
// ------------------------------------------------------------------------------------------------------------------
template <typename TM, int V, bool INFO>
__global__ __launch_bounds__(256) void convex_upsample_kernel(const float* __restrict__ flow, int flow_ld,
                                                              const float* __restrict__ info, int info_ld, int n_info,
                                                              const TM* __restrict__ mask, int mask_ld, float* __restrict__ out,
                                                              float* __restrict__ info_out, long long M, int H, int W) {
  static_assert(V == 1 || V == 4, "sub-pixels per lane");
  constexpr int NI = INFO ? UP_MAX_INFO : 0, LP = 64 / V;
  if (INFO) __builtin_assume(flow_ld > 0);
  const int lane = threadIdx.x & 63;
  const long long p = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * V + lane / LP;
  if (p >= M) return;
  const int s0 = (lane % LP) * V;
  const UpPixel px = up_pixel(p, H, W);
  const long long img = px.b * ((long long)H * W);
  const TM* mrow = mask + p * mask_ld + s0;
  float m[V][9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    if constexpr (V == 4) {
      const f32x4 t = load4_widen(mrow + k * 64);
#pragma unroll
      for (int c = 0; c < 4; ++c) m[c][k] = t[c];
    } else {
      m[0][k] = (float)mrow[k * 64];
    }
  }
  float v[2 + NI][9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    float t[2 + NI];
    up_tap<NI>(k, flow, flow_ld, info, info_ld, n_info, img, px.y, px.x, H, W, t);
#pragma unroll
    for (int ch = 0; ch < 2 + NI; ++ch) v[ch][k] = t[ch];
  }
  float o[2 + NI][V];
#pragma unroll
  for (int c = 0; c < V; ++c) {
    up_softmax9(m[c]);
#pragma unroll
    for (int ch = 0; ch < 2 + NI; ++ch) o[ch][c] = up_combine(m[c], v[ch]);
  }
  const long long HW8 = (long long)H * W * 64;
  const long long at = up_out_offset(px.y, px.x, s0 >> 3, s0 & 7, W);
#pragma unroll
  for (int ch = 0; ch < 2 + NI; ++ch) {
    if (ch >= 2 && ch - 2 >= n_info) continue;
    float* dst = (ch < 2 ? out + (px.b * 2 + ch) * HW8 : info_out + (px.b * n_info + (ch - 2)) * HW8) + at;
    if constexpr (V == 4) *reinterpret_cast<f32x4*>(dst) = f32x4{o[ch][0], o[ch][1], o[ch][2], o[ch][3]};
    else *dst = o[ch][0];
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Forward by 2: `upsample_flow(flow, mask, scale=2)` of ccmr/ccmr.py:128-139 / ms_raft_plus/ms_raft_plus.py:133-144.  36 mask logits
// per coarse pixel, channel c = k * 4 + sy * 2 + sx; out [B][2][2H][2W].  The 8x layout gives a wave the 64 sub-pixels of a pixel;
// here a pixel has four, so a lane owns one (coarse pixel, sy): the sub-pixels sx = 0, 1 of nine taps are nine 8-byte pieces of the
// pixel's 144-byte mask row, and the two results of a channel are one 8-byte store.  A wave holds 32 consecutive pixels, lanes
// 0..31 the upper output row (sy = 0) and lanes 32..63 the lower: each half wave writes 256 contiguous bytes per channel, and the
// nine reads of the wave together cover the pixels' mask rows exactly once (32 x 144 contiguous bytes where mask_ld == 36).
// VEC: mask rows and output 8-byte aligned (mask_ld even); otherwise the same lanes use 4-byte accesses.  Same arithmetic
// (up_softmax9 + up_combine on up_tap<0, 2>) either way: same bits.
// ------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void convex_upsample2_kernel(const float* __restrict__ flow, int flow_ld,
                                                               const float* __restrict__ mask, int mask_ld, float* __restrict__ out,
                                                               long long M, int H, int W) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;     // blockDim.x is a multiple of 64
  const int lane = threadIdx.x & 63, sy = lane >> 5;
  const long long p = (t >> 6) * 32 + (lane & 31);
  if (p >= M) return;
  const UpPixel px = up_pixel(p, H, W);
  const long long img = px.b * ((long long)H * W);
  const float* mrow = mask + p * mask_ld + sy * 2;
  float m[2][9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    if constexpr (VEC) {
      const f32x2 w = *reinterpret_cast<const f32x2*>(mrow + k * 4);
      m[0][k] = w[0];
      m[1][k] = w[1];
    } else {
      m[0][k] = mrow[k * 4];
      m[1][k] = mrow[k * 4 + 1];
    }
  }
  float v[2][9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    float f[2];
    up_tap<0, 2>(k, flow, flow_ld, nullptr, 0, 0, img, px.y, px.x, H, W, f);
    v[0][k] = f[0];
    v[1][k] = f[1];
  }
  up_softmax9(m[0]);
  up_softmax9(m[1]);
  const long long HW4 = (long long)H * W * 4;
  const long long at = up_out_offset<2>(px.y, px.x, sy, 0, W);
#pragma unroll
  for (int ch = 0; ch < 2; ++ch) {
    const float o0 = up_combine(m[0], v[ch]), o1 = up_combine(m[1], v[ch]);
    float* dst = out + (px.b * 2 + ch) * HW4 + at;
    if constexpr (VEC) {
      *reinterpret_cast<f32x2*>(dst) = f32x2{o0, o1};
    } else {
      dst[0] = o0;
      dst[1] = o1;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Backward of upsample_flow.  Forward, per coarse pixel p and sub-pixel (sy, sx) = lane:
//     w_k = softmax_k(mask[p][k*64 + lane]),   out[c][8y+sy][8x+sx] = sum_k w_k * 8 * flow[c][nbr_k(p)]   (zero outside)
// One wave per coarse pixel, lane = sub-pixel (as the forward's V = 1):
//     dw_k = g_x * vx_k + g_y * vy_k;   dmask[p][k*64 + lane] = w_k * (dw_k - sum_j w_j dw_j)
//     dflow[c][nbr_k(p)] += 8 * sum_lanes w_k * g_c       -> wave-reduced into part[p][k][c]; the gather kernel adds the <= 9
//                                                            contributions of each flow pixel in a fixed order (no atomics).
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void convex_upsample_bwd_kernel(const float* __restrict__ flow, int flow_ld,
                                                                  const float* __restrict__ mask, int mask_ld,
                                                                  const float* __restrict__ gout, float* __restrict__ gmask,
                                                                  int gmask_ld, float* __restrict__ part, long long M, int H,
                                                                  int W) {
  const int lane = threadIdx.x & 63;
  const long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= M) return;
  const UpPixel px = up_pixel(p, H, W);
  const long long img = px.b * ((long long)H * W);
  const float* mrow = mask + p * mask_ld + lane;
  float m[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) m[k] = mrow[k * 64];
  up_softmax9(m);
  const long long HW8 = (long long)H * W * 64;
  const long long o = up_out_offset(px.y, px.x, lane >> 3, lane & 7, W);
  const float gx = gout[(px.b * 2 + 0) * HW8 + o], gy = gout[(px.b * 2 + 1) * HW8 + o];
  float dw[9], dot = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    float v[2];
    up_tap<0>(k, flow, flow_ld, nullptr, 0, 0, img, px.y, px.x, H, W, v);
    dw[k] = gx * v[0] + gy * v[1];
    dot += m[k] * dw[k];
  }
  float* grow = gmask + p * gmask_ld + lane;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    grow[k * 64] = m[k] * (dw[k] - dot);
    float cxv = m[k] * gx, cyv = m[k] * gy;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {      // two wave_sums interleaved step by step: as two calls the kernel schedules differently
      cxv += __shfl_xor(cxv, s, 64);
      cyv += __shfl_xor(cyv, s, 64);
    }
    if (lane == 0) {
      part[(p * 9 + k) * 2 + 0] = 8.0f * cxv;
      part[(p * 9 + k) * 2 + 1] = 8.0f * cyv;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Backward of upsample_data, C = 2 + NI channels (the two flow channels x 8, then NI info channels), in the forward's V = 4 layout:
// a tap of the mask, a tap of the mask gradient and a channel of the upsampled gradient are 16 bytes per lane and 1 KiB / 4 x 128
// contiguous bytes per wave.  Per sub-pixel
//     dw_k = sum_c g_c * v_c,k  (c in order);   dmask[p][k*64 + s] = w_k * (dw_k - sum_j w_j dw_j)
//     dv[c][nbr_k(p)] += scale_c * sum_s w_k g_c     -> four sub-pixels in the lane, then xor 8, 4, 2, 1 across the pixel's 16 lanes,
//                                                       into part[p][k][c] (lane c of the pixel stores channel c: one C-float row);
// the gather kernel then adds the <= 9 contributions of each (pixel, channel) in tap order (no atomics).
// ------------------------------------------------------------------------------------------------------------------

// One step of the butterfly sum over a 16-lane row: s + (the value of lane ^ N).  Steps run N = 8, 4, 2, 1, so the value has period
// 2N inside the row when step N reads it, and the lane N further round the row (DPP row_ror: no LDS traffic) holds what lane ^ N holds.
template <int N>
__device__ inline float row16_xor_add(float s) {
  return s + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0x120 + N, 0xf, 0xf, false));
}

template <int NI>
__global__ __launch_bounds__(256) void convex_upsample_info_bwd_kernel(const float* __restrict__ flow, int flow_ld,
                                                                       const float* __restrict__ info, int info_ld,
                                                                       const float* __restrict__ mask, int mask_ld,
                                                                       const float* __restrict__ gflow_up,
                                                                       const float* __restrict__ ginfo_up, float* __restrict__ gmask,
                                                                       int gmask_ld, float* __restrict__ part, long long M, int H,
                                                                       int W) {
  constexpr int C = 2 + NI;
  __builtin_assume(flow_ld > 0);
  const int lane = threadIdx.x & 63;
  const long long p = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 4 + (lane >> 4);
  if (p >= M) return;   // whole 16-lane groups leave: the shuffles below stay inside a group
  const int idx = lane & 15;
  const UpPixel px = up_pixel(p, H, W);
  const long long img = px.b * ((long long)H * W);
  const float* mrow = mask + p * mask_ld + idx * 4;
  f32x4 w[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) w[k] = *reinterpret_cast<const f32x4*>(mrow + k * 64);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float t[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) t[k] = w[k][j];
    up_softmax9(t);
#pragma unroll
    for (int k = 0; k < 9; ++k) w[k][j] = t[k];
  }
  const long long HW8 = (long long)H * W * 64;
  const long long o = up_out_offset(px.y, px.x, idx >> 1, (idx & 1) * 4, W);
  f32x4 g[C];
  g[0] = *reinterpret_cast<const f32x4*>(gflow_up + (px.b * 2 + 0) * HW8 + o);
  g[1] = *reinterpret_cast<const f32x4*>(gflow_up + (px.b * 2 + 1) * HW8 + o);
#pragma unroll
  for (int i = 0; i < NI; ++i)
    g[2 + i] = ginfo_up ? *reinterpret_cast<const f32x4*>(ginfo_up + (px.b * NI + i) * HW8 + o) : f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 dw[9], dot = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    float v[C];
    up_tap<NI>(k, flow, flow_ld, info, info_ld, NI, img, px.y, px.x, H, W, v);
    f32x4 a = g[0] * v[0];
#pragma unroll
    for (int c = 1; c < C; ++c) a += g[c] * v[c];
    dw[k] = a;
    dot += w[k] * a;
  }
  float* grow = gmask + p * gmask_ld + idx * 4;
  float* prow = part + p * (9 * C);
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    *reinterpret_cast<f32x4*>(grow + k * 64) = w[k] * (dw[k] - dot);
    float mine = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const f32x4 t = w[k] * g[c];
      float s = (t[0] + t[1]) + (t[2] + t[3]);
      s = row16_xor_add<8>(s);
      s = row16_xor_add<4>(s);
      s = row16_xor_add<2>(s);
      s = row16_xor_add<1>(s);
      if (c < 2) s *= 8.0f;
      mine = (idx == c) ? s : mine;
    }
    if (idx < C) prow[k * C + idx] = mine;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Backward of the upsampling by 2, in the forward's lane layout (convex_upsample2_kernel): a lane owns one (coarse pixel, sy) and
// holds the sub-pixels sx = 0, 1 of nine taps — nine 8-byte pieces of the pixel's mask row, nine 8-byte pieces of its mask-gradient
// row, and 8 bytes of each channel of the upsampled gradient.  Per sub-pixel, as the x8 kernel above:
//     dw_k = g_x * vx_k + g_y * vy_k;   dmask[p][k*4 + sy*2 + sx] = w_k * (dw_k - sum_j w_j dw_j)
//     dflow[c][nbr_k(p)] += 2 * sum over the pixel's four sub-pixels of w_k * g_c
// The four sub-pixels: two in the lane, the other two in the lane 32 away.  ONE v_permlane32_swap per tap finishes both channels:
// with vdst = the x sum and src = the y sum, lanes 0..31 end up holding (own x, upper x) and lanes 32..63 (lower y, own y), so the
// lower half adds and stores channel 0 of part[p][k][.] and the upper half channel 1 — nine swaps per lane where two butterflies
// through ds_bpermute (`__shfl_xor(v, 32)`) would take eighteen LDS-crossbar operations.  The gather kernel below (C = 2) adds the
// <= 9 contributions of each flow pixel in tap order: no atomics, a fixed order, the same bits every run.
// Both lanes of a pixel leave together at `p >= M`, so a swap never reads a lane that is gone.
// VEC: mask rows, mask-gradient rows and the upsampled gradient 8-byte aligned (even row strides); otherwise 4-byte accesses.
// ------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void convex_upsample2_bwd_kernel(const float* __restrict__ flow, int flow_ld,
                                                                   const float* __restrict__ mask, int mask_ld,
                                                                   const float* __restrict__ gout, float* __restrict__ gmask,
                                                                   int gmask_ld, float* __restrict__ part, long long M, int H,
                                                                   int W) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;     // blockDim.x is a multiple of 64
  const int lane = threadIdx.x & 63, sy = lane >> 5;
  const long long p = (t >> 6) * 32 + (lane & 31);
  if (p >= M) return;
  const UpPixel px = up_pixel(p, H, W);
  const long long img = px.b * ((long long)H * W);
  const float* mrow = mask + p * mask_ld + sy * 2;
  float m[2][9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    if constexpr (VEC) {
      const f32x2 w = *reinterpret_cast<const f32x2*>(mrow + k * 4);
      m[0][k] = w[0];
      m[1][k] = w[1];
    } else {
      m[0][k] = mrow[k * 4];
      m[1][k] = mrow[k * 4 + 1];
    }
  }
  up_softmax9(m[0]);
  up_softmax9(m[1]);
  const long long HW4 = (long long)H * W * 4;
  const long long at = up_out_offset<2>(px.y, px.x, sy, 0, W);
  float g[2][2];      // [channel][sx]
#pragma unroll
  for (int ch = 0; ch < 2; ++ch) {
    const float* src = gout + (px.b * 2 + ch) * HW4 + at;
    if constexpr (VEC) {
      const f32x2 w = *reinterpret_cast<const f32x2*>(src);
      g[ch][0] = w[0];
      g[ch][1] = w[1];
    } else {
      g[ch][0] = src[0];
      g[ch][1] = src[1];
    }
  }
  float dw[2][9], dot[2] = {0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    float v[2];
    up_tap<0, 2>(k, flow, flow_ld, nullptr, 0, 0, img, px.y, px.x, H, W, v);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      dw[s][k] = g[0][s] * v[0] + g[1][s] * v[1];
      dot[s] += m[s][k] * dw[s][k];
    }
  }
  float* grow = gmask + p * gmask_ld + sy * 2;
  float* prow = part + p * 18 + sy;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const float d0 = m[0][k] * (dw[0][k] - dot[0]), d1 = m[1][k] * (dw[1][k] - dot[1]);
    if constexpr (VEC) {
      *reinterpret_cast<f32x2*>(grow + k * 4) = f32x2{d0, d1};
    } else {
      grow[k * 4] = d0;
      grow[k * 4 + 1] = d1;
    }
    const float cxv = m[0][k] * g[0][0] + m[1][k] * g[0][1];
    const float cyv = m[0][k] * g[1][0] + m[1][k] * g[1][1];
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(cxv), __float_as_uint(cyv), false, false);
    prow[k * 2] = 2.0f * (__uint_as_float(r[0]) + __uint_as_float(r[1]));      // sy = 0: channel x, sy = 1: channel y
  }
}

// grad[p][c] = sum_k part[pixel (y - ky + 1, x - kx + 1)][k][c], k ascending (the pixels whose k-th neighbour is p); one thread per
// (pixel, channel).  c < 2 goes to the flow gradient — NCHW [B][2][H][W] (gflow_ld == 0: RAFT) or pixel-major rows — the rest to the
// info rows.
__global__ __launch_bounds__(256) void convex_upsample_bwd_gather_kernel(const float* __restrict__ part, int C,
                                                                         float* __restrict__ gflow, int gflow_ld,
                                                                         float* __restrict__ ginfo, int ginfo_ld, long long M,
                                                                         int H, int W) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= M * C) return;
  const long long p = t / C;
  const int c = (int)(t - p * C);
  const UpPixel px = up_pixel(p, H, W);
  const long long hw = (long long)H * W;
  float a = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int yy = px.y - (k / 3 - 1), xx = px.x - (k % 3 - 1);
    if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) {
      const long long src = px.b * hw + (long long)yy * W + xx;
      a += part[(src * 9 + k) * C + c];
    }
  }
  if (c >= 2) ginfo[p * ginfo_ld + (c - 2)] = a;
  else if (gflow_ld > 0) gflow[p * gflow_ld + c] = a;
  else gflow[(px.b * 2 + c) * hw + (p - px.b * hw)] = a;
}

// ------------------------------------------------------------------------------------------------------------------ host side
// What all eleven entry points check first: the pointers every one of them needs, the grid, the mask row stride (at least the
// `mask_channels` = 9 S^2 logits of a pixel) and the flow layout (pixel-major rows of at least two floats; 0 = NCHW where the entry
// point reads it).
bool up_args_ok(std::initializer_list<const void*> required, int B, int H, int W, int mask_ld, int flow_ld, bool nchw_ok = false,
                int mask_channels = 576) {
  for (const void* ptr : required)
    if (!ptr) return false;
  return B > 0 && H > 0 && W > 0 && mask_ld >= mask_channels && (flow_ld >= 2 || (nchw_ok && flow_ld == 0));
}

// blocks of `per_block` items; false where the count does not fit a grid dimension
bool up_grid(long long items, int per_block, unsigned& blocks) {
  const long long n = (items + per_block - 1) / per_block;
  blocks = (unsigned)n;
  return pfk_fits_int(n);
}

template <typename TM, int V, bool INFO>
int launch_convex_upsample(const float* flow, int flow_ld, const float* info, int info_ld, int n_info, const TM* mask, int mask_ld,
                           float* out, float* info_out, int B, int H, int W, pfk_stream_t stream) {
  const long long M = (long long)B * H * W;
  unsigned blocks;
  if (!up_grid(M, 4 * V, blocks)) return PFK_ERR_UNSUPPORTED;
  hipLaunchKernelGGL((convex_upsample_kernel<TM, V, INFO>), dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), flow, flow_ld,
                     info, info_ld, n_info, mask, mask_ld, out, info_out, M, H, W);
  return pfk_launch_status();
}

// fp32 mask, flow only: four pixels per wave where the mask rows and the output allow 16-byte accesses
int convex_upsample_f32(const float* flow, int flow_ld, const float* mask, int mask_ld, float* out, int B, int H, int W,
                        pfk_stream_t stream) {
  if (pfk_aligned16(mask) && pfk_aligned16(out) && (mask_ld & 3) == 0)
    return launch_convex_upsample<float, 4, false>(flow, flow_ld, nullptr, 0, 0, mask, mask_ld, out, nullptr, B, H, W, stream);
  return launch_convex_upsample<float, 1, false>(flow, flow_ld, nullptr, 0, 0, mask, mask_ld, out, nullptr, B, H, W, stream);
}

template <typename TM>
int convex_upsample_info(const float* flow_pm, int flow_ld, const float* info_pm, int info_ld, int n_info, const TM* mask, int mask_ld,
                         float* flow_out, float* info_out, int B, int H, int W, pfk_stream_t stream) {
  if (!up_args_ok({flow_pm, info_pm, mask, flow_out, info_out}, B, H, W, mask_ld, flow_ld)) return PFK_ERR_BAD_ARG;
  if (n_info < 1 || n_info > UP_MAX_INFO || info_ld < n_info) return PFK_ERR_BAD_ARG;
  constexpr int ld_mask = 16 / (int)sizeof(TM) - 1;       // rows of 16-byte pieces
  if (!pfk_aligned16(mask) || (mask_ld & ld_mask) || !pfk_aligned16(flow_out) || !pfk_aligned16(info_out)) return PFK_ERR_ALIGNMENT;
  return launch_convex_upsample<TM, 4, true>(flow_pm, flow_ld, info_pm, info_ld, n_info, mask, mask_ld, flow_out, info_out, B, H, W, stream);
}

}  // namespace

extern "C" {

int pfk_convex_upsample_f32(const float* flow, const float* mask, int mask_ld, float* out, int B,
                            int H, int W, pfk_stream_t stream) {
  if (!up_args_ok({flow, mask, out}, B, H, W, mask_ld, 0, true)) return PFK_ERR_BAD_ARG;
  return convex_upsample_f32(flow, 0, mask, mask_ld, out, B, H, W, stream);
}

int pfk_convex_upsample_pm_f32(const float* flow_pm, int flow_ld, const float* mask, int mask_ld, float* out,
                               int B, int H, int W, pfk_stream_t stream) {
  if (!up_args_ok({flow_pm, mask, out}, B, H, W, mask_ld, flow_ld)) return PFK_ERR_BAD_ARG;
  return convex_upsample_f32(flow_pm, flow_ld, mask, mask_ld, out, B, H, W, stream);
}

int pfk_convex_upsample_pm_b16(const float* flow_pm, int flow_ld, const void* mask_bf16, int mask_ld, float* out,
                               int B, int H, int W, pfk_stream_t stream) {
  if (!up_args_ok({flow_pm, mask_bf16, out}, B, H, W, mask_ld, flow_ld)) return PFK_ERR_BAD_ARG;
  if (!pfk_aligned<8>(mask_bf16) || !pfk_aligned16(out) || (mask_ld & 3)) return PFK_ERR_ALIGNMENT;
  return launch_convex_upsample<__bf16, 4, false>(flow_pm, flow_ld, nullptr, 0, 0, static_cast<const __bf16*>(mask_bf16), mask_ld, out,
                                                  nullptr, B, H, W, stream);
}

int pfk_convex_upsample_info_pm_f32(const float* flow_pm, int flow_ld, const float* info_pm, int info_ld, int n_info,
                                    const float* mask, int mask_ld, float* flow_out, float* info_out, int B, int H, int W,
                                    pfk_stream_t stream) {
  return convex_upsample_info<float>(flow_pm, flow_ld, info_pm, info_ld, n_info, mask, mask_ld, flow_out, info_out, B, H, W, stream);
}

int pfk_convex_upsample_info_pm_b16(const float* flow_pm, int flow_ld, const float* info_pm, int info_ld, int n_info,
                                    const void* mask_bf16, int mask_ld, float* flow_out, float* info_out, int B, int H, int W,
                                    pfk_stream_t stream) {
  return convex_upsample_info<__bf16>(flow_pm, flow_ld, info_pm, info_ld, n_info, static_cast<const __bf16*>(mask_bf16), mask_ld, flow_out,
                                      info_out, B, H, W, stream);
}

int pfk_convex_upsample2_f32(const float* flow, int flow_ld, const float* mask, int mask_ld, float* out, int B, int H, int W,
                             pfk_stream_t stream) {
  if (!up_args_ok({flow, mask, out}, B, H, W, mask_ld, flow_ld, true, 36)) return PFK_ERR_BAD_ARG;
  const long long M = (long long)B * H * W;
  unsigned blocks;
  if (!up_grid(M, 32, blocks)) return PFK_ERR_UNSUPPORTED;      // one wave of 32 pixels per block: these grids are a few thousand pixels
  const bool vec = pfk_aligned<8>(mask) && pfk_aligned<8>(out) && (mask_ld & 1) == 0;
  hipLaunchKernelGGL(vec ? convex_upsample2_kernel<true> : convex_upsample2_kernel<false>, dim3(blocks), dim3(64), 0,
                     static_cast<hipStream_t>(stream), flow, flow_ld, mask, mask_ld, out, M, H, W);
  return pfk_launch_status();
}

long long pfk_convex_upsample_bwd_workspace_bytes(int B, int H, int W) {
  return (long long)B * H * W * 18 * (long long)sizeof(float);
}

int pfk_convex_upsample_bwd_f32(const float* flow, int flow_ld, const float* mask, int mask_ld, const float* grad_out,
                                float* grad_mask, int grad_mask_ld, float* grad_flow, void* workspace, long long workspace_bytes,
                                int B, int H, int W, pfk_stream_t stream) {
  if (!up_args_ok({flow, mask, grad_out, grad_mask, grad_flow, workspace}, B, H, W, mask_ld, flow_ld, true)) return PFK_ERR_BAD_ARG;
  if (grad_mask_ld < 576) return PFK_ERR_BAD_ARG;
  if (workspace_bytes < pfk_convex_upsample_bwd_workspace_bytes(B, H, W)) return PFK_ERR_BAD_ARG;
  const long long M = (long long)B * H * W;
  unsigned blocks, gather_blocks;
  if (!up_grid(M, 4, blocks) || !up_grid(M * 2, 256, gather_blocks)) return PFK_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(workspace);
  hipLaunchKernelGGL(convex_upsample_bwd_kernel, dim3(blocks), dim3(256), 0, st, flow, flow_ld, mask, mask_ld, grad_out, grad_mask,
                     grad_mask_ld, part, M, H, W);
  hipLaunchKernelGGL(convex_upsample_bwd_gather_kernel, dim3(gather_blocks), dim3(256), 0, st, part, 2, grad_flow, 0, nullptr, 0, M, H, W);
  return pfk_launch_status();
}

long long pfk_convex_upsample2_bwd_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return (long long)B * H * W * 18 * (long long)sizeof(float);
}

int pfk_convex_upsample2_bwd_f32(const float* flow, int flow_ld, const float* mask, int mask_ld, const float* grad_out,
                                 float* grad_mask, int grad_mask_ld, float* grad_flow, int grad_flow_ld, void* workspace,
                                 long long workspace_bytes, int B, int H, int W, pfk_stream_t stream) {
  if (!up_args_ok({flow, mask, grad_out, grad_mask, grad_flow, workspace}, B, H, W, mask_ld, flow_ld, true, 36)) return PFK_ERR_BAD_ARG;
  if (grad_mask_ld < 36 || !(grad_flow_ld >= 2 || grad_flow_ld == 0)) return PFK_ERR_BAD_ARG;
  if (workspace_bytes < pfk_convex_upsample2_bwd_workspace_bytes(B, H, W)) return PFK_ERR_BAD_ARG;
  const long long M = (long long)B * H * W;
  unsigned blocks, gather_blocks;
  if (!up_grid(M, 32, blocks) || !up_grid(M * 2, 256, gather_blocks)) return PFK_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(workspace);
  const bool vec = pfk_aligned<8>(mask) && (mask_ld & 1) == 0 && pfk_aligned<8>(grad_mask) && (grad_mask_ld & 1) == 0 &&
                   pfk_aligned<8>(grad_out);
  // as the forward: one wave of 32 pixels per block (these grids are a few thousand pixels; 64 against 256 threads measured
  // within the spread there, and small blocks spread a small grid over more CUs)
  hipLaunchKernelGGL(vec ? convex_upsample2_bwd_kernel<true> : convex_upsample2_bwd_kernel<false>, dim3(blocks), dim3(64), 0, st, flow,
                     flow_ld, mask, mask_ld, grad_out, grad_mask, grad_mask_ld, part, M, H, W);
  hipLaunchKernelGGL(convex_upsample_bwd_gather_kernel, dim3(gather_blocks), dim3(256), 0, st, part, 2, grad_flow, grad_flow_ld, nullptr, 0,
                     M, H, W);
  return pfk_launch_status();
}

long long pfk_convex_upsample_info_bwd_workspace_bytes(int B, int H, int W, int n_info) {
  if (B <= 0 || H <= 0 || W <= 0 || n_info < 0 || n_info > UP_MAX_INFO) return 0;
  return (long long)B * H * W * 9 * (2 + n_info) * (long long)sizeof(float);
}

int pfk_convex_upsample_info_bwd_pm_f32(const float* flow_pm, int flow_ld, const float* info_pm, int info_ld, int n_info,
                                        const float* mask, int mask_ld, const float* grad_flow_up, const float* grad_info_up,
                                        float* grad_mask, int grad_mask_ld, float* grad_flow_pm, int grad_flow_ld, float* grad_info_pm,
                                        int grad_info_ld, void* workspace, long long workspace_bytes, int B, int H, int W,
                                        pfk_stream_t stream) {
  if (!up_args_ok({flow_pm, mask, grad_flow_up, grad_mask, grad_flow_pm, workspace}, B, H, W, mask_ld, flow_ld)) return PFK_ERR_BAD_ARG;
  if (n_info < 0 || n_info > UP_MAX_INFO) return PFK_ERR_BAD_ARG;
  if (n_info > 0 && (!info_pm || !grad_info_pm || info_ld < n_info || grad_info_ld < n_info)) return PFK_ERR_BAD_ARG;
  if (grad_flow_ld < 2 || grad_mask_ld < 576) return PFK_ERR_BAD_ARG;
  if (workspace_bytes < pfk_convex_upsample_info_bwd_workspace_bytes(B, H, W, n_info)) return PFK_ERR_BAD_ARG;
  if (!pfk_aligned16(mask) || (mask_ld & 3) || !pfk_aligned16(grad_mask) || (grad_mask_ld & 3) || !pfk_aligned16(grad_flow_up) ||
      !pfk_aligned16(grad_info_up))
    return PFK_ERR_ALIGNMENT;
  const long long M = (long long)B * H * W;
  const int C = 2 + n_info;
  unsigned blocks, gather_blocks;
  if (!up_grid(M, 16, blocks) || !up_grid(M * C, 256, gather_blocks)) return PFK_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(workspace);
#define PFK_UPB_CASE(NI)                                                                                                          \
  case NI:                                                                                                                         \
    hipLaunchKernelGGL(convex_upsample_info_bwd_kernel<NI>, dim3(blocks), dim3(256), 0, st, flow_pm, flow_ld, info_pm, info_ld, mask, \
                       mask_ld, grad_flow_up, grad_info_up, grad_mask, grad_mask_ld, part, M, H, W);                               \
    break;
  switch (n_info) {
    PFK_UPB_CASE(0) PFK_UPB_CASE(1) PFK_UPB_CASE(2) PFK_UPB_CASE(3) PFK_UPB_CASE(4)
    PFK_UPB_CASE(5) PFK_UPB_CASE(6) PFK_UPB_CASE(7) PFK_UPB_CASE(8)
  }
#undef PFK_UPB_CASE
  hipLaunchKernelGGL(convex_upsample_bwd_gather_kernel, dim3(gather_blocks), dim3(256), 0, st, part, C, grad_flow_pm, grad_flow_ld,
                     grad_info_pm, grad_info_ld, M, H, W);
  return pfk_launch_status();
}

}  // extern "C"
