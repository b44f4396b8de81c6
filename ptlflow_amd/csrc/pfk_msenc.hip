// K15: the row kernels of the multi-scale GroupNorm encoders (`fnet` / `cnet` of CCMR, CCMR+ and MS-RAFT+: ccmr/extractor.py,
// ms_raft_plus/extractor.py; ptlflow_amd/ms_encoder.py) that are not convolutions, on fp32 pixel-major rows [B*HW][ld]:
//   * GroupNorm statistics with groups of 8 consecutive channels, finished into the per-(image, channel) affine pair
//     scale = rstd * gamma, shift = beta - mean * rstd * gamma;
//   * out = relu?(x * scale + shift) (+ residual, relu?): pfk_norm_apply_f32's pass with that pair in place of mean / rstd;
//   * the bilinear resize between two pyramid levels (align_corners=False, edge taps replicated), upsizing only.
// All three are memory-bound: 16-byte accesses, a thread owns 4 consecutive channels of a row, only channels [0, C) of a row are
// touched.  No atomics, every sum in an order fixed by the shape: the same bits on every run.
#include "pfk_launch.h"

namespace {

constexpr int GN_GROUP = 8;          // channels per group: every GroupNorm of the six encoders
constexpr int GN_CHUNK_ROWS = 256;   // pixels of an image per partial-sum block

// ------------------------------------------------------------------------------------------------------------------
// Statistics, pass 1.  Block (chunk, image): rows [chunk * 256, min(HW, chunk * 256 + 256)) of the image.  A thread owns 4 channels
// (half a group) and every (256 / (C/4))-th row of the chunk, and carries ONE sum and ONE sum of squares in double (an fp32 square
// is exact in double); the block combines its threads through LDS in a fixed order and writes part[which][b][chunk][group].
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void groupnorm_partial_kernel(const float* __restrict__ x, int ld, int C, int HW,
                                                                double* __restrict__ part, long long astride) {
  __shared__ double red[2][256];
  const int b = blockIdx.y, chunk = blockIdx.x, nch = (int)gridDim.x;
  const int tpr = C >> 2, rpi = 256 / tpr;
  const int t = threadIdx.x;
  const int c4 = (t % tpr) * 4, rr = t / tpr;
  const int r0 = chunk * GN_CHUNK_ROWS, r1 = min(HW, r0 + GN_CHUNK_ROWS);
  double s0 = 0., q0 = 0.;
  if (rr < rpi) {
    const float* base = x + (long long)b * HW * ld + c4;
    double s1 = 0., q1 = 0.;      // a second, independent chain: the fp64 adds of one would serialise the loop
    int r = r0 + rr;
    for (; r + rpi < r1; r += 2 * rpi) {
      const f32x4 v0 = load4_widen(base + (long long)r * ld);
      const f32x4 v1 = load4_widen(base + (long long)(r + rpi) * ld);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double d0 = (double)v0[e], d1 = (double)v1[e];
        s0 += d0; q0 = fma(d0, d0, q0);
        s1 += d1; q1 = fma(d1, d1, q1);
      }
    }
    if (r < r1) {
      const f32x4 v = load4_widen(base + (long long)r * ld);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double d = (double)v[e];
        s0 += d; q0 = fma(d, d, q0);
      }
    }
    s0 += s1; q0 += q1;
  }
  red[0][t] = s0;
  red[1][t] = q0;
  __syncthreads();
  const int G = C / GN_GROUP;
  for (int u = t; u < 2 * G; u += 256) {      // [0, G): sums; [G, 2G): sums of squares
    const int which = u >= G, g = u - which * G;
    double s = 0.;
    for (int k = 0; k < rpi; ++k) s += red[which][k * tpr + 2 * g] + red[which][k * tpr + 2 * g + 1];
    part[which * astride + ((long long)b * nch + chunk) * G + g] = s;
  }
}

// Pass 2.  One wave per (image, group): lane l adds chunks l, l + 64, ... in order, the lanes are combined by wave_sum's butterfly;
// mean, var_biased = E[x^2] - mean^2 and rstd = 1 / sqrt(var + eps) in double, then lanes 0..7 write the pair of their channel.
__global__ __launch_bounds__(256) void groupnorm_finish_kernel(const double* __restrict__ part, long long astride, int nch, int C,
                                                               int HW, int BG, float eps, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, float* __restrict__ scale,
                                                               float* __restrict__ shift) {
  const int lane = threadIdx.x & 63;
  const int bg = blockIdx.x * 4 + (threadIdx.x >> 6);      // b * G + g
  if (bg >= BG) return;
  const int G = C / GN_GROUP;
  const int b = bg / G, g = bg - b * G;
  const double* p = part + (long long)b * nch * G + g;
  double s = 0., q = 0.;
  for (int k = lane; k < nch; k += 64) {
    s += p[(long long)k * G];
    q += p[astride + (long long)k * G];
  }
  s = wave_sum(s);
  q = wave_sum(q);
  if (lane < GN_GROUP) {
    const double n = (double)HW * GN_GROUP;
    const double m = s / n;
    double var = q / n - m * m;
    var = var < 0. ? 0. : var;      // rounding may leave a constant group's variance below 0; a NaN stays a NaN
    const double rstd = 1.0 / sqrt(var + (double)eps);
    const int c = g * GN_GROUP + lane;
    const double sc = rstd * (double)gamma[c];
    scale[(long long)b * C + c] = (float)sc;
    shift[(long long)b * C + c] = (float)((double)beta[c] - m * sc);
  }
}

// out = relu?(x * scale + shift) ; [out = relu?(residual + out)]      (float4 per thread; scale / shift [B][C])
__global__ __launch_bounds__(256) void affine_apply_kernel(const float* __restrict__ x, int x_ld, const float* __restrict__ scale,
                                                           const float* __restrict__ shift, const float* __restrict__ residual,
                                                           int res_ld, float* __restrict__ out, int out_ld, long long M, int HW, int C,
                                                           int relu, int relu_after) {
  const int tpr = C >> 2;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long p = idx / tpr;
  if (p >= M) return;
  const int c4 = (int)(idx - p * tpr) * 4;
  const long long sidx = (p / HW) * C + c4;
  const f32x4 a = *reinterpret_cast<const f32x4*>(scale + sidx);
  const f32x4 d = *reinterpret_cast<const f32x4*>(shift + sidx);
  f32x4 v = load4_widen(x + p * x_ld + c4);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    v[e] = fmaf(v[e], a[e], d[e]);
    if (relu) v[e] = (v[e] < 0.f) ? 0.f : v[e];
  }
  if (residual != nullptr) {
    v = load4_widen(residual + p * res_ld + c4) + v;
    if (relu_after) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (v[e] < 0.f) ? 0.f : v[e];
    }
  }
  store4(out + p * out_ld + c4, v);
}

// ------------------------------------------------------------------------------------------------------------------
// Bilinear resize, No >= Ni per axis.  The source coordinate of output o is (o + 0.5) * Ni / No - 0.5 clamped to [0, Ni - 1]: in
// integers n = max(0, (2 o + 1) Ni - No) over 2 No, so the first tap i0 = n / (2 No) and both weights (2 No - rem) / (2 No),
// rem / (2 No) are exact integers divided once — no coordinate is ever rounded (host: 2 No Ni < 2^31, 2 No <= 2^24).  The second
// tap is min(i0 + 1, Ni - 1): past the last source pixel both taps are that pixel, and no tap leaves its image.
// ------------------------------------------------------------------------------------------------------------------
struct axis_tap { int i0, i1; float w0, w1; };
__device__ __forceinline__ axis_tap resize_tap(int o, int Ni, int No) {
  int n = (2 * o + 1) * Ni - No;
  n = n < 0 ? 0 : n;
  const int d = 2 * No;
  int i0 = n / d;
  int rem = n - i0 * d;
  if (i0 >= Ni - 1) { i0 = Ni - 1; rem = 0; }
  axis_tap t;
  t.i0 = i0;
  t.i1 = min(i0 + 1, Ni - 1);
  t.w0 = (float)(d - rem) / (float)d;
  t.w1 = (float)rem / (float)d;
  return t;
}

__global__ __launch_bounds__(256) void resize_bilinear_kernel(const float* __restrict__ in, int in_ld, float* __restrict__ out,
                                                              int out_ld, long long M_out, int Hi, int Wi, int Ho, int Wo, int C) {
  const int tpr = C >> 2;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long p = idx / tpr;
  if (p >= M_out) return;
  const int c4 = (int)(idx - p * tpr) * 4;
  const long long row = p / Wo;                    // b * Ho + oy
  const int ox = (int)(p - row * Wo);
  const long long b = row / Ho;
  const int oy = (int)(row - b * Ho);
  const axis_tap ty = resize_tap(oy, Hi, Ho), tx = resize_tap(ox, Wi, Wo);
  const float* img = in + b * Hi * Wi * in_ld + c4;
  const float* r0 = img + (long long)ty.i0 * Wi * in_ld;
  const float* r1 = img + (long long)ty.i1 * Wi * in_ld;
  const f32x4 v00 = load4_widen(r0 + (long long)tx.i0 * in_ld), v01 = load4_widen(r0 + (long long)tx.i1 * in_ld);
  const f32x4 v10 = load4_widen(r1 + (long long)tx.i0 * in_ld), v11 = load4_widen(r1 + (long long)tx.i1 * in_ld);
  f32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float top = fmaf(v01[e], tx.w1, v00[e] * tx.w0);
    const float bot = fmaf(v11[e], tx.w1, v10[e] * tx.w0);
    v[e] = fmaf(bot, ty.w1, top * ty.w0);
  }
  store4(out + p * out_ld + c4, v);
}

static inline int gn_chunks(int HW) { return (HW + GN_CHUNK_ROWS - 1) / GN_CHUNK_ROWS; }

}  // namespace

extern "C" {

long long pfk_groupnorm_workspace_bytes(int B, int HW, int C) {
  if (B <= 0 || HW <= 0 || C <= 0) return PFK_ERR_BAD_ARG;
  if (C % GN_GROUP) return PFK_ERR_UNSUPPORTED;
  return 2LL * B * gn_chunks(HW) * (C / GN_GROUP) * (long long)sizeof(double);
}

int pfk_groupnorm_stats_f32(const float* x, int ld, int B, int HW, int C, int group_size, const float* gamma, const float* beta,
                            float eps, float* scale, float* shift, void* workspace, long long workspace_bytes, pfk_stream_t stream) {
  if (!x || !gamma || !beta || !scale || !shift || !workspace || B <= 0 || HW <= 0 || C <= 0 || group_size <= 0 || ld < C ||
      !(eps >= 0.f))
    return PFK_ERR_BAD_ARG;
  if (group_size != GN_GROUP || (C % GN_GROUP) || C > 1024) return PFK_ERR_UNSUPPORTED;
  if ((ld & 3) || !pfk_aligned16(x) || !pfk_aligned<4>(gamma) || !pfk_aligned<4>(beta) || !pfk_aligned<4>(scale) ||
      !pfk_aligned<4>(shift) || !pfk_aligned<8>(workspace))
    return PFK_ERR_ALIGNMENT;
  if (workspace_bytes < pfk_groupnorm_workspace_bytes(B, HW, C)) return PFK_ERR_BAD_ARG;
  const int nch = gn_chunks(HW), G = C / GN_GROUP;
  const long long BG = (long long)B * G;
  if (B > 65535 || !pfk_fits_int(BG)) return PFK_ERR_UNSUPPORTED;      // grid.y; b * G + g as an int
  double* part = static_cast<double*>(workspace);            // 2 x [B][nch][G]: sums, sums of squares
  const long long astride = (long long)B * nch * G;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(groupnorm_partial_kernel, dim3((unsigned)nch, (unsigned)B), dim3(256), 0, st, x, ld, C, HW, part, astride);
  hipLaunchKernelGGL(groupnorm_finish_kernel, dim3((unsigned)((BG + 3) / 4)), dim3(256), 0, st, part, astride, nch, C, HW, (int)BG, eps,
                     gamma, beta, scale, shift);
  return pfk_launch_status();
}

int pfk_affine_apply_f32(const float* x, int x_ld, const float* scale, const float* shift, const float* residual, int residual_ld,
                         float* out, int out_ld, int B, int HW, int C, int relu, int relu_after_residual, pfk_stream_t stream) {
  if (!x || !scale || !shift || !out || B <= 0 || HW <= 0 || C <= 0 || x_ld < C || out_ld < C) return PFK_ERR_BAD_ARG;
  if ((C & 3) || (x_ld & 3) || (out_ld & 3) || !pfk_aligned16(x) || !pfk_aligned16(out) || !pfk_aligned16(scale) ||
      !pfk_aligned16(shift))
    return PFK_ERR_ALIGNMENT;
  if (residual && (residual_ld < C || (residual_ld & 3) || !pfk_aligned16(residual))) return PFK_ERR_ALIGNMENT;
  const long long M = (long long)B * HW;
  const long long blocks = (M * (C >> 2) + 255) / 256;
  if (!pfk_fits_int(blocks)) return PFK_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(affine_apply_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), x, x_ld, scale, shift,
                     residual, residual_ld, out, out_ld, M, HW, C, relu, relu_after_residual);
  return pfk_launch_status();
}

int pfk_resize_bilinear_pm_f32(const float* in, int in_ld, float* out, int out_ld, int B, int Hi, int Wi, int Ho, int Wo, int C,
                               pfk_stream_t stream) {
  if (!in || !out || B <= 0 || Hi <= 0 || Wi <= 0 || Ho <= 0 || Wo <= 0 || C <= 0 || in_ld < C || out_ld < C) return PFK_ERR_BAD_ARG;
  if ((C & 3) || (in_ld & 3) || (out_ld & 3) || !pfk_aligned16(in) || !pfk_aligned16(out)) return PFK_ERR_ALIGNMENT;
  if (Ho < Hi || Wo < Wi) return PFK_ERR_UNSUPPORTED;                     // downsizing: another filter (antialias)
  if (!pfk_fits32(2LL * Ho * Hi + Ho) || !pfk_fits32(2LL * Wo * Wi + Wo) || Ho > (1 << 23) || Wo > (1 << 23)) return PFK_ERR_UNSUPPORTED;
  const long long M_out = (long long)B * Ho * Wo;
  const long long blocks = (M_out * (C >> 2) + 255) / 256;
  if (!pfk_fits_int(blocks)) return PFK_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(resize_bilinear_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), in, in_ld, out,
                     out_ld, M_out, Hi, Wi, Ho, Wo, C);
  return pfk_launch_status();
}

}  // extern "C"
