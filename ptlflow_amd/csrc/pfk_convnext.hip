// SEA-RAFT's ConvNeXt block (ptlflow/models/sea_raft/layer.py:54-83): the depthwise k x k convolution fused with the channel
// LayerNorm that follows it (pfk_dwconv_layernorm_f32, include/pfk.h).  The two 1x1 "Linear" layers of the block, its GELU, layer
// scale and residual are implicit GEMMs on pfk_conv2d_f32 (PFK_EPI_LINEAR_GELU / LINEAR with a residual).
//
// Bandwidth-bound: per pixel C floats in, C floats out.  A block owns a TY x TX tile of output pixels and ALL their channels:
//   * channel chunks of CC: the (TY+k-1) x (TX+k-1) halo of the chunk and its k*k weights are staged in LDS (a pixel row piece is
//     read once per block from memory; neighbouring blocks' halo overlap comes from L2), every thread then forms one
//     (pixel, four channels) output from LDS and parks it in the block's [TY*TX][C] output tile, also in LDS;
//   * after the last chunk each wave normalises eight pixels: mean and biased variance of the pixel's C values (two passes over
//     the LDS row, wave reductions), then (x - mean) * rstd * weight + bias straight to `out`.
// Nothing but the final rows goes back to memory: one read, one write per element.
#include "pfk_launch.h"

namespace {

constexpr int DW_TY = 4, DW_TX = 8;       // output tile: 32 pixels, 224 blocks for a batch-1 55 x 128 grid
constexpr int DW_PIX = DW_TY * DW_TX;
constexpr int DW_CC = 32;                 // channels per staged chunk: 8 float4 groups x 32 pixels = one item per thread
constexpr int DW_G = DW_CC / 4;
constexpr int DW_THREADS = 256;
static_assert(DW_PIX * DW_G == DW_THREADS, "one (pixel, float4) item per thread and chunk");
constexpr int DW_MAX_C = 512;

// TRAIN (pfk_dwconv_layernorm_train_f32): the same arithmetic in the same order — `out` has the same bits — and the normalised value
// (u - mean) * rstd goes to `xhat`, the pixel's rstd to `rstd_out`: what pfk_layernorm_bwd_f32 reads.
template <int K, bool TRAIN = false>
__global__ __launch_bounds__(DW_THREADS) void dwconv_ln_kernel(const float* __restrict__ in, int in_ld, const float* __restrict__ dw_w,
                                                               const float* __restrict__ dw_b, const float* __restrict__ ln_w,
                                                               const float* __restrict__ ln_b, float eps, float* __restrict__ out,
                                                               int out_ld, int H, int W, int C, float* __restrict__ xhat = nullptr,
                                                               int xhat_ld = 0, float* __restrict__ rstd_out = nullptr) {
  constexpr int R = K / 2, HY = DW_TY + K - 1, HX = DW_TX + K - 1;
  __shared__ f32x4 halo[HY * HX * DW_G];          // [halo pixel][group]: 17.5 KB at k = 7
  __shared__ f32x4 wts[K * K * DW_G];             // [tap][group]
  extern __shared__ float tile[];                 // [DW_PIX][C + 4] (+4: the float4 stores of one wave spread over the banks)
  const int CP = C + 4;
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * DW_TX, y0 = blockIdx.y * DW_TY;
  const long long img = (long long)blockIdx.z * H * W;
  const int q = tid / DW_G, g = tid % DW_G;       // compute item: output pixel q of the tile, channels 4g .. 4g+3 of the chunk
  const int qy = q / DW_TX, qx = q % DW_TX;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int c0 = 0; c0 < C; c0 += DW_CC) {
    const int cn = (C - c0) < DW_CC ? (C - c0) : DW_CC;     // a multiple of 4
    __syncthreads();                                          // the previous chunk's LDS reads are done
    for (int i = tid; i < HY * HX * DW_G; i += DW_THREADS) {
      const int hp = i / DW_G, gg = i % DW_G;
      const int hy = hp / HX, hx = hp - hy * HX;
      const int yy = y0 + hy - R, xx = x0 + hx - R;
      f32x4 v = zero;
      if (gg * 4 < cn && (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W)
        v = *reinterpret_cast<const f32x4*>(in + (img + (long long)yy * W + xx) * in_ld + c0 + gg * 4);
      halo[i] = v;
    }
    for (int i = tid; i < K * K * DW_G; i += DW_THREADS) {
      const int t = i / DW_G, gg = i % DW_G;
      f32x4 v = zero;
      if (gg * 4 < cn) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = dw_w[(long long)(c0 + gg * 4 + e) * (K * K) + t];
      }
      wts[i] = v;
    }
    __syncthreads();
    if (g * 4 < cn) {
      f32x4 acc = zero;
      if (dw_b != nullptr) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = dw_b[c0 + g * 4 + e];
      }
#pragma unroll
      for (int ky = 0; ky < K; ++ky) {
#pragma unroll
        for (int kx = 0; kx < K; ++kx) acc += halo[((qy + ky) * HX + qx + kx) * DW_G + g] * wts[(ky * K + kx) * DW_G + g];
      }
      *reinterpret_cast<f32x4*>(tile + q * CP + c0 + g * 4) = acc;
    }
  }
  __syncthreads();
  // LayerNorm: wave wv normalises tile pixels wv*8 .. wv*8+7; lane holds channels lane + 64 t
  const int lane = tid & 63, wv = tid >> 6;
  constexpr int NT = DW_MAX_C / 64;
  const float inv_c = 1.0f / (float)C;
  for (int j = 0; j < DW_PIX / (DW_THREADS / 64); ++j) {
    const int qq = wv * (DW_PIX / (DW_THREADS / 64)) + j;
    const int y = y0 + qq / DW_TX, x = x0 + qq % DW_TX;
    if (y >= H || x >= W) continue;                            // wave-uniform
    const float* row = tile + qq * CP;
    float v[NT];
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int c = lane + 64 * t;
      v[t] = c < C ? row[c] : 0.f;
      s += v[t];
    }
    const float mean = wave_sum(s) * inv_c;
    float s2 = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int c = lane + 64 * t;
      const float d = v[t] - mean;
      if (c < C) s2 += d * d;
    }
    const float rstd = 1.0f / sqrtf(wave_sum(s2) * inv_c + eps);
    float* orow = out + (img + (long long)y * W + x) * out_ld;
    if constexpr (TRAIN) {
      float* xrow = xhat + (img + (long long)y * W + x) * xhat_ld;
      if (lane == 0) rstd_out[img + (long long)y * W + x] = rstd;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int c = lane + 64 * t;
        if (c < C) {
          const float xh = (v[t] - mean) * rstd;
          xrow[c] = xh;
          orow[c] = xh * ln_w[c] + ln_b[c];
        }
      }
    } else {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int c = lane + 64 * t;
        if (c < C) orow[c] = (v[t] - mean) * rstd * ln_w[c] + ln_b[c];
      }
    }
  }
}

template <int K, bool TRAIN = false>
int launch_dwconv_ln(const float* in, int in_ld, const float* dw_w, const float* dw_b, const float* ln_w, const float* ln_b, float eps,
                     float* out, int out_ld, int B, int H, int W, int C, hipStream_t st, float* xhat = nullptr, int xhat_ld = 0,
                     float* rstd = nullptr) {
  const size_t smem = (size_t)DW_PIX * (C + 4) * sizeof(float);
  constexpr size_t limit = (size_t)DW_PIX * (DW_MAX_C + 4) * sizeof(float);      // raised once for every C, launched with this C's bytes
  dim3 grid((unsigned)((W + DW_TX - 1) / DW_TX), (unsigned)((H + DW_TY - 1) / DW_TY), (unsigned)B);
  return pfk_launch_lds<dwconv_ln_kernel<K, TRAIN>, limit>(grid, dim3(DW_THREADS), smem, st, in, in_ld, dw_w, dw_b, ln_w, ln_b, eps, out, out_ld,
                                                           H, W, C, xhat, xhat_ld, rstd);
}

// ---- the bf16 twin (pfk_dwconv_layernorm_b16): bf16 rows in and out, fp32 arithmetic -------------------------------------------
// A block owns a BT_TY x BT_TX = 4 x 8 tile and all its channels.  Per 64-channel chunk the halo (bf16, 128 B per pixel) and the chunk's
// k*k weights (fp32) are staged in LDS; thread (strip s, pair j) then forms a strip of BT_PX = 4 consecutive output pixels of one tile
// row for channels 2j, 2j+1 as a sliding window: per filter row it reads BT_PX + k - 1 halo pairs and k weight pairs once and does
// BT_PX * k pair-FMAs with them (the fp32 kernel reads one halo value and one weight per FMA).  The pre-norm values stay in registers
// (acc[chunk][pixel]: at most 8 chunks x 4 pixels x 2 channels = 64 floats): the 32 lanes of a half-wave share a strip, so the
// LayerNorm's two reductions (mean, then the biased variance about it) are xor-shuffles inside the half-wave — no output tile in LDS.
constexpr int BT_TY = 4, BT_TX = 8, BT_PX = 4;
constexpr int BT_CC = 64;                 // channels per staged chunk: 32 pairs
constexpr int BT_NCH = DW_MAX_C / BT_CC;  // 8
constexpr int BT_THREADS = 256;           // 8 strips (2 per tile row) x 32 pairs
static_assert((BT_TY * BT_TX / BT_PX) * (BT_CC / 2) == BT_THREADS, "one (strip, channel pair) item per thread and chunk");
// TRAIN (pfk_dwconv_layernorm_train_b16): the same arithmetic in the same order — `out` has the same bits — and the fp32 normalised
// value (u - mean) * rstd goes to `xhat` rounded once, the pixel's fp32 rstd to `rstd_out`: what pfk_layernorm_bwd_b16 reads.
template <int K, bool TRAIN = false>
__global__ __launch_bounds__(BT_THREADS) void dwconv_ln_b16_kernel(const __bf16* __restrict__ in, int in_ld, const float* __restrict__ dw_w,
                                                                   const float* __restrict__ dw_b, const float* __restrict__ ln_w,
                                                                   const float* __restrict__ ln_b, float eps, __bf16* __restrict__ out,
                                                                   int out_ld, int H, int W, int C, __bf16* __restrict__ xhat = nullptr,
                                                                   int xhat_ld = 0, float* __restrict__ rstd_out = nullptr) {
  constexpr int R = K / 2, HY = BT_TY + K - 1, HX = BT_TX + K - 1, KK = K * K, WIN = BT_PX + K - 1;
  __shared__ __attribute__((aligned(16))) __bf16 halo[HY * HX * BT_CC];   // [halo pixel][64 channels]: 17.5 KB at k = 7
  __shared__ __attribute__((aligned(16))) float wts[KK * BT_CC];          // [tap][64 channels]: 12.25 KB at k = 7
  const int tid = threadIdx.x, lane = tid & 63;
  const int j = lane & 31;                                   // channel pair of the chunk
  const int s = (tid >> 6) * 2 + (lane >> 5);                // strip: tile row s / 2, columns (s % 2) * 4 .. + 3
  const int ry = s >> 1, rx = (s & 1) * BT_PX;
  const int x0 = blockIdx.x * BT_TX, y0 = blockIdx.y * BT_TY;
  const long long img = (long long)blockIdx.z * H * W;
  const unsigned* hw32 = reinterpret_cast<const unsigned*>(halo);
  f32x2 acc[BT_NCH][BT_PX];
#pragma unroll
  for (int ch = 0; ch < BT_NCH; ++ch) {
    const int c0 = ch * BT_CC;
    if (c0 < C) {                                            // block-uniform
      const int cn = (C - c0) < BT_CC ? (C - c0) : BT_CC;    // a multiple of 8
      __syncthreads();                                       // the previous chunk's LDS reads are done
      for (int i = tid; i < HY * HX * (BT_CC / 8); i += BT_THREADS) {
        const int hp = i >> 3, g = i & 7;
        const int hy = hp / HX, hx = hp - hy * HX;
        const int yy = y0 + hy - R, xx = x0 + hx - R;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};                        // 16 bytes = eight bf16 zeros
        if (g * 8 < cn && (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W)
          v = *reinterpret_cast<const f32x4*>(in + (img + (long long)yy * W + xx) * in_ld + c0 + g * 8);
        *reinterpret_cast<f32x4*>(halo + hp * BT_CC + g * 8) = v;
      }
      for (int i = tid; i < KK * BT_CC; i += BT_THREADS) {    // coalesced global reads: [channel][tap] -> [tap][channel]
        const int c = i / KK, t = i - c * KK;
        wts[t * BT_CC + c] = c < cn ? dw_w[(long long)c0 * KK + i] : 0.f;
      }
      __syncthreads();
      f32x2 b = {0.f, 0.f};
      if (dw_b != nullptr && 2 * j < cn) b = f32x2{dw_b[c0 + 2 * j], dw_b[c0 + 2 * j + 1]};
#pragma unroll
      for (int o = 0; o < BT_PX; ++o) acc[ch][o] = b;
      if (2 * j < cn) {
#pragma unroll 1
        for (int ky = 0; ky < K; ++ky) {
          f32x2 w[K];
#pragma unroll
          for (int kx = 0; kx < K; ++kx) w[kx] = *reinterpret_cast<const f32x2*>(wts + (ky * K + kx) * BT_CC + 2 * j);
          const unsigned* hrow = hw32 + ((ry + ky) * HX + rx) * (BT_CC / 2) + j;
#pragma unroll
          for (int i = 0; i < WIN; ++i) {
            const f32x2 h = widen2(hrow[i * (BT_CC / 2)]);
#pragma unroll
            for (int o = 0; o < BT_PX; ++o) {
              const int kx = i - o;
              if (kx >= 0 && kx < K) acc[ch][o] += h * w[kx];
            }
          }
        }
      }
    }
  }
  // LayerNorm of the strip's pixels: this thread's channels, then the half-wave; two passes over the registers
  const float inv_c = 1.0f / (float)C;
  float mean[BT_PX], rstd[BT_PX];
#pragma unroll
  for (int o = 0; o < BT_PX; ++o) {
    float sum = 0.f;
#pragma unroll
    for (int ch = 0; ch < BT_NCH; ++ch)
      if (ch * BT_CC + 2 * j < C) sum += acc[ch][o].x + acc[ch][o].y;
    mean[o] = wave_sum<32>(sum) * inv_c;                      // over the 32 lanes of this lane's half-wave
  }
#pragma unroll
  for (int o = 0; o < BT_PX; ++o) {
    float s2 = 0.f;
#pragma unroll
    for (int ch = 0; ch < BT_NCH; ++ch) {
      if (ch * BT_CC + 2 * j < C) {
        const float dx = acc[ch][o].x - mean[o], dy = acc[ch][o].y - mean[o];
        s2 += dx * dx + dy * dy;
      }
    }
    rstd[o] = 1.0f / sqrtf(wave_sum<32>(s2) * inv_c + eps);
  }
  const int y = y0 + ry;
  if (y >= H) return;
  if constexpr (TRAIN) {
    if (j == 0) {                                              // one lane per strip
#pragma unroll
      for (int o = 0; o < BT_PX; ++o)
        if (x0 + rx + o < W) rstd_out[img + (long long)y * W + x0 + rx + o] = rstd[o];
    }
  }
#pragma unroll
  for (int ch = 0; ch < BT_NCH; ++ch) {
    const int c = ch * BT_CC + 2 * j;
    if (c >= C) continue;
    const float w0 = ln_w[c], w1 = ln_w[c + 1], b0 = ln_b[c], b1 = ln_b[c + 1];
#pragma unroll
    for (int o = 0; o < BT_PX; ++o) {
      const int x = x0 + rx + o;
      if (x >= W) continue;
      const float xh0 = (acc[ch][o].x - mean[o]) * rstd[o], xh1 = (acc[ch][o].y - mean[o]) * rstd[o];
      bf16x2 v;                                                  // store_row<2> written out: through it the whole kernel schedules differently
      v[0] = (__bf16)(xh0 * w0 + b0);
      v[1] = (__bf16)(xh1 * w1 + b1);
      *reinterpret_cast<bf16x2*>(out + (img + (long long)y * W + x) * out_ld + c) = v;
      if constexpr (TRAIN) {
        bf16x2 n;
        n[0] = (__bf16)xh0;
        n[1] = (__bf16)xh1;
        *reinterpret_cast<bf16x2*>(xhat + (img + (long long)y * W + x) * xhat_ld + c) = n;
      }
    }
  }
}

template <int K, bool TRAIN = false>
int launch_dwconv_ln_b16(const __bf16* in, int in_ld, const float* dw_w, const float* dw_b, const float* ln_w, const float* ln_b, float eps,
                         __bf16* out, int out_ld, int B, int H, int W, int C, hipStream_t st, __bf16* xhat = nullptr, int xhat_ld = 0,
                         float* rstd = nullptr) {
  dim3 grid((unsigned)((W + BT_TX - 1) / BT_TX), (unsigned)((H + BT_TY - 1) / BT_TY), (unsigned)B);
  hipLaunchKernelGGL((dwconv_ln_b16_kernel<K, TRAIN>), grid, dim3(BT_THREADS), 0, st, in, in_ld, dw_w, dw_b, ln_w, ln_b, eps, out, out_ld, H, W,
                     C, xhat, xhat_ld, rstd);
  return pfk_launch_status();
}

// [b, e) of two row ranges intersect
bool ranges_overlap(const void* ab, const void* ae, const void* bb, const void* be) {
  return static_cast<const char*>(ab) < static_cast<const char*>(be) && static_cast<const char*>(bb) < static_cast<const char*>(ae);
}

}  // namespace

extern "C" {

int pfk_dwconv_layernorm_f32(const float* in, int in_ld, const float* dw_weight, const float* dw_bias, const float* ln_weight,
                             const float* ln_bias, float eps, float* out, int out_ld, int B, int H, int W, int C, int k,
                             pfk_stream_t stream) {
  if (!in || !dw_weight || !ln_weight || !ln_bias || !out || B <= 0 || H <= 0 || W <= 0 || C < 4 || in_ld < C || out_ld < C)
    return PFK_ERR_BAD_ARG;
  if (k < 1 || !(k & 1)) return PFK_ERR_BAD_ARG;
  if (k > 7 || C > DW_MAX_C || B > 65535 || (H + DW_TY - 1) / DW_TY > 65535) return PFK_ERR_UNSUPPORTED;
  if ((C & 3) || (in_ld & 3) || !pfk_aligned16(in)) return PFK_ERR_ALIGNMENT;
  const long long M = (long long)B * H * W;
  if (!pfk_fits32(M)) return PFK_ERR_UNSUPPORTED;
  // `out` must not overlap the input rows (other blocks still read the halo of pixels this block has written)
  const char* ib = reinterpret_cast<const char*>(in);
  const char* ie = reinterpret_cast<const char*>(in + (M - 1) * in_ld + C);
  const char* ob = reinterpret_cast<const char*>(out);
  const char* oe = reinterpret_cast<const char*>(out + (M - 1) * out_ld + C);
  if (ob < ie && ib < oe) return PFK_ERR_BAD_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (k) {
    case 1: return launch_dwconv_ln<1>(in, in_ld, dw_weight, dw_bias, ln_weight, ln_bias, eps, out, out_ld, B, H, W, C, st);
    case 3: return launch_dwconv_ln<3>(in, in_ld, dw_weight, dw_bias, ln_weight, ln_bias, eps, out, out_ld, B, H, W, C, st);
    case 5: return launch_dwconv_ln<5>(in, in_ld, dw_weight, dw_bias, ln_weight, ln_bias, eps, out, out_ld, B, H, W, C, st);
    default: return launch_dwconv_ln<7>(in, in_ld, dw_weight, dw_bias, ln_weight, ln_bias, eps, out, out_ld, B, H, W, C, st);
  }
}

int pfk_dwconv_layernorm_train_f32(const float* in, int in_ld, const float* dw_weight, const float* dw_bias, const float* ln_weight,
                                   const float* ln_bias, float eps, float* out, int out_ld, float* xhat, int xhat_ld, float* rstd,
                                   int B, int H, int W, int C, int k, pfk_stream_t stream) {
  if (!in || !dw_weight || !ln_weight || !ln_bias || !out || !xhat || !rstd || B <= 0 || H <= 0 || W <= 0 || C < 4 || in_ld < C ||
      out_ld < C || xhat_ld < C)
    return PFK_ERR_BAD_ARG;
  if (k < 1 || !(k & 1) || k > 7 || C > DW_MAX_C) return PFK_ERR_BAD_ARG;
  if (B > 65535 || (H + DW_TY - 1) / DW_TY > 65535) return PFK_ERR_UNSUPPORTED;
  if ((C & 3) || (in_ld & 3) || !pfk_aligned16(in)) return PFK_ERR_ALIGNMENT;
  const long long M = (long long)B * H * W;
  if (!pfk_fits32(M)) return PFK_ERR_UNSUPPORTED;
  // neither output may overlap the input rows (other blocks still read the halo of pixels this block has written)
  const char* ib = reinterpret_cast<const char*>(in);
  const char* ie = reinterpret_cast<const char*>(in + (M - 1) * in_ld + C);
  const char* ob = reinterpret_cast<const char*>(out);
  const char* oe = reinterpret_cast<const char*>(out + (M - 1) * out_ld + C);
  const char* xb = reinterpret_cast<const char*>(xhat);
  const char* xe = reinterpret_cast<const char*>(xhat + (M - 1) * xhat_ld + C);
  if ((ob < ie && ib < oe) || (xb < ie && ib < xe) || (xb < oe && ob < xe)) return PFK_ERR_BAD_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (k) {
    case 1: return launch_dwconv_ln<1, true>(in, in_ld, dw_weight, dw_bias, ln_weight, ln_bias, eps, out, out_ld, B, H, W, C, st, xhat, xhat_ld, rstd);
    case 3: return launch_dwconv_ln<3, true>(in, in_ld, dw_weight, dw_bias, ln_weight, ln_bias, eps, out, out_ld, B, H, W, C, st, xhat, xhat_ld, rstd);
    case 5: return launch_dwconv_ln<5, true>(in, in_ld, dw_weight, dw_bias, ln_weight, ln_bias, eps, out, out_ld, B, H, W, C, st, xhat, xhat_ld, rstd);
    default: return launch_dwconv_ln<7, true>(in, in_ld, dw_weight, dw_bias, ln_weight, ln_bias, eps, out, out_ld, B, H, W, C, st, xhat, xhat_ld, rstd);
  }
}

int pfk_dwconv_layernorm_b16(const void* in_bf16, int in_ld, const float* dw_weight, const float* dw_bias, const float* ln_weight,
                             const float* ln_bias, float eps, void* out_bf16, int out_ld, int B, int H, int W, int C, int k,
                             pfk_stream_t stream) {
  if (!in_bf16 || !dw_weight || !ln_weight || !ln_bias || !out_bf16 || B <= 0 || H <= 0 || W <= 0 || C < 8 || in_ld < C || out_ld < C)
    return PFK_ERR_BAD_ARG;
  if (k < 1 || !(k & 1) || k > 7) return PFK_ERR_BAD_ARG;
  if (C > DW_MAX_C || B > 65535 || (H + BT_TY - 1) / BT_TY > 65535) return PFK_ERR_UNSUPPORTED;
  if ((C & 7) || (in_ld & 7) || (out_ld & 7) || !pfk_aligned16(in_bf16) || !pfk_aligned16(out_bf16)) return PFK_ERR_ALIGNMENT;
  const long long M = (long long)B * H * W;
  if (!pfk_fits32(M)) return PFK_ERR_UNSUPPORTED;
  const __bf16* in = static_cast<const __bf16*>(in_bf16);
  __bf16* out = static_cast<__bf16*>(out_bf16);
  // `out` must not overlap the input rows (other blocks still read the halo of pixels this block has written)
  const char* ib = reinterpret_cast<const char*>(in);
  const char* ie = reinterpret_cast<const char*>(in + (M - 1) * in_ld + C);
  const char* ob = reinterpret_cast<const char*>(out);
  const char* oe = reinterpret_cast<const char*>(out + (M - 1) * out_ld + C);
  if (ob < ie && ib < oe) return PFK_ERR_BAD_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (k) {
    case 1: return launch_dwconv_ln_b16<1>(in, in_ld, dw_weight, dw_bias, ln_weight, ln_bias, eps, out, out_ld, B, H, W, C, st);
    case 3: return launch_dwconv_ln_b16<3>(in, in_ld, dw_weight, dw_bias, ln_weight, ln_bias, eps, out, out_ld, B, H, W, C, st);
    case 5: return launch_dwconv_ln_b16<5>(in, in_ld, dw_weight, dw_bias, ln_weight, ln_bias, eps, out, out_ld, B, H, W, C, st);
    default: return launch_dwconv_ln_b16<7>(in, in_ld, dw_weight, dw_bias, ln_weight, ln_bias, eps, out, out_ld, B, H, W, C, st);
  }
}

int pfk_dwconv_layernorm_train_b16(const void* in_bf16, int in_ld, const float* dw_weight, const float* dw_bias, const float* ln_weight,
                                   const float* ln_bias, float eps, void* out_bf16, int out_ld, void* xhat_bf16, int xhat_ld, float* rstd,
                                   int B, int H, int W, int C, int k, pfk_stream_t stream) {
  if (!in_bf16 || !dw_weight || !ln_weight || !ln_bias || !out_bf16 || !xhat_bf16 || !rstd || B <= 0 || H <= 0 || W <= 0 || C < 8 ||
      in_ld < C || out_ld < C || xhat_ld < C)
    return PFK_ERR_BAD_ARG;
  if (k < 1 || !(k & 1) || k > 7 || C > DW_MAX_C) return PFK_ERR_BAD_ARG;
  if (B > 65535 || (H + BT_TY - 1) / BT_TY > 65535) return PFK_ERR_UNSUPPORTED;
  if ((C & 7) || (in_ld & 7) || (out_ld & 7) || (xhat_ld & 7) || !pfk_aligned16(in_bf16) || !pfk_aligned16(out_bf16) ||
      !pfk_aligned16(xhat_bf16) || !pfk_aligned<4>(rstd))
    return PFK_ERR_ALIGNMENT;
  const long long M = (long long)B * H * W;
  if (!pfk_fits32(M)) return PFK_ERR_UNSUPPORTED;
  const __bf16* in = static_cast<const __bf16*>(in_bf16);
  __bf16* out = static_cast<__bf16*>(out_bf16);
  __bf16* xhat = static_cast<__bf16*>(xhat_bf16);
  // no output may overlap the input rows (other blocks still read the halo of pixels this block has written) or another output
  const void *ie = in + (M - 1) * in_ld + C, *oe = out + (M - 1) * out_ld + C, *xe = xhat + (M - 1) * xhat_ld + C, *re = rstd + M;
  if (ranges_overlap(out, oe, in, ie) || ranges_overlap(xhat, xe, in, ie) || ranges_overlap(xhat, xe, out, oe) ||
      ranges_overlap(rstd, re, in, ie) || ranges_overlap(rstd, re, out, oe) || ranges_overlap(rstd, re, xhat, xe))
    return PFK_ERR_BAD_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (k) {
    case 1: return launch_dwconv_ln_b16<1, true>(in, in_ld, dw_weight, dw_bias, ln_weight, ln_bias, eps, out, out_ld, B, H, W, C, st, xhat, xhat_ld, rstd);
    case 3: return launch_dwconv_ln_b16<3, true>(in, in_ld, dw_weight, dw_bias, ln_weight, ln_bias, eps, out, out_ld, B, H, W, C, st, xhat, xhat_ld, rstd);
    case 5: return launch_dwconv_ln_b16<5, true>(in, in_ld, dw_weight, dw_bias, ln_weight, ln_bias, eps, out, out_ld, B, H, W, C, st, xhat, xhat_ld, rstd);
    default: return launch_dwconv_ln_b16<7, true>(in, in_ld, dw_weight, dw_bias, ln_weight, ln_bias, eps, out, out_ld, B, H, W, C, st, xhat, xhat_ld, rstd);
  }
}

}  // extern "C"
