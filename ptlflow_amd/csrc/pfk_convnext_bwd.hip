// Training SEA-RAFT's ConvNeXt block (K12d): the backward of pfk_dwconv_layernorm_train_f32 in two kernels, and the
// exact GELU as a row op with its derivative.  fp32, deterministic: no atomics, every sum over pixels runs in an order fixed by the
// shape (per-block partials in a caller-provided workspace, then a fixed-order reduce).
//
//  * pfk_layernorm_bwd_f32   one wave per pixel row (lane = channel + 64 t, as the forward's statistics): the two per-pixel means are
//    wave reductions; a wave walks rows  wave, wave + #waves, ...  and keeps its columns' dgamma / dbeta sums in registers.
//  * pfk_dwconv_bwd_f32      the forward's geometry — 4 x 8 tiles, 32-channel chunks, halos in LDS — with one block per (slice of
//    tiles, chunk): the chunk's channels are independent of all others, so dx goes straight to memory and the block's weight
//    gradient [32][k*k] stays in registers over all its tiles: a thread owns (four channels, tap) items and walks the tile's 32
//    pixels out of LDS.  One partial [C][k*k + 1] per slice (the + 1: the bias gradient).
//  * pfk_gelu_f32 / pfk_gelu_bwd_f32   float4 per thread over [M][C] rows.
//
// The bf16 entries (K12f: pfk_layernorm_bwd_b16, pfk_dwconv_bwd_b16, pfk_gelu_b16, pfk_gelu_bwd_b16) are the same kernel bodies on the
// element type __bf16: rows are widened to fp32 as they are loaded (exact) and rounded once as they are stored, everything between —
// LDS tiles, sums, partials, the parameter gradients — is the fp32 code.  What differs is how many channels a lane moves at once:
// 16 bytes of a bf16 row (eight channels) in the LayerNorm and GELU kernels, 8 bytes (the (pixel, four channels) item) in the
// depthwise one.
#include "pfk_launch.h"

namespace {

constexpr int CB_TY = 4, CB_TX = 8, CB_PIX = CB_TY * CB_TX;     // pfk_convnext.hip's tile
constexpr int CB_CC = 32, CB_G = CB_CC / 4;
constexpr int CB_THREADS = 256;
static_assert(CB_PIX * CB_G == CB_THREADS, "one (pixel, float4) item per thread");
constexpr int CB_MAX_C = 512;
constexpr int CB_MAX_SLICES = 64;         // blocks per chunk: 64 x 12 chunks at C = 384
constexpr int LN_WAVES = 4;               // waves (= rows in flight) per block
constexpr int LN_MAX_BLOCKS = 1024;
constexpr int LN_RED_PARTS = 4;

// channels per 16-byte row access, and the rule the entries check: C and ld in multiples of it
template <typename T>
constexpr int QUANTUM = 16 / (int)sizeof(T);

// ---------------------------------------------------------------------------------------------------------------- LayerNorm backward
// fp32: lane = channel + 64 t, one float per access (V = 1, NT = 8); bf16: lane l holds channels 8 l .. 8 l + 7, one 16-byte access
// per row (V = 8, NT = 1: 48 lanes at C = 384).  Channel c = (lane + 64 t) V + e either way.
template <typename T>
__global__ __launch_bounds__(LN_WAVES * 64) void layernorm_bwd_kernel(const T* __restrict__ xhat, int xhat_ld,
                                                                      const float* __restrict__ rstd, const float* __restrict__ ln_w,
                                                                      const T* __restrict__ dy, int dy_ld, T* __restrict__ du,
                                                                      int du_ld, float* __restrict__ part, long long M, int C) {
  constexpr int V = sizeof(T) == 4 ? 1 : 8;
  constexpr int NT = CB_MAX_C / (64 * V);
  __shared__ float red[LN_WAVES][2][CB_MAX_C];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float inv_c = 1.0f / (float)C;
  float gam[NT][V], dg[NT][V], db[NT][V];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const int c = (lane + 64 * t) * V + e;
      gam[t][e] = c < C ? ln_w[c] : 0.f;
      dg[t][e] = 0.f;
      db[t][e] = 0.f;
    }
  }
  const long long step = (long long)gridDim.x * LN_WAVES;
  for (long long p = (long long)blockIdx.x * LN_WAVES + wv; p < M; p += step) {
    const T* xr = xhat + p * xhat_ld;
    const T* dr = dy + p * dy_ld;
    float xh[NT][V], g[NT][V];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int c = (lane + 64 * t) * V;               // C % V == 0: the V channels are real or pad together
      float d[V];
#pragma unroll
      for (int e = 0; e < V; ++e) d[e] = xh[t][e] = 0.f;
      if (c < C) {
        load_row<V>(dr + c, d);
        load_row<V>(xr + c, xh[t]);
      }
#pragma unroll
      for (int e = 0; e < V; ++e) {
        g[t][e] = d[e] * gam[t][e];
        s1 += g[t][e];
        s2 += g[t][e] * xh[t][e];
        dg[t][e] += d[e] * xh[t][e];
        db[t][e] += d[e];
      }
    }
    const float m1 = wave_sum(s1) * inv_c, m2 = wave_sum(s2) * inv_c;
    const float rs = rstd[p];
    T* o = du + p * du_ld;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int c = (lane + 64 * t) * V;
      if (c < C) {
        float u[V];
#pragma unroll
        for (int e = 0; e < V; ++e) u[e] = rs * (g[t][e] - m1 - xh[t][e] * m2);
        store_row<V>(o + c, u);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int e = 0; e < V; ++e) {
      red[wv][0][(lane + 64 * t) * V + e] = dg[t][e];
      red[wv][1][(lane + 64 * t) * V + e] = db[t][e];
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * C; i += LN_WAVES * 64) {
    const int which = i / C, c = i - which * C;
    float s = red[0][which][c];
#pragma unroll
    for (int w = 1; w < LN_WAVES; ++w) s += red[w][which][c];
    part[(long long)blockIdx.x * 2 * C + i] = s;
  }
}

// out[j] = sum over the n partial rows of part[s][j], j < cols: 64 columns per block, the rows cut into LN_RED_PARTS runs that are
// summed in order and then combined in order
__global__ __launch_bounds__(LN_RED_PARTS * 64) void column_reduce_kernel(const float* __restrict__ part, int n, int cols,
                                                                          float* __restrict__ out0, float* __restrict__ out1, int split) {
  __shared__ float red[LN_RED_PARTS][64];
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + lane;
  const int per = (n + LN_RED_PARTS - 1) / LN_RED_PARTS;
  float s = 0.f;
  if (j < cols) {
    const int e = (q + 1) * per < n ? (q + 1) * per : n;
    for (int r = q * per; r < e; ++r) s += part[(long long)r * cols + j];
  }
  red[q][lane] = s;
  __syncthreads();
  if (q == 0 && j < cols) {
    float v = red[0][lane];
#pragma unroll
    for (int w = 1; w < LN_RED_PARTS; ++w) v += red[w][lane];
    if (j < split) out0[j] = v;
    else out1[j - split] = v;
  }
}

int ln_bwd_blocks(long long M) {
  const long long b = (M + LN_WAVES - 1) / LN_WAVES;
  return (int)(b < LN_MAX_BLOCKS ? b : LN_MAX_BLOCKS);
}

// ---------------------------------------------------------------------------------------------------------------- depthwise conv backward
// T: the element type of in, du and dx; the LDS tiles and every sum are fp32 for both
template <int K, typename T>
__global__ __launch_bounds__(CB_THREADS) void dwconv_bwd_kernel(const T* __restrict__ in, int in_ld, const T* __restrict__ du,
                                                                int du_ld, const float* __restrict__ dw_w, T* __restrict__ dx,
                                                                int dx_ld, float* __restrict__ part, int H, int W, int C, int tiles_x,
                                                                int tiles_y, int tiles) {
  constexpr int R = K / 2, HY = CB_TY + K - 1, HX = CB_TX + K - 1, KK = K * K;
  constexpr int ITEMS = KK * CB_G;                              // (tap, four channels) weight-gradient items of a chunk
  constexpr int NI = (ITEMS + CB_THREADS - 1) / CB_THREADS;     // per thread: 2 at k = 7
  constexpr int BIAS_T0 = CB_THREADS - CB_G;                    // the last 8 threads (never on a second item) own the bias gradient
  __shared__ f32x4 hin[HY * HX * CB_G];                         // [halo pixel][group] of the forward's input: 17.5 KB at k = 7
  __shared__ f32x4 hdu[HY * HX * CB_G];                         // ... of du
  __shared__ f32x4 wts[KK * CB_G];                              // [tap][group]
  const int tid = threadIdx.x;
  const int c0 = blockIdx.y * CB_CC;
  const int cn = (C - c0) < CB_CC ? (C - c0) : CB_CC;           // a multiple of 4
  const int q = tid / CB_G, g = tid % CB_G;                     // dx item: pixel q of the tile, channels 4g .. 4g+3 of the chunk
  const int qy = q / CB_TX, qx = q % CB_TX;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int i = tid; i < KK * CB_G; i += CB_THREADS) {
    const int t = i / CB_G, gg = i % CB_G;
    f32x4 v = zero;
    if (gg * 4 < cn) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = dw_w[(long long)(c0 + gg * 4 + e) * KK + t];
    }
    wts[i] = v;
  }
  f32x4 acc[NI];
  int ioff[NI], ig[NI];
#pragma unroll
  for (int n = 0; n < NI; ++n) {
    const int i = tid + n * CB_THREADS;
    const int t = i / CB_G;
    acc[n] = zero;
    ig[n] = i % CB_G;
    ioff[n] = i < ITEMS ? ((t / K) * HX + t % K) * CB_G + ig[n] : -1;
  }
  f32x4 bacc = zero;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {            // a fixed slice of the tiles: shape only
    const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, b = tile / (tiles_x * tiles_y);
    const int x0 = tx * CB_TX, y0 = ty * CB_TY;
    const long long img = (long long)b * H * W;
    __syncthreads();                                                         // the previous tile's LDS reads are done
    for (int i = tid; i < HY * HX * CB_G; i += CB_THREADS) {
      const int hp = i / CB_G, gg = i % CB_G;
      const int hy = hp / HX, hx = hp - hy * HX;
      const int yy = y0 + hy - R, xx = x0 + hx - R;
      f32x4 a = zero, d = zero;
      if (gg * 4 < cn && (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) {
        const long long p = img + (long long)yy * W + xx;
        a = load4_widen(in + p * in_ld + c0 + gg * 4);
        d = load4_widen(du + p * du_ld + c0 + gg * 4);
      }
      hin[i] = a;
      hdu[i] = d;
    }
    __syncthreads();
    // dx[p] = sum_taps w[ky][kx] * du[y - ky + R, x - kx + R]: the forward's window with the taps flipped
    if (g * 4 < cn && y0 + qy < H && x0 + qx < W) {
      f32x4 s = zero;
#pragma unroll
      for (int ky = 0; ky < K; ++ky) {
#pragma unroll
        for (int kx = 0; kx < K; ++kx)
          s += hdu[((qy + K - 1 - ky) * HX + qx + K - 1 - kx) * CB_G + g] * wts[(ky * K + kx) * CB_G + g];
      }
      store4(dx + (img + (long long)(y0 + qy) * W + x0 + qx) * dx_ld + c0 + g * 4, s);
    }
    // dweight[c][ky][kx] += sum over the tile's pixels of du[p] * in[y + ky - R, x + kx - R] (du is zero outside the image)
#pragma unroll
    for (int n = 0; n < NI; ++n) {
      if (ioff[n] >= 0) {
        f32x4 s = acc[n];
#pragma unroll 8
        for (int pq = 0; pq < CB_PIX; ++pq) {
          const int py = pq / CB_TX, px = pq % CB_TX;
          s += hdu[((py + R) * HX + px + R) * CB_G + ig[n]] * hin[(py * HX + px) * CB_G + ioff[n]];
        }
        acc[n] = s;
      }
    }
    if (tid >= BIAS_T0) {
      const int gb = tid - BIAS_T0;
      f32x4 s = bacc;
#pragma unroll 8
      for (int pq = 0; pq < CB_PIX; ++pq) s += hdu[((pq / CB_TX + R) * HX + pq % CB_TX + R) * CB_G + gb];
      bacc = s;
    }
  }
  // this slice's partial: part[slice][c][0 .. KK-1] weight taps, [KK] bias
  float* prow = part + (long long)blockIdx.x * C * (KK + 1);
#pragma unroll
  for (int n = 0; n < NI; ++n) {
    const int i = tid + n * CB_THREADS;
    if (i < ITEMS && ig[n] * 4 < cn) {
      const int t = i / CB_G;
#pragma unroll
      for (int e = 0; e < 4; ++e) prow[(long long)(c0 + ig[n] * 4 + e) * (KK + 1) + t] = acc[n][e];
    }
  }
  if (tid >= BIAS_T0 && (tid - BIAS_T0) * 4 < cn) {
#pragma unroll
    for (int e = 0; e < 4; ++e) prow[(long long)(c0 + (tid - BIAS_T0) * 4 + e) * (KK + 1) + KK] = bacc[e];
  }
}

// dweight[c][t] / dbias[c] = sum over the slices, in order
__global__ __launch_bounds__(256) void dwconv_bwd_reduce_kernel(const float* __restrict__ part, int slices, int C, int KK,
                                                                float* __restrict__ dweight, float* __restrict__ dbias) {
  const int n = C * (KK + 1);
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  float s = 0.f;
  for (int r = 0; r < slices; ++r) s += part[(long long)r * n + j];
  const int c = j / (KK + 1), t = j - c * (KK + 1);
  if (t < KK) dweight[c * KK + t] = s;
  else if (dbias != nullptr) dbias[c] = s;
}

int dw_bwd_slices(int B, int H, int W) {
  const long long tiles = (long long)B * ((H + CB_TY - 1) / CB_TY) * ((W + CB_TX - 1) / CB_TX);
  return (int)(tiles < CB_MAX_SLICES ? tiles : CB_MAX_SLICES);
}

template <int K, typename T>
int launch_dwconv_bwd(const T* in, int in_ld, const T* du, int du_ld, const float* dw_w, T* dx, int dx_ld, float* dweight,
                      float* dbias, float* part, int B, int H, int W, int C, hipStream_t st) {
  const int tiles_x = (W + CB_TX - 1) / CB_TX, tiles_y = (H + CB_TY - 1) / CB_TY;
  const int tiles = B * tiles_x * tiles_y, slices = dw_bwd_slices(B, H, W);
  hipLaunchKernelGGL((dwconv_bwd_kernel<K, T>), dim3((unsigned)slices, (unsigned)((C + CB_CC - 1) / CB_CC)), dim3(CB_THREADS), 0, st, in, in_ld,
                     du, du_ld, dw_w, dx, dx_ld, part, H, W, C, tiles_x, tiles_y, tiles);
  const int n = C * (K * K + 1);
  hipLaunchKernelGGL(dwconv_bwd_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part, slices, C, K * K, dweight, dbias);
  return pfk_launch_status();
}

// ---------------------------------------------------------------------------------------------------------------- GELU
constexpr float INV_SQRT2 = 0.70710678118654752f, INV_SQRT_2PI = 0.39894228040143268f;

// 16 bytes of a row per thread: four floats | eight bf16 (CV groups per row); the formulas are evaluated on float(x)
template <bool BWD, typename T>
__global__ __launch_bounds__(256) void gelu_rows_kernel(const T* __restrict__ x, long long x_ld, const T* __restrict__ dy,
                                                        long long dy_ld, T* __restrict__ out, long long out_ld, long long M, int CV) {
  constexpr int V = QUANTUM<T>;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * CV) return;
  long long r;
  if (M * CV <= 0xffffffffLL) r = (unsigned)i / (unsigned)CV;      // grid-uniform: a 32-bit division wherever the item count allows one
  else r = i / CV;
  const int c = (int)(i - r * CV) * V;
  float v[V], o[V];
  load_row<V>(x + r * x_ld + c, v);
  if constexpr (BWD) {
    float d[V];
    load_row<V>(dy + r * dy_ld + c, d);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      // Phi(x) + x phi(x); past |x| = 40 the density term is below every fp32 (and x * 0 would be NaN at infinity)
      const float cdf = 0.5f * (1.0f + erff(v[e] * INV_SQRT2));
      const float pdf = fabsf(v[e]) > 40.f ? 0.f : v[e] * expf(-0.5f * v[e] * v[e]) * INV_SQRT_2PI;
      o[e] = d[e] * (cdf + pdf);
    }
  } else {
#pragma unroll
    for (int e = 0; e < V; ++e) o[e] = 0.5f * v[e] * (1.0f + erff(v[e] * INV_SQRT2));      // gelu_erf (pfk_common.h) written out: the call allocates this kernel's registers differently
  }
  store_row<V>(out + r * out_ld + c, o);
}

template <typename T>
bool rows_ok(const T* p, long long ld) { return pfk_aligned16(p) && !(ld & (QUANTUM<T> - 1)); }

template <typename T>
bool overlap(const T* a, long long a_ld, const T* b, long long b_ld, long long M, int C) {
  const char* ab = reinterpret_cast<const char*>(a);
  const char* ae = reinterpret_cast<const char*>(a + (M - 1) * a_ld + C);
  const char* bb = reinterpret_cast<const char*>(b);
  const char* be = reinterpret_cast<const char*>(b + (M - 1) * b_ld + C);
  return ab < be && bb < ae;
}

// ---------------------------------------------------------------------------------------------------------------- the entries, per T
template <typename T>
int layernorm_bwd_entry(const T* xhat, int xhat_ld, const float* rstd, const float* ln_weight, const T* dy, int dy_ld, T* du, int du_ld,
                        float* dgamma, float* dbeta, void* workspace, long long workspace_bytes, long long M, int C, pfk_stream_t stream) {
  constexpr int Q = QUANTUM<T>;
  if (!xhat || !rstd || !ln_weight || !dy || !du || !dgamma || !dbeta || !workspace || M <= 0 || C < Q || C > CB_MAX_C || (C & (Q - 1)) ||
      xhat_ld < C || dy_ld < C || du_ld < C)
    return PFK_ERR_BAD_ARG;
  if (!pfk_fits32(M)) return PFK_ERR_UNSUPPORTED;
  if (workspace_bytes < pfk_layernorm_bwd_workspace_bytes(M, C)) return PFK_ERR_BAD_ARG;
  if (!rows_ok(xhat, xhat_ld) || !rows_ok(dy, dy_ld) || !rows_ok(du, du_ld) || !pfk_aligned16(workspace)) return PFK_ERR_ALIGNMENT;
  if (overlap(du, du_ld, dy, dy_ld, M, C) || overlap(du, du_ld, xhat, xhat_ld, M, C)) return PFK_ERR_BAD_ARG;      // out of place only
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int blocks = ln_bwd_blocks(M);
  float* part = static_cast<float*>(workspace);
  hipLaunchKernelGGL(layernorm_bwd_kernel<T>, dim3((unsigned)blocks), dim3(LN_WAVES * 64), 0, st, xhat, xhat_ld, rstd, ln_weight, dy, dy_ld,
                     du, du_ld, part, M, C);
  hipLaunchKernelGGL(column_reduce_kernel, dim3((unsigned)((2 * C + 63) / 64)), dim3(LN_RED_PARTS * 64), 0, st, part, blocks, 2 * C, dgamma,
                     dbeta, C);
  return pfk_launch_status();
}

template <typename T>
int dwconv_bwd_entry(const T* in, int in_ld, const T* du, int du_ld, const float* dw_weight, T* dx, int dx_ld, float* dweight, float* dbias,
                     void* workspace, long long workspace_bytes, int B, int H, int W, int C, int k, pfk_stream_t stream) {
  constexpr int Q = QUANTUM<T>;
  if (!in || !du || !dw_weight || !dx || !dweight || !workspace || B <= 0 || H <= 0 || W <= 0 || C < Q || C > CB_MAX_C || (C & (Q - 1)) ||
      in_ld < C || du_ld < C || dx_ld < C)
    return PFK_ERR_BAD_ARG;
  if (k < 1 || !(k & 1) || k > 7) return PFK_ERR_BAD_ARG;
  const long long M = (long long)B * H * W;
  if (!pfk_fits32(M)) return PFK_ERR_UNSUPPORTED;
  if (workspace_bytes < pfk_dwconv_bwd_workspace_bytes(B, H, W, C, k)) return PFK_ERR_BAD_ARG;
  if (!rows_ok(in, in_ld) || !rows_ok(du, du_ld) || !rows_ok(dx, dx_ld) || !pfk_aligned16(workspace)) return PFK_ERR_ALIGNMENT;
  // dx must not overlap du or in: other blocks still read the halo of pixels this block has written
  if (overlap(dx, dx_ld, du, du_ld, M, C) || overlap(dx, dx_ld, in, in_ld, M, C)) return PFK_ERR_BAD_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(workspace);
  switch (k) {
    case 1: return launch_dwconv_bwd<1>(in, in_ld, du, du_ld, dw_weight, dx, dx_ld, dweight, dbias, part, B, H, W, C, st);
    case 3: return launch_dwconv_bwd<3>(in, in_ld, du, du_ld, dw_weight, dx, dx_ld, dweight, dbias, part, B, H, W, C, st);
    case 5: return launch_dwconv_bwd<5>(in, in_ld, du, du_ld, dw_weight, dx, dx_ld, dweight, dbias, part, B, H, W, C, st);
    default: return launch_dwconv_bwd<7>(in, in_ld, du, du_ld, dw_weight, dx, dx_ld, dweight, dbias, part, B, H, W, C, st);
  }
}

template <typename T>
int gelu_entry(bool bwd, const T* x, long long x_ld, const T* dy, long long dy_ld, T* out, long long out_ld, long long M, int C,
               pfk_stream_t stream) {
  constexpr int Q = QUANTUM<T>;
  if (!x || !out || (bwd && !dy) || M <= 0 || C < Q || (C & (Q - 1)) || x_ld < C || out_ld < C || (bwd && dy_ld < C)) return PFK_ERR_BAD_ARG;
  if (!pfk_fits32(M * (C / Q) / 256)) return PFK_ERR_UNSUPPORTED;
  if (!rows_ok(x, x_ld) || !rows_ok(out, out_ld) || (bwd && !rows_ok(dy, dy_ld))) return PFK_ERR_ALIGNMENT;
  if (overlap(out, out_ld, x, x_ld, M, C) || (bwd && overlap(out, out_ld, dy, dy_ld, M, C))) return PFK_ERR_BAD_ARG;   // out of place only
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long long n = M * (C / Q);
  const dim3 grid((unsigned)((n + 255) / 256));
  if (bwd) hipLaunchKernelGGL((gelu_rows_kernel<true, T>), grid, dim3(256), 0, st, x, x_ld, dy, dy_ld, out, out_ld, M, C / Q);
  else hipLaunchKernelGGL((gelu_rows_kernel<false, T>), grid, dim3(256), 0, st, x, x_ld, x, x_ld, out, out_ld, M, C / Q);
  return pfk_launch_status();
}

const __bf16* b16(const void* p) { return static_cast<const __bf16*>(p); }
__bf16* b16(void* p) { return static_cast<__bf16*>(p); }

}  // namespace

extern "C" {

long long pfk_layernorm_bwd_workspace_bytes(long long M, int C) {
  if (M <= 0 || C <= 0) return 0;
  return (long long)ln_bwd_blocks(M) * 2 * C * (long long)sizeof(float);
}

int pfk_layernorm_bwd_f32(const float* xhat, int xhat_ld, const float* rstd, const float* ln_weight, const float* dy, int dy_ld,
                          float* du, int du_ld, float* dgamma, float* dbeta, void* workspace, long long workspace_bytes, long long M,
                          int C, pfk_stream_t stream) {
  return layernorm_bwd_entry(xhat, xhat_ld, rstd, ln_weight, dy, dy_ld, du, du_ld, dgamma, dbeta, workspace, workspace_bytes, M, C, stream);
}

int pfk_layernorm_bwd_b16(const void* xhat_bf16, int xhat_ld, const float* rstd, const float* ln_weight, const void* dy_bf16, int dy_ld,
                          void* du_bf16, int du_ld, float* dgamma, float* dbeta, void* workspace, long long workspace_bytes, long long M,
                          int C, pfk_stream_t stream) {
  return layernorm_bwd_entry(b16(xhat_bf16), xhat_ld, rstd, ln_weight, b16(dy_bf16), dy_ld, b16(du_bf16), du_ld, dgamma, dbeta, workspace,
                             workspace_bytes, M, C, stream);
}

long long pfk_dwconv_bwd_workspace_bytes(int B, int H, int W, int C, int k) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || k <= 0) return 0;
  return (long long)dw_bwd_slices(B, H, W) * C * (k * k + 1) * (long long)sizeof(float);
}

int pfk_dwconv_bwd_f32(const float* in, int in_ld, const float* du, int du_ld, const float* dw_weight, float* dx, int dx_ld,
                       float* dweight, float* dbias, void* workspace, long long workspace_bytes, int B, int H, int W, int C, int k,
                       pfk_stream_t stream) {
  return dwconv_bwd_entry(in, in_ld, du, du_ld, dw_weight, dx, dx_ld, dweight, dbias, workspace, workspace_bytes, B, H, W, C, k, stream);
}

int pfk_dwconv_bwd_b16(const void* in_bf16, int in_ld, const void* du_bf16, int du_ld, const float* dw_weight, void* dx_bf16, int dx_ld,
                       float* dweight, float* dbias, void* workspace, long long workspace_bytes, int B, int H, int W, int C, int k,
                       pfk_stream_t stream) {
  return dwconv_bwd_entry(b16(in_bf16), in_ld, b16(du_bf16), du_ld, dw_weight, b16(dx_bf16), dx_ld, dweight, dbias, workspace,
                          workspace_bytes, B, H, W, C, k, stream);
}

int pfk_gelu_f32(const float* x, long long x_ld, float* y, long long y_ld, long long M, int C, pfk_stream_t stream) {
  return gelu_entry<float>(false, x, x_ld, nullptr, 0, y, y_ld, M, C, stream);
}

int pfk_gelu_bwd_f32(const float* x, long long x_ld, const float* dy, long long dy_ld, float* dx, long long dx_ld, long long M, int C,
                     pfk_stream_t stream) {
  return gelu_entry<float>(true, x, x_ld, dy, dy_ld, dx, dx_ld, M, C, stream);
}

int pfk_gelu_b16(const void* x_bf16, long long x_ld, void* y_bf16, long long y_ld, long long M, int C, pfk_stream_t stream) {
  return gelu_entry<__bf16>(false, b16(x_bf16), x_ld, nullptr, 0, b16(y_bf16), y_ld, M, C, stream);
}

int pfk_gelu_bwd_b16(const void* x_bf16, long long x_ld, const void* dy_bf16, long long dy_ld, void* dx_bf16, long long dx_ld, long long M,
                     int C, pfk_stream_t stream) {
  return gelu_entry<__bf16>(true, b16(x_bf16), x_ld, b16(dy_bf16), dy_ld, b16(dx_bf16), dx_ld, M, C, stream);
}

}  // extern "C"
