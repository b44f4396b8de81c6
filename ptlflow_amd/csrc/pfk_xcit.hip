// K14 — CCMR's XCiT motion aggregator (ptlflow/models/ccmr/xcit.py, XCiT(embed_dim=128, depth=1, num_heads=8, mlp_ratio=1,
// separate=True)) on pixel-major fp32 rows: the four row kernels around the 1x1 GEMMs that pfk_conv2d_f32 runs (include/pfk.h).
//
//   pfk_layernorm_rows_f32   one wave per row: mean, then the biased variance about it, optional weight / bias
//   pfk_xca_map_f32          the 8 x (16 x 16) cross-covariance map of a scale: per 256-token chunk the block-diagonal Gram
//                            sum_n q[n,h,i] k[n,h,j] and both column norms in one pass over the rows (partials in the workspace),
//                            then chunk-order sums in double, normalise, temperature, softmax over j
//   pfk_xcit_lpi1_f32        u = GELU(dw3x3(LN3(x)) + b1) and the per-block GroupNorm sums of u (double) into the workspace
//   pfk_xcit_lpi2_f32        statistics finished in block order, then x2 = x + gamma3 * (dw3x3(GN(u)) + b2) and t = LN2(x2)
//
// K17 — the same block with separate=False (CCMR's per-scale context grouping, `model.xcit[i]`) adds the two once-per-scale kernels
//   pfk_xcit_tokens_f32      NCHW (or pixel-major, _pm) input -> x0 = rows(in) + pos and xh = LayerNorm(x0) without affine, one pass
//   pfk_xca_fold_f32         the attention branch behind the map as one affine map per image: M_b, c_b
//
// The two LPI kernels own a 4 x 8 tile of pixels and all 128 channels, as dwconv_ln_kernel does (pfk_convnext.hip): the 6 x 10 halo is
// staged in LDS ALREADY NORMALISED, so a tap outside the image contributes exactly 0 (the reference pads the normalised tensor) and no
// tap crosses into the next image.  Thread (column qx = tid / 32, float4 group g = tid % 32) forms the four pixels of its tile column;
// a half-wave holds all 128 channels of those pixels, so LN2's two reductions are xor-shuffles over 32 lanes.  No atomics anywhere:
// every sum runs in an order fixed by the shape.
#include "pfk_launch.h"

namespace {

constexpr int XC_C = 128, XC_HEADS = 8, XC_DH = 16, XC_GROUPS = 8;
constexpr int XC_G4 = XC_C / 4;               // float4 groups of a row
constexpr int XC_THREADS = 256;

// ------------------------------------------------------------------------------------------------ LayerNorm over the channels of a row
constexpr int LN_MAX_C = 512;
constexpr int LN_NT = LN_MAX_C / 4 / 64;      // float4 groups per lane

__global__ __launch_bounds__(XC_THREADS) void layernorm_rows_kernel(const float* __restrict__ in, long long in_ld, const float* __restrict__ w,
                                                                    const float* __restrict__ b, float eps, float* __restrict__ out,
                                                                    long long out_ld, long long M, int C) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * (XC_THREADS / 64) + (threadIdx.x >> 6);
  if (row >= M) return;                                        // wave-uniform
  const float* src = in + row * in_ld;
  const int ng = C >> 2;
  f32x4 v[LN_NT];
  float s = 0.f;
#pragma unroll
  for (int t = 0; t < LN_NT; ++t) {
    const int g = lane + 64 * t;
    v[t] = g < ng ? *reinterpret_cast<const f32x4*>(src + 4 * g) : f32x4{0.f, 0.f, 0.f, 0.f};
    s += (v[t][0] + v[t][1]) + (v[t][2] + v[t][3]);
  }
  const float inv_c = 1.0f / (float)C;
  const float mean = wave_sum(s) * inv_c;
  float s2 = 0.f;
#pragma unroll
  for (int t = 0; t < LN_NT; ++t) {
    if (lane + 64 * t < ng) {
      v[t] -= mean;
      s2 += (v[t][0] * v[t][0] + v[t][1] * v[t][1]) + (v[t][2] * v[t][2] + v[t][3] * v[t][3]);
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(s2) * inv_c + eps);
  float* dst = out + row * out_ld;
#pragma unroll
  for (int t = 0; t < LN_NT; ++t) {
    const int g = lane + 64 * t;
    if (g < ng) {
      f32x4 y = v[t] * rstd;
      if (w != nullptr) y = y * *reinterpret_cast<const f32x4*>(w + 4 * g);
      if (b != nullptr) y = y + *reinterpret_cast<const f32x4*>(b + 4 * g);
      *reinterpret_cast<f32x4*>(dst + 4 * g) = y;
    }
  }
}

// ------------------------------------------------------------------------------------------------ cross-covariance attention map
constexpr int XCA_TILE = 32;                  // tokens staged per LDS tile: 32 x 256 floats = 32 KB
constexpr int XCA_CHUNK = 256;                // tokens per block
constexpr int XCA_QK = 2 * XC_C;              // q | k columns of a row
constexpr int XCA_GRAM = XC_HEADS * XC_DH * XC_DH;
constexpr int XCA_PART = XCA_GRAM + 2 * XC_C; // Gram | sum q^2 | sum k^2 of one chunk

// thread (h = tid / 32, i = (tid % 32) / 2, jh = tid % 2): Gram entries (h, i, 8 jh .. 8 jh + 7)
__global__ __launch_bounds__(XC_THREADS) void xca_partial_kernel(const float* __restrict__ qk, long long qk_ld, float* __restrict__ part,
                                                                 int N, int nchunk) {
  __shared__ f32x4 tile[XCA_TILE * (XCA_QK / 4)];
  const int tid = threadIdx.x;
  const int h = tid >> 5, i = (tid & 31) >> 1, jh = tid & 1;
  const long long img = (long long)blockIdx.y * N;
  const int n0 = blockIdx.x * XCA_CHUNK;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 g0 = zero, g1 = zero, kk0 = zero, kk1 = zero;
  float qq = 0.f;
  for (int tb = 0; tb < XCA_CHUNK && n0 + tb < N; tb += XCA_TILE) {
    __syncthreads();                                           // the previous tile's LDS reads are done
    for (int e = tid; e < XCA_TILE * (XCA_QK / 4); e += XC_THREADS) {
      const int tk = e >> 6, c4 = e & 63;
      const int n = n0 + tb + tk;
      tile[e] = n < N ? *reinterpret_cast<const f32x4*>(qk + (img + n) * qk_ld + 4 * c4) : zero;   // a row past N adds exact zeros
    }
    __syncthreads();
    const float* tf = reinterpret_cast<const float*>(tile);
#pragma unroll 4
    for (int tk = 0; tk < XCA_TILE; ++tk) {
      const float q = tf[tk * XCA_QK + h * XC_DH + i];
      const f32x4 k0 = tile[tk * (XCA_QK / 4) + XC_G4 + h * 4 + jh * 2];
      const f32x4 k1 = tile[tk * (XCA_QK / 4) + XC_G4 + h * 4 + jh * 2 + 1];
      g0 += q * k0; g1 += q * k1;
      kk0 += k0 * k0; kk1 += k1 * k1;
      qq += q * q;
    }
  }
  float* p = part + ((long long)blockIdx.y * nchunk + blockIdx.x) * XCA_PART;
  *reinterpret_cast<f32x4*>(p + tid * 8) = g0;
  *reinterpret_cast<f32x4*>(p + tid * 8 + 4) = g1;
  if (jh == 0) p[XCA_GRAM + h * XC_DH + i] = qq;
  if (i == 0) {
    *reinterpret_cast<f32x4*>(p + XCA_GRAM + XC_C + h * XC_DH + jh * 8) = kk0;
    *reinterpret_cast<f32x4*>(p + XCA_GRAM + XC_C + h * XC_DH + jh * 8 + 4) = kk1;
  }
}

// block (h, b), thread (i = tid / 16, j = tid % 16): the chunks' partials summed in chunk order in double, F.normalize's
// max(norm, 1e-12), the head's temperature, softmax over the 16 adjacent lanes of a row
__global__ __launch_bounds__(XC_THREADS) void xca_finish_kernel(const float* __restrict__ part, const float* __restrict__ temperature,
                                                                float* __restrict__ A, int nchunk) {
  const int tid = threadIdx.x, h = blockIdx.x, i = tid >> 4, j = tid & 15;
  const float* p = part + (long long)blockIdx.y * nchunk * XCA_PART;
  double g = 0.0, qq = 0.0, kk = 0.0;
  for (int c = 0; c < nchunk; ++c, p += XCA_PART) {
    g += (double)p[h * XC_DH * XC_DH + tid];
    qq += (double)p[XCA_GRAM + h * XC_DH + i];
    kk += (double)p[XCA_GRAM + XC_C + h * XC_DH + j];
  }
  const double nq = fmax(sqrt(qq), 1e-12), nk = fmax(sqrt(kk), 1e-12);
  const float logit = (float)((double)temperature[h] * (g / (nq * nk)));
  const float m = wave_max<16>(logit);
  const float e = expf(logit - m);
  const float s = wave_sum<16>(e);
  A[((long long)blockIdx.y * XC_HEADS + h) * (XC_DH * XC_DH) + tid] = e / s;
}

// ------------------------------------------------------------------------------------------------ local patch interaction
constexpr int LP_TY = 4, LP_TX = 8;
constexpr int LP_HY = LP_TY + 2, LP_HX = LP_TX + 2;
constexpr int LP_HALO = LP_HY * LP_HX;        // 60 pixels x 512 bytes = 30 KB
static_assert(LP_TX * XC_G4 == XC_THREADS, "one (tile column, float4 group) item per thread");
constexpr int LP_STAT = 2 * XC_GROUPS;        // sum | sum of squares of each group: doubles per block partial, floats (mean | rstd) per image

// the 3 x 3 taps of this thread's float4 group, [channel][tap] in memory
__device__ __forceinline__ void lpi_load_taps(const float* __restrict__ dw_w, int g, f32x4* w) {
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int e = 0; e < 4; ++e) w[t][e] = dw_w[(4 * g + e) * 9 + t];
}

// acc[r] += sum of the taps over the staged halo for the four pixels (r, qx) of the thread's tile column: every halo value is read once
__device__ __forceinline__ void lpi_taps(const f32x4* halo, int qx, int g, const f32x4* w, f32x4* acc) {
#pragma unroll
  for (int hy = 0; hy < LP_HY; ++hy) {
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const f32x4 hv = halo[(hy * LP_HX + qx + kx) * XC_G4 + g];
#pragma unroll
      for (int r = 0; r < LP_TY; ++r) {
        const int ky = hy - r;
        if (ky >= 0 && ky < 3) acc[r] += hv * w[ky * 3 + kx];
      }
    }
  }
}

__global__ __launch_bounds__(XC_THREADS) void lpi1_kernel(const float* __restrict__ x, long long x_ld, const float* __restrict__ ln_w,
                                                          const float* __restrict__ ln_b, float eps, const float* __restrict__ dw_w,
                                                          const float* __restrict__ dw_b, float* __restrict__ u, long long u_ld,
                                                          double* __restrict__ part, int H, int W) {
  __shared__ f32x4 halo[LP_HALO * XC_G4];
  __shared__ double red[XC_THREADS / 64][LP_STAT];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int x0 = blockIdx.x * LP_TX, y0 = blockIdx.y * LP_TY;
  const long long img = (long long)blockIdx.z * H * W;
  // halo pixel by halo pixel, one wave each, lane = channels 2 lane, 2 lane + 1: LN3 of the pixel's row, or zeros outside the image
  const f32x2 lw = *reinterpret_cast<const f32x2*>(ln_w + 2 * lane), lb = *reinterpret_cast<const f32x2*>(ln_b + 2 * lane);
  f32x2* hf = reinterpret_cast<f32x2*>(halo);
  for (int hp = wv; hp < LP_HALO; hp += XC_THREADS / 64) {
    const int hy = hp / LP_HX, hx = hp - hy * LP_HX;
    const int yy = y0 + hy - 1, xx = x0 + hx - 1;
    f32x2 v = {0.f, 0.f};
    if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) {        // wave-uniform
      v = *reinterpret_cast<const f32x2*>(x + (img + (long long)yy * W + xx) * x_ld + 2 * lane);
      const float mean = wave_sum(v.x + v.y) * (1.0f / XC_C);
      v -= mean;
      const float rstd = 1.0f / sqrtf(wave_sum(v.x * v.x + v.y * v.y) * (1.0f / XC_C) + eps);
      v = v * rstd * lw + lb;
    }
    hf[hp * (XC_C / 2) + lane] = v;
  }
  const int g = tid & 31, qx = tid >> 5;
  f32x4 w[9];
  lpi_load_taps(dw_w, g, w);
  const f32x4 bias = *reinterpret_cast<const f32x4*>(dw_b + 4 * g);
  f32x4 acc[LP_TY];
#pragma unroll
  for (int r = 0; r < LP_TY; ++r) acc[r] = bias;
  __syncthreads();
  lpi_taps(halo, qx, g, w, acc);
  double s = 0.0, s2 = 0.0;
  const int xo = x0 + qx;
#pragma unroll
  for (int r = 0; r < LP_TY; ++r) {
    const int yo = y0 + r;
    if (yo < H && xo < W) {
      f32x4 y;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        y[e] = gelu_erf(acc[r][e]);
        s += (double)y[e];
        s2 += (double)y[e] * (double)y[e];
      }
      *reinterpret_cast<f32x4*>(u + (img + (long long)yo * W + xo) * u_ld + 4 * g) = y;
    }
  }
  // GroupNorm sums of the block: a group is 16 channels = the float4 groups 4k .. 4k+3, i.e. lanes 4k .. 4k+3 of both half-waves
  s += __shfl_xor(s, 1, 64);  s2 += __shfl_xor(s2, 1, 64);
  s += __shfl_xor(s, 2, 64);  s2 += __shfl_xor(s2, 2, 64);
  s += __shfl_xor(s, 32, 64); s2 += __shfl_xor(s2, 32, 64);
  if (lane < 32 && (lane & 3) == 0) {
    red[wv][(lane >> 2) * 2] = s;
    red[wv][(lane >> 2) * 2 + 1] = s2;
  }
  __syncthreads();
  if (tid < LP_STAT) {
    double t = red[0][tid];
#pragma unroll
    for (int k = 1; k < XC_THREADS / 64; ++k) t += red[k][tid];
    const long long blk = ((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    part[blk * LP_STAT + tid] = t;
  }
}

// one block per image: the nblk block partials summed in a fixed order (16 interleaved slices, then the slices in order), in double;
// mean and rstd of each group rounded once
__global__ __launch_bounds__(XC_THREADS) void gn_finish_kernel(const double* __restrict__ part, int nblk, double count, float eps,
                                                               float* __restrict__ stats) {
  __shared__ double red[XC_THREADS / LP_STAT][LP_STAT];
  const int tid = threadIdx.x, qn = tid & (LP_STAT - 1), sl = tid / LP_STAT;
  const double* p = part + (long long)blockIdx.x * nblk * LP_STAT;
  double t = 0.0;
  for (int k = sl; k < nblk; k += XC_THREADS / LP_STAT) t += p[(long long)k * LP_STAT + qn];
  red[sl][qn] = t;
  __syncthreads();
  if (tid < XC_GROUPS) {
    double s = 0.0, s2 = 0.0;
    for (int k = 0; k < XC_THREADS / LP_STAT; ++k) {
      s += red[k][2 * tid];
      s2 += red[k][2 * tid + 1];
    }
    const double mean = s / count;
    const double var = fmax(s2 / count - mean * mean, 0.0);
    stats[blockIdx.x * LP_STAT + 2 * tid] = (float)mean;
    stats[blockIdx.x * LP_STAT + 2 * tid + 1] = (float)(1.0 / sqrt(var + (double)eps));
  }
}

__global__ __launch_bounds__(XC_THREADS) void lpi2_kernel(const float* __restrict__ u, long long u_ld, const float* __restrict__ stats,
                                                          const float* __restrict__ gn_w, const float* __restrict__ gn_b,
                                                          const float* __restrict__ dw_w, const float* __restrict__ dw_b,
                                                          const float* __restrict__ gamma, const float* __restrict__ x, long long x_ld,
                                                          float* __restrict__ x2, long long x2_ld, const float* __restrict__ ln_w,
                                                          const float* __restrict__ ln_b, float eps, float* __restrict__ t, long long t_ld,
                                                          int H, int W) {
  __shared__ f32x4 halo[LP_HALO * XC_G4];
  const int tid = threadIdx.x;
  const int g = tid & 31, qx = tid >> 5;
  const int x0 = blockIdx.x * LP_TX, y0 = blockIdx.y * LP_TY;
  const long long img = (long long)blockIdx.z * H * W;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  // GroupNorm of the halo: a thread stages its own float4 group (XC_THREADS % XC_G4 == 0), zeros outside the image
  const float mean = stats[blockIdx.z * LP_STAT + 2 * (g >> 2)], rstd = stats[blockIdx.z * LP_STAT + 2 * (g >> 2) + 1];
  const f32x4 gw = *reinterpret_cast<const f32x4*>(gn_w + 4 * g), gb = *reinterpret_cast<const f32x4*>(gn_b + 4 * g);
  for (int hp = qx; hp < LP_HALO; hp += XC_THREADS / XC_G4) {
    const int hy = hp / LP_HX, hx = hp - hy * LP_HX;
    const int yy = y0 + hy - 1, xx = x0 + hx - 1;
    f32x4 v = zero;
    if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W)
      v = (*reinterpret_cast<const f32x4*>(u + (img + (long long)yy * W + xx) * u_ld + 4 * g) - mean) * rstd * gw + gb;
    halo[hp * XC_G4 + g] = v;
  }
  f32x4 w[9];
  lpi_load_taps(dw_w, g, w);
  const f32x4 bias = *reinterpret_cast<const f32x4*>(dw_b + 4 * g), gm = *reinterpret_cast<const f32x4*>(gamma + 4 * g);
  f32x4 acc[LP_TY];
#pragma unroll
  for (int r = 0; r < LP_TY; ++r) acc[r] = bias;
  __syncthreads();
  lpi_taps(halo, qx, g, w, acc);
  const f32x4 lw = ln_w != nullptr ? *reinterpret_cast<const f32x4*>(ln_w + 4 * g) : f32x4{1.f, 1.f, 1.f, 1.f};
  const f32x4 lb = ln_b != nullptr ? *reinterpret_cast<const f32x4*>(ln_b + 4 * g) : zero;
  const int xo = x0 + qx;
#pragma unroll
  for (int r = 0; r < LP_TY; ++r) {
    const int yo = y0 + r;
    const bool live = yo < H && xo < W;                        // the same for the 32 lanes that share the pixel
    const long long p = img + (long long)yo * W + xo;
    f32x4 v = zero;
    if (live) {
      v = *reinterpret_cast<const f32x4*>(x + p * x_ld + 4 * g) + gm * acc[r];
      *reinterpret_cast<f32x4*>(x2 + p * x2_ld + 4 * g) = v;
    }
    const float m = wave_sum<32>((v[0] + v[1]) + (v[2] + v[3])) * (1.0f / XC_C);
    v -= m;
    const float rs = 1.0f / sqrtf(wave_sum<32>((v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3])) * (1.0f / XC_C) + eps);
    if (live) *reinterpret_cast<f32x4*>(t + p * t_ld + 4 * g) = v * rs * lw + lb;
  }
}

// ------------------------------------------------------------------------------------------------ K17: NCHW -> token rows + LN1
// A block owns TK_PX consecutive pixels n = y * W + x of one image, which are consecutive floats of every channel plane.  Wave w loads
// the planes w, w + 4, ... (lane = pixel: one 256-byte line per load) into LDS; then a half-wave holds one pixel's 128 channels as a
// float4 per lane (lane g: channels 4g .. 4g+3), as lpi2_kernel does for LN2.
// LDS image: channel c = 4g + e of pixel p at  e * TK_PLANE + g * TK_ROW + p,  TK_ROW = TK_PX + 1 (odd).  ds_write_b32 and ds_read_b32
// bank on (address / 4) % 32 within a 32-lane half.  The store (one channel, 32 consecutive pixels per half) walks 32 consecutive
// words; the transposed read (one pixel and e, g = 0 .. 31 per half) walks g * 65 = g (mod 32): both conflict-free.  A plain
// [128][65] image puts g and g + 8 on one bank (4g * 65 = 4g mod 32): 4-way.
constexpr int TK_PX = 64;
constexpr int TK_ROW = TK_PX + 1;
constexpr int TK_PLANE = XC_G4 * TK_ROW;

// x0 = v + pos, xh = LayerNorm(x0) without affine for the pixel this half-wave holds (g = its lane's float4 group); dead pixels (past
// the image) run the same shuffles on zeros and store nothing
__device__ __forceinline__ void tokens_finish(f32x4 v, const float* __restrict__ pos, long long n, long long row, int g, bool live, float eps,
                                              float* __restrict__ x0, long long x0_ld, float* __restrict__ xh, long long xh_ld) {
  if (live && pos != nullptr) v = v + *reinterpret_cast<const f32x4*>(pos + n * XC_C + 4 * g);
  if (live) *reinterpret_cast<f32x4*>(x0 + row * x0_ld + 4 * g) = v;
  const float m = wave_sum<32>((v[0] + v[1]) + (v[2] + v[3])) * (1.0f / XC_C);
  v -= m;
  const float rs = 1.0f / sqrtf(wave_sum<32>((v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3])) * (1.0f / XC_C) + eps);
  if (live) *reinterpret_cast<f32x4*>(xh + row * xh_ld + 4 * g) = v * rs;
}

__global__ __launch_bounds__(XC_THREADS) void tokens_nchw_kernel(const float* __restrict__ in, const float* __restrict__ pos, float eps,
                                                                 float* __restrict__ x0, long long x0_ld, float* __restrict__ xh,
                                                                 long long xh_ld, int N) {
  __shared__ float tile[4 * TK_PLANE];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n0 = blockIdx.x * TK_PX;
  const long long b = blockIdx.y;
  const float* src = in + b * XC_C * (long long)N;
  const bool have = n0 + lane < N;
#pragma unroll 8
  for (int c = wv; c < XC_C; c += XC_THREADS / 64)
    tile[(c & 3) * TK_PLANE + (c >> 2) * TK_ROW + lane] = have ? src[(long long)c * N + n0 + lane] : 0.f;
  __syncthreads();
  const int g = tid & 31, hw = tid >> 5;
  for (int p = hw; p < TK_PX; p += XC_THREADS / 32) {
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = tile[e * TK_PLANE + g * TK_ROW + p];
    const long long n = n0 + p;
    tokens_finish(v, pos, n, b * N + n, g, n < N, eps, x0, x0_ld, xh, xh_ld);      // (the same for the 32 lanes of the pixel)
  }
}

// the same from pixel-major input rows (a channels-last tensor): no transpose, one pixel per half-wave
__global__ __launch_bounds__(XC_THREADS) void tokens_pm_kernel(const float* __restrict__ in, long long in_ld, const float* __restrict__ pos,
                                                               float eps, float* __restrict__ x0, long long x0_ld, float* __restrict__ xh,
                                                               long long xh_ld, int N) {
  const int g = threadIdx.x & 31;
  const long long n = (long long)blockIdx.x * (XC_THREADS / 32) + (threadIdx.x >> 5);
  const long long row = (long long)blockIdx.y * N + n;
  const bool live = n < N;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (live) v = *reinterpret_cast<const f32x4*>(in + row * in_ld + 4 * g);
  tokens_finish(v, pos, n, row, g, live, eps, x0, x0_ld, xh, xh_ld);
}

// ------------------------------------------------------------------------------------------------ K17: the folded attention branch
// M_b = Wp blockdiag(A_b) Wv and c_b = Wp blockdiag(A_b) bv + bp for Wp = diag(gamma1) W_proj, bp = gamma1 * b_proj and the
// LN1-folded value projection Wv, bv.  Block (column tile, image): T = blockdiag(A_b) Wv[:, tile] (16 products per element), then
// M_b[:, tile] = Wp T with Wp staged 32 columns at a time.  Every sum is one fmaf chain in ascending index order.
constexpr int FD_NC = 16;                     // columns of M per block
constexpr int FD_KC = 32;                     // columns of Wp per stage
constexpr int FD_WLD = FD_KC + 4;             // row stride of the staged Wp: 16-byte rows, the 4 rows of a wave 36 words apart
constexpr int FD_R = XC_C * FD_NC / XC_THREADS;      // outputs per thread: rows mg + 16 r
static_assert(XC_THREADS / FD_NC * FD_R == XC_C, "the thread grid covers the 128 rows");

__global__ __launch_bounds__(XC_THREADS) void xca_fold_kernel(const float* __restrict__ A, const float* __restrict__ wv,
                                                              const float* __restrict__ bv, const float* __restrict__ wp,
                                                              const float* __restrict__ bp, float* __restrict__ M, float* __restrict__ c) {
  __shared__ float a_s[XCA_GRAM];
  __shared__ float wv_s[XC_C * FD_NC];
  __shared__ float t_s[XC_C * FD_NC];
  __shared__ __attribute__((aligned(16))) float wp_s[XC_C * FD_WLD];
  __shared__ float tb_s[XC_C];
  const int tid = threadIdx.x;
  const int n0 = blockIdx.x * FD_NC;
  const long long b = blockIdx.y;
  const float* Ab = A + b * XCA_GRAM;
  for (int e = tid; e < XCA_GRAM; e += XC_THREADS) a_s[e] = Ab[e];
  for (int e = tid; e < XC_C * FD_NC; e += XC_THREADS) wv_s[e] = wv[(e / FD_NC) * XC_C + n0 + (e % FD_NC)];
  __syncthreads();
  const int n = tid % FD_NC, mg = tid / FD_NC;
#pragma unroll
  for (int r = 0; r < FD_R; ++r) {
    const int k = mg + (XC_THREADS / FD_NC) * r, h = k / XC_DH;
    float t = 0.f;
#pragma unroll
    for (int j = 0; j < XC_DH; ++j) t = fmaf(a_s[k * XC_DH + j], wv_s[(h * XC_DH + j) * FD_NC + n], t);
    t_s[k * FD_NC + n] = t;
  }
  if (blockIdx.x == 0 && tid < XC_C) {
    float t = 0.f;
#pragma unroll
    for (int j = 0; j < XC_DH; ++j) t = fmaf(a_s[tid * XC_DH + j], bv[(tid / XC_DH) * XC_DH + j], t);
    tb_s[tid] = t;
  }
  float acc[FD_R];
#pragma unroll
  for (int r = 0; r < FD_R; ++r) acc[r] = 0.f;
  float cacc = 0.f;
  for (int k0 = 0; k0 < XC_C; k0 += FD_KC) {
    __syncthreads();                                           // t_s / tb_s are written; the previous stage's reads are done
    for (int e = tid; e < XC_C * (FD_KC / 4); e += XC_THREADS) {
      const int m = e / (FD_KC / 4), q = e % (FD_KC / 4);
      *reinterpret_cast<f32x4*>(wp_s + m * FD_WLD + 4 * q) = *reinterpret_cast<const f32x4*>(wp + m * XC_C + k0 + 4 * q);
    }
    __syncthreads();
#pragma unroll 2
    for (int kk = 0; kk < FD_KC; kk += 4) {
      float tv[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) tv[e] = t_s[(k0 + kk + e) * FD_NC + n];
#pragma unroll
      for (int r = 0; r < FD_R; ++r) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(wp_s + (mg + (XC_THREADS / FD_NC) * r) * FD_WLD + kk);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[r] = fmaf(w[e], tv[e], acc[r]);
      }
    }
    if (blockIdx.x == 0 && tid < XC_C)
      for (int kk = 0; kk < FD_KC; ++kk) cacc = fmaf(wp_s[tid * FD_WLD + kk], tb_s[k0 + kk], cacc);
  }
  float* Mb = M + b * XC_C * XC_C;
#pragma unroll
  for (int r = 0; r < FD_R; ++r) Mb[(mg + (XC_THREADS / FD_NC) * r) * XC_C + n0 + n] = acc[r];
  if (blockIdx.x == 0 && tid < XC_C) c[b * XC_C + tid] = cacc + bp[tid];
}

// [b, e) byte ranges of M rows of C floats with row stride ld
struct row_range { const char *b, *e; };
row_range rows_of(const float* p, long long ld, long long M, int C) {
  return {reinterpret_cast<const char*>(p), reinterpret_cast<const char*>(p + (M - 1) * ld + C)};
}
bool overlap(row_range a, row_range b) { return a.b < b.e && b.b < a.e; }
bool overlap(row_range a, const void* p, long long bytes) {
  return overlap(a, row_range{static_cast<const char*>(p), static_cast<const char*>(p) + bytes});
}

long long lpi_blocks(int H, int W) { return (long long)((H + LP_TY - 1) / LP_TY) * ((W + LP_TX - 1) / LP_TX); }
// partials [B][blocks][16] doubles, then mean | rstd [B][16] floats
long long lpi_part_bytes(int B, int H, int W) { return (long long)B * lpi_blocks(H, W) * LP_STAT * (long long)sizeof(double); }

// the checks the two LPI entries share: sizes, widths, the grid and pixel-count limits
int lpi_check_shape(int B, int H, int W, int C) {
  if (B <= 0 || H <= 0 || W <= 0 || C < 4) return PFK_ERR_BAD_ARG;
  if (C & 3) return PFK_ERR_ALIGNMENT;
  if (C != XC_C || B > 65535 || (H + LP_TY - 1) / LP_TY > 65535 || !pfk_fits32((long long)B * H * W)) return PFK_ERR_UNSUPPORTED;
  return PFK_OK;
}

}  // namespace

extern "C" {

int pfk_layernorm_rows_f32(const float* in, long long in_ld, const float* weight, const float* bias, float eps, float* out,
                           long long out_ld, long long M, int C, pfk_stream_t stream) {
  if (!in || !out || M <= 0 || C < 4 || in_ld < C || out_ld < C || !(eps >= 0.f)) return PFK_ERR_BAD_ARG;
  if ((C & 3) || (in_ld & 3) || (out_ld & 3) || !pfk_aligned16(in) || !pfk_aligned16(out) || (weight && !pfk_aligned16(weight)) ||
      (bias && !pfk_aligned16(bias)))
    return PFK_ERR_ALIGNMENT;
  if (C > LN_MAX_C) return PFK_ERR_UNSUPPORTED;
  const long long blocks = (M + XC_THREADS / 64 - 1) / (XC_THREADS / 64);
  if (!pfk_fits_int(blocks)) return PFK_ERR_UNSUPPORTED;
  // in place (the same rows) is fine: a wave holds its row before it writes it; any other overlap is not
  if (!(in == out && in_ld == out_ld) && overlap(rows_of(in, in_ld, M, C), rows_of(out, out_ld, M, C))) return PFK_ERR_BAD_ARG;
  hipLaunchKernelGGL(layernorm_rows_kernel, dim3((unsigned)blocks), dim3(XC_THREADS), 0, static_cast<hipStream_t>(stream), in, in_ld,
                     weight, bias, eps, out, out_ld, M, C);
  return pfk_launch_status();
}

long long pfk_xca_map_workspace_bytes(int B, long long N, int heads, int dh) {
  if (B <= 0 || N <= 0 || heads <= 0 || dh <= 0) return PFK_ERR_BAD_ARG;
  if (heads != XC_HEADS || dh != XC_DH) return PFK_ERR_UNSUPPORTED;
  return (long long)B * ((N + XCA_CHUNK - 1) / XCA_CHUNK) * XCA_PART * (long long)sizeof(float);
}

int pfk_xca_map_f32(const float* qk, long long qk_ld, const float* temperature, float* A, void* workspace, long long workspace_bytes, int B,
                    long long N, int heads, int dh, pfk_stream_t stream) {
  if (!qk || !temperature || !A || !workspace || B <= 0 || N <= 0 || heads <= 0 || dh <= 0) return PFK_ERR_BAD_ARG;
  if (qk_ld < 2LL * heads * dh) return PFK_ERR_BAD_ARG;
  if (heads != XC_HEADS || dh != XC_DH) return PFK_ERR_UNSUPPORTED;
  if ((qk_ld & 3) || !pfk_aligned16(qk) || !pfk_aligned16(A) || !pfk_aligned16(workspace)) return PFK_ERR_ALIGNMENT;
  const long long nchunk = (N + XCA_CHUNK - 1) / XCA_CHUNK;
  if (B > 65535 || !pfk_fits32(N) || !pfk_fits32((long long)B * N)) return PFK_ERR_UNSUPPORTED;
  const long long need = pfk_xca_map_workspace_bytes(B, N, heads, dh);
  if (workspace_bytes < need) return PFK_ERR_BAD_ARG;
  const row_range q = rows_of(qk, qk_ld, (long long)B * N, XCA_QK);
  const long long a_bytes = (long long)B * XCA_GRAM * (long long)sizeof(float);
  if (overlap(q, A, a_bytes) || overlap(q, workspace, need) || overlap(row_range{(const char*)A, (const char*)A + a_bytes}, workspace, need))
    return PFK_ERR_BAD_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(workspace);
  hipLaunchKernelGGL(xca_partial_kernel, dim3((unsigned)nchunk, (unsigned)B), dim3(XC_THREADS), 0, st, qk, qk_ld, part, (int)N, (int)nchunk);
  if (pfk_launch_status() != PFK_OK) return PFK_ERR_LAUNCH;
  hipLaunchKernelGGL(xca_finish_kernel, dim3(XC_HEADS, (unsigned)B), dim3(XC_THREADS), 0, st, part, temperature, A, (int)nchunk);
  return pfk_launch_status();
}

long long pfk_xcit_lpi_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return PFK_ERR_BAD_ARG;
  return lpi_part_bytes(B, H, W) + (long long)B * LP_STAT * (long long)sizeof(float);
}

int pfk_xcit_lpi1_f32(const float* x, long long x_ld, const float* ln_weight, const float* ln_bias, float ln_eps, const float* dw_weight,
                      const float* dw_bias, float* u, long long u_ld, void* workspace, long long workspace_bytes, int B, int H, int W,
                      int C, pfk_stream_t stream) {
  if (!x || !ln_weight || !ln_bias || !dw_weight || !dw_bias || !u || !workspace || !(ln_eps >= 0.f)) return PFK_ERR_BAD_ARG;
  const int shape = lpi_check_shape(B, H, W, C);
  if (shape == PFK_ERR_BAD_ARG || x_ld < C || u_ld < C) return PFK_ERR_BAD_ARG;
  if (shape != PFK_OK) return shape;
  if ((x_ld & 3) || (u_ld & 3) || !pfk_aligned16(x) || !pfk_aligned16(u) || !pfk_aligned16(ln_weight) || !pfk_aligned16(ln_bias) ||
      !pfk_aligned16(dw_bias) || !pfk_aligned16(workspace))
    return PFK_ERR_ALIGNMENT;
  const long long need = pfk_xcit_lpi_workspace_bytes(B, H, W);
  if (workspace_bytes < need) return PFK_ERR_BAD_ARG;
  const long long M = (long long)B * H * W;
  // other blocks still read the halo of pixels this block has written: u (and the workspace) apart from the input rows
  const row_range xr = rows_of(x, x_ld, M, C), ur = rows_of(u, u_ld, M, C);
  if (overlap(xr, ur) || overlap(xr, workspace, need) || overlap(ur, workspace, need)) return PFK_ERR_BAD_ARG;
  dim3 grid((unsigned)((W + LP_TX - 1) / LP_TX), (unsigned)((H + LP_TY - 1) / LP_TY), (unsigned)B);
  hipLaunchKernelGGL(lpi1_kernel, grid, dim3(XC_THREADS), 0, static_cast<hipStream_t>(stream), x, x_ld, ln_weight, ln_bias, ln_eps,
                     dw_weight, dw_bias, u, u_ld, static_cast<double*>(workspace), H, W);
  return pfk_launch_status();
}

int pfk_xcit_lpi2_f32(const float* u, long long u_ld, const float* gn_weight, const float* gn_bias, float gn_eps, int groups,
                      const float* dw_weight, const float* dw_bias, const float* gamma, const float* x, long long x_ld, float* x2,
                      long long x2_ld, const float* ln_weight, const float* ln_bias, float ln_eps, float* t, long long t_ld, void* workspace,
                      long long workspace_bytes, int B, int H, int W, int C, pfk_stream_t stream) {
  if (!u || !gn_weight || !gn_bias || !dw_weight || !dw_bias || !gamma || !x || !x2 || !t || !workspace || groups <= 0 ||
      !(gn_eps >= 0.f) || !(ln_eps >= 0.f))
    return PFK_ERR_BAD_ARG;
  const int shape = lpi_check_shape(B, H, W, C);
  if (shape == PFK_ERR_BAD_ARG || u_ld < C || x_ld < C || x2_ld < C || t_ld < C) return PFK_ERR_BAD_ARG;
  if (shape != PFK_OK) return shape;
  if (groups != XC_GROUPS) return PFK_ERR_UNSUPPORTED;
  if ((u_ld & 3) || (x_ld & 3) || (x2_ld & 3) || (t_ld & 3) || !pfk_aligned16(u) || !pfk_aligned16(x) || !pfk_aligned16(x2) ||
      !pfk_aligned16(t) || !pfk_aligned16(gn_weight) || !pfk_aligned16(gn_bias) || !pfk_aligned16(dw_bias) || !pfk_aligned16(gamma) ||
      (ln_weight && !pfk_aligned16(ln_weight)) || (ln_bias && !pfk_aligned16(ln_bias)) || !pfk_aligned16(workspace))
    return PFK_ERR_ALIGNMENT;
  const long long need = pfk_xcit_lpi_workspace_bytes(B, H, W);
  if (workspace_bytes < need) return PFK_ERR_BAD_ARG;
  const long long M = (long long)B * H * W;
  // u is read with a halo: no output on it; the outputs apart from each other, from x and from the workspace
  const row_range ur = rows_of(u, u_ld, M, C), xr = rows_of(x, x_ld, M, C), x2r = rows_of(x2, x2_ld, M, C), tr = rows_of(t, t_ld, M, C);
  if (overlap(ur, x2r) || overlap(ur, tr) || overlap(x2r, tr) || overlap(xr, x2r) || overlap(xr, tr) || overlap(ur, workspace, need) ||
      overlap(xr, workspace, need) || overlap(x2r, workspace, need) || overlap(tr, workspace, need))
    return PFK_ERR_BAD_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const double* part = static_cast<const double*>(workspace);
  float* stats = reinterpret_cast<float*>(static_cast<char*>(workspace) + lpi_part_bytes(B, H, W));
  hipLaunchKernelGGL(gn_finish_kernel, dim3((unsigned)B), dim3(XC_THREADS), 0, st, part, (int)lpi_blocks(H, W),
                     (double)(C / groups) * H * W, gn_eps, stats);
  if (pfk_launch_status() != PFK_OK) return PFK_ERR_LAUNCH;
  dim3 grid((unsigned)((W + LP_TX - 1) / LP_TX), (unsigned)((H + LP_TY - 1) / LP_TY), (unsigned)B);
  hipLaunchKernelGGL(lpi2_kernel, grid, dim3(XC_THREADS), 0, st, u, u_ld, stats, gn_weight, gn_bias, dw_weight, dw_bias, gamma, x, x_ld,
                     x2, x2_ld, ln_weight, ln_bias, ln_eps, t, t_ld, H, W);
  return pfk_launch_status();
}

// the checks the two token entries share (`in_bytes`: the extent of the input as the entry addresses it)
static int tokens_check(const float* in, long long in_bytes, const float* pos, float eps, float* x0, long long x0_ld, float* xh,
                        long long xh_ld, int B, int C, int H, int W) {
  if (!in || !x0 || !xh || B <= 0 || H <= 0 || W <= 0 || C < 4 || !(eps >= 0.f)) return PFK_ERR_BAD_ARG;
  if (x0_ld < C || xh_ld < C) return PFK_ERR_BAD_ARG;
  if (C & 3) return PFK_ERR_ALIGNMENT;
  const long long N = (long long)H * W;
  if (C != XC_C || B > 65535 || !pfk_fits32((long long)B * N) || N >= 0x7fffffffLL - TK_PX) return PFK_ERR_UNSUPPORTED;
  if ((x0_ld & 3) || (xh_ld & 3) || !pfk_aligned16(x0) || !pfk_aligned16(xh) || (pos && !pfk_aligned16(pos))) return PFK_ERR_ALIGNMENT;
  const row_range a = rows_of(x0, x0_ld, B * N, C), h = rows_of(xh, xh_ld, B * N, C);
  if (overlap(a, h) || overlap(a, in, in_bytes) || overlap(h, in, in_bytes)) return PFK_ERR_BAD_ARG;
  if (pos && (overlap(a, pos, N * C * 4) || overlap(h, pos, N * C * 4))) return PFK_ERR_BAD_ARG;
  return PFK_OK;
}

int pfk_xcit_tokens_f32(const float* in, const float* pos, float eps, float* x0, long long x0_ld, float* xh, long long xh_ld, int B, int C,
                        int H, int W, pfk_stream_t stream) {
  const int st = tokens_check(in, (long long)B * C * H * W * 4, pos, eps, x0, x0_ld, xh, xh_ld, B, C, H, W);
  if (st != PFK_OK) return st;
  const long long N = (long long)H * W;
  dim3 grid((unsigned)((N + TK_PX - 1) / TK_PX), (unsigned)B);
  hipLaunchKernelGGL(tokens_nchw_kernel, grid, dim3(XC_THREADS), 0, static_cast<hipStream_t>(stream), in, pos, eps, x0, x0_ld, xh, xh_ld,
                     (int)N);
  return pfk_launch_status();
}

int pfk_xcit_tokens_pm_f32(const float* in, long long in_ld, const float* pos, float eps, float* x0, long long x0_ld, float* xh,
                           long long xh_ld, int B, int C, int H, int W, pfk_stream_t stream) {
  if (in && C > 0 && in_ld < C) return PFK_ERR_BAD_ARG;
  const long long rows = (long long)B * H * W;
  const int st = tokens_check(in, rows > 0 ? ((rows - 1) * in_ld + C) * 4 : 0, pos, eps, x0, x0_ld, xh, xh_ld, B, C, H, W);
  if (st != PFK_OK) return st;
  if ((in_ld & 3) || !pfk_aligned16(in)) return PFK_ERR_ALIGNMENT;
  const long long N = (long long)H * W;
  dim3 grid((unsigned)((N + XC_THREADS / 32 - 1) / (XC_THREADS / 32)), (unsigned)B);
  hipLaunchKernelGGL(tokens_pm_kernel, grid, dim3(XC_THREADS), 0, static_cast<hipStream_t>(stream), in, in_ld, pos, eps, x0, x0_ld, xh,
                     xh_ld, (int)N);
  return pfk_launch_status();
}

int pfk_xca_fold_f32(const float* A, const float* wv, const float* bv, const float* wp, const float* bp, float* M, float* c, int B,
                     int heads, int dh, pfk_stream_t stream) {
  if (!A || !wv || !bv || !wp || !bp || !M || !c || B <= 0 || heads <= 0 || dh <= 0) return PFK_ERR_BAD_ARG;
  if (heads != XC_HEADS || dh != XC_DH || B > 65535) return PFK_ERR_UNSUPPORTED;
  if (!pfk_aligned16(A) || !pfk_aligned16(wv) || !pfk_aligned16(bv) || !pfk_aligned16(wp) || !pfk_aligned16(bp) || !pfk_aligned16(M) ||
      !pfk_aligned16(c))
    return PFK_ERR_ALIGNMENT;
  const long long m_bytes = (long long)B * XC_C * XC_C * 4, c_bytes = (long long)B * XC_C * 4, w_bytes = (long long)XC_C * XC_C * 4;
  const row_range mr = {(const char*)M, (const char*)M + m_bytes}, cr = {(const char*)c, (const char*)c + c_bytes};
  if (overlap(mr, c, c_bytes)) return PFK_ERR_BAD_ARG;
  for (const row_range& o : {mr, cr})
    if (overlap(o, A, (long long)B * XCA_GRAM * 4) || overlap(o, wv, w_bytes) || overlap(o, wp, w_bytes) || overlap(o, bv, XC_C * 4) ||
        overlap(o, bp, XC_C * 4))
      return PFK_ERR_BAD_ARG;
  hipLaunchKernelGGL(xca_fold_kernel, dim3(XC_C / FD_NC, (unsigned)B), dim3(XC_THREADS), 0, static_cast<hipStream_t>(stream), A, wv, bv, wp,
                     bp, M, c);
  return pfk_launch_status();
}

}  // extern "C"
