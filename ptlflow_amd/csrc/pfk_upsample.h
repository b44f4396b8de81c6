// Convex upsampling — RAFT.upsample_flow (raft/raft.py:112-123) and SEARAFT.upsample_data (sea_raft.py:147-163) — the arithmetic of
// one (coarse pixel, sub-pixel), written ONCE: softmax over the nine mask logits, then the convex combination of the zero-padded 3x3
// neighbourhood of S x flow (and of the info channels, no factor).  S is the upsampling factor, a template argument of the geometry
// helpers that defaults to RAFT's 8; CCMR / MS-RAFT+ upsample by 2 (ccmr/ccmr.py:128-139, `scale=2`: 9 * 4 = 36 mask channels).
// Every kernel that upsamples or differentiates the upsampling
// calls these helpers: the unfused forwards and the two backward kernels (pfk_upsample.hip), the fused mask-head kernels K13
// (pfk_gemm.hip) and K13b (pfk_gemm_b16.hip).  That is what makes their promises hold — fused = unfused, four pixels per wave = one
// pixel per wave, the info kernel's flow = the plain kernel's, the training node's forward = the inference kernel — bit for bit
// (tests/test_gpu_upsample_bits.py holds the bits themselves).
//
// Contraction: in the unfused pair the mask goes through memory between the convolution and the upsampling, and the unfused kernels
// are compiled with -ffp-contract=off, so NOTHING here may be contracted into an FMA.  pfk_gemm*.hip are compiled with contraction on
// and HIP's __fmul_rn / __fadd_rn are plain operators (they do not stop it), hence every helper carries
// `#pragma clang fp contract(off)` in its body: the result does not depend on the flags of the including file.
#pragma once
#include "pfk_common.h"

constexpr int UP_MAX_INFO = 8;   // info channels of upsample_data the kernels hold in registers

// Nine logits -> nine normalised weights, in place: max in tap order, expf(m - max), sum in tap order, ONE reciprocal, e * inv.
__device__ __forceinline__ void up_softmax9(float (&m)[9]) {
#pragma clang fp contract(off)
  float mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < 9; ++k) mx = fmaxf(mx, m[k]);
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) { m[k] = expf(m[k] - mx); sum = sum + m[k]; }
  const float inv = 1.0f / sum;
#pragma unroll
  for (int k = 0; k < 9; ++k) m[k] = m[k] * inv;
}

// sum_k w[k] * v[k] in tap order, a multiply then an add: flow x, flow y and every info channel
__device__ __forceinline__ float up_combine(const float (&w)[9], const float (&v)[9]) {
#pragma clang fp contract(off)
  float a = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const float t = w[k] * v[k];
    a = a + t;
  }
  return a;
}

// the conv epilogue's + bias, x scale on one logit of the fused kernels (pfk_gemm.h, LINEAR), un-contracted
__device__ __forceinline__ float mask_logit(float acc, float bias, float sc) {
#pragma clang fp contract(off)
  float v = acc + bias;
  v = v * sc;
  return v;
}

// pixel p of a [B][H][W] grid
struct UpPixel { long long b; int y, x; };
__device__ __forceinline__ UpPixel up_pixel(long long p, int H, int W) {
  const long long hw = (long long)H * W;
  const long long b = p / hw;
  const int pix = (int)(p - b * hw);
  const int y = pix / W;
  return {b, y, pix - y * W};
}

// sub-pixel (sy, sx) of coarse pixel (y, x) inside one [S H][S W] plane
template <int S = 8>
__device__ __forceinline__ long long up_out_offset(int y, int x, int sy, int sx, int W) {
  return (long long)(S * y + sy) * (S * W) + S * x + sx;
}

// Neighbour k = 3 (dy + 1) + (dx + 1) of pixel (y, x) of the image whose first pixel has index img = b * H * W: v[0..1] = S x flow
// (exact: a power of two), v[2 + i] = info channel i < n_info; zero outside the image (F.unfold's padding).  Flow NCHW (flow_ld == 0)
// or pixel-major rows (flow_ld >= 2); info rows.  One tap per call; the caller makes the product img once for the nine taps, and the
// two flow layouts differ in the addresses only, so the two loads of a tap issue together.
template <int NI, int S = 8>
__device__ __forceinline__ void up_tap(int k, const float* __restrict__ flow, int flow_ld, const float* __restrict__ info, int info_ld,
                                       int n_info, long long img, int y, int x, int H, int W, float (&v)[2 + NI]) {
  const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
#pragma unroll
  for (int c = 0; c < 2 + NI; ++c) v[c] = 0.f;
  if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) {
    const long long q = img + (long long)yy * W + xx;
    const float* fx = flow_ld > 0 ? flow + q * flow_ld : flow + q + img;
    const float* fy = flow_ld > 0 ? fx + 1 : fx + (long long)H * W;
    v[0] = (float)S * *fx;
    v[1] = (float)S * *fy;
    if (NI > 0) {
      const float* fi = info + q * info_ld;
#pragma unroll
      for (int i = 0; i < NI; ++i)
        if (i < n_info) v[2 + i] = fi[i];
    }
  }
}

// The epilogue of the fused mask-head kernels (K13 mask_upsample_kernel, K13b mask_upsample_b16_kernel; geometry: pfk_gemm.hip).  A
// block holds 128 pixels x 16 sub-pixels (quarter) x nine taps in acc[0][0..4]: four waves stacked in M at wm0 = 32 * wave, column c
// of tile j = tap 2j + (c >> 4) of sub-pixel c & 15 (the tenth tap is a zero weight row), so the nine logits of a (pixel, sub-pixel)
// sit in the lanes c and c ^ 16 of the same accumulator registers.  nf = the block's staging LDS, free behind the K loop's last
// barrier: [128][9] 8 x flow neighbourhoods.  BF16_LOGITS: every logit is rounded to bf16 where the unfused K8b launch stores it.
template <bool BF16_LOGITS>
__device__ __forceinline__ void mask_upsample_epilogue(const f32x16 (&acc)[1][5], f32x2* nf, const float* __restrict__ bias_perm, float sc,
                                                       const float* __restrict__ flow, int flow_ld, float* __restrict__ out, int Hi, int Wi,
                                                       long long M, unsigned wo_mul, int wo_sh, unsigned ho_mul, int ho_sh, long long m0,
                                                       int quarter, int wm0) {
  constexpr int BM = 128, NT = 5;
  const int tid = threadIdx.x, lane = tid & 63;
  const unsigned H = (unsigned)Hi, W = (unsigned)Wi;
  for (int e = tid; e < BM * 9; e += 256) {
    const int pl = e / 9, k = e - pl * 9;
    const unsigned p = (unsigned)m0 + (unsigned)pl;
    f32x2 v = {0.f, 0.f};
    if ((long long)p < M) {
      // (restates conv_pixel of pfk_gemm.h for stride 1, here and below: this epilogue gets loose scalars, no argument block)
      const unsigned prow = fastdiv_u32(p, wo_mul, wo_sh);          // b*H + y
      const unsigned bimg = fastdiv_u32(prow, ho_mul, ho_sh);
      const int x = (int)(p - prow * W), y = (int)(prow - bimg * H);
      const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
      if ((unsigned)yy < H && (unsigned)xx < W) {
        const float* f = flow + ((size_t)(bimg * H + (unsigned)yy) * W + (unsigned)xx) * (size_t)flow_ld;
        v[0] = 8.0f * f[0];
        v[1] = 8.0f * f[1];
      }
    }
    nf[e] = v;
  }
  __syncthreads();

  const int col = lane & 31;
  const int odd = col >> 4;                          // this lane's own taps are 2j + odd
  const int s = quarter * 16 + (col & 15), sy = s >> 3, sx = s & 7;
  float bias[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) bias[j] = bias_perm != nullptr ? bias_perm[quarter * (NT * 32) + j * 32 + col] : 0.f;
  const size_t HW8 = (size_t)H * W * 64;
  // The two lanes of a pair split the ROWS: of every row pair (r, r + 1) the lane with the even taps finishes row r, its partner
  // row r + 1 — one exchange per tile and row pair serves both (each lane sends the logits of the row the other finishes and
  // receives those of its own), and each lane runs the softmax (9 expf) for 8 of the wave tile's 16 rows instead of all 16.
#pragma unroll
  for (int r = 0; r < 16; r += 2) {
    const int rr = r + odd;                          // the row this lane finishes
    const int row = wm0 + (rr & 3) + 8 * (rr >> 2) + 4 * (lane >> 5);
    const unsigned p = (unsigned)m0 + (unsigned)row;
    float own[NT], oth[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      float l0 = mask_logit(acc[0][j][r], bias[j], sc), l1 = mask_logit(acc[0][j][r + 1], bias[j], sc);
      if (BF16_LOGITS) { l0 = (float)(__bf16)l0; l1 = (float)(__bf16)l1; }
      own[j] = odd ? l1 : l0;                        // tap 2j + odd of my row
      oth[j] = __shfl_xor(odd ? l0 : l1, 16, 64);    // send the partner's row, receive tap 2j + (1 - odd) of mine
    }
    float w[9], vx[9], vy[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int j = k >> 1;
      w[k] = ((k & 1) == odd) ? own[j] : oth[j];     // (tap 9 — tile 4 of the odd lanes — is the zero pad row: never read)
      const f32x2 f = nf[row * 9 + k];
      vx[k] = f[0];
      vy[k] = f[1];
    }
    up_softmax9(w);
    const float ox = up_combine(w, vx), oy = up_combine(w, vy);
    if ((long long)p < M) {
      const unsigned prow = fastdiv_u32(p, wo_mul, wo_sh);
      const unsigned bimg = fastdiv_u32(prow, ho_mul, ho_sh);
      const unsigned x = p - prow * W, y = prow - bimg * H;
      const size_t o = (size_t)up_out_offset((int)y, (int)x, sy, sx, Wi);
      out[((size_t)bimg * 2 + 0) * HW8 + o] = ox;
      out[((size_t)bimg * 2 + 1) * HW8 + o] = oy;
    }
  }
}
