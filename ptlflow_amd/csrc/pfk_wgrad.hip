// Weight gradient of the implicit-GEMM convolution: the transposed product
//
//   dW[co][k] = sum_p dY[p][co] * A[p][k],     A[p][k = (source, tap, channel)] = src_s[p + tap][c]  (zero outside the image)
//
// on the fp32 matrix cores, straight from the pixel-major tensors of the forward pass — no im2col, no transposes.  The
// reduction index is the PIXEL: a K-step is 32 consecutive pixels, staged as they lie in memory (dY: 32 rows x 128 output
// channels, A: 32 rows x 32 input channels of one (source, tap, chunk), with the tap's zero padding done by out-of-range
// buffer offsets exactly as in the forward kernel).  v_mfma_f32_32x32x2_f32 wants A[i = co][k = pixel] and B[k = pixel][j = c]:
// lane l reads LDS element [pixel 2j + (l >> 5)][l & 31] with ds_read_b32 — each half-wave reads 32 consecutive floats of
// one row, conflict-free — one read pair per MFMA.
//
// Grid: (cout tiles) x (groups of K chunks) x (pixel splits); a tile is 32*CB output channels x 32*(4/CB) K columns, CB in
// {4, 2, 1} picked per launch to pad cout the least.  The output has few tiles and a very long reduction (zr of RAFT: 2 x 60
// tiles, 22 816+ pixels), so the pixel range is cut into `splits` slices that write partial tiles to a workspace; a second kernel
// adds the slices in a fixed order (deterministic, no atomics) into the packed [cout][ktot] layout of the forward weight.
// (A 128 x 128 tile with 64x64 wave tiles — half the LDS reads per MFMA — measured 5-30 % SLOWER on every training shape:
// the loop is not LDS-bound, fewer resident waves per SIMD hurt more.)
#include "pfk_launch.h"
#include "pfk_wgrad_reduce.h"   // wgrad_reduce_unpack_kernel: the slice reduction into PyTorch's layouts, shared with pfk_wgrad_b16.hip

namespace {

constexpr unsigned OOB = 0x80000000u;

struct WgradArgs {
  const float* src0; const float* src1; const float* src2;
  int ld0, ld1, ld2, ch0, ch1, ch2, nsrc;
  const float* dy; int dy_ld; int cout;
  int H, W, kh, kw;
  int Ho, Wo, stride;     // output grid (dY rows = B*Ho*Wo = M); output (yo, xo) reads input (yo*stride + dy, xo*stride + dx)
  long long M;
  float* part;            // [splits][cout][ktot]  (== the output when splits == 1)
  int ktot, chunks, tiles_m;   // ktot / chunks include the bias chunk when with_bias
  int with_bias;               // one extra 32-column chunk whose column 0 is sum_p dY[p][co] (A = a column of ones): the bias gradient
  long long px_per_split; // multiple of 32
};

// CB = 32-row output-channel blocks per tile (4, 2 or 1); the block's four waves cover CB co-blocks x NCH = 4 / CB consecutive K
// chunks, one 32x32 accumulator each, so the tile is (32 CB) output channels x (32 NCH) K columns.  The host picks CB to waste
// the fewest MFMAs on channel padding (cout = 64: CB 2, not half-empty 128-row tiles; 96 and 192: three exact 32- / 64-row tiles).
template <int CB>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(const WgradArgs a) {
  constexpr int NCH = 4 / CB, CO = 32 * CB, KC = 32 * NCH;
  __shared__ __attribute__((aligned(16))) float sY[2][32][CO];
  __shared__ __attribute__((aligned(16))) float sX[2][32][KC];

  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int groups = (a.chunks + NCH - 1) / NCH;
  const int grp = blockIdx.x % groups;
  const int tile_m = blockIdx.x / groups;
  const int split = blockIdx.y;
  const int co0 = tile_m * CO;

  const __amdgpu_buffer_rsrc_t rsy = buffer_rsrc(a.dy);
  const long long p_begin = (long long)split * a.px_per_split;
  const long long p_end = min(a.M, p_begin + a.px_per_split);
  const int steps = p_end > p_begin ? (int)((p_end - p_begin + 31) >> 5) : 0;

  // this thread stages row (t >> 3) of every step: float4 q of each of the NCH A chunks, float4 q + 8*i of the dY tile
  const int row = t >> 3, q = t & 7;
  long long p = p_begin + row;                     // output pixel (= dY row); its input pixel is (b, y*stride, x*stride)
  int x = (int)(p % a.Wo), y = (int)((p / a.Wo) % a.Ho), bimg = (int)(p / ((long long)a.Wo * a.Ho));
  const int sd = a.stride;
  __amdgpu_buffer_rsrc_t rsx[NCH];
  int tap_off[NCH], cdy[NCH], cdx[NCH], cld[NCH];
  bool c_ok[NCH], is_bias[NCH], yok[CB];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const auto c = chunk_ref(a, grp * NCH + i);
    rsx[i] = buffer_rsrc(c.src);
    tap_off[i] = (c.dy * a.W + c.dx) * c.ld + c.c0 + q * 4;
    cdy[i] = c.dy; cdx[i] = c.dx; cld[i] = c.ld;
    c_ok[i] = c.live && !c.bias && c.c0 + q * 4 < c.cch;
    is_bias[i] = c.bias;
  }
#pragma unroll
  for (int i = 0; i < CB; ++i) yok[i] = co0 + q * 4 + 32 * i < a.cout;

  u32x4 rx[NCH], ry[CB];
  auto load = [&](void) {
    const bool in = p < p_end;
    const int yi = y * sd, xi = x * sd;
    const int pin = (bimg * a.H + yi) * a.W + xi;   // input pixel index (== p for stride 1)
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const bool ok = in && c_ok[i] && (unsigned)(yi + cdy[i]) < (unsigned)a.H && (unsigned)(xi + cdx[i]) < (unsigned)a.W;
      if (is_bias[i]) rx[i] = u32x4{(in && q == 0) ? 0x3f800000u : 0u, 0u, 0u, 0u};    // A = [1 0 0 ...] for every live pixel
      else rx[i] = __builtin_amdgcn_raw_buffer_load_b128(rsx[i], ok ? (unsigned)(pin * cld[i] + tap_off[i]) * 4u : OOB, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < CB; ++i)
      ry[i] = __builtin_amdgcn_raw_buffer_load_b128(rsy, (in && yok[i]) ? (unsigned)((int)p * a.dy_ld + co0 + q * 4 + 32 * i) * 4u : OOB, 0, 0);
    p += 32;
    x += 32;
    while (x >= a.Wo) { x -= a.Wo; if (++y == a.Ho) { y = 0; ++bimg; } }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) *reinterpret_cast<u32x4*>(&sX[buf][row][q * 4 + 32 * i]) = rx[i];
#pragma unroll
    for (int i = 0; i < CB; ++i) *reinterpret_cast<u32x4*>(&sY[buf][row][q * 4 + 32 * i]) = ry[i];
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
  const int wco = (wid % CB) * 32, wkc = (wid / CB) * 32;      // this wave's co block / chunk inside the tile
  for (int s = 0; s < steps; ++s) {
    const int buf = s & 1;
    const bool more = s + 1 < steps;
    if (more) load();
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float av = sY[buf][2 * j + hl][wco + l31];
      const float bv = sX[buf][2 * j + hl][wkc + l31];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
    }
    if (more) store(buf ^ 1);
    __syncthreads();
  }

  // D: column j = lane & 31 (input channel), rows i = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5) (output channel)
  const int chunk = grp * NCH + wid / CB;
  if (chunk >= a.chunks) return;
  float* out = a.part + (long long)split * a.cout * a.ktot;
  const int kcol = chunk * 32 + l31;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int co = co0 + wco + (e & 3) + 8 * (e >> 2) + 4 * hl;
    if (co < a.cout) out[(long long)co * a.ktot + kcol] = acc[e];
  }
}

__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                           long long n, int splits) {
  const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= n) return;
  f32x4 s = *reinterpret_cast<const f32x4*>(part + i);
  for (int k = 1; k < splits; ++k) s += *reinterpret_cast<const f32x4*>(part + (long long)k * n + i);
  *reinterpret_cast<f32x4*>(out + i) = s;
}

// ------------------------------------------------------------------------------------------------------------------
// Gate arithmetic of one (Sep)ConvGRU pass for the training path (raft/update.py:24-32, 58-73), float4 per thread over
// pixel-major [M][C] tensors.  Forward keeps what the backward needs (z, r, q); the derivative kernels produce the
// pre-activation gradients the dgrad / wgrad convolutions consume.
//   f1: z = s(a_z), r = s(a_r), rh = r*h               f2: q = tanh(a_q), h' = (1-z)*h + z*q
//   b1: da_q = dh'*z*(1-q^2), da_z = dh'*(q-h)*z*(1-z), dh = dh'*(1-z)
//   b2: da_r = d(rh)*h*r*(1-r), dh += d(rh)*r
// ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ f32x4 sigmoid4(f32x4 v) {
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = sigmoid_f(v[e]);
  return o;
}

__global__ __launch_bounds__(256) void gru_f1_kernel(const float* __restrict__ azr, const float* __restrict__ h, int h_ld,
                                                     float* __restrict__ z, float* __restrict__ r, float* __restrict__ rh,
                                                     long long M, int C) {
  const int tpr = C >> 2;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x, p = idx / tpr;
  if (p >= M) return;
  const int c = (int)(idx - p * tpr) * 4;
  const f32x4 zz = sigmoid4(load4_widen(azr + p * 2 * C + c)), rr = sigmoid4(load4_widen(azr + p * 2 * C + C + c));
  store4(z + p * C + c, zz);
  store4(r + p * C + c, rr);
  store4(rh + p * C + c, rr * load4_widen(h + p * h_ld + c));
}

__global__ __launch_bounds__(256) void gru_f2_kernel(const float* __restrict__ aq, const float* __restrict__ z,
                                                     const float* __restrict__ h, int h_ld, float* __restrict__ q,
                                                     float* __restrict__ hn, long long M, int C) {
  const int tpr = C >> 2;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x, p = idx / tpr;
  if (p >= M) return;
  const int c = (int)(idx - p * tpr) * 4;
  const f32x4 a = load4_widen(aq + p * C + c), zz = load4_widen(z + p * C + c), hh = load4_widen(h + p * h_ld + c);
  f32x4 qq;
#pragma unroll
  for (int e = 0; e < 4; ++e) qq[e] = tanhf(a[e]);
  store4(q + p * C + c, qq);
  store4(hn + p * C + c, (1.0f - zz) * hh + zz * qq);
}

__global__ __launch_bounds__(256) void gru_b1_kernel(const float* __restrict__ dhn, int dhn_ld, const float* __restrict__ z,
                                                     const float* __restrict__ q, const float* __restrict__ h, int h_ld,
                                                     float* __restrict__ daq, float* __restrict__ dazr, float* __restrict__ dh,
                                                     long long M, int C) {
  const int tpr = C >> 2;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x, p = idx / tpr;
  if (p >= M) return;
  const int c = (int)(idx - p * tpr) * 4;
  const f32x4 g = load4_widen(dhn + p * dhn_ld + c), zz = load4_widen(z + p * C + c), qq = load4_widen(q + p * C + c), hh = load4_widen(h + p * h_ld + c);
  store4(daq + p * C + c, g * zz * (1.0f - qq * qq));
  store4(dazr + p * 2 * C + c, g * (qq - hh) * zz * (1.0f - zz));
  store4(dh + p * C + c, g * (1.0f - zz));
}

__global__ __launch_bounds__(256) void gru_b2_kernel(const float* __restrict__ drh, const float* __restrict__ h, int h_ld,
                                                     const float* __restrict__ r, float* __restrict__ dazr, float* __restrict__ dh,
                                                     long long M, int C) {
  const int tpr = C >> 2;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x, p = idx / tpr;
  if (p >= M) return;
  const int c = (int)(idx - p * tpr) * 4;
  const f32x4 g = load4_widen(drh + p * C + c), hh = load4_widen(h + p * h_ld + c), rr = load4_widen(r + p * C + c);
  store4(dazr + p * 2 * C + C + c, g * hh * rr * (1.0f - rr));
  store4(dh + p * C + c, load4_widen(dh + p * C + c) + g * rr);
}

int g_wgrad_variant = 0;   // 0: tile height by padding waste (wgrad_pick_cb); 1 / 2 / 4: forced CB — pfk_debug_set_wgrad

// slices of M output pixels: K-steps of 32 pixels, at least 16 (512 pixels) per slice
int pick_splits(const WgradGrid& g, long long M) { return wgrad_pick_splits((long long)g.tiles_m * g.groups, M / 32, 16); }

}  // namespace

extern "C" {

int pfk_debug_set_wgrad(int variant) { if (!pfk_debug_knobs_enabled()) return PFK_ERR_DISABLED; g_wgrad_variant = variant; return PFK_OK; }

long long pfk_conv_wgrad_workspace_bytes(const pfk_conv_desc* d, int with_bias) {
  if (!d || d->num_src < 1 || d->num_src > 3 || d->cout <= 0) return 0;
  const int ktot = pfk_conv_k(d, 32) + (with_bias ? 32 : 0);
  const long long M = pfk_conv_geom(d).M_out;
  int splits = 1;
  for (int cb = 1; cb <= 4; cb *= 2) {        // any tile height may run (pfk_debug_set_wgrad): size for the largest split count
    const int sc = pick_splits(wgrad_grid(d->cout, ktot, cb), M);
    splits = sc > splits ? sc : splits;
  }
  return splits > 1 ? (long long)splits * d->cout * ktot * (long long)sizeof(float) : 0;
}

// Validate, fill the kernel arguments (everything but `part`) and pick the split count.
static int wgrad_plan(const pfk_conv_desc* d, const float* dy, int dy_ld, int with_bias, WgradArgs& a, WgradGrid& g, int& splits) {
  if (!d || !dy || d->num_src < 1 || d->num_src > 3) return PFK_ERR_BAD_ARG;
  if (d->B <= 0 || d->H <= 0 || d->W <= 0 || d->cout <= 0 || dy_ld < d->cout) return PFK_ERR_BAD_ARG;
  if (d->kh <= 0 || d->kw <= 0 || !(d->kh & 1) || !(d->kw & 1) || d->stride < 0) return PFK_ERR_BAD_ARG;
  if ((d->cout & 3) || (dy_ld & 3) || !pfk_aligned16(dy)) return PFK_ERR_ALIGNMENT;
  const pfk_conv_geometry geo = pfk_conv_geom(d);                // dY has M_out rows (the OUTPUT grid), the sources M_in
  for (int i = 0; i < d->num_src; ++i) {
    const int rc = pfk_check_source(d->src[i], 4, 16);
    if (rc != PFK_OK) return rc;
    if (!pfk_source_fits32(d->src[i], geo.M_in, 4)) return PFK_ERR_UNSUPPORTED;
  }
  if (!pfk_fits32(geo.M_out * dy_ld * 4)) return PFK_ERR_UNSUPPORTED;
  a = WgradArgs{};
  pfk_spread_sources(a, d);
  a.dy = dy; a.dy_ld = dy_ld; a.cout = d->cout;
  a.H = d->H; a.W = d->W; a.kh = d->kh; a.kw = d->kw; a.M = geo.M_out;
  a.Ho = geo.Ho; a.Wo = geo.Wo; a.stride = geo.stride;
  a.with_bias = with_bias ? 1 : 0;
  a.ktot = pfk_conv_k(d, 32) + (with_bias ? 32 : 0);
  a.chunks = a.ktot / 32;
  g = wgrad_grid(d->cout, a.ktot, wgrad_pick_cb(d->cout, g_wgrad_variant));
  a.tiles_m = g.tiles_m;
  splits = pick_splits(g, geo.M_out);
  a.px_per_split = ((geo.M_out + splits - 1) / splits + 31) / 32 * 32;
  return PFK_OK;
}

static void wgrad_run(const WgradArgs& a, const WgradGrid& g, int splits, hipStream_t st) {
  const dim3 grid((unsigned)(g.tiles_m * g.groups), (unsigned)splits);
  wgrad_launch_cb<conv_wgrad_kernel<4>, conv_wgrad_kernel<2>, conv_wgrad_kernel<1>>(g.cb, grid, st, a);
}

int pfk_conv_wgrad_f32(const pfk_conv_desc* d, const float* dy, int dy_ld, float* dw_packed, int with_bias, void* workspace,
                       long long workspace_bytes, pfk_stream_t stream) {
  if (!dw_packed) return PFK_ERR_BAD_ARG;
  if (!pfk_aligned16(dw_packed)) return PFK_ERR_ALIGNMENT;
  WgradArgs a;
  WgradGrid g;
  int splits;
  const int rc = wgrad_plan(d, dy, dy_ld, with_bias, a, g, splits);
  if (rc != PFK_OK) return rc;
  const long long n = (long long)d->cout * a.ktot;
  if (splits > 1) {
    if (!workspace || workspace_bytes < splits * n * (long long)sizeof(float) || !pfk_aligned16(workspace)) return PFK_ERR_BAD_ARG;
    a.part = static_cast<float*>(workspace);
  } else {
    a.part = dw_packed;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  wgrad_run(a, g, splits, st);
  if (splits > 1)
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, st,
                       static_cast<const float*>(workspace), dw_packed, n, splits);
  return pfk_launch_status();
}

long long pfk_conv_wgrad_unpacked_workspace_bytes(const pfk_conv_desc* d, int with_bias) {
  if (!d || d->num_src < 1 || d->num_src > 3 || d->cout <= 0) return 0;
  const long long packed = pfk_conv_wgrad_workspace_bytes(d, with_bias);
  const long long one = (long long)d->cout * (pfk_conv_k(d, 32) + (with_bias ? 32 : 0)) * (long long)sizeof(float);
  return packed > one ? packed : one;       // the slices always go through the workspace here, even a single one
}

int pfk_conv_wgrad_unpacked_f32(const pfk_conv_desc* d, const int* real_channels, const float* dy, int dy_ld, int cout_real,
                                float* dw, float* db, int accumulate, void* workspace, long long workspace_bytes, pfk_stream_t stream) {
  if (!dw || !real_channels || !workspace || cout_real <= 0 || !d || cout_real > d->cout) return PFK_ERR_BAD_ARG;
  if (!pfk_aligned16(workspace)) return PFK_ERR_ALIGNMENT;
  const int with_bias = db != nullptr;
  WgradArgs a;
  WgradGrid g;
  int splits;
  const int rc = wgrad_plan(d, dy, dy_ld, with_bias, a, g, splits);
  if (rc != PFK_OK) return rc;
  const long long n = (long long)d->cout * a.ktot;
  if (workspace_bytes < splits * n * (long long)sizeof(float)) return PFK_ERR_BAD_ARG;
  a.part = static_cast<float*>(workspace);
  for (int i = 0; i < d->num_src; ++i)
    if (real_channels[i] <= 0 || real_channels[i] > d->src[i].channels) return PFK_ERR_BAD_ARG;
  const UnpackArgs u = wgrad_unpack_args(d, real_channels, a.part, n, splits, a.ktot, cout_real, with_bias, dw, db, accumulate);
  hipStream_t st = static_cast<hipStream_t>(stream);
  wgrad_run(a, g, splits, st);
  const long long total = (long long)cout_real * a.ktot;
  hipLaunchKernelGGL(wgrad_reduce_unpack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, u);
  return pfk_launch_status();
}

static int gru_grid(long long M, int C, dim3* grid) {
  if (M <= 0 || C <= 0 || (C & 3)) return PFK_ERR_BAD_ARG;
  const long long blocks = (M * (C >> 2) + 255) / 256;
  if (!pfk_fits_int(blocks)) return PFK_ERR_UNSUPPORTED;
  *grid = dim3((unsigned)blocks);
  return PFK_OK;
}

int pfk_gru_gates_zr_f32(const float* a_zr, const float* h, int h_ld, float* z, float* r, float* rh, long long M, int C,
                         pfk_stream_t stream) {
  dim3 grid;
  if (!a_zr || !h || !z || !r || !rh || (h_ld & 3) || h_ld < C) return PFK_ERR_BAD_ARG;
  const int rc = gru_grid(M, C, &grid);
  if (rc != PFK_OK) return rc;
  hipLaunchKernelGGL(gru_f1_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), a_zr, h, h_ld, z, r, rh, M, C);
  return pfk_launch_status();
}

int pfk_gru_gates_q_f32(const float* a_q, const float* z, const float* h, int h_ld, float* q, float* h_new, long long M, int C,
                        pfk_stream_t stream) {
  dim3 grid;
  if (!a_q || !z || !h || !q || !h_new || (h_ld & 3) || h_ld < C) return PFK_ERR_BAD_ARG;
  const int rc = gru_grid(M, C, &grid);
  if (rc != PFK_OK) return rc;
  hipLaunchKernelGGL(gru_f2_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), a_q, z, h, h_ld, q, h_new, M, C);
  return pfk_launch_status();
}

int pfk_gru_backward_q_f32(const float* dh_new, int dh_new_ld, const float* z, const float* q, const float* h, int h_ld,
                           float* da_q, float* da_zr, float* dh, long long M, int C, pfk_stream_t stream) {
  dim3 grid;
  if (!dh_new || !z || !q || !h || !da_q || !da_zr || !dh || (h_ld & 3) || (dh_new_ld & 3)) return PFK_ERR_BAD_ARG;
  const int rc = gru_grid(M, C, &grid);
  if (rc != PFK_OK) return rc;
  hipLaunchKernelGGL(gru_b1_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), dh_new, dh_new_ld, z, q, h, h_ld, da_q,
                     da_zr, dh, M, C);
  return pfk_launch_status();
}

int pfk_gru_backward_zr_f32(const float* d_rh, const float* h, int h_ld, const float* r, float* da_zr, float* dh, long long M,
                            int C, pfk_stream_t stream) {
  dim3 grid;
  if (!d_rh || !h || !r || !da_zr || !dh || (h_ld & 3)) return PFK_ERR_BAD_ARG;
  const int rc = gru_grid(M, C, &grid);
  if (rc != PFK_OK) return rc;
  hipLaunchKernelGGL(gru_b2_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), d_rh, h, h_ld, r, da_zr, dh, M, C);
  return pfk_launch_status();
}

}  // extern "C"
