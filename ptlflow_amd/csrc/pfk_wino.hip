// K4w: 3x3 stride-1 "same" convolution as Winograd F(2x2,3x3) on the gfx950 fp32 matrix cores (v_mfma_f32_16x16x4_f32).
//
// Lavin & Gray 2016: for a 2x2 output tile whose 4x4 input patch d starts one pixel up-left of it (the zero padding),
//   Y = A^T [ sum_c (G g_c G^T) (.) (B^T d_c B) ] A
//   B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1],  G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1],  A^T = [1 1 1 0; 0 1 -1 -1]
// i.e. 16 independent GEMMs, one per transform component xi = 4*row + col:  M_xi[tile][co] = sum_c V_xi[tile][c] * U_xi[c][co],
// 16 * 2 * tiles * cin * cout flops instead of the direct form's 2 * 4 * tiles * 9 * cin * cout: 2.25x fewer fp32 products.
//
// U = G g G^T is made once per weight on the host (packing.pack_wino_weight: fp64, rounded to fp32 once).  Its layout is the LDS
// image of one (64-channel column block, 8-channel K-step), 32 KB contiguous, so a block copies it as it is:
//   weight[cb][ks][xi][nl (64)][slot (8)],  co = 64*cb + nl,  c = 8*ks + cc,
//   slot = ((cc & 3) * 2 + (cc >> 2)) ^ (((nl >> 2) & 3) * 2)
// (pad columns co >= cout are zero).  The slot order gives the MFMA lane (k = lane >> 4 of sub-step s = cc >> 2) both sub-steps'
// values in one 8-byte read; the XOR with bits 2-3 of the row spreads the 16 rows a lane group reads over all banks, for both forms
// the compiler emits (ds_read_b64: 32-lane groups, 64 banks; ds_read2st64_b64: 16-lane groups, 32 banks; the main loop keeps the
// two U reads of a component apart, as ds_read_b64).  V in LDS uses the same slot order with the tile as the row.
//
// Block = 32 consecutive 2x2 tiles (row-major over batch, tile row, tile column) x 64 output channels, 4 waves, each wave
// 16 tiles x 32 channels with ALL 16 components in registers (16 x 2 accumulators of 16x16: 128 per lane).  K-step = 8 input
// channels: each thread transforms one (tile, channel) — 16 dword buffer loads (out-of-image taps read zero through an
// out-of-range offset: that zero is the padding), B^T d B on the VALU, 16 ds_write_b32.  U never passes through registers: the
// packed image is copied by LDS-DMA (buffer_load ... lds, 8 pieces of 1 KB per wave and K-step) into one of two 32 KB buffers, so
// the copy of K-step k + 1 lands while the MFMAs of k run.  Both the DMA pieces and the tap loads of k + 1 are issued BETWEEN the
// MFMAs of k, one piece or two taps per component.  The barriers are raw s_barrier with explicit counted waits (a
// __syncthreads() would drain the LDS-DMA in flight): vmcnt(0) + barrier before a buffer is read, lgkmcnt(0) + barrier before
// sV and the other buffer are written again.  80 KB LDS, 188 registers: two blocks per CU, which fill its LDS.
//
// Epilogue: an MFMA 16x16 accumulator gives a lane four rows (tiles) of one column, at the same place in every component, so
// A^T m A is lane-local; then PFK_EPI_LINEAR's bias, NaN-propagating relu, scale.  A column's K order and transforms do not
// depend on which other columns are in the launch: `cout_active` launches fewer column blocks and gives the full launch's bits.
#include "pfk_gemm.h"

using namespace pfkg;

namespace {

constexpr int WT = 32;   // 2x2 output tiles per block
constexpr int WN = 64;   // output channels per block
constexpr int WK = 8;    // input channels per K-step
constexpr int UIMG = 16 * WN * WK;   // floats of one K-step of one column block's U: the LDS image, 32 KB

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) float lfloat;   // LDS pointers keep their address space (ds_ instructions, 32-bit)
typedef __attribute__((address_space(3))) f32x2 lf32x2;

struct WinoArgs {
  const float* src; int ld;      // pixel-major source, row stride in floats
  unsigned src_bytes;            // readable bytes from src
  int H, W;
  int tw, tpi;                   // tiles per row, tiles per image
  int ntiles;                    // B * tiles per image
  int nks;                       // cin / 8
  const float* weight; unsigned w_bytes;
  const float* bias;
  int cout;
  int ncb;                       // column blocks launched
  int relu; float scale;
  float* out; int out_ld, out_coff;
  const float* res; int res_ld;  // residual rows [pixel][res_ld], column n (conv_gemm_wino_f32_kernel<true> only)
  int relu2;                     // relu after the residual add
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc_n(const void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}

// Two of the 16 input taps of this thread's (tile, channel) of K-step ks into registers.
// (plain functions rather than lambdas: by-reference captures can put register state in scratch, see pfk_gemm.hip)
__device__ __forceinline__ void wino_load_v2(__amdgpu_buffer_rsrc_t rs, const unsigned (&voff)[16], int ks, int q, float (&d)[16]) {
  d[q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, voff[q], ks * WK * 4, 0));
  d[q + 1] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, voff[q + 1], ks * WK * 4, 0));
}

// One of the 8 LDS-DMA pieces a wave copies of a K-step of the block's U (32 KB, already the LDS image) straight into LDS: 64 lanes x
// 16 B to `dst` (wave-uniform) + 16 * lane.  No staging registers and no ds_write; the data is in LDS for every wave once each
// wave's vmcnt has retired its pieces and a barrier has passed.
__device__ __forceinline__ void wino_dma_u(__amdgpu_buffer_rsrc_t rw, lfloat* dst, unsigned wvoff, unsigned wk, int j) {
#if defined(__HIP_DEVICE_COMPILE__)       // (the host pass of hipcc does not know the LDS-DMA builtin)
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (__attribute__((address_space(3))) void*)(dst + j * 1024), 16, wvoff, wk + j * 4096u, 0, 0);
#endif
}

// One K-step (8 channels) of the wave's 16 tiles x 32 columns, all 16 components.  aU1 = aU + 16 * WK through a register the
// compiler cannot relate to aU: two ds_read_b64 (2 LDS cycles each) instead of one ds_read2st64_b64 (8).
// `more`: the next K-step's operands are requested BETWEEN the MFMAs, where their issue cycles hide under the matrix pipe (in front of
// the first MFMA, 8 LDS-DMA pieces and 16 loads are several hundred cycles in which this wave feeds it nothing): one U piece beside
// each of the components 0-7, two taps beside each of 8-15.
__device__ __forceinline__ void wino_mfma(const lfloat* aV, const lfloat* aU, const lfloat* aU1, f32x4 (&acc)[16][2], bool more,
                                          __amdgpu_buffer_rsrc_t rw, lfloat* udst, unsigned wvoff, unsigned wk,
                                          __amdgpu_buffer_rsrc_t rs, const unsigned (&voff)[16], int ks, float (&d)[16]) {
  // operands of component x + 1 are read while the MFMAs of x run (the LDS latency hides under the matrix pipe)
  f32x2 va[2], u0[2], u1[2];
  va[0] = *(const lf32x2*)(aV);
  u0[0] = *(const lf32x2*)(aU);
  u1[0] = *(const lf32x2*)(aU1);
  __builtin_amdgcn_sched_barrier(0);   // (else the reads of component 0 are merged with component 1's into ds_read2st64_b64)
#pragma unroll
  for (int x = 0; x < 16; ++x) {
    const int c = x & 1, n = c ^ 1;
    if (x + 1 < 16) {
      va[n] = *(const lf32x2*)(aV + (x + 1) * WT * WK);
      u0[n] = *(const lf32x2*)(aU + (x + 1) * WN * WK);
      u1[n] = *(const lf32x2*)(aU1 + (x + 1) * WN * WK);
    }
    if (more) {
      if (x < 8) wino_dma_u(rw, udst, wvoff, wk, x);
      else wino_load_v2(rs, voff, ks, 2 * (x - 8), d);
    }
    __builtin_amdgcn_sched_barrier(0);   // (left alone, hipcc hoists the reads of x + 1 behind the MFMAs of x again)
    acc[x][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[c][0], u0[c][0], acc[x][0], 0, 0, 0);
    acc[x][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[c][0], u1[c][0], acc[x][1], 0, 0, 0);
    acc[x][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[c][1], u0[c][1], acc[x][0], 0, 0, 0);
    acc[x][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[c][1], u1[c][1], acc[x][1], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// RES: the residual-block epilogue of pfk_conv2d_wino_res_f32 (v = residual + v, then the block's last relu); the instantiation
// without it is pfk_conv2d_wino_f32's kernel, unchanged.
template <bool RES>
__global__ __launch_bounds__(256, 2) void conv_gemm_wino_f32_kernel(const WinoArgs a) {
  // (one array, U first) 2 x 32 KB of U + 16 KB of V: two blocks fill a CU's LDS
  __shared__ __attribute__((aligned(16))) float smem[2 * UIMG + 16 * WT * WK];
  lfloat* const sU = (lfloat*)smem;    // [buffer][xi][column][slot]
  lfloat* const sV = sU + 2 * UIMG;    // [xi][tile][slot]

  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cb = blockIdx.x % a.ncb;
  const int t0 = (blockIdx.x / a.ncb) * WT;

  const __amdgpu_buffer_rsrc_t rs = rsrc_n(a.src, a.src_bytes);
  const __amdgpu_buffer_rsrc_t rw = rsrc_n(a.weight, a.w_bytes);

  // ---- staging role: tile lt, channel cc of the K-step
  const int lt = tid >> 3, cc = tid & 7;
  unsigned voff[16];
  {
    const int g = t0 + lt;
    const bool tok = g < a.ntiles;
    const int b = g / a.tpi, r = g - b * a.tpi;
    const int ty = r / a.tw, tx = r - ty * a.tw;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int y = 2 * ty - 1 + i, x = 2 * tx - 1 + j;
        const bool ok = tok && (unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W;
        voff[i * 4 + j] = ok ? ((unsigned)((b * a.H + y) * a.W + x) * (unsigned)a.ld + (unsigned)cc) * 4u : OOB;
      }
  }
  const int vslot = ((cc & 3) * 2 + (cc >> 2)) ^ (((lt >> 2) & 3) * 2);
  lfloat* const vdst = sV + lt * WK + vslot;
  const unsigned wvoff = (unsigned)lane * 16u;
  const unsigned wbase = (unsigned)cb * (unsigned)a.nks * (UIMG * 4u) + (unsigned)wid * 1024u;   // this column block's U, this wave's KB
  lfloat* const udst = sU + wid * 256;                                                          // of each 4 KB component pair

  float d[16];
  // ---- MFMA role: wave tile rows wt*16.., columns wc*32..
  const int wt = wid & 1, wc = wid >> 1;
  const int rl = lane & 15, kq = lane >> 4;
  const lfloat* const aV = sV + (wt * 16 + rl) * WK + ((kq * 2) ^ (((rl >> 2) & 3) * 2));
  const lfloat* const aU = sU + (wc * 32 + rl) * WK + ((kq * 2) ^ (((rl >> 2) & 3) * 2));
  const lfloat* aU1 = aU + 16 * WK;
  asm volatile("" : "+v"(aU1));

  f32x4 acc[16][2];
#pragma unroll
  for (int x = 0; x < 16; ++x)
#pragma unroll
    for (int c = 0; c < 2; ++c) acc[x][c] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int j = 0; j < 8; ++j) {
    wino_dma_u(rw, udst, wvoff, wbase, j);
    wino_load_v2(rs, voff, 0, 2 * j, d);
  }
  for (int ks = 0; ks < a.nks; ++ks) {
    // V = B^T d B (rows, then columns), one channel of one tile
    float t[16];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      t[0 * 4 + j] = d[0 * 4 + j] - d[2 * 4 + j];
      t[1 * 4 + j] = d[1 * 4 + j] + d[2 * 4 + j];
      t[2 * 4 + j] = d[2 * 4 + j] - d[1 * 4 + j];
      t[3 * 4 + j] = d[1 * 4 + j] - d[3 * 4 + j];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      vdst[(i * 4 + 0) * WT * WK] = t[i * 4 + 0] - t[i * 4 + 2];
      vdst[(i * 4 + 1) * WT * WK] = t[i * 4 + 1] + t[i * 4 + 2];
      vdst[(i * 4 + 2) * WT * WK] = t[i * 4 + 2] - t[i * 4 + 1];
      vdst[(i * 4 + 3) * WT * WK] = t[i * 4 + 1] - t[i * 4 + 3];
    }
    // this wave's U pieces of this K-step have landed and its V is written; the barrier extends both to every wave
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    const int ub = (ks & 1) * UIMG;
    // the next K-step's U goes to the other buffer, last read before the previous K-step's last barrier
    wino_mfma(aV, aU + ub, aU1 + ub, acc, ks + 1 < a.nks, rw, udst + (UIMG - ub), wvoff, wbase + (unsigned)(ks + 1) * (UIMG * 4u), rs,
              voff, ks + 1, d);
    // a raw barrier: __syncthreads() would wait for the LDS-DMA in flight.  Every wave is done reading sV and this U buffer
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }

  // ---- epilogue: lane holds tiles 4*kq + r (r = 0..3) of column rl in every component
  typedef __attribute__((address_space(1))) float gfloat;
  gfloat* const outp = (gfloat*)a.out;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int n = cb * WN + wc * 32 + c * 16 + rl;
    const bool nok = n < a.cout;
    const float bias = (a.bias != nullptr && nok) ? a.bias[n] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int g = t0 + wt * 16 + kq * 4 + r;
      float m[16];
#pragma unroll
      for (int x = 0; x < 16; ++x) m[x] = acc[x][c][r];
      float s0[4], s1[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        s0[j] = m[0 * 4 + j] + m[1 * 4 + j] + m[2 * 4 + j];
        s1[j] = m[1 * 4 + j] - m[2 * 4 + j] - m[3 * 4 + j];
      }
      float y[4];
      y[0] = s0[0] + s0[1] + s0[2];
      y[1] = s0[1] - s0[2] - s0[3];
      y[2] = s1[0] + s1[1] + s1[2];
      y[3] = s1[1] - s1[2] - s1[3];
      if (!nok || g >= a.ntiles) continue;
      const int b = g / a.tpi, rr = g - b * a.tpi;
      const int ty = rr / a.tw, tx = rr - ty * a.tw;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int oy = 2 * ty + (e >> 1), ox = 2 * tx + (e & 1);
        if (oy >= a.H || ox >= a.W) continue;
        float v = y[e] + bias;
        if (a.relu) v = (v < 0.f) ? 0.f : v;   // NaN-propagating like torch.relu
        v *= a.scale;
        const long long p = ((long long)b * a.H + oy) * a.W + ox;
        if constexpr (RES) {
          v = a.res[p * a.res_ld + n] + v;
          if (a.relu2) v = (v < 0.f) ? 0.f : v;
        }
        outp[p * a.out_ld + a.out_coff + n] = v;
      }
    }
  }
}

}  // namespace

extern "C" {

long long pfk_conv_wino_weight_floats(int cin, int cout) {
  if (cin <= 0 || cout <= 0 || (cin & 31)) return PFK_ERR_BAD_ARG;
  return 16LL * cin * ((cout + WN - 1) / WN * WN);
}

// `res`: pfk_conv2d_wino_res_f32 (a residual is required and relu_after_residual honoured); else pfk_conv2d_wino_f32 (both refused)
static int wino_launch(const pfk_conv_desc* d, bool res, pfk_stream_t stream) {
  if (!d) return PFK_ERR_BAD_ARG;
  if (d->num_src != 1 || d->kh != 3 || d->kw != 3 || d->stride > 1 || d->epilogue != PFK_EPI_LINEAR)
    return PFK_ERR_UNSUPPORTED;
  if (!res && (d->residual || d->relu_after_residual)) return PFK_ERR_UNSUPPORTED;
  if (res && (!d->residual || d->residual_ld < d->cout || (reinterpret_cast<uintptr_t>(d->residual) & 3u))) return PFK_ERR_BAD_ARG;
  const pfk_conv_src& s = d->src[0];
  if (!s.ptr || !d->weight || !d->out || d->B <= 0 || d->H <= 0 || d->W <= 0 || d->cout <= 0 || s.channels <= 0 ||
      s.ld < s.channels || d->out_coff < 0 || d->out_ld < d->out_coff + d->cout)
    return PFK_ERR_BAD_ARG;
  if (s.channels & 31) return PFK_ERR_UNSUPPORTED;
  if (!pfk_aligned16(d->weight) || (reinterpret_cast<uintptr_t>(s.ptr) & 3u) || (reinterpret_cast<uintptr_t>(d->out) & 3u))
    return PFK_ERR_ALIGNMENT;
  const long long M = (long long)d->B * d->H * d->W;
  const long long src_bytes = ((M - 1) * s.ld + s.channels) * 4;
  const long long wfloats = pfk_conv_wino_weight_floats(s.channels, d->cout);
  if (M * s.ld * 4 >= 0x7fffffffLL || wfloats * 4 >= 0x7fffffffLL) return PFK_ERR_UNSUPPORTED;   // 32-bit byte offsets
  int ncb = (d->cout + WN - 1) / WN;
  if (d->cout_active > 0 && d->cout_active < d->cout) {
    if (d->cout_active & (WN - 1)) return PFK_ERR_UNSUPPORTED;
    ncb = d->cout_active / WN;
  }
  WinoArgs a{};
  a.src = s.ptr; a.ld = s.ld; a.src_bytes = (unsigned)src_bytes;
  a.H = d->H; a.W = d->W;
  a.tw = (d->W + 1) / 2;
  a.tpi = a.tw * ((d->H + 1) / 2);
  const long long ntiles = (long long)d->B * a.tpi;
  const long long nblk = (ntiles + WT - 1) / WT * ncb;
  if (nblk >= 0x7fffffffLL) return PFK_ERR_UNSUPPORTED;
  a.ntiles = (int)ntiles;
  a.nks = s.channels / WK;
  a.weight = d->weight; a.w_bytes = (unsigned)(wfloats * 4);
  a.bias = d->bias;
  a.cout = d->cout;
  a.ncb = ncb;
  a.relu = d->relu ? 1 : 0; a.scale = d->scale;
  a.out = d->out; a.out_ld = d->out_ld; a.out_coff = d->out_coff;
  if (res) {
    if (d->cout_active > 0 && d->cout_active < d->cout) return PFK_ERR_UNSUPPORTED;
    a.res = d->residual; a.res_ld = d->residual_ld; a.relu2 = d->relu_after_residual ? 1 : 0;
    hipLaunchKernelGGL(conv_gemm_wino_f32_kernel<true>, dim3((unsigned)nblk), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  } else {
    hipLaunchKernelGGL(conv_gemm_wino_f32_kernel<false>, dim3((unsigned)nblk), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  }
  return pfk_launch_status();
}

int pfk_conv2d_wino_f32(const pfk_conv_desc* d, pfk_stream_t stream) { return wino_launch(d, false, stream); }

int pfk_conv2d_wino_res_f32(const pfk_conv_desc* d, pfk_stream_t stream) { return wino_launch(d, true, stream); }



}  // extern "C"
