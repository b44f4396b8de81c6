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
// sV and the other buffer are written again.  80 KB LDS, 192 registers: two blocks per CU, which fill its LDS.
//
// Epilogue: an MFMA 16x16 accumulator gives a lane four rows (tiles) of one column, at the same place in every component, so
// A^T m A is lane-local.  From that layout a store is a 64-byte piece per 16 lanes and every output needs its own pixel address, so
// the wave parks its 64 pixels (16 tiles x 4 outputs) x 32 columns of A^T m A in the LDS the loop is done with and walks them as
// rows: a lane takes 4 consecutive columns of one pixel, 8 lanes a 128-byte row piece, one 16-byte store each; the residual form
// requests its 8 row pieces per lane before it parks.  Then PFK_EPI_LINEAR's bias, NaN-propagating relu, scale (residual form: one
// fma onto the residual, second relu), in the order and rounding of the first version: same bits.  Pixel addresses come from a table
// of byte offsets, 4 per tile, that the staging role writes once per block from the (b, ty, tx) its prologue divided out: no
// division, no 64-bit multiply and no branch per output.  Predication: stores and residual loads go through buffer descriptors of
// `out` / `residual` with 32-bit offsets (the launcher refuses spans of 2 GB and more), and a lane without work — a tile past the
// end, a pixel past H or W, a column from cout on — carries an out-of-range offset, which the hardware drops (loads: zero).
// Where rows do not take 16-byte pieces (out + out_coff or residual not 16-byte aligned, a row stride % 4 != 0) and in a wave whose
// 32 columns reach past cout (cout 126), the same walk stores its 4 columns as dwords.  A column's K order and transforms do not
// depend on which other columns are in the launch: `cout_active` launches fewer column blocks and gives the full launch's bits.
//
// Instance norms around the launch (the fp32 feature encoder), two more template switches; the instantiations without them are the
// code above, instruction for instruction.  NORM: only U comes by LDS-DMA — the 16 taps pass through registers, so the norm in front
// of the convolution is applied there: the staging thread requests mean and rstd of (its tile's image, its channel) for the next
// K-step through a sized descriptor, beside the first taps between the MFMAs, and every tap becomes relu?((d - mean) * rstd) before
// B^T d B — VALU work beside a loop the matrix pipe bounds; a tap whose offset is the out-of-range one stays 0.f (the padding is zero
// after the norm).  STATS: the row walk adds what it stores to per-column double sums of x and x * x for the norm behind the
// convolution, reduced per block in a fixed order and written to a workspace [image][block of the image][cout]; for that the tile
// list is laid out per image, padded to whole blocks (a tile's arithmetic does not depend on its block: same output bits).
#include "pfk_gemm.h"

using namespace pfkg;

namespace {

constexpr int WT = 32;   // 2x2 output tiles per block
constexpr int WN = 64;   // output channels per block
constexpr int WK = 8;    // input channels per K-step
constexpr int UIMG = 16 * WN * WK;   // floats of one K-step of one column block's U: the LDS image, 32 KB

typedef __attribute__((address_space(3))) float lfloat;   // LDS pointers keep their address space (ds_ instructions, 32-bit)
typedef __attribute__((address_space(3))) f32x2 lf32x2;
typedef __attribute__((address_space(3))) f32x4 lf32x4;

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
  unsigned out_bytes;            // writable bytes from out (the last pixel's last column)
  const float* res; int res_ld;  // residual rows [pixel][res_ld], column n (conv_gemm_wino_f32_kernel<true> only)
  unsigned res_bytes;            // readable bytes from res
  int relu2;                     // relu after the residual add
  int vec;                       // the rows of out (and res) take 16-byte pieces: 16-byte aligned, row strides % 4 == 0
  // NORM: the source is a raw convolution output in front of an instance norm; a tap becomes relu?((d - mean) * rstd) on its way in
  const float* in_mean; const float* in_rstd;   // [B][cin]
  unsigned stat_bytes;           // B * cin * 4
  int cin, in_relu;
  // STATS: the tile list is laid out per image, `nbi` blocks of 32 tiles each (the last one padded); every block writes the sums of
  // x and of x * x over what it stores, per column, into part[sum, sum of squares][image][block of the image][cout]
  int nbi;
  double* part; long long astride;
};

// The epilogue's entry of one of the block's 32 tiles, made once by the staging role: bit 31 the tile exists, bit 30 / 29 its second
// output row / column lies inside the image, the low bits its first output pixel (B * H * W < 2^24: the launcher's 32-bit byte offsets).
constexpr unsigned T_OK = 0x80000000u, T_ROW2 = 0x40000000u, T_COL2 = 0x20000000u, T_PIX = 0x1fffffffu;
// A wave's parking area for A^T m A: 64 pixels (16 tiles x 4 outputs) x 32 columns, 16 floats of padding behind every 16 pixels (the
// four tile groups kq of the accumulator layout write different banks; the row walk reads 1 KB runs)
constexpr int ESZ = 64 * 32 + 4 * 16;

// NORM: mean and rstd of this thread's (image, channel) of K-step ks (zero for a tile past the end: its taps are all padding)
__device__ __forceinline__ void wino_load_stat(__amdgpu_buffer_rsrc_t rm, __amdgpu_buffer_rsrc_t rr, unsigned soff, int ks, float (&mr)[2]) {
  mr[0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rm, soff, ks * WK * 4, 0));
  mr[1] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rr, soff, ks * WK * 4, 0));
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
// NORM: the staging thread's mean and rstd of the next K-step's channel (its tile's image) are requested with the first two taps.
template <bool NORM>
__device__ __forceinline__ void wino_mfma(const lfloat* aV, const lfloat* aU, const lfloat* aU1, f32x4 (&acc)[16][2], bool more,
                                          __amdgpu_buffer_rsrc_t rw, lfloat* udst, unsigned wvoff, unsigned wk,
                                          __amdgpu_buffer_rsrc_t rs, const unsigned (&voff)[16], int ks, float (&d)[16],
                                          __amdgpu_buffer_rsrc_t rm, __amdgpu_buffer_rsrc_t rr, unsigned soff, float (&mr)[2]) {
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
      if constexpr (NORM) {
        if (x == 8) wino_load_stat(rm, rr, soff, ks, mr);
      }
    }
    __builtin_amdgcn_sched_barrier(0);   // (left alone, hipcc hoists the reads of x + 1 behind the MFMAs of x again)
    acc[x][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[c][0], u0[c][0], acc[x][0], 0, 0, 0);
    acc[x][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[c][0], u1[c][0], acc[x][1], 0, 0, 0);
    acc[x][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[c][1], u0[c][1], acc[x][0], 0, 0, 0);
    acc[x][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[c][1], u1[c][1], acc[x][1], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
}

typedef __attribute__((address_space(3))) unsigned lunsigned;

// Epilogue, row walk (see the kernel).  The lane's 8 pixels are output e = (lane >> 3) & 3 of the wave's tiles 2 * i + (lane >> 5),
// i = 0..7, its 4 columns start at n0; tT = the offset table at (e, the wave's tile lane >> 5).  Byte offsets of the 8 row pieces in
// `out` (OOB and beyond for a pixel that does not exist: the buffer store drops it) and, RES, the residual's 8 pieces, all requested
// here, before the first is used.  VEC: 16-byte pieces; else the 4 columns one by one, those from cout on read as zero.
template <bool RES, bool VEC>
__device__ __forceinline__ void wino_epi_request(const WinoArgs& a, const lunsigned* tT, int n0, unsigned (&oo)[8], f32x4 (&r4)[8]) {
  unsigned ro[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    oo[i] = tT[2 * i] + (unsigned)(a.out_coff + n0) * 4u;
    if constexpr (RES) ro[i] = tT[4 * WT + 2 * i] + (unsigned)n0 * 4u;
  }
  if constexpr (RES) {
    const __amdgpu_buffer_rsrc_t rr = buffer_rsrc(a.res, a.res_bytes);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if constexpr (VEC) {
        r4[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rr, ro[i], 0, 0));
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          r4[i][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rr, n0 + j < a.cout ? ro[i] + 4u * j : OOB, 0, 0));
      }
    }
  }
}

// Epilogue, row walk: the lane's 8 row pieces from the wave's parking area (rE = the lane's pixel 0 and column there), then the first
// version's arithmetic in its order and rounding: + bias, NaN-propagating relu, x scale (RES: one fma with the residual as the addend,
// then the second relu); a relu that is off compares with -inf and keeps every value.
// STATS: the lane also sums what it stores, and its square, per column in double (st[0..3], st[4..7]); a store the hardware drops — a
// missing tile, a pixel past H or W (its offset is OOB or beyond), a column from cout on — adds an exact zero.
template <bool RES, bool VEC, bool STATS>
__device__ __forceinline__ void wino_epi_store(const WinoArgs& a, const lfloat* rE, int n0, const unsigned (&oo)[8], const f32x4 (&r4)[8],
                                               double (&st)[8]) {
  const __amdgpu_buffer_rsrc_t ro = buffer_rsrc(a.out, a.out_bytes);
  const __amdgpu_buffer_rsrc_t rbias = buffer_rsrc(a.bias, a.bias != nullptr ? (unsigned)a.cout * 4u : 0u);   // (no bias, pad columns: zero)
  float bias4[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) bias4[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rbias, (unsigned)(n0 + j) * 4u, 0, 0));
  const float lo = a.relu ? 0.f : -__builtin_inff(), lo2 = a.relu2 ? 0.f : -__builtin_inff();
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const f32x4 y = *(const lf32x4*)(rE + i * 256 + (i >> 1) * 16);
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float t = y[j] + bias4[j];
      t = (t < lo) ? lo : t;
      if constexpr (RES) {
        t = __builtin_fmaf(t, a.scale, r4[i][j]);
        t = (t < lo2) ? lo2 : t;
      } else {
        t *= a.scale;
      }
      v[j] = t;
      if constexpr (STATS) {
        const double dv = (double)((oo[i] < OOB && (VEC || n0 + j < a.cout)) ? t : 0.f);
        st[j] += dv;
        st[4 + j] = __builtin_fma(dv, dv, st[4 + j]);
      }
    }
    if constexpr (VEC) {
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, (f32x4{v[0], v[1], v[2], v[3]})), ro, oo[i], 0, 0);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v[j]), ro, n0 + j < a.cout ? oo[i] + 4u * j : OOB, 0, 0);
    }
  }
}

// RES: the residual-block epilogue of pfk_conv2d_wino_res_f32 (v = residual + v, then the block's last relu); the instantiation
// without it is pfk_conv2d_wino_f32's kernel.
// NORM (pfk_conv2d_wino_norm_f32, pfk_conv2d_wino_stats_f32): the instance norm in front of the convolution is applied to the taps
// in registers, with norm_apply_kernel's arithmetic (subtract, multiply, compare; each rounded); a padding tap stays 0.f.
// STATS (pfk_conv2d_wino_stats_f32, plain form): the row walk sums its stores for the instance norm behind the convolution.  A block's
// 32 tiles are of one image (WinoArgs::nbi); lanes of a column, then the two wave rows are added in a fixed order through LDS — no
// atomics, the same bits on every run — and chunk_reduce_kernel<true> finishes over the image's blocks.
template <bool RES, bool NORM = false, bool STATS = false>
__global__ __launch_bounds__(256, 2) void conv_gemm_wino_f32_kernel(const WinoArgs a) {
  static_assert(!(RES && STATS), "the residual form is never in front of an instance norm");
  // (one array, U first) 2 x 32 KB of U + 16 KB of V: two blocks fill a CU's LDS
  __shared__ __attribute__((aligned(16))) float smem[2 * UIMG + 16 * WT * WK];
  lfloat* const sU = (lfloat*)smem;    // [buffer][xi][column][slot]
  lfloat* const sV = sU + 2 * UIMG;    // [xi][tile][slot]

  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cb = blockIdx.x % a.ncb;
  const int t0 = (blockIdx.x / a.ncb) * WT;

  const __amdgpu_buffer_rsrc_t rs = buffer_rsrc(a.src, a.src_bytes);
  const __amdgpu_buffer_rsrc_t rw = buffer_rsrc(a.weight, a.w_bytes);
  const __amdgpu_buffer_rsrc_t rm = buffer_rsrc(a.in_mean, NORM ? a.stat_bytes : 0u);
  const __amdgpu_buffer_rsrc_t rr = buffer_rsrc(a.in_rstd, NORM ? a.stat_bytes : 0u);

  // ---- staging role: tile lt, channel cc of the K-step
  const int lt = tid >> 3, cc = tid & 7;
  unsigned voff[16];
  unsigned tinfo;   // the tile's entry of the epilogue's table
  unsigned soff = 0;   // NORM: byte offset of (the tile's image, channel cc) in the statistics
  {
    int g, b, r;
    bool tok;
    if constexpr (STATS) {
      // block (image sb, its block sk): tiles 32 * sk .. of that image
      const int tb = blockIdx.x / a.ncb;
      b = tb / a.nbi;
      r = (tb - b * a.nbi) * WT + lt;
      tok = r < a.tpi;
    } else {
      g = t0 + lt;
      tok = g < a.ntiles;
      b = g / a.tpi;
      r = g - b * a.tpi;
    }
    if constexpr (NORM) soff = ((unsigned)b * (unsigned)a.cin + (unsigned)cc) * 4u;
    const int ty = r / a.tw, tx = r - ty * a.tw;
    tinfo = tok ? (T_OK | (2 * ty + 1 < a.H ? T_ROW2 : 0u) | (2 * tx + 1 < a.W ? T_COL2 : 0u) | (unsigned)((b * a.H + 2 * ty) * a.W + 2 * tx)) : 0u;
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
  float mr[2] = {0.f, 0.f};   // NORM: mean, rstd of the K-step whose taps are in d
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
  if constexpr (NORM) wino_load_stat(rm, rr, soff, 0, mr);
  const float nlo = a.in_relu ? 0.f : -__builtin_inff();  for (int ks = 0; ks < a.nks; ++ks) {
    if constexpr (NORM) {
      // norm_apply_kernel's y = (x - mean) * rstd, relu (a relu that is off compares with -inf); the padding is zero AFTER the norm
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const float y = __fmul_rn(__fsub_rn(d[q], mr[0]), mr[1]);
        d[q] = voff[q] == OOB ? 0.f : ((y < nlo) ? nlo : y);
      }
    }
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
    wino_mfma<NORM>(aV, aU + ub, aU1 + ub, acc, ks + 1 < a.nks, rw, udst + (UIMG - ub), wvoff, wbase + (unsigned)(ks + 1) * (UIMG * 4u),
                    rs, voff, ks + 1, d, rm, rr, soff, mr);
    // a raw barrier: __syncthreads() would wait for the LDS-DMA in flight.  Every wave is done reading sV and this U buffer
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }

  // ---- epilogue.  Every wave is past the loop's last barrier: sU and sV are free.
  // The offset table: for each of the block's 32 tiles and its 4 outputs e = 2 * row + column, the byte offset of that pixel's row in
  // out (then in the residual), OOB where the tile or the pixel does not exist.  The staging role's threads cc = e of a tile write it
  // from the entry they kept; one more barrier hands it to the MFMA role's waves.  All divisions were the prologue's.
  lfloat* const sE = (lfloat*)smem + wid * ESZ;
  lunsigned* const sT = (lunsigned*)((lfloat*)smem + 4 * ESZ);   // [out, residual][e][tile]
  static_assert(4 * ESZ + 8 * WT <= 2 * UIMG + 16 * WT * WK, "parking areas and offset table must fit into the loop's LDS");
  {
    const unsigned need = T_OK | ((cc & 2) ? T_ROW2 : 0u) | ((cc & 1) ? T_COL2 : 0u);
    const bool ok = (tinfo & need) == need;
    const unsigned pix = (tinfo & T_PIX) + (unsigned)(((cc >> 1) & 1) * a.W + (cc & 1));
    const unsigned po = ok ? pix * (unsigned)a.out_ld * 4u : OOB;
    const unsigned pr = ok ? pix * (unsigned)a.res_ld * 4u : OOB;
    if (cc < 4) {
      sT[cc * WT + lt] = po;
      if constexpr (RES) sT[(4 + cc) * WT + lt] = pr;
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

  // row-walk role: pixel li = 8 * i + prow of the wave's 64 (tile li >> 2, output li & 3), 4 columns from c4
  const int prow = lane >> 3, c4 = (lane & 7) * 4;
  const int n0 = cb * WN + wc * 32 + c4;
  const lunsigned* const tT = sT + (prow & 3) * WT + wt * 16 + (lane >> 5);
  // (wave-uniform) 16-byte pieces where the launcher found the rows aligned and the wave's 32 columns all exist
  const bool vec = a.vec && cb * WN + wc * 32 + 32 <= a.cout;
  unsigned oo[8];
  f32x4 r4[8];
  if (vec) wino_epi_request<RES, true>(a, tT, n0, oo, r4);
  else wino_epi_request<RES, false>(a, tT, n0, oo, r4);

  // MFMA role: the lane holds tiles 4*kq + r (r = 0..3) of columns c*16 + rl in every component; A^T m A is lane-local.  Parked at
  // [pixel li = (4*kq + r)*4 + e][column] of the wave's own area (no barrier: the wave's own LDS operations stay in order)
  {
    lfloat* const pE = sE + kq * (16 * 32 + 16) + rl;
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float m[16];
#pragma unroll
        for (int x = 0; x < 16; ++x) m[x] = acc[x][c][r];
        float s0[4], s1[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          s0[j] = m[0 * 4 + j] + m[1 * 4 + j] + m[2 * 4 + j];
          s1[j] = m[1 * 4 + j] - m[2 * 4 + j] - m[3 * 4 + j];
        }
        pE[(r * 4 + 0) * 32 + c * 16] = s0[0] + s0[1] + s0[2];
        pE[(r * 4 + 1) * 32 + c * 16] = s0[1] - s0[2] - s0[3];
        pE[(r * 4 + 2) * 32 + c * 16] = s1[0] + s1[1] + s1[2];
        pE[(r * 4 + 3) * 32 + c * 16] = s1[1] - s1[2] - s1[3];
      }
  }
  const lfloat* const rE = sE + prow * 32 + c4;
  double st[8] = {0., 0., 0., 0., 0., 0., 0., 0.};
  if (vec) wino_epi_store<RES, true, STATS>(a, rE, n0, oo, r4, st);
  else wino_epi_store<RES, false, STATS>(a, rE, n0, oo, r4, st);

  if constexpr (STATS) {
    // The lane's 8 sums into its wave's parking area (read for the last time above; a wave's LDS operations stay in order), 64 bytes
    // per lane.  Then thread (sum | sum of squares, column of the block's 64) adds the 8 lanes prow = 0..7 that walked the column in
    // each wave row, then the two wave rows: a fixed order.
    typedef __attribute__((address_space(3))) double ldouble;
    ldouble* const sS = (ldouble*)(sE) + lane * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) sS[j] = st[j];
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (tid < 2 * WN) {
      const int which = tid >> 6, col = tid & 63;
      const int idx = ((col & 31) >> 2) * 8 + which * 4 + (col & 3);   // lane (prow 0, column group) * 8 + entry
      double tot[2];
#pragma unroll
      for (int w = 0; w < 2; ++w) {
        const ldouble* const p = (const ldouble*)((lfloat*)smem + ((col >> 5) * 2 + w) * ESZ) + idx;
        double s = 0.;
#pragma unroll
        for (int k = 0; k < 8; ++k) s += p[k * 64];
        tot[w] = s;
      }
      const int n = cb * WN + col;
      // (block-uniform) image blockIdx / ncb / nbi, and the block's index there: together blockIdx / ncb
      if (n < a.cout) a.part[which * a.astride + (long long)(blockIdx.x / a.ncb) * a.cout + n] = tot[0] + tot[1];
    }
  }
}

// ---- K4w1: the SepConvGRU's 1x5 / 5x1 gate convolutions as 1-D Winograd F(4,5) -------------------------------------------------
// Points 0, +-1, +-2, +-1/2, inf: for 4 consecutive outputs along the convolution axis and the 8 input pixels d that start 2 in
// front of the first one (correlation form, y_i = sum_k d[i + k] g[k]),  Y = A^T [ sum_c (G g_c) (.) (B^T d_c) ]  with
//   B^T = [-1 0 21/4 0 -21/4 0 1 0; 0 1 1 -17/4 -17/4 1 1 0; 0 -1 1 17/4 -17/4 -1 1 0; 0 1/2 1/4 -5/2 -5/4 2 1 0;
//          0 -1/2 1/4 5/2 -5/4 -2 1 0; 0 2 4 -5/2 -5 1/2 1 0; 0 -2 4 5/2 -5 -1/2 1 0; 0 -1 0 21/4 0 -21/4 0 1]
//   A^T = [1 1 1 1 1 1 1 0; 0 1 -1 2 -2 1/2 -1/2 0; 0 1 1 4 4 1/4 1/4 0; 0 1 -1 8 -8 1/8 -1/8 1]
// (every entry exact in fp32; rows 1|2, 3|4, 5|6 share their even and odd parts): 8 products per 4 outputs instead of 20.
// U = G g (packing.pack_wino1d_weight: fp64, rounded once) comes as the LDS image of one (128-channel column block, K-step):
//   weight[cb][ks][xi (8)][nl (128)][slot (8)], the slot order of the 2-D kernel — again 32 KB, copied by the same 8 LDS-DMA pieces.
// With 8 components instead of 16 the wave tile doubles its columns: block = 32 tiles x 128 channels, wave = 16 tiles x 64 channels
// x 8 components = 8 x 4 accumulators of 16x16 (128 per lane), 8 x 8 = 64 MFMAs per K-step as before; V is 8 KB, 72 KB LDS in all.
// The loop, the raw barriers, the operand requests between the MFMAs (one U piece and one tap beside each component) are the 2-D
// kernel's.  VERT = false (1x5): tiles run along a row, the block's 32 tiles row-major over (image row, tile x).  VERT = true (5x1):
// tiles run down a column, the block's tiles are neighbouring x of one tile row.  The K-steps walk source 0, then source 1 (the
// torch.cat operands of the gate convolutions), each with its own descriptor and tap offsets.  Epilogues after the lane-local A^T m:
// LINEAR, GRU_ZR, GRU_Q of include/pfk.h with pfk_gemm.h's arithmetic.  Nothing depends on the grid: same input, same bits.
// The gate epilogues are the 2-D kernel's row walk with two or three operand rows per pixel: the wave parks A^T m in the LDS the loop
// has finished with and walks it as rows; pixel addresses come from offset tables that the staging role writes once per block from
// the (first pixel, outputs inside L) it kept of its tile, and every operand and result passes a sized buffer descriptor, so a lane
// without work carries an out-of-range offset instead of a test.  The first 8 pixels' operands are requested before the wave parks,
// the other 8 before the first gate is computed (see the kernel's epilogue).
constexpr int WN1 = 128;                 // output channels per block
constexpr int VIMG1 = 8 * WT * WK;       // floats of V: 8 components x 32 tiles x 8 channels

struct Wino1dArgs {
  const float* src0; const float* src1;   // pixel-major sources in K order (src1 = src0 when there is one)
  int ld0, ld1;
  unsigned bytes0, bytes1;                // readable bytes from each
  int nks0, nks;                          // K-steps of source 0, of both
  int H, W;
  int L, nt;                              // pixels and tiles along the convolution axis
  int ntiles;
  const float* weight; unsigned w_bytes;
  const float* bias;
  int cout, ncb;
  int relu; float scale;
  float* out; int out_ld, out_coff;
  const float* res; int res_ld;           // GRU epilogues: added to the pre-activation
  float* h; int h_ld;
  float* aux_z; float* aux_rh;
  int ch;
  unsigned res_bytes, h_bytes, z_bytes;   // GRU epilogues: bytes of res (0 without one), h, aux_z / aux_rh up to the last pixel's last column
};

// The gate epilogues' entry of one of the block's 32 tiles, kept by the staging role: bits 31-29 how many of the tile's 4 outputs lie
// inside L (0: there is no such tile), the low bits its first output pixel (B * H * W < 2^26: the launcher's 32-bit byte offsets).
constexpr unsigned T1_PIX = 0x1fffffffu;
// A wave's parking area for A^T m: 64 pixels (16 tiles x 4 outputs) x 64 columns, 16 floats of padding behind every 16 pixels: the
// dword stores of a lane half (16 columns of two tile groups kq) then fall into 32 different banks, and a float4 read serves 16 lanes
// at a time — 4 + 8 + 4 of them from two neighbouring pixels, which together take each 16-byte slot of the 256-byte bank row once
// when rows are exactly 256 bytes apart (rows of 68 floats made two of those lanes share a slot).  A lane's four outputs of one
// (fragment, tile) lie 64 floats apart: two ds_write2_b32.
constexpr int ES1 = 64, ESZ1 = 64 * ES1 + 4 * 16;
// The gate epilogues' offset tables behind the four parking areas: [context term, h, z | r*h, none][output e][tile], 128 words each
constexpr int TBL1 = 4 * WT;

// tile g -> the pixel of axis coordinate 0 on its line, and its tile index along the axis
template <bool VERT>
__device__ __forceinline__ void wino1d_tile(const Wino1dArgs& a, int g, int& base, int& t) {
  if constexpr (VERT) {
    const int r = g / a.W, x = g - r * a.W, b = r / a.nt;
    t = r - b * a.nt;
    base = b * a.H * a.W + x;
  } else {
    const int line = g / a.nt;
    t = g - line * a.nt;
    base = line * a.W;
  }
}

// tap q of this thread's (tile, channel) of a K-step: `s1` (block-uniform) = the K-step lies in source 1, `soff` = its channel offset there
__device__ __forceinline__ void wino1d_load_v(__amdgpu_buffer_rsrc_t rs0, __amdgpu_buffer_rsrc_t rs1, const unsigned (&voff0)[8],
                                              const unsigned (&voff1)[8], bool s1, int soff, int q, float (&d)[8]) {
  d[q] = s1 ? __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs1, voff1[q], soff, 0))
            : __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs0, voff0[q], soff, 0));
}

// One K-step of the wave's 16 tiles x 64 columns, all 8 components (see wino_mfma).  aU[f] reach the four column fragments through
// registers the compiler cannot relate: four ds_read_b64 per component.
__device__ __forceinline__ void wino1d_mfma(const lfloat* aV, const lfloat* aU0, const lfloat* aU1, const lfloat* aU2, const lfloat* aU3,
                                            f32x4 (&acc)[8][4], bool more, __amdgpu_buffer_rsrc_t rw, lfloat* udst, unsigned wvoff,
                                            unsigned wk, __amdgpu_buffer_rsrc_t rs0, __amdgpu_buffer_rsrc_t rs1,
                                            const unsigned (&voff0)[8], const unsigned (&voff1)[8], bool s1, int soff, float (&d)[8]) {
  f32x2 va[2], u[2][4];
  va[0] = *(const lf32x2*)(aV);
  u[0][0] = *(const lf32x2*)(aU0);
  u[0][1] = *(const lf32x2*)(aU1);
  u[0][2] = *(const lf32x2*)(aU2);
  u[0][3] = *(const lf32x2*)(aU3);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int x = 0; x < 8; ++x) {
    const int c = x & 1, n = c ^ 1;
    if (x + 1 < 8) {
      va[n] = *(const lf32x2*)(aV + (x + 1) * WT * WK);
      u[n][0] = *(const lf32x2*)(aU0 + (x + 1) * WN1 * WK);
      u[n][1] = *(const lf32x2*)(aU1 + (x + 1) * WN1 * WK);
      u[n][2] = *(const lf32x2*)(aU2 + (x + 1) * WN1 * WK);
      u[n][3] = *(const lf32x2*)(aU3 + (x + 1) * WN1 * WK);
    }
    if (more) {
      wino_dma_u(rw, udst, wvoff, wk, x);
      wino1d_load_v(rs0, rs1, voff0, voff1, s1, soff, x, d);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int f = 0; f < 4; ++f) acc[x][f] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[c][s], u[c][f][s], acc[x][f], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// y = A^T m of fragment f, accumulator row r (one tile of one column)
__device__ __forceinline__ void wino1d_at(const f32x4 (&acc)[8][4], int f, int r, float (&y)[4]) {
  const float p12 = acc[1][f][r] + acc[2][f][r], q12 = acc[1][f][r] - acc[2][f][r];
  const float p34 = acc[3][f][r] + acc[4][f][r], q34 = acc[3][f][r] - acc[4][f][r];
  const float p56 = acc[5][f][r] + acc[6][f][r], q56 = acc[5][f][r] - acc[6][f][r];
  y[0] = acc[0][f][r] + p12 + p34 + p56;
  y[1] = q12 + 2.f * q34 + 0.5f * q56;
  y[2] = p12 + 4.f * p34 + 0.25f * p56;
  y[3] = q12 + 8.f * q34 + 0.125f * q56 + acc[7][f][r];
}

typedef __attribute__((address_space(3))) u32x4 lu32x4;

// Gate epilogues, row walk.  The lane's 16 pixels are output e = lane >> 4 of the wave's 16 tiles, 8 per half, its 4 columns the
// same in each.  Byte offsets of one half's 8 row pieces from one table: tP = the table at (e, the half's first tile), `col` the byte
// offset of the 4 columns in a row.  A pixel that does not exist has OOB in the table and stays out of range; a lane without work
// reads the table that holds nothing else.
__device__ __forceinline__ void wino1d_epi_offsets(const lunsigned* tP, unsigned col, unsigned (&o)[8]) {
  const u32x4 t0 = *(const lu32x4*)tP, t1 = *(const lu32x4*)(tP + 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    o[j] = t0[j] + col;
    o[4 + j] = t1[j] + col;
  }
}

// the 8 row pieces of one operand, all requested before the first is used (out of range: zero)
__device__ __forceinline__ void wino1d_epi_load(__amdgpu_buffer_rsrc_t rs, const unsigned (&o)[8], f32x4 (&v)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, o[i], 0, 0));
}

// One pixel's 4 columns: (parked A^T m + bias) + context term, then the gate with pfk_gemm.h's arithmetic.  GRU_ZR: sigmoid, times h
// in the r half (`upper`).  GRU_Q: (1 - z) * h + z * tanh, each product rounded (no contraction), as the direct kernel's epilogue.
template <int EPI>
__device__ __forceinline__ f32x4 wino1d_gate(f32x4 y, f32x4 bias4, f32x4 r, f32x4 h, f32x4 z, bool upper) {
  const f32x4 v = y + bias4 + r;
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if constexpr (EPI == PFK_EPI_GRU_ZR) {
      const float s = sigmoid_f(v[e]);
      o[e] = upper ? s * h[e] : s;
    } else {
      const float keep = __fmul_rn(__fsub_rn(1.0f, z[e]), h[e]);
      const float take = __fmul_rn(z[e], tanhf(v[e]));
      o[e] = __fadd_rn(keep, take);
    }
  }
  return o;
}

__device__ __forceinline__ void wino1d_epi_put(f32x4 o, __amdgpu_buffer_rsrc_t rs, unsigned off) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), rs, off, 0, 0);
}

template <bool VERT, int EPI>
__global__ __launch_bounds__(256, 2) void conv_gemm_wino1d_f32_kernel(const Wino1dArgs a) {
  // 2 x 32 KB of U + 8 KB of V
  __shared__ __attribute__((aligned(16))) float smem[2 * UIMG + VIMG1];
  lfloat* const sU = (lfloat*)smem;    // [buffer][xi][column][slot]
  lfloat* const sV = sU + 2 * UIMG;    // [xi][tile][slot]

  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cb = blockIdx.x % a.ncb;
  const int t0 = (blockIdx.x / a.ncb) * WT;
  const int pstride = VERT ? a.W : 1;

  const __amdgpu_buffer_rsrc_t rs0 = buffer_rsrc(a.src0, a.bytes0);
  const __amdgpu_buffer_rsrc_t rs1 = buffer_rsrc(a.src1, a.bytes1);
  const __amdgpu_buffer_rsrc_t rw = buffer_rsrc(a.weight, a.w_bytes);

  // ---- staging role: tile lt, channel cc of the K-step
  const int lt = tid >> 3, cc = tid & 7;
  unsigned voff0[8], voff1[8];
  unsigned tinfo;   // the tile's entry of the gate epilogues' tables
  {
    const int g = t0 + lt;
    const bool tok = g < a.ntiles;
    int base, t;
    wino1d_tile<VERT>(a, g, base, t);
    const int nout = a.L - 4 * t;
    tinfo = tok ? ((unsigned)(nout < 4 ? nout : 4) << 29) | (unsigned)(base + 4 * t * pstride) : 0u;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int ax = 4 * t - 2 + j;
      const bool ok = tok && (unsigned)ax < (unsigned)a.L;
      const unsigned pix = (unsigned)(base + ax * pstride);
      voff0[j] = ok ? (pix * (unsigned)a.ld0 + (unsigned)cc) * 4u : OOB;
      voff1[j] = ok ? (pix * (unsigned)a.ld1 + (unsigned)cc) * 4u : OOB;
    }
  }
  const int vslot = ((cc & 3) * 2 + (cc >> 2)) ^ (((lt >> 2) & 3) * 2);
  lfloat* const vdst = sV + lt * WK + vslot;
  const unsigned wvoff = (unsigned)lane * 16u;
  const unsigned wbase = (unsigned)cb * (unsigned)a.nks * (UIMG * 4u) + (unsigned)wid * 1024u;
  lfloat* const udst = sU + wid * 256;

  float d[8];
  // ---- MFMA role: wave tile rows wt*16.., columns wc*64..
  const int wt = wid & 1, wc = wid >> 1;
  const int rl = lane & 15, kq = lane >> 4;
  const int oslot = (kq * 2) ^ (((rl >> 2) & 3) * 2);
  const lfloat* const aV = sV + (wt * 16 + rl) * WK + oslot;
  const lfloat* const aU0 = sU + (wc * 64 + rl) * WK + oslot;
  const lfloat* aU1 = aU0 + 16 * WK;
  const lfloat* aU2 = aU0 + 32 * WK;
  const lfloat* aU3 = aU0 + 48 * WK;
  asm volatile("" : "+v"(aU1));
  asm volatile("" : "+v"(aU2));
  asm volatile("" : "+v"(aU3));

  f32x4 acc[8][4];
#pragma unroll
  for (int x = 0; x < 8; ++x)
#pragma unroll
    for (int f = 0; f < 4; ++f) acc[x][f] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int j = 0; j < 8; ++j) {
    wino_dma_u(rw, udst, wvoff, wbase, j);
    wino1d_load_v(rs0, rs1, voff0, voff1, false, 0, j, d);
  }
  for (int ks = 0; ks < a.nks; ++ks) {
    // V = B^T d, one channel of one tile
    {
      const float e12 = d[2] - 4.25f * d[4] + d[6], o12 = d[1] - 4.25f * d[3] + d[5];
      const float e34 = 0.25f * d[2] - 1.25f * d[4] + d[6], o34 = 0.5f * d[1] - 2.5f * d[3] + 2.f * d[5];
      const float e56 = 4.f * d[2] - 5.f * d[4] + d[6], o56 = 2.f * d[1] - 2.5f * d[3] + 0.5f * d[5];
      vdst[0 * WT * WK] = (d[6] - d[0]) + 5.25f * (d[2] - d[4]);
      vdst[1 * WT * WK] = e12 + o12;
      vdst[2 * WT * WK] = e12 - o12;
      vdst[3 * WT * WK] = e34 + o34;
      vdst[4 * WT * WK] = e34 - o34;
      vdst[5 * WT * WK] = e56 + o56;
      vdst[6 * WT * WK] = e56 - o56;
      vdst[7 * WT * WK] = (d[7] - d[1]) + 5.25f * (d[3] - d[5]);
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    const int ub = (ks & 1) * UIMG;
    const int kn = ks + 1;
    const bool s1 = kn >= a.nks0;
    const int soff = (kn - (s1 ? a.nks0 : 0)) * WK * 4;
    wino1d_mfma(aV, aU0 + ub, aU1 + ub, aU2 + ub, aU3 + ub, acc, kn < a.nks, rw, udst + (UIMG - ub), wvoff,
                wbase + (unsigned)kn * (UIMG * 4u), rs0, rs1, voff0, voff1, s1, soff, d);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }

  // ---- epilogue: lane holds tiles 4*kq + r (r = 0..3) of column rl of each fragment, in every component
  if constexpr (EPI == PFK_EPI_LINEAR) {
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const int n = cb * WN1 + wc * 64 + f * 16 + rl;
      const bool nok = n < a.cout;
      const float bias = (a.bias != nullptr && nok) ? a.bias[n] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int g = t0 + wt * 16 + kq * 4 + r;
        float y[4];
        wino1d_at(acc, f, r, y);
        if (!nok || g >= a.ntiles) continue;
        int base, t;
        wino1d_tile<VERT>(a, g, base, t);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int ax = 4 * t + e;
          if (ax >= a.L) continue;
          const long long p = base + ax * pstride;
          float v = y[e] + bias;
          if (a.relu) v = (v < 0.f) ? 0.f : v;   // NaN-propagating like torch.relu
          v *= a.scale;
          ((gfloat*)a.out)[p * a.out_ld + a.out_coff + n] = v;
        }
      }
    }
  } else {
    // The gate epilogues read two or three rows per output (context term, h, z): from the accumulator layout that is 64-byte pieces,
    // four at a time, with the memory latency of each batch exposed.  Instead every wave parks its 64 pixels x 64 columns of A^T m in
    // its own 16 KB of the LDS the loop has finished with (all waves are past the last barrier; the layout: ESZ1) and walks them as
    // rows: a lane takes 4 columns of one pixel, 16 lanes a 256-byte row piece, 16 pixels per lane in two halves of 8.
    //
    // Pixel addresses come from tables of byte offsets that the staging role writes once per block from the entry its prologue kept:
    // per tile and output, the pixel's row in the context term, in h and in z / r*h (one table per row stride), OOB where the tile or
    // the pixel does not exist, and a fourth table that holds only OOB.  All operands and results go through buffer descriptors sized
    // to the last pixel's last column (the launcher refuses spans of 2 GB and more): a lane without work — a pixel past L, a tile past
    // the end, columns from cout on, the z half where h is read — reads the fourth table, so its loads give zero and its stores are
    // dropped.  No division, no 64-bit multiply and no bounds test per output, and no branch beyond tanhf's own and a wave-uniform
    // one around the r half's store in a wave whose 64 columns hold both halves (z and r*h are two buffers: the other waves choose
    // their descriptor once).  The first half's operands are requested before the wave parks, the second half's before the first
    // half's gates are computed.
    static_assert(4 * ESZ1 + 4 * TBL1 <= 2 * UIMG + VIMG1, "the four waves' parking areas and the offset tables must fit into the loop's LDS");
    lfloat* const sE = (lfloat*)smem + wid * ESZ1;
    lunsigned* const sT = (lunsigned*)((lfloat*)smem + 4 * ESZ1);
    if (cc < 4) {
      const bool ok = (unsigned)cc < (tinfo >> 29);
      const unsigned pix = (tinfo & T1_PIX) + (unsigned)(cc * pstride);
      sT[0 * TBL1 + cc * WT + lt] = ok ? pix * (unsigned)a.res_ld * 4u : OOB;
      sT[1 * TBL1 + cc * WT + lt] = ok ? pix * (unsigned)a.h_ld * 4u : OOB;
      sT[2 * TBL1 + cc * WT + lt] = ok ? pix * (unsigned)a.ch * 4u : OOB;
      sT[3 * TBL1 + cc * WT + lt] = OOB;
    }
    // row-walk role: pixel li = (8 * half + i) * 4 + prow of the wave's 64 (tile li >> 2, output li & 3), 4 columns from col4
    const int prow = lane >> 4, col4 = (lane & 15) * 4;
    const int w0 = cb * WN1 + wc * 64;               // (wave-uniform) the wave's first column
    const int n0 = w0 + col4;                        // cout % 4 == 0: the lane's four columns are inside or outside together
    const bool nok = n0 < a.cout;
    const int ch = a.ch;
    const bool upper = EPI == PFK_EPI_GRU_ZR && n0 >= ch;   // GRU_ZR: the r half
    const unsigned cn = (unsigned)n0 * 4u, chc = (unsigned)(upper ? n0 - ch : n0) * 4u;
    const __amdgpu_buffer_rsrc_t rbias = buffer_rsrc(a.bias, a.bias != nullptr ? (unsigned)a.cout * 4u : 0u);   // (no bias, pad columns: zero)
    f32x4 bias4;
#pragma unroll
    for (int j = 0; j < 4; ++j) bias4[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rbias, cn + 4u * j, 0, 0));
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // the tables are written

    const __amdgpu_buffer_rsrc_t rres = buffer_rsrc(a.res, a.res != nullptr ? a.res_bytes : 0u);   // (no context term: zero)
    const __amdgpu_buffer_rsrc_t rh = buffer_rsrc(a.h, a.h_bytes);
    // (wave-uniform) GRU_ZR: the wave's 64 columns lie in the z half, in the r half, or — hidden widths that are no multiple of 64 — in both
    const bool wupper = EPI == PFK_EPI_GRU_ZR && w0 >= ch, wh = EPI == PFK_EPI_GRU_ZR && w0 + 64 > ch, wmixed = wh && !wupper;
    const __amdgpu_buffer_rsrc_t rz = buffer_rsrc(wupper ? a.aux_rh : a.aux_z, a.z_bytes);   // GRU_ZR: stored; GRU_Q: read
    const __amdgpu_buffer_rsrc_t rrh = buffer_rsrc(a.aux_rh, a.z_bytes);                     // GRU_ZR, both halves in the wave: the r half's store
    const lunsigned* const tN = sT + 3 * TBL1 + prow * WT + wt * 16;   // the lane's place in the table without work
    const lunsigned* const tR = nok ? tN - 3 * TBL1 : tN;
    const lunsigned* const tH = (nok && (EPI == PFK_EPI_GRU_Q || upper)) ? tN - 2 * TBL1 : tN;
    const lunsigned* const tZ = (nok && upper == wupper) ? tN - 1 * TBL1 : tN;
    const lunsigned* const tZ2 = (nok && upper) ? tN - 1 * TBL1 : tN;

    const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};
    unsigned oo[2][8];                                // where the results go: GRU_ZR z | r*h, GRU_Q h
    f32x4 r4[2][8], h4[2][8], z4[2][8];
    {
      unsigned o[8];
      wino1d_epi_offsets(tR, cn, o);
      wino1d_epi_load(rres, o, r4[0]);
      if constexpr (EPI == PFK_EPI_GRU_ZR) {
        wino1d_epi_offsets(tZ, chc, oo[0]);
        if (wh) {
          wino1d_epi_offsets(tH, chc, o);
          wino1d_epi_load(rh, o, h4[0]);
        } else {
#pragma unroll
          for (int i = 0; i < 8; ++i) h4[0][i] = zero4;
        }
      } else {
        wino1d_epi_offsets(tZ, cn, o);
        wino1d_epi_load(rz, o, z4[0]);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    // MFMA role: A^T m is lane-local; parked at [pixel li = (4 * kq + r) * 4 + e][column] of the wave's own area (no barrier: a wave's
    // own LDS operations stay in order)
    {
      lfloat* const pE = sE + kq * (16 * ES1 + 16) + rl;
#pragma unroll
      for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float y[4];
          wino1d_at(acc, f, r, y);
#pragma unroll
          for (int e = 0; e < 4; ++e) pE[(r * 4 + e) * ES1 + f * 16] = y[e];
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    {
      unsigned o[8];
      if constexpr (EPI == PFK_EPI_GRU_Q) {
        wino1d_epi_offsets(tH, cn, oo[0]);
        wino1d_epi_load(rh, oo[0], h4[0]);
        wino1d_epi_offsets(tZ + 8, cn, o);
        wino1d_epi_load(rz, o, z4[1]);
      }
      wino1d_epi_offsets(tR + 8, cn, o);
      wino1d_epi_load(rres, o, r4[1]);
      if constexpr (EPI == PFK_EPI_GRU_ZR) {
        wino1d_epi_offsets(tZ + 8, chc, oo[1]);
        if (wh) {
          wino1d_epi_offsets(tH + 8, chc, o);
          wino1d_epi_load(rh, o, h4[1]);
        } else {
#pragma unroll
          for (int i = 0; i < 8; ++i) h4[1][i] = zero4;
        }
      } else {
        wino1d_epi_offsets(tH + 8, cn, oo[1]);
        wino1d_epi_load(rh, oo[1], h4[1]);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    const lfloat* const rE = sE + prow * ES1 + col4;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      unsigned o2[8];
      if constexpr (EPI == PFK_EPI_GRU_ZR) {
        if (wmixed) wino1d_epi_offsets(tZ2 + 8 * half, chc, o2);
      }
      f32x4 y[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int li4 = (half * 8 + i) * 4;           // the lane's pixel is li4 + prow
        y[i] = *(const lf32x4*)(rE + li4 * ES1 + (li4 >> 4) * 16);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const f32x4 o = wino1d_gate<EPI>(y[i], bias4, r4[half][i], h4[half][i], EPI == PFK_EPI_GRU_Q ? z4[half][i] : zero4, upper);
        if constexpr (EPI == PFK_EPI_GRU_ZR) {
          wino1d_epi_put(o, rz, oo[half][i]);
          if (wmixed) wino1d_epi_put(o, rrh, o2[i]);
        } else {
          wino1d_epi_put(o, rh, oo[half][i]);
        }
      }
    }
  }
}

// (not pfk_with_epilogue: its LINEAR / GRU_ZR / GRU_Q order would instantiate, hence emit, the six kernels in another order)
template <bool VERT>
static void wino1d_launch_epi(const Wino1dArgs& a, int epilogue, unsigned nblk, hipStream_t st) {
  switch (epilogue) {
    case PFK_EPI_GRU_ZR: hipLaunchKernelGGL((conv_gemm_wino1d_f32_kernel<VERT, PFK_EPI_GRU_ZR>), dim3(nblk), dim3(256), 0, st, a); break;
    case PFK_EPI_GRU_Q: hipLaunchKernelGGL((conv_gemm_wino1d_f32_kernel<VERT, PFK_EPI_GRU_Q>), dim3(nblk), dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL((conv_gemm_wino1d_f32_kernel<VERT, PFK_EPI_LINEAR>), dim3(nblk), dim3(256), 0, st, a); break;
  }
}

}  // namespace

extern "C" {

long long pfk_conv_wino1d_weight_floats(int ktot, int cout) {
  if (ktot <= 0 || cout <= 0 || (ktot & 7)) return PFK_ERR_BAD_ARG;
  return 8LL * ktot * ((cout + WN1 - 1) / WN1 * WN1);
}

int pfk_conv1d_wino_f32(const pfk_conv_desc* d, pfk_stream_t stream) {
  if (!d) return PFK_ERR_BAD_ARG;
  const bool vert = d->kh == 5 && d->kw == 1;
  if (!vert && !(d->kh == 1 && d->kw == 5)) return PFK_ERR_UNSUPPORTED;
  if (d->stride > 1 || d->num_src < 1 || d->num_src > 2 || d->relu_after_residual) return PFK_ERR_UNSUPPORTED;
  if (d->epilogue != PFK_EPI_LINEAR && d->epilogue != PFK_EPI_GRU_ZR && d->epilogue != PFK_EPI_GRU_Q) return PFK_ERR_UNSUPPORTED;
  if (d->cout_active > 0 && d->cout_active < d->cout) return PFK_ERR_UNSUPPORTED;
  if (d->epilogue == PFK_EPI_LINEAR && d->residual) return PFK_ERR_UNSUPPORTED;
  if (!d->weight || d->B <= 0 || d->H <= 0 || d->W <= 0 || d->cout <= 0) return PFK_ERR_BAD_ARG;
  const long long M = (long long)d->B * d->H * d->W;
  int ktot = 0;
  for (int i = 0; i < d->num_src; ++i) {
    const pfk_conv_src& s = d->src[i];
    if (!s.ptr || s.channels <= 0 || s.ld < s.channels) return PFK_ERR_BAD_ARG;
    if (s.channels & 7) return PFK_ERR_UNSUPPORTED;
    if (!pfk_aligned<4>(s.ptr)) return PFK_ERR_ALIGNMENT;
    if (!pfk_source_fits32(s, M, 4)) return PFK_ERR_UNSUPPORTED;   // 32-bit byte offsets
    ktot += s.channels;
  }
  const int ch = d->epilogue == PFK_EPI_GRU_ZR ? d->cout / 2 : d->cout;
  if (d->epilogue == PFK_EPI_LINEAR) {
    if (!d->out || d->out_coff < 0 || d->out_ld < d->out_coff + d->cout) return PFK_ERR_BAD_ARG;
    if (!pfk_aligned<4>(d->out)) return PFK_ERR_ALIGNMENT;
  } else {
    // the gate epilogues move float4 pieces of rows: hidden width % 4, 16-byte aligned rows
    if (!d->h || !d->aux_z || d->h_ld < ch || (d->epilogue == PFK_EPI_GRU_ZR && (!d->aux_rh || (d->cout & 1))) || (ch & 3))
      return PFK_ERR_BAD_ARG;
    if (d->residual && d->residual_ld < d->cout) return PFK_ERR_BAD_ARG;
    if (!pfk_aligned16(d->h) || !pfk_aligned16(d->aux_z) || !pfk_aligned16(d->aux_rh) || !pfk_aligned16(d->residual) || (d->h_ld & 3) ||
        (d->residual && (d->residual_ld & 3)))
      return PFK_ERR_ALIGNMENT;
    // the row walk's 32-bit byte offsets: the context term, h, z and r*h up to the last pixel's last column
    if ((d->residual && !pfk_fits32(((M - 1) * d->residual_ld + d->cout) * 4)) || !pfk_fits32(((M - 1) * d->h_ld + ch) * 4) ||
        !pfk_fits32(M * ch * 4))
      return PFK_ERR_UNSUPPORTED;
  }
  if (!pfk_aligned16(d->weight)) return PFK_ERR_ALIGNMENT;
  const long long wfloats = pfk_conv_wino1d_weight_floats(ktot, d->cout);
  if (!pfk_fits32(wfloats * 4)) return PFK_ERR_UNSUPPORTED;
  Wino1dArgs a{};
  const pfk_conv_src& s0 = d->src[0];
  const pfk_conv_src& s1 = d->src[d->num_src - 1];
  a.src0 = s0.ptr; a.ld0 = s0.ld; a.bytes0 = (unsigned)(((M - 1) * s0.ld + s0.channels) * 4);
  a.src1 = s1.ptr; a.ld1 = s1.ld; a.bytes1 = (unsigned)(((M - 1) * s1.ld + s1.channels) * 4);
  a.nks0 = s0.channels / WK; a.nks = ktot / WK;
  a.H = d->H; a.W = d->W;
  a.L = vert ? d->H : d->W;
  a.nt = (a.L + 3) / 4;
  const long long ntiles = (long long)d->B * (vert ? d->W : d->H) * a.nt;
  a.ncb = (d->cout + WN1 - 1) / WN1;
  const long long nblk = (ntiles + WT - 1) / WT * a.ncb;
  if (!pfk_fits32(nblk)) return PFK_ERR_UNSUPPORTED;
  a.ntiles = (int)ntiles;
  a.weight = d->weight; a.w_bytes = (unsigned)(wfloats * 4);
  a.bias = d->bias;
  a.cout = d->cout;
  a.relu = d->relu ? 1 : 0; a.scale = d->scale;
  a.out = d->out; a.out_ld = d->out_ld; a.out_coff = d->out_coff;
  a.res = d->residual; a.res_ld = d->residual_ld;
  a.h = d->h; a.h_ld = d->h_ld; a.aux_z = d->aux_z; a.aux_rh = d->aux_rh; a.ch = ch;
  if (d->epilogue != PFK_EPI_LINEAR) {
    a.res_bytes = d->residual ? (unsigned)(((M - 1) * d->residual_ld + d->cout) * 4) : 0u;
    a.h_bytes = (unsigned)(((M - 1) * d->h_ld + ch) * 4);
    a.z_bytes = (unsigned)(M * ch * 4);
  }
  if (vert) wino1d_launch_epi<true>(a, d->epilogue, (unsigned)nblk, static_cast<hipStream_t>(stream));
  else wino1d_launch_epi<false>(a, d->epilogue, (unsigned)nblk, static_cast<hipStream_t>(stream));
  return pfk_launch_status();
}

long long pfk_conv_wino_weight_floats(int cin, int cout) {
  if (cin <= 0 || cout <= 0 || (cin & 31)) return PFK_ERR_BAD_ARG;
  return 16LL * cin * ((cout + WN - 1) / WN * WN);
}

// blocks of 32 tiles per image where the tile list is laid out per image (the statistics form)
static inline long long wino_blocks_per_image(int H, int W) { return ((long long)((H + 1) / 2) * ((W + 1) / 2) + WT - 1) / WT; }

// What the fused forms add to a launch.  norm: the taps are normalised on load with in_mean / in_rstd [B][cin] (+ in_relu).
// stats: mean / rstd [B][cout] of the output come out of the epilogue's sums (workspace: pfk_conv_wino_stats_workspace_bytes).
struct WinoFuse {
  bool norm, stats;
  const float* in_mean; const float* in_rstd; int in_relu;
  float eps; float* out_mean; float* out_rstd; void* workspace; long long workspace_bytes;
};

// `res`: pfk_conv2d_wino_res_f32 (a residual is required and relu_after_residual honoured); else pfk_conv2d_wino_f32 (both refused)
static int wino_launch(const pfk_conv_desc* d, bool res, pfk_stream_t stream, const WinoFuse* f = nullptr) {
  if (!d) return PFK_ERR_BAD_ARG;
  const bool norm = f && f->norm, stats = f && f->stats;
  if (norm && (!f->in_mean || !f->in_rstd)) return PFK_ERR_BAD_ARG;
  if (stats && (!f->out_mean || !f->out_rstd || !f->workspace || d->residual || d->relu_after_residual)) return PFK_ERR_BAD_ARG;
  if (d->num_src != 1 || d->kh != 3 || d->kw != 3 || d->stride > 1 || d->epilogue != PFK_EPI_LINEAR)
    return PFK_ERR_UNSUPPORTED;
  if (!res && (d->residual || d->relu_after_residual)) return PFK_ERR_UNSUPPORTED;
  if (res && (!d->residual || d->residual_ld < d->cout || !pfk_aligned<4>(d->residual))) return PFK_ERR_BAD_ARG;
  const pfk_conv_src& s = d->src[0];
  if (!s.ptr || !d->weight || !d->out || d->B <= 0 || d->H <= 0 || d->W <= 0 || d->cout <= 0 || s.channels <= 0 ||
      s.ld < s.channels || d->out_coff < 0 || d->out_ld < d->out_coff + d->cout)
    return PFK_ERR_BAD_ARG;
  if (s.channels & 31) return PFK_ERR_UNSUPPORTED;
  if (!pfk_aligned16(d->weight) || !pfk_aligned<4>(s.ptr) || !pfk_aligned<4>(d->out))
    return PFK_ERR_ALIGNMENT;
  const long long M = (long long)d->B * d->H * d->W;
  const long long src_bytes = ((M - 1) * s.ld + s.channels) * 4;
  const long long wfloats = pfk_conv_wino_weight_floats(s.channels, d->cout);
  if (!pfk_source_fits32(s, M, 4) || !pfk_fits32(wfloats * 4)) return PFK_ERR_UNSUPPORTED;   // 32-bit byte offsets
  // the epilogue stores (and reads the residual) through buffer descriptors with 32-bit byte offsets from `out` (`residual`)
  const long long out_bytes = ((M - 1) * d->out_ld + d->out_coff + d->cout) * 4;
  const long long res_bytes = res ? ((M - 1) * d->residual_ld + d->cout) * 4 : 0;
  if (!pfk_fits32(out_bytes) || !pfk_fits32(res_bytes)) return PFK_ERR_UNSUPPORTED;
  int ncb = (d->cout + WN - 1) / WN;
  if (d->cout_active > 0 && d->cout_active < d->cout) {
    if (d->cout_active & (WN - 1)) return PFK_ERR_UNSUPPORTED;
    ncb = d->cout_active / WN;
    if (stats) return PFK_ERR_UNSUPPORTED;   // every column's sums are written
  }
  if (norm && (!pfk_aligned<4>(f->in_mean) || !pfk_aligned<4>(f->in_rstd))) return PFK_ERR_ALIGNMENT;
  if (stats) {
    if (!pfk_aligned<8>(f->workspace)) return PFK_ERR_ALIGNMENT;
    if (f->workspace_bytes < pfk_conv_wino_stats_workspace_bytes(d->B, d->H, d->W, d->cout)) return PFK_ERR_BAD_ARG;
  }
  WinoArgs a{};
  a.src = s.ptr; a.ld = s.ld; a.src_bytes = (unsigned)src_bytes;
  a.H = d->H; a.W = d->W;
  a.tw = (d->W + 1) / 2;
  a.tpi = a.tw * ((d->H + 1) / 2);
  const long long ntiles = (long long)d->B * a.tpi;
  const long long nbi = wino_blocks_per_image(d->H, d->W);
  const long long nblk = (stats ? d->B * nbi : (ntiles + WT - 1) / WT) * ncb;
  if (!pfk_fits32(nblk) || !pfk_fits32(ntiles)) return PFK_ERR_UNSUPPORTED;
  a.ntiles = (int)ntiles;
  a.nks = s.channels / WK;
  a.weight = d->weight; a.w_bytes = (unsigned)(wfloats * 4);
  a.bias = d->bias;
  a.cout = d->cout;
  a.ncb = ncb;
  a.relu = d->relu ? 1 : 0; a.scale = d->scale;
  a.out = d->out; a.out_ld = d->out_ld; a.out_coff = d->out_coff; a.out_bytes = (unsigned)out_bytes;
  a.vec = pfk_aligned16(d->out + d->out_coff) && !(d->out_ld & 3) && (!res || (pfk_aligned16(d->residual) && !(d->residual_ld & 3)));
  if (norm) {
    a.in_mean = f->in_mean; a.in_rstd = f->in_rstd; a.in_relu = f->in_relu ? 1 : 0;
    a.cin = s.channels; a.stat_bytes = (unsigned)((long long)d->B * s.channels * 4);
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (stats) {
    a.nbi = (int)nbi;
    a.part = static_cast<double*>(f->workspace);
    a.astride = (long long)d->B * nbi * d->cout;
    if (norm) hipLaunchKernelGGL((conv_gemm_wino_f32_kernel<false, true, true>), dim3((unsigned)nblk), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((conv_gemm_wino_f32_kernel<false, false, true>), dim3((unsigned)nblk), dim3(256), 0, st, a);
    return pfk_instnorm_finish_parts(a.part, d->B, a.nbi, d->cout, d->H * d->W, f->eps, f->out_mean, f->out_rstd, st);
  }
  if (norm) {
    if (res) return PFK_ERR_UNSUPPORTED;
    hipLaunchKernelGGL((conv_gemm_wino_f32_kernel<false, true, false>), dim3((unsigned)nblk), dim3(256), 0, st, a);
    return pfk_launch_status();
  }
  if (res) {
    if (d->cout_active > 0 && d->cout_active < d->cout) return PFK_ERR_UNSUPPORTED;
    a.res = d->residual; a.res_ld = d->residual_ld; a.res_bytes = (unsigned)res_bytes; a.relu2 = d->relu_after_residual ? 1 : 0;
    hipLaunchKernelGGL(conv_gemm_wino_f32_kernel<true>, dim3((unsigned)nblk), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  } else {
    hipLaunchKernelGGL(conv_gemm_wino_f32_kernel<false>, dim3((unsigned)nblk), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  }
  return pfk_launch_status();
}

int pfk_conv2d_wino_f32(const pfk_conv_desc* d, pfk_stream_t stream) { return wino_launch(d, false, stream); }

int pfk_conv2d_wino_res_f32(const pfk_conv_desc* d, pfk_stream_t stream) { return wino_launch(d, true, stream); }

int pfk_conv2d_wino_norm_f32(const pfk_conv_desc* d, const float* in_mean, const float* in_rstd, int in_relu, pfk_stream_t stream) {
  const WinoFuse f{true, false, in_mean, in_rstd, in_relu, 0.f, nullptr, nullptr, nullptr, 0};
  return wino_launch(d, false, stream, &f);
}

long long pfk_conv_wino_stats_workspace_bytes(int B, int H, int W, int cout) {
  if (B <= 0 || H <= 0 || W <= 0 || cout <= 0) return PFK_ERR_BAD_ARG;
  return 2LL * B * wino_blocks_per_image(H, W) * cout * (long long)sizeof(double);
}

int pfk_conv2d_wino_stats_f32(const pfk_conv_desc* d, const float* in_mean, const float* in_rstd, int in_relu, float eps,
                              float* out_mean, float* out_rstd, void* workspace, long long workspace_bytes, pfk_stream_t stream) {
  if ((in_mean == nullptr) != (in_rstd == nullptr)) return PFK_ERR_BAD_ARG;
  const WinoFuse f{in_mean != nullptr, true, in_mean, in_rstd, in_relu, eps, out_mean, out_rstd, workspace, workspace_bytes};
  return wino_launch(d, false, stream, &f);
}


}  // extern "C"
