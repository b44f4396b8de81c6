// Shared helpers for the libpfk.so translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pfk.h"

#define PFK_WAVE 64

// ------------------------------------------------------------------------------------------------ device primitives, one body each
// The kernels' "same bits as the fp32 kernel" claims rest on these being the ONLY definitions: vector types, bf16 row access, wave
// reductions, the buffer descriptor and the two activations.  LDS aliases and the MFMA operand types stay with their one user.
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
// explicit global address space: through a generic pointer hipcc emits flat_store where the kernels want global_store
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) f32x4 gf32x4;
typedef __attribute__((address_space(1))) __bf16 gbf16;
typedef __attribute__((address_space(1))) u32x2 gu32x2;
typedef __attribute__((address_space(1))) u32x4 gu32x4;

// two bf16 of one 32-bit word (element 0 in the low half) -> fp32, exact
__device__ __forceinline__ f32x2 widen2(unsigned w) {
  return f32x2{__builtin_bit_cast(float, w << 16), __builtin_bit_cast(float, w & 0xffff0000u)};
}
__device__ __forceinline__ f32x4 widen4(u32x2 w) {
  f32x4 v;
  v[0] = __builtin_bit_cast(float, w[0] << 16); v[1] = __builtin_bit_cast(float, w[0] & 0xffff0000u);
  v[2] = __builtin_bit_cast(float, w[1] << 16); v[3] = __builtin_bit_cast(float, w[1] & 0xffff0000u);
  return v;
}

// N consecutive elements of a row as fp32 (bf16: widened, exact) and back (bf16: one rounding to nearest even each, one store);
// p is N * sizeof(T) aligned
template <int N>
__device__ __forceinline__ void load_row(const float* p, float* v) {
  if constexpr (N == 1) v[0] = *p;
  else {
    static_assert(N == 4, "one float or one float4");
    const f32x4 q = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = q[e];
  }
}
template <int N>
__device__ __forceinline__ void load_row(const __bf16* p, float* v) {
  static_assert(N == 2 || N == 4 || N == 8, "4, 8 or 16 bytes of a bf16 row");
  typedef unsigned int u32xW __attribute__((ext_vector_type(N / 2)));
  const u32xW w = *reinterpret_cast<const u32xW*>(p);
#pragma unroll
  for (int e = 0; e < N / 2; ++e) {
    const f32x2 f = widen2(w[e]);
    v[2 * e] = f.x; v[2 * e + 1] = f.y;
  }
}
template <int N>
__device__ __forceinline__ void store_row(float* p, const float* v) {
  if constexpr (N == 1) *p = v[0];
  else {
    static_assert(N == 4, "one float or one float4");
    *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
  }
}
template <int N>
__device__ __forceinline__ void store_row(__bf16* p, const float* v) {
  typedef __bf16 bf16xN __attribute__((ext_vector_type(N)));
  bf16xN q;
#pragma unroll
  for (int e = 0; e < N; ++e) q[e] = (__bf16)v[e];
  *reinterpret_cast<bf16xN*>(p) = q;
}
__device__ __forceinline__ f32x4 load4_widen(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 load4_widen(const __bf16* p) {      // four bf16 (8 bytes) -> fp32, exact
  return widen4(*reinterpret_cast<const u32x2*>(p));
}
__device__ __forceinline__ void store4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ void store4(__bf16* p, f32x4 v) {
  const float a[4] = {v[0], v[1], v[2], v[3]};
  store_row<4>(p, a);
}

// Butterfly over W adjacent lanes, offsets W/2 down to 1: the order of the additions is part of every kernel's contract
template <int W = 64, class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = W / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <int W = 64>
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = W / 2; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// Raw-buffer descriptor of `bytes` bytes at p (default: no bound the kernels rely on; they mask with an offset >= 2^31 instead)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void* p, unsigned bytes = 0x7fffffffu) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}

__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }
// nn.GELU() (approximate='none'): 0.5 * v * (1 + erf(v / sqrt(2)))
__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); }

// pfk_debug_set_* are inert unless the process opted in (include/pfk.h)
#include <stdlib.h>
static inline bool pfk_debug_knobs_enabled() {
  const char* e = getenv("PFK_DEBUG_KNOBS");
  return e && e[0] == '1' && e[1] == 0;
}

// Division of n < 2^31 by a launch-invariant d through a host-made multiplier (Granlund & Montgomery 1994, N = 32):
//   l = ceil(log2 d), mul = floor(2^32 (2^l - d) / d) + 1,  n / d = (mulhi(mul, n) + n) >> l   (no overflow: mulhi(..) <= n < 2^31)
// three instructions instead of the ~30 of a runtime 32-bit (or ~100 of a 64-bit) division.
static inline void fastdiv_make(unsigned d, unsigned& mul, int& sh) {
  int l = 0;
  while ((1ull << l) < d) ++l;
  mul = (unsigned)(((1ull << 32) * ((1ull << l) - d)) / d + 1ull);
  sh = l;
}
__host__ __device__ __forceinline__ unsigned fastdiv_u32(unsigned n, unsigned mul, int sh) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (__umulhi(n, mul) + n) >> sh;
#else
  return (unsigned)((((unsigned long long)n * mul) >> 32) + n) >> sh;
#endif
}

// pfk_encoder.hip, for the Winograd kernel's statistics epilogue (pfk_wino.hip): part = sums, then sums of squares, each
// [B][nch][C] doubles, reduced over nch in chunk_reduce_kernel's fixed order and finished as pfk_instnorm_stats_f32 finishes
// (mean, rstd in double, rounded once).  Arguments are the caller's to check.
int pfk_instnorm_finish_parts(const double* part, int B, int nch, int C, int HW, float eps, float* mean, float* rstd, hipStream_t st);

// Bijective XCD-aware block remap (8 XCDs, dispatcher places block b on XCD b % 8): gives each
// XCD one contiguous range of tile ids so tiles that share operand panels share an L2.
__device__ __forceinline__ int pfk_xcd_remap(int bid, int nblk) {
  const int q = nblk >> 3, r = nblk & 7;
  const int xcd = bid & 7, local = bid >> 3;
  const int start = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return start + local;
}
