// Shared helpers for the libpfk.so translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pfk.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ f32x4 load4_widen(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 load4_widen(const __bf16* p) {      // four bf16 (8 bytes) -> fp32, exact
  typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
  const u32x2 w = *reinterpret_cast<const u32x2*>(p);
  f32x4 v;
  v.x = __builtin_bit_cast(float, w[0] << 16); v.y = __builtin_bit_cast(float, w[0] & 0xffff0000u);
  v.z = __builtin_bit_cast(float, w[1] << 16); v.w = __builtin_bit_cast(float, w[1] & 0xffff0000u);
  return v;
}

#define PFK_WAVE 64

static inline bool pfk_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// hipFuncSetAttribute is per DEVICE: a process that drives several GPUs (model.to("cuda:1"), DataParallel) must raise the
// dynamic-LDS limit of a kernel on each of them.  One flag per (kernel instantiation, device), lock-free after the first call.
#include <atomic>
constexpr int PFK_MAX_DEVICES = 64;
struct pfk_device_once {
  std::atomic<unsigned char> done[PFK_MAX_DEVICES] = {};
  template <class F>
  void run(F&& f) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= PFK_MAX_DEVICES) { f(); return; }
    if (done[dev].load(std::memory_order_acquire)) return;
    f();   // idempotent: two threads racing here both set the same attribute value
    done[dev].store(1, std::memory_order_release);
  }
};

// pfk_debug_set_* are inert unless the process opted in (include/pfk.h)
#include <stdlib.h>
static inline bool pfk_debug_knobs_enabled() {
  const char* e = getenv("PFK_DEBUG_KNOBS");
  return e && e[0] == '1' && e[1] == 0;
}

static inline int pfk_launch_status() {
  return hipGetLastError() == hipSuccess ? PFK_OK : PFK_ERR_LAUNCH;
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
