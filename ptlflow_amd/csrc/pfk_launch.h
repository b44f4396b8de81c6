// Host side shared by the launchers behind include/pfk.h, one body each: the 32-bit limits, pointer alignment, the launch that raises a
// kernel's dynamic-LDS limit, the epilogue dispatch and the view of a convolution descriptor.  Device code stays in pfk_common.h.
#pragma once
#include <atomic>
#include <type_traits>

#include "pfk_common.h"

// The kernels keep byte offsets from an operand's pointer, pixel numbers and work-unit counts in 32-bit registers, and an offset with
// bit 31 set is how the buffer instructions mask a lane off (buffer_rsrc): whatever a kernel counts that way stays BELOW 2^31 - 1.
static inline bool pfk_fits32(long long n) { return n < 0x7fffffffLL; }
// ... while a grid dimension, or a count a kernel takes as `int`, may be 2^31 - 1 itself.
static inline bool pfk_fits_int(long long n) { return n <= 0x7fffffffLL; }

static inline bool pfk_aligned(const void* p, size_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }
template <int N>
static inline bool pfk_aligned(const void* p) {
  static_assert(N > 0 && (N & (N - 1)) == 0, "a power of two");
  return pfk_aligned(p, N);
}
static inline bool pfk_aligned16(const void* p) { return pfk_aligned<16>(p); }

static inline int pfk_launch_status() { return hipGetLastError() == hipSuccess ? PFK_OK : PFK_ERR_LAUNCH; }

// hipFuncSetAttribute is per DEVICE: a process that drives several GPUs (model.to("cuda:1"), DataParallel) must raise the
// dynamic-LDS limit of a kernel on each of them.  One flag per (kernel instantiation, device), lock-free after the first call.
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

// Raise Kern's dynamic-LDS limit to LIMIT bytes, once per device.  The kernel is a template argument, so the flag below is one per
// kernel instantiation; safe with several host threads.
template <auto Kern, size_t LIMIT>
static inline void pfk_raise_lds_limit() {
  static pfk_device_once attr_once;
  attr_once.run([] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LIMIT);
  });
}
// ... and launch it with `smem` <= LIMIT bytes of dynamic LDS
template <auto Kern, size_t LIMIT, class... Args>
static inline int pfk_launch_lds(dim3 grid, dim3 block, size_t smem, hipStream_t st, const Args&... args) {
  pfk_raise_lds_limit<Kern, LIMIT>();
  hipLaunchKernelGGL(Kern, grid, block, smem, st, args...);
  return pfk_launch_status();
}

// f(std::integral_constant<int, E>{}) for the epilogue every conv kernel is instantiated on; anything else is a bad argument
template <class F>
static inline int pfk_with_epilogue(int epi, F&& f) {
  switch (epi) {
    case PFK_EPI_LINEAR: return f(std::integral_constant<int, PFK_EPI_LINEAR>{});
    case PFK_EPI_GRU_ZR: return f(std::integral_constant<int, PFK_EPI_GRU_ZR>{});
    case PFK_EPI_GRU_Q: return f(std::integral_constant<int, PFK_EPI_GRU_Q>{});
    default: return PFK_ERR_BAD_ARG;
  }
}

// ------------------------------------------------------------------------------- a convolution descriptor, seen by its launchers
// D is pfk_conv_desc or pfk_conv_b16_desc: the fields read here have one meaning in both.

// K of the packed weight: for each source and tap, the source's channels padded up to `kpad`.  A null descriptor or a source count
// outside 1..3 (which would index past src[]): PFK_ERR_BAD_ARG.
template <class D>
static inline int pfk_conv_k(const D* d, int kpad) {
  if (!d || d->num_src < 1 || d->num_src > 3) return PFK_ERR_BAD_ARG;
  int k = 0;
  for (int s = 0; s < d->num_src; ++s) k += d->kh * d->kw * ((d->src[s].channels + kpad - 1) / kpad * kpad);
  return k;
}

// stride (0 means 1), the output grid of a "same"-padded convolution, and the rows of the sources (M_in) and of the output (M_out)
struct pfk_conv_geometry { int stride, Ho, Wo; long long M_in, M_out; };
template <class D>
static inline pfk_conv_geometry pfk_conv_geom(const D* d) {
  pfk_conv_geometry g;
  g.stride = d->stride > 0 ? d->stride : 1;
  g.Ho = (d->H - 1) / g.stride + 1;
  g.Wo = (d->W - 1) / g.stride + 1;
  g.M_in = (long long)d->B * d->H * d->W;
  g.M_out = (long long)d->B * g.Ho * g.Wo;
  return g;
}

// One source, in the launchers' order of precedence: no pointer, no channels or rows shorter than the channels — BAD_ARG; a pointer
// off `align` bytes, a row stride or channel count off `quantum` elements — ALIGNMENT.
template <class S>
static inline int pfk_check_source(const S& s, int quantum, int align) {
  if (!s.ptr || s.channels <= 0 || s.ld < s.channels) return PFK_ERR_BAD_ARG;
  if (!pfk_aligned(s.ptr, align) || (s.ld & (quantum - 1)) || (s.channels & (quantum - 1))) return PFK_ERR_ALIGNMENT;
  return PFK_OK;
}
// `rows` rows of the source, `esize` bytes per element, within 32-bit byte offsets
template <class S>
static inline bool pfk_source_fits32(const S& s, long long rows, int esize) { return pfk_fits32(rows * s.ld * esize); }

// src0 / ld0 / ch0 .. src2 / ld2 / ch2 and nsrc of a kernel's argument block (sources past num_src keep what `a` holds: zeros)
template <class A, class D>
static inline void pfk_spread_sources(A& a, const D* d) {
  a.src0 = d->src[0].ptr; a.ld0 = d->src[0].ld; a.ch0 = d->src[0].channels;
  if (d->num_src > 1) { a.src1 = d->src[1].ptr; a.ld1 = d->src[1].ld; a.ch1 = d->src[1].channels; }
  if (d->num_src > 2) { a.src2 = d->src[2].ptr; a.ld2 = d->src[2].ld; a.ch2 = d->src[2].channels; }
  a.nsrc = d->num_src;
}
