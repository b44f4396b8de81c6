// The K order of the packed convolution weight, one body each.  K-step k of a launch is one (source, tap with ky major, channel
// chunk of BK with the source's channels padded up to BK): packing.pack_conv_weight lays the weight out in this order, pfk_conv_k
// (pfk_launch.h) counts it, the forward stagers walk it (conv_k_advance), the stream-K kernels seek into it (conv_k_decode), the
// weight-gradient kernels enumerate it (chunk_ref) and wgrad_reduce_unpack_kernel inverts it.  Pure integer arithmetic that
// includes nothing: scripts/conv_k_order_main.cpp compiles it for the host alone and tests/test_conv_k_order.py holds it to the
// packing.
#pragma once

#if defined(__HIP__)   // what __host__ __device__ __forceinline__ of the HIP runtime header stand for
#define PFK_K_FN __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define PFK_K_FN inline
#endif

// K-step -> (source, tap (ky, kx), first channel of the chunk).  ch = the sources' channel counts, three consecutive ints (the
// argument blocks and the stagers keep ch0, ch1, ch2 next to each other for this); a count past nsrc is never read.
// (Returns ky and kx, not the tap number, and takes the counts through a pointer: in this form the stream-K and persistent
//  kernels compile to what they were when seek() and seek_args() each wrote the walk out.)
struct ConvKPos { int seg, ky, kx, c0; };
template <int BK>
PFK_K_FN ConvKPos conv_k_decode(int step, int kh, int kw, int nsrc, const int* ch) {
  const int taps = kh * kw;
  int r = step, sg = 0, cps = (ch[0] + BK - 1) / BK;
  if (nsrc > 1 && r >= taps * cps) {
    r -= taps * cps; sg = 1; cps = (ch[1] + BK - 1) / BK;
    if (nsrc > 2 && r >= taps * cps) { r -= taps * cps; sg = 2; cps = (ch[2] + BK - 1) / BK; }
  }
  const int tap = r / cps, ky = tap / kw;
  return ConvKPos{sg, ky, tap - ky * kw, (r - tap * cps) * BK};
}

// One K-step forward: next chunk -> next tap -> next source.  S keeps seg, ky, kx, c0, kofs (and the running `tap` when TAPS), the
// current source's channel count cch, kh, kw, nsrc, and re-derives its per-source / per-tap state in set_segment() / set_tap().
template <int BK, bool TAPS = false, class S>
PFK_K_FN void conv_k_advance(S& st) {
  st.kofs += BK;
  st.c0 += BK;
  if (st.c0 >= st.cch) {
    st.c0 = 0;
    if constexpr (TAPS) ++st.tap;
    if (++st.kx == st.kw) {
      st.kx = 0;
      if (++st.ky == st.kh) {
        st.ky = 0;
        if constexpr (TAPS) st.tap = 0;
        ++st.seg;
        if (st.seg < st.nsrc) st.set_segment(st.seg);
      }
    }
    st.set_tap();
  }
}

// One 32-channel entry of the K enumeration as the weight-gradient kernels see it: the source's rows, the chunk's first channel and
// the tap re-centred on the output pixel.  A = WgradArgs / WgradB16Args (chunks counts the bias chunk when with_bias: the last one).
template <class P>
struct ChunkRef { P src; int ld, cch, c0, dy, dx, bias, live; };
template <class A>
PFK_K_FN auto chunk_ref(const A& a, int chunk) {
  ChunkRef<decltype(a.src0)> c;
  // restates conv_k_decode<32>'s walk (selecting the source along the way, chunks per source by shift): through the call both
  // weight-gradient kernels came out with other instructions.  tests/test_conv_k_order.py holds the two to each other.
  const int taps = a.kh * a.kw;
  int r = chunk, cps = (a.ch0 + 31) >> 5;
  c.src = a.src0; c.ld = a.ld0; c.cch = a.ch0;
  if (a.nsrc > 1 && r >= taps * cps) {
    r -= taps * cps; cps = (a.ch1 + 31) >> 5; c.src = a.src1; c.ld = a.ld1; c.cch = a.ch1;
    if (a.nsrc > 2 && r >= taps * cps) { r -= taps * cps; cps = (a.ch2 + 31) >> 5; c.src = a.src2; c.ld = a.ld2; c.cch = a.ch2; }
  }
  c.live = chunk < a.chunks;
  c.bias = a.with_bias && chunk == a.chunks - 1;
  const bool plain = c.live && !c.bias;
  const int tap = plain ? r / cps : 0;
  c.c0 = plain ? (r - tap * cps) * 32 : 0;
  c.dy = plain ? tap / a.kw - (a.kh >> 1) : 0;
  c.dx = plain ? tap % a.kw - (a.kw >> 1) : 0;
  return c;
}
