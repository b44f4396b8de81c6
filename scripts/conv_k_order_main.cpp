// The K order of ptlflow_amd/csrc/pfk_conv_k.h, printed by a host program for tests/test_conv_k_order.py (no HIP, no GPU):
//
//   clang++ -std=c++17 -Iptlflow_amd/csrc scripts/conv_k_order_main.cpp -o conv_k_order && ./conv_k_order < cases
//
// A case is one line `bk nsrc ch0 ch1 ch2 kh kw` (bk 32 or 64).  Per case: `C <the case> <steps>`, then one line per K-step
//   S step | decode(step): seg ky kx c0 | the position advance() reached from step 0: seg ky kx c0 kofs tap
// and, for bk 32, one line per chunk 0 .. steps + 1 of a weight-gradient launch WITH a bias chunk (chunk `steps`; the one past it is dead)
//   R chunk | chunk_ref(chunk): ld c0 dy dx bias live          (source s has ld 100 + s)
#include <cstdio>

#include "pfk_conv_k.h"

namespace {

// what conv_k_advance asks of a stager
struct Walk {
  int seg = 0, ky = 0, kx = 0, c0 = 0, kofs = 0, tap = 0;
  int cch, kh, kw, nsrc, ch[3];
  void set_segment(int s) { cch = ch[s]; }
  void set_tap() {}
};

// what chunk_ref asks of a weight-gradient argument block
struct Args {
  const void* src0; const void* src1; const void* src2;
  int ld0, ld1, ld2, ch0, ch1, ch2, nsrc;
  int kh, kw, chunks, with_bias;
};

template <int BK>
int steps_of(const Walk& w) {
  int s = 0;
  for (int i = 0; i < w.nsrc; ++i) s += w.kh * w.kw * ((w.ch[i] + BK - 1) / BK);
  return s;
}

template <int BK, bool TAPS>
void run(Walk w) {
  const int steps = steps_of<BK>(w);
  std::printf("C %d %d %d %d %d %d %d %d\n", BK, w.nsrc, w.ch[0], w.ch[1], w.ch[2], w.kh, w.kw, steps);
  w.set_segment(0);
  w.set_tap();
  for (int step = 0; step < steps; ++step) {
    const ConvKPos k = conv_k_decode<BK>(step, w.kh, w.kw, w.nsrc, w.ch);
    std::printf("S %d %d %d %d %d %d %d %d %d %d %d\n", step, k.seg, k.ky, k.kx, k.c0, w.seg, w.ky, w.kx, w.c0, w.kofs,
                TAPS ? w.tap : w.ky * w.kw + w.kx);
    if (step + 1 < steps) conv_k_advance<BK, TAPS>(w);   // as the kernels: never past the last step
  }
  if (BK != 32) return;
  Args a{};
  a.ld0 = 100; a.ld1 = 101; a.ld2 = 102; a.ch0 = w.ch[0]; a.ch1 = w.ch[1]; a.ch2 = w.ch[2]; a.nsrc = w.nsrc;
  a.kh = w.kh; a.kw = w.kw; a.chunks = steps + 1; a.with_bias = 1;
  for (int c = 0; c <= steps + 1; ++c) {
    const auto r = chunk_ref(a, c);
    std::printf("R %d %d %d %d %d %d %d\n", c, r.ld, r.c0, r.dy, r.dx, r.bias, r.live);
  }
}

}  // namespace

int main() {
  int bk;
  Walk w;
  while (std::scanf("%d %d %d %d %d %d %d", &bk, &w.nsrc, &w.ch[0], &w.ch[1], &w.ch[2], &w.kh, &w.kw) == 7) {
    if (w.nsrc < 1 || w.nsrc > 3 || w.kh < 1 || w.kw < 1 || w.ch[0] < 1) return 2;
    if (bk == 32) run<32, false>(w);
    else if (bk == 64) run<64, true>(w);      // the bf16 stager also counts a running tap
    else return 2;
  }
  return 0;
}
