// Slice reduction of the weight-gradient kernels (pfk_wgrad.hip: fp32 operands, pfk_wgrad_b16.hip: bf16 operands), written
// straight into PyTorch's layouts: dw [cout][cin][kh][kw] (cin = the sources' REAL channels one after the other) and db [cout]
// — the inverse of the host's weight packing (ptlflow_amd/packing.py), so a training step needs no per-call permute / copy
// kernels between the weight-gradient launch and autograd's accumulation.  Both main kernels leave fp32 partial tiles
// [splits][cout][ktot] whose K enumeration is (source, tap, channel padded to 32) [+ one 32-column bias chunk].
// In front of it, what the two launchers plan alike: tile height, grid, pixel slices and the launch by tile height.
#pragma once
#include "pfk_conv_k.h"   // chunk_ref: the main kernels' (source, tap, chunk) entries, in the K order this file's kernel inverts
#include "pfk_launch.h"

namespace {

struct UnpackArgs {
  const float* part; long long n; int splits;
  int ktot, cout_real, taps, nseg, cin_total, with_bias, accumulate;
  int first[3], nreal[3], cpad[3];
  float* dw; float* db;
};

// 32-row output-channel blocks per tile: the tallest tile among {4, 2, 1} blocks that pads cout the least (forced: 1 / 2 / 4)
inline int wgrad_pick_cb(int cout, int forced = 0) {
  if (forced == 1 || forced == 2 || forced == 4) return forced;
  int best = 4, waste = (cout + 127) / 128 * 128 - cout;
  const int w2 = (cout + 63) / 64 * 64 - cout, w1 = (cout + 31) / 32 * 32 - cout;
  if (w2 < waste) { best = 2; waste = w2; }
  if (w1 < waste) best = 1;
  return best;
}

// grid of the main launch for a tile height: (cout tiles) x (groups of 4 / cb K chunks of 32 columns)
struct WgradGrid { int cb, tiles_m, groups; };
inline WgradGrid wgrad_grid(int cout, int ktot, int cb) {
  return WgradGrid{cb, (cout + 32 * cb - 1) / (32 * cb), (ktot / 32 + 4 / cb - 1) / (4 / cb)};
}

// Pixel slices: about 1024 blocks in all, at least `min_steps` of the slice's `ksteps` K-steps each, at most 64 (forced > 0: that
// many, as far as there are K-steps)
inline int wgrad_pick_splits(long long tiles, long long ksteps, int min_steps, int forced = 0) {
  long long s = forced;
  if (forced <= 0) {
    s = 1024 / (tiles > 0 ? tiles : 1);
    const long long max_s = ksteps / min_steps > 0 ? ksteps / min_steps : 1;
    if (s > max_s) s = max_s;
  }
  if (s > ksteps) s = ksteps;
  if (s > 64) s = 64;
  return s < 1 ? 1 : (int)s;
}

// the main kernel of tile height cb
template <auto K4, auto K2, auto K1, class Args>
inline void wgrad_launch_cb(int cb, dim3 grid, hipStream_t st, const Args& a) {
  if (cb == 4) hipLaunchKernelGGL(K4, grid, dim3(256), 0, st, a);
  else if (cb == 2) hipLaunchKernelGGL(K2, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(K1, grid, dim3(256), 0, st, a);
}

// arguments of the slice reduction below; real_channels[s] in 1..src[s].channels is the caller's to check
template <class D>
inline UnpackArgs wgrad_unpack_args(const D* d, const int* real_channels, const float* part, long long n, int splits, int ktot, int cout_real,
                                    int with_bias, float* dw, float* db, int accumulate) {
  UnpackArgs u{};
  u.part = part; u.n = n; u.splits = splits; u.ktot = ktot; u.cout_real = cout_real; u.taps = d->kh * d->kw;
  u.nseg = d->num_src; u.with_bias = with_bias; u.dw = dw; u.db = db; u.accumulate = accumulate != 0;
  int first = 0;
  for (int i = 0; i < d->num_src; ++i) {
    u.first[i] = first; u.nreal[i] = real_channels[i]; u.cpad[i] = (d->src[i].channels + 31) / 32 * 32;
    first += real_channels[i];
  }
  u.cin_total = first;
  return u;
}

__global__ __launch_bounds__(256) void wgrad_reduce_unpack_kernel(const UnpackArgs u) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)u.cout_real * u.ktot) return;
  const int co = (int)(idx / u.ktot), k = (int)(idx - (long long)co * u.ktot);
  float s = u.part[idx];
  for (int j = 1; j < u.splits; ++j) s += u.part[(long long)j * u.n + idx];      // same fixed order as wgrad_reduce_kernel
  int kk = k;
  if (u.with_bias && k >= u.ktot - 32) {
    if (k == u.ktot - 32 && u.db) u.db[co] = u.accumulate ? u.db[co] + s : s;
    return;
  }
  int sg = 0;
  while (sg < u.nseg - 1 && kk >= u.taps * u.cpad[sg]) { kk -= u.taps * u.cpad[sg]; ++sg; }
  const int tap = kk / u.cpad[sg], c = kk - tap * u.cpad[sg];
  if (c < u.nreal[sg]) {
    float* dst = u.dw + ((long long)co * u.cin_total + u.first[sg] + c) * u.taps + tap;
    *dst = u.accumulate ? *dst + s : s;     // (one thread per element: the running sum's order is the order of the calls)
  }
}

}  // namespace
