// Slice reduction of the weight-gradient kernels (pfk_wgrad.hip: fp32 operands, pfk_wgrad_b16.hip: bf16 operands), written
// straight into PyTorch's layouts: dw [cout][cin][kh][kw] (cin = the sources' REAL channels one after the other) and db [cout]
// — the inverse of the host's weight packing (ptlflow_amd/packing.py), so a training step needs no per-call permute / copy
// kernels between the weight-gradient launch and autograd's accumulation.  Both main kernels leave fp32 partial tiles
// [splits][cout][ktot] whose K enumeration is (source, tap, channel padded to 32) [+ one 32-column bias chunk].
#pragma once
#include "pfk_common.h"

namespace {

struct UnpackArgs {
  const float* part; long long n; int splits;
  int ktot, cout_real, taps, nseg, cin_total, with_bias, accumulate;
  int first[3], nreal[3], cpad[3];
  float* dw; float* db;
};

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
