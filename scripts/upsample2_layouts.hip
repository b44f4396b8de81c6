// Lane-layout experiment behind `convex_upsample2_kernel` (pfk_upsample.hip; profiles/r27_a_ms_upsample.md §1) — a stand-alone program,
// not part of the library: three layouts around the same arithmetic (pfk_upsample.h), checked bit for bit against each other, timed
// alternately (10 rounds of 50 back-to-back launches each, the first dropped; median and max - min in us).
//   A  lane = (coarse pixel, sy): nine 8-byte mask reads, one 8-byte store per channel; a wave = 32 consecutive pixels  (the library's)
//   B  as A, but a 256-thread block first stages its 128 pixels' mask rows into LDS with coalesced 4-byte reads
//   C  lane = (coarse pixel, sy, sx): nine 4-byte mask reads, one 4-byte store per channel; a wave = 16 consecutive pixels
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Iptlflow_amd/csrc -Iinclude scripts/upsample2_layouts.hip -o upsample2_layouts
//   ./upsample2_layouts
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pfk_upsample.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(2); } } while (0)

__device__ __forceinline__ void finish(float (&m)[2][9], const float* flow, long long img, const UpPixel& px, int sy, float* out, int H, int W) {
  float v[2][9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    float f[2];
    up_tap<0, 2>(k, flow, 0, nullptr, 0, 0, img, px.y, px.x, H, W, f);
    v[0][k] = f[0];
    v[1][k] = f[1];
  }
  up_softmax9(m[0]);
  up_softmax9(m[1]);
  const long long HW4 = (long long)H * W * 4;
  const long long at = up_out_offset<2>(px.y, px.x, sy, 0, W);
#pragma unroll
  for (int ch = 0; ch < 2; ++ch) {
    const float o0 = up_combine(m[0], v[ch]), o1 = up_combine(m[1], v[ch]);
    *reinterpret_cast<f32x2*>(out + (px.b * 2 + ch) * HW4 + at) = f32x2{o0, o1};
  }
}

__global__ __launch_bounds__(256) void layout_a(const float* __restrict__ flow, const float* __restrict__ mask, int mask_ld,
                                                float* __restrict__ out, long long M, int H, int W) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63, sy = lane >> 5;
  const long long p = (t >> 6) * 32 + (lane & 31);
  if (p >= M) return;
  const UpPixel px = up_pixel(p, H, W);
  const float* mrow = mask + p * mask_ld + sy * 2;
  float m[2][9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const f32x2 w = *reinterpret_cast<const f32x2*>(mrow + k * 4);
    m[0][k] = w[0];
    m[1][k] = w[1];
  }
  finish(m, flow, px.b * ((long long)H * W), px, sy, out, H, W);
}

__global__ __launch_bounds__(256) void layout_b(const float* __restrict__ flow, const float* __restrict__ mask, int mask_ld,
                                                float* __restrict__ out, long long M, int H, int W) {
  __shared__ float rows[128 * 36];
  const long long p0 = (long long)blockIdx.x * 128;
  for (int e = threadIdx.x; e < 128 * 36; e += 256) {
    const int r = e / 36, c = e - r * 36;
    rows[e] = p0 + r < M ? mask[(p0 + r) * mask_ld + c] : 0.f;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, sy = lane >> 5, pl = (threadIdx.x >> 6) * 32 + (lane & 31);
  const long long p = p0 + pl;
  if (p >= M) return;
  const UpPixel px = up_pixel(p, H, W);
  float m[2][9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const f32x2 w = *reinterpret_cast<const f32x2*>(rows + pl * 36 + k * 4 + sy * 2);
    m[0][k] = w[0];
    m[1][k] = w[1];
  }
  finish(m, flow, px.b * ((long long)H * W), px, sy, out, H, W);
}

__global__ __launch_bounds__(256) void layout_c(const float* __restrict__ flow, const float* __restrict__ mask, int mask_ld,
                                                float* __restrict__ out, long long M, int H, int W) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63, s = lane >> 4;      // lanes 0..15: (sy, sx) = (0, 0) of 16 pixels, 16..31: (0, 1), ...
  const long long p = (t >> 6) * 16 + (lane & 15);
  if (p >= M) return;
  const UpPixel px = up_pixel(p, H, W);
  const long long img = px.b * ((long long)H * W);
  const float* mrow = mask + p * mask_ld + s;
  float m[9], vx[9], vy[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) m[k] = mrow[k * 4];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    float f[2];
    up_tap<0, 2>(k, flow, 0, nullptr, 0, 0, img, px.y, px.x, H, W, f);
    vx[k] = f[0];
    vy[k] = f[1];
  }
  up_softmax9(m);
  const long long HW4 = (long long)H * W * 4;
  const long long at = up_out_offset<2>(px.y, px.x, s >> 1, s & 1, W);
  out[(px.b * 2 + 0) * HW4 + at] = up_combine(m, vx);
  out[(px.b * 2 + 1) * HW4 + at] = up_combine(m, vy);
}

typedef void (*kern_t)(const float*, const float*, int, float*, long long, int, int);

static void launch(int which, int block, const float* flow, const float* mask, float* out, long long M, int H, int W) {
  if (which == 1) {
    hipLaunchKernelGGL(layout_b, dim3((unsigned)((M + 127) / 128)), dim3(256), 0, 0, flow, mask, 36, out, M, H, W);
    return;
  }
  const int per_wave = which == 0 ? 32 : 16;
  const long long waves = (M + per_wave - 1) / per_wave, wpb = block / 64;
  hipLaunchKernelGGL(which == 0 ? layout_a : layout_c, dim3((unsigned)((waves + wpb - 1) / wpb)), dim3(block), 0, 0, flow, mask, 36, out, M, H,
                     W);
}

int main() {
  const int grids[4][2] = {{28, 64}, {56, 128}, {112, 256}, {224, 512}};
  // (layout, block size)
  const int variants[5][2] = {{0, 64}, {0, 256}, {1, 256}, {2, 64}, {2, 256}};
  const char* names[5] = {"A block 64", "A block 256", "B (LDS) 256", "C block 64", "C block 256"};
  printf("| grid | %s | %s | %s | %s | %s |\n", names[0], names[1], names[2], names[3], names[4]);
  for (int B : {1, 8}) {
    for (const auto& g : grids) {
      const int H = g[0], W = g[1];
      const long long M = (long long)B * H * W;
      std::vector<float> hf(M * 2), hm(M * 36);
      srand(7);
      for (auto& x : hf) x = (rand() / (float)RAND_MAX - 0.5f) * 12.f;
      for (auto& x : hm) x = (rand() / (float)RAND_MAX - 0.5f) * 6.f;
      float *flow, *mask, *out[5];
      CK(hipMalloc(&flow, hf.size() * 4));
      CK(hipMalloc(&mask, hm.size() * 4));
      CK(hipMemcpy(flow, hf.data(), hf.size() * 4, hipMemcpyHostToDevice));
      CK(hipMemcpy(mask, hm.data(), hm.size() * 4, hipMemcpyHostToDevice));
      std::vector<std::vector<float>> host(5, std::vector<float>(M * 8));
      for (int v = 0; v < 5; ++v) {
        CK(hipMalloc(&out[v], M * 8 * 4));
        CK(hipMemset(out[v], 0xff, M * 8 * 4));
        launch(variants[v][0], variants[v][1], flow, mask, out[v], M, H, W);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(host[v].data(), out[v], M * 8 * 4, hipMemcpyDeviceToHost));
        if (memcmp(host[v].data(), host[0].data(), M * 8 * 4) != 0) {
          printf("variant %s differs from A at %dx%dx%d\n", names[v], B, H, W);
          return 1;
        }
      }
      hipEvent_t e0, e1;
      CK(hipEventCreate(&e0));
      CK(hipEventCreate(&e1));
      std::vector<std::vector<float>> ts(5);
      const int reps = 50;
      for (int round = 0; round < 10; ++round) {      // round 0 warms up; the variants alternate
        for (int v = 0; v < 5; ++v) {
          CK(hipEventRecord(e0, 0));
          for (int r = 0; r < reps; ++r) launch(variants[v][0], variants[v][1], flow, mask, out[v], M, H, W);
          CK(hipEventRecord(e1, 0));
          CK(hipEventSynchronize(e1));
          float ms;
          CK(hipEventElapsedTime(&ms, e0, e1));
          if (round) ts[v].push_back(ms * 1e3f / reps);
        }
      }
      printf("| %dx%dx%d |", B, H, W);
      for (int v = 0; v < 5; ++v) {
        std::sort(ts[v].begin(), ts[v].end());
        printf(" %.2f [%.2f] |", ts[v][ts[v].size() / 2], ts[v].back() - ts[v].front());
      }
      printf("\n");
      fflush(stdout);
      CK(hipFree(flow));
      CK(hipFree(mask));
      for (int v = 0; v < 5; ++v) CK(hipFree(out[v]));
    }
  }
  return 0;
}
