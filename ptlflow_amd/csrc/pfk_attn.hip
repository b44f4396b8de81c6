// Training of GMA's attention (gma/gma_utils.py:50-78, 100-113): the two kernels around the GEMMs.
//  * pfk_softmax_rows_bwd_{f32,bf16}: backward of pfk_softmax_rows_f32, one block per row, the row sum in a fixed order.
//  * pfk_transpose_pack_{f32,b16}:    the attention map's transposed copy (the A operand of dV = P^T dAgg) and, in the same pass,
//                                     its untransposed packed copy, fp32 bits or bf16 (round to nearest even), pad columns zero.
// Both are bandwidth bound and run once per training step.
#include "pfk_launch.h"

namespace {

// An explicit bit rule, not the (__bf16) cast of store_row: its NaN handling is part of the contract.
// round to nearest even on the bits (what torch's Tensor.to(bfloat16) does); NaN stays a quiet NaN, denormals stay denormals
__device__ __forceinline__ unsigned f32_to_bf16_bits(float f) {
  const unsigned u = __builtin_bit_cast(unsigned, f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// dS[r][j] = P[r][j] * (dP[r][j] - sum_k dP[r][k] P[r][k]),  j < cols;  dS[r][j] = 0,  cols <= j < ld_out.
// One 256-thread block per row, two passes (the row stays in L2 between them).  Every thread adds its columns in ascending
// order, the 64 lanes of a wave meet in a butterfly and the four waves' partials are added in one fixed order: the same bits
// on every run.  dS may be dP itself (fp32): a thread writes only the columns it has read, after the barrier of pass 1.
// BF16: dP holds bf16 rows (4-byte aligned pairs: ld_dp even), read two columns at a time.
template <bool BF16>
__global__ __launch_bounds__(256) void softmax_rows_bwd_kernel(const float* p, long long ld_p, const void* dp_, long long ld_dp,
                                                               float* ds, long long ld_out, int cols, int cols_out) {
  __shared__ float red[4];
  const float* prow = p + (long long)blockIdx.x * ld_p;
  float* orow = ds + (long long)blockIdx.x * ld_out;
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  float sum = 0.f;
  if constexpr (BF16) {
    const unsigned* drow = reinterpret_cast<const unsigned*>(static_cast<const unsigned short*>(dp_) + (long long)blockIdx.x * ld_dp);
    for (int c = 2 * t; c < cols; c += 512) {
      const f32x2 d = widen2(drow[c >> 1]);
      sum += d.x * prow[c];
      if (c + 1 < cols) sum += d.y * prow[c + 1];
    }
  } else {
    const float* drow = static_cast<const float*>(dp_) + (long long)blockIdx.x * ld_dp;
    for (int c = t; c < cols; c += 256) sum += drow[c] * prow[c];
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) sum += __shfl_xor(sum, s, 64);      // wave_sum written out: the call moves the LDS address computation
  if (lane == 0) red[wid] = sum;
  __syncthreads();
  sum = (red[0] + red[1]) + (red[2] + red[3]);
  if constexpr (BF16) {
    const unsigned* drow = reinterpret_cast<const unsigned*>(static_cast<const unsigned short*>(dp_) + (long long)blockIdx.x * ld_dp);
    for (int c = 2 * t; c < cols; c += 512) {
      const f32x2 d = widen2(drow[c >> 1]);
      orow[c] = prow[c] * (d.x - sum);
      if (c + 1 < cols) orow[c + 1] = prow[c + 1] * (d.y - sum);
    }
  } else {
    const float* drow = static_cast<const float*>(dp_) + (long long)blockIdx.x * ld_dp;
    for (int c = t; c < cols; c += 256) orow[c] = prow[c] * (drow[c] - sum);
  }
  for (int c = cols + t; c < cols_out; c += 256) orow[c] = 0.f;
}

// One 64 x 64 tile of one batch element through LDS: rows of `in` are read along their columns (coalesced), the transposed tile
// is written along the rows of `outT` (coalesced).  The tile's leading dimension is 65 floats: the column read `tile[lane][j]`
// then falls on 32 different banks per half-wave (ds_read_b32 banks: dword address % 32), like the row write.
// grid.x covers the N input columns (rows of outT), grid.y covers [0, ld_out): where the input has no element (row or column >= N)
// the tile holds zeros, which is what the pad columns of outT receive, and those of `out` that lie inside the last x tile; the
// blocks of the last x tile also zero whatever pad columns of `out` lie past it.
// BF16: a lane converts two neighbouring columns and stores them as one dword (a half-wave per output row; the paired column
// reads `tile[2l][j]`, `tile[2l + 1][j]` are two-way conflicts, lanes l and l + 16, in a kernel bound by its global traffic).
constexpr int TP = 64;

template <bool BF16>
__global__ __launch_bounds__(256) void transpose_pack_kernel(const float* __restrict__ in, long long ld_in, long long in_bs,
                                                             void* __restrict__ outT_, void* __restrict__ out_, long long ld_out,
                                                             long long out_bs, int N, int cols_out) {
  __shared__ float tile[TP][TP + 1];
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int r0 = blockIdx.x * TP;      // input columns = rows of outT
  const int c0 = blockIdx.y * TP;      // input rows    = columns of outT
  const float* src = in + (long long)blockIdx.z * in_bs;
  for (int j = wid; j < TP; j += 4) {
    const int row = c0 + j, col = r0 + lane;
    tile[j][lane] = (row < N && col < N) ? src[(long long)row * ld_in + col] : 0.f;
  }
  __syncthreads();
  if constexpr (BF16) {
    unsigned short* outT = static_cast<unsigned short*>(outT_) + (long long)blockIdx.z * out_bs;
    unsigned short* out = out_ ? static_cast<unsigned short*>(out_) + (long long)blockIdx.z * out_bs : nullptr;
    const int half = lane >> 5, l2 = (lane & 31) * 2;      // ld_out and the tile origin are even: a pair never straddles cols_out
    if (out && blockIdx.x == gridDim.x - 1)
      for (int j = wid; j < TP && c0 + j < N; j += 4)
        for (int c = gridDim.x * TP + lane; c < cols_out; c += 64) out[(long long)(c0 + j) * ld_out + c] = 0;
    for (int j = 2 * wid + half; j < TP; j += 8) {
      if (r0 + j < N && c0 + l2 < cols_out) {
        const unsigned w = f32_to_bf16_bits(tile[l2][j]) | (f32_to_bf16_bits(tile[l2 + 1][j]) << 16);
        *reinterpret_cast<unsigned*>(outT + (long long)(r0 + j) * ld_out + c0 + l2) = w;
      }
      if (out && c0 + j < N && r0 + l2 < cols_out) {
        const unsigned w = f32_to_bf16_bits(tile[j][l2]) | (f32_to_bf16_bits(tile[j][l2 + 1]) << 16);
        *reinterpret_cast<unsigned*>(out + (long long)(c0 + j) * ld_out + r0 + l2) = w;
      }
    }
  } else {
    float* outT = static_cast<float*>(outT_) + (long long)blockIdx.z * out_bs;
    float* out = out_ ? static_cast<float*>(out_) + (long long)blockIdx.z * out_bs : nullptr;
    if (out && blockIdx.x == gridDim.x - 1)
      for (int j = wid; j < TP && c0 + j < N; j += 4)
        for (int c = gridDim.x * TP + lane; c < cols_out; c += 64) out[(long long)(c0 + j) * ld_out + c] = 0.f;
    for (int j = wid; j < TP; j += 4) {
      if (r0 + j < N && c0 + lane < cols_out) outT[(long long)(r0 + j) * ld_out + c0 + lane] = tile[lane][j];
      if (out && c0 + j < N && r0 + lane < cols_out) out[(long long)(c0 + j) * ld_out + r0 + lane] = tile[j][lane];
    }
  }
}

int softmax_rows_bwd_launch(bool bf16, const float* p, long long ld_p, const void* dp, long long ld_dp, float* ds, long long ld_out,
                            long long rows, int cols, pfk_stream_t stream) {
  if (!p || !dp || !ds || rows <= 0 || cols <= 0 || !pfk_fits_int(rows)) return PFK_ERR_BAD_ARG;
  if (ld_p < cols || ld_dp < cols || ld_out < cols || !pfk_fits_int(ld_out)) return PFK_ERR_BAD_ARG;
  if (static_cast<const void*>(ds) == dp && (bf16 || ld_out != ld_dp)) return PFK_ERR_BAD_ARG;      // in place: fp32, same rows
  if (bf16 && (!pfk_aligned16(dp) || (ld_dp & 7))) return PFK_ERR_ALIGNMENT;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (bf16)
    hipLaunchKernelGGL(softmax_rows_bwd_kernel<true>, dim3((unsigned)rows), dim3(256), 0, st, p, ld_p, dp, ld_dp, ds, ld_out, cols, (int)ld_out);
  else
    hipLaunchKernelGGL(softmax_rows_bwd_kernel<false>, dim3((unsigned)rows), dim3(256), 0, st, p, ld_p, dp, ld_dp, ds, ld_out, cols, (int)ld_out);
  return pfk_launch_status();
}

int transpose_pack_launch(bool bf16, const float* in, long long ld_in, void* outT, void* out, long long ld_out, int B, int N,
                          pfk_stream_t stream) {
  if (!in || !outT || B <= 0 || N <= 0 || ld_in < N || ld_out < N || !pfk_fits_int(ld_out)) return PFK_ERR_BAD_ARG;
  if (in == outT || in == out || outT == out) return PFK_ERR_BAD_ARG;
  if (bf16 && (!pfk_aligned16(outT) || (out && !pfk_aligned16(out)) || (ld_out & 7))) return PFK_ERR_ALIGNMENT;
  const long long tiles = (ld_out + TP - 1) / TP;
  if (tiles > 65535 || B > 65535) return PFK_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)((N + TP - 1) / TP), (unsigned)tiles, (unsigned)B);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long long in_bs = (long long)N * ld_in, out_bs = (long long)N * ld_out;
  if (bf16)
    hipLaunchKernelGGL(transpose_pack_kernel<true>, grid, dim3(256), 0, st, in, ld_in, in_bs, outT, out, ld_out, out_bs, N, (int)ld_out);
  else
    hipLaunchKernelGGL(transpose_pack_kernel<false>, grid, dim3(256), 0, st, in, ld_in, in_bs, outT, out, ld_out, out_bs, N, (int)ld_out);
  return pfk_launch_status();
}

}  // namespace

extern "C" {

int pfk_softmax_rows_bwd_f32(const float* p, long long ld_p, const float* dp, long long ld_dp, float* ds, long long ld_out,
                             long long rows, int cols, pfk_stream_t stream) {
  return softmax_rows_bwd_launch(false, p, ld_p, dp, ld_dp, ds, ld_out, rows, cols, stream);
}

int pfk_softmax_rows_bwd_bf16(const float* p, long long ld_p, const void* dp_bf16, long long ld_dp, float* ds, long long ld_out,
                              long long rows, int cols, pfk_stream_t stream) {
  return softmax_rows_bwd_launch(true, p, ld_p, dp_bf16, ld_dp, ds, ld_out, rows, cols, stream);
}

int pfk_transpose_pack_f32(const float* in, long long ld_in, float* outT, float* out, long long ld_out, int B, int N,
                           pfk_stream_t stream) {
  return transpose_pack_launch(false, in, ld_in, outT, out, ld_out, B, N, stream);
}

int pfk_transpose_pack_b16(const float* in, long long ld_in, void* outT_bf16, void* out_bf16, long long ld_out, int B, int N,
                           pfk_stream_t stream) {
  return transpose_pack_launch(true, in, ld_in, outT_bf16, out_bf16, ld_out, B, N, stream);
}

}  // extern "C"
