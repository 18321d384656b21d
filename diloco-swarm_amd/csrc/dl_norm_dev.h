// Device-side pieces of the gradient-norm sum shared by the kernels that leave per-chunk Σ g²
// partials (dl_norm.hip; dl_q8_grad.hip's decoder). The summation order is stated in dl_norm.hip
// and restated in tests/clip_restatement.py.
#pragma once
#include "dl_device.h"

namespace dl {
namespace {

__device__ __forceinline__ void sq1(double& acc, float g) { acc += double(g) * double(g); }
__device__ __forceinline__ void sq4(double& acc, const float4& x) {
  sq1(acc, x.x);
  sq1(acc, x.y);
  sq1(acc, x.z);
  sq1(acc, x.w);
}

// Σ over the workgroup's 256 lanes in dl_norm.hip's fixed order; the result is valid in lane 0
__device__ __forceinline__ double block_sum(double v, int tid) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);  // 64-lane wave
  __shared__ double part[kThreads / 64];
  if ((tid & 63) == 0) part[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) v = ((part[0] + part[1]) + part[2]) + part[3];
  __syncthreads();  // `part` is reused by the workgroup's next chunk
  return v;
}

__device__ __forceinline__ double sumsq_rows(const float4 (&x)[kUnroll], int nv, int tid) {
  double acc = 0.0;
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) {
    const int v = u * kThreads + tid;
    if (v < nv) sq4(acc, x[u]);
  }
  return acc;
}

}  // namespace
}  // namespace dl
