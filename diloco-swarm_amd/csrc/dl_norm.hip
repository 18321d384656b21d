// Gradient-norm clipping on device gradients: torch.nn.utils.clip_grad_norm_(params, max_norm)
// with norm_type 2 (src/train.py:255, every step, right after sync_gradients at :251) as walker
// passes over the bound gradient slot:
//   dl_grad_sumsq        SumSq: partials[c] = Σ g² over chunk c; one read, 4 B/param
//   dl_unpack_avg_sumsq  UnpackAvgSumSq: dl_unpack_avg that also leaves partials[c] of the values
//                        it stores -- on a sync step the norm costs no traffic of its own
//   dl_norm_finish       k_norm_finish: norm = sqrt(Σ partials), coef = clamp(max_norm/(norm+1e-6))
//   dl_scale_by          ScaleBy: g *= coef, or nothing at all when coef == 1 (no step clips
//                        once warm-up is over: that step reads 4 B/param and writes none)
//
// Summation order (restated in numpy by tests/clip_restatement.py; bit-exact contract). All sums
// are fp64; the square of an fp32 value is exact in fp64, so no fma needs emulating.
//   lane:      acc = 0; for u = 0..3, for x, y, z, w of float4 v = u*256 + tid of the chunk:
//              acc += double(g)*double(g); then the tail element 4*(len>>2) + tid. A tensor
//              that is not 16-B aligned takes the same elements with scalar loads, so the norm
//              depends on the values and the tensor sizes, never on addresses.
//   wave:      xor-butterfly, o = 32, 16, .., 1: v += shfl_xor(v, o)
//   workgroup: the four waves' sums through LDS, ((w0 + w1) + w2) + w3, by lane 0 -> partials[c]
//   finish:    one workgroup; lane t sums partials[t], partials[t + 256], ..; the same butterfly
//              and four-wave sum; sqrt in fp64; norm = float(sqrt)
// partials[c] is indexed by the tree's global chunk index and a chunk is summed by exactly one
// workgroup, so the result does not depend on the grid (dl_tree_tune) or on the bucket split.
// One deliberate difference from torch: torch accumulates in fp32 and overflows to inf at
// |g| >~ 1.8e19; the fp64 sum does not (1e25 has a finite norm here).
// No MFMA, no scratch; 32 B of LDS (profiles/clip_norm_resource_usage.txt).
#include "dl_device.h"
#include "dl_norm_dev.h"

namespace dl {
namespace {

// the float4 rows of a chunk a lane owns, from a tensor that may be only 4-B aligned
template <bool NTL>
__device__ __forceinline__ void load_rows(const float* src, int nv, int tid, float4 (&x)[kUnroll]) {
  if (aligned16(src)) {
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int v = u * kThreads + tid;
      if (v < nv) x[u] = ldf4<NTL>(src, v);
    }
  } else {
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int v = u * kThreads + tid;
      if (v < nv) x[u] = make_float4(src[4 * v], src[4 * v + 1], src[4 * v + 2], src[4 * v + 3]);
    }
  }
}

struct SumSq {
  int src_slot;
  double* partials;
  template <bool NTL, int NTS>
  __device__ __forceinline__ void run(const Chunk& ck, int c, void* const* caddr, int nchunk, int tid) const {
    const float* src = slot_ptr<const float>(caddr, nchunk, src_slot, c);
    const int nv = ck.len >> 2;
    float4 x[kUnroll];
    load_rows<NTL>(src, nv, tid, x);
    double acc = sumsq_rows(x, nv, tid);
    const int i = (nv << 2) + tid;
    if (i < ck.len) sq1(acc, src[i]);
    acc = block_sum(acc, tid);
    if (tid == 0) partials[c] = acc;
  }
};

// dl_unpack_avg (UnpackAvg, dl_kernels.hip: the same bytes stored) + SumSq over the stored values
template <typename W, bool DIV>
struct UnpackAvgSumSq {
  const W* wire;
  int dst_slot;
  float* dst_packed;
  float d;
  double* partials;
  template <bool NTL, int NTS>
  __device__ __forceinline__ void run(const Chunk& ck, int c, void* const* caddr, int nchunk, int tid) const {
    float* dst = dst_slot >= 0 ? slot_ptr<float>(caddr, nchunk, dst_slot, c) : dst_packed + ck.poff;
    const W* w = wire + ck.poff;  // packed: always 16-B aligned
    const int nv = ck.len >> 2;
    float4 x[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int v = u * kThreads + tid;
      if (v < nv) x[u] = WireIO<W>::template ld4<NTL>(w, v);
    }
    if (DIV) {
#pragma unroll
      for (int u = 0; u < kUnroll; ++u)
        if (u * kThreads + tid < nv) x[u] = div4(x[u], d);
    }
    if (aligned16(dst)) {
      store_rows<NTS>(dst, x, nv, tid);
    } else {
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int v = u * kThreads + tid;
        if (v < nv) {
          dst[4 * v] = x[u].x;
          dst[4 * v + 1] = x[u].y;
          dst[4 * v + 2] = x[u].z;
          dst[4 * v + 3] = x[u].w;
        }
      }
    }
    double acc = sumsq_rows(x, nv, tid);
    const int i = (nv << 2) + tid;
    if (i < ck.len) {
      float g = WireIO<W>::ld1(w, i);
      if (DIV) g = g / d;
      dst[i] = g;
      sq1(acc, g);
    }
    acc = block_sum(acc, tid);
    if (tid == 0) partials[c] = acc;
  }
};

// g *= *coef in place; coef == 1 (nothing to clip): no load, no store. A NaN or zero
// coefficient is not 1 and multiplies, as torch's unconditional _foreach_mul_ does.
struct ScaleBy {
  int slot;
  const float* coef;  // device memory (dl_norm_finish's out2 + 1): a wave-uniform load
  template <bool NTL, int NTS>
  __device__ __forceinline__ void run(const Chunk& ck, int c, void* const* caddr, int nchunk, int tid) const {
    const float k = *coef;
    if (k == 1.0f) return;
    float* g = slot_ptr<float>(caddr, nchunk, slot, c);
    if (aligned16(g)) {
      const int nv = ck.len >> 2;
      float4 x[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int v = u * kThreads + tid;
        if (v < nv) x[u] = ldf4<NTL>(g, v);
      }
      const int i = (nv << 2) + tid;
      float t = 0.f;
      if (i < ck.len) t = g[i];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int v = u * kThreads + tid;
        if (v < nv)
          stf4<NTS>(g, v, make_float4(x[u].x * k, x[u].y * k, x[u].z * k, x[u].w * k));
      }
      if (i < ck.len) g[i] = t * k;
    } else {
      for (int i = tid; i < ck.len; i += kThreads) g[i] = g[i] * k;
    }
  }
};

// norm and clip coefficient from the per-chunk partial sums; out[0] = norm, out[1] = coef.
// The coefficient is torch's own fp32 sequence (torch/nn/utils/clip_grad.py):
//   clip_coef = max_norm / (total_norm + 1e-6)  with a Python float on the left, which torch
//               evaluates as total.add(1e-6).reciprocal().mul(max_norm): two roundings
//   clamp(max=1.0)                              a NaN stays a NaN
__global__ void __launch_bounds__(kThreads)
    k_norm_finish(const double* __restrict__ partials, int32_t n, float max_norm,
                  float* __restrict__ out) {
  const int tid = int(threadIdx.x);
  double acc = 0.0;
  // A lane's partials are added one by one in index order. kFinishLoads of them are loaded
  // ahead of the adds: one load per add leaves the single workgroup waiting a full memory
  // round trip per element (T1.3B has 1,253 per lane).
  constexpr int kFinishLoads = 16;
  int32_t i = tid;
  for (; i < n - (kFinishLoads - 1) * kThreads; i += kFinishLoads * kThreads) {
    double p[kFinishLoads];
#pragma unroll
    for (int j = 0; j < kFinishLoads; ++j) p[j] = partials[i + j * kThreads];
#pragma unroll
    for (int j = 0; j < kFinishLoads; ++j) acc += p[j];
  }
  for (; i < n; i += kThreads) acc += partials[i];
  acc = block_sum(acc, tid);
  if (tid == 0) {
    const float norm = float(__builtin_sqrt(acc));
    const float c = (1.0f / (norm + 1e-6f)) * max_norm;
    out[0] = norm;
    out[1] = c < 1.0f ? c : (c != c ? c : 1.0f);
  }
}

template <typename W>
hipError_t unpack_avg_sumsq_t(const Launch& L, const W* w, int divisor, int dst_slot,
                              float* dst_packed, double* partials) {
  const float d = float(divisor);
  if (divisor == 1) return run(L, UnpackAvgSumSq<W, false>{w, dst_slot, dst_packed, d, partials});
  return run(L, UnpackAvgSumSq<W, true>{w, dst_slot, dst_packed, d, partials});
}

}  // namespace

hipError_t launch_grad_sumsq(const Launch& L, int src_slot, double* partials) {
  return run(L, SumSq{src_slot, partials});
}

hipError_t launch_unpack_avg_sumsq(const Launch& L, const void* wire, int wire_dtype, int divisor,
                                   int dst_slot, float* dst_packed, double* partials) {
  if (wire_dtype == DL_BF16)
    return unpack_avg_sumsq_t(L, static_cast<const bf16_t*>(wire), divisor, dst_slot, dst_packed,
                              partials);
  return unpack_avg_sumsq_t(L, static_cast<const float*>(wire), divisor, dst_slot, dst_packed,
                            partials);
}

hipError_t launch_norm_finish(const double* partials, int32_t n, float max_norm, float* out2,
                              hipStream_t s) {
  hipLaunchKernelGGL(k_norm_finish, dim3(1), dim3(kThreads), 0, s, partials, n, max_norm, out2);
  return hipGetLastError();
}

hipError_t launch_scale_by(const Launch& L, int slot, const float* coef) {
  return run(L, ScaleBy{slot, coef});
}

}  // namespace dl
