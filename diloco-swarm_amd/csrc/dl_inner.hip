// The inner AdamW step (src/train.py:257, inner_optimizer.step(), every training step, right
// after clip_grad_norm_ at :255) as one fused pass over the inner model's own tensors:
//   dl_adamw_step  InnerAdamW: g' = g * *coef (coef given: one rounded fp32 multiply), then
//                  adam1(g', m, v, θ) of dl_device.h -- one element of torch's
//                  _single_tensor_adamw. Reads g, θ, m, v and writes θ, m, v once: 28 B/param,
//                  where torch's _multi_tensor_adam makes nine foreach passes (about 92).
// θ is the bound parameter slot, stepped in place (per-tensor storage); g the bound gradient
// slot, only read; m and v are packed arenas in the tree's layout. Every other AdamW kernel
// (dl_adamw.hip) steps a θ that lives in a packed arena.
// The body has OuterStep's shape (dl_outer_step.h): every 16-B load up front, the arithmetic
// with none on rows past the chunk, then the stores one stream at a time (θ, m, v); the < 4
// elements past the last float4 go one per lane; a chunk whose θ or g is only 4-B aligned goes
// element-wise through the same arithmetic, so results never depend on alignment. The arenas'
// padding is never written. coef (dl_norm_finish's out2 + 1, may be null) is read
// wave-uniformly as ScaleBy reads it; there is no == 1 branch: x * 1 is x for every x.
// Pure streaming: no LDS, no cross-lane work. Four float4[kUnroll] arrays are live per lane
// (g, θ, m, v: 64 VGPRs). Compiler's report (make asm, profiles/inner_adamw_resource_usage.txt):
// 89 VGPRs without coef, 91 with it; 5 waves per SIMD; scratch 0, no spills, no LDS --
// dl_unpack_adamw's footprint (90 to 96 VGPRs, 5 waves).
#include "dl_device.h"

namespace dl {
namespace {

template <bool kCoef>
struct InnerAdamW {
  int param_slot, grad_slot;
  float* m1;          // exp_avg, packed
  float* m2;          // exp_avg_sq, packed
  const float* coef;  // device memory, kCoef only: a wave-uniform load
  AdamArgs a;

  __device__ __forceinline__ void apply(float g, float k, float& m, float& v, float& th) const {
    if constexpr (kCoef) g = g * k;  // contract off: rounded before adam1 sees it
    adam1(g, m, v, th, a);
  }
  __device__ __forceinline__ void apply4(const float4& g, float k, float4& m, float4& v,
                                         float4& th) const {
    apply(g.x, k, m.x, v.x, th.x);
    apply(g.y, k, m.y, v.y, th.y);
    apply(g.z, k, m.z, v.z, th.z);
    apply(g.w, k, m.w, v.w, th.w);
  }

  template <bool NTL, int NTS>
  __device__ __forceinline__ void run(const Chunk& ck, int c, void* const* caddr, int nchunk, int tid) const {
    float* th = slot_ptr<float>(caddr, nchunk, param_slot, c);
    const float* g = slot_ptr<const float>(caddr, nchunk, grad_slot, c);
    float* p1 = m1 + ck.poff;  // packed: always 16-B aligned
    float* p2 = m2 + ck.poff;
    float k = 1.0f;
    if constexpr (kCoef) k = *coef;

    auto one = [&](int i) {
      float t = th[i], e1 = p1[i], e2 = p2[i];
      apply(g[i], k, e1, e2, t);
      th[i] = t;
      p1[i] = e1;
      p2[i] = e2;
    };

    if (aligned16(th) && aligned16(g)) {
      const int nv = ck.len >> 2;
      float4 x[kUnroll], t[kUnroll], m[kUnroll], v2[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int v = u * kThreads + tid;
        if (v < nv) {
          x[u] = ldf4<NTL>(g, v);
          t[u] = ldf4<NTL>(th, v);
          m[u] = ldf4<NTL>(p1, v);
          v2[u] = ldf4<NTL>(p2, v);
        }
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        // rows past the chunk hold no data: no sqrt / division (AdamRule::kSkipPastChunk)
        if (u * kThreads + tid < nv) apply4(x[u], k, m[u], v2[u], t[u]);
      }
      store_rows<NTS>(th, t, nv, tid);
      store_rows<NTS>(p1, m, nv, tid);
      store_rows<NTS>(p2, v2, nv, tid);
      const int i = (nv << 2) + tid;
      if (i < ck.len) one(i);
    } else {
      for (int i = tid; i < ck.len; i += kThreads) one(i);
    }
  }
};

}  // namespace

hipError_t launch_adamw_step(const Launch& L, int param_slot, int grad_slot, float* m1, float* m2,
                             const float* coef, AdamArgs a) {
  if (coef) return run(L, InnerAdamW<true>{param_slot, grad_slot, m1, m2, coef, a});
  return run(L, InnerAdamW<false>{param_slot, grad_slot, m1, m2, nullptr, a});
}

}  // namespace dl
