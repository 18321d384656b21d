// The AdamW outer step (src/utils.py:60-61, configs/optimizer/adamw.toml, stepped at
// src/train.py:267) as one fused pass per chunk, on the segment walker of dl_device.h.
//
// One element of torch's _single_tensor_adamw (adam1, dl_device.h), every operation rounded on
// its own except the two explicit fmas; the host hands in the scalars narrowed to fp32 once:
//   g   = wire / divisor               (IEEE division; divisor 1: untouched)
//   θ   = θ * decay                    (decay = 1 - lr*wd)
//   m   = fma(w1, g - m, m)            (exp_avg.lerp_(g, 1 - β1), β1 > 0.5)
//   v   = v * β2; v = fma(w2 * g, g, v)  (exp_avg_sq.mul_(β2).addcmul_(g, g, value=1 - β2))
//   den = sqrt(v) / bs + eps           (bs = sqrt(1 - β2^t); correctly rounded sqrt, division)
//   θ   = θ + (nss * m) / den          (nss = -(lr / (1 - β1^t)); addcdiv_)
// A zero state (m = v = 0) is the first step: there is no separate first-step body.
//   dl_unpack_adamw      N > 1: reads the summed wire, θ, m, v; writes θ, m, v (+ inner):
//                        28 B/param + 4 for the inner write (fp32 wire)
//   dl_delta_pack_adamw  one peer: g = θ - inner, the wire written as dl_delta_pack writes it;
//                        16 B read + 20 B written per param (fp32 wire)
// Pure streaming: no LDS, no cross-lane work. Four float4[kUnroll] arrays are live per lane
// (g, θ, m, v: 64 VGPRs), so the kernels stay far from spilling (make asm prints the report).
#include "dl_device.h"

namespace dl {
namespace {

__device__ __forceinline__ void adam4(const float4& g, float4& m, float4& v, float4& t,
                                      const AdamArgs& a) {
  adam1(g.x, m.x, v.x, t.x, a);
  adam1(g.y, m.y, v.y, t.y, a);
  adam1(g.z, m.z, v.z, t.z, a);
  adam1(g.w, m.w, v.w, t.w, a);
}

template <typename W, bool DIV>
struct UnpackAdamW {
  const W* wire;
  float* outer;
  float* m1;  // exp_avg
  float* m2;  // exp_avg_sq
  float d;
  AdamArgs a;
  int inner_slot;
  __device__ __forceinline__ void one(const W* w, float* th, float* mb, float* vb, float* in,
                                      int i) const {
    float g = WireIO<W>::ld1(w, i);
    if (DIV) g = g / d;
    float m = mb[i], v = vb[i], t = th[i];
    adam1(g, m, v, t, a);
    th[i] = t;
    mb[i] = m;
    vb[i] = v;
    if (in) in[i] = t;
  }
  template <bool NTL, int NTS>
  __device__ __forceinline__ void run(const Chunk& ck, int c, void* const* caddr, int nchunk, int tid) const {
    float* in = inner_slot >= 0 ? slot_ptr<float>(caddr, nchunk, inner_slot, c) : nullptr;
    const W* w = wire + ck.poff;
    float* th = outer + ck.poff;
    float* mb = m1 + ck.poff;
    float* vb = m2 + ck.poff;
    if (in == nullptr || aligned16(in)) {
      const int nv = ck.len >> 2;
      float4 g[kUnroll], t[kUnroll], m[kUnroll], v[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int k = u * kThreads + tid;
        if (k < nv) {
          g[u] = WireIO<W>::template ld4<NTL>(w, k);
          t[u] = ldf4<NTL>(th, k);
          m[u] = ldf4<NTL>(mb, k);
          v[u] = ldf4<NTL>(vb, k);
        }
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        if (u * kThreads + tid < nv)  // rows past the chunk hold no data: no sqrt / division
          adam4(DIV ? div4(g[u], d) : g[u], m[u], v[u], t[u], a);
      }
      store_rows<NTS>(th, t, nv, tid);
      store_rows<NTS>(mb, m, nv, tid);
      store_rows<NTS>(vb, v, nv, tid);
      if (in) store_rows<NTS>(in, t, nv, tid);
      const int i = (nv << 2) + tid;
      if (i < ck.len) one(w, th, mb, vb, in, i);
    } else {
      for (int i = tid; i < ck.len; i += kThreads) one(w, th, mb, vb, in, i);
    }
  }
};

// One peer (src/comm.py:118-119: no all-reduce, no division), the pseudo-gradient kept on the
// wire as dl_delta_pack_sgd keeps it: a bf16 wire rounds g first and AdamW steps on the rounded
// value, as dl_unpack_adamw would read it back. Bit-identical to dl_delta_pack followed by
// dl_unpack_adamw with divisor 1, wire included.
template <typename W>
struct DeltaPackAdamW {
  float* outer;
  W* wire;
  float* m1;
  float* m2;
  AdamArgs a;
  int inner_slot;
  static __device__ __forceinline__ float on_wire(float g) {
    if constexpr (sizeof(W) == 2) return bf2f(f2bf(g));
    else return g;
  }
  __device__ __forceinline__ void one(W* w, float* th, float* mb, float* vb, float* in,
                                      int i) const {
    float t = th[i];
    const float g0 = t - in[i];
    WireIO<W>::st1(w, i, g0);
    float m = mb[i], v = vb[i];
    adam1(on_wire(g0), m, v, t, a);
    th[i] = t;
    mb[i] = m;
    vb[i] = v;
    in[i] = t;
  }
  template <bool NTL, int NTS>
  __device__ __forceinline__ void run(const Chunk& ck, int c, void* const* caddr, int nchunk, int tid) const {
    float* in = slot_ptr<float>(caddr, nchunk, inner_slot, c);
    float* th = outer + ck.poff;
    float* mb = m1 + ck.poff;
    float* vb = m2 + ck.poff;
    W* w = wire + ck.poff;
    if (aligned16(in)) {
      const int nv = ck.len >> 2;
      float4 x[kUnroll], t[kUnroll], m[kUnroll], v[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int k = u * kThreads + tid;
        if (k < nv) {
          t[u] = ldf4<NTL>(th, k);
          x[u] = ldf4<NTL>(in, k);
          m[u] = ldf4<NTL>(mb, k);
          v[u] = ldf4<NTL>(vb, k);
        }
      }
      // the wire rows leave first (their values are ready after one subtract), then the
      // arithmetic, then θ, exp_avg, exp_avg_sq and inner, each stream's rows back to back
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int k = u * kThreads + tid;
        if (k < nv) {
          x[u] = sub4(t[u], x[u]);  // the pseudo-gradient
          WireIO<W>::template st4<NTS>(w, k, x[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        if (u * kThreads + tid < nv) {
          const float4 g = make_float4(on_wire(x[u].x), on_wire(x[u].y), on_wire(x[u].z),
                                       on_wire(x[u].w));
          adam4(g, m[u], v[u], t[u], a);
        }
      }
      store_rows<NTS>(th, t, nv, tid);
      store_rows<NTS>(mb, m, nv, tid);
      store_rows<NTS>(vb, v, nv, tid);
      store_rows<NTS>(in, t, nv, tid);
      const int i = (nv << 2) + tid;
      if (i < ck.len) one(w, th, mb, vb, in, i);
    } else {
      for (int i = tid; i < ck.len; i += kThreads) one(w, th, mb, vb, in, i);
    }
  }
};

template <typename W>
hipError_t unpack_adamw_t(const Launch& L, const W* w, int divisor, float* outer, float* m1,
                          float* m2, AdamArgs a, int inner_slot) {
  const float d = float(divisor);
  if (divisor == 1) return run(L, UnpackAdamW<W, false>{w, outer, m1, m2, d, a, inner_slot});
  return run(L, UnpackAdamW<W, true>{w, outer, m1, m2, d, a, inner_slot});
}

}  // namespace

hipError_t launch_unpack_adamw(const Launch& L, const void* wire, int wire_dtype, int divisor,
                               float* outer, float* m1, float* m2, AdamArgs a, int inner_slot) {
  if (wire_dtype == DL_BF16)
    return unpack_adamw_t(L, static_cast<const bf16_t*>(wire), divisor, outer, m1, m2, a,
                          inner_slot);
  return unpack_adamw_t(L, static_cast<const float*>(wire), divisor, outer, m1, m2, a, inner_slot);
}

hipError_t launch_delta_pack_adamw(const Launch& L, int inner_slot, float* outer, void* wire,
                                   int wire_dtype, float* m1, float* m2, AdamArgs a) {
  if (wire_dtype == DL_BF16)
    return run(L, DeltaPackAdamW<bf16_t>{outer, static_cast<bf16_t*>(wire), m1, m2, a, inner_slot});
  return run(L, DeltaPackAdamW<float>{outer, static_cast<float*>(wire), m1, m2, a, inner_slot});
}

}  // namespace dl
