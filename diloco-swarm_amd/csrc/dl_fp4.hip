// 4-bit wire codec for the pseudo-gradient exchange: OCP MX block-scaled E2M1 ("MXFP4"), the
// narrow format gfx950 is built around, on the int8 wire's slot plan and exchange.
//
// Wire = one DL_FP4_SLOT_BYTES (2176-B) SLOT per tree chunk: 128 scale bytes E (one per group of
// 32 elements, E8M0: the scale is 2^(E-127)), then 2048 payload bytes, element i in byte
// 128 + i/2, low nibble for even i; a nibble is sign << 3 | code, code indexing
// {0, 0.5, 1, 1.5, 2, 3, 4, 6}. Elements past the chunk's length count as +0. 0.531 B/param.
//   dl_delta_fp4        x = θ - inner (+ r); slot <- enc(x); (r <- x - deq(slot))
//   all_to_all          every peer receives its 1/n of the slots from every peer
//   dl_fp4_reduce       avg = (Σ_r deq_r) / n in rank order (+ r2); re-encoded
//   all_gather          every peer receives every averaged slot (identical on all peers)
//   dl_unpack_sgd_fp4 / dl_unpack_adamw_fp4   g = deq(slot); the rule of dl_unpack_sgd /
//                       dl_unpack_adamw (divisor 1); inner = θ
// Scale of a group: the smallest power of two with amax·2^-e <= 6, so nothing saturates (the
// OCP floor(log2) - 2 rule clamps amax in (6, 8)·2^e); a NaN or Inf anywhere in the group gives
// E = 255 and the group decodes to NaN. Quantiser: nearest grid point, ties to the even code.
// Decoding is an exact multiply by a power of two (dl_fp4_dev.h).
#include "dl_fp4_dev.h"
#include "dl_outer_step.h"

namespace dl {
namespace {

// a2 with the fp4 codec: slot(c) <- enc(θ - inner) over chunk c; EF: x = d + r replaces d and
// r <- x - deq(slot) goes back in place by the lane that read it, nothing of r touched past the
// chunk's length. Every global load is issued before any reduction; a group's amax is three
// shuffles among the 8 lanes of a float4 row (16-B path) or five among 32 lanes (4-B-aligned
// tensor storage). The slot is staged whole in LDS and leaves as 136 16-B stores.
template <bool EF>
struct DeltaFp4 {
  int inner_slot;
  const float* outer;
  uint8_t* slots;  // slot of chunk c at (c - c0) * DL_FP4_SLOT_BYTES
  int c0;
  float* resid;  // EF: the packed residual arena

  static __device__ __forceinline__ float x1(const float* th, const float* in, const float* rs, int i) {
    if constexpr (EF) return (th[i] - in[i]) + rs[i];
    else return th[i] - in[i];
  }

  template <bool NTL, int NTS>
  __device__ __forceinline__ void run(const Chunk& ck, int c, void* const* caddr, int nchunk, int tid) const {
    __shared__ u32x4 stage[kFp4Vec];
    uint8_t* st = reinterpret_cast<uint8_t*>(stage);
    const float* in = slot_ptr<const float>(caddr, nchunk, inner_slot, c);
    const float* th = outer + ck.poff;
    float* rs = EF ? resid + ck.poff : nullptr;
    uint8_t* slot = slots + size_t(c - c0) * DL_FP4_SLOT_BYTES;
    const int nv = ck.len >> 2;
    float4 x[kUnroll];
    if (aligned16(in)) {
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int v = u * kThreads + tid;
        if (v < nv) {
          const float4 d = sub4(ldf4<NTL>(th, v), ldf4<NTL>(in, v));
          if constexpr (EF) x[u] = add4(d, ldf4<NTL>(rs, v));
          else x[u] = d;
        } else {  // the row of the < 4 tail elements stays with its group's lanes; +0 past the length
          float e[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) e[j] = 4 * v + j < ck.len ? x1(th, in, rs, 4 * v + j) : 0.f;
          x[u] = make_float4(e[0], e[1], e[2], e[3]);
        }
      }
      fp4_encode_rows<EF>(x, st, tid);
      if constexpr (EF) {
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          const int v = u * kThreads + tid;
          if (v < nv) {
            stf4<NTS>(rs, v, x[u]);
          } else {
            const float e[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (4 * v + j < ck.len) rs[4 * v + j] = e[j];
          }
        }
      }
    } else {  // element k*256 + tid of the chunk in x[k/4].k%4: a group is 32 consecutive lanes
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        float e[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int i = (4 * u + j) * kThreads + tid;
          e[j] = i < ck.len ? x1(th, in, rs, i) : 0.f;
        }
        x[u] = make_float4(e[0], e[1], e[2], e[3]);
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const float e[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int i = (4 * u + j) * kThreads + tid;
          const uint32_t sc = fp4_scale(group_umax<32>(abs_bits(e[j])));
          const uint32_t nib = fp4_nibble(e[j], fp4_up(sc));
          const uint32_t odd = uint32_t(__shfl_xor(int(nib), 1, 64));
          if ((tid & 1) == 0) st[kFp4Scales + (i >> 1)] = uint8_t(nib | (odd << 4));
          if ((tid & 31) == 0) st[i >> 5] = uint8_t(sc);
          if constexpr (EF) {
            if (i < ck.len) rs[i] = e[j] - fp4_value(nib, fp4_half(sc));
          }
        }
      }
    }
    fp4_store_slot<NTS>(stage, slot, tid);
  }
};

// a4 + a5 from the averaged fp4 slots under either rule (SgdRule<MODE>, AdamRule of
// dl_outer_step.h: the arithmetic of dl_unpack_sgd / dl_unpack_adamw). The slot side is written
// once: the whole slot arrives as 136 non-temporal 16-B loads issued before the loads of θ and
// the state, goes through LDS, and every lane takes its rows' 16 payload bits and scale byte;
// the rule runs on the rows inside the chunk only and the stores leave one stream at a time:
// θ, the state, inner.
template <class Rule>
struct UnpackFp4 {
  static constexpr int K = Rule::kStates;
  const uint8_t* slots;
  int c0;
  float* outer;
  Rule rule;
  int inner_slot;

  template <int J>
  __device__ __forceinline__ void step(float g, float4 (&m)[K][kUnroll], int u, float4& t) const {
    float e[K];
#pragma unroll
    for (int k = 0; k < K; ++k) e[k] = Rule::kLoadState ? comp<J>(m[k][u]) : 0.f;
    rule.apply(g, e, comp<J>(t));
#pragma unroll
    for (int k = 0; k < K; ++k) comp<J>(m[k][u]) = e[k];
  }

  template <bool NTL, int NTS>
  __device__ __forceinline__ void run(const Chunk& ck, int c, void* const* caddr, int nchunk, int tid) const {
    float* in = inner_slot >= 0 ? slot_ptr<float>(caddr, nchunk, inner_slot, c) : nullptr;
    const uint8_t* slot = slots + size_t(c - c0) * DL_FP4_SLOT_BYTES;
    float* th = outer + ck.poff;
    float* sp[K];
#pragma unroll
    for (int k = 0; k < K; ++k) sp[k] = rule.state(k) + ck.poff;
    auto one = [&](int i) {
      const float g = fp4_load1(slot, i);
      float t1 = th[i];
      float e[K];
#pragma unroll
      for (int k = 0; k < K; ++k) e[k] = Rule::kLoadState ? sp[k][i] : 0.f;
      rule.apply(g, e, t1);
      th[i] = t1;
      if (Rule::kStoreState) {
#pragma unroll
        for (int k = 0; k < K; ++k) sp[k][i] = e[k];
      }
      if (in) in[i] = t1;
    };
    if (in == nullptr || aligned16(in)) {
      const int nv = ck.len >> 2;
      float4 t[kUnroll], m[K][kUnroll];
      uint32_t w[kUnroll], sc[kUnroll];
      __shared__ u32x4 stage[kFp4Vec];
      u32x4 qv = {0u, 0u, 0u, 0u};
      if (tid < kFp4Vec) qv = __builtin_nontemporal_load((const DL_GLOBAL u32x4*)slot + tid);
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int v = u * kThreads + tid;
        if (v < nv) {
          t[u] = ldf4<NTL>(th, v);
          if (Rule::kLoadState) {
#pragma unroll
            for (int k = 0; k < K; ++k) m[k][u] = ldf4<NTL>(sp[k], v);
          }
        }
      }
      if (tid < kFp4Vec) stage[tid] = qv;
      __syncthreads();
      const uint8_t* st = reinterpret_cast<const uint8_t*>(stage);
      const uint16_t* st16 = reinterpret_cast<const uint16_t*>(stage);
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int v = u * kThreads + tid;
        w[u] = st16[kFp4Scales / 2 + v];
        sc[u] = st[v >> 3];
      }
      __syncthreads();  // `stage` is reused by the workgroup's next chunk
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        if (u * kThreads + tid < nv) {
          const float4 g = fp4_unpack4(w[u], fp4_half(sc[u]));
          step<0>(g.x, m, u, t[u]);
          step<1>(g.y, m, u, t[u]);
          step<2>(g.z, m, u, t[u]);
          step<3>(g.w, m, u, t[u]);
        }
      }
      store_rows<NTS>(th, t, nv, tid);
      if (Rule::kStoreState) {
#pragma unroll
        for (int k = 0; k < K; ++k) store_rows<NTS>(sp[k], m[k], nv, tid);
      }
      if (in) store_rows<NTS>(in, t, nv, tid);
      const int i = (nv << 2) + tid;
      if (i < ck.len) one(i);
    } else {
      for (int i = tid; i < ck.len; i += kThreads) one(i);
    }
  }
};

// Σ over n peers' copies of m slots (recv laid out [peer][slot]) -> averaged, re-encoded slots;
// one workgroup per slot, lane rows as in the encoder (16 payload bits and one scale byte per
// row and peer). EF: the owner's residual r2 (m · DL_CHUNK_ELEMS floats) is added to the average
// before the encoder and rewritten by the same lane; a zero slot keeps a zero residual.
template <bool EF>
__global__ void __launch_bounds__(kThreads)
    k_fp4_reduce(const uint8_t* recv, int32_t n, int32_t m, int32_t divisor, float* resid,
                 uint8_t* out) {  // recv == out at one peer (in place): no __restrict__
  const int j = blockIdx.x;
  const int tid = threadIdx.x;
  float* rs = EF ? resid + size_t(j) * DL_CHUNK_ELEMS : nullptr;
  float4 acc[kUnroll], r2[kUnroll];
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) {
    acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (EF) r2[u] = ldf4<true>(rs, u * kThreads + tid);
  }
  for (int r = 0; r < n; ++r) {  // rank order: the sum is identical on every peer
    const uint8_t* slot = recv + (size_t(r) * m + j) * DL_FP4_SLOT_BYTES;
    const DL_GLOBAL uint16_t* q = (const DL_GLOBAL uint16_t*)(slot + kFp4Scales);
    const DL_GLOBAL uint8_t* sc = (const DL_GLOBAL uint8_t*)slot;
    uint32_t w[kUnroll], e[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int v = u * kThreads + tid;
      w[u] = q[v];
      e[u] = sc[v >> 3];
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) acc[u] = add4(acc[u], fp4_unpack4(w[u], fp4_half(e[u])));
  }
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) {
    if (divisor > 1) acc[u] = div4(acc[u], float(divisor));
    if constexpr (EF) acc[u] = add4(acc[u], r2[u]);
  }
  __shared__ u32x4 stage[kFp4Vec];
  fp4_encode_rows<EF>(acc, reinterpret_cast<uint8_t*>(stage), tid);
  if constexpr (EF) {
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) stf4<kStNT>(rs, u * kThreads + tid, acc[u]);
  }
  fp4_store_slot<kStNT>(stage, out + size_t(j) * DL_FP4_SLOT_BYTES, tid);
}

}  // namespace

hipError_t launch_delta_fp4(const Launch& L, int inner_slot, const float* outer, float* resid,
                            uint8_t* slots) {
  if (resid) return run(L, DeltaFp4<true>{inner_slot, outer, slots, L.c0, resid});
  return run(L, DeltaFp4<false>{inner_slot, outer, slots, L.c0, nullptr});
}

hipError_t launch_unpack_sgd_fp4(const Launch& L, const uint8_t* slots, float* outer, float* mom,
                                 SgdArgs a, int inner_slot) {
  return with_sgd_rule(mom, a, [&](auto rule) {
    return run(L, UnpackFp4<decltype(rule)>{slots, L.c0, outer, rule, inner_slot});
  });
}

hipError_t launch_unpack_adamw_fp4(const Launch& L, const uint8_t* slots, float* outer, float* m1,
                                   float* m2, AdamArgs a, int inner_slot) {
  return run(L, UnpackFp4<AdamRule>{slots, L.c0, outer, AdamRule{m1, m2, a}, inner_slot});
}

hipError_t launch_fp4_reduce(const uint8_t* recv, int32_t n, int32_t m, int32_t divisor,
                             float* resid, uint8_t* out, hipStream_t s) {
  if (m <= 0) return hipSuccess;
  if (resid)
    hipLaunchKernelGGL(k_fp4_reduce<true>, dim3(m), dim3(kThreads), 0, s, recv, n, m, divisor,
                       resid, out);
  else
    hipLaunchKernelGGL(k_fp4_reduce<false>, dim3(m), dim3(kThreads), 0, s, recv, n, m, divisor,
                       resid, out);
  return hipGetLastError();
}

}  // namespace dl
