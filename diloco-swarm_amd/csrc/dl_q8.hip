// int8 wire codec for the pseudo-gradient exchange ("wire codecs beyond
// bf16, int8 with a per-bucket scale, for the cross-DC stand-in").
//
// Wire = one fixed-size SLOT per tree chunk: a 64-B header whose first 4 bytes are the fp32
// scale, then DL_CHUNK_ELEMS int8 values (bytes past the chunk's length stay zero). A bucket's
// slots are contiguous, in chunk order, padded with zero slots to a multiple of the peer count,
// so the exchange is two equal-split RCCL collectives ("int8 wire"):
//   dl_delta_q8       d = θ - inner; amax over the chunk (wave shuffles + LDS); q = rint(d/s)
//   all_to_all        every peer receives its 1/n of the slots from every peer
//   dl_q8_reduce      avg = (Σ_r q_r·s_r) / n in rank order; re-quantised with its own amax
//   all_gather        every peer receives every averaged slot (identical on all peers)
//   dl_unpack_sgd_q8  g = q·s; SGD exactly as dl_unpack_sgd; inner = θ
//   dl_unpack_adamw_q8  the same slots under the AdamW rule: g = q·s; adam1 on θ, exp_avg and
//                     exp_avg_sq exactly as dl_unpack_adamw (divisor 1); inner = θ
// Quantiser: s = amax / 127 (IEEE division); q = s == 0 ? 0 : clamp(rint(x / s), -127, 127);
// dequantised value q·s. Bus bytes per peer 2(n-1)/n · 1.016 B/param vs 8(n-1)/n for fp32.
//
// Error feedback (off by default): both lossy stages can carry what rounding removed into the
// next outer step, so an element that stays below s/2 of its chunk is sent late, not never:
//   dl_delta_q8_ef    x = (θ - inner) + r; slot <- quantise(x); r <- x - q·s   (r: fp32, packed)
//   dl_q8_reduce_ef   x = avg + r2;        slot <- quantise(x); r2 <- x - q·s  (r2: the owner's
//                     n_slots · DL_CHUNK_ELEMS floats)
// q·s is the product the unpack kernels decode, so r is exactly what the receiver did not get.
// The residuals stay local; every peer still receives byte-identical averaged slots. Non-finite
// values get no special case: a NaN/Inf element of x leaves a NaN/Inf residual (IEEE rules)
// until the residual is reset.
#include "dl_outer_step.h"
#include "dl_q8_dev.h"

namespace dl {
namespace {

// a2 with the int8 codec: slot(c) <- quantise(θ - inner) over chunk c.
// The 4096-B payload is assembled in LDS (zero beyond the chunk's length) and leaves in ONE
// 16-B store per lane: four 4-B-per-lane stores per lane (256 B per wave instruction) cost
// ~10 % of the kernel cold at T1.3B size against one 1-KB-per-wave store (tools/q8_layout.hip,
// profiles/r02_q8_layout.txt).
// EF: x = d + r replaces d, and r <- x - q·s is written back in place by the lane that read it
// (12 B read, 1.016 + 4 B written per param against 8 + 1.016); nothing of r is touched past the
// chunk's length. Every global load (θ, inner, r) is issued before the amax reduction.
template <bool EF>
struct DeltaQ8 {
  int inner_slot;
  const float* outer;
  uint8_t* slots;  // slot of chunk c at (c - c0) * DL_Q8_SLOT_BYTES
  int c0;
  float* resid;  // EF: the packed residual arena
  // the value to quantise, 16 B per stream: θ - inner, + r with error feedback
  template <bool NTL>
  static __device__ __forceinline__ float4 x4(const float* th, const float* in, const float* rs, int v) {
    const float4 d = sub4(ldf4<NTL>(th, v), ldf4<NTL>(in, v));
    if constexpr (EF) return add4(d, ldf4<NTL>(rs, v));
    else return d;
  }
  template <bool NTL, int NTS>
  __device__ __forceinline__ void run(const Chunk& ck, int c, void* const* caddr, int nchunk, int tid) const {
    __shared__ u32x4 stage[DL_CHUNK_ELEMS / 16];  // the payload, 16 B per lane
    uint32_t* st32 = reinterpret_cast<uint32_t*>(stage);
    uint8_t* st8 = reinterpret_cast<uint8_t*>(stage);
    const float* in = slot_ptr<const float>(caddr, nchunk, inner_slot, c);
    const float* th = outer + ck.poff;
    float* rs = EF ? resid + ck.poff : nullptr;
    uint8_t* slot = slots + size_t(c - c0) * DL_Q8_SLOT_BYTES;
    const int nv = ck.len >> 2;
    const bool vec = aligned16(in);
    stage[tid] = u32x4{0u, 0u, 0u, 0u};  // bytes past the chunk's length stay zero
    float4 d[kUnroll];
    float dt = 0.f;  // vector path: the < 4 tail elements
    float am = 0.f;
    if (vec) {
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int v = u * kThreads + tid;
        d[u] = v < nv ? x4<NTL>(th, in, rs, v) : make_float4(0.f, 0.f, 0.f, 0.f);
        am = fmaxf(am, amax4(d[u]));
      }
      const int i = (nv << 2) + tid;
      if (i < ck.len) dt = EF ? (th[i] - in[i]) + rs[i] : th[i] - in[i];
    } else {  // 4-B-aligned tensor storage: element k*256 + tid of the chunk in d[k/4].k%4
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        float e[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int i = (4 * u + j) * kThreads + tid;
          e[j] = i < ck.len ? (EF ? (th[i] - in[i]) + rs[i] : th[i] - in[i]) : 0.f;
        }
        d[u] = make_float4(e[0], e[1], e[2], e[3]);
        am = fmaxf(am, amax4(d[u]));
      }
    }
    am = fmaxf(am, fabsf(dt));
    const float s = block_amax(am) / 127.f;  // its barriers also order the zeroing above
    if (vec) {
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int v = u * kThreads + tid;
        if (v < nv) {
          st32[v] = pack4(d[u], s);
          if constexpr (EF) stf4<NTS>(rs, v, resid4(d[u], s));
        }
      }
      const int i = (nv << 2) + tid;
      if (i < ck.len) {
        st8[i] = uint8_t(q8(dt, s));
        if constexpr (EF) rs[i] = resid1(dt, s);
      }
    } else {
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const float e[4] = {d[u].x, d[u].y, d[u].z, d[u].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int i = (4 * u + j) * kThreads + tid;
          if (i < ck.len) {
            st8[i] = uint8_t(q8(e[j], s));
            if constexpr (EF) rs[i] = resid1(e[j], s);
          }
        }
      }
    }
    __syncthreads();
    const u32x4 w = stage[tid];
    DL_GLOBAL u32x4* q = (DL_GLOBAL u32x4*)(slot + kQ8Header);
    if constexpr (NTS)
      __builtin_nontemporal_store(w, q + tid);
    else
      q[tid] = w;
    store_header<NTS>(slot, s, tid);
    __syncthreads();  // `stage` is reused by the workgroup's next chunk
  }
};

// a3 /n happened in dl_q8_reduce; a4 + a5 from the averaged int8 slots
template <int MODE>
struct UnpackSgdQ8 {
  const uint8_t* slots;
  int c0;
  float* outer;
  float* mom;
  SgdArgs a;
  int inner_slot;
  template <bool NTL, int NTS>
  __device__ __forceinline__ void run(const Chunk& ck, int c, void* const* caddr, int nchunk, int tid) const {
    float* in = inner_slot >= 0 ? slot_ptr<float>(caddr, nchunk, inner_slot, c) : nullptr;
    const uint8_t* slot = slots + size_t(c - c0) * DL_Q8_SLOT_BYTES;
    const uint8_t* q = slot + kQ8Header;
    const float s = *reinterpret_cast<const float*>(slot);
    float* th = outer + ck.poff;
    float* mb = mom + ck.poff;
    auto one = [&](int i) {
      const float g = float(int8_t(q[i])) * s;
      float b = (MODE == 2) ? mb[i] : 0.f, t1 = th[i];
      sgd1<MODE>(g, b, t1, a);
      th[i] = t1;
      if (MODE != 0) mb[i] = b;
      if (in) in[i] = t1;
    };
    if (in == nullptr || aligned16(in)) {
      const int nv = ck.len >> 2;
      uint32_t w[kUnroll];
      float4 t[kUnroll], m[kUnroll];
      // the slot's 4 KB payload arrives as one non-temporal 16-B load per lane, staged in LDS
      // (tools/gpu_ab_q8.sh: -1 % at T1.3B against four 4-B loads per lane)
      __shared__ u32x4 stage[DL_CHUNK_ELEMS / 16];
      const u32x4 qv = __builtin_nontemporal_load((const DL_GLOBAL u32x4*)q + tid);
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int v = u * kThreads + tid;
        if (v < nv) {
          t[u] = ldf4<NTL>(th, v);
          if (MODE == 2) m[u] = ldf4<NTL>(mb, v);
        }
      }
      stage[tid] = qv;
      __syncthreads();
      const uint32_t* st32 = reinterpret_cast<const uint32_t*>(stage);
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) w[u] = st32[u * kThreads + tid];
      __syncthreads();  // `stage` is reused by the workgroup's next chunk
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int v = u * kThreads + tid;
        if (v < nv) {
          sgd4<MODE>(unpack4(w[u], s), m[u], t[u], a);
          stf4<NTS>(th, v, t[u]);
          if (MODE != 0) stf4<NTS>(mb, v, m[u]);
          if (in) stf4<NTS>(in, v, t[u]);
        }
      }
      const int i = (nv << 2) + tid;
      if (i < ck.len) one(i);
    } else {
      for (int i = tid; i < ck.len; i += kThreads) one(i);
    }
  }
};

// UnpackSgdQ8's slot side (one 16-B payload load per lane, the LDS round trip, the wave-uniform
// scale) under the AdamW rule, laid out as the AdamW body of dl_outer_step.h: the payload and
// every 16-B load of θ, exp_avg and exp_avg_sq are issued before the LDS round trip, the rule
// (AdamRule: adam1, written once) runs per component on the rows inside the chunk only, and
// the stores leave one stream at a time: θ, exp_avg, exp_avg_sq, inner. Reads 1.016 + 12 B,
// writes 12 B (+ 4 with the inner write) per param.
struct UnpackAdamWQ8 {
  static constexpr int K = AdamRule::kStates;
  const uint8_t* slots;
  int c0;
  float* outer;
  AdamRule rule;
  int inner_slot;

  template <int J>
  __device__ __forceinline__ void step(float g, float4 (&m)[K][kUnroll], int u, float4& t) const {
    float e[K];
#pragma unroll
    for (int k = 0; k < K; ++k) e[k] = comp<J>(m[k][u]);
    rule.apply(g, e, comp<J>(t));
#pragma unroll
    for (int k = 0; k < K; ++k) comp<J>(m[k][u]) = e[k];
  }

  template <bool NTL, int NTS>
  __device__ __forceinline__ void run(const Chunk& ck, int c, void* const* caddr, int nchunk, int tid) const {
    float* in = inner_slot >= 0 ? slot_ptr<float>(caddr, nchunk, inner_slot, c) : nullptr;
    const uint8_t* slot = slots + size_t(c - c0) * DL_Q8_SLOT_BYTES;
    const uint8_t* q = slot + kQ8Header;
    const float s = *reinterpret_cast<const float*>(slot);
    float* th = outer + ck.poff;
    float* sp[K];
#pragma unroll
    for (int k = 0; k < K; ++k) sp[k] = rule.state(k) + ck.poff;
    auto one = [&](int i) {
      const float g = float(int8_t(q[i])) * s;
      float t1 = th[i];
      float e[K];
#pragma unroll
      for (int k = 0; k < K; ++k) e[k] = sp[k][i];
      rule.apply(g, e, t1);
      th[i] = t1;
#pragma unroll
      for (int k = 0; k < K; ++k) sp[k][i] = e[k];
      if (in) in[i] = t1;
    };
    if (in == nullptr || aligned16(in)) {
      const int nv = ck.len >> 2;
      uint32_t w[kUnroll];
      float4 t[kUnroll], m[K][kUnroll];
      __shared__ u32x4 stage[DL_CHUNK_ELEMS / 16];
      // the whole slot payload (zero past the chunk's length), as in UnpackSgdQ8
      const u32x4 qv = __builtin_nontemporal_load((const DL_GLOBAL u32x4*)q + tid);
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int v = u * kThreads + tid;
        if (v < nv) {
          t[u] = ldf4<NTL>(th, v);
#pragma unroll
          for (int k = 0; k < K; ++k) m[k][u] = ldf4<NTL>(sp[k], v);
        }
      }
      stage[tid] = qv;
      __syncthreads();
      const uint32_t* st32 = reinterpret_cast<const uint32_t*>(stage);
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) w[u] = st32[u * kThreads + tid];
      __syncthreads();  // `stage` is reused by the workgroup's next chunk
      static_assert(AdamRule::kSkipPastChunk, "rows past the chunk do no arithmetic");
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        if (u * kThreads + tid < nv) {
          const float4 g = unpack4(w[u], s);
          step<0>(g.x, m, u, t[u]);
          step<1>(g.y, m, u, t[u]);
          step<2>(g.z, m, u, t[u]);
          step<3>(g.w, m, u, t[u]);
        }
      }
      store_rows<NTS>(th, t, nv, tid);
#pragma unroll
      for (int k = 0; k < K; ++k) store_rows<NTS>(sp[k], m[k], nv, tid);
      if (in) store_rows<NTS>(in, t, nv, tid);
      const int i = (nv << 2) + tid;
      if (i < ck.len) one(i);
    } else {
      for (int i = tid; i < ck.len; i += kThreads) one(i);
    }
  }
};

// Σ over n peers' copies of m slots (recv laid out [peer][slot]) -> averaged, re-quantised slots
// EF: the owner's residual r2 (m · DL_CHUNK_ELEMS floats) is added to the average before the
// quantiser and rewritten by the same lane; a zero slot keeps a zero residual (x = q = r2 = 0).
template <bool EF>
__global__ void __launch_bounds__(kThreads)
    k_q8_reduce(const uint8_t* recv, int32_t n, int32_t m, int32_t divisor, float* resid,
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
    const uint8_t* slot = recv + (size_t(r) * m + j) * DL_Q8_SLOT_BYTES;
    const float s = *reinterpret_cast<const float*>(slot);
    const uint8_t* q = slot + kQ8Header;
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const float4 x = unpack4(((gcu32)q)[u * kThreads + tid], s);
      acc[u] = make_float4(acc[u].x + x.x, acc[u].y + x.y, acc[u].z + x.z, acc[u].w + x.w);
    }
  }
  float am = 0.f;
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) {
    if (divisor > 1) acc[u] = div4(acc[u], float(divisor));
    if constexpr (EF) acc[u] = add4(acc[u], r2[u]);
    am = fmaxf(am, amax4(acc[u]));
  }
  const float s = block_amax(am) / 127.f;
  // the averaged payload leaves as one non-temporal 16-B store per lane (as in DeltaQ8)
  __shared__ u32x4 stage[DL_CHUNK_ELEMS / 16];
  uint32_t* st32 = reinterpret_cast<uint32_t*>(stage);
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) {
    st32[u * kThreads + tid] = pack4(acc[u], s);
    if constexpr (EF) stf4<kStNT>(rs, u * kThreads + tid, resid4(acc[u], s));
  }
  __syncthreads();
  uint8_t* o = out + size_t(j) * DL_Q8_SLOT_BYTES;
  __builtin_nontemporal_store(stage[tid], (DL_GLOBAL u32x4*)(o + kQ8Header) + tid);
  store_header<kStNT>(o, s, tid);
}

}  // namespace

hipError_t launch_delta_q8(const Launch& L, int inner_slot, const float* outer, uint8_t* slots) {
  return run(L, DeltaQ8<false>{inner_slot, outer, slots, L.c0, nullptr});
}

hipError_t launch_delta_q8_ef(const Launch& L, int inner_slot, const float* outer, float* resid,
                              uint8_t* slots) {
  return run(L, DeltaQ8<true>{inner_slot, outer, slots, L.c0, resid});
}

hipError_t launch_unpack_sgd_q8(const Launch& L, const uint8_t* slots, float* outer, float* mom,
                                SgdArgs a, int inner_slot) {
  if (a.momentum == 0.f) return run(L, UnpackSgdQ8<0>{slots, L.c0, outer, mom, a, inner_slot});
  if (a.first) return run(L, UnpackSgdQ8<1>{slots, L.c0, outer, mom, a, inner_slot});
  return run(L, UnpackSgdQ8<2>{slots, L.c0, outer, mom, a, inner_slot});
}

hipError_t launch_unpack_adamw_q8(const Launch& L, const uint8_t* slots, float* outer, float* m1,
                                  float* m2, AdamArgs a, int inner_slot) {
  return run(L, UnpackAdamWQ8{slots, L.c0, outer, AdamRule{m1, m2, a}, inner_slot});
}

hipError_t launch_q8_reduce(const uint8_t* recv, int32_t n, int32_t m, int32_t divisor,
                            float* resid, uint8_t* out, hipStream_t s) {
  if (m <= 0) return hipSuccess;
  if (resid)
    hipLaunchKernelGGL(k_q8_reduce<true>, dim3(m), dim3(kThreads), 0, s, recv, n, m, divisor,
                       resid, out);
  else
    hipLaunchKernelGGL(k_q8_reduce<false>, dim3(m), dim3(kThreads), 0, s, recv, n, m, divisor,
                       resid, out);
  return hipGetLastError();
}

}  // namespace dl
