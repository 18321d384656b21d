// Top-k sparse wire codec for the pseudo-gradient exchange: per tree chunk the k entries of
// largest magnitude, exact fp32 values with u16 positions, on the int8 / fp4 wires' slot plan and
// exchange. What selection leaves out stays in the residual (error feedback).
//
// Wire = one DL_TOPK_SLOT_BYTES(k) = 6k-byte SLOT per tree chunk: k fp32 values, then k u16
// indices, ascending (include/diloco_hip.h states the order and its tie rule). 6k/4096 B/param.
//   dl_delta_topk       x = θ - inner (+ r); slot <- select_k(x); (r <- x, +0 where selected)
//   all_to_all          every peer receives its 1/n of the slots from every peer
//   dl_topk_reduce      acc = Σ_r decode_r in rank order, / n (+ r2); selected again
//   all_gather          every peer receives every averaged slot (identical on all peers)
//   dl_unpack_sgd_topk / dl_unpack_adamw_topk   g = decode(slot); the rule of dl_unpack_sgd /
//                       dl_unpack_adamw (divisor 1); inner = θ
// The selection is topk_select of dl_topk_dev.h, shared by the encoder and the reduce. Decoding
// scatters a slot's entries into a dense 16-KiB chunk in LDS, one lane per entry (indices are
// distinct within a slot, so no atomics), and every lane reads its rows back from it.
#include "dl_topk_dev.h"

namespace dl {
namespace {

// a2 with the top-k codec. Every global load is issued before the selection; the keys stay in
// the registers that hold x. EF: x = d + r replaces d, and r <- x with +0 at the selected
// positions goes back in place from registers by the lane that read it, nothing of r touched
// past the chunk's length.
template <bool EF>
struct DeltaTopk {
  int inner_slot;
  const float* outer;
  uint8_t* slots;  // slot of chunk c at (c - c0) * 6k
  int c0;
  float* resid;  // EF: the packed residual arena
  int k;

  static __device__ __forceinline__ float x1(const float* th, const float* in, const float* rs, int i) {
    if constexpr (EF) return (th[i] - in[i]) + rs[i];
    else return th[i] - in[i];
  }

  template <bool NTL, int NTS>
  __device__ __forceinline__ void run(const Chunk& ck, int c, void* const* caddr, int nchunk, int tid) const {
    __shared__ TopkLds lds;
    const float* in = slot_ptr<const float>(caddr, nchunk, inner_slot, c);
    const float* th = outer + ck.poff;
    float* rs = EF ? resid + ck.poff : nullptr;
    uint8_t* slot = slots + size_t(c - c0) * DL_TOPK_SLOT_BYTES(k);
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
        } else {  // the row of the < 4 tail elements; +0 past the length
          float e[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) e[j] = 4 * v + j < ck.len ? x1(th, in, rs, 4 * v + j) : 0.f;
          x[u] = make_float4(e[0], e[1], e[2], e[3]);
        }
      }
      topk_select<true, EF>(x, k, lds, tid);
      if constexpr (EF) {
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          const int v = u * kThreads + tid;
          if (v < nv) {
            stf4<NTS>(rs, v, x[u]);
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (4 * v + j < ck.len) rs[4 * v + j] = elem(x[u], j);
          }
        }
      }
    } else {  // element (4u + j)·256 + tid of the chunk in x[u].j
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
      topk_select<false, EF>(x, k, lds, tid);
      if constexpr (EF) {
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int i = (4 * u + j) * kThreads + tid;
            if (i < ck.len) rs[i] = elem(x[u], j);
          }
        }
      }
    }
    topk_store_slot<NTS>(lds, slot, k, tid);
  }
};

// Σ over n peers' copies of m slots (recv laid out [peer][slot]) -> averaged slots, selected
// again; one workgroup per slot. The accumulator is the dense chunk in LDS: per peer, in rank
// order, lane e adds entry e at its index (one rounded add per entry; an all-zero slot has k
// entries at index 0 that all store the same sum), one barrier per peer, the next peer's entry
// loaded ahead of it. Then every lane takes its float4 rows: / divisor, + r2, topk_select over
// all 4096 positions, r2 rewritten by the same lane.
template <bool EF>
__global__ void __launch_bounds__(kThreads)
    k_topk_reduce(const uint8_t* recv, int32_t n, int32_t m, int32_t divisor, float* resid,
                  int32_t k, uint8_t* out) {  // recv == out at one peer (in place): no __restrict__
  __shared__ float4 dense4[DL_CHUNK_ELEMS / 4];
  __shared__ TopkLds lds;
  float* dense = reinterpret_cast<float*>(dense4);
  const int j = blockIdx.x;
  const int tid = threadIdx.x;
  const size_t sb = size_t(DL_TOPK_SLOT_BYTES(k));
  float* rs = EF ? resid + size_t(j) * DL_CHUNK_ELEMS : nullptr;
  float4 r2[kUnroll];
  TopkEntry en = {0.f, 0u};
  if (tid < k) en = topk_entry(recv + size_t(j) * sb, k, tid);
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) {
    if constexpr (EF) r2[u] = ldf4<true>(rs, u * kThreads + tid);
    dense4[u * kThreads + tid] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();
  for (int r = 0; r < n; ++r) {  // rank order: the sum is identical on every peer
    TopkEntry nx = {0.f, 0u};
    if (r + 1 < n && tid < k) nx = topk_entry(recv + (size_t(r + 1) * m + j) * sb, k, tid);
    if (tid < k) dense[en.idx] = dense[en.idx] + en.val;
    __syncthreads();
    en = nx;
  }
  float4 acc[kUnroll];
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) {
    acc[u] = dense4[u * kThreads + tid];
    if (divisor > 1) acc[u] = div4(acc[u], float(divisor));
    if constexpr (EF) acc[u] = add4(acc[u], r2[u]);
  }
  topk_select<true, EF>(acc, k, lds, tid);
  if constexpr (EF) {
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) stf4<kStNT>(rs, u * kThreads + tid, acc[u]);
  }
  topk_store_slot<kStNT>(lds, out + size_t(j) * sb, k, tid);
}

}  // namespace

hipError_t launch_delta_topk(const Launch& L, int inner_slot, const float* outer, float* resid,
                             int k, uint8_t* slots) {
  if (resid) return run(L, DeltaTopk<true>{inner_slot, outer, slots, L.c0, resid, k});
  return run(L, DeltaTopk<false>{inner_slot, outer, slots, L.c0, nullptr, k});
}

hipError_t launch_unpack_sgd_topk(const Launch& L, const uint8_t* slots, int k, float* outer,
                                  float* mom, SgdArgs a, int inner_slot) {
  return with_sgd_rule(mom, a, [&](auto rule) {
    return run(L, UnpackTopk<decltype(rule), TopkF32>{slots, L.c0, outer, rule, inner_slot, k});
  });
}

hipError_t launch_unpack_adamw_topk(const Launch& L, const uint8_t* slots, int k, float* outer,
                                    float* m1, float* m2, AdamArgs a, int inner_slot) {
  return run(L, UnpackTopk<AdamRule, TopkF32>{slots, L.c0, outer, AdamRule{m1, m2, a}, inner_slot, k});
}

hipError_t launch_topk_reduce(const uint8_t* recv, int32_t n, int32_t m, int32_t divisor,
                              float* resid, int32_t k, uint8_t* out, hipStream_t s) {
  if (m <= 0) return hipSuccess;
  if (resid)
    hipLaunchKernelGGL(k_topk_reduce<true>, dim3(m), dim3(kThreads), 0, s, recv, n, m, divisor,
                       resid, k, out);
  else
    hipLaunchKernelGGL(k_topk_reduce<false>, dim3(m), dim3(kThreads), 0, s, recv, n, m, divisor,
                       resid, k, out);
  return hipGetLastError();
}

}  // namespace dl
