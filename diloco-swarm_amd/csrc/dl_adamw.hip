// The AdamW outer step (src/utils.py:60-61, configs/optimizer/adamw.toml, stepped at
// src/train.py:267) as one fused pass per chunk: the body of dl_outer_step.h with AdamRule (one
// element of torch's _single_tensor_adamw: adam1, dl_device.h, with the formula), over two of
// its gradient sources:
//   dl_unpack_adamw      FromWire, N > 1: reads the summed wire, θ, m, v; writes θ, m, v
//                        (+ inner): 28 B/param + 4 for the inner write (fp32 wire)
//   dl_unpack_adamw_merge  the same with the Merge policy: inner is read too and receives
//                        fmaf(alpha, inner - θ, θ): 36 B/param (20 read, 16 written)
//   dl_delta_pack_adamw  FromDeltaKeptOnWire, one peer (src/comm.py:118-119: no all-reduce, no
//                        division): g = θ - inner, the wire written as dl_delta_pack writes it
//                        and AdamW stepping on the value it holds; 16 B read + 20 B written per
//                        param (fp32 wire). Equal to dl_delta_pack followed by dl_unpack_adamw
//                        with divisor 1, wire included: the same body.
//   dl_shard_adamw       dl_unpack_adamw's body (inner_slot -1) over a flat shard after a
//                        reduce-scatter (k_flat, dl_flat.h): 28 B per shard element
// and, after an all_to_all, dl_shard_reduce_adamw (k_slices_adamw below): the rank-order sum
// of dl_flat.h, /n, then adam1.
// Pure streaming: no LDS, no cross-lane work. Four float4[kUnroll] arrays are live per lane
// (g, θ, m, v: 64 VGPRs), so the kernels stay far from spilling (make asm prints the report).
#include "dl_flat.h"

namespace dl {

hipError_t launch_unpack_adamw(const Launch& L, const void* wire, int wire_dtype, int divisor,
                               float* outer, float* m1, float* m2, AdamArgs a, int inner_slot) {
  return with_wire(wire, wire_dtype, divisor, [&](auto grad) {
    return run(L, outer_step(outer, grad, AdamRule{m1, m2, a}, inner_slot));
  });
}

// dl_unpack_adamw whose inner write merges (dl_outer_step.h, Merge): five load streams, 36 B/param
hipError_t launch_unpack_adamw_merge(const Launch& L, const void* wire, int wire_dtype, int divisor,
                                     float* outer, float* m1, float* m2, AdamArgs a, int inner_slot,
                                     float alpha) {
  return with_wire(wire, wire_dtype, divisor, [&](auto grad) {
    return run(L, outer_step_merge(outer, grad, AdamRule{m1, m2, a}, inner_slot, alpha));
  });
}

hipError_t launch_delta_pack_adamw(const Launch& L, int inner_slot, float* outer, void* wire,
                                   int wire_dtype, float* m1, float* m2, AdamArgs a) {
  return with_kept_wire(wire, wire_dtype, [&](auto grad) {
    return run(L, outer_step(outer, grad, AdamRule{m1, m2, a}, inner_slot));
  });
}

hipError_t launch_shard_adamw(const void* wire, int wire_dtype, int divisor, float* outer,
                              float* m1, float* m2, int64_t n, AdamArgs a, hipStream_t s) {
  return with_wire(wire, wire_dtype, divisor, [&](auto grad) {
    return run_flat(n, outer_step(outer, grad, AdamRule{m1, m2, a}, -1), s);
  });
}

// a3 + a4 after an all_to_all with the AdamW rule: dl_shard_reduce_sgd's slices and rank-order
// sum (slice_sum, dl_flat.h: the loads and the sum are that kernel's), g = Σ / n (n = 1: no
// division), avg_out[k] = g when AVG (what a later .grad read shows), then adam1 on this peer's
// θ, exp_avg and exp_avg_sq shards. A row past `len` does no arithmetic at all (no sqrt, no
// division), as AdamRule::kSkipPastChunk has it in the walker. Reads n·sizeof(W) + 12 B, writes
// 12 B (+ 4 with avg_out) per shard element; stores leave row by row: avg_out, θ, m, v.
// float4 rows per lane (adamw_slice_rows), chosen from the compiler's report of every
// candidate (profiles/shard_adamw_resource_usage.txt; none uses scratch). A lane carries θ and
// TWO state rows where SGD carries θ and one, 4 VGPRs more per row than slice_rows<N>() pays:
//   N = 1, 2: 4 rows -- 89 / 95 VGPRs, 5 waves per SIMD: the footprint and occupancy of the
//             walker's own AdamW body (dl_unpack_adamw, 4 rows, 90 to 96 VGPRs), so 5 x 4 rows of
//             every stream in flight per SIMD where 2 rows at 8 waves have 16;
//   N = 3..8: 2 rows -- 68 to 102 VGPRs, 7 to 4 waves; 4 rows would take 118 to 192 and leave
//             4 to 2 waves, fewer rows in flight, and 1 row (8 waves throughout) as many as 2
//             rows only at N = 7, 8;
//   N = 0 (run-time n > 8): 2 rows -- the slices accumulate on arrival, 57 VGPRs, 8 waves.
// The choice is slice_rows<N>()'s: the extra state row never crosses an occupancy step that
// the other row count would not cross too.
template <int N>
constexpr int adamw_slice_rows() {
#ifdef DL_ADAMW_SLICE_ROWS  // the candidates of the committed table
  return DL_ADAMW_SLICE_ROWS;
#else
  return N >= 1 && N <= 2 ? 4 : 2;
#endif
}
template <int N, typename W, bool AVG>
__global__ void __launch_bounds__(kThreads)
    k_slices_adamw(const W* __restrict__ slices, int32_t n, int64_t len, float* __restrict__ th,
                   float* __restrict__ m1, float* __restrict__ m2, float* __restrict__ avg,
                   AdamArgs a) {
  constexpr int kSU = adamw_slice_rows<N>();
  constexpr int64_t kSliceStep = kThreads * kSU * 4;
  const int nn = N > 0 ? N : n;
  for (int64_t base = int64_t(blockIdx.x) * kSliceStep; base < len;
       base += int64_t(gridDim.x) * kSliceStep) {
    const int32_t nv = slice_tile_rows(len, base, kSU);
    float* t0 = th + base;
    float* p1 = m1 + base;
    float* p2 = m2 + base;
    float4 g[kSU], t[kSU], m[kSU], v2[kSU];
    slice_sum<N>(slices, nn, len, base, nv, g, [&](int u, int v) {
      t[u] = ldf4<true>(t0, v);
      m[u] = ldf4<true>(p1, v);
      v2[u] = ldf4<true>(p2, v);
    });
#pragma unroll
    for (int u = 0; u < kSU; ++u) {
      const int v = u * kThreads + int(threadIdx.x);
      if (v < nv) {
        const float4 gg = nn > 1 ? div4(g[u], float(nn)) : g[u];
        if constexpr (AVG) stf4<kStNT>(avg + base, v, gg);
        adam1(gg.x, m[u].x, v2[u].x, t[u].x, a);
        adam1(gg.y, m[u].y, v2[u].y, t[u].y, a);
        adam1(gg.z, m[u].z, v2[u].z, t[u].z, a);
        adam1(gg.w, m[u].w, v2[u].w, t[u].w, a);
        stf4<kStNT>(t0, v, t[u]);
        stf4<kStNT>(p1, v, m[u]);
        stf4<kStNT>(p2, v, v2[u]);
      }
    }
  }
}

template <int N, typename W>
static hipError_t slices_adamw_n(const W* w, int32_t n, int64_t len, float* th, float* m1,
                                 float* m2, float* avg, AdamArgs a, hipStream_t s) {
  const int32_t grid = slice_grid(len, adamw_slice_rows<N>());
  if (avg)
    hipLaunchKernelGGL((k_slices_adamw<N, W, true>), dim3(grid), dim3(kThreads), 0, s, w, n, len,
                       th, m1, m2, avg, a);
  else
    hipLaunchKernelGGL((k_slices_adamw<N, W, false>), dim3(grid), dim3(kThreads), 0, s, w, n, len,
                       th, m1, m2, avg, a);
  return hipGetLastError();
}

template <typename W>
static hipError_t slices_adamw_t(const W* w, int32_t n, int64_t len, float* th, float* m1,
                                 float* m2, float* avg, AdamArgs a, hipStream_t s) {
  switch (n) {
    case 1: return slices_adamw_n<1>(w, n, len, th, m1, m2, avg, a, s);
    case 2: return slices_adamw_n<2>(w, n, len, th, m1, m2, avg, a, s);
    case 3: return slices_adamw_n<3>(w, n, len, th, m1, m2, avg, a, s);
    case 4: return slices_adamw_n<4>(w, n, len, th, m1, m2, avg, a, s);
    case 5: return slices_adamw_n<5>(w, n, len, th, m1, m2, avg, a, s);
    case 6: return slices_adamw_n<6>(w, n, len, th, m1, m2, avg, a, s);
    case 7: return slices_adamw_n<7>(w, n, len, th, m1, m2, avg, a, s);
    case 8: return slices_adamw_n<8>(w, n, len, th, m1, m2, avg, a, s);
    default: return slices_adamw_n<0>(w, n, len, th, m1, m2, avg, a, s);
  }
}

hipError_t launch_slices_adamw(const void* slices, int wire_dtype, int32_t n, int64_t len,
                               float* outer, float* m1, float* m2, float* avg_out, AdamArgs a,
                               hipStream_t s) {
  if (len <= 0) return hipSuccess;
  if (wire_dtype == DL_BF16)
    return slices_adamw_t(static_cast<const bf16_t*>(slices), n, len, outer, m1, m2, avg_out, a, s);
  return slices_adamw_t(static_cast<const float*>(slices), n, len, outer, m1, m2, avg_out, a, s);
}

}  // namespace dl
