// fp4 (MXFP4) wire for the per-step DP gradient average (GradSync, src/train.py:249-251):
// dl_fp4.hip's codec, slots and reduce with the gradient side of the exchange, the step
// dl_q8_grad.hip took for the int8 wire.
//   dl_gather_fp4      x = g (+ r); slot(c) <- enc(x) over chunk c of the bound gradient slot;
//                      (r <- x - deq(slot))                                (r: fp32, packed)
//   all_to_all, dl_fp4_reduce (divisor n), all_gather: as for the pseudo-gradient
//   dl_unpack_avg_fp4  dst = deq(slot) into .grad; optionally partials[c] = Σ of the stored values²
// The encoder is DeltaFp4 (dl_fp4.hip) with g in the place of θ - inner: x - (+0) = x bit for
// bit, so dl_gather_fp4 writes the bytes dl_delta_fp4 writes for outer = g, inner = +0. The
// decoder is UnpackFp4's slot side with UnpackAvgQ8's destination side: lane tid holds float4
// rows u*256 + tid of the chunk, so the lane rows -- and with them dl_norm.hip's summation
// order -- are those of dl_grad_sumsq on the destination.
// No MFMA, no scratch (profiles/gradsync_fp4_resource_usage.txt).
#include "dl_fp4_dev.h"
#include "dl_norm_dev.h"

namespace dl {
namespace {

// Reads 4 B (+ 4 B of r), writes 0.531 B (+ 4 B of r) per param. Every global load (g, r) is
// issued before any reduction; a group's amax is three shuffles among the 8 lanes of a float4
// row (16-B-aligned tensor storage) or five among 32 lanes (storage one float off). The slot is
// staged whole in LDS (zero scales and nibbles past the chunk's length) and leaves as 136 16-B
// stores; nothing of g or r is touched past the chunk's length.
template <bool EF>
struct GatherFp4 {
  int src_slot;
  uint8_t* slots;  // slot of chunk c at (c - c0) * DL_FP4_SLOT_BYTES
  int c0;
  float* resid;  // EF: the packed residual arena

  static __device__ __forceinline__ float x1(const float* g, const float* rs, int i) {
    if constexpr (EF) return g[i] + rs[i];
    else return g[i];
  }

  template <bool NTL, int NTS>
  __device__ __forceinline__ void run(const Chunk& ck, int c, void* const* caddr, int nchunk, int tid) const {
    __shared__ u32x4 stage[kFp4Vec];
    uint8_t* st = reinterpret_cast<uint8_t*>(stage);
    const float* g = slot_ptr<const float>(caddr, nchunk, src_slot, c);
    float* rs = EF ? resid + ck.poff : nullptr;
    uint8_t* slot = slots + size_t(c - c0) * DL_FP4_SLOT_BYTES;
    const int nv = ck.len >> 2;
    float4 x[kUnroll];
    if (aligned16(g)) {
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int v = u * kThreads + tid;
        if (v < nv) {
          x[u] = ldf4<NTL>(g, v);
          if constexpr (EF) x[u] = add4(x[u], ldf4<NTL>(rs, v));
        } else {  // the row of the < 4 tail elements stays with its group's lanes; +0 past the length
          float e[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) e[j] = 4 * v + j < ck.len ? x1(g, rs, 4 * v + j) : 0.f;
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
          e[j] = i < ck.len ? x1(g, rs, i) : 0.f;
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

// Reads 0.531 B, writes 4 B per param; the slots are only read. The whole slot arrives as 136
// non-temporal 16-B loads and goes through LDS; every lane takes its rows' 16 payload bits and
// scale byte, the lanes of the < 4 tail elements their own nibble. SUM: the chunk's Σ of the
// stored values² in dl_norm.hip's order (rows, tail element, block_sum).
template <bool SUM>
struct UnpackAvgFp4 {
  const uint8_t* slots;
  int c0;
  int dst_slot;
  double* partials;
  template <bool NTL, int NTS>
  __device__ __forceinline__ void run(const Chunk& ck, int c, void* const* caddr, int nchunk, int tid) const {
    float* dst = slot_ptr<float>(caddr, nchunk, dst_slot, c);
    const uint8_t* slot = slots + size_t(c - c0) * DL_FP4_SLOT_BYTES;
    const int nv = ck.len >> 2;
    __shared__ u32x4 stage[kFp4Vec];
    if (tid < kFp4Vec) stage[tid] = __builtin_nontemporal_load((const DL_GLOBAL u32x4*)slot + tid);
    __syncthreads();
    const uint8_t* st = reinterpret_cast<const uint8_t*>(stage);
    const uint16_t* st16 = reinterpret_cast<const uint16_t*>(stage);
    uint32_t w[kUnroll], sc[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int v = u * kThreads + tid;
      w[u] = st16[kFp4Scales / 2 + v];
      sc[u] = st[v >> 3];
    }
    const int i = (nv << 2) + tid;  // the < 4 tail elements
    uint32_t bt = 0u, sct = 0u;
    if (i < ck.len) {
      bt = st[kFp4Scales + (i >> 1)];
      sct = st[i >> 5];
    }
    __syncthreads();  // `stage` is reused by the workgroup's next chunk
    float4 x[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u)
      if (u * kThreads + tid < nv) x[u] = fp4_unpack4(w[u], fp4_half(sc[u]));
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
    const float gt = fp4_value((i & 1) ? bt >> 4 : bt, fp4_half(sct));
    if (i < ck.len) dst[i] = gt;
    if constexpr (SUM) {
      double acc = sumsq_rows(x, nv, tid);
      if (i < ck.len) sq1(acc, gt);
      acc = block_sum(acc, tid);
      if (tid == 0) partials[c] = acc;
    }
  }
};

}  // namespace

hipError_t launch_gather_fp4(const Launch& L, int src_slot, float* resid, uint8_t* slots) {
  if (resid) return run(L, GatherFp4<true>{src_slot, slots, L.c0, resid});
  return run(L, GatherFp4<false>{src_slot, slots, L.c0, nullptr});
}

hipError_t launch_unpack_avg_fp4(const Launch& L, const uint8_t* slots, int dst_slot,
                                 double* partials) {
  if (partials) return run(L, UnpackAvgFp4<true>{slots, L.c0, dst_slot, partials});
  return run(L, UnpackAvgFp4<false>{slots, L.c0, dst_slot, nullptr});
}

}  // namespace dl
