// Top-k sparse wire for the per-step DP gradient average (GradSync, src/train.py:249-251): the
// slots, selection and reduce of dl_topk.hip / dl_topk_fp4.hip with the gradient side of the
// exchange, the step dl_fp4_grad.hip took for the fp4 wire.
//   dl_gather_topk[_fp4]      x = g (+ r); slot(c) <- select_k(x) over chunk c of the bound
//                             gradient slot; (r <- x, +0 / x - deq where selected)
//   all_to_all, dl_topk[_fp4]_reduce (divisor n), all_gather: as for the pseudo-gradient
//   dl_unpack_avg_topk[_fp4]  dst = decode(slot) into .grad; optionally partials[c] = Σ of the
//                             stored values²
// The encoder is DeltaTopk / DeltaTopkFp4 with g in the place of θ - inner: x - (+0) = x bit for
// bit, so the slots are the bytes dl_delta_topk[_fp4] writes for outer = g, inner = +0. One body
// serves both value formats (Q4 picks topk_select + topk_store_slot or topk_fp4_encode).
// The decoder writes 4 B/param and reads 6k/4096: it keeps no dense copy of the chunk in LDS. A
// slot's entries become a 4096-bit occupancy map, a byte per position that names the entry, and
// the k values; every lane reads the four bits of each of its float4 rows and follows the byte
// only where a bit is set (k/4096 of the positions). 5.6 KiB of LDS against the 16 KiB of the
// dense chunk, one 4-B LDS read per row against a 16-B write and a 16-B read.
// Compiled as dl_topk.hip is, without packed fp32 instructions. No MFMA, no scratch.
#include <type_traits>

#include "dl_norm_dev.h"
#include "dl_topk_fp4_dev.h"

namespace dl {
namespace {

// Reads 4 B (+ 4 B of r), writes 6k/4096 or (16 + 2k)/4096 B (+ 4 B of r) per param. Every
// global load (g, r) is issued before the selection; the keys stay in the registers that hold x
// (Q4: the quantiser works on the k staged entries, no dense copy beside x). The residual goes
// back in place from registers by the lane that read it; nothing of g or r is touched past the
// chunk's length.
template <bool EF, bool Q4>
struct GatherTopk {
  int src_slot;
  uint8_t* slots;  // slot of chunk c at (c - c0) * slot_bytes(k)
  int c0;
  float* resid;  // EF: the packed residual arena
  int k;

  static __device__ __forceinline__ float x1(const float* g, const float* rs, int i) {
    if constexpr (EF) return g[i] + rs[i];
    else return g[i];
  }

  struct NoLds {};
  using QLds = std::conditional_t<Q4, TopkFp4Lds, NoLds>;  // the quantiser's LDS, Q4 only

  template <bool ROWS, int NTS>
  __device__ __forceinline__ void encode(float4 (&x)[kUnroll], TopkLds& lds, QLds& qlds, uint8_t* slot,
                                         int tid) const {
    if constexpr (Q4) topk_fp4_encode<ROWS, EF, NTS>(x, k, lds, qlds, slot, tid);
    else topk_select<ROWS, EF>(x, k, lds, tid);
  }

  template <bool NTL, int NTS>
  __device__ __forceinline__ void run(const Chunk& ck, int c, void* const* caddr, int nchunk, int tid) const {
    __shared__ TopkLds lds;
    __shared__ QLds qlds;
    const float* g = slot_ptr<const float>(caddr, nchunk, src_slot, c);
    float* rs = EF ? resid + ck.poff : nullptr;
    const size_t sb = Q4 ? size_t(DL_TOPK_FP4_SLOT_BYTES(k)) : size_t(DL_TOPK_SLOT_BYTES(k));
    uint8_t* slot = slots + size_t(c - c0) * sb;
    const int nv = ck.len >> 2;
    float4 x[kUnroll];
    if (aligned16(g)) {
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int v = u * kThreads + tid;
        if (v < nv) {
          x[u] = ldf4<NTL>(g, v);
          if constexpr (EF) x[u] = add4(x[u], ldf4<NTL>(rs, v));
        } else {  // the row of the < 4 tail elements; +0 past the length
          float e[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) e[j] = 4 * v + j < ck.len ? x1(g, rs, 4 * v + j) : 0.f;
          x[u] = make_float4(e[0], e[1], e[2], e[3]);
        }
      }
      encode<true, NTS>(x, lds, qlds, slot, tid);
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
          e[j] = i < ck.len ? x1(g, rs, i) : 0.f;
        }
        x[u] = make_float4(e[0], e[1], e[2], e[3]);
      }
      encode<false, NTS>(x, lds, qlds, slot, tid);
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
    if constexpr (!Q4) topk_store_slot<NTS>(lds, slot, k, tid);
  }
};

// what the decoder keeps of a slot in LDS
struct TopkMapLds {
  uint32_t bits[DL_CHUNK_ELEMS / 32];  // bit i: an entry names position i
  uint8_t tag[DL_CHUNK_ELEMS];         // where bit i is set: the entry; never cleared
  float val[DL_TOPK_MAX_K];            // entry e's value
};
static_assert(DL_TOPK_MAX_K <= 256, "an entry's number is one byte");
static_assert(DL_CHUNK_ELEMS / 32 <= kThreads && kThreads % 8 == 0, "one lane per map word");

// Reads 6k/4096 or (16 + 2k)/4096 B, writes 4 B per param; the slots are only read. Lane e < k
// takes entry e (Codec: TopkF32, TopkFp4) ahead of everything else, sets its position's bit and
// leaves its number and value; the lanes then build their rows in registers from +0: a row's
// four bits are one nibble of a map word, and only a set bit costs the two dependent reads of
// tag and val. Entries of one slot name distinct positions, so no value is lost; an all-zero
// slot names position 0 k times with the value +0. Nothing is stored past the chunk's length.
// SUM: the chunk's Σ of the stored values² in dl_norm.hip's order (rows, tail element,
// block_sum) over the dense registers, zeros included.
template <class Codec, bool SUM>
struct UnpackAvgTopk {
  const uint8_t* slots;
  int c0;
  int dst_slot;
  double* partials;
  int k;

  static __device__ __forceinline__ float at(const TopkMapLds& M, uint32_t word, int i) {
    return (word >> (i & 31)) & 1u ? M.val[M.tag[i]] : 0.f;
  }

  template <bool NTL, int NTS>
  __device__ __forceinline__ void run(const Chunk& ck, int c, void* const* caddr, int nchunk, int tid) const {
    __shared__ TopkMapLds M;
    float* dst = slot_ptr<float>(caddr, nchunk, dst_slot, c);
    const uint8_t* slot = slots + size_t(c - c0) * Codec::slot_bytes(k);
    const int nv = ck.len >> 2;
    TopkEntry en = {0.f, 0u};
    if (tid < k) en = Codec::entry(slot, k, tid);
    if (tid < DL_CHUNK_ELEMS / 32) M.bits[tid] = 0u;
    __syncthreads();
    if (tid < k) {
      atomicOr(&M.bits[en.idx >> 5], 1u << (en.idx & 31));
      M.tag[en.idx] = uint8_t(tid);
      M.val[tid] = en.val;
    }
    __syncthreads();
    float4 x[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int v = u * kThreads + tid;  // row v: bits 4v .. 4v + 3 of the map
      const uint32_t word = M.bits[v >> 3];
      x[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if ((word >> (4 * (v & 7))) & 15u)
        x[u] = make_float4(at(M, word, 4 * v), at(M, word, 4 * v + 1), at(M, word, 4 * v + 2),
                           at(M, word, 4 * v + 3));
    }
    const int i = (nv << 2) + tid;  // the < 4 tail elements
    float gt = 0.f;
    if (i < ck.len) gt = at(M, M.bits[i >> 5], i);
    __syncthreads();  // the map is reused by the workgroup's next chunk
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
    if (i < ck.len) dst[i] = gt;
    if constexpr (SUM) {
      double acc = sumsq_rows(x, nv, tid);
      if (i < ck.len) sq1(acc, gt);
      acc = block_sum(acc, tid);
      if (tid == 0) partials[c] = acc;
    }
  }
};

template <bool Q4>
hipError_t gather_topk(const Launch& L, int src_slot, float* resid, int k, uint8_t* slots) {
  if (resid) return run(L, GatherTopk<true, Q4>{src_slot, slots, L.c0, resid, k});
  return run(L, GatherTopk<false, Q4>{src_slot, slots, L.c0, nullptr, k});
}

template <class Codec>
hipError_t unpack_avg_topk(const Launch& L, const uint8_t* slots, int k, int dst_slot,
                           double* partials) {
  if (partials) return run(L, UnpackAvgTopk<Codec, true>{slots, L.c0, dst_slot, partials, k});
  return run(L, UnpackAvgTopk<Codec, false>{slots, L.c0, dst_slot, nullptr, k});
}

}  // namespace

hipError_t launch_gather_topk(const Launch& L, int src_slot, float* resid, int k, uint8_t* slots) {
  return gather_topk<false>(L, src_slot, resid, k, slots);
}

hipError_t launch_gather_topk_fp4(const Launch& L, int src_slot, float* resid, int k,
                                  uint8_t* slots) {
  return gather_topk<true>(L, src_slot, resid, k, slots);
}

hipError_t launch_unpack_avg_topk(const Launch& L, const uint8_t* slots, int k, int dst_slot,
                                  double* partials) {
  return unpack_avg_topk<TopkF32>(L, slots, k, dst_slot, partials);
}

hipError_t launch_unpack_avg_topk_fp4(const Launch& L, const uint8_t* slots, int k, int dst_slot,
                                      double* partials) {
  return unpack_avg_topk<TopkFp4>(L, slots, k, dst_slot, partials);
}

}  // namespace dl
