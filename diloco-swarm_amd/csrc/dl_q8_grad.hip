// int8 wire for the per-step DP gradient average (GradSync, src/train.py:249-251; SURVEY §8f
// row 1): dl_q8.hip's codec, slots and reduce with the gradient side of the exchange.
//   dl_gather_q8      slot(c) <- quantise(g) over chunk c of the bound gradient slot
//   dl_gather_q8_ef   x = g + r; slot(c) <- quantise(x); r <- x - q·s      (r: fp32, packed)
//   all_to_all, dl_q8_reduce[_ef] (divisor n), all_gather: as for the pseudo-gradient
//   dl_unpack_avg_q8  dst = q·s into .grad; optionally partials[c] = Σ of the stored values²
// The encoders are DeltaQ8 (dl_q8.hip) with g in the place of θ - inner: x - (+0) = x bit for
// bit, so dl_gather_q8 writes the bytes dl_delta_q8 writes for outer = g, inner = +0. The decoder
// is UnpackSgdQ8's slot side with UnpackAvgSumSq's destination side (dl_norm.hip): st32 word
// u*256 + tid holds the four elements of float4 row u*256 + tid, so the lane rows -- and with
// them dl_norm.hip's summation order -- are those of dl_grad_sumsq on the destination.
// No MFMA, no scratch (profiles/gradsync_q8_resource_usage.txt).
#include "dl_norm_dev.h"
#include "dl_q8_dev.h"

namespace dl {
namespace {

// Reads 4 B (+ 4 B of r), writes 1.016 B (+ 4 B of r) per param. Every global load (g, r) is
// issued before the amax reduction; the payload is assembled in LDS (zero beyond the chunk's
// length) and leaves in one 16-B store per lane; nothing of g or r is touched past the
// chunk's length.
template <bool EF>
struct GatherQ8 {
  int src_slot;
  uint8_t* slots;  // slot of chunk c at (c - c0) * DL_Q8_SLOT_BYTES
  int c0;
  float* resid;  // EF: the packed residual arena
  template <bool NTL, int NTS>
  __device__ __forceinline__ void run(const Chunk& ck, int c, void* const* caddr, int nchunk, int tid) const {
    __shared__ u32x4 stage[DL_CHUNK_ELEMS / 16];  // the payload, 16 B per lane
    uint32_t* st32 = reinterpret_cast<uint32_t*>(stage);
    uint8_t* st8 = reinterpret_cast<uint8_t*>(stage);
    const float* g = slot_ptr<const float>(caddr, nchunk, src_slot, c);
    float* rs = EF ? resid + ck.poff : nullptr;
    uint8_t* slot = slots + size_t(c - c0) * DL_Q8_SLOT_BYTES;
    const int nv = ck.len >> 2;
    const bool vec = aligned16(g);
    stage[tid] = u32x4{0u, 0u, 0u, 0u};  // bytes past the chunk's length stay zero
    float4 d[kUnroll];
    float dt = 0.f;  // vector path: the < 4 tail elements
    float am = 0.f;
    if (vec) {
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int v = u * kThreads + tid;
        d[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (v < nv) {
          d[u] = ldf4<NTL>(g, v);
          if constexpr (EF) d[u] = add4(d[u], ldf4<NTL>(rs, v));
        }
        am = fmaxf(am, amax4(d[u]));
      }
      const int i = (nv << 2) + tid;
      if (i < ck.len) dt = EF ? g[i] + rs[i] : g[i];
    } else {  // 4-B-aligned tensor storage: element k*256 + tid of the chunk in d[k/4].k%4
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        float e[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int i = (4 * u + j) * kThreads + tid;
          e[j] = i < ck.len ? (EF ? g[i] + rs[i] : g[i]) : 0.f;
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

// Reads 1.016 B, writes 4 B per param; the slots are only read. The payload arrives as one
// non-temporal 16-B load per lane and goes through LDS; the scale is wave-uniform. SUM: the
// chunk's Σ of the stored values² in dl_norm.hip's order (rows, tail element, block_sum).
template <bool SUM>
struct UnpackAvgQ8 {
  const uint8_t* slots;
  int c0;
  int dst_slot;
  double* partials;
  template <bool NTL, int NTS>
  __device__ __forceinline__ void run(const Chunk& ck, int c, void* const* caddr, int nchunk, int tid) const {
    float* dst = slot_ptr<float>(caddr, nchunk, dst_slot, c);
    const uint8_t* slot = slots + size_t(c - c0) * DL_Q8_SLOT_BYTES;
    const uint8_t* q = slot + kQ8Header;
    const float s = *reinterpret_cast<const float*>(slot);
    const int nv = ck.len >> 2;
    __shared__ u32x4 stage[DL_CHUNK_ELEMS / 16];
    // the whole slot payload (zero past the chunk's length), as in UnpackSgdQ8
    stage[tid] = __builtin_nontemporal_load((const DL_GLOBAL u32x4*)q + tid);
    __syncthreads();
    const uint32_t* st32 = reinterpret_cast<const uint32_t*>(stage);
    const uint8_t* st8 = reinterpret_cast<const uint8_t*>(stage);
    uint32_t w[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) w[u] = st32[u * kThreads + tid];
    const int i = (nv << 2) + tid;  // the < 4 tail elements
    const int8_t qt = i < ck.len ? int8_t(st8[i]) : int8_t(0);
    __syncthreads();  // `stage` is reused by the workgroup's next chunk
    float4 x[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u)
      if (u * kThreads + tid < nv) x[u] = unpack4(w[u], s);
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
    const float gt = float(qt) * s;
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

hipError_t launch_gather_q8(const Launch& L, int src_slot, float* resid, uint8_t* slots) {
  if (resid) return run(L, GatherQ8<true>{src_slot, slots, L.c0, resid});
  return run(L, GatherQ8<false>{src_slot, slots, L.c0, nullptr});
}

hipError_t launch_unpack_avg_q8(const Launch& L, const uint8_t* slots, int dst_slot,
                                double* partials) {
  if (partials) return run(L, UnpackAvgQ8<true>{slots, L.c0, dst_slot, partials});
  return run(L, UnpackAvgQ8<false>{slots, L.c0, dst_slot, nullptr});
}

}  // namespace dl
