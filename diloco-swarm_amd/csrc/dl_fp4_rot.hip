// The fp4 (MXFP4) wire of dl_fp4.hip behind a randomised Hadamard rotation: each 256-element
// block of a chunk is multiplied by random signs and transformed before the quantiser, and
// transformed back after the decoder, so an outlier is spread over its block instead of pushing
// the other 31 elements of its group onto the coarse end of the E2M1 grid. The transform R, its
// inverse and the sign hash are stated in include/diloco_hip.h; slot format, scale and nibble
// rules are dl_fp4.hip's, and dl_fp4_reduce serves unchanged (R is linear).
//   dl_delta_fp4_rot     x = θ - inner (+ r); slot <- enc(R(x)); (r <- x - R^-1(deq(slot)))
//   dl_unpack_sgd_fp4_rot / dl_unpack_adamw_fp4_rot   g = R^-1(deq(slot)); the rule of
//                        dl_unpack_sgd / dl_unpack_adamw (divisor 1); inner = θ
//   dl_decode_fp4_rot    dst <- R^-1(deq(slot)), the value those steps used
// One register layout for both alignments, the float4 rows of fp4_encode_rows: a block is then
// the row of one wavefront and the butterfly runs in registers and across lanes
// (dl_fp4_rot_dev.h). A tensor whose storage is only 4-B aligned is loaded and stored element by
// element INTO that layout; the arithmetic is the same instructions, so the results do not
// depend on alignment. Compiled without packed fp32 instructions (the Makefile).
#include "dl_fp4_rot_dev.h"
#include "dl_outer_step.h"

namespace dl {
namespace {

// Every global load is issued before the first stage. The transform runs on all 4096 positions
// (+0 at and past the length), so a short chunk's last live block has non-zero groups past the
// length and blocks wholly past it encode to zero bytes. EF: the original x stays in registers
// beside R(x); what rounding puts on positions past the length is dropped.
template <bool EF>
struct DeltaFp4Rot {
  int inner_slot;
  const float* outer;
  uint8_t* slots;  // slot of chunk c at (c - c0) * DL_FP4_SLOT_BYTES
  int c0;
  float* resid;  // EF: the packed residual arena
  uint32_t seed;

  template <bool NTL, int NTS>
  __device__ __forceinline__ void run(const Chunk& ck, int c, void* const* caddr, int nchunk, int tid) const {
    __shared__ u32x4 stage[kFp4Vec];
    const float* in = slot_ptr<const float>(caddr, nchunk, inner_slot, c);
    const float* th = outer + ck.poff;
    float* rs = EF ? resid + ck.poff : nullptr;
    const bool vec = aligned16(in);
    float4 x[kUnroll], y[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int v = u * kThreads + tid;
      x[u] = sub4(ld_row<NTL>(th, v, ck.len, true), ld_row<NTL>(in, v, ck.len, vec));
      if constexpr (EF) x[u] = add4(x[u], ld_row<NTL>(rs, v, ck.len, true));
      y[u] = x[u];
    }
    rotate_rows(y, seed, tid);
    if constexpr (EF) {
      fp4_encode_rows_deq(y, reinterpret_cast<uint8_t*>(stage), tid);
      unrotate_rows(y, seed, tid);
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) x[u] = sub4(x[u], y[u]);
      st_rows<NTS>(rs, x, ck.len, true, tid);
    } else {
      fp4_encode_rows<false>(y, reinterpret_cast<uint8_t*>(stage), tid);
    }
    fp4_store_slot<NTS>(stage, slots + size_t(c - c0) * DL_FP4_SLOT_BYTES, tid);
  }
};

// UnpackFp4 with g = R^-1(deq(slot)) over whole blocks, then the rule on the rows that hold an
// element of the chunk (the components of the last row past the length step on zeros and are
// never stored). Stores leave one stream at a time: θ, the state, inner.
template <class Rule>
struct UnpackFp4Rot {
  static constexpr int K = Rule::kStates;
  const uint8_t* slots;
  int c0;
  float* outer;
  Rule rule;
  int inner_slot;
  uint32_t seed;

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
    __shared__ u32x4 stage[kFp4Vec];
    float* in = inner_slot >= 0 ? slot_ptr<float>(caddr, nchunk, inner_slot, c) : nullptr;
    float* th = outer + ck.poff;
    float* sp[K];
#pragma unroll
    for (int k = 0; k < K; ++k) sp[k] = rule.state(k) + ck.poff;
    float4 g[kUnroll], t[kUnroll], m[K][kUnroll];
    fp4_load_rows(slots + size_t(c - c0) * DL_FP4_SLOT_BYTES, stage, tid, g, [&] {
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int v = u * kThreads + tid;
        t[u] = ld_row<NTL>(th, v, ck.len, true);
        if (Rule::kLoadState) {
#pragma unroll
          for (int k = 0; k < K; ++k) m[k][u] = ld_row<NTL>(sp[k], v, ck.len, true);
        }
      }
    });
    unrotate_rows(g, seed, tid);
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      if (4 * (u * kThreads + tid) < ck.len) {
        step<0>(g[u].x, m, u, t[u]);
        step<1>(g[u].y, m, u, t[u]);
        step<2>(g[u].z, m, u, t[u]);
        step<3>(g[u].w, m, u, t[u]);
      }
    }
    st_rows<NTS>(th, t, ck.len, true, tid);
    if (Rule::kStoreState) {
#pragma unroll
      for (int k = 0; k < K; ++k) st_rows<NTS>(sp[k], m[k], ck.len, true, tid);
    }
    if (in) st_rows<NTS>(in, t, ck.len, aligned16(in), tid);
  }
};

// dst_packed <- R^-1(deq(slot)) inside each chunk: .grad's read of the rotated wire
struct DecodeFp4Rot {
  const uint8_t* slots;
  int c0;
  float* dst;
  uint32_t seed;

  template <bool NTL, int NTS>
  __device__ __forceinline__ void run(const Chunk& ck, int c, void* const*, int, int tid) const {
    __shared__ u32x4 stage[kFp4Vec];
    float4 g[kUnroll];
    fp4_load_rows(slots + size_t(c - c0) * DL_FP4_SLOT_BYTES, stage, tid, g, [] {});
    unrotate_rows(g, seed, tid);
    st_rows<NTS>(dst + ck.poff, g, ck.len, true, tid);
  }
};

}  // namespace

hipError_t launch_delta_fp4_rot(const Launch& L, int inner_slot, const float* outer, float* resid,
                                uint32_t seed, uint8_t* slots) {
  if (resid) return run(L, DeltaFp4Rot<true>{inner_slot, outer, slots, L.c0, resid, seed});
  return run(L, DeltaFp4Rot<false>{inner_slot, outer, slots, L.c0, nullptr, seed});
}

hipError_t launch_unpack_sgd_fp4_rot(const Launch& L, const uint8_t* slots, uint32_t seed,
                                     float* outer, float* mom, SgdArgs a, int inner_slot) {
  return with_sgd_rule(mom, a, [&](auto rule) {
    return run(L, UnpackFp4Rot<decltype(rule)>{slots, L.c0, outer, rule, inner_slot, seed});
  });
}

hipError_t launch_unpack_adamw_fp4_rot(const Launch& L, const uint8_t* slots, uint32_t seed,
                                       float* outer, float* m1, float* m2, AdamArgs a,
                                       int inner_slot) {
  return run(L, UnpackFp4Rot<AdamRule>{slots, L.c0, outer, AdamRule{m1, m2, a}, inner_slot, seed});
}

hipError_t launch_decode_fp4_rot(const Launch& L, const uint8_t* slots, uint32_t seed,
                                 float* dst) {
  return run(L, DecodeFp4Rot{slots, L.c0, dst, seed});
}

}  // namespace dl
