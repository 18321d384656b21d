// Device-side pieces of the rotated fp4 wire (dl_fp4_rot.hip): the sign hash, the 256-point
// Hadamard butterfly of one wavefront's float4 row, and the row loads / stores that serve a
// 16-B-aligned and a 4-B-aligned tensor in the same register layout. The transform is stated in
// include/diloco_hip.h. Lane `tid` of row u holds elements [4v, 4v + 4), v = u·kThreads + tid, so
// a 256-element block is the row of ONE wave: stages 0-1 work on the four components of a lane,
// stages 2-7 exchange with lane ^ 1 ... lane ^ 32. No LDS, no barrier; every lane of the wave
// must be active (the callers run it outside any divergent branch).
#pragma once
#include "dl_fp4_dev.h"

namespace dl {
namespace {

constexpr float kRotNorm = 0.0625f;  // 1 / sqrt(256), exact

// the sign of chunk position i under `seed` as a sign-bit mask
__device__ __forceinline__ uint32_t rot_sign(uint32_t i, uint32_t seed) {
  uint32_t h = (i + seed) * 0x9E3779B1u;
  h ^= h >> 15;
  h *= 0x85EBCA77u;
  h ^= h >> 13;
  h *= 0xC2B2AE3Du;
  h ^= h >> 16;
  return h & 0x80000000u;
}
__device__ __forceinline__ float rot_flip1(float x, uint32_t i, uint32_t seed) {
  return __uint_as_float(__float_as_uint(x) ^ rot_sign(i, seed));
}
// row v of the chunk: positions [4v, 4v + 4)
__device__ __forceinline__ float4 rot_flip4(float4 x, int v, uint32_t seed) {
  const uint32_t i = uint32_t(v) << 2;
  return make_float4(rot_flip1(x.x, i, seed), rot_flip1(x.y, i + 1, seed),
                     rot_flip1(x.z, i + 2, seed), rot_flip1(x.w, i + 3, seed));
}

// The value lane ^ M of the wave holds. Each distance takes the cheapest vector move gfx950 has
// for it: DPP quad_perm (1, 2) and row_ror:8 (8; a rotation by 8 in a row of 16 is xor 8), which
// the compiler folds into the add that follows; ds_swizzle in bit mode (4); and the row / half
// swaps v_permlane16_swap and v_permlane32_swap (16, 32), which hand back both halves of the
// exchange: with the value in both operands, the lane whose bit is clear finds its partner in
// the second result, the other in the first.
template <int M>
__device__ __forceinline__ float lane_xor(float x, int lane) {
  const int v = __float_as_int(x);
  int r;
  if constexpr (M == 1) {
    r = __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xf, 0xf, true);  // quad_perm:[1,0,3,2]
  } else if constexpr (M == 2) {
    r = __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xf, 0xf, true);  // quad_perm:[2,3,0,1]
  } else if constexpr (M == 4) {
    r = __builtin_amdgcn_ds_swizzle(v, 0x101F);  // and 0x1f, or 0, xor 4
  } else if constexpr (M == 8) {
    r = __builtin_amdgcn_update_dpp(v, v, 0x128, 0xf, 0xf, true);  // row_ror:8
  } else if constexpr (M == 16) {
    const auto p = __builtin_amdgcn_permlane16_swap(uint32_t(v), uint32_t(v), false, false);
    r = int((lane & 16) ? p[0] : p[1]);
  } else {
    static_assert(M == 32, "a wave has 64 lanes");
    const auto p = __builtin_amdgcn_permlane32_swap(uint32_t(v), uint32_t(v), false, false);
    r = int((lane & 32) ? p[0] : p[1]);
  }
  return __int_as_float(r);
}

// one stage across lanes: the lane whose bit is clear takes own + partner, the other
// partner - own, written partner + (-own): one sign xor and one add, the same bits
template <int M>
__device__ __forceinline__ void rot_stage(float4& x, int lane) {
  const uint32_t neg = (lane & M) ? 0x80000000u : 0u;
  const float4 p = make_float4(lane_xor<M>(x.x, lane), lane_xor<M>(x.y, lane),
                               lane_xor<M>(x.z, lane), lane_xor<M>(x.w, lane));
  x.x = p.x + __uint_as_float(__float_as_uint(x.x) ^ neg);
  x.y = p.y + __uint_as_float(__float_as_uint(x.y) ^ neg);
  x.z = p.z + __uint_as_float(__float_as_uint(x.z) ^ neg);
  x.w = p.w + __uint_as_float(__float_as_uint(x.w) ^ neg);
}

// the eight stages in order and the normalisation: H·x / 16 of one row
__device__ __forceinline__ float4 hadamard_row(float4 x, int tid) {
  const int lane = tid & 63;
  float4 a = make_float4(x.x + x.y, x.x - x.y, x.z + x.w, x.z - x.w);  // stage 0
  a = make_float4(a.x + a.z, a.y + a.w, a.x - a.z, a.y - a.w);         // stage 1
  rot_stage<1>(a, lane);
  rot_stage<2>(a, lane);
  rot_stage<4>(a, lane);
  rot_stage<8>(a, lane);
  rot_stage<16>(a, lane);
  rot_stage<32>(a, lane);
  return make_float4(a.x * kRotNorm, a.y * kRotNorm, a.z * kRotNorm, a.w * kRotNorm);
}

// R and R^-1 over the chunk's rows, in place
__device__ __forceinline__ void rotate_rows(float4 (&x)[kUnroll], uint32_t seed, int tid) {
#pragma unroll
  for (int u = 0; u < kUnroll; ++u)
    x[u] = hadamard_row(rot_flip4(x[u], u * kThreads + tid, seed), tid);
}
__device__ __forceinline__ void unrotate_rows(float4 (&y)[kUnroll], uint32_t seed, int tid) {
#pragma unroll
  for (int u = 0; u < kUnroll; ++u)
    y[u] = rot_flip4(hadamard_row(y[u], tid), u * kThreads + tid, seed);
}

// Row v of a stream of `len` elements: one 16-B load where the stream is 16-B aligned (vec)
// and the row lies inside it, else its elements one by one, +0 at and past the length.
template <bool NTL>
__device__ __forceinline__ float4 ld_row(const float* p, int v, int len, bool vec) {
  if (vec && v < (len >> 2)) return ldf4<NTL>(p, v);
  float e[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) e[j] = 4 * v + j < len ? p[4 * v + j] : 0.f;
  return make_float4(e[0], e[1], e[2], e[3]);
}
// The chunk's rows to one stream, back to back (store_rows); nothing at or past the length.
template <int NTS>
__device__ __forceinline__ void st_rows(float* p, const float4 (&x)[kUnroll], int len, bool vec,
                                        int tid) {
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) {
    const int v = u * kThreads + tid;
    if (vec && v < (len >> 2)) {
      stf4<NTS>(p, v, x[u]);
    } else {
      const float e[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (4 * v + j < len) p[4 * v + j] = e[j];
    }
  }
}

// fp4_encode_rows with the rows replaced by the values the slot decodes to
__device__ __forceinline__ void fp4_encode_rows_deq(float4 (&y)[kUnroll], uint8_t* st, int tid) {
  uint16_t* st16 = reinterpret_cast<uint16_t*>(st);
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) {
    const int v = u * kThreads + tid;
    const uint32_t e = fp4_scale(group_umax<8>(abs_bits4(y[u])));
    const uint32_t w = fp4_pack4(y[u], fp4_up(e));
    st16[kFp4Scales / 2 + v] = uint16_t(w);
    if ((tid & 7) == 0) st[v >> 3] = uint8_t(e);
    y[u] = fp4_unpack4(w, fp4_half(e));
  }
}

// A slot through LDS into the rows' decoded values (UnpackFp4's movement): 136 non-temporal
// 16-B loads, then every lane takes its rows' 16 payload bits and scale byte. `issue` runs
// between the slot's loads and the first barrier: the caller's own global loads.
template <class Issue>
__device__ __forceinline__ void fp4_load_rows(const uint8_t* slot, u32x4* stage, int tid,
                                              float4 (&g)[kUnroll], Issue&& issue) {
  u32x4 qv = {0u, 0u, 0u, 0u};
  if (tid < kFp4Vec) qv = __builtin_nontemporal_load((const DL_GLOBAL u32x4*)slot + tid);
  issue();
  if (tid < kFp4Vec) stage[tid] = qv;
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
  __syncthreads();  // `stage` is reused by the workgroup's next chunk
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) g[u] = fp4_unpack4(w[u], fp4_half(sc[u]));
}

}  // namespace
}  // namespace dl
