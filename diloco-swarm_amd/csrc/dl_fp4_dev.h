// Device-side pieces of the 4-bit (MXFP4) wire codec of dl_fp4.hip: the group scale, the element
// quantiser, the decoder, and the two movements every kernel shares -- float4 rows -> a whole
// slot staged in LDS -> 136 gap-free 16-B stores, and a slot -> LDS -> the rows' nibbles and
// scales. Slot layout and rules are stated in include/diloco_hip.h. Everything is plain
// integer / compare C++: the scale is a power of two, so the only roundings are the compares
// of the quantiser; decoding is exact.
#pragma once
#include "dl_q8_dev.h"

namespace dl {
namespace {

constexpr int kFp4Group = 32;                            // elements per scale byte
constexpr int kFp4Scales = DL_CHUNK_ELEMS / kFp4Group;   // 128 scale bytes, then the payload
constexpr int kFp4Vec = DL_FP4_SLOT_BYTES / 16;          // 136 16-B pieces per slot
static_assert(kFp4Scales + DL_CHUNK_ELEMS / 2 == DL_FP4_SLOT_BYTES, "fp4 slot layout");
static_assert(DL_FP4_SLOT_BYTES % 64 == 0 && kFp4Vec <= kThreads, "fp4 slot layout");

__device__ __forceinline__ uint32_t abs_bits(float x) { return __float_as_uint(x) & 0x7fffffffu; }
__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint32_t abs_bits4(float4 x) {
  return umax(umax(abs_bits(x.x), abs_bits(x.y)), umax(abs_bits(x.z), abs_bits(x.w)));
}
// the maximum over the `lanes` (8 or 32) consecutive lanes of a group: no LDS, no barrier
template <int LANES>
__device__ __forceinline__ uint32_t group_umax(uint32_t a) {
#pragma unroll
  for (int o = 1; o < LANES; o <<= 1) a = umax(a, uint32_t(__shfl_xor(int(a), o, 64)));
  return a;
}

// E of a group from A = max |x| as bits. amax = m·2^k, m in [0.5, 1): k = exp - 126 and
// m <= 0.75 is mantissa <= 0x400000, so e + 127 = exp - 2 (+ 1 above 0.75): the smallest scale
// with amax·2^-e <= 6. A denormal or zero amax has exp = 0 and clamps to E = 0.
__device__ __forceinline__ uint32_t fp4_scale(uint32_t a) {
  if (a >= 0x7f800000u) return 255u;
  const int e = int(a >> 23) - 2 + ((a & 0x7fffffu) > 0x400000u ? 1 : 0);
  return uint32_t(e > 0 ? e : 0);
}
// 2^(127 - E), the factor of the quantiser; 0 for a non-finite group (every compare is then
// false or the product NaN: code 0)
__device__ __forceinline__ float fp4_up(uint32_t e) {
  return e == 255u ? 0.f : __uint_as_float((254u - e) << 23);
}
// 2^(E - 128), half the scale (the decoder multiplies 2·grid by it); NaN for E = 255
__device__ __forceinline__ float fp4_half(uint32_t e) {
  if (e == 255u) return __uint_as_float(0x7fc00000u);
  return __uint_as_float(e >= 2u ? (e - 1u) << 23 : 0x00200000u << e);
}

// sign << 3 | code: the grid point nearest |x|·up, ties to the even code (0.25 -> 0, 0.75 -> 1,
// 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4); no sign on code 0
__device__ __forceinline__ uint32_t fp4_nibble(float x, float up) {
  const float y = fabsf(x) * up;
  const uint32_t code = uint32_t(y > 0.25f) + uint32_t(y >= 0.75f) + uint32_t(y > 1.25f) +
                        uint32_t(y >= 1.75f) + uint32_t(y > 2.5f) + uint32_t(y >= 3.5f) +
                        uint32_t(y > 5.f);
  return code | (code != 0u ? (__float_as_uint(x) >> 28) & 8u : 0u);
}
__device__ __forceinline__ uint32_t fp4_pack4(float4 x, float up) {
  return fp4_nibble(x.x, up) | (fp4_nibble(x.y, up) << 4) | (fp4_nibble(x.z, up) << 8) |
         (fp4_nibble(x.w, up) << 12);
}
// ±grid[code]·2^(E-127) as (±2·grid[code]) · half: one exact multiply (2·grid as 4-bit integers)
__device__ __forceinline__ float fp4_value(uint32_t nib, float half) {
  const int t = int((0xC8643210u >> ((nib & 7u) * 4u)) & 15u);
  return float((nib & 8u) ? -t : t) * half;
}
__device__ __forceinline__ float4 fp4_unpack4(uint32_t w, float half) {
  return make_float4(fp4_value(w, half), fp4_value(w >> 4, half), fp4_value(w >> 8, half),
                     fp4_value(w >> 12, half));
}

// Rows -> slot. x[u] holds elements [4v, 4v + 4) of the chunk, v = u·kThreads + tid, +0 past the
// chunk's length, so a group is the 8 consecutive lanes of one row. Every byte of `st` (the
// slot, in LDS) is written. EF: x[u] <- x[u] - deq, the residual.
template <bool EF>
__device__ __forceinline__ void fp4_encode_rows(float4 (&x)[kUnroll], uint8_t* st, int tid) {
  uint16_t* st16 = reinterpret_cast<uint16_t*>(st);
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) {
    const int v = u * kThreads + tid;
    const uint32_t e = fp4_scale(group_umax<8>(abs_bits4(x[u])));
    const uint32_t w = fp4_pack4(x[u], fp4_up(e));
    st16[kFp4Scales / 2 + v] = uint16_t(w);
    if ((tid & 7) == 0) st[v >> 3] = uint8_t(e);
    if constexpr (EF) {
      const float4 d = fp4_unpack4(w, fp4_half(e));
      x[u] = sub4(x[u], d);
    }
  }
}

// the staged slot leaves as 136 gap-free 16-B stores (the finding at store_header, dl_q8_dev.h);
// the barriers order the staging before it and the reuse of `st` by the next chunk after it
template <int NTS>
__device__ __forceinline__ void fp4_store_slot(const u32x4* st, uint8_t* slot, int tid) {
  __syncthreads();
  if (tid < kFp4Vec) {
    const u32x4 w = st[tid];
    DL_GLOBAL u32x4* q = (DL_GLOBAL u32x4*)slot + tid;
    if constexpr (NTS == kStNT)
      __builtin_nontemporal_store(w, q);
    else
      *q = w;
  }
  __syncthreads();
}

// one element straight from a slot in global memory (the element-wise paths)
__device__ __forceinline__ float fp4_load1(const uint8_t* slot, int i) {
  const uint32_t b = slot[kFp4Scales + (i >> 1)];
  return fp4_value((i & 1) ? b >> 4 : b, fp4_half(slot[i >> 5]));
}

}  // namespace
}  // namespace dl
