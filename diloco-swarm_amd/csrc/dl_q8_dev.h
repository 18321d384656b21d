// Device-side pieces of the int8 codec shared by its translation units (dl_q8.hip: the
// pseudo-gradient exchange; dl_q8_grad.hip: the per-step gradient exchange): the quantiser, the
// chunk amax, the slot header and the residual step of error feedback. Slot layout and
// quantiser are stated in dl_q8.hip and include/diloco_hip.h.
#pragma once
#include "dl_device.h"

namespace dl {
namespace {

constexpr int kQ8Header = DL_Q8_SLOT_BYTES - DL_CHUNK_ELEMS;  // 64 B: fp32 scale + padding

__device__ __forceinline__ float block_amax(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));  // 64-lane wave
  __shared__ float part[kThreads / 64];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  v = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
  __syncthreads();  // `part` is reused by the workgroup's next chunk
  return v;
}

__device__ __forceinline__ int q8(float x, float s) {
  if (s == 0.f) return 0;
  const float r = fminf(fmaxf(__builtin_rintf(x / s), -127.f), 127.f);
  return int(r);
}

__device__ __forceinline__ uint32_t pack4(float4 x, float s) {
  return (uint32_t(q8(x.x, s)) & 0xffu) | ((uint32_t(q8(x.y, s)) & 0xffu) << 8) |
         ((uint32_t(q8(x.z, s)) & 0xffu) << 16) | ((uint32_t(q8(x.w, s)) & 0xffu) << 24);
}

__device__ __forceinline__ float4 unpack4(uint32_t w, float s) {
  return make_float4(float(int8_t(w & 0xffu)) * s, float(int8_t((w >> 8) & 0xffu)) * s,
                     float(int8_t((w >> 16) & 0xffu)) * s, float(int8_t(w >> 24)) * s);
}

__device__ __forceinline__ float amax4(float4 x) {
  return fmaxf(fmaxf(fabsf(x.x), fabsf(x.y)), fmaxf(fabsf(x.z), fabsf(x.w)));
}

// The slot header: the scale, then zeros, written whole as four 16-B stores (lanes 0-3) so
// consecutive slots leave as one gap-free stream. A lone 4-B store of the scale left 60 B of
// every 4160 unwritten: the encoder ran 1.1-1.8 % slower cold in three interleaved A/B pairs
// on T1.3B and T125 (profiles/r03_ab_q8_header_*.txt); the zeros match the zero-filled wire.
template <int NTS>
__device__ __forceinline__ void store_header(uint8_t* slot, float s, int tid) {
  if (tid < kQ8Header / 16) {
    const u32x4 w = {tid == 0 ? __float_as_uint(s) : 0u, 0u, 0u, 0u};
    DL_GLOBAL u32x4* h = (DL_GLOBAL u32x4*)slot + tid;
    if constexpr (NTS == kStNT)
      __builtin_nontemporal_store(w, h);
    else
      *h = w;
  }
}

typedef DL_GLOBAL uint32_t* gu32;
typedef DL_GLOBAL const uint32_t* gcu32;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// The residual step of error feedback: what the receiver does not get, x - q·s, with q·s the
// product the unpack kernels decode.
__device__ __forceinline__ float resid1(float x, float s) { return x - float(q8(x, s)) * s; }
__device__ __forceinline__ float4 resid4(float4 x, float s) {
  return make_float4(resid1(x.x, s), resid1(x.y, s), resid1(x.z, s), resid1(x.w, s));
}
__device__ __forceinline__ float4 add4(float4 a, float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

}  // namespace
}  // namespace dl
