// Device-side pieces of the top-k wire with 4-bit values (dl_topk_fp4.hip): topk_select of
// dl_topk_dev.h picks the entries from the exact fp32 values, then each entry is quantised to an
// E2M1 nibble under a scale shared by its ENTRY group (32 consecutive entries of the slot, the
// fp4 wire's scale and nibble rules of dl_fp4_dev.h) and packed with its 12-bit position into one
// u16. Slot layout and rules are stated in include/diloco_hip.h.
//
// topk_fp4_encode, after the selection has staged value and index at each entry's rank:
//   1. lane e < k takes entry e into registers. An entry group is 32 consecutive lanes of one
//      wave, so its amax is five lane exchanges, no LDS and no barrier; lanes at or past k carry
//      +0 and take part.
//   2. the lane packs index | nibble << 12 into the staged slot and (EF) leaves x - deq at its
//      rank in `err`: the element belongs to the lane that read position i, not to this one.
//   3. one barrier; the owning lanes walk their 16 components again with the ranks the selection
//      left them (topk_walk) and take the error into the register that holds the residual, while
//      the slot leaves as (16 + 2k)/16 gap-free 16-B stores. No dense chunk anywhere.
// Barriers per chunk after the selection: two. Nothing is needed after the last reads: the next
// chunk's selection has at least two barriers ahead of its first write to `err`, the staged slot
// or L.stage.
#pragma once
#include "dl_fp4_dev.h"
#include "dl_topk_dev.h"

namespace dl {
namespace {

static_assert(DL_CHUNK_ELEMS == 4096, "an entry is a 12-bit index | nibble << 12");
static_assert(kThreads == 8 * kFp4Group && DL_TOPK_MAX_K <= kThreads, "eight entry groups of 32 lanes");
static_assert(DL_TOPK_FP4_SLOT_BYTES(DL_TOPK_MIN_K) % 16 == 0, "slots keep 16-B alignment");
constexpr int kTopkFp4Head = 16;  // 8 scale bytes, 8 zero bytes
constexpr int kTopkFp4Vec = DL_TOPK_FP4_SLOT_BYTES(DL_TOPK_MAX_K) / 16;  // 33 16-B pieces at most

// beside TopkLds, which the selection keeps as it is
struct TopkFp4Lds {
  u32x4 slot[kTopkFp4Vec];    // the packed slot
  float err[DL_TOPK_MAX_K];   // x - deq of entry e, at its rank
};

// ROWS as topk_select. EF: the selected components of x become x - deq (the residual), the
// others stay. Every byte of the slot is written.
template <bool ROWS, bool EF, int NTS>
__device__ __forceinline__ void topk_fp4_encode(float4 (&x)[kUnroll], int k, TopkLds& L, TopkFp4Lds& Q,
                                                uint8_t* slot, int tid) {
  TopkRanks<ROWS> R;
  topk_select<ROWS, false>(x, k, L, tid, R);
  __syncthreads();
  const uint32_t* sv = reinterpret_cast<const uint32_t*>(L.stage);
  const uint16_t* si = reinterpret_cast<const uint16_t*>(sv + k);
  const bool live = tid < k;
  const float val = live ? __uint_as_float(sv[tid]) : 0.f;
  const uint32_t idx = live ? uint32_t(si[tid]) : 0u;
  const uint32_t e = fp4_scale(group_umax<kFp4Group>(abs_bits(val)));
  const uint32_t nib = fp4_nibble(val, fp4_up(e));
  uint8_t* q8 = reinterpret_cast<uint8_t*>(Q.slot);
  uint16_t* q16 = reinterpret_cast<uint16_t*>(Q.slot);
  if ((tid & 31) == 0) q8[tid >> 5] = uint8_t(e);  // a group with no entry: amax 0, E = 0
  if ((tid & 31) == 1) q8[8 + (tid >> 5)] = 0;
  if (live) {
    q16[kTopkFp4Head / 2 + tid] = uint16_t(idx | (nib << 12));
    if constexpr (EF) Q.err[tid] = val - fp4_value(nib, fp4_half(e));
  }
  __syncthreads();
  if constexpr (EF)
    topk_walk<ROWS>(x, R, tid, [&](int u, int j, float, uint32_t, uint32_t rank) {
      set_elem(x[u], j, Q.err[rank]);
    });
  if (tid < (DL_TOPK_FP4_SLOT_BYTES(k) >> 4)) {
    const u32x4 v = Q.slot[tid];
    DL_GLOBAL u32x4* q = (DL_GLOBAL u32x4*)slot + tid;
    if constexpr (NTS == kStNT)
      __builtin_nontemporal_store(v, q);
    else
      *q = v;
  }
}

// entry `e` of a slot in global memory, decoded: exact, NaN under an E = 255 group scale
__device__ __forceinline__ TopkEntry topk_fp4_entry(const uint8_t* slot, int e) {
  const DL_GLOBAL uint16_t* q = (const DL_GLOBAL uint16_t*)(slot + kTopkFp4Head);
  const uint32_t w = __builtin_nontemporal_load(q + e);
  const uint32_t sc = __builtin_nontemporal_load((const DL_GLOBAL uint8_t*)slot + (e >> 5));
  return {fp4_value(w >> 12, fp4_half(sc)), w & (DL_CHUNK_ELEMS - 1)};
}

// the 4-bit-value slot as UnpackTopk's codec
struct TopkFp4 {
  static __device__ __forceinline__ size_t slot_bytes(int k) { return size_t(DL_TOPK_FP4_SLOT_BYTES(k)); }
  static __device__ __forceinline__ TopkEntry entry(const uint8_t* slot, int, int e) {
    return topk_fp4_entry(slot, e);
  }
};

}  // namespace
}  // namespace dl
