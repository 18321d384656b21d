// Device-side pieces of the top-k sparse wire codec of dl_topk.hip: the selection of the k
// largest keys of a chunk inside the workgroup that holds it in registers, the staged slot's
// 16-B stores, the decode of a slot into a dense chunk in LDS, and the fused optimizer pass over
// it (UnpackTopk, shared with the 4-bit-value slot of dl_topk_fp4.hip). Slot layout and rules are
// stated in include/diloco_hip.h. Nothing here rounds: keys are integer views of the values, the
// slot carries the values' own bits.
//
// topk_select, for the 16 values a lane holds (4096 per workgroup, +0 past the chunk's length):
//   1. MSB-first radix select of the k-th largest key, digits of 8 + 8 + 8 + 7 bits. A pass adds
//      the candidates (keys that match the prefix found so far) into a 256-bin histogram with LDS
//      adds, one private histogram per wave: the first digit is the exponent byte, where real
//      gradients pile into a handful of bins and same-address adds serialise -- measured: 64
//      lanes adding into one bin made the encoder 9x slower than the fp4 one. So of the 64 keys
//      an instruction sees, the first kTopkHot distinct digits are counted by ballot and added
//      once by one lane; only what is left adds per lane. After ONE barrier
//      every wave sums the four histograms (four bins per lane, 16-B reads), suffix-scans the 64
//      lane totals, and finds the bin that holds the k-th key and the count above it -- all four
//      waves redundantly, so the result needs no second barrier to travel. The histograms are
//      double-buffered and a wave clears only its own, in program order with its own adds. The
//      passes stop as soon as the bin holds exactly the entries still needed.
//   2. selected = (key & mask) > prefix, plus the first `need` positions in index order with
//      (key & mask) == prefix. Both counts in index order come from ballots: a lane's count of
//      lower lanes (mbcnt) and the wave's total (popcount), the (group, wave) totals through a
//      64-entry LDS table that every wave scans in registers. Index order is rows-then-lanes for
//      the float4-row layout (element 4(u·256 + tid) + j) and element-rows-then-lanes for the
//      4-B-aligned layout (element (4u + j)·256 + tid): ROWS picks the walk.
//   3. An entry is staged in LDS at its rank, value and index; ranks ascend with the index.
// Barriers per chunk: one per digit pass (<= 4), one for the totals table, two around the store.
#pragma once
#include "dl_outer_step.h"
#include "dl_q8_dev.h"

namespace dl {
namespace {

constexpr int kWaves = kThreads / 64;
constexpr int kTopkBins = 256;
constexpr int kTopkHot = 4;  // digits per 64 keys counted by ballot before the per-lane adds
constexpr int kTopkStageVec = DL_TOPK_SLOT_BYTES(DL_TOPK_MAX_K) / 16;  // 96 16-B pieces at most
static_assert(DL_TOPK_MAX_K <= kThreads, "one lane per entry in the decoders");
static_assert(DL_TOPK_MIN_K % 8 == 0 && DL_TOPK_SLOT_BYTES(8) % 16 == 0, "slots keep 16-B alignment");
static_assert(DL_CHUNK_ELEMS <= 65536, "u16 indices");

struct TopkLds {
  uint32_t hist[2][kWaves][kTopkBins];  // double-buffered, one histogram per wave
  uint32_t wtab[64];                    // (group, wave) totals: selected-above << 16 | ties
  u32x4 stage[kTopkStageVec];           // the slot: k values, then k u16 indices
};

__device__ __forceinline__ uint32_t topk_key(float x) { return __float_as_uint(x) & 0x7fffffffu; }
__device__ __forceinline__ uint32_t lanes_below(uint64_t ballot) {
  return __builtin_amdgcn_mbcnt_hi(uint32_t(ballot >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(ballot), 0u));
}
__device__ __forceinline__ uint32_t lane_get(uint32_t v, int lane) {  // lane: wave-uniform
  return uint32_t(__builtin_amdgcn_readlane(int(v), lane));
}
__device__ __forceinline__ float elem(const float4& v, int j) {
  return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w;
}
__device__ __forceinline__ void set_elem(float4& v, int j, float a) {
  if (j == 0) v.x = a;
  else if (j == 1) v.y = a;
  else if (j == 2) v.z = a;
  else v.w = a;
}

// What a selection leaves in a lane's registers for another walk over its 16 components: the
// threshold (prefix under mask, `need` ties taken) and the counts in index order ahead of the
// lane, per (group, wave) in lane g·kWaves + w of `ex`, inside the wave in below[g].
template <bool ROWS>
struct TopkRanks {
  static constexpr int kGroups = ROWS ? kUnroll : 4 * kUnroll;
  uint32_t prefix, mask, need, ex;
  uint32_t below[kGroups];
};

// group g (a row u, or an element row 4u + j) of the lane's components against the threshold:
// R.below[g] <- the lanes below in the wave, the wave's total returned; ties in the low half,
// keys above the threshold in the high half.
template <bool ROWS>
__device__ __forceinline__ uint32_t topk_group_counts(const float4 (&x)[kUnroll], TopkRanks<ROWS>& R, int g) {
  uint32_t b = 0u, tot = 0u;
#pragma unroll
  for (int j = 0; j < (ROWS ? 4 : 1); ++j) {
    const uint32_t m = topk_key(ROWS ? elem(x[g], j) : elem(x[g >> 2], g & 3)) & R.mask;
    const uint64_t bg = __ballot(m > R.prefix), be = __ballot(m == R.prefix);
    b += (lanes_below(bg) << 16) | lanes_below(be);
    tot += (uint32_t(__builtin_popcountll(bg)) << 16) | uint32_t(__builtin_popcountll(be));
  }
  R.below[g] = b;
  return tot;
}

// the lane's components in index order: f(u, j, value, position, rank) for every selected one
// (f may rewrite x[u] component j)
template <bool ROWS, class Fn>
__device__ __forceinline__ void topk_walk(float4 (&x)[kUnroll], const TopkRanks<ROWS>& R, int tid, Fn&& f) {
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
#pragma unroll
  for (int g = 0; g < TopkRanks<ROWS>::kGroups; ++g) {
    uint32_t run = lane_get(R.ex, g * kWaves + w) + R.below[g];
#pragma unroll
    for (int j = 0; j < (ROWS ? 4 : 1); ++j) {
      const int u = ROWS ? g : g >> 2, jj = ROWS ? j : g & 3;
      const float val = elem(x[u], jj);
      const uint32_t m = topk_key(val) & R.mask;
      const uint32_t ties = run & 0xffffu;
      if (m > R.prefix || (m == R.prefix && ties < R.need)) {
        const uint32_t rank = (run >> 16) + (ties < R.need ? ties : R.need);
        f(u, jj, val, uint32_t(ROWS ? 4 * (g * kThreads + tid) + j : g * kThreads + tid), rank);
      }
      run += m > R.prefix ? 0x10000u : m == R.prefix ? 1u : 0u;
    }
  }
}

// x[u] component j is position 4(u·kThreads + tid) + j (ROWS) or (4u + j)·kThreads + tid of the
// chunk. Stages the slot of the k first-ranked positions in L.stage; CLEAR: the selected
// components of x become +0 (the residual). No barrier at the end: topk_store_slot has it. R keeps
// the ranks for a caller that walks the components again (dl_topk_fp4_dev.h).
template <bool ROWS, bool CLEAR>
__device__ __forceinline__ void topk_select(float4 (&x)[kUnroll], int k, TopkLds& L, int tid,
                                            TopkRanks<ROWS>& R) {
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  reinterpret_cast<u32x4*>(L.hist[0][w])[lane] = zero4;
  uint32_t prefix = 0u, mask = 0u, need = uint32_t(k);
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int shift = p == 0 ? 23 : p == 1 ? 15 : p == 2 ? 7 : 0;
    const uint32_t dm = p == 3 ? 0x7fu : 0xffu;
    uint32_t* own = L.hist[p & 1][w];
    __builtin_amdgcn_wave_barrier();  // the clears above stay ahead of the adds
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t key = topk_key(elem(x[u], j));
        const uint32_t d = (key >> shift) & dm;
        bool cand = (key & mask) == prefix;
        uint64_t rem = __ballot(cand);
#pragma unroll
        for (int it = 0; it < kTopkHot; ++it) {  // a hot bin: one add of the wave's count
          if (rem == 0) break;
          const int leader = __builtin_ctzll(rem);
          const uint32_t d0 = lane_get(d, leader);
          const uint64_t same = __ballot(cand && d == d0);
          if (lane == leader) atomicAdd(&own[d0], uint32_t(__builtin_popcountll(same)));
          rem &= ~same;
          cand = cand && d != d0;
        }
        if (cand) atomicAdd(&own[d], 1u);
      }
    }
    __syncthreads();
    u32x4 c = zero4;
#pragma unroll
    for (int ww = 0; ww < kWaves; ++ww) c += reinterpret_cast<const u32x4*>(L.hist[p & 1][ww])[lane];
    // the other buffer was last read before this pass's barrier: this wave's part is free
    reinterpret_cast<u32x4*>(L.hist[(p + 1) & 1][w])[lane] = zero4;
    const uint32_t t = c.x + c.y + c.z + c.w;
    uint32_t s = t;  // inclusive suffix sum over the lanes: the candidates in bins >= 4·lane
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t v = uint32_t(__shfl_down(int(s), o, 64));
      if (lane + o < 64) s += v;
    }
    // the highest lane whose suffix still reaches `need` holds the bin of the k-th key
    const int ls = 63 - __builtin_clzll(__ballot(s >= need));
    uint32_t a = s - t, cnt = c.w;
    int bin = 3;
    if (a + cnt < need) a += cnt, bin = 2, cnt = c.z;  // downwards from the lane's top bin
    if (bin == 2 && a + cnt < need) a += cnt, bin = 1, cnt = c.y;
    if (bin == 1 && a + cnt < need) a += cnt, bin = 0, cnt = c.x;
    const uint32_t above = lane_get(a, ls);
    prefix |= (uint32_t(4 * ls) + lane_get(uint32_t(bin), ls)) << shift;
    mask |= dm << shift;
    need -= above;
    if (lane_get(cnt, ls) == need) break;  // every candidate left is taken
  }

  // counts in index order: per group (a row u, or an element row 4u + j) the lanes below and the
  // wave's total, ties in the low half, keys above the threshold in the high half
  constexpr int kGroups = TopkRanks<ROWS>::kGroups;
  R.prefix = prefix, R.mask = mask, R.need = need;
#pragma unroll
  for (int g = 0; g < kGroups; ++g) {
    const uint32_t tot = topk_group_counts<ROWS>(x, R, g);
    if (lane == 0) L.wtab[g * kWaves + w] = tot;
  }
  __syncthreads();
  const uint32_t tv = lane < kGroups * kWaves ? L.wtab[lane] : 0u;
  uint32_t ex = tv;  // exclusive prefix over (group, wave), every wave for itself
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t v = uint32_t(__shfl_up(int(ex), o, 64));
    if (lane >= o) ex += v;
  }
  R.ex = ex - tv;
  uint32_t* sv = reinterpret_cast<uint32_t*>(L.stage);
  uint16_t* si = reinterpret_cast<uint16_t*>(sv + k);
  topk_walk<ROWS>(x, R, tid, [&](int u, int j, float val, uint32_t pos, uint32_t rank) {
    sv[rank] = __float_as_uint(val);
    si[rank] = uint16_t(pos);
    if constexpr (CLEAR) set_elem(x[u], j, 0.f);
  });
}
template <bool ROWS, bool CLEAR>
__device__ __forceinline__ void topk_select(float4 (&x)[kUnroll], int k, TopkLds& L, int tid) {
  TopkRanks<ROWS> R;
  topk_select<ROWS, CLEAR>(x, k, L, tid, R);
}

// the staged slot leaves as 6k/16 gap-free 16-B stores; the barriers order the staging before
// it and the reuse of the LDS by the workgroup's next chunk after it
template <int NTS>
__device__ __forceinline__ void topk_store_slot(const TopkLds& L, uint8_t* slot, int k, int tid) {
  __syncthreads();
  if (tid < (DL_TOPK_SLOT_BYTES(k) >> 4)) {
    const u32x4 v = L.stage[tid];
    DL_GLOBAL u32x4* q = (DL_GLOBAL u32x4*)slot + tid;
    if constexpr (NTS == kStNT)
      __builtin_nontemporal_store(v, q);
    else
      *q = v;
  }
  __syncthreads();
}

// entry `e` of a slot in global memory: its value and its position in the chunk (modulo the
// chunk, so no byte pattern reaches outside the dense chunk)
struct TopkEntry {
  float val;
  uint32_t idx;
};
__device__ __forceinline__ TopkEntry topk_entry(const uint8_t* slot, int k, int e) {
  const DL_GLOBAL float* v = (const DL_GLOBAL float*)slot;
  const DL_GLOBAL uint16_t* i = (const DL_GLOBAL uint16_t*)(slot + 4 * k);
  return {__builtin_nontemporal_load(v + e), uint32_t(__builtin_nontemporal_load(i + e)) & (DL_CHUNK_ELEMS - 1)};
}

// the exact-value top-k slot as UnpackTopk's codec
struct TopkF32 {
  static __device__ __forceinline__ size_t slot_bytes(int k) { return size_t(DL_TOPK_SLOT_BYTES(k)); }
  static __device__ __forceinline__ TopkEntry entry(const uint8_t* slot, int k, int e) {
    return topk_entry(slot, k, e);
  }
};

// a4 + a5 from the averaged top-k slots under either rule (SgdRule<MODE>, AdamRule of
// dl_outer_step.h: the arithmetic of dl_unpack_sgd / dl_unpack_adamw). The slot's entries are
// loaded (one per lane, non-temporal) ahead of the loads of θ and the state, scattered into the
// zeroed dense chunk in LDS, and every lane takes its rows of the gradient from it; the rule
// runs on every element inside the chunk (a zero gradient still decays momentum) and the stores
// leave one stream at a time: θ, the state, inner. Codec (TopkF32; TopkFp4 of
// dl_topk_fp4_dev.h) is the slot's size and the decode of one entry: the only place the two
// top-k wires differ here.
template <class Rule, class Codec>
struct UnpackTopk {
  static constexpr int K = Rule::kStates;
  const uint8_t* slots;
  int c0;
  float* outer;
  Rule rule;
  int inner_slot;
  int k;

  template <int J>
  __device__ __forceinline__ void step(float g, float4 (&m)[K][kUnroll], int u, float4& t) const {
    float e[K];
#pragma unroll
    for (int s = 0; s < K; ++s) e[s] = Rule::kLoadState ? comp<J>(m[s][u]) : 0.f;
    rule.apply(g, e, comp<J>(t));
#pragma unroll
    for (int s = 0; s < K; ++s) comp<J>(m[s][u]) = e[s];
  }

  template <bool NTL, int NTS>
  __device__ __forceinline__ void run(const Chunk& ck, int c, void* const* caddr, int nchunk, int tid) const {
    __shared__ float4 dense4[DL_CHUNK_ELEMS / 4];
    float* dense = reinterpret_cast<float*>(dense4);
    float* in = inner_slot >= 0 ? slot_ptr<float>(caddr, nchunk, inner_slot, c) : nullptr;
    const uint8_t* slot = slots + size_t(c - c0) * Codec::slot_bytes(k);
    float* th = outer + ck.poff;
    float* sp[K];
#pragma unroll
    for (int s = 0; s < K; ++s) sp[s] = rule.state(s) + ck.poff;
    auto one = [&](int i, float g) {
      float t1 = th[i];
      float e[K];
#pragma unroll
      for (int s = 0; s < K; ++s) e[s] = Rule::kLoadState ? sp[s][i] : 0.f;
      rule.apply(g, e, t1);
      th[i] = t1;
      if (Rule::kStoreState) {
#pragma unroll
        for (int s = 0; s < K; ++s) sp[s][i] = e[s];
      }
      if (in) in[i] = t1;
    };
    TopkEntry en = {0.f, 0u};
    if (tid < k) en = Codec::entry(slot, k, tid);
    const bool rows = in == nullptr || aligned16(in);
    const int nv = ck.len >> 2;
    float4 t[kUnroll], m[K][kUnroll], g[kUnroll];
    if (rows) {
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int v = u * kThreads + tid;
        if (v < nv) {
          t[u] = ldf4<NTL>(th, v);
          if (Rule::kLoadState) {
#pragma unroll
            for (int s = 0; s < K; ++s) m[s][u] = ldf4<NTL>(sp[s], v);
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) dense4[u * kThreads + tid] = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    if (tid < k) dense[en.idx] = en.val;
    __syncthreads();
    if (rows) {
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) g[u] = dense4[u * kThreads + tid];
      const int i = (nv << 2) + tid;  // the < 4 elements past the last float4, one per lane
      const float gt = i < ck.len ? dense[i] : 0.f;
      __syncthreads();  // the dense chunk is reused by the workgroup's next chunk
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        if (u * kThreads + tid < nv) {
          step<0>(g[u].x, m, u, t[u]);
          step<1>(g[u].y, m, u, t[u]);
          step<2>(g[u].z, m, u, t[u]);
          step<3>(g[u].w, m, u, t[u]);
        }
      }
      store_rows<NTS>(th, t, nv, tid);
      if (Rule::kStoreState) {
#pragma unroll
        for (int s = 0; s < K; ++s) store_rows<NTS>(sp[s], m[s], nv, tid);
      }
      if (in) store_rows<NTS>(in, t, nv, tid);
      if (i < ck.len) one(i, gt);
    } else {
      for (int i = tid; i < ck.len; i += kThreads) one(i, dense[i]);
      __syncthreads();
    }
  }
};

}  // namespace
}  // namespace dl
