// Device-side front end of the all-gather exchange of the top-k wires (dl_topk_ag.hip): the
// rank-ordered sparse sum of n peers' slots of one chunk into the dense 16-KiB chunk in LDS,
// written once over the codecs of dl_topk_dev.h (TopkF32) and dl_topk_fp4_dev.h (TopkFp4).
// Layout and arithmetic are stated in include/diloco_hip.h.
//
// acc = +0 over the chunk; for r = 0 .. n-1 in that order every entry (value, position) of peer
// r's slot does acc[pos] = acc[pos] + value, one rounded fp32 add. The one precondition is that a
// slot's positions are distinct, so no two lanes of an instruction meet at one address -- but in
// the all-zero slot, whose k entries are (+0, 0): every lane stores acc[0] + 0 = acc[0], the same
// bits. A slot that repeats a position otherwise is not a valid slot: which of the colliding adds
// lands is unspecified, and nothing leaves the dense chunk.
//
// Two forms, each measured in both kernels that use them: the write-only gradient decoder of
// dl_topk_ag.hip (tools/topk_ag_bench.py, profiles/topk_ag_t125.json) and the outer step of
// dl_topk_ag_outer.hip (tools/topk_ag_outer_bench.py, profiles/topk_ag_outer_t125.json). The
// product library holds one form per kernel, the tuning build both (dl_tune_topk_ag_form).
//   TopkAgBarriers  the gradient decoder's. One lane per entry, one workgroup barrier per peer, the next
//                   peer's entry loaded ahead of the add: dl_topk_reduce's accumulate loop.
//                   n + 1 barriers per chunk, one entry load per lane and peer.
//   TopkAgWaves     the outer step's. No barrier between peers: the dense chunk is cut into
//                   kWaves quarters of 1024 positions and wave w alone zeroes, reads and writes
//                   quarter w; every wave walks every peer's k entries itself (k/64 <= 4 per
//                   lane) and adds only those whose position lies in its quarter, whatever their
//                   order in the slot; peers stay ordered by the wave's program order (LDS
//                   operations of one wave complete in issue order), and one barrier at the end
//                   publishes the quarters. kWaves times the entry loads, and up to eight entries
//                   in a lane's registers. In the gradient decoder it was 10 us slower at n = 2
//                   and at n = 8: with nothing else in flight that kernel waits on the entry
//                   loads, not on the barriers. In the outer step the dense rows of θ and the
//                   state are in flight behind the entry loads and every barrier holds all four
//                   waves until the slowest has its entries: there it is level at n = 2 and 12 us
//                   faster for SGD at n = 8, at the same occupancy.
#pragma once
#include "dl_topk_fp4_dev.h"

namespace dl {
namespace {

// where the peers' slots of a launch lie: slot of chunk c from peer r at
// gathered + (r * peer_stride + (c - c0)) * Codec::slot_bytes(k)
struct TopkAgSrc {
  const uint8_t* gathered;
  int c0;
  int n_peers;
  int peer_stride;  // in slots
  int k;
};

template <class Codec>
struct TopkAgBarriers {
  TopkEntry en;
  const uint8_t* slot;  // peer r's slot of the chunk
  size_t step;          // bytes from a peer's slot to the next peer's

  // peer 0's entries: issued ahead of everything else the caller does
  __device__ __forceinline__ void begin(const TopkAgSrc& S, int c, int tid) {
    const size_t sb = Codec::slot_bytes(S.k);
    slot = S.gathered + size_t(c - S.c0) * sb;
    step = size_t(S.peer_stride) * sb;
    en = {0.f, 0u};
    if (tid < S.k) en = Codec::entry(slot, S.k, tid);
  }

  // dense <- the sum; ends with the barrier after which every lane may read any position
  __device__ __forceinline__ void sum(const TopkAgSrc& S, float4* dense4, int tid) {
    float* dense = reinterpret_cast<float*>(dense4);
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) dense4[u * kThreads + tid] = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    for (int r = 0; r < S.n_peers; ++r) {  // rank order: the sum is identical on every peer
      TopkEntry nx = {0.f, 0u};
      slot += step;
      if (r + 1 < S.n_peers && tid < S.k) nx = Codec::entry(slot, S.k, tid);
      if (tid < S.k) dense[en.idx] = dense[en.idx] + en.val;
      __syncthreads();
      en = nx;
    }
  }
};

constexpr int kAgQuarter = DL_CHUNK_ELEMS / kWaves;  // positions a wave owns
constexpr int kAgPerLane = DL_TOPK_MAX_K / 64;        // entries of one slot a lane walks at most
static_assert(kAgQuarter % (4 * 64) == 0, "a wave zeroes its quarter in float4 rows");

template <class Codec>
struct TopkAgWaves {
  TopkEntry en[kAgPerLane];
  const uint8_t* slot;
  size_t step;

  __device__ __forceinline__ void load(const TopkAgSrc& S, int lane) {
#pragma unroll
    for (int i = 0; i < kAgPerLane; ++i) {
      en[i] = {0.f, ~0u};  // past the slot's k entries: a position in no wave's quarter
      if (64 * i + lane < S.k) en[i] = Codec::entry(slot, S.k, 64 * i + lane);
    }
  }

  __device__ __forceinline__ void begin(const TopkAgSrc& S, int c, int tid) {
    const size_t sb = Codec::slot_bytes(S.k);
    slot = S.gathered + size_t(c - S.c0) * sb;
    step = size_t(S.peer_stride) * sb;
    load(S, tid & 63);
  }

  __device__ __forceinline__ void sum(const TopkAgSrc& S, float4* dense4, int tid) {
    float* dense = reinterpret_cast<float*>(dense4);
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t lo = uint32_t(w * kAgQuarter);
#pragma unroll
    for (int u = 0; u < kAgQuarter / (4 * 64); ++u)
      dense4[w * (kAgQuarter / 4) + u * 64 + lane] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int r = 0; r < S.n_peers; ++r) {
      TopkEntry cur[kAgPerLane];
#pragma unroll
      for (int i = 0; i < kAgPerLane; ++i) cur[i] = en[i];
      if (r + 1 < S.n_peers) {
        slot += step;
        load(S, lane);
      }
      // the zeroes and the previous peer's adds of this wave are ahead of these in LDS order
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int i = 0; i < kAgPerLane; ++i)
        if (64 * i < S.k && cur[i].idx - lo < uint32_t(kAgQuarter))
          dense[cur[i].idx] = dense[cur[i].idx] + cur[i].val;
    }
    __syncthreads();
  }
};

}  // namespace
}  // namespace dl
