// All-gather exchange of the top-k wires on the per-step DP gradient sync: every peer receives
// every peer's slots and sums them itself, so the selection runs once (in the encoder), nothing is
// selected again and there is no second residual.
//   dl_gather_topk[_fp4]          the encoders of dl_topk_grad.hip, unchanged
//   all_gather_into_tensor        gathered = [peer][slot]
//   dl_unpack_avg_topk[_fp4]_ag   .grad <- (Σ_r decode_r) / n, optionally partials[c] = Σ of the
//                                 stored values²
// The front end is TopkAgBarriers of dl_topk_ag_dev.h: the rank-ordered sparse sum into the dense
// chunk in LDS, one barrier per peer. Peer 0's entry loads are issued first; after the sum a lane
// reads its float4 rows back and divides by float(n) when n > 1 (IEEE division, as div4). The
// dense chunk is the only large LDS. Compiled as dl_topk.hip is, without packed fp32 instructions.
#include "dl_norm_dev.h"
#include "dl_topk_ag_dev.h"

namespace dl {
namespace {

// Write-only: dst <- g inside the chunk, nothing past its length; dst is the bound tensor slot (a
// gradient, 4-B or 16-B aligned). SUM: partials[c] = the chunk's Σ of the stored values² in
// dl_norm.hip's order (rows, tail element, block_sum), as UnpackAvgTopk leaves it.
template <class Walk, bool SUM>
struct UnpackAvgTopkAg {
  TopkAgSrc src;
  int dst_slot;
  double* partials;

  template <bool NTL, int NTS>
  __device__ __forceinline__ void run(const Chunk& ck, int c, void* const* caddr, int nchunk, int tid) const {
    __shared__ float4 dense4[DL_CHUNK_ELEMS / 4];
    const float* dense = reinterpret_cast<const float*>(dense4);
    float* dst = slot_ptr<float>(caddr, nchunk, dst_slot, c);
    const int nv = ck.len >> 2;
    Walk walk;
    walk.begin(src, c, tid);
    walk.sum(src, dense4, tid);
    float4 g[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) g[u] = dense4[u * kThreads + tid];
    const int i = (nv << 2) + tid;  // the < 4 elements past the last float4, one per lane
    float gt = i < ck.len ? dense[i] : 0.f;
    __syncthreads();  // the dense chunk is reused by the workgroup's next chunk
    if (src.n_peers > 1) {
      const float d = float(src.n_peers);
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) g[u] = div4(g[u], d);
      gt = gt / d;
    }
    if (aligned16(dst)) {
      store_rows<NTS>(dst, g, nv, tid);
    } else {
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int v = u * kThreads + tid;
        if (v < nv) {
          dst[4 * v] = g[u].x;
          dst[4 * v + 1] = g[u].y;
          dst[4 * v + 2] = g[u].z;
          dst[4 * v + 3] = g[u].w;
        }
      }
    }
    if (i < ck.len) dst[i] = gt;
    if constexpr (SUM) {
      double acc = sumsq_rows(g, nv, tid);
      if (i < ck.len) sq1(acc, gt);
      acc = block_sum(acc, tid);
      if (tid == 0) partials[c] = acc;
    }
  }
};

#ifdef DL_TUNING
bool g_ag_waves = false;  // dl_tune_topk_ag_form: the measured alternative
#endif

template <class Walk>
hipError_t unpack_avg_ag(const Launch& L, const TopkAgSrc& src, int dst_slot, double* partials) {
  if (partials) return run(L, UnpackAvgTopkAg<Walk, true>{src, dst_slot, partials});
  return run(L, UnpackAvgTopkAg<Walk, false>{src, dst_slot, nullptr});
}

template <class Codec>
hipError_t unpack_avg_ag(const Launch& L, const uint8_t* gathered, int n_peers, int peer_stride,
                         int k, int dst_slot, double* partials) {
  const TopkAgSrc src{gathered, L.c0, n_peers, peer_stride, k};
#ifdef DL_TUNING
  if (g_ag_waves) return unpack_avg_ag<TopkAgWaves<Codec>>(L, src, dst_slot, partials);
#endif
  return unpack_avg_ag<TopkAgBarriers<Codec>>(L, src, dst_slot, partials);
}

}  // namespace

#ifdef DL_TUNING
void set_topk_ag_form(int waves) { g_ag_waves = waves != 0; }
bool topk_ag_form_waves() { return g_ag_waves; }
#endif

hipError_t launch_unpack_avg_topk_ag(const Launch& L, const uint8_t* gathered, int n_peers,
                                     int peer_stride, int k, int dst_slot, double* partials) {
  return unpack_avg_ag<TopkF32>(L, gathered, n_peers, peer_stride, k, dst_slot, partials);
}

hipError_t launch_unpack_avg_topk_fp4_ag(const Launch& L, const uint8_t* gathered, int n_peers,
                                         int peer_stride, int k, int dst_slot, double* partials) {
  return unpack_avg_ag<TopkFp4>(L, gathered, n_peers, peer_stride, k, dst_slot, partials);
}

}  // namespace dl
