// The outer step on the gathered top-k slots: the all-gather exchange of dl_topk_ag.hip under the
// rules of dl_outer_step.h, so the outer exchange selects once, runs one collective and has no
// reduce kernel and no second residual.
//   dl_delta_topk[_fp4]              the encoders of dl_topk.hip / dl_topk_fp4.hip, unchanged
//   all_gather_into_tensor           gathered = [peer][slot]
//   dl_unpack_{sgd,adamw}_topk[_fp4]_ag   g = (Σ_r decode_r) / n; the rule of dl_unpack_sgd /
//                                    dl_unpack_adamw (divisor 1); inner = θ
// One body, UnpackTopkAg<Rule, Walk>: Rule is SgdRule<MODE> or AdamRule, Walk a front end of
// dl_topk_ag_dev.h over a codec (TopkF32, TopkFp4): TopkAgWaves in the product (see there).
// Unlike the write-only gradient decoder this pass has two to four dense 16-B streams per lane
// to wait for, so the order of issue is the
// design: peer 0's entry load, then every float4 row of θ and the state (non-temporal), and only
// then the LDS work -- the zeroing and the rank-ordered sparse sum, peer r + 1's entries loaded
// ahead of peer r's adds -- which runs while the dense rows are in flight. A lane then reads its
// rows of the sum back, crosses the one barrier that frees the chunk for the workgroup's next
// one, divides by float(n) when n > 1 (IEEE division, as div4) and applies the rule; the stores
// leave one stream at a time: θ, the state, inner. The 16-KiB dense chunk is the only large LDS.
// Compiled as dl_topk_ag.hip is, without packed fp32 instructions: the division and the rules
// after it are the scalar operations of the kernels this pass is bit-identical to.
#include "dl_topk_ag_dev.h"

namespace dl {
namespace {

template <class Rule, class Walk>
struct UnpackTopkAg {
  static constexpr int K = Rule::kStates;
  TopkAgSrc src;
  float* outer;
  Rule rule;
  int inner_slot;

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
    const float* dense = reinterpret_cast<const float*>(dense4);
    float* in = inner_slot >= 0 ? slot_ptr<float>(caddr, nchunk, inner_slot, c) : nullptr;
    float* th = outer + ck.poff;
    float* sp[K];
#pragma unroll
    for (int s = 0; s < K; ++s) sp[s] = rule.state(s) + ck.poff;
    const bool avg = src.n_peers > 1;
    const float d = float(src.n_peers);
    auto one = [&](int i, float g) {
      float t1 = th[i];
      float e[K];
#pragma unroll
      for (int s = 0; s < K; ++s) e[s] = Rule::kLoadState ? sp[s][i] : 0.f;
      rule.apply(avg ? g / d : g, e, t1);
      th[i] = t1;
      if (Rule::kStoreState) {
#pragma unroll
        for (int s = 0; s < K; ++s) sp[s][i] = e[s];
      }
      if (in) in[i] = t1;
    };
    Walk walk;
    walk.begin(src, c, tid);  // peer 0's entries: the first loads in flight
    const bool rows = in == nullptr || aligned16(in);
    const int nv = ck.len >> 2;
    float4 t[kUnroll], m[K][kUnroll], g[kUnroll];
    if (rows) {  // every dense row, before any LDS work
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
    walk.sum(src, dense4, tid);  // zeroes, then the peers in rank order; ends with a barrier
    if (rows) {
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) g[u] = dense4[u * kThreads + tid];
      const int i = (nv << 2) + tid;  // the < 4 elements past the last float4, one per lane
      const float gt = i < ck.len ? dense[i] : 0.f;
      __syncthreads();  // the dense chunk is reused by the workgroup's next chunk
      if (avg) {
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) g[u] = div4(g[u], d);
      }
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

template <class Walk>
hipError_t sgd_ag(const Launch& L, const TopkAgSrc& src, float* outer, float* mom, const SgdArgs& a,
                  int inner_slot) {
  return with_sgd_rule(mom, a, [&](auto rule) {
    return run(L, UnpackTopkAg<decltype(rule), Walk>{src, outer, rule, inner_slot});
  });
}

template <class Walk>
hipError_t adamw_ag(const Launch& L, const TopkAgSrc& src, float* outer, float* m1, float* m2,
                    const AdamArgs& a, int inner_slot) {
  return run(L, UnpackTopkAg<AdamRule, Walk>{src, outer, AdamRule{m1, m2, a}, inner_slot});
}

// The product's front end is TopkAgWaves: measured level with TopkAgBarriers at n = 2 and ahead
// of it at n = 8 (tools/topk_ag_outer_bench.py). The tuning build also instantiates the body over
// TopkAgBarriers, which dl_tune_topk_ag_form(0) selects there (and which that build starts with).
template <class Codec>
hipError_t sgd_ag(const Launch& L, const uint8_t* gathered, int n_peers, int peer_stride, int k,
                  float* outer, float* mom, const SgdArgs& a, int inner_slot) {
  const TopkAgSrc src{gathered, L.c0, n_peers, peer_stride, k};
#ifdef DL_TUNING
  if (!topk_ag_form_waves()) return sgd_ag<TopkAgBarriers<Codec>>(L, src, outer, mom, a, inner_slot);
#endif
  return sgd_ag<TopkAgWaves<Codec>>(L, src, outer, mom, a, inner_slot);
}

template <class Codec>
hipError_t adamw_ag(const Launch& L, const uint8_t* gathered, int n_peers, int peer_stride, int k,
                    float* outer, float* m1, float* m2, const AdamArgs& a, int inner_slot) {
  const TopkAgSrc src{gathered, L.c0, n_peers, peer_stride, k};
#ifdef DL_TUNING
  if (!topk_ag_form_waves())
    return adamw_ag<TopkAgBarriers<Codec>>(L, src, outer, m1, m2, a, inner_slot);
#endif
  return adamw_ag<TopkAgWaves<Codec>>(L, src, outer, m1, m2, a, inner_slot);
}

}  // namespace

hipError_t launch_unpack_sgd_topk_ag(const Launch& L, const uint8_t* gathered, int n_peers,
                                     int peer_stride, int k, float* outer, float* mom, SgdArgs a,
                                     int inner_slot) {
  return sgd_ag<TopkF32>(L, gathered, n_peers, peer_stride, k, outer, mom, a, inner_slot);
}

hipError_t launch_unpack_sgd_topk_fp4_ag(const Launch& L, const uint8_t* gathered, int n_peers,
                                         int peer_stride, int k, float* outer, float* mom,
                                         SgdArgs a, int inner_slot) {
  return sgd_ag<TopkFp4>(L, gathered, n_peers, peer_stride, k, outer, mom, a, inner_slot);
}

hipError_t launch_unpack_adamw_topk_ag(const Launch& L, const uint8_t* gathered, int n_peers,
                                       int peer_stride, int k, float* outer, float* m1, float* m2,
                                       AdamArgs a, int inner_slot) {
  return adamw_ag<TopkF32>(L, gathered, n_peers, peer_stride, k, outer, m1, m2, a, inner_slot);
}

hipError_t launch_unpack_adamw_topk_fp4_ag(const Launch& L, const uint8_t* gathered, int n_peers,
                                           int peer_stride, int k, float* outer, float* m1,
                                           float* m2, AdamArgs a, int inner_slot) {
  return adamw_ag<TopkFp4>(L, gathered, n_peers, peer_stride, k, outer, m1, m2, a, inner_slot);
}

}  // namespace dl
