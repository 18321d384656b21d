// The outer step as ONE walker body, OuterStep<Grad, Rule>, with two axes:
//   Grad  where a chunk's gradient comes from: the wire (with or without the division by the
//         peer count), θ - inner, θ - inner with the wire written and the rule stepping on
//         the value as the wire holds it, or that after a pending step whose θ and state were
//         never stored (they are recomputed from the wire that step left);
//   Rule  what is done with it: SGD (one state stream, the momentum buffer) or AdamW (two,
//         exp_avg and exp_avg_sq); the arithmetic is sgd1 / adam1 of dl_device.h.
// and two policies. kDefer: θ and the state are not stored (the wire and inner are), so the step
// stays pending: the streams as they were plus the wire determine it. Merge (wire sources only):
// the inner rows are loaded beside the other streams and inner receives fmaf(alpha, x - θ, θ),
// x the inner value as loaded, instead of θ (Streaming DiLoCo's merge of a model that moved on
// while the exchange was in flight).
// Every outer-step kernel of dl_kernels.hip and dl_adamw.hip is an instantiation, so the fused
// kernels equal the dl_delta_pack + dl_unpack_* pair bit for bit by construction: the element
// arithmetic is written once, for the float4 rows, the tail lane and the unaligned loop alike.
#pragma once
#include "dl_device.h"

namespace dl {
namespace {

// ---- update rules --------------------------------------------------------------------------
// A rule states: its state streams (kStates, and whether they are loaded and stored), whether
// the arithmetic is skipped on rows past the chunk (kSkipPastChunk), and where a kept wire's
// rows are stored (kWireFirst: before the arithmetic; otherwise after it, ahead of θ).
template <int MODE>  // sgd1's MODE
struct SgdRule {
  static constexpr int kStates = 1;
  static constexpr bool kLoadState = MODE == 2;
  static constexpr bool kStoreState = MODE != 0;
  static constexpr bool kSkipPastChunk = false;
  // before the arithmetic the wire rows cost 4 VGPRs (bf16 wire, MODE 2: 64 -> 68, occupancy 8 -> 7)
  static constexpr bool kWireFirst = false;
  float* mom;
  SgdArgs a;
  __device__ __forceinline__ float* state(int) const { return mom; }
  __device__ __forceinline__ void apply(float g, float (&s)[kStates], float& th) const {
    sgd1<MODE>(g, s[0], th, a);
  }
};

struct AdamRule {
  static constexpr int kStates = 2;
  static constexpr bool kLoadState = true;
  static constexpr bool kStoreState = true;
  static constexpr bool kSkipPastChunk = true;  // rows past the chunk hold no data: no sqrt / division
  // after the arithmetic the wire rows cost 4 VGPRs (90 -> 94): they leave as soon as they are ready
  static constexpr bool kWireFirst = true;
  float* m1;  // exp_avg
  float* m2;  // exp_avg_sq
  AdamArgs a;
  __device__ __forceinline__ float* state(int k) const { return k == 0 ? m1 : m2; }
  __device__ __forceinline__ void apply(float g, float (&s)[kStates], float& th) const {
    adam1(g, s[0], s[1], th, a);
  }
};

// ---- gradient sources ----------------------------------------------------------------------
// kDelta: the stream loaded beside θ is the inner parameter and the raw gradient is θ - inner
// (otherwise it is the wire's value). kKeepsWire: the raw gradient is stored to the wire.
// kPending: θ and the state as loaded are one step behind; `pend`, the rule of that step, is
// applied to the wire's old value first. fin: the raw gradient -> the value the rule steps on.
template <typename W, bool DIV>
struct FromWire {  // a3: the summed wire / n (DIV false: one peer's own wire, untouched)
  using Wire = W;
  static constexpr bool kDelta = false, kKeepsWire = false, kPending = false;
  const W* wire;
  float d;
  __device__ __forceinline__ const W* at(int64_t poff) const { return wire + poff; }
  __device__ __forceinline__ float fin(float g) const { return DIV ? g / d : g; }
};

// a2 at ONE peer (src/comm.py:118-119: no all-reduce, no division): the delta never leaves
// registers
struct FromDelta {
  using Wire = float;
  static constexpr bool kDelta = true, kKeepsWire = false, kPending = false;
  __device__ __forceinline__ const float* at(int64_t) const { return nullptr; }
  __device__ __forceinline__ float fin(float g) const { return g; }
};

// a2 at one peer with the pseudo-gradient kept (outer.grad of src/utils.py:221, the reference's
// observable .grad after the step): wire = W(θ - inner), and the rule consumes the value on the
// wire -- a bf16 wire rounds it first, as dl_unpack_* would read it back
template <typename W>
struct FromDeltaKeptOnWire {
  using Wire = W;
  static constexpr bool kDelta = true, kKeepsWire = true, kPending = false;
  W* wire;
  __device__ __forceinline__ W* at(int64_t poff) const { return wire + poff; }
  __device__ __forceinline__ float fin(float g) const {
    if constexpr (sizeof(W) == 2) return bf2f(f2bf(g));
    else return g;
  }
};

// FromDeltaKeptOnWire (fp32 wire) after a step run with kDefer: θ, the state and the wire are
// loaded, `pend` (that step's rule: the same arithmetic, so the same bits it would have stored)
// brings θ and the state up to date in registers, then g = θ - inner goes over the old wire in
// place -- the lane that stores a wire element is the one that loaded it
template <class Pend>
struct FromDeltaAfterPending {
  using Wire = float;
  static constexpr bool kDelta = true, kKeepsWire = true, kPending = true;
  float* wire;
  Pend pend;
  __device__ __forceinline__ float* at(int64_t poff) const { return wire + poff; }
  __device__ __forceinline__ float fin(float g) const { return g; }
};

// ---- the inner write -------------------------------------------------------------------------
// What inner receives once the rule has produced θ. NoMerge: θ (sync_inner_model). MergeInner:
// alpha·x + (1 - alpha)·θ as ONE rounded subtract and ONE fma (contract off, like sgd1's), x the
// inner value loaded before any store. No special case: a non-finite x stays in its own element.
struct NoMerge {
  static constexpr bool kOn = false;
  __device__ __forceinline__ float operator()(float, float th) const { return th; }
};
struct MergeInner {
  static constexpr bool kOn = true;
  float alpha;
  __device__ __forceinline__ float operator()(float x, float th) const {
    return __builtin_fmaf(alpha, x - th, th);
  }
};

template <int J>
__device__ __forceinline__ float& comp(float4& v) {
  if constexpr (J == 0) return v.x;
  else if constexpr (J == 1) return v.y;
  else if constexpr (J == 2) return v.z;
  else return v.w;
}

// which state streams a step loads and stores: the rule's, and a pending rule's beside them
template <class Rule, class Grad>
struct StateIO {
  static constexpr bool kLoad = Rule::kLoadState, kStore = Rule::kStoreState;
};
template <class Rule, class Pend>
struct StateIO<Rule, FromDeltaAfterPending<Pend>> {
  static_assert(Pend::kStates == Rule::kStates, "the pending rule steps the same state streams");
  static constexpr bool kLoad = Rule::kLoadState || Pend::kLoadState;
  static constexpr bool kStore = Rule::kStoreState || Pend::kStoreState;
};

// ---- the body ------------------------------------------------------------------------------
// Per chunk: every 16-B load up front (gradient stream, θ, states), the subtraction or
// division, the rule per component, then the stores, one stream's rows back to back: wire, θ,
// state..., inner (inner_slot -1, wire sources only: no copy-back; kDefer: no θ, no state; Merge:
// the merged rows, computed row by row as they leave). The < 4 elements past the last float4 go
// one per lane; a tensor whose storage is only 4-B aligned goes element-wise.
template <class Grad, class Rule, bool kDefer = false, class Merge = NoMerge>
struct OuterStep {
  static constexpr int K = Rule::kStates;
  static constexpr bool kWireFirst = Grad::kKeepsWire && Rule::kWireFirst;
  static constexpr bool kLoadState = StateIO<Rule, Grad>::kLoad;
  static constexpr bool kStoreState = StateIO<Rule, Grad>::kStore;
  static_assert(!(Grad::kPending && kWireFirst), "a pending step's wire is read before it is stored");
  static_assert(!kDefer || (Grad::kKeepsWire && !Grad::kPending), "a deferred step leaves its wire");
  static_assert(!Merge::kOn || (!Grad::kDelta && !kDefer), "the merge reads inner beside a wire source");
  using WIO = WireIO<typename Grad::Wire>;
  float* outer;
  Grad grad;
  Rule rule;
  int inner_slot;
  [[no_unique_address]] Merge merge;  // NoMerge: empty, the kernel arguments are as without it

  // component J of row u (a pending source: g holds inner coming in, the gradient going out,
  // old the wire as the pending step left it)
  template <int J>
  __device__ __forceinline__ void step(float4& g, float4 (&s)[K][kUnroll], int u, float4& t,
                                       float4 old) const {
    float e[K];
#pragma unroll
    for (int k = 0; k < K; ++k) e[k] = kLoadState ? comp<J>(s[k][u]) : 0.f;
    if constexpr (Grad::kPending) {
      grad.pend.apply(comp<J>(old), e, comp<J>(t));  // θ and the state the pending step meant
      comp<J>(g) = comp<J>(t) - comp<J>(g);          // the pseudo-gradient
    }
    rule.apply(grad.fin(comp<J>(g)), e, comp<J>(t));
    if (kStoreState) {
#pragma unroll
      for (int k = 0; k < K; ++k) comp<J>(s[k][u]) = e[k];
    }
  }

  template <bool NTL, int NTS>
  __device__ __forceinline__ void run(const Chunk& ck, int c, void* const* caddr, int nchunk, int tid) const {
    float* in = (Grad::kDelta || inner_slot >= 0) ? slot_ptr<float>(caddr, nchunk, inner_slot, c) : nullptr;
    const bool copy_back = Grad::kDelta || in != nullptr;
    const auto w = grad.at(ck.poff);
    float* th = outer + ck.poff;
    float* sp[K];
#pragma unroll
    for (int k = 0; k < K; ++k) sp[k] = rule.state(k) + ck.poff;

    auto one = [&](int i) {
      float t = th[i], g, xi = 0.f;
      float e[K];
      if constexpr (Merge::kOn) xi = in[i];
#pragma unroll
      for (int k = 0; k < K; ++k) e[k] = kLoadState ? sp[k][i] : 0.f;
      if constexpr (Grad::kPending) grad.pend.apply(WIO::ld1(w, i), e, t);
      if constexpr (Grad::kDelta) g = t - in[i];
      else g = WIO::ld1(w, i);
      if constexpr (Grad::kKeepsWire) WIO::st1(w, i, g);
      rule.apply(grad.fin(g), e, t);
      if constexpr (!kDefer) th[i] = t;
      if (kStoreState && !kDefer) {
#pragma unroll
        for (int k = 0; k < K; ++k) sp[k][i] = e[k];
      }
      if (copy_back) in[i] = merge(xi, t);
    };

    if (!copy_back || aligned16(in)) {
      const int nv = ck.len >> 2;
      float4 x[kUnroll], t[kUnroll], s[K][kUnroll], old[kUnroll], xi[Merge::kOn ? kUnroll : 1];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int v = u * kThreads + tid;
        if (v < nv) {
          if constexpr (!Grad::kDelta) x[u] = WIO::template ld4<NTL>(w, v);
          if constexpr (Grad::kPending) old[u] = WIO::template ld4<NTL>(w, v);
          t[u] = ldf4<NTL>(th, v);
          if constexpr (Grad::kDelta) x[u] = ldf4<NTL>(in, v);
          if constexpr (Merge::kOn) xi[u] = ldf4<NTL>(in, v);
          if (kLoadState) {
#pragma unroll
            for (int k = 0; k < K; ++k) s[k][u] = ldf4<NTL>(sp[k], v);
          }
        }
      }
      if constexpr (kWireFirst) {  // per row inside the guard: one subtract, and the row leaves
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          const int v = u * kThreads + tid;
          if (v < nv) {
            x[u] = sub4(t[u], x[u]);
            WIO::template st4<NTS>(w, v, x[u]);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        if (!Rule::kSkipPastChunk || u * kThreads + tid < nv) {
          if constexpr (Grad::kDelta && !kWireFirst && !Grad::kPending)
            x[u] = sub4(t[u], x[u]);  // the pseudo-gradient
          step<0>(x[u], s, u, t[u], old[u]);
          step<1>(x[u], s, u, t[u], old[u]);
          step<2>(x[u], s, u, t[u], old[u]);
          step<3>(x[u], s, u, t[u], old[u]);
        }
      }
      if constexpr (Grad::kKeepsWire && !kWireFirst) {
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          const int v = u * kThreads + tid;
          if (v < nv) WIO::template st4<NTS>(w, v, x[u]);
        }
      }
      if constexpr (!kDefer) store_rows<NTS>(th, t, nv, tid);
      if (kStoreState && !kDefer) {
#pragma unroll
        for (int k = 0; k < K; ++k) store_rows<NTS>(sp[k], s[k], nv, tid);
      }
      if constexpr (Merge::kOn) {
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          const int v = u * kThreads + tid;
          if (v < nv)
            stf4<NTS>(in, v, make_float4(merge(xi[u].x, t[u].x), merge(xi[u].y, t[u].y),
                                         merge(xi[u].z, t[u].z), merge(xi[u].w, t[u].w)));
        }
      } else if (copy_back) {
        store_rows<NTS>(in, t, nv, tid);
      }
      const int i = (nv << 2) + tid;
      if (i < ck.len) one(i);
    } else {
      for (int i = tid; i < ck.len; i += kThreads) one(i);
    }
  }
};

template <bool kDefer = false, class Grad, class Rule>
OuterStep<Grad, Rule, kDefer> outer_step(float* outer, Grad grad, Rule rule, int inner_slot) {
  return {outer, grad, rule, inner_slot};
}

// the step whose inner write merges (inner_slot bound: the caller checked)
template <class Grad, class Rule>
OuterStep<Grad, Rule, false, MergeInner> outer_step_merge(float* outer, Grad grad, Rule rule,
                                                          int inner_slot, float alpha) {
  return {outer, grad, rule, inner_slot, MergeInner{alpha}};
}

// ---- host-side dispatch: f is called with the gradient source / rule the arguments select ----
template <class F>
hipError_t with_wire(const void* wire, int wire_dtype, int divisor, F&& f) {
  const float d = float(divisor);
  if (wire_dtype == DL_BF16) {
    const bf16_t* w = static_cast<const bf16_t*>(wire);
    return divisor == 1 ? f(FromWire<bf16_t, false>{w, d}) : f(FromWire<bf16_t, true>{w, d});
  }
  const float* w = static_cast<const float*>(wire);
  return divisor == 1 ? f(FromWire<float, false>{w, d}) : f(FromWire<float, true>{w, d});
}

template <class F>
hipError_t with_kept_wire(void* wire, int wire_dtype, F&& f) {
  if (wire_dtype == DL_BF16) return f(FromDeltaKeptOnWire<bf16_t>{static_cast<bf16_t*>(wire)});
  return f(FromDeltaKeptOnWire<float>{static_cast<float*>(wire)});
}

template <class F>
hipError_t with_sgd_rule(float* mom, const SgdArgs& a, F&& f) {
  if (a.momentum == 0.f) return f(SgdRule<0>{mom, a});
  if (a.first) return f(SgdRule<1>{mom, a});
  return f(SgdRule<2>{mom, a});
}

}  // namespace
}  // namespace dl
