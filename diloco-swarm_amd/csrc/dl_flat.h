// The flat-shard forms shared by dl_kernels.hip (SGD) and dl_adamw.hip (AdamW): the launcher
// that runs a walker body over a contiguous shard, and the slice loads + rank-order sum of the
// kernels that follow an all_to_all.
#pragma once
#include "dl_outer_step.h"

namespace dl {

// Sharded outer step: after the reduce-scatter each peer owns a contiguous 1/n of
// every bucket; dl_unpack_sgd's body runs over it as flat 4096-element chunks (no tree, no
// inner copy: θ is all-gathered and scattered to the inner params afterwards).
template <class Body>
__global__ void __launch_bounds__(kThreads) k_flat(int64_t n, Body body) {
  for (int64_t base = int64_t(blockIdx.x) * DL_CHUNK_ELEMS; base < n;
       base += int64_t(gridDim.x) * DL_CHUNK_ELEMS) {
    Chunk ck;
    ck.poff = base;
    ck.len = int32_t(n - base < DL_CHUNK_ELEMS ? n - base : DL_CHUNK_ELEMS);
    ck.seg = 0;
    body.template run<true, kStNT>(ck, 0, nullptr, 0, int(threadIdx.x));  // NT loads + stores
  }
}

template <class Body>
static hipError_t run_flat(int64_t n, const Body& body, hipStream_t s) {
  const int32_t grid = int32_t((n + DL_CHUNK_ELEMS - 1) / DL_CHUNK_ELEMS);
  hipLaunchKernelGGL(k_flat<Body>, dim3(grid), dim3(kThreads), 0, s, n, body);
  return hipGetLastError();
}

namespace {

// The slice side of a workgroup's tile after an all_to_all: `slices` holds nn equal slices of
// `len` elements of wire type W, slice q being rank q's copy of this peer's shard; the tile is
// the R float4 rows per lane from element `base`, nv of them inside the shard. g[u] receives
// (s_0 + s_1) + ... + s_{nn-1} of row u in fp32, in rank order (undivided; a bf16 wire is
// widened on load and never re-rounded). N = 1..8: every slice row is loaded before the first
// add; N = 0: nn is a run-time count (> 8) and the slices are accumulated as they arrive.
// also(u, v) is called once per row inside the guard, among the slice loads, for the caller's
// own loads (θ, its state rows): all of a tile's loads are issued before any arithmetic.
template <int N, int R, typename W, class Also>
__device__ __forceinline__ void slice_sum(const W* slices, int nn, int64_t len, int64_t base,
                                          int32_t nv, float4 (&g)[R], Also&& also) {
  if constexpr (N > 0) {
    float4 w[N][R];
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const int v = u * kThreads + int(threadIdx.x);
      if (v < nv) {
#pragma unroll
        for (int q = 0; q < N; ++q) w[q][u] = WireIO<W>::template ld4<true>(slices + q * len + base, v);
        also(u, v);
      }
    }
#pragma unroll
    for (int u = 0; u < R; ++u) {
      g[u] = w[0][u];
#pragma unroll
      for (int q = 1; q < N; ++q)
        g[u] = make_float4(g[u].x + w[q][u].x, g[u].y + w[q][u].y, g[u].z + w[q][u].z,
                           g[u].w + w[q][u].w);
    }
  } else {
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const int v = u * kThreads + int(threadIdx.x);
      if (v < nv) {
        also(u, v);
        g[u] = WireIO<W>::template ld4<true>(slices + base, v);
        for (int q = 1; q < nn; ++q) {
          const float4 d = WireIO<W>::template ld4<true>(slices + q * len + base, v);
          g[u] = make_float4(g[u].x + d.x, g[u].y + d.y, g[u].z + d.z, g[u].w + d.w);
        }
      }
    }
  }
}

// rows of a tile inside the shard, and the grid of a slice kernel with R rows per lane
__device__ __forceinline__ int32_t slice_tile_rows(int64_t len, int64_t base, int rows) {
  return int32_t((len - base) / 4 < kThreads * rows ? (len - base) / 4 : kThreads * rows);
}
inline int32_t slice_grid(int64_t len, int rows) {
  const int64_t step = int64_t(kThreads) * rows * 4;
  const int64_t blocks = (len + step - 1) / step;
  return int32_t(blocks < (1 << 20) ? blocks : (1 << 20));
}

}  // namespace
}  // namespace dl
