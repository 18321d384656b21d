// The AdamW outer step (src/utils.py:60-61, configs/optimizer/adamw.toml, stepped at
// src/train.py:267) as one fused pass per chunk: the body of dl_outer_step.h with AdamRule (one
// element of torch's _single_tensor_adamw: adam1, dl_device.h, with the formula), over two of
// its gradient sources:
//   dl_unpack_adamw      FromWire, N > 1: reads the summed wire, θ, m, v; writes θ, m, v
//                        (+ inner): 28 B/param + 4 for the inner write (fp32 wire)
//   dl_delta_pack_adamw  FromDeltaKeptOnWire, one peer (src/comm.py:118-119: no all-reduce, no
//                        division): g = θ - inner, the wire written as dl_delta_pack writes it
//                        and AdamW stepping on the value it holds; 16 B read + 20 B written per
//                        param (fp32 wire). Equal to dl_delta_pack followed by dl_unpack_adamw
//                        with divisor 1, wire included: the same body.
// Pure streaming: no LDS, no cross-lane work. Four float4[kUnroll] arrays are live per lane
// (g, θ, m, v: 64 VGPRs), so the kernels stay far from spilling (make asm prints the report).
#include "dl_outer_step.h"

namespace dl {

hipError_t launch_unpack_adamw(const Launch& L, const void* wire, int wire_dtype, int divisor,
                               float* outer, float* m1, float* m2, AdamArgs a, int inner_slot) {
  return with_wire(wire, wire_dtype, divisor, [&](auto grad) {
    return run(L, outer_step(outer, grad, AdamRule{m1, m2, a}, inner_slot));
  });
}

hipError_t launch_delta_pack_adamw(const Launch& L, int inner_slot, float* outer, void* wire,
                                   int wire_dtype, float* m1, float* m2, AdamArgs a) {
  return with_kept_wire(wire, wire_dtype, [&](auto grad) {
    return run(L, outer_step(outer, grad, AdamRule{m1, m2, a}, inner_slot));
  });
}

}  // namespace dl
