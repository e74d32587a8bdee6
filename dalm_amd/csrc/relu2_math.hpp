// The ReLU^2 element arithmetic (ArceeMLP: act_fn = torch.square(F.relu(x))), once: the row-wise kernels (tower.hip) and the live-row
// GEMM epilogue (linear_live.hip) round at the same points and produce the same bits.  RB names the tensor dtype's round trip
// (`RB::rb`, e.g. Vec16<T> or Bf16Round): every place an eager elementwise op would round.
//
// The eager chain and its autograd, which these restate:
//   forward   r = relu(y) (exact; NaN stays NaN);  act = rb(r r)
//   backward  square: d_r = rb(d_act rb(2 r)) (pow_backward with exponent 2; 2 r is exact short of overflow, where f32 and bf16
//             both give inf);  relu: d_y = (r <= 0) ? 0 : d_r - a zero whatever d_act holds, and d_act NaN = NaN for a NaN y
// Products go through __fmul_rn: nothing here may contract, whatever pragma is in force where the functions are inlined.
#pragma once

#include "common.hpp"

namespace dalm {
namespace {

template <typename RB>
__device__ __forceinline__ float relu2_fwd_elem(float y) {
  const float r = y <= 0.0f ? 0.0f : y;                    // a NaN compares false: it passes
  return RB::rb(__fmul_rn(r, r));
}

template <typename RB>
__device__ __forceinline__ float relu2_bwd_elem(float da, float y) {
  return y <= 0.0f ? 0.0f : RB::rb(__fmul_rn(da, RB::rb(__fmul_rn(2.0f, y))));
}

}  // namespace
}  // namespace dalm
