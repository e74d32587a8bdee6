// The SwiGLU element arithmetic, once: the row-wise kernels (tower.hip) and the live-row GEMM epilogues (linear_live.hip) round at the
// same points and produce the same bits.  RB names the tensor dtype's round trip (`RB::rb`, e.g. Vec16<T> or Bf16Round): every
// place an eager elementwise op would round.
//
// Contraction is pinned here, not left to the including file: products that must round on their own go through __fmul_rn (forward:
// s u; backward: da u, da s), and the d_gate expression - torch's silu_backward, `ds sig (1 + g (1 - sig))` - is compiled under an
// explicit `fp contract(fast)`, hipcc's default and what the row-wise kernels have always been built with, whatever pragma is in
// force where the function is inlined (tower.hip carries contract(off) regions).
#pragma once

#include "common.hpp"

namespace dalm {
namespace {

struct Bf16Round {
  __device__ static __forceinline__ float rb(float x) { return bf16_to_f32(f32_to_bf16(x)); }
};

__device__ __forceinline__ float silu_f32(float x) { return x / (1.0f + expf(-x)); }

// act = rb(s u) with s = rb(silu(g)).  The two halves are separate functions because s depends on g alone: a caller whose g is
// bf16 may take s from a table of all 65536 values FILLED WITH swiglu_silu_rb (linear_live.hip does) - the same bits by construction.
template <typename RB>
__device__ __forceinline__ float swiglu_silu_rb(float g) { return RB::rb(silu_f32(g)); }
template <typename RB>
__device__ __forceinline__ float swiglu_act_of(float s, float u) { return RB::rb(__fmul_rn(s, u)); }
template <typename RB>
__device__ __forceinline__ float swiglu_fwd_elem(float g, float u) {
  return swiglu_act_of<RB>(swiglu_silu_rb<RB>(g), u);
}

// d_up = rb(da s) with s = rb(silu(g)) (the activation the eager chain saved); d_gate = rb(ds sig (1 + g (1 - sig))) with ds = rb(da u)
template <typename RB>
__device__ __forceinline__ void swiglu_bwd_elem(float da, float g, float u, float& d_gate, float& d_up) {
#pragma clang fp contract(fast)
  const float s = RB::rb(silu_f32(g));
  const float ds = RB::rb(__fmul_rn(da, u));
  d_up = RB::rb(__fmul_rn(da, s));
  const float sig = 1.0f / (1.0f + expf(-g));
  d_gate = RB::rb(ds * sig * (1.0f + g * (1.0f - sig)));
}

}  // namespace
}  // namespace dalm
