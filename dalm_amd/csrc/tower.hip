// dalm_rope_qk / dalm_swiglu_*: the two elementwise chains of a Llama-family generator layer that the step spends the most
// launches on, each as ONE streaming kernel per direction (gfx950).
//
// The reference runs its generator through transformers (dalm/models/rag_e2e_base_model.py:104-106 ->
// transformers/models/llama/modeling_llama.py): apply_rotary_pos_emb is  q*cos + rotate_half(q)*sin  for q and k
// (8 eager launches forward, ~14 backward per layer) and LlamaMLP is  down(silu(gate(x)) * up(x))  (2 forward, 4 backward,
// plus a saved [tokens, intermediate] activation).  Both are pure HBM streams; measured in the cfg3 step they were ~12 ms +
// ~5 ms of 175 ms (profiles/history/r04_bench_step_kernel_stats.txt: roll / addcmul / MulFunctor / silu / silu_backward rows).
//
// Rounding contract: torch evaluates every eager elementwise op in f32 and rounds its result to the tensor dtype.  These
// kernels round at exactly the same points (Vec16<T>::rb: a bf16 round trip for bf16 tensors, the identity for f32; separate
// mul / add, never a fused multiply-add), so forward AND backward results are the values the eager chain - and autograd's
// backward of it - produce, not merely close to them.
//   rope forward :  o1 = rb(rb(x1 c1) - rb(x2 s1))          o2 = rb(rb(x2 c2) + rb(x1 s2))        (halves 1 | 2 of head_dim)
//   rope backward:  d1 = rb(rb(g1 c1) + rb(g2 s2))          d2 = rb(rb(g2 c2) - rb(g1 s1))
//   swiglu forward :  s = rb(g / (1 + exp(-g)));  a = rb(s u)
//   swiglu backward:  ds = rb(da u);  du = rb(da s);  sig = 1 / (1 + exp(-g));  dg = rb(ds sig (1 + g (1 - sig)))
// Algorithmic bytes: rope 2 * (|q| + |k|) * el (+ cos/sin, shared by all heads); swiglu forward 3 * n * el, backward 5 * n * el.
// Further down: RMSNorm with the residual add (dalm_rms_norm_*), Qwen3's head norm + rotary (dalm_head_norm_*), and Gemma's two
// formulas - GeGLU and the (1 + w) RMSNorm (dalm_geglu_*, dalm_gemma_norm_*) - Arcee's ReLU^2 (dalm_relu2_*), and OLMo-2's norm-then-add
// and row-wide q / k norm + rotary (dalm_norm_add_*, dalm_row_norm_*), and Granite's scaled residual add with and without the norm
// behind it (dalm_rms_norm_scaled_*, dalm_scale_add), and Cohere's interleaved f32 rotary embedding, bias-free f32 LayerNorm and
// three-way residual add (dalm_rope_il_qk, dalm_cohere_norm_*, dalm_add3_live), and Phi-3's partial rotary embedding
// (dalm_rope_partial_qk), each with its own comment block.
#include "dispatch.hpp"
#include "relu2_math.hpp"
#include "swiglu_math.hpp"
#include "vec16.hpp"

namespace dalm {
namespace {

// ---------------------------------------------------------------------------------------------------
// rotary embedding of q and k in one launch.  Tensors are [B, H, T, hd] VIEWS with arbitrary (b, h, t) strides and a
// contiguous last dimension (transformers hands over transposed views of the [B, T, H*hd] projections); cos / sin are
// [B, T, hd] with (b, t) strides.  A row = one (b, t, head); rows are walked head-fastest, the memory order of those views.
// ---------------------------------------------------------------------------------------------------
struct RopeTensor { const void* x; void* o; int64_t xs[3]; int64_t os[3]; };   // strides of (b, h, t) in elements
struct RopeParams {
  RopeTensor q, k;
  const void* cos; const void* sin; int64_t cs[2];   // strides of (b, t)
  int B, T, Hq, Hk, hd, backward;
  const unsigned char* live;                         // [B * T] or NULL: a dead (b, t) is not read, its outputs are zeros
};

template <typename T, bool VECTOR>
__global__ __launch_bounds__(256) void rope_qk_kernel(const RopeParams p) {
#pragma clang fp contract(off)   // the eager chain is separate mul and add kernels: a fused multiply-add would round once less (f32)
  constexpr int VEC = VECTOR ? Vec16<T>::VEC : 1;
  const int h = p.hd >> 1;
  const int tpr = h / VEC;                       // threads per row
  const int64_t gid = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const int64_t row = gid / tpr;
  const int c = static_cast<int>(gid - row * tpr) * VEC;
  const int H = p.Hq + p.Hk;
  const int64_t rows = static_cast<int64_t>(p.B) * p.T * H;
  if (row >= rows) return;
  const int hh = static_cast<int>(row % H);
  const int64_t bt = row / H;
  const int t = static_cast<int>(bt % p.T), b = static_cast<int>(bt / p.T);
  const bool is_k = hh >= p.Hq;
  const RopeTensor& R = is_k ? p.k : p.q;
  const int head = is_k ? hh - p.Hq : hh;
  const T* x = static_cast<const T*>(R.x) + b * R.xs[0] + head * R.xs[1] + t * R.xs[2] + c;
  T* o = static_cast<T*>(R.o) + b * R.os[0] + head * R.os[1] + t * R.os[2] + c;
  if (p.live && !p.live[bt]) {
    float z[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) z[e] = 0.f;
    if constexpr (VECTOR) { Vec16<T>::store(o, z); Vec16<T>::store(o + h, z); }
    else { Vec16<T>::put(o, 0.f); Vec16<T>::put(o + h, 0.f); }
    return;
  }
  const T* cs = static_cast<const T*>(p.cos) + b * p.cs[0] + t * p.cs[1] + c;
  const T* sn = static_cast<const T*>(p.sin) + b * p.cs[0] + t * p.cs[1] + c;
  float x1[VEC], x2[VEC], c1[VEC], c2[VEC], s1[VEC], s2[VEC], o1[VEC], o2[VEC];
  if constexpr (VECTOR) {
    Vec16<T>::load(x, x1); Vec16<T>::load(x + h, x2);
    Vec16<T>::load(cs, c1); Vec16<T>::load(cs + h, c2);
    Vec16<T>::load(sn, s1); Vec16<T>::load(sn + h, s2);
  } else {
    x1[0] = Vec16<T>::get(x); x2[0] = Vec16<T>::get(x + h);
    c1[0] = Vec16<T>::get(cs); c2[0] = Vec16<T>::get(cs + h);
    s1[0] = Vec16<T>::get(sn); s2[0] = Vec16<T>::get(sn + h);
  }
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    // plain operators on purpose: the contract(off) pragma above governs THIS function's operations (the __f*_rn helpers are
    // inlined from a header compiled with contraction allowed and would fuse)
    const float a1 = Vec16<T>::rb(x1[e] * c1[e]), a2 = Vec16<T>::rb(x2[e] * c2[e]);
    if (!p.backward) {
      const float b1 = Vec16<T>::rb(x2[e] * s1[e]), b2 = Vec16<T>::rb(x1[e] * s2[e]);
      o1[e] = Vec16<T>::rb(a1 - b1);
      o2[e] = Vec16<T>::rb(a2 + b2);
    } else {
      const float b1 = Vec16<T>::rb(x2[e] * s2[e]), b2 = Vec16<T>::rb(x1[e] * s1[e]);
      o1[e] = Vec16<T>::rb(a1 + b1);
      o2[e] = Vec16<T>::rb(a2 - b2);
    }
  }
  if constexpr (VECTOR) {
    Vec16<T>::store(o, o1); Vec16<T>::store(o + h, o2);
  } else {
    Vec16<T>::put(o, o1[0]); Vec16<T>::put(o + h, o2[0]);
  }
}

// ---------------------------------------------------------------------------------------------------
// SwiGLU over n contiguous elements.  A workgroup walks STEPS tiles of 256*VEC elements with every load issued before the
// first store (single-tile workgroups are bound by workgroup dispatch at this size: profiles/history/r04_nf4_steps.txt).
// ---------------------------------------------------------------------------------------------------
// (the element arithmetic - silu_f32, swiglu_fwd_elem, swiglu_bwd_elem - is swiglu_math.hpp's: the live-row GEMM epilogues share it)

// [R, C] views with a row stride (gate and up as the two halves of ONE [R, 2C] GEMM output, models/frozen_linear.py): element
// e of the logical [R, C] matrix lives at (e / C) * ld + e % C; C is a multiple of VEC, so a vector never crosses a row
struct SwigluLd { int64_t C, g, u, a, dg, du; };
// element index -> (row, column): 32-bit arithmetic (the entry points require R C < 2^32; a 64-bit division per vector made the
// first form of these kernels run at 0.47 of HBM where the contiguous ones reach 0.66)
struct RowCol { unsigned int row, col; };
__device__ __forceinline__ RowCol row_col(int64_t e, int64_t C) {
  const unsigned int ee = static_cast<unsigned int>(e), cc = static_cast<unsigned int>(C), r = ee / cc;
  return {r, ee - r * cc};
}
__device__ __forceinline__ int64_t ld_at(const RowCol& rc, int64_t ld) { return static_cast<int64_t>(rc.row) * ld + rc.col; }
// the tile `step` elements further on: no division (ONE per thread for its first tile; the silu itself is a dozen f32 operations
// per element, eight divisions per thread cost the first form a third of its rate)
__device__ __forceinline__ RowCol advance(RowCol rc, unsigned int step, unsigned int C) {
  rc.col += step;
  while (rc.col >= C) { rc.col -= C; ++rc.row; }
  return rc;
}

template <typename T, int STEPS>
__global__ __launch_bounds__(256) void swiglu_fwd_2d_kernel(const T* __restrict__ g, const T* __restrict__ u, T* __restrict__ a,
                                                            int64_t n, SwigluLd ld, const unsigned char* __restrict__ live) {
  constexpr int VEC = Vec16<T>::VEC;
  const int64_t base = (static_cast<int64_t>(blockIdx.x) * STEPS * 256 + threadIdx.x) * VEC;
  float gv[STEPS][VEC], uv[STEPS][VEC];
  RowCol rc[STEPS];
  bool lv[STEPS];                                                    // in range and (with `live`) a row that matters
  rc[0] = row_col(base < n ? base : 0, ld.C);
#pragma unroll
  for (int k = 1; k < STEPS; ++k) rc[k] = advance(rc[k - 1], 256 * VEC, static_cast<unsigned int>(ld.C));
#pragma unroll
  for (int k = 0; k < STEPS; ++k) {
    const int64_t e0 = base + static_cast<int64_t>(k) * 256 * VEC;
    lv[k] = e0 < n && (!live || live[rc[k].row]);
  }
#pragma unroll
  for (int k = 0; k < STEPS; ++k) {
    if (lv[k]) {
      Vec16<T>::load(g + ld_at(rc[k], ld.g), gv[k]);
      Vec16<T>::load(u + ld_at(rc[k], ld.u), uv[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < STEPS; ++k) {
    const int64_t e0 = base + static_cast<int64_t>(k) * 256 * VEC;
    if (e0 >= n) continue;
    float o[VEC];
    if (lv[k]) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) o[e] = swiglu_fwd_elem<Vec16<T>>(gv[k][e], uv[k][e]);
    } else {                                                         // a dead row: nothing was loaded, zeros leave
#pragma unroll
      for (int e = 0; e < VEC; ++e) o[e] = 0.f;
    }
    Vec16<T>::store(a + ld_at(rc[k], ld.a), o);
  }
}

template <typename T, int STEPS>
__global__ __launch_bounds__(256) void swiglu_bwd_2d_kernel(const T* __restrict__ da, const T* __restrict__ g,
                                                            const T* __restrict__ u, T* __restrict__ dg, T* __restrict__ du,
                                                            int64_t n, SwigluLd ld, const unsigned char* __restrict__ live) {
  constexpr int VEC = Vec16<T>::VEC;
  const int64_t base = (static_cast<int64_t>(blockIdx.x) * STEPS * 256 + threadIdx.x) * VEC;
  float av[STEPS][VEC], gv[STEPS][VEC], uv[STEPS][VEC];
  RowCol rc[STEPS];
  bool lv[STEPS];
  rc[0] = row_col(base < n ? base : 0, ld.C);
#pragma unroll
  for (int k = 1; k < STEPS; ++k) rc[k] = advance(rc[k - 1], 256 * VEC, static_cast<unsigned int>(ld.C));
#pragma unroll
  for (int k = 0; k < STEPS; ++k) {
    const int64_t e0 = base + static_cast<int64_t>(k) * 256 * VEC;
    lv[k] = e0 < n && (!live || live[rc[k].row]);
  }
#pragma unroll
  for (int k = 0; k < STEPS; ++k) {
    if (lv[k]) {
      Vec16<T>::load(da + ld_at(rc[k], ld.a), av[k]);
      Vec16<T>::load(g + ld_at(rc[k], ld.g), gv[k]);
      Vec16<T>::load(u + ld_at(rc[k], ld.u), uv[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < STEPS; ++k) {
    const int64_t e0 = base + static_cast<int64_t>(k) * 256 * VEC;
    if (e0 >= n) continue;
    float og[VEC], ou[VEC];
    if (lv[k]) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) swiglu_bwd_elem<Vec16<T>>(av[k][e], gv[k][e], uv[k][e], og[e], ou[e]);
    } else {
#pragma unroll
      for (int e = 0; e < VEC; ++e) { og[e] = 0.f; ou[e] = 0.f; }
    }
    Vec16<T>::store(dg + ld_at(rc[k], ld.dg), og);
    Vec16<T>::store(du + ld_at(rc[k], ld.du), ou);
  }
}

template <typename T, int STEPS>
__global__ __launch_bounds__(256) void swiglu_fwd_kernel(const T* __restrict__ g, const T* __restrict__ u, T* __restrict__ a,
                                                         int64_t n) {
  constexpr int VEC = Vec16<T>::VEC;
  const int64_t base = (static_cast<int64_t>(blockIdx.x) * STEPS * 256 + threadIdx.x) * VEC;
  float gv[STEPS][VEC], uv[STEPS][VEC];
#pragma unroll
  for (int k = 0; k < STEPS; ++k) {
    const int64_t e0 = base + static_cast<int64_t>(k) * 256 * VEC;
    if (e0 + VEC <= n) { Vec16<T>::load(g + e0, gv[k]); Vec16<T>::load(u + e0, uv[k]); }
    else {
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        gv[k][e] = e0 + e < n ? Vec16<T>::get(g + e0 + e) : 0.f;
        uv[k][e] = e0 + e < n ? Vec16<T>::get(u + e0 + e) : 0.f;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < STEPS; ++k) {
    const int64_t e0 = base + static_cast<int64_t>(k) * 256 * VEC;
    if (e0 >= n) continue;
    float o[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) o[e] = swiglu_fwd_elem<Vec16<T>>(gv[k][e], uv[k][e]);
    if (e0 + VEC <= n) Vec16<T>::store(a + e0, o);
    else
      for (int e = 0; e < VEC && e0 + e < n; ++e) Vec16<T>::put(a + e0 + e, o[e]);
  }
}

template <typename T, int STEPS>
__global__ __launch_bounds__(256) void swiglu_bwd_kernel(const T* __restrict__ da, const T* __restrict__ g,
                                                         const T* __restrict__ u, T* __restrict__ dg, T* __restrict__ du,
                                                         int64_t n) {
  constexpr int VEC = Vec16<T>::VEC;
  const int64_t base = (static_cast<int64_t>(blockIdx.x) * STEPS * 256 + threadIdx.x) * VEC;
  float av[STEPS][VEC], gv[STEPS][VEC], uv[STEPS][VEC];
#pragma unroll
  for (int k = 0; k < STEPS; ++k) {
    const int64_t e0 = base + static_cast<int64_t>(k) * 256 * VEC;
    if (e0 + VEC <= n) { Vec16<T>::load(da + e0, av[k]); Vec16<T>::load(g + e0, gv[k]); Vec16<T>::load(u + e0, uv[k]); }
    else {
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const bool ok = e0 + e < n;
        av[k][e] = ok ? Vec16<T>::get(da + e0 + e) : 0.f;
        gv[k][e] = ok ? Vec16<T>::get(g + e0 + e) : 0.f;
        uv[k][e] = ok ? Vec16<T>::get(u + e0 + e) : 0.f;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < STEPS; ++k) {
    const int64_t e0 = base + static_cast<int64_t>(k) * 256 * VEC;
    if (e0 >= n) continue;
    float og[VEC], ou[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) swiglu_bwd_elem<Vec16<T>>(av[k][e], gv[k][e], uv[k][e], og[e], ou[e]);
    if (e0 + VEC <= n) { Vec16<T>::store(dg + e0, og); Vec16<T>::store(du + e0, ou); }
    else
      for (int e = 0; e < VEC && e0 + e < n; ++e) { Vec16<T>::put(dg + e0 + e, og[e]); Vec16<T>::put(du + e0 + e, ou[e]); }
  }
}

// ---------------------------------------------------------------------------------------------------
// RMSNorm with the residual add in front of it, forward and backward, one wave per row (the row stays in registers between
// the reduction and the scaling: every byte moves once).
//   forward : h = rb(res + delta)   [ADD; h = x otherwise]     rstd = rsqrt(mean(h^2) + eps)     y = rb(w * rb(h * rstd))
//             - the two roundings of transformers' LlamaRMSNorm (hidden.to(input_dtype), then the product with the weight)
//   backward: g = dy * w;  xh = h * rstd;  dx = rstd * (g - xh * mean(g * xh))  [+ dres: the gradient that reaches h through
//             the residual path, ADD]  - f32 throughout, rounded once
// torch's own kernels for the same work in the cfg3 step: add 17.8 us + rms_norm 21 us forward, layer_norm_grad_input 60 us +
// add 17 us backward per norm ([4608, 4096] bf16).  Algorithmic bytes: forward (2 or 4) * R * D * el, backward (3 or 4) * R * D * el.
// ---------------------------------------------------------------------------------------------------

template <typename T, int NCH, bool ADD>
__global__ __launch_bounds__(256) void rms_norm_fwd_kernel(const T* __restrict__ x, const T* __restrict__ delta,
                                                           const T* __restrict__ w, T* __restrict__ h_out, T* __restrict__ y,
                                                           float* __restrict__ rstd_out, int R, int D, float eps,
                                                           const unsigned char* __restrict__ live) {
  constexpr int N = Vec16<T>::VEC;
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const int64_t base = static_cast<int64_t>(row) * D;
  if (live && !live[row]) {                      // a dead row (wave-uniform): nothing is read, h, y and rstd leave as zeros
    float z[N];
#pragma unroll
    for (int e = 0; e < N; ++e) z[e] = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int d = (c * 64 + lane) * N;
      if (d < D) {
        if constexpr (ADD) Vec16<T>::store(h_out + base + d, z);
        Vec16<T>::store(y + base + d, z);
      }
    }
    if (lane == 0) rstd_out[row] = 0.f;
    return;
  }
  float v[NCH][N];
  float ss = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = (c * 64 + lane) * N;
    if (d < D) {
      Vec16<T>::load(x + base + d, v[c]);
      if constexpr (ADD) {
        float dl[N];
        Vec16<T>::load(delta + base + d, dl);
#pragma unroll
        for (int e = 0; e < N; ++e) v[c][e] = Vec16<T>::rb(v[c][e] + dl[e]);
        Vec16<T>::store(h_out + base + d, v[c]);
      }
#pragma unroll
      for (int e = 0; e < N; ++e) ss = fmaf(v[c][e], v[c][e], ss);
    }
  }
  ss = wave_sum(ss);
  const float rstd = rsqrtf(ss / static_cast<float>(D) + eps);
  if (lane == 0) rstd_out[row] = rstd;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = (c * 64 + lane) * N;
    if (d < D) {
      float wv[N], o[N];
      Vec16<T>::load(w + d, wv);
#pragma unroll
      for (int e = 0; e < N; ++e) o[e] = Vec16<T>::rb(wv[e] * Vec16<T>::rb(v[c][e] * rstd));
      Vec16<T>::store(y + base + d, o);
    }
  }
}

template <typename T, int NCH, bool ADD>
__global__ __launch_bounds__(256) void rms_norm_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ h,
                                                           const T* __restrict__ w, const float* __restrict__ rstd_in,
                                                           const T* __restrict__ dres, T* __restrict__ dx, int R, int D,
                                                           const unsigned char* __restrict__ live) {
  constexpr int N = Vec16<T>::VEC;
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const int64_t base = static_cast<int64_t>(row) * D;
  if (live && !live[row]) {                      // a dead row (wave-uniform): dx leaves as zeros
    float z[N];
#pragma unroll
    for (int e = 0; e < N; ++e) z[e] = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int d = (c * 64 + lane) * N;
      if (d < D) Vec16<T>::store(dx + base + d, z);
    }
    return;
  }
  const float rstd = rstd_in[row];
  float g[NCH][N], xh[NCH][N];
  float dot = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = (c * 64 + lane) * N;
    if (d < D) {
      float wv[N];
      Vec16<T>::load(dy + base + d, g[c]);
      Vec16<T>::load(h + base + d, xh[c]);
      Vec16<T>::load(w + d, wv);
#pragma unroll
      for (int e = 0; e < N; ++e) {
        g[c][e] *= wv[e];
        xh[c][e] *= rstd;
        dot = fmaf(g[c][e], xh[c][e], dot);
      }
    }
  }
  dot = wave_sum(dot) / static_cast<float>(D);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = (c * 64 + lane) * N;
    if (d < D) {
      float o[N];
#pragma unroll
      for (int e = 0; e < N; ++e) o[e] = rstd * (g[c][e] - xh[c][e] * dot);
      if constexpr (ADD) {
        float r[N];
        Vec16<T>::load(dres + base + d, r);
#pragma unroll
        for (int e = 0; e < N; ++e) o[e] += r[e];
      }
#pragma unroll
      for (int e = 0; e < N; ++e) o[e] = Vec16<T>::rb(o[e]);
      Vec16<T>::store(dx + base + d, o);
    }
  }
}

// Second form (bf16 rows of up to 8 chunks per lane; the first form takes wider rows): the three streams of a row (dy, h, and
// the residual-path gradient) are requested as raw 16-byte chunks BEFORE the wave reduction - 3 NCH loads in flight per lane
// instead of 2 NCH, then NCH after the reduction - and decoded twice (raw data in registers instead of f32 copies).
// [4608, 4096] bf16, 151 MB: 26.2 -> 23.4 us (profiles/r05_tower_attempts.txt).
template <int NCH, bool ADD>
__global__ __launch_bounds__(256) void rms_norm_bwd_v2_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ h,
                                                              const bf16_t* __restrict__ w, const float* __restrict__ rstd_in,
                                                              const bf16_t* __restrict__ dres, bf16_t* __restrict__ dx, int R, int D,
                                                              const unsigned char* __restrict__ live) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const int64_t base = static_cast<int64_t>(row) * D;
  if (live && !live[row]) {                      // a dead row (wave-uniform): dx leaves as zeros
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int d = (c * 64 + lane) * 8;
      if (d < D) *reinterpret_cast<uint4*>(dx + base + d) = make_uint4(0u, 0u, 0u, 0u);
    }
    return;
  }
  uint4 rg[NCH], rh[NCH], rr[NCH], rw[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = (c * 64 + lane) * 8;
    const bool ok = d < D;
    rg[c] = ok ? *reinterpret_cast<const uint4*>(dy + base + d) : make_uint4(0u, 0u, 0u, 0u);
    rh[c] = ok ? *reinterpret_cast<const uint4*>(h + base + d) : make_uint4(0u, 0u, 0u, 0u);
    if constexpr (ADD) rr[c] = ok ? *reinterpret_cast<const uint4*>(dres + base + d) : make_uint4(0u, 0u, 0u, 0u);
    rw[c] = ok ? *reinterpret_cast<const uint4*>(w + d) : make_uint4(0u, 0u, 0u, 0u);
  }
  const float rstd = rstd_in[row];
  float dot = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    float g[8], xh[8], wv[8];
    dec8(rg[c], g); dec8(rh[c], xh); dec8(rw[c], wv);
#pragma unroll
    for (int e = 0; e < 8; ++e) dot = fmaf(g[e] * wv[e], xh[e] * rstd, dot);
  }
  dot = wave_sum(dot) / static_cast<float>(D);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = (c * 64 + lane) * 8;
    if (d >= D) continue;
    float g[8], xh[8], wv[8], o[8];
    dec8(rg[c], g); dec8(rh[c], xh); dec8(rw[c], wv);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = rstd * (g[e] * wv[e] - (xh[e] * rstd) * dot);
    if constexpr (ADD) {
      float r[8];
      dec8(rr[c], r);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] += r[e];
    }
    *reinterpret_cast<uint4*>(dx + base + d) = make_uint4(pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]),
                                                           pack_bf16x2(o[4], o[5]), pack_bf16x2(o[6], o[7]));
  }
}

}  // namespace
}  // namespace dalm

using namespace dalm;

extern "C" int dalm_rope_qk_live(const void* q, const void* k, void* q_out, void* k_out, const void* cos, const void* sin, int dtype,
                                 int64_t B, int64_t T, int64_t Hq, int64_t Hk, int64_t hd, const int64_t* q_strides,
                                 const int64_t* k_strides, const int64_t* qo_strides, const int64_t* ko_strides,
                                 const int64_t* cs_strides, int backward, const uint8_t* row_live, dalm_stream_t stream) {
  DALM_REQUIRE(q && k && q_out && k_out && cos && sin && q_strides && k_strides && qo_strides && ko_strides && cs_strides,
               DALM_E_NULL, "null pointer argument");
  DALM_REQUIRE(dtype == DALM_F32 || dtype == DALM_BF16, DALM_E_DTYPE, "dtype must be DALM_F32 or DALM_BF16");
  DALM_REQUIRE(B > 0 && T > 0 && Hq > 0 && Hk >= 0 && hd >= 2 && hd % 2 == 0 && hd <= 4096 && Hq + Hk <= 65535,
               DALM_E_SHAPE, "need B, T, Hq > 0, Hk >= 0, even 2 <= head_dim <= 4096");
  const int64_t rows = B * T * (Hq + Hk);
  DALM_REQUIRE(rows * (hd / 2) < (1ll << 40), DALM_E_SHAPE, "tensor too large for one launch");
  RopeParams p;
  p.q.x = q; p.q.o = q_out; p.k.x = k; p.k.o = k_out;
  const int vec = dtype == DALM_F32 ? 4 : 8;
  bool vector = (hd / 2) % vec == 0 && aligned16(q, k, q_out, k_out, cos, sin);
  for (int i = 0; i < 3; ++i) {
    p.q.xs[i] = q_strides[i]; p.k.xs[i] = k_strides[i]; p.q.os[i] = qo_strides[i]; p.k.os[i] = ko_strides[i];
    vector = vector && q_strides[i] % vec == 0 && k_strides[i] % vec == 0 && qo_strides[i] % vec == 0 && ko_strides[i] % vec == 0;
  }
  p.cos = cos; p.sin = sin; p.cs[0] = cs_strides[0]; p.cs[1] = cs_strides[1];
  vector = vector && cs_strides[0] % vec == 0 && cs_strides[1] % vec == 0;
  p.B = static_cast<int>(B); p.T = static_cast<int>(T); p.Hq = static_cast<int>(Hq); p.Hk = static_cast<int>(Hk);
  p.hd = static_cast<int>(hd); p.backward = backward != 0;
  p.live = row_live;
  const int64_t threads = rows * ((hd / 2) / (vector ? vec : 1));
  const int64_t blocks = (threads + 255) / 256;
  DALM_REQUIRE(blocks <= 0x7fffffffLL, DALM_E_SHAPE, "tensor too large for one launch");
  const dim3 grid(static_cast<unsigned>(blocks));
  hipStream_t s = as_stream(stream);
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    by_bool(vector, [&](auto wide) { hipLaunchKernelGGL((rope_qk_kernel<T, wide>), grid, dim3(256), 0, s, p); });
  });
  return check_launch(__func__);
}

extern "C" int dalm_rope_qk(const void* q, const void* k, void* q_out, void* k_out, const void* cos, const void* sin, int dtype,
                            int64_t B, int64_t T, int64_t Hq, int64_t Hk, int64_t hd, const int64_t* q_strides,
                            const int64_t* k_strides, const int64_t* qo_strides, const int64_t* ko_strides,
                            const int64_t* cs_strides, int backward, dalm_stream_t stream) {
  return dalm_rope_qk_live(q, k, q_out, k_out, cos, sin, dtype, B, T, Hq, Hk, hd, q_strides, k_strides, qo_strides, ko_strides,
                           cs_strides, backward, nullptr, stream);
}

namespace {
// tiles of 256 * VEC elements per workgroup: 8 / 12 sixteen-byte loads in flight per lane (forward / backward).  8 tiles
// measured SLOWER at [4608, 11008] bf16 (forward 70.3 -> 76.2 us, backward 110.7 -> 123.7 us: profiles/r05_tower_attempts.txt)
constexpr int kSwigluSteps = 4;
inline int64_t swiglu_blocks(int64_t n, int vec) {
  const int64_t per = static_cast<int64_t>(kSwigluSteps) * 256 * vec;
  return (n + per - 1) / per;
}
}  // namespace

extern "C" int dalm_swiglu_fwd(const void* gate, const void* up, void* act, int dtype, int64_t n, dalm_stream_t stream) {
  DALM_REQUIRE(n >= 0, DALM_E_SHAPE, "n must be >= 0");
  if (n == 0) return 0;
  DALM_REQUIRE(gate && up && act, DALM_E_NULL, "null pointer argument");
  DALM_REQUIRE(dtype == DALM_F32 || dtype == DALM_BF16, DALM_E_DTYPE, "dtype must be DALM_F32 or DALM_BF16");
  DALM_REQUIRE(aligned16(gate, up, act), DALM_E_ALIGN, "gate / up / act must be 16-byte aligned");
  const int64_t blocks = swiglu_blocks(n, dtype == DALM_F32 ? 4 : 8);
  DALM_REQUIRE(blocks <= 0x7fffffffLL, DALM_E_SHAPE, "n too large for one launch");
  const dim3 grid(static_cast<unsigned>(blocks));
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((swiglu_fwd_kernel<T, kSwigluSteps>), grid, dim3(256), 0, as_stream(stream),
                       static_cast<const T*>(gate), static_cast<const T*>(up), static_cast<T*>(act), n);
  });
  return check_launch(__func__);
}

extern "C" int dalm_swiglu_bwd(const void* d_act, const void* gate, const void* up, void* d_gate, void* d_up, int dtype,
                               int64_t n, dalm_stream_t stream) {
  DALM_REQUIRE(n >= 0, DALM_E_SHAPE, "n must be >= 0");
  if (n == 0) return 0;
  DALM_REQUIRE(d_act && gate && up && d_gate && d_up, DALM_E_NULL, "null pointer argument");
  DALM_REQUIRE(dtype == DALM_F32 || dtype == DALM_BF16, DALM_E_DTYPE, "dtype must be DALM_F32 or DALM_BF16");
  DALM_REQUIRE(aligned16(d_act, gate, up, d_gate, d_up), DALM_E_ALIGN,
               "all tensors must be 16-byte aligned");
  const int64_t blocks = swiglu_blocks(n, dtype == DALM_F32 ? 4 : 8);
  DALM_REQUIRE(blocks <= 0x7fffffffLL, DALM_E_SHAPE, "n too large for one launch");
  const dim3 grid(static_cast<unsigned>(blocks));
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((swiglu_bwd_kernel<T, kSwigluSteps>), grid, dim3(256), 0, as_stream(stream),
                       static_cast<const T*>(d_act), static_cast<const T*>(gate), static_cast<const T*>(up),
                       static_cast<T*>(d_gate), static_cast<T*>(d_up), n);
  });
  return check_launch(__func__);
}

extern "C" int dalm_swiglu_fwd_2d_live(const void* gate, const void* up, void* act, int dtype, int64_t R, int64_t C, int64_t ld_gate,
                                       int64_t ld_up, int64_t ld_act, const uint8_t* row_live, dalm_stream_t stream) {
  DALM_REQUIRE(R >= 0 && C >= 0, DALM_E_SHAPE, "R, C must be >= 0");
  if (R == 0 || C == 0) return 0;
  DALM_REQUIRE(gate && up && act, DALM_E_NULL, "null pointer argument");
  DALM_REQUIRE(dtype == DALM_F32 || dtype == DALM_BF16, DALM_E_DTYPE, "dtype must be DALM_F32 or DALM_BF16");
  const int vec = dtype == DALM_F32 ? 4 : 8;
  DALM_REQUIRE(aligned16(gate, up, act) && C % vec == 0 && ld_gate % vec == 0 && ld_up % vec == 0 && ld_act % vec == 0
                   && ld_gate >= C && ld_up >= C && ld_act >= C,
               DALM_E_ALIGN, "16-byte aligned pointers, C and the row strides multiples of 16 bytes, strides >= C");
  const int64_t n = R * C, blocks = swiglu_blocks(n, vec);
  DALM_REQUIRE(n < (1ll << 32) && blocks <= 0x7fffffffLL, DALM_E_SHAPE, "tensor too large for one launch (R C must stay below 2^32)");
  const dim3 grid(static_cast<unsigned>(blocks));
  const SwigluLd ld = {C, ld_gate, ld_up, ld_act, 0, 0};
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((swiglu_fwd_2d_kernel<T, kSwigluSteps>), grid, dim3(256), 0, as_stream(stream),
                       static_cast<const T*>(gate), static_cast<const T*>(up), static_cast<T*>(act), n, ld, row_live);
  });
  return check_launch(__func__);
}

extern "C" int dalm_swiglu_fwd_2d(const void* gate, const void* up, void* act, int dtype, int64_t R, int64_t C, int64_t ld_gate,
                                  int64_t ld_up, int64_t ld_act, dalm_stream_t stream) {
  return dalm_swiglu_fwd_2d_live(gate, up, act, dtype, R, C, ld_gate, ld_up, ld_act, nullptr, stream);
}

extern "C" int dalm_swiglu_bwd_2d_live(const void* d_act, const void* gate, const void* up, void* d_gate, void* d_up, int dtype,
                                       int64_t R, int64_t C, int64_t ld_dact, int64_t ld_gate, int64_t ld_up, int64_t ld_dgate,
                                       int64_t ld_dup, const uint8_t* row_live, dalm_stream_t stream) {
  DALM_REQUIRE(R >= 0 && C >= 0, DALM_E_SHAPE, "R, C must be >= 0");
  if (R == 0 || C == 0) return 0;
  DALM_REQUIRE(d_act && gate && up && d_gate && d_up, DALM_E_NULL, "null pointer argument");
  DALM_REQUIRE(dtype == DALM_F32 || dtype == DALM_BF16, DALM_E_DTYPE, "dtype must be DALM_F32 or DALM_BF16");
  const int vec = dtype == DALM_F32 ? 4 : 8;
  bool ok = aligned16(d_act, gate, up, d_gate, d_up) && C % vec == 0;
  for (int64_t l : {ld_dact, ld_gate, ld_up, ld_dgate, ld_dup}) ok = ok && l % vec == 0 && l >= C;
  DALM_REQUIRE(ok, DALM_E_ALIGN, "16-byte aligned pointers, C and the row strides multiples of 16 bytes, strides >= C");
  const int64_t n = R * C, blocks = swiglu_blocks(n, vec);
  DALM_REQUIRE(n < (1ll << 32) && blocks <= 0x7fffffffLL, DALM_E_SHAPE, "tensor too large for one launch (R C must stay below 2^32)");
  const dim3 grid(static_cast<unsigned>(blocks));
  const SwigluLd ld = {C, ld_gate, ld_up, ld_dact, ld_dgate, ld_dup};
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((swiglu_bwd_2d_kernel<T, kSwigluSteps>), grid, dim3(256), 0, as_stream(stream),
                       static_cast<const T*>(d_act), static_cast<const T*>(gate), static_cast<const T*>(up),
                       static_cast<T*>(d_gate), static_cast<T*>(d_up), n, ld, row_live);
  });
  return check_launch(__func__);
}

extern "C" int dalm_swiglu_bwd_2d(const void* d_act, const void* gate, const void* up, void* d_gate, void* d_up, int dtype, int64_t R,
                                  int64_t C, int64_t ld_dact, int64_t ld_gate, int64_t ld_up, int64_t ld_dgate, int64_t ld_dup,
                                  dalm_stream_t stream) {
  return dalm_swiglu_bwd_2d_live(d_act, gate, up, d_gate, d_up, dtype, R, C, ld_dact, ld_gate, ld_up, ld_dgate, ld_dup, nullptr, stream);
}

// the contiguous layout with a row structure ([R, C], row stride C).  Without `row_live` these are dalm_swiglu_{fwd,bwd} over R C
// elements; with it the rows go through the strided kernels (the same arithmetic, statement for statement), which know a vector's row
extern "C" int dalm_swiglu_fwd_live(const void* gate, const void* up, void* act, int dtype, int64_t R, int64_t C,
                                    const uint8_t* row_live, dalm_stream_t stream) {
  DALM_REQUIRE(R >= 0 && C >= 0, DALM_E_SHAPE, "R, C must be >= 0");
  if (!row_live) return dalm_swiglu_fwd(gate, up, act, dtype, R * C, stream);
  return dalm_swiglu_fwd_2d_live(gate, up, act, dtype, R, C, C, C, C, row_live, stream);
}

extern "C" int dalm_swiglu_bwd_live(const void* d_act, const void* gate, const void* up, void* d_gate, void* d_up, int dtype,
                                    int64_t R, int64_t C, const uint8_t* row_live, dalm_stream_t stream) {
  DALM_REQUIRE(R >= 0 && C >= 0, DALM_E_SHAPE, "R, C must be >= 0");
  if (!row_live) return dalm_swiglu_bwd(d_act, gate, up, d_gate, d_up, dtype, R * C, stream);
  return dalm_swiglu_bwd_2d_live(d_act, gate, up, d_gate, d_up, dtype, R, C, C, C, C, C, C, row_live, stream);
}

#define DALM_RMS_CHECKS                                                                                                  \
  DALM_REQUIRE(dtype == DALM_F32 || dtype == DALM_BF16, DALM_E_DTYPE, "dtype must be DALM_F32 or DALM_BF16");             \
  const int vecn = dtype == DALM_F32 ? 4 : 8;                                                                            \
  DALM_REQUIRE(R > 0 && D > 0 && D % vecn == 0 && D <= 64ll * vecn * 16 && R <= 0x7ffffff0ll, DALM_E_SHAPE,               \
               "need rows > 0 and a width that is a multiple of 16 bytes, at most 8192 (bf16) / 4096 (f32) elements");    \
  const int nch = static_cast<int>((D + 64 * vecn - 1) / (64 * vecn));                                                   \
  const dim3 grid(static_cast<unsigned>((R + 3) / 4))

extern "C" int dalm_rms_norm_fwd_live(const void* x, const void* delta, const void* w, int dtype, int64_t R, int64_t D, float eps,
                                      void* h_out, void* y, float* rstd, const uint8_t* row_live, dalm_stream_t stream) {
  DALM_REQUIRE(x && w && y && rstd, DALM_E_NULL, "null pointer argument");
  DALM_REQUIRE((delta == nullptr) == (h_out == nullptr), DALM_E_NULL, "delta and h_out go together");
  DALM_RMS_CHECKS;
  DALM_REQUIRE(aligned16(x, w, y, delta, h_out), DALM_E_ALIGN, "tensors must be 16-byte aligned");
  const int Ri = static_cast<int>(R), Di = static_cast<int>(D);
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    by_bool(delta != nullptr, [&](auto add) {
      by_ceil<1, 2, 4, 8, 16>(nch, [&](auto n) {
        hipLaunchKernelGGL((rms_norm_fwd_kernel<T, n, add>), grid, dim3(256), 0, as_stream(stream), static_cast<const T*>(x),
                           static_cast<const T*>(delta), static_cast<const T*>(w), static_cast<T*>(h_out), static_cast<T*>(y), rstd,
                           Ri, Di, eps, row_live);
      });
    });
  });
  return check_launch(__func__);
}

extern "C" int dalm_rms_norm_fwd(const void* x, const void* delta, const void* w, int dtype, int64_t R, int64_t D, float eps,
                                 void* h_out, void* y, float* rstd, dalm_stream_t stream) {
  return dalm_rms_norm_fwd_live(x, delta, w, dtype, R, D, eps, h_out, y, rstd, nullptr, stream);
}

extern "C" int dalm_rms_norm_bwd_live(const void* dy, const void* h, const void* w, const float* rstd, const void* dres, int dtype,
                                      int64_t R, int64_t D, void* dx, const uint8_t* row_live, dalm_stream_t stream) {
  DALM_REQUIRE(dy && h && w && rstd && dx, DALM_E_NULL, "null pointer argument");
  DALM_RMS_CHECKS;
  DALM_REQUIRE(aligned16(dy, h, w, dx, dres), DALM_E_ALIGN, "tensors must be 16-byte aligned");
  const int Ri = static_cast<int>(R), Di = static_cast<int>(D);
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    by_bool(dres != nullptr, [&](auto add) {
      by_ceil<1, 2, 4, 8, 16>(nch, [&](auto n) {
        const auto launch = [&](auto kernel) {
          hipLaunchKernelGGL(kernel, grid, dim3(256), 0, as_stream(stream), static_cast<const T*>(dy), static_cast<const T*>(h),
                             static_cast<const T*>(w), rstd, static_cast<const T*>(dres), static_cast<T*>(dx), Ri, Di, row_live);
        };
        // bf16 rows of up to 8 chunks take the second form; the first form exists for f32 and for the 16-chunk bf16 rows only
        if constexpr (std::is_same_v<T, bf16_t> && n <= 8) launch(rms_norm_bwd_v2_kernel<n, add>);
        else launch(rms_norm_bwd_kernel<T, n, add>);
      });
    });
  });
  return check_launch(__func__);
}

extern "C" int dalm_rms_norm_bwd(const void* dy, const void* h, const void* w, const float* rstd, const void* dres, int dtype,
                                 int64_t R, int64_t D, void* dx, dalm_stream_t stream) {
  return dalm_rms_norm_bwd_live(dy, h, w, rstd, dres, dtype, R, D, dx, nullptr, stream);
}

// ---------------------------------------------------------------------------------------------------
// Qwen3: RMSNorm over the HEAD dimension of q and of k (q_norm / k_norm, one weight [hd] for all heads) followed by the rotary
// embedding, one launch for q and k; and the backward of the norm alone (the rotation's backward is in dalm_attn_bwd's
// epilogues).  transformers runs Qwen3RMSNorm x 2 and apply_rotary_pos_emb as ~12 eager launches forward (modeling_qwen3.py).
// A head row of hd bf16 is hd / 8 sixteen-byte accesses: a GROUP of 16 (hd 128) or 8 (hd 64) adjacent lanes holds it, a wave
// 4 or 8 head rows, rows walked head-fastest like rope_qk_kernel (q's rows first, then k's).  The mean is an xor-shuffle reduction inside the group; the
// rotary partner of a lane's 8 elements (hd / 2 columns away) sits in lane ^ (group / 2).  Every lane of a wave runs the
// shuffles - a group past the last row or of a dead (b, t) carries zeros, loads nothing and (in range) stores zeros.
//   forward :  rstd = rsqrt(mean(x^2) + eps)   xh = rb(x rstd)   y = rb(w xh)   out = rope forward of y (rounding as above)
//   backward:  gw = g w;  xh = x rstd (f32);  dx = rb(rstd (gw - xh mean(gw xh)))     - dalm_rms_norm_bwd's arithmetic
// Algorithmic bytes: forward 2 (|q| + |k|) el + rstd, backward 3 (|q| + |k|) el + rstd (+ cos / sin / w, shared).
// ---------------------------------------------------------------------------------------------------
namespace {

struct HeadNormTensor {
  const void* x;                 // pre-norm projection output, [B, H, T, hd] view
  const void* g;                 // backward: gradient of the normed, un-rotated value
  void* o;                       // forward: normed + rotated; backward: gradient of x
  const void* w;                 // [hd]
  float* rstd;                   // [B, T, H] f32: written by the forward, read by the backward
  int64_t xs[3], gs[3], os[3];   // element strides of (b, h, t)
  float eps;
};
struct HeadNormParams {
  HeadNormTensor q, k;
  const void* cos; const void* sin; int64_t cs[2];   // strides of (b, t); forward only
  int B, T, Hq, Hk;
  unsigned q_blocks;                                 // workgroups that serve q; the rest serve k
  const unsigned char* live;                         // [B * T] or NULL
};

template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// where lane `gid` works: head row -> (b, t, head of q or k); `in`: the row exists, `act`: and its (b, t) is live.  Workgroups
// [0, q_blocks) walk the head rows of q, the rest those of k: which tensor a workgroup serves is uniform, so its pointers and
// strides are chosen by scalar selects (a per-lane choice between the two sets cost the first form ~60 VALU operations a lane)
struct HeadRow { bool in, act, is_k; int b, t, head, c; unsigned bt, row; };
template <int G>
__device__ __forceinline__ HeadRow head_row(const HeadNormParams& p) {
  HeadRow r;
  r.is_k = blockIdx.x >= p.q_blocks;
  const unsigned H = static_cast<unsigned>(r.is_k ? p.Hk : p.Hq);
  const unsigned gid = (r.is_k ? blockIdx.x - p.q_blocks : blockIdx.x) * 256u + threadIdx.x;   // the launcher keeps rows * G below 2^31
  const unsigned row = gid / G;
  r.c = static_cast<int>(gid % G) * 8;
  r.in = row < static_cast<unsigned>(p.B) * p.T * H;
  r.row = r.in ? row : 0u;                                  // also the index into rstd [B, T, H]
  r.head = static_cast<int>(r.row % H);
  r.bt = r.row / H;
  r.t = static_cast<int>(r.bt % p.T); r.b = static_cast<int>(r.bt / p.T);
  r.act = r.in && (!p.live || p.live[r.bt]);
  return r;
}
__device__ __forceinline__ int64_t head_at(const HeadRow& r, const int64_t (&s)[3]) {
  return r.b * s[0] + r.head * s[1] + r.t * s[2] + r.c;
}

template <int HD>
__global__ __launch_bounds__(256) void head_norm_rope_fwd_kernel(const HeadNormParams p) {
#pragma clang fp contract(off)   // the eager chain is separate mul and add kernels (see rope_qk_kernel)
  using V = Vec16<bf16_t>;
  constexpr int G = HD / 8;
  const HeadRow r = head_row<G>(p);
  const HeadNormTensor& R = r.is_k ? p.k : p.q;
  float x[8], w[8], cs[8], sn[8], y[8], o[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] = w[e] = cs[e] = sn[e] = 0.f;
  if (r.act) {                                   // every load of the row in flight before the reduction
    const int64_t ca = r.b * p.cs[0] + r.t * p.cs[1] + r.c;
    V::load(static_cast<const bf16_t*>(R.x) + head_at(r, R.xs), x);
    V::load(static_cast<const bf16_t*>(R.w) + r.c, w);
    V::load(static_cast<const bf16_t*>(p.cos) + ca, cs);
    V::load(static_cast<const bf16_t*>(p.sin) + ca, sn);
  }
  float ss = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) ss = fmaf(x[e], x[e], ss);
  ss = group_sum<G>(ss);
  const float rstd = r.act ? rsqrtf(ss / static_cast<float>(HD) + R.eps) : 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) y[e] = V::rb(w[e] * V::rb(x[e] * rstd));
  // the other half of the head row: y is exact in bf16, so it travels as four packed words
  const uint4 mine = enc8(y);
  float z[8];
  dec8(make_uint4(__shfl_xor(mine.x, G / 2, 64), __shfl_xor(mine.y, G / 2, 64), __shfl_xor(mine.z, G / 2, 64),
                  __shfl_xor(mine.w, G / 2, 64)), z);
  const bool second = r.c >= HD / 2;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float a = V::rb(y[e] * cs[e]), b = V::rb(z[e] * sn[e]);
    o[e] = V::rb(second ? a + b : a - b);
  }
  if (!r.in) return;
  V::store(static_cast<bf16_t*>(R.o) + head_at(r, R.os), o);                     // a dead row: zeros
  if (r.c == 0) R.rstd[r.row] = rstd;
}

template <int HD>
__global__ __launch_bounds__(256) void head_norm_bwd_kernel(const HeadNormParams p) {
  using V = Vec16<bf16_t>;
  constexpr int G = HD / 8;
  const HeadRow r = head_row<G>(p);
  const HeadNormTensor& R = r.is_k ? p.k : p.q;
  float g[8], xh[8], w[8], o[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) g[e] = xh[e] = w[e] = 0.f;
  float rstd = 0.f;
  if (r.act) {
    V::load(static_cast<const bf16_t*>(R.g) + head_at(r, R.gs), g);
    V::load(static_cast<const bf16_t*>(R.x) + head_at(r, R.xs), xh);
    V::load(static_cast<const bf16_t*>(R.w) + r.c, w);
    rstd = R.rstd[r.row];
  }
  float dot = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    g[e] *= w[e];
    xh[e] *= rstd;
    dot = fmaf(g[e], xh[e], dot);
  }
  dot = group_sum<G>(dot) / static_cast<float>(HD);
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = rstd * (g[e] - xh[e] * dot);
  if (!r.in) return;
  V::store(static_cast<bf16_t*>(R.o) + head_at(r, R.os), o);                     // rounded once; a dead row: zeros
}

// the checks the two entry points share; fills B, T, Hq, Hk and the grid
int head_norm_shape(const char* fn, int64_t B, int64_t T, int64_t Hq, int64_t Hk, int64_t hd, HeadNormParams& p, dim3& grid) {
  if (!(hd == 64 || hd == 128)) return fail(DALM_E_SHAPE, fn, "head width must be 64 or 128");
  if (!(B > 0 && T > 0 && Hq > 0 && Hk > 0 && Hq + Hk <= 65535)) return fail(DALM_E_SHAPE, fn, "need B, T, Hq, Hk > 0");
  if (!(B <= 0x7fffffffLL && T <= 0x7fffffffLL && B * T <= 0x7fffffffLL && B * T * (Hq + Hk) * (hd / 8) <= 0x7fffffffLL))
    return fail(DALM_E_SHAPE, fn, "tensor too large for one launch");
  p.B = static_cast<int>(B); p.T = static_cast<int>(T); p.Hq = static_cast<int>(Hq); p.Hk = static_cast<int>(Hk);
  const int64_t qb = (B * T * Hq * (hd / 8) + 255) / 256, kb = (B * T * Hk * (hd / 8) + 255) / 256;
  p.q_blocks = static_cast<unsigned>(qb);
  grid = dim3(static_cast<unsigned>(qb + kb));
  return 0;
}
bool strides_mult8(const int64_t* s, int n) {
  for (int i = 0; i < n; ++i)
    if (s[i] % 8 != 0) return false;
  return true;
}

}  // namespace

extern "C" int dalm_head_norm_rope_fwd(const void* q, const void* k, const void* wq, const void* wk, float eps_q, float eps_k,
                                       const void* cos, const void* sin, int64_t B, int64_t T, int64_t Hq, int64_t Hk, int64_t hd,
                                       const int64_t* q_strides, const int64_t* k_strides, const int64_t* qo_strides,
                                       const int64_t* ko_strides, const int64_t* cs_strides, void* q_out, void* k_out,
                                       float* rstd_q, float* rstd_k, const uint8_t* row_live, dalm_stream_t stream) {
  DALM_REQUIRE(q && k && wq && wk && cos && sin && q_strides && k_strides && qo_strides && ko_strides && cs_strides && q_out && k_out
                   && rstd_q && rstd_k, DALM_E_NULL, "null pointer argument");
  HeadNormParams p;
  dim3 grid;
  if (const int rc = head_norm_shape(__func__, B, T, Hq, Hk, hd, p, grid)) return rc;
  DALM_REQUIRE(aligned16(q, k, wq, wk, cos, sin, q_out, k_out) && reinterpret_cast<uintptr_t>(rstd_q) % 4 == 0
                   && reinterpret_cast<uintptr_t>(rstd_k) % 4 == 0 && strides_mult8(q_strides, 3) && strides_mult8(k_strides, 3)
                   && strides_mult8(qo_strides, 3) && strides_mult8(ko_strides, 3) && strides_mult8(cs_strides, 2),
               DALM_E_ALIGN, "tensors must be 16-byte aligned and every stride a multiple of 8 elements");
  p.q.x = q; p.q.g = nullptr; p.q.o = q_out; p.q.w = wq; p.q.rstd = rstd_q; p.q.eps = eps_q;
  p.k.x = k; p.k.g = nullptr; p.k.o = k_out; p.k.w = wk; p.k.rstd = rstd_k; p.k.eps = eps_k;
  for (int i = 0; i < 3; ++i) {
    p.q.xs[i] = q_strides[i]; p.q.os[i] = qo_strides[i]; p.q.gs[i] = 0;
    p.k.xs[i] = k_strides[i]; p.k.os[i] = ko_strides[i]; p.k.gs[i] = 0;
  }
  p.cos = cos; p.sin = sin; p.cs[0] = cs_strides[0]; p.cs[1] = cs_strides[1];
  p.live = row_live;
  by_exact<64, 128>(static_cast<int>(hd), [&](auto width) {
    hipLaunchKernelGGL((head_norm_rope_fwd_kernel<width>), grid, dim3(256), 0, as_stream(stream), p);
  });
  return check_launch(__func__);
}

extern "C" int dalm_head_norm_bwd(const void* gq, const void* gk, const void* q, const void* k, const void* wq, const void* wk,
                                  const float* rstd_q, const float* rstd_k, int64_t B, int64_t T, int64_t Hq, int64_t Hk, int64_t hd,
                                  const int64_t* gq_strides, const int64_t* gk_strides, const int64_t* q_strides,
                                  const int64_t* k_strides, const int64_t* dq_strides, const int64_t* dk_strides, void* dq, void* dk,
                                  const uint8_t* row_live, dalm_stream_t stream) {
  DALM_REQUIRE(gq && gk && q && k && wq && wk && rstd_q && rstd_k && gq_strides && gk_strides && q_strides && k_strides && dq_strides
                   && dk_strides && dq && dk, DALM_E_NULL, "null pointer argument");
  HeadNormParams p;
  dim3 grid;
  if (const int rc = head_norm_shape(__func__, B, T, Hq, Hk, hd, p, grid)) return rc;
  DALM_REQUIRE(aligned16(gq, gk, q, k, wq, wk, dq, dk) && reinterpret_cast<uintptr_t>(rstd_q) % 4 == 0
                   && reinterpret_cast<uintptr_t>(rstd_k) % 4 == 0 && strides_mult8(gq_strides, 3) && strides_mult8(gk_strides, 3)
                   && strides_mult8(q_strides, 3) && strides_mult8(k_strides, 3) && strides_mult8(dq_strides, 3)
                   && strides_mult8(dk_strides, 3),
               DALM_E_ALIGN, "tensors must be 16-byte aligned and every stride a multiple of 8 elements");
  p.q.x = q; p.q.g = gq; p.q.o = dq; p.q.w = wq; p.q.rstd = const_cast<float*>(rstd_q); p.q.eps = 0.f;
  p.k.x = k; p.k.g = gk; p.k.o = dk; p.k.w = wk; p.k.rstd = const_cast<float*>(rstd_k); p.k.eps = 0.f;
  for (int i = 0; i < 3; ++i) {
    p.q.xs[i] = q_strides[i]; p.q.gs[i] = gq_strides[i]; p.q.os[i] = dq_strides[i];
    p.k.xs[i] = k_strides[i]; p.k.gs[i] = gk_strides[i]; p.k.os[i] = dk_strides[i];
  }
  p.cos = nullptr; p.sin = nullptr; p.cs[0] = p.cs[1] = 0;
  p.live = row_live;
  by_exact<64, 128>(static_cast<int>(hd), [&](auto width) {
    hipLaunchKernelGGL((head_norm_bwd_kernel<width>), grid, dim3(256), 0, as_stream(stream), p);
  });
  return check_launch(__func__);
}

// ---------------------------------------------------------------------------------------------------
// Gemma (modeling_gemma.py): the two row-wise formulas of its decoder layer that differ from Llama's.
//   GemmaMLP      down(gelu_tanh(gate(x)) * up(x))                                        - dalm_geglu_{fwd,bwd}
//   GemmaRMSNorm  (x.float() * rsqrt(mean(x.float()^2) + eps) * (1 + w.float())).type_as(x)   - dalm_gemma_norm_{fwd,bwd}
// Rounding points are the eager chain's and its autograd's (rb = a round trip through the tensor dtype):
//   geglu forward :  a = rb(gelu_tanh(g));  act = rb(a u)
//   geglu backward:  du = rb(dact a);  da = rb(dact u);  dg = rb(torch's tanh-GELU backward of da at g)   - a is recomputed
//   norm forward  :  h = rb(x + delta) [with delta];  rstd = rsqrt(mean(h^2) + eps);  y = rb(h rstd (1 + w))   - ONE rounding
//   norm backward :  g = dy (1 + w);  xh = h rstd;  dx = rb(rstd (g - xh mean(g xh)) [+ dres])   - where rms_norm_bwd_kernel adds dres
// Algorithmic bytes: geglu forward 3 R C el, backward 5 R C el; norm forward (2 or 4) R D el, backward (3 or 4) R D el.
// ---------------------------------------------------------------------------------------------------
namespace {

// torch's tanh-GELU in f32, operation for operation (ATen's GeluCUDAKernelImpl / GeluBackwardCUDAKernelImpl, approximate = "tanh")
constexpr float kGeluBeta = 0.7978845608028654f;   // sqrt(2) * (2 / sqrt(pi)) * 0.5
constexpr float kGeluKappa = 0.044715f;
__device__ __forceinline__ float gelu_tanh_f32(float x) {
  const float x_cube = x * x * x;
  const float inner = kGeluBeta * (x + kGeluKappa * x_cube);
  return 0.5f * x * (1.0f + tanhf(inner));
}
__device__ __forceinline__ float gelu_tanh_bwd_f32(float dy, float x) {
  const float x_sq = x * x;
  const float x_cube = x_sq * x;
  const float inner = kGeluBeta * (x + kGeluKappa * x_cube);
  const float tanh_inner = tanhf(inner);
  const float left = 0.5f * x;
  const float right = 1.0f + tanh_inner;
  const float left_derivative = 0.5f * right;
  const float tanh_derivative = 1.0f - tanh_inner * tanh_inner;
  const float inner_derivative = kGeluBeta * (1.0f + 3.0f * kGeluKappa * x_sq);
  const float right_derivative = left * tanh_derivative * inner_derivative;
  return dy * (left_derivative + right_derivative);
}

// [R, C] views with row strides, walked as tiles of 256 vectors by a capped grid: the tile one grid stride further on lies
// step_row rows and step_col columns away (the launcher divides once; a thread divides once, for its first tile)
struct GegluLd { int64_t g, u, a, dg, du; unsigned int C, step_row, step_col; };
template <class Ld>                               // GegluLd, or Relu2Ld further down: the same three tile fields
__device__ __forceinline__ RowCol next_tile(RowCol rc, const Ld& ld) {
  rc.row += ld.step_row;
  rc.col += ld.step_col;
  if (rc.col >= ld.C) { rc.col -= ld.C; ++rc.row; }
  return rc;
}
// tiles a thread has in flight per trip of its grid-stride loop; 1, 2 and 4 were measured by building with
// -DDALM_GEGLU_TILES=<n>
#ifndef DALM_GEGLU_TILES
#define DALM_GEGLU_TILES 2
#endif
constexpr int kGegluTiles = DALM_GEGLU_TILES;
constexpr int kStreamBlocks = 256 * 8;  // 256 CUs x 8 workgroups

template <typename T>
__global__ __launch_bounds__(256) void geglu_fwd_kernel(const T* __restrict__ g, const T* __restrict__ u, T* __restrict__ a,
                                                        int64_t n, GegluLd ld, const unsigned char* __restrict__ live) {
  constexpr int VEC = Vec16<T>::VEC, K = kGegluTiles;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * 256 * VEC;
  int64_t e0 = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) * VEC;
  if (e0 >= n) return;
  RowCol at = row_col(e0, ld.C);
  for (; e0 < n; e0 += K * stride) {
    RowCol rc[K];
    bool in[K], lv[K];
    float gv[K][VEC], uv[K][VEC];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      rc[k] = at;
      at = next_tile(at, ld);
      in[k] = e0 + k * stride < n;
      lv[k] = in[k] && (!live || live[rc[k].row]);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (lv[k]) {
        Vec16<T>::load(g + ld_at(rc[k], ld.g), gv[k]);
        Vec16<T>::load(u + ld_at(rc[k], ld.u), uv[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (!in[k]) continue;
      float o[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) o[e] = lv[k] ? Vec16<T>::rb(__fmul_rn(Vec16<T>::rb(gelu_tanh_f32(gv[k][e])), uv[k][e])) : 0.f;
      Vec16<T>::store(a + ld_at(rc[k], ld.a), o);                    // a dead row: nothing was loaded, zeros leave
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void geglu_bwd_kernel(const T* __restrict__ da, const T* __restrict__ g, const T* __restrict__ u,
                                                        T* __restrict__ dg, T* __restrict__ du, int64_t n, GegluLd ld,
                                                        const unsigned char* __restrict__ live) {
  constexpr int VEC = Vec16<T>::VEC, K = kGegluTiles;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * 256 * VEC;
  int64_t e0 = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) * VEC;
  if (e0 >= n) return;
  RowCol at = row_col(e0, ld.C);
  for (; e0 < n; e0 += K * stride) {
    RowCol rc[K];
    bool in[K], lv[K];
    float dav[K][VEC], gv[K][VEC], uv[K][VEC];                      // d_act, gate, up
#pragma unroll
    for (int k = 0; k < K; ++k) {
      rc[k] = at;
      at = next_tile(at, ld);
      in[k] = e0 + k * stride < n;
      lv[k] = in[k] && (!live || live[rc[k].row]);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (lv[k]) {
        Vec16<T>::load(da + ld_at(rc[k], ld.a), dav[k]);
        Vec16<T>::load(g + ld_at(rc[k], ld.g), gv[k]);
        Vec16<T>::load(u + ld_at(rc[k], ld.u), uv[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (!in[k]) continue;
      float og[VEC], ou[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        if (lv[k]) {
          const float x = gv[k][e];
          const float a = Vec16<T>::rb(gelu_tanh_f32(x));                            // the activation the eager chain saved
          const float d_a = Vec16<T>::rb(__fmul_rn(dav[k][e], uv[k][e]));
          ou[e] = Vec16<T>::rb(__fmul_rn(dav[k][e], a));
          og[e] = Vec16<T>::rb(gelu_tanh_bwd_f32(d_a, x));
        } else {
          og[e] = 0.f; ou[e] = 0.f;
        }
      }
      Vec16<T>::store(dg + ld_at(rc[k], ld.dg), og);
      Vec16<T>::store(du + ld_at(rc[k], ld.du), ou);
    }
  }
}

// N weights from column d on, f32 or bf16 whatever the activations are (the formula casts once, at the end)
template <int N>
__device__ __forceinline__ void load_weight(const void* w, bool w_f32, int d, float (&wv)[N]) {
  if (w_f32) {
    const float* p = static_cast<const float*>(w) + d;
#pragma unroll
    for (int i = 0; i < N; i += 4) {
      const float4 v = *reinterpret_cast<const float4*>(p + i);
      wv[i] = v.x; wv[i + 1] = v.y; wv[i + 2] = v.z; wv[i + 3] = v.w;
    }
  } else {
    const bf16_t* p = static_cast<const bf16_t*>(w) + d;
    if constexpr (N == 8) {
      Vec16<bf16_t>::load(p, wv);
    } else {
      const uint2 v = *reinterpret_cast<const uint2*>(p);
      wv[0] = __uint_as_float(v.x << 16); wv[1] = __uint_as_float(v.x & 0xffff0000u);
      wv[2] = __uint_as_float(v.y << 16); wv[3] = __uint_as_float(v.y & 0xffff0000u);
    }
  }
}

// 16 raw bytes of a row as f32 (rows are kept raw between the reduction and the second pass: 4 registers a chunk, not 8)
__device__ __forceinline__ void dec16(const uint4& v, float (&x)[8]) { dec8(v, x); }
__device__ __forceinline__ void dec16(const uint4& v, float (&x)[4]) {
  x[0] = __uint_as_float(v.x); x[1] = __uint_as_float(v.y); x[2] = __uint_as_float(v.z); x[3] = __uint_as_float(v.w);
}

template <typename T, int NCH, bool ADD>
__global__ __launch_bounds__(256) void gemma_norm_fwd_kernel(const T* __restrict__ x, const T* __restrict__ delta,
                                                             const void* __restrict__ w, bool w_f32, T* __restrict__ h_out,
                                                             T* __restrict__ y, float* __restrict__ rstd_out, int R, int D, float eps,
                                                             const unsigned char* __restrict__ live) {
  constexpr int N = Vec16<T>::VEC;
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const int64_t base = static_cast<int64_t>(row) * D;
  if (live && !live[row]) {                      // a dead row (wave-uniform): nothing is read, h, y and rstd leave as zeros
    float z[N];
#pragma unroll
    for (int e = 0; e < N; ++e) z[e] = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int d = (c * 64 + lane) * N;
      if (d < D) {
        if constexpr (ADD) Vec16<T>::store(h_out + base + d, z);
        Vec16<T>::store(y + base + d, z);
      }
    }
    if (lane == 0) rstd_out[row] = 0.f;
    return;
  }
  float v[NCH][N];
  float ss = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = (c * 64 + lane) * N;
    if (d < D) {
      Vec16<T>::load(x + base + d, v[c]);
      if constexpr (ADD) {
        float dl[N];
        Vec16<T>::load(delta + base + d, dl);
#pragma unroll
        for (int e = 0; e < N; ++e) v[c][e] = Vec16<T>::rb(v[c][e] + dl[e]);
        Vec16<T>::store(h_out + base + d, v[c]);
      }
#pragma unroll
      for (int e = 0; e < N; ++e) ss = fmaf(v[c][e], v[c][e], ss);
    }
  }
  ss = wave_sum(ss);
  const float rstd = rsqrtf(ss / static_cast<float>(D) + eps);
  if (lane == 0) rstd_out[row] = rstd;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = (c * 64 + lane) * N;
    if (d < D) {
      float wv[N], o[N];
      load_weight<N>(w, w_f32, d, wv);
#pragma unroll
      for (int e = 0; e < N; ++e) o[e] = __fmul_rn(__fmul_rn(v[c][e], rstd), 1.0f + wv[e]);   // f32 throughout, rounded by the store
      Vec16<T>::store(y + base + d, o);
    }
  }
}

// PLUS1: Gemma's (1 + w) weight; without it the plain weight in f32 - OLMo-2's norm (dalm_norm_add_bwd, further down), whose weight
// dtype is its own as well
template <typename T, int NCH, bool ADD, bool PLUS1 = true>
__global__ __launch_bounds__(256) void gemma_norm_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ h,
                                                             const void* __restrict__ w, bool w_f32, const float* __restrict__ rstd_in,
                                                             const T* __restrict__ dres, T* __restrict__ dx, int R, int D,
                                                             const unsigned char* __restrict__ live) {
  constexpr int N = Vec16<T>::VEC;
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const int64_t base = static_cast<int64_t>(row) * D;
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  if (live && !live[row]) {                      // a dead row (wave-uniform): dx leaves as zeros
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int d = (c * 64 + lane) * N;
      if (d < D) *reinterpret_cast<uint4*>(dx + base + d) = zero;
    }
    return;
  }
  // the streams of a row are requested as raw 16-byte chunks before the wave reduction and decoded twice (rms_norm_bwd_v2_kernel)
  uint4 rg[NCH], rh[NCH], rr[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = (c * 64 + lane) * N;
    const bool ok = d < D;
    rg[c] = ok ? *reinterpret_cast<const uint4*>(dy + base + d) : zero;
    rh[c] = ok ? *reinterpret_cast<const uint4*>(h + base + d) : zero;
    if constexpr (ADD) rr[c] = ok ? *reinterpret_cast<const uint4*>(dres + base + d) : zero;
  }
  const float rstd = rstd_in[row];
  float dot = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = (c * 64 + lane) * N;
    if (d >= D) continue;
    float g[N], xh[N], wv[N];
    dec16(rg[c], g); dec16(rh[c], xh);
    load_weight<N>(w, w_f32, d, wv);
#pragma unroll
    for (int e = 0; e < N; ++e) dot = fmaf(g[e] * (PLUS1 ? 1.0f + wv[e] : wv[e]), xh[e] * rstd, dot);
  }
  dot = wave_sum(dot) / static_cast<float>(D);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = (c * 64 + lane) * N;
    if (d >= D) continue;
    float g[N], xh[N], wv[N], o[N];
    dec16(rg[c], g); dec16(rh[c], xh);
    load_weight<N>(w, w_f32, d, wv);
#pragma unroll
    for (int e = 0; e < N; ++e) o[e] = rstd * (g[e] * (PLUS1 ? 1.0f + wv[e] : wv[e]) - (xh[e] * rstd) * dot);
    if constexpr (ADD) {
      float r[N];
      dec16(rr[c], r);
#pragma unroll
      for (int e = 0; e < N; ++e) o[e] += r[e];
    }
    Vec16<T>::store(dx + base + d, o);                             // rounded once
  }
}

// the checks the two GeGLU entry points share, after the NULL and dtype checks; fills the grid, the element count and the tile steps
template <class Ld>
int geglu_plan(const char* fn, int dtype, int64_t R, int64_t C, std::initializer_list<int64_t> lds, dim3& grid, int64_t& n, Ld& ld) {
  const int vec = dtype == DALM_F32 ? 4 : 8;
  bool ok = C % vec == 0;
  for (int64_t l : lds) ok = ok && l % vec == 0 && l >= C;
  if (!ok) return fail(DALM_E_ALIGN, fn, "16-byte aligned pointers, C and the row strides multiples of 16 bytes, strides >= C");
  if (R > ((1ll << 32) - 1) / C)                 // C > 0 here; bounded before the product is taken: R C cannot wrap
    return fail(DALM_E_SHAPE, fn, "tensor too large for one launch (R C must stay below 2^32)");
  n = R * C;
  const int64_t tiles = (n + 256 * vec - 1) / (256 * vec), blocks = tiles < kStreamBlocks ? tiles : kStreamBlocks;
  const int64_t stride = blocks * 256 * vec;
  grid = dim3(static_cast<unsigned>(blocks));
  ld.C = static_cast<unsigned int>(C);
  ld.step_row = static_cast<unsigned int>(stride / C);
  ld.step_col = static_cast<unsigned int>(stride % C);
  return 0;
}

}  // namespace

extern "C" int dalm_geglu_fwd(const void* gate, const void* up, void* act, int dtype, int64_t R, int64_t C, int64_t ld_gate,
                              int64_t ld_up, int64_t ld_act, const uint8_t* row_live, dalm_stream_t stream) {
  DALM_REQUIRE(R >= 0 && C >= 0, DALM_E_SHAPE, "R, C must be >= 0");
  if (R == 0 || C == 0) return 0;
  DALM_REQUIRE(gate && up && act, DALM_E_NULL, "null pointer argument");
  DALM_REQUIRE(dtype == DALM_F32 || dtype == DALM_BF16, DALM_E_DTYPE, "dtype must be DALM_F32 or DALM_BF16");
  DALM_REQUIRE(aligned16(gate, up, act), DALM_E_ALIGN, "gate / up / act must be 16-byte aligned");
  dim3 grid;
  int64_t n;
  GegluLd ld = {ld_gate, ld_up, ld_act, 0, 0, 0u, 0u, 0u};
  if (const int rc = geglu_plan(__func__, dtype, R, C, {ld_gate, ld_up, ld_act}, grid, n, ld)) return rc;
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((geglu_fwd_kernel<T>), grid, dim3(256), 0, as_stream(stream), static_cast<const T*>(gate),
                       static_cast<const T*>(up), static_cast<T*>(act), n, ld, row_live);
  });
  return check_launch(__func__);
}

extern "C" int dalm_geglu_bwd(const void* d_act, const void* gate, const void* up, void* d_gate, void* d_up, int dtype, int64_t R,
                              int64_t C, int64_t ld_dact, int64_t ld_gate, int64_t ld_up, int64_t ld_dgate, int64_t ld_dup,
                              const uint8_t* row_live, dalm_stream_t stream) {
  DALM_REQUIRE(R >= 0 && C >= 0, DALM_E_SHAPE, "R, C must be >= 0");
  if (R == 0 || C == 0) return 0;
  DALM_REQUIRE(d_act && gate && up && d_gate && d_up, DALM_E_NULL, "null pointer argument");
  DALM_REQUIRE(dtype == DALM_F32 || dtype == DALM_BF16, DALM_E_DTYPE, "dtype must be DALM_F32 or DALM_BF16");
  DALM_REQUIRE(aligned16(d_act, gate, up, d_gate, d_up), DALM_E_ALIGN, "all tensors must be 16-byte aligned");
  dim3 grid;
  int64_t n;
  GegluLd ld = {ld_gate, ld_up, ld_dact, ld_dgate, ld_dup, 0u, 0u, 0u};
  if (const int rc = geglu_plan(__func__, dtype, R, C, {ld_dact, ld_gate, ld_up, ld_dgate, ld_dup}, grid, n, ld)) return rc;
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((geglu_bwd_kernel<T>), grid, dim3(256), 0, as_stream(stream), static_cast<const T*>(d_act),
                       static_cast<const T*>(gate), static_cast<const T*>(up), static_cast<T*>(d_gate), static_cast<T*>(d_up), n, ld,
                       row_live);
  });
  return check_launch(__func__);
}

// dalm_rms_norm_*'s width rules; the weight has a dtype of its own and no rows is no work
#define DALM_GEMMA_NORM_CHECKS                                                                                           \
  DALM_REQUIRE(dtype == DALM_F32 || dtype == DALM_BF16, DALM_E_DTYPE, "dtype must be DALM_F32 or DALM_BF16");             \
  DALM_REQUIRE(w_dtype == DALM_F32 || w_dtype == DALM_BF16, DALM_E_DTYPE, "w_dtype must be DALM_F32 or DALM_BF16");       \
  const int vecn = dtype == DALM_F32 ? 4 : 8;                                                                            \
  DALM_REQUIRE(R >= 0 && D > 0 && D % vecn == 0 && D <= 64ll * vecn * 16 && R <= 0x7ffffff0ll, DALM_E_SHAPE,              \
               "need rows >= 0 and a width that is a multiple of 16 bytes, at most 8192 (bf16) / 4096 (f32) elements");   \
  const int nch = static_cast<int>((D + 64 * vecn - 1) / (64 * vecn));                                                   \
  const dim3 grid(static_cast<unsigned>((R + 3) / 4))

extern "C" int dalm_gemma_norm_fwd(const void* x, const void* delta, const void* w, int dtype, int w_dtype, int64_t R, int64_t D,
                                   float eps, void* h_out, void* y, float* rstd, const uint8_t* row_live, dalm_stream_t stream) {
  DALM_REQUIRE(x && w && y && rstd, DALM_E_NULL, "null pointer argument");
  DALM_REQUIRE((delta == nullptr) == (h_out == nullptr), DALM_E_NULL, "delta and h_out go together");
  DALM_GEMMA_NORM_CHECKS;
  DALM_REQUIRE(aligned16(x, w, y, delta, h_out), DALM_E_ALIGN, "tensors must be 16-byte aligned");
  if (R == 0) return 0;
  const int Ri = static_cast<int>(R), Di = static_cast<int>(D);
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    by_bool(delta != nullptr, [&](auto add) {
      by_ceil<1, 2, 4, 8, 16>(nch, [&](auto n) {
        hipLaunchKernelGGL((gemma_norm_fwd_kernel<T, n, add>), grid, dim3(256), 0, as_stream(stream), static_cast<const T*>(x),
                           static_cast<const T*>(delta), w, w_dtype == DALM_F32, static_cast<T*>(h_out), static_cast<T*>(y), rstd,
                           Ri, Di, eps, row_live);
      });
    });
  });
  return check_launch(__func__);
}

extern "C" int dalm_gemma_norm_bwd(const void* dy, const void* h, const void* w, const float* rstd, const void* dres, int dtype,
                                   int w_dtype, int64_t R, int64_t D, void* dx, const uint8_t* row_live, dalm_stream_t stream) {
  DALM_REQUIRE(dy && h && w && rstd && dx, DALM_E_NULL, "null pointer argument");
  DALM_GEMMA_NORM_CHECKS;
  DALM_REQUIRE(aligned16(dy, h, w, dx, dres), DALM_E_ALIGN, "tensors must be 16-byte aligned");
  if (R == 0) return 0;
  const int Ri = static_cast<int>(R), Di = static_cast<int>(D);
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    by_bool(dres != nullptr, [&](auto add) {
      by_ceil<1, 2, 4, 8, 16>(nch, [&](auto n) {
        hipLaunchKernelGGL((gemma_norm_bwd_kernel<T, n, add>), grid, dim3(256), 0, as_stream(stream), static_cast<const T*>(dy),
                           static_cast<const T*>(h), w, w_dtype == DALM_F32, rstd, static_cast<const T*>(dres), static_cast<T*>(dx),
                           Ri, Di, row_live);
      });
    });
  });
  return check_launch(__func__);
}

// ---------------------------------------------------------------------------------------------------
// Arcee (modeling_arcee.py; AFM): the decoder layer, attention and norm are Llama's, the MLP is not - no gate:
//   ArceeMLP  down(relu(up(x))^2)     act_fn = ReLUSquaredActivation = torch.square(F.relu(x))            - dalm_relu2_{fwd,bwd}
// Rounding points are the eager chain's and its autograd's (relu2_math.hpp: the live-row up-GEMM's epilogue shares the arithmetic):
//   forward :  act = rb(relu(y)^2)
//   backward:  d_y = rb(d_act rb(2 relu(y))) where relu(y) > 0 or y is NaN, zero elsewhere   - nothing but y was saved
// The GeGLU kernels' walk: [R, C] views with row strides, tiles of 256 vectors, a capped grid, kGegluTiles tiles in flight.
// Algorithmic bytes: forward 2 R C el, backward 3 R C el.
// ---------------------------------------------------------------------------------------------------
namespace {

struct Relu2Ld { int64_t y, a, dy; unsigned int C, step_row, step_col; };

template <typename T>
__global__ __launch_bounds__(256) void relu2_fwd_kernel(const T* __restrict__ y, T* __restrict__ a, int64_t n, Relu2Ld ld,
                                                        const unsigned char* __restrict__ live) {
  constexpr int VEC = Vec16<T>::VEC, K = kGegluTiles;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * 256 * VEC;
  int64_t e0 = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) * VEC;
  if (e0 >= n) return;
  RowCol at = row_col(e0, ld.C);
  for (; e0 < n; e0 += K * stride) {
    RowCol rc[K];
    bool in[K], lv[K];
    float yv[K][VEC];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      rc[k] = at;
      at = next_tile(at, ld);
      in[k] = e0 + k * stride < n;
      lv[k] = in[k] && (!live || live[rc[k].row]);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (lv[k]) Vec16<T>::load(y + ld_at(rc[k], ld.y), yv[k]);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (!in[k]) continue;
      float o[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) o[e] = lv[k] ? relu2_fwd_elem<Vec16<T>>(yv[k][e]) : 0.f;
      Vec16<T>::store(a + ld_at(rc[k], ld.a), o);                    // a dead row: nothing was loaded, zeros leave
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void relu2_bwd_kernel(const T* __restrict__ da, const T* __restrict__ y, T* __restrict__ dy,
                                                        int64_t n, Relu2Ld ld, const unsigned char* __restrict__ live) {
  constexpr int VEC = Vec16<T>::VEC, K = kGegluTiles;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * 256 * VEC;
  int64_t e0 = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) * VEC;
  if (e0 >= n) return;
  RowCol at = row_col(e0, ld.C);
  for (; e0 < n; e0 += K * stride) {
    RowCol rc[K];
    bool in[K], lv[K];
    float dav[K][VEC], yv[K][VEC];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      rc[k] = at;
      at = next_tile(at, ld);
      in[k] = e0 + k * stride < n;
      lv[k] = in[k] && (!live || live[rc[k].row]);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (lv[k]) {
        Vec16<T>::load(da + ld_at(rc[k], ld.a), dav[k]);
        Vec16<T>::load(y + ld_at(rc[k], ld.y), yv[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (!in[k]) continue;
      float o[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) o[e] = lv[k] ? relu2_bwd_elem<Vec16<T>>(dav[k][e], yv[k][e]) : 0.f;
      Vec16<T>::store(dy + ld_at(rc[k], ld.dy), o);
    }
  }
}

}  // namespace

extern "C" int dalm_relu2_fwd(const void* y, void* act, int dtype, int64_t R, int64_t C, int64_t ld_y, int64_t ld_act,
                              const uint8_t* row_live, dalm_stream_t stream) {
  DALM_REQUIRE(R >= 0 && C >= 0, DALM_E_SHAPE, "R, C must be >= 0");
  if (R == 0 || C == 0) return 0;
  DALM_REQUIRE(y && act, DALM_E_NULL, "null pointer argument");
  DALM_REQUIRE(dtype == DALM_F32 || dtype == DALM_BF16, DALM_E_DTYPE, "dtype must be DALM_F32 or DALM_BF16");
  DALM_REQUIRE(aligned16(y, act), DALM_E_ALIGN, "y / act must be 16-byte aligned");
  dim3 grid;
  int64_t n;
  Relu2Ld ld = {ld_y, ld_act, 0, 0u, 0u, 0u};
  if (const int rc = geglu_plan(__func__, dtype, R, C, {ld_y, ld_act}, grid, n, ld)) return rc;
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((relu2_fwd_kernel<T>), grid, dim3(256), 0, as_stream(stream), static_cast<const T*>(y), static_cast<T*>(act), n,
                       ld, row_live);
  });
  return check_launch(__func__);
}

extern "C" int dalm_relu2_bwd(const void* d_act, const void* y, void* d_y, int dtype, int64_t R, int64_t C, int64_t ld_dact,
                              int64_t ld_y, int64_t ld_dy, const uint8_t* row_live, dalm_stream_t stream) {
  DALM_REQUIRE(R >= 0 && C >= 0, DALM_E_SHAPE, "R, C must be >= 0");
  if (R == 0 || C == 0) return 0;
  DALM_REQUIRE(d_act && y && d_y, DALM_E_NULL, "null pointer argument");
  DALM_REQUIRE(dtype == DALM_F32 || dtype == DALM_BF16, DALM_E_DTYPE, "dtype must be DALM_F32 or DALM_BF16");
  DALM_REQUIRE(aligned16(d_act, y, d_y), DALM_E_ALIGN, "all tensors must be 16-byte aligned");
  dim3 grid;
  int64_t n;
  Relu2Ld ld = {ld_y, ld_dact, ld_dy, 0u, 0u, 0u};
  if (const int rc = geglu_plan(__func__, dtype, R, C, {ld_dact, ld_y, ld_dy}, grid, n, ld)) return rc;
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((relu2_bwd_kernel<T>), grid, dim3(256), 0, as_stream(stream), static_cast<const T*>(d_act),
                       static_cast<const T*>(y), static_cast<T*>(d_y), n, ld, row_live);
  });
  return check_launch(__func__);
}

// ---------------------------------------------------------------------------------------------------
// OLMo-2 (modeling_olmo2.py): SwiGLU and the attention are Llama's; two row-wise formulas are not.
//   Olmo2RMSNorm       (w * (x.float() * rsqrt(mean(x.float()^2) + eps))).to(x.dtype)   - the weight enters in f32, ONE rounding
//   Olmo2DecoderLayer  h = residual + norm(sub_block(h)): the norm comes AFTER the sub-block, inside the residual   - dalm_norm_add_*
//   Olmo2Attention     q_norm / k_norm over the WHOLE projection width (all heads of a token), in front of the head split and the
//                      rotary embedding                                               - dalm_row_norm_rope_fwd / dalm_row_norm_bwd
// Rounding points are the eager chain's (rb = a round trip through the tensor dtype):
//   norm_add forward :  rstd = rsqrt(mean(x^2) + eps);  y = rb(w (x rstd));  out = rb(res + y)
//   norm_add backward:  g = dy w;  xh = x rstd;  dx = rb(rstd (g - xh mean(g xh)));  the residual's gradient IS dy (no kernel).  With
//                       the weight in the activation dtype this is dalm_rms_norm_bwd_live without dres, and the entry point calls it;
//                       a weight of the other dtype goes through gemma_norm_bwd_kernel without its (1 + w)
//   row_norm forward :  per (b, t): rstd = rsqrt(mean over H hd of x^2 + eps);  y = rb(w (x rstd));  out = rope forward of y per head
//   row_norm backward:  gw = g w;  xh = x rstd (f32);  dx = rb(rstd (gw - xh mean over H hd of (gw xh)))
// One wave per row, the row kept as raw 16-byte chunks between the reduction and the second pass (rms_norm_bwd_v2_kernel).  In the
// row-norm kernels a chunk of 64 lanes holds 512 / hd whole heads, so the column inside the head - and with it a lane's cos / sin
// vector and its rotary partner lane ^ (hd / 16) - is the same for every chunk: cos / sin are loaded once per lane.
// Algorithmic bytes: norm_add forward 3 R D el, backward 3 R D el; row_norm forward 2 (|q| + |k|) el, backward 3 (|q| + |k|) el.
// ---------------------------------------------------------------------------------------------------
namespace {

// The row statistic of the two forward kernels below: the sum of squares is accumulated in f64 (exact products of f32 values, a sum
// that carries no visible error) and rsqrt(ss / n + eps) is rounded to f32 ONCE - the hardware's f32 estimate (2^-23) and one Newton
// step in f64.  With f32 activations and f32 weights nothing downstream rounds coarser than f32 and torch's own mean and rsqrt are
// that accurate: with an f32 fma chain and the bare instruction, weight gradients of one-row inputs came out at twice the eager
// chain's error.  The arithmetic is a convert and an fma per element, far below the kernels' memory time; the rest is once per row.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ float rstd_of(double ss, int n, float eps) {
  const double v = ss / static_cast<double>(n) + static_cast<double>(eps);
  const double r = static_cast<double>(rsqrtf(static_cast<float>(v)));
  return static_cast<float>(r * (1.5 - 0.5 * v * r * r));
}

template <typename T, int NCH>
__global__ __launch_bounds__(256) void norm_add_fwd_kernel(const T* __restrict__ x, const T* __restrict__ res,
                                                           const void* __restrict__ w, bool w_f32, T* __restrict__ out,
                                                           float* __restrict__ rstd_out, int R, int D, float eps,
                                                           const unsigned char* __restrict__ live) {
#pragma clang fp contract(off)   // w (x rstd) and the add are separate eager kernels: in f32 a fused multiply-add would round once less
  constexpr int N = Vec16<T>::VEC;
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const int64_t base = static_cast<int64_t>(row) * D;
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  if (live && !live[row]) {                      // a dead row (wave-uniform): nothing is read, out and rstd leave as zeros
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int d = (c * 64 + lane) * N;
      if (d < D) *reinterpret_cast<uint4*>(out + base + d) = zero;
    }
    if (lane == 0) rstd_out[row] = 0.f;
    return;
  }
  uint4 rx[NCH], rr[NCH];                        // both streams of the row in flight before the reduction
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = (c * 64 + lane) * N;
    const bool ok = d < D;
    rx[c] = ok ? *reinterpret_cast<const uint4*>(x + base + d) : zero;
    rr[c] = ok ? *reinterpret_cast<const uint4*>(res + base + d) : zero;
  }
  double ss = 0.0;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    float v[N];
    dec16(rx[c], v);                             // past the row: zeros
#pragma unroll
    for (int e = 0; e < N; ++e) ss = fma(static_cast<double>(v[e]), static_cast<double>(v[e]), ss);
  }
  const float rstd = rstd_of(wave_sum_f64(ss), D, eps);
  if (lane == 0) rstd_out[row] = rstd;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = (c * 64 + lane) * N;
    if (d >= D) continue;
    float v[N], r[N], wv[N], o[N];
    dec16(rx[c], v); dec16(rr[c], r);
    load_weight<N>(w, w_f32, d, wv);
#pragma unroll
    for (int e = 0; e < N; ++e) o[e] = r[e] + Vec16<T>::rb(wv[e] * (v[e] * rstd));
    Vec16<T>::store(out + base + d, o);          // the second rounding
  }
}

// (a value, not a named constant: one whose address the two uses below take was kept in scratch memory)
__device__ __forceinline__ uint4 zero16() { return make_uint4(0u, 0u, 0u, 0u); }

struct RowNormTensor {
  const void* x;                 // pre-norm projection output, [B, H, T, hd] view
  const void* g;                 // backward: gradient of the normed, un-rotated value
  void* o;                       // forward: normed + rotated; backward: gradient of x
  const void* w;                 // [H hd]
  float* rstd;                   // [B, T] f32: written by the forward, read by the backward
  int64_t xs[3], gs[3], os[3];   // element strides of (b, h, t)
  float eps;
  int H;
};
struct RowNormParams {
  RowNormTensor q, k;
  const void* cos; const void* sin; int64_t cs[2];   // strides of (b, t); forward only
  int B, T;
  unsigned q_blocks;                                 // workgroups that serve q (4 tokens each); the rest serve k
  bool w_f32;
  const unsigned char* live;                         // [B * T] or NULL
};

// where a wave works: token (b, t) of q or of k (uniform per workgroup, as in head_row), and its lane inside every 64-lane chunk:
// head c * (64 / G) + lane / G of the chunk c, column (lane % G) * 8 of that head
template <int HD>
struct RowNormAt {
  static constexpr int G = HD / 8, HPC = 64 / G;
  bool in, is_k;
  unsigned bt;
  int b, t, h0, hc;
  __device__ __forceinline__ explicit RowNormAt(const RowNormParams& p) {
    is_k = blockIdx.x >= p.q_blocks;
    bt = (is_k ? blockIdx.x - p.q_blocks : blockIdx.x) * 4u + (threadIdx.x >> 6);
    in = bt < static_cast<unsigned>(p.B) * p.T;
    const int lane = threadIdx.x & 63;
    t = static_cast<int>(bt % p.T); b = static_cast<int>(bt / p.T);
    h0 = lane / G; hc = (lane % G) * 8;
  }
  // a [B, H, T, hd] view with strides s at this lane's (b, t, column): where head 0 starts and how far apart the heads lie
  struct View { int64_t base, hs; __device__ __forceinline__ int64_t operator()(int head) const { return base + head * hs; } };
  __device__ __forceinline__ View view(const int64_t (&s)[3]) const { return {b * s[0] + t * s[2] + hc, s[1]}; }
};

template <int HD, int NCH>
__global__ __launch_bounds__(256) void row_norm_rope_fwd_kernel(const RowNormParams p) {
#pragma clang fp contract(off)   // the eager chain is separate mul and add kernels (see rope_qk_kernel)
  using V = Vec16<bf16_t>;
  using At = RowNormAt<HD>;
  const At r(p);
  if (!r.in) return;                             // wave-uniform, and so is everything up to the lanes' `head < H`
  const RowNormTensor& R = r.is_k ? p.k : p.q;
  const int H = R.H;
  const bf16_t* xp = static_cast<const bf16_t*>(R.x);
  bf16_t* op = static_cast<bf16_t*>(R.o);
  const typename At::View xv = r.view(R.xs), ov = r.view(R.os);
  if (p.live && !p.live[r.bt]) {                 // a dead (b, t): nothing is read, the outputs and rstd leave as zeros
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int head = c * At::HPC + r.h0;
      if (head < H) *reinterpret_cast<uint4*>(op + ov(head)) = zero16();
    }
    if ((threadIdx.x & 63) == 0) R.rstd[r.bt] = 0.f;
    return;
  }
  uint4 rx[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int head = c * At::HPC + r.h0;
    rx[c] = head < H ? *reinterpret_cast<const uint4*>(xp + xv(head)) : zero16();
  }
  float cs[8], sn[8];                            // one vector per lane: the column inside the head does not depend on the chunk
  const int64_t ca = r.b * p.cs[0] + r.t * p.cs[1] + r.hc;
  V::load(static_cast<const bf16_t*>(p.cos) + ca, cs);
  V::load(static_cast<const bf16_t*>(p.sin) + ca, sn);
  double ss = 0.0;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    float x[8];
    dec8(rx[c], x);
#pragma unroll
    for (int e = 0; e < 8; ++e) ss = fma(static_cast<double>(x[e]), static_cast<double>(x[e]), ss);
  }
  const float rstd = rstd_of(wave_sum_f64(ss), H * HD, R.eps);
  if ((threadIdx.x & 63) == 0) R.rstd[r.bt] = rstd;
  const bool second = r.hc >= HD / 2;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    if (c * At::HPC >= H) break;                 // wave-uniform: every lane of the wave runs the shuffles below or none does
    const int head = c * At::HPC + r.h0;
    const bool ok = head < H;                    // a head's G lanes agree, and the rotary partner is one of them
    float x[8], w[8], y[8], z[8], o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) w[e] = 0.f;
    dec8(rx[c], x);
    if (ok) load_weight<8>(R.w, p.w_f32, head * HD + r.hc, w);
#pragma unroll
    for (int e = 0; e < 8; ++e) y[e] = V::rb(w[e] * (x[e] * rstd));
    // the other half of the head row: y is exact in bf16, so it travels as four packed words (head_norm_rope_fwd_kernel)
    const uint4 mine = enc8(y);
    dec8(make_uint4(__shfl_xor(mine.x, At::G / 2, 64), __shfl_xor(mine.y, At::G / 2, 64), __shfl_xor(mine.z, At::G / 2, 64),
                    __shfl_xor(mine.w, At::G / 2, 64)), z);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float a = V::rb(y[e] * cs[e]), b = V::rb(z[e] * sn[e]);
      o[e] = second ? a + b : a - b;
    }
    if (ok) V::store(op + ov(head), o);
  }
}

template <int HD, int NCH>
__global__ __launch_bounds__(256) void row_norm_bwd_kernel(const RowNormParams p) {
  using V = Vec16<bf16_t>;
  using At = RowNormAt<HD>;
  const At r(p);
  if (!r.in) return;
  const RowNormTensor& R = r.is_k ? p.k : p.q;
  const int H = R.H;
  const bf16_t* gp = static_cast<const bf16_t*>(R.g);
  const bf16_t* xp = static_cast<const bf16_t*>(R.x);
  bf16_t* op = static_cast<bf16_t*>(R.o);
  const typename At::View gv = r.view(R.gs), xv = r.view(R.xs), ov = r.view(R.os);
  if (p.live && !p.live[r.bt]) {                 // a dead (b, t): nothing is read, dx leaves as zeros
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int head = c * At::HPC + r.h0;
      if (head < H) *reinterpret_cast<uint4*>(op + ov(head)) = zero16();
    }
    return;
  }
  uint4 rg[NCH], rx[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int head = c * At::HPC + r.h0;
    const bool ok = head < H;
    rg[c] = ok ? *reinterpret_cast<const uint4*>(gp + gv(head)) : zero16();
    rx[c] = ok ? *reinterpret_cast<const uint4*>(xp + xv(head)) : zero16();
  }
  const float rstd = R.rstd[r.bt];
  float dot = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int head = c * At::HPC + r.h0;
    if (head >= H) continue;
    float g[8], xh[8], w[8];
    dec8(rg[c], g); dec8(rx[c], xh);
    load_weight<8>(R.w, p.w_f32, head * HD + r.hc, w);
#pragma unroll
    for (int e = 0; e < 8; ++e) dot = fmaf(g[e] * w[e], xh[e] * rstd, dot);
  }
  dot = wave_sum(dot) / static_cast<float>(H * HD);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int head = c * At::HPC + r.h0;
    if (head >= H) continue;
    float g[8], xh[8], w[8], o[8];
    dec8(rg[c], g); dec8(rx[c], xh);
    load_weight<8>(R.w, p.w_f32, head * HD + r.hc, w);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = rstd * (g[e] * w[e] - (xh[e] * rstd) * dot);
    V::store(op + ov(head), o);                                                  // rounded once
  }
}

// the checks the two row-norm entry points share; fills B, T, the head counts and the grid, returns the chunk count through `nch`
int row_norm_shape(const char* fn, int64_t B, int64_t T, int64_t Hq, int64_t Hk, int64_t hd, int w_dtype, RowNormParams& p, dim3& grid,
                   int& nch) {
  if (!(w_dtype == DALM_F32 || w_dtype == DALM_BF16)) return fail(DALM_E_DTYPE, fn, "w_dtype must be DALM_F32 or DALM_BF16");
  if (!(hd == 64 || hd == 128)) return fail(DALM_E_SHAPE, fn, "head width must be 64 or 128");
  if (!(B > 0 && T > 0 && Hq > 0 && Hk > 0)) return fail(DALM_E_SHAPE, fn, "need B, T, Hq, Hk > 0");
  if (!(Hq * hd <= 8192 && Hk * hd <= 8192)) return fail(DALM_E_SHAPE, fn, "a row (Hq hd, Hk hd) holds at most 8192 elements");
  if (!(B <= 0x7fffffffLL && T <= 0x7fffffffLL && B * T <= 0x7fffffffLL && B * T * (Hq + Hk) * (hd / 8) <= 0x7fffffffLL))
    return fail(DALM_E_SHAPE, fn, "tensor too large for one launch");
  p.B = static_cast<int>(B); p.T = static_cast<int>(T); p.q.H = static_cast<int>(Hq); p.k.H = static_cast<int>(Hk);
  p.w_f32 = w_dtype == DALM_F32;
  const int64_t blocks = (B * T + 3) / 4, wide = (Hq > Hk ? Hq : Hk) * hd;
  p.q_blocks = static_cast<unsigned>(blocks);
  grid = dim3(static_cast<unsigned>(2 * blocks));
  nch = static_cast<int>((wide + 511) / 512);
  return 0;
}

}  // namespace

extern "C" int dalm_norm_add_fwd(const void* x, const void* res, const void* w, int dtype, int w_dtype, int64_t R, int64_t D, float eps,
                                 void* out, float* rstd, const uint8_t* row_live, dalm_stream_t stream) {
  DALM_REQUIRE(x && res && w && out && rstd, DALM_E_NULL, "null pointer argument");
  DALM_GEMMA_NORM_CHECKS;
  DALM_REQUIRE(aligned16(x, res, w, out), DALM_E_ALIGN, "tensors must be 16-byte aligned");
  if (R == 0) return 0;
  const int Ri = static_cast<int>(R), Di = static_cast<int>(D);
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    by_ceil<1, 2, 4, 8, 16>(nch, [&](auto n) {
      hipLaunchKernelGGL((norm_add_fwd_kernel<T, n>), grid, dim3(256), 0, as_stream(stream), static_cast<const T*>(x),
                         static_cast<const T*>(res), w, w_dtype == DALM_F32, static_cast<T*>(out), rstd, Ri, Di, eps, row_live);
    });
  });
  return check_launch(__func__);
}

extern "C" int dalm_norm_add_bwd(const void* dy, const void* x, const void* w, const float* rstd, int dtype, int w_dtype, int64_t R,
                                 int64_t D, void* dx, const uint8_t* row_live, dalm_stream_t stream) {
  DALM_REQUIRE(dy && x && w && rstd && dx, DALM_E_NULL, "null pointer argument");
  DALM_GEMMA_NORM_CHECKS;
  DALM_REQUIRE(aligned16(dy, x, w, dx), DALM_E_ALIGN, "tensors must be 16-byte aligned");
  if (R == 0) return 0;
  // the weight in the activation dtype: dalm_rms_norm_bwd's arithmetic without a residual-path gradient, rounded where it rounds
  if (w_dtype == dtype) return dalm_rms_norm_bwd_live(dy, x, w, rstd, nullptr, dtype, R, D, dx, row_live, stream);
  const int Ri = static_cast<int>(R), Di = static_cast<int>(D);
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    by_ceil<1, 2, 4, 8, 16>(nch, [&](auto n) {
      hipLaunchKernelGGL((gemma_norm_bwd_kernel<T, n, false, false>), grid, dim3(256), 0, as_stream(stream), static_cast<const T*>(dy),
                         static_cast<const T*>(x), w, w_dtype == DALM_F32, rstd, static_cast<const T*>(nullptr), static_cast<T*>(dx),
                         Ri, Di, row_live);
    });
  });
  return check_launch(__func__);
}

extern "C" int dalm_row_norm_rope_fwd(const void* q, const void* k, const void* wq, const void* wk, int w_dtype, float eps_q,
                                      float eps_k, const void* cos, const void* sin, int64_t B, int64_t T, int64_t Hq, int64_t Hk,
                                      int64_t hd, const int64_t* q_strides, const int64_t* k_strides, const int64_t* qo_strides,
                                      const int64_t* ko_strides, const int64_t* cs_strides, void* q_out, void* k_out, float* rstd_q,
                                      float* rstd_k, const uint8_t* row_live, dalm_stream_t stream) {
  DALM_REQUIRE(q && k && wq && wk && cos && sin && q_strides && k_strides && qo_strides && ko_strides && cs_strides && q_out && k_out
                   && rstd_q && rstd_k, DALM_E_NULL, "null pointer argument");
  RowNormParams p;
  dim3 grid;
  int nch;
  if (const int rc = row_norm_shape(__func__, B, T, Hq, Hk, hd, w_dtype, p, grid, nch)) return rc;
  DALM_REQUIRE(aligned16(q, k, wq, wk, cos, sin, q_out, k_out) && reinterpret_cast<uintptr_t>(rstd_q) % 4 == 0
                   && reinterpret_cast<uintptr_t>(rstd_k) % 4 == 0 && strides_mult8(q_strides, 3) && strides_mult8(k_strides, 3)
                   && strides_mult8(qo_strides, 3) && strides_mult8(ko_strides, 3) && strides_mult8(cs_strides, 2),
               DALM_E_ALIGN, "tensors must be 16-byte aligned and every stride a multiple of 8 elements");
  p.q.x = q; p.q.g = nullptr; p.q.o = q_out; p.q.w = wq; p.q.rstd = rstd_q; p.q.eps = eps_q;
  p.k.x = k; p.k.g = nullptr; p.k.o = k_out; p.k.w = wk; p.k.rstd = rstd_k; p.k.eps = eps_k;
  for (int i = 0; i < 3; ++i) {
    p.q.xs[i] = q_strides[i]; p.q.os[i] = qo_strides[i]; p.q.gs[i] = 0;
    p.k.xs[i] = k_strides[i]; p.k.os[i] = ko_strides[i]; p.k.gs[i] = 0;
  }
  p.cos = cos; p.sin = sin; p.cs[0] = cs_strides[0]; p.cs[1] = cs_strides[1];
  p.live = row_live;
  by_exact<64, 128>(static_cast<int>(hd), [&](auto width) {
    by_ceil<1, 2, 4, 8, 16>(nch, [&](auto n) {
      hipLaunchKernelGGL((row_norm_rope_fwd_kernel<width, n>), grid, dim3(256), 0, as_stream(stream), p);
    });
  });
  return check_launch(__func__);
}

extern "C" int dalm_row_norm_bwd(const void* gq, const void* gk, const void* q, const void* k, const void* wq, const void* wk,
                                 int w_dtype, const float* rstd_q, const float* rstd_k, int64_t B, int64_t T, int64_t Hq, int64_t Hk,
                                 int64_t hd, const int64_t* gq_strides, const int64_t* gk_strides, const int64_t* q_strides,
                                 const int64_t* k_strides, const int64_t* dq_strides, const int64_t* dk_strides, void* dq, void* dk,
                                 const uint8_t* row_live, dalm_stream_t stream) {
  DALM_REQUIRE(gq && gk && q && k && wq && wk && rstd_q && rstd_k && gq_strides && gk_strides && q_strides && k_strides && dq_strides
                   && dk_strides && dq && dk, DALM_E_NULL, "null pointer argument");
  RowNormParams p;
  dim3 grid;
  int nch;
  if (const int rc = row_norm_shape(__func__, B, T, Hq, Hk, hd, w_dtype, p, grid, nch)) return rc;
  DALM_REQUIRE(aligned16(gq, gk, q, k, wq, wk, dq, dk) && reinterpret_cast<uintptr_t>(rstd_q) % 4 == 0
                   && reinterpret_cast<uintptr_t>(rstd_k) % 4 == 0 && strides_mult8(gq_strides, 3) && strides_mult8(gk_strides, 3)
                   && strides_mult8(q_strides, 3) && strides_mult8(k_strides, 3) && strides_mult8(dq_strides, 3)
                   && strides_mult8(dk_strides, 3),
               DALM_E_ALIGN, "tensors must be 16-byte aligned and every stride a multiple of 8 elements");
  p.q.x = q; p.q.g = gq; p.q.o = dq; p.q.w = wq; p.q.rstd = const_cast<float*>(rstd_q); p.q.eps = 0.f;
  p.k.x = k; p.k.g = gk; p.k.o = dk; p.k.w = wk; p.k.rstd = const_cast<float*>(rstd_k); p.k.eps = 0.f;
  for (int i = 0; i < 3; ++i) {
    p.q.xs[i] = q_strides[i]; p.q.gs[i] = gq_strides[i]; p.q.os[i] = dq_strides[i];
    p.k.xs[i] = k_strides[i]; p.k.gs[i] = gk_strides[i]; p.k.os[i] = dk_strides[i];
  }
  p.cos = nullptr; p.sin = nullptr; p.cs[0] = p.cs[1] = 0;
  p.live = row_live;
  by_exact<64, 128>(static_cast<int>(hd), [&](auto width) {
    by_ceil<1, 2, 4, 8, 16>(nch, [&](auto n) {
      hipLaunchKernelGGL((row_norm_bwd_kernel<width, n>), grid, dim3(256), 0, as_stream(stream), p);
    });
  });
  return check_launch(__func__);
}

// ---------------------------------------------------------------------------------------------------
// Granite (modeling_granite.py): a Llama layer whose sub-block outputs enter the residual stream scaled,
//   hidden_states = residual + hidden_states * residual_multiplier        (twice per GraniteDecoderLayer.forward)
// with the multiplier a Python float: torch forms the product in f32 and rounds it to the tensor dtype, then adds and rounds again.
//   scaled norm forward :  t = rb(delta mult);  h = rb(x + t);  rstd = rsqrt(mean(h^2) + eps);  y = rb(w rb(h rstd))
//   scaled norm backward:  g = dy w;  xh = h rstd;  dx = rb(rstd (g - xh mean(g xh)) [+ dres]);  ddelta = rb(dx mult), dx as rounded -
//                          what autograd's backward of the eager multiply makes of the rounded dx, in the same launch
//   scale_add           :  out = rb(res + rb(x mult)), or rb(x mult) without res: the layer's trailing add, its backward, and the
//                          division of the logits by logits_scaling
// With mult == 1 the two norm kernels give the bits of dalm_rms_norm_fwd_live / dalm_rms_norm_bwd_live: the sums run in their order,
// and what the compiler fuses there - fma(-xh, mean, g) and fma(rstd, ., dres) - is written out here, with contraction off for the
// rest (in f32 a fused delta mult + x would round once less than the eager pair).
// One wave per row; the row's streams are requested as raw 16-byte chunks before the reduction (rms_norm_bwd_v2_kernel) and h stays
// in registers, encoded, between the reduction and the scaling.  scale_add has no reduction: a flat grid over 16-byte vectors, four
// in flight per lane.  Algorithmic bytes: forward 4 R D el, backward (4 or 5) R D el, scale_add (2 or 3) R D el.
// ---------------------------------------------------------------------------------------------------
namespace {

__device__ __forceinline__ uint4 enc16(const float (&x)[8]) { return enc8(x); }
__device__ __forceinline__ uint4 enc16(const float (&x)[4]) {
  return make_uint4(__float_as_uint(x[0]), __float_as_uint(x[1]), __float_as_uint(x[2]), __float_as_uint(x[3]));
}

template <typename T, int NCH>
__global__ __launch_bounds__(256) void rms_norm_scaled_fwd_kernel(const T* __restrict__ x, const T* __restrict__ delta, float mult,
                                                                  const T* __restrict__ w, T* __restrict__ h_out, T* __restrict__ y,
                                                                  float* __restrict__ rstd_out, int R, int D, float eps,
                                                                  const unsigned char* __restrict__ live) {
#pragma clang fp contract(off)
  constexpr int N = Vec16<T>::VEC;
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const int64_t base = static_cast<int64_t>(row) * D;
  if (live && !live[row]) {                      // a dead row (wave-uniform): nothing is read, h, y and rstd leave as zeros
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int d = (c * 64 + lane) * N;
      if (d < D) {
        *reinterpret_cast<uint4*>(h_out + base + d) = zero16();
        *reinterpret_cast<uint4*>(y + base + d) = zero16();
      }
    }
    if (lane == 0) rstd_out[row] = 0.f;
    return;
  }
  uint4 rx[NCH], rd[NCH];                        // both streams of the row in flight before the reduction
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = (c * 64 + lane) * N;
    const bool ok = d < D;
    rx[c] = ok ? *reinterpret_cast<const uint4*>(x + base + d) : zero16();
    rd[c] = ok ? *reinterpret_cast<const uint4*>(delta + base + d) : zero16();
  }
  float ss = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = (c * 64 + lane) * N;
    if (d >= D) continue;
    float v[N], dl[N];
    dec16(rx[c], v); dec16(rd[c], dl);
#pragma unroll
    for (int e = 0; e < N; ++e) v[e] += Vec16<T>::rb(dl[e] * mult);
    rx[c] = enc16(v);                            // h, rounded: the chunk is kept encoded for the second pass
    *reinterpret_cast<uint4*>(h_out + base + d) = rx[c];
    dec16(rx[c], v);
#pragma unroll
    for (int e = 0; e < N; ++e) ss = fmaf(v[e], v[e], ss);
  }
  ss = wave_sum(ss);
  const float rstd = rsqrtf(ss / static_cast<float>(D) + eps);
  if (lane == 0) rstd_out[row] = rstd;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = (c * 64 + lane) * N;
    if (d >= D) continue;
    float v[N], wv[N], o[N];
    dec16(rx[c], v);
    Vec16<T>::load(w + d, wv);
#pragma unroll
    for (int e = 0; e < N; ++e) o[e] = wv[e] * Vec16<T>::rb(v[e] * rstd);
    Vec16<T>::store(y + base + d, o);
  }
}

// EARLY (rows of up to 8 chunks per lane): the weight and the residual-path gradient are requested with dy and h, four streams in
// flight; wider rows load them where they are used, as rms_norm_bwd_kernel does, and keep two streams in registers.
template <typename T, int NCH, bool ADD>
__global__ __launch_bounds__(256) void rms_norm_scaled_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ h,
                                                                  const T* __restrict__ w, const float* __restrict__ rstd_in,
                                                                  const T* __restrict__ dres, float mult, T* __restrict__ dx,
                                                                  T* __restrict__ ddelta, int R, int D,
                                                                  const unsigned char* __restrict__ live) {
#pragma clang fp contract(off)
  constexpr int N = Vec16<T>::VEC;
  constexpr bool EARLY = NCH <= 8;
  constexpr int NE = EARLY ? NCH : 1;
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const int64_t base = static_cast<int64_t>(row) * D;
  if (live && !live[row]) {                      // a dead row (wave-uniform): dx and ddelta leave as zeros
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int d = (c * 64 + lane) * N;
      if (d < D) {
        *reinterpret_cast<uint4*>(dx + base + d) = zero16();
        *reinterpret_cast<uint4*>(ddelta + base + d) = zero16();
      }
    }
    return;
  }
  uint4 rg[NCH], rh[NCH], rr[NE], rw[NE];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = (c * 64 + lane) * N;
    const bool ok = d < D;
    rg[c] = ok ? *reinterpret_cast<const uint4*>(dy + base + d) : zero16();
    rh[c] = ok ? *reinterpret_cast<const uint4*>(h + base + d) : zero16();
    if constexpr (EARLY) {
      if constexpr (ADD) rr[c] = ok ? *reinterpret_cast<const uint4*>(dres + base + d) : zero16();
      rw[c] = ok ? *reinterpret_cast<const uint4*>(w + d) : zero16();
    }
  }
  const float rstd = rstd_in[row];
  float dot = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = (c * 64 + lane) * N;
    float g[N], xh[N], wv[N];
    dec16(rg[c], g); dec16(rh[c], xh);           // past the row: zeros, which leave the sum as it is
    if constexpr (EARLY) dec16(rw[c], wv);
    else dec16(d < D ? *reinterpret_cast<const uint4*>(w + d) : zero16(), wv);
#pragma unroll
    for (int e = 0; e < N; ++e) dot = fmaf(g[e] * wv[e], xh[e] * rstd, dot);
  }
  dot = wave_sum(dot) / static_cast<float>(D);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = (c * 64 + lane) * N;
    if (d >= D) continue;
    float g[N], xh[N], wv[N], o[N];
    dec16(rg[c], g); dec16(rh[c], xh);
    if constexpr (EARLY) dec16(rw[c], wv);
    else Vec16<T>::load(w + d, wv);
#pragma unroll
    for (int e = 0; e < N; ++e) o[e] = fmaf(-(xh[e] * rstd), dot, g[e] * wv[e]);
    if constexpr (ADD) {
      float r[N];
      if constexpr (EARLY) dec16(rr[c], r);
      else Vec16<T>::load(dres + base + d, r);
#pragma unroll
      for (int e = 0; e < N; ++e) o[e] = fmaf(rstd, o[e], r[e]);
    } else {
#pragma unroll
      for (int e = 0; e < N; ++e) o[e] *= rstd;
    }
    const uint4 q = enc16(o);                    // dx, rounded
    *reinterpret_cast<uint4*>(dx + base + d) = q;
    dec16(q, o);
#pragma unroll
    for (int e = 0; e < N; ++e) o[e] *= mult;
    Vec16<T>::store(ddelta + base + d, o);
  }
}

constexpr int kScaleAddVecs = 4;                 // 16-byte vectors per lane, all requested before the first is used

template <typename T, bool RES>
__global__ __launch_bounds__(256) void scale_add_kernel(const T* __restrict__ res, const T* __restrict__ x, float mult,
                                                        T* __restrict__ out, unsigned int nvec, unsigned int vecs_per_row,
                                                        const unsigned char* __restrict__ live) {
#pragma clang fp contract(off)
  constexpr int N = Vec16<T>::VEC, K = kScaleAddVecs;
  const unsigned int i0 = blockIdx.x * (256u * K) + threadIdx.x;
  uint4 rx[K], rr[K];
  bool in[K], lv[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const unsigned int i = i0 + k * 256u;
    in[k] = i < nvec;
    lv[k] = in[k] && (!live || live[i / vecs_per_row]);
    const int64_t at = static_cast<int64_t>(i) * N;
    rx[k] = lv[k] ? *reinterpret_cast<const uint4*>(x + at) : zero16();
    if constexpr (RES) rr[k] = lv[k] ? *reinterpret_cast<const uint4*>(res + at) : zero16();
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if (!in[k]) continue;
    const int64_t at = static_cast<int64_t>(i0 + k * 256u) * N;
    float v[N];
    dec16(rx[k], v);
#pragma unroll
    for (int e = 0; e < N; ++e) v[e] *= mult;
    if constexpr (RES) {
      float r[N];
      dec16(rr[k], r);
#pragma unroll
      for (int e = 0; e < N; ++e) v[e] = r[e] + Vec16<T>::rb(v[e]);
    }
    *reinterpret_cast<uint4*>(out + at) = lv[k] ? enc16(v) : zero16();      // a dead row: nothing was loaded, zeros leave
  }
}

}  // namespace

extern "C" int dalm_rms_norm_scaled_fwd(const void* x, const void* delta, float mult, const void* w, int dtype, int64_t R, int64_t D,
                                        float eps, void* h_out, void* y, float* rstd, const uint8_t* row_live, dalm_stream_t stream) {
  DALM_REQUIRE(x && delta && w && h_out && y && rstd, DALM_E_NULL, "null pointer argument");
  DALM_RMS_CHECKS;
  DALM_REQUIRE(aligned16(x, delta, w, h_out, y), DALM_E_ALIGN, "tensors must be 16-byte aligned");
  const int Ri = static_cast<int>(R), Di = static_cast<int>(D);
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    by_ceil<1, 2, 4, 8, 16>(nch, [&](auto n) {
      hipLaunchKernelGGL((rms_norm_scaled_fwd_kernel<T, n>), grid, dim3(256), 0, as_stream(stream), static_cast<const T*>(x),
                         static_cast<const T*>(delta), mult, static_cast<const T*>(w), static_cast<T*>(h_out), static_cast<T*>(y),
                         rstd, Ri, Di, eps, row_live);
    });
  });
  return check_launch(__func__);
}

extern "C" int dalm_rms_norm_scaled_bwd(const void* dy, const void* h, const void* w, const float* rstd, const void* dres, float mult,
                                        int dtype, int64_t R, int64_t D, void* dx, void* ddelta, const uint8_t* row_live,
                                        dalm_stream_t stream) {
  DALM_REQUIRE(dy && h && w && rstd && dx && ddelta, DALM_E_NULL, "null pointer argument");
  DALM_RMS_CHECKS;
  DALM_REQUIRE(aligned16(dy, h, w, dres, dx, ddelta), DALM_E_ALIGN, "tensors must be 16-byte aligned");
  const int Ri = static_cast<int>(R), Di = static_cast<int>(D);
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    by_bool(dres != nullptr, [&](auto add) {
      by_ceil<1, 2, 4, 8, 16>(nch, [&](auto n) {
        hipLaunchKernelGGL((rms_norm_scaled_bwd_kernel<T, n, add>), grid, dim3(256), 0, as_stream(stream), static_cast<const T*>(dy),
                           static_cast<const T*>(h), static_cast<const T*>(w), rstd, static_cast<const T*>(dres), mult,
                           static_cast<T*>(dx), static_cast<T*>(ddelta), Ri, Di, row_live);
      });
    });
  });
  return check_launch(__func__);
}

extern "C" int dalm_scale_add(const void* res, const void* x, float mult, void* out, int dtype, int64_t R, int64_t D,
                              const uint8_t* row_live, dalm_stream_t stream) {
  DALM_REQUIRE(x && out, DALM_E_NULL, "null pointer argument");
  DALM_REQUIRE(dtype == DALM_F32 || dtype == DALM_BF16, DALM_E_DTYPE, "dtype must be DALM_F32 or DALM_BF16");
  const int vecn = dtype == DALM_F32 ? 4 : 8;
  DALM_REQUIRE(R >= 0 && D >= 0 && D % vecn == 0 && (R == 0 || D / vecn <= 0x7fffffffll / R), DALM_E_SHAPE,
               "need rows >= 0, a width that is a multiple of 16 bytes, and R D / (16 bytes) < 2^31");
  DALM_REQUIRE(aligned16(res, x, out), DALM_E_ALIGN, "tensors must be 16-byte aligned");
  if (R == 0 || D == 0) return 0;
  const unsigned int vecs_per_row = static_cast<unsigned int>(D / vecn), nvec = static_cast<unsigned int>(R) * vecs_per_row;
  const dim3 grid((nvec + 256u * kScaleAddVecs - 1) / (256u * kScaleAddVecs));
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    by_bool(res != nullptr, [&](auto with_res) {
      hipLaunchKernelGGL((scale_add_kernel<T, with_res>), grid, dim3(256), 0, as_stream(stream), static_cast<const T*>(res),
                         static_cast<const T*>(x), mult, static_cast<T*>(out), nvec, vecs_per_row, row_live);
    });
  });
  return check_launch(__func__);
}

// ---------------------------------------------------------------------------------------------------
// Cohere (modeling_cohere.py; Command-R, Aya): a parallel block behind ONE norm, n = LayerNorm(x); out = x + attn(n) + mlp(n), with
// an INTERLEAVED rotary embedding computed in f32 and a bias-free LayerNorm computed in f32:
//   rope forward :  o[2i] = rb(f32(x[2i] c[2i]) - f32(x[2i+1] s[2i]))       o[2i+1] = rb(f32(x[2i+1] c[2i+1]) + f32(x[2i] s[2i+1]))
//   rope backward:  d[2i] = rb(f32(g[2i] c[2i]) + f32(g[2i+1] s[2i+1]))     d[2i+1] = rb(f32(g[2i+1] c[2i+1]) - f32(g[2i] s[2i]))
//                   apply_rotary_pos_emb up-casts q and k, multiplies with the tables in f32 (separate mul and add kernels: no
//                   fused multiply-add here) and rounds once, at the end; its autograd backward rounds once as well.  The
//                   tables may be f32 beside bf16 activations (autocast over f32 weights); cos[2i] and cos[2i+1] are read as
//                   given.  A lane holds one 16-byte chunk of a head row: a pair never crosses a lane.
//   norm forward :  mean = mean_d(x);  rstd = rsqrt(mean_d((x - mean)^2) + eps);  y = rb(f32(w) f32((x - mean) rstd))   - f32
//                   throughout, one rounding (CohereLayerNorm.forward); only the summation order of the two means is the kernel's.
//                   f32 rows: statistics and y in f64, rounded once (see cohere_norm_fwd_kernel)
//   norm backward:  g = dy w;  xh = (x - mean) rstd;  dx = rb(rstd (g - mean_d(g) - xh mean_d(g xh)) [+ dres])
//   add3_live    :  out = rb(rb(res + a) + b): the layer's `residual + attn + mlp`, two eager adds
// The norms: one wave per row, the row kept as raw 16-byte chunks between the reductions (rms_norm_scaled_fwd_kernel).  The rotary
// kernel and add3 have no reduction: flat grids.  Algorithmic bytes: rope 2 (|q| + |k|) el (+ tables, shared by all heads); norm
// forward 2 R D el, backward (3 or 4) R D el; add3 4 R D el.
// ---------------------------------------------------------------------------------------------------
namespace {

struct RopeIlParams {
  RopeTensor q, k;
  const void* cos; const void* sin; int64_t cs[2];   // strides of (b, t)
  int B, T, Hq, Hk, backward;
  const unsigned char* live;                         // [B * T] or NULL: a dead (b, t) is not read, its outputs are zeros
};

// N table values from p on: the activations' dtype (one 16-byte load) or f32 beside bf16 activations (two)
template <typename T, bool TAB_F32>
__device__ __forceinline__ void load_table(const void* tab, int64_t at, float (&v)[Vec16<T>::VEC]) {
  if constexpr (TAB_F32) {
    const float* p = static_cast<const float*>(tab) + at;
#pragma unroll
    for (int i = 0; i < Vec16<T>::VEC; i += 4) {
      const float4 f = *reinterpret_cast<const float4*>(p + i);
      v[i] = f.x; v[i + 1] = f.y; v[i + 2] = f.z; v[i + 3] = f.w;
    }
  } else {
    Vec16<T>::load(static_cast<const T*>(tab) + at, v);
  }
}

template <typename T, int HD, bool TAB_F32>
__global__ __launch_bounds__(256) void rope_il_kernel(const RopeIlParams p) {
#pragma clang fp contract(off)   // the eager chain is separate f32 mul and add kernels: a fused multiply-add would round once less
  constexpr int N = Vec16<T>::VEC, G = HD / N;       // lanes per head row
  const unsigned H = static_cast<unsigned>(p.Hq + p.Hk);
  const unsigned gid = blockIdx.x * 256u + threadIdx.x;   // the launcher keeps rows * G below 2^31
  const unsigned row = gid / G;
  const int c = static_cast<int>(gid % G) * N;
  if (row >= static_cast<unsigned>(p.B) * p.T * H) return;
  const unsigned hh = row % H, bt = row / H;              // rows are walked head-fastest (rope_qk_kernel)
  const int t = static_cast<int>(bt % p.T), b = static_cast<int>(bt / p.T);
  const bool is_k = hh >= static_cast<unsigned>(p.Hq);
  const RopeTensor& R = is_k ? p.k : p.q;
  const int head = static_cast<int>(is_k ? hh - p.Hq : hh);
  T* o = static_cast<T*>(R.o) + b * R.os[0] + head * R.os[1] + t * R.os[2] + c;
  if (p.live && !p.live[bt]) {
    *reinterpret_cast<uint4*>(o) = zero16();
    return;
  }
  float x[N], cs[N], sn[N], out[N];
  const int64_t ta = b * p.cs[0] + t * p.cs[1] + c;
  Vec16<T>::load(static_cast<const T*>(R.x) + b * R.xs[0] + head * R.xs[1] + t * R.xs[2] + c, x);
  load_table<T, TAB_F32>(p.cos, ta, cs);
  load_table<T, TAB_F32>(p.sin, ta, sn);
#pragma unroll
  for (int e = 0; e < N; e += 2) {
    // plain operators: the contract(off) pragma above governs this function's operations (see rope_qk_kernel)
    const float a0 = x[e] * cs[e], a1 = x[e + 1] * cs[e + 1];
    if (!p.backward) {
      const float b0 = x[e + 1] * sn[e], b1 = x[e] * sn[e + 1];
      out[e] = a0 - b0;
      out[e + 1] = a1 + b1;
    } else {
      const float b0 = x[e + 1] * sn[e + 1], b1 = x[e] * sn[e];
      out[e] = a0 + b0;
      out[e + 1] = a1 - b1;
    }
  }
  Vec16<T>::store(o, out);                           // rounded once
}

// ---------------------------------------------------------------------------------------------------
// Phi-3 / Phi-4 (modeling_phi3.py apply_rotary_pos_emb): only the first `rot` = cos.shape[-1] elements of a head rotate, half-split
// WITHIN those rot (i pairs with i + rot/2); the other hd - rot pass through.  The pair gets rope_qk_kernel's arithmetic and rounding
// points - with rot == hd this kernel IS that one - and the pass part is copied as 16 raw bytes, forward and backward alike.
// Lanes of a head row: rot/2 / VEC rotate (each loads its chunk and the partner's and writes both), then, out of place only,
// (hd - rot) / VEC copy one chunk each: 6 + 4 of 10 at rot 96 / hd 128 bf16, none idle (a power-of-two 16 would idle 6).  The row
// index comes from ONE 32-bit division by that lane count (the launcher keeps rows * lanes below 2^31).  In place (q_out == q and
// k_out == k) the copying lanes do not exist and a dead row is left as it is.
// ---------------------------------------------------------------------------------------------------
struct RopePartialParams {
  RopeTensor q, k;
  const void* cos; const void* sin; int64_t cs[2];   // strides of (b, t); tables [B or 1, T, rot]
  int B, T, Hq, Hk, hd, rot, backward, in_place;
  const unsigned char* live;                         // [B * T] or NULL
};

template <typename T>
__global__ __launch_bounds__(256) void rope_partial_kernel(const RopePartialParams p) {
#pragma clang fp contract(off)   // the eager chain is separate mul and add kernels (see rope_qk_kernel)
  constexpr int N = Vec16<T>::VEC;
  const int h = p.rot >> 1;
  const unsigned nrot = static_cast<unsigned>(h / N);
  const unsigned lpr = nrot + (p.in_place ? 0u : static_cast<unsigned>((p.hd - p.rot) / N));   // lanes per head row
  const unsigned H = static_cast<unsigned>(p.Hq + p.Hk);
  const unsigned gid = blockIdx.x * 256u + threadIdx.x;
  const unsigned row = gid / lpr, l = gid - row * lpr;
  if (row >= static_cast<unsigned>(p.B) * p.T * H) return;
  const unsigned bt = row / H, hh = row - bt * H;         // rows are walked head-fastest (rope_qk_kernel)
  const unsigned b = bt / static_cast<unsigned>(p.T), t = bt - b * p.T;
  const bool is_k = hh >= static_cast<unsigned>(p.Hq);
  const RopeTensor& R = is_k ? p.k : p.q;
  const int64_t head = is_k ? hh - p.Hq : hh;
  const bool dead = p.live && !p.live[bt];
  if (dead && p.in_place) return;
  const bool rotates = l < nrot;
  const int c = rotates ? static_cast<int>(l) * N : p.rot + static_cast<int>(l - nrot) * N;
  const T* x = static_cast<const T*>(R.x) + b * R.xs[0] + head * R.xs[1] + t * R.xs[2] + c;
  T* o = static_cast<T*>(R.o) + b * R.os[0] + head * R.os[1] + t * R.os[2] + c;
  if (dead) {
    *reinterpret_cast<uint4*>(o) = zero16();
    if (rotates) *reinterpret_cast<uint4*>(o + h) = zero16();
    return;
  }
  if (!rotates) {                                    // the pass part: bit for bit, in both directions
    *reinterpret_cast<uint4*>(o) = *reinterpret_cast<const uint4*>(x);
    return;
  }
  const int64_t ta = b * p.cs[0] + t * p.cs[1] + c;
  const T* cs = static_cast<const T*>(p.cos) + ta;
  const T* sn = static_cast<const T*>(p.sin) + ta;
  float x1[N], x2[N], c1[N], c2[N], s1[N], s2[N], o1[N], o2[N];
  Vec16<T>::load(x, x1); Vec16<T>::load(x + h, x2);
  Vec16<T>::load(cs, c1); Vec16<T>::load(cs + h, c2);
  Vec16<T>::load(sn, s1); Vec16<T>::load(sn + h, s2);
#pragma unroll
  for (int e = 0; e < N; ++e) {
    // plain operators: the contract(off) pragma above governs this function's operations (see rope_qk_kernel)
    const float a1 = Vec16<T>::rb(x1[e] * c1[e]), a2 = Vec16<T>::rb(x2[e] * c2[e]);
    if (!p.backward) {
      const float b1 = Vec16<T>::rb(x2[e] * s1[e]), b2 = Vec16<T>::rb(x1[e] * s2[e]);
      o1[e] = Vec16<T>::rb(a1 - b1);
      o2[e] = Vec16<T>::rb(a2 + b2);
    } else {
      const float b1 = Vec16<T>::rb(x2[e] * s2[e]), b2 = Vec16<T>::rb(x1[e] * s1[e]);
      o1[e] = Vec16<T>::rb(a1 + b1);
      o2[e] = Vec16<T>::rb(a2 - b2);
    }
  }
  Vec16<T>::store(o, o1); Vec16<T>::store(o + h, o2);
}

// every lane's partial sum and the shuffles across the wave, in the accumulator's type
template <typename A>
__device__ __forceinline__ A wave_sum_as(A v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// The statistics and the output are formed in A: float for bf16 rows - the eager chain's own f32 operations, whose roundings vanish
// under the one rounding to bf16 - and double for f32 rows, where the chain's roundings ARE the result: there the kernel rounds
// once, from the exact value (at most half an ulp, whatever the summation order of the eager means)
template <typename T, int NCH>
__global__ __launch_bounds__(256) void cohere_norm_fwd_kernel(const T* __restrict__ x, const void* __restrict__ w, bool w_f32,
                                                              T* __restrict__ y, float* __restrict__ mean_out,
                                                              float* __restrict__ rstd_out, int R, int D, float eps,
                                                              const unsigned char* __restrict__ live) {
#pragma clang fp contract(off)   // (x - mean) rstd and the weight product round separately in the eager chain
  constexpr int N = Vec16<T>::VEC;
  using A = std::conditional_t<std::is_same_v<T, float>, double, float>;
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const int64_t base = static_cast<int64_t>(row) * D;
  if (live && !live[row]) {                      // a dead row (wave-uniform): nothing is read, y, mean and rstd leave as zeros
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int d = (c * 64 + lane) * N;
      if (d < D) *reinterpret_cast<uint4*>(y + base + d) = zero16();
    }
    if (lane == 0) { mean_out[row] = 0.f; rstd_out[row] = 0.f; }
    return;
  }
  uint4 rx[NCH];                                 // the row in flight before the first reduction, kept raw for the other two passes
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = (c * 64 + lane) * N;
    rx[c] = d < D ? *reinterpret_cast<const uint4*>(x + base + d) : zero16();
  }
  A s = 0;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    float v[N];
    dec16(rx[c], v);                             // past the row: zeros, which leave the sum as it is
#pragma unroll
    for (int e = 0; e < N; ++e) s += static_cast<A>(v[e]);
  }
  const A mean = wave_sum_as(s) / static_cast<A>(D);
  A ss = 0;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = (c * 64 + lane) * N;
    if (d >= D) continue;
    float v[N];
    dec16(rx[c], v);
#pragma unroll
    for (int e = 0; e < N; ++e) {
      const A xc = static_cast<A>(v[e]) - mean;
      ss = fma(xc, xc, ss);
    }
  }
  const A var = wave_sum_as(ss) / static_cast<A>(D) + static_cast<A>(eps);
  A rstd;
  if constexpr (std::is_same_v<A, double>) rstd = 1.0 / sqrt(var);
  else rstd = rsqrtf(var);
  if (lane == 0) { mean_out[row] = static_cast<float>(mean); rstd_out[row] = static_cast<float>(rstd); }
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = (c * 64 + lane) * N;
    if (d >= D) continue;
    float v[N], wv[N], o[N];
    dec16(rx[c], v);
    load_weight<N>(w, w_f32, d, wv);
#pragma unroll
    for (int e = 0; e < N; ++e) o[e] = static_cast<float>(static_cast<A>(wv[e]) * ((static_cast<A>(v[e]) - mean) * rstd));
    Vec16<T>::store(y + base + d, o);              // rounded once
  }
}

template <typename T, int NCH, bool ADD>
__global__ __launch_bounds__(256) void cohere_norm_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                              const void* __restrict__ w, bool w_f32,
                                                              const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
                                                              const T* __restrict__ dres, T* __restrict__ dx, int R, int D,
                                                              const unsigned char* __restrict__ live) {
  constexpr int N = Vec16<T>::VEC;
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const int64_t base = static_cast<int64_t>(row) * D;
  if (live && !live[row]) {                      // a dead row (wave-uniform): dx leaves as zeros
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int d = (c * 64 + lane) * N;
      if (d < D) *reinterpret_cast<uint4*>(dx + base + d) = zero16();
    }
    return;
  }
  // the streams of a row are requested as raw 16-byte chunks before the wave reductions and decoded twice (gemma_norm_bwd_kernel)
  uint4 rg[NCH], rh[NCH], rr[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = (c * 64 + lane) * N;
    const bool ok = d < D;
    rg[c] = ok ? *reinterpret_cast<const uint4*>(dy + base + d) : zero16();
    rh[c] = ok ? *reinterpret_cast<const uint4*>(x + base + d) : zero16();
    if constexpr (ADD) rr[c] = ok ? *reinterpret_cast<const uint4*>(dres + base + d) : zero16();
  }
  const float mean = mean_in[row], rstd = rstd_in[row];
  float sg = 0.f, dot = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = (c * 64 + lane) * N;
    if (d >= D) continue;
    float g[N], xv[N], wv[N];
    dec16(rg[c], g); dec16(rh[c], xv);
    load_weight<N>(w, w_f32, d, wv);
#pragma unroll
    for (int e = 0; e < N; ++e) {
      const float gw = g[e] * wv[e];
      sg += gw;
      dot = fmaf(gw, (xv[e] - mean) * rstd, dot);
    }
  }
  sg = wave_sum(sg) / static_cast<float>(D);
  dot = wave_sum(dot) / static_cast<float>(D);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = (c * 64 + lane) * N;
    if (d >= D) continue;
    float g[N], xv[N], wv[N], o[N];
    dec16(rg[c], g); dec16(rh[c], xv);
    load_weight<N>(w, w_f32, d, wv);
#pragma unroll
    for (int e = 0; e < N; ++e) o[e] = rstd * (g[e] * wv[e] - sg - ((xv[e] - mean) * rstd) * dot);
    if constexpr (ADD) {
      float r[N];
      dec16(rr[c], r);
#pragma unroll
      for (int e = 0; e < N; ++e) o[e] += r[e];
    }
    Vec16<T>::store(dx + base + d, o);             // rounded once
  }
}

template <typename T>
__global__ __launch_bounds__(256) void add3_live_kernel(const T* __restrict__ res, const T* __restrict__ a, const T* __restrict__ b,
                                                        T* __restrict__ out, unsigned int nvec, unsigned int vecs_per_row,
                                                        const unsigned char* __restrict__ live) {
  constexpr int N = Vec16<T>::VEC, K = kScaleAddVecs;
  const unsigned int i0 = blockIdx.x * (256u * K) + threadIdx.x;
  uint4 rr[K], ra[K], rb[K];
  bool in[K], lv[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const unsigned int i = i0 + k * 256u;
    in[k] = i < nvec;
    lv[k] = in[k] && (!live || live[i / vecs_per_row]);
    const int64_t at = static_cast<int64_t>(i) * N;
    rr[k] = lv[k] ? *reinterpret_cast<const uint4*>(res + at) : zero16();
    ra[k] = lv[k] ? *reinterpret_cast<const uint4*>(a + at) : zero16();
    rb[k] = lv[k] ? *reinterpret_cast<const uint4*>(b + at) : zero16();
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if (!in[k]) continue;
    const int64_t at = static_cast<int64_t>(i0 + k * 256u) * N;
    float r[N], x[N], y[N];
    dec16(rr[k], r); dec16(ra[k], x); dec16(rb[k], y);
#pragma unroll
    for (int e = 0; e < N; ++e) r[e] = Vec16<T>::rb(r[e] + x[e]) + y[e];
    *reinterpret_cast<uint4*>(out + at) = lv[k] ? enc16(r) : zero16();      // a dead row: nothing was loaded, zeros leave
  }
}

bool strides_mult(const int64_t* s, int n, int q) {
  for (int i = 0; i < n; ++i)
    if (s[i] % q != 0) return false;
  return true;
}

}  // namespace

extern "C" int dalm_rope_il_qk(const void* q, const void* k, void* q_out, void* k_out, const void* cos, const void* sin, int dtype,
                               int tab_dtype, int64_t B, int64_t T, int64_t Hq, int64_t Hk, int64_t hd, const int64_t* q_strides,
                               const int64_t* k_strides, const int64_t* qo_strides, const int64_t* ko_strides,
                               const int64_t* cs_strides, int backward, const uint8_t* row_live, dalm_stream_t stream) {
  DALM_REQUIRE(q && k && q_out && k_out && cos && sin && q_strides && k_strides && qo_strides && ko_strides && cs_strides,
               DALM_E_NULL, "null pointer argument");
  DALM_REQUIRE(dtype == DALM_F32 || dtype == DALM_BF16, DALM_E_DTYPE, "dtype must be DALM_F32 or DALM_BF16");
  DALM_REQUIRE(tab_dtype == dtype || tab_dtype == DALM_F32, DALM_E_DTYPE, "the tables are of the activations' dtype or f32");
  DALM_REQUIRE(hd == 32 || hd == 64 || hd == 128, DALM_E_SHAPE, "head width must be 32, 64 or 128");
  DALM_REQUIRE(B > 0 && T > 0 && Hq > 0 && Hk >= 0 && Hq + Hk <= 65535, DALM_E_SHAPE, "need B, T, Hq > 0, Hk >= 0");
  const int vec = dtype == DALM_F32 ? 4 : 8;
  DALM_REQUIRE(B <= 0x7fffffffLL && T <= 0x7fffffffLL && B * T <= 0x7fffffffLL && B * T * (Hq + Hk) * (hd / vec) <= 0x7fffffffLL,
               DALM_E_SHAPE, "tensor too large for one launch");
  DALM_REQUIRE(aligned16(q, k, q_out, k_out, cos, sin) && strides_mult(q_strides, 3, vec) && strides_mult(k_strides, 3, vec)
                   && strides_mult(qo_strides, 3, vec) && strides_mult(ko_strides, 3, vec) && strides_mult(cs_strides, 2, vec),
               DALM_E_ALIGN, "tensors must be 16-byte aligned and every stride a multiple of 16 bytes of `dtype`");
  RopeIlParams p;
  p.q.x = q; p.q.o = q_out; p.k.x = k; p.k.o = k_out;
  for (int i = 0; i < 3; ++i) {
    p.q.xs[i] = q_strides[i]; p.k.xs[i] = k_strides[i]; p.q.os[i] = qo_strides[i]; p.k.os[i] = ko_strides[i];
  }
  p.cos = cos; p.sin = sin; p.cs[0] = cs_strides[0]; p.cs[1] = cs_strides[1];
  p.B = static_cast<int>(B); p.T = static_cast<int>(T); p.Hq = static_cast<int>(Hq); p.Hk = static_cast<int>(Hk);
  p.backward = backward != 0;
  p.live = row_live;
  const dim3 grid(static_cast<unsigned>((B * T * (Hq + Hk) * (hd / vec) + 255) / 256));
  by_dtype(dtype, [&](auto t) {
    using T_ = typename decltype(t)::type;
    by_exact<32, 64, 128>(static_cast<int>(hd), [&](auto width) {
      if constexpr (std::is_same_v<T_, float>) {       // f32 activations: the tables are f32, read as the activations are
        hipLaunchKernelGGL((rope_il_kernel<T_, width, false>), grid, dim3(256), 0, as_stream(stream), p);
      } else {
        by_bool(tab_dtype == DALM_F32, [&](auto tab_f32) {
          hipLaunchKernelGGL((rope_il_kernel<T_, width, tab_f32>), grid, dim3(256), 0, as_stream(stream), p);
        });
      }
    });
  });
  return check_launch(__func__);
}

extern "C" int dalm_rope_partial_qk(const void* q, const void* k, void* q_out, void* k_out, const void* cos, const void* sin, int dtype,
                                    int64_t B, int64_t T, int64_t Hq, int64_t Hk, int64_t hd, int64_t rot, const int64_t* q_strides,
                                    const int64_t* k_strides, const int64_t* qo_strides, const int64_t* ko_strides,
                                    const int64_t* cs_strides, int backward, const uint8_t* row_live, dalm_stream_t stream) {
  DALM_REQUIRE(q && k && q_out && k_out && cos && sin && q_strides && k_strides && qo_strides && ko_strides && cs_strides,
               DALM_E_NULL, "null pointer argument");
  DALM_REQUIRE(dtype == DALM_F32 || dtype == DALM_BF16, DALM_E_DTYPE, "dtype must be DALM_F32 or DALM_BF16");
  DALM_REQUIRE(hd == 32 || hd == 64 || hd == 128, DALM_E_SHAPE, "head width must be 32, 64 or 128");
  const int vec = dtype == DALM_F32 ? 4 : 8;
  DALM_REQUIRE(rot > 0 && rot <= hd && rot % (2 * vec) == 0, DALM_E_SHAPE,
               "rotary width must be positive, at most the head width, and half of it a multiple of 16 bytes of `dtype`: "
               "a multiple of 16 for bf16 (16, 32, 48, 64, 80, 96, 112, 128), of 8 for f32");
  DALM_REQUIRE(B >= 0 && T >= 0 && Hq > 0 && Hk >= 0 && Hq + Hk <= 65535, DALM_E_SHAPE, "need B, T, Hk >= 0 and Hq > 0");
  DALM_REQUIRE(B <= 0x7fffffffLL && T <= 0x7fffffffLL && B * T <= 0x7fffffffLL && B * T * (Hq + Hk) * (hd / vec) <= 0x7fffffffLL,
               DALM_E_SHAPE, "tensor too large for one launch: need B T (Hq + Hk) hd / (16 bytes) < 2^31");
  DALM_REQUIRE(aligned16(q, k, q_out, k_out, cos, sin) && strides_mult(q_strides, 3, vec) && strides_mult(k_strides, 3, vec)
                   && strides_mult(qo_strides, 3, vec) && strides_mult(ko_strides, 3, vec) && strides_mult(cs_strides, 2, vec),
               DALM_E_ALIGN, "tensors must be 16-byte aligned and every stride a multiple of 16 bytes of `dtype`");
  const bool in_place = q_out == q && k_out == k;
  if (in_place)
    for (int i = 0; i < 3; ++i)
      DALM_REQUIRE(qo_strides[i] == q_strides[i] && ko_strides[i] == k_strides[i], DALM_E_SHAPE,
                   "in place (q_out == q, k_out == k) the output strides are the input strides");
  if (B == 0 || T == 0) return 0;
  RopePartialParams p;
  p.q.x = q; p.q.o = q_out; p.k.x = k; p.k.o = k_out;
  for (int i = 0; i < 3; ++i) {
    p.q.xs[i] = q_strides[i]; p.k.xs[i] = k_strides[i]; p.q.os[i] = qo_strides[i]; p.k.os[i] = ko_strides[i];
  }
  p.cos = cos; p.sin = sin; p.cs[0] = cs_strides[0]; p.cs[1] = cs_strides[1];
  p.B = static_cast<int>(B); p.T = static_cast<int>(T); p.Hq = static_cast<int>(Hq); p.Hk = static_cast<int>(Hk);
  p.hd = static_cast<int>(hd); p.rot = static_cast<int>(rot);
  p.backward = backward != 0; p.in_place = in_place;
  p.live = row_live;
  const int64_t lanes_per_row = (rot / 2 + (in_place ? 0 : hd - rot)) / vec;     // at most hd / vec: below 2^31 in all
  const dim3 grid(static_cast<unsigned>((B * T * (Hq + Hk) * lanes_per_row + 255) / 256));
  by_dtype(dtype, [&](auto t) {
    using T_ = typename decltype(t)::type;
    hipLaunchKernelGGL((rope_partial_kernel<T_>), grid, dim3(256), 0, as_stream(stream), p);
  });
  return check_launch(__func__);
}

// dalm_rms_norm_*'s width rules and R > 0; the weight has a dtype of its own
#define DALM_COHERE_NORM_CHECKS                                                                                         \
  DALM_REQUIRE(dtype == DALM_F32 || dtype == DALM_BF16, DALM_E_DTYPE, "dtype must be DALM_F32 or DALM_BF16");             \
  DALM_REQUIRE(w_dtype == DALM_F32 || w_dtype == DALM_BF16, DALM_E_DTYPE, "w_dtype must be DALM_F32 or DALM_BF16");       \
  const int vecn = dtype == DALM_F32 ? 4 : 8;                                                                            \
  DALM_REQUIRE(R > 0 && D > 0 && D % vecn == 0 && D <= 64ll * vecn * 16 && R <= 0x7ffffff0ll, DALM_E_SHAPE,               \
               "need rows > 0 and a width that is a multiple of 16 bytes, at most 8192 (bf16) / 4096 (f32) elements");    \
  const int nch = static_cast<int>((D + 64 * vecn - 1) / (64 * vecn));                                                   \
  const dim3 grid(static_cast<unsigned>((R + 3) / 4))

extern "C" int dalm_cohere_norm_fwd(const void* x, const void* w, int dtype, int w_dtype, int64_t R, int64_t D, float eps, void* y,
                                    float* mean, float* rstd, const uint8_t* row_live, dalm_stream_t stream) {
  DALM_REQUIRE(x && w && y && mean && rstd, DALM_E_NULL, "null pointer argument");
  DALM_COHERE_NORM_CHECKS;
  DALM_REQUIRE(aligned16(x, w, y), DALM_E_ALIGN, "tensors must be 16-byte aligned");
  const int Ri = static_cast<int>(R), Di = static_cast<int>(D);
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    by_ceil<1, 2, 4, 8, 16>(nch, [&](auto n) {
      hipLaunchKernelGGL((cohere_norm_fwd_kernel<T, n>), grid, dim3(256), 0, as_stream(stream), static_cast<const T*>(x), w,
                         w_dtype == DALM_F32, static_cast<T*>(y), mean, rstd, Ri, Di, eps, row_live);
    });
  });
  return check_launch(__func__);
}

extern "C" int dalm_cohere_norm_bwd(const void* dy, const void* x, const void* w, const float* mean, const float* rstd,
                                    const void* dres, int dtype, int w_dtype, int64_t R, int64_t D, void* dx,
                                    const uint8_t* row_live, dalm_stream_t stream) {
  DALM_REQUIRE(dy && x && w && mean && rstd && dx, DALM_E_NULL, "null pointer argument");
  DALM_COHERE_NORM_CHECKS;
  DALM_REQUIRE(aligned16(dy, x, w, dres, dx), DALM_E_ALIGN, "tensors must be 16-byte aligned");
  const int Ri = static_cast<int>(R), Di = static_cast<int>(D);
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    by_bool(dres != nullptr, [&](auto add) {
      by_ceil<1, 2, 4, 8, 16>(nch, [&](auto n) {
        hipLaunchKernelGGL((cohere_norm_bwd_kernel<T, n, add>), grid, dim3(256), 0, as_stream(stream), static_cast<const T*>(dy),
                           static_cast<const T*>(x), w, w_dtype == DALM_F32, mean, rstd, static_cast<const T*>(dres),
                           static_cast<T*>(dx), Ri, Di, row_live);
      });
    });
  });
  return check_launch(__func__);
}

extern "C" int dalm_add3_live(const void* res, const void* a, const void* b, void* out, int dtype, int64_t R, int64_t D,
                              const uint8_t* row_live, dalm_stream_t stream) {
  DALM_REQUIRE(res && a && b && out, DALM_E_NULL, "null pointer argument");
  DALM_REQUIRE(dtype == DALM_F32 || dtype == DALM_BF16, DALM_E_DTYPE, "dtype must be DALM_F32 or DALM_BF16");
  const int vecn = dtype == DALM_F32 ? 4 : 8;
  DALM_REQUIRE(R >= 0 && D >= 0 && D % vecn == 0 && (R == 0 || D / vecn <= 0x7fffffffll / R), DALM_E_SHAPE,
               "need rows >= 0, a width that is a multiple of 16 bytes, and R D / (16 bytes) < 2^31");
  DALM_REQUIRE(aligned16(res, a, b, out), DALM_E_ALIGN, "tensors must be 16-byte aligned");
  if (R == 0 || D == 0) return 0;
  const unsigned int vecs_per_row = static_cast<unsigned int>(D / vecn), nvec = static_cast<unsigned int>(R) * vecs_per_row;
  const dim3 grid((nvec + 256u * kScaleAddVecs - 1) / (256u * kScaleAddVecs));
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((add3_live_kernel<T>), grid, dim3(256), 0, as_stream(stream), static_cast<const T*>(res),
                       static_cast<const T*>(a), static_cast<const T*>(b), static_cast<T*>(out), nvec, vecs_per_row, row_live);
  });
  return check_launch(__func__);
}
