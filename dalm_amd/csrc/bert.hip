// BERT encoder layer: `dropout + residual add + LayerNorm` as ONE HIP launch per direction (gfx950).
// transformers' BertSelfOutput / BertOutput (modeling_bert.py) evaluate, after their dense projection,
//     hidden = dropout(hidden);  hidden = LayerNorm(hidden + input_tensor)
// as eager ops; the reference reaches them through self.retriever_model(...) (dalm/models/rag_e2e_base_model.py:84-93,
// retriever_only_base_model.py:43-64).  Under bf16 autocast - the configuration bench.py measures - that chain is: a bf16 dropout
// (+ its mask), a bf16 + f32 -> f32 add, an f32 LayerNorm (autocast runs layer_norm in f32) and, in front of every consumer GEMM,
// a cast of the f32 result back to bf16: 4-5 launches forward, 6-7 backward, ~25 bytes per element each way; 33 % of the kernel time
// of the retriever-only step (profiles/r05cfg2_step_by_stream.txt).  Here, rounding where that chain rounds:
//   forward   d = bf16(a keep / (1 - p));  s = f32(d) + res;  y32 = (s - mean) rstd w + b  (f32);  y16 = bf16(y32)
//             a [R, D] bf16 (the dense output), res [R, D] f32 (the previous LayerNorm's f32 output), w / b f32 or bf16;
//             writes y32 (the module's output, and the next residual), y16 (what the consumers' casts would produce),
//             mean / rstd [R], and the keep mask as BITS [R][D / 8] (bit e of byte c = element 8 c + e survives)
//   backward  dy = g32 + f32(g16);  ds = LayerNorm backward of dy (f32);  d_res = ds;  d_a = bf16(bf16(ds) keep / (1 - p))
//             s is recomputed from a, res and the bits (nothing [R, D]-sized is saved beyond the inputs)
// The keep mask is this library's generator (lora_common.hpp: one two-multiply hash per chunk of 8 elements, four words chained by
// xorshift32, 16-bit fields against round(p 65536); oracle/lora_mask.py::keep_mask_v2 restates it) - torch's philox stream
// differs between devices and kernels, there is no reference stream to match.  One wave per row, the row stays in registers.
// Algorithmic bytes per element: forward 2 + 4 read, 4 + 2 + 1/8 written; backward 4 + 2 + 2 + 4 + 1/8 read, 4 + 2 written.
#include "lora_common.hpp"

namespace dalm {
namespace {

using lora::DropArgs;
using lora::DropKey;
using F8 = lora::Chunk8<float>;   // 8 f32 as two 16-byte accesses

// weight / bias vector element chunk, f32 or bf16 storage
template <bool WBF16>
__device__ __forceinline__ void ldw(const void* w, int d, float (&x)[8]) {
  if constexpr (WBF16) dec8(*reinterpret_cast<const uint4*>(static_cast<const unsigned short*>(w) + d), x);
  else F8::load(static_cast<const float*>(w) + d, x);
}

// keep bits of the chunk of 8 elements with flat chunk index c (mask v2 of lora2.hip): bit e = element 8 c + e survives
__device__ __forceinline__ unsigned int keep_bits8(unsigned int c, const DropKey& k, unsigned int thr) {
  unsigned int x = c ^ k.a;
  x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x += k.b; x *= 0x846ca68bU; x ^= x >> 16;
  unsigned int bits = 0u;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (q) { x ^= x << 13; x ^= x >> 17; x ^= x << 5; }
    bits |= ((x & 0xffffu) >= thr ? 1u : 0u) << (2 * q);
    bits |= ((x >> 16) >= thr ? 1u : 0u) << (2 * q + 1);
  }
  return bits;
}

struct AddNormArgs {
  const unsigned short* a;      // [R, D] bf16
  const float* res;             // [R, D] f32
  const void *w, *b;            // [D]
  float* y32;
  unsigned short* y16;
  unsigned char* bits;          // [R][D / 8] or NULL (no dropout)
  float *mean, *rstd;
  const float* g32;             // backward: gradient of y32 (may be NULL)
  const unsigned short* g16;    // backward: gradient of y16 (may be NULL)
  float* d_res;
  unsigned short* d_a;
  int R, D;
  float eps, keep_scale;        // 1 / (1 - p)
  DropArgs drop;                // forward only (thr16 == 0: no dropout)
  const unsigned char* live;    // [R] or NULL: a dead row is not read, everything written for it is zero (its keep bits are not written)
};

// s = f32(bf16(a keep / (1 - p))) + res for one chunk
__device__ __forceinline__ void sum_chunk(const uint4& ra, const float (&r)[8], unsigned int bits, float ks, bool drop, float (&s)[8]) {
  float av[8];
  dec8(ra, av);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float d = drop ? (((bits >> e) & 1u) ? Vec16<bf16_t>::rb(av[e] * ks) : 0.f) : av[e];
    s[e] = d + r[e];
  }
}

template <int NCH, bool WBF16>
__global__ __launch_bounds__(256) void bert_add_norm_fwd_kernel(const AddNormArgs p) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.R) return;
  const int64_t base = static_cast<int64_t>(row) * p.D;
  if (p.live && !p.live[row]) {                                    // wave-uniform
    float z[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) z[e] = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int d = (c * 64 + lane) * 8;
      if (d >= p.D) continue;
      F8::store(p.y32 + base + d, z);
      *reinterpret_cast<uint4*>(p.y16 + base + d) = make_uint4(0u, 0u, 0u, 0u);
    }
    if (lane == 0) { p.mean[row] = 0.f; p.rstd[row] = 0.f; }
    return;
  }
  const bool drop = p.drop.thr16 != 0u;
  DropKey key = {0u, 1u};
  if (drop) key = lora::drop_key(p.drop);
  float s[NCH][8];
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = (c * 64 + lane) * 8;
    if (d >= p.D) {
#pragma unroll
      for (int e = 0; e < 8; ++e) s[c][e] = 0.f;
      continue;
    }
    const uint4 ra = *reinterpret_cast<const uint4*>(p.a + base + d);
    float r[8];
    F8::load(p.res + base + d, r);
    unsigned int bits = 0xffu;
    if (drop) {
      bits = keep_bits8(static_cast<unsigned int>((base + d) >> 3), key, p.drop.thr16);
      p.bits[(base + d) >> 3] = static_cast<unsigned char>(bits);
    }
    sum_chunk(ra, r, bits, p.keep_scale, drop, s[c]);
#pragma unroll
    for (int e = 0; e < 8; ++e) sum += s[c][e];
  }
  const float mean = wave_sum(sum) / static_cast<float>(p.D);
  float ss = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = (c * 64 + lane) * 8;
    if (d >= p.D) continue;
#pragma unroll
    for (int e = 0; e < 8; ++e) ss = fmaf(s[c][e] - mean, s[c][e] - mean, ss);
  }
  const float rstd = rsqrtf(wave_sum(ss) / static_cast<float>(p.D) + p.eps);
  if (lane == 0) { p.mean[row] = mean; p.rstd[row] = rstd; }
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = (c * 64 + lane) * 8;
    if (d >= p.D) continue;
    float wv[8], bv[8], o[8];
    ldw<WBF16>(p.w, d, wv);
    ldw<WBF16>(p.b, d, bv);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = fmaf((s[c][e] - mean) * rstd, wv[e], bv[e]);
    F8::store(p.y32 + base + d, o);
    *reinterpret_cast<uint4*>(p.y16 + base + d) = enc8(o);
  }
}

template <int NCH, bool WBF16>
__global__ __launch_bounds__(256) void bert_add_norm_bwd_kernel(const AddNormArgs p) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.R) return;
  const int64_t base = static_cast<int64_t>(row) * p.D;
  if (p.live && !p.live[row]) {                                    // wave-uniform
    float z[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) z[e] = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int d = (c * 64 + lane) * 8;
      if (d >= p.D) continue;
      F8::store(p.d_res + base + d, z);
      *reinterpret_cast<uint4*>(p.d_a + base + d) = make_uint4(0u, 0u, 0u, 0u);
    }
    return;
  }
  const bool drop = p.bits != nullptr;
  const float mean = p.mean[row], rstd = p.rstd[row];
  float xh[NCH][8], g[NCH][8];
  unsigned int kb[NCH];
  float sg = 0.f, sgx = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = (c * 64 + lane) * 8;
    kb[c] = 0xffu;
    if (d >= p.D) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { xh[c][e] = 0.f; g[c][e] = 0.f; }
      continue;
    }
    const uint4 ra = *reinterpret_cast<const uint4*>(p.a + base + d);
    float r[8], s[8], wv[8], dy[8];
    F8::load(p.res + base + d, r);
    if (drop) kb[c] = p.bits[(base + d) >> 3];
    sum_chunk(ra, r, kb[c], p.keep_scale, drop, s);
    ldw<WBF16>(p.w, d, wv);
    if (p.g32) F8::load(p.g32 + base + d, dy);
    else {
#pragma unroll
      for (int e = 0; e < 8; ++e) dy[e] = 0.f;
    }
    if (p.g16) {
      float h[8];
      dec8(*reinterpret_cast<const uint4*>(p.g16 + base + d), h);
#pragma unroll
      for (int e = 0; e < 8; ++e) dy[e] += h[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      xh[c][e] = (s[e] - mean) * rstd;
      g[c][e] = dy[e] * wv[e];
      sg += g[c][e];
      sgx = fmaf(g[c][e], xh[c][e], sgx);
    }
  }
  sg = wave_sum(sg) / static_cast<float>(p.D);
  sgx = wave_sum(sgx) / static_cast<float>(p.D);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = (c * 64 + lane) * 8;
    if (d >= p.D) continue;
    float ds[8], da[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      ds[e] = rstd * (g[c][e] - sg - xh[c][e] * sgx);
      const float h = Vec16<bf16_t>::rb(ds[e]);                   // the gradient of the bf16 operand of the add, cast to bf16
      da[e] = drop ? (((kb[c] >> e) & 1u) ? h * p.keep_scale : 0.f) : h;
    }
    F8::store(p.d_res + base + d, ds);
    *reinterpret_cast<uint4*>(p.d_a + base + d) = enc8(da);
  }
}

// ---- RoBERTa-family embeddings front end: ids -> the first layer's input in one launch (forward only) ----
// transformers' {Roberta,XLMRoberta,Camembert}Embeddings.forward evaluates, as ~20 eager launches,
//     position_ids = create_position_ids_from_input_ids(input_ids, padding_idx)     (ne, int, cumsum, type_as, add, mul, long, add)
//     embeddings = (word_embeddings(input_ids) + token_type_embeddings(token_type_ids)) + position_embeddings(position_ids)
//     embeddings = dropout(LayerNorm(embeddings))                                   (f32 under bf16 autocast)
// Here one wave per row (b, t): the position is padding_idx + |{j <= t : ids[b, j] != padding_idx}| for a non-pad id and padding_idx
// for a pad id (ballot + popcount over ids[b, 0..t]), or read from `pos` where the caller has it (the packed route); the three
// table rows are summed in eager's order in f32, normalised in f32, y32 = keep ? y / (1 - p) : 0, y16 = bf16(y32).
// Every table index is CLAMPED into its table: eager device-asserts on an out-of-range id, this kernel reads row 0 / the last row
// instead of memory outside the allocation.  Used only where the tables and the LayerNorm are frozen: nothing is saved.
struct EmbedNormArgs {
  const long long *ids, *tt, *pos;   // [B, T]; tt NULL: type 0; pos NULL: derived from ids
  const float *word, *type, *ptab;   // [V, D], [NT, D], [NP, D]
  const void *w, *b;                 // [D]
  float* y32;
  unsigned short* y16;
  const unsigned char* live;         // [B T] or NULL
  long long V, NT, NP, pad;
  int R, T, D;
  float eps, keep_scale;
  DropArgs drop;                     // thr16 == 0: no dropout
};

__device__ __forceinline__ long long clamp_index(long long i, long long n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

template <int NCH, bool WBF16>
__global__ __launch_bounds__(256) void embed_norm_fwd_kernel(const EmbedNormArgs p) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.R) return;
  const int64_t base = static_cast<int64_t>(row) * p.D;
  if (p.live && !p.live[row]) {                                    // wave-uniform
    float z[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) z[e] = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int d = (c * 64 + lane) * 8;
      if (d >= p.D) continue;
      F8::store(p.y32 + base + d, z);
      *reinterpret_cast<uint4*>(p.y16 + base + d) = make_uint4(0u, 0u, 0u, 0u);
    }
    return;
  }
  const int bi = row / p.T, t = row - bi * p.T;
  const long long* idrow = p.ids + static_cast<int64_t>(bi) * p.T;
  const long long id = idrow[t];
  long long pos;
  if (p.pos) pos = p.pos[row];
  else {
    int cnt = 0;
    for (int j0 = 0; j0 <= t; j0 += 64) {                          // wave-uniform trip count: every lane reaches the ballot
      const int j = j0 + lane;
      const bool tok = j <= t && idrow[j] != p.pad;
      cnt += __popcll(__ballot(tok));
    }
    pos = id != p.pad ? p.pad + cnt : p.pad;
  }
  const float* wr = p.word + clamp_index(id, p.V) * p.D;
  const float* tr = p.type + clamp_index(p.tt ? p.tt[row] : 0, p.NT) * p.D;
  const float* pr = p.ptab + clamp_index(pos, p.NP) * p.D;
  const bool drop = p.drop.thr16 != 0u;
  DropKey key = {0u, 1u};
  if (drop) key = lora::drop_key(p.drop);
  float s[NCH][8];
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = (c * 64 + lane) * 8;
    if (d >= p.D) {
#pragma unroll
      for (int e = 0; e < 8; ++e) s[c][e] = 0.f;
      continue;
    }
    float a[8], ty[8], po[8];
    F8::load(wr + d, a);
    F8::load(tr + d, ty);
    F8::load(pr + d, po);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      s[c][e] = (a[e] + ty[e]) + po[e];
      sum += s[c][e];
    }
  }
  const float mean = wave_sum(sum) / static_cast<float>(p.D);
  float ss = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = (c * 64 + lane) * 8;
    if (d >= p.D) continue;
#pragma unroll
    for (int e = 0; e < 8; ++e) ss = fmaf(s[c][e] - mean, s[c][e] - mean, ss);
  }
  const float rstd = rsqrtf(wave_sum(ss) / static_cast<float>(p.D) + p.eps);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int d = (c * 64 + lane) * 8;
    if (d >= p.D) continue;
    float wv[8], bv[8], o[8];
    ldw<WBF16>(p.w, d, wv);
    ldw<WBF16>(p.b, d, bv);
    unsigned int bits = 0xffu;
    if (drop) bits = keep_bits8(static_cast<unsigned int>((base + d) >> 3), key, p.drop.thr16);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      o[e] = fmaf((s[c][e] - mean) * rstd, wv[e], bv[e]);
      if (drop) o[e] = ((bits >> e) & 1u) ? o[e] * p.keep_scale : 0.f;
    }
    F8::store(p.y32 + base + d, o);
    *reinterpret_cast<uint4*>(p.y16 + base + d) = enc8(o);
  }
}

}  // namespace
}  // namespace dalm

using namespace dalm;

extern "C" int dalm_bert_add_norm_fwd_live(const void* a, const float* res, const void* w, const void* b, int w_bf16, int64_t R,
                                           int64_t D, float eps, float dropout_p, const void* seed, uint32_t salt, float* y32,
                                           void* y16, uint8_t* keep_bits, float* mean, float* rstd, const uint8_t* row_live,
                                           dalm_stream_t stream) {
  DALM_REQUIRE(R >= 0, DALM_E_SHAPE, "R must be >= 0");
  if (R == 0) return 0;
  DALM_REQUIRE(a && res && w && b && y32 && y16 && mean && rstd, DALM_E_NULL, "null pointer argument");
  DALM_REQUIRE(D > 0 && D % 8 == 0 && D <= 2048 && R <= (1ll << 30), DALM_E_SHAPE, "D must be a multiple of 8, at most 2048");
  DALM_REQUIRE(aligned16(a, res, w, b, y32, y16), DALM_E_ALIGN, "tensors must be 16-byte aligned");
  DALM_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f && (dropout_p == 0.f || (seed && keep_bits)), DALM_E_SHAPE,
               "dropout needs 0 <= p < 1, a device seed word and the keep-bit buffer");
  DALM_REQUIRE(R * D < (1ll << 35), DALM_E_SHAPE, "tensor too large (the mask's chunk index is 32 bits)");
  AddNormArgs p = {};
  p.a = static_cast<const unsigned short*>(a); p.res = res; p.w = w; p.b = b;
  p.y32 = y32; p.y16 = static_cast<unsigned short*>(y16); p.bits = dropout_p > 0.f ? keep_bits : nullptr;
  p.mean = mean; p.rstd = rstd;
  p.R = static_cast<int>(R); p.D = static_cast<int>(D); p.eps = eps;
  p.keep_scale = dropout_p > 0.f ? 1.0f / (1.0f - dropout_p) : 1.0f;
  p.drop = lora::drop_args(dropout_p, seed, salt);
  if (dropout_p == 0.f) p.drop.thr16 = 0u;
  p.live = row_live;
  const dim3 grid(static_cast<unsigned>((R + 3) / 4));
  by_ceil<1, 2, 4>(static_cast<int>((D + 511) / 512), [&](auto nch) {   // chunks of 64 lanes x 8 elements per row
    by_bool(w_bf16 != 0, [&](auto wb) {
      hipLaunchKernelGGL((bert_add_norm_fwd_kernel<nch, wb>), grid, dim3(256), 0, as_stream(stream), p);
    });
  });
  return check_launch(__func__);
}

extern "C" int dalm_bert_add_norm_fwd(const void* a, const float* res, const void* w, const void* b, int w_bf16, int64_t R, int64_t D,
                                      float eps, float dropout_p, const void* seed, uint32_t salt, float* y32, void* y16,
                                      uint8_t* keep_bits, float* mean, float* rstd, dalm_stream_t stream) {
  return dalm_bert_add_norm_fwd_live(a, res, w, b, w_bf16, R, D, eps, dropout_p, seed, salt, y32, y16, keep_bits, mean, rstd, nullptr,
                                     stream);
}

extern "C" int dalm_bert_add_norm_bwd_live(const float* g32, const void* g16, const void* a, const float* res, const void* w,
                                           int w_bf16, const uint8_t* keep_bits, const float* mean, const float* rstd, int64_t R,
                                           int64_t D, float dropout_p, float* d_res, void* d_a, const uint8_t* row_live,
                                           dalm_stream_t stream) {
  DALM_REQUIRE(R >= 0, DALM_E_SHAPE, "R must be >= 0");
  if (R == 0) return 0;
  DALM_REQUIRE((g32 || g16) && a && res && w && mean && rstd && d_res && d_a, DALM_E_NULL, "null pointer argument");
  DALM_REQUIRE(D > 0 && D % 8 == 0 && D <= 2048 && R <= (1ll << 30), DALM_E_SHAPE, "D must be a multiple of 8, at most 2048");
  DALM_REQUIRE(aligned16(g32, g16, a, res, w, d_res, d_a), DALM_E_ALIGN,
               "tensors must be 16-byte aligned");
  DALM_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f && (dropout_p == 0.f || keep_bits), DALM_E_SHAPE,
               "dropout needs 0 <= p < 1 and the forward's keep bits");
  AddNormArgs p = {};
  p.a = static_cast<const unsigned short*>(a); p.res = res; p.w = w;
  p.bits = dropout_p > 0.f ? const_cast<unsigned char*>(keep_bits) : nullptr;
  p.mean = const_cast<float*>(mean); p.rstd = const_cast<float*>(rstd);
  p.g32 = g32; p.g16 = static_cast<const unsigned short*>(g16);
  p.d_res = d_res; p.d_a = static_cast<unsigned short*>(d_a);
  p.R = static_cast<int>(R); p.D = static_cast<int>(D);
  p.keep_scale = dropout_p > 0.f ? 1.0f / (1.0f - dropout_p) : 1.0f;
  p.live = row_live;
  const dim3 grid(static_cast<unsigned>((R + 3) / 4));
  by_ceil<1, 2, 4>(static_cast<int>((D + 511) / 512), [&](auto nch) {   // chunks of 64 lanes x 8 elements per row
    by_bool(w_bf16 != 0, [&](auto wb) {
      hipLaunchKernelGGL((bert_add_norm_bwd_kernel<nch, wb>), grid, dim3(256), 0, as_stream(stream), p);
    });
  });
  return check_launch(__func__);
}

extern "C" int dalm_bert_add_norm_bwd(const float* g32, const void* g16, const void* a, const float* res, const void* w, int w_bf16,
                                      const uint8_t* keep_bits, const float* mean, const float* rstd, int64_t R, int64_t D,
                                      float dropout_p, float* d_res, void* d_a, dalm_stream_t stream) {
  return dalm_bert_add_norm_bwd_live(g32, g16, a, res, w, w_bf16, keep_bits, mean, rstd, R, D, dropout_p, d_res, d_a, nullptr, stream);
}

extern "C" int dalm_embed_norm_fwd(const int64_t* ids, const int64_t* token_type_ids, const int64_t* position_ids, const float* word,
                                   const float* type, const float* pos, int64_t vocab, int64_t type_vocab, int64_t max_pos,
                                   int64_t padding_idx, const void* w, const void* b, int w_bf16, int64_t B, int64_t T, int64_t D,
                                   float eps, float dropout_p, const void* seed, uint32_t salt, float* y32, void* y16,
                                   const uint8_t* row_live, dalm_stream_t stream) {
  DALM_REQUIRE(B >= 0 && T >= 0, DALM_E_SHAPE, "B and T must be >= 0");
  if (B == 0 || T == 0) return 0;
  DALM_REQUIRE(ids && word && type && pos && w && b && y32 && y16, DALM_E_NULL, "null pointer argument");
  DALM_REQUIRE(B <= (1ll << 30) && T <= (1ll << 30) && B * T <= (1ll << 30), DALM_E_SHAPE, "too many rows");
  DALM_REQUIRE(D > 0 && D % 8 == 0 && D <= 2048, DALM_E_SHAPE, "D must be a multiple of 8, at most 2048");
  DALM_REQUIRE(vocab > 0 && type_vocab > 0 && max_pos > 0, DALM_E_SHAPE, "every table needs at least one row");
  DALM_REQUIRE(aligned16(word, type, pos, w, b, y32, y16), DALM_E_ALIGN, "tensors must be 16-byte aligned");
  DALM_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f && (dropout_p == 0.f || seed), DALM_E_SHAPE,
               "dropout needs 0 <= p < 1 and a device seed word");
  const int64_t R = B * T;
  DALM_REQUIRE(R * D < (1ll << 35), DALM_E_SHAPE, "tensor too large (the mask's chunk index is 32 bits)");
  EmbedNormArgs p = {};
  p.ids = reinterpret_cast<const long long*>(ids);
  p.tt = reinterpret_cast<const long long*>(token_type_ids);
  p.pos = reinterpret_cast<const long long*>(position_ids);
  p.word = word; p.type = type; p.ptab = pos; p.w = w; p.b = b;
  p.y32 = y32; p.y16 = static_cast<unsigned short*>(y16); p.live = row_live;
  p.V = vocab; p.NT = type_vocab; p.NP = max_pos; p.pad = padding_idx;
  p.R = static_cast<int>(R); p.T = static_cast<int>(T); p.D = static_cast<int>(D); p.eps = eps;
  p.keep_scale = dropout_p > 0.f ? 1.0f / (1.0f - dropout_p) : 1.0f;
  p.drop = lora::drop_args(dropout_p, seed, salt);
  if (dropout_p == 0.f) p.drop.thr16 = 0u;
  const dim3 grid(static_cast<unsigned>((R + 3) / 4));
  by_ceil<1, 2, 4>(static_cast<int>((D + 511) / 512), [&](auto nch) {   // chunks of 64 lanes x 8 elements per row
    by_bool(w_bf16 != 0, [&](auto wb) {
      hipLaunchKernelGGL((embed_norm_fwd_kernel<nch, wb>), grid, dim3(256), 0, as_stream(stream), p);
    });
  });
  return check_launch(__func__);
}
