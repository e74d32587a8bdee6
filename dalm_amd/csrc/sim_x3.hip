// The bf16x3 similarity: row statistics, the exact top-k's first pass and the backward, at f32 accuracy on the bf16 matrix cores.
// All of it runs on the GEMM core of gemm256.hpp in its SPLIT3 form; the workspace layouts are in gemm256_plan.hpp.
#include "gemm256_epilogues.hpp"

namespace dalm {
namespace {

// ------------------------------------------------------------------------------------------------------------------
// bf16x3: the f32-accurate similarity on the bf16 matrix cores.
//   reference: S = matmul(Q, P^T) * scale, get_cosine_sim, dalm/training/utils/train_utils.py:76-77 (rows of log-sum-exp:
//   :80-88); evaluation scores dalm/eval/utils.py:44-68.
// x = hi + mid + lo with hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid): every difference is exact in f32 and the
// three thirds carry 24 significand bits.  Of the nine products of two such sums the six down to 2^-16 relative are kept
// (hi lo, lo hi and mid mid are the 2^-16 ones; mid lo, lo mid, lo lo <= 2^-24 are dropped); a product of two bf16 values is
// exact in f32, the matrix core accumulates in f32.  Laid out along K - smallest products first - the whole thing is ONE
// bf16 contraction of depth 6 D that runs through the GEMM core (gemm256.hpp), row log-sum-exp epilogue included:
// 6 x the flops of the f32 kernel on a pipe with 16 x its rate.  `scale` is folded into A before the split.
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void split3_bf16_kernel(const float* __restrict__ X, int rows, int D, float scale,
                                                          unsigned short* __restrict__ out, int64_t* __restrict__ labels,
                                                          int64_t diag_offset) {
  const int per_row = D >> 3;                                   // threads per row: 8 elements each
  const int64_t gid = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const int64_t row = gid / per_row;
  const int c = static_cast<int>(gid % per_row) * 8;
  if (row >= rows) return;
  if (labels && c == 0) labels[row] = diag_offset + row;
  const float4 a = *reinterpret_cast<const float4*>(X + row * D + c);
  const float4 b = *reinterpret_cast<const float4*>(X + row * D + c + 4);
  const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  float h[8], m[8], l[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float v = __fmul_rn(x[e], scale);
    h[e] = bf16_to_f32(f32_to_bf16(v));
    const float r1 = v - h[e];                                  // exact
    m[e] = bf16_to_f32(f32_to_bf16(r1));
    l[e] = (r1 - m[e]);                                         // exact; rounded to bf16 by the pack below
  }
  unsigned short* o = out + row * (3 * static_cast<int64_t>(D)) + c;
  *reinterpret_cast<uint4*>(o) = make_uint4(pack_bf16x2(h[0], h[1]), pack_bf16x2(h[2], h[3]), pack_bf16x2(h[4], h[5]), pack_bf16x2(h[6], h[7]));
  *reinterpret_cast<uint4*>(o + D) = make_uint4(pack_bf16x2(m[0], m[1]), pack_bf16x2(m[2], m[3]), pack_bf16x2(m[4], m[5]), pack_bf16x2(m[6], m[7]));
  *reinterpret_cast<uint4*>(o + 2 * D) = make_uint4(pack_bf16x2(l[0], l[1]), pack_bf16x2(l[2], l[3]), pack_bf16x2(l[4], l[5]), pack_bf16x2(l[6], l[7]));
}

// out[d][third * ncp + j] = third(scale * B[j0 + j][d]) for j < nc, zero for nc <= j < ncp: the K-contiguous (j-contiguous)
// bf16x3 image of a block of rows of B, transposed - the B operand of dA = dS . B.  64 x 64 tiles through LDS.
__global__ __launch_bounds__(256) void split3_transpose_kernel(const float* __restrict__ Bm, int64_t j0, int nc, int D, float scale,
                                                               unsigned short* __restrict__ out, int ncp) {
  __shared__ float tile[64][65];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int d_in = blockIdx.y * 64 + tx;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int j = blockIdx.x * 64 + ty + 4 * k;
    tile[ty + 4 * k][tx] = (j < nc && d_in < D) ? __fmul_rn(Bm[(j0 + j) * static_cast<int64_t>(D) + d_in], scale) : 0.f;
  }
  __syncthreads();
  const int j_out = blockIdx.x * 64 + tx;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int d_out = blockIdx.y * 64 + ty + 4 * k;
    if (d_out >= D || j_out >= ncp) continue;
    const float v = tile[tx][ty + 4 * k];
    const float h = bf16_to_f32(f32_to_bf16(v));
    const float r1 = v - h;
    const float m = bf16_to_f32(f32_to_bf16(r1));
    unsigned short* o = out + static_cast<int64_t>(d_out) * (3 * static_cast<int64_t>(ncp)) + j_out;
    o[0] = f32_to_bf16(v);
    o[ncp] = f32_to_bf16(r1);
    o[2 * static_cast<int64_t>(ncp)] = f32_to_bf16(r1 - m);
  }
}

// MODE_GMAX epilogue (exact top-k, first pass): one maximum per (row, 32 consecutive columns) = per accumulator tile,
// written to gmax[row][column / 32] - the layout topk_threshold_kernel / topk_refine_kernel (sim.hip) read.  Zero-filled
// columns >= V count as -inf.  VALU only: 5 DPP steps per accumulator register.
__device__ __forceinline__ void lm_tile_epilogue_gmax(const Lm8Params& p, f32x16 (&acc)[4][4], int r0, int c0, int wr, int wc,
                                                      int tid) {
  const int lane = tid & 63, l31 = lane & 31, lhi = lane >> 5, l15 = lane & 15;
  const int colw = wc * 128 + l31;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float pen = (c0 + colw + 32 * j < p.V) ? 0.f : -INFINITY;
    const int g = (c0 + wc * 128 + 32 * j) >> 5;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float keep = -INFINITY;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float x0 = acc[i][j][4 * q + 0] + pen, x1 = acc[i][j][4 * q + 1] + pen;
        float x2 = acc[i][j][4 * q + 2] + pen, x3 = acc[i][j][4 * q + 3] + pen;
        half32_max4(x0, x1, x2, x3);
        keep = (l15 == 4 * q + 0) ? x0 : keep;
        keep = (l15 == 4 * q + 1) ? x1 : keep;
        keep = (l15 == 4 * q + 2) ? x2 : keep;
        keep = (l15 == 4 * q + 3) ? x3 : keep;
      }
      const int row = r0 + wr * 128 + i * 32 + (l15 & 3) + 8 * (l15 >> 2) + 4 * lhi;
      if ((l31 >> 4) == 1 && row < p.R && g < p.ng) p.gmax[static_cast<int64_t>(row) * p.ng + g] = keep;
    }
  }
}
struct EpiGmax : Gemm256Epi {
  static __device__ __forceinline__ void tile(const Lm8Params& p, f32x16 (&acc)[4][4], unsigned char*,
                                            int r0, int c0, int nt, int nlive, int wr, int wc, int tid) {
    lm_tile_epilogue_gmax(p, acc, r0, c0, wr, wc, tid);
  }
};

// EPI_DS3: the similarity backward's dS tile (reference: the autograd of get_nt_xent_loss(S) + get_nt_xent_loss(S.t()) +
// the doc term, dalm/training/utils/train_utils.py:76-88,121-124; closed form SURVEY 8a):
//   dS[i][j] = rc_i e^{S_ij - rl_i} + cc_j e^{S_ij - cl_j} - [j == diag_offset + i] (rc_i + cc_j)
// from the f32 accumulator tile of S, split into bf16 hi / mid / lo thirds (24 significand bits) and written as three images
// side by side in a row of `out` - the A operand of the dA = dS . B contraction, which runs through this same kernel
// (SPLIT3 + EPI_CSTORE).
__device__ __forceinline__ void lm_tile_epilogue_ds3(const Lm8Params& p, f32x16 (&acc)[4][4], unsigned char* lds, int r0, int c0,
                                                     int wr, int wc, int tid) {
  const int lane = tid & 63, l31 = lane & 31, lhi = lane >> 5;
  float* nrl_s = reinterpret_cast<float*>(lds);               // [256] -row_lse * log2(e)
  float* rc_s = nrl_s + 256;                                   // [256] row_coef
  float* ncl_s = nrl_s + 512;                                  // [256] -col_lse * log2(e)
  float* cc_s = nrl_s + 768;                                   // [256] col_coef
  {
    const int r = r0 + tid, c = c0 + tid;
    float a = 0.f, b = 0.f, cl = 0.f, cc = 0.f;
    if (r < p.R) { a = -p.row_lse[r] * kLog2e; b = p.coef[r]; }
    if (c < p.V) { cl = -p.col_lse[p.col_base + c] * kLog2e; cc = p.col_coef[p.col_base + c]; }
    nrl_s[tid] = a; rc_s[tid] = b; ncl_s[tid] = cl; cc_s[tid] = cc;
  }
  __syncthreads();
  const int colw = wc * 128 + l31;
  const bool odd = (lane & 1) != 0;
  unsigned short* outp = static_cast<unsigned short*>(p.out);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = colw + 32 * j;                             // relative to c0
    const bool live = c0 + col < p.V;
    const float ncl = ncl_s[col], ccj = cc_s[col];
    const int64_t gcol = static_cast<int64_t>(p.col_base) + c0 + col;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int rl4 = wr * 128 + i * 32 + 8 * g + 4 * lhi;
        const float4 l4 = *reinterpret_cast<const float4*>(nrl_s + rl4);
        const float4 c4 = *reinterpret_cast<const float4*>(rc_s + rl4);
        const float ls[4] = {l4.x, l4.y, l4.z, l4.w}, cs[4] = {c4.x, c4.y, c4.z, c4.w};
        float v[4];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const float t = acc[i][j][4 * g + rr] * kLog2e;
          float d = cs[rr] * __builtin_amdgcn_exp2f(t + ls[rr]) + ccj * __builtin_amdgcn_exp2f(t + ncl);
          const int row = r0 + rl4 + rr;
          if (gcol == p.diag_offset + row) d -= cs[rr] + ccj;
          v[rr] = (live && row < p.R) ? d : 0.f;
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const float mine_a = v[2 * h], mine_b = v[2 * h + 1];
          const float send = odd ? mine_a : mine_b;
          const float got = __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(send), 0xB1, 0xf, 0xf, false));
          const float x0 = odd ? got : mine_a, x1 = odd ? mine_b : got;      // columns (even, odd) of this lane's row
          const int row = r0 + rl4 + 2 * h + (odd ? 1 : 0);
          const int ce = c0 + (col & ~1);
          if (row < p.R && ce < p.out_cols) {
            // thirds of both columns: hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid); every difference is exact
            const unsigned int hi = pack_bf16x2(x0, x1);
            const float r0a = x0 - __uint_as_float(hi << 16), r0b = x1 - __uint_as_float(hi & 0xffff0000u);
            const unsigned int mid = pack_bf16x2(r0a, r0b);
            const unsigned int lo = pack_bf16x2(r0a - __uint_as_float(mid << 16), r0b - __uint_as_float(mid & 0xffff0000u));
            unsigned short* dst = outp + static_cast<int64_t>(row) * p.out_pitch + ce;
            *reinterpret_cast<unsigned int*>(dst) = hi;
            *reinterpret_cast<unsigned int*>(dst + p.out_third) = mid;
            *reinterpret_cast<unsigned int*>(dst + 2 * p.out_third) = lo;
          }
        }
      }
    }
  }
}
struct EpiDs3 : Gemm256Epi {
  static __device__ __forceinline__ void tile(const Lm8Params& p, f32x16 (&acc)[4][4], unsigned char* lds,
                                            int r0, int c0, int nt, int nlive, int wr, int wc, int tid) {
    lm_tile_epilogue_ds3(p, acc, lds, r0, c0, wr, wc, tid);
  }
};

// the two images every entry point starts from: scale * A and B as (hi, mid, lo) thirds; `labels` (may be NULL) gets the positives
void split3_operands(hipStream_t s, const float* A, const float* Bm, int64_t m, int64_t n, int64_t D, float scale, unsigned short* a3,
                     unsigned short* b3, int64_t* labels, int64_t diag_offset) {
  const int per_row = static_cast<int>(D / 8);
  hipLaunchKernelGGL(split3_bf16_kernel, dim3(static_cast<unsigned>((m * per_row + 255) / 256)), dim3(256), 0, s, A,
                     static_cast<int>(m), static_cast<int>(D), scale, a3, labels, diag_offset);
  hipLaunchKernelGGL(split3_bf16_kernel, dim3(static_cast<unsigned>((n * per_row + 255) / 256)), dim3(256), 0, s, Bm,
                     static_cast<int>(n), static_cast<int>(D), 1.0f, b3, static_cast<int64_t*>(nullptr), static_cast<int64_t>(0));
}
// the pointer the offsets of a layout count from: 256 bytes below the caller's pointer aligned up to 256 (offsets start at 256, so
// base + L.x is 256-byte aligned and inside the caller's buffer)
inline char* x3_base(void* ws) { return align_up(ws, 256) - 256; }

// The 4 GB and tile-count checks of gemm256_params cannot trip in this file: dalm_sim_rowstats_bf16x3_supported and
// dalm_sim_grad_bf16x3_supported bound the very spans it checks, and an operand of rows of 384 bytes or more below 4 GB has fewer
// than 2^16 tiles a side.  The two launches of the backward, which had no tile-count check of their own, get it from there like
// everyone else; no accepted call starts failing.
const char* const kTooBig = "operand images above 4 GB";

}  // namespace
}  // namespace dalm

using namespace dalm;

extern "C" int dalm_sim_rowstats_bf16x3_supported(int64_t m, int64_t n, int64_t D) {
  if (m <= 0 || n <= 0 || D < 64 || D % 64 != 0) return 0;
  if (D / 64 > 1024) return 0;                                                       // the reciprocal of the tile lookup
  if (static_cast<uint64_t>(m + 256) * 3 * D * 2 >= 0xffffff00ull) return 0;           // 32-bit buffer offsets
  if (static_cast<uint64_t>(n + 256) * 3 * D * 2 >= 0xffffff00ull) return 0;
  return 1;
}

extern "C" size_t dalm_sim_rowstats_bf16x3_workspace_bytes(int64_t m, int64_t n, int64_t D) {
  if (!dalm_sim_rowstats_bf16x3_supported(m, n, D)) return 0;
  return x3_layout(m, n, D).total;
}

extern "C" int dalm_sim_rowstats_bf16x3(const float* A, const float* Bm, int64_t m, int64_t n, int64_t D, float scale,
                                        int64_t diag_offset, float* row_lse, float* diag, void* ws, size_t ws_bytes,
                                        dalm_stream_t stream) {
  DALM_REQUIRE(A && Bm && row_lse && diag && ws, DALM_E_NULL, "null pointer argument");
  DALM_REQUIRE(dalm_sim_rowstats_bf16x3_supported(m, n, D), DALM_E_SHAPE,
               "bf16x3 similarity needs D % 64 == 0 and operand images below 4 GB (dalm_sim_rowstats_bf16x3_supported)");
  DALM_REQUIRE(diag_offset >= 0 && diag_offset + m <= n, DALM_E_SHAPE, "diag_offset + m must be <= n");
  DALM_REQUIRE(reinterpret_cast<uintptr_t>(A) % 16 == 0 && reinterpret_cast<uintptr_t>(Bm) % 16 == 0, DALM_E_ALIGN,
               "A / B must be 16-byte aligned");
  const X3Layout L = x3_layout(m, n, D);
  DALM_REQUIRE(ws_bytes >= L.total, DALM_E_WORKSPACE, "workspace too small");
  hipStream_t s = as_stream(stream);
  char* base = x3_base(ws);
  auto* a3 = region<unsigned short>(base, L.a3);
  auto* b3 = region<unsigned short>(base, L.b3);
  auto* labels = region<int64_t>(base, L.labels);
  split3_operands(s, A, Bm, m, n, D, scale, a3, b3, labels, diag_offset);
  Lm8Params q{};
  int rc = gemm256_params(q, __func__, a3, b3, gemm256_split3(m, n, D), kTooBig);
  if (rc != DALM_OK) return rc;
  q.labels = labels;
  q.pm = region(base, L.pm); q.pl = region(base, L.pl); q.z = region(base, L.z);
  rc = launch_gemm256<EpiLse, true>(q, s, __func__);
  if (rc != DALM_OK) return rc;
  hipLaunchKernelGGL(lm_head_lse_merge_kernel, dim3(static_cast<unsigned>((m + 15) / 16)), dim3(256), 0, s, q.pm, q.pl, q.z,
                     labels, q.R, q.V, static_cast<int>(L.P4), row_lse, static_cast<float*>(nullptr), diag);
  return check_launch(__func__);
}


// ---- bf16x3 group maxima for the exact top-k (first pass of dalm_sim_topk): gmax[m][ng], ng groups of 32 columns ----
extern "C" size_t dalm_x3_group_max_workspace_bytes(int64_t m, int64_t n, int64_t D) {
  if (!dalm_sim_rowstats_bf16x3_supported(m, n, D)) return 0;
  return x3_images_layout(m, n, D).total;
}

extern "C" int dalm_x3_group_max(const float* A, const float* Bm, int64_t m, int64_t n, int64_t D, float scale, float* gmax,
                                 int64_t ng, void* ws, size_t ws_bytes, dalm_stream_t stream) {
  DALM_REQUIRE(A && Bm && gmax && ws, DALM_E_NULL, "null pointer argument");
  DALM_REQUIRE(dalm_sim_rowstats_bf16x3_supported(m, n, D), DALM_E_SHAPE, "shape outside the bf16x3 form");
  DALM_REQUIRE(ws_bytes >= dalm_x3_group_max_workspace_bytes(m, n, D), DALM_E_WORKSPACE, "workspace too small");
  DALM_REQUIRE(ng > 0 && ng <= 0x7fffffffll, DALM_E_SHAPE, "need ng > 0");
  hipStream_t s = as_stream(stream);
  const X3Layout L = x3_images_layout(m, n, D);
  char* base = x3_base(ws);
  auto* a3 = region<unsigned short>(base, L.a3);
  auto* b3 = region<unsigned short>(base, L.b3);
  split3_operands(s, A, Bm, m, n, D, scale, a3, b3, nullptr, 0);
  Lm8Params q{};
  const int rc = gemm256_params(q, __func__, a3, b3, gemm256_split3(m, n, D), kTooBig);
  if (rc != DALM_OK) return rc;
  q.gmax = gmax; q.ng = static_cast<int>(ng);
  return launch_gemm256<EpiGmax, true>(q, s, __func__);
}

// ---- round 5: the similarity BACKWARD on the bf16 pipe ---------------------------------------------------
//   reference: the autograd of get_cosine_sim + get_nt_xent_loss (x2) + the doc term, dalm/training/utils/train_utils.py:76-88
// dA = scale * dS . B with dS rebuilt from S = scale * A . B^T: both contractions as bf16x3 (six significant products, f32
// accumulation) through the lm_head core - per block of `nc` columns of S: (1) S tile -> dS thirds image (EPI_DS3), (2) the
// transposed thirds image of the block's rows of B, (3) dA (+)= dS_blk . B_blk (SPLIT3 + EPI_CSTORE).  24 m n D bf16 flops
// instead of 6 m n D on the f32 pipe (1/16 of the rate).
extern "C" int dalm_sim_grad_bf16x3_supported(int64_t m, int64_t n, int64_t D) {
  if (!dalm_sim_rowstats_bf16x3_supported(m, n, D)) return 0;
  const int64_t blk = x3_grad_block(m);
  const int64_t ncp = n < blk ? (n + 255) / 256 * 256 : blk;
  if (static_cast<uint64_t>(m + 256) * 3 * ncp * 2 >= 0xffffff00ull) return 0;       // 32-bit buffer offsets of the dS image
  if (static_cast<uint64_t>(D + 256) * 3 * ncp * 2 >= 0xffffff00ull) return 0;
  return 1;
}

extern "C" size_t dalm_sim_grad_bf16x3_workspace_bytes(int64_t m, int64_t n, int64_t D) {
  if (!dalm_sim_grad_bf16x3_supported(m, n, D)) return 0;
  return x3_grad_layout(m, n, D).total;
}

extern "C" int dalm_sim_grad_bf16x3(const float* A, const float* Bm, int64_t m, int64_t n, int64_t D, float scale,
                                    int64_t diag_offset, const float* row_coef, const float* row_lse, const float* col_coef,
                                    const float* col_lse, float* dA, void* ws, size_t ws_bytes, dalm_stream_t stream) {
  DALM_REQUIRE(A && Bm && row_coef && row_lse && col_coef && col_lse && dA && ws, DALM_E_NULL, "null pointer argument");
  DALM_REQUIRE(dalm_sim_grad_bf16x3_supported(m, n, D), DALM_E_SHAPE,
               "bf16x3 similarity backward needs D % 64 == 0 and operand images below 4 GB (dalm_sim_grad_bf16x3_supported)");
  DALM_REQUIRE(diag_offset >= 0 && diag_offset + m <= n, DALM_E_SHAPE, "diag_offset + m must be <= n");
  DALM_REQUIRE(reinterpret_cast<uintptr_t>(A) % 16 == 0 && reinterpret_cast<uintptr_t>(Bm) % 16 == 0, DALM_E_ALIGN,
               "A / B must be 16-byte aligned");
  const X3GradLayout L = x3_grad_layout(m, n, D);
  DALM_REQUIRE(ws_bytes >= L.total, DALM_E_WORKSPACE, "workspace too small");
  hipStream_t s = as_stream(stream);
  char* base = x3_base(ws);
  auto* a3 = region<unsigned short>(base, L.a3);
  auto* b3 = region<unsigned short>(base, L.b3);
  auto* ds3 = region<unsigned short>(base, L.ds3);
  auto* bt3 = region<unsigned short>(base, L.bt3);
  split3_operands(s, A, Bm, m, n, D, scale, a3, b3, nullptr, 0);
  for (int64_t j0 = 0; j0 < n; j0 += L.ncp) {
    const int64_t nc = n - j0 < L.ncp ? n - j0 : L.ncp;
    {  // (1) S tile -> dS thirds
      Lm8Params q{};
      int rc = gemm256_params(q, __func__, a3, b3 + j0 * 3 * D, gemm256_split3(m, nc, D), kTooBig);
      if (rc != DALM_OK) return rc;
      q.row_lse = row_lse; q.coef = row_coef; q.col_lse = col_lse; q.col_coef = col_coef;
      q.col_base = static_cast<int>(j0); q.diag_offset = diag_offset;
      q.out = ds3; q.out_pitch = 3 * L.ncp; q.out_third = L.ncp; q.out_cols = static_cast<int>(L.ncp);
      rc = launch_gemm256<EpiDs3, true>(q, s, __func__);
      if (rc != DALM_OK) return rc;
    }
    hipLaunchKernelGGL(split3_transpose_kernel, dim3(static_cast<unsigned>(L.ncp / 64), static_cast<unsigned>((D + 63) / 64)),
                       dim3(256), 0, s, Bm, j0, static_cast<int>(nc), static_cast<int>(D), scale, bt3, static_cast<int>(L.ncp));
    {  // (3) dA (+)= dS_blk . B_blk: the thirds are L.ncp wide here
      Lm8Params q{};
      int rc = gemm256_params(q, __func__, ds3, bt3, gemm256_split3(m, D, L.ncp), kTooBig);
      if (rc != DALM_OK) return rc;
      q.out = dA; q.out_pitch = D; q.out_cols = static_cast<int>(D); q.accumulate = j0 > 0;
      rc = launch_gemm256<EpiCstore, true>(q, s, __func__);
      if (rc != DALM_OK) return rc;
    }
  }
  return check_launch(__func__);
}
