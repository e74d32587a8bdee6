// Epilogue policies of the GEMM core that more than one translation unit uses: the row log-sum-exp partials with their merge
// kernel (lm_head forward, bf16x3 similarity row statistics) and the f32 store / accumulate (d(hidden), the similarity's dA).
#pragma once
#include "gemm256.hpp"

namespace dalm {
namespace {

// Epilogue of a wave's 128 x 128 block, all in registers (VALU only).  A 16-lane DPP row holds 16 of the 32 columns of every
// 32 x 32 tile: it reduces ITS 64 columns of a row to one (max, sum exp) partial - 2 partials per row and wave, no exchange
// between the two 16-lane rows of a half-wave.  After the butterflies every lane of the row holds the result, lane k keeps the
// one of accumulator register k and the 16 rows of a 32 x 32 tile leave in ONE store instruction.
// Labels go through the (now free) LDS: lab_s[256] = label - c0 of the tile's rows when the label falls into the tile's 256
// columns (and below V), else -1: no lane matches.
__device__ __forceinline__ void lm_tile_epilogue(const Lm8Params& p, f32x16 (&acc)[4][4], unsigned char* lds, int r0, int c0,
                                                 int nt, int wr, int wc, int tid) {
  const int lane = tid & 63, l31 = lane & 31, lhi = lane >> 5, l15 = lane & 15;
  int* lab_s = reinterpret_cast<int*>(lds);
  {
    const int r = r0 + tid;
    int y = -1;
    if (r < p.R) {
      const int64_t yl = p.labels[r] - c0;               // rows past R and labels outside this tile's columns: no match
      y = (yl >= 0 && yl < 256 && yl + c0 < p.V) ? static_cast<int>(yl) : -1;
    }
    lab_s[tid] = y;
  }
  __syncthreads();
  const int colw = wc * 128 + l31;                       // column of accumulator tile j = colw + 32 j, relative to c0
  const int64_t prow = static_cast<int64_t>((nt * 2 + wc) * 2 + (l31 >> 4)) * p.R;
  float pen[4];             // 0, or -inf for the zero-filled columns >= V of the last vocabulary tile (x + 0 is exact)
#pragma unroll
  for (int j = 0; j < 4; ++j) pen[j] = (c0 + colw + 32 * j < p.V) ? 0.f : -INFINITY;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float keep_m = 0.f, keep_s = 0.f;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int rl4 = wr * 128 + i * 32 + 8 * g + 4 * lhi;       // rows rl4 .. rl4 + 3 = accumulator registers 4 g .. 4 g + 3
      const int4 lab4 = *reinterpret_cast<const int4*>(lab_s + rl4);
      float x[4][4], m4[4], s4[4];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
#pragma unroll
        for (int j = 0; j < 4; ++j) x[rr][j] = acc[i][j][4 * g + rr] + pen[j];
        m4[rr] = max4_raw(x[rr][0], x[rr][1], x[rr][2], x[rr][3]);
      }
      row16_max4(m4[0], m4[1], m4[2], m4[3]);
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const float mneg = (m4[rr] == -INFINITY) ? 0.f : -m4[rr] * kLog2e;   // a strip entirely beyond V: (max -inf, sum 0)
        float sx = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) sx += __builtin_amdgcn_exp2f(__builtin_fmaf(x[rr][j], kLog2e, mneg));
        s4[rr] = sx;
      }
      row16_sum4(s4[0], s4[1], s4[2], s4[3]);
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int r = 4 * g + rr;
        keep_m = (l15 == r) ? m4[rr] : keep_m;
        keep_s = (l15 == r) ? s4[rr] : keep_s;
        const int dy = (rr == 0 ? lab4.x : (rr == 1 ? lab4.y : (rr == 2 ? lab4.z : lab4.w))) - colw;
        if ((dy & ~96) == 0) {                                // dy in {0, 32, 64, 96}; select chain: no run-time index into x[]
          const int jy = dy >> 5;
          p.z[r0 + rl4 + rr] = jy == 0 ? x[rr][0] : (jy == 1 ? x[rr][1] : (jy == 2 ? x[rr][2] : x[rr][3]));
        }
      }
    }
    const int row = r0 + wr * 128 + i * 32 + (l15 & 3) + 8 * (l15 >> 2) + 4 * lhi;
    if (row < p.R) {
      p.pm[prow + row] = keep_m;
      p.pl[prow + row] = keep_s;
    }
  }
}
struct EpiLse : Gemm256Epi {
  static __device__ __forceinline__ void tile(const Lm8Params& p, f32x16 (&acc)[4][4], unsigned char* lds,
                                            int r0, int c0, int nt, int nlive, int wr, int wc, int tid) {
    lm_tile_epilogue(p, acc, lds, r0, c0, nt, wr, wc, tid);
  }
};

// EPI_CSTORE: the 256 x 256 tile is stored (or added) as f32 into out[row][c0 + column]: d(hidden) += dlogits_chunk . W_chunk
__device__ __forceinline__ void lm_tile_epilogue_cstore(const Lm8Params& p, f32x16 (&acc)[4][4], int r0, int c0, int wr, int wc,
                                                        int tid) {
  const int lane = tid & 63, l31 = lane & 31, lhi = lane >> 5;
  const int col0 = c0 + wc * 128 + l31;
  float* base = static_cast<float*>(p.out) + col0;
  const int pitch = static_cast<int>(p.out_pitch);
  const bool ok0 = col0 < p.out_cols, ok1 = col0 + 32 < p.out_cols, ok2 = col0 + 64 < p.out_cols, ok3 = col0 + 96 < p.out_cols;
  const bool add = p.accumulate != 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = r0 + wr * 128 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
      if (row >= p.R) continue;
      float* dst = base + static_cast<int64_t>(row) * pitch;
      float v0 = acc[i][0][r], v1 = acc[i][1][r], v2 = acc[i][2][r], v3 = acc[i][3][r];
      if (add) {
        if (ok0) v0 += dst[0];
        if (ok1) v1 += dst[32];
        if (ok2) v2 += dst[64];
        if (ok3) v3 += dst[96];
      }
      if (ok0) dst[0] = v0;
      if (ok1) dst[32] = v1;
      if (ok2) dst[64] = v2;
      if (ok3) dst[96] = v3;
    }
  }
}
struct EpiCstore : Gemm256Epi {
  static __device__ __forceinline__ void tile(const Lm8Params& p, f32x16 (&acc)[4][4], unsigned char*,
                                            int r0, int c0, int nt, int nlive, int wr, int wc, int tid) {
    lm_tile_epilogue_cstore(p, acc, r0, c0, wr, wc, tid);
  }
};

// One workgroup = 16 rows: thread t folds the partials p = t/16, t/16 + 16, .. of row t % 16 (16 consecutive rows per
// load instruction = one 64-byte segment of the [P][R] partial arrays, 8 loads in flight), then the 16 folds of a row are
// combined through LDS in fixed order.  R/16 workgroups: the whole chip takes part (the round-2 form used R/64 = 56).
__global__ __launch_bounds__(256) void lm_head_lse_merge_kernel(const float* __restrict__ pm, const float* __restrict__ pl,
                                                                const float* __restrict__ z,
                                                                const int64_t* __restrict__ labels, int R, int V, int P,
                                                                float* __restrict__ row_lse, float* __restrict__ row_nll,
                                                                float* __restrict__ z_out = nullptr) {
  __shared__ float ms[16][17], ls[16][17];
  const int rl = threadIdx.x & 15, sub = threadIdx.x >> 4;
  const int row = blockIdx.x * 16 + rl;
  const int rr = min(row, R - 1);
  float m = -INFINITY, l = 0.f;
  for (int p0 = sub; p0 < P; p0 += 128) {
    float vm[8], vl[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int pp = min(p0 + 16 * u, P - 1);
      vm[u] = pm[static_cast<int64_t>(pp) * R + rr];
      vl[u] = pl[static_cast<int64_t>(pp) * R + rr];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (p0 + 16 * u < P && vm[u] != -INFINITY) {
        const float mn = fmaxf(m, vm[u]);
        l = l * __builtin_amdgcn_exp2f((m - mn) * kLog2e) + vl[u] * __builtin_amdgcn_exp2f((vm[u] - mn) * kLog2e);
        m = mn;
      }
    }
  }
  ms[sub][rl] = m;
  ls[sub][rl] = l;
  __syncthreads();
  if (sub == 0 && row < R) {
    float M = ms[0][rl];
#pragma unroll
    for (int i = 1; i < 16; ++i) M = fmaxf(M, ms[i][rl]);
    float L = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) L += (ms[i][rl] == -INFINITY) ? 0.f : ls[i][rl] * __builtin_amdgcn_exp2f((ms[i][rl] - M) * kLog2e);
    const float lse = M + __logf(L);
    row_lse[row] = lse;
    const int64_t y = labels[row];
    if (row_nll) row_nll[row] = (y < 0) ? 0.f : (y < V ? lse - z[row] : __builtin_nanf(""));
    if (z_out) z_out[row] = z[row];      // the similarity path wants the label's logit itself (the diagonal score)
  }
}

}  // namespace
}  // namespace dalm
