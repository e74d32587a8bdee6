// lm_head + log-sum-exp + label gather in ONE bf16 MFMA kernel: forward value of the generator loss with the
// [rows, V] logits never written anywhere (evaluation path of SURVEY.md section 8 f1).
//
// Stands in for   logits = lm_head(hidden)            dalm/models/rag_e2e_base_model.py:104-106
//                 logsumexp / gather of the label     dalm/training/utils/train_utils.py:113-131
// for rows that carry loss.  Each workgroup owns a 128 x 128 tile of (row, vocabulary) pairs, contracts it over the
// hidden width on v_mfma_f32_32x32x16_bf16 and reduces the tile IN REGISTERS to a per-row (max, sum exp) pair per 64
// columns plus the label's logit; lm_head_lse_merge_kernel folds the 2*V/128 partials of a row.
// Round 5: the backward on the same core (dalm_lm_head_dlogits / dalm_lm_head_dhidden below): with the finished row
// log-sum-exp the logits tile is RECOMPUTED per vocabulary chunk, turned into coef * (softmax - onehot) in registers, staged
// in bf16 in a chunk-sized workspace and contracted with the (transposed) chunk of W for d(hidden) - a logits-free training
// step that is hand-written end to end.
//
// Data flow per K step of 64: 16-byte global loads (full 128-byte lines per row) -> registers -> ds_write_b128 into
// rows padded to 144 bytes (conflict-free 16-byte fragment reads) -> ds_read_b128 fragments -> MFMA.  Both operands are
// K-contiguous ("B^T input"), so A and B fragments use the same addressing; the loads of step i+1 are in flight while
// step i is multiplied.  That is the round-2 kernel below, kept for operands above 4 GB; everything else runs on the 256 x 256
// core of gemm256.hpp with the epilogue policies of this file and of gemm256_epilogues.hpp.
#include "gemm256_epilogues.hpp"

namespace dalm {
namespace {

constexpr int LBN = 128;

struct LmParams {
  const unsigned short* H;   // [R, K] bf16
  const unsigned short* W;   // [V, K] bf16
  const int64_t* labels;     // [R]; < 0: row carries no loss
  int R, V, K, MT, NT, xcd_order;
  float* pm;                 // [2*NT, R] partial maxima
  float* pl;                 // [2*NT, R] partial sums of exp(x - max)
  float* z;                  // [R] logit of the label
};

// TM = 32-row MFMA tiles per wave along the rows: the workgroup tile is (64 TM) x 128, waves as 2 x 2, each 32 TM x 64.
// TM = 4 halves the LDS fragment bytes per MFMA of TM = 2 (0.75 instead of 1 fragment per MFMA).
// Measured at 3584 x 32000 x 4096 (MI355X): TM = 2: 838 TF/s, TM = 4: 881 TF/s (936 at V = 65024).  Tried and slower: a second
// LDS stage with one barrier per step (786 / 635 TF/s for TM = 2 / 4: the occupancy it costs was already doing the overlapping),
// K steps of 128 (783 TF/s).  This is the two-barrier LDS structure's ceiling (guide, section 5: ~900 TF/s); hipBLASLt's
// hand-scheduled kernel plus the forward CE kernel runs the same problem at 1285 TF/s.
template <int TM, int LBK>
__global__ __launch_bounds__(256, 2) void lm_head_lse_kernel(const LmParams p) {
  constexpr int LBM = 64 * TM;
  constexpr int LROW = LBK * 2 + 16;    // bytes per LDS row: LBK bf16 + 16 bytes of padding (conflict-free 16-byte reads)
  constexpr int CH = LBK / 8, RP = 256 / CH;   // 16-byte chunks per row; rows covered by one pass of the 256 threads
  constexpr int ATILE = LBM * LROW;     // A tile in LDS; the B tile (128 rows) follows it
  __shared__ __attribute__((aligned(16))) unsigned char lds[ATILE + LBN * LROW];
  __shared__ int lab_s[LBM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lhi = lane >> 5;
  const int wm = wave >> 1, wn = wave & 1;
  // XCD-aware order: workgroup L runs on XCD L % 8 (own 4 MB L2).  Every XCD gets a contiguous run of tile ids = a range
  // of vocabulary tiles with all their row tiles, so a 1 MB W tile is pulled into ONE L2 and shared by the row tiles that
  // use it (plain order: each W tile lands in up to 8 L2s and is shared by < 2 workgroups per XCD).  The launchers always set it.
  unsigned wgid = blockIdx.x;
  if (p.xcd_order) {
    const unsigned nwg = gridDim.x, L = blockIdx.x;
    const unsigned q8 = nwg >> 3, r8 = nwg & 7u, xcd = L & 7u;
    wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (L >> 3);
  }
  const int mt = static_cast<int>(wgid) % p.MT, nt = static_cast<int>(wgid) / p.MT;
  const int r0 = mt * LBM, c0 = nt * LBN;

  for (int t = tid; t < LBM; t += 256) {
    const int r = r0 + t;
    int y = -1;
    if (r < p.R) {
      const int64_t yl = p.labels[r];
      y = (yl < 0) ? -1 : (yl >= p.V ? -2 : static_cast<int>(yl));
    }
    lab_s[t] = y;
  }

  // staging geometry: thread t moves the 16-byte chunk (t % CH) of rows (t / CH) + RP j of both tiles
  const int srow = tid / CH, sch = tid % CH;
  constexpr int NA = LBM / RP, NB = LBN / RP;   // 16-byte loads per thread and K step
  const unsigned short* ga[NA];
  const unsigned short* gb[NB];
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    const int ra = min(r0 + srow + RP * j, p.R - 1);          // clamped: unconditional loads, results masked later
    ga[j] = p.H + static_cast<int64_t>(ra) * p.K + sch * 8;
  }
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int rb = min(c0 + srow + RP * j, p.V - 1);
    gb[j] = p.W + static_cast<int64_t>(rb) * p.K + sch * 8;
  }
  unsigned char* sa = lds + srow * LROW + sch * 16;
  unsigned char* sb = lds + ATILE + srow * LROW + sch * 16;
  const unsigned char* fa = lds + (wm * 32 * TM + l31) * LROW + lhi * 16;
  const unsigned char* fb = lds + ATILE + (wn * 64 + l31) * LROW + lhi * 16;

  f32x16 acc[TM][2];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  u32x4 ra4[NA], rb4[NB];
#pragma unroll
  for (int j = 0; j < NA; ++j) ra4[j] = *reinterpret_cast<const u32x4*>(ga[j]);
#pragma unroll
  for (int j = 0; j < NB; ++j) rb4[j] = *reinterpret_cast<const u32x4*>(gb[j]);
#pragma unroll
  for (int j = 0; j < NA; ++j) *reinterpret_cast<u32x4*>(sa + RP * j * LROW) = ra4[j];
#pragma unroll
  for (int j = 0; j < NB; ++j) *reinterpret_cast<u32x4*>(sb + RP * j * LROW) = rb4[j];
  __syncthreads();

  const int nk = p.K / LBK;
  for (int it = 0; it < nk; ++it) {
    const int kn = min(it + 1, nk - 1) * LBK;                  // last step re-reads its own tile: no branch around loads
#pragma unroll
    for (int j = 0; j < NA; ++j) ra4[j] = *reinterpret_cast<const u32x4*>(ga[j] + kn);
#pragma unroll
    for (int j = 0; j < NB; ++j) rb4[j] = *reinterpret_cast<const u32x4*>(gb[j] + kn);
    __builtin_amdgcn_sched_barrier(0);   // keep the prefetch AHEAD of the multiply (the scheduler otherwise sinks it to the barrier)
#pragma unroll
    for (int kk = 0; kk < LBK / 16; ++kk) {
      bf16x8 a[TM], b[2];
#pragma unroll
      for (int i = 0; i < TM; ++i) a[i] = *reinterpret_cast<const bf16x8*>(fa + i * 32 * LROW + kk * 32);
#pragma unroll
      for (int i = 0; i < 2; ++i) b[i] = *reinterpret_cast<const bf16x8*>(fb + i * 32 * LROW + kk * 32);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();                                           // every wave has read this step's tiles
#pragma unroll
    for (int j = 0; j < NA; ++j) *reinterpret_cast<u32x4*>(sa + RP * j * LROW) = ra4[j];
#pragma unroll
    for (int j = 0; j < NB; ++j) *reinterpret_cast<u32x4*>(sb + RP * j * LROW) = rb4[j];
    __syncthreads();
  }

  // ---- epilogue: the tile never leaves the registers ----
  // C layout of the 32x32 MFMA: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  const int colA = c0 + wn * 64 + l31, colB = colA + 32;
  const bool okA = colA < p.V, okB = colB < p.V;
  const int64_t prow = static_cast<int64_t>(nt * 2 + wn) * p.R;
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rl = wm * 32 * TM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
      const int row = r0 + rl;
      const float x0 = okA ? acc[i][0][r] : -INFINITY;
      const float x1 = okB ? acc[i][1][r] : -INFINITY;
      float m = fmaxf(x0, x1);
#pragma unroll
      for (int off = 16; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));   // stays inside the 32-lane half
      const float mref = (m == -INFINITY) ? 0.f : m;           // a 64-column strip entirely beyond V: (max -inf, sum 0)
      float s = __builtin_amdgcn_exp2f((x0 - mref) * kLog2e) + __builtin_amdgcn_exp2f((x1 - mref) * kLog2e);
#pragma unroll
      for (int off = 16; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
      if (row < p.R) {
        if (l31 == 0) {
          p.pm[prow + row] = m;
          p.pl[prow + row] = s;
        }
        const int y = lab_s[rl];
        if (y == colA) p.z[row] = x0;
        else if (y == colB) p.z[row] = x1;
      }
    }
  }
}

// EPI_DLOGITS: the 256 x 256 logits tile becomes coef_r * (exp(x - lse_r) - [column == label_r]) in registers and leaves as
// bf16 into the chunk workspace out[row][c0 + column] (columns >= V up to out_cols are written as zeros: the workspace is the A
// operand of the d(hidden) contraction).  Reference math: dalm/training/utils/train_utils.py:113-138 differentiated (SURVEY 8a:
// dL/dlogits[b,t,:] = (m_bt / M) (softmax - onehot)); coef carries m_bt / M.  Lanes l and l ^ 1 hold adjacent columns: one DPP
// exchange per pair of accumulator registers lets every lane store one dword (2 bf16) instead of two shorts.
// RAW (EPI_LOGITS): the tile leaves as it is, rounded to bf16 - the logits chunk of the two-contraction training path (round 6:
// logits chunk kept in the Infinity Cache, the fused CE kernel turns it into d(logits) in place, dalm_lm_head_dhidden contracts it).
template <bool RAW>
__device__ __forceinline__ void lm_tile_epilogue_dlogits(const Lm8Params& p, f32x16 (&acc)[4][4], unsigned char* lds, int r0, int c0,
                                                         int wr, int wc, int tid) {
  const int lane = tid & 63, l31 = lane & 31, lhi = lane >> 5;
  float* lse_s = reinterpret_cast<float*>(lds);              // [256] -lse * log2(e)
  float* cf_s = lse_s + 256;                                  // [256] coef
  int* lab_s = reinterpret_cast<int*>(lse_s + 512);           // [256] label - c0 (or -1)
  if constexpr (!RAW) {
    const int r = r0 + tid;
    float l = 0.f, c = 0.f;
    int y = -1;
    if (r < p.R) {
      l = -p.row_lse[r] * kLog2e;
      c = p.coef[r];
      const int64_t yl = p.labels[r] - p.col_base - c0;
      y = (yl >= 0 && yl < 256 && yl + c0 < p.V) ? static_cast<int>(yl) : -1;
    }
    lse_s[tid] = l; cf_s[tid] = c; lab_s[tid] = y;
  }
  __syncthreads();
  const int colw = wc * 128 + l31;                            // column of accumulator tile j = colw + 32 j, relative to c0
  const bool odd = (lane & 1) != 0;
  unsigned short* outp = static_cast<unsigned short*>(p.out);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int rl4 = wr * 128 + i * 32 + 8 * g + 4 * lhi;     // rows rl4 .. rl4 + 3 = accumulator registers 4 g .. 4 g + 3
      float ls[4] = {0.f, 0.f, 0.f, 0.f}, cs[4] = {0.f, 0.f, 0.f, 0.f};
      int ys[4] = {-1, -1, -1, -1};
      if constexpr (!RAW) {
        const float4 l4 = *reinterpret_cast<const float4*>(lse_s + rl4);
        const float4 c4 = *reinterpret_cast<const float4*>(cf_s + rl4);
        const int4 y4 = *reinterpret_cast<const int4*>(lab_s + rl4);
        ls[0] = l4.x; ls[1] = l4.y; ls[2] = l4.z; ls[3] = l4.w;
        cs[0] = c4.x; cs[1] = c4.y; cs[2] = c4.z; cs[3] = c4.w;
        ys[0] = y4.x; ys[1] = y4.y; ys[2] = y4.z; ys[3] = y4.w;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = colw + 32 * j;
        const bool live = c0 + col < p.V;
        float v[4];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          if constexpr (RAW) {
            v[rr] = live ? acc[i][j][4 * g + rr] : 0.f;
          } else {
            const float pr = __builtin_amdgcn_exp2f(__builtin_fmaf(acc[i][j][4 * g + rr], kLog2e, ls[rr]));
            v[rr] = live ? cs[rr] * (pr - (ys[rr] == col ? 1.f : 0.f)) : 0.f;
          }
        }
        // register pairs (0, 1) and (2, 3): the even lane stores row a (its column and the odd neighbour's), the odd lane row b
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const float mine_a = v[2 * h], mine_b = v[2 * h + 1];
          const float send = odd ? mine_a : mine_b;
          const float got = __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(send), 0xB1, 0xf, 0xf, false));
          const unsigned int word = odd ? pack_bf16x2(got, mine_b) : pack_bf16x2(mine_a, got);
          const int row = r0 + rl4 + 2 * h + (odd ? 1 : 0);
          const int ce = c0 + (col & ~1);                      // even column of the pair, relative to the chunk
          if (row < p.R && ce < p.out_cols)
            *reinterpret_cast<unsigned int*>(outp + static_cast<int64_t>(row) * p.out_pitch + ce) = word;
        }
      }
    }
  }
}
template <bool RAW>
struct EpiDlogits : Gemm256Epi {
  static __device__ __forceinline__ void tile(const Lm8Params& p, f32x16 (&acc)[4][4], unsigned char* lds,
                                            int r0, int c0, int nt, int nlive, int wr, int wc, int tid) {
    lm_tile_epilogue_dlogits<RAW>(p, acc, lds, r0, c0, wr, wc, tid);
  }
};

// dst[c][r] = src[r][c] for a [rows, cols] bf16 matrix (rows of `ld_src` elements) -> [cols][ld_dst], columns r >= rows of dst
// zero-filled up to ld_dst: a vocabulary chunk of the lm_head weight [Vc, K] becomes the K-contiguous B operand [K, Vc_pad] of the
// d(hidden) contraction.  64 x 64 tiles through LDS, 128-byte rows on both sides.
__global__ __launch_bounds__(256) void transpose_bf16_kernel(const unsigned short* __restrict__ src, int rows, int cols, int64_t ld_src,
                                                             unsigned short* __restrict__ dst, int64_t ld_dst) {
  __shared__ unsigned short tile[64][66];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c_in = blockIdx.x * 64 + tx;                      // source column
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int r = blockIdx.y * 64 + ty + 4 * k;               // source row
    tile[ty + 4 * k][tx] = (r < rows && c_in < cols) ? src[static_cast<int64_t>(r) * ld_src + c_in] : static_cast<unsigned short>(0);
  }
  __syncthreads();
  const int r_out = blockIdx.y * 64 + tx;                     // destination column = source row
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int c_out = blockIdx.x * 64 + ty + 4 * k;           // destination row = source column
    if (c_out < cols && r_out < ld_dst) dst[static_cast<int64_t>(c_out) * ld_dst + r_out] = tile[tx][ty + 4 * k];
  }
}

// dst (bf16) = src (f32) * scale, 8 elements per thread
__global__ __launch_bounds__(256) void f32_to_bf16_kernel(const float* __restrict__ src, unsigned short* __restrict__ dst, int64_t n8) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n8) return;
  const float4 a = *reinterpret_cast<const float4*>(src + i * 8), b = *reinterpret_cast<const float4*>(src + i * 8 + 4);
  *reinterpret_cast<uint4*>(dst + i * 8) = make_uint4(pack_bf16x2(a.x, a.y), pack_bf16x2(a.z, a.w), pack_bf16x2(b.x, b.y), pack_bf16x2(b.z, b.w));
}

}  // namespace
}  // namespace dalm

using namespace dalm;

extern "C" size_t dalm_lm_head_lse_workspace_bytes(int64_t R, int64_t V) {
  if (R <= 0 || V <= 0) return 0;
  const int64_t NT = (V + LBN - 1) / LBN;       // 2 partials per 128 columns, or 4 per 256: <= 2 NT + 2 either way
  return static_cast<size_t>((4 * NT + 8) * 2 + 1) * static_cast<size_t>(R) * sizeof(float);
}

extern "C" int dalm_lm_head_lse_fwd(const void* hidden, const void* weight, const int64_t* labels, int64_t R,
                                    int64_t V, int64_t K, float* row_lse, float* row_nll, void* ws, size_t ws_bytes,
                                    dalm_stream_t stream) {
  DALM_REQUIRE(hidden && weight && labels && row_lse && row_nll && ws, DALM_E_NULL, "null pointer argument");
  DALM_REQUIRE(R > 0 && V > 0 && K > 0 && R <= 0x7fffff00ll && V <= 0x7fffff00ll, DALM_E_SHAPE, "need R, V, K > 0");
  DALM_REQUIRE(K % 64 == 0, DALM_E_SHAPE, "the hidden width must be a multiple of 64");
  DALM_REQUIRE(reinterpret_cast<uintptr_t>(hidden) % 16 == 0 && reinterpret_cast<uintptr_t>(weight) % 16 == 0,
               DALM_E_ALIGN, "hidden / weight must be 16-byte aligned");
  DALM_REQUIRE(ws_bytes >= dalm_lm_head_lse_workspace_bytes(R, V), DALM_E_SHAPE, "workspace too small");
  hipStream_t s = as_stream(stream);
  // the 256 x 256 core needs 32-bit buffer offsets.  Unlike every other entry, this one does not fail where the shared checks
  // do: operands above 4 GB (or more tiles than one launch takes) go to the round-2 kernel below, which has its own tile check
  const Gemm256Plan pl = gemm256_plan(gemm256_dense(R, V, K), nullptr);
  if (pl.code == DALM_OK) {
    Lm8Params q{};
    gemm256_fill(q, hidden, weight, pl.g);
    q.labels = labels;
    float* f8 = static_cast<float*>(ws);
    const int64_t P4 = 4ll * q.NT;
    q.pm = f8; q.pl = f8 + P4 * R; q.z = f8 + 2 * P4 * R;
    const int rc = launch_gemm256<EpiLse>(q, s, __func__);
    if (rc != DALM_OK) return rc;
    hipLaunchKernelGGL(lm_head_lse_merge_kernel, dim3(static_cast<unsigned>((R + 15) / 16)), dim3(256), 0, s, q.pm, q.pl,
                       q.z, labels, q.R, q.V, static_cast<int>(P4), row_lse, row_nll);
    return check_launch(__func__);
  }
  // 256-row tiles (fewer LDS bytes per MFMA) once they still give every CU several tiles; 128-row tiles below that
  const int64_t NT = (V + LBN - 1) / LBN;
  const int tm = (((R + 255) / 256) * NT >= 1024) ? 4 : 2;
  const int64_t LBM = 64 * tm, MT = (R + LBM - 1) / LBM;
  DALM_REQUIRE(MT * NT <= 0x7fffffffll, DALM_E_SHAPE, "too many tiles for one launch");
  LmParams p;
  p.H = static_cast<const unsigned short*>(hidden);
  p.W = static_cast<const unsigned short*>(weight);
  p.labels = labels;
  p.R = static_cast<int>(R); p.V = static_cast<int>(V); p.K = static_cast<int>(K);
  p.MT = static_cast<int>(MT); p.NT = static_cast<int>(NT);
  p.xcd_order = 1;
  float* f = static_cast<float*>(ws);
  p.pm = f;
  p.pl = f + 2 * NT * R;
  p.z = f + 4 * NT * R;
  const dim3 grid(static_cast<unsigned>(MT * NT));
  if (tm == 4) hipLaunchKernelGGL((lm_head_lse_kernel<4, 64>), grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL((lm_head_lse_kernel<2, 64>), grid, dim3(256), 0, s, p);
  hipLaunchKernelGGL(lm_head_lse_merge_kernel, dim3(static_cast<unsigned>((R + 15) / 16)), dim3(256), 0, s, p.pm, p.pl,
                     p.z, labels, p.R, p.V, static_cast<int>(2 * NT), row_lse, row_nll);
  return check_launch(__func__);
}

// ---- round 5: the backward of the fused head -----------------------------------------------------------------
static const char* const kTooBig = "operands above 4 GB: use smaller chunks";

extern "C" int dalm_lm_head_dlogits(const void* hidden, const void* weight_chunk, const int64_t* labels, const float* row_lse,
                                    const float* coef, int64_t R, int64_t Vc, int64_t K, int64_t col_base, void* dl,
                                    int64_t pitch, dalm_stream_t stream) {
  DALM_REQUIRE(hidden && weight_chunk && labels && row_lse && coef && dl, DALM_E_NULL, "null pointer argument");
  DALM_REQUIRE(R > 0 && Vc > 0 && K > 0 && K % 64 == 0 && col_base >= 0, DALM_E_SHAPE, "need R, Vc > 0 and K a positive multiple of 64");
  DALM_REQUIRE(pitch >= Vc && pitch % 64 == 0 && pitch <= (Vc + 255) / 256 * 256, DALM_E_SHAPE,
               "pitch must be a multiple of 64 in [Vc, round_up(Vc, 256)]");
  DALM_REQUIRE(reinterpret_cast<uintptr_t>(hidden) % 16 == 0 && reinterpret_cast<uintptr_t>(weight_chunk) % 16 == 0 &&
               reinterpret_cast<uintptr_t>(dl) % 4 == 0, DALM_E_ALIGN, "hidden / weight must be 16-byte aligned");
  Lm8Params q{};
  const int rc = gemm256_params(q, __func__, hidden, weight_chunk, gemm256_dense(R, Vc, K), kTooBig);
  if (rc != DALM_OK) return rc;
  q.labels = labels; q.row_lse = row_lse; q.coef = coef; q.col_base = static_cast<int>(col_base);
  q.out = dl; q.out_pitch = pitch; q.out_cols = static_cast<int>(pitch);
  return launch_gemm256<EpiDlogits<false>>(q, as_stream(stream), __func__);
}

extern "C" int dalm_lm_head_logits(const void* hidden, const void* weight, int64_t R, int64_t V, int64_t K, void* logits, int64_t pitch,
                                   dalm_stream_t stream) {
  DALM_REQUIRE(hidden && weight && logits, DALM_E_NULL, "null pointer argument");
  DALM_REQUIRE(R > 0 && V > 0 && K > 0 && K % 64 == 0, DALM_E_SHAPE, "need R, V > 0 and K a positive multiple of 64");
  DALM_REQUIRE(pitch >= V && pitch % 2 == 0, DALM_E_SHAPE, "pitch must be even and at least V");
  DALM_REQUIRE(reinterpret_cast<uintptr_t>(hidden) % 16 == 0 && reinterpret_cast<uintptr_t>(weight) % 16 == 0 &&
               reinterpret_cast<uintptr_t>(logits) % 4 == 0, DALM_E_ALIGN, "hidden / weight must be 16-byte aligned");
  Lm8Params q{};
  const int rc = gemm256_params(q, __func__, hidden, weight, gemm256_dense(R, V, K), kTooBig);
  if (rc != DALM_OK) return rc;
  q.out = logits; q.out_pitch = pitch; q.out_cols = static_cast<int>(V % 2 ? V + 1 : V) <= pitch ? static_cast<int>(V % 2 ? V + 1 : V) : static_cast<int>(pitch);
  return launch_gemm256<EpiDlogits<true>>(q, as_stream(stream), __func__);
}

extern "C" int dalm_lm_head_dhidden(const void* dl, const void* wt, int64_t R, int64_t Vp, int64_t K, float* dh, int accumulate,
                                    dalm_stream_t stream) {
  DALM_REQUIRE(dl && wt && dh, DALM_E_NULL, "null pointer argument");
  DALM_REQUIRE(R > 0 && Vp > 0 && K > 0 && Vp % 64 == 0, DALM_E_SHAPE, "need R, K > 0 and a chunk width that is a multiple of 64");
  DALM_REQUIRE(reinterpret_cast<uintptr_t>(dl) % 16 == 0 && reinterpret_cast<uintptr_t>(wt) % 16 == 0, DALM_E_ALIGN,
               "dl / wt must be 16-byte aligned");
  Lm8Params q{};
  const int rc = gemm256_params(q, __func__, dl, wt, gemm256_dense(R, K, Vp), kTooBig);   // contracted over the chunk's vocabulary
  if (rc != DALM_OK) return rc;
  q.out = dh; q.out_pitch = K; q.out_cols = static_cast<int>(K); q.accumulate = accumulate;
  return launch_gemm256<EpiCstore>(q, as_stream(stream), __func__);
}

extern "C" int dalm_transpose_bf16(const void* src, int64_t rows, int64_t cols, int64_t ld_src, void* dst, int64_t ld_dst,
                                   dalm_stream_t stream) {
  DALM_REQUIRE(src && dst, DALM_E_NULL, "null pointer argument");
  DALM_REQUIRE(rows > 0 && cols > 0 && ld_src >= cols && ld_dst >= rows && rows <= 0x7fffffffll && cols <= 0x7fffffffll,
               DALM_E_SHAPE, "need rows, cols > 0, ld_src >= cols, ld_dst >= rows");
  const dim3 grid(static_cast<unsigned>((cols + 63) / 64), static_cast<unsigned>((ld_dst + 63) / 64));
  DALM_REQUIRE(grid.y <= 65535, DALM_E_SHAPE, "too many rows for one launch");
  hipLaunchKernelGGL(transpose_bf16_kernel, grid, dim3(256), 0, as_stream(stream), static_cast<const unsigned short*>(src),
                     static_cast<int>(rows), static_cast<int>(cols), ld_src, static_cast<unsigned short*>(dst), ld_dst);
  return check_launch(__func__);
}

extern "C" int dalm_f32_to_bf16(const float* src, void* dst, int64_t n, dalm_stream_t stream) {
  DALM_REQUIRE(src && dst, DALM_E_NULL, "null pointer argument");
  DALM_REQUIRE(n > 0 && n % 8 == 0, DALM_E_SHAPE, "need a positive multiple of 8 elements");
  DALM_REQUIRE(reinterpret_cast<uintptr_t>(src) % 16 == 0 && reinterpret_cast<uintptr_t>(dst) % 16 == 0, DALM_E_ALIGN,
               "src / dst must be 16-byte aligned");
  hipLaunchKernelGGL(f32_to_bf16_kernel, dim3(static_cast<unsigned>((n / 8 + 255) / 256)), dim3(256), 0, as_stream(stream), src,
                     static_cast<unsigned short*>(dst), n / 8);
  return check_launch(__func__);
}
