// The padded step's frozen projections over the live rows only (DESIGN.md "Live-row GEMM"): the row partition, dalm_linear_live and
// the SwiGLU MLP node's fused gate | up GEMM, the ReLU^2 MLP node's fused up GEMM - epilogue policies of the GEMM core of gemm256.hpp
// whose rows go through the partition.
#include "gemm256.hpp"
#include "relu2_math.hpp"
#include "swiglu_math.hpp"
#include <atomic>
#include <mutex>

namespace dalm {
namespace {

// EPI_LIVE (dalm_linear_live): tile position i stands for row perm[i] of A and of C.  The 256 x 256 tile leaves as bf16 into
// out[perm[i]][c0 + column] - or is added in f32 to the bf16 value already there, one rounding - with the pair exchange of the
// EPI_LOGITS epilogue (one dword per lane).  Positions n_live <= i < R of the boundary tile are dead rows: zeros when the output
// is fresh, untouched when accumulating.  A perm entry outside [0, R) stores nothing.
__device__ __forceinline__ void lm_tile_epilogue_live(const Lm8Params& p, f32x16 (&acc)[4][4], unsigned char* lds, int r0, int c0,
                                                      int nlive, int wr, int wc, int tid) {
  const int lane = tid & 63, l31 = lane & 31, lhi = lane >> 5;
  int* row_s = reinterpret_cast<int*>(lds);                   // [256] row of C behind every tile position, -1: none
  if (tid < 256) {      // true for every thread; without it the kernel compiles to other instructions (profiles/live_gemm_forms_removed.md)
    const int i = r0 + tid;
    int row = -1;
    if (i < p.R) {
      row = p.perm[i];
      if (static_cast<unsigned>(row) >= static_cast<unsigned>(p.R)) row = -1;
    }
    row_s[tid] = row;
  }
  __syncthreads();
  const int colw = wc * 128 + l31;
  const bool odd = (lane & 1) != 0;
  const bool add = p.accumulate != 0;
  unsigned short* outp = static_cast<unsigned short*>(p.out);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int rl4 = wr * 128 + i * 32 + 8 * g + 4 * lhi;   // positions rl4 .. rl4 + 3 = accumulator registers 4 g .. 4 g + 3
      const int4 rw = *reinterpret_cast<const int4*>(row_s + rl4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = colw + 32 * j;
        const int ce = c0 + (col & ~1);                          // even column of the lane pair
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const float mine_a = acc[i][j][4 * g + 2 * h], mine_b = acc[i][j][4 * g + 2 * h + 1];
          const float send = odd ? mine_a : mine_b;
          const float got = __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(send), 0xB1, 0xf, 0xf, false));
          float x0 = odd ? got : mine_a, x1 = odd ? mine_b : got;   // columns (even, odd) of this lane's position
          const int pos = r0 + rl4 + 2 * h + (odd ? 1 : 0);
          const int row = h == 0 ? (odd ? rw.y : rw.x) : (odd ? rw.w : rw.z);
          const bool live = pos < nlive;
          if (row >= 0 && ce < p.out_cols && (live || !add)) {
            unsigned int* dst = reinterpret_cast<unsigned int*>(outp + static_cast<int64_t>(row) * p.out_pitch + ce);
            unsigned int word = 0u;
            if (live) {
              if (add) {
                const unsigned int old = *dst;
                x0 += __uint_as_float(old << 16);
                x1 += __uint_as_float(old & 0xffff0000u);
              }
              word = pack_bf16x2(x0, x1);
            }
            *dst = word;
          }
        }
      }
    }
  }
}

// rb(silu(g)) for every bf16 g, indexed by g's 16 bits: 128 KB that stay in the caches.  The forward epilogue below is VALU-bound
// with its one wave per SIMD - silu is an exp, an IEEE division and two transcendental-rate instructions per element, ~14 us per
// tile against ~3 for the rest of the epilogue - and g has only 65536 values.  Filled once per device by silu_table_kernel with
// swiglu_math.hpp's own function, so an entry holds the very bits the row-wise kernel computes (NaN payloads included).
__device__ unsigned short g_silu_bf16_tab[65536];
__global__ __launch_bounds__(256) void silu_table_kernel() {
  const unsigned int i = blockIdx.x * 256 + threadIdx.x;
  g_silu_bf16_tab[i] = f32_to_bf16(swiglu_silu_rb<Bf16Round>(bf16_to_f32(static_cast<unsigned short>(i))));
}

// The row behind every position of a 256-position live tile, for the MLP epilogue below: -1 for a dead position (>= n_live)
// and for a perm entry outside [0, R) - nothing is stored for either.
__device__ __forceinline__ void lm_live_rows_to_lds(const Lm8Params& p, int* row_s, int r0, int nlive, int tid) {
  const int i = r0 + tid;
  int row = -1;
  if (i < nlive) {
    row = p.perm[i];
    if (static_cast<unsigned>(row) >= static_cast<unsigned>(p.R)) row = -1;
  }
  row_s[tid] = row;
  __syncthreads();
}

// EPI_LIVE_SWIGLU (dalm_linear_live_swiglu): the tile's 256 B rows are 128 gate rows and the 128 up rows of the SAME activation
// columns c0 .. c0 + 127, so wave (wr, 0) holds gate and wave (wr, 1) up for the same (position, column) in the same accumulator
// register of the same lane.  Both leave rounded to bf16 into y[perm[i]][c0 + col] / y[perm[i]][y_half + c0 + col] (the backward
// reads them), and act = rb(s u), s = rb(silu(g)) from the table above, leaves into out2: each wave of a pair hands the packed
// words of two of its four 32-row blocks to its partner through the LDS (free after the main loop; 16 KB per wave, lane-linear
// dwords) and computes the other two.
// Dead positions and corrupt perm entries store nothing, anywhere.
// One 32-row block of a wave in two steps.  `hand over`: pack, store this wave's half of y, leave the words in the LDS for the
// partner.  `finish`: pack, take the partner's words, gather s for all 32 words at once - the kernel runs one wave per SIMD, nothing
// else hides a load's latency, so the 64 gathers go out together and ahead of the arithmetic - then act, then the stores, whose row
// address is computed once per row.  A block is its own function so that the accumulator indices stay static.
template <bool FINISH>
__device__ __forceinline__ void lm_swiglu_block(const Lm8Params& p, const f32x16 (&a)[4], const int* row_s, unsigned int* xmine,
                                                const unsigned int* xtheirs, int rl, int ce0, bool odd, int lhi, int wc) {
  unsigned short* yp = static_cast<unsigned short*>(p.out) + (wc ? p.y_half : 0);
  unsigned short* ap = static_cast<unsigned short*>(p.out2);
  int row[4][2];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int4 rw = *reinterpret_cast<const int4*>(row_s + rl + 8 * g + 4 * lhi);
    row[g][0] = odd ? rw.y : rw.x;
    row[g][1] = odd ? rw.w : rw.z;
  }
  unsigned int word[4][4][2], actw[4][4][2];
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float mine_a = a[j][4 * g + 2 * h], mine_b = a[j][4 * g + 2 * h + 1];
        const float send = odd ? mine_a : mine_b;
        const float got = __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(send), 0xB1, 0xf, 0xf, false));
        word[g][j][h] = odd ? pack_bf16x2(got, mine_b) : pack_bf16x2(mine_a, got);
        if constexpr (!FINISH) xmine[((g * 4 + j) * 2 + h) * 64] = word[g][j][h];
      }
  if constexpr (FINISH) {
    unsigned int other[4][4][2];
    unsigned short s0[4][4][2], s1[4][4][2];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int h = 0; h < 2; ++h) other[g][j][h] = xtheirs[((g * 4 + j) * 2 + h) * 64];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const unsigned int gw = wc ? other[g][j][h] : word[g][j][h];
          s0[g][j][h] = g_silu_bf16_tab[gw & 0xffffu];
          s1[g][j][h] = g_silu_bf16_tab[gw >> 16];
        }
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const unsigned int uw = wc ? word[g][j][h] : other[g][j][h];
          const float a0 = swiglu_act_of<Bf16Round>(bf16_to_f32(s0[g][j][h]), __uint_as_float(uw << 16));
          const float a1 = swiglu_act_of<Bf16Round>(bf16_to_f32(s1[g][j][h]), __uint_as_float(uw & 0xffff0000u));
          actw[g][j][h] = pack_bf16x2(a0, a1);
        }
  }
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (row[g][h] < 0) continue;
      unsigned short* yr = yp + static_cast<int64_t>(row[g][h]) * p.out_pitch + ce0;
      unsigned short* ar = ap + static_cast<int64_t>(row[g][h]) * p.out2_pitch + ce0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        *reinterpret_cast<unsigned int*>(yr + 32 * j) = word[g][j][h];
        if constexpr (FINISH) *reinterpret_cast<unsigned int*>(ar + 32 * j) = actw[g][j][h];
      }
    }
}
__device__ __forceinline__ void lm_tile_epilogue_live_swiglu(const Lm8Params& p, f32x16 (&acc)[4][4], unsigned char* lds, int r0,
                                                             int c0, int nlive, int wr, int wc, int tid) {
  const int lane = tid & 63, l31 = lane & 31, lhi = lane >> 5;
  int* row_s = reinterpret_cast<int*>(lds);                    // [256]
  unsigned int* xch = reinterpret_cast<unsigned int*>(lds + 4096);   // [4 waves][2 blocks][32 words][64 lanes]
  lm_live_rows_to_lds(p, row_s, r0, nlive, tid);
  const bool odd = (lane & 1) != 0;
  const int ce0 = c0 + (l31 & ~1);                             // even column of the lane pair in accumulator tile j = 0 (C % 128 == 0: inside)
  unsigned int* mine = xch + (wr * 2 + wc) * 4096 + lane;
  const unsigned int* theirs = xch + (wr * 2 + (wc ^ 1)) * 4096 + lane;
  const int rl = wr * 128;
  // wave wc finishes blocks 2 wc and 2 wc + 1 and hands the other two over (wave-uniform branch, static accumulator indices)
  if (wc == 0) {
    lm_swiglu_block<false>(p, acc[2], row_s, mine, theirs, rl + 64, ce0, odd, lhi, wc);
    lm_swiglu_block<false>(p, acc[3], row_s, mine + 2048, theirs, rl + 96, ce0, odd, lhi, wc);
  } else {
    lm_swiglu_block<false>(p, acc[0], row_s, mine, theirs, rl, ce0, odd, lhi, wc);
    lm_swiglu_block<false>(p, acc[1], row_s, mine + 2048, theirs, rl + 32, ce0, odd, lhi, wc);
  }
  __syncthreads();
  if (wc == 0) {
    lm_swiglu_block<true>(p, acc[0], row_s, mine, theirs, rl, ce0, odd, lhi, wc);
    lm_swiglu_block<true>(p, acc[1], row_s, mine, theirs + 2048, rl + 32, ce0, odd, lhi, wc);
  } else {
    lm_swiglu_block<true>(p, acc[2], row_s, mine, theirs, rl + 64, ce0, odd, lhi, wc);
    lm_swiglu_block<true>(p, acc[3], row_s, mine, theirs + 2048, rl + 96, ce0, odd, lhi, wc);
  }
}

// EPI_LIVE_RELU2 (dalm_linear_live_relu2): EPI_LIVE's 256 x 256 tile and pair exchange with two outputs and no accumulating form.
// y = bf16(A . Wup^T) leaves into out[perm[i]][c0 + column], act = relu(y)^2 OF THE ROUNDED y (relu2_math.hpp: the row-wise
// kernel's function on the row-wise kernel's input) into out2 at the same place.  No partner, no table: every lane holds what its
// two columns need.  Dead positions and corrupt perm entries store nothing, anywhere; columns from out_cols on (a partial tile:
// out_cols % 8 == 0, so a column pair is inside or outside) store nothing either.
__device__ __forceinline__ void lm_tile_epilogue_live_relu2(const Lm8Params& p, f32x16 (&acc)[4][4], unsigned char* lds, int r0,
                                                            int c0, int nlive, int wr, int wc, int tid) {
  const int lane = tid & 63, l31 = lane & 31, lhi = lane >> 5;
  int* row_s = reinterpret_cast<int*>(lds);                    // [256]
  lm_live_rows_to_lds(p, row_s, r0, nlive, tid);
  const int colw = wc * 128 + l31;
  const bool odd = (lane & 1) != 0;
  unsigned short* yp = static_cast<unsigned short*>(p.out);
  unsigned short* ap = static_cast<unsigned short*>(p.out2);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int rl4 = wr * 128 + i * 32 + 8 * g + 4 * lhi;   // positions rl4 .. rl4 + 3 = accumulator registers 4 g .. 4 g + 3
      const int4 rw = *reinterpret_cast<const int4*>(row_s + rl4);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int row = h == 0 ? (odd ? rw.y : rw.x) : (odd ? rw.w : rw.z);
        unsigned short* yr = yp + static_cast<int64_t>(row) * p.out_pitch;
        unsigned short* ar = ap + static_cast<int64_t>(row) * p.out2_pitch;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int ce = c0 + ((colw + 32 * j) & ~1);            // even column of the lane pair
          const float mine_a = acc[i][j][4 * g + 2 * h], mine_b = acc[i][j][4 * g + 2 * h + 1];
          const float send = odd ? mine_a : mine_b;
          const float got = __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(send), 0xB1, 0xf, 0xf, false));
          const unsigned int word = odd ? pack_bf16x2(got, mine_b) : pack_bf16x2(mine_a, got);   // columns (even, odd) of this lane's position
          if (row >= 0 && ce < p.out_cols) {
            const float a0 = relu2_fwd_elem<Bf16Round>(__uint_as_float(word << 16));
            const float a1 = relu2_fwd_elem<Bf16Round>(__uint_as_float(word & 0xffff0000u));
            *reinterpret_cast<unsigned int*>(yr + ce) = word;
            *reinterpret_cast<unsigned int*>(ar + ce) = pack_bf16x2(a0, a1);
          }
        }
      }
    }
  }
}

// EPI_LIVE, a tile whose every position is dead (block index past the live tiles): multiplies nothing.  A fresh output gets its
// zeros here - tile positions r0 .. r0 + 255 of perm, 256 columns from c0, 16 bytes per lane - an accumulating one nothing.
__device__ __forceinline__ void lm_tile_zero_live(const Lm8Params& p, int r0, int c0, int tid) {
  if (p.accumulate) return;
  const int col = c0 + (tid & 31) * 8;
  if (col >= p.out_cols) return;                                // out_cols % 8 == 0: a 16-byte piece is inside or outside
  unsigned short* outp = static_cast<unsigned short*>(p.out);
  for (int t = tid >> 5; t < 256; t += 8) {
    const int i = r0 + t;
    if (i >= p.R) break;
    const int row = p.perm[i];
    if (static_cast<unsigned>(row) >= static_cast<unsigned>(p.R)) continue;
    *reinterpret_cast<uint4*>(outp + static_cast<int64_t>(row) * p.out_pitch + col) = make_uint4(0u, 0u, 0u, 0u);
  }
}

// ---- the policies: both gather their rows through the partition.  dalm_linear_live writes the caller's output, so its skipping
// blocks zero-fill; the MLP nodes' forwards write node-private buffers whose dead rows nobody reads: their skipping blocks return at once
struct EpiLive : Gemm256Epi {
  static constexpr bool LIVE = true;
  static __device__ __forceinline__ void skipped(const Lm8Params& p, int r0, int c0, int tid) { lm_tile_zero_live(p, r0, c0, tid); }
  static __device__ __forceinline__ void tile(const Lm8Params& p, f32x16 (&acc)[4][4], unsigned char* lds,
                                            int r0, int c0, int nt, int nlive, int wr, int wc, int tid) {
    lm_tile_epilogue_live(p, acc, lds, r0, c0, nlive, wr, wc, tid);
  }
};
struct EpiLiveSwiglu : Gemm256Epi {
  static constexpr bool LIVE = true;
  static constexpr int COLS = 128;      // a column tile is 128 activation columns - 128 gate rows and 128 up rows of W = [Wgate; Wup]
  static __device__ __forceinline__ int w_half(const Lm8Params& p) { return p.y_half; }   // gate rows c0 .., up rows y_half + c0 ..
  static __device__ __forceinline__ void tile(const Lm8Params& p, f32x16 (&acc)[4][4], unsigned char* lds,
                                            int r0, int c0, int nt, int nlive, int wr, int wc, int tid) {
    lm_tile_epilogue_live_swiglu(p, acc, lds, r0, c0, nlive, wr, wc, tid);
  }
};

struct EpiLiveRelu2 : Gemm256Epi {      // full 256-column tiles of Wup; node-private outputs: skipping blocks return at once
  static constexpr bool LIVE = true;
  static __device__ __forceinline__ void tile(const Lm8Params& p, f32x16 (&acc)[4][4], unsigned char* lds,
                                            int r0, int c0, int nt, int nlive, int wr, int wc, int tid) {
    lm_tile_epilogue_live_relu2(p, acc, lds, r0, c0, nlive, wr, wc, tid);
  }
};

// Stable partition of a row-liveness vector in ONE workgroup: thread t owns the contiguous run of rows [t per, (t + 1) per),
// counts its live rows, an inclusive scan over the 1024 counts gives every run its first live and first dead slot.  R is a
// few thousand rows per tower call: one pass of a few microseconds on the caller's stream.
__global__ __launch_bounds__(1024) void row_partition_kernel(const uint8_t* __restrict__ live, int R, int* __restrict__ perm,
                                                             int* __restrict__ n_live) {
  __shared__ int scan[1024];
  const int t = threadIdx.x;
  const int per = (R + 1023) / 1024;
  const int lo = min(t * per, R), hi = min(lo + per, R);
  int cnt = 0;
  for (int r = lo; r < hi; ++r) cnt += live[r] != 0;
  scan[t] = cnt;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int add = t >= off ? scan[t - off] : 0;
    __syncthreads();
    scan[t] += add;
    __syncthreads();
  }
  const int total = scan[1023];
  int li = scan[t] - cnt;               // live rows before this run
  int di = total + (lo - li);           // dead rows before it, behind all the live ones
  for (int r = lo; r < hi; ++r) {
    if (live[r] != 0) perm[li++] = r;
    else perm[di++] = r;
  }
  if (t == 0) *n_live = total;
}

const char* const kTooBig = "operands above 4 GB: use fewer rows per call";
}  // namespace
}  // namespace dalm

using namespace dalm;

extern "C" int dalm_row_partition(const uint8_t* live, int64_t R, int32_t* perm, int32_t* n_live, dalm_stream_t stream) {
  DALM_REQUIRE(live && perm && n_live, DALM_E_NULL, "null pointer argument");
  DALM_REQUIRE(R > 0 && R <= 0x7fffff00ll, DALM_E_SHAPE, "need 0 < R < 2^31");
  DALM_REQUIRE(reinterpret_cast<uintptr_t>(perm) % 4 == 0 && reinterpret_cast<uintptr_t>(n_live) % 4 == 0, DALM_E_ALIGN,
               "perm / n_live must be 4-byte aligned");
  hipLaunchKernelGGL(row_partition_kernel, dim3(1), dim3(1024), 0, as_stream(stream), live, static_cast<int>(R), perm, n_live);
  return check_launch(__func__);
}

extern "C" int dalm_linear_live(const void* A, int64_t lda, const void* W, void* C, int64_t ldc, int64_t R, int64_t N, int64_t K,
                                const int32_t* perm, const int32_t* n_live, int accumulate, dalm_stream_t stream) {
  DALM_REQUIRE(A && W && C && perm && n_live, DALM_E_NULL, "null pointer argument");
  DALM_REQUIRE(R > 0 && N > 0 && K > 0 && K % 64 == 0 && N % 8 == 0, DALM_E_SHAPE,
               "need R, N, K > 0, K a multiple of 64 and N a multiple of 8");
  DALM_REQUIRE(lda >= K && ldc >= N && lda % 8 == 0 && ldc % 8 == 0, DALM_E_SHAPE,
               "row strides: lda >= K, ldc >= N, both multiples of 8 elements");
  DALM_REQUIRE(R <= 0x7fffff00ll && N <= 0x7fffff00ll && lda <= 0x7fffffffll && ldc <= 0x7fffffffll, DALM_E_SHAPE,
               "operands above 4 GB: use fewer rows per call");      // also keeps the products below inside 64 bits
  DALM_REQUIRE(accumulate == 0 || accumulate == 1, DALM_E_SHAPE, "accumulate: 0 or 1");
  DALM_REQUIRE(reinterpret_cast<uintptr_t>(A) % 16 == 0 && reinterpret_cast<uintptr_t>(W) % 16 == 0 &&
               reinterpret_cast<uintptr_t>(C) % 16 == 0, DALM_E_ALIGN, "A / W / C must be 16-byte aligned");
  Lm8Params q{};
  const int rc = gemm256_params(q, __func__, A, W, gemm256_live(R, N, K, lda, N, 256), kTooBig);
  if (rc != DALM_OK) return rc;
  q.out = C; q.out_pitch = ldc; q.out_cols = static_cast<int>(N); q.accumulate = accumulate;
  q.perm = perm; q.n_live = n_live;
  return launch_gemm256<EpiLive>(q, as_stream(stream), __func__);
}

// ---- the frozen SwiGLU MLP node of the padded step: SwiGLU inside the epilogue of its gate | up live-row GEMM ------------------
namespace {
// The silu table of the current device: filled on the first call, outside any stream capture, and complete (the stream is drained)
// before the flag is set - a later call from any stream finds it whole.
std::atomic<int> g_silu_tab_ready[64];
std::mutex g_silu_tab_mutex;
int ensure_silu_table(const char* fn, dalm_stream_t stream) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return ::dalm::fail(static_cast<int>(hipErrorInvalidDevice), fn, "no current device");
  if (g_silu_tab_ready[dev].load(std::memory_order_acquire)) return DALM_OK;
  std::lock_guard<std::mutex> lock(g_silu_tab_mutex);
  if (g_silu_tab_ready[dev].load(std::memory_order_acquire)) return DALM_OK;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(as_stream(stream), &st) != hipSuccess || st != hipStreamCaptureStatusNone)
    return ::dalm::fail(static_cast<int>(hipErrorStreamCaptureUnsupported), fn,
                        "the silu table of this device is not filled yet: call dalm_linear_live_swiglu_prepare outside a stream capture first");
  hipLaunchKernelGGL(silu_table_kernel, dim3(256), dim3(256), 0, as_stream(stream));
  const hipError_t e = hipStreamSynchronize(as_stream(stream));
  if (e != hipSuccess) return ::dalm::fail(static_cast<int>(e), fn, hipGetErrorString(e));
  g_silu_tab_ready[dev].store(1, std::memory_order_release);
  return DALM_OK;
}
}  // namespace

extern "C" int dalm_linear_live_swiglu_prepare(dalm_stream_t stream) { return ensure_silu_table(__func__, stream); }

extern "C" int dalm_linear_live_swiglu(const void* A, int64_t lda, const void* Wcat, void* Y, int64_t ldy, void* Act, int64_t ldact,
                                       int64_t R, int64_t C, int64_t K, const int32_t* perm, const int32_t* n_live,
                                       dalm_stream_t stream) {
  DALM_REQUIRE(A && Wcat && Y && Act && perm && n_live, DALM_E_NULL, "null pointer argument");
  DALM_REQUIRE(C > 0 && C % 128 == 0, DALM_E_SHAPE, "need C a positive multiple of 128 (a column tile is 128 gate and 128 up rows)");
  DALM_REQUIRE(ldy >= 2 * C && ldact >= C && ldy % 8 == 0 && ldact % 8 == 0 && ldy <= 0x7fffffffll && ldact <= 0x7fffffffll,
               DALM_E_SHAPE, "row strides: ldy >= 2 C, ldact >= C, both multiples of 8 elements");
  DALM_REQUIRE(reinterpret_cast<uintptr_t>(A) % 16 == 0 && reinterpret_cast<uintptr_t>(Wcat) % 16 == 0 &&
               reinterpret_cast<uintptr_t>(Y) % 16 == 0 && reinterpret_cast<uintptr_t>(Act) % 16 == 0, DALM_E_ALIGN,
               "A / Wcat / Y / Act must be 16-byte aligned");
  // the operand checks dalm_linear_live makes: A [R, K] (stride lda) against Wcat [2 C, K]
  DALM_REQUIRE(R > 0 && C > 0 && K > 0 && K % 64 == 0 && C % 8 == 0, DALM_E_SHAPE,
               "need R, C, K > 0, K a multiple of 64 and C a multiple of 8");
  DALM_REQUIRE(lda >= K && lda % 8 == 0, DALM_E_SHAPE, "row strides: lda >= K, a multiple of 8 elements");
  DALM_REQUIRE(R <= 0x7fffff00ll && 2 * C <= 0x7fffff00ll && lda <= 0x7fffffffll, DALM_E_SHAPE, kTooBig);
  Lm8Params q{};
  const int rc = gemm256_params(q, __func__, A, Wcat, gemm256_live(R, C, K, lda, 2 * C, 128), kTooBig);
  if (rc != DALM_OK) return rc;
  q.out_cols = static_cast<int>(C);
  q.perm = perm; q.n_live = n_live;
  q.out = Y; q.out_pitch = ldy; q.y_half = static_cast<int>(C);
  q.out2 = Act; q.out2_pitch = ldact;
  const int tab = ensure_silu_table(__func__, stream);
  if (tab != DALM_OK) return tab;
  return launch_gemm256<EpiLiveSwiglu>(q, as_stream(stream), __func__);
}

// ---- the frozen ReLU^2 MLP node of the padded step (Arcee): relu(y)^2 inside the epilogue of its up GEMM ------------------------
extern "C" int dalm_linear_live_relu2(const void* A, int64_t lda, const void* Wup, void* Y, int64_t ldy, void* Act, int64_t ldact,
                                      int64_t R, int64_t C, int64_t K, const int32_t* perm, const int32_t* n_live,
                                      dalm_stream_t stream) {
  DALM_REQUIRE(R >= 0 && C >= 0, DALM_E_SHAPE, "R, C must be >= 0");
  if (R == 0 || C == 0) return 0;
  DALM_REQUIRE(A && Wup && Y && Act && perm && n_live, DALM_E_NULL, "null pointer argument");
  // the operand checks dalm_linear_live makes: A [R, K] (stride lda) against Wup [C, K]
  DALM_REQUIRE(K > 0 && K % 64 == 0 && C % 8 == 0, DALM_E_SHAPE, "need K > 0, K a multiple of 64 and C a multiple of 8");
  DALM_REQUIRE(lda >= K && ldy >= C && ldact >= C && lda % 8 == 0 && ldy % 8 == 0 && ldact % 8 == 0, DALM_E_SHAPE,
               "row strides: lda >= K, ldy >= C, ldact >= C, all multiples of 8 elements");
  DALM_REQUIRE(R <= 0x7fffff00ll && C <= 0x7fffff00ll && lda <= 0x7fffffffll && ldy <= 0x7fffffffll && ldact <= 0x7fffffffll,
               DALM_E_SHAPE, kTooBig);
  DALM_REQUIRE(reinterpret_cast<uintptr_t>(A) % 16 == 0 && reinterpret_cast<uintptr_t>(Wup) % 16 == 0 &&
               reinterpret_cast<uintptr_t>(Y) % 16 == 0 && reinterpret_cast<uintptr_t>(Act) % 16 == 0, DALM_E_ALIGN,
               "A / Wup / Y / Act must be 16-byte aligned");
  Lm8Params q{};
  const int rc = gemm256_params(q, __func__, A, Wup, gemm256_live(R, C, K, lda, C, 256), kTooBig);
  if (rc != DALM_OK) return rc;
  q.out_cols = static_cast<int>(C);
  q.perm = perm; q.n_live = n_live;
  q.out = Y; q.out_pitch = ldy;
  q.out2 = Act; q.out2_pitch = ldact;
  return launch_gemm256<EpiLiveRelu2>(q, as_stream(stream), __func__);
}
