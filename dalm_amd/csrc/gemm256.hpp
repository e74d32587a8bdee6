// The in-house bf16 MFMA GEMM core: C [R, V] = H [R, K] . W [V, K]^T on 256 x 256 x 64 tiles, f32 accumulators that never leave
// the registers before an EPILOGUE POLICY has turned them into what its entry point wants.  The core knows no user: lmhead.hip
// (fused lm_head forward and backward), sim_x3.hip (bf16x3 similarity) and linear_live.hip (live-row frozen projections, SwiGLU
// MLP node) each define their policies, fill an Lm8Params through gemm256_params (geometry and checks: gemm256_plan.hpp) and
// launch through launch_gemm256.  Every translation unit that includes this header compiles its own instantiations.
#pragma once
#include "common.hpp"
#include "gemm256_plan.hpp"

namespace dalm {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------------------------
// The structure, built from measurements on the MI355X for the lm_head contraction (round 3; ablation builds,
// profiles/history/r03_lm_head_*): 256 x 256 x 64 tiles, FOUR waves = one per SIMD with the whole 512-register file each,
// operands straight from global memory into LDS (buffer_load_dwordx4 ... lds), ONE barrier per K tile, a VALU-only epilogue,
// one workgroup per tile.  What the intermediate forms showed:
//   * 8 waves in ping-pong with two barriers per 8 MFMAs (the published "8-phase" shape): even its MFMA-and-barriers-only
//     skeleton stops at 1.2 PF/s - an s_barrier hand-off costs ~150 cycles during which nothing multiplies;
//   * 32-lane __shfl_xor reductions in the epilogue = 640 ds_bpermute round trips per lane and tile: 30 % of the kernel;
//   * every direct-to-LDS piece costs the issuing wave ~25-50 cycles that no second wave per SIMD hides (8 free-running
//     waves measured SLOWER than 4), issuing a tile's 16 pieces as early as possible beats spreading them, and a four-stage
//     ring of 32-deep tiles (3 stages of prefetch) is no faster than two 64-deep buffers;
//   * L2 hit rate 50 % -> 78 % with the banded tile order below.
//
// Workgroup = 4 waves as 2 x 2; a wave owns 128 x 128 outputs = 16 accumulator tiles of 32 x 32 (256 AGPRs).  A K tile
// (64 deep) is walked in four k-steps of 16 MFMAs (512 matrix-pipe cycles); the 8 fragments of the NEXT k-step are read from
// LDS and the load pieces of a later K tile are issued in the shadow of the current k-step's MFMAs (explicit
// sched_group_barrier interleave: MFMA / ds_read / MFMA / ds_read ... MFMA / buffer_load ...):
//     k-step 0..2 of tile t : multiply | read k-step +1 of tile t            | 8 of the 16 pieces of tile t+1 (k-step 0)
//     s_waitcnt vmcnt(0) lgkmcnt(0); s_barrier          -> tile t+1 has landed for everybody, tile t's buffer is free
//     k-step 3 of tile t    : multiply | read k-step 0 of tile t+1           | the first 8 pieces of tile t+2 (tile t's buffer)
// LDS image of a K tile: per operand [256 rows][128 bytes], 16-byte chunk c of row r stored at chunk c ^ ((r >> 1) & 7): the
// 16 lanes a ds_read_b128 services together (16 rows, one k-chunk) hit 16 different 16-byte slots of the 256-byte bank row.
// The LDS-DMA writes lane-linear, so the permutation is applied to the per-lane SOURCE offset (within one 128-byte line: still
// full-line requests) and again on the read.  Rows / vocabulary entries past the end read as zero through the buffer
// descriptor's range check (no clamping, no branches); the zero-filled vocabulary columns leave the reduction in the epilogue.
// One workgroup per output tile, dispatched in the banded order below.  (A persistent form - every workgroup walking its share
// of the tile list and requesting the next tile's first K tile ahead of the epilogue - measured 3-4 % SLOWER: static
// assignment loses the dispatcher's load balancing and the extra live state spilled.)
struct Lm8Params {
  const void* H;             // [R, K] bf16
  const void* W;             // [V, K] bf16
  const int64_t* labels;     // [R]
  int R, V, K, MT, NT, xcd_order;
  int gh;                    // row tiles per band of the tile order (see lm_tile_of)
  unsigned bytesH, bytesW;
  unsigned pitchH, pitchW;   // bytes between rows of H / W (K * 2 for the lm_head; 3 D * 2 for the bf16x3 similarity operands)
  int tpd;                   // SPLIT3: K tiles (64 deep) per segment = D / 64
  unsigned tpd_inv;          // SPLIT3: ceil(2^24 / tpd): u / tpd == (u * tpd_inv) >> 24 for u < 6 tpd, tpd <= 1024 (gemm256_tpd_inv)
  unsigned seg_bytes;        // SPLIT3: D * 2
  float* gmax;               // [R][ng] one maximum per (row, 32 consecutive columns)
  int ng;
  float* pm;                 // [4*NT, R]
  float* pl;                 // [4*NT, R]
  float* z;                  // [R]
  // epilogue operands: what each slot means is its policy's business; the comments name the first user
  const float* row_lse;      // [R] log-sum-exp of every row over the WHOLE vocabulary
  const float* coef;         // [R] d loss / d log-prob of the row's label (0 for rows without loss)
  union {
    int col_base;            // first vocabulary entry of this chunk (labels are global ids)
    int y_half;              // gate | up policies: columns between the two halves of a row of y (= C)
  };
  void* out;                 // bf16 or f32 [R][out_pitch]
  int64_t out_pitch;         // elements
  int out_cols;              // columns that exist in `out` (zero-filled from V up to here where the policy says so)
  int accumulate;            // add to what `out` holds
  // the similarity backward's dS policy; row statistics ride in row_lse / coef above
  // The frozen MLP node's forward policy keeps its second output in the same slots - the struct, and with it the kernel-argument
  // layout every other instantiation was compiled against, does not grow: y = [gate | up] leaves through `out`, act through out2
  const float* col_lse;                                  // [V] column log-sum-exp (global column = col_base + local)
  union { const float* col_coef; void* out2; };          // [V]
  int64_t diag_offset;                                   // the positive of row i is global column diag_offset + i
  union { int64_t out_third; int64_t out2_pitch; };      // elements between the hi / mid / lo images inside a row of `out`
  // live policies: the rows of H and `out` go through a stable partition of the row-liveness vector
  const int* perm;           // [R] live rows first (ascending), then the dead ones
  const int* n_live;         // device scalar: how many leading entries of perm are live (clamped to [0, R] by the kernel)
};
// the kernel-argument layout every instantiation is compiled against
static_assert(sizeof(Lm8Params) == 216 && offsetof(Lm8Params, gmax) == 80 && offsetof(Lm8Params, out) == 144 &&
              offsetof(Lm8Params, perm) == 200, "Lm8Params changed its layout");

constexpr int L8_BUF = 65536;

// the tile of a block in the banded order of gemm256_plan.hpp
__device__ __forceinline__ void lm_tile_of(const Lm8Params& p, unsigned block, unsigned nblocks, int& mt, int& nt) {
  lm_tile_order(p.xcd_order, static_cast<unsigned>(p.gh), static_cast<unsigned>(p.NT), static_cast<unsigned>(p.MT), block, nblocks,
                mt, nt);
}

typedef __attribute__((address_space(3))) void lds_void_t;

// Four independent reductions over the 16 lanes of a DPP row at once (xor 1, xor 2 as quad_perm, then the two mirrors; every
// lane receives the result), written out in assembly: (1) fmaxf() lowers to a canonicalising v_max x, x in front of every
// v_max and keeps the DPP move separate (3 instructions + s_nop 1 per step); (2) a VALU result needs two wait states before a
// DPP instruction may read it - with four chains interleaved the next step of a chain is 3 instructions behind its producer
// and no s_nop is needed.  v_max_f32 returns the other operand for a NaN, as fmaxf does.
#define DALM_DPP4(OP, CTRL)                                                                                          \
  OP " %0, %0, %0 " CTRL " row_mask:0xf bank_mask:0xf\n\t" OP " %1, %1, %1 " CTRL " row_mask:0xf bank_mask:0xf\n\t"  \
  OP " %2, %2, %2 " CTRL " row_mask:0xf bank_mask:0xf\n\t" OP " %3, %3, %3 " CTRL " row_mask:0xf bank_mask:0xf\n\t"
__device__ __forceinline__ void row16_max4(float& a, float& b, float& c, float& d) {
  asm volatile("s_nop 1\n\t" DALM_DPP4("v_max_f32_dpp", "quad_perm:[1,0,3,2]") DALM_DPP4("v_max_f32_dpp", "quad_perm:[2,3,0,1]")
               DALM_DPP4("v_max_f32_dpp", "row_half_mirror") DALM_DPP4("v_max_f32_dpp", "row_mirror") "s_nop 0"
               : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
}
__device__ __forceinline__ void row16_sum4(float& a, float& b, float& c, float& d) {
  asm volatile("s_nop 1\n\t" DALM_DPP4("v_add_f32_dpp", "quad_perm:[1,0,3,2]") DALM_DPP4("v_add_f32_dpp", "quad_perm:[2,3,0,1]")
               DALM_DPP4("v_add_f32_dpp", "row_half_mirror") DALM_DPP4("v_add_f32_dpp", "row_mirror") "s_nop 0"
               : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
}
// max over the 32 lanes of each half-wave for four registers at once: the 16-lane butterflies of row16_max4, then lane 15
// of rows 0 / 2 (which holds its row's maximum) is broadcast into rows 1 / 3 (`row_bcast:15`, a GFX9 DPP control; row_mask
// 0xa enables rows 1 and 3 only): the lanes of rows 1 and 3 end up with the half-wave maximum, rows 0 and 2 keep theirs.
__device__ __forceinline__ void half32_max4(float& a, float& b, float& c, float& d) {
  asm volatile("s_nop 1\n\t" DALM_DPP4("v_max_f32_dpp", "quad_perm:[1,0,3,2]") DALM_DPP4("v_max_f32_dpp", "quad_perm:[2,3,0,1]")
               DALM_DPP4("v_max_f32_dpp", "row_half_mirror") DALM_DPP4("v_max_f32_dpp", "row_mirror")
               "v_max_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
               "v_max_f32_dpp %1, %1, %1 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
               "v_max_f32_dpp %2, %2, %2 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
               "v_max_f32_dpp %3, %3, %3 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
               "s_nop 0"
               : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
}
#undef DALM_DPP4
// max of four finite-or--inf values without the canonicalising self-max fmaxf() puts in front of every operand
__device__ __forceinline__ float max4_raw(float a, float b, float c, float d) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3\n\tv_max_f32 %0, %0, %4" : "=&v"(r) : "v"(a), "v"(b), "v"(c), "v"(d));
  return r;
}

// one direct-to-LDS piece: 64 lanes x 16 bytes -> dst + 16 * lane (dst wave-uniform); its own function so that the host pass,
// which has no such builtin, never sees it inside a kernel body
__device__ __forceinline__ void lds_dma16(__amdgpu_buffer_rsrc_t rs, unsigned char* dst, unsigned voff, int soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t*)dst, 16, static_cast<int>(voff), soff, 0, 0);
}

// What the core asks of an epilogue policy `Epi`; a policy derives from this and overrides what differs.
struct Gemm256Epi {
  static constexpr bool LIVE = false;   // tile position i stands for row perm[i]; blocks past the live row tiles skip the multiply
  // output columns behind a column tile.  256: its B rows are rows c0 .. c0 + 255 of W.  128: two halves of 128 rows, c0 .. and
  // w_half(p) + c0 .., which wave columns 0 and 1 hold for the same output columns and the epilogue combines
  static constexpr int COLS = 256;
  static __device__ __forceinline__ int w_half(const Lm8Params&) { return 0; }
  // LIVE: a block whose every position is dead; (r0, c0) is the tile it would have had
  static __device__ __forceinline__ void skipped(const Lm8Params&, int, int, int) {}
  // every policy defines
  //   static __device__ void tile(const Lm8Params& p, f32x16 (&acc)[4][4], unsigned char* lds,
  //                               int r0, int c0, int nt, int nlive, int wr, int wc, int tid)
  // for the accumulators of wave (wr, wc)'s 128 x 128 block of the tile at (r0, c0), the whole LDS free for its use
};

// SPLIT3 (the bf16x3 similarity, sim_x3.hip): the operands are [rows][3 D] bf16 images holding the (hi, mid,
// lo) bf16 thirds of an f32 matrix side by side; the contraction walks SIX segments of D - the six significant products of
// (hi + mid + lo) x (hi + mid + lo), smallest first - and K tile u reads third segA[u / tpd] of H against third segB[u / tpd]
// of W: the same main loop, only the K offset of a tile is looked up instead of being u * 128.
template <class Epi, bool SPLIT3 = false>
__global__ __launch_bounds__(256, 1) void gemm256_kernel(const Lm8Params p) {
  constexpr bool LIVE = Epi::LIVE;
  static_assert(Epi::COLS == 256 || Epi::COLS == 128, "tiles of 256 or 128 columns");
  constexpr int NA = 8, NP = 16;                 // load pieces of 32 rows per K tile: NA of the A tile, then 8 of the B tile
  constexpr int NM = 16, NR = 8;                 // MFMAs and fragment reads per k-step
  // load pieces (NP per K tile and wave) issued in k-step 3 (right after the barrier) / 0 / 1 / 2: measured best of the placements
  constexpr int N3 = NP / 2, N0 = NP - NP / 2, N1 = 0, N2 = 0;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * L8_BUF];
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lhi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 1, wc = wave & 1;
  int mt, nt;
  int nlive = 0;
  if constexpr (LIVE) {
    // the live row-tile count is a device value: the banded order runs over the live tiles, the skipping tiles come last
    nlive = min(max(*p.n_live, 0), p.R);
    const unsigned NT = static_cast<unsigned>(p.NT), mtl = static_cast<unsigned>((nlive + 255) / 256);
    const unsigned nlb = mtl * NT;
    if (blockIdx.x >= nlb) {
      const unsigned s = blockIdx.x - nlb;
      Epi::skipped(p, static_cast<int>(mtl + s / NT) * 256, static_cast<int>(s % NT) * Epi::COLS, tid);
      return;
    }
    lm_tile_order(p.xcd_order, gemm256_band(mtl), NT, mtl, blockIdx.x, nlb, mt, nt);
  } else {
    lm_tile_of(p, blockIdx.x, gridDim.x, mt, nt);
  }
  const int r0 = mt * 256, c0 = nt * Epi::COLS;
  const __amdgpu_buffer_rsrc_t rsH = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.H), 0, static_cast<int>(p.bytesH), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.W), 0, static_cast<int>(p.bytesW), 0x00020000);

  // load piece q (0..NA-1: rows 32 q .. 32 q + 31 of the A tile, NA..NP-1: of the B tile): thread -> row 32 q + tid / 8, chunk tid % 8
  const int srow = tid >> 3;
  const unsigned schunk = static_cast<unsigned>(((tid & 7) ^ ((srow >> 1) & 7)) * 16);
  unsigned voff[NP];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    if constexpr (LIVE) {
      // row gather: the A row of position i is perm[i]; a dead position gets row R = past the descriptor's range, reads zero
      const int i = r0 + q * 32 + srow;
      int row = p.R;
      if (i < nlive) {
        row = p.perm[i];
        if (static_cast<unsigned>(row) >= static_cast<unsigned>(p.R)) row = p.R;
      }
      voff[q] = static_cast<unsigned>(row) * p.pitchH + schunk;
    } else {
      voff[q] = static_cast<unsigned>(r0 + q * 32 + srow) * p.pitchH + schunk;
    }
    if constexpr (Epi::COLS == 128)         // pieces 0..3: the first half, 4..7: the second
      voff[NA + q] = static_cast<unsigned>((q < 4 ? c0 + q * 32 : Epi::w_half(p) + c0 + (q - 4) * 32) + srow) * p.pitchW + schunk;
    else
      voff[NA + q] = static_cast<unsigned>(c0 + q * 32 + srow) * p.pitchW + schunk;
  }
  const int wave_lds = wave * 1024;
#define L4_DMA(BUF, Q, KSA, KSB) lds_dma16((Q) < NA ? rsH : rsW, lds + (BUF) * L8_BUF + (Q) * 4096 + wave_lds, voff[Q], (Q) < NA ? (KSA) : (KSB));

  const int f = (l31 >> 1) & 7;
  int koff[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) koff[kk] = ((kk * 2 + lhi) ^ f) * 16;
  const int abase = (wr * 128 + l31) * 128;
  const int bbase = NA * 4096 + (wc * 128 + l31) * 128;

  f32x16 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nkt = p.K / 64;
  // byte offset of K tile u inside a row of H (SIDE 0) / W (SIDE 1); tiles past the end re-read the last one (no branch)
  //   pairs in contraction order: (m,m) (h,l) (l,h) (h,m) (m,h) (h,h) with h = third 0, m = third 1, l = third 2
  //   third of H per pair, 2 bits each: 1,0,2,0,1,0 -> 0x121;  of W: 1,2,0,1,0,0 -> 0x049
  auto ks = [&](int u, int side) -> int {
    u = min(u, nkt - 1);
    if constexpr (!SPLIT3) {
      return u * 128;
    } else {
      const int sg = static_cast<int>((static_cast<unsigned>(u) * p.tpd_inv) >> 24);
      const int w = u - sg * p.tpd;
      const unsigned third = ((side ? 0x049u : 0x121u) >> (2 * sg)) & 3u;
      return static_cast<int>(third * p.seg_bytes) + w * 128;
    }
  };
  bf16x8 fa0[4], fb0[4], fa1[4], fb1[4];

  // (the A and B reads of one i interleave)
#define L4_READ(BUF, KK, FA, FB)                                                                                      \
  _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                                    \
    FA[i] = *reinterpret_cast<const bf16x8*>(lds + (BUF) * L8_BUF + i * 4096 + abase + koff[KK]);                     \
    FB[i] = *reinterpret_cast<const bf16x8*>(lds + (BUF) * L8_BUF + i * 4096 + bbase + koff[KK]);                     \
  }
#define L4_MFMA(FA, FB)                                                                                               \
  _Pragma("unroll") for (int i = 0; i < 4; ++i) _Pragma("unroll") for (int j = 0; j < 4; ++j)                          \
      acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(FA[i], FB[j], acc[i][j], 0, 0, 0);
  // NM MFMAs, NR fragment reads behind the first NR, ND load pieces behind the last ones
#define L4_SCHED(ND)                                                                                                  \
  _Pragma("unroll") for (int i = 0; i < NM; ++i) {                                                                    \
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                                                \
    if (i < NR) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                                                    \
    if ((ND) <= NM - NR ? (i >= NR && i - NR < (ND)) : (i >= NM - (ND))) __builtin_amdgcn_sched_group_barrier(0x010, 1, 0); \
  }
#define L4_PIECES(BUF, FIRST, COUNT, KSA, KSB)                                                                        \
  _Pragma("unroll") for (int q = 0; q < NP; ++q) if (q >= (FIRST) && q < (FIRST) + (COUNT)) { L4_DMA(BUF, q, KSA, KSB) }

  // one K tile in buffer BUF (OTH = the other buffer); fragments of its k-step 0 are already in fa0 / fb0
#define L4_TILE(BUF, OTH, t)                                                                                          \
  {                                                                                                                   \
    const int ks1a = ks((t) + 1, 0), ks1b = ks((t) + 1, 1), ks2a = ks((t) + 2, 0), ks2b = ks((t) + 2, 1);             \
    L4_READ(BUF, 1, fa1, fb1) L4_PIECES(OTH, N3, N0, ks1a, ks1b) L4_MFMA(fa0, fb0) L4_SCHED(N0)                        \
    __builtin_amdgcn_sched_barrier(0);                                                                                \
    L4_READ(BUF, 2, fa0, fb0) L4_PIECES(OTH, N3 + N0, N1, ks1a, ks1b) L4_MFMA(fa1, fb1) L4_SCHED(N1)                   \
    __builtin_amdgcn_sched_barrier(0);                                                                                \
    L4_READ(BUF, 3, fa1, fb1) L4_PIECES(OTH, N3 + N0 + N1, N2, ks1a, ks1b) L4_MFMA(fa0, fb0) L4_SCHED(N2)              \
    __builtin_amdgcn_sched_barrier(0);                                                                                \
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                                                       \
    __builtin_amdgcn_s_barrier();                                                                                     \
    __builtin_amdgcn_sched_barrier(0);                                                                                \
    L4_READ(OTH, 0, fa0, fb0) L4_PIECES(BUF, 0, N3, ks2a, ks2b) L4_MFMA(fa1, fb1) L4_SCHED(N3)                         \
    __builtin_amdgcn_sched_barrier(0);                                                                                \
  }

  // ---- prologue: tile 0 complete, then the first pieces of tile 1 ----
  _Pragma("unroll") for (int q = 0; q < NP; ++q) lds_dma16(q < NA ? rsH : rsW, lds + q * 4096 + wave_lds, voff[q], ks(0, q < NA ? 0 : 1));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  L4_READ(0, 0, fa0, fb0)
  L4_PIECES(1, 0, N3, ks(1, 0), ks(1, 1))
  __builtin_amdgcn_sched_barrier(0);

  int t = 0;
  for (; t + 1 < nkt; t += 2) {
    L4_TILE(0, 1, t)
    L4_TILE(1, 0, t + 1)
  }
  if (t < nkt) L4_TILE(0, 1, t)
#undef L4_TILE
#undef L4_PIECES
#undef L4_SCHED
#undef L4_MFMA
#undef L4_READ
#undef L4_DMA
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // tail re-reads still target the LDS about to be reused
  __builtin_amdgcn_s_barrier();

  Epi::tile(p, acc, lds, r0, c0, nt, nlive, wr, wc, tid);
}

// ---- host side: one way to fill the geometry, one way to launch -------------------------------------------------------------------
inline void gemm256_fill(Lm8Params& q, const void* H, const void* W, const Gemm256Geom& g) {
  q.H = H; q.W = W;
  q.R = g.R; q.V = g.V; q.K = g.K; q.MT = g.MT; q.NT = g.NT; q.xcd_order = g.xcd_order; q.gh = g.gh;
  q.bytesH = g.bytesH; q.bytesW = g.bytesW; q.pitchH = g.pitchH; q.pitchW = g.pitchW;
  q.tpd = g.tpd; q.tpd_inv = g.tpd_inv; q.seg_bytes = g.seg_bytes;
}
// operands and geometry of a value-initialised `q`, or the error of the shared checks under the caller's name `fn`; the caller
// then sets the few fields its epilogue policy reads
inline int gemm256_params(Lm8Params& q, const char* fn, const void* H, const void* W, const Gemm256Shape& s, const char* too_big) {
  const Gemm256Plan pl = gemm256_plan(s, too_big);
  if (pl.code != DALM_OK) return ::dalm::fail(pl.code, fn, pl.what);
  gemm256_fill(q, H, W, pl.g);
  return DALM_OK;
}
template <class Epi, bool SPLIT3 = false>
inline int launch_gemm256(const Lm8Params& q, hipStream_t stream, const char* fn) {
  hipLaunchKernelGGL((gemm256_kernel<Epi, SPLIT3>), dim3(static_cast<unsigned>(q.MT) * q.NT), dim3(256), 0, stream, q);
  return check_launch(fn);
}

}  // namespace
}  // namespace dalm
