// Plans and workspace layouts of the similarity launchers (sim.hip, sim_small.hip): which kernel form a shape takes, how its
// grid is cut, and where every region of its workspace lies.  One layout function per workspace yields the offsets AND the
// total, so a `*_workspace_bytes` function returns `.total` and the launcher carves from the same struct: a stated size
// and a carve cannot disagree.  Host-only, plain C++17 (no HIP); tests/sim_plan_check.cpp checks every layout on the host.
#pragma once
#include <stddef.h>
#include "dispatch.hpp"

namespace dalm {

constexpr int FBM = 32, FBN = 128;   // flash / streaming kernels: rows per row tile, columns per column block
constexpr int BK_SMALL = 128;        // 64x64 GEMM tiles of latency-bound small problems: 4x fewer barrier rounds
constexpr int GK = 256;              // small backward: contraction chunk
constexpr int SK_MAX = 16;           // small forward: most K slices a tile is split into

// Hands out consecutive regions of a workspace: every region starts where the last one ended, sizes rounded up to `q` bytes.
struct Carve {
  size_t o = 0;
  size_t take(size_t bytes, size_t q = 16) { const size_t at = o; o += (bytes + q - 1) / q * q; return at; }
};

// An entry point that accepts a workspace aligned to fewer bytes than a region needs aligns the pointer up itself; the layout
// keeps `q` bytes of slack in its total.
inline char* align_up(void* p, uintptr_t q) { return reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(p) + q - 1) / q * q); }

// the region at byte offset `off` of a workspace
template <typename T = float>
inline T* region(void* ws, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(ws) + off); }

// ---- plans ------------------------------------------------------------------------------------------------------------
struct FlashPlan { bool ok; int nt, row_blocks, nsplit, blocks_per_split; int64_t ldm, ldn; };
inline FlashPlan flash_plan(int64_t m, int64_t n, int64_t D) {
  FlashPlan f{false, 0, 0, 1, 0, 0, 0};
  if (D > 1024 || D % 128 != 0) return f;        // accumulators hold 32 x D per workgroup, D = 128 * NT
  if ((n + 128) * D * 4 >= (1ll << 31) || (m + 32) * D * 4 >= (1ll << 31)) return f;   // 32-bit buffer offsets
  f.nt = static_cast<int>(D / 128);
  f.row_blocks = static_cast<int>((m + FBM - 1) / FBM);
  const int64_t col_blocks = (n + FBN - 1) / FBN;
  // Column split: cost model fitted to MI355X timings (us).  One workgroup alone on a CU retires a 128-column
  // block in ~38 us (+ ~5 us of fill/drain), two co-resident ones a pair of blocks in ~66 us (+ ~15 us): two per CU
  // wins in steady state (4096^2: 4 splits), one per CU wins when a workgroup only has a block or two
  // (1200^2: 5 splits -> 190 workgroups instead of 10 -> 380 on 256 CUs).  Partial-output traffic is charged at 4 TB/s.
  double best = 1e30;
  int64_t best_ns = 1;
  for (int64_t ns = 1; ns <= col_blocks && ns <= 64; ++ns) {
    const int64_t bps = (col_blocks + ns - 1) / ns;
    const int64_t real_ns = (col_blocks + bps - 1) / bps;
    if (real_ns != ns) continue;
    const int64_t W = static_cast<int64_t>(f.row_blocks) * ns;
    double t;
    if (W <= 256) t = 5.0 + 38.0 * bps;
    else t = 15.0 + 66.0 * bps * ((W + 511) / 512);
    if (ns > 1) t += static_cast<double>(ns) * m * D * 8.0 / 4.0e6;
    if (t < best) { best = t; best_ns = ns; }
  }
  f.blocks_per_split = static_cast<int>((col_blocks + best_ns - 1) / best_ns);
  f.nsplit = static_cast<int>(best_ns);
  f.ldm = static_cast<int64_t>(f.row_blocks) * FBM;
  f.ldn = col_blocks * FBN;
  f.ok = true;
  return f;
}

// Streaming row statistics: used once the problem is MFMA-sized (the small-batch path and the latency-bound
// split-K form cover everything below); any D (the k-major copies are zero-padded to a multiple of 16).
struct StreamPlan { bool ok; int rt, row_blocks, nsplit, blocks_per_split; int64_t ldm, ldn, kpad; int ks; };
inline StreamPlan stream_plan(int64_t m, int64_t n, int64_t D, bool always = false) {
  StreamPlan f{false, 1, 0, 1, 0, 0, 0, 0, 1};
  if (!always && (m * n < 512 * 512 || D < 64)) return f;
  f.rt = (m >= 4096) ? 2 : 1;   // measured: 2048^2 86 vs 77 TF, 4096^2 100 vs 107, 16384^2 118 vs 141
  const int64_t bm = 32 * f.rt;
  f.row_blocks = static_cast<int>((m + bm - 1) / bm);
  // K slices per column tile, for the sizes whose 128-column blocks give the chip only one or two workgroups per CU
  // (grid = row blocks x column blocks; measured, whole call, us: 768^2 (144) 36.0 / 37.7 / 37.5 for 1 / 2 / 4 slices,
  // 1200^2 (380) 57.2 / 54.0 / 56.2, 1536^2 (576) 74.3 / 76.4 / 68.1, 2048^2 (1024) 90.8 / 103.6 / 108.2).  What did NOT
  // move these sizes (profiles/history/r03_sim_midsize_experiments.txt): 16-byte operand loads from 4-k granule copies (slower),
  // capping workgroups per CU through LDS padding (slower), XCD rectangles + an L2 warm-up pass (no change).
  if (!always && f.rt == 1) {
    const int64_t g128 = static_cast<int64_t>(f.row_blocks) * ((n + 127) / 128);
    f.ks = (g128 >= 450 && g128 < 640) ? 4 : (g128 >= 300 && g128 < 450) ? 2 : 1;
  }
  f.kpad = (D + 16 * f.ks - 1) / (16 * f.ks) * (16 * f.ks);
  if ((n + 128) * f.kpad * 4 >= (1ll << 31) || (m + 64) * f.kpad * 4 >= (1ll << 31)) return f;   // 32-bit buffer offsets
  const int64_t col_blocks = (n + FBN / f.ks - 1) / (FBN / f.ks);
  int64_t ns = ((f.rt == 2 ? 512 : 768) + f.row_blocks - 1) / f.row_blocks;      // 2-3 workgroups per CU (by registers)
  if (ns > col_blocks) ns = col_blocks;
  if (ns < 1) ns = 1;
  if (ns > 64) ns = 64;
  f.blocks_per_split = static_cast<int>((col_blocks + ns - 1) / ns);
  f.nsplit = static_cast<int>((col_blocks + f.blocks_per_split - 1) / f.blocks_per_split);
  f.ldm = static_cast<int64_t>(f.row_blocks) * bm;
  f.ldn = (n + FBN - 1) / FBN * FBN;
  f.ok = true;
  return f;
}

// 128x128 tiles once the grid fills the chip, 64x64 below that.
inline bool use_big_tiles(int64_t M, int64_t N) {
  return ((M + 127) / 128) * ((N + 127) / 128) >= 128;
}
inline int64_t rowstats_parts(int64_t m, int64_t n) {
  const int64_t bn = use_big_tiles(m, n) ? 128 : 64;
  return 2 * ((n + bn - 1) / bn);
}

// Split-K for S = A.B^T problems that cannot fill 256 CUs with 64x64 tiles (the real batch sizes: 18 ... ~1200
// rows): SK partial slabs + a one-block-per-row epilogue.  Returns 1 when the direct kernels are used.
inline int sim_splitk(int64_t m, int64_t n, int64_t D) {
  if (use_big_tiles(m, n)) return 1;
  const int64_t tiles = ((m + 63) / 64) * ((n + 63) / 64);
  if (tiles > 512 || D < 256 || n > 8192) return 1;
  int sk = 1;
  while (sk < 8 && tiles * sk * 2 <= 1024 && D / (sk * 2) >= BK_SMALL) sk *= 2;
  return sk;
}

struct SmallPlan { int sk, k_chunk; int64_t ldn, ldm; };
inline SmallPlan small_plan(int64_t m, int64_t n, int64_t D) {
  const int64_t tiles = ((m + 31) / 32) * ((n + 31) / 32);
  constexpr int64_t target = 256;               // workgroups aimed at
  int64_t sk = (target + tiles - 1) / tiles;
  const int64_t sk_max = (D + 31) / 32;        // every workgroup gets at least 32 of K (8 per wave)
  if (sk > SK_MAX) sk = SK_MAX;
  if (sk > sk_max) sk = sk_max;
  if (sk < 1) sk = 1;
  const int64_t k_chunk = round_up((D + sk - 1) / sk, 32);
  sk = (D + k_chunk - 1) / k_chunk;
  return {static_cast<int>(sk), static_cast<int>(k_chunk), round_up(n, 4), round_up(m, 4)};
}

// contraction slices of the small backward: as many as keep the grid at <= 1024 workgroups, at most one per 256-chunk; only
// when ONE direction is asked for (the sharded form; with both directions the grid is already two problems wide)
inline int small_bwd_slices(int64_t m, int64_t n, int64_t D, bool want_dA, bool want_dB) {
  if (want_dA == want_dB) return 1;
  const int64_t R = want_dA ? m : n, Kd = want_dA ? n : m;
  const int64_t blocks = ((R + 31) / 32) * ((D + 31) / 32), chunks = (Kd + GK - 1) / GK;
  int64_t nsl = blocks > 0 ? 1024 / blocks : 1;
  if (nsl > chunks) nsl = chunks;
  return static_cast<int>(nsl < 1 ? 1 : nsl);
}

// ---- workspace layouts: byte offsets from the (aligned) workspace pointer, and the total ------------------------------------
inline size_t f32_bytes(int64_t a, int64_t b = 1, int64_t c = 1) {
  return static_cast<size_t>(a) * static_cast<size_t>(b) * static_cast<size_t>(c) * sizeof(float);
}

// dalm_sim_rowstats_f32.  Stream form (f.ok): k-major copies | (max, sum) granules [nsplit][m], 8 bytes each | tickets
// [row_blocks]; the caller's pointer is 4-byte aligned, the launcher aligns it up to 8.  Split-K form (sk > 1): `sk` slabs
// [m][ldc] of raw partial products.  Parts form: (max, sum) partials [parts][m] each.
struct RowstatsLayout { StreamPlan f; int sk; int64_t parts, ldc; size_t at, bt, part, tickets, slabs, part_m, part_l, total; };
inline RowstatsLayout rowstats_layout(int64_t m, int64_t n, int64_t D) {
  RowstatsLayout L{};
  L.f = stream_plan(m, n, D);
  L.sk = L.f.ok ? 1 : sim_splitk(m, n, D);
  Carve c;
  if (L.f.ok) {
    L.at = c.take(f32_bytes(L.f.kpad, L.f.ldm), 8);
    L.bt = c.take(f32_bytes(L.f.kpad, L.f.ldn), 8);
    L.part = c.take(static_cast<size_t>(L.f.nsplit) * m * 8, 8);
    L.tickets = c.take(f32_bytes(L.f.row_blocks), 4);
    c.take(8, 4);                 // slack of the align-up
  } else if (L.sk > 1) {
    L.ldc = round_up(n, 4);
    L.slabs = c.take(f32_bytes(L.sk, m, L.ldc), 4);
  } else {
    L.parts = rowstats_parts(m, n);
    L.part_m = c.take(f32_bytes(L.parts, m), 4);
    L.part_l = c.take(f32_bytes(L.parts, m), 4);
  }
  L.total = c.o;
  return L;
}

// dalm_sim_grad (16-byte aligned).  Flash form (f.ok): k-major copies | per-split partial outputs [nsplit][m][D] when
// nsplit > 1.  Panel form: dS panel [m][ldd] | `sk` split-K slabs [m][ldd] when sk > 1.
struct GradLayout { FlashPlan f; int sk; int64_t ldd; size_t at, bt, slabs, ds, part, total; };
inline GradLayout grad_layout(int64_t m, int64_t n, int64_t D) {
  GradLayout L{};
  L.f = flash_plan(m, n, D);
  L.sk = L.f.ok ? 1 : sim_splitk(m, n, D);
  Carve c;
  if (L.f.ok) {
    L.at = c.take(f32_bytes(D, L.f.ldm));
    L.bt = c.take(f32_bytes(D, L.f.ldn));
    L.slabs = c.take(L.f.nsplit > 1 ? f32_bytes(L.f.nsplit, m, D) : 0, 4);
  } else {
    L.ldd = round_up(n, 4);
    L.ds = c.take(f32_bytes(m, L.ldd));
    L.part = c.take(L.sk > 1 ? f32_bytes(L.sk, m, L.ldd) : 0);
  }
  L.total = c.o;
  return L;
}

// dalm_sim_gold_rank (16-byte aligned): the k-major copies.  dalm_sim_topk continues the same carve: group maxima [m][ldn / 32] |
// thresholds [m] | the bf16x3 first pass's own workspace (`x3_bytes`, 0 where that pass cannot be taken).
struct RankLayout { StreamPlan f; size_t at, bt, total; };
inline RankLayout rank_layout(int64_t m, int64_t n, int64_t D) {
  RankLayout L{};
  L.f = stream_plan(m, n, D, true);
  Carve c;
  L.at = c.take(f32_bytes(L.f.kpad, L.f.ldm));
  L.bt = c.take(f32_bytes(L.f.kpad, L.f.ldn));
  L.total = c.o;
  return L;
}
struct TopkLayout : RankLayout { int cap; size_t gmax, thr, x3, x3_bytes; };
inline TopkLayout topk_layout(int64_t m, int64_t n, int64_t D, int64_t k, size_t x3_bytes) {
  TopkLayout L{};
  static_cast<RankLayout&>(L) = rank_layout(m, n, D);
  L.cap = static_cast<int>(8 * k + 64);
  Carve c{L.total};
  L.gmax = c.take(f32_bytes(m, L.f.ldn / 32));
  L.thr = c.take(f32_bytes(m));
  L.x3_bytes = x3_bytes;
  L.x3 = c.take(x3_bytes);
  L.total = c.o;
  return L;
}

// dalm_sim_small_fwd (4-byte aligned): partial slabs [sk][m][ldn] | transposed slabs [sk][n][ldm] when column statistics are wanted
struct SmallFwdLayout { SmallPlan pl; size_t slab, slabT, total; };
inline SmallFwdLayout small_fwd_layout(int64_t m, int64_t n, int64_t D, int want_cols) {
  SmallFwdLayout L{};
  L.pl = small_plan(m, n, D);
  Carve c;
  L.slab = c.take(f32_bytes(L.pl.sk, m, L.pl.ldn), 4);
  L.slabT = c.take(want_cols ? f32_bytes(L.pl.sk, n, L.pl.ldm) : 0, 4);
  L.total = c.o;
  return L;
}

// dalm_sim_small_fwd1 (any alignment: the launcher aligns the pointer up to 256): partial tiles [sk][tiles][1024] when sk > 1 |
// row granules [tiles_n][tiles_m * 32] | column granules [tiles_m][tiles_n * 32] when wanted
struct Fused1Layout { SmallPlan pl; int tiles_m, tiles_n; size_t tslab, rowpart, colpart, total; };
inline Fused1Layout fused1_layout(int64_t m, int64_t n, int64_t D, int want_cols) {
  Fused1Layout L{};
  L.pl = small_plan(m, n, D);
  L.tiles_m = static_cast<int>((m + 31) / 32); L.tiles_n = static_cast<int>((n + 31) / 32);
  const size_t tiles = static_cast<size_t>(L.tiles_m) * L.tiles_n;
  Carve c;
  L.tslab = c.take(L.pl.sk > 1 ? static_cast<size_t>(L.pl.sk) * tiles * 4096 : 0);
  L.rowpart = c.take(tiles * 32 * 8);
  L.colpart = c.take(want_cols ? tiles * 32 * 8 : 0);
  c.take(256);                    // slack of the align-up
  L.total = c.o;
  return L;
}

// dalm_sim_small_bwd_ws / _bwd1 (16-byte aligned; total 0 = unsliced, no workspace): `nsl` contraction slices of the one
// output asked for, row-major [nsl][R][D] (two-launch form) or tile-major [nsl][tiles][1024] (one-launch form, `tiled`)
struct SmallBwdLayout { int nsl; size_t slab, total; };
inline SmallBwdLayout small_bwd_layout(int64_t m, int64_t n, int64_t D, bool want_dA, bool want_dB, bool tiled) {
  SmallBwdLayout L{};
  L.nsl = small_bwd_slices(m, n, D, want_dA, want_dB);
  const int64_t R = want_dA ? m : n;
  Carve c;
  if (L.nsl > 1) L.slab = c.take(tiled ? static_cast<size_t>(L.nsl) * ((R + 31) / 32) * ((D + 31) / 32) * 4096 : f32_bytes(L.nsl, R, D), 4);
  L.total = c.o;
  return L;
}

}  // namespace dalm
