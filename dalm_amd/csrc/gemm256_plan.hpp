// Launch geometry of the 256 x 256 MFMA GEMM core (gemm256.hpp): the tile order, the band rule, the integer kernel arguments every
// launcher needs and the checks that guard them, and the workspace layouts of the bf16x3 similarity launchers (sim_x3.hip).
// Host-only, plain C++17 (no HIP); the tile-order arithmetic is shared with the kernel through DALM_HD, which is empty under a host
// compiler.  tests/gemm256_plan_check.cpp checks all of it on the host.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "sim_plan.hpp"

#ifdef __HIPCC__
#define DALM_HD __host__ __device__ __forceinline__
#else
#define DALM_HD inline
#endif

namespace dalm {

// Tile order.  The ordered tile list walks the output in bands of gh row tiles - within a band vocabulary tile by vocabulary
// tile, the band's row tiles innermost - and every XCD (workgroup L runs on XCD L % 8, own 4 MB L2) works through ONE
// contiguous run of that list.  The 32 tiles an XCD has in flight are then ~gh row panels x 32/gh vocabulary panels
// (7 + 4.6 instead of 14 + 2.3 panels of 2 MB at 14 row tiles): every panel a CU pulls into the L2 is shared by 4-7 neighbours.
DALM_HD void lm_tile_order(int xcd_order, unsigned gh, unsigned NT, unsigned MT, unsigned block, unsigned nblocks, int& mt, int& nt) {
  unsigned g = block;
  if (xcd_order) {
    const unsigned q8 = nblocks >> 3, r8 = nblocks & 7u, xcd = block & 7u;
    g = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (block >> 3);
  }
  const unsigned nfull = MT / gh, full = nfull * gh * NT;
  if (g < full) {
    const unsigned mg = g / (gh * NT), r = g % (gh * NT);
    nt = static_cast<int>(r / gh);
    mt = static_cast<int>(mg * gh + r % gh);
  } else {
    const unsigned rem = MT - nfull * gh, r = g - full;
    nt = static_cast<int>(r / rem);
    mt = static_cast<int>(nfull * gh + r % rem);
  }
}

// The band rule: row tiles per band for MT >= 1 row tiles - bands of <= 8 row tiles, as even as possible.  The launchers call it
// with the row-tile count of the shape, the kernel's live path with the live row-tile count (a device value).
DALM_HD unsigned gemm256_band(unsigned MT) {
  const unsigned bands = (MT + 7) / 8;
  return (MT + bands - 1) / bands;
}

// SPLIT3: K tile u of the six-segment contraction lies in segment u / tpd; the kernel divides by multiplying with
// tpd_inv = ceil(2^24 / tpd): u / tpd == (u * tpd_inv) >> 24 for u < 6 tpd and tpd <= 1024, inside 32 bits (the host check walks
// every such pair).
inline unsigned gemm256_tpd_inv(int tpd) { return ((1u << 24) + static_cast<unsigned>(tpd) - 1) / static_cast<unsigned>(tpd); }

// ---- the integer kernel arguments of one launch ---------------------------------------------------------------------------
struct Gemm256Geom {
  int R, V, K, MT, NT, xcd_order, gh;
  unsigned bytesH, bytesW, pitchH, pitchW;
  int tpd;
  unsigned tpd_inv, seg_bytes;
};

// C [R, V] = H [R, K] . W [w_rows, K]^T, both operands bf16 and K-contiguous
struct Gemm256Shape {
  int64_t R, V, K;
  int64_t ldh, ldw;        // elements between rows of H / W
  int64_t w_rows;          // rows of W: V, or 2 V where a column tile gathers gate and up rows
  int64_t D;               // SPLIT3: width of one third (K = 6 D over rows of 3 D); 0 otherwise
  int tile_cols;           // output columns per column tile: 256, or 128 for the gate | up tiles (a row tile is 256 rows)
  bool live;               // rows go through the partition: the kernel bands the LIVE row tiles itself
};
inline Gemm256Shape gemm256_dense(int64_t R, int64_t V, int64_t K) { return {R, V, K, K, K, V, 0, 256, false}; }
inline Gemm256Shape gemm256_split3(int64_t R, int64_t V, int64_t D) { return {R, V, 6 * D, 3 * D, 3 * D, V, D, 256, false}; }
inline Gemm256Shape gemm256_live(int64_t R, int64_t N, int64_t K, int64_t lda, int64_t w_rows, int tile_cols) {
  return {R, N, K, lda, K, w_rows, 0, tile_cols, true};
}

struct Gemm256Plan { int code; const char* what; Gemm256Geom g; };

// The checks every launcher shares, in the order the launchers always made them, and the geometry.  `too_big` is the caller's own
// text for operands above 4 GB (the lm_head entries say "use smaller chunks", the live-row ones "use fewer rows per call").  The
// caller has bounded R, V, w_rows and the strides below 2^31, so the products below stay inside 64 bits.
inline Gemm256Plan gemm256_plan(const Gemm256Shape& s, const char* too_big) {
  Gemm256Plan pl{DALM_OK, nullptr, {}};
  auto fail = [&](int code, const char* what) { pl.code = code; pl.what = what; return pl; };
  // every launcher states this in its own argument check first (the bf16x3 ones through their *_supported functions, which also
  // keep D / 64 inside the reciprocal's domain); kept here so that the builder alone is safe to call
  if (s.K <= 0 || s.K % 64 != 0 || s.D % 64 != 0 || s.D / 64 > 1024)
    return fail(DALM_E_SHAPE, "the contraction width must be a positive multiple of 64");
  // 32-bit buffer offsets: a tile past the last row still forms offsets of up to 256 rows beyond it
  const uint64_t spanH = static_cast<uint64_t>(s.R + 256) * s.ldh * 2, spanW = static_cast<uint64_t>(s.w_rows + 256) * s.ldw * 2;
  if (spanH >= 0xffffff00ull || spanW >= 0xffffff00ull) return fail(DALM_E_SHAPE, too_big);
  Gemm256Geom& g = pl.g;
  g.R = static_cast<int>(s.R); g.V = static_cast<int>(s.V); g.K = static_cast<int>(s.K);
  g.MT = static_cast<int>((s.R + 255) / 256);
  g.NT = static_cast<int>((s.V + s.tile_cols - 1) / s.tile_cols);
  g.xcd_order = 1;
  g.gh = s.live ? 1 : static_cast<int>(gemm256_band(static_cast<unsigned>(g.MT)));
  // the descriptor of H ends with its last row: (R - 1) ldh + width elements.  Written this way for the live entries, whose rows
  // may be strided (ldh > K); for the dense and bf16x3 operands it is R ldh, what their launchers always passed
  const int64_t width = s.D ? 3 * s.D : s.K;
  g.bytesH = static_cast<unsigned>((static_cast<uint64_t>(s.R - 1) * s.ldh + width) * 2);
  g.bytesW = static_cast<unsigned>(static_cast<uint64_t>(s.w_rows) * s.ldw * 2);
  g.pitchH = static_cast<unsigned>(s.ldh * 2); g.pitchW = static_cast<unsigned>(s.ldw * 2);
  if (s.D) {
    g.tpd = static_cast<int>(s.D / 64);
    g.tpd_inv = gemm256_tpd_inv(g.tpd);
    g.seg_bytes = static_cast<unsigned>(s.D * 2);
  }
  if (static_cast<int64_t>(g.MT) * g.NT > 0x7fffffffll) return fail(DALM_E_SHAPE, "too many tiles for one launch");
  return pl;
}

// ---- workspace layouts of the bf16x3 launchers: byte offsets from (the caller's pointer aligned up to 256) - 256 ------------------
// Every layout opens with 256 bytes of slack for that align-up, so offsets start at 256 and base + offset is 256-byte aligned and
// inside the caller's buffer.
inline size_t x3_image_bytes(int64_t rows, int64_t D) { return static_cast<size_t>(rows) * 3 * D * 2; }

// dalm_x3_group_max: the thirds images of A [m][3 D] and B [n][3 D].  dalm_sim_rowstats_bf16x3 continues the same carve: labels [m]
// int64 | (max, sum) partials [P4][m] each | the label's logit [m]
struct X3Layout { size_t a3, b3, labels, pm, pl, z, total; int64_t P4; };
inline X3Layout x3_images_layout(int64_t m, int64_t n, int64_t D) {
  X3Layout L{};
  Carve c;
  c.take(256, 256);
  L.a3 = c.take(x3_image_bytes(m, D), 256);
  L.b3 = c.take(x3_image_bytes(n, D), 256);
  L.total = c.o;
  return L;
}
inline X3Layout x3_layout(int64_t m, int64_t n, int64_t D) {
  X3Layout L = x3_images_layout(m, n, D);
  Carve c{L.total};
  L.P4 = 4 * ((n + 255) / 256);
  L.labels = c.take(static_cast<size_t>(m) * 8, 256);
  L.pm = c.take(f32_bytes(L.P4, m), 256);
  L.pl = c.take(f32_bytes(L.P4, m), 256);
  L.z = c.take(f32_bytes(m), 256);
  L.total = c.o;
  return L;
}

// Columns of S per block (a multiple of 256); the dS image is m x 3 x block x 2 bytes.  Larger blocks = fewer, fuller launches
// (16384^2, profiles/r05_sim_grad_x3.txt: block 2048 163 TF f32-equivalent, 4096 179, 8192 188): as large as a 1 GiB dS image
// allows, between 2048 and 8192.
inline int64_t x3_grad_block(int64_t m) {
  int64_t b = (int64_t(1) << 30) / (6 * (m > 0 ? m : 1));
  if (b > 8192) b = 8192;
  if (b < 2048) b = 2048;
  return b / 256 * 256;
}
// dalm_sim_grad_bf16x3: the two images | dS thirds [m][3 ncp] | transposed thirds of a block of B [D][3 ncp]
struct X3GradLayout { size_t a3, b3, ds3, bt3, total; int64_t ncp; };
inline X3GradLayout x3_grad_layout(int64_t m, int64_t n, int64_t D) {
  X3GradLayout L{};
  const int64_t blk = x3_grad_block(m);
  L.ncp = n < blk ? round_up(n, 256) : blk;
  const X3Layout I = x3_images_layout(m, n, D);
  L.a3 = I.a3; L.b3 = I.b3;
  Carve c{I.total};
  L.ds3 = c.take(x3_image_bytes(m, L.ncp), 256);
  L.bt3 = c.take(x3_image_bytes(D, L.ncp), 256);
  L.total = c.o;
  return L;
}

}  // namespace dalm
