// Stand-alone host check of dalm_amd/csrc/gemm256_plan.hpp (built and run by tests/test_abi.py with a plain C++17 compiler under
// -fsanitize=address,undefined; no HIP, no GPU).  Nothing is sampled: the tile order over every (row tiles, column tiles, xcd_order)
// listed below in its plain and its live form, the reciprocal of the SPLIT3 tile lookup over its whole domain, the builder's fields
// and guards against expectations restated here as literal formulas, and the bf16x3 workspace layouts over the "m n D" lines of
// the file named on the command line.
#include <stdio.h>
#include <string.h>
#include <initializer_list>
#include <vector>

#include "gemm256_plan.hpp"

using namespace dalm;

static int failures = 0;
static long long c0, c1, c2, c3;   // the case under check, for the failure message
#define CHECK(cond) \
  do { if (!(cond)) { if (++failures < 50) fprintf(stderr, "%s:%d: (%lld, %lld, %lld, %lld) %s\n", __FILE__, __LINE__, c0, c1, c2, c3, #cond); } } while (0)

// blocks [0, nblocks) of lm_tile_order map one-to-one onto the MT x NT tile grid
static void check_bijection(int xcd_order, unsigned gh, unsigned NT, unsigned MT, unsigned nblocks) {
  CHECK(gh >= 1 && gh <= MT && nblocks == MT * NT);
  std::vector<char> seen(static_cast<size_t>(MT) * NT, 0);
  std::vector<unsigned> per_band(MT / gh + 1, 0);
  for (unsigned b = 0; b < nblocks; ++b) {
    int mt = -1, nt = -1;
    lm_tile_order(xcd_order, gh, NT, MT, b, nblocks, mt, nt);
    CHECK(mt >= 0 && nt >= 0 && static_cast<unsigned>(mt) < MT && static_cast<unsigned>(nt) < NT);
    if (mt < 0 || nt < 0 || static_cast<unsigned>(mt) >= MT || static_cast<unsigned>(nt) >= NT) continue;
    CHECK(!seen[static_cast<size_t>(mt) * NT + nt]);
    seen[static_cast<size_t>(mt) * NT + nt] = 1;
    ++per_band[mt / gh];
    // in list order the bands follow each other: every band but the last holds gh row tiles, the last one the remainder
    if (!xcd_order) CHECK(static_cast<unsigned>(mt) / gh == (b / (gh * NT) < MT / gh ? b / (gh * NT) : MT / gh));
  }
  for (unsigned band = 0; band < MT / gh; ++band) CHECK(per_band[band] == gh * NT);
  CHECK(per_band[MT / gh] == (MT % gh) * NT);
}

static void check_tile_order() {
  for (unsigned MT = 1; MT <= 40; ++MT)
    for (const unsigned NT : {1u, 2u, 3u, 4u, 5u, 6u, 7u, 8u, 9u, 31u, 125u})
      for (const int xcd_order : {0, 1}) {
        c0 = MT; c1 = NT; c2 = xcd_order; c3 = -1;
        const unsigned bands = (MT + 7) / 8;                      // restated: bands of <= 8 row tiles, as even as possible
        CHECK(gemm256_band(MT) == (MT + bands - 1) / bands && gemm256_band(MT) <= 8);
        check_bijection(xcd_order, gemm256_band(MT), NT, MT, MT * NT);
        // the live form: the kernel bands the mtl live row tiles (256 rows each) and walks them with the first mtl * NT blocks;
        // block nlb + s skips tile (mtl + s / NT, s % NT)
        for (unsigned want = 0; want <= MT; ++want)
          for (const int nlive : {static_cast<int>(want) * 256, static_cast<int>(want) * 256 - 255}) {
            if (nlive < 0) continue;
            c3 = nlive;
            const unsigned mtl = static_cast<unsigned>((nlive + 255) / 256), nlb = mtl * NT;
            CHECK(mtl == want);
            if (mtl) check_bijection(xcd_order, gemm256_band(mtl), NT, mtl, nlb);
            std::vector<char> dead(static_cast<size_t>(MT - mtl) * NT, 0);
            for (unsigned b = nlb; b < MT * NT; ++b) {
              const unsigned s = b - nlb, mt = mtl + s / NT, nt = s % NT;
              CHECK(mt >= mtl && mt < MT && !dead[static_cast<size_t>(mt - mtl) * NT + nt]);
              if (mt < MT) dead[static_cast<size_t>(mt - mtl) * NT + nt] = 1;
            }
          }
      }
}

static void check_reciprocal() {
  for (int tpd = 1; tpd <= 1024; ++tpd) {
    const unsigned inv = gemm256_tpd_inv(tpd);
    c0 = tpd; c1 = inv; c2 = c3 = -1;
    CHECK(inv == ((1ull << 24) + tpd - 1) / tpd);
    for (unsigned u = 0; u < 6u * tpd; ++u) {
      const unsigned long long wide = static_cast<unsigned long long>(u) * inv;
      const bool reciprocal_holds = wide <= 0xffffffffull && (static_cast<unsigned>(wide) >> 24) == u / tpd;
      if (!reciprocal_holds) { c2 = u; CHECK(reciprocal_holds); break; }
    }
  }
}

static int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
static int band_of(int64_t MT) { const int64_t bands = (MT + 7) / 8; return static_cast<int>((MT + bands - 1) / bands); }

static void expect_ok(const Gemm256Plan& pl) { CHECK(pl.code == DALM_OK && pl.what == nullptr); }
static void expect_fail(const Gemm256Plan& pl, const char* what) {
  CHECK(pl.code == DALM_E_SHAPE && pl.what && strcmp(pl.what, what) == 0);
}

static void check_dense(int64_t R, int64_t V, int64_t K) {
  c0 = R; c1 = V; c2 = K; c3 = 0;
  const Gemm256Plan pl = gemm256_plan(gemm256_dense(R, V, K), "too big");
  expect_ok(pl);
  const Gemm256Geom& g = pl.g;
  CHECK(g.R == R && g.V == V && g.K == K && g.MT == ceil_div(R, 256) && g.NT == ceil_div(V, 256) && g.xcd_order == 1);
  CHECK(g.gh == band_of(g.MT) && g.gh >= 1 && g.gh <= g.MT);
  CHECK(g.bytesH == static_cast<uint64_t>(R) * K * 2 && g.bytesW == static_cast<uint64_t>(V) * K * 2);
  CHECK(g.pitchH == K * 2 && g.pitchW == K * 2 && g.tpd == 0 && g.tpd_inv == 0 && g.seg_bytes == 0);
}

static void check_live(int64_t R, int64_t N, int64_t K, int64_t lda, int64_t w_rows, int cols) {
  c0 = R; c1 = N; c2 = K; c3 = lda;
  const Gemm256Plan pl = gemm256_plan(gemm256_live(R, N, K, lda, w_rows, cols), "too big");
  expect_ok(pl);
  const Gemm256Geom& g = pl.g;
  CHECK(g.R == R && g.V == N && g.K == K && g.MT == ceil_div(R, 256) && g.NT == ceil_div(N, cols) && g.xcd_order == 1 && g.gh == 1);
  CHECK(g.bytesH == static_cast<uint64_t>(R - 1) * lda * 2 + static_cast<uint64_t>(K) * 2);
  CHECK(g.bytesW == static_cast<uint64_t>(w_rows) * K * 2 && g.pitchH == lda * 2 && g.pitchW == K * 2);
  CHECK(g.tpd == 0 && g.tpd_inv == 0 && g.seg_bytes == 0);
}

static bool x3_supported(int64_t m, int64_t n, int64_t D) {      // dalm_sim_rowstats_bf16x3_supported, restated
  return m > 0 && n > 0 && D >= 64 && D % 64 == 0 && D / 64 <= 1024 && static_cast<uint64_t>(m + 256) * 3 * D * 2 < 0xffffff00ull &&
         static_cast<uint64_t>(n + 256) * 3 * D * 2 < 0xffffff00ull;
}
static size_t up256(size_t x) { return (x + 255) / 256 * 256; }

static void check_split3(int64_t R, int64_t V, int64_t D) {
  const Gemm256Plan pl = gemm256_plan(gemm256_split3(R, V, D), "too big");
  expect_ok(pl);
  const Gemm256Geom& g = pl.g;
  CHECK(g.R == R && g.V == V && g.K == 6 * D && g.MT == ceil_div(R, 256) && g.NT == ceil_div(V, 256) && g.xcd_order == 1);
  CHECK(g.gh == band_of(g.MT));
  CHECK(g.bytesH == static_cast<uint64_t>(R) * 3 * D * 2 && g.bytesW == static_cast<uint64_t>(V) * 3 * D * 2);
  CHECK(g.pitchH == 3 * D * 2 && g.pitchW == 3 * D * 2);
  CHECK(g.tpd == D / 64 && g.tpd_inv == ((1u << 24) + g.tpd - 1) / g.tpd && g.seg_bytes == D * 2);
}

struct Region { size_t at, bytes; };
static void check_regions(std::initializer_list<Region> regions, size_t total) {
  size_t end = 256;                                            // the leading slack of the align-up
  for (const Region& r : regions) {
    CHECK(r.at >= end && r.at % 256 == 0);                     // in order, disjoint, aligned
    end = r.at + r.bytes;
  }
  CHECK(end <= total);
}

static void check_shape(int64_t m, int64_t n, int64_t D) {
  c0 = m; c1 = n; c2 = D; c3 = -1;
  check_dense(m, n, (D + 63) / 64 * 64);
  c0 = m; c1 = n; c2 = D; c3 = -1;
  if (!x3_supported(m, n, D)) {
    // what the x3 entry points refuse, the builder refuses: the width of a third, or the span of an image
    CHECK(gemm256_plan(gemm256_split3(m, n, D), "too big").code == DALM_E_SHAPE);
    return;
  }
  check_split3(m, n, D);
  const size_t ia = static_cast<size_t>(m) * 3 * D * 2, ib = static_cast<size_t>(n) * 3 * D * 2;
  {  // group maxima: the two images
    const X3Layout L = x3_images_layout(m, n, D);
    check_regions({{L.a3, ia}, {L.b3, ib}}, L.total);
    CHECK(L.total == 256 + up256(ia) + up256(ib));
  }
  {  // row statistics
    const X3Layout L = x3_layout(m, n, D);
    const int64_t P4 = 4 * ((n + 255) / 256);
    CHECK(L.P4 == P4);
    const size_t part = static_cast<size_t>(P4) * m * 4;
    check_regions({{L.a3, ia}, {L.b3, ib}, {L.labels, static_cast<size_t>(m) * 8}, {L.pm, part}, {L.pl, part},
                   {L.z, static_cast<size_t>(m) * 4}}, L.total);
    CHECK(L.total == 256 + up256(ia) + up256(ib) + up256(static_cast<size_t>(m) * 8) + 2 * up256(part) + up256(static_cast<size_t>(m) * 4));
  }
  {  // backward
    const int64_t blk = x3_grad_block(m);
    CHECK(blk >= 2048 && blk <= 8192 && blk % 256 == 0);
    const X3GradLayout L = x3_grad_layout(m, n, D);
    const int64_t ncp = n < blk ? (n + 255) / 256 * 256 : blk;
    CHECK(L.ncp == ncp);
    const size_t ds = static_cast<size_t>(m) * 3 * ncp * 2, bt = static_cast<size_t>(D) * 3 * ncp * 2;
    check_regions({{L.a3, ia}, {L.b3, ib}, {L.ds3, ds}, {L.bt3, bt}}, L.total);
    CHECK(L.total == 256 + up256(ia) + up256(ib) + up256(ds) + up256(bt));
    // the two contractions of a block, where dalm_sim_grad_bf16x3_supported (restated) admits the shape
    if (static_cast<uint64_t>(m + 256) * 3 * ncp * 2 < 0xffffff00ull && static_cast<uint64_t>(D + 256) * 3 * ncp * 2 < 0xffffff00ull) {
      check_split3(m, n < ncp ? n : ncp, D);
      check_split3(m, D, ncp);
    }
  }
}

static void check_guards() {
  c0 = c1 = c2 = c3 = -2;
  // 0xffffff00 = 33554430 * 128: with K = 64 (128 bytes a row) the span (rows + 256) * 128 reaches it at rows + 256 = 33554430
  const int64_t last = 33554429 - 256;
  expect_ok(gemm256_plan(gemm256_dense(last, 1, 64), "too big"));
  expect_fail(gemm256_plan(gemm256_dense(last + 1, 1, 64), "too big"), "too big");
  expect_ok(gemm256_plan(gemm256_dense(1, last, 64), "too big"));
  expect_fail(gemm256_plan(gemm256_dense(1, last + 1, 64), "too big"), "too big");
  // the live entries: the span of A counts lda, the span of W its w_rows (2 C for the gate | up weight)
  expect_ok(gemm256_plan(gemm256_live(33554430 / 2 - 1 - 256, 8, 64, 128, 8, 256), "too big"));
  expect_fail(gemm256_plan(gemm256_live(33554430 / 2 - 256, 8, 64, 128, 8, 256), "too big"), "too big");
  expect_ok(gemm256_plan(gemm256_live(1, (last - 1) / 2, 64, 64, last - 1, 128), "too big"));
  expect_fail(gemm256_plan(gemm256_live(1, (last + 1) / 2, 64, 64, last + 1, 128), "too big"), "too big");
  // tiles: 46340 * 46341 = 2147441940 <= 0x7fffffff < 2147488281 = 46341 * 46341 (the spans stay far below 4 GB)
  expect_ok(gemm256_plan(gemm256_dense(46340 * 256, 46341 * 256, 64), "too big"));
  expect_fail(gemm256_plan(gemm256_dense(46341 * 256, 46341 * 256, 64), "too big"), "too many tiles for one launch");
  expect_ok(gemm256_plan(gemm256_live(46340 * 256, 46341 * 128, 64, 64, 2 * 46341 * 128, 128), "too big"));
  expect_fail(gemm256_plan(gemm256_live(46340 * 256 + 1, 46341 * 128, 64, 64, 2 * 46341 * 128, 128), "too big"),
              "too many tiles for one launch");
  // the contraction width
  expect_fail(gemm256_plan(gemm256_dense(8, 8, 96), "too big"), "the contraction width must be a positive multiple of 64");
  expect_fail(gemm256_plan(gemm256_dense(8, 8, 0), "too big"), "the contraction width must be a positive multiple of 64");
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: gemm256_plan_check SHAPES.txt\n"); return 2; }
  FILE* in = fopen(argv[1], "r");
  if (!in) { perror(argv[1]); return 2; }
  check_tile_order();
  check_reciprocal();
  check_guards();
  // lm_head and live-row shapes: one row, the 256 / 257 tile edge, strided rows, the narrowest output, the padded step's own
  check_dense(1, 1, 64); check_dense(256, 32000, 4096); check_dense(257, 50257, 768); check_dense(3584, 32000, 4096);
  check_dense(3584, 4096, 32000);
  check_live(1, 8, 64, 64, 8, 256); check_live(256, 264, 64, 72, 264, 256); check_live(257, 8, 128, 136, 8, 256);
  check_live(257, 264, 64, 64, 264, 256); check_live(2897, 5504, 2048, 2048, 11008, 128);
  check_live(300, 2048, 5504, 5512, 2048, 256);
  long long m, n, D;
  int shapes = 0;
  while (fscanf(in, "%lld %lld %lld", &m, &n, &D) == 3) { check_shape(m, n, D); ++shapes; }
  fclose(in);
  if (failures || shapes == 0) return 1;
  printf("gemm256 plans ok: %d shapes\n", shapes);
  return 0;
}
