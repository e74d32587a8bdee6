// Stand-alone host check of dalm_amd/csrc/sim_plan.hpp (built and run by tests/test_abi.py with a plain C++17 compiler under
// -fsanitize=address,undefined; no HIP, no GPU).  Reads "m n D" lines from the file named on the command line and checks every
// workspace layout of every shape: regions in order, disjoint, inside `total` and aligned as their launcher needs; the column
// splits cover the column blocks; padded leading dimensions cover the matrices; 32-bit buffer offsets hold whenever a plan is
// ok.  With `--print` as a second argument it also prints the plan of every shape.
#include <stdio.h>
#include <string.h>
#include <initializer_list>

#include "sim_plan.hpp"

using namespace dalm;

static int failures = 0;
static long long cm, cn, cD;   // the shape under check, for the failure message
#define CHECK(cond) \
  do { if (!(cond)) { fprintf(stderr, "%s:%d: (%lld, %lld, %lld) %s\n", __FILE__, __LINE__, cm, cn, cD, #cond); ++failures; } } while (0)

struct Region { size_t at, bytes, align; };

// `base_align`: what the launcher guarantees for the pointer the offsets count from; `slack`: bytes its align-up may consume
static void check_regions(std::initializer_list<Region> regions, size_t total, size_t base_align, size_t slack = 0) {
  size_t end = 0;
  for (const Region& r : regions) {
    CHECK(r.at >= end);                                     // in order and disjoint
    CHECK(r.at % r.align == 0 && base_align % r.align == 0);
    end = r.at + r.bytes;
  }
  CHECK(end + slack <= total);
}

static void check_stream(const StreamPlan& f, int64_t m, int64_t n, int64_t D) {
  if (!f.ok) return;
  const int64_t cbn = FBN / f.ks, col_blocks = (n + cbn - 1) / cbn;
  CHECK(f.rt == 1 || f.rt == 2);
  CHECK(f.ks == 1 || ((f.ks == 2 || f.ks == 4) && f.rt == 1));
  CHECK(static_cast<int64_t>(f.nsplit) * f.blocks_per_split >= col_blocks && f.nsplit >= 1 && f.nsplit <= 64);
  CHECK(static_cast<int64_t>(f.row_blocks) * 32 * f.rt >= m && f.ldm >= m && f.ldn >= n && f.ldm % 32 == 0 && f.ldn % FBN == 0);
  CHECK(f.ldn >= col_blocks * cbn);                         // the last column block reads inside the padded copy
  CHECK(f.kpad >= D && f.kpad % (16 * f.ks) == 0);
  CHECK(f.kpad * f.ldm * 4 < (1ll << 31) && f.kpad * f.ldn * 4 < (1ll << 31));
}

static void check_shape(int64_t m, int64_t n, int64_t D, bool print) {
  cm = m; cn = n; cD = D;
  {  // row statistics
    const RowstatsLayout L = rowstats_layout(m, n, D);
    check_stream(L.f, m, n, D);
    if (L.f.ok) {
      const size_t a = f32_bytes(L.f.kpad, L.f.ldm), b = f32_bytes(L.f.kpad, L.f.ldn);
      check_regions({{L.at, a, 4}, {L.bt, b, 4}, {L.part, static_cast<size_t>(L.f.nsplit) * m * 8, 8},
                     {L.tickets, f32_bytes(L.f.row_blocks), 4}}, L.total, 8, 8);
    } else if (L.sk > 1) {
      CHECK(L.ldc >= n && L.sk <= 8);
      check_regions({{L.slabs, f32_bytes(L.sk, m, L.ldc), 4}}, L.total, 4);
    } else {
      CHECK(L.parts == rowstats_parts(m, n));
      check_regions({{L.part_m, f32_bytes(L.parts, m), 4}, {L.part_l, f32_bytes(L.parts, m), 4}}, L.total, 4);
    }
    if (print) printf("%lld %lld %lld rowstats: %s rt %d ks %d kpad %lld nsplit %d x %d | sk %d parts %lld (%s tiles) total %zu\n", cm, cn, cD,
                      L.f.ok ? "stream" : L.sk > 1 ? "split-K" : "parts", L.f.rt, L.f.ks, static_cast<long long>(L.f.kpad), L.f.nsplit,
                      L.f.blocks_per_split, L.sk, static_cast<long long>(L.parts), use_big_tiles(m, n) ? "128^2" : "64^2", L.total);
  }
  {  // similarity gradient
    const GradLayout L = grad_layout(m, n, D);
    if (L.f.ok) {
      const int64_t col_blocks = (n + FBN - 1) / FBN;
      CHECK(L.f.nt >= 1 && L.f.nt <= 8 && L.f.nt * 128 == D);
      CHECK(static_cast<int64_t>(L.f.nsplit) * L.f.blocks_per_split >= col_blocks && L.f.nsplit >= 1 && L.f.nsplit <= 64);
      CHECK(L.f.ldm >= m && L.f.ldn >= n && L.f.ldn >= col_blocks * FBN && static_cast<int64_t>(L.f.row_blocks) * FBM >= m);
      CHECK(D * L.f.ldm * 4 < (1ll << 31) && D * L.f.ldn * 4 < (1ll << 31) && n * D * 4 < (1ll << 31));
      check_regions({{L.at, f32_bytes(D, L.f.ldm), 16}, {L.bt, f32_bytes(D, L.f.ldn), 16},
                     {L.slabs, L.f.nsplit > 1 ? f32_bytes(L.f.nsplit, m, D) : 0, 16}}, L.total, 16);
    } else {
      CHECK(L.ldd >= n && L.ldd % 4 == 0);
      check_regions({{L.ds, f32_bytes(m, L.ldd), 16}, {L.part, L.sk > 1 ? f32_bytes(L.sk, m, L.ldd) : 0, 16}}, L.total, 16);
    }
    if (print) printf("%lld %lld %lld grad: %s nt %d nsplit %d x %d | sk %d total %zu\n", cm, cn, cD, L.f.ok ? "flash" : "panel", L.f.nt,
                      L.f.nsplit, L.f.blocks_per_split, L.sk, L.total);
  }
  for (const int64_t k : {1, 7, 100}) {  // gold rank and top-k (the x3 pass's own workspace: absent, and an odd size)
    for (const size_t x3 : {size_t{0}, size_t{1000}}) {
      const TopkLayout L = topk_layout(m, n, D, k, x3);
      const RankLayout R = rank_layout(m, n, D);
      check_stream(L.f, m, n, D);
      CHECK(L.f.ks == 1 && L.at == R.at && L.bt == R.bt && L.gmax == R.total);   // the rank layout is the prefix
      if (!L.f.ok) continue;
      check_regions({{R.at, f32_bytes(R.f.kpad, R.f.ldm), 16}, {R.bt, f32_bytes(R.f.kpad, R.f.ldn), 16}}, R.total, 16);
      check_regions({{L.at, f32_bytes(L.f.kpad, L.f.ldm), 16}, {L.bt, f32_bytes(L.f.kpad, L.f.ldn), 16},
                     {L.gmax, f32_bytes(m, L.f.ldn / 32), 16}, {L.thr, f32_bytes(m), 16}, {L.x3, L.x3_bytes, 16}}, L.total, 16);
      CHECK(L.cap == 8 * k + 64 && L.x3_bytes == x3);
      if (print && k == 7 && x3 == 0) printf("%lld %lld %lld topk / rank: rt %d kpad %lld nsplit %d x %d total %zu / %zu\n", cm, cn, cD, L.f.rt,
                                            static_cast<long long>(L.f.kpad), L.f.nsplit, L.f.blocks_per_split, L.total, R.total);
    }
  }
  if (m > 1024 || n > 8192 || m * n > (1ll << 20)) return;   // the small path's own limits (dalm_sim_small_supported)
  for (const int want_cols : {0, 1}) {  // small forward, two launches and one
    const SmallFwdLayout L = small_fwd_layout(m, n, D, want_cols);
    const SmallPlan& pl = L.pl;
    CHECK(pl.sk >= 1 && pl.sk <= SK_MAX && pl.k_chunk % 32 == 0 && static_cast<int64_t>(pl.sk) * pl.k_chunk >= D);
    CHECK(static_cast<int64_t>(pl.sk - 1) * pl.k_chunk < D && pl.ldn >= n && pl.ldm >= m);
    check_regions({{L.slab, f32_bytes(pl.sk, m, pl.ldn), 4}, {L.slabT, want_cols ? f32_bytes(pl.sk, n, pl.ldm) : 0, 4}}, L.total, 4);
    const Fused1Layout F = fused1_layout(m, n, D, want_cols);
    const size_t tiles = static_cast<size_t>(F.tiles_m) * F.tiles_n;
    CHECK(F.tiles_m * 32 >= m && F.tiles_n * 32 >= n && F.pl.sk == pl.sk);
    check_regions({{F.tslab, pl.sk > 1 ? static_cast<size_t>(pl.sk) * tiles * 4096 : 0, 16}, {F.rowpart, tiles * 32 * 8, 8},
                   {F.colpart, want_cols ? tiles * 32 * 8 : 0, 8}}, F.total, 256, 256);
    if (print && want_cols) {
      const int rounds = (pl.k_chunk % 128 == 0 && static_cast<int64_t>(pl.k_chunk) * pl.sk == D) ? pl.k_chunk / 128 : 0;
      printf("%lld %lld %lld small fwd: sk %d k_chunk %d rounds %d (%s) %s statistics total %zu / %zu\n", cm, cn, cD, pl.sk, pl.k_chunk, rounds,
             rounds == 4 || rounds == 8 ? "pipe" : D % 8 == 0 ? "fast" : "guarded", (m > n ? m : n) > 256 ? "wide" : "narrow", L.total, F.total);
    }
  }
  for (const int dirs : {1, 2, 3}) {  // small backward: dA only, dB only, both
    const bool want_dA = dirs & 1, want_dB = dirs & 2;
    const int64_t R = want_dA ? m : n, Kd = want_dA ? n : m;
    for (const bool tiled : {false, true}) {
      const SmallBwdLayout L = small_bwd_layout(m, n, D, want_dA, want_dB, tiled);
      CHECK(L.nsl >= 1 && (dirs != 3 || L.nsl == 1) && L.nsl <= (Kd + GK - 1) / GK);
      CHECK((L.nsl > 1) == (L.total > 0));
      const size_t bytes = tiled ? static_cast<size_t>(L.nsl) * ((R + 31) / 32) * ((D + 31) / 32) * 4096 : f32_bytes(L.nsl, R, D);
      if (L.nsl > 1) check_regions({{L.slab, bytes, 16}}, L.total, 16);
      if (print && !tiled && dirs != 2)
        printf("%lld %lld %lld small bwd %s: nsl %d %s total %zu\n", cm, cn, cD, dirs == 3 ? "both" : "dA", L.nsl,
               (dirs == 3 ? (m < n ? m : n) : n) > 64 ? "LONG" : "short", L.total);
    }
  }
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: sim_plan_check SHAPES.txt [--print]\n"); return 2; }
  FILE* in = fopen(argv[1], "r");
  if (!in) { perror(argv[1]); return 2; }
  const bool print = argc > 2 && strcmp(argv[2], "--print") == 0;
  long long m, n, D;
  int shapes = 0;
  while (fscanf(in, "%lld %lld %lld", &m, &n, &D) == 3) { check_shape(m, n, D, print); ++shapes; }
  fclose(in);
  if (failures || shapes == 0) return 1;
  printf("sim plans ok: %d shapes\n", shapes);
  return 0;
}
