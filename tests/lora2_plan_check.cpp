// Stand-alone host check of dalm_amd/csrc/lora2_plan.hpp (built and run by tests/test_abi.py with a plain C++17 compiler under
// -fsanitize=address,undefined; no HIP, no GPU).  Reads "R C" lines from the file named on the command line (the grid of
// tests/test_lora2_sizes.py) and checks the invariants of every plan - rankupd with and without masks in modes 1 to 3, colacc at
// ranks 8 and 16 in modes 1 to 3 - at every shape of the file AND at every row count from 1 to the file's largest for each of its
// column counts, so that both sides of every threshold are walked.  Then the plans of the benchmark's shape and of the shapes
// tests/test_lora2_forms_gpu.py names are compared with literally restated expectations.  With `--print` as a second argument it
// prints the plan of each named shape.
#include <stdio.h>
#include <string.h>
#include <set>

#include "lora2_plan.hpp"

using namespace dalm;

static int failures = 0;
static long long cR, cC;
static int crank, cmode;   // the case under check, for the failure message
#define CHECK(cond) \
  do { if (!(cond)) { if (++failures < 50) fprintf(stderr, "%s:%d: (R %lld, C %lld, rank %d, mode %d) %s\n", __FILE__, __LINE__, cR, cC, \
                                                  crank, cmode, #cond); } } while (0)

static void check_rankupd(int64_t R, int64_t C, int mode) {
  cR = R; cC = C; crank = 0; cmode = mode;
  for (const bool bits : {false, true}) {
    const RankupdPlan p = rankupd_plan(R, C, mode, bits);
    const int64_t rows = p.rows_per_wg, S = (R + rows - 1) / rows;
    CHECK(rows > 0 && rows % 4 == 0 && rows <= 256);
    CHECK((S - 1) * rows < R && R <= S * rows);
    CHECK(p.ok == (S <= 65535) && (!p.ok || p.S == S));
    CHECK(p.nt == (mode == 2 ? 2 : 1) && p.nprob == (mode == 3 ? 2 : 1) && p.slabs == (C + 511) / 512);
    CHECK(p.stage == (bits && C % 128 == 0));
    CHECK(p.lds == (p.stage ? static_cast<size_t>(p.nt) * rows * 64 : 0) && p.lds <= 65536);
    const int64_t budget = (mode == 2 ? 512 : 768) / (static_cast<int64_t>(p.slabs) * p.nprob);
    if (p.arm == Lora2Arm::max_s) CHECK(rows == 4 && budget > (R + 3) / 4);
    if (p.arm == Lora2Arm::min_s) CHECK(R > 256 * budget && S == (R + 255) / 256 && (S < 2 || rows > 128));
    if (p.arm == Lora2Arm::budget) CHECK(budget >= 1 && S <= budget && R <= 256 * budget);
    CHECK(p.arm != Lora2Arm::cap);
  }
}

static void check_colacc(int64_t R, int64_t C, int rank, int mode) {
  cR = R; cC = C; crank = rank; cmode = mode;
  const ColaccPlan g = colacc_plan(R, C, rank, mode);
  const int64_t rows = g.rows_per_split, S = (R + rows - 1) / rows, nt = mode == 2 ? 2 : 1, nprob = mode == 3 ? 2 : 1;
  CHECK(rows > 0 && rows % 32 == 0);
  CHECK((S - 1) * rows < R && R <= S * rows);
  CHECK(g.ok == (S <= 65535) && (!g.ok || g.S == S));
  CHECK(g.nt == nt && g.nprob == nprob && g.slabs == (C + 63) / 64);
  // the three stages lie in order, each aligned for its widest access (z float4, mask bytes uint2), and the launch stays in 64 KB
  const size_t zstage = static_cast<size_t>(nt * rows * rank * 4), red = static_cast<size_t>(4 * 8 * nt * 8 * rank * 4);
  CHECK(static_cast<size_t>(g.bits_off) >= zstage && static_cast<size_t>(g.bits_off) >= red && g.bits_off % 16 == 0);
  CHECK(static_cast<size_t>(g.live_off) == g.bits_off + static_cast<size_t>(nt * rows * 8));
  CHECK(g.lds == g.live_off + static_cast<size_t>(rows));
  CHECK(g.lds + kColaccStaticLds <= 65536);
  CHECK(g.ws_bytes == static_cast<size_t>(2) * S * C * rank * 4);
  CHECK(g.ticket_words == static_cast<size_t>((C + 63) / 64) * nprob);
  CHECK(g.ticket_words == colacc_plan(1, C, 8, mode).ticket_words);       // what dalm_lora2_colacc_ticket_words asks for
  const int64_t cap = colacc_row_cap(rank, static_cast<int>(nt));
  const int64_t budget = (512 + g.slabs * nprob - 1) / (g.slabs * nprob);
  CHECK(cap % 32 == 0 && rows <= cap && cap * (nt * rank * 4 + nt * 8 + 1) + kColaccStaticLds <= 65536);
  CHECK((cap + 32) * (nt * rank * 4 + nt * 8 + 1) + kColaccStaticLds > 65536);   // and no smaller than it has to be
  if (g.arm == Lora2Arm::cap) CHECK(rows == cap && S > budget);
  if (g.arm == Lora2Arm::max_s) CHECK(rows == 64 || (rows == 32 && R <= 32));
  if (g.arm == Lora2Arm::budget) CHECK(S <= budget);
  CHECK(g.arm != Lora2Arm::min_s);
}

// ---- literally restated plans ---------------------------------------------------------------------------------------------
struct Named { const char* kernel; long long R, C; int rank, mode; int rows, S, last; const char* arm; const char* why; };
static const Named NAMED[] = {
    // the benchmark's shape: unchanged by the move and by the cap fix
    {"rankupd", 4608, 4096, 8, 1, 48, 96, 48, "budget", "benchmark"},
    {"rankupd", 4608, 4096, 8, 2, 72, 64, 72, "budget", "benchmark"},
    {"rankupd", 4608, 4096, 8, 3, 96, 48, 96, "budget", "benchmark"},
    {"colacc", 4608, 4096, 8, 1, 576, 8, 576, "budget", "benchmark"},
    {"colacc", 4608, 4096, 8, 2, 576, 8, 576, "budget", "benchmark"},
    {"colacc", 4608, 4096, 8, 3, 1152, 4, 1152, "budget", "benchmark"},
    // rankupd: the double-buffered loop (second buffer from 16 rows; re-issue from 32 rows, 24 with two terms) and ragged tails
    {"rankupd", 1160, 16384, 8, 1, 52, 23, 16, "budget", "pipelined loop, re-issue, last workgroup 16 rows"},
    {"rankupd", 1160, 16384, 16, 1, 52, 23, 16, "budget", "the same at rank 16"},
    {"rankupd", 530, 16384, 8, 3, 48, 12, 2, "budget", "pipelined loop, last workgroup 2 rows (two waves idle)"},
    {"rankupd", 530, 16384, 16, 3, 48, 12, 2, "budget", "the same at rank 16"},
    {"rankupd", 530, 16384, 8, 2, 36, 15, 26, "budget", "UN = 3: re-issue, partial second round, last workgroup 26 rows"},
    {"rankupd", 1300, 4096, 8, 2, 24, 55, 4, "budget", "UN = 3: exactly one full round of both buffers, last workgroup 4 rows"},
    {"rankupd", 2300, 32768, 8, 2, 256, 9, 252, "min_s", "256 rows per workgroup: ballot bit 63; last workgroup 252 rows"},
    {"rankupd", 70, 640, 8, 1, 4, 18, 2, "max_s", "mask stage with a partial last slab (128 | C, 512 does not)"},
    {"rankupd", 70, 1152, 8, 2, 4, 18, 2, "max_s", "mask stage, two terms, partial last slab"},
    {"rankupd", 70, 136, 8, 3, 4, 18, 2, "max_s", "mask bytes read per lane"},
    {"rankupd", 530, 640, 8, 2, 4, 133, 2, "max_s", "mask stage, partial last slab, many workgroups"},
    {"rankupd", 1160, 1152, 16, 1, 8, 145, 8, "budget", "mask stage, partial last slab, 8 rows per workgroup"},
    // colacc
    {"colacc", 2400, 4096, 8, 1, 320, 8, 160, "budget", "UN = 4: two loop iterations, last split 160 rows"},
    {"colacc", 2400, 4096, 16, 1, 320, 8, 160, "budget", "UN = 2: three loop iterations"},
    {"colacc", 1300, 4096, 8, 2, 192, 7, 148, "budget", "two terms, UN = 2: two loop iterations, last split 148 rows"},
    {"colacc", 1030, 1024, 8, 1, 64, 17, 6, "max_s", "S = 17: the last arriver's third round of 8 holds one split; last split 6 rows"},
    {"colacc", 1030, 1024, 8, 2, 64, 17, 6, "max_s", "the same with two terms"},
    {"colacc", 577, 512, 8, 1, 64, 10, 1, "max_s", "S = 10, last split one row"},
    {"colacc", 577, 512, 16, 3, 64, 10, 1, "max_s", "the same, two problems at rank 16"},
    // colacc's row cap: all three stages within 64 KB (before the fix: 1024 / 1024 / 2048 rows, 82944 / 74752 / 83968 bytes)
    {"colacc", 8200, 4096, 8, 2, 800, 11, 200, "cap", "cap, two terms, last split 200 rows"},
    {"colacc", 4100, 4096, 16, 3, 896, 5, 516, "cap", "cap, rank 16, two problems, last split 516 rows"},
    {"colacc", 7210, 4096, 8, 2, 800, 10, 10, "cap", "cap, two terms, last split 10 rows"},
    {"colacc", 4487, 4096, 16, 3, 896, 6, 7, "cap", "cap, rank 16, two problems, last split 7 rows"},
    {"colacc", 12550, 4096, 8, 1, 1568, 9, 6, "cap", "cap, rank 8, one term, last split 6 rows, S = 9"},
};

static void check_named(bool print) {
  for (const Named& n : NAMED) {
    cR = n.R; cC = n.C; crank = n.rank; cmode = n.mode;
    int rows, S;
    size_t lds;
    Lora2Arm arm;
    if (strcmp(n.kernel, "rankupd") == 0) {
      const RankupdPlan p = rankupd_plan(n.R, n.C, n.mode, true);
      rows = p.rows_per_wg; S = p.S; lds = p.lds; arm = p.arm;
    } else {
      const ColaccPlan g = colacc_plan(n.R, n.C, n.rank, n.mode);
      rows = g.rows_per_split; S = g.S; lds = g.lds; arm = g.arm;
    }
    const long long last = n.R - static_cast<long long>(S - 1) * rows;
    CHECK(rows == n.rows);
    CHECK(S == n.S);
    CHECK(last == n.last);
    CHECK(strcmp(lora2_arm_name(arm), n.arm) == 0);
    if (print) printf("%s (%lld, %lld) rank %d mode %d: arm %s, %d rows x %d, last %lld rows, LDS %zu bytes - %s\n", n.kernel, n.R, n.C, n.rank,
                      n.mode, lora2_arm_name(arm), rows, S, last, lds, n.why);
  }
  // the cap fix at the three shapes that asked for the most LDS: the new stages
  cR = 0; cC = 0; crank = 0; cmode = 0;
  CHECK(colacc_plan(8200, 4096, 8, 2).lds == 800 * 81 && colacc_plan(4100, 4096, 16, 3).lds == 896 * 73);
  CHECK(colacc_plan(40000, 4096, 8, 1).lds == 1568 * 41 && colacc_plan(40000, 4096, 8, 1).rows_per_split == 1568);
  // the launch limit on S: one either side
  CHECK(rankupd_plan(65535ll * 256, 65536, 2, false).ok && !rankupd_plan(65535ll * 256 + 1, 65536, 2, false).ok);
  CHECK(colacc_plan(65535ll * 800, 65536, 8, 2).ok && !colacc_plan(65535ll * 800 + 1, 65536, 8, 2).ok);
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: lora2_plan_check SHAPES.txt [--print]\n"); return 2; }
  FILE* in = fopen(argv[1], "r");
  if (!in) { perror(argv[1]); return 2; }
  const bool print = argc > 2 && strcmp(argv[2], "--print") == 0;
  long long R, C, maxR = 0;
  int shapes = 0;
  std::set<long long> cols;
  static const int RANK_MODE[5][2] = {{8, 1}, {16, 1}, {8, 2}, {8, 3}, {16, 3}};
  while (fscanf(in, "%lld %lld", &R, &C) == 2) {
    for (int mode = 1; mode <= 3; ++mode) check_rankupd(R, C, mode);
    for (const auto& rm : RANK_MODE) check_colacc(R, C, rm[0], rm[1]);
    cols.insert(C);
    if (R > maxR) maxR = R;
    ++shapes;
  }
  fclose(in);
  for (const long long c : cols)
    for (long long r = 1; r <= maxR; ++r) {
      for (int mode = 1; mode <= 3; ++mode) check_rankupd(r, c, mode);
      for (const auto& rm : RANK_MODE) check_colacc(r, c, rm[0], rm[1]);
    }
  check_named(print);
  if (failures || shapes == 0) return 1;
  printf("lora2 plans ok: %d shapes, rows 1..%lld at %zu widths\n", shapes, maxR, cols.size());
  return 0;
}
