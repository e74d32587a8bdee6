// Launch geometry of the stacked LoRA kernels (lora2.hip): rows per workgroup / per row split, grid extents, dynamic LDS bytes and
// the colacc workspace and ticket sizes.  Host-only, plain C++17 (no HIP): the launchers and the size functions of lora2.hip take
// every one of these numbers from here, and tests/lora2_plan_check.cpp checks them on the host.
//   mode 1: one problem;  mode 2: two terms over ONE activation (rank 8);  mode 3: two independent problems (grid z).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace dalm {

// which bound decided the row count of a workgroup (rankupd) / a split (colacc)
enum class Lora2Arm {
  budget,   // the workgroup budget of one resident round
  max_s,    // fewer rows than the budget would hand out: the smallest unit per workgroup (rankupd 4 rows, colacc 64)
  min_s,    // rankupd: more rows than budget x 256: 256 rows per workgroup
  cap       // colacc: more rows per split than its LDS stages hold: the row cap
};
inline const char* lora2_arm_name(Lora2Arm a) {
  return a == Lora2Arm::budget ? "budget" : a == Lora2Arm::max_s ? "max_s" : a == Lora2Arm::min_s ? "min_s" : "cap";
}

// ---- rankupd: grid (slabs of 512 columns, S row groups, nprob) ----
constexpr int kRankupdMaxRows = 256;      // per workgroup: the LDS mask stage and the 64-bit liveness ballot (4 waves x 64 rows)
struct RankupdPlan {
  bool ok;                                // false: S > 65535, the call is rejected
  Lora2Arm arm;
  int rows_per_wg, S, slabs, nprob, nt;
  bool stage;                             // the mask bytes come in through LDS (the call carries masks and 128 | C)
  size_t lds;                             // dynamic LDS bytes: the mask stage [nt][rows_per_wg][64]
};
inline RankupdPlan rankupd_plan(int64_t R, int64_t C, int mode, bool bits) {
  RankupdPlan p;
  const int64_t slabs = (C + 511) / 512, nprob = mode == 3 ? 2 : 1;
  p.slabs = static_cast<int>(slabs);
  p.nprob = static_cast<int>(nprob);
  p.nt = mode == 2 ? 2 : 1;
  // one resident round of workgroups (2 per CU with two terms' W slices in registers, 3 with one): every workgroup pays its W
  // loads and mask stage once (1536 workgroups of 24 rows measured no faster than round 4's kernel)
  int64_t S = (mode == 2 ? 512 : 768) / (slabs * nprob);
  const int64_t max_s = (R + 3) / 4, min_s = (R + kRankupdMaxRows - 1) / kRankupdMaxRows;   // at most 256 rows per workgroup
  p.arm = Lora2Arm::budget;
  if (S > max_s) { S = max_s; p.arm = Lora2Arm::max_s; }
  if (S < min_s) { S = min_s; p.arm = Lora2Arm::min_s; }
  if (S < 1) S = 1;
  const int64_t rows = ((R + S - 1) / S + 3) / 4 * 4;
  p.rows_per_wg = static_cast<int>(rows);
  S = (R + rows - 1) / rows;
  p.ok = S <= 65535;
  p.S = static_cast<int>(S);
  p.stage = bits && C % 128 == 0;
  p.lds = p.stage ? static_cast<size_t>(p.nt) * p.rows_per_wg * 64 : 0;
  return p;
}

// ---- colacc: grid (slabs of 64 columns, S row splits, nprob) ----
constexpr int64_t kLdsBytes = 65536;      // what a workgroup may use without raising the kernel's dynamic LDS limit
constexpr int64_t kColaccStaticLds = 16;  // the ticket `slot` (4 bytes), padded to the alignment of the dynamic segment behind it
struct ColaccPlan {
  bool ok;                                // false: S > 65535, the call is rejected
  Lora2Arm arm;
  int rows_per_split, S, slabs, nprob, nt;
  size_t lds;                             // dynamic LDS bytes: z stage (later the 4 waves' sums) | mask stage | liveness bytes
  int bits_off, live_off;                 // where the mask stage and the liveness bytes start
  size_t ws_bytes;                        // [2][S][C * rank] floats
  size_t ticket_words;                    // one per slab and problem
};
// rows of a split that fit: z stage [nt][rows][rank] f32 + mask stage [nt][rows][8] + one liveness byte per row, beside the
// static slot, in 64 KB; a multiple of 32 (the row lanes of a workgroup)
inline int64_t colacc_row_cap(int rank, int nt) {
  const int64_t per_row = static_cast<int64_t>(nt) * rank * 4 + static_cast<int64_t>(nt) * 8 + 1;
  const int64_t cap = (kLdsBytes - kColaccStaticLds) / per_row / 32 * 32;
  return cap < 32 ? 32 : cap;
}
inline ColaccPlan colacc_plan(int64_t R, int64_t C, int rank, int mode) {
  ColaccPlan g;
  const int nt = mode == 2 ? 2 : 1, nprob = mode == 3 ? 2 : 1;
  g.nt = nt;
  g.nprob = nprob;
  g.slabs = static_cast<int>((C + 63) / 64);
  int64_t S = (512 + static_cast<int64_t>(g.slabs) * nprob - 1) / (static_cast<int64_t>(g.slabs) * nprob);
  const int64_t max_s = (R + 63) / 64;
  g.arm = Lora2Arm::budget;
  if (S > max_s) { S = max_s; g.arm = Lora2Arm::max_s; }
  if (S < 1) S = 1;
  int64_t rows = (R + S - 1) / S;
  const int64_t cap = colacc_row_cap(rank, nt);
  if (rows > cap) { rows = cap; g.arm = Lora2Arm::cap; }
  rows = (rows + 31) / 32 * 32;
  g.rows_per_split = static_cast<int>(rows);
  S = (R + rows - 1) / rows;
  g.ok = S <= 65535;
  g.S = static_cast<int>(S);
  const size_t stage = static_cast<size_t>(nt) * rows * rank * sizeof(float);
  const size_t red = static_cast<size_t>(4) * 8 * nt * 8 * rank * sizeof(float);
  g.lds = stage > red ? stage : red;
  g.bits_off = static_cast<int>(g.lds);
  g.lds += static_cast<size_t>(nt) * rows * 8;                          // the mask stage (used when the call carries masks)
  g.live_off = static_cast<int>(g.lds);
  g.lds += static_cast<size_t>(rows);                                   // the rows' liveness bytes (used when the call carries them)
  g.ws_bytes = static_cast<size_t>(2) * static_cast<size_t>(S) * C * rank * sizeof(float);
  g.ticket_words = static_cast<size_t>(g.slabs) * nprob;
  return g;
}

}  // namespace dalm
