// K1: masked mean-pool + L2 normalise of bi-encoder token states (gfx950).
//
// Stands in for AutoModelForRagE2E.mean_pooling + F.normalize
//   dalm/models/rag_e2e_base_model.py:95-97,108-111
//   dalm/models/retriever_only_base_model.py:60-68
// The reference materialises three [B,T,D] temporaries (mask.expand().float(),
// the product, the sum); here each unmasked token row is read once with 16-byte
// lane accesses and padded tokens are never touched.  HBM-bound:
//   forward : n_tok*D*eh bytes read (n_tok = unmasked tokens) + B*D*4 written
//   backward: B*T*D*eh bytes written
#include "dispatch.hpp"
#include "vec16.hpp"

namespace dalm {
namespace {

// grid (DC, B); 4 waves share one 64*VEC-wide d-chunk and split the tokens.
template <typename T>
__global__ __launch_bounds__(256) void pool_sum_kernel(const T* __restrict__ h, const int64_t* __restrict__ mask,
                                                       int Tn, int D, int vec_ok, float* __restrict__ emb,
                                                       float* __restrict__ inv_count) {
  constexpr int VEC = Vec16<T>::VEC;
  __shared__ float part[4][64 * VEC];
  __shared__ float cnt_part[4];
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int d = (blockIdx.x * 64 + lane) * VEC;
  int nvalid = D - d;
  nvalid = nvalid < 0 ? 0 : (nvalid > VEC ? VEC : nvalid);
  const T* hb = h + static_cast<int64_t>(b) * Tn * D + d;
  const int64_t* mb = mask + static_cast<int64_t>(b) * Tn;

  float acc[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
  float cnt = 0.f;
  // tokens wave, wave+4, ... ; two in flight per iteration
  for (int t = wave; t < Tn; t += 8) {
    const int t2 = t + 4;
    const int64_t m0 = mb[t];
    const int64_t m1 = (t2 < Tn) ? mb[t2] : 0;
    float x0[VEC], x1[VEC];
    if (m0 != 0 && nvalid > 0) Vec16<T>::load(hb + static_cast<int64_t>(t) * D, nvalid, vec_ok, x0);
    if (m1 != 0 && nvalid > 0) Vec16<T>::load(hb + static_cast<int64_t>(t2) * D, nvalid, vec_ok, x1);
    const float f0 = static_cast<float>(m0), f1 = static_cast<float>(m1);
    cnt += f0 + f1;
    if (m0 != 0 && nvalid > 0) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[e] = fmaf(f0, x0[e], acc[e]);
    }
    if (m1 != 0 && nvalid > 0) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[e] = fmaf(f1, x1[e], acc[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < VEC; ++e) part[wave][lane * VEC + e] = acc[e];
  if (lane == 0) cnt_part[wave] = cnt;
  __syncthreads();
  if (wave == 0) {
    const float c = fmaxf(cnt_part[0] + cnt_part[1] + cnt_part[2] + cnt_part[3], 1e-9f);
    const float ic = 1.f / c;
    if (blockIdx.x == 0 && lane == 0) inv_count[b] = ic;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const int i = lane * VEC + e;
      const float s = (part[0][i] + part[1][i]) + (part[2][i] + part[3][i]);
      if (e < nvalid) emb[static_cast<int64_t>(b) * D + d + e] = s / c;
    }
  }
}

// one block per sample: |u| and (optionally) e = u / max(|u|, 1e-12) in place
__global__ __launch_bounds__(256) void l2norm_rows_kernel(float* __restrict__ emb, int D, int normalize,
                                                          float* __restrict__ norm) {
  __shared__ float red[4];
  float* row = emb + static_cast<int64_t>(blockIdx.x) * D;
  float ss = 0.f;
  for (int i = threadIdx.x; i < D; i += 256) ss = fmaf(row[i], row[i], ss);
  ss = block_sum<256>(ss, red);
  const float nrm = sqrtf(ss);
  if (threadIdx.x == 0) norm[blockIdx.x] = nrm;
  if (normalize) {
    const float denom = fmaxf(nrm, 1e-12f);
    for (int i = threadIdx.x; i < D; i += 256) row[i] = row[i] / denom;
  }
}

// ---------------------------------------------------------------------------------------------------
// Fused forward: one 1024-thread workgroup walks the unmasked tokens of ONE sample (or of one token slice of
// it, grid.x = TZ) across the full embedding width, so the mean, |u| and the normalisation happen in the
// same launch (the two-launch form above costs ~20 us at batch 18 for ~2 us of data movement).
//   TPR threads cover one token row (VEC elements each, NCH d-chunks per thread when D > TPR*VEC),
//   G = NT/TPR token groups stride through the tokens, 4-8 token rows in flight per group.
//   NT = 1024 threads when the batch is small (one workgroup has to keep a CU's memory pipe full on its own);
//   NT = 256 for large batches: with >= 2 samples per CU, 1024-thread workgroups run in ceil(B/512) rounds and the
//   reduction tail of each round leaves the memory pipe idle (B = 1200: 3 rounds for 2.3 rounds of work).
//   TZ == 1: sums are combined through LDS in fixed group order, then u, |u|, e are written.
//   TZ  > 1: raw partial sums go to part[b][z][D] (+ counts) and pool_finish_kernel completes the sample;
//            used when B alone cannot occupy the chip (B * bytes per sample is large but B < ~128).
// ---------------------------------------------------------------------------------------------------
template <typename T, int NCH, int NT>
__global__ __launch_bounds__(NT) void pool_fused_kernel(const T* __restrict__ h, const int64_t* __restrict__ mask,
                                                          int Tn, int D, int tpr_log2, int vec_ok, int normalize,
                                                          float* __restrict__ emb, float* __restrict__ norm,
                                                          float* __restrict__ inv_count, float* __restrict__ part,
                                                          float* __restrict__ part_cnt) {
  constexpr int VEC = Vec16<T>::VEC;
  constexpr int TIF = (NCH == 1) ? 8 : 4;   // token rows in flight per group on the fast path (128 B per thread)
  extern __shared__ float lds[];       // [G][Dp] partial sums, then reduction scratch
  __shared__ float red[16];
  __shared__ float cnt_s[16];
  const int b = blockIdx.y, z = blockIdx.x, TZ = gridDim.x;
  const int tid = threadIdx.x;
  const int TPR = 1 << tpr_log2, G = NT >> tpr_log2;
  const int g = tid >> tpr_log2, c = tid & (TPR - 1);
  const int per = (Tn + TZ - 1) / TZ;
  const int t_lo = z * per, t_hi = min(Tn, t_lo + per);
  const T* hb = h + static_cast<int64_t>(b) * Tn * D;
  const int64_t* mb = mask + static_cast<int64_t>(b) * Tn;

  float acc[NCH][VEC];
#pragma unroll
  for (int q = 0; q < NCH; ++q)
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[q][e] = 0.f;
  float cnt = 0.f;
  if (vec_ok) {
    // Fast path (16-byte aligned rows, D % VEC == 0): UNCONDITIONAL vector loads - a predicated load compiles to a
    // branch and the compiler then waits with vmcnt(0), which serialises the four rows in flight.  A padded token
    // is redirected to the slice's first row instead (an L1/L2 hit, no HBM traffic) and its value discarded.
    const int t_anchor = min(t_lo + g, Tn - 1);
    for (int t0 = t_lo + g; t0 < t_hi; t0 += TIF * G) {
      int64_t m[TIF];
#pragma unroll
      for (int u = 0; u < TIF; ++u) {
        const int t = t0 + u * G;
        const int64_t mv = mb[min(t, t_hi - 1)];
        m[u] = (t < t_hi) ? mv : 0;
      }
#pragma unroll
      for (int q = 0; q < NCH; ++q) {
        const int d = (q * TPR + c) * VEC;
        const bool dok = d < D;
        const int dd = dok ? d : 0;
        float x[TIF][VEC];
#pragma unroll
        for (int u = 0; u < TIF; ++u) {
          const int tt = (m[u] != 0) ? (t0 + u * G) : t_anchor;
          Vec16<T>::load(hb + static_cast<int64_t>(tt) * D + dd, VEC, true, x[u]);
        }
#pragma unroll
        for (int u = 0; u < TIF; ++u) {
          const float f = static_cast<float>(m[u]);
          const bool use = (m[u] != 0) && dok;
#pragma unroll
          for (int e = 0; e < VEC; ++e) acc[q][e] += use ? f * x[u][e] : 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < TIF; ++u) cnt += static_cast<float>(m[u]);
    }
  } else {
    for (int t0 = t_lo + g; t0 < t_hi; t0 += 4 * G) {
      int64_t m[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) m[u] = (t0 + u * G < t_hi) ? mb[t0 + u * G] : 0;
#pragma unroll
      for (int q = 0; q < NCH; ++q) {
        const int d = (q * TPR + c) * VEC;
        int nvalid = D - d;
        nvalid = nvalid < 0 ? 0 : (nvalid > VEC ? VEC : nvalid);
        float x[4][VEC];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (m[u] != 0 && nvalid > 0) Vec16<T>::load(hb + static_cast<int64_t>(t0 + u * G) * D + d, nvalid, false, x[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (m[u] != 0 && nvalid > 0) {
            const float f = static_cast<float>(m[u]);
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[q][e] = fmaf(f, x[u][e], acc[q][e]);
          }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) cnt += static_cast<float>(m[u]);
    }
  }
  // ---- combine the G token groups (fixed order) ----
  const int Dp = TPR * VEC * NCH;
#pragma unroll
  for (int q = 0; q < NCH; ++q)
#pragma unroll
    for (int e = 0; e < VEC; ++e) lds[g * Dp + (q * TPR + c) * VEC + e] = acc[q][e];
  if (c == 0) cnt_s[g] = cnt;
  __syncthreads();
  float total = 0.f;
  for (int i = 0; i < G; ++i) total += cnt_s[i];
  float ss = 0.f;
  float u[NCH][VEC];
  if (g == 0) {
#pragma unroll
    for (int q = 0; q < NCH; ++q)
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const int i = (q * TPR + c) * VEC + e;
        float s = 0.f;
        for (int k = 0; k < G; ++k) s += lds[k * Dp + i];
        u[q][e] = s;
      }
  }
  if (TZ > 1) {
    if (g == 0) {
      float* pr = part + (static_cast<int64_t>(b) * TZ + z) * D;
#pragma unroll
      for (int q = 0; q < NCH; ++q)
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const int i = (q * TPR + c) * VEC + e;
          if (i < D) pr[i] = u[q][e];
        }
      if (c == 0) part_cnt[b * TZ + z] = total;
    }
    return;
  }
  const float cden = fmaxf(total, 1e-9f);
  if (g == 0) {
#pragma unroll
    for (int q = 0; q < NCH; ++q)
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const int i = (q * TPR + c) * VEC + e;
        u[q][e] = (i < D) ? u[q][e] / cden : 0.f;
        ss = fmaf(u[q][e], u[q][e], ss);
      }
  }
  ss = block_sum<NT>(ss, red);
  const float nrm = sqrtf(ss);
  if (tid == 0) { norm[b] = nrm; inv_count[b] = 1.f / cden; }
  if (g == 0) {
    const float denom = fmaxf(nrm, 1e-12f);
#pragma unroll
    for (int q = 0; q < NCH; ++q)
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const int i = (q * TPR + c) * VEC + e;
        if (i < D) emb[static_cast<int64_t>(b) * D + i] = normalize ? u[q][e] / denom : u[q][e];
      }
  }
}

// completes a sample from TZ partial sums (fixed z order): one block per sample
__global__ __launch_bounds__(256) void pool_finish_kernel(const float* __restrict__ part,
                                                          const float* __restrict__ part_cnt, int TZ, int D,
                                                          int normalize, float* __restrict__ emb,
                                                          float* __restrict__ norm, float* __restrict__ inv_count) {
  __shared__ float red[4];
  const int b = blockIdx.x;
  float total = 0.f;
  for (int z = 0; z < TZ; ++z) total += part_cnt[b * TZ + z];
  const float cden = fmaxf(total, 1e-9f);
  float* row = emb + static_cast<int64_t>(b) * D;
  float ss = 0.f;
  for (int i = threadIdx.x; i < D; i += 256) {
    float pv[32];   // TZ <= 32: one batch of loads (a `for z < TZ` loop of loads is a serial latency chain)
#pragma unroll
    for (int z = 0; z < 32; ++z) pv[z] = part[(static_cast<int64_t>(b) * TZ + min(z, TZ - 1)) * D + i];
    float s = 0.f;
#pragma unroll
    for (int z = 0; z < 32; ++z) s += (z < TZ) ? pv[z] : 0.f;
    s /= cden;
    row[i] = s;   // re-read below by the same thread only
    ss = fmaf(s, s, ss);
  }
  ss = block_sum<256>(ss, red);
  const float nrm = sqrtf(ss);
  if (threadIdx.x == 0) { norm[b] = nrm; inv_count[b] = 1.f / cden; }
  if (normalize) {
    const float denom = fmaxf(nrm, 1e-12f);
    for (int i = threadIdx.x; i < D; i += 256) row[i] = row[i] / denom;
  }
}

// grid (DC, B, TZ).  dh[b,t,:] = mask[b,t] * inv_count[b] * du[b,:], with
//   du = d_emb                                  (normalize == 0)
//   du = (d_emb - e (e . d_emb)) / |u|           (|u| >= 1e-12)
//   du = d_emb / 1e-12                           (|u| <  1e-12: clamp_min branch)
template <typename T>
__global__ __launch_bounds__(256) void pool_bwd_kernel(const float* __restrict__ d_emb,
                                                       const float* __restrict__ emb,
                                                       const float* __restrict__ norm,
                                                       const float* __restrict__ inv_count,
                                                       const int64_t* __restrict__ mask, int Tn, int D,
                                                       int normalize, int vec_ok, T* __restrict__ dh) {
  constexpr int VEC = Vec16<T>::VEC;
  __shared__ float red[4];
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int d = (blockIdx.x * 64 + lane) * VEC;
  int nvalid = D - d;
  nvalid = nvalid < 0 ? 0 : (nvalid > VEC ? VEC : nvalid);
  const float* de = d_emb + static_cast<int64_t>(b) * D;
  const float* eb = emb + static_cast<int64_t>(b) * D;

  float g[VEC];
  const float ic = inv_count[b];
  if (normalize) {
    float dot = 0.f;
    for (int i = threadIdx.x; i < D; i += 256) dot = fmaf(eb[i], de[i], dot);
    dot = block_sum<256>(dot, red);
    const float nrm = norm[b];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      float v = 0.f;
      if (e < nvalid) v = (nrm >= 1e-12f) ? (de[d + e] - eb[d + e] * dot) / nrm : de[d + e] / 1e-12f;
      g[e] = v * ic;
    }
  } else {
#pragma unroll
    for (int e = 0; e < VEC; ++e) g[e] = (e < nvalid) ? de[d + e] * ic : 0.f;
  }
  if (nvalid == 0) return;
  T* hb = dh + static_cast<int64_t>(b) * Tn * D + d;
  const int64_t* mb = mask + static_cast<int64_t>(b) * Tn;
  const int tz = gridDim.z, z = blockIdx.z;
  const int per = (Tn + tz - 1) / tz;
  const int t_end = min(Tn, (z + 1) * per);
  for (int t = z * per + wave; t < t_end; t += 4) {
    const float f = static_cast<float>(mb[t]);
    float o[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) o[e] = f * g[e];
    Vec16<T>::store(hb + static_cast<int64_t>(t) * D, nvalid, vec_ok, o);
  }
}


// Row-major backward for large batches: grid (TZ, B), 256 threads.  TPR threads cover one token row (NCH d-chunks each), the
// G = 256/TPR token groups write CONSECUTIVE rows, so a workgroup streams whole contiguous rows (2-4 KB per step at D = 1024)
// and rebuilds du once per sample slice instead of once per 64*VEC-wide d-chunk.  Needs 16-byte aligned rows (vec_ok).
template <typename T, int NCH>
__global__ __launch_bounds__(256) void pool_bwd_rows_kernel(const float* __restrict__ d_emb,
                                                            const float* __restrict__ emb,
                                                            const float* __restrict__ norm,
                                                            const float* __restrict__ inv_count,
                                                            const int64_t* __restrict__ mask, int Tn, int D,
                                                            int normalize, int tpr_log2, T* __restrict__ dh) {
  constexpr int VEC = Vec16<T>::VEC;
  __shared__ float red[4];
  const int b = blockIdx.y, z = blockIdx.x, TZ = gridDim.x, tid = threadIdx.x;
  const int TPR = 1 << tpr_log2, G = 256 >> tpr_log2;
  const int g = tid >> tpr_log2, c = tid & (TPR - 1);
  const float* de = d_emb + static_cast<int64_t>(b) * D;
  const float* eb = emb + static_cast<int64_t>(b) * D;
  const float ic = inv_count[b];
  float dot = 0.f, nrm = 1.f;
  if (normalize) {
    for (int i = tid; i < D; i += 256) dot = fmaf(eb[i], de[i], dot);
    dot = block_sum<256>(dot, red);
    nrm = norm[b];
  }
  float gv[NCH][VEC];
#pragma unroll
  for (int q = 0; q < NCH; ++q) {
    const int d = (q * TPR + c) * VEC;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      float v = 0.f;
      if (d + e < D) {
        if (!normalize) v = de[d + e];
        else v = (nrm >= 1e-12f) ? (de[d + e] - eb[d + e] * dot) / nrm : de[d + e] / 1e-12f;
      }
      gv[q][e] = v * ic;
    }
  }
  const int per = (Tn + TZ - 1) / TZ;
  const int t_lo = z * per, t_hi = min(Tn, t_lo + per);
  T* hb = dh + static_cast<int64_t>(b) * Tn * D;
  const int64_t* mb = mask + static_cast<int64_t>(b) * Tn;
  for (int t0 = t_lo + g; t0 < t_hi; t0 += 4 * G) {
    float f[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) f[u] = static_cast<float>(mb[min(t0 + u * G, t_hi - 1)]);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int t = t0 + u * G;
      if (t < t_hi) {
#pragma unroll
        for (int q = 0; q < NCH; ++q) {
          const int d = (q * TPR + c) * VEC;
          if (d < D) {
            float o[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) o[e] = f[u] * gv[q][e];
            Vec16<T>::store(hb + static_cast<int64_t>(t) * D + d, VEC, true, o);
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// Packed forward (evaluation sweeps; no backward): h [n, D] holds live token rows only, sequence s owns rows
// cu[s] .. cu[s+1], every row weighs 1.  A wave covers a whole token row (64 lanes x VEC elements x NCH d-chunks: 16-byte
// loads, TIF rows in flight), the 4 waves of a workgroup are 4 / wps sequences x wps row slices: short sequences (a query
// is ~12 rows) get one wave each, 4 per workgroup; long ones are split over the 4 waves, whose sums are added in wave order
// through LDS.  The first wave of a sequence then forms the mean, |u| and e and writes the f32 row at emb + s * ld_emb,
// so a batch lands directly in its slice of a larger matrix.  HBM-bound: n*D*eh bytes read + nseq_out*D*4 written.
// ---------------------------------------------------------------------------------------------------
template <typename T, int NCH>
__global__ __launch_bounds__(256) void pool_packed_kernel(const T* __restrict__ h, const int* __restrict__ cu, int n,
                                                          int nseq_out, int D, int wps, float* __restrict__ emb,
                                                          int64_t ld_emb, float* __restrict__ norm,
                                                          float* __restrict__ inv_count) {
  constexpr int VEC = Vec16<T>::VEC;
  constexpr int TIF = (NCH <= 2) ? 4 : 2;       // token rows in flight per wave
  constexpr int DP = 64 * VEC * NCH;
  extern __shared__ float part[];               // [4][DP] when the waves of a sequence combine (wps > 1), nothing otherwise
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int spw = 4 / wps;                      // sequences per workgroup
  const int s = static_cast<int>(blockIdx.x) * spw + wave / wps, sub = wave % wps;
  const bool live = s < nseq_out;
  int lo = 0, hi = 0;
  if (live) {                                   // clamped: a malformed cu cannot send a load out of h
    hi = min(max(cu[s + 1], 0), n);
    lo = min(max(cu[s], 0), hi);
  }
  float acc[NCH][VEC];
#pragma unroll
  for (int q = 0; q < NCH; ++q)
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[q][e] = 0.f;
  // unconditional vector loads (a predicated load compiles to a branch + vmcnt(0) and serialises the rows in flight):
  // a row past the end is redirected to an in-range row (n >= 1) and its value discarded
  const int anchor = min(lo, n - 1);
  for (int r0 = lo + sub; r0 < hi; r0 += TIF * wps) {
#pragma unroll
    for (int q = 0; q < NCH; ++q) {
      const int d = (q * 64 + lane) * VEC;
      const bool dok = d < D;
      const int dd = dok ? d : 0;
      float x[TIF][VEC];
#pragma unroll
      for (int u = 0; u < TIF; ++u) {
        const int r = r0 + u * wps;
        Vec16<T>::load(h + static_cast<int64_t>(r < hi ? r : anchor) * D + dd, VEC, true, x[u]);
      }
#pragma unroll
      for (int u = 0; u < TIF; ++u) {
        const bool use = dok && (r0 + u * wps < hi);
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[q][e] += use ? x[u][e] : 0.f;
      }
    }
  }
  if (wps > 1) {
#pragma unroll
    for (int q = 0; q < NCH; ++q)
#pragma unroll
      for (int e = 0; e < VEC; ++e) part[wave * DP + (q * 64 + lane) * VEC + e] = acc[q][e];
    __syncthreads();
    if (sub != 0) return;
    for (int w = 1; w < wps; ++w)               // fixed order: slice 0 + 1 + 2 + 3
#pragma unroll
      for (int q = 0; q < NCH; ++q)
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[q][e] += part[(wave + w) * DP + (q * 64 + lane) * VEC + e];
  }
  if (!live) return;
  const float cden = fmaxf(static_cast<float>(hi - lo), 1e-9f);
  float ss = 0.f;
#pragma unroll
  for (int q = 0; q < NCH; ++q)
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const bool ok = (q * 64 + lane) * VEC + e < D;
      acc[q][e] = ok ? acc[q][e] / cden : 0.f;
      ss = fmaf(acc[q][e], acc[q][e], ss);
    }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
  const float nrm = sqrtf(ss);
  const float denom = fmaxf(nrm, 1e-12f);
  if (lane == 0) {
    if (norm) norm[s] = nrm;
    if (inv_count) inv_count[s] = 1.f / cden;
  }
  float* row = emb + static_cast<int64_t>(s) * ld_emb;
#pragma unroll
  for (int q = 0; q < NCH; ++q) {
    const int d = (q * 64 + lane) * VEC;
    if (d < D) {                                // D % VEC == 0: a chunk is inside the row or outside it
#pragma unroll
      for (int e4 = 0; e4 < VEC; e4 += 4)
        *reinterpret_cast<float4*>(row + d + e4) =
            make_float4(acc[q][e4] / denom, acc[q][e4 + 1] / denom, acc[q][e4 + 2] / denom, acc[q][e4 + 3] / denom);
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// Last-token pooling from packed rows (causal-LM retrievers: the reference pools the state of the last column, which a
// `pack_plan(..., last_column=True)` keeps as the last row of every sequence).  Forward: one workgroup per sequence reads
// ONE row, cu[s+1] - 1, into registers (up to 8192 elements: 32 f32 values per thread), forms |u| and writes the f32 row.
// HBM: nseq_out*D*eh bytes read + nseq_out*D*4 written - a latency-sized kernel, the point is that nothing else is touched.
// ---------------------------------------------------------------------------------------------------
constexpr int POOL_LAST_MAX_D = 8192;

template <typename T>
__global__ __launch_bounds__(256) void pool_last_fwd_kernel(const T* __restrict__ h, const int* __restrict__ cu, int n, int D,
                                                            int normalize, float* __restrict__ emb, int64_t ld_emb,
                                                            float* __restrict__ norm) {
  constexpr int VEC = Vec16<T>::VEC;
  constexpr int NCH = POOL_LAST_MAX_D / VEC / 256;     // 16-byte chunks per thread at the widest row: 8 (f32) / 4 (bf16)
  __shared__ float red[4];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int hi = min(max(cu[s + 1], 0), n);            // clamped: a malformed cu cannot send a load out of h
  const int lo = min(max(cu[s], 0), hi);
  const bool some = hi > lo;
  const T* row = h + static_cast<int64_t>(some ? hi - 1 : 0) * D;
  float x[NCH][VEC];
  float ss = 0.f;
#pragma unroll
  for (int q = 0; q < NCH; ++q) {
    const int d = (q * 256 + tid) * VEC;
    const bool ok = some && d < D;                     // D % VEC == 0: a chunk is inside the row or outside it
    Vec16<T>::load(row + (d < D ? d : 0), x[q]);       // unconditional (n >= 1, D >= VEC): the value is dropped when !ok
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      x[q][e] = ok ? x[q][e] : 0.f;
      ss = fmaf(x[q][e], x[q][e], ss);
    }
  }
  ss = block_sum<256>(ss, red);
  const float nrm = sqrtf(ss);
  if (tid == 0 && norm) norm[s] = nrm;
  const float denom = fmaxf(nrm, 1e-12f);
  float* out = emb + static_cast<int64_t>(s) * ld_emb;
#pragma unroll
  for (int q = 0; q < NCH; ++q) {
    const int d = (q * 256 + tid) * VEC;
    if (d < D) {
#pragma unroll
      for (int e4 = 0; e4 < VEC; e4 += 4)
        *reinterpret_cast<float4*>(out + d + e4) =
            normalize ? make_float4(x[q][e4] / denom, x[q][e4 + 1] / denom, x[q][e4 + 2] / denom, x[q][e4 + 3] / denom)
                      : make_float4(x[q][e4], x[q][e4 + 1], x[q][e4 + 2], x[q][e4 + 3]);
    }
  }
}

// Backward: dh [n, D] is written once, by one launch.  Workgroup w owns the rows [w R, (w + 1) R) - one contiguous byte range -
// and walks it as zero segments between the rows that close a sequence < nseq_out: a binary search over cu finds the first
// sequence end at or after its first row, the following ends are met in order.  The zero segments are flat 16-byte stores
// (4 in flight per thread), a closing row gets du (the dot product e . d_e over the block first).  Everything that steers
// the walk is the same in every lane; a malformed cu can only change WHICH of the workgroup's own rows count as closing.
//   du = d_e                                       (normalize == 0)
//   du = (d_e - e (e . d_e)) / |u|                 (|u| >= 1e-12)
//   du = d_e / 1e-12                               (|u| <  1e-12: clamp_min branch, as pool_bwd_kernel)
template <typename T>
__global__ __launch_bounds__(256) void pool_last_bwd_kernel(const float* __restrict__ d_emb, int64_t ld_demb,
                                                            const float* __restrict__ emb, int64_t ld_emb,
                                                            const float* __restrict__ norm, const int* __restrict__ cu, int n,
                                                            int nseq_out, int D, int rows_per_wg, int normalize,
                                                            T* __restrict__ dh) {
  constexpr int VEC = Vec16<T>::VEC;
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * rows_per_wg;
  const int r1 = static_cast<int>(min(static_cast<int64_t>(n), r0 + rows_per_wg));
  const int lanes = D / VEC;                           // 16-byte chunks of a row
  float zero[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) zero[e] = 0.f;
  // first j in [1, nseq_out] with cu[j] >= r0 + 1 (nseq_out + 1: none)
  int jl = 1, jh = nseq_out + 1;
  while (jl < jh) {
    const int jm = (jl + jh) >> 1;
    if (cu[jm] < r0 + 1) jl = jm + 1; else jh = jm;
  }
  int j = jl;
  int cur = static_cast<int>(r0);
  while (cur < r1) {
    while (j <= nseq_out && cu[j] < cur + 1) ++j;      // ends already behind: empty sequences repeat an end
    const int close = (j <= nseq_out && cu[j] - 1 < r1) ? cu[j] - 1 : r1;
    // zero rows [cur, close): one flat range of 16-byte chunks
    T* base = dh + static_cast<int64_t>(cur) * D;
    const int64_t chunks = static_cast<int64_t>(close - cur) * lanes;
    for (int64_t i = tid; i < chunks; i += 4 * 256) {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (i + u * 256 < chunks) Vec16<T>::store(base + (i + u * 256) * VEC, zero);
    }
    if (close >= r1) break;
    const int s = j - 1;
    const bool some = cu[s] <= close;                  // a non-empty sequence (always, for a monotone cu)
    const float* de = d_emb + static_cast<int64_t>(s) * ld_demb;
    const float* eb = emb + static_cast<int64_t>(s) * ld_emb;
    float dot = 0.f, nrm = 1.f;
    if (normalize && some) {
      for (int i = tid; i < D; i += 256) dot = fmaf(eb[i], de[i], dot);
      dot = block_sum<256>(dot, red);
      nrm = norm[s];
    }
    T* row = dh + static_cast<int64_t>(close) * D;
    for (int c = tid; c < lanes; c += 256) {
      const int d = c * VEC;
      float o[VEC];
#pragma unroll
      for (int e4 = 0; e4 < VEC; e4 += 4) {            // both rows are 16-byte aligned by contract
        const float4 g4 = some ? *reinterpret_cast<const float4*>(de + d + e4) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 q4 = (some && normalize) ? *reinterpret_cast<const float4*>(eb + d + e4) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float g[4] = {g4.x, g4.y, g4.z, g4.w}, q[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float v = g[e];
          if (normalize) v = (nrm >= 1e-12f) ? (g[e] - q[e] * dot) / nrm : g[e] / 1e-12f;
          o[e4 + e] = some ? v : 0.f;
        }
      }
      Vec16<T>::store(row + d, o);
    }
    cur = close + 1;
  }
}

}  // namespace
}  // namespace dalm

using namespace dalm;

namespace dalm {
namespace {
// Geometry of the fused forward: TPR threads per token row (power of two), NCH chunks per thread, TZ token slices.
struct PoolPlan { int tpr_log2, nch, tz, nt; bool fused; };
inline PoolPlan pool_plan(int64_t B, int64_t T, int64_t D, int vec) {
  PoolPlan p{0, 1, 1, 1024, false};
  const int64_t lanes = (D + vec - 1) / vec;
  int lg = 6;                                  // at least one wave per row
  while ((1ll << lg) < lanes && lg < 10) ++lg;
  const int64_t tpr = 1ll << lg;
  const int64_t nch = (lanes + tpr - 1) / tpr;
  const int64_t lds_bytes = (1024 / tpr) * tpr * vec * nch * 4;
  if (nch > 4 || lds_bytes > 64 * 1024) return p;   // very wide rows: two-launch kernels
  p.tpr_log2 = lg; p.nch = static_cast<int>(nch); p.fused = true;
  // token slices: only when the batch alone leaves most CUs idle AND a sample is big enough to matter
  const int64_t groups = 1024 / tpr;
  int64_t tz = 1;
  // one CU streams ~50-80 GB/s on its own: slice when a sample is more than a few microseconds of that
  if (B < 64 && T * D * (16 / vec) >= (1ll << 20)) {
    tz = (192 + B - 1) / B;
    const int64_t tz_max = (T + 4 * groups - 1) / (4 * groups);
    if (tz > tz_max) tz = tz_max;
    if (tz > 32) tz = 32;
    if (tz < 1) tz = 1;
  }
  p.tz = static_cast<int>(tz);
  if (tz == 1 && tpr <= 256 && B >= 512) p.nt = 256;
  return p;
}
template <typename T>
void launch_pool_fused(const PoolPlan& pl, const T* h, const int64_t* mask, int B, int Tn, int D, int vok, int normalize,
                       float* emb, float* norm, float* inv_count, float* part, float* part_cnt, hipStream_t s) {
  const int vec = Vec16<T>::VEC;
  const size_t lds = static_cast<size_t>(pl.nt) * vec * pl.nch * sizeof(float);
  const dim3 grid(static_cast<unsigned>(pl.tz), static_cast<unsigned>(B));
  by_exact<256, 1024>(pl.nt, [&](auto nt) {
    by_exact<1, 2, 3, 4>(pl.nch, [&](auto nch) {
      hipLaunchKernelGGL((pool_fused_kernel<T, nch, nt>), grid, dim3(nt), lds, s, h, mask, Tn, D, pl.tpr_log2, vok, normalize,
                         emb, norm, inv_count, part, part_cnt);
    });
  });
  if (pl.tz > 1)
    hipLaunchKernelGGL(pool_finish_kernel, dim3(static_cast<unsigned>(B)), dim3(256), 0, s, part, part_cnt, pl.tz, D,
                       normalize, emb, norm, inv_count);
}
}  // namespace
}  // namespace dalm

extern "C" size_t dalm_pool_l2norm_fwd_workspace_bytes(int64_t B, int64_t T, int64_t D, int dtype) {
  if (B <= 0 || T <= 0 || D <= 0) return 0;
  const PoolPlan pl = pool_plan(B, T, D, dtype == DALM_F32 ? 4 : 8);
  if (!pl.fused || pl.tz <= 1) return 0;
  return static_cast<size_t>(B) * pl.tz * (static_cast<size_t>(D) + 1) * sizeof(float);
}

extern "C" int dalm_pool_l2norm_fwd_ws(const void* h, int dtype, const int64_t* mask, int64_t B, int64_t T,
                                       int64_t D, int normalize, float* emb, float* norm, float* inv_count,
                                       void* ws, size_t ws_bytes, dalm_stream_t stream) {
  DALM_REQUIRE(h && mask && emb && norm && inv_count, DALM_E_NULL, "null pointer argument");
  DALM_REQUIRE(dtype == DALM_F32 || dtype == DALM_BF16, DALM_E_DTYPE, "dtype must be DALM_F32 or DALM_BF16");
  DALM_REQUIRE(B > 0 && T > 0 && D > 0 && B <= 65535 && T <= 0x7fffffffll && D <= 0x3fffffffll, DALM_E_SHAPE,
               "need 0<B<=65535, T>0, D>0");
  hipStream_t s = as_stream(stream);
  const int vec = (dtype == DALM_F32) ? 4 : 8;
  const int vok = aligned16(h) && (D % vec == 0);
  PoolPlan pl = pool_plan(B, T, D, vec);
  const size_t need = dalm_pool_l2norm_fwd_workspace_bytes(B, T, D, dtype);
  if (pl.fused && pl.tz > 1 && (ws == nullptr || ws_bytes < need)) pl.tz = 1;   // no scratch: one slice per sample
  if (pl.fused) {
    float* part = static_cast<float*>(ws);
    float* part_cnt = part ? part + static_cast<size_t>(B) * pl.tz * D : nullptr;
    by_dtype(dtype, [&](auto t) {
      using Elt = typename decltype(t)::type;
      launch_pool_fused<Elt>(pl, static_cast<const Elt*>(h), mask, static_cast<int>(B), static_cast<int>(T), static_cast<int>(D), vok,
                           normalize, emb, norm, inv_count, part, part_cnt, s);
    });
    return check_launch(__func__);
  }
  const dim3 grid(static_cast<unsigned>((D + 64 * vec - 1) / (64 * vec)), static_cast<unsigned>(B));
  by_dtype(dtype, [&](auto t) {
    using Elt = typename decltype(t)::type;
    hipLaunchKernelGGL(pool_sum_kernel<Elt>, grid, dim3(256), 0, s, static_cast<const Elt*>(h), mask, static_cast<int>(T),
                       static_cast<int>(D), vok, emb, inv_count);
  });
  hipLaunchKernelGGL(l2norm_rows_kernel, dim3(static_cast<unsigned>(B)), dim3(256), 0, s, emb,
                     static_cast<int>(D), normalize, norm);
  return check_launch(__func__);
}

extern "C" int dalm_pool_l2norm_fwd(const void* h, int dtype, const int64_t* mask, int64_t B, int64_t T,
                                    int64_t D, int normalize, float* emb, float* norm, float* inv_count,
                                    dalm_stream_t stream) {
  return dalm_pool_l2norm_fwd_ws(h, dtype, mask, B, T, D, normalize, emb, norm, inv_count, nullptr, 0, stream);
}

extern "C" int dalm_pool_l2norm_bwd(const float* d_emb, const float* emb, const float* norm,
                                    const float* inv_count, const int64_t* mask, int64_t B, int64_t T,
                                    int64_t D, int normalize, void* dh, int dtype, dalm_stream_t stream) {
  DALM_REQUIRE(d_emb && emb && norm && inv_count && mask && dh, DALM_E_NULL, "null pointer argument");
  DALM_REQUIRE(dtype == DALM_F32 || dtype == DALM_BF16, DALM_E_DTYPE, "dtype must be DALM_F32 or DALM_BF16");
  DALM_REQUIRE(B > 0 && T > 0 && D > 0 && B <= 65535 && T <= 0x7fffffffll && D <= 0x3fffffffll, DALM_E_SHAPE,
               "need 0<B<=65535, T>0, D>0");
  hipStream_t s = as_stream(stream);
  const int vec = (dtype == DALM_F32) ? 4 : 8;
  const int vok = aligned16(dh) && (D % vec == 0);
  const int64_t dc = (D + 64 * vec - 1) / (64 * vec);
  // token slices: every workgroup first rebuilds du (dot product over D, ~16 scalar loads per lane), so many thin slices
  // cost more than they spread - measured (tools/kernel_bench.py, hipGraph timing): cfg3 passage bf16 [18,128,1024]
  // 1044 WGs 12.4 us, 540 WGs 9.2 us, 396 WGs 7.7 us; at B = 150 two slices beat one (17.3 vs 19.2 us bf16)
  int64_t tz = (384 + B * dc - 1) / (B * dc);
  if (B * dc < 1024 && T >= 64 && tz < 2) tz = 2;
  // (slicing large batches further does NOT help: every workgroup first rebuilds du, and at [1200,128,1024] bf16 2 / 4 / 8
  // slices measured 91 / 123 / 192 us against 81 us for one - profiles/history/r04_pool_probe_bwd_tz.txt; large batches take the
  // row-major kernel below instead)
  const int64_t tz_max = (T + 3) / 4;
  if (tz > tz_max) tz = tz_max;
  if (tz < 1) tz = 1;
  if (tz > 64) tz = 64;
  // cached stores: the encoder's backward reads dh next (non-temporal stores measured alone: 17.5 -> 13.8 us at
  // [150,128,1024] bf16, 79 -> 84 us at B = 1200; profiles/history/r04_pool_probe.txt)
  PoolPlan pl{6, 1, 1, 256, true};                 // rows kernel: TPR <= 256 threads per row, up to 4 d-chunks per thread
  const int64_t row_lanes = (D + vec - 1) / vec;
  while ((1ll << pl.tpr_log2) < row_lanes && pl.tpr_log2 < 8) ++pl.tpr_log2;
  pl.nch = static_cast<int>((row_lanes + (1ll << pl.tpr_log2) - 1) >> pl.tpr_log2);
  if (vok && pl.nch <= 4) {
    // token slices: ~768 workgroups, at most 8 slices (measured, profiles/history/r04_pool_probe_bwd_rows.txt: [18,128,1024] bf16
    // 16.8 / 10.9 / 7.9 / 6.5 / 7.5 us for 1 / 2 / 4 / 8 / 16 slices; [1200,128,1024] 71.7 / 78.6 / 86.4 / 112 us for 1 / 2 / 4 / 8)
    int64_t rz = (768 + B - 1) / B;
    if (rz > 8) rz = 8;
    const int64_t groups = 256 >> pl.tpr_log2;
    const int64_t rz_max = (T + 4 * groups - 1) / (4 * groups);
    if (rz > rz_max) rz = rz_max;
    if (rz < 1) rz = 1;
    const dim3 rgrid(static_cast<unsigned>(rz), static_cast<unsigned>(B));
    by_dtype(dtype, [&](auto t) {
      using Elt = typename decltype(t)::type;
      by_exact<1, 2, 3, 4>(pl.nch, [&](auto nch) {
        hipLaunchKernelGGL((pool_bwd_rows_kernel<Elt, nch>), rgrid, dim3(256), 0, s, d_emb, emb, norm, inv_count, mask,
                           static_cast<int>(T), static_cast<int>(D), normalize, pl.tpr_log2, static_cast<Elt*>(dh));
      });
    });
    return check_launch(__func__);
  }
  const dim3 grid(static_cast<unsigned>(dc), static_cast<unsigned>(B), static_cast<unsigned>(tz));
  by_dtype(dtype, [&](auto t) {
    using Elt = typename decltype(t)::type;
    hipLaunchKernelGGL((pool_bwd_kernel<Elt>), grid, dim3(256), 0, s, d_emb, emb, norm, inv_count, mask, static_cast<int>(T),
                       static_cast<int>(D), normalize, vok, static_cast<Elt*>(dh));
  });
  return check_launch(__func__);
}

extern "C" int dalm_pool_l2norm_packed_fwd(const void* h, int dtype, const int32_t* cu, int64_t n, int64_t nseq,
                                           int64_t nseq_out, int64_t D, float* emb, int64_t ld_emb, float* norm,
                                           float* inv_count, dalm_stream_t stream) {
  DALM_REQUIRE(h && cu && emb, DALM_E_NULL, "null pointer argument");
  DALM_REQUIRE(dtype == DALM_F32 || dtype == DALM_BF16, DALM_E_DTYPE, "dtype must be DALM_F32 or DALM_BF16");
  const int vec = (dtype == DALM_F32) ? 4 : 8;
  DALM_REQUIRE(n > 0 && nseq > 0 && nseq_out >= 0 && nseq_out <= nseq && n <= 0x7fffffffll && nseq <= 0x7ffffff0ll &&
                   D > 0 && D % vec == 0 && D <= 64 * vec * 4 && ld_emb >= D,
               DALM_E_SHAPE, "need n>0, 0<=nseq_out<=nseq, D a multiple of 16 bytes and <= 256 lanes of them, ld_emb>=D");
  DALM_REQUIRE(aligned16(h, emb) && ld_emb % 4 == 0,
               DALM_E_ALIGN, "h and emb rows must be 16-byte aligned");
  if (nseq_out == 0) return 0;
  const int64_t lanes = D / vec;
  const int nch = static_cast<int>((lanes + 63) / 64);
  // waves per sequence by the mean sequence length: one wave keeps TIF rows in flight, so a sequence of a few rows gains
  // nothing from more waves, a 128-row passage does
  const int64_t mean_rows = n / nseq;
  const int wps = mean_rows >= 48 ? 4 : (mean_rows >= 24 ? 2 : 1);
  const int spw = 4 / wps;
  const dim3 grid(static_cast<unsigned>((nseq_out + spw - 1) / spw));
  hipStream_t s = as_stream(stream);
  by_dtype(dtype, [&](auto t) {
    using Elt = typename decltype(t)::type;
    by_exact<1, 2, 3, 4>(nch, [&](auto nc) {
      hipLaunchKernelGGL((pool_packed_kernel<Elt, nc>), grid, dim3(256), wps > 1 ? 4 * 64 * vec * nc * sizeof(float) : 0, s,
                         static_cast<const Elt*>(h), cu, static_cast<int>(n), static_cast<int>(nseq_out), static_cast<int>(D), wps,
                         emb, ld_emb, norm, inv_count);
    });
  });
  return check_launch(__func__);
}

namespace dalm {
namespace {
// the argument checks the two last-token entry points share (before anything is enqueued)
inline int pool_last_check(const char* fn, int dtype, int64_t n, int64_t nseq, int64_t nseq_out, int64_t D, int64_t ld_a, int64_t ld_b,
                           bool aligned) {
  if (dtype != DALM_F32 && dtype != DALM_BF16) return fail(DALM_E_DTYPE, fn, "dtype must be DALM_F32 or DALM_BF16");
  const int vec = (dtype == DALM_F32) ? 4 : 8;
  if (!(n > 0 && nseq > 0 && nseq_out >= 0 && nseq_out <= nseq && n <= 0x7fffffffll && nseq <= 0x7ffffff0ll && D > 0 &&
        D % vec == 0 && D <= POOL_LAST_MAX_D && ld_a >= D && ld_b >= D))
    return fail(DALM_E_SHAPE, fn, "need n>0, 0<=nseq_out<=nseq, D a multiple of 16 bytes and <= 8192, leading dimensions >= D");
  if (!(aligned && ld_a % 4 == 0 && ld_b % 4 == 0))
    return fail(DALM_E_ALIGN, fn, "rows must be 16-byte aligned: base pointers, and leading dimensions a multiple of 4");
  return 0;
}
}  // namespace
}  // namespace dalm

extern "C" int dalm_pool_last_packed_fwd(const void* h, int dtype, const int32_t* cu, int64_t n, int64_t nseq, int64_t nseq_out,
                                         int64_t D, int normalize, float* emb, int64_t ld_emb, float* norm, dalm_stream_t stream) {
  DALM_REQUIRE(h && cu && (nseq_out == 0 || emb), DALM_E_NULL, "null pointer argument");
  if (const int rc = pool_last_check(__func__, dtype, n, nseq, nseq_out, D, ld_emb, ld_emb, aligned16(h, emb))) return rc;
  if (nseq_out == 0) return 0;
  hipStream_t s = as_stream(stream);
  by_dtype(dtype, [&](auto t) {
    using Elt = typename decltype(t)::type;
    hipLaunchKernelGGL((pool_last_fwd_kernel<Elt>), dim3(static_cast<unsigned>(nseq_out)), dim3(256), 0, s,
                       static_cast<const Elt*>(h), cu, static_cast<int>(n), static_cast<int>(D), normalize, emb, ld_emb, norm);
  });
  return check_launch(__func__);
}

extern "C" int dalm_pool_last_packed_bwd(const float* d_emb, int64_t ld_demb, const float* emb, int64_t ld_emb, const float* norm,
                                         const int32_t* cu, int64_t n, int64_t nseq, int64_t nseq_out, int64_t D, int normalize,
                                         void* dh, int dtype, dalm_stream_t stream) {
  // nseq_out == 0 pools nothing (dh is all zeros): the pooled side may then be empty tensors, i.e. NULL
  DALM_REQUIRE(cu && dh && (nseq_out == 0 || (d_emb && emb && norm)), DALM_E_NULL, "null pointer argument");
  if (const int rc = pool_last_check(__func__, dtype, n, nseq, nseq_out, D, ld_demb, ld_emb, aligned16(d_emb, emb, dh))) return rc;
  // Rows per workgroup: at most 2048 workgroups (256 CUs x 8 resident 256-thread workgroups: the whole grid is resident at once
  // and each workgroup streams one contiguous range), and at least 16 KB per workgroup (256 threads x 4 stores of 16 bytes in
  // flight) so that a narrow row does not leave most of a workgroup idle.
  const int64_t row_bytes = D * (dtype == DALM_F32 ? 4 : 2);
  int64_t R = (n + 2047) / 2048;
  const int64_t r_min = (16384 + row_bytes - 1) / row_bytes;
  if (R < r_min) R = r_min;
  const int64_t grid = (n + R - 1) / R;
  hipStream_t s = as_stream(stream);
  by_dtype(dtype, [&](auto t) {
    using Elt = typename decltype(t)::type;
    hipLaunchKernelGGL((pool_last_bwd_kernel<Elt>), dim3(static_cast<unsigned>(grid)), dim3(256), 0, s, d_emb, ld_demb, emb, ld_emb,
                       norm, cu, static_cast<int>(n), static_cast<int>(nseq_out), static_cast<int>(D), static_cast<int>(R), normalize,
                       static_cast<Elt*>(dh));
  });
  return check_launch(__func__);
}
