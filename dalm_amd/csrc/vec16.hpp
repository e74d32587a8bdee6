// How a lane reads and writes 16 bytes of a row as f32: the one bf16x8 <-> f32 decode / encode and the Vec16<T> trait
// (float: 4 elements, bf16_t: 8) that every row-wise kernel goes through.  Everything here is forced inline: a kernel
// that calls a helper compiles to what it would with the loop written in place.
#pragma once
#include "bf16.hpp"
#include "common.hpp"

namespace dalm {
namespace {

// 8 bf16 in four words -> f32 (a shift and a mask per word) and back (v_cvt_pk_bf16_f32: RNE)
__device__ __forceinline__ void dec8(const uint4& v, float (&x)[8]) {
  const unsigned int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    x[2 * i] = __uint_as_float(w[i] << 16);
    x[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}
__device__ __forceinline__ uint4 enc8(const float (&x)[8]) {
  return make_uint4(pack_bf16x2(x[0], x[1]), pack_bf16x2(x[2], x[3]), pack_bf16x2(x[4], x[5]), pack_bf16x2(x[6], x[7]));
}

// 4 floats of which the first `nvalid` exist; one 16-byte load when all four do and the address allows it
__device__ __forceinline__ float4 ld4_guard(const float* p, int nvalid, bool vec_ok) {
  if (nvalid >= 4 && vec_ok) return *reinterpret_cast<const float4*>(p);
  float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
  if (nvalid > 0) r.x = p[0];
  if (nvalid > 1) r.y = p[1];
  if (nvalid > 2) r.z = p[2];
  if (nvalid > 3) r.w = p[3];
  return r;
}

// Vec16<T>: VEC elements = 16 bytes.
//   load / store          one 16-byte access
//   load_nt / store_nt    the same, non-temporal (ce.hip: every logit is read once, every gradient written once)
//   load / store (nvalid, vec_ok)   guarded: element-wise when the chunk is partial or the row is not 16-byte aligned
//   get / put             one element
//   rb                    the round trip through the tensor dtype (where an eager elementwise op would round)
template <typename T> struct Vec16;
template <> struct Vec16<float> {
  static constexpr int VEC = 4;
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  __device__ static __forceinline__ float rb(float x) { return x; }
  __device__ static __forceinline__ void load(const float* p, float (&x)[4]) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
  }
  __device__ static __forceinline__ void store(float* p, const float (&x)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
  }
  __device__ static __forceinline__ void load_nt(const float* p, float (&x)[4]) {
    const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
    x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
  }
  __device__ static __forceinline__ void store_nt(float* p, const float (&x)[4]) {
    f32x4 v;
    v.x = x[0]; v.y = x[1]; v.z = x[2]; v.w = x[3];
    __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p));
  }
  __device__ static __forceinline__ void load(const float* p, int nvalid, bool vec_ok, float (&x)[4]) {
    if (nvalid >= 4 && vec_ok) {
      // cached loads on purpose (pool.hip): the token states were just written by the encoder's last layer and sit in
      // L2 / Infinity Cache (non-temporal loads measured 20 % slower here, unlike the CE kernels)
      load(p, x);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) x[e] = (e < nvalid) ? p[e] : 0.f;
    }
  }
  __device__ static __forceinline__ void store(float* p, int nvalid, bool vec_ok, const float (&x)[4]) {
    if (nvalid >= 4 && vec_ok) {
      store(p, x);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) if (e < nvalid) p[e] = x[e];
    }
  }
  __device__ static __forceinline__ float get(const float* p) { return *p; }
  __device__ static __forceinline__ void put(float* p, float x) { *p = x; }
};
template <> struct Vec16<bf16_t> {
  static constexpr int VEC = 8;
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  __device__ static __forceinline__ float rb(float x) { return bf16_to_f32(f32_to_bf16(x)); }
  __device__ static __forceinline__ void load(const bf16_t* p, float (&x)[8]) { dec8(*reinterpret_cast<const uint4*>(p), x); }
  __device__ static __forceinline__ void store(bf16_t* p, const float (&x)[8]) { *reinterpret_cast<uint4*>(p) = enc8(x); }
  __device__ static __forceinline__ void load_nt(const bf16_t* p, float (&x)[8]) {
    const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
    dec8(make_uint4(v.x, v.y, v.z, v.w), x);
  }
  __device__ static __forceinline__ void store_nt(bf16_t* p, const float (&x)[8]) {
    const uint4 o = enc8(x);
    u32x4 v;
    v.x = o.x; v.y = o.y; v.z = o.z; v.w = o.w;
    __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p));
  }
  __device__ static __forceinline__ void load(const bf16_t* p, int nvalid, bool vec_ok, float (&x)[8]) {
    if (nvalid >= 8 && vec_ok) {
      load(p, x);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = (e < nvalid) ? bf16_to_f32(p[e].v) : 0.f;
    }
  }
  __device__ static __forceinline__ void store(bf16_t* p, int nvalid, bool vec_ok, const float (&x)[8]) {
    if (nvalid >= 8 && vec_ok) {
      store(p, x);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) if (e < nvalid) p[e].v = f32_to_bf16(x[e]);
    }
  }
  __device__ static __forceinline__ float get(const bf16_t* p) { return bf16_to_f32(p->v); }
  __device__ static __forceinline__ void put(bf16_t* p, float x) { p->v = f32_to_bf16(x); }
};

}  // namespace
}  // namespace dalm
