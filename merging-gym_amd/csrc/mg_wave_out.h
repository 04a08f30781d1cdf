// mg_wave_out.h -- a wave's outputs: observations staged through LDS, the won mask, the packed step bytes.
// A part of the one translation unit merging_hip.hip (see its head comment).
#pragma once

#include "mg_common.h"
#include "mg_env.h"

namespace {

// Wave-scope ordering of LDS accesses between the lanes of ONE wave (no s_barrier): the LDS
// executes a wave's accesses in order; this only stops the compiler from moving them.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A wave's [rows,10] fp32 observations written through its LDS slice as contiguous 16-byte stores
// (64 rows of 40 B become 160 dwordx4 lanes instead of 640 scattered dwords): the slice holds the
// new observations afterwards, and no other wave is waited for (no block barrier).
__device__ __forceinline__ void wave_copy_rows(const float* wtile, float* dst, int nrows);

// One observation (fp64, or a step's obs_t) as the fp32 row of an LDS tile, in 8-byte pieces.
template <class T>
__device__ __forceinline__ void put_obs_row(float* row, const T (&o)[kObs]) {
  float2* t2 = reinterpret_cast<float2*>(row);
#pragma unroll
  for (int k = 0; k < kObs / 2; ++k)
    t2[k] = make_float2(static_cast<float>(o[2 * k]), static_cast<float>(o[2 * k + 1]));
}

__device__ __forceinline__ void wave_store_obs(float* wtile, const obs_t (&o)[kObs], float* dst,
                                               int nrows) {
  put_obs_row(wtile + (threadIdx.x & 63) * kObs, o);
  wave_lds_sync();
  wave_copy_rows(wtile, dst, nrows);
  wave_lds_sync();
}

// wave_store_obs for N consecutive 64-row slices (slice j = r[j].o of every lane), written out
// as one run of nrows <= 64 N rows.
template <int N>
__device__ __forceinline__ void wave_store_obs_n(float* wtile, const StepOut (&r)[N], float* dst,
                                                 int nrows) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < N; ++j) put_obs_row(wtile + (64 * j + lane) * kObs, r[j].o);
  wave_lds_sync();
  wave_copy_rows(wtile, dst, nrows);
  wave_lds_sync();
}

// A wave's nrows x 10 fp32 LDS slice to dst: 16-byte stores when dst allows, else 8-byte.
__device__ __forceinline__ void wave_copy_rows(const float* wtile, float* dst, int nrows) {
  const int lane = threadIdx.x & 63;
  // a full wave (64 rows = 160 16-byte pieces) into a 16-byte aligned destination: three fixed
  // lane passes instead of the strided loop (wave-uniform test)
  if (dst != nullptr && nrows == 64 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
    f32x4* d4 = reinterpret_cast<f32x4*>(dst);
    const f32x4* s4 = reinterpret_cast<const f32x4*>(wtile);
    const f32x4 v0 = s4[lane], v1 = s4[64 + lane];
    const f32x4 v2 = s4[128 + (lane & 31)];
    st_out(d4 + lane, v0);
    st_out(d4 + 64 + lane, v1);
    if (lane < 32) st_out(d4 + 128 + lane, v2);
    return;
  }
  if (dst != nullptr && nrows > 0) {
    const int nfl = nrows * kObs;
    if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
      const int n4 = nfl >> 2;
      f32x4* d4 = reinterpret_cast<f32x4*>(dst);
      const f32x4* s4 = reinterpret_cast<const f32x4*>(wtile);
      for (int j = lane; j < n4; j += 64) st_out(d4 + j, s4[j]);
      const int tail = nfl - (n4 << 2);
      if (lane < tail) st_out(dst + (n4 << 2) + lane, wtile[(n4 << 2) + lane]);
    } else {
      const int n2 = nfl >> 1;
      f32x2* d2 = reinterpret_cast<f32x2*>(dst);
      const f32x2* s2 = reinterpret_cast<const f32x2*>(wtile);
      for (int j = lane; j < n2; j += 64) st_out(d2 + j, s2[j]);
    }
  }
}

// Step t's won bits of one wave (every lane calls it): word t * ceil(n/64) + wbase / 64.
__device__ __forceinline__ void store_won_mask(uint64_t* mask, bool won, int t, int64_t n,
                                               int64_t wbase, int wrows) {
  if (mask == nullptr) return;
  const uint64_t m = __ballot(won);
  if ((threadIdx.x & 63) == 0 && wrows > 0)
    st_out(mask + static_cast<int64_t>(t) * ((n + 63) >> 6) + (wbase >> 6), m);
}

// The env index through an empty asm: the state stores recompute their addresses from it
// instead of keeping the load addresses (two VGPRs per array) live across the step.
__device__ __forceinline__ int64_t opaque_index(int64_t i) {
  asm volatile("" : "+v"(i));
  return i;
}

// One env-step's four byte outputs (a1, a2, done, collision) as the little-endian u32 of an
// interleaved [.., 4] uint8 buffer (mg_outputs.flags, mg_traj.flags).
MG_HD uint32_t pack_step_bytes(int a1, int a2, bool done, bool coll) {
  return static_cast<uint32_t>(a1 & 0xff) | (static_cast<uint32_t>(a2 & 0xff) << 8) |
         (done ? 0x10000u : 0u) | (coll ? 0x1000000u : 0u);
}

// One env-step's four byte outputs of a trajectory (a1, a2, done, collision): a single 32-bit
// store into the interleaved [T, n, 4] buffer when the caller gave one, else four byte stores.
__device__ __forceinline__ void store_step_bytes(const mg_traj& T, int64_t row, int a1, int a2, bool done,
                                                 bool coll) {
  if (T.flags) {
    st_out(reinterpret_cast<uint32_t*>(T.flags) + row, pack_step_bytes(a1, a2, done, coll));
    return;
  }
  if (T.a1) st_out(T.a1 + row, static_cast<int8_t>(a1));
  if (T.a2) st_out(T.a2 + row, static_cast<int8_t>(a2));
  if (T.done) st_out(T.done + row, static_cast<uint8_t>(done ? 1 : 0));
  if (T.coll) st_out(T.coll + row, static_cast<uint8_t>(coll ? 1 : 0));
}

}  // namespace
