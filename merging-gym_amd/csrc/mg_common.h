// mg_common.h -- block size, the host+device function macro, vector types, the two kinds of store.
// A part of the one translation unit merging_hip.hip (see its head comment).
#pragma once

#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "merging_hip.h"

#pragma clang fp contract(off)

namespace {

// One build, no compile-time variants: every alternative measured against the shipped choice
// (profiles/r01, profiles/r02/ab) was removed from the product source once it lost.
constexpr int kBlock = 256;  // 4 waves of 64 (128 and 512 measured within 0.8 %)
constexpr int kObs = MG_OBS_DIM;
constexpr int kMaxMembers = 64;  // of one call: entries in the kernel argument, bits of the learner's target-copy mask

// The step's functions compile for the host as well: the CPU single-env path (mg_host_step,
// BASELINE config 1, scripts/human_player.py's 20 Hz loop on a machine without a GPU) runs this
// same code. The host side is built with the same -ffp-contract=off, and fma / fabs / sqrt are
// correctly rounded there too, so host and device give the same doubles; only the cold sin/cos
// branch (|theta| >= 1/16) uses glibc on the host and the device library on the GPU, which agree
// within 1 ulp. Live episodes do reach it: an arrived car drives on until the episode ends.
#define MG_HD __host__ __device__ __forceinline__
#define MG_STR_(x) #x
#define MG_STR(x) MG_STR_(x)

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// Store of a per-step output (observation, reward, flags, actions): written once, never
// re-read by the step, so optionally non-temporal. The env state is stored normally: the
// next step reads it back (write-through or non-temporal state stores measured 0 to +4 %).
template <class T>
__device__ __forceinline__ void st_out(T* p, T v) {
  __builtin_nontemporal_store(v, p);
}

template <class T>
MG_HD void st_state(T* p, T v) {
  *p = v;
}

}  // namespace
