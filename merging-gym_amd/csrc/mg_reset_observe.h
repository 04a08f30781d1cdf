// mg_reset_observe.h -- reset_kernel and observe_kernel.
// A part of the one translation unit merging_hip.hip (see its head comment).
#pragma once

#include "mg_common.h"
#include "mg_env.h"

namespace {

__global__ __launch_bounds__(kBlock) void reset_kernel(const mg_params P, const mg_state S,
                                                       const uint8_t* mask, const mg_outputs O,
                                                       int64_t n) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  if (mask && !mask[i]) return;
  S.p1[i] = P.start_point;
  S.v1[i] = P.start_vel;
  S.p2[i] = P.start_point;
  S.v2[i] = P.start_vel;
  S.ret1[i] = 0.0;
  S.ret2[i] = 0.0;
  S.tf[i] = 0u;
  if (O.obs || O.rec64) {
    double o[kObs];
    reset_obs(P, o);
    if (O.obs) {
#pragma unroll
      for (int k = 0; k < kObs; ++k) O.obs[i * kObs + k] = static_cast<float>(o[k]);
    }
    if (O.rec64) {
      mg_rec64* rec = O.rec64 + i;
#pragma unroll
      for (int k = 0; k < kObs; ++k) rec->obs[k] = o[k];
      rec->rew[0] = rec->rew[1] = 0.0;
      rec->acc[0] = rec->acc[1] = 0.0;
      rec->pos[0] = rec->pos[1] = P.start_point;
      rec->vel[0] = rec->vel[1] = P.start_vel;
      rec->ret[0] = rec->ret[1] = 0.0;
      rec->tf = 0u;
      rec->status = 0u;
    }
  }
}

__global__ __launch_bounds__(kBlock) void observe_kernel(const mg_params P, const mg_state S,
                                                         const mg_outputs O, int64_t n) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  const double p1 = S.p1[i], v1 = S.v1[i], p2 = S.p2[i], v2 = S.v2[i];
  double x1, y1, x2, y2, o[kObs];
  lon2coord(P, p1, true, x1, y1);
  lon2coord(P, p2, false, x2, y2);
  observe(P, p1, v1, p2, v2, x1, y1, x2, y2, o);
  if (O.obs) {
#pragma unroll
    for (int k = 0; k < kObs; ++k) O.obs[i * kObs + k] = static_cast<float>(o[k]);
  }
  if (O.rec64) {
#pragma unroll
    for (int k = 0; k < kObs; ++k) O.rec64[i].obs[k] = o[k];
  }
  uint8_t* coll = O.flags ? O.flags + 4 * i + 3 : (O.coll ? O.coll + i : nullptr);
  if (coll) *coll = boxes_intersect(vehicle_box(P, y1, x1), vehicle_box(P, y2, x2)) ? 1 : 0;
}

}  // namespace
