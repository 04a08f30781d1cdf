// mg_host_env.h -- the CPU single-env path: host_step_env, host_step_all, host_reset_env, host_observe_env.
// A part of the one translation unit merging_hip.hip (see its head comment).
#pragma once

#include "mg_common.h"
#include "mg_env.h"
#include "mg_stats.h"
#include "mg_step.h"
#include "mg_wave_out.h"

namespace {

// ============================================================================ host (CPU) path
// The step kernel's per-env body on the host, over host pointers: the single env of BASELINE
// config 1 (MergeEnv.step / reset / observe, merging_env.py:118-230, driven one step at a time by
// scripts/human_player.py:112-187 at 20 Hz), where a kernel launch plus a stream synchronisation
// per step (28.5 us, BENCH_r03 dropin_single_env) costs 20x the step's own ~1 us of fp64 work.
// The same MG_HD functions as the kernels, so a host step gives the kernel's doubles bit for bit
// (tests/test_dropin.py: golden traces on the CPU; test_host_step_equals_kernel on the GPU box).
// Outputs and their conditions follow step_kernel<kActArrays, OUT64 = rec64 != NULL> exactly.
void host_step_env(const Launch& L, int64_t i, bool& done, bool& won) {
  const mg_params& P = L.P;
  const int a1 = L.a1[i];
  const int a2 = L.a2 ? static_cast<int>(L.a2[i]) : MG_ACTION_NONE;
  Env e = load_env(L.S, i);
  StepOut r;
  env_step_sp(P, e, a1, a2, action_speed_or0(P, a1), action_speed_or0(P, a2), r);
  done = won = false;
  if (r.bad) {
    if (L.O.error) *L.O.error |= r.bad;
    store_env(L.S, i, e);
  } else {
    if (L.O.rec64) {
      mg_rec64* rec = L.O.rec64 + i;
      double x1, y1, x2, y2, od[kObs];
      lon2coord(P, e.p1, true, x1, y1);
      lon2coord(P, e.p2, false, x2, y2);
      observe(P, e.p1, e.v1, e.p2, e.v2, x1, y1, x2, y2, od);
      for (int k = 0; k < kObs; ++k) rec->obs[k] = od[k];
      rec->rew[0] = r.r1;
      rec->rew[1] = r.r2;
      rec->acc[0] = r.acc1;
      rec->acc[1] = r.acc2;
      rec->pos[0] = e.p1;
      rec->pos[1] = e.p2;
      rec->vel[0] = e.v1;
      rec->vel[1] = e.v2;
      rec->ret[0] = e.ret1;
      rec->ret[1] = e.ret2;
      rec->tf = pack_tf(e);
      rec->status = (r.done ? MG_ST_DONE : 0u) | (r.coll ? MG_ST_COLLISION : 0u) |
                    (r.r1_int ? MG_ST_R1_INT : 0u) | (r.r2_int ? MG_ST_R2_INT : 0u) |
                    (r.v1_int ? MG_ST_V1_INT : 0u) | (r.v2_int ? MG_ST_V2_INT : 0u);
    } else if (L.O.rew) {
      L.O.rew[2 * i] = static_cast<float>(r.r1);
      L.O.rew[2 * i + 1] = static_cast<float>(r.r2);
    }
    if (L.O.flags) {
      reinterpret_cast<uint32_t*>(L.O.flags)[i] = pack_step_bytes(a1, a2, r.done, r.coll);
    } else {
      if (L.O.done) L.O.done[i] = r.done ? 1 : 0;
      if (L.O.coll) L.O.coll[i] = r.coll ? 1 : 0;
    }
    done = r.done;
    won = e.winner == 1;
    after_step(P, e, r, L.St, L.O.final_obs ? L.O.final_obs + i * kObs : nullptr, i,
               (L.flags & MG_AUTORESET) != 0, nullptr, &L.R0);
    store_env(L.S, i, e);
  }
  if (!L.O.rec64 && L.O.obs) {  // the kernel's observation tile: zeros for a bad action's env
    for (int k = 0; k < kObs; ++k) L.O.obs[i * kObs + k] = r.o[k];
  }
}

// Every env of a batch, with the kernel's done / won mask words: one per 64-env group.
void host_step_all(const Launch& L) {
  for (int64_t w = 0; w < L.n; w += 64) {
    uint64_t dm = 0, wm = 0;
    const int64_t end = L.n - w < 64 ? L.n : w + 64;
    for (int64_t i = w; i < end; ++i) {
      bool d, won;
      host_step_env(L, i, d, won);
      dm |= static_cast<uint64_t>(d) << (i - w);
      wm |= static_cast<uint64_t>(won) << (i - w);
    }
    if (L.O.done_mask) L.O.done_mask[w >> 6] = dm;
    if (L.O.won_mask) L.O.won_mask[w >> 6] = wm;
  }
}

void host_reset_env(const mg_params& P, const mg_state& S, const mg_outputs& O, int64_t i) {
  S.p1[i] = S.p2[i] = P.start_point;
  S.v1[i] = S.v2[i] = P.start_vel;
  S.ret1[i] = S.ret2[i] = 0.0;
  S.tf[i] = 0u;
  if (!O.obs && !O.rec64) return;
  double o[kObs];
  reset_obs(P, o);
  if (O.obs)
    for (int k = 0; k < kObs; ++k) O.obs[i * kObs + k] = static_cast<float>(o[k]);
  if (O.rec64) {
    mg_rec64* rec = O.rec64 + i;
    std::memset(rec, 0, sizeof(*rec));
    for (int k = 0; k < kObs; ++k) rec->obs[k] = o[k];
    rec->pos[0] = rec->pos[1] = P.start_point;
    rec->vel[0] = rec->vel[1] = P.start_vel;
  }
}

void host_observe_env(const mg_params& P, const mg_state& S, const mg_outputs& O, int64_t i) {
  const double p1 = S.p1[i], v1 = S.v1[i], p2 = S.p2[i], v2 = S.v2[i];
  double x1, y1, x2, y2, o[kObs];
  lon2coord(P, p1, true, x1, y1);
  lon2coord(P, p2, false, x2, y2);
  observe(P, p1, v1, p2, v2, x1, y1, x2, y2, o);
  if (O.obs)
    for (int k = 0; k < kObs; ++k) O.obs[i * kObs + k] = static_cast<float>(o[k]);
  if (O.rec64)
    for (int k = 0; k < kObs; ++k) O.rec64[i].obs[k] = o[k];
  uint8_t* coll = O.flags ? O.flags + 4 * i + 3 : (O.coll ? O.coll + i : nullptr);
  if (coll) *coll = boxes_intersect(vehicle_box(P, y1, x1), vehicle_box(P, y2, x2)) ? 1 : 0;
}

}  // namespace
