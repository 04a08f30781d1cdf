// mg_stats.h -- episode statistics of one env: EpStats, finish_episode, after_step, the no-wait atomics variants.
// A part of the one translation unit merging_hip.hip (see its head comment).
#pragma once

#include "mg_common.h"
#include "mg_env.h"

namespace {

// Completed-episode statistics (mg_episode_stats) of one env held in registers for a multi-step
// launch: the fp64 sums and ret1_pending are loaded once and accumulated in the same order as the
// per-step read-modify-write (so bit-identical); the counts are this launch's increments, added
// to the record once at the end. A finishing lane then never waits on a global load.
// The counts are 16-bit fields of three words (a launch finishes at most num_steps <= 65535
// episodes per env, mg_rollout_random checks it): two VGPRs fewer, which keeps the rollout
// kernel within 128 VGPRs (4 waves per SIMD).
struct EpStats {
  double r1, r2, rm, pend;
  uint32_t ep_coll;   // episodes | collisions << 16
  uint32_t ego_wm;    // ego_first | win_main << 16
  uint32_t wh;        // win_hdqn
  uint32_t steps;
  bool dirty_f, dirty_c;  // the fp64 half / the counts changed
};

// the record as 4 x 16 bytes: {ret[0], ret[1]}, {ret_main, ret1_pending}, counts 0-3, counts 4-7
MG_HD double2* stats_f64(const mg_stats& St, int64_t i) {
  return reinterpret_cast<double2*>(St.rec + i);
}
MG_HD uint4* stats_u32(const mg_stats& St, int64_t i) {
  return reinterpret_cast<uint4*>(St.rec + i) + 2;
}

MG_HD void stats_load(const mg_stats& St, int64_t i, EpStats& s) {
  s.dirty_f = s.dirty_c = false;
  s.r1 = s.r2 = s.rm = s.pend = 0.0;
  s.ep_coll = s.ego_wm = s.wh = s.steps = 0u;
  if (St.rec) {
    const double2 a = stats_f64(St, i)[0], b = stats_f64(St, i)[1];
    s.r1 = a.x;
    s.r2 = a.y;
    s.rm = b.x;
    s.pend = b.y;
  }
}

MG_HD void stats_store(const mg_stats& St, int64_t i, const EpStats& s) {
  if (!St.rec) return;
  if (s.dirty_f) {
    stats_f64(St, i)[0] = make_double2(s.r1, s.r2);
    stats_f64(St, i)[1] = make_double2(s.rm, s.pend);
  }
  if (s.dirty_c) {  // once per launch: the load's latency is not on the step loop
    uint4 c = stats_u32(St, i)[0], d = stats_u32(St, i)[1];
    c.x += s.ep_coll & 0xFFFFu;
    c.y += s.ep_coll >> 16;
    c.z += s.ego_wm & 0xFFFFu;
    c.w += s.steps;
    d.x += s.ego_wm >> 16;
    d.y += s.wh;
    stats_u32(St, i)[0] = c;
    stats_u32(St, i)[1] = d;
  }
}

// The ego arrived first on a step that did not end the episode: keep r1_accumulate as it stood
// before that step -- main.py's ep_reward stops there (:209-211), since winner stays 1.
MG_HD void note_first_arrival(const mg_stats& St, int64_t i, const StepOut& r,
                                                   EpStats* sreg = nullptr) {
  if (sreg) {
    sreg->pend = r.ret_pre;
    sreg->dirty_f = true;
  } else if (St.rec) {
    reinterpret_cast<double*>(St.rec + i)[3] = r.ret_pre;  // ret1_pending
  }
}

// gym.vector autoreset after the episode was recorded: keep its terminal observation, reset the
// env (merging_env.py:208-230) and put the reset observation in r.o (r0: the launch's precomputed
// one, reset0).
MG_HD void autoreset_env(const mg_params& P, Env& e, StepOut& r, float* final_obs_row, const Reset0* r0) {
  if (final_obs_row) {
#pragma unroll
    for (int k = 0; k < kObs; ++k) final_obs_row[k] = static_cast<float>(r.o[k]);
  }
  e.p1 = e.p2 = P.start_point;
  e.v1 = e.v2 = P.start_vel;
  e.ret1 = e.ret2 = 0.0;
  e.steps = 0;
  e.winner = 0;
  e.done = false;
  if (r0) {
#pragma unroll
    for (int k = 0; k < kObs; ++k) r.o[k] = r0->o[k];
    r.dx1 = r0->dx1;
  } else {
    reset_obs(P, r.o, &r.dx1);
  }
}

// Record the finished episode, then autoreset (autoreset_env). sreg: statistics held in registers
// (the random rollout), nullptr: read-modify-write them in memory (the one-step kernels and the host
// path; the Q-net kernels use finish_episode_nowait below). The episode's statistics:
// r{1,2}_accumulate (hdqn.py's ep_reward), main.py's winner-filtered ep_reward (r1_accumulate
// before the ego-first step while winner == 1), main.py:225's win test on the state the last step
// acted on (r.win_pre) and hdqn.py:342's on the terminal state.
MG_HD void finish_episode(const mg_params& P, Env& e, StepOut& r,
                                               const mg_stats& St, float* final_obs_row,
                                               int64_t i, EpStats* sreg = nullptr, const Reset0* r0 = nullptr) {
  const bool ego_won = e.winner == 1;
  const bool win_hdqn = (P.end_point - e.p2) > (P.end_point - e.p1);
  if (sreg) {
    const double pend = r.first1 ? r.ret_pre : sreg->pend;
    sreg->r1 += e.ret1;
    sreg->r2 += e.ret2;
    sreg->rm += ego_won ? pend : e.ret1;
    sreg->ep_coll += 1u + (r.coll ? 0x10000u : 0u);
    sreg->ego_wm += (ego_won ? 1u : 0u) + (r.win_pre ? 0x10000u : 0u);
    sreg->wh += win_hdqn ? 1u : 0u;
    sreg->steps += e.steps;
    sreg->dirty_f = sreg->dirty_c = true;
  } else if (St.rec) {
    // one 64-byte record per env: a finishing env reads and writes one cache line
    double2* fp = stats_f64(St, i);
    const double2 a = fp[0], b = fp[1];
    const double pend = r.first1 ? r.ret_pre : b.y;
    fp[0] = make_double2(a.x + e.ret1, a.y + e.ret2);
    fp[1] = make_double2(b.x + (ego_won ? pend : e.ret1), b.y);
    uint4* cp = stats_u32(St, i);
    uint4 c = cp[0];
    uint2 d = reinterpret_cast<const uint2*>(cp + 1)[0];
    c.x += 1;
    c.y += r.coll ? 1u : 0u;
    c.z += ego_won ? 1u : 0u;
    c.w += e.steps;
    d.x += r.win_pre ? 1u : 0u;
    d.y += win_hdqn ? 1u : 0u;
    cp[0] = c;
    reinterpret_cast<uint2*>(cp + 1)[0] = d;
  }
  autoreset_env(P, e, r, final_obs_row, r0);
}

// After a step with statistics: the first-arrival bookkeeping, then autoreset where done.
MG_HD void after_step(const mg_params& P, Env& e, StepOut& r, const mg_stats& St,
                                           float* final_obs_row, int64_t i, bool autoreset,
                                           EpStats* sreg = nullptr, const Reset0* r0 = nullptr) {
  const bool finish = autoreset && r.done;
  if (r.first1 && !finish) note_first_arrival(St, i, r, sreg);
  if (finish) finish_episode(P, e, r, St, final_obs_row, i, sreg, r0);
}

// Episode statistics without a load on the step path (round 4), for the batched device kernels: a
// finishing env's record update is a handful of no-return atomics, so the lane never waits for its
// record (finish_episode's read-modify-write stalls the wave on a global load). The env's lane is
// the only writer of its record during a launch and atomics from one lane to one address are
// performed in issue order, so the sums are the sequential ones, bit for bit. The one value read
// back at an episode end is main.py's pending r1_accumulate (ret1_pending), and only when the ego
// arrived first on an earlier step: it is held in a register `pend`, loaded at the launch start
// for the lanes whose episode is in that state (pend_load: winner == 1, a small fraction) and set
// on the first arrival (also stored to the record then, a store without a wait).
__device__ __forceinline__ double pend_load(const mg_stats& St, int64_t i, const Env& e) {
  return St.rec && e.winner == 1 ? St.rec[i].ret1_pending : 0.0;
}

__device__ __forceinline__ void finish_episode_nowait(const mg_params& P, Env& e, StepOut& r, const mg_stats& St,
                                                      float* final_obs_row, int64_t i, double pend,
                                                      const Reset0* r0) {
  if (St.rec) {
    mg_episode_stats* rec = St.rec + i;
    const bool ego_won = e.winner == 1;
    const bool win_hdqn = (P.end_point - e.p2) > (P.end_point - e.p1);
    unsafeAtomicAdd(&rec->ret[0], e.ret1);
    unsafeAtomicAdd(&rec->ret[1], e.ret2);
    unsafeAtomicAdd(&rec->ret_main, ego_won ? (r.first1 ? r.ret_pre : pend) : e.ret1);
    atomicAdd(&rec->episodes, 1u);
    atomicAdd(&rec->steps, e.steps);
    if (r.coll) atomicAdd(&rec->collisions, 1u);
    if (ego_won) atomicAdd(&rec->ego_first, 1u);
    if (r.win_pre) atomicAdd(&rec->win_main, 1u);
    if (win_hdqn) atomicAdd(&rec->win_hdqn, 1u);
  }
  autoreset_env(P, e, r, final_obs_row, r0);
}

// after_step with the no-wait statistics; returns whether the episode finished (autoreset)
__device__ __forceinline__ bool after_step_nowait(const mg_params& P, Env& e, StepOut& r, const mg_stats& St,
                                                  float* final_obs_row, int64_t i, bool autoreset, double& pend,
                                                  const Reset0* r0) {
  const bool finish = autoreset && r.done;
  if (finish) {
    finish_episode_nowait(P, e, r, St, final_obs_row, i, pend, r0);
  } else if (r.first1) {
    pend = r.ret_pre;
    if (St.rec) St.rec[i].ret1_pending = r.ret_pre;  // note_first_arrival
  }
  return finish;
}

// The Q value a finished episode adds to its record (mg_episode_stats.q_eval), without a wait
__device__ __forceinline__ void add_q_eval_nowait(const mg_stats& St, int64_t i, double q) {
  if (St.rec) unsafeAtomicAdd(&St.rec[i].q_eval, q);
}

}  // namespace
