// mg_step.h -- the one-step kernel (Launch, step_kernel) and the random-policy rollout (Rollout, rollout_kernel).
// A part of the one translation unit merging_hip.hip (see its head comment).
#pragma once

#include "mg_common.h"
#include "mg_env.h"
#include "mg_stats.h"
#include "mg_wave_out.h"

namespace {

struct Launch {
  mg_params P;
  Reset0 R0;
  mg_state S;
  mg_outputs O;
  mg_stats St;
  const int8_t* a1;
  const int8_t* a2;
  int8_t* a1_out;
  int8_t* a2_out;
  uint64_t seed;
  uint64_t step_idx;
  int64_t env_offset;
  int64_t n;
  uint32_t flags;
  int32_t opp_random;
};

// The step kernel. OUT64 = the single-env path (packed fp64 record, no LDS staging).
template <int ACT, bool OUT64>
__global__ __launch_bounds__(kBlock) void step_kernel(const Launch L) {
  __shared__ __attribute__((aligned(16))) float obs_tile[kBlock * kObs];

  const mg_params& P = L.P;
  const int tid = threadIdx.x;
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kBlock;
  const int64_t i = base + tid;
  const bool live = i < L.n;
  StepOut r;
  r.done = false;
  bool won = false;

  if (live) {
    int a1, a2;
    if constexpr (ACT == kActPhilox) {
      draw_actions(static_cast<uint64_t>(L.env_offset + i), L.step_idx, L.seed, L.opp_random, a1, a2);
      if (!L.O.flags) {  // with O.flags the actions go out with done / collision below
        if (L.a1_out) st_out(L.a1_out + i, static_cast<int8_t>(a1));
        if (L.a2_out) st_out(L.a2_out + i, static_cast<int8_t>(a2));
      }
    } else {
      a1 = L.a1[i];
      a2 = L.a2 ? static_cast<int>(L.a2[i]) : MG_ACTION_NONE;
    }
    // the two action_dict lookups (vector loads from the launch arguments) issued before the
    // state loads, so they are in flight together (looked up inside the step, the first one's
    // wait came after the state had arrived): -1 to -1.5 % per launch (r03q)
    const double sp1 = action_speed_or0(P, a1), sp2 = action_speed_or0(P, a2);
    Env e = load_env(L.S, i);
    env_step_sp(P, e, a1, a2, sp1, sp2, r);
    if (r.bad) {
      if (L.O.error) atomicOr(L.O.error, r.bad);
      store_env(L.S, i, e);  // clock (and the ego for a bad action2) advanced, nothing else
    } else {
      if constexpr (OUT64) {
        mg_rec64* rec = L.O.rec64 + i;
        {  // the fp64 observation of the state after the step (score_step's values, recomputed)
          double x1, y1, x2, y2, od[kObs];
          lon2coord(P, e.p1, true, x1, y1);
          lon2coord(P, e.p2, false, x2, y2);
          observe(P, e.p1, e.v1, e.p2, e.v2, x1, y1, x2, y2, od);
#pragma unroll
          for (int k = 0; k < kObs; ++k) rec->obs[k] = od[k];
        }
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
        st_out(reinterpret_cast<f32x2*>(L.O.rew) + i,
               f32x2{static_cast<float>(r.r1), static_cast<float>(r.r2)});
      }
      if (L.O.flags) {
        st_out(reinterpret_cast<uint32_t*>(L.O.flags) + i, pack_step_bytes(a1, a2, r.done, r.coll));
      } else {
        if (L.O.done) st_out(L.O.done + i, static_cast<uint8_t>(r.done ? 1 : 0));
        if (L.O.coll) st_out(L.O.coll + i, static_cast<uint8_t>(r.coll ? 1 : 0));
      }
      won = e.winner == 1;
      // statistics by read-modify-write: the no-wait atomics (finish_episode_nowait) measured
      // +4 % per launch here at 2^20 (r04j), where the finishing lanes' loads hit the Infinity Cache
      after_step(P, e, r, L.St, L.O.final_obs ? L.O.final_obs + i * kObs : nullptr, i,
                 (L.flags & MG_AUTORESET) != 0, nullptr, &L.R0);
      store_env(L.S, opaque_index(i), e);
    }
  }

  if (L.O.done_mask) {
    const uint64_t m = __ballot(live && r.done);
    if ((tid & 63) == 0 && live) L.O.done_mask[i >> 6] = m;
  }
  if (L.O.won_mask) {
    const uint64_t m = __ballot(won);
    if ((tid & 63) == 0 && live) L.O.won_mask[i >> 6] = m;
  }
  if constexpr (!OUT64) {
    // per-wave staging, no block barrier: a wave held up by a finishing lane's statistics
    // read-modify-write (a DRAM read past the Infinity Cache) no longer holds up the block's
    // other three at the barrier (2^22 envs: 107.0 -> 104.8 us per launch with the lookups
    // above, r03q; +-0 at 2^20)
    if (L.O.obs) {
      const int64_t wbase = base + (tid & ~63);
      const int64_t wrem = L.n - wbase;
      wave_store_obs(obs_tile + (tid & ~63) * kObs, r.o, L.O.obs + wbase * kObs,
                     wrem <= 0 ? 0 : (wrem < 64 ? static_cast<int>(wrem) : 64));
    }
  }
}

struct Rollout {
  mg_params P;
  Reset0 R0;
  mg_state S;
  mg_traj T;
  mg_stats St;
  uint64_t seed;
  uint64_t first_step;
  int64_t env_offset;
  int64_t n;
  int32_t num_steps;
  int32_t opp_random;
  uint32_t flags;
};

// num_steps consecutive mg_step_random steps with the env kept in registers: the state is
// read once and written once per launch; step t's outputs go to slice t of the trajectory.
// FULL: the outputs every MergeVecEnv rollout passes are present (obs, rew, the interleaved step
// record, statistics, autoreset; final observations and the won mask stay optional). The
// instance assumes so, which drops null tests the compiler otherwise keeps live across the loop
// as 64-bit lane masks (SGPR pairs, spilled into VGPR lanes: a v_readlane per use).
template <bool FULL>
__global__ __launch_bounds__(kBlock) void rollout_kernel(const Rollout R) {
  __shared__ __attribute__((aligned(16))) float obs_tile[kBlock * kObs];

  if constexpr (FULL) {
    __builtin_assume(R.T.obs != nullptr);
    __builtin_assume(R.T.rew != nullptr);
    __builtin_assume(R.T.flags != nullptr);
    __builtin_assume(R.St.rec != nullptr);
    __builtin_assume((R.flags & MG_AUTORESET) != 0);
  }
  const mg_params& P = R.P;
  const int tid = threadIdx.x;
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kBlock;
  const int64_t i = base + tid;
  const bool live = i < R.n;
  const int64_t wbase = base + (tid & ~63);
  const int64_t wrem = R.n - wbase;
  const int wrows = wrem <= 0 ? 0 : (wrem < 64 ? static_cast<int>(wrem) : 64);
  const bool autoreset = (R.flags & MG_AUTORESET) != 0;

  Env e;
  // statistics in registers for the launch: -9.5 % per step against the read-modify-write (the
  // finishing lanes no longer wait on a load); the no-wait atomics measured +16 % median (r04j)
  EpStats sreg;
  if (live) {
    e = load_env(R.S, i);
    stats_load(R.St, i, sreg);
  }
  bool won = false;
  uint4 u = make_uint4(0u, 0u, 0u, 0u);  // the Philox block of the current eight steps
  for (int t = 0; t < R.num_steps; ++t) {
    StepOut r;  // per step: no loop-carried copy of the observation (dead lanes store nothing)
    const int64_t row = static_cast<int64_t>(t) * R.n + i;
    const uint64_t k = R.first_step + t;
    if (t == 0 || k % kStepsPerPhilox == 0)  // wave-uniform
      u = philox_block(static_cast<uint64_t>(R.env_offset + i), k / kStepsPerPhilox, R.seed, /*opaque_key=*/true);
    if (live) {
      int a1, a2;
      actions_from_block(u, k, R.opp_random, a1, a2);
      env_step<false>(P, e, a1, a2, r);  // Philox actions are always valid: the unchecked step
      if (R.T.rew)
        st_out(reinterpret_cast<f32x2*>(R.T.rew) + row,
               f32x2{static_cast<float>(r.r1), static_cast<float>(r.r2)});
      store_step_bytes(R.T, row, a1, a2, r.done, r.coll);
      won = e.winner == 1;
      after_step(P, e, r, R.St, R.T.final_obs ? R.T.final_obs + row * kObs : nullptr, i, autoreset, &sreg, &R.R0);
    }
    store_won_mask(R.T.won_mask, won, t, R.n, wbase, wrows);
    if (R.T.obs)  // staged per wave: waves never wait for each other
      wave_store_obs(obs_tile + (tid & ~63) * kObs, r.o,
                     R.T.obs + (static_cast<int64_t>(t) * R.n + wbase) * kObs, wrows);
  }
  if (live) {
    store_env(R.S, i, e);
    stats_store(R.St, i, sreg);
  }
}

}  // namespace
