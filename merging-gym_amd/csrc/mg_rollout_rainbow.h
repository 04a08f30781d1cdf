// mg_rollout_rainbow.h -- Rainbow's acting loop fused with the env step: RbRollout, rainbow_rollout_kernel.
// A part of the one translation unit merging_hip.hip (see its head comment).
#pragma once

#include "mg_common.h"
#include "mg_env.h"
#include "mg_rainbow.h"
#include "mg_stats.h"
#include "mg_wave_out.h"

namespace {

// scripts/ranbowdqn.py:662-680, T steps per launch: action = current_model.act(state) (:668), action_op =
// current_model.act(state[3:] + state[:3]) (:669) or None, env.step(action, action_op) (:671), the reset at an
// episode end (:664). No draws: the exploration is in the noisy layers' effective weights, fixed between two
// learns. The simplest shape (tools/variants/qnet_uniform_waves.patch for the DQN): every wave forwards its
// own 64 envs from their rows of the block's observation tile, steps them, and writes the new observations
// back into those rows; the packed net sits in LDS once per block and no wave waits for another after the
// copy. The net and the tile (74,192 + 20,480 B) leave room for one block per CU.
constexpr int kRbThreads = 512;  // envs per block, one per thread

struct RbRollout {
  mg_params P;
  Reset0 R0;
  mg_state S;
  mg_traj T;
  mg_stats St;
  const uint8_t* net;
  int64_t n;
  int32_t num_steps;
  uint32_t flags;
};

// OPP 0: a2 = None, the env's own L0 opponent; OPP 2: the same net on the view rotated by three.
template <int OPP>
__global__ __launch_bounds__(kRbThreads) void rainbow_rollout_kernel(const RbRollout R) {
  static_assert(OPP == 0 || OPP == 2, "opponent modes: 0 (None) and 2 (the same net)");
  __shared__ __attribute__((aligned(16))) uint8_t lds_net[kRbNetBytes];
  __shared__ __attribute__((aligned(16))) float tile[kRbThreads * kObs];
  const mg_params& P = R.P;
  const int tid = threadIdx.x;
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kRbThreads;
  const int64_t i = base + tid;
  const bool live = i < R.n;
  const int64_t wbase = base + (tid & ~63);
  const int64_t wrem = R.n - wbase;
  const int wrows = wrem <= 0 ? 0 : (wrem < 64 ? static_cast<int>(wrem) : 64);
  const bool autoreset = (R.flags & MG_AUTORESET) != 0;
  float* wtile = tile + (tid & ~63) * kObs;

  rainbow_to_lds(R.net, lds_net);
  Env e;
  EpStats sreg;
  {  // the observation the first step acts on, into the env's tile row (zeros past n)
    double o[kObs];
    if (live) {
      e = load_env(R.S, i);
      stats_load(R.St, i, sreg);
      double x1, y1, x2, y2;
      lon2coord(P, e.p1, true, x1, y1);
      lon2coord(P, e.p2, false, x2, y2);
      observe(P, e.p1, e.v1, e.p2, e.v2, x1, y1, x2, y2, o);
    } else {
#pragma unroll
      for (int k = 0; k < kObs; ++k) o[k] = 0.0;
    }
    put_obs_row(wtile + (tid & 63) * kObs, o);
  }
  __syncthreads();  // the net in LDS (and every wave's rows, which only that wave reads)
  bool won = false;
  for (int t = 0; t < R.num_steps; ++t) {
    float q[kRbActions];
    int a1, a2 = MG_ACTION_NONE;
    rainbow_forward_wave(lds_net, wtile, 0, q, a1, nullptr, 0);
    if constexpr (OPP == 2) rainbow_forward_wave(lds_net, wtile, 3, q, a2, nullptr, 0);
    wave_lds_sync();  // every read of the wave's rows precedes the writes below
    StepOut r;
    const int64_t row = static_cast<int64_t>(t) * R.n + i;
    if (live) {
      env_step<false>(P, e, a1, a2, r);  // an argmax over five actions is always valid: the unchecked step
      if (R.T.rew)
        st_out(reinterpret_cast<f32x2*>(R.T.rew) + row, f32x2{static_cast<float>(r.r1), static_cast<float>(r.r2)});
      store_step_bytes(R.T, row, a1, a2, r.done, r.coll);
      won = e.winner == 1;
      after_step(P, e, r, R.St, R.T.final_obs ? R.T.final_obs + row * kObs : nullptr, i, autoreset, &sreg, &R.R0);
    } else {
#pragma unroll
      for (int k = 0; k < kObs; ++k) r.o[k] = 0.0f;
    }
    store_won_mask(R.T.won_mask, won, t, R.n, wbase, wrows);
    // the new observations into the wave's rows (the next forward's input) and out
    wave_store_obs(wtile, r.o, R.T.obs ? R.T.obs + (static_cast<int64_t>(t) * R.n + wbase) * kObs : nullptr, wrows);
  }
  if (live) {
    store_env(R.S, i, e);
    stats_store(R.St, i, sreg);
  }
}

}  // namespace
