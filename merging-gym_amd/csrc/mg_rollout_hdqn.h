// mg_rollout_hdqn.h -- the h-DQN acting loop: HRollout, fresh_goal_words, hdqn_rollout_kernel.
// A part of the one translation unit merging_hip.hip (see its head comment).
#pragma once

#include "mg_common.h"
#include "mg_env.h"
#include "mg_qnet.h"
#include "mg_rollout_qnet.h"
#include "mg_stats.h"
#include "mg_wave_out.h"

namespace {

// ============================================================================ h-DQN acting loop
// hdqn.py's inner loop (scripts/hdqn.py:280-323) in one launch: Goal_DQN's meta-net picks the
// sub-goal on every next state (:303), the lower-level Net acts on the goal state
// [goal] + state (:291-292), goal_status (:223-237) gives the intrinsic reward (:314) and ends
// the inner loop (:320-322), after which -- and after every episode end (:278-283, the outer
// loops) -- a fresh goal is chosen. Both nets live in LDS (compact packing, 2 x 60.5 KB).
//
// OPP 2 is hdqn.py's Strategy_OP "selfplay" (:262-264, upper_op = upper, lower_op = lower): the
// same two nets also choose the opponent's goal on the swapped state at every outer-loop
// iteration (:285) and its action on [goal_op] + swapped state (:299-300), two more forwards per
// phase on the Q-net waves.
// Per env-step k (global step index) the Philox4x32-10 streams are
//   A = Philox(counter (gi, k)):            x ego explore draw, y ego random action,
//                                           z goal explore draw, w random goal (the goal
//                                           chosen on the step's next state, :303)
//   B = Philox(counter (gi ^ 2^63, k)):     x, y the same for a fresh goal (after a goal was
//                                           reached or the episode ended, :283), z the uniform
//                                           opponent's action (opponent_mode 1)
//   C = Philox(counter (gi ^ 2^62, k)):     (OPP 2) x explore, y action of the opponent's
//                                           step, z explore, w goal of its fresh goal at k + 1
// and a launch whose env has no goal yet (goal[i] < 0) starts it with B of step first_step - 1.
// Roles as in qnet_rollout_ws_kernel: waves 0-3 run both nets (meta then lower, one 64-env tile
// each per phase), waves 4-7 the fp64 env step (one env per lane), on two groups of 256 envs
// pipelined over 2T + 2 phases: Q(A,0) | Q(B,0) + E(A,0) | ... | Q(A,T) + E(B,T-1) | Q(B,T).
// Q(X,t) finishes step t-1's goal logic (meta on its next state: the terminal observation where
// the episode ended, kept in LDS as bf16 pairs) and picks step t's action; E(X,t) steps.
struct HRollout {
  mg_params P;
  Reset0 R0;
  mg_state S;
  mg_traj T;
  mg_hdqn_traj H;
  mg_stats St;
  int8_t* goal;     // [n] in / out
  int8_t* goal_op;  // [n] in / out, the self-play opponent's goal (OPP 2)
  double* ext_acc;  // [n] in / out, extrinsic reward since the inner loop began (Goal_DQN rows)
  const uint8_t* meta;
  const uint8_t* lower;
  const uint8_t* meta_op;   // OPP 3: the opponent's own nets, fragment-major (read from L2)
  const uint8_t* lower_op;
  uint64_t seed;
  uint64_t first_step;
  uint64_t greedy_thr;
  int64_t env_offset;
  int64_t n;
  int32_t num_steps;
  int32_t num_goals;
  int32_t reset_goal;
  uint32_t flags;
  // fused goal ring (hdqn.py:316 stores every transition, so slots need no scan): rows
  // [goal, s, a, r, next_goal, s'] of transition (t, i) at (counter0 + t n + i) % capacity
  float* ring;  // [capacity, 24] or NULL
  const uint64_t* ring_counter;
  int64_t ring_capacity;
};

constexpr int kHEnvs = 512;              // envs per block: two groups of 256
constexpr int kRowGoalF = 2 * kObs + 4;  // goal ring row floats (hdqn.py:158)
constexpr int kHHalf = kHEnvs / 2;
constexpr uint8_t kHGreedy = 0xFF;       // draw byte: take the greedy choice

__device__ __forceinline__ uint8_t draw_byte(uint32_t explore, uint32_t pick, uint64_t thr, int k) {
  return static_cast<uint8_t>(static_cast<uint64_t>(explore) < thr
                                  ? kHGreedy
                                  : (static_cast<uint64_t>(pick) * static_cast<uint64_t>(k)) >> 32);
}

// The fresh-goal draws (explore, goal) of step k from stream B (counter gi ^ 2^63). Every opponent
// but the uniform one uses two words of B per step, so one call serves two steps (ABI 20): call
// k div 2, words (x, y) on even steps and (z, w) on odd ones; `keep` carries the odd step's pair
// from the even step (fresh: compute the call, as at a launch's first step). The uniform opponent
// also draws its action from B (word z of call k), one call per step.
template <int OPP>
__device__ __forceinline__ uint2 fresh_goal_words(uint64_t gi, uint64_t k, uint64_t seed, bool fresh, uint2& keep,
                                                  uint32_t& opp_word) {
  if constexpr (OPP == 1) {
    const uint4 u = philox_env_step(gi ^ (uint64_t{1} << 63), k, seed);
    opp_word = u.z;
    return make_uint2(u.x, u.y);
  } else {
    opp_word = 0u;
    if ((k & 1) == 0 || fresh) {
      const uint4 u = philox_env_step(gi ^ (uint64_t{1} << 63), k >> 1, seed);
      keep = make_uint2(u.z, u.w);
      return (k & 1) ? keep : make_uint2(u.x, u.y);
    }
    return keep;
  }
}

// lower-net input of one env: goal state [goal] + state (hdqn.py:291), features 0..10, zero at
// 11..12 and the bias inputs 1.0 at 13..15; swap: [goal] + state[5:] + state[:5] (the
// opponent's goal state, :299)
__device__ __forceinline__ bf16x8 qnet_input_goal(const float* row, int goal, int h, bool swap = false) {
  float v[kObs];
#pragma unroll
  for (int k = 0; k < kObs / 2; ++k) {
    const f32x2 t = reinterpret_cast<const f32x2*>(row)[k];
    // swapped view state[5:] + state[:5]: pair (4, 5) straddles the halves, so each element
    // takes its own destination (element 5 -> v[0], element 4 -> v[9])
    const int d0 = swap ? (2 * k + kObs / 2) % kObs : 2 * k;
    const int d1 = swap ? (2 * k + 1 + kObs / 2) % kObs : 2 * k + 1;
    v[d0] = t[0];
    v[d1] = t[1];
  }
  auto pk = [](float a, float b) { return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{a, b}, bf16x2)); };
  const u32x4 w = h ? u32x4{pk(v[7], v[8]), pk(v[9], 0.f), 0x3F800000u, 0x3F803F80u}
                    : u32x4{pk(static_cast<float>(goal), v[0]), pk(v[1], v[2]), pk(v[3], v[4]), pk(v[5], v[6])};
  return __builtin_bit_cast(bf16x8, w);
}

// meta-net input of one env from its bf16-pair side row (the terminal observation)
__device__ __forceinline__ bf16x8 qnet_input_pairs(const uint32_t* side, int h) {
  return __builtin_bit_cast(bf16x8, h ? u32x4{side[4], 0u, 0x3F800000u, 0x3F803F80u}
                                      : u32x4{side[0], side[1], side[2], side[3]});
}

template <int OPP>
__global__ __launch_bounds__(512, 2) void hdqn_rollout_kernel(const HRollout R) {
  __shared__ __attribute__((aligned(16))) uint8_t lds_meta[kQNetBytes];
  __shared__ __attribute__((aligned(16))) uint8_t lds_lower[kQNetBytes];
  __shared__ __attribute__((aligned(16))) float tile[kHEnvs * kObs];    // s' (reset obs where done)
  __shared__ __attribute__((aligned(16))) uint32_t side[kHEnvs * 5];    // terminal obs, bf16 pairs
  __shared__ uint8_t b_act[kHEnvs], b_goal[kHEnvs], b_done[kHEnvs], b_st_old[kHEnvs],
      b_st_new[kHEnvs], b_dg[kHEnvs], b_df[kHEnvs], b_g2[kHEnvs];
  // OPP 2 / 3: the opponent's greedy action, current goal and fresh-goal draw
  constexpr bool kOpNets = OPP >= 2;  // the opponent acts through h-DQN nets
  __shared__ uint8_t b_aop[kOpNets ? kHEnvs : 1], b_gop[kOpNets ? kHEnvs : 1], b_dfo[kOpNets ? kHEnvs : 1];
  // the opponent meta-net's compacted items per Q-net wave and their goals (round 5)
  __shared__ uint8_t b_olist[kOpNets ? 4 : 1][64], b_gos[kOpNets ? kHEnvs : 1];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kHEnvs;
  const int T = R.num_steps;
  const int phases = 2 * T + 2;
  {
    const f32x4* s1 = reinterpret_cast<const f32x4*>(R.meta);
    const f32x4* s2 = reinterpret_cast<const f32x4*>(R.lower);
    f32x4* d1 = reinterpret_cast<f32x4*>(lds_meta);
    f32x4* d2 = reinterpret_cast<f32x4*>(lds_lower);
    for (int j = tid; j < kQNetBytes / 16; j += blockDim.x) {
      d1[j] = s1[j];
      d2[j] = s2[j];
    }
  }
  if (wave < 4) {
    // ---------------------------------------------------------------- the two nets
    __syncthreads();
    const int r = lane & 31, h = lane >> 5;
    for (int p = 0; p < phases; ++p) {
      const int g = p & 1, t = p >> 1;
      const int row0 = g * kHHalf + 64 * wave;  // this wave's 64 envs: rows row0 + lane
      const int j = row0 + lane;
      const int64_t i = base + j;
      const bool live = i < R.n;
      // This env's bytes for the phase, read together before the meta forward and held across it
      // (round 5: read where used, after the forward, each put an LDS round trip on the Q-net
      // waves' chain -- the goal logic took ~1.1 k cycles per phase, tools/clk_segments.py)
      const int goal_prev = static_cast<int8_t>(b_goal[j]);
      const int dg = b_dg[j], df = b_df[j], st_new = b_st_new[j], st_old = b_st_old[j];
      const bool done = t > 0 && b_done[j] != 0;
      int gop_prev = 0, dfo = 0;
      if constexpr (kOpNets) {
        gop_prev = static_cast<int8_t>(b_gop[j]);
        dfo = b_dfo[j];
      }
      int goal_t;
      const bool need_meta = t > 0 || __ballot(live && goal_prev < 0) != 0;
      int gstar = 0;
      float qe = 0.f;  // meta_eval_net(terminal state)[goal chosen on it], logged at an episode end (:330)
      if (need_meta) {  // meta-net on the next state of step t - 1 (on s_0 for a launch's first goals)
        // both sources read at once, the terminal observation's bf16 pairs chosen where the episode
        // ended (one LDS round trip, not the done byte's and then the row's)
        const bool d0 = t > 0 && b_done[row0 + r], d1 = t > 0 && b_done[row0 + 32 + r];
        const bf16x8 p0 = qnet_input_pairs(side + (row0 + r) * 5, h), p1 = qnet_input_pairs(side + (row0 + 32 + r) * 5, h);
        const bf16x8 o0 = qnet_input(tile + (row0 + r) * kObs, false, h);
        const bf16x8 o1 = qnet_input(tile + (row0 + 32 + r) * kObs, false, h);
        const bf16x8 x0 = d0 ? p0 : o0, x1 = d1 ? p1 : o1;
        // the bytes above arrive with the inputs (one wait), not after the forward
        asm volatile("" ::"v"(dg), "v"(df), "v"(st_new), "v"(st_old), "v"(gop_prev), "v"(dfo));
        float q[8];
        qnet_mlp_swp(lds_meta, x0, x1, q);
        gstar = argmax_first(q, R.num_goals);
        const int g2 = dg == kHGreedy ? gstar : dg;
#pragma unroll
        for (int k = 0; k < 8; ++k) qe = k == g2 ? q[k] : qe;
      }
      bool brk = false;  // step t - 1 left the inner loop (:322): a new outer iteration starts
      if (t > 0) {  // hdqn.py:303-322 for step t - 1
        const int goal2 = dg == kHGreedy ? gstar : dg;
        brk = done || goal2 == st_new;
        goal_t = done ? (df == kHGreedy ? R.reset_goal : df) : (brk ? (df == kHGreedy ? gstar : df) : goal2);
        if (live) {
          const int64_t row = static_cast<int64_t>(t - 1) * R.n + i;
          if (R.H.next_goal) st_out(R.H.next_goal + row, static_cast<float>(goal2));
          if (R.H.reward) st_out(R.H.reward + row, goal2 == st_old ? 1.0f : 0.0f);
        }
        b_g2[j] = static_cast<uint8_t>(goal2);  // for the fused ring row of step t - 1
        // the episode's q_eval (hdqn.py:330): the env wave recorded the episode in E(X, t - 1); this
        // lane is the only writer of the field, so no-return atomics keep the adds in step order
        if (done && live) add_q_eval_nowait(R.St, i, static_cast<double>(qe));
      } else {
        goal_t = goal_prev >= 0 ? goal_prev : (df == kHGreedy ? gstar : df);
      }
      int gop_t = 0;
      if constexpr (kOpNets) {  // upper_op.choose_goal(swapped state) at a new outer iteration (:285)
        const bool fresh_op = t > 0 ? brk : gop_prev < 0;
        // Only where the reference evaluates it (round 5): at a new outer iteration, on the greedy
        // branch (:86-92) -- about a quarter of the envs. The wave's items are compacted into one
        // forward on 32 envs (two column tiles) when they fit, else the full 64; the other passes
        // run at three quarters or more and stay uncompacted (a forward's weight stream costs as
        // much as two column tiles, so a narrower pass than two tiles' saving does not pay).
        const bool need_o = live && fresh_op && dfo == kHGreedy;
        const uint64_t mo = __ballot(need_o);
        int gop_star = 0;
        if (mo != 0) {  // on the state acted on at step t (reset obs after an end)
          const int L = __popcll(mo);
          uint8_t* list = b_olist[wave];
          if (need_o) list[lane_rank(mo)] = static_cast<uint8_t>(lane);
          wave_lds_sync();
          const int ea = list[r < L ? r : 0], ec = list[32 + r < L ? 32 + r : 0], eo = list[lane < L ? lane : 0];
          float q[8];
          const bf16x8 x0 = qnet_input(tile + (row0 + ea) * kObs, true, h);
          const bf16x8 x1 = qnet_input(tile + (row0 + ec) * kObs, true, h);
          if constexpr (OPP == 3) {  // the opponent's own Goal_DQN (:267)
            if (L <= 32)
              qnet_mlp<2 * kQGlobalAhead, 2>(qnet_global(R.meta_op), x0, x1, q);
            else
              qnet_mlp<kQGlobalAhead>(qnet_global(R.meta_op), x0, x1, q);
          } else {
            if (L <= 32)
              qnet_mlp<2 * kQLdsAhead, 2>(qnet_lds(lds_meta), x0, x1, q);
            else
              qnet_mlp_swp(lds_meta, x0, x1, q);
          }
          if (lane < L) b_gos[row0 + eo] = static_cast<uint8_t>(argmax_first(q, R.num_goals));
          wave_lds_sync();
          gop_star = b_gos[j];  // this env's item where need_o
        }
        gop_t = fresh_op ? (dfo == kHGreedy ? gop_star : dfo) : gop_prev;
      }
      if (t < T) {
        b_goal[j] = static_cast<uint8_t>(goal_t);
        if (live && R.H.goal) st_out(R.H.goal + static_cast<int64_t>(t) * R.n + i, static_cast<float>(goal_t));
        if constexpr (kOpNets) {
          b_gop[j] = static_cast<uint8_t>(gop_t);
          if (live && R.H.goal_op) st_out(R.H.goal_op + static_cast<int64_t>(t) * R.n + i, static_cast<float>(gop_t));
        }
        wave_lds_sync();  // the wave's goals are in LDS before the lanes read their column envs'
        const bf16x8 xe0 = qnet_input_goal(tile + (row0 + r) * kObs, b_goal[row0 + r], h);
        const bf16x8 xe1 = qnet_input_goal(tile + (row0 + 32 + r) * kObs, b_goal[row0 + 32 + r], h);
        // the opponent's inputs too, before the ego's forward (held across it)
        bf16x8 xo0 = xe0, xo1 = xe1;
        if constexpr (kOpNets) {
          xo0 = qnet_input_goal(tile + (row0 + r) * kObs, b_gop[row0 + r], h, true);
          xo1 = qnet_input_goal(tile + (row0 + 32 + r) * kObs, b_gop[row0 + 32 + r], h, true);
        }
        float q[8];
        qnet_mlp_swp(lds_lower, xe0, xe1, q);
        b_act[j] = static_cast<uint8_t>(argmax_first(q, MG_NUM_ACTIONS));
        if constexpr (kOpNets) {  // lower_op.choose_action([goal_op] + swapped state) (:299-300)
          float qo[8];
          const bf16x8 x0 = xo0, x1 = xo1;
          if constexpr (OPP == 3)
            qnet_mlp<kQGlobalAhead>(qnet_global(R.lower_op), x0, x1, qo);  // the opponent's own HDQN (:268)
          else
            qnet_mlp_swp(lds_lower, x0, x1, qo);
          b_aop[j] = static_cast<uint8_t>(argmax_first(qo, MG_NUM_ACTIONS));
        }
      } else if (live) {
        R.goal[i] = static_cast<int8_t>(goal_t);  // the next launch's starting goal
        if constexpr (kOpNets) R.goal_op[i] = static_cast<int8_t>(gop_t);
      }
      __syncthreads();
    }
    return;
  }
  // ------------------------------------------------------------------ the env step
  const int ew = wave - 4;
  Env e[2];
  bool live[2];
  double pend[2] = {0.0, 0.0};  // main.py's pending values (pend_load, after_step_nowait)
  int stc[2];  // goal_status of each group's current state, from its fp64 dx1 and v2
  // the fused ring row of each group's last step, completed once the Q-net waves have chosen
  // its next goal: s, s' (terminal where done), goal, action
  float ps[2][kObs], ps2[2][kObs];
  int pgoal[2], pact[2];
  // Goal_DQN's memory (hdqn.py:286, :311-313, :322, :325): the extrinsic reward since each env's
  // inner loop began, and at each step whether that loop ended (known once Q(X, t + 1) has chosen
  // the step's next goal, so it is emitted together with the ring row of the step)
  // kept whenever the caller holds the running sums (ext_acc), so turning ext_reward / no_break
  // on in a later launch continues the loops already in flight correctly
  const bool outer = R.ext_acc != nullptr;
  double acc[2] = {0.0, 0.0};
  uint2 kb[2] = {make_uint2(0u, 0u), make_uint2(0u, 0u)};  // each group's odd-step fresh-goal words
  auto finish_outer = [&](int g, int t, double& ac) __attribute__((always_inline)) {
    const int j = g * kHHalf + 64 * ew + lane;
    const int64_t i = base + j;
    const int64_t wbase = base + g * kHHalf + 64 * ew;
    const bool lv = i < R.n;
    const bool brk = b_done[j] != 0 || b_g2[j] == b_st_new[j];
    if (R.H.ext_reward && lv) st_out(R.H.ext_reward + static_cast<int64_t>(t) * R.n + i, static_cast<float>(ac));
    if (R.H.no_break) {
      const uint64_t m = __ballot(lv && !brk);
      if (lane == 0 && wbase < R.n) st_out(R.H.no_break + static_cast<int64_t>(t) * ((R.n + 63) >> 6) + (wbase >> 6), m);
    }
    if (brk) ac = 0.0;  // :286 extrinsic_reward = 0 for the next outer iteration
  };
  const bool ring = R.ring != nullptr;
  const uint64_t c0 = ring ? *R.ring_counter : 0;
  const int64_t total = static_cast<int64_t>(T) * R.n;
  auto write_row = [&](int g, int t, const float (&s0)[kObs], const float (&s1)[kObs], int pg,
                       int pa) __attribute__((always_inline)) {
    const int j = g * kHHalf + 64 * ew + lane;
    const int64_t i = base + j;
    const int64_t k = static_cast<int64_t>(t) * R.n + i;  // transition index within the launch
    if (!ring || i >= R.n || k < total - R.ring_capacity) return;  // the newest capacity rows only
    const int goal2 = b_g2[j];
    const int st_old = b_st_old[j];
    float* row = R.ring + static_cast<int64_t>((c0 + static_cast<uint64_t>(k)) %
                                               static_cast<uint64_t>(R.ring_capacity)) * kRowGoalF;
    f32x4 v[6];
    float f[kRowGoalF];
    f[0] = static_cast<float>(pg);
#pragma unroll
    for (int q = 0; q < kObs; ++q) f[1 + q] = s0[q];
    f[11] = static_cast<float>(pa);
    f[12] = goal2 == st_old ? 1.0f : 0.0f;
    f[13] = static_cast<float>(goal2);
#pragma unroll
    for (int q = 0; q < kObs; ++q) f[14 + q] = s1[q];
#pragma unroll
    for (int q = 0; q < 6; ++q) v[q] = f32x4{f[4 * q], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3]};
#pragma unroll
    for (int q = 0; q < 6; ++q) st_out(reinterpret_cast<f32x4*>(row) + q, v[q]);
  };
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const int j = g * kHHalf + 64 * ew + lane;
    const int64_t i = base + j;
    live[g] = i < R.n;
    double o[kObs];
    if (live[g]) {
      e[g] = load_env(R.S, i);
      pend[g] = pend_load(R.St, i, e[g]);
      double x1, y1, x2, y2;
      lon2coord(R.P, e[g].p1, true, x1, y1);
      lon2coord(R.P, e[g].p2, false, x2, y2);
      observe(R.P, e[g].p1, e[g].v1, e[g].p2, e[g].v2, x1, y1, x2, y2, o);
    } else {  // a defined state, stepped but never stored
      e[g].p1 = e[g].p2 = R.P.start_point;
      e[g].v1 = e[g].v2 = R.P.start_vel;
      e[g].ret1 = e[g].ret2 = 0.0;
      e[g].steps = 0;
      e[g].winner = 0;
      e[g].done = false;
#pragma unroll
      for (int k = 0; k < kObs; ++k) o[k] = 0.0;
    }
    stc[g] = goal_status(o[0], o[9]);
    float2* t2 = reinterpret_cast<float2*>(tile + j * kObs);
#pragma unroll
    for (int k = 0; k < kObs / 2; ++k) t2[k] = make_float2(static_cast<float>(o[2 * k]), static_cast<float>(o[2 * k + 1]));
    const uint64_t gi = static_cast<uint64_t>(R.env_offset + i);
    uint2 unused_keep;
    uint32_t unused_word;
    const uint2 fb = fresh_goal_words<OPP>(gi, R.first_step - 1, R.seed, true, unused_keep, unused_word);
    b_df[j] = draw_byte(fb.x, fb.y, R.greedy_thr, R.num_goals);
    b_goal[j] = live[g] ? static_cast<uint8_t>(R.goal[i]) : 0;
    if (outer && live[g]) acc[g] = R.ext_acc[i];
    if constexpr (kOpNets) {
      const uint4 fc = philox_env_step(gi ^ (uint64_t{1} << 62), R.first_step - 1, R.seed);
      b_dfo[j] = draw_byte(fc.z, fc.w, R.greedy_thr, R.num_goals);
      b_gop[j] = live[g] ? static_cast<uint8_t>(R.goal_op[i]) : 0;
    }
    b_done[j] = 0;
  }
  __syncthreads();
  for (int p = 0; p < phases; ++p) {
    if (p > 0 && ((p - 1) >> 1) < T) {
      const int g = (p - 1) & 1, t = (p - 1) >> 1;
      const int j = g * kHHalf + 64 * ew + lane;
      const int64_t i = base + j;
      const int64_t wbase = base + g * kHHalf + 64 * ew;
      const uint64_t gi = static_cast<uint64_t>(R.env_offset + i), k = R.first_step + t;
      const uint4 ua = philox_env_step(gi, k, R.seed);
      uint32_t opp_word;
      const uint2 ub = g == 0 ? fresh_goal_words<OPP>(gi, k, R.seed, t == 0, kb[0], opp_word)
                              : fresh_goal_words<OPP>(gi, k, R.seed, t == 0, kb[1], opp_word);
      const int a1 = static_cast<uint64_t>(ua.x) < R.greedy_thr ? static_cast<int>(b_act[j]) : action_from_u32(ua.y);
      int a2 = OPP == 1 ? action_from_u32(opp_word) : MG_ACTION_NONE;
      uint4 uc = make_uint4(0u, 0u, 0u, 0u);
      if constexpr (kOpNets) {  // the self-play opponent's epsilon-greedy action (:300)
        uc = philox_env_step(gi ^ (uint64_t{1} << 62), k, R.seed);
        a2 = static_cast<uint64_t>(uc.x) < R.greedy_thr ? static_cast<int>(b_aop[j]) : action_from_u32(uc.y);
      }
      if (t > 0) {  // step t - 1's next goal is in LDS now (Q(X, t)); wave-uniform branch per group
        if (g == 0)
          write_row(0, t - 1, ps[0], ps2[0], pgoal[0], pact[0]);
        else
          write_row(1, t - 1, ps[1], ps2[1], pgoal[1], pact[1]);
        if (outer) {
          if (g == 0)
            finish_outer(0, t - 1, acc[0]);
          else
            finish_outer(1, t - 1, acc[1]);
        }
      }
      auto step = [&](Env& ev, bool lv, float (&s0)[kObs], float (&s1)[kObs], int& pg, int& pa, double& ac,
                      int& st, double& pd) __attribute__((always_inline)) {
        StepOut rv;  // per step: the state acted on is the env's tile row, so no observation is carried
        b_st_old[j] = static_cast<uint8_t>(st);  // status of the state acted on (:314)
        if (ring) {
          const f32x2* trow = reinterpret_cast<const f32x2*>(tile + j * kObs);
#pragma unroll
          for (int q = 0; q < kObs / 2; ++q) {
            const f32x2 v = trow[q];
            s0[2 * q] = v[0];
            s0[2 * q + 1] = v[1];
          }
          pg = b_goal[j];
          pa = a1;
        }
        // every action here is in action_dict: the lower nets' argmax runs over the first
        // NUM_ACTIONS outputs, the random draws are 0..4, so the step needs no KeyError path
        env_step<false>(R.P, ev, a1, a2, rv);
        ac += rv.r1;  // :311-313 extrinsic_reward += reward
        if (ring) {
#pragma unroll
          for (int q = 0; q < kObs; ++q) s1[q] = static_cast<float>(rv.o[q]);  // terminal where done
        }
        const int64_t row = static_cast<int64_t>(t) * R.n + i;
        if (lv) {
          if (R.T.rew) st_out(reinterpret_cast<f32x2*>(R.T.rew) + row, f32x2{static_cast<float>(rv.r1), static_cast<float>(rv.r2)});
          store_step_bytes(R.T, row, a1, a2, rv.done, rv.coll);
        }
        b_done[j] = rv.done ? 1 : 0;
        st = goal_status(rv.dx1, ev.v2);  // of the next state (:322), terminal where done
        b_st_new[j] = static_cast<uint8_t>(st);
        b_dg[j] = draw_byte(ua.z, ua.w, R.greedy_thr, R.num_goals);
        b_df[j] = draw_byte(ub.x, ub.y, R.greedy_thr, R.num_goals);
        if constexpr (kOpNets) b_dfo[j] = draw_byte(uc.z, uc.w, R.greedy_thr, R.num_goals);
        const bool won = lv && ev.winner == 1;
        const int64_t rem = R.n - wbase;
        store_won_mask(R.T.won_mask, won, t, R.n, wbase, rem <= 0 ? 0 : (rem < 64 ? static_cast<int>(rem) : 64));
        if (lv && (R.flags & MG_AUTORESET) && rv.done) {
          uint32_t* sd = side + j * 5;  // the terminal observation for the meta-net
#pragma unroll
          for (int q2 = 0; q2 < kObs / 2; ++q2)
            sd[q2] = __builtin_bit_cast(uint32_t, __builtin_convertvector(
                                                      f32x2{static_cast<float>(rv.o[2 * q2]), static_cast<float>(rv.o[2 * q2 + 1])}, bf16x2));
          after_step_nowait(R.P, ev, rv, R.St, R.T.final_obs ? R.T.final_obs + row * kObs : nullptr, i, true, pd,
                            &R.R0);
          st = goal_status(rv.dx1, ev.v2);  // the reset state the next step acts on
        } else if (lv) {
          after_step_nowait(R.P, ev, rv, R.St, nullptr, i, false, pd, &R.R0);  // the first arrival, if any
        }
        const int64_t wrem = R.n - wbase;
        wave_store_obs(tile + (g * kHHalf + 64 * ew) * kObs, rv.o,
                       R.T.obs ? R.T.obs + (static_cast<int64_t>(t) * R.n + wbase) * kObs : nullptr,
                       wrem <= 0 ? 0 : (wrem < 64 ? static_cast<int>(wrem) : 64));
      };
      if (g == 0)
        step(e[0], live[0], ps[0], ps2[0], pgoal[0], pact[0], acc[0], stc[0], pend[0]);
      else
        step(e[1], live[1], ps[1], ps2[1], pgoal[1], pact[1], acc[1], stc[1], pend[1]);
    }
    __syncthreads();
  }
  // both groups' last rows: Q(A,T) and Q(B,T) chose their next goals in the last two phases
  write_row(0, T - 1, ps[0], ps2[0], pgoal[0], pact[0]);
  write_row(1, T - 1, ps[1], ps2[1], pgoal[1], pact[1]);
  if (outer) {
    finish_outer(0, T - 1, acc[0]);
    finish_outer(1, T - 1, acc[1]);
#pragma unroll
    for (int g = 0; g < 2; ++g)
      if (live[g]) R.ext_acc[base + g * kHHalf + 64 * ew + lane] = acc[g];
  }
#pragma unroll
  for (int g = 0; g < 2; ++g)
    if (live[g]) store_env(R.S, base + g * kHHalf + 64 * ew + lane, e[g]);
}

}  // namespace
