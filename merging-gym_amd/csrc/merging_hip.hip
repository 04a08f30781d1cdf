// merging_hip.hip — batched MergingEnv step for MI355X (gfx950, CDNA4).
//
// One thread owns one env. The env batch lives in HBM as a struct of arrays
// (include/merging_hip.h: mg_state); a step streams every array once in and once out,
// so the kernel is bound by HBM bandwidth, not by arithmetic (no contraction -> no MFMA).
//
// Reference being replaced (all paths relative to YikangZhang1641/merging-gym):
//   MergeEnv.step            merging_gym/envs/merging_env.py:138-195
//   MergeEnv.action_to_acc   merging_env.py:134-136  -> scripts/helper.py:152-191 mpc_1d
//   MergeEnv.observe         merging_env.py:118-132  -> lon2coord :48-58
//   MergeEnv.is_collided     merging_env.py:198-206  -> corners :232-239 (pygame Rect / Vector2,
//                                                        shapely Polygon.intersects)
//   MergeEnv.reset           merging_env.py:208-230
//
// Numerics: fp64 throughout, IEEE add/mul/div without contraction (the file is compiled
// with -ffp-contract=off and the pragma below), so positions, speeds, arrival tests and
// rewards are the same doubles the reference's Python floats hold (mpc_1d's first control
// carries the QP solver's own rounding, see mpc_acc). sin/cos: for |theta| < 1/16 (both cars
// up to END_POINT) a degree-9/10 Taylor polynomial in fma form, identical to glibc's
// sin/cos in 99.98 % of 2e7 samples and otherwise 1 ulp off; larger angles, which live episodes
// do reach once a car has arrived, use the device math library (<= 1 ulp). Every other
// operation is correctly rounded.
//
// One translation unit in parts, one subsystem each. Every part includes what it uses and compiles
// on its own; this file includes them in the order that fixes the kernels' order in the code object,
// and keeps only the C entry points (include/merging_hip.h): a call's checks, fill and launches are in its part.
#pragma clang fp contract(off)

#include "mg_common.h"          // block size, MG_HD, vector types, st_out / st_state
#include "mg_env.h"             // the fp64 env step host and device share, Philox and the action draws
#include "mg_stats.h"           // episode statistics of one env
#include "mg_wave_out.h"        // a wave's outputs: LDS-staged observations, won mask, step bytes
#include "mg_step.h"            // step_kernel, rollout_kernel
#include "mg_qnet.h"            // the bf16 MFMA Q-net: pack kernels, forwards
#include "mg_rainbow.h"         // Rainbow's acting net: pack kernel, MFMA forward, the fp32 head
#include "mg_rollout_qnet.h"    // config 5: qnet_rollout_ws_kernel, lone and with the member in the grid, their host side
#include "mg_rollout_hdqn.h"    // the h-DQN acting loop: hdqn_rollout_kernel
#include "mg_rollout_rainbow.h" // Rainbow's acting loop: rainbow_rollout_kernel, lone and with the member in the grid
#include "mg_reset_observe.h"   // reset_kernel, observe_kernel
#include "mg_replay.h"          // the replay ring: scan, write and sample kernels, counter_add_kernel, the stores' host side
#include "mg_launch.h"          // error text, armed events, argument checks, launch helpers
#include "mg_mpc_qp.h"          // mpc_qp_constants (host only)
#include "mg_stats_reduce.h"    // the fixed-order statistics reduction, goal_status_kernel
#include "mg_host_env.h"        // the CPU single-env path
#include "mg_learn_core.h"      // the fixed-order fp32 primitives both learners share, learn_bwd_kernel
#include "mg_learn.h"           // DQN.learn, lone and population: the update kernels with the member in the grid,
                                // their launch order, host twin and the drivers of a call
#include "mg_per.h"             // prioritized replay alone: the sum / min trees, pow, store, sample, update
#include "mg_rainbow_learn.h"   // Rainbow's compute_td_loss, plain or prioritized: replay stores, update kernels,
                                // the launch order, host twin and the drivers of a call
#include "mg_rainbow_noise.h"   // the learner's noise factors drawn on the device: Philox, inverse normal CDF, host twin

extern "C" {

int mg_abi_version(void) { return MG_ABI_VERSION; }


int mg_time_next_launch(void* start_event, void* stop_event) {
  g_ev_start = static_cast<hipEvent_t>(start_event);
  g_ev_stop = static_cast<hipEvent_t>(stop_event);
  return 0;
}

const char* mg_last_error(void) { return g_err; }

// The compiler that built this library (its hipcc version decides the inline-asm permlane hazard
// padding of qnet_gather_q, which hipcc 7.2's builtins miscompiled): printed in the GPU test log
// header and the bench line.
#ifndef MG_SRC_SHA
#define MG_SRC_SHA "unknown"  // merging_gym/build.py passes the sha256 of source + header + flags
#endif
const char* mg_build_info(void) {
  return "clang " __clang_version__ "; HIP " MG_STR(HIP_VERSION_MAJOR) "." MG_STR(HIP_VERSION_MINOR) "."
         MG_STR(HIP_VERSION_PATCH) "; ABI " MG_STR(MG_ABI_VERSION) "; gfx950, -ffp-contract=off; src " MG_SRC_SHA;
}

void mg_params_default(mg_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->R = 30000.0;
  p->H = 1000.0;
  p->W = 300.0;
  p->dT = 0.2;
  p->r_first = 2.0;
  p->r_second = 1.0;
  p->r_collision = -10.0;
  p->vel_penalty = 0.001;
  p->time_penalty = 0.0;
  p->start_point = 50.0;
  p->end_point = 950.0;
  p->start_vel = 20.0;
  p->vel_ref = 20.0;
  p->prediction_t = 3.0;
  volatile double h = 1000.0, r = 30000.0;  // libm at run time, as np.arctan2 does
  p->angle0 = std::atan2(h, r);                 // merging_env.py:49
  for (int k = 0; k < MG_NUM_ACTIONS; ++k) p->action_speed[k] = 10.0 * k;
  p->veh_w = 4;
  p->veh_h = 8;
  p->timeout_steps = 2501;
  p->inv_R = 1.0 / p->R;
  mpc_qp_constants(p->prediction_t, &p->qp_nz, &p->qp_z0, &p->qp_vsmall);
  p->qp_inv_nz = 1.0 / p->qp_nz;
}

int mg_goal_status(const double* dx1, const double* v2, int8_t* status, int64_t n, void* stream) {
  if (!dx1 || !v2 || !status) return fail(hipErrorInvalidValue, "%s", "mg_goal_status: NULL pointer");
  if (n < 0) return fail(hipErrorInvalidValue, "%s", "n < 0");
  if (n == 0) return 0;
  hipLaunchKernelGGL(goal_status_kernel, dim3(grid_blocks(n)), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), dx1, v2, status, n);
  return finish_launch("mg_goal_status");
}

int mg_step(const mg_params* params, const mg_state* state, const int8_t* a1, const int8_t* a2,
            const mg_outputs* out, const mg_stats* stats, int64_t n, uint32_t flags,
            void* stream) {
  if (int e = check_common(params, state, out, n)) return e;
  if (n == 0) return 0;
  if (!a1) return fail(hipErrorInvalidValue, "%s", "a1 is NULL");
  Launch L = make_launch(params, state, out, stats, n, flags);
  L.a1 = a1;
  L.a2 = a2;
  return launch_step<kActArrays>(L, static_cast<hipStream_t>(stream), "mg_step");
}

int mg_step_random(const mg_params* params, const mg_state* state, int8_t* a1_out,
                   int8_t* a2_out, const mg_outputs* out, const mg_stats* stats, int64_t n,
                   int64_t env_offset, uint64_t seed, uint64_t step_idx, int32_t opponent_random, uint32_t flags,
                   void* stream) {
  if (int e = check_common(params, state, out, n)) return e;
  if (n == 0) return 0;
  Launch L = make_launch(params, state, out, stats, n, flags);
  if (out->flags && (a1_out || a2_out))
    return fail(hipErrorInvalidValue, "%s", "flags records the actions: pass NULL a1_out / a2_out");
  L.a1_out = a1_out;
  L.a2_out = a2_out;
  L.seed = seed;
  L.step_idx = step_idx;
  L.env_offset = env_offset;
  L.opp_random = opponent_random;
  return launch_step<kActPhilox>(L, static_cast<hipStream_t>(stream), "mg_step_random");
}

int mg_rollout_random(const mg_params* params, const mg_state* state, const mg_traj* traj,
                      const mg_stats* stats, int64_t n, int64_t env_offset, uint64_t seed,
                      uint64_t first_step, int32_t num_steps, int32_t opponent_random,
                      uint32_t flags, void* stream) {
  if (int e = check_rollout_args(params, state, traj, n)) return e;
  if (num_steps < 0 || num_steps > 65535)
    return fail(hipErrorInvalidValue, "%s", "need 0 <= num_steps <= 65535 (split longer rollouts)");
  if (int e = check_traj(traj)) return e;
  if (n == 0 || num_steps == 0) return 0;
  Rollout R = make_rollout<Rollout>(params, state, traj, stats, seed, first_step, env_offset, n, num_steps, flags);
  R.opp_random = opponent_random;
  return launch_rollout(R, static_cast<hipStream_t>(stream));
}

size_t mg_qnet_packed_bytes(void) { return static_cast<size_t>(kQNetBytes + kQ32NetBytes); }

int mg_qnet_pack(const float* fc1_w, const float* fc1_b, const float* fc2_w, const float* fc2_b,
                 const float* out_w, const float* out_b, int32_t in_dim, int32_t out_dim,
                 void* packed, void* stream) {
  if (!fc1_w || !fc1_b || !fc2_w || !fc2_b || !out_w || !out_b || !packed)
    return fail(hipErrorInvalidValue, "%s", "mg_qnet_pack: NULL pointer");
  if (int e = check_net_dims("mg_qnet_pack", in_dim, out_dim)) return e;
  if (misaligned(packed, 15))
    return fail(hipErrorInvalidValue, "%s", "mg_qnet_pack: packed buffer must be 16-byte aligned");
  hipLaunchKernelGGL(qnet_pack_kernel, dim3(kQPackBlocks), dim3(kQPackBlock), 0,
                     static_cast<hipStream_t>(stream), fc1_w, fc1_b, fc2_w, fc2_b, out_w, out_b,
                     in_dim, out_dim, static_cast<uint8_t*>(packed));
  // the 32x32 layout behind it (qnet32_mlp: the config-5 kernel without a net opponent)
  hipLaunchKernelGGL(qnet32_pack_kernel, dim3(kQ32PackBlocks), dim3(kQPackBlock), 0,
                     static_cast<hipStream_t>(stream), fc1_w, fc1_b, fc2_w, fc2_b, out_w, out_b,
                     in_dim, out_dim, static_cast<uint8_t*>(packed) + kQNetBytes);
  return finish_launch("mg_qnet_pack");
}

size_t mg_qnet_fragment_bytes(void) { return static_cast<size_t>(kQNetBytes); }

int mg_qnet_fragments(const void* packed, void* fragments, void* stream) {
  if (!packed || !fragments) return fail(hipErrorInvalidValue, "%s", "mg_qnet_fragments: NULL pointer");
  if (misaligned(packed, 15) || misaligned(fragments, 15))
    return fail(hipErrorInvalidValue, "%s", "mg_qnet_fragments: buffers must be 16-byte aligned");
  hipLaunchKernelGGL(qnet_fragments_kernel, dim3(kQNetBytes / 1024), dim3(64), 0, static_cast<hipStream_t>(stream),
                     static_cast<const uint8_t*>(packed), static_cast<uint8_t*>(fragments));
  return finish_launch("mg_qnet_fragments");
}

int mg_qnet_forward(const void* packed, const float* x, int32_t in_dim, int32_t swap_halves, float* q,
                    int64_t n, void* stream) {
  if (!packed || !x || !q) return fail(hipErrorInvalidValue, "%s", "mg_qnet_forward: NULL pointer");
  if (n < 0) return fail(hipErrorInvalidValue, "%s", "n < 0");
  if (in_dim < 1 || in_dim > kQMaxIn || (swap_halves && in_dim != kObs))
    return fail(hipErrorInvalidValue, "%s", "mg_qnet_forward: need 1 <= in_dim <= 13 (swap_halves: in_dim 10)");
  if (int e = check_packed_net(packed, "packed net must be 16-byte aligned")) return e;
  if (n == 0) return 0;
  hipLaunchKernelGGL(qnet_forward_kernel, dim3(grid_blocks(n)), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), static_cast<const uint8_t*>(packed), x, in_dim,
                     swap_halves, q, n);
  return finish_launch("mg_qnet_forward");
}

int mg_rollout_qnet(const mg_params* params, const mg_state* state, const mg_traj* traj,
                    const mg_stats* stats, int64_t n, int64_t env_offset, uint64_t seed,
                    uint64_t first_step, int32_t num_steps, const void* net, int32_t out_dim,
                    uint64_t greedy_threshold, int32_t opponent_mode,
                    uint64_t opp_greedy_threshold, const void* opp_net, uint32_t flags, void* stream) {
  if (int e = check_rollout_args(params, state, traj, n)) return e;
  if (int e = check_packed_net(net, "net must be a 16-byte aligned packed Q-net")) return e;
  if (int e = check_qrollout_dims_mode(false, num_steps, out_dim, opponent_mode)) return e;
  if (opponent_mode == 3)
    if (int e = check_packed_net(opp_net, "opponent_mode 3 needs opp_net, a 16-byte aligned packed Q-net")) return e;
  if (int e = check_traj(traj)) return e;
  if (n == 0 || num_steps == 0) return 0;
  QRollout R = make_rollout<QRollout>(params, state, traj, stats, seed, first_step, env_offset, n, num_steps, flags);
  R.out_dim = out_dim, R.fin = finish_bound(*params);
  R.net = static_cast<const uint8_t*>(net), R.opp_net = static_cast<const uint8_t*>(opp_net);
  R.greedy_thr = greedy_threshold, R.opp_greedy_thr = opp_greedy_threshold;
  launch(qnet_rollout_instance<QRollout>(opponent_mode, out_dim > MG_NUM_ACTIONS), grid_blocks(n, kQWsEnvs), kQWsThreads,
         static_cast<hipStream_t>(stream), R);
  return finish_launch("mg_rollout_qnet");
}

int mg_rollout_qnet_many(const mg_params* params, const mg_state* state, const mg_traj* traj,
                         const mg_stats* stats, int64_t n_member, int32_t members, int64_t env_offset,
                         uint64_t first_step, int32_t num_steps, const mg_qnet_actor* actors, int32_t out_dim,
                         int32_t opponent_mode, uint32_t flags, void* stream) {
  const char* const who = "mg_rollout_qnet_many: %s";
  if (!members_ok(members)) return fail(hipErrorInvalidValue, who, "need 1 <= members <= 64");
  if (n_member < 0) return fail(hipErrorInvalidValue, who, "n_member < 0");
  if (n_member % 64 != 0)
    return fail(hipErrorInvalidValue, who,
                "n_member must be a multiple of 64 (a won-mask word covers 64 envs and is stored whole, so no "
                "two members may share one)");
  if (n_member > (static_cast<int64_t>(0x7fffffff) * kBlock) / members)
    return fail(hipErrorInvalidValue, who, "members * n_member exceeds the grid limit");
  const int64_t n = n_member * members;
  if (int e = check_rollout_args(params, state, traj, n)) return e;
  if (!actors) return fail(hipErrorInvalidValue, who, "actors is NULL (members mg_qnet_actor entries)");
  if (int e = check_qrollout_dims_mode(true, num_steps, out_dim, opponent_mode)) return e;
  if (int e = check_qnet_actors(actors, members, opponent_mode)) return e;
  if (int e = check_traj(traj)) return e;
  if (n_member == 0 || num_steps == 0) return 0;
  QRollout R = make_rollout<QRollout>(params, state, traj, stats, 0, first_step, env_offset, n, num_steps, flags);
  R.out_dim = out_dim, R.fin = finish_bound(*params);
  const QRolloutMany A = make_qrollout_many(R, n_member, actors, members, opponent_mode);
  launch(qnet_rollout_instance<QRolloutMany>(opponent_mode, out_dim > MG_NUM_ACTIONS),
         static_cast<unsigned>(members) * static_cast<unsigned>(A.blocks_per_member), kQWsThreads,
         static_cast<hipStream_t>(stream), A);
  return finish_launch("mg_rollout_qnet_many");
}

int mg_rollout_qnet_league(const mg_params* params, const mg_state* state, const mg_traj* traj,
                           const mg_stats* stats, int64_t n_pair, int32_t nets, int64_t env_offset,
                           uint64_t first_step, int32_t num_steps, const mg_league_net* league, int32_t out_dim,
                           uint32_t flags, void* stream) {
  const char* const who = "mg_rollout_qnet_league: %s";
  if (!members_ok(nets)) return fail(hipErrorInvalidValue, who, "need 1 <= nets <= 64");
  if (n_pair < 0) return fail(hipErrorInvalidValue, who, "n_pair < 0");
  if (n_pair % 64 != 0)
    return fail(hipErrorInvalidValue, who,
                "n_pair must be a multiple of 64 (a won-mask word covers 64 envs and is stored whole, so no "
                "two pairings may share one)");
  const int64_t pairs = static_cast<int64_t>(nets) * nets;
  // the envs within what a grid of kBlock-env blocks covers (check_common's limit), and the kernel's own blocks
  if (n_pair > (static_cast<int64_t>(0x7fffffff) * kBlock) / pairs ||
      pairs * ((n_pair + kQWsEnvs - 1) / kQWsEnvs) > 0x7fffffff)
    return fail(hipErrorInvalidValue, who, "nets * nets * n_pair exceeds the grid limit");
  const int64_t n = n_pair * pairs;
  if (int e = check_rollout_args(params, state, traj, n)) return e;
  if (!league) return fail(hipErrorInvalidValue, who, "league is NULL (nets mg_league_net entries)");
  if (int e = check_qrollout_dims(who, num_steps, out_dim)) return e;
  if (int e = check_league_nets(league, nets)) return e;
  if (int e = check_traj(traj)) return e;
  if (n_pair == 0 || num_steps == 0) return 0;
  QRollout R = make_rollout<QRollout>(params, state, traj, stats, 0, first_step, env_offset, n, num_steps, flags);
  R.out_dim = out_dim, R.fin = finish_bound(*params);
  const QRolloutLeague A = make_qrollout_league(R, n_pair, league, nets);
  // mode 3's instance is the checked one whatever out_dim is (qnet_rollout_instance)
  launch(qnet_rollout_ws_kernel<3, true, QRolloutLeague>,
         static_cast<unsigned>(pairs) * static_cast<unsigned>(A.blocks_per_pair), kQWsThreads,
         static_cast<hipStream_t>(stream), A);
  return finish_launch("mg_rollout_qnet_league");
}

int mg_rollout_hdqn(const mg_params* params, const mg_state* state, const mg_traj* traj,
                    const mg_hdqn_traj* htraj, const mg_stats* stats, int8_t* goal, int8_t* goal_op,
                    double* ext_acc, int64_t n, int64_t env_offset, uint64_t seed, uint64_t first_step,
                    int32_t num_steps,
                    const void* meta_net, int32_t num_goals, const void* lower_net, int32_t reset_goal,
                    uint64_t greedy_threshold, int32_t opponent_mode, const void* opp_meta_net,
                    const void* opp_lower_net, float* ring_rows,
                    uint64_t* ring_counter, int64_t ring_capacity, uint32_t flags, void* stream) {
  if (ring_rows && (!ring_counter || ring_capacity < 1 || misaligned(ring_rows, 15)))
    return fail(hipErrorInvalidValue, "%s", "ring_rows needs ring_counter, capacity >= 1 and 16-byte alignment");
  if (int e = check_rollout_args(params, state, traj, n)) return e;
  if (!goal) return fail(hipErrorInvalidValue, "%s", "goal is NULL (an [n] int8 device array)");
  if (!meta_net || !lower_net || misaligned(meta_net, 15) || misaligned(lower_net, 15))
    return fail(hipErrorInvalidValue, "%s", "meta_net / lower_net must be 16-byte aligned packed Q-nets");
  if (num_steps < 0 || num_goals < 1 || num_goals > 8 || reset_goal < 0 || reset_goal >= num_goals)
    return fail(hipErrorInvalidValue, "%s", "need num_steps >= 0, 1 <= num_goals <= 8, 0 <= reset_goal < num_goals");
  if (opponent_mode < 0 || opponent_mode > 3)
    return fail(hipErrorInvalidValue, "%s",
                "opponent_mode must be 0 (None), 1 (uniform), 2 (self-play) or 3 (other h-DQN)");
  if (opponent_mode >= 2 && !goal_op)
    return fail(hipErrorInvalidValue, "%s", "opponent_mode 2 / 3 needs goal_op (an [n] int8 device array)");
  if (opponent_mode == 3 &&
      (!opp_meta_net || !opp_lower_net || misaligned(opp_meta_net, 15) || misaligned(opp_lower_net, 15)))
    return fail(hipErrorInvalidValue, "%s",
                "opponent_mode 3 needs 16-byte aligned opp_meta_net / opp_lower_net (mg_qnet_fragments copies)");
  if (htraj && (htraj->ext_reward || htraj->no_break) && !ext_acc)
    return fail(hipErrorInvalidValue, "%s", "ext_reward / no_break need ext_acc (an [n] double device array)");
  if (htraj && misaligned(htraj->no_break, 7))
    return fail(hipErrorInvalidValue, "%s", "no_break must be 8-byte aligned");
  if (int e = check_traj(traj)) return e;
  if (n == 0 || num_steps == 0) return 0;
  if (!(flags & MG_AUTORESET))  // hdqn.py's loop resets at every episode end (:276-277)
    return fail(hipErrorInvalidValue, "%s", "mg_rollout_hdqn needs MG_AUTORESET (hdqn.py resets every episode)");
  HRollout R = make_rollout<HRollout>(params, state, traj, stats, seed, first_step, env_offset, n, num_steps, flags);
  if (htraj) R.H = *htraj;
  R.goal = goal;
  R.goal_op = goal_op;
  R.ext_acc = ext_acc;
  R.meta = static_cast<const uint8_t*>(meta_net);
  R.lower = static_cast<const uint8_t*>(lower_net);
  R.meta_op = static_cast<const uint8_t*>(opp_meta_net);
  R.lower_op = static_cast<const uint8_t*>(opp_lower_net);
  R.greedy_thr = greedy_threshold;
  R.num_goals = num_goals;
  R.reset_goal = reset_goal;
  R.ring = ring_rows;
  R.ring_counter = ring_counter;
  R.ring_capacity = ring_capacity;
  hipStream_t st = static_cast<hipStream_t>(stream);
  static void (*const kernels[4])(HRollout) = {hdqn_rollout_kernel<0>, hdqn_rollout_kernel<1>,
                                               hdqn_rollout_kernel<2>, hdqn_rollout_kernel<3>};
  // not launch(): this entry point leaves the events of mg_time_next_launch armed
  hipLaunchKernelGGL(kernels[opponent_mode], dim3(grid_blocks(n, kHEnvs)), dim3(512), 0, st, R);
  if (ring_rows)  // after every block has read the old counter: the same stream orders it
    hipLaunchKernelGGL(counter_add_kernel, dim3(1), dim3(1), 0, st, ring_counter,
                       static_cast<uint64_t>(num_steps) * static_cast<uint64_t>(n));
  return finish_launch("mg_rollout_hdqn");
}

size_t mg_replay_scratch_bytes(int64_t n, int32_t num_steps) { return replay_scratch_bytes(n, num_steps); }

int mg_replay_store(float* rows, uint64_t* counter, int64_t capacity, int32_t row_floats,
                    const mg_transitions* tr, int64_t n, int32_t num_steps, int32_t skip_ego_won,
                    void* scratch, size_t scratch_bytes, void* stream) {
  const ReplayStore C{&rows, &counter, 1, capacity, row_floats, tr, n, num_steps, skip_ego_won, scratch, scratch_bytes};
  if (int e = check_replay_store("mg_replay_store", C, false)) return e;
  return replay_store_device<false>("mg_replay_store", C, static_cast<hipStream_t>(stream));
}

size_t mg_replay_scratch_many_bytes(int64_t n_member, int32_t num_steps, int32_t members) {
  return members_ok(members) ? static_cast<size_t>(members) * replay_scratch_bytes(n_member, num_steps) : 0;
}

int mg_replay_store_many(float* const* rows, uint64_t* const* counters, int32_t members, int64_t capacity,
                         int32_t row_floats, const mg_transitions* tr, int64_t n_member, int32_t num_steps,
                         int32_t skip_ego_won, void* scratch, size_t scratch_bytes, void* stream) {
  const ReplayStore C{rows, counters, members, capacity, row_floats, tr, n_member, num_steps, skip_ego_won, scratch,
                      scratch_bytes};
  if (int e = check_replay_store("mg_replay_store_many", C, true)) return e;
  return replay_store_device<true>("mg_replay_store_many", C, static_cast<hipStream_t>(stream));
}

int mg_replay_sample(const float* rows, const uint64_t* counter, int64_t capacity,
                     int32_t row_floats, uint64_t seed, uint64_t draw, int32_t filled_only,
                     float* out, int64_t* idx_out, int64_t batch, void* stream) {
  if (row_floats != kRow && row_floats != kRowGoal)
    return fail(hipErrorInvalidValue, "%s", "mg_replay_sample: row_floats must be 22 or 24");
  if (!rows || !out || (filled_only && !counter))
    return fail(hipErrorInvalidValue, "%s", "mg_replay_sample: NULL pointer");
  if (capacity < 1 || capacity > (int64_t{1} << 32) || batch < 0)
    return fail(hipErrorInvalidValue, "%s", "mg_replay_sample: need 1 <= capacity <= 2^32 and batch >= 0");
  if (misaligned(rows, 7) || misaligned(out, 7))
    return fail(hipErrorInvalidValue, "%s", "mg_replay_sample: rows and out must be 8-byte aligned");
  if (batch == 0) return 0;
  hipLaunchKernelGGL(replay_sample_kernel, dim3(grid_blocks(batch)), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), rows, counter, capacity, row_floats, seed, draw,
                     filled_only, out, idx_out, batch);
  return finish_launch("mg_replay_sample");
}

int mg_reset(const mg_params* params, const mg_state* state, const uint8_t* mask,
             const mg_outputs* out, int64_t n, void* stream) {
  if (int e = check_params(params)) return e;
  if (n < 0) return fail(hipErrorInvalidValue, "%s", "n < 0");
  if (int e = check_state(state)) return e;
  if (n == 0) return 0;
  mg_outputs o{};
  if (out) o = *out;
  hipLaunchKernelGGL(reset_kernel, dim3(grid_blocks(n)), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), *params, *state, mask, o, n);
  return finish_launch("mg_reset");
}

int mg_observe(const mg_params* params, const mg_state* state, const mg_outputs* out, int64_t n,
               void* stream) {
  if (int e = check_common(params, state, out, n)) return e;
  if (n == 0) return 0;
  hipLaunchKernelGGL(observe_kernel, dim3(grid_blocks(n)), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), *params, *state, *out, n);
  return finish_launch("mg_observe");
}

size_t mg_stats_reduce_scratch_bytes(int64_t n) {
  if (n <= 0) return 0;
  return static_cast<size_t>((n + kRedEnvs - 1) / kRedEnvs) * sizeof(mg_stats_totals);
}

int mg_stats_reduce(const mg_episode_stats* rec, int64_t n, mg_stats_totals* totals, void* scratch,
                    size_t scratch_bytes, void* stream) {
  if (!totals || (n > 0 && !rec)) return fail(hipErrorInvalidValue, "%s", "mg_stats_reduce: NULL pointer");
  if (n < 0) return fail(hipErrorInvalidValue, "%s", "n < 0");
  if (misaligned(rec, 15) || misaligned(scratch, 15) || misaligned(totals, 7))
    return fail(hipErrorInvalidValue, "%s", "mg_stats_reduce: rec and scratch must be 16-byte, totals 8-byte aligned");
  const int64_t nb = (n + kRedEnvs - 1) / kRedEnvs;
  if (nb > 0x7fffffff) return fail(hipErrorInvalidValue, "%s", "n exceeds the grid limit");
  if (n > 0 && (!scratch || scratch_bytes < mg_stats_reduce_scratch_bytes(n)))
    return fail(hipErrorInvalidValue, "%s", "mg_stats_reduce: scratch smaller than mg_stats_reduce_scratch_bytes(n)");
  hipStream_t st = static_cast<hipStream_t>(stream);
  mg_stats_totals* part = static_cast<mg_stats_totals*>(scratch);
  if (nb > 0)
    hipLaunchKernelGGL(stats_reduce_kernel, dim3(static_cast<unsigned>(nb)), dim3(kRedThreads), 0, st, rec, n, part);
  hipLaunchKernelGGL(stats_reduce_final_kernel, dim3(1), dim3(kRedThreads), 0, st, part, nb, totals);
  return finish_launch("mg_stats_reduce");
}

constexpr int32_t kRedMaxSegments = 4096;  // the league's 64 x 64 pairings; the grid's second dimension holds 65,535

size_t mg_stats_reduce_many_scratch_bytes(int64_t n_segment, int32_t segments) {
  if (segments < 1 || segments > kRedMaxSegments) return 0;
  return static_cast<size_t>(segments) * mg_stats_reduce_scratch_bytes(n_segment);
}

int mg_stats_reduce_many(const mg_episode_stats* rec, int64_t n_segment, int32_t segments, mg_stats_totals* totals,
                         void* scratch, size_t scratch_bytes, void* stream) {
  const char* const who = "mg_stats_reduce_many: %s";
  if (segments < 1 || segments > kRedMaxSegments) return fail(hipErrorInvalidValue, who, "need 1 <= segments <= 4096");
  if (n_segment < 0) return fail(hipErrorInvalidValue, who, "n_segment < 0");
  if (!totals || (n_segment > 0 && !rec)) return fail(hipErrorInvalidValue, who, "NULL pointer");
  if (misaligned(rec, 15) || misaligned(scratch, 15) || misaligned(totals, 7))
    return fail(hipErrorInvalidValue, who, "rec and scratch must be 16-byte, totals 8-byte aligned");
  // before the scratch size, which is only then a product that fits
  const int64_t nb = n_segment / kRedEnvs + (n_segment % kRedEnvs != 0);
  if (nb > 0x7fffffff) return fail(hipErrorInvalidValue, who, "n_segment exceeds the grid limit");
  if (n_segment > 0 && (!scratch || scratch_bytes < mg_stats_reduce_many_scratch_bytes(n_segment, segments)))
    return fail(hipErrorInvalidValue, who,
                "scratch smaller than mg_stats_reduce_many_scratch_bytes(n_segment, segments)");
  hipStream_t st = static_cast<hipStream_t>(stream);
  mg_stats_totals* part = static_cast<mg_stats_totals*>(scratch);
  const unsigned S = static_cast<unsigned>(segments);
  if (nb > 0)
    hipLaunchKernelGGL(stats_reduce_many_kernel, dim3(static_cast<unsigned>(nb), S), dim3(kRedThreads), 0, st, rec,
                       n_segment, nb, part);
  hipLaunchKernelGGL(stats_reduce_final_many_kernel, dim3(S), dim3(kRedThreads), 0, st, part, nb, totals);
  return finish_launch("mg_stats_reduce_many");
}

int mg_host_step(const mg_params* params, const mg_state* state, const int8_t* a1, const int8_t* a2,
                 const mg_outputs* out, const mg_stats* stats, int64_t n, uint32_t flags) {
  if (int e = check_common(params, state, out, n)) return e;
  if (n == 0) return 0;
  if (!a1) return fail(hipErrorInvalidValue, "%s", "a1 is NULL");
  Launch L = make_launch(params, state, out, stats, n, flags);
  L.a1 = a1;
  L.a2 = a2;
  host_step_all(L);
  g_err[0] = '\0';
  return 0;
}

int mg_host_reset(const mg_params* params, const mg_state* state, const uint8_t* mask,
                  const mg_outputs* out, int64_t n) {
  if (int e = check_params(params)) return e;
  if (n < 0) return fail(hipErrorInvalidValue, "%s", "n < 0");
  if (int e = check_state(state)) return e;
  mg_outputs o{};
  if (out) o = *out;
  for (int64_t i = 0; i < n; ++i)
    if (!mask || mask[i]) host_reset_env(*params, *state, o, i);
  g_err[0] = '\0';
  return 0;
}

int mg_host_observe(const mg_params* params, const mg_state* state, const mg_outputs* out, int64_t n) {
  if (int e = check_common(params, state, out, n)) return e;
  for (int64_t i = 0; i < n; ++i) host_observe_env(*params, *state, *out, i);
  g_err[0] = '\0';
  return 0;
}

// ---- DQN.learn (scripts/main.py:122-157, hdqn.py:104-139, :186-221) -------------------------------
size_t mg_dqn_learner_bytes(int32_t in_dim, int32_t out_dim) {
  if (!net_dims_ok(in_dim, out_dim)) return 0;
  return static_cast<size_t>(learn_layout(in_dim, out_dim).total) * 4 * sizeof(float);
}

int mg_dqn_learner_init(float* learner, const float* fc1_w, const float* fc1_b, const float* fc2_w,
                        const float* fc2_b, const float* out_w, const float* out_b, int32_t in_dim,
                        int32_t out_dim, void* stream) {
  if (!learner || !fc1_w || !fc1_b || !fc2_w || !fc2_b || !out_w || !out_b)
    return fail(hipErrorInvalidValue, "%s", "mg_dqn_learner_init: NULL pointer");
  if (int e = check_net_dims("mg_dqn_learner_init", in_dim, out_dim)) return e;
  if (misaligned(learner, 15) || misaligned(fc1_w, 3) || misaligned(fc1_b, 3) || misaligned(fc2_w, 3) ||
      misaligned(fc2_b, 3) || misaligned(out_w, 3) || misaligned(out_b, 3))
    return fail(hipErrorInvalidValue, "%s", "mg_dqn_learner_init: learner must be 16-byte, the tensors 4-byte aligned");
  const LearnLayout O = learn_layout(in_dim, out_dim);
  const float* src[6] = {fc1_w, fc1_b, fc2_w, fc2_b, out_w, out_b};
  const int off[7] = {O.w1, O.b1, O.w2, O.b2, O.w3, O.b3, O.total};
  hipStream_t st = static_cast<hipStream_t>(stream);
  for (int blk = 0; blk < 2; ++blk)  // eval, target
    for (int k = 0; k < 6; ++k) {
      const int n = off[k + 1] - off[k];
      hipLaunchKernelGGL(learn_copy_kernel, dim3(grid_blocks(n)), dim3(kBlock), 0, st, src[k],
                         learner + blk * O.total + off[k], n);
    }
  if (hipError_t e = hipMemsetAsync(learner + 2 * O.total, 0, 2 * sizeof(float) * O.total, st)) {  // m, v
    std::snprintf(g_err, sizeof(g_err), "mg_dqn_learner_init: %s", hipGetErrorString(e));
    return static_cast<int>(e);
  }
  return finish_launch("mg_dqn_learner_init");
}

size_t mg_dqn_learn_scratch_bytes(int32_t batch, int32_t in_dim, int32_t out_dim) {
  if (batch < 1 || batch > 1024 || !net_dims_ok(in_dim, out_dim)) return 0;
  return static_cast<size_t>(learn_scratch(batch, in_dim, out_dim).total) * sizeof(float);
}

int mg_dqn_learn(float* learner, const float* rows, const uint64_t* counter, int64_t capacity, int32_t row_floats,
                 int32_t in_dim, int32_t out_dim, int32_t batch, int32_t num_updates, uint64_t first_update,
                 uint64_t seed, uint64_t first_draw, int32_t filled_only, const mg_dqn_hyper* hyper, float* loss_out,
                 float* rows_out, void* packed_out, void* scratch, size_t scratch_bytes, void* stream) {
  if (int e = check_learn("mg_dqn_learn", learner, rows, counter, capacity, row_floats, in_dim, out_dim, batch,
                          num_updates, filled_only, hyper, loss_out, rows_out, packed_out, scratch, scratch_bytes))
    return e;
  mg_dqn_member one{rows, counter, seed, first_update, first_draw, *hyper};  // the population of one, no table
  LearnMany Q = make_learn_many(learner, nullptr, &one, 1, capacity, in_dim, out_dim, batch, filled_only, scratch);
  return learn_many_device("mg_dqn_learn", Q, &one, num_updates, loss_out, rows_out, packed_out,
                           mg_qnet_packed_bytes(), static_cast<hipStream_t>(stream));
}

int mg_host_dqn_learn(float* learner, const float* rows, const uint64_t* counter, int64_t capacity, int32_t row_floats,
                      int32_t in_dim, int32_t out_dim, int32_t batch, int32_t num_updates, uint64_t first_update,
                      uint64_t seed, uint64_t first_draw, int32_t filled_only, const mg_dqn_hyper* hyper,
                      float* loss_out, float* rows_out, void* scratch, size_t scratch_bytes) {
  if (int e = check_learn("mg_host_dqn_learn", learner, rows, counter, capacity, row_floats, in_dim, out_dim, batch,
                          num_updates, filled_only, hyper, loss_out, rows_out, nullptr, scratch, scratch_bytes))
    return e;
  mg_dqn_member one{rows, counter, seed, first_update, first_draw, *hyper};
  LearnMany Q = make_learn_many(learner, nullptr, &one, 1, capacity, in_dim, out_dim, batch, filled_only, scratch);
  return learn_many_host(Q, &one, num_updates, loss_out, rows_out);
}

// ---- a population of DQN learners in mg_dqn_learn's launches ---------------------------------------
size_t mg_dqn_learn_many_table_bytes(int32_t members) {
  return members_ok(members) ? sizeof(LearnMember) * static_cast<size_t>(members) : 0;
}

int mg_dqn_learn_many_init(void* table, size_t table_bytes, const mg_dqn_member* member, int32_t members,
                           void* stream) {
  if (int e = check_members("mg_dqn_learn_many_init", member, members, 0)) return e;
  if (int e = check_member_table("mg_dqn_learn_many_init", table, table_bytes, members)) return e;
  for (int m = 0; m < members; ++m)  // by value, on the stream: nothing is copied from the caller's memory later
    hipLaunchKernelGGL(learn_many_entry_kernel, dim3(1), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                       static_cast<LearnMember*>(table) + m, learn_member_entry(member[m]));
  return finish_launch("mg_dqn_learn_many_init");
}

int mg_dqn_learn_many(float* learners, const void* table, size_t table_bytes, mg_dqn_member* member, int32_t members,
                      int64_t capacity, int32_t row_floats, int32_t in_dim, int32_t out_dim, int32_t batch,
                      int32_t num_updates, int32_t filled_only, float* loss_out, float* rows_out, void* packed_out,
                      size_t packed_stride, void* scratch, size_t scratch_bytes, void* stream) {
  if (int e = check_learn_many("mg_dqn_learn_many", learners, member, members, capacity, row_floats, in_dim, out_dim,
                               batch, num_updates, filled_only, loss_out, rows_out, packed_out, packed_stride, scratch,
                               scratch_bytes))
    return e;
  if (int e = check_member_table("mg_dqn_learn_many", table, table_bytes, members)) return e;
  LearnMany Q = make_learn_many(learners, static_cast<const LearnMember*>(table), member, members, capacity, in_dim,
                                out_dim, batch, filled_only, scratch);
  return learn_many_device("mg_dqn_learn_many", Q, member, num_updates, loss_out, rows_out, packed_out, packed_stride,
                           static_cast<hipStream_t>(stream));
}

int mg_host_dqn_learn_many(float* learners, mg_dqn_member* member, int32_t members, int64_t capacity,
                           int32_t row_floats, int32_t in_dim, int32_t out_dim, int32_t batch, int32_t num_updates,
                           int32_t filled_only, float* loss_out, float* rows_out, void* scratch,
                           size_t scratch_bytes) {
  if (int e = check_learn_many("mg_host_dqn_learn_many", learners, member, members, capacity, row_floats, in_dim,
                               out_dim, batch, num_updates, filled_only, loss_out, rows_out, nullptr, 0, scratch,
                               scratch_bytes))
    return e;
  LearnMember table[kMaxMembers];
  for (int m = 0; m < members; ++m) table[m] = learn_member_entry(member[m]);
  LearnMany Q =
      make_learn_many(learners, table, member, members, capacity, in_dim, out_dim, batch, filled_only, scratch);
  return learn_many_host(Q, member, num_updates, loss_out, rows_out);
}

// ---- Rainbow acting (scripts/ranbowdqn.py:517-548, :662-680) ----------------------------------------
size_t mg_rainbow_packed_bytes(void) { return static_cast<size_t>(kRbNetBytes); }

int mg_rainbow_pack(const float* linear1_w, const float* linear1_b, const float* linear2_w, const float* linear2_b,
                    const float* value1_w, const float* value1_b, const float* value2_w, const float* value2_b,
                    const float* advantage1_w, const float* advantage1_b, const float* advantage2_w,
                    const float* advantage2_b, const float* support, int32_t in_dim, int32_t hidden1,
                    int32_t hidden2, int32_t hidden_stream, int32_t num_actions, int32_t num_atoms, void* packed,
                    void* stream) {
  const RbTensors T{linear1_w, linear1_b, linear2_w, linear2_b, value1_w, value1_b, value2_w,
                    value2_b, advantage1_w, advantage1_b, advantage2_w, advantage2_b, support};
  if (!T.w1 || !T.b1 || !T.w2 || !T.b2 || !T.wv1 || !T.bv1 || !T.wv2 || !T.bv2 || !T.wa1 || !T.ba1 || !T.wa2 ||
      !T.ba2 || !T.z || !packed)
    return fail(hipErrorInvalidValue, "%s", "mg_rainbow_pack: NULL pointer");
  if (in_dim != kRbIn || hidden1 != kRbH1 || hidden2 != kRbH2 || hidden_stream != kRbHS ||
      num_actions != kRbActions || num_atoms != kRbAtoms)
    return fail(hipErrorInvalidValue, "%s",
                "mg_rainbow_pack: only RainbowDQN(10, 5) is packed: in_dim 10, hidden 32 / 64 / 64, 5 actions, 51 atoms");
  if (misaligned(packed, 15))
    return fail(hipErrorInvalidValue, "%s", "mg_rainbow_pack: packed buffer must be 16-byte aligned");
  for (const float* p : {T.w1, T.b1, T.w2, T.b2, T.wv1, T.bv1, T.wv2, T.bv2, T.wa1, T.ba1, T.wa2, T.ba2, T.z})
    if (misaligned(p, 3)) return fail(hipErrorInvalidValue, "%s", "mg_rainbow_pack: the tensors must be 4-byte aligned");
  hipLaunchKernelGGL(rainbow_pack_kernel, dim3(grid_blocks(kRbNetBytes / 4)), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), T, static_cast<uint8_t*>(packed));
  return finish_launch("mg_rainbow_pack");
}

int mg_rainbow_forward(const void* packed, const float* obs, int32_t rotate, float* logits, float* q,
                       int8_t* action, int64_t n, void* stream) {
  if (!obs) return fail(hipErrorInvalidValue, "%s", "mg_rainbow_forward: obs is NULL");
  if (int e = check_packed_net(packed, "mg_rainbow_forward: packed must be a 16-byte aligned packed Rainbow net"))
    return e;
  if (rotate < 0 || rotate >= kObs) return fail(hipErrorInvalidValue, "%s", "mg_rainbow_forward: need 0 <= rotate < 10");
  if (n < 0) return fail(hipErrorInvalidValue, "%s", "n < 0");
  if (n > (static_cast<int64_t>(0x7fffffff) * kBlock)) return fail(hipErrorInvalidValue, "%s", "n exceeds the grid limit");
  if (misaligned(obs, 3) || misaligned(logits, 3) || misaligned(q, 3))
    return fail(hipErrorInvalidValue, "%s", "mg_rainbow_forward: obs, logits and q must be 4-byte aligned");
  if (n == 0) return 0;
  hipLaunchKernelGGL(rainbow_forward_kernel, dim3(grid_blocks(n)), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                     static_cast<const uint8_t*>(packed), obs, rotate, logits, q, action, n);
  return finish_launch("mg_rainbow_forward");
}

int mg_rollout_rainbow(const mg_params* params, const mg_state* state, const mg_traj* traj, const mg_stats* stats,
                       int64_t n, int32_t num_steps, const void* net, int32_t opponent_mode, uint32_t flags,
                       void* stream) {
  if (int e = check_rollout_args(params, state, traj, n)) return e;
  if (int e = check_packed_net(net, "mg_rollout_rainbow: net must be a 16-byte aligned packed Rainbow net")) return e;
  if (int e = check_rb_rollout_steps_mode(false, num_steps, opponent_mode)) return e;
  if (int e = check_traj(traj)) return e;
  if (n == 0 || num_steps == 0) return 0;
  RbRollout R = make_rb_rollout(params, state, traj, stats, n, num_steps, flags);
  R.net = static_cast<const uint8_t*>(net);
  launch(rainbow_rollout_instance<false>(opponent_mode), grid_blocks(n, kRbThreads), kRbThreads,
         static_cast<hipStream_t>(stream), R);
  return finish_launch("mg_rollout_rainbow");
}

int mg_rollout_rainbow_many(const mg_params* params, const mg_state* state, const mg_traj* traj, const mg_stats* stats,
                            int64_t n_member, int32_t members, int32_t num_steps, const void* const* nets,
                            int32_t opponent_mode, uint32_t flags, void* stream) {
  const char* const who = "mg_rollout_rainbow_many";
  if (int e = check_rb_rollout_members(who, n_member, members)) return e;
  const int64_t n = n_member * members;
  if (int e = check_rollout_args(params, state, traj, n)) return e;
  if (int e = check_rb_member_nets(who, nets, members, "net")) return e;
  if (int e = check_rb_rollout_steps_mode(true, num_steps, opponent_mode)) return e;
  if (int e = check_traj(traj)) return e;
  if (n_member == 0 || num_steps == 0) return 0;
  return launch_rb_rollout_many(who, rainbow_rollout_instance<true>(opponent_mode),
                                make_rb_rollout(params, state, traj, stats, n, num_steps, flags), n_member, members,
                                nets, nullptr, static_cast<hipStream_t>(stream));
}

int mg_rollout_rainbow_vs(const mg_params* params, const mg_state* state, const mg_traj* traj, const mg_stats* stats,
                          int64_t n, int32_t num_steps, const void* net, const void* opponent, uint32_t flags,
                          void* stream) {
  if (int e = check_rollout_args(params, state, traj, n)) return e;
  if (int e = check_packed_net(net, "mg_rollout_rainbow_vs: net must be a 16-byte aligned packed Rainbow net"))
    return e;
  if (int e = check_packed_net(opponent,
                               "mg_rollout_rainbow_vs: opponent must be a 16-byte aligned packed Rainbow net"))
    return e;
  if (int e = check_rb_rollout_steps("mg_rollout_rainbow_vs", num_steps)) return e;
  if (int e = check_traj(traj)) return e;
  if (n == 0 || num_steps == 0) return 0;
  RbRolloutVs A{make_rb_rollout(params, state, traj, stats, n, num_steps, flags),
                static_cast<const uint8_t*>(opponent)};
  A.R.net = static_cast<const uint8_t*>(net);
  launch(rainbow_rollout_kernel<3, false>, grid_blocks(n, kRbThreads), kRbThreads, static_cast<hipStream_t>(stream),
         A);
  return finish_launch("mg_rollout_rainbow_vs");
}

int mg_rollout_rainbow_vs_many(const mg_params* params, const mg_state* state, const mg_traj* traj,
                               const mg_stats* stats, int64_t n_member, int32_t members, int32_t num_steps,
                               const void* const* nets, const void* const* opponents, uint32_t flags, void* stream) {
  const char* const who = "mg_rollout_rainbow_vs_many";
  if (int e = check_rb_rollout_members(who, n_member, members)) return e;
  const int64_t n = n_member * members;
  if (int e = check_rollout_args(params, state, traj, n)) return e;
  if (int e = check_rb_member_nets(who, nets, members, "net")) return e;
  if (int e = check_rb_member_nets(who, opponents, members, "opponent")) return e;
  if (int e = check_rb_rollout_steps(who, num_steps)) return e;
  if (int e = check_traj(traj)) return e;
  if (n_member == 0 || num_steps == 0) return 0;
  return launch_rb_rollout_many(who, rainbow_rollout_kernel<3, true>,
                                make_rb_rollout(params, state, traj, stats, n, num_steps, flags), n_member, members,
                                nets, opponents, static_cast<hipStream_t>(stream));
}

int mg_host_rainbow_head(const float* logits, const float* support, float* q, int8_t* action, int64_t n) {
  if (n < 0) return fail(hipErrorInvalidValue, "%s", "n < 0");
  if (!logits || !support) return fail(hipErrorInvalidValue, "%s", "mg_host_rainbow_head: logits or support is NULL");
  if (misaligned(logits, 3) || misaligned(support, 3) || misaligned(q, 3))
    return fail(hipErrorInvalidValue, "%s", "mg_host_rainbow_head: logits, support and q must be 4-byte aligned");
  for (int64_t i = 0; i < n; ++i)
    host_rainbow_head_row(logits + i * kRbLogits, support, q ? q + i * kRbActions : nullptr, action ? action + i : nullptr);
  g_err[0] = '\0';
  return 0;
}


int mg_host_rainbow_exp(const float* x, float* y, int64_t n) {
  if (n < 0) return fail(hipErrorInvalidValue, "%s", "n < 0");
  if (!x || !y) return fail(hipErrorInvalidValue, "%s", "mg_host_rainbow_exp: NULL pointer");
  for (int64_t i = 0; i < n; ++i) y[i] = x[i] > 0.0f ? NAN : rb_exp(x[i]);  // the head never passes x > 0
  g_err[0] = '\0';
  return 0;
}

// ---- Rainbow learning (scripts/ranbowdqn.py:265-323, :551-609) --------------------------------------
int mg_rainbow_replay_store(float* rows, uint64_t* counter, int64_t capacity, const mg_transitions* tr, int64_t n,
                            int32_t num_steps, void* stream) {
  if (int e = check_rainbow_store("mg_rainbow_replay_store", RlStoreCall{&rows, &counter, 1, capacity, tr, n, num_steps}))
    return e;
  if (n == 0 || num_steps == 0) return 0;
  rainbow_store(rows, counter, capacity, tr, n, num_steps, nullptr, 0.0, false, static_cast<hipStream_t>(stream));
  return finish_launch("mg_rainbow_replay_store");
}

int mg_rainbow_replay_store_many(float* const* rows, uint64_t* const* counters, int32_t members, int64_t capacity,
                                 const mg_transitions* tr, int64_t n_member, int32_t num_steps, void* stream) {
  const RlStoreCall C{rows, counters, members, capacity, tr, n_member, num_steps};
  if (int e = check_rainbow_store("mg_rainbow_replay_store_many", C, true)) return e;
  if (n_member == 0 || num_steps == 0) return 0;
  rainbow_store_many(C, false, static_cast<hipStream_t>(stream));
  return finish_launch("mg_rainbow_replay_store_many");
}

int mg_host_rainbow_replay_store_many(float* const* rows, uint64_t* const* counters, int32_t members, int64_t capacity,
                                      const mg_transitions* tr, int64_t n_member, int32_t num_steps) {
  const RlStoreCall C{rows, counters, members, capacity, tr, n_member, num_steps};
  if (int e = check_rainbow_store("mg_host_rainbow_replay_store_many", C, true)) return e;
  g_err[0] = '\0';
  if (n_member == 0 || num_steps == 0) return 0;
  rainbow_store_many(C, true, nullptr);
  return 0;
}

size_t mg_rainbow_learner_bytes(void) { return static_cast<size_t>(kRlLearner) * sizeof(float); }

size_t mg_rainbow_learn_scratch_bytes(int32_t batch) {
  if (batch < 1 || batch > 1024) return 0;
  return static_cast<size_t>(rl_scratch(batch, false).total) * sizeof(float);
}

// The four learners: the call as given, the check, one driver (the plain learner is the prioritized one without a
// tree).

int mg_rainbow_learn(float* learner, const float* rows, const uint64_t* counter, int64_t capacity, int32_t batch,
                     int32_t num_updates, uint64_t first_update, uint64_t seed, uint64_t first_draw,
                     const mg_dqn_hyper* hyper, const float* noise, float* loss_out, float* rows_out, float* proj_out,
                     float* grads_out, void* packed_out, void* scratch, size_t scratch_bytes, void* stream) {
  RLearnCall C{learner, rows, counter, capacity, batch, num_updates, first_update, seed, first_draw, hyper, noise,
               loss_out, rows_out, proj_out, grads_out, packed_out, scratch, scratch_bytes};
  if (int e = check_rainbow_learn("mg_rainbow_learn", C)) return e;
  return rainbow_learn_device("mg_rainbow_learn", C, static_cast<hipStream_t>(stream));
}

int mg_host_rainbow_learn(float* learner, const float* rows, const uint64_t* counter, int64_t capacity, int32_t batch,
                          int32_t num_updates, uint64_t first_update, uint64_t seed, uint64_t first_draw,
                          const mg_dqn_hyper* hyper, const float* noise, float* loss_out, float* rows_out,
                          float* proj_out, float* grads_out, void* scratch, size_t scratch_bytes) {
  RLearnCall C{learner, rows, counter, capacity, batch, num_updates, first_update, seed, first_draw, hyper, noise,
               loss_out, rows_out, proj_out, grads_out, nullptr, scratch, scratch_bytes};
  if (int e = check_rainbow_learn("mg_host_rainbow_learn", C)) return e;
  return rainbow_learn_host(C);
}

// ---- a population of Rainbow learners in mg_rainbow_learn's launches -------------------------------
size_t mg_rainbow_learn_many_table_bytes(int32_t members) {
  return members_ok(members) ? sizeof(LearnMember) * static_cast<size_t>(members) : 0;
}

int mg_rainbow_learn_many_init(void* table, size_t table_bytes, const mg_dqn_member* member, int32_t members,
                               void* stream) {
  const char* what = "mg_rainbow_learn_many_init";
  if (!members_ok(members)) return fail(hipErrorInvalidValue, "%s: need 1 <= members <= 64", what);
  if (!member) return fail(hipErrorInvalidValue, "%s: NULL pointer", what);
  if (int e = check_rainbow_members_null(what, member, members)) return e;
  if (int e = check_rainbow_members_betas(what, member, members)) return e;
  if (int e = check_rainbow_members_aligned(what, member, members)) return e;
  if (int e = check_rainbow_member_table(what, table, table_bytes, members)) return e;
  for (int m = 0; m < members; ++m)  // by value, on the stream: nothing is copied from the caller's memory later
    hipLaunchKernelGGL(learn_many_entry_kernel, dim3(1), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                       static_cast<LearnMember*>(table) + m, learn_member_entry(member[m]));
  return finish_launch(what);
}

int mg_rainbow_learn_many(float* learners, const void* table, size_t table_bytes, mg_dqn_member* member,
                          int32_t members, int64_t capacity, int32_t batch, int32_t num_updates, const float* noise,
                          float* loss_out, float* rows_out, float* proj_out, float* grads_out, void* packed_out,
                          size_t packed_stride, void* scratch, size_t scratch_bytes, void* stream) {
  const RLearnManyCall C{learners, table, table_bytes, member, members, capacity, batch, num_updates, noise,
                         loss_out, rows_out, proj_out, grads_out, packed_out, packed_stride, scratch, scratch_bytes,
                         false};
  if (int e = check_rainbow_learn_many("mg_rainbow_learn_many", C)) return e;
  return rainbow_learn_many_device("mg_rainbow_learn_many", C, static_cast<hipStream_t>(stream));
}

int mg_host_rainbow_learn_many(float* learners, mg_dqn_member* member, int32_t members, int64_t capacity,
                               int32_t batch, int32_t num_updates, const float* noise, float* loss_out,
                               float* rows_out, float* proj_out, float* grads_out, void* scratch,
                               size_t scratch_bytes) {
  const RLearnManyCall C{learners, nullptr, 0, member, members, capacity, batch, num_updates, noise,
                         loss_out, rows_out, proj_out, grads_out, nullptr, 0, scratch, scratch_bytes, true};
  if (int e = check_rainbow_learn_many("mg_host_rainbow_learn_many", C)) return e;
  return rainbow_learn_many_host(C);
}

int mg_rainbow_sync_target_many(float* learners, int32_t members, uint64_t mask, void* stream) {
  if (int e = check_rainbow_sync_many("mg_rainbow_sync_target_many", learners, members, mask)) return e;
  if (mask == 0) return 0;
  hipLaunchKernelGGL(rl_sync_many_kernel, dim3(grid_blocks(kRlParams + kRlEps), static_cast<unsigned>(members)),
                     dim3(kBlock), 0, static_cast<hipStream_t>(stream), learners, mask);
  return finish_launch("mg_rainbow_sync_target_many");
}

int mg_host_rainbow_project(const float* next_dist, const float* reward, const float* done, const float* support,
                            double gamma, float* proj, int64_t n) {
  if (n < 0) return fail(hipErrorInvalidValue, "%s", "n < 0");
  if (!next_dist || !reward || !done || !support || !proj)
    return fail(hipErrorInvalidValue, "%s", "mg_host_rainbow_project: NULL pointer");
  if (misaligned(next_dist, 3) || misaligned(reward, 3) || misaligned(done, 3) || misaligned(support, 3) ||
      misaligned(proj, 3))
    return fail(hipErrorInvalidValue, "%s", "mg_host_rainbow_project: the arrays must be 4-byte aligned");
  const float g = static_cast<float>(gamma);
  for (int64_t r = 0; r < n; ++r) {
    float bb[kRbAtoms];
    for (int i = 0; i < kRbAtoms; ++i) bb[i] = rl_b(reward[r], done[r], g, support[i]);
    for (int j = 0; j < kRbAtoms; ++j) proj[r * kRbAtoms + j] = rl_proj_slot(j, next_dist + r * kRbAtoms, bb);
  }
  g_err[0] = '\0';
  return 0;
}

int mg_host_rainbow_log(const float* x, float* y, int64_t n) {
  if (n < 0) return fail(hipErrorInvalidValue, "%s", "n < 0");
  if (!x || !y) return fail(hipErrorInvalidValue, "%s", "mg_host_rainbow_log: NULL pointer");
  for (int64_t i = 0; i < n; ++i) y[i] = x[i] >= 1.17549435e-38f && x[i] < INFINITY ? rb_log(x[i]) : NAN;
  g_err[0] = '\0';
  return 0;
}

// ---- Prioritized replay (scripts/ranbowdqn.py:130-262, :326-437) ------------------------------------
size_t mg_per_bytes(int64_t capacity) {
  if (capacity < 1 || capacity > (int64_t{1} << 32)) return 0;
  return static_cast<size_t>(per_doubles(capacity)) * sizeof(double);
}

int mg_per_init(void* tree, size_t tree_bytes, int64_t capacity, void* stream) {
  if (int e = check_per_tree("mg_per_init", tree, tree_bytes, capacity)) return e;
  const PerTree T = per_tree(tree, capacity);
  hipLaunchKernelGGL(per_init_kernel, dim3(grid_blocks(2 * T.C + 1)), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                     T);
  return finish_launch("mg_per_init");
}

int mg_host_per_init(void* tree, size_t tree_bytes, int64_t capacity) {
  if (int e = check_per_tree("mg_host_per_init", tree, tree_bytes, capacity)) return e;
  const PerTree T = per_tree(tree, capacity);
  for (int64_t i = 0; i <= 2 * T.C; ++i) per_init_at(T, i);
  g_err[0] = '\0';
  return 0;
}

int mg_per_store(float* rows, uint64_t* counter, int64_t capacity, const mg_transitions* tr, int64_t n,
                 int32_t num_steps, void* tree, size_t tree_bytes, double alpha, void* stream) {
  if (int e = check_rainbow_store("mg_per_store", RlStoreCall{&rows, &counter, 1, capacity, tr, n, num_steps})) return e;
  if (int e = check_per_tree("mg_per_store", tree, tree_bytes, capacity)) return e;
  if (int e = check_per_alpha("mg_per_store", alpha)) return e;
  if (n == 0 || num_steps == 0) return 0;
  rainbow_store(rows, counter, capacity, tr, n, num_steps, tree, alpha, false, static_cast<hipStream_t>(stream));
  return finish_launch("mg_per_store");
}

int mg_host_per_store(float* rows, uint64_t* counter, int64_t capacity, const mg_transitions* tr, int64_t n,
                      int32_t num_steps, void* tree, size_t tree_bytes, double alpha) {
  if (int e = check_rainbow_store("mg_host_per_store", RlStoreCall{&rows, &counter, 1, capacity, tr, n, num_steps}))
    return e;
  if (int e = check_per_tree("mg_host_per_store", tree, tree_bytes, capacity)) return e;
  if (int e = check_per_alpha("mg_host_per_store", alpha)) return e;
  g_err[0] = '\0';
  if (n == 0 || num_steps == 0) return 0;
  rainbow_store(rows, counter, capacity, tr, n, num_steps, tree, alpha, true, nullptr);
  return 0;
}

int mg_per_sample(const void* tree, size_t tree_bytes, const uint64_t* counter, int64_t capacity, double beta,
                  uint64_t seed, uint64_t draw, int32_t batch, int64_t* idx_out, float* weight_out, void* stream) {
  if (int e = check_per_sample("mg_per_sample", tree, tree_bytes, counter, capacity, beta, batch, idx_out, weight_out))
    return e;
  const PerSample P{per_tree(const_cast<void*>(tree), capacity), counter, beta, seed, draw, batch, idx_out, nullptr,
                    weight_out, nullptr};
  hipLaunchKernelGGL(per_sample_kernel<PerSample>, dim3(grid_blocks(batch)), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), P);
  return finish_launch("mg_per_sample");
}

int mg_host_per_sample(const void* tree, size_t tree_bytes, const uint64_t* counter, int64_t capacity, double beta,
                       uint64_t seed, uint64_t draw, int32_t batch, int64_t* idx_out, float* weight_out) {
  if (int e = check_per_sample("mg_host_per_sample", tree, tree_bytes, counter, capacity, beta, batch, idx_out,
                               weight_out))
    return e;
  const PerSample P{per_tree(const_cast<void*>(tree), capacity), counter, beta, seed, draw, batch, idx_out, nullptr,
                    weight_out, nullptr};
  for (int b = 0; b < batch; ++b) per_sample_at(P, b);
  g_err[0] = '\0';
  return 0;
}

int mg_per_update(void* tree, size_t tree_bytes, const uint64_t* counter, int64_t capacity, double alpha,
                  const int64_t* idx, const float* priority, int32_t batch, void* stream) {
  if (int e = check_per_update("mg_per_update", tree, tree_bytes, counter, capacity, alpha, idx, priority, batch))
    return e;
  const PerUpdate U{per_tree(tree, capacity), counter, alpha, idx, priority, 0.0f, 0, batch};
  hipLaunchKernelGGL(per_update_kernel, dim3(1), dim3(kPerTail), 0, static_cast<hipStream_t>(stream), U);
  return finish_launch("mg_per_update");
}

int mg_host_per_update(void* tree, size_t tree_bytes, const uint64_t* counter, int64_t capacity, double alpha,
                       const int64_t* idx, const float* priority, int32_t batch) {
  if (int e = check_per_update("mg_host_per_update", tree, tree_bytes, counter, capacity, alpha, idx, priority, batch))
    return e;
  host_per_update(PerUpdate{per_tree(tree, capacity), counter, alpha, idx, priority, 0.0f, 0, batch});
  g_err[0] = '\0';
  return 0;
}

double mg_host_per_uniform(uint64_t b, uint64_t draw, uint64_t seed) { return per_uniform(b, draw, seed); }

int mg_host_per_total(const void* tree, size_t tree_bytes, const uint64_t* counter, int64_t capacity, double* total) {
  if (!counter || !total) return fail(hipErrorInvalidValue, "%s: NULL pointer", "mg_host_per_total");
  if (int e = check_per_tree("mg_host_per_total", tree, tree_bytes, capacity)) return e;
  const int64_t len = per_len(counter, capacity);
  *total = len >= 2 ? per_total(per_tree(const_cast<void*>(tree), capacity), len) : 0.0;
  g_err[0] = '\0';
  return 0;
}

int mg_host_per_pow(const double* x, const double* y, double* out, int64_t n) {
  if (n < 0) return fail(hipErrorInvalidValue, "%s", "n < 0");
  if (!x || !y || !out) return fail(hipErrorInvalidValue, "%s: NULL pointer", "mg_host_per_pow");
  for (int64_t i = 0; i < n; ++i) out[i] = per_pow(x[i], y[i]);
  g_err[0] = '\0';
  return 0;
}

size_t mg_rainbow_learn_prioritized_scratch_bytes(int32_t batch) {
  if (batch < 1 || batch > 1024) return 0;
  return static_cast<size_t>(rl_scratch(batch, true).total) * sizeof(float);
}

int mg_rainbow_learn_prioritized(float* learner, const float* rows, const uint64_t* counter, int64_t capacity,
                                 int32_t batch, int32_t num_updates, uint64_t first_update, uint64_t seed,
                                 uint64_t first_draw, const mg_dqn_hyper* hyper, const float* noise, float* loss_out,
                                 float* rows_out, float* proj_out, float* grads_out, void* packed_out, void* scratch,
                                 size_t scratch_bytes, void* tree, size_t tree_bytes, double alpha, double beta,
                                 double prio_eps, int64_t* idx_out, float* weight_out, void* stream) {
  RLearnCall C{learner, rows, counter, capacity, batch, num_updates, first_update, seed, first_draw, hyper, noise,
               loss_out, rows_out, proj_out, grads_out, packed_out, scratch, scratch_bytes, true, tree, tree_bytes,
               alpha, beta, prio_eps, idx_out, weight_out};
  if (int e = check_rainbow_learn("mg_rainbow_learn_prioritized", C)) return e;
  return rainbow_learn_device("mg_rainbow_learn_prioritized", C, static_cast<hipStream_t>(stream));
}

int mg_host_rainbow_learn_prioritized(float* learner, const float* rows, const uint64_t* counter, int64_t capacity,
                                      int32_t batch, int32_t num_updates, uint64_t first_update, uint64_t seed,
                                      uint64_t first_draw, const mg_dqn_hyper* hyper, const float* noise,
                                      float* loss_out, float* rows_out, float* proj_out, float* grads_out,
                                      void* scratch, size_t scratch_bytes, void* tree, size_t tree_bytes, double alpha,
                                      double beta, double prio_eps, int64_t* idx_out, float* weight_out) {
  RLearnCall C{learner, rows, counter, capacity, batch, num_updates, first_update, seed, first_draw, hyper, noise,
               loss_out, rows_out, proj_out, grads_out, nullptr, scratch, scratch_bytes, true, tree, tree_bytes,
               alpha, beta, prio_eps, idx_out, weight_out};
  if (int e = check_rainbow_learn("mg_host_rainbow_learn_prioritized", C)) return e;
  return rainbow_learn_host(C);
}

// ---- a population of prioritized Rainbow learners: mg_rainbow_learn_many with every member's tree ---
int mg_rainbow_learn_prioritized_many(float* learners, const void* table, size_t table_bytes, mg_dqn_member* member,
                                      int32_t members, int64_t capacity, int32_t batch, int32_t num_updates,
                                      const float* noise, float* loss_out, float* rows_out, float* proj_out,
                                      float* grads_out, void* packed_out, size_t packed_stride, void* scratch,
                                      size_t scratch_bytes, const mg_per_member* per, size_t tree_bytes,
                                      int64_t* idx_out, float* weight_out, void* stream) {
  const RLearnManyCall C{learners, table, table_bytes, member, members, capacity, batch, num_updates, noise,
                         loss_out, rows_out, proj_out, grads_out, packed_out, packed_stride, scratch, scratch_bytes,
                         false, true, per, tree_bytes, idx_out, weight_out};
  if (int e = check_rainbow_learn_many("mg_rainbow_learn_prioritized_many", C)) return e;
  return rainbow_learn_many_device("mg_rainbow_learn_prioritized_many", C, static_cast<hipStream_t>(stream));
}

int mg_host_rainbow_learn_prioritized_many(float* learners, mg_dqn_member* member, int32_t members, int64_t capacity,
                                           int32_t batch, int32_t num_updates, const float* noise, float* loss_out,
                                           float* rows_out, float* proj_out, float* grads_out, void* scratch,
                                           size_t scratch_bytes, const mg_per_member* per, size_t tree_bytes,
                                           int64_t* idx_out, float* weight_out) {
  const RLearnManyCall C{learners, nullptr, 0, member, members, capacity, batch, num_updates, noise,
                         loss_out, rows_out, proj_out, grads_out, nullptr, 0, scratch, scratch_bytes,
                         true, true, per, tree_bytes, idx_out, weight_out};
  if (int e = check_rainbow_learn_many("mg_host_rainbow_learn_prioritized_many", C)) return e;
  return rainbow_learn_many_host(C);
}

int mg_per_store_many(float* const* rows, uint64_t* const* counters, int32_t members, int64_t capacity,
                      const mg_transitions* tr, int64_t n, int32_t num_steps, void* const* trees, size_t tree_bytes,
                      const double* alpha, void* stream) {
  const RlStoreCall C{rows, counters, members, capacity, tr, n, num_steps};
  if (int e = check_rainbow_store("mg_per_store_many", C, true)) return e;
  if (int e = check_per_store_many("mg_per_store_many", C, trees, tree_bytes, alpha)) return e;
  if (n == 0 || num_steps == 0) return 0;
  rainbow_store_many(C, false, static_cast<hipStream_t>(stream), trees, alpha);
  return finish_launch("mg_per_store_many");
}

int mg_host_per_store_many(float* const* rows, uint64_t* const* counters, int32_t members, int64_t capacity,
                           const mg_transitions* tr, int64_t n, int32_t num_steps, void* const* trees,
                           size_t tree_bytes, const double* alpha) {
  const RlStoreCall C{rows, counters, members, capacity, tr, n, num_steps};
  if (int e = check_rainbow_store("mg_host_per_store_many", C, true)) return e;
  if (int e = check_per_store_many("mg_host_per_store_many", C, trees, tree_bytes, alpha)) return e;
  g_err[0] = '\0';
  if (n == 0 || num_steps == 0) return 0;
  rainbow_store_many(C, true, nullptr, trees, alpha);
  return 0;
}

// ---- Rainbow noise on the device (the factors of RainbowDQN.reset_noise, :486-496, :537-541) --------
int mg_rainbow_noise(uint64_t noise_seed, uint64_t first_update, int32_t num_updates, float* noise_out, void* stream) {
  if (int e = check_rainbow_noise("mg_rainbow_noise", num_updates, noise_out)) return e;
  if (num_updates == 0) return 0;
  launch_rainbow_noise(noise_seed, first_update, num_updates, noise_out, static_cast<hipStream_t>(stream));
  return finish_launch("mg_rainbow_noise");
}

int mg_host_rainbow_noise(uint64_t noise_seed, uint64_t first_update, int32_t num_updates, float* noise_out) {
  if (int e = check_rainbow_noise("mg_host_rainbow_noise", num_updates, noise_out)) return e;
  host_rainbow_noise(noise_seed, first_update, num_updates, noise_out);
  g_err[0] = '\0';
  return 0;
}

int mg_rainbow_noise_many(const uint64_t* noise_seed, const uint64_t* first_update, int32_t members,
                          int32_t num_updates, float* noise_out, void* stream) {
  if (int e = check_rainbow_noise_many("mg_rainbow_noise_many", noise_seed, first_update, members, num_updates,
                                       noise_out))
    return e;
  if (num_updates == 0) return 0;
  launch_rainbow_noise_many(make_rainbow_noise_many(noise_seed, first_update, members), num_updates, noise_out,
                            static_cast<hipStream_t>(stream));
  return finish_launch("mg_rainbow_noise_many");
}

int mg_host_rainbow_noise_many(const uint64_t* noise_seed, const uint64_t* first_update, int32_t members,
                               int32_t num_updates, float* noise_out) {
  if (int e = check_rainbow_noise_many("mg_host_rainbow_noise_many", noise_seed, first_update, members, num_updates,
                                       noise_out))
    return e;
  host_rainbow_noise_many(make_rainbow_noise_many(noise_seed, first_update, members), num_updates, noise_out);
  g_err[0] = '\0';
  return 0;
}

int mg_rainbow_ndtri(const double* u, double* z, int64_t n, void* stream) {
  if (int e = check_rainbow_ndtri("mg_rainbow_ndtri", u, z, n)) return e;
  if (n == 0) return 0;
  launch_rainbow_ndtri(u, z, n, static_cast<hipStream_t>(stream));
  return finish_launch("mg_rainbow_ndtri");
}

int mg_host_rainbow_ndtri(const double* u, double* z, int64_t n) {
  if (int e = check_rainbow_ndtri("mg_host_rainbow_ndtri", u, z, n)) return e;
  host_rainbow_ndtri(u, z, n);
  g_err[0] = '\0';
  return 0;
}

}  // extern "C"
