/*
 * merging_hip.h — C-ABI of libmerging_hip.so, the MI355X (gfx950) batched MergingEnv.
 *
 * The reference (YikangZhang1641/merging-gym) is pure Python and has no FFI. Its plugin
 * boundary is the gym.Env registered as "merging_env-v0" (merging_gym/__init__.py:3-6).
 * Each entry point below replaces one method of that env for a whole batch of envs held
 * as a struct-of-arrays in device memory; merging_gym/_native.py binds them with ctypes.
 *
 *   mg_step         replaces MergeEnv.step(action1, action2=None)   merging_env.py:138-195
 *                     (with action_to_acc :134-136 -> helper.mpc_1d helper.py:152-191,
 *                      observe :118-132, lon2coord :48-58, is_collided :198-206,
 *                      corners :232-239)
 *   mg_step_random  the same step, actions drawn on the device (Philox4x32-10); it replaces
 *                     the callers' env.action_space.sample() / np.random.randint(0, 5)
 *                     exploration branch (scripts/main.py:110, scripts/hdqn.py:175)
 *   mg_replay_store / mg_replay_sample / mg_replay_scratch_bytes: the DQN replay memory on the
 *                     device -- DQN.store_transition (scripts/main.py:115-119, hdqn.py:180-184)
 *                     for a whole batch of transitions, and learn()'s uniform minibatch draw
 *                     np.random.choice(MEMORY_CAPACITY, BATCH_SIZE) (main.py:130-131)
 *   mg_stats_reduce (ABI 20) the batch's episode-statistics records summed in a fixed order: the
 *                     running totals of the scripts' logging loops (hdqn.py:330-346, main.py:221-228)
 *   mg_reset        replaces MergeEnv.reset()                        merging_env.py:208-230
 *   mg_observe      replaces MergeEnv.observe() and is_collided()    merging_env.py:118-132,
 *                     :198-206 (no state change)
 *   mg_rollout_random  T steps of mg_step_random in one launch (trajectory outputs); it
 *                     replaces the callers' per-step collection loop (scripts/main.py:192-220)
 *   mg_rollout_qnet T steps with the epsilon-greedy DQN policy fused in (bf16 MFMA): replaces
 *                     DQN.choose_action (scripts/main.py:99-112, hdqn.py:165-177) + env.step
 *   mg_rollout_hdqn   T steps of hdqn.py's acting loop (meta-net goal, lower net on [goal] + state,
 *                     goal_status intrinsic reward) fused with the env step: replaces
 *                     Goal_DQN.choose_goal / HDQN.choose_action + env.step (hdqn.py:280-323)
 *   mg_qnet_pack / mg_qnet_forward / mg_qnet_packed_bytes / mg_qnet_fragments /
 *   mg_qnet_fragment_bytes: the Q-net Net (main.py:30-47,
 *                     hdqn.py:38-55) in the kernel's packed bf16 layout, and its forward pass
 *   mg_host_step / mg_host_reset / mg_host_observe (ABI 20): mg_step / mg_reset / mg_observe on
 *                     HOST memory, for the single env of BASELINE config 1 (the reference's CPU
 *                     MergeEnv, merging_env.py:118-230, driven one step at a time by
 *                     scripts/human_player.py:112-187 and the scripts' list API)
 *   mg_dqn_learn / mg_dqn_learner_init / mg_dqn_learner_bytes / mg_dqn_learn_scratch_bytes /
 *   mg_host_dqn_learn (ABI 21): DQN.learn (scripts/main.py:122-157; HDQN.learn hdqn.py:186-221,
 *                     Goal_DQN.learn hdqn.py:104-139) -- the minibatch update from the replay ring:
 *                     Double-DQN target, MSE, Adam, the target copy; fp32 in a documented order
 *   mg_dqn_learn_many / mg_dqn_learn_many_init / mg_dqn_learn_many_table_bytes / mg_host_dqn_learn_many: up to
 *                     64 such learners of one shape, each on its own net, memory, seed and hyperparameters,
 *                     in the same seven launches; every member bit for bit a lone mg_dqn_learn
 *   mg_rollout_qnet_many / mg_replay_store_many / mg_replay_scratch_many_bytes: the acting half of such a
 *                     population -- up to 64 members' epsilon-greedy rollouts on slices of one env batch in
 *                     one launch, and their transitions into 64 rings in three; every member bit for bit a
 *                     lone mg_rollout_qnet / mg_replay_store
 *   mg_rollout_qnet_league / mg_stats_reduce_many / mg_stats_reduce_many_scratch_bytes: league evaluation of
 *                     such a population -- every ordered pair (ego i, opponent j) of up to 64 nets plays on its
 *                     own slice of one env batch in one launch, and the batch's episode records become one
 *                     total per pairing in two; every pairing bit for bit a lone mode-3 mg_rollout_qnet, every
 *                     total a lone mg_stats_reduce (the reference's question, main.py:161-168: a net trained
 *                     against L1, or in self-play, compared with the others as ego and as opponent)
 *   mg_rainbow_pack / mg_rainbow_packed_bytes / mg_rainbow_forward / mg_host_rainbow_head: RainbowDQN's
 *                     acting forward (scripts/ranbowdqn.py:517-548: noisy dueling C51 net, act()) -- bf16
 *                     MFMA layers, the distributional head in fp32 in a documented order
 *   mg_rollout_rainbow T steps of ranbowdqn.py's acting loop (:662-680: act on the state, act on the
 *                     view rotated by three, env.step) in one launch
 *   mg_rainbow_replay_store / mg_rainbow_learn / mg_rainbow_learner_bytes / mg_rainbow_learn_scratch_bytes /
 *   mg_host_rainbow_learn / mg_host_rainbow_project / mg_host_rainbow_log: ranbowdqn.py's ReplayBuffer.push
 *                     (:281-288) and compute_td_loss (:554-609) -- C51 projection, noisy-net backward, Adam,
 *                     the noise reset; fp32 in a documented order
 *   mg_per_* / mg_rainbow_learn_prioritized: PrioritizedReplayBuffer (:326-437) and its segment trees
 *                     (:130-262) beside those rows, and compute_td_loss drawing from them
 *   mg_rainbow_noise / mg_host_rainbow_noise / mg_rainbow_ndtri / mg_host_rainbow_ndtri: the factors of
 *                     RainbowDQN.reset_noise (:486-496, :537-541) drawn on the device from a counter-based
 *                     stream in a documented order, and its inverse normal CDF alone
 *   mg_rollout_rainbow_many / mg_rainbow_replay_store_many / mg_host_rainbow_replay_store_many: the acting
 *                     half of a Rainbow population -- up to 64 members' rollouts on slices of one env batch
 *                     in one launch, and their transitions into 64 replay memories in two; every member bit
 *                     for bit a lone mg_rollout_rainbow / mg_rainbow_replay_store
 *   mg_rollout_rainbow_vs / mg_rollout_rainbow_vs_many: that loop with action_op from a second Rainbow net
 *                     (a frozen checkpoint, another member of the population), lone and per member
 *   mg_abi_version, mg_last_error, mg_build_info, mg_params_default, mg_time_next_launch: library plumbing
 *                     and profiling (no reference twin).
 *
 * Conventions
 *   - Every pointer inside mg_state / mg_outputs / mg_stats / action arrays is a DEVICE
 *     pointer owned by the caller (HOST pointers for the mg_host_* entry points). The library
 *     never allocates, frees or synchronises.
 *   - Calls are stream-ordered on `stream` (a hipStream_t, NULL = default stream) and
 *     return immediately. Return value: 0 on success, otherwise a hipError_t value
 *     (as int) and mg_last_error() describes it (thread-local). No exception crosses
 *     the ABI.
 *   - Arithmetic is IEEE fp64 with no contraction, like the reference's Python floats;
 *     the fp32 outputs are the fp64 results rounded once.
 */
#ifndef MERGING_HIP_H_
#define MERGING_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MG_ABI_VERSION 21
#define MG_OBS_DIM 10   /* merging_env.py:75 observation_shape = (10) */
#define MG_NUM_ACTIONS 5 /* merging_env.py:101-102 action_dict / Discrete(5) */
#define MG_ACTION_NONE (-1) /* action2=None: the constant-speed "L0" opponent, merging_env.py:152 */

/* Bits of mg_state.tf (one uint16 per env). The step count only decides the timeout (done from
 * step 2501, merging_env.py:141-143), so it saturates at 8191. */
#define MG_TF_STEPS_MASK 0x1FFFu  /* steps since reset, saturating at 8191 */
#define MG_TF_WINNER_SHIFT 13     /* 2 bits: 0 = None, 1 = ego, 2 = opponent (self.winner) */
#define MG_TF_WINNER_MASK 0x6000u
#define MG_TF_DONE 0x8000u        /* self.done */

/* Flags argument of mg_step / mg_step_random. */
#define MG_AUTORESET 0x1u /* gym.vector semantics: an env that is done after this step is reset
                             in place; obs receives the reset observation and
                             out->final_obs (if non-NULL) the terminal one */

/* Bits of mg_rec64.status (single-env drop-in path). */
#define MG_ST_DONE 0x1u
#define MG_ST_COLLISION 0x2u
#define MG_ST_R1_INT 0x4u /* reward1 is the Python int the reference returns (merging_env.py:168) */
#define MG_ST_R2_INT 0x8u /* reward2 likewise (merging_env.py:178) */
#define MG_ST_V1_INT 0x10u /* vel1 is int 0 from max(0, ...) (merging_env.py:149) */
#define MG_ST_V2_INT 0x20u /* vel2 likewise (merging_env.py:153) */

/* Environment constants, merging_env.py:22-46 and :101. Fill with mg_params_default(), then change
 * what differs. Every field is read by the kernels, and the parity bar of the default values -- flags
 * exact, fp32 outputs the oracle's fp64 values rounded once, fp64 state bit for bit -- holds across
 * mg_params (tests/params_cases.py).
 *
 * Derived fields: a caller that changes R, H, prediction_t, dT or the time limit recomputes them, as
 * mg_params_default does for the defaults (tests/params_cases.py fill_native restates it):
 *   angle0        = atan2(H, R)
 *   inv_R         = 1 / R, rounded
 *   end_point     the reference's H - 50 (any value on the road is accepted)
 *   qp_nz, qp_z0, qp_vsmall   qpgen2's constants for the horizon prediction_t
 *   qp_inv_nz     = 1 / qp_nz, rounded
 *   timeout_steps = the first k at which k sequential fp64 additions of dT exceed the time limit
 *                   (merging_env.py:141-142; 500 s there): dT = 0.1 gives 5000, not 5001.
 * Accepted ranges, checked on the host by every entry point that takes params (a non-zero return,
 * mg_last_error() names the field): 1 <= timeout_steps <= 8191 (mg_state.tf's step count saturates
 * there, so a larger value would never time out); R, dT positive and finite; veh_w, veh_h positive;
 * inv_R == 1 / R and qp_inv_nz == 1 / qp_nz exactly (the kernels' division needs the rounded
 * reciprocal of its divisor). Nothing else is checked: an angle0 or a qp constant that does not follow
 * from the other fields is computed with as given.
 * One exception to the bar: where |angle0 - pos / R| >= 1/16 (R = 300, say) sin / cos are the device
 * library's on the GPU and glibc's in the oracle and the host path, one ulp apart, which can move
 * the collision flag of boxes that exactly touch; there the flags are checked on the host path only. */
typedef struct mg_params {
  double R;            /* 30000: arc radius                          merging_env.py:22 */
  double H;            /* 1000                                        merging_env.py:23 */
  double W;            /* 300                                         merging_env.py:23 */
  double dT;           /* 0.2 s per step                              merging_env.py:25 */
  double r_first;      /* 2.0  RFirst                                 merging_env.py:28 */
  double r_second;     /* 1.0  RSecond                                merging_env.py:29 */
  double r_collision;  /* -10  RCollision                             merging_env.py:30 */
  double vel_penalty;  /* 0.001                                       merging_env.py:31 */
  double time_penalty; /* 0                                           merging_env.py:32 */
  double start_point;  /* 50                                          merging_env.py:36 */
  double end_point;    /* 950 = H - 50                                merging_env.py:37 */
  double start_vel;    /* 20.0 (reset)                                merging_env.py:216-217 */
  double vel_ref;      /* 20.0 (reward reference speed)               merging_env.py:158-159 */
  double prediction_t; /* 3.0 MPC horizon                             merging_env.py:43 */
  double angle0;       /* atan2(H, R), host-precomputed               merging_env.py:49 */
  double action_speed[MG_NUM_ACTIONS]; /* {0,10,20,30,40}             merging_env.py:101 */
  int32_t veh_w;       /* 4  lateral box size                         merging_env.py:40,97 */
  int32_t veh_h;       /* 8  longitudinal box size                    merging_env.py:40,97 */
  int32_t timeout_steps; /* 2501: first step with time_stamp > 500    merging_env.py:141-143 */
  int32_t _pad;
  double inv_R;        /* 1 / R, rounded: the kernel divides by R (and by qp_nz) with an
                          FMA-corrected reciprocal multiply (still correctly rounded) */
  /* mpc_1d's QP (scripts/helper.py:152-191) as quadprog 0.1.11's qpgen2 (the Goldfarb-Idnani
   * dual method, reached through qpsolvers 1.8.0 at helper.py:182) runs it: P = R'R by LINPACK
   * dpofa, J = R^-1 by dpori, then for the one equality (normal n = A[1], b = vt - v0, its sign
   * folded into n when the residual is positive) d = J'n, z = J d, t = |b| / z'n and
   * u = 0 + t z; a residual |b| < vsmall counts as satisfied (u = 0). So u0 = (b / z'n) * z0
   * with the two constants below computed in that operation order by mg_params_default (ABI
   * 17; ABI <= 16 used Cholesky substitution, an ulp apart). Restated from the published
   * algorithm -- quadprog is not importable here, so bit parity with it is unpinned. */
  double qp_nz;        /* z'n = 90.0000000000015 (t = 3) */
  double qp_z0;        /* z[0] = 30.000000000000533 */
  double qp_inv_nz;    /* 1 / qp_nz, rounded */
  double qp_vsmall;    /* qpgen2's vsmall: the first 1e-60 * 2^k with 1 + 0.1 vsmall > 1 and
                          1 + 0.2 vsmall > 1 (1.4272476927059598e-15) */
} mg_params;

/* Per-env state, struct of arrays, n entries each (device pointers). */
typedef struct mg_state {
  double* p1;   /* state1['pos']  (ego) */
  double* v1;   /* state1['vel'] */
  double* p2;   /* state2['pos']  (opponent) */
  double* v2;   /* state2['vel'] */
  double* ret1; /* r1_accumulate */
  double* ret2; /* r2_accumulate */
  uint16_t* tf; /* step count | winner | done, see MG_TF_* */
} mg_state;

/* Packed fp64 record for the single-env (list API) path. */
typedef struct mg_rec64 {
  double obs[MG_OBS_DIM];
  double rew[2];
  double acc[2];  /* state1['acc'], state2['acc'] */
  double pos[2];
  double vel[2];
  double ret[2];
  uint32_t tf;
  uint32_t status; /* MG_ST_* */
} mg_rec64;

/* Outputs of one step. Any pointer may be NULL to skip that output. */
typedef struct mg_outputs {
  float* obs;           /* [n,10] fp32, 16-byte aligned */
  float* rew;           /* [n,2]  fp32, 8-byte aligned */
  uint8_t* done;        /* [n] 0/1 */
  uint8_t* coll;        /* [n] 0/1, info["collision"] */
  uint64_t* done_mask;  /* [ceil(n/64)] bit j of word w = done of env 64w+j */
  float* final_obs;     /* [n,10] written only for envs that finished (with MG_AUTORESET) */
  mg_rec64* rec64;      /* [n] fp64 record (single-env drop-in path) */
  int32_t* error;       /* [1] OR-ed with 1 (a1) / 2 (a2) when an action is outside the valid set.
                           Such an env is advanced exactly as far as the reference gets before its
                           action_dict[...] KeyError (merging_env.py:141-147, :152): the clock
                           always, the ego too when only a2 is invalid; nothing else is written. */
  uint64_t* won_mask;   /* [ceil(n/64)] bit = env.winner == 1 after this step (read before any
                           autoreset): main.py:209 stores a transition only when it is 0 */
  uint8_t* flags;       /* [n,4] interleaved a1, a2 (int8), done, collision (0/1), 4-byte aligned:
                           one 32-bit store per env instead of four byte stores. When set, done
                           and coll must be NULL, and so must mg_step_random's a1_out / a2_out
                           (the actions land here); mg_observe writes byte 3. Not with rec64. */
} mg_outputs;

/* Trajectory buffers of mg_rollout_random: the outputs of step t for env i sit at row
 * t * n + i. Any pointer may be NULL to skip that output. */
typedef struct mg_traj {
  float* obs;       /* [T, n, 10] fp32, 16-byte aligned (reset observation where autoreset fired) */
  float* rew;       /* [T, n, 2] fp32 */
  uint8_t* done;    /* [T, n] */
  uint8_t* coll;    /* [T, n] */
  int8_t* a1;       /* [T, n] actions drawn */
  int8_t* a2;       /* [T, n] (-1 = None) */
  float* final_obs; /* [T, n, 10] written only at rows whose env finished at that step */
  uint64_t* won_mask; /* [T, ceil(n/64)] as mg_outputs.won_mask, one bitmask per step */
  uint8_t* flags;   /* [T, n, 4] = (a1, a2, done, coll) interleaved, 4-byte aligned, or NULL. When
                       set, the four byte arrays above are ignored and each env-step's four bytes
                       leave as one 32-bit store (separate byte arrays cost the rollout ~5 %) */
} mg_traj;

/* A batch of transitions for the replay memory, T steps of n envs in [T, n, ...] layout (the
 * trajectory buffers of a rollout, or one step's outputs with T = 1). Transition (t, i) is
 *   s  = obs_first[i] (t = 0) or obs[t-1, i],   a = a1[t, i],   r = rew[t, i, 0] (the ego's),
 *   s' = final_obs[t, i] where done[t, i] (autoreset put the reset observation in obs), else obs[t, i]
 * -- exactly what the reference's loop hands store_transition (main.py:195-211).
 * Goal-augmented rows (hdqn.py's lower-level memory, :158 np.zeros((MEMORY_CAPACITY,
 * (NUM_STATES + 1) * 2 + 2)), :180-184, fed at :291-316 with goal_state = [goal] + state):
 * with goal != NULL a row is 24 floats [goal, s(10), a, r, next_goal, s'(10)]; reward != NULL
 * replaces rew[t, i, 0] (hdqn's intrinsic reward, :314). */
typedef struct mg_transitions {
  const float* obs_first;   /* [n, 10] observation before step 0 */
  const float* obs;         /* [T, n, 10] */
  const float* final_obs;   /* [T, n, 10] or NULL (then s' = obs even where done) */
  const int8_t* a1;         /* [T, n] (or NULL with flags) */
  const float* rew;         /* [T, n, 2] */
  const uint8_t* done;      /* [T, n] or NULL (never done; ignored with flags) */
  const uint64_t* won_mask; /* [T, ceil(n/64)] or NULL (nobody has won) */
  const float* goal;        /* [T, n] goal column of s, or NULL (22-float rows) */
  const float* next_goal;   /* [T, n] goal column of s' (required with goal) */
  const float* reward;      /* [T, n] r of the row, or NULL (r = rew[t, i, 0]) */
  const uint8_t* flags;     /* [T, n, 4] interleaved (a1, a2, done, coll) of mg_traj.flags, or NULL:
                               then a1 = flags[4 row], done = flags[4 row + 2] */
  const float* meta_goal;   /* (ABI 15) [T, n] or NULL: Goal_DQN's memory instead (hdqn.py:97-101,
                               stored at :325 once an inner loop broke): row [s', meta_goal, reward,
                               s'] with s' the next state (terminal where done) for the transitions
                               whose won_mask bit is CLEAR -- the mask then marks the steps that did
                               not end an inner loop (mg_hdqn_traj.no_break) and is required, as is
                               reward (the extrinsic reward, mg_hdqn_traj.ext_reward); 22-float rows,
                               goal NULL, skip_ego_won ignored */
} mg_transitions;

/* Completed-episode statistics of one env, updated when it finishes (MG_AUTORESET): the
 * quantities the reference's training scripts log per episode, summed over the env's episodes
 * (ABI 17). One 64-byte record per env, so a finishing env's read-modify-write stays within one
 * cache line: as separate arrays (ABI <= 7) those scattered updates cost the one-step kernel 12 %
 * of its time at 2^22 envs (tools/steady_probe.py).
 *   main.py:189-227   ep_reward sums the ego's reward only over steps after which
 *                     `env.winner is not 1` (:209-211); win_count counts `state[8] > state[3]`
 *                     on the observation the episode's LAST step acted on (`state = next_state`
 *                     is skipped at the :218-220 break), i.e. END_POINT - p2 > END_POINT - p1
 *                     in fp64 on the state before that step;
 *   hdqn.py:276-346   ep_reward is every step's reward (= r1_accumulate, :312); win_count tests
 *                     `state[8] > state[3]` on the terminal observation (state = next_state at
 *                     :320 before the break).
 * winner never returns to 1 once it is 2, and stays 1 once set, so main.py's filtered sum is
 * r1_accumulate as it stood before the step on which the ego arrived first (or the whole
 * r1_accumulate when it never did): the kernels keep that value in ret1_pending. */
typedef struct mg_episode_stats {
  double ret[2];        /* sum of completed-episode returns r{1,2}_accumulate (hdqn.py's ep_reward) */
  double ret_main;      /* sum of main.py's winner-filtered ep_reward */
  double ret1_pending;  /* scratch (per env): r1_accumulate before the current episode's ego-first
                           arrival step; read only while winner == 1 */
  uint32_t episodes;    /* completed episodes */
  uint32_t collisions;  /* of which ended in a collision */
  uint32_t ego_first;   /* of which the ego arrived first (winner == 1) */
  uint32_t steps;       /* total steps of the completed episodes */
  uint32_t win_main;    /* main.py:225's win test on the pre-terminal observation */
  uint32_t win_hdqn;    /* hdqn.py:342's win test on the terminal observation */
  double q_eval;        /* (ABI 20; reserved zero bytes until ABI 19) sum over the completed episodes
                           of the Q value the scripts log for each (q_eval_value): the fused policy
                           kernels add eval_net(state)[action] on the last step's input and action
                           (mg_rollout_qnet, main.py:221) or meta_eval_net(state)[goal] on the terminal
                           state and the goal chosen on it (mg_rollout_hdqn, hdqn.py:330); the kernels
                           without a net leave it unchanged */
} mg_episode_stats;

typedef struct mg_stats {
  mg_episode_stats* rec;  /* [n] records, or NULL: no statistics */
} mg_stats;

/* (ABI 20) The records of a batch summed: what the logging loops of scripts/hdqn.py:330-346 and
 * scripts/main.py:221-228 total over completed episodes: the per-rank contribution of the
 * multi-GPU statistics all-gather (merging_gym/distributed.py), 80 bytes. */
typedef struct mg_stats_totals {
  double ret[3];      /* sums of ret[0], ret[1], ret_main */
  double q_eval;      /* sum of q_eval */
  int64_t counts[6];  /* sums of episodes, collisions, ego_first, steps, win_main, win_hdqn */
} mg_stats_totals;

int mg_abi_version(void);
const char* mg_last_error(void);
/* (ABI 20) The compiler and HIP version the library was built with, e.g. for test logs. */
const char* mg_build_info(void);

/* Profiling hook: the next mg_step / mg_step_random / mg_rollout_random launch made by the calling thread records
 * start_event / stop_event (hipEvent_t created by the caller; either may be NULL) in its own
 * dispatch packet (hipExtLaunchKernel), so hipEventElapsedTime(start, stop) is the kernel's
 * duration without the launch gap. Consumed by that launch. Always returns 0. */
int mg_time_next_launch(void* start_event, void* stop_event);

/* Fills *p with the reference constants (merging_env.py:22-46, :101). Host only. */
void mg_params_default(mg_params* p);

/* One env step for n envs. a1[n] in {0..4}; a2[n] in {0..4, -1 = None} or a2 == NULL (all None).
 * Replaces MergeEnv.step (merging_env.py:138-195). */
int mg_step(const mg_params* params, const mg_state* state, const int8_t* a1, const int8_t* a2,
            const mg_outputs* out, const mg_stats* stats, int64_t n, uint32_t flags, void* stream);

/* As mg_step, with actions drawn on the device (ABI 12): w = word ((step_idx div 2) mod 4) of
 * Philox4x32-10 (key = seed, counter = (env_offset + env index, step_idx div 8)) -- one call
 * covers eight steps of a rollout, two draws per word; a shard of a larger batch passes its first
 * global env index as env_offset and draws the same actions it would draw unsharded. A draw of
 * m outcomes is floor(m w / 2^32); an odd step_idx draws from m w mod 2^32 instead (the first
 * draw's remainder). opponent_random != 0: m = 25, the pair x = draw, a1 = x / 5, a2 = x % 5;
 * else m = 5, a1 = draw, a2 None.
 * If a1_out / a2_out are non-NULL the actions used are written there (-1 for None). */
int mg_step_random(const mg_params* params, const mg_state* state, int8_t* a1_out,
                   int8_t* a2_out, const mg_outputs* out, const mg_stats* stats, int64_t n,
                   int64_t env_offset, uint64_t seed, uint64_t step_idx,
                   int32_t opponent_random, uint32_t flags, void* stream);

/* num_steps consecutive steps with device-drawn actions in ONE launch: identical results to
 * num_steps calls of mg_step_random with step_idx = first_step + t, output of step t written
 * to slice t of *traj. Each env stays in registers for the whole launch, so its state is read
 * and written once instead of once per step. Replaces the callers' collection loop around
 * MergeEnv.step (scripts/main.py:192-220, scripts/hdqn.py:288-323) for a random policy. */
int mg_rollout_random(const mg_params* params, const mg_state* state, const mg_traj* traj,
                      const mg_stats* stats, int64_t n, int64_t env_offset, uint64_t seed,
                      uint64_t first_step, int32_t num_steps, int32_t opponent_random,
                      uint32_t flags, void* stream);

/* ---- DQN policy (scripts/main.py:30-47 Net, :99-112 choose_action) ---------------------------
 * A packed Q-net is one device buffer of mg_qnet_packed_bytes() bytes (16-byte aligned) made by
 * mg_qnet_pack from the fp32 torch tensors fc1.weight [200,in], fc1.bias [200], fc2.weight
 * [100,200], fc2.bias [100], out.weight [out,100], out.bias [out] (device pointers, row-major).
 * Weights are stored as bf16; each fp32 bias as three bf16 parts (hi + mid + lo == bias exactly)
 * in padded K slots whose inputs are 1.0, so the matrix cores add it inside the K sum; hidden
 * sizes are the reference's 200 and 100; 1 <= in_dim <= 13, 1 <= out_dim <= 8. ABI 19: the buffer
 * holds two layouts of the same bf16 values -- first the operand fragments of the 16x16x32 forward
 * (self-play / other-net opponents, h-DQN, mg_qnet_forward), then the 32x32x16 layout of the
 * config-5 instances without a net opponent. */
size_t mg_qnet_packed_bytes(void);
int mg_qnet_pack(const float* fc1_w, const float* fc1_b, const float* fc2_w, const float* fc2_b,
                 const float* out_w, const float* out_b, int32_t in_dim, int32_t out_dim,
                 void* packed, void* stream);

/* The fragment-major copy of a packed net, mg_qnet_fragment_bytes() = mg_qnet_packed_bytes(). Since
 * ABI 19 the packed layout itself is fragment-major -- the MFMA operand fragments of one forward in
 * the order the kernel consumes them, each the 64 lanes' 16 bytes contiguous (1 KB; the four
 * layer-3 fragments 512 B) -- so this is a plain copy, kept for ABI-18 callers (ABI 18: a
 * separate 66-KB layout). mg_rollout_hdqn reads an opponent from another checkpoint
 * (opponent_mode 3) from global memory in this layout: a fragment load touches 8 cache lines.
 * fragments: 16-byte aligned device buffer. */
size_t mg_qnet_fragment_bytes(void);
int mg_qnet_fragments(const void* packed, void* fragments, void* stream);

/* q[n,8] fp32 = Net(x[n,in_dim]) with bf16 operands and fp32 accumulation (rows >= out_dim are
 * padding; in_dim is the net's, 1..13: 10 for main.py's Net on observations, 11 for hdqn.py's
 * lower-level Net on goal states [goal] + state, :145, :291). swap_halves != 0 (in_dim 10 only)
 * feeds the opponent's view x[5:] + x[:5] (main.py:199). */
int mg_qnet_forward(const void* packed, const float* x, int32_t in_dim, int32_t swap_halves, float* q,
                    int64_t n, void* stream);

/* num_steps steps in ONE launch with the epsilon-greedy Q-net policy computed on the device,
 * Philox4x32-10 draws with key = seed. The ego acts greedily (argmax of Q(obs), lowest index on
 * ties) when its explore draw e < greedy_threshold and at random otherwise -- greedy_threshold =
 * round(Phi(0.7) 2^32) reproduces `np.random.randn() <= EPISILO` (main.py:105).
 * opponent_mode 0 (None) and 1 (uniform) -- two draws per step (ABI 20): step k = first_step + t
 * of env gi = env_offset + i takes words (u0, u1) of counter (gi, k div 2) when k is even and
 * (u2, u3) when k is odd; e = the first, and the second w gives the random action floor(5 w / 2^32)
 * (mode 0, opponent None) or the pair x = floor(25 w / 2^32), a1 = x div 5 (used when exploring),
 * a2 = x mod 5 (the uniform opponent, mode 1).
 * opponent_mode 2 and 3 -- counter (gi, k): u0 / u1 the ego's explore draw / random action
 * floor(5 u1 / 2^32), u2 / u3 the opponent's with opp_greedy_threshold: the same net on the swapped
 * observation (2, Strategy_OP "selfplay", main.py:165-166),
 * or another packed net opp_net (same out_dim) on the swapped observation the same way (3,
 * main.py's default Strategy_OP "L1": a separately trained DQN as the opponent, :161-168, :199;
 * ABI 14; opp_net is ignored by the other modes). Outputs as mg_rollout_random
 * (traj->obs[t] = observation after step t, the network input of step t + 1). */
int mg_rollout_qnet(const mg_params* params, const mg_state* state, const mg_traj* traj,
                    const mg_stats* stats, int64_t n, int64_t env_offset, uint64_t seed,
                    uint64_t first_step, int32_t num_steps, const void* net, int32_t out_dim,
                    uint64_t greedy_threshold, int32_t opponent_mode,
                    uint64_t opp_greedy_threshold, const void* opp_net, uint32_t flags, void* stream);

/* ---- a population acting in one launch (additive to ABI 21) ------------------------------------
 * mg_rollout_qnet for `members` (1 .. 64) actors on ONE env batch of n = members * n_member envs: member m
 * owns envs [m n_member, (m + 1) n_member) and acts there with its own net, opponent net (opponent_mode 3:
 * any packed net of the same out_dim, another member's included -- cross-play), seed and thresholds.
 * state, traj and stats are the whole batch's ([T, n, ...] trajectory rows, ceil(n / 64) won-mask words per
 * step); params, opponent_mode, out_dim, first_step, num_steps, flags and env_offset are shared. The Philox
 * env index stays env_offset + i with i the index in the whole batch, so member m is bit for bit
 * mg_rollout_qnet on its slice alone: n = n_member, env_offset + m n_member, its mg_qnet_actor's fields.
 * The member is a grid dimension: members * ceil(n_member / 1024) blocks, each reading its member's scalars
 * from the kernel argument, so changing a threshold or seed between calls allocates and synchronises
 * nothing. n_member must be a multiple of 64 (a won-mask word covers 64 envs and is stored whole, so two
 * members never share one). Refused before any launch: a NULL or misaligned pointer (each member's net,
 * and its opp_net in mode 3), members outside 1 .. 64, n_member % 64 != 0, opponent_mode outside 0 .. 3;
 * n_member == 0 or num_steps == 0 returns 0 and launches nothing. */
typedef struct mg_qnet_actor {
  const void* net;      /* packed Q-net (mg_qnet_pack), 16-byte aligned */
  const void* opp_net;  /* opponent_mode 3: the member's opponent; ignored otherwise */
  uint64_t seed;
  uint64_t greedy_threshold;
  uint64_t opp_greedy_threshold;
} mg_qnet_actor;

int mg_rollout_qnet_many(const mg_params* params, const mg_state* state, const mg_traj* traj,
                         const mg_stats* stats, int64_t n_member, int32_t members, int64_t env_offset,
                         uint64_t first_step, int32_t num_steps, const mg_qnet_actor* actors, int32_t out_dim,
                         int32_t opponent_mode, uint32_t flags, void* stream);

/* ---- a league: every ordered pair of `nets` nets in one launch (additive to ABI 21) ----------------
 * Cross-play of nets (1 .. 64) packed Q-nets of one out_dim on ONE env batch of n = nets * nets * n_pair envs:
 * pairing p = i nets + j owns envs [p n_pair, (p + 1) n_pair), where net i is the ego and net j its opponent
 * through opponent mode 3 (the diagonal i == j too: the net against a copy of itself on the mode-3 path, not
 * mode 2). The draws are keyed by the ego's seed; each side explores by its own net's threshold. Pairing p is
 * bit for bit mg_rollout_qnet on its slice alone: n = n_pair, env_offset + p n_pair, seed = league[i].seed, net =
 * league[i].net, greedy_threshold = league[i]'s, opponent_mode 3, opp_net = league[j].net, opp_greedy_threshold =
 * league[j]'s. The pairing is a grid dimension: nets^2 * ceil(n_pair / 1024) blocks, each reading its two nets'
 * entries from the kernel argument (nets entries name nets^2 pairings), so a call allocates and synchronises
 * nothing. state, traj and stats are the whole batch's; every traj pointer is optional (an evaluation that reads
 * only the statistics records passes a zeroed mg_traj). n_pair must be a multiple of 64. Refused before any
 * launch: nets outside 1 .. 64, n_pair < 0 or no multiple of 64, a batch past the grid limit, a NULL league, a
 * NULL or misaligned net; n_pair == 0 or num_steps == 0 returns 0 and launches nothing. */
typedef struct mg_league_net {
  const void* net;  /* packed Q-net (mg_qnet_pack), 16-byte aligned */
  uint64_t seed;    /* of the pairings where this net is the ego */
  uint64_t greedy_threshold;
} mg_league_net;

int mg_rollout_qnet_league(const mg_params* params, const mg_state* state, const mg_traj* traj,
                           const mg_stats* stats, int64_t n_pair, int32_t nets, int64_t env_offset,
                           uint64_t first_step, int32_t num_steps, const mg_league_net* league, int32_t out_dim,
                           uint32_t flags, void* stream);

/* ---- h-DQN acting loop (scripts/hdqn.py:280-323) ----------------------------------------------
 * The per-step outputs of mg_rollout_hdqn besides mg_traj, [T, n] fp32 each (NULL skips one):
 * exactly the goal columns and intrinsic reward hdqn.py's lower-level store_transition takes
 * (:291, :304, :314, :316) -- feed them to mg_replay_store as mg_transitions.goal / next_goal /
 * reward for the 24-float goal rows. */
typedef struct mg_hdqn_traj {
  float* goal;       /* goal of step t's goal state [goal] + state (:291) */
  float* next_goal;  /* goal Goal_DQN chose on step t's next state (:303; the terminal one at an
                        episode end), the row's next goal */
  float* reward;     /* 1.0 if next_goal == goal_status(state) else 0.0 (:314) */
  float* goal_op;    /* (optional, opponent_mode 2 / 3) the opponent's goal of step t, the
                        goal of its goal state [goal_op] + swapped state (:285, :299) */
  float* ext_reward; /* (optional, ABI 15) extrinsic reward summed since the inner loop began,
                        through step t (:286, :311-313): Goal_DQN's row reward at a break;
                        needs ext_acc */
  uint64_t* no_break; /* (optional, ABI 15) [T, ceil(n/64)] bit i of word t ceil(n/64) + i/64 set
                        where step t did not end the inner loop (:322): the rows Goal_DQN does not
                        store (mg_transitions.meta_goal) */
} mg_hdqn_traj;

/* num_steps steps of hdqn.py's inner loop in ONE launch (opponent L0 or uniform random): per env
 * and step, the lower-level Net (lower_net: in 11, out 5) acts epsilon-greedily on the goal
 * state [goal] + state, the env steps, Goal_DQN's meta-net (meta_net: in 10, out num_goals)
 * chooses the next goal epsilon-greedily on the next state, goal_status gives the intrinsic
 * reward, and a fresh goal is chosen when that goal is already reached or the episode ended
 * (:320-322, :278-283; reset_goal = the meta-net's argmax on the reset observation, which the
 * caller computes once). goal_status is evaluated on the fp64 x2 - x1 and v2 of the state (ABI 17;
 * see mg_goal_status). flags must include MG_AUTORESET (hdqn.py resets at every episode end, :277;
 * ABI 17 rejects a launch without it). goal [n] int8 holds each env's current goal across launches (< 0: none
 * yet -- chosen by the meta-net at the first step). Random draws: Philox4x32-10 with key seed,
 * counter (env_offset + i, first_step + t) for the action and next goal (x, y, z, w = explore,
 * action, explore, goal) and stream B, counter ((env_offset + i) ^ 2^63, c), for a fresh goal's
 * explore / goal draws of step k: with the uniform opponent (mode 1) words (x, y) of c = k, its
 * action from z; otherwise (ABI 20) one call per two steps, c = k div 2, words (x, y) on even k
 * and (z, w) on odd k. A launch's first fresh goals use step first_step - 1.
 * Greedy when the explore draw < greedy_threshold (np.random.randn() <= EPISILO, :84, :168).
 * traj as mg_rollout_qnet; opponent_mode 0 (None, Strategy_OP "L0", :261, :294-296), 1 (uniform),
 * 2 (Strategy_OP "selfplay", :262-264: upper_op = upper, lower_op = lower, so the same two
 * nets) or 3 (any other Strategy_OP, :265-268: upper_op / lower_op loaded from another h-DQN
 * checkpoint -- opp_meta_net / opp_lower_net, the mg_qnet_fragments copies of its packed nets
 * (ABI 18; packed nets until ABI 17), 16-byte aligned, ignored by the other modes; ABI 16. Four
 * nets exceed one CU's LDS, so the opponent's two are read from global memory, where they stay
 * L2-resident): the opponent's goal is chosen by its
 * meta-net on the swapped state
 * state[5:] + state[:5] at every outer-loop iteration (:285 -- the launch's first step when
 * goal_op[i] < 0, and the step after a break: the ego's goal reached or the episode ended) and
 * kept in between; its action is its lower net's epsilon-greedy choice on
 * [goal_op] + swapped state every step (:299-300). Its draws: counter
 * ((env_offset + i) ^ 2^62, first_step + t), x explore and y action of step t, z explore and
 * w goal of a fresh opponent goal at step t + 1 (the launch's first at step first_step - 1).
 * goal_op [n] int8 (required for modes 2 and 3, else ignored) holds each env's opponent goal across
 * launches like goal. ext_acc [n] double (required with htraj->ext_reward or no_break, ABI 15)
 * holds each env's extrinsic reward since its inner loop began, across launches (0 at a break);
 * whenever it is given the sums are kept, with or without those outputs (ABI 17).
 * ring_rows (optional, 16-byte aligned [ring_capacity, 24] fp32, with ring_counter: one device
 * uint64): the launch also appends every transition to hdqn.py's lower-level memory
 * (HDQN.store_transition, :316, which stores them all) -- row [goal, s, a, r, next_goal, s'] of
 * (t, i) at slot (counter + t n + i) % ring_capacity, exactly what mg_replay_store with
 * skip_ego_won = 0 writes from this launch's outputs (only the newest ring_capacity rows when
 * more are appended), then counter += T n. No scan is needed since every row is kept. */
int mg_rollout_hdqn(const mg_params* params, const mg_state* state, const mg_traj* traj,
                    const mg_hdqn_traj* htraj, const mg_stats* stats, int8_t* goal, int8_t* goal_op,
                    double* ext_acc, int64_t n,
                    int64_t env_offset, uint64_t seed, uint64_t first_step, int32_t num_steps,
                    const void* meta_net, int32_t num_goals, const void* lower_net, int32_t reset_goal,
                    uint64_t greedy_threshold, int32_t opponent_mode, const void* opp_meta_net,
                    const void* opp_lower_net, float* ring_rows,
                    uint64_t* ring_counter, int64_t ring_capacity, uint32_t flags, void* stream);

/* status[i] = goal_status on (dx1[i], v2[i]) in fp64 (ABI 17): 0 if dx1 < -0.5 v2, 1 if dx1 < 0.5 v2,
 * else 2 -- replaces hdqn.py's goal_status (scripts/hdqn.py:223-236, dx1 = state[0], v2 = state[9]),
 * the same device function mg_rollout_hdqn evaluates on each step's fp64 x2 - x1 and v2 for the
 * intrinsic reward (:314) and the inner-loop break (:322). Device pointers, stream-ordered. */
int mg_goal_status(const double* dx1, const double* v2, int8_t* status, int64_t n, void* stream);

/* ---- replay memory (scripts/main.py:91-92, :115-119, :130-135) --------------------------------
 * rows: [capacity, row_floats] fp32 device buffer, row = [s(10), a, r, s'(10)] like
 * np.hstack((state, [action, reward], next_state)) (row_floats 22), or the goal-augmented
 * [goal, s(10), a, r, next_goal, s'(10)] of hdqn.py's lower memory (row_floats 24, tr->goal set);
 * counter: one device uint64, the reference's memory_counter.
 * mg_replay_store appends the transitions of *tr in (t, i) order -- the order in which
 * stepping env 0..n-1 at each step and calling store_transition would append them -- at
 * slot (memory_counter + k) % capacity, skipping those whose won bit is set when
 * skip_ego_won != 0 (main.py:209 `if env.winner is not 1`; hdqn.py:316 stores every one), and
 * adds the number appended to *counter. When more than capacity transitions are appended only
 * the newest capacity are written, as sequential stores would leave them. scratch: a device
 * buffer of at least mg_replay_scratch_bytes(n, num_steps) bytes, 8-byte aligned, any contents;
 * one scratch buffer per stream. Three launches, stream-ordered, no host synchronisation. */
size_t mg_replay_scratch_bytes(int64_t n, int32_t num_steps);
int mg_replay_store(float* rows, uint64_t* counter, int64_t capacity, int32_t row_floats,
                    const mg_transitions* tr, int64_t n, int32_t num_steps, int32_t skip_ego_won,
                    void* scratch, size_t scratch_bytes, void* stream);

/* (additive to ABI 21) mg_replay_store for `members` (1 .. 64) rings from ONE [T, N, ...] mg_transitions,
 * N = members * n_member: member m's transitions -- columns [m n_member, (m + 1) n_member) -- go to
 * rows[m] / counters[m] (host arrays of device pointers) in the member's own (t, i) order, i within its
 * slice, at slot (counter_m + k) % capacity; the skip_ego_won filter and the newest-capacity rule apply per
 * member, then counter_m += kept_m: exactly what mg_replay_store leaves when given a contiguous copy of the
 * slice. The tensors are read in place (rows stride by N, the won mask has ceil(N / 64) words per step);
 * the same three launches with the member as a grid dimension. n_member must be a multiple of 64 (a
 * member's won bits begin a mask word). 22-float rows only: goal, next_goal and meta_goal are refused, as
 * is a ring listed twice (two members' appends to one ring have no defined order). capacity and
 * skip_ego_won are shared. scratch: mg_replay_scratch_many_bytes(n_member, num_steps, members) =
 * members * mg_replay_scratch_bytes(n_member, num_steps) bytes (0 for members outside 1 .. 64), 8-byte
 * aligned. n_member == 0 or num_steps == 0 returns 0. */
size_t mg_replay_scratch_many_bytes(int64_t n_member, int32_t num_steps, int32_t members);
int mg_replay_store_many(float* const* rows, uint64_t* const* counters, int32_t members, int64_t capacity,
                         int32_t row_floats, const mg_transitions* tr, int64_t n_member, int32_t num_steps,
                         int32_t skip_ego_won, void* scratch, size_t scratch_bytes, void* stream);

/* out[batch, row_floats] = rows[idx[b]], idx[b] = floor(u0 * M / 2^32) with u = Philox4x32-10(key = seed,
 * counter = (b, draw)) and M = capacity (np.random.choice(MEMORY_CAPACITY, BATCH_SIZE),
 * main.py:130 -- the reference learns only once the memory is full) or, when filled_only != 0,
 * M = min(*counter, capacity) (at least 1). idx_out[batch] (int64, may be NULL) gets the slots. */
int mg_replay_sample(const float* rows, const uint64_t* counter, int64_t capacity,
                     int32_t row_floats, uint64_t seed, uint64_t draw, int32_t filled_only,
                     float* out, int64_t* idx_out, int64_t batch, void* stream);

/* (ABI 20) *totals = the n records summed on the device, in a fixed order so the fp64 sums are
 * reproducible bit for bit: blocks of 1,024 records, thread t of 256 adding records t, t + 256,
 * t + 512, t + 768 of its block in that order onto -0.0, the 256 values folded in halves
 * (v[t] += v[t + o] for o = 128, 64, ..., 1); then the block partials the same way (thread t adding
 * partials t, t + 256, ... in order, then the fold). Counts are exact. scratch: device buffer of at
 * least mg_stats_reduce_scratch_bytes(n) bytes (16-byte aligned); rec 16-byte aligned, totals (a
 * device mg_stats_totals) 8-byte aligned. Two launches, stream-ordered; n == 0 gives zero counts
 * and -0.0 sums. */
size_t mg_stats_reduce_scratch_bytes(int64_t n);
int mg_stats_reduce(const mg_episode_stats* rec, int64_t n, mg_stats_totals* totals, void* scratch,
                    size_t scratch_bytes, void* stream);

/* (additive to ABI 21) mg_stats_reduce on `segments` (1 .. 4096) equal runs of the records at once:
 * totals[s] = records [s n_segment, (s + 1) n_segment) summed in mg_stats_reduce's order, bit for bit what
 * mg_stats_reduce(rec + s n_segment, n_segment, ...) gives -- the members of mg_rollout_qnet_many or the pairings
 * of mg_rollout_qnet_league. The same two launches with the segment as a grid dimension. scratch: at least
 * mg_stats_reduce_many_scratch_bytes(n_segment, segments) = segments * mg_stats_reduce_scratch_bytes(n_segment)
 * bytes (0 for segments outside 1 .. 4096), 16-byte aligned; rec 16-byte, totals (segments device
 * mg_stats_totals) 8-byte aligned. n_segment == 0 gives every segment zero counts and -0.0 sums. */
size_t mg_stats_reduce_many_scratch_bytes(int64_t n_segment, int32_t segments);
int mg_stats_reduce_many(const mg_episode_stats* rec, int64_t n_segment, int32_t segments, mg_stats_totals* totals,
                         void* scratch, size_t scratch_bytes, void* stream);

/* Resets the envs whose mask byte is non-zero (mask == NULL: all n) and writes their reset
 * observation to out->obs / out->rec64 when given. Replaces MergeEnv.reset (merging_env.py:208-230). */
int mg_reset(const mg_params* params, const mg_state* state, const uint8_t* mask,
             const mg_outputs* out, int64_t n, void* stream);

/* Observation and collision test of the current state, no state change: out->obs /
 * out->rec64 (obs only) and out->coll. Replaces MergeEnv.observe (merging_env.py:118-132)
 * and MergeEnv.is_collided (:198-206). */
int mg_observe(const mg_params* params, const mg_state* state, const mg_outputs* out, int64_t n,
               void* stream);

/* ---- host (CPU) path, ABI 20 ---------------------------------------------------------------------
 * The same step, reset and observation functions the kernels run, compiled for the host and applied
 * to HOST pointers, synchronously, one env after another: every output and condition is exactly
 * mg_step's / mg_reset's / mg_observe's (done_mask / won_mask words per 64 envs included), and the
 * doubles are the kernel's bit for bit (the host build has no contraction either), except that sin /
 * cos for |theta| >= 1/16 are glibc's there and the device library's on the GPU, within 1 ulp of each
 * other: live episodes do reach such angles once a car has arrived. For one env at the scripts'
 * pace (merging_env.py:138-230 called per step, scripts/human_player.py:112-187) a step costs
 * ~1 us here against a kernel launch plus a stream synchronisation on the GPU; batches belong on
 * the device (mg_step and the rollout kernels). */
int mg_host_step(const mg_params* params, const mg_state* state, const int8_t* a1, const int8_t* a2,
                 const mg_outputs* out, const mg_stats* stats, int64_t n, uint32_t flags);
int mg_host_reset(const mg_params* params, const mg_state* state, const uint8_t* mask,
                  const mg_outputs* out, int64_t n);
int mg_host_observe(const mg_params* params, const mg_state* state, const mg_outputs* out, int64_t n);

/* ---- DQN.learn on the device, ABI 21 --------------------------------------------------------------
 * One learner serves DQN.learn (scripts/main.py:122-157, Net 10 -> 5), HDQN.learn (hdqn.py:186-221,
 * 11 -> 5 on the 24-float goal rows) and Goal_DQN.learn (hdqn.py:104-139, 10 -> 3): Double-DQN target,
 * MSE loss, Adam (main.py:96, lr 0.01), the target net copied from the eval net every target_period
 * learns (main.py:125-127). Net is main.py:30-47: Linear(in, 200), ReLU, Linear(200, 100), ReLU,
 * Linear(100, out).
 *
 * The learner is one caller-owned device buffer of mg_dqn_learner_bytes(in_dim, out_dim) = 16 P bytes,
 * P = 200 in + 200 + 20000 + 100 + 100 out + out: four blocks of P contiguous fp32 -- eval parameters,
 * target parameters, Adam's exp_avg (m), Adam's exp_avg_sq (v) -- each in torch's parameter order
 * fc1.weight [200, in], fc1.bias, fc2.weight [100, 200], fc2.bias, out.weight [out, 100], out.bias.
 * mg_dqn_learner_init copies six fp32 device tensors into eval and target and zeroes m and v.
 *
 * A row of the replay memory is [x(in), a, r, x'(in)], row_floats = 2 in + 2 (mg_replay_store's 22-
 * and 24-float rows). The minibatch of update u is exactly what mg_replay_sample(seed, draw =
 * first_draw + u, filled_only) returns for the same ring.
 *
 * Arithmetic: fp32, in this fixed order -- the same for every grid, with no float atomics -- where
 * fmaf is the correctly rounded fused multiply-add and every other operation is rounded once:
 *   forward, per layer  y[b, j] = fmaf(x[b, K-1], W[j, K-1], ... fmaf(x[b, 0], W[j, 0], bias[j])), k
 *                       ascending; the hidden layers keep h = y > 0 ? y : 0. Three passes: eval on x,
 *                       eval on x', target on x'.
 *   target and loss     a = the row's action column truncated to int (kept inside 0 .. out - 1; NaN: 0);
 *                       am = argmax_j eval(x')[j], lowest index on ties; t = r + gamma * target(x')[am]
 *                       (one product, one add); d[b] = eval(x)[a] - t;
 *                       loss = (((0 + d[0] d[0]) + d[1] d[1]) + ...) * fp32(1 / B);
 *                       dq[b, a] = d[b] * fp32(2 / B), 0 for the other actions.
 *   backward, per layer dW[j, k] = the fmaf chain over b ascending of dy[b, j] x[b, k] from +0;
 *                       db[j] = ((0 + dy[0, j]) + dy[1, j]) + ...;
 *                       dx[b, k] = the fmaf chain over j ascending of dy[b, j] W[j, k] from +0, then 0
 *                       where the layer's input h[b, k] is not > 0.
 *   Adam, per parameter m = fmaf(fp32(1 - beta1), g, fp32(beta1) * m);
 *                       v = fmaf(fp32(1 - beta2) * g, g, fp32(beta2) * v);
 *                       den = sqrtf(v) / fp32(sqrt(1 - beta2^s)) + fp32(eps);
 *                       p = p - fp32(lr / (1 - beta1^s)) * (m / den), s = update number + 1;
 *                       the scalars inside fp32( ) are computed on the host in double (libm pow and
 *                       sqrt) and rounded once.
 *   target copy         before update number t = first_update + u (counted from 0), when
 *                       t % target_period == 0, target = eval.
 * gamma is rounded to fp32 once. fp32 division and sqrtf are correctly rounded on both sides, so
 * mg_host_dqn_learn -- the same functions on HOST pointers, synchronously, like mg_host_step -- gives
 * the kernels' bits.
 *
 * mg_dqn_learn enqueues num_updates updates back to back on `stream` with no host synchronisation:
 * seven launches each (layer 1 with the row gather, layer 2, layer 3 with target and dq, three
 * backward layers, Adam), one more when the target copy is due. loss_out [num_updates] and rows_out
 * [num_updates, batch, row_floats] (the sampled rows) are optional. packed_out (optional, 16-byte
 * aligned, mg_qnet_packed_bytes()): the eval net after the last update in mg_qnet_pack's layout, so
 * the acting kernels read the new weights. scratch: mg_dqn_learn_scratch_bytes(batch, in_dim,
 * out_dim) bytes, 16-byte aligned, any contents, one per stream. Accepted: 1 <= in_dim <= 13,
 * 1 <= out_dim <= 8, row_floats == 2 in_dim + 2, 1 <= batch <= 1024, 1 <= capacity <= 2^32,
 * target_period >= 1, 0 <= beta < 1, num_updates >= 0 (0 is a no-op); counter is read only with
 * filled_only. learner 16-byte, rows and counter 8-byte, loss_out and rows_out 4-byte aligned. */
typedef struct mg_dqn_hyper {
  double lr;             /* main.py:13 LR = 0.01 */
  double gamma;          /* main.py:14 GAMMA = 0.9 */
  double beta1;          /* torch.optim.Adam's defaults: 0.9, 0.999, 1e-8 */
  double beta2;
  double eps;
  int32_t target_period; /* main.py:17 Q_NETWORK_ITERATION = 100 */
  int32_t reserved;      /* 0 */
} mg_dqn_hyper;

size_t mg_dqn_learner_bytes(int32_t in_dim, int32_t out_dim);
int mg_dqn_learner_init(float* learner, const float* fc1_w, const float* fc1_b, const float* fc2_w,
                        const float* fc2_b, const float* out_w, const float* out_b, int32_t in_dim,
                        int32_t out_dim, void* stream);
size_t mg_dqn_learn_scratch_bytes(int32_t batch, int32_t in_dim, int32_t out_dim);
int mg_dqn_learn(float* learner, const float* rows, const uint64_t* counter, int64_t capacity, int32_t row_floats,
                 int32_t in_dim, int32_t out_dim, int32_t batch, int32_t num_updates, uint64_t first_update,
                 uint64_t seed, uint64_t first_draw, int32_t filled_only, const mg_dqn_hyper* hyper, float* loss_out,
                 float* rows_out, void* packed_out, void* scratch, size_t scratch_bytes, void* stream);
int mg_host_dqn_learn(float* learner, const float* rows, const uint64_t* counter, int64_t capacity,
                      int32_t row_floats, int32_t in_dim, int32_t out_dim, int32_t batch, int32_t num_updates,
                      uint64_t first_update, uint64_t seed, uint64_t first_draw, int32_t filled_only,
                      const mg_dqn_hyper* hyper, float* loss_out, float* rows_out, void* scratch,
                      size_t scratch_bytes);

/* ---- A population of DQN learners in one set of launches (additive to ABI 21) -----------------------
 * `members` (1 .. 64) independent learners of one shape (in_dim, out_dim, batch, capacity), each on its
 * own net, memory, seed, counters and hyperparameters, trained by the same launches: one update of all
 * members is mg_dqn_learn's seven launches with the member in the grid, an eighth (the target copy, under
 * a 64-bit member mask) when any member's copy is due, and the repack of all eval nets is two launches
 * per call. Nothing in mg_dqn_learn_many synchronises or copies from the host.
 *
 * Contract: for every member m, the effect on its learner block, its losses, its rows and its packed net
 * is bit for bit that of mg_dqn_learn on that member's buffers with that member's seed, first_update,
 * first_draw and hyper (the kernels rebase the member and run the same per-element functions). K updates
 * in one call equal K calls.
 *
 * Member state is contiguous: learners [members, 4 P] fp32 (member m's block is an mg_dqn_learn learner),
 * scratch [members, mg_dqn_learn_scratch_bytes(batch, in_dim, out_dim)], packed_out [members,
 * packed_stride] bytes (optional; packed_stride a multiple of 16, >= mg_qnet_packed_bytes()). Each member's
 * ring and counter come by pointer in its mg_dqn_member, so members may share one ring (it is only read).
 * loss_out [num_updates, members] and rows_out [num_updates, members, batch, row_floats] are optional.
 *
 * `member` is a HOST array of `members` entries. What does not change from update to update -- rows,
 * counter, seed, gamma, Adam's betas and eps, each rounded as mg_dqn_learn rounds it -- lives in a device
 * table of mg_dqn_learn_many_table_bytes(members) bytes (16-byte aligned) that mg_dqn_learn_many_init
 * writes on `stream` from the same array; call it again after changing any of those fields. Each
 * update's draw index, Adam's step and bias-correction scalars (from the host's doubles, libm pow) and
 * the copy mask travel in the kernel argument. On success mg_dqn_learn_many and mg_host_dqn_learn_many
 * advance every member's first_update and first_draw by num_updates, so the next call continues the run.
 * mg_host_dqn_learn_many is the loop over members of mg_host_dqn_learn's update, on HOST pointers, and
 * needs no table.
 *
 * Refused before anything is read or launched: members outside 1 .. 64, NULL pointers (counter only with
 * filled_only), what mg_dqn_learn refuses of the shape, any member's target_period < 1 or betas outside
 * [0, 1) (the text names the member), misaligned pointers or stride (learners, scratch, table, packed_out
 * 16-byte; every member's rows and counter 8-byte; loss_out, rows_out 4-byte), scratch smaller than
 * members * mg_dqn_learn_scratch_bytes, table smaller than mg_dqn_learn_many_table_bytes. */
typedef struct mg_dqn_member {
  const float* rows;       /* the member's ring [capacity, row_floats] */
  const uint64_t* counter; /* its counter (read only with filled_only) */
  uint64_t seed;           /* key of its minibatch draws */
  uint64_t first_update;   /* updates it has made: Adam's step count - 1, the target copy's clock */
  uint64_t first_draw;     /* minibatches it has drawn */
  mg_dqn_hyper hyper;
} mg_dqn_member;

size_t mg_dqn_learn_many_table_bytes(int32_t members); /* 0 outside 1 .. 64 */
int mg_dqn_learn_many_init(void* table, size_t table_bytes, const mg_dqn_member* member, int32_t members,
                           void* stream);
int mg_dqn_learn_many(float* learners, const void* table, size_t table_bytes, mg_dqn_member* member, int32_t members,
                      int64_t capacity, int32_t row_floats, int32_t in_dim, int32_t out_dim, int32_t batch,
                      int32_t num_updates, int32_t filled_only, float* loss_out, float* rows_out, void* packed_out,
                      size_t packed_stride, void* scratch, size_t scratch_bytes, void* stream);
int mg_host_dqn_learn_many(float* learners, mg_dqn_member* member, int32_t members, int64_t capacity,
                           int32_t row_floats, int32_t in_dim, int32_t out_dim, int32_t batch, int32_t num_updates,
                           int32_t filled_only, float* loss_out, float* rows_out, void* scratch,
                           size_t scratch_bytes);

/* ---- Rainbow acting (additive to ABI 21) ------------------------------------------------------------
 * The acting path of scripts/ranbowdqn.py: RainbowDQN.forward / act (:517-548) and the loop that calls
 * them once per env step (:662-680). The net is exactly the reference's RainbowDQN(10, 5): Linear(10, 32),
 * ReLU, Linear(32, 64), ReLU; value stream NoisyLinear(64, 64), ReLU, NoisyLinear(64, 51); advantage
 * stream NoisyLinear(64, 64), ReLU, NoisyLinear(64, 5 * 51); support z = linspace(Vmin, Vmax, 51). The
 * caller passes each layer's EFFECTIVE fp32 weight and bias (mu + sigma * epsilon of a noisy layer in
 * training mode, :468-470, or mu), so between two reset_noise() calls the policy is a fixed function. Learning
 * (compute_td_loss :584-609, projection_distribution :554-582) is the next section's.
 *
 * mg_rainbow_pack (replaces nothing of the reference: it prepares the weights): writes
 * mg_rainbow_packed_bytes() = 74,192 bytes, 16-byte aligned -- bf16 weights (round to nearest even) as the
 * forward's MFMA fragments in consumption order, the fp32 biases of layers 2..6, the fp32 support. Accepted:
 * in_dim 10, hidden 32 / 64 / 64, 5 actions, 51 atoms; any other shape is refused.
 *
 * Arithmetic of the forward (mg_rainbow_forward, mg_rollout_rainbow), the contract the tests restate:
 *   matrix layers  bf16 operands, fp32 accumulation on v_mfma_f32_16x16x32_bf16, one chain of MFMAs per
 *                  output over its k-blocks of 32 in ascending order. The input is x[j] = obs[(j + rotate)
 *                  % 10] rounded to bf16. Layer 1 (K = 10): the chain starts at +0 and b1 is inside the K
 *                  sum as three bf16 parts hi + mid + lo == b1 at k = 10, 11, 12 against inputs 1.0 (k = 13
 *                  .. 31 are zero). Layers 2..6 (K = 32 or 64): the chain starts from the fp32 bias; within
 *                  a k-block of 32 the hidden unit at k = 8 g + j is 32 kb + 16 (j >> 2) + 4 g + (j & 3).
 *                  A hidden activation is the accumulator rounded to bf16 once, then max(., +0).
 *   head, fp32     in this fixed order (no contraction; every operation rounded once), per env, with
 *                  v[i] the value logits and A[a][i] the advantage logits:
 *                    mean[i] = ((((A[0][i] + A[1][i]) + A[2][i]) + A[3][i]) + A[4][i]) / 5
 *                    x[a][i] = (v[i] + A[a][i]) - mean[i]
 *                    m[a]    = max_i x[a][i]
 *                    e[a][i] = exp(x[a][i] - m[a])   (below)
 *                    S[a], N[a]: the 51 atoms as FOUR chains over i = 13 g .. min(13 g + 12, 50), g = 0..3,
 *                              each from +0 in ascending i -- S_g = S_g + e, N_g = N_g + e * z[i] (product
 *                              rounded, then the sum) -- combined as (c0 + c1) + (c2 + c3)
 *                    q[a]    = N[a] / S[a];   action = the lowest a with the largest q[a].
 *                  (Four chains, not one over i = 0..50: the lane that holds an accumulator row owns its
 *                  atom, and a column of the 16x16 tile is spread over four lanes.)
 *   exp            the library's own, identical bits on host and device: 0 for x < -87 (and NaN); else
 *                  k = rint(x * fp32(log2 e)), r = fmaf(k, 2.12194440e-4f, fmaf(k, -0.693359375f, x)),
 *                  p = the degree-7 Taylor polynomial of exp(r) in Horner form, one fmaf per coefficient
 *                  1/5040, 1/720, 1/120, 1/24, 1/6, 1/2, 1, 1, and the result p * 2^k (exact: normal).
 *                  Never the hardware exponential.
 *
 * mg_rainbow_forward replaces RainbowDQN.forward up to the logits and act() (:543-548) for obs [n, 10]:
 * optional outputs logits [n, 306] (value [51], then advantage [5][51]: the rows the head consumes), q [n, 5]
 * fp32 and action [n] int8; a NULL output is not written. 0 <= rotate < 10; the opponent's view
 * state[3:] + state[:3] (:669) is rotate = 3.
 *
 * mg_rollout_rainbow replaces :662-680 (act, act on the rotated view, env.step, reset at an episode end) for
 * num_steps steps in one launch: mg_rollout_qnet's arguments without the Philox ones (there is no draw).
 * opponent_mode 0: action_op = None, the env's own L0 opponent; 2: the same net on the rotated view.
 * traj and stats as mg_rollout_random; mg_episode_stats.q_eval is left unchanged (the script logs none) and
 * ret1_sum is ranbowdqn.py's episode_reward (:676).
 *
 * mg_host_rainbow_head: the head above on HOST memory, synchronously -- logits [n, 306] and support [51] to
 * q [n, 5] and action [n] (either may be NULL) -- the same functions the kernels compile.
 * mg_host_rainbow_exp: y[i] = that exp of x[i] on host memory, so its error can be measured (the head only
 * ever passes x <= 0; x > 0 gives NaN here). */
size_t mg_rainbow_packed_bytes(void);
int mg_rainbow_pack(const float* linear1_w, const float* linear1_b, const float* linear2_w, const float* linear2_b,
                    const float* value1_w, const float* value1_b, const float* value2_w, const float* value2_b,
                    const float* advantage1_w, const float* advantage1_b, const float* advantage2_w,
                    const float* advantage2_b, const float* support, int32_t in_dim, int32_t hidden1,
                    int32_t hidden2, int32_t hidden_stream, int32_t num_actions, int32_t num_atoms, void* packed,
                    void* stream);
int mg_rainbow_forward(const void* packed, const float* obs, int32_t rotate, float* logits, float* q,
                       int8_t* action, int64_t n, void* stream);
int mg_rollout_rainbow(const mg_params* params, const mg_state* state, const mg_traj* traj, const mg_stats* stats,
                       int64_t n, int32_t num_steps, const void* net, int32_t opponent_mode, uint32_t flags,
                       void* stream);
int mg_host_rainbow_head(const float* logits, const float* support, float* q, int8_t* action, int64_t n);
int mg_host_rainbow_exp(const float* x, float* y, int64_t n);

/* ---- a Rainbow population acting in one launch (additive to ABI 21) ----------------------------------
 * mg_rollout_rainbow for `members` (1 .. 64) actors on ONE env batch of n = members * n_member envs: member m
 * owns envs [m n_member, (m + 1) n_member) and acts there with its own packed net nets[m] (a host array of
 * `members` device pointers, each 16-byte aligned; read during the call only). state, traj and stats are the
 * whole batch's ([T, n, ...] trajectory rows, ceil(n / 64) won-mask words per step); params, opponent_mode,
 * num_steps and flags are shared. There is no draw, so there are no seeds and no env_offset: member m is bit
 * for bit mg_rollout_rainbow with nets[m] on its slice alone (n = n_member) -- trajectory rows, env state,
 * episode records and won bits. The member is a grid dimension: members * ceil(n_member / 512) blocks, each
 * copying its member's net into LDS, the nets' addresses in the kernel argument, so a call allocates and
 * synchronises nothing. n_member must be a multiple of 64 (a won-mask word covers 64 envs and is stored whole,
 * so two members never share a wave or a word). opponent_mode 0 or 2 as mg_rollout_rainbow; cross-play (a
 * member against another member's net) is mg_rollout_rainbow_vs_many, below. Refused before anything is read or launched, in this order: members outside 1 .. 64, n_member < 0,
 * n_member % 64 != 0, members * n_member past the grid limit, what mg_rollout_rainbow refuses of params, state
 * and traj, nets NULL, a NULL or misaligned member net (the text names the member), num_steps outside
 * 0 .. 65535, opponent_mode other than 0 or 2, a misaligned traj buffer; then n_member == 0 or num_steps == 0
 * returns 0 and launches nothing. */
int mg_rollout_rainbow_many(const mg_params* params, const mg_state* state, const mg_traj* traj,
                            const mg_stats* stats, int64_t n_member, int32_t members, int32_t num_steps,
                            const void* const* nets, int32_t opponent_mode, uint32_t flags, void* stream);

/* ---- Rainbow against another Rainbow net (additive to ABI 21) -----------------------------------------
 * mg_rollout_rainbow_vs replaces :662-680 with action_op taken from a SECOND model -- action =
 * current_model.act(state), action_op = other_model.act(state[3:] + state[:3]), env.step(action, action_op) --
 * for num_steps steps in one launch: mg_rollout_rainbow's arguments with the opponent's packed net (`opponent`, as
 * `net` a device pointer, 16-byte aligned, mg_rainbow_packed_bytes() long) in the place of opponent_mode. The
 * contract is the composition's, bit for bit: at every step traj.a1 is mg_rainbow_forward(net, obs, rotate 0)'s
 * action, traj.a2 is mg_rainbow_forward(opponent, obs, rotate 3)'s, and everything else is mg_step on those two
 * actions (MFMA columns are independent and the head runs on registers, so a forward inside the rollout is the
 * stand-alone forward's bits). opponent == net is allowed and is then bit for bit opponent_mode 2 of
 * mg_rollout_rainbow: the diagonal of a pairing grid needs no other call.
 * LDS of a 512-env block: the ego's whole net (74,192 B), the opponent's net from its value stream's bias on
 * (both hidden streams, the six head streams, the support: 67,792 B) and the observation tile (20,480 B), 162,464
 * of the CU's 163,840 B; the opponent's first two layers (6,400 B) are read from `opponent` in device memory at
 * every forward, so `opponent` must stay unchanged while the launch runs, as `net` must.
 * Refused before anything is read or launched, in this order: what mg_rollout_rainbow refuses of params, state,
 * traj and n (the same texts), a NULL or misaligned net, a NULL or misaligned opponent, num_steps outside
 * 0 .. 65535 (these three texts start with the call's name), a misaligned traj buffer; then n == 0 or num_steps
 * == 0 returns 0 and launches nothing.
 *
 * mg_rollout_rainbow_vs_many is mg_rollout_rainbow_many with an opponent per member: member m acts with nets[m]
 * against opponents[m] on its slice, bit for bit mg_rollout_rainbow_vs(nets[m], opponents[m]) on the slice
 * alone. opponents is a host array of `members` device pointers like nets; entries may repeat, may be entries
 * of nets, and opponents[m] == nets[m] is member m in self-play. A block of member m copies nets[m] and the stream
 * part of opponents[m] into LDS; all the addresses travel in the kernel argument. Refused in
 * mg_rollout_rainbow_many's order with this call's name in front: the member count and n_member checks, params /
 * state / traj, nets NULL, a NULL or misaligned nets[m], opponents NULL, a NULL or misaligned opponents[m] (the
 * text names the first such member), num_steps, a misaligned traj buffer. */
int mg_rollout_rainbow_vs(const mg_params* params, const mg_state* state, const mg_traj* traj, const mg_stats* stats,
                          int64_t n, int32_t num_steps, const void* net, const void* opponent, uint32_t flags,
                          void* stream);
int mg_rollout_rainbow_vs_many(const mg_params* params, const mg_state* state, const mg_traj* traj,
                               const mg_stats* stats, int64_t n_member, int32_t members, int32_t num_steps,
                               const void* const* nets, const void* const* opponents, uint32_t flags, void* stream);

/* ---- Rainbow learning (additive to ABI 21) ----------------------------------------------------------
 * compute_td_loss (scripts/ranbowdqn.py:584-609) with projection_distribution (:554-582) on the device, and
 * the (s, a, r, s', done) ReplayBuffer (:265-323) it samples from.
 *
 * mg_rainbow_replay_store replaces replay_buffer.push (:281-288, :673) for num_steps steps of n envs: rows
 * [capacity, 24] fp32 = [s(10), a, r, s'(10), done, 0]. Transition (t, i) goes to slot (counter + t n + i) %
 * capacity; s = obs_first[i] at t = 0, else obs[t - 1, i]; s' = final_obs[t, i] where done (and final_obs is
 * given), else obs[t, i]; a and done from a1 / done or from flags; r = rew[t, i, 0]. Every transition is kept
 * (no winner filter); when n num_steps > capacity only the newest `capacity` are written, so no two threads
 * write one slot. One store launch, then counter += n num_steps on the same stream. mg_transitions' goal,
 * next_goal, reward, meta_goal and won_mask have no meaning here (the first four must be NULL).
 * mg_replay_sample(row_floats 24, filled_only 1) draws from these rows.
 *
 * The learner is one caller-owned device buffer of mg_rainbow_learner_bytes() = 4 (4 P + 2 E + 52) bytes,
 * 16-byte aligned: current, target, Adam's exp_avg, Adam's exp_avg_sq -- P = 58,884 fp32 each in
 * RainbowDQN.named_parameters() order: linear1.weight [32, 10], linear1.bias, linear2.weight [64, 32],
 * linear2.bias, then per noisy layer (noisy_value1 [64, 64], noisy_value2 [51, 64], noisy_advantage1
 * [64, 64], noisy_advantage2 [255, 64]) weight_mu, weight_sigma, bias_mu, bias_sigma -- then the current and the
 * target model's noise, E = 28,210 fp32 each: per noisy layer weight_epsilon, bias_epsilon, the full buffers
 * as the reference's state dict holds them -- then the support z[51] and one zero. The caller fills it (a
 * target := current copy, noise included, is update_target, :551-552) and draws the noise factors.
 *
 * One update, fp32, in this fixed order -- the same for every grid, no float atomics; fmaf is the fused
 * multiply-add, every other operation is rounded once:
 *   minibatch   row b = the ring row at mg_replay_sample's slot (seed, draw = first_draw + u, filled_only 1).
 *   effective   W = mu + sigma * eps (the product rounded, then the sum) of both models' noisy layers.
 *   forwards    target(s') then current(s), both with their noise: per unit y = fmaf(x[K-1], W[j, K-1], ...
 *               fmaf(x[0], W[j, 0], bias[j])), k ascending; ReLU keeps y > 0 ? y : 0. Per action the head of
 *               the acting path: mean, x = (v + A) - mean, m = max, e = exp(x - m) (that exp), S = the four
 *               13-atom chains combined (c0 + c1) + (c2 + c3), y[a][i] = e / S.
 *   target      nd[a][i] = y[a][i] * z[i]; q[a] = the same four chains over nd[a]; a' = the first maximum;
 *               the gathered row nd[a'] stays support-scaled (:560-563). Tz = r + ((1 - done) * fp32(gamma))
 *               * z[i], clamped to [-10, 10]; b = (Tz - -10) / 0.4f; proj[j] = from +0, for i ascending where
 *               floor(b_i) == j: + nd[i] * (ceil(b_i) - b_i); then for i ascending where ceil(b_i) == j:
 *               + nd[i] * (b_i - floor(b_i)). Where floor == ceil both terms are zero (:579-580).
 *   loss        a = the row's action (truncated, kept in 0..4); c_i = min(max(y[a][i], 0.01f), 0.99f);
 *               loss_b = -(((0 + proj_0 log(c_0)) + proj_1 log(c_1)) + ...), log below;
 *               loss = (((0 + loss_0) + loss_1) + ...) * fp32(1 / B).
 *   dlogits     g_i = -(proj_i / c_i) * fp32(1 / B); dot = fmaf(g_50, y_50, ... fmaf(g_0, y_0, 0));
 *               dx_i = y_i * (g_i - dot); value logits: dv_i = dx_i; advantage logits: t = dx_i / 5,
 *               dA[a][i] = dx_i - t, every other action -t.
 *   backward    per layer as mg_dqn_learn: dW[j, k] the fmaf chain over b of dy[b, j] x[b, k] from +0, db[j]
 *               the sequential sum, dx[b, k] the fmaf chain over j of dy[b, j] W[j, k] from +0 masked by the
 *               input's ReLU, with W the effective weights. linear2's output gradient is (the value stream's
 *               chain + the advantage stream's chain), then the mask. g_mu = g_W, g_sigma = g_W * eps.
 *   Adam        mg_dqn_learn's, step s = first_update + u + 1.
 *   noise       afterwards both models' buffers are rebuilt from noise[u] = [2][1124] (current, target; per
 *               noisy layer eps_in[64], eps_out[out], bias noise[out]): weight_epsilon[j, k] = eps_out[j] *
 *               eps_in[k], bias_epsilon = the bias noise (:486-491, :606-607).
 *   log         the library's own, identical bits on host and device: x = 2^k m, m in [sqrt(1/2), sqrt 2),
 *               f = m - 1, s = f / (2 + f), z = s s, w = z z, R = z (L1 + w L3) + w (L2 + w L4), h = (0.5 f) f,
 *               log = (((s (h + R) + k ln2_lo) - h) + f) + k ln2_hi (fdlibm's logf, no fmaf).
 * Launches per update: the row kernel (one block per minibatch row), four backward launches (the two head
 * layers, the two hidden streams with linear2's output gradient, linear2, linear1), Adam with the loss sum,
 * the noise reset with the next effective weights; one launch before the first update forms the effective
 * weights of the stored noise. Optional outputs: loss_out [U], rows_out [U, B, 24], proj_out [U, B, 51],
 * grads_out [U, P]; packed_out (16-byte aligned, mg_rainbow_packed_bytes()): the current model's effective
 * weights after the last update in mg_rainbow_pack's layout (num_updates 0: of the stored state). scratch:
 * mg_rainbow_learn_scratch_bytes(batch) bytes, 16-byte aligned. hyper: mg_dqn_hyper (target_period is not
 * read: the caller syncs the target by episode count, :690-691). Accepted: 1 <= batch <= 1024, 1 <= capacity
 * <= 2^32, num_updates >= 0, 0 <= beta < 1.
 * mg_host_rainbow_learn: the same functions on HOST pointers, synchronously. mg_host_rainbow_project: the
 * projection alone, next_dist [n, 51] (support-scaled), reward [n], done [n], support [51] -> proj [n, 51].
 * mg_host_rainbow_log: y[i] = that log of x[i] for normal positive x (NaN otherwise). */
int mg_rainbow_replay_store(float* rows, uint64_t* counter, int64_t capacity, const mg_transitions* tr, int64_t n,
                            int32_t num_steps, void* stream);
/* (additive to ABI 21) mg_rainbow_replay_store for `members` (1 .. 64) replay memories from ONE [T, N, ...]
 * mg_transitions, N = members * n_member: rows[m] / counters[m] are host arrays of device pointers (read during
 * the call only). Member m's transition k = t n_member + j (0 <= j < n_member) reads column c = m n_member + j
 * of the tensors in place -- s = obs_first[c] at t = 0, else obs[t - 1, c]; s' = final_obs[t, c] where done (and
 * final_obs is given), else obs[t, c]; a and done from a1 / done or flags at [t, c]; r = rew[t, c, 0] -- and goes
 * to slot (counter_m + k) % capacity of rows[m]. With total_m = T n_member > capacity only the member's newest
 * `capacity` transitions (k >= total_m - capacity) are written, per member. Then counter_m += T n_member: exactly
 * what mg_rainbow_replay_store leaves when given a contiguous copy of the slice. Two launches for all members:
 * the store on a grid (ceil(T n_member / 256), members) with the members' pointers in the kernel argument, then
 * one thread per member moves its counter. The store reads no won mask, so any n_member >= 0 is accepted.
 * capacity is shared. Refused before anything is read or launched, in this order: members outside 1 .. 64; rows,
 * counters or tr NULL; member by member a NULL rows / counter, one not 8-byte aligned, a ring or counter listed
 * twice (two members' appends to one ring have no defined order); capacity outside 1 .. 2^32; n_member < 0 or
 * num_steps < 0; a non-NULL goal / next_goal / reward / meta_goal; then n_member == 0 or num_steps == 0 returns
 * 0; then a missing obs_first / obs / a1 (or flags) / rew, a float buffer not 4-byte aligned, n_member *
 * num_steps past the grid limit. Appending from inside the rollout kernel and prioritized members (whose trees
 * need mg_per_store) are not offered.
 * mg_host_rainbow_replay_store_many: the same functions on HOST pointers, synchronously. */
int mg_rainbow_replay_store_many(float* const* rows, uint64_t* const* counters, int32_t members, int64_t capacity,
                                 const mg_transitions* tr, int64_t n_member, int32_t num_steps, void* stream);
int mg_host_rainbow_replay_store_many(float* const* rows, uint64_t* const* counters, int32_t members,
                                      int64_t capacity, const mg_transitions* tr, int64_t n_member,
                                      int32_t num_steps);
size_t mg_rainbow_learner_bytes(void);
size_t mg_rainbow_learn_scratch_bytes(int32_t batch);
int mg_rainbow_learn(float* learner, const float* rows, const uint64_t* counter, int64_t capacity, int32_t batch,
                     int32_t num_updates, uint64_t first_update, uint64_t seed, uint64_t first_draw,
                     const mg_dqn_hyper* hyper, const float* noise, float* loss_out, float* rows_out, float* proj_out,
                     float* grads_out, void* packed_out, void* scratch, size_t scratch_bytes, void* stream);
int mg_host_rainbow_learn(float* learner, const float* rows, const uint64_t* counter, int64_t capacity, int32_t batch,
                          int32_t num_updates, uint64_t first_update, uint64_t seed, uint64_t first_draw,
                          const mg_dqn_hyper* hyper, const float* noise, float* loss_out, float* rows_out,
                          float* proj_out, float* grads_out, void* scratch, size_t scratch_bytes);
int mg_host_rainbow_project(const float* next_dist, const float* reward, const float* done, const float* support,
                            double gamma, float* proj, int64_t n);
int mg_host_rainbow_log(const float* x, float* y, int64_t n);

/* ---- Prioritized replay (additive to ABI 21) --------------------------------------------------------
 * SumSegmentTree / MinSegmentTree (scripts/ranbowdqn.py:130-262) and PrioritizedReplayBuffer (:326-437) beside
 * the rows of mg_rainbow_replay_store. The script defines the class and never instantiates it; these entries
 * are pinned to the class itself.
 *
 * The tree is one caller-owned device buffer of mg_per_bytes(capacity) = 8 (4 C + 2) bytes, 16-byte aligned,
 * C = the smallest power of two >= capacity (:345-347): fp64 sum[2 C], fp64 min[2 C] -- node 1 the root, leaf
 * i at C + i, node 0 unused, as SegmentTree._value -- then fp64 max_priority and one pad. fp64 because the
 * reference's nodes are Python floats and the sampled indices have to be the reference's. mg_per_init writes
 * 0.0 (:218), +inf (:256) and 1.0 (:351). Every inner node is always written as left + right, or
 * min(left, right), of finished children (:202-205), so the tree is a pure function of its leaves: no float
 * atomics, the same bits for every grid.
 *
 *   pow       x ** y = exp(y * log x) in fp64 for a normal positive finite x, the library's own, identical bits
 *             on host and device: fdlibm's e_log.c and e_exp.c without their special cases, every operation
 *             rounded once, no fma. A priority p enters the tree as p ** alpha; alpha == 1 takes p itself, so
 *             that tree equals the reference's bit for bit. Error against libm pow: DESIGN.md section 5.
 *   store     mg_per_store = mg_rainbow_replay_store (the same arguments, the same rows), then the leaves of
 *             the written slots := max_priority ** alpha in both trees (:353-358), then their ancestors level
 *             by level -- the written slots are a range modulo capacity, so each level's dirty nodes are that
 *             range shifted right; one launch per level while a level is wider than a block, then one block
 *             with a barrier per level -- then counter += n num_steps. n num_steps > capacity: the newest
 *             `capacity` transitions are written.
 *   sample    len = min(counter, capacity). Draw b: u = ((w0 >> 5) 2^26 + (w1 >> 6)) 2^-53 from words x, y of
 *             mg_replay_sample's Philox block (key seed, counter (b, draw)) -- random.random()'s construction;
 *             mass = u * S with S = sum(0, len - 1) (:364), the leaves 0 .. len - 2 in _reduce_helper's
 *             association, right-nested over the covering nodes, widest first (:159-172). THE NEWEST SLOT
 *             len - 1 IS THEREFORE NEVER DRAWN, as in the reference. Then find_prefixsum_idx (:241-248): from
 *             the root, left where sum[left] > mass, else mass -= sum[left] and right. Weight (:405-412) in
 *             fp64: p_min = min[1] / sum[1], p = sum[C + idx] / sum[1],
 *             w = fp32((p len) ** -beta / (p_min len) ** -beta). A buffer whose priorities were never updated
 *             gives every weight exactly 1. With len < 2 the reference recurses out of its tree; here slot 0
 *             with weight 1.
 *   update    mg_per_update (:417-437): leaf idx[b] := fp64(priority[b]) ** alpha in both trees, the last b
 *             of a repeated index winning as in the reference's loop; max_priority := max(max_priority, every
 *             priority[b]); the ancestors rebuilt a level at a time. One block, one thread per entry. Entries
 *             the reference's asserts reject (:432-433: priority <= 0 or NaN, idx outside 0 .. len - 1) are
 *             left out.
 * Accepted: 1 <= capacity <= 2^32, alpha > 0, beta > 0, 1 <= batch <= 1024, tree_bytes >= mg_per_bytes.
 * mg_host_per_init / _store / _sample / _update: the same functions on HOST pointers, synchronously.
 * mg_host_per_uniform: the u of draw b. mg_host_per_total: S. mg_host_per_pow: out[i] = x[i] ** y[i] as above.
 *
 * mg_rainbow_learn_prioritized = mg_rainbow_learn drawing from the tree: its arguments, then the tree, alpha,
 * beta, prio_eps and the optional outputs idx_out [U, B] int64 and weight_out [U, B] fp32. Per update, on the
 * stream, nothing synchronised -- nine launches for mg_rainbow_learn's seven:
 *   1. sample (seed, draw = first_draw + u) -> idx[b], w[b].
 *   2. the row kernel reads ring row idx[b]; the gradient of row b carries fp32(w[b] * fp32(1 / B)), one
 *      rounded product, where mg_rainbow_learn's carries fp32(1 / B). loss_b stays the unweighted row loss.
 *   3. backward, Adam, noise as mg_rainbow_learn.
 *   4. loss_out[u] = (((0 + w_0 loss_0) + w_1 loss_1) + ...) * fp32(1 / B), each product rounded once.
 *   5. update with priority[b] = loss_b + fp32(prio_eps), one fp32 sum.
 * The script never uses the weights (it has no prioritized run); this is the convention of the notebooks it
 * was taken from (loss = (loss * weights).mean(), priorities loss + 1e-5). scratch:
 * mg_rainbow_learn_prioritized_scratch_bytes(batch). prio_eps >= 0. */
size_t mg_per_bytes(int64_t capacity);
int mg_per_init(void* tree, size_t tree_bytes, int64_t capacity, void* stream);
int mg_per_store(float* rows, uint64_t* counter, int64_t capacity, const mg_transitions* tr, int64_t n,
                 int32_t num_steps, void* tree, size_t tree_bytes, double alpha, void* stream);
int mg_per_sample(const void* tree, size_t tree_bytes, const uint64_t* counter, int64_t capacity, double beta,
                  uint64_t seed, uint64_t draw, int32_t batch, int64_t* idx_out, float* weight_out, void* stream);
int mg_per_update(void* tree, size_t tree_bytes, const uint64_t* counter, int64_t capacity, double alpha,
                  const int64_t* idx, const float* priority, int32_t batch, void* stream);
int mg_host_per_init(void* tree, size_t tree_bytes, int64_t capacity);
int mg_host_per_store(float* rows, uint64_t* counter, int64_t capacity, const mg_transitions* tr, int64_t n,
                      int32_t num_steps, void* tree, size_t tree_bytes, double alpha);
int mg_host_per_sample(const void* tree, size_t tree_bytes, const uint64_t* counter, int64_t capacity, double beta,
                       uint64_t seed, uint64_t draw, int32_t batch, int64_t* idx_out, float* weight_out);
int mg_host_per_update(void* tree, size_t tree_bytes, const uint64_t* counter, int64_t capacity, double alpha,
                       const int64_t* idx, const float* priority, int32_t batch);
double mg_host_per_uniform(uint64_t b, uint64_t draw, uint64_t seed);
int mg_host_per_total(const void* tree, size_t tree_bytes, const uint64_t* counter, int64_t capacity, double* total);
int mg_host_per_pow(const double* x, const double* y, double* out, int64_t n);
size_t mg_rainbow_learn_prioritized_scratch_bytes(int32_t batch);
int mg_rainbow_learn_prioritized(float* learner, const float* rows, const uint64_t* counter, int64_t capacity,
                                 int32_t batch, int32_t num_updates, uint64_t first_update, uint64_t seed,
                                 uint64_t first_draw, const mg_dqn_hyper* hyper, const float* noise, float* loss_out,
                                 float* rows_out, float* proj_out, float* grads_out, void* packed_out, void* scratch,
                                 size_t scratch_bytes, void* tree, size_t tree_bytes, double alpha, double beta,
                                 double prio_eps, int64_t* idx_out, float* weight_out, void* stream);
int mg_host_rainbow_learn_prioritized(float* learner, const float* rows, const uint64_t* counter, int64_t capacity,
                                      int32_t batch, int32_t num_updates, uint64_t first_update, uint64_t seed,
                                      uint64_t first_draw, const mg_dqn_hyper* hyper, const float* noise,
                                      float* loss_out, float* rows_out, float* proj_out, float* grads_out,
                                      void* scratch, size_t scratch_bytes, void* tree, size_t tree_bytes, double alpha,
                                      double beta, double prio_eps, int64_t* idx_out, float* weight_out);

/* ---- Rainbow noise on the device (additive to ABI 21) -----------------------------------------------
 * The factors mg_rainbow_learn and mg_rainbow_learn_prioritized read from `noise`, drawn by a kernel instead of
 * 24 host torch.randn calls per update: mg_rainbow_noise fills noise_out [num_updates][2][1124] fp32 (the layout
 * above: model 0 current, 1 target; per noisy layer eps_in [64], eps_out [out], the bias noise [out], in
 * reset_noise's layer order) on the stream. The stream of numbers is counter-based: element (u, m, f) is a pure
 * function of (noise_seed, t = first_update + u, m, f), there is no generator state and no rejection loop, and any
 * element can be drawn on its own. The distribution is torch.randn's (a standard normal through _scale_noise);
 * the numbers are not torch's. In this fixed order, every operation rounded once, no contraction, no fma:
 *   1. words    w0, w1 = words x, y of Philox4x32-10 with key noise_seed and counter (b, t), as mg_replay_sample's
 *               block (low word first), with b = 2^63 | (m * 1124 + f). The minibatch draws use b < 1024, so the
 *               two streams never share a counter, also where noise_seed equals the learner's seed.
 *   2. uniform  k = ((uint64)(w0 >> 6) << 26) | (w1 >> 6), 52 bits; u = (k + 0.5) * 2^-52, exact in fp64. u is
 *               never 0, 0.5 or 1, and 1 - u is exact too.
 *   3. normal   z = Phi^-1(u) in fp64 by Wichura's algorithm AS 241, routine PPND16, with the coefficients as
 *               CPython's statistics.py (_normal_dist_inv_cdf) writes them. q = u - 0.5.
 *               |q| <= 0.425: r = 0.180625 - q * q; z = (A(r) * q) / B(r).
 *               otherwise: p = u where q < 0, else 1 - u; r = sqrt(-log(p)) with the fp64 log of the prioritized
 *               replay's pow above (fdlibm's e_log.c) and a correctly rounded sqrt;
 *               r <= 5: r' = r - 1.6, z = C(r') / D(r'); r > 5: r' = r - 5, z = E(r') / F(r'); z negated where
 *               q < 0.
 *               Each polynomial c0 + c1 r + ... + c7 r^7 is evaluated in Horner form from c7 down,
 *               acc = acc * r + c_i (a rounded product, then a rounded sum); the numerator first, then the
 *               denominator, then one division. No library transcendental.
 *   4. factor   x = fp32(z), rounded to nearest; the factor is sqrtf(x) for x > 0 and -sqrtf(-x) for x < 0 --
 *               _scale_noise's x.sign().mul(x.abs().sqrt()) (:493-496), elementwise. x is never 0.
 * mg_rainbow_ndtri: z[i] = that Phi^-1 of u[i] on DEVICE pointers (a probe: the r > 5 branch needs u < e^-25,
 * which no small stream reaches). NaN for u outside (0, 1), for a NaN and for a subnormal u (the log takes normal
 * numbers). ndtri(1 - u) == -ndtri(u) bit for bit wherever 1 - u is exact, as for every u of step 2.
 * mg_host_rainbow_noise / mg_host_rainbow_ndtri: the same functions on HOST pointers, synchronously.
 * Refused: a NULL pointer, num_updates < 0 or n < 0, noise_out not 4-byte or u / z not 8-byte aligned. A count of 0
 * is accepted and does nothing. */
int mg_rainbow_noise(uint64_t noise_seed, uint64_t first_update, int32_t num_updates, float* noise_out, void* stream);
int mg_host_rainbow_noise(uint64_t noise_seed, uint64_t first_update, int32_t num_updates, float* noise_out);
int mg_rainbow_ndtri(const double* u, double* z, int64_t n, void* stream);
int mg_host_rainbow_ndtri(const double* u, double* z, int64_t n);

/* ---- A population of Rainbow learners in one set of launches (additive to ABI 21) -------------------
 * Up to 64 independent Rainbow learners of one batch size and capacity trained by mg_rainbow_learn's seven
 * launches per update, the member a grid dimension. Members share `batch` and `capacity`; each has its own
 * learner block, replay rows and counter, minibatch seed, counters (first_update, first_draw) and
 * hyperparameters (lr, gamma, betas, eps), given as an mg_dqn_member (hyper.target_period is not read, as in
 * mg_rainbow_learn; two members may name the same rows and counter: learning only reads them).
 *
 *   learners  [members, mg_rainbow_learner_bytes() / 4] fp32, member m's block as mg_rainbow_learn takes it
 *   table     mg_rainbow_learn_many_table_bytes(members) device bytes, 16-byte aligned, written by
 *             mg_rainbow_learn_many_init from the member list: what does not change between updates (rows, counter,
 *             seed, gamma, Adam's beta1, 1 - beta1, beta2, 1 - beta2, eps, each rounded to fp32 once as the lone call
 *             rounds it). Write it again after any of these changes; the counters are not in it.
 *   noise     [num_updates][members][2][1124] fp32: update u's factors of member m, current model then target,
 *             mg_rainbow_learn's layout per member. mg_rainbow_noise_many fills it in one launch: element
 *             (u, m, model, f) is element (u, model, f) of mg_rainbow_noise(noise_seed[m], first_update[m], ...);
 *             noise_seed and first_update are HOST arrays [members] (they travel in the kernel argument).
 *   loss_out [U][M], rows_out [U][M][B][24], proj_out [U][M][B][51], grads_out [U][M][58884]: optional (NULL).
 *   packed_out  optional: member m's acting net (mg_rainbow_pack's layout of its current model's effective
 *             weights) at packed_out + m * packed_stride; packed_stride a multiple of 16, >= mg_rainbow_packed_bytes()
 *   scratch   members * mg_rainbow_learn_scratch_bytes(batch) bytes, 16-byte aligned
 *
 * Contract: for every member m, its learner block, loss, rows, proj, grads and packed net are bit for bit what
 * mg_rainbow_learn gives on that member's buffers, counters, hyperparameters and slice of the noise. K updates
 * in one call equal K calls. The launch order of a call is the lone learner's: the effective weights of the
 * stored noise, the updates, one pack of all members -- so num_updates == 0 launches the first and the last and
 * leaves packed_out current. On success the two learn calls advance every member's first_update and first_draw
 * by num_updates; a refused call changes nothing. mg_host_rainbow_learn_many is the loop over the members of
 * mg_host_rainbow_learn's update on HOST pointers, synchronously; it needs no table.
 * mg_rainbow_sync_target_many: update_target (ranbowdqn.py:551-552) -- target := current, parameters and noise
 * block -- for every member whose bit of `mask` is set, in one launch; a bit at or above `members` is refused.
 * Refused before anything is read or launched, in mg_rainbow_learn's order: members outside 1 .. 64; a NULL
 * learners, member or scratch, a member's NULL rows or counter; batch outside 1 .. 1024, capacity outside
 * 1 .. 2^32, num_updates < 0; num_updates > 0 with noise NULL; a member's betas outside [0, 1); learners, scratch
 * or packed_out not 16-byte, noise or an optional output not 4-byte aligned, packed_stride no multiple of 16; a
 * member's rows or counter not 8-byte aligned; packed_stride or scratch too small; (device) table NULL, not
 * 16-byte aligned or too small. A refusal of one member's fields names the member. */
size_t mg_rainbow_learn_many_table_bytes(int32_t members); /* 0 outside 1 .. 64 */
int mg_rainbow_learn_many_init(void* table, size_t table_bytes, const mg_dqn_member* member, int32_t members,
                               void* stream);
int mg_rainbow_learn_many(float* learners, const void* table, size_t table_bytes, mg_dqn_member* member,
                          int32_t members, int64_t capacity, int32_t batch, int32_t num_updates, const float* noise,
                          float* loss_out, float* rows_out, float* proj_out, float* grads_out, void* packed_out,
                          size_t packed_stride, void* scratch, size_t scratch_bytes, void* stream);
int mg_host_rainbow_learn_many(float* learners, mg_dqn_member* member, int32_t members, int64_t capacity,
                               int32_t batch, int32_t num_updates, const float* noise, float* loss_out,
                               float* rows_out, float* proj_out, float* grads_out, void* scratch,
                               size_t scratch_bytes);
int mg_rainbow_noise_many(const uint64_t* noise_seed, const uint64_t* first_update, int32_t members,
                          int32_t num_updates, float* noise_out, void* stream);
int mg_host_rainbow_noise_many(const uint64_t* noise_seed, const uint64_t* first_update, int32_t members,
                               int32_t num_updates, float* noise_out);
int mg_rainbow_sync_target_many(float* learners, int32_t members, uint64_t mask, void* stream);

/* ---- A population of prioritized Rainbow learners (additive to ABI 21) -------------------------------
 * mg_rainbow_learn_many whose members each draw from a tree of their own: mg_rainbow_learn_prioritized's nine
 * launches per update -- the sample, mg_rainbow_learn_many's seven, the priority update -- for all members, the
 * member a grid dimension; nothing is synchronised. The arguments are mg_rainbow_learn_many's, the same table
 * included, then
 *
 *   per         HOST array [members] of mg_per_member: member m's tree buffer (mg_per_bytes(capacity) device
 *               bytes, 16-byte aligned, as mg_per_init and the stores leave it), the alpha of its priorities, this
 *               call's beta and its prio_eps; they travel in the kernel argument
 *   tree_bytes  the bytes of every member's tree buffer
 *   idx_out [U][M][B] int64, weight_out [U][M][B] fp32: optional (NULL), each update's sampled slots and weights
 *   scratch     members * mg_rainbow_learn_prioritized_scratch_bytes(batch) bytes, 16-byte aligned
 *
 * Contract: for every member m, its learner block, loss, rows, proj, grads, packed net, idx, weights and every
 * double of its tree (max_priority included) are bit for bit what mg_rainbow_learn_prioritized gives on that
 * member's buffers, counters, hyperparameters, alpha, beta, prio_eps and slice of the noise. K updates in one call
 * equal K calls; num_updates == 0 is mg_rainbow_learn_many's. On success the two calls advance every member's
 * first_update and first_draw by num_updates; a refused call changes nothing.
 * mg_host_rainbow_learn_prioritized_many is the loop over the members of mg_host_rainbow_learn_prioritized's
 * update on HOST pointers, synchronously; it needs no table.
 * Refused before anything is read or launched: what mg_rainbow_learn_many refuses, in its order; then, in
 * mg_rainbow_learn_prioritized's order, a NULL per, a member's NULL tree, a member's tree not 16-byte aligned;
 * tree_bytes < mg_per_bytes(capacity); a member's alpha <= 0, beta <= 0 or prio_eps < 0; idx_out not 8-byte or
 * weight_out not 4-byte aligned; scratch too small; two members that name one tree or one rows buffer (here
 * learning writes the tree, so a shared replay has no defined order). A refusal of one member's fields names the
 * member.
 *
 * mg_per_store_many: mg_rainbow_replay_store_many into `members` prioritized replays -- member m's slice of one
 * [T, members * n, ...] batch into rows[m], and into trees[m] what mg_per_store leaves there, with alpha[m]. rows,
 * counters, trees and alpha are HOST arrays [members]; the capacity and tree_bytes are shared, so every launch
 * has the lone store's grid, the member beside it: the rows, the leaves, the levels, the single-block tail (a
 * block per member), then one launch moves every counter by num_steps * n; every launch before it reads the
 * counters as they were. Contract: member m's rows, counter and tree are bit for bit what mg_per_store leaves when
 * given a contiguous copy of the slice. Refused: what mg_rainbow_replay_store_many refuses, in its order; then a
 * NULL trees or alpha, a member's NULL tree, a member's tree not 16-byte aligned, tree_bytes <
 * mg_per_bytes(capacity), a member's alpha <= 0, a tree listed twice. n == 0 or num_steps == 0 is a no-op.
 * mg_host_per_store_many: the same on HOST pointers, member by member. */
typedef struct mg_per_member {
  void* tree;
  double alpha, beta, prio_eps;
} mg_per_member;
int mg_rainbow_learn_prioritized_many(float* learners, const void* table, size_t table_bytes, mg_dqn_member* member,
                                      int32_t members, int64_t capacity, int32_t batch, int32_t num_updates,
                                      const float* noise, float* loss_out, float* rows_out, float* proj_out,
                                      float* grads_out, void* packed_out, size_t packed_stride, void* scratch,
                                      size_t scratch_bytes, const mg_per_member* per, size_t tree_bytes,
                                      int64_t* idx_out, float* weight_out, void* stream);
int mg_host_rainbow_learn_prioritized_many(float* learners, mg_dqn_member* member, int32_t members, int64_t capacity,
                                           int32_t batch, int32_t num_updates, const float* noise, float* loss_out,
                                           float* rows_out, float* proj_out, float* grads_out, void* scratch,
                                           size_t scratch_bytes, const mg_per_member* per, size_t tree_bytes,
                                           int64_t* idx_out, float* weight_out);
int mg_per_store_many(float* const* rows, uint64_t* const* counters, int32_t members, int64_t capacity,
                      const mg_transitions* tr, int64_t n, int32_t num_steps, void* const* trees, size_t tree_bytes,
                      const double* alpha, void* stream);
int mg_host_per_store_many(float* const* rows, uint64_t* const* counters, int32_t members, int64_t capacity,
                           const mg_transitions* tr, int64_t n, int32_t num_steps, void* const* trees,
                           size_t tree_bytes, const double* alpha);

#ifdef __cplusplus
}
#endif

#endif /* MERGING_HIP_H_ */
