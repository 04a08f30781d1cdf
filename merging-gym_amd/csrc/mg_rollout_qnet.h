// mg_rollout_qnet.h -- config 5, the Q-net policy rollout: FinishBound, QRollout, qnet_rollout_ws_kernel, and
// the same kernel with the member in the grid (QRolloutMany, QMemberRollout, the member instances) or every
// ordered pair of K nets in the grid (QRolloutLeague, the league instance), and the host side of mg_rollout_qnet,
// mg_rollout_qnet_many and mg_rollout_qnet_league: their shared checks, the launch's fill, the choice of instance.
// A part of the one translation unit merging_hip.hip (see its head comment).
#pragma once

#include <type_traits>

#include "mg_common.h"
#include "mg_env.h"
#include "mg_launch.h"
#include "mg_qnet.h"
#include "mg_stats.h"
#include "mg_wave_out.h"

namespace {

// specialised kernel: 4 Q-net waves + kQWsEnvWaves env waves (8 env waves -- 3 waves per SIMD,
// a Q-net wave within 168 VGPRs -- measured 19 % slower); each env lane steps kQWsIlp envs per
// phase, in lockstep (independent fp64 chains interleaved in one instruction stream), so a group
// is 64 x env waves x ILP envs and a block holds two
constexpr int kQWsEnvWaves = 4;
constexpr int kQWsIlp = 2;
constexpr int kQWsThreads = 64 * (4 + kQWsEnvWaves);
constexpr int kQWsWavesPerSimd = (4 + kQWsEnvWaves) / 4;
constexpr int kQWsEnvs = 2 * 64 * kQWsEnvWaves * kQWsIlp;  // envs per block
constexpr int kQWsHalf = kQWsEnvs / 2;                     // envs per group
constexpr int kQWsTiles = kQWsHalf / 256;                  // 64-env tiles each Q-net wave computes per phase
static_assert(kQWsTiles >= 1 && kQWsHalf % 256 == 0, "group = 4 Q-net waves x kQWsTiles x 64 envs");

// This lane's rank among the set lanes of a ballot (lanes below it whose bit is set).
__device__ __forceinline__ int lane_rank(uint64_t m) {
  return static_cast<int>(__builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32),
                                                    __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u)));
}

// 16-env column tiles of a forward over n (1..64) compacted items
__device__ __forceinline__ int col_tiles(int n) { return (n + 15) >> 4; }

__device__ __forceinline__ int argmax_first(const float (&q)[8], int out_dim) {
  int best = 0;
  float v = q[0];
#pragma unroll
  for (int j = 1; j < 8; ++j)
    if (j < out_dim && q[j] > v) {
      v = q[j];
      best = j;
    }
  return best;
}

// may_finish_next's constants (below)
struct FinishBound {
  float smin, smax, g;  // min / max of action_dict, the MPC's speed gain per step
  float lat, lon;       // collision reach before the step: lateral |y1 - y2| and longitudinal |x1 - x2|
                        // (finish_bound, from veh_w / veh_h / R / dT and the speeds: 5.75 / 9 by default)
};

// may_finish_next's constants for these params (host). Collision after the step needs
// trunc(y1) - trunc(y2) <= veh_w, so y1 - y2 < veh_w + 1, and |x1 - x2| < veh_h + 1 (the pygame
// Rect truncation of vehicle_box). A step moves a car by dl <= dT vmax along its arc, vmax =
// max(start_vel, action speeds) + 0.5 (a speed only moves toward an action's target), and so its
// lateral y by at most dl |sin theta|; where y1 - y2 < lat the ego's 1 - cos theta < lat / R, so
// |sin theta| < min(1, sqrt(2 lat / R) + dl / R) over the step. lat = veh_w + 1 + max(0.75, 2 dl sin + 0.25):
// the default params' 0.75 (5.75) stands unless the geometry needs more. lat appears in its own bound,
// and the bound grows with lat, so the passes climb from below until lat stops changing: the least
// fixed point, which satisfies the inequality (a fixed number of passes stops under it). |sin| <= 1
// caps it at veh_w + 1.25 + 2 dl. Rounded up to fp32. The longitudinal reach of the speeds is added
// at run time (rel in may_finish_next).
inline FinishBound finish_bound(const mg_params& P) {
  double smin = P.action_speed[0], smax = smin;
  for (int a = 1; a < MG_NUM_ACTIONS; ++a) {
    smin = std::min(smin, P.action_speed[a]);
    smax = std::max(smax, P.action_speed[a]);
  }
  const double vmax = std::max(smax, P.start_vel) + 0.5;
  const double dl = P.dT * vmax;
  const double cap = P.veh_w + 1.25 + 2.0 * dl;
  double lat = P.veh_w + 1.75;
  for (int it = 0; it < 4096; ++it) {  // monotone from below and bounded by cap: ends at the fixed point
    const double sn = std::min(1.0, std::sqrt(2.0 * lat / P.R) + dl / P.R);
    const double next = std::min(cap, P.veh_w + 1.0 + std::max(0.75, 2.0 * dl * sn + 0.25));
    if (!(next > lat)) break;
    lat = next;
  }
  float latf = static_cast<float>(lat);
  if (latf < lat) latf = std::nextafterf(latf, INFINITY);
  // rounded outward by a margin: the bound only has to contain every speed a step reaches
  return FinishBound{static_cast<float>(smin) - 0.5f, static_cast<float>(smax) + 0.5f,
                     static_cast<float>(P.dT * P.qp_z0 / P.qp_nz) * 1.01f, latf,
                     static_cast<float>(P.veh_h + 1)};
}
struct QRollout {
  mg_params P;
  Reset0 R0;
  mg_state S;
  mg_traj T;
  mg_stats St;
  const uint8_t* net;
  const uint8_t* opp_net;   // OPP 3: the opponent's own net (main.py's Strategy_OP "L1")
  uint64_t seed;
  uint64_t first_step;
  uint64_t greedy_thr;      // greedy iff u32 draw < greedy_thr (2^32: always)
  uint64_t opp_greedy_thr;
  int64_t env_offset;
  int64_t n;
  int32_t num_steps;
  int32_t out_dim;
  uint32_t flags;
  FinishBound fin;  // may_finish_next's constants
  // n is the row stride of every [T, n, ...] output; end() is where the envs this block may touch stop
  // (the same number here; a member's slice end in QMemberRollout)
  __device__ int64_t end() const { return n; }
};

// ---- the member in the grid (mg_rollout_qnet_many; the kernel's MANY instances): one batch of members * n_member envs, member m
// owning envs [m n_member, (m + 1) n_member) and acting with its own net, opponent net, seed and
// thresholds. The kernel argument carries the shared launch and the members' scalars.
struct QMember {
  const uint8_t* net;
  const uint8_t* opp_net;
  uint64_t seed;
  uint64_t greedy_thr;
  uint64_t opp_greedy_thr;
};
struct QRolloutMany {
  QRollout R;        // shared: n = members * n_member (the row stride); net, seed, thresholds unused
  int64_t n_member;  // a multiple of 64: no won-mask word spans two members
  int32_t blocks_per_member;  // ceil(n_member / kQWsEnvs)
  int32_t members;
  QMember mem[kMaxMembers];
};
static_assert(sizeof(QRolloutMany) <= 4096, "HIP's kernel argument limit");

// ---- every ordered pair in the grid (mg_rollout_qnet_league; the kernel's league instance): one batch of
// nets * nets * n_pair envs, pairing p = i nets + j owning envs [p n_pair, (p + 1) n_pair), where net i is the ego
// and net j the opponent (OPP 3), each with its own threshold, the draws keyed by the ego's seed. K entries name
// K * K pairings, so 4,096 of them fit the argument that holds 64 members.
struct QLeagueNet {
  const uint8_t* net;
  uint64_t seed;
  uint64_t greedy_thr;
};
struct QRolloutLeague {
  QRollout R;               // shared: n = nets * nets * n_pair (the row stride); net, seed, thresholds unused
  int64_t n_pair;           // a multiple of 64: no won-mask word spans two pairings
  int32_t blocks_per_pair;  // ceil(n_pair / kQWsEnvs)
  int32_t nets;             // K
  QLeagueNet net[kMaxMembers];
};
static_assert(sizeof(QLeagueNet) == 24, "three words per net");
static_assert(sizeof(QRolloutLeague) <= 4096, "HIP's kernel argument limit");

// What the role functions see of a member's block: the shared launch by reference (the kernel
// argument, never copied) and the member's own scalars, block-uniform. Field for field QRollout's names.
struct QMemberRollout {
  const mg_params& P;
  const Reset0& R0;
  const mg_state& S;
  const mg_traj& T;
  const mg_stats& St;
  const uint8_t* net;
  const uint8_t* opp_net;
  uint64_t seed;
  uint64_t first_step;
  uint64_t greedy_thr;
  uint64_t opp_greedy_thr;
  int64_t env_offset;
  int64_t n;    // row stride: the whole batch
  int64_t lim;  // the member's end, (m + 1) n_member
  int32_t num_steps;
  int32_t out_dim;
  uint32_t flags;
  const FinishBound& fin;
  __device__ int64_t end() const { return lim; }
};

// Whether env e's next step can end its episode, for ANY pair of actions (a conservative superset of
// env_step's done, tests/test_may_finish.py): main.py:221 logs eval_net(state)[action] of an
// episode's last step whatever branch chose the action, so the config-5 kernels evaluate the net for
// these envs even where the ego explores. From the state a step acts on (o: its fp32 observation;
// every margin below is >= 0.25 m, far above the fp32 rounding of o):
//   timeout   the step count reaches timeout_steps (env_clock);
//   arrival   a car can pass END_POINT within the step and that ends the episode (the other car
//             already won, or both arrive): p' = p + dT v' with v' between v and the action's target
//             speed, so END_POINT - p < dT max(v, smax) + 0.5;
//   collision the boxes can overlap afterwards. Laterally trunc(y1) - trunc(y2) <= veh_w needs
//             y1 - y2 < veh_w + 1 (y1 >= y2 on the two arcs), and a step moves each y by at most
//             |sin theta| dT v' (< 0.17 m there by default); B.lat (finish_bound) covers both.
//             Longitudinally |t1 - t2| <= veh_h needs |x1 - x2| < veh_h + 1 (B.lon), and a
//             step changes x1 - x2 by at most dT |v1' - v2'| (+ 0.2 % for the arc): the MPC moves each
//             speed by g (s - v), g = dT z0 / z'n = 1/15 (mpc_acc), so |v1' - v2'| <= |v1 - v2| +
//             g (max(smax, v1, v2) - min(smin, v1, v2)).
// Flags ~2.2 % of env-steps in uniform random play (tests/test_may_finish.py).
MG_HD bool may_finish_next(const mg_params& P, const Env& e, const obs_t (&o)[kObs], const FinishBound& B) {
  if (static_cast<int32_t>(e.steps) + 1 >= P.timeout_steps) return true;
  const float dt = static_cast<float>(P.dT);
  const bool ego = o[3] < dt * fmaxf(o[4], B.smax) + 0.5f;  // o[3] = END_POINT - p1, o[4] = v1
  const bool opp = o[8] < dt * fmaxf(o[9], B.smax) + 0.5f;  // o[8] = END_POINT - p2, o[9] = v2
  const bool arrive = e.winner == 1 ? opp : (e.winner == 2 ? ego : (ego && opp));
  const float spread = fmaxf(B.smax, fmaxf(o[4], o[9])) - fminf(B.smin, fminf(o[4], o[9]));
  const float rel = dt * (fabsf(o[2]) + B.g * spread) + 0.5f;  // o[2] = v2 - v1
  const bool coll = -o[1] < B.lat && fabsf(o[0]) < B.lon + rel;  // o[1] = y2 - y1, o[0] = x2 - x1
  return arrive || coll;
}

// The need bits of env gi's step `step` for the config-5 Q-net waves (opponent modes 2 / 3): bit 0
// the ego's forward (its greedy draw, or may_finish_next while statistics are kept), bit 1 the
// opponent's (its greedy draw). u: the step's Philox words (qnet_policy_step_n's stream).
template <class RT>
__device__ __forceinline__ uint8_t qnet_need_bits(const RT& R, const uint4& u, bool live, const Env& e,
                                                  const obs_t (&o)[kObs]) {
  if (!live) return 0;
  const bool fin = R.St.rec != nullptr && (R.flags & MG_AUTORESET) && may_finish_next(R.P, e, o, R.fin);
  return static_cast<uint8_t>(((static_cast<uint64_t>(u.x) < R.greedy_thr || fin) ? 1 : 0) |
                              (static_cast<uint64_t>(u.z) < R.opp_greedy_thr ? 2 : 0) | (fin ? 4 : 0));
}

// Where the Q-net waves find them: OPP 2 reads both bits from greedy[1][j]; OPP 3 (round 5, the
// waves split by net) gives each net's waves a byte of their own -- greedy[0][j] the ego's (bit 0
// need, bit 1 may finish), greedy[1][j] the opponent's (bit 0 its greedy draw, bit 1 may finish) --
// which those waves then overwrite with the greedy actions, so no byte is shared between waves.
template <int OPP>
__device__ __forceinline__ void qnet_put_need(uint8_t* g0, uint8_t* g1, uint8_t b) {
  if constexpr (OPP == 3) {
    const uint8_t fin = static_cast<uint8_t>((b >> 1) & 2);
    *g0 = static_cast<uint8_t>((b & 1) | fin);
    *g1 = static_cast<uint8_t>(((b >> 1) & 1) | fin);
  } else {
    *g1 = b;
  }
}

// eval_net(state)[0..4] into an env's tile row, once every forward has read its observation: the
// env wave logs q[action] from it when the episode ends (main.py:221), before it writes the next
// observation into the row
__device__ __forceinline__ void put_q_row(float* row, const float (&q)[8]) {
  reinterpret_cast<f32x2*>(row)[0] = f32x2{q[0], q[1]};
  reinterpret_cast<f32x2*>(row)[1] = f32x2{q[2], q[3]};
  row[4] = q[4];
}

// One epsilon-greedy step (main.py:99-112) of the N envs i0 + 64 j of one env-wave lane given their
// greedy actions, stepped in lockstep. Draws (ABI 20), Philox4x32-10 keyed by seed:
//  * OPP 0 / 1 (no net opponent): two draws per step, so one call serves two steps -- step k takes
//    words (x, y) of call (gi, k div 2) when k is even and (z, w) when k is odd (kept from the even
//    step in `keep`, or computed when a launch starts on an odd step). The first word is the ego's
//    explore draw; the second its random action floor(5 w / 2^32), or with the uniform opponent the
//    pair x = floor(25 w / 2^32), a1 = x div 5, a2 = x mod 5 (one word, as the random-policy stream).
//  * OPP 2 / 3: call (gi, k) per step: u.x the ego's explore draw, u.y its random action, u.z the
//    opponent's explore draw, u.w its random action.
// Envs past n (live[j] false) are stepped too but never stored. A greedy action outside 0..4 (a
// net with out_dim > 5) gets env_step's KeyError semantics (env_step_lockstep).
// qrow: the tile row of env i0 (rows of envs i0 + 64 j follow 64 rows apart), where the Q-net wave
// left eval_net(state)[0..4] of the state the step acts on: a finishing env logs q[a1] (main.py:221).
template <int OPP, int N, bool CHECKED, class RT>
__device__ __forceinline__ void qnet_policy_step_n(const RT& R, Env (&e)[N], StepOut (&r)[N],
                                                   int64_t i0, const bool (&live)[N], int t,
                                                   const int (&greedy1)[N], const int (&greedy2)[N],
                                                   bool (&won)[N], const float* qrow, uint2 (&keep)[N],
                                                   double (&pend)[N], uint4 (&un)[N], uint8_t* need0,
                                                   uint8_t* need1) {
  const uint64_t step = R.first_step + t;
  int a1[N], a2[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const uint64_t gi = static_cast<uint64_t>(R.env_offset + i0 + 64 * j);
    if constexpr (OPP < 2) {
      uint32_t ex, pick;
      if ((step & 1) == 0 || t == 0) {  // wave-uniform: a fresh call feeds this step and the next
        const uint4 u = philox4x32_10(
            make_uint4(static_cast<uint32_t>(gi), static_cast<uint32_t>(gi >> 32),
                       static_cast<uint32_t>(step >> 1), static_cast<uint32_t>(step >> 33)),
            static_cast<uint32_t>(R.seed), static_cast<uint32_t>(R.seed >> 32));
        keep[j] = make_uint2(u.z, u.w);
        ex = (step & 1) ? u.z : u.x;
        pick = (step & 1) ? u.w : u.y;
      } else {
        ex = keep[j].x;
        pick = keep[j].y;
      }
      const bool greedy = static_cast<uint64_t>(ex) < R.greedy_thr;
      if constexpr (OPP == 1) {  // (random a1, uniform a2) from one 25-way draw
        const uint32_t x = static_cast<uint32_t>((static_cast<uint64_t>(pick) * 25u) >> 32);
        const int b1 = static_cast<int>((x * 13u) >> 6);  // x div 5 for x < 25
        a1[j] = greedy ? greedy1[j] : b1;
        a2[j] = static_cast<int>(x) - 5 * b1;
      } else {
        a1[j] = greedy ? greedy1[j] : action_from_u32(pick);
        a2[j] = MG_ACTION_NONE;
      }
    } else {
      const uint4 u = un[j];  // drawn one phase ahead, with the need bits the Q-net waves compacted by
      a1[j] = (static_cast<uint64_t>(u.x) < R.greedy_thr) ? greedy1[j] : action_from_u32(u.y);
      a2[j] = (static_cast<uint64_t>(u.z) < R.opp_greedy_thr) ? greedy2[j] : action_from_u32(u.w);
    }
  }
  env_step_lockstep<N, CHECKED>(R.P, e, a1, a2, r);
#pragma unroll
  for (int j = 0; j < N; ++j) {
    won[j] = false;
    if (!live[j]) continue;
    const int64_t i = i0 + 64 * j;
    const int64_t row = static_cast<int64_t>(t) * R.n + i;
    if (R.T.rew)
      st_out(reinterpret_cast<f32x2*>(R.T.rew) + row,
             f32x2{static_cast<float>(r[j].r1), static_cast<float>(r[j].r2)});
    store_step_bytes(R.T, row, a1[j], a2[j], r[j].done, r[j].coll);
    won[j] = e[j].winner == 1;
    // the Q value the scripts log for a finished episode (q_eval_value, main.py:221); a1 in 0..4
    // here (a bad action leaves done false)
    if (after_step_nowait(R.P, e[j], r[j], R.St, R.T.final_obs ? R.T.final_obs + row * kObs : nullptr, i,
                          (R.flags & MG_AUTORESET) != 0, pend[j], &R.R0))
      add_q_eval_nowait(R.St, i, qrow[64 * j * kObs + a1[j]]);
  }
  if constexpr (OPP >= 2) {  // the next step's draws and need bits, for Q(X, t + 1)
    if (t + 1 < R.num_steps) {
#pragma unroll
      for (int j = 0; j < N; ++j) {
        un[j] = philox_env_step(static_cast<uint64_t>(R.env_offset + i0 + 64 * j), step + 1, R.seed);
        qnet_put_need<OPP>(need0 + 64 * j, need1 + 64 * j, qnet_need_bits(R, un[j], live[j], e[j], r[j].o));
      }
    }
  }
}

// Observation of env i (or zeros past n) into its fp32 tile row; returns live.
template <class RT>
__device__ __forceinline__ bool qnet_load_env(const RT& R, int64_t i, Env& e, float* row) {
  const mg_params& P = R.P;
  double o[kObs];
  const bool live = i < R.end();
  if (live) {
    e = load_env(R.S, i);
    double x1, y1, x2, y2;
    lon2coord(P, e.p1, true, x1, y1);
    lon2coord(P, e.p2, false, x2, y2);
    observe(P, e.p1, e.v1, e.p2, e.v2, x1, y1, x2, y2, o);
  } else {  // a defined state for the lockstep step, which also steps envs past n (never stored)
    e.p1 = e.p2 = P.start_point;
    e.v1 = e.v2 = P.start_vel;
    e.ret1 = e.ret2 = 0.0;
    e.steps = 0;
    e.winner = 0;
    e.done = false;
#pragma unroll
    for (int k = 0; k < kObs; ++k) o[k] = 0.0;
  }
  put_obs_row(row, o);
  return live;
}

// The same T steps with the waves specialised: waves 0-3 run only the Q-net (matrix cores +
// ReLU), waves 4-7 only the fp64 env step, so each SIMD pairs a matrix-heavy wave with a
// vector-heavy one (waves w and w + 4 share a SIMD). The block's 512 envs are two groups
// of 256, pipelined over 2T + 1 barrier-separated phases:
//   Q(A,0) | Q(B,0) + step(A,0) | Q(A,1) + step(B,0) | ... | step(B,T-1)
// Greedy actions go to the env waves through LDS; the new observations come back through the
// tile rows. Each env-wave lane holds the two envs (one per group) it steps.
// OPP 3 (main.py's default Strategy_OP "L1", :161-168: the opponent is another trained DQN)
// keeps a second net in LDS: with the 16x16 layouts (2 x 59,392 B, ABI 19) the two nets, the
// 1,024-env tile and the greedy bytes take 161,792 B, so it runs ILP 2 like the others (the
// 32x32 layouts, 2 x 60,496 B, did not fit and ran ILP 1 on 512-env blocks: 1 % slower).
// The items a Q-net wave runs itself out of a list of n (round 5): all of them, or 192 (three full
// forwards) when 1..16 remain past those, which then run on the env wave of the same index.
__device__ __forceinline__ int qws_own_items(int n) { return n > 192 && n <= 192 + 16 ? 192 : n; }
__device__ __forceinline__ void qws_publish_tail(int (&qt)[4], int p, int nq, int nn, int nf) {
  if ((threadIdx.x & 63) == 0) {
    qt[1] = nq;
    qt[2] = nn;
    qt[3] = nf;
    __hip_atomic_store(&qt[0], p, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
}
__device__ __forceinline__ void qws_wait(const int* flag, int p) {
  while (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != p) __builtin_amdgcn_s_sleep(1);
}

// ---- the Q-net waves' phase Q(X, t) with a net opponent, one function per mode: the forwards of
// group X's envs on the state step t acts on (wave = threadIdx.x / 64 < 4).

// OPP 2: the tile row of item e of Q-net wave w's list, in the group whose rows begin at gb
__device__ __forceinline__ int qws2_row(int gb, int w, int e) { return gb + (4 * ((e >> 6) & 1) + w) * 64 + (e & 63); }

// OPP 2, after a forward: the lanes that hold an item (on) write its greedy byte, and the ego's
// q[0..4] into the env's row, after every read of that row (the opponent items come first)
__device__ __forceinline__ void qws2_put(const float (&q)[8], int out_dim, bool on, int e, int gb, int w,
                                         uint8_t* greedy0, uint8_t* greedy1, float* tile) {
  if (!on) return;
  const int row = qws2_row(gb, w, e);
  const uint8_t a = static_cast<uint8_t>(argmax_first(q, out_dim));
  if (e & 0x80) {
    greedy1[row] = a;
  } else {
    greedy0[row] = a;
    put_q_row(tile + row * kObs, q);
  }
}

// OPP 2 (self-play). Only the forwards the reference evaluates (round 5): choose_action runs the
// net on its greedy branch only (main.py:105-107), and :221 evaluates it on an episode's last step.
// The wave's 128 envs of the group are compacted by their need bits into one list, the opponent's
// items (swapped view) first, and run through the forward 64 at a time on col_tiles(count) column
// tiles. list / stage / qt: this wave's qlist, qstage ([h][item]) and qtail.
template <class RT>
__device__ __forceinline__ void qws_q_selfplay(const RT& R, const uint8_t* lds_net, float* tile,
                                               uint8_t* greedy0, uint8_t* greedy1, uint8_t* list, u32x4* stage,
                                               int (&qt)[4], int p) {
  static_assert(kQWsTiles == 2, "the list holds the wave's two 64-env tiles");
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int gb = (p & 1) * kQWsHalf;
  const int nb0 = greedy1[qws2_row(gb, wave, lane)], nb1 = greedy1[qws2_row(gb, wave, 64 + lane)];
  const uint64_t mo0 = __ballot(nb0 & 2), mo1 = __ballot(nb1 & 2);
  const uint64_t me0 = __ballot(nb0 & 1), me1 = __ballot(nb1 & 1);
  const int Lo0 = __popcll(mo0), Lo = Lo0 + __popcll(mo1);
  const int Le0 = __popcll(me0), Ln = Lo + Le0 + __popcll(me1);
  if (nb0 & 2) list[lane_rank(mo0)] = static_cast<uint8_t>(0x80 | lane);
  if (nb1 & 2) list[Lo0 + lane_rank(mo1)] = static_cast<uint8_t>(0x80 | 64 | lane);
  if (nb0 & 1) list[Lo + lane_rank(me0)] = static_cast<uint8_t>(lane);
  if (nb1 & 1) list[Lo + Le0 + lane_rank(me1)] = static_cast<uint8_t>(64 | lane);
  {
    // the same net for both views: stage every item's fragments from its env's lane (both
    // views of the row from one read), then run the whole list 64 items per forward
    auto put = [&](int row, int nb, int po, int pe) __attribute__((always_inline)) {
      float f[kObs];
#pragma unroll
      for (int k = 0; k < kObs / 2; ++k) {
        const f32x2 t2 = reinterpret_cast<const f32x2*>(tile + row * kObs)[k];
        f[2 * k] = t2[0];
        f[2 * k + 1] = t2[1];
      }
      auto pk = [](float a, float b) { return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{a, b}, bf16x2)); };
      if (nb & 2) {  // the opponent's view state[5:] + state[:5] (main.py:199)
        stage[po] = u32x4{pk(f[5], f[6]), pk(f[7], f[8]), pk(f[9], f[0]), pk(f[1], f[2])};
        stage[256 + po] = u32x4{pk(f[3], f[4]), 0u, 0x3F800000u, 0x3F803F80u};
      }
      if (nb & 1) {
        stage[pe] = u32x4{pk(f[0], f[1]), pk(f[2], f[3]), pk(f[4], f[5]), pk(f[6], f[7])};
        stage[256 + pe] = u32x4{pk(f[8], f[9]), 0u, 0x3F800000u, 0x3F803F80u};
      }
    };
    put(qws2_row(gb, wave, lane), nb0, lane_rank(mo0), Lo + lane_rank(me0));
    put(qws2_row(gb, wave, 64 + lane), nb1, Lo0 + lane_rank(mo1), Lo + Le0 + lane_rank(me1));
  }
  wave_lds_sync();
  const int nq = qws_own_items(Ln);
  qws_publish_tail(qt, p, nq, Ln, 0);
  const int r = lane & 31, h = lane >> 5;
#pragma unroll 1
  for (int c0 = 0; c0 < nq;) {
    // staged fragments, any mix of views (a view chosen per lane by selects on the features
    // cost +35 % per launch, r05f q1 / q2)
    const int cnt = nq - c0 < 64 ? nq - c0 : 64;
    auto input = [&](int it) __attribute__((always_inline)) {
      return __builtin_bit_cast(bf16x8, stage[256 * h + c0 + (it < cnt ? it : 0)]);
    };
    const int e_out = list[c0 + (lane < cnt ? lane : 0)];  // read ahead: its wait hides under the forward
    float q[8];
    qnet_mlp_swp_nc(lds_net, input(r), input(32 + r), q, col_tiles(cnt));
    qws2_put(q, R.out_dim, lane < cnt, e_out, gb, wave, greedy0, greedy1, tile);
    wave_lds_sync();
    c0 += cnt;
  }
}

// OPP 3, after the forward over items c0 .. c0 + cnt of a list of nn whose may-finish items are the
// first nf (an opponent wave) or the last nf (an ego wave): the greedy byte; an opponent wave then
// publishes the phase in *rows_read once a forward has consumed the may-finish rows, and an ego
// wave waits for that before it writes its may-finish items' Q rows.
__device__ __forceinline__ void qws3_put(const float (&q)[8], int out_dim, bool oppw, int c0, int cnt, int nn, int nf,
                                         int p, int* rows_read, uint8_t* gbyte, float* qrow) {
  const int lane = threadIdx.x & 63;
  if (lane < cnt) *gbyte = static_cast<uint8_t>(argmax_first(q, out_dim));
  if (oppw) {
    if (c0 < nf && c0 + cnt >= nf && lane == 0) __hip_atomic_store(rows_read, p, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
  } else if (c0 + cnt > nn - nf) {
    qws_wait(rows_read, p);
    if (lane < cnt && c0 + lane >= nn - nf) put_q_row(qrow, q);
  }
}

// OPP 3 (the opponent's own net). Only the forwards the reference evaluates (round 5; OPP 2 above
// for the common part), with the waves split by net: waves 0-1 run the opponent's net, 2-3 the
// ego's, each over 256 of the group's 512 envs (rows rb + e). One net per wave keeps the view
// uniform and gives each wave ~194 items = three full 64-item forwards and a narrow one; split by
// env instead, each wave ran both nets on ~97 items apiece (two forwards per net, the second three
// tiles wide). An ego wave writes eval_net(state)[0..4] into the tile rows of its may-finish items
// only (an episode can end only there, main.py:221) and only once the opponent wave of the same
// rows has read them: that wave lists those items first and publishes the phase in qrows_read[hw]
// after their forward; the ego wave lists them last.
template <class RT>
__device__ __forceinline__ void qws_q_split(const RT& R, const uint8_t* lds_net, const uint8_t* lds_net2,
                                            float* tile, uint8_t* greedy0, uint8_t* greedy1, uint8_t* list,
                                            int (&qt)[4], int* qrows_read, int p) {
  static_assert(kQWsHalf == 512, "two waves per net, 256 envs each");
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool oppw = wave < 2;
  const int hw = wave & 1;
  const int rb = (p & 1) * kQWsHalf + 256 * hw;
  uint8_t* gout = (oppw ? greedy1 : greedy0) + rb;
  uint64_t mn[4], mf[4];
  int nn = 0, nf = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int nb = gout[64 * k + lane];
    mn[k] = __ballot(nb & 1);
    mf[k] = __ballot((nb & 3) == 3);
    nn += __popcll(mn[k]);
    nf += __popcll(mf[k]);
  }
  int of = oppw ? 0 : nn - nf, on = oppw ? nf : 0;  // may-finish items first / last
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint64_t mo = mn[k] & ~mf[k];
    if ((mf[k] >> lane) & 1)
      list[of + lane_rank(mf[k])] = static_cast<uint8_t>(64 * k + lane);
    else if ((mo >> lane) & 1)
      list[on + lane_rank(mo)] = static_cast<uint8_t>(64 * k + lane);
    of += __popcll(mf[k]);
    on += __popcll(mo);
  }
  wave_lds_sync();
  const int nq = qws_own_items(nn);
  qws_publish_tail(qt, p, nq, nn, nf);
  if (oppw && nf == 0 && lane == 0) __hip_atomic_store(&qrows_read[hw], p, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
  const int r = lane & 31, h = lane >> 5;
  const uint8_t* net = oppw ? lds_net2 : lds_net;
  // the tile rows of a chunk's items (column envs r and 32 + r, and this lane's result row),
  // read one chunk ahead: a forward's inputs then wait for one LDS read, not two
  auto rows_of = [&](int c, int& ra, int& rc, int& ro) __attribute__((always_inline)) {
    const int n = nn - c < 64 ? nn - c : 64;
    ra = rb + list[c + (r < n ? r : 0)];
    rc = rb + list[c + (32 + r < n ? 32 + r : 0)];
    ro = rb + list[c + (lane < n ? lane : 0)];
  };
  int ra, rc, row;
  rows_of(0, ra, rc, row);
#pragma unroll 1
  for (int c0 = 0; c0 < nq;) {
    const int cnt = nq - c0 < 64 ? nq - c0 : 64;
    auto input = [&](int j) __attribute__((always_inline)) {
      const float* rw = tile + j * kObs;
      return oppw ? qnet_input(rw, true, h) : qnet_input(rw, false, h);
    };
    const bf16x8 x0 = input(ra), x1 = input(rc);
    const int rcur = row;
    if (c0 + cnt < nq) rows_of(c0 + cnt, ra, rc, row);
    float q[8];
    qnet_mlp_swp_nc(net, x0, x1, q, col_tiles(cnt));
    // (nf > nq: the env wave running the tail publishes the phase)
    qws3_put(q, R.out_dim, oppw, c0, cnt, nn, nf, p, &qrows_read[hw], gout + (rcur - rb), tile + rcur * kObs);
    wave_lds_sync();
    c0 += cnt;
  }
}

// OPP 2 / 3, env wave ew: Q-net wave ew's list tail for Q(group p & 1, step p / 2) -- its 1..16
// items past three full forwards, one column tile -- as that wave would run it (qtail).
template <int OPP, class RT>
__device__ __forceinline__ void qws_env_tail(const RT& R, const uint8_t* lds_net, const uint8_t* lds_net2,
                                             float* tile, uint8_t* greedy0, uint8_t* greedy1, const uint8_t* list,
                                             const u32x4* stage, const int (&qt)[4], int* qrows_read, int p, int ew) {
  qws_wait(&qt[0], p);
  const int nq = qt[1], nn = qt[2];
  if (nn <= nq) return;
  const int cnt = nn - nq;
  const int lane = threadIdx.x & 63, r32 = lane & 31, h = lane >> 5;
  const int it = nq + (r32 < cnt ? r32 : 0), io = nq + (lane < cnt ? lane : 0);
  float q[8];
  if constexpr (OPP == 3) {
    const bool oppw = ew < 2;
    const int hw = ew & 1, nf = qt[3];
    const int rb = (p & 1) * kQWsHalf + 256 * hw;
    const float* rw = tile + (rb + list[it]) * kObs;
    const int row = rb + list[io];
    const bf16x8 x = oppw ? qnet_input(rw, true, h) : qnet_input(rw, false, h);
    qnet_mlp<2 * kQLdsAhead, 1>(qnet_lds(oppw ? lds_net2 : lds_net), x, x, q);
    qws3_put(q, R.out_dim, oppw, nq, cnt, nn, nf, p, &qrows_read[hw], (oppw ? greedy1 : greedy0) + row,
             tile + row * kObs);
  } else {
    const bf16x8 x = __builtin_bit_cast(bf16x8, stage[256 * h + it]);
    qnet_mlp<2 * kQLdsAhead, 1>(qnet_lds(lds_net), x, x, q);
    qws2_put(q, R.out_dim, lane < cnt, list[io], (p & 1) * kQWsHalf, ew, greedy0, greedy1, tile);
  }
}

// What a block of the kernel below works on, lone (the launch itself, envs from kQWsEnvs blockIdx.x) and
// with the member in the grid (the member's view, envs from its slice's start).
__device__ __forceinline__ const QRollout& qws_block_view(const QRollout& R) { return R; }
__device__ __forceinline__ int64_t qws_block_base(const QRollout&) {
  return static_cast<int64_t>(blockIdx.x) * kQWsEnvs;
}
__device__ __forceinline__ int qws_member(const QRolloutMany& A) {
  return static_cast<int>(blockIdx.x) / A.blocks_per_member;
}
__device__ __forceinline__ QMemberRollout qws_block_view(const QRolloutMany& A) {
  const int m = qws_member(A);
  const QMember& me = A.mem[m];
  return QMemberRollout{A.R.P,          A.R.R0,          A.R.S,          A.R.T,
                        A.R.St,         me.net,          me.opp_net,     me.seed,
                        A.R.first_step, me.greedy_thr,   me.opp_greedy_thr, A.R.env_offset,
                        A.R.n,          (m + 1) * A.n_member, A.R.num_steps, A.R.out_dim,
                        A.R.flags,      A.R.fin};
}
__device__ __forceinline__ int64_t qws_block_base(const QRolloutMany& A) {
  const int m = qws_member(A);
  const int local = static_cast<int>(blockIdx.x) - m * A.blocks_per_member;
  return m * A.n_member + static_cast<int64_t>(local) * kQWsEnvs;
}
// The league: block b serves pairing p = b div blocks_per_pair, ego p div K against opponent p mod K; the view is a
// member's, its two nets and thresholds picked from two entries of the list. It is a QMemberRollout under a name
// of its own: with the plain type the league instance shared the member instances' role-function instantiations
// (two callers of each where there was one), and qnet_rollout_ws_kernel<3, true, QRolloutMany> came out with 232
// VGPRs instead of its 234. Instantiated apart, every earlier instance compiles as before, the league one as its twin.
struct QPairRollout : QMemberRollout {};
__device__ __forceinline__ int qws_pairing(const QRolloutLeague& A) {
  return static_cast<int>(blockIdx.x) / A.blocks_per_pair;
}
__device__ __forceinline__ QPairRollout qws_block_view(const QRolloutLeague& A) {
  const int p = qws_pairing(A);
  const int i = p / A.nets, j = p - i * A.nets;
  const QLeagueNet& ego = A.net[i];
  const QLeagueNet& opp = A.net[j];
  return QPairRollout{{A.R.P,          A.R.R0,         A.R.S,          A.R.T,
                       A.R.St,         ego.net,        opp.net,        ego.seed,
                       A.R.first_step, ego.greedy_thr, opp.greedy_thr, A.R.env_offset,
                       A.R.n,          (p + 1) * A.n_pair, A.R.num_steps, A.R.out_dim,
                       A.R.flags,      A.R.fin}};
}
__device__ __forceinline__ int64_t qws_block_base(const QRolloutLeague& A) {
  const int p = qws_pairing(A);
  const int local = static_cast<int>(blockIdx.x) - p * A.blocks_per_pair;
  return p * A.n_pair + static_cast<int64_t>(local) * kQWsEnvs;
}

// CHECKED: a greedy action may fall outside action_dict (a net with out_dim > 5): the lockstep step
// carries the KeyError selects. Every other launch takes CHECKED = false (-2 % on the ego-only
// leg, r03i; the self-play and other-net instances showed no gain and keep the checked step).
// MANY: the member in the grid (mg_rollout_qnet_many, below) -- the same block on a member's slice of a
// wider batch. Block b is then local block b mod blocks_per_member of member b div blocks_per_member, its
// first env m n_member + kQWsEnvs local -- off the kQWsEnvs grid whenever n_member is no multiple of it,
// so a member's last block ends at the member's end (R.end()), not the batch's. Rows stride by the whole
// batch (R.n); the Philox env index stays env_offset + i, i within the batch, so member m is a lone launch
// on n_member envs at env_offset + m n_member. The member's scalars are block-uniform: read once from the
// kernel argument by a uniform index (scalar loads).
// ARG: the form of the argument, which is all that tells the three apart -- QRollout (lone), QRolloutMany (the member
// in the grid) or QRolloutLeague (every ordered pair of K nets in the grid, mg_rollout_qnet_league: a member's block
// whose two nets are entries i and j of one list; only the OPP 3, checked instance exists).
template <int OPP, bool CHECKED, class ARG = QRollout>
__global__ __launch_bounds__(kQWsThreads, kQWsWavesPerSimd) void qnet_rollout_ws_kernel(const ARG A) {
  decltype(auto) R = qws_block_view(A);  // QRollout itself, or the member's / the pairing's QMemberRollout
  constexpr int kIlp = kQWsIlp;
  constexpr int kEnvs = kQWsEnvs;  // envs per block
  constexpr int kHalf = kQWsHalf;  // envs per group
  // OPP 0 / 1: the 32x32 layout (second part of the packed buffer) and forward, see qnet32_mlp
  constexpr bool kNet32 = OPP < 2;
  __shared__ __attribute__((aligned(16))) uint8_t lds_net[kNet32 ? kQ32NetBytes : kQNetBytes];
  __shared__ __attribute__((aligned(16))) uint8_t lds_net2[OPP == 3 ? kQNetBytes : 16];
  __shared__ __attribute__((aligned(16))) float tile[kEnvs * kObs];
  __shared__ uint8_t greedy[2][kEnvs];
  // OPP 2 / 3 (round 5): per Q-net wave the compacted items of a phase -- OPP 2: env e of the wave's
  // 128 | 0x80 the opponent's view; OPP 3: env e of the wave's 256 (one net per wave). When a phase
  // begins the greedy bytes hold the need bits (qnet_need_bits, qnet_put_need)
  __shared__ uint8_t qlist[OPP >= 2 ? 4 : 1][OPP >= 2 ? 256 : 1];
  // OPP 2: each listed item's layer-1 B fragment halves (the view it needs), staged by the env's own
  // lane, so one forward can hold both views' items (one net) and reads its inputs lane-linearly:
  // half-major ([wave][h][item]), so the 32 lanes reading one half read 512 contiguous bytes (round 6;
  // item-major, the 32-B item stride left half of the banks idle: SQ_LDS_BANK_CONFLICT / IDX_ACTIVE
  // 0.097, valu_busy.json)
  __shared__ __attribute__((aligned(16))) u32x4 qstage[OPP == 2 ? 4 : 1][2][OPP == 2 ? 256 : 1];
  // OPP 3: phase p once opponent wave h has read every tile row an ego wave will overwrite with
  // Q-values (the may-finish rows, which it lists first)
  __shared__ int qrows_read[2];
  // OPP 2 / 3: a Q-net wave's list tail -- its items past three full forwards, when at most 16 -- runs
  // on env wave w (the same index) after that wave's step, so the Q-net waves' phase ends after three
  // forwards instead of three and a narrow fourth (whose weight stream costs half a full one). Wave w
  // publishes {phase, items it runs, list length, may-finish items} once its list (and OPP 2's staged
  // fragments) are in LDS; the phase word last, with release order.
  __shared__ int qtail[OPP >= 2 ? 4 : 1][4];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t base = qws_block_base(A);
  const int ew = wave - 4;

  if constexpr (kNet32) {
    const f32x4* src = reinterpret_cast<const f32x4*>(R.net + kQNetBytes);
    for (int j = tid; j < kQ32NetBytes / 16; j += blockDim.x) reinterpret_cast<f32x4*>(lds_net)[j] = src[j];
  } else {
    qnet_to_lds(R.net, lds_net);
  }
  if constexpr (OPP == 3) qnet_to_lds(R.opp_net, lds_net2);
  if (tid < 2) qrows_read[tid] = -1;
  if (OPP >= 2 && tid < 4) qtail[tid][0] = -1;
  const int phases = 2 * R.num_steps + 1;
  if (wave < 4) {
    // Q-net waves: the barrier count matches the env waves' loop below, phase for phase
    // (roles are whole waves, so s_barrier pairs up; the two loops keep each role's live
    // registers apart -- in one loop the env state sat beside the accumulators and spilled)
    __syncthreads();
    for (int p = 0; p < phases; ++p) {
      if (p < 2 * R.num_steps) {
        if constexpr (OPP == 3)
          qws_q_split(R, lds_net, lds_net2, tile, greedy[0], greedy[1], qlist[wave], qtail[wave],
                      qrows_read, p);
        else if constexpr (OPP == 2)
          qws_q_selfplay(R, lds_net, tile, greedy[0], greedy[1], qlist[wave], &qstage[wave][0][0],
                         qtail[wave], p);
        else  // OPP 0 / 1: the 32x32 forward over each of the wave's 64-env tiles of the group
#pragma unroll 1
          for (int tt = 0; tt < kQWsTiles; ++tt) {
            const int row0 = (p & 1) * kHalf + (4 * tt + wave) * 64;
            float q[8];
            qnet32_forward(lds_net, tile, row0, false, q);
            greedy[0][row0 + lane] = static_cast<uint8_t>(argmax_first(q, R.out_dim));
            // the row's observation has been read: the MFMA chain behind q waits for every read
            put_q_row(tile + (row0 + lane) * kObs, q);
          }
      }
      __syncthreads();
    }
    return;
  }
  // env lane: envs lbase + 64 j + lane (j < kIlp) of group 0 (e0) and of group 1 (e1)
  const int lbase = ew * 64 * kIlp;
  Env e0[kIlp], e1[kIlp];
  StepOut r[kIlp];
  bool live0[kIlp], live1[kIlp];
  uint2 keep0[kIlp], keep1[kIlp];  // OPP 0 / 1: the odd step's two draw words (qnet_policy_step_n)
  double pend0[kIlp], pend1[kIlp];  // main.py's pending values (pend_load, after_step_nowait)
  uint4 un0[kIlp], un1[kIlp];       // OPP 2 / 3: each env's draws of its next step (one phase ahead)
#pragma unroll
  for (int j = 0; j < kIlp; ++j) {
    const int la = lbase + 64 * j + lane, lb = kHalf + la;
    live0[j] = qnet_load_env(R, base + la, e0[j], tile + la * kObs);
    live1[j] = qnet_load_env(R, base + lb, e1[j], tile + lb * kObs);
    pend0[j] = live0[j] ? pend_load(R.St, base + la, e0[j]) : 0.0;
    pend1[j] = live1[j] ? pend_load(R.St, base + lb, e1[j]) : 0.0;
    if constexpr (OPP >= 2) {  // step 0's draws and need bits (the observation as the tile row holds it)
      obs_t o0[kObs], o1[kObs];
#pragma unroll
      for (int k = 0; k < kObs; ++k) {
        o0[k] = tile[la * kObs + k];
        o1[k] = tile[lb * kObs + k];
      }
      un0[j] = philox_env_step(static_cast<uint64_t>(R.env_offset + base + la), R.first_step, R.seed);
      un1[j] = philox_env_step(static_cast<uint64_t>(R.env_offset + base + lb), R.first_step, R.seed);
      qnet_put_need<OPP>(&greedy[0][la], &greedy[1][la], qnet_need_bits(R, un0[j], live0[j], e0[j], o0));
      qnet_put_need<OPP>(&greedy[0][lb], &greedy[1][lb], qnet_need_bits(R, un1[j], live1[j], e1[j], o1));
    }
#pragma unroll
    for (int k = 0; k < kObs; ++k) r[j].o[k] = 0.0;
  }
  __syncthreads();
  for (int p = 0; p < phases; ++p) {
    if (p > 0) {
      const int g = (p - 1) & 1, t = (p - 1) >> 1;
      const int local0 = g * kHalf + lbase;
      int greedy1[kIlp], greedy2[kIlp];
#pragma unroll
      for (int j = 0; j < kIlp; ++j) {
        greedy1[j] = greedy[0][local0 + 64 * j + lane];
        greedy2[j] = OPP >= 2 ? greedy[1][local0 + 64 * j + lane] : 0;
      }
      bool won[kIlp];
      // wave-uniform branch: each group's envs stay in named registers
      const float* qrow = tile + (local0 + lane) * kObs;
      uint8_t* need0 = &greedy[0][local0 + lane];
      uint8_t* need1 = &greedy[1][local0 + lane];
      if (g == 0)
        qnet_policy_step_n<OPP, kIlp, CHECKED>(R, e0, r, base + local0 + lane, live0, t, greedy1, greedy2, won, qrow,
                                               keep0, pend0, un0, need0, need1);
      else
        qnet_policy_step_n<OPP, kIlp, CHECKED>(R, e1, r, base + local0 + lane, live1, t, greedy1, greedy2, won, qrow,
                                               keep1, pend1, un1, need0, need1);
      const int64_t wbase = base + local0;
#pragma unroll
      for (int j = 0; j < kIlp; ++j) {
        const int64_t rem = R.end() - (wbase + 64 * j);
        store_won_mask(R.T.won_mask, won[j], t, R.n, wbase + 64 * j,
                       rem <= 0 ? 0 : (rem < 64 ? static_cast<int>(rem) : 64));
      }
      const int64_t wrem = R.end() - wbase;
      const int wrows = wrem <= 0 ? 0 : (wrem < 64 * kIlp ? static_cast<int>(wrem) : 64 * kIlp);
      wave_store_obs_n<kIlp>(tile + local0 * kObs, r,
                             R.T.obs ? R.T.obs + (static_cast<int64_t>(t) * R.n + wbase) * kObs : nullptr,
                             wrows);
    }
    if constexpr (OPP >= 2) {
      if (p < 2 * R.num_steps)
        qws_env_tail<OPP>(R, lds_net, lds_net2, tile, greedy[0], greedy[1], qlist[ew], &qstage[OPP == 2 ? ew : 0][0][0],
                          qtail[ew], qrows_read, p, ew);
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < kIlp; ++j) {
    const int la = lbase + 64 * j + lane;
    if (live0[j]) store_env(R.S, base + la, e0[j]);
    if (live1[j]) store_env(R.S, base + kHalf + la, e1[j]);
  }
}

// ============================================================================ the host side of a call
// What mg_rollout_qnet, mg_rollout_qnet_many and mg_rollout_qnet_league share. Each keeps its own order of checks
// (the lone call looks at its net before out_dim, the member call at every member's nets after the mode, the league
// call has no mode): the pieces are shared, not the walk.
// The launch's fill is make_rollout (mg_launch.h) and two more fields, out_dim and fin, set where it is made.

// num_steps and out_dim; who: the text's frame, "%s" or "<entry point>: %s"
int check_qrollout_dims(const char* who, int32_t num_steps, int32_t out_dim) {
  if (num_steps < 0 || out_dim < 1 || out_dim > kLMaxOut)
    return fail(hipErrorInvalidValue, who, "need num_steps >= 0 and 1 <= out_dim <= 8");
  return 0;
}

// num_steps and out_dim, then the mode: neighbours in both orders. The member call's texts carry its name.
int check_qrollout_dims_mode(bool many, int32_t num_steps, int32_t out_dim, int32_t opponent_mode) {
  const char* const who = many ? "mg_rollout_qnet_many: %s" : "%s";
  if (int e = check_qrollout_dims(who, num_steps, out_dim)) return e;
  if (opponent_mode < 0 || opponent_mode > 3)
    return fail(hipErrorInvalidValue, who,
                many ? "opponent_mode must be 0 (None), 1 (uniform), 2 (same net) or 3 (each member's opp_net)"
                     : "opponent_mode must be 0 (None), 1 (uniform), 2 (same net) or 3 (opp_net)");
  return 0;
}

// Every member's net, and in mode 3 its opponent's: member by member, so member 0's opp_net before member 1's net.
int check_qnet_actors(const mg_qnet_actor* actors, int32_t members, int32_t opponent_mode) {
  for (int m = 0; m < members; ++m) {
    if (!actors[m].net || misaligned(actors[m].net, 15))
      return fail_member("mg_rollout_qnet_many", m, "net must be a 16-byte aligned packed Q-net");
    if (opponent_mode == 3 && (!actors[m].opp_net || misaligned(actors[m].opp_net, 15)))
      return fail_member("mg_rollout_qnet_many", m, "opponent_mode 3 needs opp_net, a 16-byte aligned packed Q-net");
  }
  return 0;
}

// The member call's argument: the launch (n = members * n_member; seed, nets, thresholds unused), the entries.
QRolloutMany make_qrollout_many(const QRollout& R, int64_t n_member, const mg_qnet_actor* actors, int32_t members,
                                int32_t opponent_mode) {
  QRolloutMany A{R, n_member, static_cast<int32_t>(grid_blocks(n_member, kQWsEnvs)), members};
  for (int m = 0; m < members; ++m)
    A.mem[m] = QMember{static_cast<const uint8_t*>(actors[m].net),
                       opponent_mode == 3 ? static_cast<const uint8_t*>(actors[m].opp_net) : nullptr, actors[m].seed,
                       actors[m].greedy_threshold, actors[m].opp_greedy_threshold};
  return A;
}

// The instance for a launch. checked: an argmax may name an action past action_dict (out_dim > 5); a net opponent's
// instances are always checked. They come out in the code object in the order of first naming: the lone call's.
template <class ARG>
auto qnet_rollout_instance(int32_t opponent_mode, bool checked) -> void (*)(ARG) {
  return opponent_mode == 0   ? (checked ? qnet_rollout_ws_kernel<0, true, ARG> : qnet_rollout_ws_kernel<0, false, ARG>)
         : opponent_mode == 1 ? (checked ? qnet_rollout_ws_kernel<1, true, ARG> : qnet_rollout_ws_kernel<1, false, ARG>)
         : opponent_mode == 2 ? qnet_rollout_ws_kernel<2, true, ARG>
                              : qnet_rollout_ws_kernel<3, true, ARG>;
}

// ---- mg_rollout_qnet_league
// Every net of the list: each is some pairing's ego and some pairing's opponent.
int check_league_nets(const mg_league_net* league, int32_t nets) {
  for (int k = 0; k < nets; ++k)
    if (!league[k].net || misaligned(league[k].net, 15)) {
      std::snprintf(g_err, sizeof(g_err), "mg_rollout_qnet_league: net %d: net must be a 16-byte aligned packed Q-net", k);
      return static_cast<int>(hipErrorInvalidValue);
    }
  return 0;
}

// The league call's argument: the launch (n = nets * nets * n_pair; seed, nets, thresholds unused), the entries.
QRolloutLeague make_qrollout_league(const QRollout& R, int64_t n_pair, const mg_league_net* league, int32_t nets) {
  QRolloutLeague A{R, n_pair, static_cast<int32_t>(grid_blocks(n_pair, kQWsEnvs)), nets};
  for (int k = 0; k < nets; ++k)
    A.net[k] = QLeagueNet{static_cast<const uint8_t*>(league[k].net), league[k].seed, league[k].greedy_threshold};
  return A;
}

}  // namespace
