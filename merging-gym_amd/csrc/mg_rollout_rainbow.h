// mg_rollout_rainbow.h -- Rainbow's acting loop fused with the env step: RbRollout, rainbow_rollout_kernel, the
// same kernel with the member in the grid (RbRolloutMany, the MANY instances), and the host side the lone and the
// member entry point share.
// A part of the one translation unit merging_hip.hip (see its head comment).
#pragma once

#include <type_traits>

#include "mg_common.h"
#include "mg_env.h"
#include "mg_launch.h"
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
//
// Against another net (OPP 3: action_op from a second model on the rotated view) two whole nets and the tile would be
// 168,864 B, 5,024 B more than the CU's 163,840 B of LDS. So the opponent's copy starts at kRbOffBV1 -- both hidden
// streams, the six head streams and the support, 67,792 B -- behind the ego's whole net: 74,192 + 67,792 + 20,480 =
// 162,464 B. The opponent's trunk (W1, b2, W2: bytes [0, kRbOffBV1) = 6,400 B, six 1 KB fragments and one bias read
// per 16-env column tile) is read from its packed net in global memory, where the 64 lanes' 16-byte pieces are
// contiguous and 6.4 KB per net stays in L2.
constexpr int kRbThreads = 512;  // envs per block, one per thread
constexpr int kRbOppLdsBytes = kRbNetBytes - kRbOffBV1;  // the opponent's part in LDS
static_assert(kRbOppLdsBytes == 67792 && kRbOffBV1 == 6400 && kRbOffBV1 % 16 == 0, "the split of the opponent's net");
static_assert(kRbNetBytes + kRbOppLdsBytes + kRbThreads * kObs * 4 <= 163840, "one CU's LDS");

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

// The lone launch against another net (mg_rollout_rainbow_vs; the kernel's OPP 3 instance): the opponent's packed
// net behind the launch, so that the other instances' argument stays what it is.
struct RbRolloutVs {
  RbRollout R;
  const uint8_t* opp;  // may be R.net itself
};

// ---- the member in the grid (mg_rollout_rainbow_many; the kernel's MANY instances): one batch of members * n_member
// envs, member m owning envs [m n_member, (m + 1) n_member) and acting with its own packed net. There are no draws,
// so a member has no seed and no env offset: its net is all the kernel argument carries beside the shared launch.
struct RbRolloutMany {
  RbRollout R;                // shared: n = members * n_member, the row stride of every [T, n, ...] output; net unused
  int64_t n_member;           // a multiple of 64: no wave and no won-mask word spans two members
  int32_t blocks_per_member;  // ceil(n_member / kRbThreads)
  int32_t members;
  const uint8_t* net[kMaxMembers];
  const uint8_t* opp_net[kMaxMembers];  // OPP 3: member m's opponent (entries may repeat and may be members' nets)
};
static_assert(sizeof(RbRolloutMany) <= 4096, "HIP's kernel argument limit");

// What a block works on: the shared launch, its first env, where the envs it may touch stop, its net. The lone
// launch's block b starts at env kRbThreads b and stops at n; with the member in the grid block b is local block
// b mod blocks_per_member of member b div blocks_per_member and stops at the member's end, all block-uniform.
__device__ __forceinline__ const RbRollout& rb_launch(const RbRollout& R) { return R; }
__device__ __forceinline__ const RbRollout& rb_launch(const RbRolloutVs& A) { return A.R; }
__device__ __forceinline__ const RbRollout& rb_launch(const RbRolloutMany& A) { return A.R; }
__device__ __forceinline__ int64_t rb_block_base(const RbRollout&) {
  return static_cast<int64_t>(blockIdx.x) * kRbThreads;
}
__device__ __forceinline__ int64_t rb_block_base(const RbRolloutVs& A) { return rb_block_base(A.R); }
__device__ __forceinline__ int64_t rb_block_base(const RbRolloutMany& A) {
  const int m = static_cast<int>(blockIdx.x) / A.blocks_per_member;
  const int local = static_cast<int>(blockIdx.x) - m * A.blocks_per_member;
  return m * A.n_member + static_cast<int64_t>(local) * kRbThreads;
}
__device__ __forceinline__ int64_t rb_block_end(const RbRollout& R) { return R.n; }
__device__ __forceinline__ int64_t rb_block_end(const RbRolloutVs& A) { return A.R.n; }
__device__ __forceinline__ int64_t rb_block_end(const RbRolloutMany& A) {
  return (static_cast<int>(blockIdx.x) / A.blocks_per_member + 1) * A.n_member;
}
__device__ __forceinline__ const uint8_t* rb_block_net(const RbRollout& R) { return R.net; }
__device__ __forceinline__ const uint8_t* rb_block_net(const RbRolloutVs& A) { return A.R.net; }
__device__ __forceinline__ const uint8_t* rb_block_net(const RbRolloutMany& A) {
  return A.net[static_cast<int>(blockIdx.x) / A.blocks_per_member];
}
__device__ __forceinline__ const uint8_t* rb_block_opp(const RbRollout&) { return nullptr; }
__device__ __forceinline__ const uint8_t* rb_block_opp(const RbRolloutVs& A) { return A.opp; }
__device__ __forceinline__ const uint8_t* rb_block_opp(const RbRolloutMany& A) {
  return A.opp_net[static_cast<int>(blockIdx.x) / A.blocks_per_member];
}

// OPP 0: a2 = None, the env's own L0 opponent; OPP 2: the same net on the view rotated by three; OPP 3: another
// net on that view, its stream part in LDS behind the ego's net and its trunk read from global memory (above).
// MANY: the member in the grid (mg_rollout_rainbow_many) -- the same block on a member's slice of a wider batch:
// liveness, a wave's rows and its won-mask word end at the member's end, rows stride by the whole batch (R.n).
template <int OPP, bool MANY>
using RbRolloutArg = std::conditional_t<MANY, RbRolloutMany, std::conditional_t<OPP == 3, RbRolloutVs, RbRollout>>;

template <int OPP, bool MANY = false>
__global__ __launch_bounds__(kRbThreads) void rainbow_rollout_kernel(const RbRolloutArg<OPP, MANY> A) {
  static_assert(OPP == 0 || OPP == 2 || OPP == 3, "opponent modes: 0 (None), 2 (the same net), 3 (another net)");
  __shared__ __attribute__((aligned(16))) uint8_t lds_net[kRbNetBytes + (OPP == 3 ? kRbOppLdsBytes : 0)];
  __shared__ __attribute__((aligned(16))) float tile[kRbThreads * kObs];
  const RbRollout& R = rb_launch(A);
  const mg_params& P = R.P;
  const int tid = threadIdx.x;
  const int64_t base = rb_block_base(A);
  const int64_t end = rb_block_end(A);
  const int64_t i = base + tid;
  const bool live = i < end;
  const int64_t wbase = base + (tid & ~63);
  const int64_t wrem = end - wbase;
  const int wrows = wrem <= 0 ? 0 : (wrem < 64 ? static_cast<int>(wrem) : 64);
  const bool autoreset = (R.flags & MG_AUTORESET) != 0;
  float* wtile = tile + (tid & ~63) * kObs;

  rainbow_to_lds(rb_block_net(A), lds_net);
  // the opponent: bytes [kRbOffBV1, kRbNetBytes) at lds_net + kRbNetBytes, so the base that puts packed offset x at
  // its LDS place is kRbNetBytes - kRbOffBV1 into the array; nothing below kRbOffBV1 is ever read through it
  const uint8_t* const opp = rb_block_opp(A);
  const uint8_t* const opp_streams = lds_net + (kRbNetBytes - kRbOffBV1);
  if constexpr (OPP == 3) rainbow_to_lds(opp + kRbOffBV1, lds_net + kRbNetBytes, kRbOppLdsBytes);
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
    rainbow_forward_wave(lds_net, lds_net, wtile, 0, q, a1, nullptr, 0);
    if constexpr (OPP == 2) rainbow_forward_wave(lds_net, lds_net, wtile, 3, q, a2, nullptr, 0);
    if constexpr (OPP == 3) rainbow_forward_wave(opp, opp_streams, wtile, 3, q, a2, nullptr, 0);
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

// ============================================================================ the host side of a call
// What mg_rollout_rainbow, mg_rollout_rainbow_many and the two calls against another net (mg_rollout_rainbow_vs,
// mg_rollout_rainbow_vs_many) share: the check of num_steps (`who`: the call's name in front, NULL for the lone
// call's bare text), the mode check of the first two, the member call's shape and net checks, the fill of the launch,
// the instance.
int check_rb_rollout_steps(const char* who, int32_t num_steps) {
  if (num_steps < 0 || num_steps > 65535)
    return fail_in(who, "need 0 <= num_steps <= 65535 (split longer rollouts)");
  return 0;
}

int check_rb_rollout_steps_mode(bool many, int32_t num_steps, int32_t opponent_mode) {
  if (int e = check_rb_rollout_steps(many ? "mg_rollout_rainbow_many" : nullptr, num_steps)) return e;
  if (opponent_mode != 0 && opponent_mode != 2)
    return fail(hipErrorInvalidValue, many ? "mg_rollout_rainbow_many: %s" : "mg_rollout_rainbow: %s",
                "opponent_mode must be 0 (None) or 2 (the same net on state[3:] + state[:3])");
  return 0;
}

// members in 1 .. 64, n_member a multiple of 64 whose batch fits the grid
int check_rb_rollout_members(const char* who, int64_t n_member, int32_t members) {
  if (!members_ok(members)) return fail_in(who, "need 1 <= members <= 64");
  if (n_member < 0) return fail_in(who, "n_member < 0");
  if (n_member % 64 != 0)
    return fail_in(who,
                   "n_member must be a multiple of 64 (a won-mask word covers 64 envs and is stored whole, so no "
                   "two members may share one)");
  if (n_member > (static_cast<int64_t>(0x7fffffff) * kBlock) / members)
    return fail_in(who, "members * n_member exceeds the grid limit");
  return 0;
}

// a host array of `members` packed nets, each present and 16-byte aligned; `what` names them in the texts
int check_rb_member_nets(const char* who, const void* const* nets, int32_t members, const char* what) {
  char text[64];
  std::snprintf(text, sizeof(text), "%ss is NULL (members packed Rainbow nets)", what);
  if (!nets) return fail_in(who, text);
  std::snprintf(text, sizeof(text), "%s must be a 16-byte aligned packed Rainbow net", what);
  for (int m = 0; m < members; ++m)
    if (!nets[m] || misaligned(nets[m], 15)) return fail_member(who, m, text);
  return 0;
}

RbRollout make_rb_rollout(const mg_params* params, const mg_state* state, const mg_traj* traj, const mg_stats* stats,
                          int64_t n, int32_t num_steps, uint32_t flags) {
  RbRollout R{};
  R.P = *params;
  R.R0 = reset0(*params);
  R.S = *state;
  R.T = *traj;
  if (stats) R.St = *stats;
  R.n = n;
  R.num_steps = num_steps;
  R.flags = flags;
  return R;
}

// They come out in the code object in the order of first naming: the lone call's.
template <bool MANY>
auto rainbow_rollout_instance(int32_t opponent_mode) -> void (*)(std::conditional_t<MANY, RbRolloutMany, RbRollout>) {
  return opponent_mode == 0 ? rainbow_rollout_kernel<0, MANY> : rainbow_rollout_kernel<2, MANY>;
}

// The member launch of mg_rollout_rainbow_many (opponents NULL) and of mg_rollout_rainbow_vs_many (the OPP 3
// instance).
int launch_rb_rollout_many(const char* who, void (*kernel)(RbRolloutMany), const RbRollout& R, int64_t n_member,
                           int32_t members, const void* const* nets, const void* const* opponents,
                           hipStream_t stream) {
  RbRolloutMany A{R, n_member, static_cast<int32_t>(grid_blocks(n_member, kRbThreads)), members};
  for (int m = 0; m < members; ++m) {
    A.net[m] = static_cast<const uint8_t*>(nets[m]);
    if (opponents) A.opp_net[m] = static_cast<const uint8_t*>(opponents[m]);
  }
  launch(kernel, static_cast<unsigned>(members) * static_cast<unsigned>(A.blocks_per_member), kRbThreads, stream, A);
  return finish_launch(who);
}

}  // namespace
