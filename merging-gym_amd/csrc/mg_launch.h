// mg_launch.h -- host side of a launch: error text, armed events, argument checks, launch and make_* helpers.
// A part of the one translation unit merging_hip.hip (see its head comment).
#pragma once

#include "mg_common.h"
#include "mg_env.h"
#include "mg_qnet.h"
#include "mg_step.h"

namespace {

thread_local char g_err[512] = "";
// mg_time_next_launch: events the next step launch of this thread records at its dispatch
thread_local hipEvent_t g_ev_start = nullptr;
thread_local hipEvent_t g_ev_stop = nullptr;

int fail(int code, const char* fmt, const char* what) {
  std::snprintf(g_err, sizeof(g_err), fmt, what);
  return code ? code : static_cast<int>(hipErrorInvalidValue);
}

// a refusal with the call's name in front; who == NULL gives the bare text
int fail_in(const char* who, const char* text) {
  if (who) std::snprintf(g_err, sizeof(g_err), "%s: %s", who, text);
  else std::snprintf(g_err, sizeof(g_err), "%s", text);
  return static_cast<int>(hipErrorInvalidValue);
}

// p is not aligned to mask + 1 bytes (a NULL pointer is aligned)
bool misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

int check_state(const mg_state* s) {
  if (!s || !s->p1 || !s->v1 || !s->p2 || !s->v2 || !s->ret1 || !s->ret2 || !s->tf)
    return fail(hipErrorInvalidValue, "%s", "mg_state has a NULL array");
  return 0;
}

// The params a launch cannot run with (include/merging_hip.h, mg_params): a few scalar compares per
// call. The step count of mg_state.tf saturates at MG_TF_STEPS_MASK, so a larger timeout_steps would
// never time out; div_const needs the rounded reciprocals of its two divisors.
int check_params(const mg_params* p) {
  if (!p) return fail(hipErrorInvalidValue, "%s", "params is NULL");
  const char* bad = nullptr;
  if (p->timeout_steps < 1 || p->timeout_steps > static_cast<int32_t>(MG_TF_STEPS_MASK))
    bad = "timeout_steps must be in 1..8191 (the step count of mg_state.tf saturates at 8191)";
  else if (!(p->R > 0.0 && p->R < HUGE_VAL)) bad = "R must be positive and finite";
  else if (!(p->dT > 0.0 && p->dT < HUGE_VAL)) bad = "dT must be positive and finite";
  else if (p->veh_w <= 0) bad = "veh_w must be positive";
  else if (p->veh_h <= 0) bad = "veh_h must be positive";
  else if (!(p->inv_R == 1.0 / p->R)) bad = "inv_R must be 1 / R, rounded";
  else if (!(p->qp_inv_nz == 1.0 / p->qp_nz)) bad = "qp_inv_nz must be 1 / qp_nz, rounded";
  return bad ? fail(hipErrorInvalidValue, "mg_params: %s", bad) : 0;
}

int check_common(const mg_params* p, const mg_state* s, const mg_outputs* o, int64_t n) {
  if (int e = check_params(p)) return e;
  if (n < 0) return fail(hipErrorInvalidValue, "%s", "n < 0");
  if (n > (static_cast<int64_t>(0x7fffffff) * kBlock))
    return fail(hipErrorInvalidValue, "%s", "n exceeds the grid limit");
  if (int e = check_state(s)) return e;
  if (!o) return fail(hipErrorInvalidValue, "%s", "outputs is NULL (pass a zeroed mg_outputs)");
  if (misaligned(o->obs, 15)) return fail(hipErrorInvalidValue, "%s", "obs must be 16-byte aligned");
  if (misaligned(o->rew, 7)) return fail(hipErrorInvalidValue, "%s", "rew must be 8-byte aligned");
  if (o->flags) {
    if (misaligned(o->flags, 3))
      return fail(hipErrorInvalidValue, "%s", "flags must be 4-byte aligned");
    if (o->done || o->coll || o->rec64)
      return fail(hipErrorInvalidValue, "%s", "flags replaces done / coll (and rec64 has its own status): pass NULL");
  }
  return 0;
}

// the blocks of `per` items that cover n items (n within the grid limit: check_common, the callers)
unsigned grid_blocks(int64_t n, int64_t per = kBlock) { return static_cast<unsigned>((n + per - 1) / per); }

// the trajectory buffers' alignment (the three rollouts)
int check_traj(const mg_traj* traj) {
  if (misaligned(traj->obs, 15) || misaligned(traj->final_obs, 7) || misaligned(traj->rew, 7) ||
      misaligned(traj->flags, 3))
    return fail(hipErrorInvalidValue, "%s", "traj.obs must be 16-byte, rew/final_obs 8-byte, flags 4-byte aligned");
  return 0;
}

// What the three rollouts check first: params, n, the state arrays, then traj itself.
int check_rollout_args(const mg_params* p, const mg_state* s, const mg_traj* traj, int64_t n) {
  const mg_outputs none{};
  if (int e = check_common(p, s, &none, n)) return e;
  return traj ? 0 : fail(hipErrorInvalidValue, "%s", "traj is NULL (pass a zeroed mg_traj)");
}

// a packed Q-net (mg_qnet_pack, mg_qnet_fragments): present and 16-byte aligned, or `text`
int check_packed_net(const void* net, const char* text) {
  return net && !misaligned(net, 15) ? 0 : fail(hipErrorInvalidValue, "%s", text);
}

// the widths a net can have (the packed layouts and the learner share them)
bool net_dims_ok(int32_t in_dim, int32_t out_dim) {
  return in_dim >= 1 && in_dim <= kQMaxIn && out_dim >= 1 && out_dim <= kLMaxOut;
}

int check_net_dims(const char* what, int32_t in_dim, int32_t out_dim) {
  if (net_dims_ok(in_dim, out_dim)) return 0;
  std::snprintf(g_err, sizeof(g_err), "%s: need 1 <= in_dim <= %d, 1 <= out_dim <= %d", what, kQMaxIn, kLMaxOut);
  return static_cast<int>(hipErrorInvalidValue);
}

bool members_ok(int32_t members) { return members >= 1 && members <= kMaxMembers; }

// a refusal that names the member it is about
int fail_member(const char* what, int m, const char* text) {
  std::snprintf(g_err, sizeof(g_err), "%s: member %d: %s", what, m, text);
  return static_cast<int>(hipErrorInvalidValue);
}

int finish_launch(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    std::snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return static_cast<int>(e);
  }
  g_err[0] = '\0';
  return 0;
}

// One launch of a kernel that takes its arguments as one struct, with the dispatch-packet events
// mg_time_next_launch armed for this thread (taken and cleared here) or without.
template <class A>
void launch(void (*kernel)(A), unsigned blocks, unsigned threads, hipStream_t stream, const A& args) {
  hipEvent_t start = g_ev_start, stop = g_ev_stop;
  g_ev_start = g_ev_stop = nullptr;
  if (start || stop)  // profiling: the dispatch packet itself records both events
    hipExtLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), 0, stream, start, stop, 0, args);
  else
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), 0, stream, args);
}

// The launch arguments mg_step, mg_step_random and mg_host_step share.
Launch make_launch(const mg_params* params, const mg_state* state, const mg_outputs* out, const mg_stats* stats,
                   int64_t n, uint32_t flags) {
  Launch L{};
  L.P = *params;
  L.R0 = reset0(*params);
  L.S = *state;
  L.O = *out;
  if (stats) L.St = *stats;
  L.n = n;
  L.flags = flags;
  return L;
}

// The fields Rollout, QRollout and HRollout share.
template <class R>
R make_rollout(const mg_params* params, const mg_state* state, const mg_traj* traj, const mg_stats* stats,
               uint64_t seed, uint64_t first_step, int64_t env_offset, int64_t n, int32_t num_steps,
               uint32_t flags) {
  R r{};
  r.P = *params;
  r.R0 = reset0(*params);
  r.S = *state;
  r.T = *traj;
  if (stats) r.St = *stats;
  r.seed = seed;
  r.first_step = first_step;
  r.env_offset = env_offset;
  r.n = n;
  r.num_steps = num_steps;
  r.flags = flags;
  return r;
}

template <int ACT>
int launch_step(const Launch& L, hipStream_t stream, const char* what) {
  launch(L.O.rec64 ? step_kernel<ACT, true> : step_kernel<ACT, false>, grid_blocks(L.n), kBlock, stream, L);
  return finish_launch(what);
}

int launch_rollout(const Rollout& R, hipStream_t stream) {
  const bool full = R.T.obs && R.T.rew && R.T.flags && R.St.rec &&
                    (R.flags & MG_AUTORESET);
  launch(full ? rollout_kernel<true> : rollout_kernel<false>, grid_blocks(R.n), kBlock, stream, R);
  return finish_launch("mg_rollout_random");
}

}  // namespace
