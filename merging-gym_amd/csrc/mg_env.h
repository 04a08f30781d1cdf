// mg_env.h -- the fp64 env step host and device share: geometry, collision, observe, Philox draws, env_step*.
// A part of the one translation unit merging_hip.hip (see its head comment).
#pragma once

#include "mg_common.h"

namespace {

// Action codes after host/device decoding: 0..4 valid, -1 None (opponent only), anything
// else is the reference's KeyError.
MG_HD bool valid_action(int a) { return a >= 0 && a < MG_NUM_ACTIONS; }

// x / d for a divisor fixed per launch, correctly rounded: q = x * (1/d), then Markstein's
// FMA correction. With inv = RN(1/d) this returns RN(x / d) for d = 3 and d = 30000 (the
// only divisors used; 0 mismatches in 8e8 random tests, incl. random exponents,
// tests/test_division.py) at 3 instructions instead of the ~10 of a general fp64 division.
MG_HD double div_const(double x, double d, double inv) {
  const double q = x * inv;
  const double r = fma(-q, d, x);
  return fma(r, inv, q);
}

// sin and cos of the double theta. For |theta| < 1/16 -- pos in [-875, 2875], which covers
// both cars up to END_POINT (pos 50..~1000) -- a degree-9 / degree-10 Taylor polynomial
// in fma form: the correction terms are < 7e-4 of the result, so the one rounding of the
// final fma dominates and the result agrees with libm's sin/cos to <= 1 ulp (identical in
// 99.98 % of 2e7 samples vs glibc). Larger |theta| takes the device library's sincos, within
// 1 ulp; live episodes do reach it (an arrived car drives on, <= 8 m per step, until the other
// arrives or the 2501-step timeout, to ~20 km).
// The device library's sincos for |t| >= 1/16. Kept out of line: inlined, the compiler hoists its polynomial
// constants into VGPRs for the whole step loop of the T-step kernels, which then spill. Its
// results come back by value (round 4): through pointers they were private-memory loads in the
// caller, and the wait for those at the join after the branch -- one in-order counter for vector
// loads and stores on gfx950 -- also waited for every store the wave had in flight, on the common
// path too. Config 5 -1.5 to -3 % per step, the rollout and h-DQN within noise (profiles/r04/ab/
// r04z_*, and r04ab_*: the rollout in both orders, and by-value in the lockstep path only, which tied).
__device__ __attribute__((noinline, unused)) double2 sincos_cold(double t) {
  double s, c;
  sincos(t, &s, &c);
  return make_double2(s, c);
}

// the polynomial branch (|t| < 1/16)
MG_HD void sincos_poly(double t, double& s, double& c) {
  const double t2 = t * t;
  const double ps = fma(t2, fma(t2, fma(t2, 2.7557319223985893e-06, -1.9841269841269841e-04),
                                8.3333333333333332e-03),
                        -1.6666666666666666e-01);
  s = fma(t * t2, ps, t);
  const double pc =
      fma(t2, fma(t2, fma(t2, fma(t2, -2.7557319223985888e-07, 2.4801587301587302e-05),
                          -1.3888888888888889e-03),
                  4.1666666666666664e-02),
          -0.5);
  c = fma(t2, pc, 1.0);
}

MG_HD void arc_sincos(double t, double& s, double& c) {
  if (fabs(t) < 0.0625) {
    sincos_poly(t, s, c);
    return;
  }
#if defined(__HIP_DEVICE_COMPILE__)
  const double2 sc = sincos_cold(t);
  s = sc.x;
  c = sc.y;
#else
  s = std::sin(t);
  c = std::cos(t);
#endif
}

// arc_sincos of M angles: when every one is in the polynomial's range (the usual case) the M
// polynomials form one straight-line block the scheduler can interleave; otherwise each angle
// takes arc_sincos's own branch. Same results as M arc_sincos calls.
template <int M>
__device__ __forceinline__ void arc_sincos_n(const double (&t)[M], double (&s)[M], double (&c)[M]) {
  bool fast = true;
#pragma unroll
  for (int k = 0; k < M; ++k) fast = fast && fabs(t[k]) < 0.0625;
  if (fast) {
#pragma unroll
    for (int k = 0; k < M; ++k) sincos_poly(t[k], s[k], c[k]);
    return;
  }
#pragma unroll
  for (int k = 0; k < M; ++k) arc_sincos(t[k], s[k], c[k]);
}

// lon2coord (merging_env.py:48-58): position along the arc -> (x longitudinal, y lateral).
// The ego rides the arc on +y, the opponent its mirror image on -y. Split in three so the
// lockstep step can batch the sin/cos of several cars.
MG_HD double arc_angle(const mg_params& P, double lon) {
  return P.angle0 - div_const(lon, P.R, P.inv_R);
}

MG_HD void arc_xy(const mg_params& P, double s, double c, bool ego, double& x,
                                       double& y) {
  x = P.R * s;
  const double d = P.R - P.R * c;
  const double half_w = P.W * 0.5;  // W/2 = 150.0 exactly
  y = ego ? (half_w + d) : (half_w - d);
}

MG_HD void lon2coord(const mg_params& P, double lon, bool ego, double& x,
                                          double& y) {
  double s, c;
  arc_sincos(arc_angle(P, lon), s, c);
  arc_xy(P, s, c, ego, x, y);
}

// corners (merging_env.py:232-239) is called as corners(agent, y=x, x=y, 0) (:201-202), so
// the pygame Rect is centred at (lateral, longitudinal) with w = VEHICLE_W (lateral) and
// h = VEHICLE_H (longitudinal) (surfaces :97-98). pygame converts a float centre with a C
// (int) cast, i.e. truncation toward zero, then sets x = cx - w/2, y = cy - h/2. Each corner
// is ((double)corner - pivot) + pivot in fp64 (Vector2 difference, rotate(0) = identity,
// 1.0 * v, + pivot), which is not always the integer corner (no Sterbenz near 0).
struct Box {
  double l, r, t, b;  // lateral [l, r], longitudinal [t, b]
};

MG_HD Box vehicle_box(const mg_params& P, double lat, double lon) {
  const int rx = static_cast<int>(lat) - P.veh_w / 2;
  const int ry = static_cast<int>(lon) - P.veh_h / 2;
  Box bx;
  bx.l = (static_cast<double>(rx) - lat) + lat;
  bx.r = (static_cast<double>(rx + P.veh_w) - lat) + lat;
  bx.t = (static_cast<double>(ry) - lon) + lon;
  bx.b = (static_cast<double>(ry + P.veh_h) - lon) + lon;
  return bx;
}

// shapely Polygon.intersects on two axis-aligned rectangles: the closed boxes share a point.
MG_HD bool boxes_intersect(const Box& a, const Box& b) {
  return a.l <= b.r && b.l <= a.r && a.t <= b.b && b.t <= a.b;
}

// is_collided (:198-206) of cars at (lateral y, longitudinal x): boxes_intersect(vehicle_box(y1, x1),
// vehicle_box(y2, x2)) with the lateral edges as integers where that is exact. For y >= 8 and the
// default veh_w / 2 = 2 the corner k = trunc(y) -+ 2 lies within [y/2, 2y], so k - y is exact (Sterbenz)
// and (k - y) + y is k itself: the fp64 lateral edges are the integer ones and their comparison is an
// integer one. For wider boxes a corner can leave [y/2, 2y] (y < 2 veh_w) and its fp64 edge can then be
// k +- an ulp -- but only an edge that decides nothing: y1 >= y2 on the two arcs, so the deciding pair is
// the ego's left edge against the opponent's right edge, and they are within an ulp of each other only
// where trunc(y1) - trunc(y2) = veh_w. There y1 >= veh_w, so the ego's k = trunc(y1) - veh_w / 2 is in
// (0, y1]: k - y1 is a multiple of y1's ulp no larger than y1, hence exact; the opponent's right edge r = trunc(y2) + veh_w - veh_w / 2 >= |r - y2|,
// so the error of r - y2 (at most half an ulp of r) rounds away again in (r - y2) + y2. Up to
// |theta| = 1/16 a default lateral coordinate is 150 +- d with d <= 59; a car that drives on after
// arriving (live episodes do get there) can bring the opponent's mirror arc to y < 8, where the fp64
// form stays. Same result as the fp64 test for every input (tests/test_host_step.py drives both on the
// host, wide boxes at small y included).
MG_HD bool vehicles_collide(const mg_params& P, double y1, double x1, double y2, double x2) {
  if (y1 >= 8.0 && y2 >= 8.0) {
    const int l1 = static_cast<int>(y1) - P.veh_w / 2, l2 = static_cast<int>(y2) - P.veh_w / 2;
    if (l1 > l2 + P.veh_w || l2 > l1 + P.veh_w) return false;
    const int t1 = static_cast<int>(x1) - P.veh_h / 2, t2 = static_cast<int>(x2) - P.veh_h / 2;
    const double a_t = (static_cast<double>(t1) - x1) + x1, a_b = (static_cast<double>(t1 + P.veh_h) - x1) + x1;
    const double b_t = (static_cast<double>(t2) - x2) + x2, b_b = (static_cast<double>(t2 + P.veh_h) - x2) + x2;
    return a_t <= b_b && b_t <= a_b;
  }
  return boxes_intersect(vehicle_box(P, y1, x1), vehicle_box(P, y2, x2));
}

// observe (merging_env.py:118-132): computed in fp64, stored as OT (fp64 for the single-env
// record; fp32 -- the one rounding every fp32 output gets -- for the batched kernels)
template <class OT>
MG_HD void observe(const mg_params& P, double p1, double v1, double p2,
                                        double v2, double x1, double y1, double x2, double y2,
                                        OT (&o)[kObs]) {
  o[0] = static_cast<OT>(x2 - x1);
  o[1] = static_cast<OT>(y2 - y1);
  o[2] = static_cast<OT>(v2 - v1);
  o[3] = static_cast<OT>(P.end_point - p1);
  o[4] = static_cast<OT>(v1);
  o[5] = static_cast<OT>(x1 - x2);
  o[6] = static_cast<OT>(y1 - y2);
  o[7] = static_cast<OT>(v1 - v2);
  o[8] = static_cast<OT>(P.end_point - p2);
  o[9] = static_cast<OT>(v2);
}

template <class OT>
MG_HD void reset_obs(const mg_params& P, OT (&o)[kObs], double* dx1 = nullptr) {
  double x1, y1, x2, y2;
  lon2coord(P, P.start_point, true, x1, y1);
  lon2coord(P, P.start_point, false, x2, y2);
  observe(P, P.start_point, P.start_vel, P.start_point, P.start_vel, x1, y1, x2, y2, o);
  if (dx1) *dx1 = x2 - x1;
}

// The reset observation (merging_env.py:208-230 then observe): the same ten fp32 values and fp64
// x2 - x1 for every env, so each launch computes it once on the host (the same MG_HD functions, the
// same doubles) and the kernels copy it from the launch arguments (scalar loads) where autoreset
// fires, instead of two sin / cos and the observation in the divergent finishing branch.
struct Reset0 {
  float o[kObs];
  double dx1;
};

MG_HD Reset0 reset0(const mg_params& P) {
  Reset0 z;
  reset_obs(P, z.o, &z.dx1);
  return z;
}

// goal_status (scripts/hdqn.py:223-236) on the reference's fp64 values: dx1 = state[0] = x2 - x1,
// v2 = state[9] (an int 0 after max(0, ...) compares as 0.0). 0: dx1 < -v2/2, 1: dx1 < v2/2, else 2.
MG_HD int goal_status(double dx1, double v2) {
  return dx1 < -0.5 * v2 ? 0 : (dx1 < 0.5 * v2 ? 1 : 2);
}

// Philox4x32-10 (Salmon et al., SC'11 "Parallel random numbers: as easy as 1, 2, 3").
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const uint32_t lo0 = 0xD2511F53u * c.x, hi0 = __umulhi(0xD2511F53u, c.x);
    const uint32_t lo1 = 0xCD9E8D57u * c.z, hi1 = __umulhi(0xCD9E8D57u, c.z);
    c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
  }
  return c;
}

// floor(5 u / 2^32): uniform over {0..4} up to a 5/2^32 bias.
__device__ __forceinline__ int action_from_u32(uint32_t u) {
  return static_cast<int>((static_cast<uint64_t>(u) * MG_NUM_ACTIONS) >> 32);
}

enum ActMode { kActArrays = 0, kActPhilox = 1 };

// One env's state, held in registers for the duration of a launch.
struct Env {
  double p1, v1, p2, v2, ret1, ret2;
  uint32_t steps, winner;
  bool done;
};

MG_HD Env load_env(const mg_state& S, int64_t i) {
  Env e;
  e.p1 = S.p1[i];
  e.v1 = S.v1[i];
  e.p2 = S.p2[i];
  e.v2 = S.v2[i];
  e.ret1 = S.ret1[i];
  e.ret2 = S.ret2[i];
  const uint32_t tf = S.tf[i];
  e.steps = tf & MG_TF_STEPS_MASK;
  e.winner = (tf & MG_TF_WINNER_MASK) >> MG_TF_WINNER_SHIFT;
  e.done = (tf & MG_TF_DONE) != 0;
  return e;
}

MG_HD uint32_t pack_tf(const Env& e) {
  return e.steps | (e.winner << MG_TF_WINNER_SHIFT) | (e.done ? MG_TF_DONE : 0u);
}

MG_HD void store_env(const mg_state& S, int64_t i, const Env& e) {
  st_state(S.p1 + i, e.p1);
  st_state(S.v1 + i, e.v1);
  st_state(S.p2 + i, e.p2);
  st_state(S.v2 + i, e.v2);
  st_state(S.ret1 + i, e.ret1);
  st_state(S.ret2 + i, e.ret2);
  st_state(S.tf + i, static_cast<uint16_t>(pack_tf(e)));
}

// What one step returns besides the new state.
// The observation a step hands back, held as fp32: every batched output is fp32, and fp32
// here frees 10 VGPRs (66 -> fewer in the one-step kernel). The single-env record, which returns
// the reference's fp64 floats, recomputes its observation in fp64 from the state.
typedef float obs_t;

struct StepOut {
  obs_t o[kObs];  // observation (the reset observation once autoreset has fired)
  double r1, r2, acc1, acc2;
  double dx1;     // x2 - x1 of o in fp64 (hdqn.py goal_status's dx1; the reset one after autoreset)
  double ret_pre; // r1_accumulate before this step (read where first1)
  bool done, coll, r1_int, r2_int, v1_int, v2_int;
  bool first1;    // the ego arrived first on this step (winner None -> 1, merging_env.py:164-166)
  bool win_pre;   // main.py:225's END_POINT - p2 > END_POINT - p1 on the state this step acted on
  int bad;  // 1: action1 invalid, 2: action2 invalid (the reference's KeyError)
};

// The random-policy action stream: step k of global env gi takes word (k div 2) mod 4 of
// u = Philox4x32-10(counter (gi, k div 8), key seed) -- one call covers eight steps, two draws per
// 32-bit word, so a T-step rollout pays an eighth of a call's 40 multiplies per env-step (one call
// per step had been a third of the rollout kernel's VALU). A draw of m outcomes from word w is
// floor(m w / 2^32); an odd step draws from w' = m w mod 2^32 instead, the remainder of the first
// draw (m is odd, so w -> w' is a bijection of the 32-bit words and w' is again uniform; the two
// draws of one word are independent up to an m^2 / 2^32 bias). With both players random m = 25 and
// x = draw is the action pair, a1 = x div 5, a2 = x mod 5; with the None opponent m = 5, a1 = draw.
__device__ __forceinline__ uint4 philox_block(uint64_t gi, uint64_t block, uint64_t seed,
                                              bool opaque_key = false) {
  uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
  // opaque_key: a uniform key the compiler cannot hoist. In a multi-step loop the 20 round keys
  // are then scalar adds at each use instead of loop invariants spilled into VGPR lanes (one
  // v_readlane, a vector instruction, per round): -2 % per rollout step (A/B).
  if (opaque_key) asm volatile("" : "+s"(k0), "+s"(k1));
  return philox4x32_10(make_uint4(static_cast<uint32_t>(gi), static_cast<uint32_t>(gi >> 32),
                                  static_cast<uint32_t>(block), static_cast<uint32_t>(block >> 32)),
                       k0, k1);
}

// The four words of counter (gi, k): one env's draws of step (or call) k.
__device__ __forceinline__ uint4 philox_env_step(uint64_t gi, uint64_t step, uint64_t seed) {
  return philox4x32_10(make_uint4(static_cast<uint32_t>(gi), static_cast<uint32_t>(gi >> 32),
                                  static_cast<uint32_t>(step), static_cast<uint32_t>(step >> 32)),
                       static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32));
}

constexpr int kStepsPerPhilox = 8;  // steps one Philox4x32-10 call feeds: 4 words x 2 draws

__device__ __forceinline__ void actions_from_block(const uint4& u, uint64_t step, int opp_random, int& a1,
                                                   int& a2) {
  // word (step div 2) & 3 by a 64-bit select and shift on values: no indexed private array, no branch
  const uint64_t lo = (static_cast<uint64_t>(u.y) << 32) | u.x, hi = (static_cast<uint64_t>(u.w) << 32) | u.z;
  const uint32_t m = opp_random ? 25u : static_cast<uint32_t>(MG_NUM_ACTIONS);
  uint32_t w = static_cast<uint32_t>(((step & 4) ? hi : lo) >> (32 * ((step >> 1) & 1)));
  if (step & 1) w *= m;  // the second draw of the word
  const uint32_t x = static_cast<uint32_t>((static_cast<uint64_t>(w) * m) >> 32);
  const int b1 = static_cast<int>((x * 13u) >> 6);  // x div 5 for x < 25
  a1 = opp_random ? b1 : static_cast<int>(x);
  a2 = opp_random ? static_cast<int>(x) - 5 * b1 : MG_ACTION_NONE;
}

__device__ __forceinline__ void draw_actions(uint64_t gi, uint64_t step, uint64_t seed, int opp_random,
                                             int& a1, int& a2) {
  actions_from_block(philox_block(gi, step / kStepsPerPhilox, seed), step, opp_random, a1, a2);
}

// time_stamp += dT; done if time_stamp > 500 (:141-143). The fp64 clock first exceeds 500
// on step 2501; an integer count reproduces that exactly.
MG_HD void env_clock(const mg_params& P, Env& e) {
  e.steps = e.steps < MG_TF_STEPS_MASK ? e.steps + 1 : e.steps;
  if (static_cast<int32_t>(e.steps) >= P.timeout_steps) e.done = true;
}

// mpc_1d (helper.py:152-191): min u'(D'D + 0.01 I)u s.t. A[1] u = b, b = vt - v0 (only the
// velocity row of the constraint reaches solve_qp, :172-173, :182). quadprog's dual active-set
// method starts at the unconstrained minimiser u = 0 and adds the one equality in a single step,
// u = (b / z'n) z with z = J J'n, J = R^-1; action() = u[0]. z'n and z[0] are per-launch
// constants (mg_params.qp_nz / qp_z0, computed by mg_params_default in qpgen2's operation order),
// so this is two correctly rounded operations with the solver's own rounding; a residual |b| below
// qpgen2's vsmall counts as already satisfied and leaves the unconstrained minimiser u = -0.0 (dposl
// of a = -q, q = 0). (Mathematically u0 = b / t, since
// D.1 = 0; evaluating that closed form instead moves u0 by an ulp in most steps.)
MG_HD double mpc_acc_speed(const mg_params& P, double speed, double v) {
  const double b = speed - v;
  const double u = div_const(b, P.qp_nz, P.qp_inv_nz) * P.qp_z0;
  return fabs(b) < P.qp_vsmall ? -0.0 : u;  // dposl's -0.0 (a = -q = -0.0): nothing violated
}

MG_HD double mpc_acc(const mg_params& P, int a, double v) {
  return mpc_acc_speed(P, P.action_speed[a], v);
}

// action_dict[a] (merging_env.py:101) or 0.0 where a is not in it (the value is then unused)
MG_HD double action_speed_or0(const mg_params& P, int a) {
  return valid_action(a) ? P.action_speed[a] : 0.0;
}

// v = max(0, v + acc*dT) (an int 0 when the max picks 0), p += v*dT  (:149-150, :153-154)
MG_HD void move_car(const mg_params& P, double acc, double& p, double& v,
                                         bool& v_int) {
  const double nv = v + acc * P.dT;
  v_int = !(nv > 0.0);
  v = v_int ? 0.0 : nv;
  p = p + v * P.dT;
}

MG_HD void score_step(const mg_params& P, Env& e, double x1, double y1,
                                           double x2, double y2, StepOut& r, bool frozen = false);

// main.py:225's win test, state[8] > state[3] = END_POINT - p2 > END_POINT - p1, on the state a step
// acts on, evaluated before the move: left to the compiler it sinks into the rare finishing branch
// and keeps the pre-step positions live across the step (66 instead of 61 VGPRs in the step
// kernel: 7 waves per SIMD, a third round of blocks at 2^20 envs).
MG_HD bool win_test_early(const mg_params& P, const Env& e) {
  int w = (P.end_point - e.p2) > (P.end_point - e.p1) ? 1 : 0;
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(w));
#endif
  return w != 0;
}

// MergeEnv.step (merging_env.py:138-195) for one env held in registers. CHECKED = false: the
// caller guarantees a1 in 0..4 and a2 in -1..4 (device-drawn actions), so the KeyError path and
// its zeroed outputs are not compiled in.
// sp1 / sp2: action_dict[a1] / [a2], looked up by the caller (action_speed_or0), so it can issue
// those loads before the state loads (the step kernel; env_step below looks them up itself)
template <bool CHECKED = true>
MG_HD void env_step_sp(const mg_params& P, Env& e, int a1, int a2, double sp1, double sp2,
                                            StepOut& r) {
  r.win_pre = win_test_early(P, e);
  r.first1 = false;
  r.dx1 = 0.0;
  env_clock(P, e);
  const bool bad1 = CHECKED && !valid_action(a1);
  const bool bad2 = CHECKED && !(a2 == MG_ACTION_NONE || valid_action(a2));
  r.bad = (bad1 ? 1 : 0) | (bad2 ? 2 : 0);
  r.acc1 = r.acc2 = 0.0;
  r.v1_int = r.v2_int = false;
  r.done = r.coll = r.r1_int = r.r2_int = false;
  r.r1 = r.r2 = 0.0;
  if (!bad1) {
    r.acc1 = mpc_acc_speed(P, sp1, e.v1);
    move_car(P, r.acc1, e.p1, e.v1, r.v1_int);
  }
  if (r.bad) {  // the reference raises KeyError at action_dict[...] after advancing this far
#pragma unroll
    for (int k = 0; k < kObs; ++k) r.o[k] = 0.0;
    return;
  }
  // action2 None -> acc 0 (:152): the "L0" constant-speed opponent
  if (a2 != MG_ACTION_NONE) r.acc2 = mpc_acc_speed(P, sp2, e.v2);
  move_car(P, r.acc2, e.p2, e.v2, r.v2_int);

  double x1, y1, x2, y2;
  lon2coord(P, e.p1, true, x1, y1);
  lon2coord(P, e.p2, false, x2, y2);
  score_step(P, e, x1, y1, x2, y2, r);
}

template <bool CHECKED = true>
MG_HD void env_step(const mg_params& P, Env& e, int a1, int a2, StepOut& r) {
  env_step_sp<CHECKED>(P, e, a1, a2, action_speed_or0(P, a1), action_speed_or0(P, a2), r);
}

// N envs stepped statement by statement, so their independent fp64 chains interleave in one
// instruction stream. Identical results to N env_step calls, invalid actions included: those
// are computed with a stand-in action and their effects dropped by selects (the ego keeps its
// move unless action1 is bad; nothing after the moves happens, as in env_step's early return).
template <int N, bool CHECKED = true>
__device__ __forceinline__ void env_step_lockstep(const mg_params& P, Env (&e)[N], const int (&a1)[N],
                                                  const int (&a2)[N], StepOut (&r)[N]) {
  double ang[2 * N], sn[2 * N], cs[2 * N];
  bool bad[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const bool bad1 = CHECKED && !valid_action(a1[j]);
    const bool none2 = a2[j] == MG_ACTION_NONE;
    const bool bad2 = CHECKED && !(none2 || valid_action(a2[j]));
    bad[j] = bad1 || bad2;
    r[j].bad = (bad1 ? 1 : 0) | (bad2 ? 2 : 0);
    r[j].r1_int = r[j].r2_int = false;
    r[j].win_pre = win_test_early(P, e[j]);
    r[j].first1 = false;
    env_clock(P, e[j]);
    const double acc1 = mpc_acc(P, bad1 ? 0 : a1[j], e[j].v1);
    r[j].acc1 = bad1 ? 0.0 : acc1;
    double p = e[j].p1, v = e[j].v1;
    bool vi;
    move_car(P, r[j].acc1, p, v, vi);
    e[j].p1 = bad1 ? e[j].p1 : p;
    e[j].v1 = bad1 ? e[j].v1 : v;
    r[j].v1_int = !bad1 && vi;
    const double acc2 = mpc_acc(P, (none2 || bad2) ? 0 : a2[j], e[j].v2);
    r[j].acc2 = (none2 || bad[j]) ? 0.0 : acc2;
    p = e[j].p2;
    v = e[j].v2;
    move_car(P, r[j].acc2, p, v, vi);
    e[j].p2 = bad[j] ? e[j].p2 : p;
    e[j].v2 = bad[j] ? e[j].v2 : v;
    r[j].v2_int = !bad[j] && vi;
    ang[2 * j] = arc_angle(P, e[j].p1);
    ang[2 * j + 1] = arc_angle(P, e[j].p2);
  }
  arc_sincos_n<2 * N>(ang, sn, cs);
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double x1, y1, x2, y2;
    arc_xy(P, sn[2 * j], cs[2 * j], true, x1, y1);
    arc_xy(P, sn[2 * j + 1], cs[2 * j + 1], false, x2, y2);
    score_step(P, e[j], x1, y1, x2, y2, r[j], bad[j]);
  }
}

// The rest of a step once both cars have moved (merging_env.py:156-192): observation, rewards,
// arrival / winner, collision, returns. r.r1_int / r.r2_int must be false on entry. frozen: an
// invalid action -- the step stops before any of this (observation and rewards 0, no state
// change), as env_step's early return.
MG_HD void score_step(const mg_params& P, Env& e, double x1, double y1,
                                           double x2, double y2, StepOut& r, bool frozen) {
  observe(P, e.p1, e.v1, e.p2, e.v2, x1, y1, x2, y2, r.o);
  r.dx1 = x2 - x1;
  r.ret_pre = e.ret1;
  if (frozen) {
#pragma unroll
    for (int k = 0; k < kObs; ++k) r.o[k] = 0.0;
  }

  // rewards (:158-159): -time_penalty - vel_penalty * |v - 20|
  double r1 = (0.0 - P.time_penalty) - P.vel_penalty * fabs(e.v1 - P.vel_ref);
  double r2 = (0.0 - P.time_penalty) - P.vel_penalty * fabs(e.v2 - P.vel_ref);

  // arrival / winner state machine (:163-181); ego strict '>', opponent '>='
  if (!frozen && e.p1 > P.end_point) {
    if (e.winner == 0) {
      e.winner = 1;
      r1 += P.r_first;
      r.first1 = true;
    } else if (e.winner == 1) {
      r1 = 0.0;
      r.r1_int = true;
    } else {
      r1 += P.r_second;
      e.done = true;
    }
  }
  if (!frozen && e.p2 >= P.end_point) {
    if (e.winner == 0) {
      e.winner = 2;
      r2 += P.r_first;
    } else if (e.winner == 2) {
      r2 = 0.0;
      r.r2_int = true;
    } else {
      r2 += P.r_second;
      e.done = true;
    }
  }

  // is_collided (:183-187, :198-206)
  r.coll = !frozen && vehicles_collide(P, y1, x1, y2, x2);
  if (r.coll) {
    e.done = true;
    r1 += P.r_collision;
    r2 += P.r_collision;
  }
  if (!frozen) {
    e.ret1 += r1;  // :191-192
    e.ret2 += r2;
  }
  r.r1 = frozen ? 0.0 : r1;
  r.r2 = frozen ? 0.0 : r2;
  r.done = !frozen && e.done;
}

}  // namespace
