// mg_rainbow_learn.h -- Rainbow's compute_td_loss on the device: the done-carrying replay store, the C51
// projection, the noisy-net forward and backward, Adam and the noise reset, with the per-element functions
// the host twins (mg_host_rainbow_learn*) run too. The learner in both forms: the plain one is the prioritized
// one (mg_per.h's tree, sample and update) without a tree, so a call has one check, one launch order beside
// its host twin and one pair of drivers; the replay stores likewise. A population of up to 64 plain learners
// (mg_rainbow_learn_many) runs the same kernel bodies with the member in the grid: each kernel is a template on
// its argument, RLearn for the lone call or RLearnMany, from which rl_member rebases member m's RLearn. The members
// may be prioritized too (mg_rainbow_learn_prioritized_many): PerMany carries their trees to mg_per.h's sample and
// update kernels, templated the same way, and mg_per_store_many is the member store with the trees' launches.
// A part of the one translation unit merging_hip.hip (see its head comment).
#pragma once

#include "mg_common.h"
#include "mg_env.h"
#include "mg_launch.h"
#include "mg_learn.h"
#include "mg_learn_core.h"
#include "mg_per.h"
#include "mg_rainbow.h"
#include "mg_replay.h"

namespace {

// ============================================================================ Rainbow's replay rows
// ReplayBuffer (scripts/ranbowdqn.py:265-323) as a ring of 24-float rows [s(10), a, r, s'(10), done, 0]:
// push (:281-288) keeps every transition, so slot (counter + t n + i) % capacity needs no scan.
constexpr int kRlRow = 24;
constexpr int kRlColA = kObs, kRlColR = kObs + 1, kRlColS2 = kObs + 2, kRlColDone = 2 * kObs + 2;

struct RlStore {
  mg_transitions X;
  int64_t n;
  int64_t total;  // T n
};

// transition idx = t n + i of a store (the host twin of the prioritized store runs it too). The tensors are
// [T, stride, ...] and the store's envs their columns [col0, col0 + n): the lone stores pass (n, 0), the member
// store the whole batch's width and the member's first column.
MG_HD void rl_store_at(const RlStore& R, const uint64_t* counter, float* rows, int64_t cap, int64_t idx,
                       int64_t stride, int64_t col0) {
  // only the newest `cap` transitions survive sequential pushes: they occupy distinct slots
  const int64_t skip = R.total > cap ? R.total - cap : 0;
  if (idx >= R.total || idx < skip) return;
  const int64_t t = idx / R.n;
  const int64_t c = col0 + (idx - t * R.n);  // the column in the tensors
  const int64_t row = t * stride + c;
  const bool done = R.X.flags ? R.X.flags[4 * row + 2] != 0 : (R.X.done != nullptr && R.X.done[row] != 0);
  const float* s = t == 0 ? R.X.obs_first + c * kObs : R.X.obs + (row - stride) * kObs;
  const float* s2 = (done && R.X.final_obs ? R.X.final_obs : R.X.obs) + row * kObs;
  float v[kRlRow];
#pragma unroll
  for (int k = 0; k < kObs; ++k) v[k] = s[k], v[kRlColS2 + k] = s2[k];
  v[kRlColA] = static_cast<float>(R.X.flags ? static_cast<int8_t>(R.X.flags[4 * row]) : R.X.a1[row]);
  v[kRlColR] = R.X.rew[2 * row];
  v[kRlColDone] = done ? 1.0f : 0.0f;
  v[kRlRow - 1] = 0.0f;
  const uint64_t slot = (*counter + static_cast<uint64_t>(idx)) % static_cast<uint64_t>(cap);
  f32x2* d = reinterpret_cast<f32x2*>(rows + slot * kRlRow);
#pragma unroll
  for (int k = 0; k < kRlRow / 2; ++k) d[k] = f32x2{v[2 * k], v[2 * k + 1]};
}

__global__ __launch_bounds__(kBlock) void rl_store_kernel(const RlStore R, const uint64_t* counter, float* rows,
                                                          int64_t cap) {
  rl_store_at(R, counter, rows, cap, static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x, R.n, 0);
}

// ---- the member in the grid (mg_rainbow_replay_store_many): member m's slice [m n_member, (m + 1) n_member) of one
// [T, N, ...] batch into ring m, as the lone store would store a contiguous copy of the slice. Every transition is
// kept, so a member's slots need no scan: grid (ceil(T n_member / kBlock), members), the rings and counters in
// the kernel argument, then one thread per member moves its counter.
struct RlStoreMany {
  RlStore R;  // X: the whole batch; n = n_member; total = T n_member
  int64_t N;  // the batch's envs, the row stride
  int64_t cap;
  int32_t members;
  float* rows[kMaxMembers];
  uint64_t* counter[kMaxMembers];
};
static_assert(sizeof(RlStoreMany) <= 4096, "HIP's kernel argument limit");

__global__ __launch_bounds__(kBlock) void rl_store_many_kernel(const RlStoreMany A) {
  const int m = blockIdx.y;
  rl_store_at(A.R, A.counter[m], A.rows[m], A.cap, static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x, A.N,
              m * A.R.n);
}

// launched behind the store, after every thread of it has read the old counters: the stream orders it
__global__ __launch_bounds__(kMaxMembers) void rl_counter_add_many_kernel(const RlStoreMany A) {
  const int m = threadIdx.x;
  if (m < A.members) *A.counter[m] += static_cast<uint64_t>(A.R.total);
}

// ============================================================================ compute_td_loss
// scripts/ranbowdqn.py:554-609 on RainbowDQN(10, 5) with 51 atoms, all fp32 in the fixed order
// include/merging_hip.h documents at mg_rainbow_learn. The learner buffer: current, target, Adam m, Adam v
// (kRlParams each, RainbowDQN.named_parameters() order), the two models' full noise buffers (kRlEps each,
// per noisy layer weight_epsilon then bias_epsilon), the support z[52].
constexpr int kRlW1 = 0, kRlB1 = kRbH1 * kRbIn, kRlW2 = kRlB1 + kRbH1, kRlB2 = kRlW2 + kRbH2 * kRbH1;
constexpr int kRlPlain = kRlB2 + kRbH2;  // 2,464
constexpr int kRlParams = 58884, kRlEps = 28210, kRlFactors = 1124, kRlZ = 52;
constexpr int kRlOffM = 2 * kRlParams, kRlOffV = 3 * kRlParams, kRlOffEps = 4 * kRlParams;
constexpr int kRlOffZ = kRlOffEps + 2 * kRlEps, kRlLearner = kRlOffZ + kRlZ;
constexpr int kRlThreads = 320;  // one thread per head unit (306)
static_assert(kRlLearner % 4 == 0 && kRlThreads >= kRbLogits, "16-byte learner, a thread per logit");

// Noisy layer l (0 value1, 1 value2, 2 advantage1, 3 advantage2; reset_noise's order, :537-541): its width,
// the offset p of weight_mu in a parameter block (then weight_sigma, bias_mu, bias_sigma), the offset e of
// weight_epsilon in a noise block (then bias_epsilon; the effective weights use the same layout) and the
// offset f of its factors eps_in, eps_out, bias noise in one model's kRlFactors.
struct RlNoisy {
  int out, p, e, f;
};
MG_HD RlNoisy rl_noisy(int l) {
  switch (l) {
    case 0: return {kRbHS, kRlPlain, 0, 0};
    case 1: return {kRbAtoms, kRlPlain + 8320, 4160, 192};
    case 2: return {kRbHS, kRlPlain + 14950, 7475, 358};
    default: return {kRbActions * kRbAtoms, kRlPlain + 23270, 11635, 550};
  }
}
// the noisy layer that holds index i of a block whose layer l starts at start(l)
MG_HD int rl_layer_of_eps(int e) { return e < 4160 ? 0 : e < 7475 ? 1 : e < 11635 ? 2 : 3; }
MG_HD int rl_layer_of_param(int i) { return i < kRlPlain + 8320 ? 0 : i < kRlPlain + 14950 ? 1 : i < kRlPlain + 23270 ? 2 : 3; }

struct RlScratch {  // sections (floats), each a multiple of four; prioritized: then idx [B] int64 and w [B]
  int64_t rows, h1, h2, hv, ha, dlog, dhv, dha, dh2, dh1, lossb, g, geff, eff, pidx, pw, total;
};
MG_HD RlScratch rl_scratch(int64_t B, bool prioritized) {
  RlScratch S;
  S.rows = 0;
  S.h1 = S.rows + B * kRlRow;
  S.h2 = S.h1 + B * kRbH1;
  S.hv = S.h2 + B * kRbH2;
  S.ha = S.hv + B * kRbHS;
  S.dlog = S.ha + B * kRbHS;
  S.dhv = S.dlog + learn_round4(B * kRbLogits);
  S.dha = S.dhv + B * kRbHS;
  S.dh2 = S.dha + B * kRbHS;
  S.dh1 = S.dh2 + B * kRbH2;
  S.lossb = S.dh1 + B * kRbH1;
  S.g = S.lossb + learn_round4(B);
  S.geff = S.g + kRlPlain;
  S.eff = S.geff + learn_round4(kRlEps);
  S.pidx = S.eff + learn_round4(2 * kRlEps);
  S.pw = S.pidx + (prioritized ? learn_round4(2 * B) : 0);
  S.total = S.pw + (prioritized ? learn_round4(B) : 0);
  return S;
}

// Everything one update's launches (or the host loops) read.
struct RLearn {
  float* buf;  // the learner buffer
  const float* ring;
  const uint64_t* counter;
  int64_t cap;
  uint64_t seed, draw;
  int32_t B;
  float *rows, *h1, *h2, *hv, *ha, *dlog, *dhv, *dha, *dh2, *dh1, *lossb, *g, *geff, *eff;  // scratch sections
  const float* noise;  // this update's factors [2][kRlFactors]: current, target
  float *rows_out, *loss_out, *proj_out, *grads_out;  // this update's, or NULL
  float gamma, inv_b;
  LearnAdam A;
  // prioritized replay (mg_per.h), or NULL: row b is ring row pidx[b] and its loss is weighted by pw[b]
  const int64_t* pidx;
  const float* pw;
};

// the ring row of minibatch row b, and the factor its gradient carries: 1 / B, or w_b * (1 / B) rounded once
MG_HD uint64_t rl_row_slot(const RLearn& L, uint64_t live, int b) {
  return L.pidx ? static_cast<uint64_t>(L.pidx[b]) : learn_slot(static_cast<uint64_t>(b), L.draw, L.seed, live);
}
MG_HD float rl_row_scale(const RLearn& L, int b) { return L.pw ? L.pw[b] * L.inv_b : L.inv_b; }

// ---------------------------------------------------------------------------- per-element functions
// log(x) for a normal x > 0, the same bits on host and device (the loss takes it on [0.01, 0.99]): x = 2^k m
// with m in [sqrt(1/2), sqrt 2), f = m - 1, s = f / (2 + f), log(1 + f) = f - f^2/2 + s (f^2/2 + R(s^2)) with
// the classic degree-4 minimax R in s^2 (fdlibm's logf), and k ln 2 added in two parts. Every operation is
// rounded once; no fmaf. Not the hardware v_log_f32, which the host cannot reproduce.
MG_HD float rb_log(float x) {
  uint32_t ix = __builtin_bit_cast(uint32_t, x);
  ix += 0x3f800000u - 0x3f3504f3u;
  const float dk = static_cast<float>(static_cast<int>(ix >> 23) - 127);
  ix = (ix & 0x007fffffu) + 0x3f3504f3u;
  const float f = __builtin_bit_cast(float, ix) - 1.0f;
  const float s = f / (2.0f + f);
  const float z = s * s;
  const float w = z * z;
  const float t1 = w * (0.40000972152f + w * 0.24279078841f);
  const float t2 = z * (0.66666662693f + w * 0.28498786688f);
  const float R = t2 + t1;
  const float hfsq = (0.5f * f) * f;
  return (((s * (hfsq + R) + dk * 9.0580006145e-06f) - hfsq) + f) + dk * 6.9313812256e-01f;
}

// the 51 atoms as four chains over 13 g .. 13 g + 12, each from +0 ascending, combined (c0 + c1) + (c2 + c3)
// (host_rainbow_head_row's order)
MG_HD float rl_sum4(const float* v) {
  float c[4];
  for (int g = 0; g < 4; ++g) {
    c[g] = 0.0f;
    for (int i = kRbSlots * g; i < kRbSlots * (g + 1) && i < kRbAtoms; ++i) c[g] = c[g] + v[i];
  }
  return (c[0] + c[1]) + (c[2] + c[3]);
}

// element t = 51 a + i of the dueling combination from the logits lg [306] (value [51], advantage [5][51])
MG_HD float rl_head_x(const float* lg, int t) {
  const float* A = lg + kRbAtoms;
  const int i = t % kRbAtoms;
  const float mean = rb_mean(A[i], A[kRbAtoms + i], A[2 * kRbAtoms + i], A[3 * kRbAtoms + i], A[4 * kRbAtoms + i]);
  return rb_duel(lg[i], A[t], mean);
}
MG_HD float rl_max51(const float* x) {
  float m = -INFINITY;
  for (int i = 0; i < kRbAtoms; ++i) m = fmaxf(m, x[i]);
  return m;
}
// softmax over the atoms of action a into p [51], in the head's order: x, m = max, e = exp(x - m), S the four
// chains, e / S (the kernel runs the same steps with one thread per element)
MG_HD void rl_softmax(const float* lg, int a, float* p) {
  for (int i = 0; i < kRbAtoms; ++i) p[i] = rl_head_x(lg, a * kRbAtoms + i);
  const float m = rl_max51(p);
  for (int i = 0; i < kRbAtoms; ++i) p[i] = rb_exp(p[i] - m);
  const float S = rl_sum4(p);
  for (int i = 0; i < kRbAtoms; ++i) p[i] = p[i] / S;
}

// b of atom z (:569-571): Tz = r + ((1 - done) gamma) z clamped to the support, (Tz - Vmin) / delta_z
MG_HD float rl_b(float r, float done, float gamma, float z) {
  float tz = r + ((1.0f - done) * gamma) * z;
  tz = fminf(fmaxf(tz, -10.0f), 10.0f);
  return (tz - -10.0f) / 0.4f;
}

// slot j of proj_dist (:578-580): every l contribution in atom order, then every u contribution, each a
// rounded product added into the slot from +0; nd is the support-scaled row of the chosen action
MG_HD float rl_proj_slot(int j, const float* nd, const float* bb) {
  const float fj = static_cast<float>(j);
  float acc = 0.0f;
  for (int i = 0; i < kRbAtoms; ++i)
    if (floorf(bb[i]) == fj) acc = acc + nd[i] * (ceilf(bb[i]) - bb[i]);
  for (int i = 0; i < kRbAtoms; ++i)
    if (ceilf(bb[i]) == fj) acc = acc + nd[i] * (bb[i] - floorf(bb[i]));
  return acc;
}

// loss_b = -sum_i proj_i log(c_i), c = clamp(y, 0.01, 0.99) (:598-599), the products summed from +0 in atom
// order; dx [51] = the gradient at the chosen action's logits: g_i = -(proj_i / c_i) (1 / B) (log's backward
// sees the clamped copy), dot = the fmaf chain of g_k y_k from +0, dx_i = y_i (g_i - dot) (softmax's backward
// sees y)
MG_HD float rl_loss_row(const float* y, const float* proj, float inv_b, float* dx) {
  float acc = 0.0f, dot = 0.0f;
  for (int i = 0; i < kRbAtoms; ++i) {
    const float c = fminf(fmaxf(y[i], 0.01f), 0.99f);
    acc = acc + proj[i] * rb_log(c);
    dx[i] = -(proj[i] / c) * inv_b;
    dot = fmaf(dx[i], y[i], dot);
  }
  for (int i = 0; i < kRbAtoms; ++i) dx[i] = y[i] * (dx[i] - dot);
  return -acc;
}

// the gradient at logit t of [306] through the dueling combination: dv_i = dx_i, dA[a][i] = dx_i (d(a, a*) - 1/5)
MG_HD float rl_dlogit(const float* dx, int astar, int t) {
  if (t < kRbAtoms) return dx[t];
  const int a = (t - kRbAtoms) / kRbAtoms, i = (t - kRbAtoms) - a * kRbAtoms;
  const float fifth = dx[i] / 5.0f;
  return a == astar ? dx[i] - fifth : -fifth;
}

// one unit of each layer: P a parameter block, eff that model's effective noisy weights
MG_HD float rl_unit_h1(const float* P, const float* x, int j) {
  return learn_relu(learn_fwd(x, P + kRlW1 + j * kRbIn, P[kRlB1 + j], kRbIn));
}
MG_HD float rl_unit_h2(const float* P, const float* h1, int j) {
  return learn_relu(learn_fwd(h1, P + kRlW2 + j * kRbH1, P[kRlB2 + j], kRbH1));
}
MG_HD float rl_unit_noisy(const float* eff, int l, const float* x, int j) {
  const RlNoisy N = rl_noisy(l);
  return learn_fwd(x, eff + N.e + j * kRbHS, eff[N.e + N.out * kRbHS + j], kRbHS);
}
MG_HD float rl_unit_logit(const float* eff, const float* hv, const float* ha, int t) {
  return t < kRbAtoms ? rl_unit_noisy(eff, 1, hv, t) : rl_unit_noisy(eff, 3, ha, t - kRbAtoms);
}

// the first maximum of q [5]
MG_HD int rl_argmax(const float* q) {
  int best = 0;
  for (int a = 1; a < kRbActions; ++a)
    if (q[a] > q[best]) best = a;
  return best;
}

// Element idx of (model, e) over the two noise blocks: with factors, the new epsilon (eps_out[j] eps_in[k],
// one rounded product as ger gives; the bias noise as drawn) is stored first; then the effective value
// mu + sigma * eps (the product rounded, then the sum) of that model.
MG_HD void rl_noise_eff_at(const RLearn& L, int idx, bool redraw) {
  const int model = idx / kRlEps, e = idx - model * kRlEps;
  const RlNoisy N = rl_noisy(rl_layer_of_eps(e));
  const int r = e - N.e, nw = N.out * kRbHS;
  float* eps = L.buf + kRlOffEps + model * kRlEps + e;
  if (redraw) {
    const float* F = L.noise + model * kRlFactors + N.f;
    *eps = r < nw ? F[kRbHS + r / kRbHS] * F[r % kRbHS] : F[kRbHS + N.out + (r - nw)];
  }
  const float* P = L.buf + model * kRlParams + N.p;
  const float mu = r < nw ? P[r] : P[2 * nw + (r - nw)];
  const float sigma = r < nw ? P[nw + r] : P[2 * nw + N.out + (r - nw)];
  L.eff[model * kRlEps + e] = mu + sigma * *eps;
}

// the gradient of parameter i: the plain layers' as computed; a noisy layer's g_mu = g_w, g_sigma = g_w eps
MG_HD float rl_param_grad(const RLearn& L, int i) {
  if (i < kRlPlain) return L.g[i];
  const RlNoisy N = rl_noisy(rl_layer_of_param(i));
  const int nw = N.out * kRbHS;
  int r = i - N.p;
  const float* eps = L.buf + kRlOffEps;  // the current model's
  if (r < nw) return L.geff[N.e + r];
  if (r < 2 * nw) return L.geff[N.e + r - nw] * eps[N.e + r - nw];
  r -= 2 * nw;
  if (r < N.out) return L.geff[N.e + nw + r];
  return L.geff[N.e + nw + r - N.out] * eps[N.e + nw + r - N.out];
}

// item i of the Adam launch: parameter i, or at i == kRlParams the loss, the sequential sum of loss_b (with
// weights: of w_b * loss_b, each product rounded once) times 1 / B
MG_HD void rl_adam_at(const RLearn& L, int i) {
  if (i == kRlParams) {
    if (L.loss_out) *L.loss_out = (L.pw ? learn_wsum(L.pw, L.lossb, L.B) : learn_sum(L.lossb, 1, L.B)) * L.inv_b;
    return;
  }
  const float g = rl_param_grad(L, i);
  if (L.grads_out) L.grads_out[i] = g;
  learn_adam(L.buf[i], L.buf[kRlOffM + i], L.buf[kRlOffV + i], g, L.A);
}

// the hidden streams' input gradient: dh2[b, k] = the value stream's chain plus the advantage stream's, then
// the mask of linear2's ReLU
MG_HD void rl_dh2_at(const RLearn& L, int64_t idx) {
  const int64_t b = idx / kRbH2;
  const int k = static_cast<int>(idx - b * kRbH2);
  const float v = learn_chain(L.dhv + b * kRbHS, 1, L.eff + rl_noisy(0).e + k, kRbH2, kRbHS);
  const float a = learn_chain(L.dha + b * kRbHS, 1, L.eff + rl_noisy(2).e + k, kRbH2, kRbHS);
  const float s = v + a;
  L.dh2[idx] = L.h2[idx] > 0.0f ? s : 0.0f;
}

// The backward launches' layers: 0 value2, 1 advantage2 (with the hidden streams' dx), 2 value1, 3 advantage1
// (gradients only: rl_dh2_at sums their dx), 4 linear2, 5 linear1.
MG_HD LearnBwd rl_bwd_layer(const RLearn& L, int which) {
  LearnBwd G{};
  G.B = L.B;
  G.inv_b = L.inv_b;
  if (which < 4) {
    static_assert(kRbH2 == kRbHS, "the streams' inputs are all 64 wide");
    const int l = which == 0 ? 1 : which == 1 ? 3 : which == 2 ? 0 : 2;
    const RlNoisy N = rl_noisy(l);
    G.nJ = N.out, G.nK = kRbHS, G.sx = kRbHS;
    G.W = L.eff + N.e, G.gW = L.geff + N.e, G.gb = L.geff + N.e + N.out * kRbHS;
    if (which == 0) G.dy = L.dlog, G.sdy = kRbLogits, G.x = L.hv, G.dx = L.dhv;
    if (which == 1) G.dy = L.dlog + kRbAtoms, G.sdy = kRbLogits, G.x = L.ha, G.dx = L.dha;
    if (which == 2) G.dy = L.dhv, G.sdy = kRbHS, G.x = L.h2;
    if (which == 3) G.dy = L.dha, G.sdy = kRbHS, G.x = L.h2;
  } else if (which == 4) {
    G.dy = L.dh2, G.sdy = kRbH2, G.nJ = kRbH2;
    G.x = L.h1, G.sx = kRbH1, G.nK = kRbH1;
    G.W = L.buf + kRlW2, G.gW = L.g + kRlW2, G.gb = L.g + kRlB2;
    G.dx = L.dh1;
  } else {
    G.dy = L.dh1, G.sdy = kRbH1, G.nJ = kRbH1;
    G.x = L.rows, G.sx = kRlRow, G.nK = kRbIn;
    G.W = L.buf + kRlW1, G.gW = L.g + kRlW1, G.gb = L.g + kRlB1;
  }
  return G;
}

// Row b's part of an update on plain memory -- both forwards, the projection, loss_b and dlogits -- which the
// host twin runs as it stands; rl_forward_kernel gives the same steps one thread per unit.
inline void host_rl_forward_row(const RLearn& L, uint64_t live, int b) {
  const float* row = L.ring + rl_row_slot(L, live, b) * kRlRow;
  const float* z = L.buf + kRlOffZ;
  float h1[kRbH1], h2[kRbH2], hv[kRbHS], ha[kRbHS], lg[kRbLogits], p[kRbActions * kRbAtoms], q[kRbActions];
  float bb[kRbAtoms], proj[kRbAtoms], dx[kRbAtoms];
  for (int k = 0; k < kRlRow; ++k) {
    L.rows[b * kRlRow + k] = row[k];
    if (L.rows_out) L.rows_out[b * kRlRow + k] = row[k];
  }
  for (int pass = 1; pass >= 0; --pass) {  // target(s'), then current(s)
    const float* P = L.buf + pass * kRlParams;
    const float* eff = L.eff + pass * kRlEps;
    const float* x = row + (pass ? kRlColS2 : 0);
    for (int j = 0; j < kRbH1; ++j) h1[j] = rl_unit_h1(P, x, j);
    for (int j = 0; j < kRbH2; ++j) h2[j] = rl_unit_h2(P, h1, j);
    for (int j = 0; j < kRbHS; ++j) hv[j] = learn_relu(rl_unit_noisy(eff, 0, h2, j));
    for (int j = 0; j < kRbHS; ++j) ha[j] = learn_relu(rl_unit_noisy(eff, 2, h2, j));
    for (int t = 0; t < kRbLogits; ++t) lg[t] = rl_unit_logit(eff, hv, ha, t);
    for (int a = 0; a < kRbActions; ++a) rl_softmax(lg, a, p + a * kRbAtoms);
    if (pass) {
      for (int a = 0; a < kRbActions; ++a) {
        for (int i = 0; i < kRbAtoms; ++i) p[a * kRbAtoms + i] = p[a * kRbAtoms + i] * z[i];
        q[a] = rl_sum4(p + a * kRbAtoms);
      }
      const float* nd = p + rl_argmax(q) * kRbAtoms;
      for (int i = 0; i < kRbAtoms; ++i) bb[i] = rl_b(row[kRlColR], row[kRlColDone], L.gamma, z[i]);
      for (int j = 0; j < kRbAtoms; ++j) {
        proj[j] = rl_proj_slot(j, nd, bb);
        if (L.proj_out) L.proj_out[b * kRbAtoms + j] = proj[j];
      }
    } else {
      const int astar = learn_action(row[kRlColA], kRbActions);
      L.lossb[b] = rl_loss_row(p + astar * kRbAtoms, proj, rl_row_scale(L, b), dx);
      for (int t = 0; t < kRbLogits; ++t) L.dlog[b * kRbLogits + t] = rl_dlogit(dx, astar, t);
      for (int j = 0; j < kRbH1; ++j) L.h1[b * kRbH1 + j] = h1[j];
      for (int j = 0; j < kRbH2; ++j) L.h2[b * kRbH2 + j] = h2[j];
      for (int j = 0; j < kRbHS; ++j) L.hv[b * kRbHS + j] = hv[j], L.ha[b * kRbHS + j] = ha[j];
    }
  }
}

// ---------------------------------------------------------------------------- the members of a call
// A population (mg_rainbow_learn_many): up to 64 learners of one batch size and capacity in the lone learner's
// launches, the member in the grid's y. What a member keeps for all its updates -- ring, counter, seed, gamma,
// Adam's constants, rounded as learn_adam_scalars rounds them -- is mg_learn.h's LearnMember in a device table
// (mg_rainbow_learn_many_init); the per-update values -- each member's draw, Adam's step and bc2s from the
// host's doubles -- travel by value. The table is a typed global pointer of the kernel argument, so an entry
// arrives by scalar loads.
struct RLearnMany {
  float* learners;           // [members, kRlLearner]
  float* scratch;            // [members, stride]
  const LearnMember* table;  // [members]
  const float* noise;        // this update's factors [members][2][kRlFactors]
  float *rows_out, *loss_out, *proj_out, *grads_out;  // this update's [members, ...], or NULL
  int64_t stride;            // floats of one member's scratch: rl_scratch(B, prioritized).total
  int64_t cap;
  int32_t B, members;
  float inv_b;
  int32_t prioritized;       // the members' rows and weights are their scratch's pidx and pw (PerMany's sample)
  uint64_t draw[kMaxMembers];
  float step[kMaxMembers];
  float bc2s[kMaxMembers];
};
static_assert(sizeof(RLearnMany) <= 1200, "the by-value kernel argument stays well inside HIP's 4096 bytes");

// the scratch sections of a learner whose scratch starts at s
MG_HD void rl_set_scratch(RLearn& L, float* s, const RlScratch& S) {
  L.rows = s + S.rows, L.h1 = s + S.h1, L.h2 = s + S.h2, L.hv = s + S.hv, L.ha = s + S.ha, L.dlog = s + S.dlog;
  L.dhv = s + S.dhv, L.dha = s + S.dha, L.dh2 = s + S.dh2, L.dh1 = s + S.dh1, L.lossb = s + S.lossb;
  L.g = s + S.g, L.geff = s + S.geff, L.eff = s + S.eff;
}

// Member m's RLearn: its block, its scratch, its rows of the outputs and the noise, its entry and per-update
// scalars. The lone call's argument is its one member's already.
MG_HD RLearn rl_member(const RLearnMany& Q, int m) {
  const LearnMember& T = Q.table[m];
  RLearn L{};
  L.buf = Q.learners + static_cast<int64_t>(m) * kRlLearner;
  L.ring = T.ring, L.counter = T.counter, L.cap = Q.cap, L.seed = T.seed, L.draw = Q.draw[m], L.B = Q.B;
  const RlScratch S = rl_scratch(Q.B, Q.prioritized != 0);
  float* s = Q.scratch + m * Q.stride;
  rl_set_scratch(L, s, S);
  if (Q.prioritized) L.pidx = reinterpret_cast<const int64_t*>(s + S.pidx), L.pw = s + S.pw;
  L.noise = Q.noise ? Q.noise + static_cast<int64_t>(m) * 2 * kRlFactors : nullptr;  // NULL in front of the updates
  L.rows_out = Q.rows_out ? Q.rows_out + static_cast<int64_t>(m) * Q.B * kRlRow : nullptr;
  L.loss_out = Q.loss_out ? Q.loss_out + m : nullptr;
  L.proj_out = Q.proj_out ? Q.proj_out + static_cast<int64_t>(m) * Q.B * kRbAtoms : nullptr;
  L.grads_out = Q.grads_out ? Q.grads_out + static_cast<int64_t>(m) * kRlParams : nullptr;
  L.gamma = T.gamma, L.inv_b = Q.inv_b;
  L.A = LearnAdam{T.b1, T.omb1, T.b2, T.omb2, Q.step[m], Q.bc2s[m], T.eps};
  return L;
}
MG_HD const RLearn& rl_member(const RLearn& L, int) { return L; }

// A population of prioritized learners (mg_rainbow_learn_prioritized_many): what the sample in front of an update
// and the priority update behind it read, for all members (mg_per.h's sample kernel, templated as the learner's
// are, and its update block).
// A member's idx [B], w [B] and the loss_b its update reads are its slice of the learners' scratch; its counter
// and seed are its entry of the learners' table; its tree, alpha, beta, prio_eps and draw travel by value.
struct PerMany {
  PerTree shape;   // C, cap, logC, shared; the pointers are unused
  float* scratch;  // [members, stride]
  const LearnMember* table;
  int64_t stride, pidx, pw, lossb;  // floats: RLearnMany's stride, rl_scratch's sections
  int64_t* idx_out;                 // this update's [members, B], or NULL
  float* w_out;
  int32_t B;
  void* tree[kMaxMembers];
  double alpha[kMaxMembers], beta[kMaxMembers];
  uint64_t draw[kMaxMembers];
  float add[kMaxMembers];  // prio_eps, rounded as the lone call rounds it
};
static_assert(sizeof(PerMany) <= 2560, "the by-value kernel argument stays inside HIP's 4096 bytes");

MG_HD PerSample per_sample_member(const PerMany& Q, int m) {
  const LearnMember& T = Q.table[m];
  float* s = Q.scratch + m * Q.stride;
  PerSample P;
  P.T = per_tree_at(Q.shape, Q.tree[m]);
  P.counter = T.counter, P.beta = Q.beta[m], P.seed = T.seed, P.draw = Q.draw[m], P.B = Q.B;
  P.idx = reinterpret_cast<int64_t*>(s + Q.pidx), P.w = s + Q.pw;
  P.idx_out = Q.idx_out ? Q.idx_out + static_cast<int64_t>(m) * Q.B : nullptr;
  P.w_out = Q.w_out ? Q.w_out + static_cast<int64_t>(m) * Q.B : nullptr;
  return P;
}
MG_HD PerUpdate per_update_member(const PerMany& Q, int m) {
  const float* s = Q.scratch + m * Q.stride;
  return PerUpdate{per_tree_at(Q.shape, Q.tree[m]), Q.table[m].counter, Q.alpha[m],
                   reinterpret_cast<const int64_t*>(s + Q.pidx), s + Q.lossb, Q.add[m], 1, Q.B};
}

// per_update_kernel's block for every member: block m on member m's tree
__global__ __launch_bounds__(kPerTail) void per_update_many_kernel(const PerMany Q) {
  per_update_block(per_update_member(Q, blockIdx.x));
}

// What the two noisy backward launches read: the lone call's layers as the host built them, or member m's
// built where they are used.
struct RlHeads {
  LearnBwd G0, G1;
};
struct RlStreams {
  RLearn L;
  LearnBwd Gv, Ga;
};
MG_HD const RlHeads& rl_heads(const RlHeads& H, int) { return H; }
MG_HD const RlStreams& rl_streams(const RlStreams& S, int) { return S; }
MG_HD RlHeads rl_heads(const RLearnMany& Q, int m) {
  const RLearn L = rl_member(Q, m);
  return RlHeads{rl_bwd_layer(L, 0), rl_bwd_layer(L, 1)};
}
MG_HD RlStreams rl_streams(const RLearnMany& Q, int m) {
  const RLearn L = rl_member(Q, m);
  return RlStreams{L, rl_bwd_layer(L, 2), rl_bwd_layer(L, 3)};
}

// ---------------------------------------------------------------------------- kernels
// One body each for the lone learner (Arg = RLearn, RlHeads, RlStreams: blockIdx.y is 0 and unused) and the
// population (Arg = RLearnMany: blockIdx.y is the member).
// One block per minibatch row: host_rl_forward_row's steps, the activations in LDS, one thread per unit. The two
// forwards run side by side -- threads 0..319 the target's on s' (pass 1), 320..639 the current's on s (pass 0) --
// through the same phases; only the loss waits for the projection.
template <class Arg>
__global__ __launch_bounds__(2 * kRlThreads) void rl_forward_kernel(const Arg Q) {
  const RLearn& L = rl_member(Q, blockIdx.y);
  __shared__ float srow[kRlRow], h1[2][kRbH1], h2[2][kRbH2], hv[2][kRbHS], ha[2][kRbHS], lg[2][kRbLogits];
  __shared__ float p[2][kRbActions * kRbAtoms], q[2][kRbActions], bb[kRbAtoms], proj[kRbAtoms], dx[kRbAtoms];
  const int b = blockIdx.x;
  const int pass = threadIdx.x < kRlThreads ? 1 : 0, t = threadIdx.x - (pass ? 0 : kRlThreads);
  const float* z = L.buf + kRlOffZ;
  if (threadIdx.x < kRlRow) {
    const uint64_t live = learn_rows_live(L.cap, L.counter, 1);
    const float v = L.ring[rl_row_slot(L, live, b) * kRlRow + threadIdx.x];
    srow[threadIdx.x] = v;
    L.rows[b * kRlRow + threadIdx.x] = v;
    if (L.rows_out) L.rows_out[b * kRlRow + threadIdx.x] = v;
  }
  __syncthreads();
  const float* P = L.buf + pass * kRlParams;
  const float* eff = L.eff + pass * kRlEps;
  const float* x = srow + (pass ? kRlColS2 : 0);
  if (t < kRbH1) h1[pass][t] = rl_unit_h1(P, x, t);
  __syncthreads();
  if (t < kRbH2) h2[pass][t] = rl_unit_h2(P, h1[pass], t);
  __syncthreads();
  if (t < kRbHS)
    hv[pass][t] = learn_relu(rl_unit_noisy(eff, 0, h2[pass], t));
  else if (t < 2 * kRbHS)
    ha[pass][t - kRbHS] = learn_relu(rl_unit_noisy(eff, 2, h2[pass], t - kRbHS));
  __syncthreads();
  if (t < kRbLogits) lg[pass][t] = rl_unit_logit(eff, hv[pass], ha[pass], t);
  __syncthreads();
  // rl_softmax's steps, one thread per (action, atom), the two reductions one thread per action
  const int ha5 = t / kRbAtoms;  // the action of element t < 255
  if (t < kRbActions * kRbAtoms) p[pass][t] = rl_head_x(lg[pass], t);
  if (pass && t >= 256 && t < 256 + kRbAtoms)  // another wave than the reductions'
    bb[t - 256] = rl_b(srow[kRlColR], srow[kRlColDone], L.gamma, z[t - 256]);
  __syncthreads();
  if (t < kRbActions) q[pass][t] = rl_max51(p[pass] + t * kRbAtoms);
  __syncthreads();
  if (t < kRbActions * kRbAtoms) p[pass][t] = rb_exp(p[pass][t] - q[pass][ha5]);
  __syncthreads();
  if (t < kRbActions) q[pass][t] = rl_sum4(p[pass] + t * kRbAtoms);
  __syncthreads();
  if (t < kRbActions * kRbAtoms) {
    const float y = p[pass][t] / q[pass][ha5];
    p[pass][t] = pass ? y * z[t - ha5 * kRbAtoms] : y;
  }
  __syncthreads();
  if (pass && t < kRbActions) q[1][t] = rl_sum4(p[1] + t * kRbAtoms);
  if (!pass) {  // the current model's activations, for the backward launches
    if (t < kRbH1) L.h1[b * kRbH1 + t] = h1[0][t];
    if (t >= 64 && t < 64 + kRbH2) L.h2[b * kRbH2 + t - 64] = h2[0][t - 64];
    if (t >= 128 && t < 128 + kRbHS) L.hv[b * kRbHS + t - 128] = hv[0][t - 128];
    if (t >= 192 && t < 192 + kRbHS) L.ha[b * kRbHS + t - 192] = ha[0][t - 192];
  }
  __syncthreads();
  if (pass && t < kRbAtoms) {
    proj[t] = rl_proj_slot(t, p[1] + rl_argmax(q[1]) * kRbAtoms, bb);
    if (L.proj_out) L.proj_out[b * kRbAtoms + t] = proj[t];
  }
  __syncthreads();
  const int astar = learn_action(srow[kRlColA], kRbActions);
  if (!pass && t == 0) L.lossb[b] = rl_loss_row(p[0] + astar * kRbAtoms, proj, rl_row_scale(L, b), dx);
  __syncthreads();
  if (!pass && t < kRbLogits) L.dlog[b * kRbLogits + t] = rl_dlogit(dx, astar, t);
}

// two layers' items in one launch
template <class Arg>
__global__ __launch_bounds__(kBlock) void rl_bwd_heads_kernel(const Arg Q) {
  const RlHeads& H = rl_heads(Q, blockIdx.y);
  const LearnBwd &G0 = H.G0, &G1 = H.G1;
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const int64_t n0 = learn_bwd_items(G0);
  if (idx < n0)
    learn_bwd_at(G0, idx);
  else if (idx < n0 + learn_bwd_items(G1))
    learn_bwd_at(G1, idx - n0);
}

// the hidden streams' gradients and, behind them, the B x 64 items of rl_dh2_at
template <class Arg>
__global__ __launch_bounds__(kBlock) void rl_bwd_streams_kernel(const Arg Q) {
  const RlStreams& S = rl_streams(Q, blockIdx.y);
  const RLearn& L = S.L;
  const LearnBwd &Gv = S.Gv, &Ga = S.Ga;
  int64_t idx = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const int64_t nv = learn_bwd_items(Gv), na = learn_bwd_items(Ga);
  if (idx < nv) return learn_bwd_at(Gv, idx);
  idx -= nv;
  if (idx < na) return learn_bwd_at(Ga, idx);
  idx -= na;
  if (idx < static_cast<int64_t>(L.B) * kRbH2) rl_dh2_at(L, idx);
}
MG_HD int64_t rl_bwd_heads_items(const RlHeads& H) { return learn_bwd_items(H.G0) + learn_bwd_items(H.G1); }
MG_HD int64_t rl_bwd_streams_items(const RlStreams& S) {
  return learn_bwd_items(S.Gv) + learn_bwd_items(S.Ga) + static_cast<int64_t>(S.L.B) * kRbH2;
}

// learn_bwd_kernel (mg_learn_core.h, the DQN learner's too) for a member's plain layer WHICH (4 linear2, 5 linear1)
template <int WHICH>
__global__ __launch_bounds__(kBlock) void rl_bwd_plain_many_kernel(const RLearnMany Q) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const LearnBwd G = rl_bwd_layer(rl_member(Q, blockIdx.y), WHICH);
  if (idx < learn_bwd_items(G)) learn_bwd_at(G, idx);
}

template <class Arg>
__global__ __launch_bounds__(kBlock) void rl_adam_kernel(const Arg Q) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i <= kRlParams) rl_adam_at(rl_member(Q, blockIdx.y), i);
}

template <class Arg>
__global__ __launch_bounds__(kBlock) void rl_noise_eff_kernel(const Arg Q, int redraw) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < 2 * kRlEps) rl_noise_eff_at(rl_member(Q, blockIdx.y), i, redraw != 0);
}

// update_target (:551-552) for every member whose bit is set: target := current, the parameters and the noise
// block.
__global__ __launch_bounds__(kBlock) void rl_sync_many_kernel(float* learners, uint64_t mask) {
  const int m = blockIdx.y, i = blockIdx.x * kBlock + threadIdx.x;
  if (!((mask >> m) & 1)) return;
  float* buf = learners + static_cast<int64_t>(m) * kRlLearner;
  if (i < kRlParams)
    buf[kRlParams + i] = buf[i];
  else if (i < kRlParams + kRlEps)
    buf[kRlOffEps + kRlEps + (i - kRlParams)] = buf[kRlOffEps + (i - kRlParams)];
}

// ---------------------------------------------------------------------------- host side of a call
// What mg_rainbow_replay_store and the prioritized stores refuse (n == 0 or num_steps == 0 is a no-op the caller
// returns from before the required arrays are looked at).
// The lone stores are the member store's list of one ring: both fill an RlStoreCall and one walk checks it. The
// member call (`many`) adds the checks of its lists, which come before anything else of a member is looked at.
struct RlStoreCall {  // in the order of mg_rainbow_replay_store_many's arguments
  float* const* rows;  // `members` rings and their counters (a lone call: the addresses of its two arguments)
  uint64_t* const* counter;
  int32_t members;
  int64_t capacity;
  const mg_transitions* tr;
  int64_t n;  // envs of one member
  int32_t T;
};

int check_rainbow_store(const char* what, const RlStoreCall& C, bool many = false) {
  const auto bad = [what](const char* fmt) { return fail(hipErrorInvalidValue, fmt, what); };
  if (many && !members_ok(C.members)) return bad("%s: need 1 <= members <= 64");
  if (!C.rows || !C.counter || !C.tr || (!many && (!C.rows[0] || !C.counter[0]))) return bad("%s: NULL pointer");
  for (int m = 0; many && m < C.members; ++m) {
    if (!C.rows[m] || !C.counter[m]) return bad("%s: NULL pointer (a member's rows or counter)");
    if (misaligned(C.rows[m], 7) || misaligned(C.counter[m], 7))
      return bad("%s: every member's rows and counter must be 8-byte aligned");
    for (int k = 0; k < m; ++k)
      if (C.rows[k] == C.rows[m] || C.counter[k] == C.counter[m])
        return bad("%s: a ring is listed twice (two members' appends to one ring have no defined order)");
  }
  if (C.capacity < 1 || C.capacity > (int64_t{1} << 32)) return bad("%s: need 1 <= capacity <= 2^32");
  if (C.n < 0 || C.T < 0) return bad(many ? "%s: n_member < 0 or num_steps < 0" : "%s: n < 0 or num_steps < 0");
  const mg_transitions& X = *C.tr;
  if (X.goal || X.next_goal || X.reward || X.meta_goal)
    return bad("%s: goal, next_goal, reward and meta_goal must be NULL (Rainbow rows have none)");
  if (C.n == 0 || C.T == 0) return 0;
  if (!X.obs_first || !X.obs || !(X.a1 || X.flags) || !X.rew)
    return bad("%s: obs_first, obs, a1 (or flags) and rew are required");
  if ((!many && (misaligned(C.rows[0], 7) || misaligned(C.counter[0], 7))) || misaligned(X.obs_first, 3) ||
      misaligned(X.obs, 3) || misaligned(X.final_obs, 3) || misaligned(X.rew, 3))
    return bad(many ? "%s: the float buffers must be 4-byte aligned"
                    : "%s: rows and counter must be 8-byte, the float buffers 4-byte aligned");
  if (C.n > (static_cast<int64_t>(0x7fffffff) * kBlock) / C.T)
    return bad(many ? "%s: n_member * num_steps exceeds the grid limit" : "%s: n * num_steps exceeds the grid limit");
  return 0;
}

// A store after its checks, on the stream or (host) as loops: the rows, the tree's part if there is a tree, then
// the counter moves.
void rainbow_store(float* rows, uint64_t* counter, int64_t capacity, const mg_transitions* tr, int64_t n,
                   int32_t num_steps, void* tree, double alpha, bool host, hipStream_t st) {
  RlStore R{};
  R.X = *tr;
  R.n = n;
  R.total = n * num_steps;
  if (host) {
    for (int64_t i = 0; i < R.total; ++i) rl_store_at(R, counter, rows, capacity, i, n, 0);
    if (tree) host_per_store_tree(per_tree(tree, capacity), counter, R.total, alpha);
    *counter += static_cast<uint64_t>(R.total);
    return;
  }
  hipLaunchKernelGGL(rl_store_kernel, dim3(grid_blocks(R.total)), dim3(kBlock), 0, st, R, counter, rows, capacity);
  if (tree) launch_per_store_tree(per_tree(tree, capacity), counter, R.total, alpha, st);
  hipLaunchKernelGGL(counter_add_kernel, dim3(1), dim3(1), 0, st, counter, static_cast<uint64_t>(R.total));
}

// What mg_per_store_many refuses of its trees, behind check_rainbow_store's walk of the rings.
int check_per_store_many(const char* what, const RlStoreCall& C, void* const* trees, size_t tree_bytes,
                         const double* alpha) {
  if (!trees || !alpha) return fail(hipErrorInvalidValue, "%s: NULL pointer", what);
  for (int m = 0; m < C.members; ++m)
    if (!trees[m]) return fail_member(what, m, "NULL pointer (tree)");
  for (int m = 0; m < C.members; ++m)
    if (misaligned(trees[m], 15)) return fail_member(what, m, "the tree buffer must be 16-byte aligned");
  if (tree_bytes < static_cast<size_t>(per_doubles(C.capacity)) * sizeof(double))
    return fail(hipErrorInvalidValue, "%s: tree buffer smaller than mg_per_bytes(capacity)", what);
  for (int m = 0; m < C.members; ++m)
    if (!(alpha[m] > 0.0)) return fail_member(what, m, "need alpha > 0");
  for (int m = 0; m < C.members; ++m)
    for (int k = 0; k < m; ++k)
      if (trees[k] == trees[m])
        return fail_member(what, m,
                           "its tree is another member's (two members' stores to one tree have no defined order)");
  return 0;
}

// The member store after its checks: every member's rows (the member in the grid, or on the host member by member),
// with trees the trees' part (launch_per_store_tree's launches, which read the counters before they move), then
// every counter moves by T n_member.
void rainbow_store_many(const RlStoreCall& C, bool host, hipStream_t st, void* const* trees = nullptr,
                        const double* alpha = nullptr) {
  RlStoreMany A{};
  A.R.X = *C.tr;
  A.R.n = C.n;
  A.R.total = C.n * C.T;
  A.N = C.n * C.members;
  A.cap = C.capacity;
  A.members = C.members;
  std::copy(C.rows, C.rows + C.members, A.rows);
  std::copy(C.counter, C.counter + C.members, A.counter);
  if (host) {
    for (int m = 0; m < C.members; ++m) {
      for (int64_t i = 0; i < A.R.total; ++i) rl_store_at(A.R, A.counter[m], A.rows[m], A.cap, i, A.N, m * C.n);
      if (trees) host_per_store_tree(per_tree(trees[m], A.cap), A.counter[m], A.R.total, alpha[m]);
      *A.counter[m] += static_cast<uint64_t>(A.R.total);
    }
    return;
  }
  hipLaunchKernelGGL(rl_store_many_kernel, dim3(grid_blocks(A.R.total), static_cast<unsigned>(C.members)),
                     dim3(kBlock), 0, st, A);
  if (trees) {
    PerStoreMany P{};
    P.shape = per_tree(trees[0], A.cap);
    P.total = A.R.total;
    std::copy(trees, trees + C.members, P.tree);
    std::copy(A.counter, A.counter + C.members, P.counter);
    std::copy(alpha, alpha + C.members, P.alpha);
    launch_per_store_tree_many(P, C.members, st);
  }
  hipLaunchKernelGGL(rl_counter_add_many_kernel, dim3(1), dim3(kMaxMembers), 0, st, A);
}

// One call of mg_rainbow_learn, mg_rainbow_learn_prioritized or a host twin: the arguments as the entry point
// took them (packed_out NULL on the host; without `prioritized` the fields behind it stay zero), then what
// make_rainbow_learn derives from them.
struct RLearnCall {
  float* learner;
  const float* rows;
  const uint64_t* counter;
  int64_t capacity;
  int32_t batch, num_updates;
  uint64_t first_update, seed, first_draw;
  const mg_dqn_hyper* hyper;
  const float* noise;
  float *loss_out, *rows_out, *proj_out, *grads_out;
  void *packed_out, *scratch;
  size_t scratch_bytes;
  bool prioritized;
  void* tree;
  size_t tree_bytes;
  double alpha, beta, prio_eps;
  int64_t* idx_out;
  float* weight_out;
  RLearn L;
  PerSample P;  // with `prioritized`: the sample in front of the seven launches
  PerUpdate U;  // and the priorities behind them
};

// What the four learners refuse, before anything is read or launched.
int check_rainbow_learn(const char* what, const RLearnCall& C) {
  if (!C.learner || !C.rows || !C.counter || !C.hyper || !C.scratch)
    return fail(hipErrorInvalidValue, "%s: NULL pointer", what);
  if (int e = check_learn_sizes(what, C.batch, C.capacity, C.num_updates)) return e;
  if (C.num_updates > 0 && !C.noise)
    return fail(hipErrorInvalidValue, "%s: noise is NULL (num_updates x 2 x 1124 factors)", what);
  if (int e = check_adam_betas(what, C.hyper)) return e;
  if (misaligned(C.learner, 15) || misaligned(C.scratch, 15) || misaligned(C.packed_out, 15) ||
      misaligned(C.rows, 7) || misaligned(C.counter, 7) || misaligned(C.noise, 3) || misaligned(C.loss_out, 3) ||
      misaligned(C.rows_out, 3) || misaligned(C.proj_out, 3) || misaligned(C.grads_out, 3))
    return fail(hipErrorInvalidValue,
                "%s: learner, scratch and packed_out must be 16-byte, rows and counter 8-byte, noise and the "
                "optional outputs 4-byte aligned", what);
  if (C.scratch_bytes < static_cast<size_t>(rl_scratch(C.batch, false).total) * sizeof(float))
    return fail(hipErrorInvalidValue, "%s: scratch smaller than mg_rainbow_learn_scratch_bytes(batch)", what);
  if (!C.prioritized) return 0;
  if (int e = check_per_tree(what, C.tree, C.tree_bytes, C.capacity)) return e;
  if (int e = check_per_alpha(what, C.alpha)) return e;
  if (int e = check_per_beta(what, C.beta)) return e;
  if (!(C.prio_eps >= 0.0)) return fail(hipErrorInvalidValue, "%s: need prio_eps >= 0", what);
  if (misaligned(C.idx_out, 7) || misaligned(C.weight_out, 3))
    return fail(hipErrorInvalidValue, "%s: idx_out must be 8-byte, weight_out 4-byte aligned", what);
  if (C.scratch_bytes < static_cast<size_t>(rl_scratch(C.batch, true).total) * sizeof(float))
    return fail(hipErrorInvalidValue, "%s: scratch smaller than mg_rainbow_learn_prioritized_scratch_bytes(batch)", what);
  return 0;
}

// The fields of L, P and U that do not change from one update of a call to the next.
void make_rainbow_learn(RLearnCall& C) {
  const RlScratch S = rl_scratch(C.batch, C.prioritized);
  float* s = static_cast<float*>(C.scratch);
  RLearn& L = C.L;
  L.buf = C.learner;
  L.ring = C.rows, L.counter = C.counter, L.cap = C.capacity, L.seed = C.seed, L.B = C.batch;
  rl_set_scratch(L, s, S);
  L.gamma = static_cast<float>(C.hyper->gamma);
  L.inv_b = static_cast<float>(1.0 / C.batch);
  if (!C.prioritized) return;
  C.P.T = C.U.T = per_tree(C.tree, C.capacity);
  C.P.counter = C.U.counter = C.counter;
  C.P.beta = C.beta, C.P.seed = C.seed, C.P.B = C.U.B = C.batch;
  C.P.idx = reinterpret_cast<int64_t*>(s + S.pidx), C.P.w = s + S.pw;
  C.U.alpha = C.alpha, C.U.idx = C.P.idx, C.U.priority = L.lossb;
  C.U.add = static_cast<float>(C.prio_eps), C.U.has_add = 1;
  L.pidx = C.P.idx, L.pw = C.P.w;
}

// Update number u of a call: its draw, factors, optional outputs and Adam's step t + 1 (t = first_update + u).
void rainbow_learn_set_update(RLearnCall& C, int32_t u) {
  RLearn& L = C.L;
  const int64_t ub = static_cast<int64_t>(u) * L.B;
  L.A = learn_adam_scalars(C.hyper, C.first_update + static_cast<uint64_t>(u));
  L.draw = C.P.draw = C.first_draw + static_cast<uint64_t>(u);
  L.noise = C.noise + static_cast<int64_t>(u) * 2 * kRlFactors;
  L.loss_out = C.loss_out ? C.loss_out + u : nullptr;
  L.rows_out = C.rows_out ? C.rows_out + ub * kRlRow : nullptr;
  L.proj_out = C.proj_out ? C.proj_out + ub * kRbAtoms : nullptr;
  L.grads_out = C.grads_out ? C.grads_out + static_cast<int64_t>(u) * kRlParams : nullptr;
  C.P.idx_out = C.idx_out ? C.idx_out + ub : nullptr;
  C.P.w_out = C.weight_out ? C.weight_out + ub : nullptr;
}

// One update on the device, after rainbow_learn_set_update: the launch order that host_rainbow_learn_update
// below restates loop for loop. With a tree the sample goes in front and its rows and weights are what the
// seven launches read; the priorities loss_b + prio_eps go back into the tree behind them. The last of the
// seven leaves the next update's effective weights.
void launch_rainbow_learn_update(const RLearnCall& C, hipStream_t st) {
  const RLearn& L = C.L;
  if (C.prioritized) hipLaunchKernelGGL(per_sample_kernel<PerSample>, dim3(grid_blocks(L.B)), dim3(kBlock), 0, st, C.P);
  hipLaunchKernelGGL(rl_forward_kernel<RLearn>, dim3(L.B), dim3(2 * kRlThreads), 0, st, L);
  const RlHeads H{rl_bwd_layer(L, 0), rl_bwd_layer(L, 1)};
  const RlStreams S{L, rl_bwd_layer(L, 2), rl_bwd_layer(L, 3)};
  hipLaunchKernelGGL(rl_bwd_heads_kernel<RlHeads>, dim3(grid_blocks(rl_bwd_heads_items(H))), dim3(kBlock), 0, st, H);
  hipLaunchKernelGGL(rl_bwd_streams_kernel<RlStreams>, dim3(grid_blocks(rl_bwd_streams_items(S))), dim3(kBlock), 0, st,
                     S);
  for (int which = 4; which < 6; ++which) {
    const LearnBwd G = rl_bwd_layer(L, which);
    hipLaunchKernelGGL(learn_bwd_kernel, dim3(grid_blocks(learn_bwd_items(G))), dim3(kBlock), 0, st, G);
  }
  hipLaunchKernelGGL(rl_adam_kernel<RLearn>, dim3(grid_blocks(kRlParams + 1)), dim3(kBlock), 0, st, L);
  hipLaunchKernelGGL(rl_noise_eff_kernel<RLearn>, dim3(grid_blocks(2 * kRlEps)), dim3(kBlock), 0, st, L, 1);
  if (C.prioritized) hipLaunchKernelGGL(per_update_kernel, dim3(1), dim3(kPerTail), 0, st, C.U);
}

// One update on the host: the kernels' per-item functions in the kernels' order. First the seven launches'
// loops on one learner (a member's too), then the update around them.
void host_rl_update(const RLearn& L) {
  const uint64_t live = learn_rows_live(L.cap, L.counter, 1);
  for (int b = 0; b < L.B; ++b) host_rl_forward_row(L, live, b);
  for (int which = 0; which < 6; ++which) {
    const LearnBwd G = rl_bwd_layer(L, which);
    for (int64_t i = 0; i < learn_bwd_items(G); ++i) learn_bwd_at(G, i);
    if (which == 3)
      for (int64_t i = 0; i < static_cast<int64_t>(L.B) * kRbH2; ++i) rl_dh2_at(L, i);
  }
  for (int i = 0; i <= kRlParams; ++i) rl_adam_at(L, i);
  for (int i = 0; i < 2 * kRlEps; ++i) rl_noise_eff_at(L, i, true);
}
void host_rainbow_learn_update(const RLearnCall& C) {
  if (C.prioritized)
    for (int b = 0; b < C.L.B; ++b) per_sample_at(C.P, b);
  host_rl_update(C.L);
  if (C.prioritized) host_per_update(C.U);
}

// What rainbow_pack_kernel packs for acting: the current model's plain layers, effective weights e = L.eff, support.
MG_HD RbTensors rainbow_learn_tensors(const float* learner, const float* e) {
  const RlNoisy V1 = rl_noisy(0), V2 = rl_noisy(1), A1 = rl_noisy(2), A2 = rl_noisy(3);
  return RbTensors{learner + kRlW1, learner + kRlB1, learner + kRlW2, learner + kRlB2,
                   e + V1.e, e + V1.e + V1.out * kRbHS, e + V2.e, e + V2.e + V2.out * kRbHS,
                   e + A1.e, e + A1.e + A1.out * kRbHS, e + A2.e, e + A2.e + A2.out * kRbHS, learner + kRlOffZ};
}

// ---------------------------------------------------------------------------- the drivers of a call
// The device learners after their check: the effective weights of the stored noise (every update's last of the
// seven launches leaves the next one's), the updates back to back on the stream, then the acting kernels' layout
// of the current model's effective weights.
int rainbow_learn_device(const char* what, RLearnCall& C, hipStream_t st) {
  make_rainbow_learn(C);
  hipLaunchKernelGGL(rl_noise_eff_kernel<RLearn>, dim3(grid_blocks(2 * kRlEps)), dim3(kBlock), 0, st, C.L, 0);
  for (int32_t u = 0; u < C.num_updates; ++u) {
    rainbow_learn_set_update(C, u);
    launch_rainbow_learn_update(C, st);
  }
  if (C.packed_out)
    hipLaunchKernelGGL(rainbow_pack_kernel, dim3(grid_blocks(kRbNetBytes / 4)), dim3(kBlock), 0, st,
                       rainbow_learn_tensors(C.learner, C.L.eff), static_cast<uint8_t*>(C.packed_out));
  return finish_launch(what);
}

// The host learners after their check.
int rainbow_learn_host(RLearnCall& C) {
  make_rainbow_learn(C);
  for (int i = 0; i < 2 * kRlEps; ++i) rl_noise_eff_at(C.L, i, false);
  for (int32_t u = 0; u < C.num_updates; ++u) {
    rainbow_learn_set_update(C, u);
    host_rainbow_learn_update(C);
  }
  g_err[0] = '\0';
  return 0;
}

// ============================================================================ a population of learners
// rainbow_pack_kernel with blockIdx.y the member: its current model's plain layers, effective weights and support
// into its row of the packed buffer.
__global__ void rainbow_pack_many_kernel(const float* learners, const float* scratch, int64_t stride, int64_t eff,
                                         uint8_t* packed, int64_t packed_stride) {
  const int64_t m = blockIdx.y;
  rainbow_pack_at(blockIdx.x * blockDim.x + threadIdx.x,
                  rainbow_learn_tensors(learners + m * kRlLearner, scratch + m * stride + eff),
                  packed + m * packed_stride);
}

// What the population's entry points refuse of the member list, in check_rainbow_learn's three steps: the
// pointers, Adam's betas, the alignment (hyper.target_period is not read).
int check_rainbow_members_null(const char* what, const mg_dqn_member* member, int32_t members) {
  for (int m = 0; m < members; ++m)
    if (!member[m].rows || !member[m].counter) return fail_member(what, m, "NULL pointer (rows or counter)");
  return 0;
}
int check_rainbow_members_betas(const char* what, const mg_dqn_member* member, int32_t members) {
  for (int m = 0; m < members; ++m) {
    const mg_dqn_hyper& H = member[m].hyper;
    if (!(H.beta1 >= 0.0 && H.beta1 < 1.0 && H.beta2 >= 0.0 && H.beta2 < 1.0))
      return fail_member(what, m, "need 0 <= beta1 < 1 and 0 <= beta2 < 1");
  }
  return 0;
}
int check_rainbow_members_aligned(const char* what, const mg_dqn_member* member, int32_t members) {
  for (int m = 0; m < members; ++m)
    if (misaligned(member[m].rows, 7) || misaligned(member[m].counter, 7))
      return fail_member(what, m, "rows and counter must be 8-byte aligned");
  return 0;
}

int check_rainbow_member_table(const char* what, const void* table, size_t table_bytes, int32_t members) {
  if (!table) return fail(hipErrorInvalidValue, "%s: table is NULL", what);
  if (misaligned(table, 15)) return fail(hipErrorInvalidValue, "%s: table must be 16-byte aligned", what);
  if (table_bytes < sizeof(LearnMember) * static_cast<size_t>(members))
    return fail(hipErrorInvalidValue, "%s: table smaller than mg_rainbow_learn_many_table_bytes(members)", what);
  return 0;
}

// One call of mg_rainbow_learn_many or its host twin, as the entry point took it (table and packed_out NULL on
// the host).
struct RLearnManyCall {
  float* learners;
  const void* table;
  size_t table_bytes;
  mg_dqn_member* member;
  int32_t members;
  int64_t capacity;
  int32_t batch, num_updates;
  const float* noise;
  float *loss_out, *rows_out, *proj_out, *grads_out;
  void* packed_out;
  size_t packed_stride;
  void* scratch;
  size_t scratch_bytes;
  bool host;
  // mg_rainbow_learn_prioritized_many and its twin (else zero): every member's tree and exponents, the optional
  // outputs [U][M][B]
  bool prioritized;
  const mg_per_member* per;
  size_t tree_bytes;
  int64_t* idx_out;
  float* weight_out;
};

// What the prioritized population's calls refuse behind check_rainbow_learn_many's checks: check_rainbow_learn's
// prioritized part in its order, a member's named, then the replays two members share.
int check_rainbow_learn_many_per(const char* what, const RLearnManyCall& C) {
  if (!C.per) return fail(hipErrorInvalidValue, "%s: NULL pointer", what);
  for (int m = 0; m < C.members; ++m)
    if (!C.per[m].tree) return fail_member(what, m, "NULL pointer (tree)");
  for (int m = 0; m < C.members; ++m)
    if (misaligned(C.per[m].tree, 15)) return fail_member(what, m, "the tree buffer must be 16-byte aligned");
  if (C.tree_bytes < static_cast<size_t>(per_doubles(C.capacity)) * sizeof(double))
    return fail(hipErrorInvalidValue, "%s: tree buffer smaller than mg_per_bytes(capacity)", what);
  for (int m = 0; m < C.members; ++m) {
    if (!(C.per[m].alpha > 0.0)) return fail_member(what, m, "need alpha > 0");
    if (!(C.per[m].beta > 0.0)) return fail_member(what, m, "need beta > 0");
    if (!(C.per[m].prio_eps >= 0.0)) return fail_member(what, m, "need prio_eps >= 0");
  }
  if (misaligned(C.idx_out, 7) || misaligned(C.weight_out, 3))
    return fail(hipErrorInvalidValue, "%s: idx_out must be 8-byte, weight_out 4-byte aligned", what);
  const size_t one = static_cast<size_t>(rl_scratch(C.batch, true).total) * sizeof(float);
  if (C.scratch_bytes < one * static_cast<size_t>(C.members))
    return fail(hipErrorInvalidValue,
                "%s: scratch smaller than members * mg_rainbow_learn_prioritized_scratch_bytes(batch)", what);
  for (int m = 0; m < C.members; ++m)
    for (int k = 0; k < m; ++k)
      if (C.per[k].tree == C.per[m].tree || C.member[k].rows == C.member[m].rows)
        return fail_member(what, m, "its tree or rows are another member's (learning writes the tree: a shared "
                                    "replay has no defined order)");
  return 0;
}

// What the two refuse, before anything is read or launched: check_rainbow_learn's checks in its order, the
// members' behind the call's at each step.
int check_rainbow_learn_many(const char* what, const RLearnManyCall& C) {
  if (!members_ok(C.members)) return fail(hipErrorInvalidValue, "%s: need 1 <= members <= 64", what);
  if (!C.learners || !C.member || !C.scratch) return fail(hipErrorInvalidValue, "%s: NULL pointer", what);
  if (int e = check_rainbow_members_null(what, C.member, C.members)) return e;
  if (int e = check_learn_sizes(what, C.batch, C.capacity, C.num_updates)) return e;
  if (C.num_updates > 0 && !C.noise)
    return fail(hipErrorInvalidValue, "%s: noise is NULL (num_updates x members x 2 x 1124 factors)", what);
  if (int e = check_rainbow_members_betas(what, C.member, C.members)) return e;
  if (misaligned(C.learners, 15) || misaligned(C.scratch, 15) || misaligned(C.packed_out, 15) ||
      misaligned(C.noise, 3) || misaligned(C.loss_out, 3) || misaligned(C.rows_out, 3) || misaligned(C.proj_out, 3) ||
      misaligned(C.grads_out, 3) || (C.packed_out && C.packed_stride % 16 != 0))
    return fail(hipErrorInvalidValue,
                "%s: learners, scratch and packed_out must be 16-byte, noise and the optional outputs 4-byte "
                "aligned, packed_stride a multiple of 16", what);
  if (int e = check_rainbow_members_aligned(what, C.member, C.members)) return e;
  if (C.packed_out && C.packed_stride < static_cast<size_t>(kRbNetBytes))
    return fail(hipErrorInvalidValue, "%s: packed_stride smaller than mg_rainbow_packed_bytes()", what);
  const size_t one = static_cast<size_t>(rl_scratch(C.batch, false).total) * sizeof(float);
  if (C.scratch_bytes < one * static_cast<size_t>(C.members))
    return fail(hipErrorInvalidValue, "%s: scratch smaller than members * mg_rainbow_learn_scratch_bytes(batch)", what);
  if (!C.host)
    if (int e = check_rainbow_member_table(what, C.table, C.table_bytes, C.members)) return e;
  return C.prioritized ? check_rainbow_learn_many_per(what, C) : 0;
}

// The fields of RLearnMany that do not change from one update of a call to the next.
RLearnMany make_rainbow_learn_many(const RLearnManyCall& C, const LearnMember* table) {
  RLearnMany Q{};
  Q.learners = C.learners, Q.scratch = static_cast<float*>(C.scratch), Q.table = table;
  Q.stride = rl_scratch(C.batch, C.prioritized).total;
  Q.cap = C.capacity, Q.B = C.batch, Q.members = C.members;
  Q.inv_b = static_cast<float>(1.0 / C.batch);
  Q.prioritized = C.prioritized ? 1 : 0;
  return Q;
}

// The same of PerMany, for a prioritized call: make_rainbow_learn's P and U for every member.
PerMany make_per_many(const RLearnManyCall& C, const RLearnMany& Q) {
  const RlScratch S = rl_scratch(C.batch, true);
  PerMany P{};
  P.shape = per_tree(C.per[0].tree, C.capacity);
  P.scratch = Q.scratch, P.table = Q.table, P.stride = Q.stride;
  P.pidx = S.pidx, P.pw = S.pw, P.lossb = S.lossb, P.B = C.batch;
  for (int m = 0; m < C.members; ++m) {
    P.tree[m] = C.per[m].tree, P.alpha[m] = C.per[m].alpha, P.beta[m] = C.per[m].beta;
    P.add[m] = static_cast<float>(C.per[m].prio_eps);
  }
  return P;
}

// Update number u of a prioritized call: the members' draws as RLearnMany carries them, the update's rows of
// idx_out and weight_out.
void per_many_set_update(PerMany& P, const RLearnManyCall& C, const RLearnMany& Q, int32_t u) {
  std::copy(Q.draw, Q.draw + Q.members, P.draw);
  const int64_t umb = static_cast<int64_t>(u) * Q.members * Q.B;
  P.idx_out = C.idx_out ? C.idx_out + umb : nullptr;
  P.w_out = C.weight_out ? C.weight_out + umb : nullptr;
}

// Update number u of a call: every member's draw and Adam's step t + 1 (t = its first_update + u) from the
// host's doubles, and the update's rows of the noise and the outputs.
void rainbow_learn_many_set_update(RLearnMany& Q, const RLearnManyCall& C, int32_t u) {
  for (int m = 0; m < Q.members; ++m) {
    const LearnAdam A = learn_adam_scalars(&C.member[m].hyper, C.member[m].first_update + static_cast<uint64_t>(u));
    Q.step[m] = A.step, Q.bc2s[m] = A.bc2s;
    Q.draw[m] = C.member[m].first_draw + static_cast<uint64_t>(u);
  }
  const int64_t um = static_cast<int64_t>(u) * Q.members;
  Q.noise = C.noise + um * 2 * kRlFactors;
  Q.loss_out = C.loss_out ? C.loss_out + um : nullptr;
  Q.rows_out = C.rows_out ? C.rows_out + um * Q.B * kRlRow : nullptr;
  Q.proj_out = C.proj_out ? C.proj_out + um * Q.B * kRbAtoms : nullptr;
  Q.grads_out = C.grads_out ? C.grads_out + um * kRlParams : nullptr;
}

// One update of all members on the device: launch_rainbow_learn_update's seven launches, the member in the
// grid's y. The grids depend on the batch size alone.
void launch_rainbow_learn_many_update(const RLearnMany& Q, hipStream_t st) {
  const unsigned M = static_cast<unsigned>(Q.members);
  RLearn shape{};
  shape.B = Q.B;
  rl_set_scratch(shape, Q.scratch, rl_scratch(Q.B, false));
  const RlHeads H{rl_bwd_layer(shape, 0), rl_bwd_layer(shape, 1)};
  const RlStreams S{shape, rl_bwd_layer(shape, 2), rl_bwd_layer(shape, 3)};
  const auto plain = [&](int which) { return dim3(grid_blocks(learn_bwd_items(rl_bwd_layer(shape, which))), M); };
  hipLaunchKernelGGL(rl_forward_kernel<RLearnMany>, dim3(Q.B, M), dim3(2 * kRlThreads), 0, st, Q);
  hipLaunchKernelGGL(rl_bwd_heads_kernel<RLearnMany>, dim3(grid_blocks(rl_bwd_heads_items(H)), M), dim3(kBlock), 0, st,
                     Q);
  hipLaunchKernelGGL(rl_bwd_streams_kernel<RLearnMany>, dim3(grid_blocks(rl_bwd_streams_items(S)), M), dim3(kBlock), 0,
                     st, Q);
  hipLaunchKernelGGL(rl_bwd_plain_many_kernel<4>, plain(4), dim3(kBlock), 0, st, Q);
  hipLaunchKernelGGL(rl_bwd_plain_many_kernel<5>, plain(5), dim3(kBlock), 0, st, Q);
  hipLaunchKernelGGL(rl_adam_kernel<RLearnMany>, dim3(grid_blocks(kRlParams + 1), M), dim3(kBlock), 0, st, Q);
  hipLaunchKernelGGL(rl_noise_eff_kernel<RLearnMany>, dim3(grid_blocks(2 * kRlEps), M), dim3(kBlock), 0, st, Q, 1);
}

// mg_rainbow_learn_many or mg_rainbow_learn_prioritized_many after its check: rainbow_learn_device's order for all
// members at once -- the effective weights of the stored noise, the updates, the pack -- so num_updates == 0
// still packs.
int rainbow_learn_many_device(const char* what, const RLearnManyCall& C, hipStream_t st) {
  RLearnMany Q = make_rainbow_learn_many(C, static_cast<const LearnMember*>(C.table));
  const unsigned M = static_cast<unsigned>(Q.members);
  hipLaunchKernelGGL(rl_noise_eff_kernel<RLearnMany>, dim3(grid_blocks(2 * kRlEps), M), dim3(kBlock), 0, st, Q, 0);
  PerMany P{};
  if (C.prioritized) P = make_per_many(C, Q);
  for (int32_t u = 0; u < C.num_updates; ++u) {
    rainbow_learn_many_set_update(Q, C, u);
    if (C.prioritized) {  // launch_rainbow_learn_update's nine: the members' samples in front, their priorities behind
      per_many_set_update(P, C, Q, u);
      hipLaunchKernelGGL(per_sample_kernel<PerMany>, dim3(grid_blocks(Q.B), M), dim3(kBlock), 0, st, P);
    }
    launch_rainbow_learn_many_update(Q, st);
    if (C.prioritized) hipLaunchKernelGGL(per_update_many_kernel, dim3(M), dim3(kPerTail), 0, st, P);
  }
  if (C.packed_out)
    hipLaunchKernelGGL(rainbow_pack_many_kernel, dim3(grid_blocks(kRbNetBytes / 4), M), dim3(kBlock), 0, st, Q.learners,
                       Q.scratch, Q.stride, rl_scratch(Q.B, false).eff, static_cast<uint8_t*>(C.packed_out),
                       static_cast<int64_t>(C.packed_stride));
  if (int e = finish_launch(what)) return e;
  learn_advance(C.member, C.members, C.num_updates);
  return 0;
}

// mg_host_rainbow_learn_many or mg_host_rainbow_learn_prioritized_many after its check: host_rl_update member by
// member, each on the RLearn the kernels rebase, from a table on the stack.
int rainbow_learn_many_host(const RLearnManyCall& C) {
  LearnMember table[kMaxMembers];
  for (int m = 0; m < C.members; ++m) table[m] = learn_member_entry(C.member[m]);
  RLearnMany Q = make_rainbow_learn_many(C, table);
  for (int m = 0; m < Q.members; ++m) {
    const RLearn L = rl_member(Q, m);
    for (int i = 0; i < 2 * kRlEps; ++i) rl_noise_eff_at(L, i, false);
  }
  PerMany P{};
  if (C.prioritized) P = make_per_many(C, Q);
  for (int32_t u = 0; u < C.num_updates; ++u) {
    rainbow_learn_many_set_update(Q, C, u);
    if (C.prioritized) per_many_set_update(P, C, Q, u);
    for (int m = 0; m < Q.members; ++m) {  // host_rainbow_learn_update, member by member
      if (C.prioritized) {
        const PerSample S = per_sample_member(P, m);
        for (int b = 0; b < Q.B; ++b) per_sample_at(S, b);
      }
      host_rl_update(rl_member(Q, m));
      if (C.prioritized) host_per_update(per_update_member(P, m));
    }
  }
  learn_advance(C.member, C.members, C.num_updates);
  g_err[0] = '\0';
  return 0;
}

// mg_rainbow_sync_target_many's refusals.
int check_rainbow_sync_many(const char* what, const float* learners, int32_t members, uint64_t mask) {
  if (!members_ok(members)) return fail(hipErrorInvalidValue, "%s: need 1 <= members <= 64", what);
  if (!learners) return fail(hipErrorInvalidValue, "%s: NULL pointer", what);
  if (misaligned(learners, 15)) return fail(hipErrorInvalidValue, "%s: learners must be 16-byte aligned", what);
  if (members < kMaxMembers && (mask >> members) != 0)
    return fail(hipErrorInvalidValue, "%s: mask has a bit at or above members", what);
  return 0;
}

}  // namespace

