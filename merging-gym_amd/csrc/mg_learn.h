// mg_learn.h -- DQN.learn on the device: the minibatch update (Double-DQN target, MSE, Adam) and
// the target copy, with the per-element functions the host twin (mg_host_dqn_learn) runs too.
// A part of the one translation unit merging_hip.hip (see its head comment).
#pragma once

#include "mg_common.h"
#include "mg_env.h"
#include "mg_launch.h"
#include "mg_learn_core.h"
#include "mg_qnet.h"

namespace {

// ============================================================================ DQN.learn
// scripts/main.py:122-157 (DQN.learn), hdqn.py:186-221 (HDQN.learn), :104-139 (Goal_DQN.learn): the
// same code on Net(in, out) with hidden widths 200 / 100 (main.py:30-47). All arithmetic is fp32 in
// the fixed order include/merging_hip.h documents at mg_dqn_learn: every dot product a sequential
// fmaf chain, no float atomics, nothing that depends on the grid (the shared primitives are
// mg_learn_core.h's). One update is seven launches, in launch_learn_update's order:
//   learn_l1_kernel    minibatch rows (the draw of mg_replay_sample) -> scratch, layer 1 of the
//                      three passes: eval(s), eval(s'), target(s')
//   learn_l2_kernel    layer 2 of the three passes, W2 and the inputs tiled through LDS
//   learn_l3_kernel    layer 3, the Double-DQN target, d = q_eval[a] - t, dq
//   learn_bwd_kernel   x3: the weight / bias gradients and the input gradient of layers 3, 2, 1
//                      (the layer-3 launch also sums the loss)
//   learn_adam_kernel  Adam over all parameters
// and learn_copy_kernel before it when the target net is due (main.py:125-127).
constexpr int kLH1 = 200;  // main.py:34
constexpr int kLH2 = 100;  // main.py:36
constexpr int kLTileJ = 32;  // learn_l2_kernel: units per block
constexpr int kLTileB = 8;   //                  rows per block
constexpr int kLRows3 = 8;   // learn_l3_kernel: rows per block (32 slots each: 3 passes x out <= 24 used)

// Offsets (floats) of torch's parameter order inside one block of the learner buffer.
struct LearnLayout {
  int w1, b1, w2, b2, w3, b3, total;
};

MG_HD LearnLayout learn_layout(int in, int out) {
  LearnLayout L;
  L.w1 = 0;
  L.b1 = kLH1 * in;
  L.w2 = L.b1 + kLH1;
  L.b2 = L.w2 + kLH2 * kLH1;
  L.w3 = L.b2 + kLH2;
  L.b3 = L.w3 + out * kLH2;
  L.total = L.b3 + out;
  return L;
}

// The scratch buffer's sections (floats), each a multiple of four floats.
struct LearnScratch {
  int64_t rows, h1, h2, d, dq, dh2, dh1, g, total;
};

MG_HD LearnScratch learn_scratch(int64_t B, int in, int out) {
  LearnScratch S;
  S.rows = 0;
  S.h1 = S.rows + learn_round4(B * (2 * in + 2));
  S.h2 = S.h1 + learn_round4(3 * B * kLH1);
  S.d = S.h2 + learn_round4(3 * B * kLH2);
  S.dq = S.d + learn_round4(B);
  S.dh2 = S.dq + learn_round4(B * kLMaxOut);
  S.dh1 = S.dh2 + learn_round4(B * kLH2);
  S.g = S.dh1 + learn_round4(B * kLH1);
  S.total = S.g + learn_round4(learn_layout(in, out).total);
  return S;
}

// Everything one update's launches (or the host loops) read.
struct Learn {
  float* eval;    // the learner buffer's four blocks
  float* target;
  float* m;
  float* v;
  const float* ring;
  const uint64_t* counter;
  int64_t cap;
  uint64_t seed, draw;
  int32_t filled_only;
  int32_t in, out, rf, B;
  float* rows;  // scratch sections
  float* h1;
  float* h2;
  float* d;
  float* dq;
  float* dh2;
  float* dh1;
  float* g;
  float* rows_out;  // this update's [B, rf], or NULL
  float* loss_out;  // this update's loss, or NULL
  float gamma, inv_b, two_inv_b;
  LearnAdam A;
};

// ---------------------------------------------------------------------------- per-element functions
// d = q_eval(s)[a] - (r + gamma target(s')[argmax eval(s')]) (main.py:144-152), lowest index on ties.
MG_HD float learn_td(const float* qe, const float* qe2, const float* qt2, int out, int a, float r, float gamma) {
  int am = 0;
  for (int j = 1; j < out; ++j)
    if (qe2[j] > qe2[am]) am = j;
  const float t = r + gamma * qt2[am];
  return qe[a] - t;
}

// ---------------------------------------------------------------------------- per-output steps
// (the kernels give one thread per index; the host twin walks the indices in a loop)
// Layer 1, index over (pass, b, j); pass 0 also keeps the sampled row.
MG_HD void learn_l1_at(const Learn& L, uint64_t live, int64_t idx) {
  const int j = static_cast<int>(idx % kLH1);
  const int64_t pb = idx / kLH1;
  const int b = static_cast<int>(pb % L.B), pass = static_cast<int>(pb / L.B);
  const float* row = L.ring + learn_slot(static_cast<uint64_t>(b), L.draw, L.seed, live) * L.rf;
  const float* P = pass == 2 ? L.target : L.eval;
  const LearnLayout O = learn_layout(L.in, L.out);
  const float* x = row + (pass == 0 ? 0 : L.in + 2);
  L.h1[idx] = learn_relu(learn_fwd(x, P + O.w1 + j * L.in, P[O.b1 + j], L.in));
  if (pass == 0 && j < L.rf) {
    const float val = row[j];
    L.rows[b * L.rf + j] = val;
    if (L.rows_out) L.rows_out[b * L.rf + j] = val;
  }
}

// Layer 3 of row b's three passes into q[3 out], slot = pass out + j.
MG_HD float learn_l3_at(const Learn& L, int b, int slot) {
  const int pass = slot / L.out, j = slot - pass * L.out;
  const float* P = pass == 2 ? L.target : L.eval;
  const LearnLayout O = learn_layout(L.in, L.out);
  return learn_fwd(L.h2 + (static_cast<int64_t>(pass) * L.B + b) * kLH2, P + O.w3 + j * kLH2, P[O.b3 + j], kLH2);
}

// Row b's d and dq[b, j] from its q[3 out].
MG_HD void learn_td_at(const Learn& L, int b, int j, const float* q) {
  const float* row = L.rows + b * L.rf;
  const int a = learn_action(row[L.in], L.out);
  const float d = learn_td(q, q + L.out, q + 2 * L.out, L.out, a, row[L.in + 1], L.gamma);
  if (j == 0) L.d[b] = d;
  L.dq[b * kLMaxOut + j] = j == a ? d * L.two_inv_b : 0.0f;
}

// The three backward launches of one update, layer 3 first.
MG_HD LearnBwd learn_bwd_layer(const Learn& L, int layer) {
  const LearnLayout O = learn_layout(L.in, L.out);
  LearnBwd G{};
  G.B = L.B;
  G.inv_b = L.inv_b;
  if (layer == 3) {
    G.dy = L.dq, G.sdy = kLMaxOut, G.nJ = L.out;
    G.x = L.h2, G.sx = kLH2, G.nK = kLH2;
    G.W = L.eval + O.w3, G.gW = L.g + O.w3, G.gb = L.g + O.b3;
    G.dx = L.dh2;
    G.d = L.d, G.loss_out = L.loss_out;
  } else if (layer == 2) {
    G.dy = L.dh2, G.sdy = kLH2, G.nJ = kLH2;
    G.x = L.h1, G.sx = kLH1, G.nK = kLH1;
    G.W = L.eval + O.w2, G.gW = L.g + O.w2, G.gb = L.g + O.b2;
    G.dx = L.dh1;
  } else {
    G.dy = L.dh1, G.sdy = kLH1, G.nJ = kLH1;
    G.x = L.rows, G.sx = L.rf, G.nK = L.in;
    G.W = L.eval + O.w1, G.gW = L.g + O.w1, G.gb = L.g + O.b1;
  }
  return G;
}

MG_HD void learn_adam_at(const Learn& L, int64_t i) { learn_adam(L.eval[i], L.m[i], L.v[i], L.g[i], L.A); }

// ---------------------------------------------------------------------------- kernels
__global__ __launch_bounds__(kBlock) void learn_l1_kernel(const Learn L) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (idx >= static_cast<int64_t>(3) * L.B * kLH1) return;
  learn_l1_at(L, learn_rows_live(L.cap, L.counter, L.filled_only), idx);
}

// blockIdx = (unit tile, row tile, pass); thread = (unit, row) of the tile.
__global__ __launch_bounds__(kLTileJ* kLTileB) void learn_l2_kernel(const Learn L) {
  __shared__ float ws[kLTileJ * (kLH1 + 1)];  // odd row stride: a wave's 32 units hit 32 banks
  __shared__ float xs[kLTileB * kLH1];
  const int pass = blockIdx.z, j0 = blockIdx.x * kLTileJ, b0 = blockIdx.y * kLTileB;
  const float* P = pass == 2 ? L.target : L.eval;
  const LearnLayout O = learn_layout(L.in, L.out);
  const float* h1 = L.h1 + static_cast<int64_t>(pass) * L.B * kLH1;
  for (int e = threadIdx.x; e < kLTileJ * kLH1; e += kLTileJ * kLTileB) {
    const int jj = e / kLH1, k = e - jj * kLH1;
    ws[jj * (kLH1 + 1) + k] = j0 + jj < kLH2 ? P[O.w2 + (j0 + jj) * kLH1 + k] : 0.0f;
  }
  for (int e = threadIdx.x; e < kLTileB * kLH1; e += kLTileJ * kLTileB) {
    const int bb = e / kLH1;
    xs[e] = b0 + bb < L.B ? h1[static_cast<int64_t>(b0) * kLH1 + e] : 0.0f;
  }
  __syncthreads();
  const int tj = threadIdx.x % kLTileJ, tb = threadIdx.x / kLTileJ;
  const int j = j0 + tj, b = b0 + tb;
  if (j >= kLH2 || b >= L.B) return;
  L.h2[(static_cast<int64_t>(pass) * L.B + b) * kLH2 + j] =
      learn_relu(learn_fwd(xs + tb * kLH1, ws + tj * (kLH1 + 1), P[O.b2 + j], kLH1));
}

__global__ __launch_bounds__(32 * kLRows3) void learn_l3_kernel(const Learn L) {
  __shared__ float q[kLRows3][3 * kLMaxOut];
  const int slot = threadIdx.x & 31, rb = threadIdx.x >> 5;
  const int b = blockIdx.x * kLRows3 + rb;
  if (b < L.B && slot < 3 * L.out) q[rb][slot] = learn_l3_at(L, b, slot);
  __syncthreads();
  if (b < L.B && slot < L.out) learn_td_at(L, b, slot, q[rb]);
}

__global__ __launch_bounds__(kBlock) void learn_adam_kernel(const Learn L, int n) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) learn_adam_at(L, i);
}

// ---------------------------------------------------------------------------- host side of a call
// What mg_dqn_learn and mg_host_dqn_learn refuse, before anything is read or launched.
int check_learn(const char* what, const float* learner, const float* rows, const uint64_t* counter, int64_t capacity,
                int32_t row_floats, int32_t in_dim, int32_t out_dim, int32_t batch, int32_t num_updates,
                int32_t filled_only, const mg_dqn_hyper* hyper, const float* loss_out, const float* rows_out,
                const void* packed_out, const void* scratch, size_t scratch_bytes) {
  if (!learner || !rows || !hyper || !scratch || (filled_only && !counter))
    return fail(hipErrorInvalidValue, "%s: NULL pointer", what);
  if (int e = check_net_dims(what, in_dim, out_dim)) return e;
  if (row_floats != 2 * in_dim + 2)
    return fail(hipErrorInvalidValue, "%s: row_floats must be 2 * in_dim + 2", what);
  if (int e = check_learn_sizes(what, batch, capacity, num_updates)) return e;
  if (hyper->target_period < 1) return fail(hipErrorInvalidValue, "%s: target_period must be >= 1", what);
  if (int e = check_adam_betas(what, hyper)) return e;
  if (misaligned(learner, 15) || misaligned(scratch, 15) || misaligned(packed_out, 15) || misaligned(rows, 7) ||
      misaligned(counter, 7) || misaligned(loss_out, 3) || misaligned(rows_out, 3))
    return fail(hipErrorInvalidValue,
                "%s: learner, scratch and packed_out must be 16-byte, rows and counter 8-byte, loss_out and "
                "rows_out 4-byte aligned", what);
  if (scratch_bytes < static_cast<size_t>(learn_scratch(batch, in_dim, out_dim).total) * sizeof(float))
    return fail(hipErrorInvalidValue, "%s: scratch smaller than mg_dqn_learn_scratch_bytes(batch, in_dim, out_dim)",
                what);
  return 0;
}

// The fields of Learn that do not change from one update of a call to the next.
Learn make_learn(float* learner, const float* rows, const uint64_t* counter, int64_t capacity, int32_t in_dim,
                 int32_t out_dim, int32_t batch, uint64_t seed, int32_t filled_only, const mg_dqn_hyper* hyper,
                 void* scratch) {
  const int P = learn_layout(in_dim, out_dim).total;
  const LearnScratch S = learn_scratch(batch, in_dim, out_dim);
  float* s = static_cast<float*>(scratch);
  Learn L{};
  L.eval = learner, L.target = learner + P, L.m = learner + 2 * P, L.v = learner + 3 * P;
  L.ring = rows, L.counter = counter, L.cap = capacity;
  L.seed = seed, L.filled_only = filled_only;
  L.in = in_dim, L.out = out_dim, L.rf = 2 * in_dim + 2, L.B = batch;
  L.rows = s + S.rows, L.h1 = s + S.h1, L.h2 = s + S.h2, L.d = s + S.d, L.dq = s + S.dq;
  L.dh2 = s + S.dh2, L.dh1 = s + S.dh1, L.g = s + S.g;
  L.gamma = static_cast<float>(hyper->gamma);
  L.inv_b = static_cast<float>(1.0 / batch);
  L.two_inv_b = static_cast<float>(2.0 / batch);
  return L;
}

// Update number u of a call: its draw, optional outputs and Adam's step t + 1 (t = first_update + u).
void learn_set_update(Learn& L, const mg_dqn_hyper* h, uint64_t t, uint64_t draw, int32_t u, float* loss_out,
                      float* rows_out) {
  L.A = learn_adam_scalars(h, t);
  L.draw = draw;
  L.loss_out = loss_out ? loss_out + u : nullptr;
  L.rows_out = rows_out ? rows_out + static_cast<int64_t>(u) * L.B * L.rf : nullptr;
}

// One update on the device (mg_dqn_learn), after learn_set_update: the launch order that
// host_learn_update below restates loop for loop.
void launch_learn_update(const Learn& L, const LearnLayout& O, bool sync_target, hipStream_t st) {
  const int P = O.total;
  if (sync_target)
    hipLaunchKernelGGL(learn_copy_kernel, dim3(grid_blocks(P)), dim3(kBlock), 0, st, L.eval, L.target, P);
  hipLaunchKernelGGL(learn_l1_kernel, dim3(grid_blocks(int64_t{3} * L.B * kLH1)), dim3(kBlock), 0, st, L);
  hipLaunchKernelGGL(learn_l2_kernel, dim3((kLH2 + kLTileJ - 1) / kLTileJ, (L.B + kLTileB - 1) / kLTileB, 3),
                     dim3(kLTileJ * kLTileB), 0, st, L);
  hipLaunchKernelGGL(learn_l3_kernel, dim3((L.B + kLRows3 - 1) / kLRows3), dim3(32 * kLRows3), 0, st, L);
  for (int layer = 3; layer >= 1; --layer) {
    const LearnBwd G = learn_bwd_layer(L, layer);
    hipLaunchKernelGGL(learn_bwd_kernel, dim3(grid_blocks(learn_bwd_items(G))), dim3(kBlock), 0, st, G);
  }
  hipLaunchKernelGGL(learn_adam_kernel, dim3(grid_blocks(P)), dim3(kBlock), 0, st, L, P);
}

// One update on the host (mg_host_dqn_learn), after learn_set_update: the kernels' per-item
// functions in the kernels' order, so the same fp32 chains.
void host_learn_update(const Learn& L, const LearnLayout& O, bool sync_target) {
  if (sync_target) std::memcpy(L.target, L.eval, sizeof(float) * O.total);
  const int64_t batch = L.B;
  const uint64_t live = learn_rows_live(L.cap, L.counter, L.filled_only);
  for (int64_t i = 0; i < 3 * batch * kLH1; ++i) learn_l1_at(L, live, i);
  for (int pass = 0; pass < 3; ++pass) {  // learn_l2_kernel without its LDS tiles: the same chains
    const float* Pm = pass == 2 ? L.target : L.eval;
    for (int64_t b = 0; b < batch; ++b)
      for (int j = 0; j < kLH2; ++j)
        L.h2[(pass * batch + b) * kLH2 + j] =
            learn_relu(learn_fwd(L.h1 + (pass * batch + b) * kLH1, Pm + O.w2 + j * kLH1, Pm[O.b2 + j], kLH1));
  }
  for (int b = 0; b < L.B; ++b) {
    float q[3 * kLMaxOut];
    for (int slot = 0; slot < 3 * L.out; ++slot) q[slot] = learn_l3_at(L, b, slot);
    for (int j = 0; j < L.out; ++j) learn_td_at(L, b, j, q);
  }
  for (int layer = 3; layer >= 1; --layer) {
    const LearnBwd G = learn_bwd_layer(L, layer);
    for (int64_t i = 0; i < learn_bwd_items(G); ++i) learn_bwd_at(G, i);
  }
  for (int i = 0; i < O.total; ++i) learn_adam_at(L, i);
}

}  // namespace
