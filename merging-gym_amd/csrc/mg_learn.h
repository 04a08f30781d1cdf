// mg_learn.h -- DQN.learn on the device: the minibatch update (Double-DQN target, MSE, Adam) and the target
// copy for a population of up to 64 learners of one shape in one set of launches -- the lone learner
// (mg_dqn_learn) is the population of one -- with the per-element functions the host twins run too.
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
// mg_learn_core.h's). Every kernel takes its member from the grid, rebases a Learn for it
// (learn_member) and runs the per-element functions below, so member m's bits are those of a lone
// learner on its buffers. One update of all members is seven launches, in launch_learn_many_update's
// order:
//   learn_l1_kernel    minibatch rows (the draw of mg_replay_sample) -> scratch, layer 1 of the
//                      three passes: eval(s), eval(s'), target(s')
//   learn_l2_kernel    layer 2 of the three passes, W2 and the inputs tiled through LDS
//   learn_l3_kernel    layer 3, the Double-DQN target, d = q_eval[a] - t, dq
//   learn_bwd_layer_kernel<3 / 2 / 1>  the weight / bias gradients and the input gradient of a layer
//                      (the layer-3 launch also sums the loss)
//   learn_adam_kernel  Adam over all parameters
// and learn_sync_kernel before them when any member's target net is due (main.py:125-127): the copy
// under a 64-bit member mask.
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

// Everything one update's launches (or the host loops) read of one member: learn_member builds it.
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

// ---------------------------------------------------------------------------- the members of a call
// What a member keeps for all its updates: one entry of the device-resident member table
// (mg_dqn_learn_many_init writes it once), or for the lone learner the entry LearnMany carries.
struct LearnMember {
  const float* ring;
  const uint64_t* counter;
  uint64_t seed;
  float gamma, b1, omb1, b2, omb2, eps;
};
static_assert(sizeof(LearnMember) == 48, "mg_dqn_learn_many_table_bytes is 48 bytes per member");

// Everything one update's launches (or the host loops) read, for all members. The per-update values -- each
// member's draw, Adam's step and bc2s from the host's doubles, the target-copy mask -- travel by value.
struct LearnMany {
  float* learners;           // [members, 4 P]
  float* scratch;            // [members, stride]
  const LearnMember* table;  // [members], or NULL: the one member is `one` (mg_dqn_learn has no table)
  float* rows_out;           // this update's [members, B, rf], or NULL
  float* loss_out;           // this update's [members], or NULL
  int64_t stride;            // floats of one member's scratch
  int64_t cap;
  int32_t filled_only, in, out, B, members;
  float inv_b, two_inv_b;
  uint64_t sync;  // bit m: member m's target copy is due before this update
  uint64_t draw[kMaxMembers];
  float step[kMaxMembers];
  float bc2s[kMaxMembers];
  LearnMember one;  // last: the fields above keep the offsets the table's kernels read them at
};
static_assert(sizeof(LearnMany) <= 1200, "the by-value kernel argument stays well inside HIP's 4096 bytes");

// Member m's Learn: its blocks, its scratch, its row of the outputs, its entry and per-update scalars.
// TABLE says where the entry is: Q.table[m], or Q.one for the call without a table. It is a template argument
// of every kernel and not `Q.table ? Q.table[m] : Q.one` at run time because a pointer to either the table or
// the kernel argument is a generic one: the compiler then fetches the entry with per-lane flat loads instead
// of scalar loads, which cost the population 1.3 to 2.4 % per update at every M.
template <bool TABLE>
MG_HD const LearnMember& learn_entry(const LearnMany& Q, int m) {
  if constexpr (TABLE)
    return Q.table[m];
  else
    return Q.one;
}

template <bool TABLE>
MG_HD Learn learn_member(const LearnMany& Q, int m) {
  const int P = learn_layout(Q.in, Q.out).total;
  const LearnScratch S = learn_scratch(Q.B, Q.in, Q.out);
  const LearnMember& T = learn_entry<TABLE>(Q, m);
  float* learner = Q.learners + static_cast<int64_t>(m) * 4 * P;
  float* s = Q.scratch + m * Q.stride;
  Learn L{};
  L.eval = learner, L.target = learner + P, L.m = learner + 2 * P, L.v = learner + 3 * P;
  L.ring = T.ring, L.counter = T.counter, L.cap = Q.cap;
  L.seed = T.seed, L.draw = Q.draw[m], L.filled_only = Q.filled_only;
  L.in = Q.in, L.out = Q.out, L.rf = 2 * Q.in + 2, L.B = Q.B;
  L.rows = s + S.rows, L.h1 = s + S.h1, L.h2 = s + S.h2, L.d = s + S.d, L.dq = s + S.dq;
  L.dh2 = s + S.dh2, L.dh1 = s + S.dh1, L.g = s + S.g;
  L.rows_out = Q.rows_out ? Q.rows_out + static_cast<int64_t>(m) * L.B * L.rf : nullptr;
  L.loss_out = Q.loss_out ? Q.loss_out + m : nullptr;
  L.gamma = T.gamma, L.inv_b = Q.inv_b, L.two_inv_b = Q.two_inv_b;
  L.A = LearnAdam{T.b1, T.omb1, T.b2, T.omb2, Q.step[m], Q.bc2s[m], T.eps};
  return L;
}


// ---------------------------------------------------------------------------- kernels
// blockIdx.y is the member (learn_l2_kernel: blockIdx.z = 3 member + pass); one body each, instantiated with and
// without a table.
__global__ __launch_bounds__(kBlock) void learn_many_entry_kernel(LearnMember* dst, const LearnMember e) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *dst = e;
}

__global__ __launch_bounds__(kBlock) void learn_sync_kernel(const LearnMany Q) {
  const int m = blockIdx.y, i = blockIdx.x * kBlock + threadIdx.x;
  if (!((Q.sync >> m) & 1)) return;
  const int P = learn_layout(Q.in, Q.out).total;
  float* learner = Q.learners + static_cast<int64_t>(m) * 4 * P;
  if (i < P) learner[P + i] = learner[i];
}

template <bool TABLE>
__global__ __launch_bounds__(kBlock) void learn_l1_kernel(const LearnMany Q) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (idx >= static_cast<int64_t>(3) * Q.B * kLH1) return;
  const Learn L = learn_member<TABLE>(Q, blockIdx.y);
  learn_l1_at(L, learn_rows_live(L.cap, L.counter, L.filled_only), idx);
}

// blockIdx = (unit tile, row tile, 3 member + pass); thread = (unit, row) of the tile.
template <bool TABLE>
__global__ __launch_bounds__(kLTileJ* kLTileB) void learn_l2_kernel(const LearnMany Q) {
  __shared__ float ws[kLTileJ * (kLH1 + 1)];  // odd row stride: a wave's 32 units hit 32 banks
  __shared__ float xs[kLTileB * kLH1];
  const int pass = blockIdx.z % 3, j0 = blockIdx.x * kLTileJ, b0 = blockIdx.y * kLTileB;
  const Learn L = learn_member<TABLE>(Q, blockIdx.z / 3);
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

template <bool TABLE>
__global__ __launch_bounds__(32 * kLRows3) void learn_l3_kernel(const LearnMany Q) {
  __shared__ float q[kLRows3][3 * kLMaxOut];
  const Learn L = learn_member<TABLE>(Q, blockIdx.y);
  const int slot = threadIdx.x & 31, rb = threadIdx.x >> 5;
  const int b = blockIdx.x * kLRows3 + rb;
  if (b < L.B && slot < 3 * L.out) q[rb][slot] = learn_l3_at(L, b, slot);
  __syncthreads();
  if (b < L.B && slot < L.out) learn_td_at(L, b, slot, q[rb]);
}

// learn_bwd_kernel per member; the layer a template argument: no scratch for the choice of LearnBwd.
template <bool TABLE, int LAYER>
__global__ __launch_bounds__(kBlock) void learn_bwd_layer_kernel(const LearnMany Q) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const LearnBwd G = learn_bwd_layer(learn_member<TABLE>(Q, blockIdx.y), LAYER);
  if (idx < learn_bwd_items(G)) learn_bwd_at(G, idx);
}

template <bool TABLE>
__global__ __launch_bounds__(kBlock) void learn_adam_kernel(const LearnMany Q, int n) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) learn_adam_at(learn_member<TABLE>(Q, blockIdx.y), i);
}

// qnet_pack_kernel / qnet32_pack_kernel with blockIdx.y the member: its eval block into its packed net.
__global__ void qnet_pack_many_kernel(const float* learners, int in_dim, int out_dim, uint8_t* packed, int64_t stride) {
  const LearnLayout O = learn_layout(in_dim, out_dim);
  const float* p = learners + static_cast<int64_t>(blockIdx.y) * 4 * O.total;
  qnet_pack_at(blockIdx.x * blockDim.x + threadIdx.x, p + O.w1, p + O.b1, p + O.w2, p + O.b2, p + O.w3, p + O.b3, in_dim,
               out_dim, packed + blockIdx.y * stride);
}

__global__ void qnet32_pack_many_kernel(const float* learners, int in_dim, int out_dim, uint8_t* packed,
                                        int64_t stride) {
  const LearnLayout O = learn_layout(in_dim, out_dim);
  const float* p = learners + static_cast<int64_t>(blockIdx.y) * 4 * O.total;
  qnet32_pack_at(blockIdx.x * blockDim.x + threadIdx.x, p + O.w1, p + O.b1, p + O.w2, p + O.b2, p + O.w3, p + O.b3,
                 in_dim, out_dim, packed + blockIdx.y * stride + kQNetBytes);
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

// What mg_dqn_learn_many_init, mg_dqn_learn_many and mg_host_dqn_learn_many refuse of the member list.
int check_members(const char* what, const mg_dqn_member* member, int32_t members, int32_t filled_only) {
  if (!members_ok(members)) return fail(hipErrorInvalidValue, "%s: need 1 <= members <= 64", what);
  if (!member) return fail(hipErrorInvalidValue, "%s: NULL pointer", what);
  for (int m = 0; m < members; ++m) {
    const mg_dqn_member& M = member[m];
    if (!M.rows || (filled_only && !M.counter)) return fail(hipErrorInvalidValue, "%s: NULL pointer", what);
    if (misaligned(M.rows, 7) || misaligned(M.counter, 7))
      return fail_member(what, m, "rows and counter must be 8-byte aligned");
    if (M.hyper.target_period < 1) return fail_member(what, m, "target_period must be >= 1");
    if (!(M.hyper.beta1 >= 0.0 && M.hyper.beta1 < 1.0 && M.hyper.beta2 >= 0.0 && M.hyper.beta2 < 1.0))
      return fail_member(what, m, "need 0 <= beta1 < 1 and 0 <= beta2 < 1");
  }
  return 0;
}

int check_member_table(const char* what, const void* table, size_t table_bytes, int32_t members) {
  if (!table) return fail(hipErrorInvalidValue, "%s: NULL pointer", what);
  if (misaligned(table, 15)) return fail(hipErrorInvalidValue, "%s: table must be 16-byte aligned", what);
  if (table_bytes < sizeof(LearnMember) * static_cast<size_t>(members))
    return fail(hipErrorInvalidValue, "%s: table smaller than mg_dqn_learn_many_table_bytes(members)", what);
  return 0;
}

// What mg_dqn_learn_many and mg_host_dqn_learn_many refuse, before anything is read or launched (the device
// call checks its table besides).
int check_learn_many(const char* what, const float* learners, const mg_dqn_member* member, int32_t members,
                     int64_t capacity, int32_t row_floats, int32_t in_dim, int32_t out_dim, int32_t batch,
                     int32_t num_updates, int32_t filled_only, const float* loss_out, const float* rows_out,
                     const void* packed_out, size_t packed_stride, const void* scratch, size_t scratch_bytes) {
  if (!members_ok(members)) return fail(hipErrorInvalidValue, "%s: need 1 <= members <= 64", what);
  if (!learners || !member || !scratch) return fail(hipErrorInvalidValue, "%s: NULL pointer", what);
  if (int e = check_net_dims(what, in_dim, out_dim)) return e;
  if (row_floats != 2 * in_dim + 2)
    return fail(hipErrorInvalidValue, "%s: row_floats must be 2 * in_dim + 2", what);
  if (int e = check_learn_sizes(what, batch, capacity, num_updates)) return e;
  if (int e = check_members(what, member, members, filled_only)) return e;
  if (misaligned(learners, 15) || misaligned(scratch, 15) || misaligned(packed_out, 15) || misaligned(loss_out, 3) ||
      misaligned(rows_out, 3) || (packed_out && packed_stride % 16 != 0))
    return fail(hipErrorInvalidValue,
                "%s: learners, scratch and packed_out must be 16-byte, loss_out and rows_out 4-byte aligned, "
                "packed_stride a multiple of 16", what);
  if (packed_out && packed_stride < static_cast<size_t>(kQNetBytes + kQ32NetBytes))
    return fail(hipErrorInvalidValue, "%s: packed_stride smaller than mg_qnet_packed_bytes()", what);
  const size_t one = static_cast<size_t>(learn_scratch(batch, in_dim, out_dim).total) * sizeof(float);
  if (scratch_bytes < one * static_cast<size_t>(members))
    return fail(hipErrorInvalidValue,
                "%s: scratch smaller than members * mg_dqn_learn_scratch_bytes(batch, in_dim, out_dim)", what);
  return 0;
}

// A member's table entry: gamma and Adam's constants, each rounded to fp32 once (learn_adam_scalars).
inline LearnMember learn_member_entry(const mg_dqn_member& M) {
  const LearnAdam A = learn_adam_scalars(&M.hyper, 0);
  return LearnMember{M.rows, M.counter, M.seed, static_cast<float>(M.hyper.gamma), A.b1, A.omb1, A.b2, A.omb2, A.eps};
}

// The fields of LearnMany that do not change from one update of a call to the next. Without a table the call
// has one member, whose entry travels in the argument.
LearnMany make_learn_many(float* learners, const LearnMember* table, const mg_dqn_member* member, int32_t members,
                          int64_t capacity, int32_t in_dim, int32_t out_dim, int32_t batch, int32_t filled_only,
                          void* scratch) {
  LearnMany Q{};
  Q.learners = learners, Q.scratch = static_cast<float*>(scratch), Q.table = table;
  if (!table) Q.one = learn_member_entry(member[0]);
  Q.stride = learn_scratch(batch, in_dim, out_dim).total;
  Q.cap = capacity, Q.filled_only = filled_only;
  Q.in = in_dim, Q.out = out_dim, Q.B = batch, Q.members = members;
  Q.inv_b = static_cast<float>(1.0 / batch);
  Q.two_inv_b = static_cast<float>(2.0 / batch);
  return Q;
}

// Update number u of a call: every member's draw, Adam's step t + 1 (t = its first_update + u) from the host's
// doubles, whose target copy is due, and the update's rows of the outputs.
void learn_many_set_update(LearnMany& Q, const mg_dqn_member* member, int32_t u, float* loss_out, float* rows_out) {
  Q.sync = 0;
  for (int m = 0; m < Q.members; ++m) {
    const uint64_t t = member[m].first_update + static_cast<uint64_t>(u);
    const LearnAdam A = learn_adam_scalars(&member[m].hyper, t);
    Q.step[m] = A.step, Q.bc2s[m] = A.bc2s;
    Q.draw[m] = member[m].first_draw + static_cast<uint64_t>(u);
    if (t % static_cast<uint64_t>(member[m].hyper.target_period) == 0) Q.sync |= uint64_t{1} << m;
  }
  Q.loss_out = loss_out ? loss_out + static_cast<int64_t>(u) * Q.members : nullptr;
  Q.rows_out = rows_out ? rows_out + static_cast<int64_t>(u) * Q.members * Q.B * (2 * Q.in + 2) : nullptr;
}

// One update of all members on the device, after learn_many_set_update: the launch order that
// host_learn_update below restates loop for loop, the member in the grid's y (layer 2: in z with the pass).
template <bool TABLE>
void launch_learn_many_update(const LearnMany& Q, hipStream_t st) {
  const unsigned M = static_cast<unsigned>(Q.members);
  const int P = learn_layout(Q.in, Q.out).total;
  const Learn shape = learn_member<false>(Q, 0);  // the backward grids: the same for every member and entry
  const auto bwd_grid = [&](int layer) { return dim3(grid_blocks(learn_bwd_items(learn_bwd_layer(shape, layer))), M); };
  if (Q.sync) hipLaunchKernelGGL(learn_sync_kernel, dim3(grid_blocks(P), M), dim3(kBlock), 0, st, Q);
  hipLaunchKernelGGL(learn_l1_kernel<TABLE>, dim3(grid_blocks(int64_t{3} * Q.B * kLH1), M), dim3(kBlock), 0, st, Q);
  hipLaunchKernelGGL(learn_l2_kernel<TABLE>, dim3((kLH2 + kLTileJ - 1) / kLTileJ, (Q.B + kLTileB - 1) / kLTileB, 3 * M),
                     dim3(kLTileJ * kLTileB), 0, st, Q);
  hipLaunchKernelGGL(learn_l3_kernel<TABLE>, dim3((Q.B + kLRows3 - 1) / kLRows3, M), dim3(32 * kLRows3), 0, st, Q);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(learn_bwd_layer_kernel<TABLE, 3>), bwd_grid(3), dim3(kBlock), 0, st, Q);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(learn_bwd_layer_kernel<TABLE, 2>), bwd_grid(2), dim3(kBlock), 0, st, Q);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(learn_bwd_layer_kernel<TABLE, 1>), bwd_grid(1), dim3(kBlock), 0, st, Q);
  hipLaunchKernelGGL(learn_adam_kernel<TABLE>, dim3(grid_blocks(P), M), dim3(kBlock), 0, st, Q, P);
}

// One member's update on the host: the kernels' per-item functions in the kernels' order, so the same
// fp32 chains.
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

// One update of all members on the host: host_learn_update member by member, each on the Learn the kernels
// rebase.
void host_learn_many_update(const LearnMany& Q) {
  const LearnLayout O = learn_layout(Q.in, Q.out);
  for (int m = 0; m < Q.members; ++m)
    host_learn_update(Q.table ? learn_member<true>(Q, m) : learn_member<false>(Q, m), O, (Q.sync >> m) & 1);
}

// ---------------------------------------------------------------------------- the drivers of a call
// What a successful call leaves in the member list: the next call continues the run.
void learn_advance(mg_dqn_member* member, int32_t members, int32_t num_updates) {
  for (int m = 0; m < members; ++m) {
    member[m].first_update += static_cast<uint64_t>(num_updates);
    member[m].first_draw += static_cast<uint64_t>(num_updates);
  }
}

// mg_dqn_learn and mg_dqn_learn_many after their checks: the updates back to back on the stream, then the
// acting kernels' layouts of all the new eval nets (mg_qnet_pack's grids and element functions).
int learn_many_device(const char* what, LearnMany& Q, mg_dqn_member* member, int32_t num_updates, float* loss_out,
                      float* rows_out, void* packed_out, size_t packed_stride, hipStream_t st) {
  if (num_updates == 0) return 0;
  for (int32_t u = 0; u < num_updates; ++u) {
    learn_many_set_update(Q, member, u, loss_out, rows_out);
    Q.table ? launch_learn_many_update<true>(Q, st) : launch_learn_many_update<false>(Q, st);
  }
  if (packed_out) {
    const unsigned M = static_cast<unsigned>(Q.members);
    hipLaunchKernelGGL(qnet_pack_many_kernel, dim3(kQPackBlocks, M), dim3(kQPackBlock), 0, st, Q.learners, Q.in, Q.out,
                       static_cast<uint8_t*>(packed_out), static_cast<int64_t>(packed_stride));
    hipLaunchKernelGGL(qnet32_pack_many_kernel, dim3(kQ32PackBlocks, M), dim3(kQPackBlock), 0, st, Q.learners, Q.in,
                       Q.out, static_cast<uint8_t*>(packed_out), static_cast<int64_t>(packed_stride));
  }
  if (int e = finish_launch(what)) return e;
  learn_advance(member, Q.members, num_updates);
  return 0;
}

// mg_host_dqn_learn and mg_host_dqn_learn_many after their checks.
int learn_many_host(LearnMany& Q, mg_dqn_member* member, int32_t num_updates, float* loss_out, float* rows_out) {
  for (int32_t u = 0; u < num_updates; ++u) {
    learn_many_set_update(Q, member, u, loss_out, rows_out);
    host_learn_many_update(Q);
  }
  learn_advance(member, Q.members, num_updates);
  g_err[0] = '\0';
  return 0;
}

}  // namespace
