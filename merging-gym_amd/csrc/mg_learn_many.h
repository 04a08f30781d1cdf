// mg_learn_many.h -- a population of DQN learners in one set of launches: `members` independent learners of
// one shape, each on its own net, memory, seed and hyperparameters, through mg_learn.h's seven launches with the
// member taken from the grid. Every kernel rebases a Learn for its member and calls mg_learn.h's per-element
// functions unchanged, so member m's bits are those of mg_dqn_learn on its buffers (include/merging_hip.h at
// mg_dqn_learn_many). A part of the one translation unit merging_hip.hip (see its head comment).
#pragma once

#include "mg_common.h"
#include "mg_launch.h"
#include "mg_learn.h"
#include "mg_learn_core.h"
#include "mg_qnet.h"

namespace {

constexpr int kLMaxMembers = 64;  // one bit each in the target-copy mask

// What a member keeps for all its updates: one entry of the device-resident member table, written once by
// mg_dqn_learn_many_init.
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
  const LearnMember* table;  // [members]
  float* rows_out;           // this update's [members, B, rf], or NULL
  float* loss_out;           // this update's [members], or NULL
  int64_t stride;            // floats of one member's scratch
  int64_t cap;
  int32_t filled_only, in, out, B, members;
  float inv_b, two_inv_b;
  uint64_t sync;  // bit m: member m's target copy is due before this update
  uint64_t draw[kLMaxMembers];
  float step[kLMaxMembers];
  float bc2s[kLMaxMembers];
};
static_assert(sizeof(LearnMany) <= 1152, "the by-value kernel argument stays well inside HIP's 4096 bytes");

// Member m's Learn: its blocks, its scratch, its row of the outputs, its table entry and per-update scalars.
MG_HD Learn learn_member(const LearnMany& Q, int m) {
  const int P = learn_layout(Q.in, Q.out).total;
  const LearnScratch S = learn_scratch(Q.B, Q.in, Q.out);
  const LearnMember& T = Q.table[m];
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

// Items of one backward launch (learn_bwd_items of learn_bwd_layer): the same for every member.
inline int64_t learn_many_bwd_items(int in, int out, int B, int layer) {
  const int64_t nJ = layer == 3 ? out : layer == 2 ? kLH2 : kLH1;
  const int64_t nK = layer == 3 ? kLH2 : layer == 2 ? kLH1 : in;
  return nJ * (nK + 1) + (layer == 1 ? 0 : B * nK) + 1;
}

// ---------------------------------------------------------------------------- kernels
// mg_learn.h's kernels with blockIdx.y the member (learn_many_l2_kernel: blockIdx.z = 3 member + pass).
__global__ __launch_bounds__(kBlock) void learn_many_entry_kernel(LearnMember* dst, const LearnMember e) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *dst = e;
}

__global__ __launch_bounds__(kBlock) void learn_many_copy_kernel(const LearnMany Q) {
  const int m = blockIdx.y, i = blockIdx.x * kBlock + threadIdx.x;
  if (!((Q.sync >> m) & 1)) return;
  const int P = learn_layout(Q.in, Q.out).total;
  float* learner = Q.learners + static_cast<int64_t>(m) * 4 * P;
  if (i < P) learner[P + i] = learner[i];
}

__global__ __launch_bounds__(kBlock) void learn_many_l1_kernel(const LearnMany Q) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (idx >= static_cast<int64_t>(3) * Q.B * kLH1) return;
  const Learn L = learn_member(Q, blockIdx.y);
  learn_l1_at(L, learn_rows_live(L.cap, L.counter, L.filled_only), idx);
}

// blockIdx = (unit tile, row tile, 3 member + pass); thread = (unit, row) of the tile: learn_l2_kernel's tiles.
__global__ __launch_bounds__(kLTileJ* kLTileB) void learn_many_l2_kernel(const LearnMany Q) {
  __shared__ float ws[kLTileJ * (kLH1 + 1)];
  __shared__ float xs[kLTileB * kLH1];
  const int pass = blockIdx.z % 3, j0 = blockIdx.x * kLTileJ, b0 = blockIdx.y * kLTileB;
  const Learn L = learn_member(Q, blockIdx.z / 3);
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

__global__ __launch_bounds__(32 * kLRows3) void learn_many_l3_kernel(const LearnMany Q) {
  __shared__ float q[kLRows3][3 * kLMaxOut];
  const Learn L = learn_member(Q, blockIdx.y);
  const int slot = threadIdx.x & 31, rb = threadIdx.x >> 5;
  const int b = blockIdx.x * kLRows3 + rb;
  if (b < L.B && slot < 3 * L.out) q[rb][slot] = learn_l3_at(L, b, slot);
  __syncthreads();
  if (b < L.B && slot < L.out) learn_td_at(L, b, slot, q[rb]);
}

template <int LAYER>
__global__ __launch_bounds__(kBlock) void learn_many_bwd_kernel(const LearnMany Q) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const LearnBwd G = learn_bwd_layer(learn_member(Q, blockIdx.y), LAYER);
  if (idx < learn_bwd_items(G)) learn_bwd_at(G, idx);
}

__global__ __launch_bounds__(kBlock) void learn_many_adam_kernel(const LearnMany Q, int n) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) learn_adam_at(learn_member(Q, blockIdx.y), i);
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
inline bool members_ok(int32_t members) { return members >= 1 && members <= kLMaxMembers; }

inline int fail_member(const char* what, int m, const char* text) {
  std::snprintf(g_err, sizeof(g_err), "%s: member %d: %s", what, m, text);
  return static_cast<int>(hipErrorInvalidValue);
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

// A member's table entry: the scalars make_learn and learn_adam_scalars round to fp32, rounded the same way.
inline LearnMember learn_member_entry(const mg_dqn_member& M) {
  const LearnAdam A = learn_adam_scalars(&M.hyper, 0);
  return LearnMember{M.rows, M.counter, M.seed, static_cast<float>(M.hyper.gamma), A.b1, A.omb1, A.b2, A.omb2, A.eps};
}

// The fields of LearnMany that do not change from one update of a call to the next.
LearnMany make_learn_many(float* learners, const LearnMember* table, int32_t members, int64_t capacity, int32_t in_dim,
                          int32_t out_dim, int32_t batch, int32_t filled_only, void* scratch) {
  LearnMany Q{};
  Q.learners = learners, Q.scratch = static_cast<float*>(scratch), Q.table = table;
  Q.stride = learn_scratch(batch, in_dim, out_dim).total;
  Q.cap = capacity, Q.filled_only = filled_only;
  Q.in = in_dim, Q.out = out_dim, Q.B = batch, Q.members = members;
  Q.inv_b = static_cast<float>(1.0 / batch);
  Q.two_inv_b = static_cast<float>(2.0 / batch);
  return Q;
}

// Update number u of a call: every member's draw, Adam's step t + 1 (t = its first_update + u) from the host's
// doubles as learn_set_update takes them, whose target copy is due, and the update's rows of the outputs.
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

// One update of all members on the device, after learn_many_set_update: launch_learn_update's order, the
// member in the grid's y (layer 2: in z with the pass).
void launch_learn_many_update(const LearnMany& Q, hipStream_t st) {
  const unsigned M = static_cast<unsigned>(Q.members);
  const int P = learn_layout(Q.in, Q.out).total;
  if (Q.sync) hipLaunchKernelGGL(learn_many_copy_kernel, dim3(grid_blocks(P), M), dim3(kBlock), 0, st, Q);
  hipLaunchKernelGGL(learn_many_l1_kernel, dim3(grid_blocks(int64_t{3} * Q.B * kLH1), M), dim3(kBlock), 0, st, Q);
  hipLaunchKernelGGL(learn_many_l2_kernel, dim3((kLH2 + kLTileJ - 1) / kLTileJ, (Q.B + kLTileB - 1) / kLTileB, 3 * M),
                     dim3(kLTileJ * kLTileB), 0, st, Q);
  hipLaunchKernelGGL(learn_many_l3_kernel, dim3((Q.B + kLRows3 - 1) / kLRows3, M), dim3(32 * kLRows3), 0, st, Q);
  const auto bwd_grid = [&](int layer) { return dim3(grid_blocks(learn_many_bwd_items(Q.in, Q.out, Q.B, layer)), M); };
  hipLaunchKernelGGL(learn_many_bwd_kernel<3>, bwd_grid(3), dim3(kBlock), 0, st, Q);
  hipLaunchKernelGGL(learn_many_bwd_kernel<2>, bwd_grid(2), dim3(kBlock), 0, st, Q);
  hipLaunchKernelGGL(learn_many_bwd_kernel<1>, bwd_grid(1), dim3(kBlock), 0, st, Q);
  hipLaunchKernelGGL(learn_many_adam_kernel, dim3(grid_blocks(P), M), dim3(kBlock), 0, st, Q, P);
}

// The same on the host: host_learn_update member by member, each on the Learn the kernels rebase.
void host_learn_many_update(const LearnMany& Q) {
  const LearnLayout O = learn_layout(Q.in, Q.out);
  for (int m = 0; m < Q.members; ++m) host_learn_update(learn_member(Q, m), O, (Q.sync >> m) & 1);
}

}  // namespace
