// mg_learn.h -- DQN.learn on the device: the minibatch update (Double-DQN target, MSE, Adam) and
// the target copy, with the per-element functions the host twin (mg_host_dqn_learn) runs too.
// A part of the one translation unit merging_hip.hip (see its head comment).
#pragma once

#include "mg_common.h"
#include "mg_env.h"
#include "mg_launch.h"
#include "mg_qnet.h"

namespace {

// ============================================================================ DQN.learn
// scripts/main.py:122-157 (DQN.learn), hdqn.py:186-221 (HDQN.learn), :104-139 (Goal_DQN.learn): the
// same code on Net(in, out) with hidden widths 200 / 100 (main.py:30-47). All arithmetic is fp32 in
// the fixed order include/merging_hip.h documents at mg_dqn_learn: every dot product a sequential
// fmaf chain, no float atomics, nothing that depends on the grid. One update is seven launches:
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
constexpr int kLBatch = 16;  // loads a chain issues together before it consumes them, in order: a
                             // one-by-one chain waits a memory latency per term (166 us per update
                             // at batch 128 before)
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

MG_HD int64_t learn_round4(int64_t n) { return (n + 3) & ~int64_t{3}; }

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

struct LearnAdam {  // one update's scalars: doubles on the host, each rounded to fp32 once
  float b1, omb1, b2, omb2, step, bc2s, eps;
};

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
// Slot of minibatch row b: mg_replay_sample's draw (replay_sample_kernel), word x of
// Philox4x32-10(key = seed, counter = (b, draw)) scaled to [0, m).
MG_HD uint64_t learn_slot(uint64_t b, uint64_t draw, uint64_t seed, uint64_t m) {
#ifdef __HIP_DEVICE_COMPILE__
  const uint4 u = philox4x32_10(make_uint4(static_cast<uint32_t>(b), static_cast<uint32_t>(b >> 32),
                                           static_cast<uint32_t>(draw), static_cast<uint32_t>(draw >> 32)),
                                static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32));
  return (static_cast<uint64_t>(u.x) * m) >> 32;
#else
  uint32_t c0 = static_cast<uint32_t>(b), c1 = static_cast<uint32_t>(b >> 32);
  uint32_t c2 = static_cast<uint32_t>(draw), c3 = static_cast<uint32_t>(draw >> 32);
  uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
  for (int r = 0; r < 10; ++r) {
    if (r) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const uint64_t p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c1 ^ k0, n2 = static_cast<uint32_t>(p0 >> 32) ^ c3 ^ k1;
    c1 = static_cast<uint32_t>(p1);
    c3 = static_cast<uint32_t>(p0);
    c0 = n0;
    c2 = n2;
  }
  return (static_cast<uint64_t>(c0) * m) >> 32;
#endif
}

// Rows the draw chooses among: the capacity, or with filled_only the rows stored so far (>= 1).
MG_HD uint64_t learn_rows_live(int64_t cap, const uint64_t* counter, int32_t filled_only) {
  uint64_t m = static_cast<uint64_t>(cap);
  if (filled_only) {
    const uint64_t c = *counter;
    m = c < m ? c : m;
    if (m == 0) m = 1;
  }
  return m;
}

// y = fmaf(x[K-1], w[K-1], ... fmaf(x[0], w[0], bias)), k ascending.
MG_HD float learn_fwd(const float* x, const float* w, float bias, int K) {
  float acc = bias;
  int k = 0;
  for (; k + kLBatch <= K; k += kLBatch) {  // the batch's loads issued together, the chain's order kept
    float xv[kLBatch], wv[kLBatch];
#pragma unroll
    for (int u = 0; u < kLBatch; ++u) xv[u] = x[k + u], wv[u] = w[k + u];
#pragma unroll
    for (int u = 0; u < kLBatch; ++u) acc = fmaf(xv[u], wv[u], acc);
  }
  for (; k < K; ++k) acc = fmaf(x[k], w[k], acc);
  return acc;
}

MG_HD float learn_relu(float y) { return y > 0.0f ? y : 0.0f; }

// fmaf chain over i ascending of a[i sa] b[i sb], from +0 (weight and input gradients).
MG_HD float learn_chain(const float* a, int64_t sa, const float* b, int64_t sb, int n) {
  float acc = 0.0f;
  int i = 0;
  for (; i + kLBatch <= n; i += kLBatch) {
    float av[kLBatch], bv[kLBatch];
#pragma unroll
    for (int u = 0; u < kLBatch; ++u) av[u] = a[(i + u) * sa], bv[u] = b[(i + u) * sb];
#pragma unroll
    for (int u = 0; u < kLBatch; ++u) acc = fmaf(av[u], bv[u], acc);
  }
  for (; i < n; ++i) acc = fmaf(a[i * sa], b[i * sb], acc);
  return acc;
}

// Sequential sum over i ascending of a[i sa], from +0 (bias gradients).
MG_HD float learn_sum(const float* a, int64_t sa, int n) {
  float acc = 0.0f;
  int i = 0;
  for (; i + kLBatch <= n; i += kLBatch) {
    float av[kLBatch];
#pragma unroll
    for (int u = 0; u < kLBatch; ++u) av[u] = a[(i + u) * sa];
#pragma unroll
    for (int u = 0; u < kLBatch; ++u) acc = acc + av[u];
  }
  for (; i < n; ++i) acc = acc + a[i * sa];
  return acc;
}

// The row's action column truncated to int (main.py:133 astype(int)), kept inside 0..out-1 (the
// reference's gather would raise outside; NaN gives 0).
MG_HD int learn_action(float a, int out) {
  if (!(a >= 0.0f)) return 0;
  if (a >= static_cast<float>(out)) return out - 1;
  return static_cast<int>(a);
}

// d = q_eval(s)[a] - (r + gamma target(s')[argmax eval(s')]) (main.py:144-152), lowest index on ties.
MG_HD float learn_td(const float* qe, const float* qe2, const float* qt2, int out, int a, float r, float gamma) {
  int am = 0;
  for (int j = 1; j < out; ++j)
    if (qe2[j] > qe2[am]) am = j;
  const float t = r + gamma * qt2[am];
  return qe[a] - t;
}

// loss = (sum over b ascending of d[b] d[b], from +0) (1 / B) (nn.MSELoss, main.py:153).
MG_HD float learn_loss(const float* d, int B, float inv_b) {
  float acc = 0.0f;
  int b = 0;
  for (; b + kLBatch <= B; b += kLBatch) {
    float dv[kLBatch];
#pragma unroll
    for (int u = 0; u < kLBatch; ++u) dv[u] = d[b + u];
#pragma unroll
    for (int u = 0; u < kLBatch; ++u) acc = acc + dv[u] * dv[u];
  }
  for (; b < B; ++b) acc = acc + d[b] * d[b];
  return acc * inv_b;
}

// torch.optim.Adam's single-tensor step (main.py:96, :157), every operation rounded once.
MG_HD void learn_adam(float& p, float& m, float& v, float g, const LearnAdam& A) {
  m = fmaf(A.omb1, g, A.b1 * m);
  v = fmaf(A.omb2 * g, g, A.b2 * v);
  const float den = sqrtf(v) / A.bc2s + A.eps;
  p = p - A.step * (m / den);
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

// One layer's backward pass: y[b, j] = sum_k x[b, k] W[j, k] + bias[j] with dy given.
struct LearnBwd {
  const float* dy;  // [B, nJ] with row stride sdy
  const float* x;   // [B, nK] with row stride sx: the layer's input
  const float* W;   // [nJ, nK] (eval)
  float* gW;        // [nJ, nK]
  float* gb;        // [nJ]
  float* dx;        // [B, nK] = (dy W) where x > 0, or NULL (layer 1)
  const float* d;   // with loss_out: the launch that also sums the loss
  float* loss_out;
  float inv_b;
  int32_t sdy, sx, nJ, nK, B;
};

MG_HD int64_t learn_bwd_grads(const LearnBwd& G) { return static_cast<int64_t>(G.nJ) * (G.nK + 1); }
MG_HD int64_t learn_bwd_items(const LearnBwd& G) {
  return learn_bwd_grads(G) + (G.dx ? static_cast<int64_t>(G.B) * G.nK : 0) + 1;
}

MG_HD void learn_bwd_at(const LearnBwd& G, int64_t idx) {
  const int64_t ng = learn_bwd_grads(G);
  if (idx < ng) {
    const int j = static_cast<int>(idx / (G.nK + 1)), k = static_cast<int>(idx - static_cast<int64_t>(j) * (G.nK + 1));
    if (k < G.nK)
      G.gW[j * G.nK + k] = learn_chain(G.dy + j, G.sdy, G.x + k, G.sx, G.B);
    else
      G.gb[j] = learn_sum(G.dy + j, G.sdy, G.B);
    return;
  }
  idx -= ng;
  const int64_t nx = G.dx ? static_cast<int64_t>(G.B) * G.nK : 0;
  if (idx < nx) {
    const int b = static_cast<int>(idx / G.nK), k = static_cast<int>(idx - static_cast<int64_t>(b) * G.nK);
    const float v = learn_chain(G.dy + static_cast<int64_t>(b) * G.sdy, 1, G.W + k, G.nK, G.nJ);
    G.dx[idx] = G.x[static_cast<int64_t>(b) * G.sx + k] > 0.0f ? v : 0.0f;
    return;
  }
  if (idx == nx && G.loss_out) *G.loss_out = learn_loss(G.d, G.B, G.inv_b);
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
__global__ __launch_bounds__(kBlock) void learn_copy_kernel(const float* src, float* dst, int n) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

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

__global__ __launch_bounds__(kBlock) void learn_bwd_kernel(const LearnBwd G) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (idx < learn_bwd_items(G)) learn_bwd_at(G, idx);
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
  if (batch < 1 || batch > 1024) return fail(hipErrorInvalidValue, "%s: need 1 <= batch <= 1024", what);
  if (capacity < 1 || capacity > (int64_t{1} << 32))
    return fail(hipErrorInvalidValue, "%s: need 1 <= capacity <= 2^32", what);
  if (num_updates < 0) return fail(hipErrorInvalidValue, "%s: num_updates < 0", what);
  if (hyper->target_period < 1) return fail(hipErrorInvalidValue, "%s: target_period must be >= 1", what);
  if (!(hyper->beta1 >= 0.0 && hyper->beta1 < 1.0 && hyper->beta2 >= 0.0 && hyper->beta2 < 1.0))
    return fail(hipErrorInvalidValue, "%s: need 0 <= beta1 < 1 and 0 <= beta2 < 1", what);
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

// Update number t's fields (t counted from 0; Adam's step count is t + 1): the scalars in double,
// libm pow as Python's float ** int, each rounded to fp32 once.
void learn_set_update(Learn& L, const mg_dqn_hyper* h, uint64_t t, uint64_t draw, float* loss_out, float* rows_out) {
  const double step = static_cast<double>(t + 1);
  L.draw = draw;
  L.loss_out = loss_out;
  L.rows_out = rows_out;
  L.A.b1 = static_cast<float>(h->beta1);
  L.A.omb1 = static_cast<float>(1.0 - h->beta1);
  L.A.b2 = static_cast<float>(h->beta2);
  L.A.omb2 = static_cast<float>(1.0 - h->beta2);
  L.A.step = static_cast<float>(h->lr / (1.0 - std::pow(h->beta1, step)));
  L.A.bc2s = static_cast<float>(std::sqrt(1.0 - std::pow(h->beta2, step)));
  L.A.eps = static_cast<float>(h->eps);
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
