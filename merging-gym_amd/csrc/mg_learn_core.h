// mg_learn_core.h -- the fixed-order fp32 primitives both learners (mg_learn.h, mg_rainbow_learn.h) are built
// on: the minibatch draw, the fmaf chains, Adam, one layer's backward pass. They are the bit-for-bit contract
// include/merging_hip.h documents at mg_dqn_learn and mg_rainbow_learn -- every dot product a sequential fmaf
// chain, no float atomics, nothing that depends on the grid -- and host and device run the same functions.
// A part of the one translation unit merging_hip.hip (see its head comment).
#pragma once

#include "mg_common.h"
#include "mg_env.h"
#include "mg_launch.h"

namespace {

constexpr int kLBatch = 16;  // loads a chain issues together before it consumes them, in order: a
                             // one-by-one chain waits a memory latency per term (166 us per update
                             // at batch 128 before)

MG_HD int64_t learn_round4(int64_t n) { return (n + 3) & ~int64_t{3}; }

struct LearnAdam {  // one update's scalars: doubles on the host, each rounded to fp32 once
  float b1, omb1, b2, omb2, step, bc2s, eps;
};

// Update number t's scalars (t counted from 0; Adam's step count is t + 1): computed in double,
// libm pow as Python's float ** int, each rounded to fp32 once.
inline LearnAdam learn_adam_scalars(const mg_dqn_hyper* h, uint64_t t) {
  const double step = static_cast<double>(t + 1);
  LearnAdam A;
  A.b1 = static_cast<float>(h->beta1);
  A.omb1 = static_cast<float>(1.0 - h->beta1);
  A.b2 = static_cast<float>(h->beta2);
  A.omb2 = static_cast<float>(1.0 - h->beta2);
  A.step = static_cast<float>(h->lr / (1.0 - std::pow(h->beta1, step)));
  A.bc2s = static_cast<float>(std::sqrt(1.0 - std::pow(h->beta2, step)));
  A.eps = static_cast<float>(h->eps);
  return A;
}

// ---------------------------------------------------------------------------- per-element functions
// Words x, y of Philox4x32-10(key = seed, counter = (b, draw)): the block every minibatch draw of row b takes
// its bits from.
MG_HD void learn_words(uint64_t b, uint64_t draw, uint64_t seed, uint32_t& w0, uint32_t& w1) {
#ifdef __HIP_DEVICE_COMPILE__
  const uint4 u = philox4x32_10(make_uint4(static_cast<uint32_t>(b), static_cast<uint32_t>(b >> 32),
                                           static_cast<uint32_t>(draw), static_cast<uint32_t>(draw >> 32)),
                                static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32));
  w0 = u.x, w1 = u.y;
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
  w0 = c0, w1 = c1;
#endif
}

// Slot of minibatch row b: mg_replay_sample's draw (replay_sample_kernel), word x of that block scaled to
// [0, m).
MG_HD uint64_t learn_slot(uint64_t b, uint64_t draw, uint64_t seed, uint64_t m) {
  uint32_t w0, w1;
  learn_words(b, draw, seed, w0, w1);
  return (static_cast<uint64_t>(w0) * m) >> 32;
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

// Sequential sum over i ascending of w[i] a[i], each product rounded once, from +0 (the weighted loss).
MG_HD float learn_wsum(const float* w, const float* a, int n) {
  float acc = 0.0f;
  for (int i = 0; i < n; ++i) acc = acc + w[i] * a[i];
  return acc;
}

// The row's action column truncated to int (main.py:133 astype(int)), kept inside 0..out-1 (the
// reference's gather would raise outside; NaN gives 0).
MG_HD int learn_action(float a, int out) {
  if (!(a >= 0.0f)) return 0;
  if (a >= static_cast<float>(out)) return out - 1;
  return static_cast<int>(a);
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

// ---------------------------------------------------------------------------- kernels
__global__ __launch_bounds__(kBlock) void learn_copy_kernel(const float* src, float* dst, int n) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

__global__ __launch_bounds__(kBlock) void learn_bwd_kernel(const LearnBwd G) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (idx < learn_bwd_items(G)) learn_bwd_at(G, idx);
}

// ---------------------------------------------------------------------------- the refusals both learners share
inline int check_learn_sizes(const char* what, int32_t batch, int64_t capacity, int32_t num_updates) {
  if (batch < 1 || batch > 1024) return fail(hipErrorInvalidValue, "%s: need 1 <= batch <= 1024", what);
  if (capacity < 1 || capacity > (int64_t{1} << 32))
    return fail(hipErrorInvalidValue, "%s: need 1 <= capacity <= 2^32", what);
  if (num_updates < 0) return fail(hipErrorInvalidValue, "%s: num_updates < 0", what);
  return 0;
}

inline int check_adam_betas(const char* what, const mg_dqn_hyper* hyper) {
  if (hyper->beta1 >= 0.0 && hyper->beta1 < 1.0 && hyper->beta2 >= 0.0 && hyper->beta2 < 1.0) return 0;
  return fail(hipErrorInvalidValue, "%s: need 0 <= beta1 < 1 and 0 <= beta2 < 1", what);
}

}  // namespace
