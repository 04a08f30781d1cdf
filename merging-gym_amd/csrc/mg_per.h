// mg_per.h -- prioritized replay for Rainbow: SumSegmentTree, MinSegmentTree and PrioritizedReplayBuffer
// (scripts/ranbowdqn.py:130-262, :326-437) as one fp64 tree buffer beside RainbowReplay's rows, with the store,
// sample and update kernels and the per-element functions the host twins (mg_host_per_*) run too. It stands
// alone: the learner that samples from the tree is mg_rainbow_learn.h's. Up to 64 members' trees of one capacity
// go through the same functions with the member in the grid (PerStoreMany; mg_rainbow_learn.h's PerMany): a
// member has its own buffer, counter and scalars, nothing else.
// A part of the one translation unit merging_hip.hip (see its head comment).
#pragma once

#include "mg_common.h"
#include "mg_env.h"
#include "mg_launch.h"
#include "mg_learn_core.h"
#include "mg_replay.h"

namespace {

// ============================================================================ the tree buffer
// C = the smallest power of two >= capacity (:345-347). fp64 sum[2 C], min[2 C] (node 1 the root, leaf i at
// C + i, node 0 unused, as SegmentTree._value), max_priority, one pad: (4 C + 2) doubles. fp64 because the
// reference's nodes are Python floats and the sampled indices must be the reference's.
struct PerTree {
  double *sum, *mn, *maxp;
  int64_t C, cap;
  int32_t logC;
};
MG_HD int64_t per_leaves(int64_t capacity) {
  int64_t C = 1;
  while (C < capacity) C *= 2;
  return C;
}
MG_HD PerTree per_tree(void* buf, int64_t capacity) {
  PerTree T;
  T.C = per_leaves(capacity);
  T.cap = capacity;
  T.logC = 0;
  while ((int64_t{1} << T.logC) < T.C) ++T.logC;
  T.sum = static_cast<double*>(buf);
  T.mn = T.sum + 2 * T.C;
  T.maxp = T.mn + 2 * T.C;
  return T;
}
MG_HD int64_t per_doubles(int64_t capacity) { return 4 * per_leaves(capacity) + 2; }
// the tree of `shape`'s capacity in another buffer: the members of a call share C, cap and logC
MG_HD PerTree per_tree_at(const PerTree& shape, void* buf) {
  PerTree T = shape;
  T.sum = static_cast<double*>(buf);
  T.mn = T.sum + 2 * T.C;
  T.maxp = T.mn + 2 * T.C;
  return T;
}

// element i of the fresh buffer: sums 0.0 (:218), minima +inf (:256), max_priority 1.0 (:351), the pad 0
MG_HD void per_init_at(const PerTree& T, int64_t i) {
  if (i < 2 * T.C)
    T.sum[i] = 0.0, T.mn[i] = INFINITY;
  else if (i == 2 * T.C)
    T.maxp[0] = 1.0, T.maxp[1] = 0.0;
}

// ============================================================================ pow
// log(x) for a normal x > 0 and exp(a), fp64, the same bits on host and device: the algorithms and constants of
// fdlibm's e_log.c and e_exp.c (Sun Microsystems, 1993, freely distributable) without their special cases, every
// operation rounded once (contraction is off), no library call.
MG_HD double per_log(double x) {
  uint64_t ix = __builtin_bit_cast(uint64_t, x);
  uint32_t hx = static_cast<uint32_t>(ix >> 32);
  int k = static_cast<int>(hx >> 20) - 1023;
  hx &= 0x000fffffu;
  const uint32_t i = (hx + 0x95f64u) & 0x100000u;  // m in [sqrt(1/2), sqrt 2)
  k += static_cast<int>(i >> 20);
  ix = (static_cast<uint64_t>(hx | (i ^ 0x3ff00000u)) << 32) | (ix & 0xffffffffull);
  const double f = __builtin_bit_cast(double, ix) - 1.0;
  const double dk = static_cast<double>(k);
  const double s = f / (2.0 + f);
  const double z = s * s;
  const double w = z * z;
  const double t1 = w * (3.999999999940941908e-01 + w * (2.222219843214978396e-01 + w * 1.531383769920937332e-01));
  const double t2 = z * (6.666666666666735130e-01 +
                         w * (2.857142874366239149e-01 + w * (1.818357216161805012e-01 + w * 1.479819860511658591e-01)));
  const double R = t2 + t1;
  const double hfsq = (0.5 * f) * f;
  return dk * 6.93147180369123816490e-01 - ((hfsq - (s * (hfsq + R) + dk * 1.90821492927058770002e-10)) - f);
}

MG_HD double per_exp(double a) {
  if (a > 709.0) return INFINITY;
  if (!(a >= -708.0)) return 0.0;  // the results below stay normal
  const int k = static_cast<int>(1.44269504088896338700e+00 * a + (a < 0.0 ? -0.5 : 0.5));
  const double t = static_cast<double>(k);
  const double hi = a - t * 6.93147180369123816490e-01;  // exact: ln2_hi has 32 trailing zero bits
  const double lo = t * 1.90821492927058770002e-10;
  const double x = hi - lo;
  const double xx = x * x;
  const double c = x - xx * (1.66666666666666019037e-01 +
                             xx * (-2.77777777770155933842e-03 +
                                   xx * (6.61375632143793436117e-05 +
                                         xx * (-1.65339022054652515390e-06 + xx * 4.13813679705723846039e-08))));
  const double y = 1.0 - ((lo - (x * c) / (2.0 - c)) - hi);
  return y * __builtin_bit_cast(double, static_cast<uint64_t>(k + 1023) << 52);
}

// x ** y for a normal positive finite x (NaN otherwise): exp(y log x)
MG_HD double per_pow(double x, double y) {
  if (!(x >= 2.2250738585072014e-308 && x < INFINITY)) return NAN;
  return per_exp(y * per_log(x));
}

// priority ** alpha (:357, :434); alpha == 1 takes the priority itself, so that tree is the reference's bit for bit
MG_HD double per_prio(double p, double alpha) { return alpha == 1.0 ? p : per_pow(p, alpha); }

// Python's min(a, b): b where b < a, else a
MG_HD double per_min(double a, double b) { return b < a ? b : a; }

// node = left op right (:202-205)
MG_HD void per_node_at(const PerTree& T, int64_t node) {
  T.sum[node] = T.sum[2 * node] + T.sum[2 * node + 1];
  T.mn[node] = per_min(T.mn[2 * node], T.mn[2 * node + 1]);
}

// ============================================================================ store
// The slots a store of `total` transitions writes: the newest min(total, capacity) of them, a range modulo the
// capacity, as at most two leaf ranges [a, b).
struct PerSegs {
  int64_t a0, b0, a1, b1, start, count;
};
MG_HD int64_t per_store_count(int64_t total, int64_t cap) { return total < cap ? total : cap; }
MG_HD PerSegs per_segs(uint64_t counter, int64_t total, int64_t cap) {
  PerSegs G;
  G.count = per_store_count(total, cap);
  G.start = static_cast<int64_t>((counter + static_cast<uint64_t>(total - G.count)) % static_cast<uint64_t>(cap));
  const int64_t end = G.start + G.count;
  G.a0 = G.start, G.b0 = end < cap ? end : cap;
  G.a1 = 0, G.b1 = end > cap ? end - cap : 0;
  return G;
}
// an upper bound of the nodes of level j (the leaves are level 0) above `count` consecutive slots modulo the
// capacity: the host sizes the launches with it, since the position is on the device
MG_HD int64_t per_level_items(int64_t count, int j) { return (count >> j) + 4; }

// item i of level 0: the leaf of a written slot takes max_priority ** alpha in both trees (:353-358)
MG_HD void per_fill_at(const PerTree& T, const PerSegs& G, double alpha, int64_t i) {
  if (i >= G.count) return;
  const int64_t leaf = T.C + (G.start + i) % T.cap;
  const double v = per_prio(*T.maxp, alpha);
  T.sum[leaf] = v;
  T.mn[leaf] = v;
}
// item i of level j >= 1: each range's dirty nodes are the range shifted right
MG_HD void per_level_at(const PerTree& T, const PerSegs& G, int j, int64_t i) {
  const int64_t lo0 = (T.C + G.a0) >> j, n0 = G.b0 > G.a0 ? ((T.C + G.b0 - 1) >> j) - lo0 + 1 : 0;
  if (i < n0) return per_node_at(T, lo0 + i);
  i -= n0;
  const int64_t lo1 = (T.C + G.a1) >> j, n1 = G.b1 > G.a1 ? ((T.C + G.b1 - 1) >> j) - lo1 + 1 : 0;
  if (i < n1) per_node_at(T, lo1 + i);
}

constexpr int kPerTail = 1024;  // the threads of the single-block kernels
// the first level whose bound fits one block
MG_HD int per_tail_level(int64_t count) {
  int j = 1;
  while (per_level_items(count, j) > kPerTail) ++j;
  return j;
}

__global__ __launch_bounds__(kBlock) void per_init_kernel(const PerTree T) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  per_init_at(T, i);
}

__global__ __launch_bounds__(kBlock) void per_fill_kernel(const PerTree T, const uint64_t* counter, int64_t total,
                                                          double alpha) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  per_fill_at(T, per_segs(*counter, total, T.cap), alpha, i);
}

__global__ __launch_bounds__(kBlock) void per_level_kernel(const PerTree T, const uint64_t* counter, int64_t total,
                                                           int j) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  per_level_at(T, per_segs(*counter, total, T.cap), j, i);
}

// levels j0 .. logC in one block: a barrier between a level and its parents
__global__ __launch_bounds__(kPerTail) void per_tail_kernel(const PerTree T, const uint64_t* counter, int64_t total,
                                                            int j0) {
  const PerSegs G = per_segs(*counter, total, T.cap);
  for (int j = j0; j <= T.logC; ++j) {
    per_level_at(T, G, j, threadIdx.x);
    __syncthreads();
  }
}

// ---- the member in the grid (mg_per_store_many): the capacity and the store's size are shared, so the count, the
// levels and every grid are the lone store's; member m = blockIdx.y reads its own counter and writes its own tree.
struct PerStoreMany {
  PerTree shape;  // C, cap, logC; the pointers are member 0's and unused
  int64_t total;
  void* tree[kMaxMembers];
  const uint64_t* counter[kMaxMembers];
  double alpha[kMaxMembers];
};
static_assert(sizeof(PerStoreMany) <= 4096, "HIP's kernel argument limit");

__global__ __launch_bounds__(kBlock) void per_fill_many_kernel(const PerStoreMany A) {
  const int m = blockIdx.y;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  per_fill_at(per_tree_at(A.shape, A.tree[m]), per_segs(*A.counter[m], A.total, A.shape.cap), A.alpha[m], i);
}

__global__ __launch_bounds__(kBlock) void per_level_many_kernel(const PerStoreMany A, int j) {
  const int m = blockIdx.y;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  per_level_at(per_tree_at(A.shape, A.tree[m]), per_segs(*A.counter[m], A.total, A.shape.cap), j, i);
}

// one block per member: the barrier is between a member's level and its own parents
__global__ __launch_bounds__(kPerTail) void per_tail_many_kernel(const PerStoreMany A, int j0) {
  const int m = blockIdx.x;
  const PerTree T = per_tree_at(A.shape, A.tree[m]);
  const PerSegs G = per_segs(*A.counter[m], A.total, T.cap);
  for (int j = j0; j <= T.logC; ++j) {
    per_level_at(T, G, j, threadIdx.x);
    __syncthreads();
  }
}

// The tree's part of a store, after the rows and before the counter moves.
void launch_per_store_tree(const PerTree& T, const uint64_t* counter, int64_t total, double alpha, hipStream_t st) {
  const int64_t count = per_store_count(total, T.cap);
  hipLaunchKernelGGL(per_fill_kernel, dim3(grid_blocks(count)), dim3(kBlock), 0, st, T, counter, total, alpha);
  if (T.logC == 0) return;
  const int j0 = per_tail_level(count);
  for (int j = 1; j < j0 && j <= T.logC; ++j)
    hipLaunchKernelGGL(per_level_kernel, dim3(grid_blocks(per_level_items(count, j))), dim3(kBlock), 0, st, T, counter,
                       total, j);
  if (j0 <= T.logC) hipLaunchKernelGGL(per_tail_kernel, dim3(1), dim3(kPerTail), 0, st, T, counter, total, j0);
}

// launch_per_store_tree for all members: the same launches in the same order, the member in the grid
void launch_per_store_tree_many(const PerStoreMany& A, int32_t members, hipStream_t st) {
  const unsigned M = static_cast<unsigned>(members);
  const PerTree& T = A.shape;
  const int64_t count = per_store_count(A.total, T.cap);
  hipLaunchKernelGGL(per_fill_many_kernel, dim3(grid_blocks(count), M), dim3(kBlock), 0, st, A);
  if (T.logC == 0) return;
  const int j0 = per_tail_level(count);
  for (int j = 1; j < j0 && j <= T.logC; ++j)
    hipLaunchKernelGGL(per_level_many_kernel, dim3(grid_blocks(per_level_items(count, j)), M), dim3(kBlock), 0, st, A,
                       j);
  if (j0 <= T.logC) hipLaunchKernelGGL(per_tail_many_kernel, dim3(M), dim3(kPerTail), 0, st, A, j0);
}

void host_per_store_tree(const PerTree& T, const uint64_t* counter, int64_t total, double alpha) {
  const PerSegs G = per_segs(*counter, total, T.cap);
  for (int64_t i = 0; i < G.count; ++i) per_fill_at(T, G, alpha, i);
  for (int j = 1; j <= T.logC; ++j)
    for (int64_t i = 0; i < per_level_items(G.count, j); ++i) per_level_at(T, G, j, i);
}

// ============================================================================ sample
// random.random()'s construction from words x, y of learn_slot's Philox block: 53 bits in [0, 1)
MG_HD double per_uniform(uint64_t b, uint64_t draw, uint64_t seed) {
  uint32_t w0, w1;
  learn_words(b, draw, seed, w0, w1);
  return (static_cast<double>(w0 >> 5) * 67108864.0 + static_cast<double>(w1 >> 6)) * (1.0 / 9007199254740992.0);
}

MG_HD int64_t per_len(const uint64_t* counter, int64_t cap) {
  const uint64_t c = *counter;
  return c < static_cast<uint64_t>(cap) ? static_cast<int64_t>(c) : cap;
}

// sum(0, len - 1) (:364): the leaves 0 .. len - 2, in _reduce_helper's association -- right-nested over the
// nodes that cover the prefix, widest first (:159-172) -- so built here from the narrowest node up. len >= 2.
MG_HD double per_total(const PerTree& T, int64_t len) {
  const int64_t m = len - 1;  // the leaves summed
  double acc = 0.0;
  bool first = true;
  for (int j = 0; j <= T.logC; ++j) {
    if (!((m >> j) & 1)) continue;
    const double v = T.sum[(T.C + ((m >> (j + 1)) << (j + 1))) >> j];
    acc = first ? v : v + acc;
    first = false;
  }
  return acc;
}

// find_prefixsum_idx (:241-248), kept below len whatever the buffer holds
MG_HD int64_t per_find(const PerTree& T, double mass, int64_t len) {
  int64_t idx = 1;
  while (idx < T.C) {
    const double left = T.sum[2 * idx];
    if (left > mass)
      idx = 2 * idx;
    else
      mass -= left, idx = 2 * idx + 1;
  }
  idx -= T.C;
  return idx < len ? idx : len - 1;
}

struct PerSample {
  PerTree T;
  const uint64_t* counter;
  double beta;
  uint64_t seed, draw;
  int32_t B;
  int64_t *idx, *idx_out;  // idx_out, w_out: a second copy, or NULL
  float *w, *w_out;
};

// Draw b (:360-367) and its weight (:405-412). With fewer than two transitions the reference recurses out of
// its tree; here slot 0 with weight 1.
MG_HD void per_sample_at(const PerSample& P, int b) {
  const int64_t len = per_len(P.counter, P.T.cap);
  int64_t idx = 0;
  float w = 1.0f;
  if (len >= 2) {
    const double mass = per_uniform(static_cast<uint64_t>(b), P.draw, P.seed) * per_total(P.T, len);
    idx = per_find(P.T, mass, len);
    const double root = P.T.sum[1], n = static_cast<double>(len);
    const double p_min = P.T.mn[1] / root, p_sample = P.T.sum[P.T.C + idx] / root;
    w = static_cast<float>(per_pow(p_sample * n, -P.beta) / per_pow(p_min * n, -P.beta));
  }
  P.idx[b] = idx, P.w[b] = w;
  if (P.idx_out) P.idx_out[b] = idx;
  if (P.w_out) P.w_out[b] = w;
}

// One body for the lone sample (Arg = PerSample: blockIdx.y is 0 and unused) and a population's (Arg =
// mg_rainbow_learn.h's PerMany, from which per_sample_member rebases member blockIdx.y's PerSample).
MG_HD const PerSample& per_sample_member(const PerSample& P, int) { return P; }
template <class Arg>
__global__ __launch_bounds__(kBlock) void per_sample_kernel(const Arg Q) {
  const PerSample& P = per_sample_member(Q, blockIdx.y);
  const int b = blockIdx.x * kBlock + threadIdx.x;
  if (b < P.B) per_sample_at(P, b);
}

// ============================================================================ update
struct PerUpdate {
  PerTree T;
  const uint64_t* counter;
  double alpha;
  const int64_t* idx;
  const float* priority;
  float add;  // with has_add: priority[b] + add, one fp32 sum (the learner's loss_b + prio_eps)
  int32_t has_add, B;
};
MG_HD float per_update_priority(const PerUpdate& U, int b) {
  return U.has_add ? U.priority[b] + U.add : U.priority[b];
}
// what the reference's asserts let through (:432-433): a positive priority at a stored slot; anything else is
// left out of the update
MG_HD bool per_update_valid(const PerUpdate& U, int b, int64_t len) {
  return U.idx[b] >= 0 && U.idx[b] < len && per_update_priority(U, b) > 0.0f;
}
MG_HD void per_update_leaf_at(const PerUpdate& U, int b) {
  const double v = per_prio(static_cast<double>(per_update_priority(U, b)), U.alpha);
  U.T.sum[U.T.C + U.idx[b]] = v;
  U.T.mn[U.T.C + U.idx[b]] = v;
}

// One block, one thread per entry: the last of the entries that name a slot sets its leaf (the reference's
// loop order, :431-435), max_priority takes every entry's priority, then each path is rebuilt a level at a time.
// per_update_kernel runs it as its one block; a population's (mg_rainbow_learn.h's per_update_many_kernel) as one
// block per member, each on its own tree, so the barriers order a member's own levels.
__device__ __forceinline__ void per_update_block(const PerUpdate& U) {
  __shared__ int64_t sidx[kPerTail];
  __shared__ float smax[kPerTail];
  const int b = threadIdx.x;
  const int64_t len = per_len(U.counter, U.T.cap);
  const bool valid = b < U.B && per_update_valid(U, b, len);
  sidx[b] = valid ? U.idx[b] : -1;
  smax[b] = valid ? per_update_priority(U, b) : 0.0f;
  __syncthreads();
  bool mine = valid;
  for (int o = b + 1; mine && o < U.B; ++o) mine = sidx[o] != sidx[b];
  if (mine) per_update_leaf_at(U, b);
  for (int s = kPerTail / 2; s > 0; s >>= 1) {
    if (b < s) smax[b] = fmaxf(smax[b], smax[b + s]);
    __syncthreads();
  }
  if (b == 0 && static_cast<double>(smax[0]) > *U.T.maxp) *U.T.maxp = static_cast<double>(smax[0]);
  for (int j = 1; j <= U.T.logC; ++j) {
    if (mine) per_node_at(U.T, (U.T.C + sidx[b]) >> j);
    __syncthreads();
  }
}

__global__ __launch_bounds__(kPerTail) void per_update_kernel(const PerUpdate U) { per_update_block(U); }

void host_per_update(const PerUpdate& U) {
  const int64_t len = per_len(U.counter, U.T.cap);
  for (int b = 0; b < U.B; ++b) {
    if (!per_update_valid(U, b, len)) continue;
    per_update_leaf_at(U, b);
    const double p = static_cast<double>(per_update_priority(U, b));
    if (p > *U.T.maxp) *U.T.maxp = p;
  }
  for (int j = 1; j <= U.T.logC; ++j)
    for (int b = 0; b < U.B; ++b)
      if (per_update_valid(U, b, len)) per_node_at(U.T, (U.T.C + U.idx[b]) >> j);
}

// ============================================================================ host side of a call
int check_per_tree(const char* what, const void* tree, size_t tree_bytes, int64_t capacity) {
  if (!tree) return fail(hipErrorInvalidValue, "%s: NULL pointer", what);
  if (capacity < 1 || capacity > (int64_t{1} << 32))
    return fail(hipErrorInvalidValue, "%s: need 1 <= capacity <= 2^32", what);
  if (misaligned(tree, 15)) return fail(hipErrorInvalidValue, "%s: the tree buffer must be 16-byte aligned", what);
  if (tree_bytes < static_cast<size_t>(per_doubles(capacity)) * sizeof(double))
    return fail(hipErrorInvalidValue, "%s: tree buffer smaller than mg_per_bytes(capacity)", what);
  return 0;
}

int check_per_alpha(const char* what, double alpha) {
  return alpha > 0.0 ? 0 : fail(hipErrorInvalidValue, "%s: need alpha > 0", what);
}
int check_per_beta(const char* what, double beta) {
  return beta > 0.0 ? 0 : fail(hipErrorInvalidValue, "%s: need beta > 0", what);
}
int check_per_batch(const char* what, int32_t batch) {
  return batch >= 1 && batch <= kPerTail ? 0 : fail(hipErrorInvalidValue, "%s: need 1 <= batch <= 1024", what);
}

int check_per_sample(const char* what, const void* tree, size_t tree_bytes, const uint64_t* counter, int64_t capacity,
                     double beta, int32_t batch, const int64_t* idx_out, const float* weight_out) {
  if (!counter || !idx_out || !weight_out) return fail(hipErrorInvalidValue, "%s: NULL pointer", what);
  if (int e = check_per_tree(what, tree, tree_bytes, capacity)) return e;
  if (int e = check_per_beta(what, beta)) return e;
  if (int e = check_per_batch(what, batch)) return e;
  if (misaligned(counter, 7) || misaligned(idx_out, 7) || misaligned(weight_out, 3))
    return fail(hipErrorInvalidValue, "%s: counter and idx_out must be 8-byte, weight_out 4-byte aligned", what);
  return 0;
}

int check_per_update(const char* what, const void* tree, size_t tree_bytes, const uint64_t* counter, int64_t capacity,
                     double alpha, const int64_t* idx, const float* priority, int32_t batch) {
  if (!counter || !idx || !priority) return fail(hipErrorInvalidValue, "%s: NULL pointer", what);
  if (int e = check_per_tree(what, tree, tree_bytes, capacity)) return e;
  if (int e = check_per_alpha(what, alpha)) return e;
  if (int e = check_per_batch(what, batch)) return e;
  if (misaligned(counter, 7) || misaligned(idx, 7) || misaligned(priority, 3))
    return fail(hipErrorInvalidValue, "%s: counter and idx must be 8-byte, priority 4-byte aligned", what);
  return 0;
}

}  // namespace
