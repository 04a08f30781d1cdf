// mg_stats_reduce.h -- the fixed-order reduction of the statistics records, and goal_status_kernel.
// A part of the one translation unit merging_hip.hip (see its head comment).
#pragma once

#include "mg_common.h"
#include "mg_env.h"

namespace {

// ============================================================================ statistics reduction
// The per-env 64-byte records (mg_episode_stats) summed to one mg_stats_totals in a FIXED order, so
// the fp64 sums are reproducible bit for bit (oracle/merge_oracle.py stats_reduce_fixed restates it):
//   pass 1 (block b of kRedThreads threads, kRedEnvs envs): thread t adds the records of envs
//          b kRedEnvs + j kRedThreads + t, j = 0..kRedPer-1, in j order onto -0.0 (the additive
//          identity), then the block folds its kRedThreads values in halves (v[t] += v[t + o],
//          o = 128, 64, ..., 1) -> partial b;
//   pass 2 (one block): thread t adds partials t, t + 256, ... in order onto -0.0, then the same fold.
// mg_stats_reduce_many runs both passes on many equal runs of the records at once (stats_reduce_many_kernel below).
// The counts are exact int64 sums; the fp64 ones are ret[0], ret[1], ret_main and q_eval. Replaces the logging loops' running totals (hdqn.py:330-346,
// main.py:221-228) for a whole batch; a torch sum over strided record columns took 7.6 ms at 2^20
// envs (BENCH_r03 episodes.reduce_ms) for 64 MB of records.
constexpr int kRedThreads = 256;
constexpr int kRedPer = 4;
constexpr int kRedEnvs = kRedThreads * kRedPer;  // 1,024 records (64 KB) per pass-1 block

constexpr int kRedSums = 4;  // ret[0], ret[1], ret_main, q_eval

__device__ __forceinline__ void red_fold(double (*sd)[kRedThreads], int64_t (*si)[kRedThreads], int t) {
#pragma unroll
  for (int o = kRedThreads / 2; o > 0; o >>= 1) {
    __syncthreads();
    if (t < o) {
#pragma unroll
      for (int k = 0; k < kRedSums; ++k) sd[k][t] = sd[k][t] + sd[k][t + o];
#pragma unroll
      for (int k = 0; k < 6; ++k) si[k][t] += si[k][t + o];
    }
  }
  __syncthreads();
}

__device__ __forceinline__ void red_store(mg_stats_totals* out, double (*sd)[kRedThreads],
                                          int64_t (*si)[kRedThreads]) {
  mg_stats_totals o;
#pragma unroll
  for (int k = 0; k < 3; ++k) o.ret[k] = sd[k][0];
  o.q_eval = sd[3][0];
#pragma unroll
  for (int k = 0; k < 6; ++k) o.counts[k] = si[k][0];
  *out = o;
}

// Pass 1 of one run of n records: block `block` (of this run's own blocks) -> part[block].
__device__ __forceinline__ void red_pass1(const mg_episode_stats* rec, int64_t n, unsigned block,
                                          mg_stats_totals* part) {
  __shared__ double sd[kRedSums][kRedThreads];
  __shared__ int64_t si[6][kRedThreads];
  const int t = threadIdx.x;
  double a0 = -0.0, a1 = -0.0, a2 = -0.0, a3 = -0.0;
  int64_t c[6] = {0, 0, 0, 0, 0, 0};
  const int64_t base = static_cast<int64_t>(block) * kRedEnvs + t;
#pragma unroll
  for (int j = 0; j < kRedPer; ++j) {
    const int64_t i = base + j * kRedThreads;
    if (i < n) {
      // the record as four 16-byte loads: {ret[0], ret[1]}, {ret_main, pending}, counts 0-3, 4-7
      const f64x2* r2 = reinterpret_cast<const f64x2*>(rec + i);
      const f64x2 f0 = __builtin_nontemporal_load(r2), f1 = __builtin_nontemporal_load(r2 + 1);
      const u32x4* u = reinterpret_cast<const u32x4*>(rec + i) + 2;
      const u32x4 u0 = __builtin_nontemporal_load(u), u1 = __builtin_nontemporal_load(u + 1);
      a0 = a0 + f0.x;
      a1 = a1 + f0.y;
      a2 = a2 + f1.x;
      a3 = a3 + __builtin_bit_cast(double, (static_cast<uint64_t>(u1.w) << 32) | u1.z);
      c[0] += u0.x;
      c[1] += u0.y;
      c[2] += u0.z;
      c[3] += u0.w;
      c[4] += u1.x;
      c[5] += u1.y;
    }
  }
  sd[0][t] = a0;
  sd[1][t] = a1;
  sd[2][t] = a2;
  sd[3][t] = a3;
#pragma unroll
  for (int k = 0; k < 6; ++k) si[k][t] = c[k];
  red_fold(sd, si, t);
  if (t == 0) red_store(part + block, sd, si);
}

// Pass 2 of one run: its nb partials -> *out.
__device__ __forceinline__ void red_pass2(const mg_stats_totals* part, int64_t nb, mg_stats_totals* out) {
  __shared__ double sd[kRedSums][kRedThreads];
  __shared__ int64_t si[6][kRedThreads];
  const int t = threadIdx.x;
  double a[kRedSums] = {-0.0, -0.0, -0.0, -0.0};
  int64_t c[6] = {0, 0, 0, 0, 0, 0};
  for (int64_t k = t; k < nb; k += kRedThreads) {
    const mg_stats_totals p = part[k];
#pragma unroll
    for (int q = 0; q < 3; ++q) a[q] = a[q] + p.ret[q];
    a[3] = a[3] + p.q_eval;
#pragma unroll
    for (int q = 0; q < 6; ++q) c[q] += p.counts[q];
  }
#pragma unroll
  for (int q = 0; q < kRedSums; ++q) sd[q][t] = a[q];
#pragma unroll
  for (int q = 0; q < 6; ++q) si[q][t] = c[q];
  red_fold(sd, si, t);
  if (t == 0) red_store(out, sd, si);
}

__global__ __launch_bounds__(kRedThreads) void stats_reduce_kernel(const mg_episode_stats* rec, int64_t n,
                                                                   mg_stats_totals* part) {
  red_pass1(rec, n, blockIdx.x, part);
}

__global__ __launch_bounds__(kRedThreads) void stats_reduce_final_kernel(const mg_stats_totals* part, int64_t nb,
                                                                         mg_stats_totals* out) {
  red_pass2(part, nb, out);
}

// The same two passes over `segments` runs of n_segment records each, the segment in the grid (mg_stats_reduce_many):
// segment s reads records [s n_segment, (s + 1) n_segment), keeps its nb = ceil(n_segment / kRedEnvs) partials at
// part[s nb ..] and writes out[s] -- each bit for bit the lone pair on that run, whose order never looks past it.
__global__ __launch_bounds__(kRedThreads) void stats_reduce_many_kernel(const mg_episode_stats* rec, int64_t n_segment,
                                                                        int64_t nb, mg_stats_totals* part) {
  const int64_t s = blockIdx.y;
  red_pass1(rec + s * n_segment, n_segment, blockIdx.x, part + s * nb);
}

__global__ __launch_bounds__(kRedThreads) void stats_reduce_final_many_kernel(const mg_stats_totals* part, int64_t nb,
                                                                              mg_stats_totals* out) {
  const int64_t s = blockIdx.x;
  red_pass2(part + s * nb, nb, out + s);
}

// goal_status of n (dx1, v2) pairs, the function the h-DQN kernel evaluates (tests, evaluation)
__global__ __launch_bounds__(kBlock) void goal_status_kernel(const double* dx1, const double* v2, int8_t* out,
                                                             int64_t n) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i < n) out[i] = static_cast<int8_t>(goal_status(dx1[i], v2[i]));
}

}  // namespace
