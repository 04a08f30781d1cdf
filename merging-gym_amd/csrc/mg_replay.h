// mg_replay.h -- the DQN replay ring: ReplayIn, ReplayScratch, the scan, write and sample kernels, counter_add_kernel,
// the store with the member in the grid (ReplayMany), and the host side of a store: the one call struct, check
// and driver of mg_replay_store and mg_replay_store_many.
// A part of the one translation unit merging_hip.hip (see its head comment).
#pragma once

#include <type_traits>

#include "mg_common.h"
#include "mg_env.h"
#include "mg_launch.h"

namespace {

// ============================================================================ replay memory
// The DQN replay memory (scripts/main.py:91-92 np.zeros((MEMORY_CAPACITY, 2*NUM_STATES+2)),
// :115-119 store_transition, :130-135 the minibatch draw). A batch of T x n transitions is
// appended in (t, i) order with three launches (kernel boundaries publish the partial sums;
// a last-arriver ticket with device-scope fences measured 8 % slower for the whole store):
//   replay_scan_kernel        one wave per 64 "write blocks" (t, 256-env slice): keep counts
//                             straight from the won bits, a wave scan (in-group offsets), the
//                             group's total;
//   replay_group_scan_kernel  one wave: group totals -> ring positions, memory_counter advanced;
//   replay_write_kernel       one block per 256 envs x kRTChunk steps, the step's
//                             observation kept in registers as the next transition's s; rows
//                             gathered in LDS in ring order and written as contiguous 8-byte
//                             stores (a row is 88 B: 16-byte alignment alternates).
// Rows are kRow floats [s(10), a, r, s'(10)], or kRowGoal [goal, s(10), a, r, next_goal, s'(10)]
// for hdqn.py's lower-level memory (:158, :180-184; goal_state = [goal] + state at :291, :304).
constexpr int kRow = 2 * kObs + 2;       // 22
constexpr int kRowGoal = 2 * kObs + 4;   // 24
constexpr int kRBlock = 256;        // envs per write block
constexpr int kRTChunk = 2;         // steps one write block walks (obs carried in registers; 1 step
                                    // measured +6 %, all 16 per block +11 %: DESIGN.md section 4)
constexpr int kRGroup = 64;         // write blocks per scan wave

struct ReplayIn {
  mg_transitions X;
  int64_t n;
  int64_t words;  // ceil(n / 64): won-mask words per step
  int64_t nbx;    // ceil(n / 256): write blocks per step
  int64_t nb;     // nbx * T
  int32_t T;
  int32_t skip_won;
  // n is the live limit of a column index and, here, also the row stride of the [T, n, ...] tensors, whose
  // first column is this batch's (ReplayMany: a member's slice of a wider batch)
  __device__ int64_t stride() const { return n; }
  __device__ int64_t col0() const { return 0; }
};

struct ReplayScratch {  // carved from the caller's scratch buffer (8-byte header reserved)
  uint64_t* group_base;  // [ngroups] memory_counter before the group's first transition
  uint32_t* local;       // [nb] transitions of earlier write blocks of the same group
  uint32_t* group_total; // [ngroups]
};

__host__ __device__ inline int64_t replay_groups(int64_t nb) { return (nb + kRGroup - 1) / kRGroup; }

__host__ __device__ inline ReplayScratch replay_scratch(void* base, int64_t nb) {
  const int64_t ng = replay_groups(nb);
  ReplayScratch S;
  S.group_base = static_cast<uint64_t*>(base) + 1;
  S.local = reinterpret_cast<uint32_t*>(S.group_base + ng);
  S.group_total = S.local + nb;
  return S;
}

// col0: the batch's first column in the tensors (a multiple of 64; 0 but for a member's slice)
__device__ __forceinline__ bool replay_keep(const ReplayIn& R, int t, int64_t i, int64_t col0 = 0) {
  if (i >= R.n) return false;
  if (!R.skip_won || R.X.won_mask == nullptr) return true;
  const uint64_t w = R.X.won_mask[static_cast<int64_t>(t) * R.words + ((col0 + i) >> 6)];
  return ((w >> (i & 63)) & 1u) == 0;
}

// Kept transitions of write block (t, bx).
__device__ __forceinline__ uint32_t replay_block_count(const ReplayIn& R, int t, int64_t bx, int64_t col0 = 0) {
  const int64_t i0 = bx * kRBlock;
  const int64_t live = R.n - i0 < kRBlock ? R.n - i0 : kRBlock;
  if (!R.skip_won || R.X.won_mask == nullptr) return static_cast<uint32_t>(live);
  const uint64_t* w = R.X.won_mask + static_cast<int64_t>(t) * R.words + ((col0 + i0) >> 6);
  uint64_t wk[kRBlock / 64];
#pragma unroll
  for (int k = 0; k < kRBlock / 64; ++k) wk[k] = live > 64 * k ? w[k] : ~0ull;  // loads issued together
  uint32_t c = 0;
#pragma unroll
  for (int k = 0; k < kRBlock / 64; ++k) {
    const int64_t v = live - 64 * k;  // live envs of this word
    const uint64_t m = v >= 64 ? ~0ull : (v <= 0 ? 0ull : ((1ull << v) - 1));
    c += __popcll(~wk[k] & m);
  }
  return c;
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t u = __shfl_up(v, off);
    if (lane >= off) v += u;
  }
  return v;
}

// One wave: group_base[g] = counter + sum(group_total[0..g)), then counter += sum.
__device__ __forceinline__ void replay_group_scan(const ReplayScratch& S, int64_t ng, uint64_t* counter) {
  const int lane = threadIdx.x & 63;
  const uint64_t c0 = *counter;
  uint64_t carry = 0;
  constexpr int kBatch = 16;  // loads issued together, then scanned: one memory wait per batch
  for (int64_t g0 = 0; g0 < ng; g0 += 64 * kBatch) {
    uint32_t v[kBatch];
#pragma unroll
    for (int b = 0; b < kBatch; ++b) {
      const int64_t g = g0 + 64 * b + lane;
      v[b] = g < ng ? __atomic_load_n(S.group_total + g, __ATOMIC_RELAXED) : 0u;
    }
#pragma unroll
    for (int b = 0; b < kBatch; ++b) {
      const int64_t g = g0 + 64 * b + lane;
      const uint32_t gi = wave_incl_scan(v[b]);
      if (g < ng) S.group_base[g] = c0 + carry + (gi - v[b]);
      carry += __shfl(gi, 63);
    }
  }
  if (lane == 0) *counter = c0 + carry;
}

__global__ __launch_bounds__(64) void replay_group_scan_kernel(const ReplayScratch S, int64_t ng,
                                                               uint64_t* counter) {
  replay_group_scan(S, ng, counter);
}

// One wave: the keep counts of group g's write blocks, their in-group offsets, the group's total.
__device__ __forceinline__ void replay_scan_group(const ReplayIn& R, const ReplayScratch& S, unsigned g,
                                                  int64_t col0 = 0) {
  const int lane = threadIdx.x;
  const int64_t b = static_cast<int64_t>(g) * kRGroup + lane;
  uint32_t c = 0;
  if (b < R.nb) c = replay_block_count(R, static_cast<int>(b / R.nbx), b % R.nbx, col0);
  const uint32_t incl = wave_incl_scan(c);
  if (b < R.nb) S.local[b] = incl - c;
  if (lane == 63) S.group_total[g] = incl;
}

__global__ __launch_bounds__(64) void replay_scan_kernel(const ReplayIn R, ReplayScratch S) {
  replay_scan_group(R, S, blockIdx.x);
}

// Rank of the calling thread among the block's kept threads, and the block total.
__device__ __forceinline__ int block_rank(bool keep, int* wave_cnt, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t m = __ballot(keep);
  const int below = __popcll(m & ((lane == 0) ? 0ull : (~0ull >> (64 - lane))));
  if (lane == 0) wave_cnt[wave] = __popcll(m);
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < kRBlock / 64; ++w) {
    before += (w < wave) ? wave_cnt[w] : 0;
    total += wave_cnt[w];
  }
  return before + below;
}

__device__ __forceinline__ void load_row10(const float* src, float (&v)[kObs]) {
  const f32x2* s2 = reinterpret_cast<const f32x2*>(src);
#pragma unroll
  for (int k = 0; k < kObs / 2; ++k) {
    const f32x2 a = s2[k];
    v[2 * k] = a[0];
    v[2 * k + 1] = a[1];
  }
}

// ---- the member in the grid (mg_replay_store_many): member m's slice [m n_member, (m + 1) n_member) of one
// [T, N, ...] batch into ring m, as mg_replay_store would store a contiguous copy of the slice. A block's
// column index i stays local to its member (live while i < n = n_member; write blocks, scan groups and ring
// positions are per member); the tensors are addressed at column col0() + i with the batch's row stride N
// and its ceil(N / 64) won-mask words per step. n_member is a multiple of 64, so a member's won bits begin
// a word. 22-float rows (KIND 0) only. The member is the grid's last dimension.
struct ReplayMany : ReplayIn {  // X: the whole batch; n = n_member; words = ceil(N / 64); nbx, nb: per member
  int64_t N;               // the batch's envs, the row stride
  int64_t scratch_stride;  // bytes of one member's scratch
  uint8_t* scratch;
  int64_t cap;
  int64_t ng;              // replay_groups(nb)
  float* ring[kMaxMembers];
  uint64_t* counter[kMaxMembers];
  __device__ int64_t stride() const { return N; }
  __device__ int64_t col0() const { return static_cast<int64_t>(blockIdx.z) * n; }  // the write kernel's grid
  __device__ ReplayScratch member_scratch(int m) const {
    return replay_scratch(scratch + static_cast<int64_t>(m) * scratch_stride, nb);
  }
};
static_assert(sizeof(ReplayMany) <= 4096, "HIP's kernel argument limit");

__global__ __launch_bounds__(64) void replay_scan_many_kernel(const ReplayMany A) {  // grid (groups, members)
  replay_scan_group(A, A.member_scratch(blockIdx.y), blockIdx.x, static_cast<int64_t>(blockIdx.y) * A.n);
}

__global__ __launch_bounds__(64) void replay_group_scan_many_kernel(const ReplayMany A) {  // grid (members)
  replay_group_scan(A.member_scratch(blockIdx.x), A.ng, A.counter[blockIdx.x]);
}

// KIND 0: main.py's DQN rows [s, a, r, s']; 1: hdqn.py's lower-level goal rows
// [goal, s, a, r, next_goal, s']; 2: Goal_DQN's rows [s', meta_goal, r, s'] (hdqn.py:97-101 at
// :325, where state is already next_state).
// MANY: the member in the grid (mg_replay_store_many; ReplayMany above) -- grid (write blocks, chunks, members),
// the first argument a ReplayMany and the other four unused: ring, counter and scratch are member blockIdx.z's.
template <int KIND, bool MANY = false>
__global__ __launch_bounds__(kRBlock) void replay_write_kernel(const std::conditional_t<MANY, ReplayMany, ReplayIn> R,
                                                               const ReplayScratch S1, const uint64_t* counter1,
                                                               float* rows1, int64_t cap1) {
  ReplayScratch S = S1;
  const uint64_t* counter = counter1;
  float* rows = rows1;
  int64_t cap = cap1;
  if constexpr (MANY) S = R.member_scratch(blockIdx.z), counter = R.counter[blockIdx.z], rows = R.ring[blockIdx.z], cap = R.cap;
  constexpr bool GOAL = KIND == 1;
  constexpr bool META = KIND == 2;
  constexpr int kRow = GOAL ? kRowGoal : 2 * kObs + 2;  // floats per row
  constexpr int kS = GOAL ? 1 : 0;                      // column of s[0]
  constexpr int kS2 = kS + kObs + 2 + kS;               // column of s'[0]
  __shared__ __attribute__((aligned(16))) float tile[kRBlock * kRow];
  __shared__ int wave_cnt[kRBlock / 64];
  const int64_t bx = blockIdx.x;
  const int64_t i = bx * kRBlock + threadIdx.x;
  const bool live = i < R.n;
  const int64_t c = R.col0() + i;  // the column in the tensors
  const int t0 = blockIdx.y * kRTChunk;
  const int t1 = t0 + kRTChunk < R.T ? t0 + kRTChunk : R.T;
  const uint64_t end = *counter;  // memory_counter after this whole store
  // Only the newest `cap` transitions survive sequential stores; they occupy distinct slots,
  // so no two writes of this launch collide.
  const uint64_t first = end > static_cast<uint64_t>(cap) ? end - static_cast<uint64_t>(cap) : 0u;
  float s[kObs], o[kObs];
  if (live) {
    load_row10(t0 == 0 ? R.X.obs_first + c * kObs : R.X.obs + ((t0 - 1) * R.stride() + c) * kObs, s);
    load_row10(R.X.obs + (t0 * R.stride() + c) * kObs, o);
  }
  for (int t = t0; t < t1; ++t) {
    const int64_t row = static_cast<int64_t>(t) * R.stride() + c;
    const bool keep = replay_keep(R, t, i, R.col0());
    float on[kObs];  // next step's row in flight while this step is gathered and written
    if (live && t + 1 < t1) load_row10(R.X.obs + (row + R.stride()) * kObs, on);
    int total;
    const int rank = block_rank(keep, wave_cnt, total);
    if (total > 0) {  // uniform across the block
      const int64_t b = static_cast<int64_t>(t) * R.nbx + bx;
      const uint64_t base = S.group_base[b / kRGroup] + S.local[b];
      if (keep) {
        float* d = tile + rank * kRow;
        const bool done = R.X.flags ? R.X.flags[4 * row + 2] != 0 : (R.X.done != nullptr && R.X.done[row] != 0);
        float s2[kObs];
        if (done && R.X.final_obs)
          load_row10(R.X.final_obs + row * kObs, s2);
        else
#pragma unroll
          for (int k = 0; k < kObs; ++k) s2[k] = o[k];
#pragma unroll
        for (int k = 0; k < kObs; ++k) {
          d[kS + k] = META ? s2[k] : s[k];
          d[kS2 + k] = s2[k];
        }
        if constexpr (META)
          d[kS + kObs] = R.X.meta_goal[row];
        else
          d[kS + kObs] = static_cast<float>(R.X.flags ? static_cast<int8_t>(R.X.flags[4 * row]) : R.X.a1[row]);
        d[kS + kObs + 1] = R.X.reward ? R.X.reward[row] : R.X.rew[2 * row];
        if constexpr (GOAL) {
          d[0] = R.X.goal[row];
          d[kS2 - 1] = R.X.next_goal[row];
        }
      }
      __syncthreads();
      const int skip = base >= first ? 0 : static_cast<int>(min<uint64_t>(first - base, total));
      const uint64_t slot0 = (base + skip) % static_cast<uint64_t>(cap);
      const int cnt = total - skip;  // <= cap: at most one wrap
      // the kept rows are one contiguous byte run of the ring (two at a wrap): an 8-byte head
      // when the run starts off 16-byte alignment, then 16-byte stores, then an 8-byte tail
      const int n_a = static_cast<int>(min<uint64_t>(static_cast<uint64_t>(cnt), static_cast<uint64_t>(cap) - slot0));
#pragma unroll
      for (int run = 0; run < 2; ++run) {
        const int r0 = run == 0 ? 0 : n_a, nr = run == 0 ? n_a : cnt - n_a;
        if (nr <= 0) continue;  // uniform
        float* d = rows + (run == 0 ? slot0 : 0) * kRow;
        const float* sp = tile + (skip + r0) * kRow;
        const int nf = nr * kRow;
        const int hd = (reinterpret_cast<uintptr_t>(d) & 15) ? 2 : 0;
        const int nb = (nf - hd) >> 2;
        const int tl = nf - hd - 4 * nb;  // 0 or 2
        if (threadIdx.x == 0 && hd) st_out(reinterpret_cast<f32x2*>(d), *reinterpret_cast<const f32x2*>(sp));
        if (threadIdx.x == 1 && tl)
          st_out(reinterpret_cast<f32x2*>(d + nf - 2), *reinterpret_cast<const f32x2*>(sp + nf - 2));
        const f32x2* s2 = reinterpret_cast<const f32x2*>(sp + hd);  // 8-byte aligned in LDS
        f32x4* d4 = reinterpret_cast<f32x4*>(d + hd);
        for (int k = threadIdx.x; k < nb; k += kRBlock) {
          const f32x2 lo = s2[2 * k], hi = s2[2 * k + 1];
          st_out(d4 + k, f32x4{lo[0], lo[1], hi[0], hi[1]});
        }
      }
    }
    __syncthreads();  // tile and wave counts are reused by the next step
#pragma unroll
    for (int k = 0; k < kObs; ++k) s[k] = o[k];
#pragma unroll
    for (int k = 0; k < kObs; ++k) o[k] = on[k];
  }
}

__global__ __launch_bounds__(kBlock) void replay_sample_kernel(const float* rows,
                                                               const uint64_t* counter, int64_t cap,
                                                               int row_floats, uint64_t seed, uint64_t draw,
                                                               int32_t filled_only, float* out,
                                                               int64_t* idx_out, int64_t batch) {
  const int64_t b = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (b >= batch) return;
  uint64_t m = static_cast<uint64_t>(cap);
  if (filled_only) {
    const uint64_t c = *counter;
    m = c < m ? c : m;
    if (m == 0) m = 1;
  }
  const uint4 u = philox4x32_10(
      make_uint4(static_cast<uint32_t>(b), static_cast<uint32_t>(static_cast<uint64_t>(b) >> 32),
                 static_cast<uint32_t>(draw), static_cast<uint32_t>(draw >> 32)),
      static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32));
  const uint64_t idx = (static_cast<uint64_t>(u.x) * m) >> 32;
  if (idx_out) idx_out[b] = static_cast<int64_t>(idx);
  const f32x2* src = reinterpret_cast<const f32x2*>(rows + idx * row_floats);
  f32x2* dst = reinterpret_cast<f32x2*>(out + b * row_floats);
  for (int k = 0; k < row_floats / 2; ++k) dst[k] = src[k];
}

// memory_counter += k for the stores that keep every transition, so need no scan (the fused goal ring, Rainbow's
// rows): launched behind the store, after every thread of it has read the old counter; the stream orders it
__global__ void counter_add_kernel(uint64_t* counter, uint64_t k) { *counter += k; }

// ============================================================================ the host side of a call
// mg_replay_store is mg_replay_store_many's list of one ring: both fill a ReplayStore, check_replay_store refuses
// what either refuses, in that entry point's order and words, and replay_store_device<MANY> launches.

// the bytes replay_scratch carves for one ring's store (a member store takes `members` of them back to back)
inline size_t replay_scratch_bytes(int64_t n, int32_t num_steps) {
  if (n <= 0 || num_steps <= 0) return 0;
  const int64_t nb = ((n + kRBlock - 1) / kRBlock) * num_steps;
  const int64_t ng = replay_groups(nb);
  return static_cast<size_t>((8 + ng * 8 + nb * 4 + ng * 4 + 7) & ~int64_t{7});
}

struct ReplayStore {  // in the order of mg_replay_store_many's arguments
  float* const* ring;  // `members` rings and their counters (the lone call: the addresses of its two arguments)
  uint64_t* const* counter;
  int32_t members;
  int64_t capacity;
  int32_t row_floats;
  const mg_transitions* tr;
  int64_t n;  // envs of one member
  int32_t T, skip_won;
  void* scratch;
  size_t scratch_bytes;
  int64_t nbx() const { return (n + kRBlock - 1) / kRBlock; }  // a member's write blocks per step,
  int64_t nb() const { return nbx() * T; }                     // write blocks,
  int64_t ng() const { return replay_groups(nb()); }           // and scan groups
  int64_t chunks() const { return (int64_t{T} + kRTChunk - 1) / kRTChunk; }
};

// One walk for both: the member call (`many`) adds the checks of its lists, takes 22-float rows only and checks the
// won mask's alignment. A call with nothing to store returns 0 midway, as replay_store_device does at once.
int check_replay_store(const char* who, const ReplayStore& C, bool many) {
  const auto bad = [who](const char* fmt) { return fail(hipErrorInvalidValue, fmt, who); };
  if (many && !members_ok(C.members)) return bad("%s: need 1 <= members <= 64");
  if (!C.ring || !C.counter || !C.tr || (!many && (!C.ring[0] || !C.counter[0]))) return bad("%s: NULL pointer");
  for (int m = 0; many && m < C.members; ++m) {
    if (!C.ring[m] || !C.counter[m]) return bad("%s: NULL pointer (a member's rows or counter)");
    if (misaligned(C.ring[m], 7) || misaligned(C.counter[m], 7))
      return bad("%s: every member's rows and counter must be 8-byte aligned");
    for (int k = 0; k < m; ++k)
      if (C.ring[k] == C.ring[m] || C.counter[k] == C.counter[m])
        return bad("%s: a ring is listed twice (two members' appends to one ring have no defined order)");
  }
  if (C.capacity < 1) return bad("%s: capacity < 1");
  const mg_transitions& X = *C.tr;
  if (many && (C.row_floats != kRow || X.goal || X.next_goal || X.meta_goal))
    return bad("%s: 22-float rows only: row_floats must be 22 and goal, next_goal, meta_goal NULL");
  if (C.row_floats != (X.goal ? kRowGoal : kRow) || (X.goal != nullptr) != (X.next_goal != nullptr))
    return bad("%s: row_floats must be 22, or 24 with both goal and next_goal set");
  if (X.meta_goal && (X.goal || !X.reward || !X.won_mask))
    return bad("%s: meta_goal (Goal_DQN rows) needs reward and won_mask (no_break) and no goal");
  if (C.n < 0 || C.T < 0) return bad(many ? "%s: n_member < 0 or num_steps < 0" : "%s: n < 0 or num_steps < 0");
  if (many && C.n % 64 != 0)
    return bad("%s: n_member must be a multiple of 64 (a member's won bits begin a word of the mask)");
  if (C.n == 0 || C.T == 0) return 0;
  if (!X.obs_first || !X.obs || !(X.a1 || X.flags) || !X.rew)
    return bad("%s: obs_first, obs, a1 (or flags) and rew are required");
  if ((many ? misaligned(X.won_mask, 7) : misaligned(C.ring[0], 7)) || misaligned(X.obs_first, 7) ||
      misaligned(X.obs, 7) || misaligned(X.final_obs, 7) || misaligned(X.rew, 7) || misaligned(C.scratch, 7))
    return bad(many ? "%s: float buffers, won_mask and scratch must be 8-byte aligned"
                    : "%s: float buffers and scratch must be 8-byte aligned");
  if (misaligned(X.goal, 3) || misaligned(X.next_goal, 3) || misaligned(X.reward, 3))  // member call: no goals
    return bad(many ? "%s: reward must be 4-byte aligned" : "%s: goal, next_goal and reward must be 4-byte aligned");
  if (C.nbx() > 0x7fffffff || C.ng() > 0x7fffffff)
    return bad(many ? "%s: n_member * num_steps exceeds the grid limit" : "%s: n * num_steps exceeds the grid limit");
  if (!C.scratch || C.scratch_bytes < static_cast<size_t>(C.members) * replay_scratch_bytes(C.n, C.T))
    return bad(many ? "%s: scratch smaller than mg_replay_scratch_many_bytes(n_member, num_steps, members)"
                    : "%s: scratch smaller than mg_replay_scratch_bytes(n, num_steps)");
  return C.chunks() > 65535 ? bad("%s: num_steps too large") : 0;
}

// A checked store's three launches: the scan, the group scan, the write, the member in each grid's last dimension;
// the lone call is the batch of one member (N = n: the same won-mask words). A template, so that each entry point
// first names its write instances where it stands: they come out in the code object in the order of first naming.
template <bool MANY>
int replay_store_device(const char* who, const ReplayStore& C, hipStream_t st) {
  if (C.n == 0 || C.T == 0) return 0;
  const unsigned nbx = static_cast<unsigned>(C.nbx()), ng = static_cast<unsigned>(C.ng());
  const unsigned chunks = static_cast<unsigned>(C.chunks()), M = static_cast<unsigned>(C.members);
  const int64_t N = C.n * C.members;  // below: Goal_DQN rows (meta_goal) keep the steps that broke
  const ReplayIn R{*C.tr, C.n, (N + 63) >> 6, C.nbx(), C.nb(), C.T, C.tr->meta_goal ? 1 : C.skip_won};
  if constexpr (!MANY) {
    const ReplayScratch S = replay_scratch(C.scratch, C.nb());
    hipLaunchKernelGGL(replay_scan_kernel, dim3(ng), dim3(64), 0, st, R, S);
    hipLaunchKernelGGL(replay_group_scan_kernel, dim3(1), dim3(64), 0, st, S, C.ng(), C.counter[0]);
    auto write_kernel = replay_write_kernel<1>;  // rows with goal and next_goal
    if (!R.X.goal) write_kernel = R.X.meta_goal ? replay_write_kernel<2> : replay_write_kernel<0>;
    hipLaunchKernelGGL(write_kernel, dim3(nbx, chunks), dim3(kRBlock), 0, st, R, S, C.counter[0], C.ring[0],
                       C.capacity);
  } else {
    ReplayMany A{R, N, static_cast<int64_t>(replay_scratch_bytes(C.n, C.T)), static_cast<uint8_t*>(C.scratch),
                 C.capacity, C.ng()};
    std::copy(C.ring, C.ring + C.members, A.ring);
    std::copy(C.counter, C.counter + C.members, A.counter);
    hipLaunchKernelGGL(replay_scan_many_kernel, dim3(ng, M), dim3(64), 0, st, A);
    hipLaunchKernelGGL(replay_group_scan_many_kernel, dim3(M), dim3(64), 0, st, A);
    hipLaunchKernelGGL((replay_write_kernel<0, true>), dim3(nbx, chunks, M), dim3(kRBlock), 0, st, A, ReplayScratch{},
                       static_cast<const uint64_t*>(nullptr), static_cast<float*>(nullptr), int64_t{0});
  }
  return finish_launch(who);
}

}  // namespace
