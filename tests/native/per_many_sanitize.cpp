// Host sanitizer driver for the prioritized population's entry points (test infrastructure):
// tests/test_per_many_sanitize.py compiles merging_hip.hip with -Xarch_host -fsanitize=address / undefined and
// links this file. mg_host_per_store_many and mg_host_rainbow_learn_prioritized_many run with three members at
// batch 33 on exactly sized heap buffers -- rings of 13 rows under trees of 16 leaves, one store larger than the
// ring -- so the sanitizers see every access they make: a member's scratch slice, its idx and w behind the
// learner's sections, its rows of idx_out and weight_out, its tree. Each member is then compared with the lone
// host calls on buffers of its own. The device entry points only get as far as their argument checks (nothing
// here launches a kernel). Any sanitizer report aborts the run.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "merging_hip.h"

// `count` elements at a 16-byte boundary, not one more (posix_memalign keeps the size exact for ASan).
template <class T>
static T* exact(size_t count) {
  void* p = nullptr;
  if (posix_memalign(&p, 16, count * sizeof(T)) != 0 || !p) std::abort();
  std::memset(p, 0, count * sizeof(T));
  return static_cast<T*>(p);
}

static uint32_t g_lcg = 977u;
static float unit() {  // in [-1, 1)
  g_lcg = g_lcg * 1664525u + 1013904223u;
  return static_cast<float>(static_cast<int32_t>(g_lcg >> 8) - (1 << 23)) / static_cast<float>(1 << 23);
}

static int expect_error(int rc, const char* needle, const char* what) {
  if (rc == 0 || !std::strstr(mg_last_error(), needle)) {
    std::printf("FAIL: %s: rc %d, message '%s'\n", what, rc, mg_last_error());
    return 1;
  }
  return 0;
}

constexpr int kParams = 58884, kEps = 28210, kFactors = 1124, kRow = 24, kObs = 10;
constexpr int kLearner = 4 * kParams + 2 * kEps + 52;
constexpr int M = 3, B = 33, U = 2, N = 5, T = 4;
constexpr int64_t kCap = 13;

struct Replay {
  float* rows;
  uint64_t* counter;
  void* tree;
};
static Replay replay(size_t tree_bytes, uint64_t start) {
  Replay r{exact<float>(kCap * kRow), exact<uint64_t>(1), exact<char>(tree_bytes)};
  *r.counter = start;
  if (mg_host_per_init(r.tree, tree_bytes, kCap) != 0) std::abort();
  return r;
}

// Two stores of [T, M * N] transitions (20 per member: more than the ring) into three members at different
// counters, two updates of all of them with every output, and the same through the lone calls.
static int host_run() {
  int bad = 0;
  const size_t tb = mg_per_bytes(kCap);
  const double alpha[M] = {1.0, 0.6, 0.8};
  const uint64_t start[M] = {0, 7, 11};
  Replay many[M], lone[M];
  for (int m = 0; m < M; ++m) many[m] = replay(tb, start[m]), lone[m] = replay(tb, start[m]);
  float* obs_first = exact<float>(M * N * kObs);
  float* obs = exact<float>(static_cast<size_t>(T) * M * N * kObs);
  float* final_obs = exact<float>(static_cast<size_t>(T) * M * N * kObs);
  float* rew = exact<float>(static_cast<size_t>(T) * M * N * 2);
  uint8_t* flags = exact<uint8_t>(static_cast<size_t>(T) * M * N * 4);
  // a member's contiguous copy of its slice, for the lone store
  float* s_first = exact<float>(N * kObs);
  float* s_obs = exact<float>(static_cast<size_t>(T) * N * kObs);
  float* s_final = exact<float>(static_cast<size_t>(T) * N * kObs);
  float* s_rew = exact<float>(static_cast<size_t>(T) * N * 2);
  uint8_t* s_flags = exact<uint8_t>(static_cast<size_t>(T) * N * 4);
  float* rows_p[M];
  uint64_t* counters_p[M];
  void* trees_p[M];
  for (int m = 0; m < M; ++m) rows_p[m] = many[m].rows, counters_p[m] = many[m].counter, trees_p[m] = many[m].tree;
  for (int round = 0; round < 2; ++round) {
    for (int i = 0; i < M * N * kObs; ++i) obs_first[i] = 3.0f * unit();
    for (int i = 0; i < T * M * N * kObs; ++i) obs[i] = 3.0f * unit(), final_obs[i] = 3.0f * unit();
    for (int i = 0; i < T * M * N; ++i) {
      rew[2 * i] = i % 5 == 0 ? 10.0f : i % 5 == 1 ? -25.0f : 0.4f * static_cast<float>(i % 9);
      flags[4 * i] = static_cast<uint8_t>(i % 5), flags[4 * i + 2] = static_cast<uint8_t>(i % 3 == 0);
    }
    mg_transitions X{};
    X.obs_first = obs_first, X.obs = obs, X.final_obs = final_obs, X.rew = rew, X.flags = flags;
    if (mg_host_per_store_many(rows_p, counters_p, M, kCap, &X, N, T, trees_p, tb, alpha) != 0) {
      std::printf("FAIL: mg_host_per_store_many: %s\n", mg_last_error());
      ++bad;
    }
    for (int m = 0; m < M; ++m) {
      std::memcpy(s_first, obs_first + m * N * kObs, sizeof(float) * N * kObs);
      for (int t = 0; t < T; ++t) {
        const size_t at = static_cast<size_t>(t) * M * N + m * N;
        std::memcpy(s_obs + t * N * kObs, obs + at * kObs, sizeof(float) * N * kObs);
        std::memcpy(s_final + t * N * kObs, final_obs + at * kObs, sizeof(float) * N * kObs);
        std::memcpy(s_rew + t * N * 2, rew + at * 2, sizeof(float) * N * 2);
        std::memcpy(s_flags + t * N * 4, flags + at * 4, N * 4);
      }
      mg_transitions S{};
      S.obs_first = s_first, S.obs = s_obs, S.final_obs = s_final, S.rew = s_rew, S.flags = s_flags;
      if (mg_host_per_store(lone[m].rows, lone[m].counter, kCap, &S, N, T, lone[m].tree, tb, alpha[m]) != 0) ++bad;
      if (*many[m].counter != *lone[m].counter || std::memcmp(many[m].rows, lone[m].rows, sizeof(float) * kCap * kRow) ||
          std::memcmp(many[m].tree, lone[m].tree, tb)) {
        std::printf("FAIL: store %d, member %d differs from mg_host_per_store\n", round, m);
        ++bad;
      }
    }
  }
  float* L = exact<float>(static_cast<size_t>(M) * kLearner);
  for (int m = 0; m < M; ++m) {
    float* l = L + static_cast<size_t>(m) * kLearner;
    for (int i = 0; i < kParams; ++i) l[i] = 0.1f * unit();
    std::memcpy(l + kParams, l, sizeof(float) * kParams);
    for (int i = 0; i < 2 * kEps; ++i) l[4 * kParams + i] = unit();
    for (int i = 0; i < 51; ++i) l[4 * kParams + 2 * kEps + i] = -10.0f + 0.4f * static_cast<float>(i);
  }
  float* L1 = exact<float>(static_cast<size_t>(M) * kLearner);
  std::memcpy(L1, L, sizeof(float) * M * kLearner);
  mg_dqn_member* member = exact<mg_dqn_member>(M);
  mg_per_member* per = exact<mg_per_member>(M);
  for (int m = 0; m < M; ++m) {
    member[m] = mg_dqn_member{many[m].rows, many[m].counter, 5u + 11u * m, static_cast<uint64_t>(3 * m),
                              static_cast<uint64_t>(m), {0.001 * (m + 1), 0.99 - 0.01 * m, 0.9, 0.999, 1e-8, 1, 0}};
    per[m] = mg_per_member{many[m].tree, alpha[m], m == 1 ? 1.0 : 0.4, 1e-5 * m};
  }
  float* noise = exact<float>(static_cast<size_t>(U) * M * 2 * kFactors);
  for (int i = 0; i < U * M * 2 * kFactors; ++i) noise[i] = unit();
  const size_t one = mg_rainbow_learn_prioritized_scratch_bytes(B), sbytes = M * one;
  char* scratch = exact<char>(sbytes);
  float* loss = exact<float>(U * M);
  float* rows = exact<float>(static_cast<size_t>(U) * M * B * kRow);
  float* proj = exact<float>(static_cast<size_t>(U) * M * B * 51);
  float* grads = exact<float>(static_cast<size_t>(U) * M * kParams);
  int64_t* idx = exact<int64_t>(static_cast<size_t>(U) * M * B);
  float* w = exact<float>(static_cast<size_t>(U) * M * B);
  if (mg_host_rainbow_learn_prioritized_many(L, member, M, kCap, B, U, noise, loss, rows, proj, grads, scratch, sbytes,
                                             per, tb, idx, w) != 0) {
    std::printf("FAIL: mg_host_rainbow_learn_prioritized_many: %s\n", mg_last_error());
    ++bad;
  }
  // the lone learner per member: its slice of the noise, its own outputs
  float* n1 = exact<float>(static_cast<size_t>(U) * 2 * kFactors);
  char* s1 = exact<char>(one);
  float* loss1 = exact<float>(U);
  int64_t* idx1 = exact<int64_t>(static_cast<size_t>(U) * B);
  float* w1 = exact<float>(static_cast<size_t>(U) * B);
  for (int m = 0; m < M; ++m) {
    for (int u = 0; u < U; ++u)
      std::memcpy(n1 + static_cast<size_t>(u) * 2 * kFactors, noise + (static_cast<size_t>(u) * M + m) * 2 * kFactors,
                  sizeof(float) * 2 * kFactors);
    float* l1 = L1 + static_cast<size_t>(m) * kLearner;
    const mg_dqn_hyper h = member[m].hyper;
    if (mg_host_rainbow_learn_prioritized(l1, lone[m].rows, lone[m].counter, kCap, B, U, 3 * m, 5u + 11u * m, m, &h, n1,
                                          loss1, nullptr, nullptr, nullptr, s1, one, lone[m].tree, tb, alpha[m],
                                          per[m].beta, per[m].prio_eps, idx1, w1) != 0)
      ++bad;
    bool same = std::memcmp(l1, L + static_cast<size_t>(m) * kLearner, sizeof(float) * kLearner) == 0 &&
                std::memcmp(lone[m].tree, many[m].tree, tb) == 0;
    for (int u = 0; u < U; ++u) {
      same = same && std::memcmp(loss1 + u, loss + u * M + m, sizeof(float)) == 0 &&
             std::memcmp(idx1 + u * B, idx + (static_cast<size_t>(u) * M + m) * B, sizeof(int64_t) * B) == 0 &&
             std::memcmp(w1 + u * B, w + (static_cast<size_t>(u) * M + m) * B, sizeof(float) * B) == 0;
      for (int b = 0; b < B; ++b) {
        const int64_t i = idx[(static_cast<size_t>(u) * M + m) * B + b];
        const float wb = w[(static_cast<size_t>(u) * M + m) * B + b];
        if (i < 0 || i >= kCap || !(wb > 0.0f && wb <= 1.0f)) same = false;
      }
    }
    if (!same || !std::isfinite(loss[m])) {
      std::printf("FAIL: member %d differs from mg_host_rainbow_learn_prioritized\n", m);
      ++bad;
    }
    if (member[m].first_update != static_cast<uint64_t>(3 * m + U) || member[m].first_draw != static_cast<uint64_t>(m + U))
      ++bad;
  }
  // no outputs, then no update: needs no noise, moves no counter
  if (mg_host_rainbow_learn_prioritized_many(L, member, M, kCap, B, 1, noise, nullptr, nullptr, nullptr, nullptr, scratch,
                                             sbytes, per, tb, nullptr, nullptr) != 0)
    ++bad;
  if (mg_host_rainbow_learn_prioritized_many(L, member, M, kCap, B, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                                             scratch, sbytes, per, tb, nullptr, nullptr) != 0)
    ++bad;
  if (member[0].first_update != static_cast<uint64_t>(U + 1)) ++bad;
  for (int m = 0; m < M; ++m)
    for (void* p : {static_cast<void*>(many[m].rows), static_cast<void*>(many[m].counter), many[m].tree,
                    static_cast<void*>(lone[m].rows), static_cast<void*>(lone[m].counter), lone[m].tree})
      std::free(p);
  for (void* p : {static_cast<void*>(obs_first), static_cast<void*>(obs), static_cast<void*>(final_obs),
                  static_cast<void*>(rew), static_cast<void*>(flags), static_cast<void*>(s_first),
                  static_cast<void*>(s_obs), static_cast<void*>(s_final), static_cast<void*>(s_rew),
                  static_cast<void*>(s_flags), static_cast<void*>(L), static_cast<void*>(L1),
                  static_cast<void*>(member), static_cast<void*>(per), static_cast<void*>(noise),
                  static_cast<void*>(scratch), static_cast<void*>(loss), static_cast<void*>(rows),
                  static_cast<void*>(proj), static_cast<void*>(grads), static_cast<void*>(idx), static_cast<void*>(w),
                  static_cast<void*>(n1), static_cast<void*>(s1), static_cast<void*>(loss1), static_cast<void*>(idx1),
                  static_cast<void*>(w1)})
    std::free(p);
  return bad;
}

// The device entry points refuse before anything is launched or read; the host twins refuse the same.
static int refusals() {
  int bad = 0;
  float* t = exact<float>(64);
  float* t2 = exact<float>(64);
  uint64_t* c = exact<uint64_t>(8);
  char* big = exact<char>(256);
  char* tree0 = exact<char>(64);
  char* tree1 = exact<char>(64);
  const size_t sb = 2 * mg_rainbow_learn_prioritized_scratch_bytes(32);
  const size_t tb = mg_rainbow_learn_many_table_bytes(2);
  const size_t pb = mg_per_bytes(10);
  const mg_dqn_hyper h = {0.001, 0.99, 0.9, 0.999, 1e-8, 1, 0};
  mg_dqn_member ok[2] = {{t, c, 1, 0, 0, h}, {t2, c + 1, 2, 0, 0, h}};
  mg_dqn_member same_rows[2] = {{t, c, 1, 0, 0, h}, {t, c + 1, 2, 0, 0, h}};
  const mg_per_member good[2] = {{tree0, 0.6, 0.4, 1e-5}, {tree1, 0.6, 0.4, 1e-5}};
  auto with = [&](int m, void* tree, double alpha, double beta, double eps) {
    struct Two {
      mg_per_member p[2];
    } two{{good[0], good[1]}};
    two.p[m] = mg_per_member{tree, alpha, beta, eps};
    return two;
  };
  for (int which = 0; which < 2; ++which) {
    auto call = [&](mg_dqn_member* mem, int b, const mg_per_member* per, size_t tree_bytes, int64_t* io, float* wo,
                    size_t bytes) {
      return which ? mg_host_rainbow_learn_prioritized_many(t, mem, 2, 10, b, 1, t, nullptr, nullptr, nullptr, nullptr, big,
                                                            bytes, per, tree_bytes, io, wo)
                   : mg_rainbow_learn_prioritized_many(t, big, tb, mem, 2, 10, b, 1, t, nullptr, nullptr, nullptr, nullptr,
                                                       nullptr, 0, big, bytes, per, tree_bytes, io, wo, nullptr);
    };
    bad += expect_error(call(ok, 0, good, pb, nullptr, nullptr, sb), "batch", "learn: batch 0 comes first");
    bad += expect_error(call(ok, 32, nullptr, pb, nullptr, nullptr, sb), "NULL pointer", "learn: NULL per");
    bad += expect_error(call(ok, 32, with(1, nullptr, 0.6, 0.4, 0).p, pb, nullptr, nullptr, sb), "member 1: NULL pointer (tree)",
                        "learn: member 1 NULL tree");
    bad += expect_error(call(ok, 32, with(0, tree0 + 8, 0.6, 0.4, 0).p, pb, nullptr, nullptr, sb), "member 0: the tree buffer",
                        "learn: member 0 tree misaligned");
    bad += expect_error(call(ok, 32, good, pb - 1, nullptr, nullptr, sb), "tree buffer smaller", "learn: tree short");
    bad += expect_error(call(ok, 32, with(1, tree1, 0.0, 0.4, 0).p, pb, nullptr, nullptr, sb), "member 1: need alpha > 0",
                        "learn: alpha 0");
    bad += expect_error(call(ok, 32, with(0, tree0, 0.6, 0.0, 0).p, pb, nullptr, nullptr, sb), "member 0: need beta > 0",
                        "learn: beta 0");
    bad += expect_error(call(ok, 32, with(1, tree1, 0.6, 0.4, -1e-9).p, pb, nullptr, nullptr, sb),
                        "member 1: need prio_eps >= 0", "learn: prio_eps < 0");
    bad += expect_error(call(ok, 32, good, pb, reinterpret_cast<int64_t*>(big + 4), nullptr, sb), "idx_out must be",
                        "learn: idx_out misaligned");
    bad += expect_error(call(ok, 32, good, pb, nullptr, reinterpret_cast<float*>(big + 2), sb), "idx_out must be",
                        "learn: weight_out misaligned");
    bad += expect_error(call(ok, 32, good, pb, nullptr, nullptr, sb - 1), "mg_rainbow_learn_prioritized_scratch_bytes",
                        "learn: scratch short");
    bad += expect_error(call(ok, 32, with(1, tree0, 0.6, 0.4, 0).p, pb, nullptr, nullptr, sb), "member 1: its tree or rows",
                        "learn: one tree twice");
    bad += expect_error(call(same_rows, 32, good, pb, nullptr, nullptr, sb), "member 1: its tree or rows",
                        "learn: one rows buffer twice");
  }
  bad += expect_error(mg_rainbow_learn_prioritized_many(t, nullptr, tb, ok, 2, 10, 32, 1, t, nullptr, nullptr, nullptr,
                                                        nullptr, nullptr, 0, big, sb, nullptr, pb, nullptr, nullptr, nullptr),
                      "table is NULL", "learn: the table comes before the trees");
  for (int m = 0; m < 2; ++m)
    if (ok[m].first_update != 0 || ok[m].first_draw != 0) ++bad;  // a refused call moves no counter
  // the store
  mg_transitions X{};
  float* rows2[2] = {t, t2};
  float* rows_same[2] = {t, t};
  uint64_t* counters2[2] = {c, c + 1};
  void* trees2[2] = {tree0, tree1};
  void* trees_null[2] = {tree0, nullptr};
  void* trees_odd[2] = {tree0, tree1 + 8};
  void* trees_same[2] = {tree0, tree0};
  const double a2[2] = {0.6, 1.0}, a_bad[2] = {0.6, 0.0};
  for (int which = 0; which < 2; ++which) {
    // n = 0: the rings' walk ends before the transitions' arrays are asked for, and the trees' checks follow
    auto call = [&](float* const* rows, int members, void* const* trees, size_t tree_bytes, const double* alpha,
                    int64_t n = 0) {
      return which ? mg_host_per_store_many(rows, counters2, members, 10, &X, n, 2, trees, tree_bytes, alpha)
                   : mg_per_store_many(rows, counters2, members, 10, &X, n, 2, trees, tree_bytes, alpha, nullptr);
    };
    bad += expect_error(call(rows2, 0, trees2, pb, a2), "members", "store: 0 members");
    bad += expect_error(call(rows_same, 2, trees2, pb, a2), "listed twice", "store: one ring twice");
    bad += expect_error(call(rows2, 2, nullptr, pb, a2), "NULL pointer", "store: NULL trees");
    bad += expect_error(call(rows2, 2, trees2, pb, nullptr), "NULL pointer", "store: NULL alpha");
    bad += expect_error(call(rows2, 2, trees_null, pb, a2), "member 1: NULL pointer (tree)", "store: member 1 NULL tree");
    bad += expect_error(call(rows2, 2, trees_odd, pb, a2), "member 1: the tree buffer", "store: member 1 misaligned");
    bad += expect_error(call(rows2, 2, trees2, pb - 1, a2), "tree buffer smaller", "store: tree short");
    bad += expect_error(call(rows2, 2, trees2, pb, a_bad), "member 1: need alpha > 0", "store: alpha 0");
    bad += expect_error(call(rows2, 2, trees_same, pb, a2), "member 1: its tree is another", "store: one tree twice");
    bad += expect_error(call(rows2, 2, trees2, pb, a2, 4), "obs_first, obs", "store: no arrays");
    if (call(rows2, 2, trees2, pb, a2) != 0) ++bad;  // nothing to store: a no-op
  }
  if (c[0] != 0 || c[1] != 0) ++bad;
  for (void* p : {static_cast<void*>(t), static_cast<void*>(t2), static_cast<void*>(c), static_cast<void*>(big),
                  static_cast<void*>(tree0), static_cast<void*>(tree1)})
    std::free(p);
  return bad;
}

int main() {
  int bad = 0;
  if (mg_abi_version() != 21) ++bad;
  bad += host_run();
  bad += refusals();
  std::printf("prioritized population sanitizer run: %d failures\n", bad);
  return bad ? 1 : 0;
}
