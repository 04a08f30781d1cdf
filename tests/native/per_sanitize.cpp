// Host sanitizer driver for the prioritized replay entry points (test infrastructure):
// tests/test_per_sanitize.py links this file against merging_hip.hip compiled with -Xarch_host
// -fsanitize=address / undefined. The host twins mg_host_per_* and mg_host_rainbow_learn_prioritized run on
// exactly sized heap buffers, so the sanitizers see every access they make; the device entry points only get as
// far as their argument checks (nothing here launches a kernel). Any sanitizer report aborts the run.
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

static uint32_t g_lcg = 4242u;
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

constexpr int kRow = 24, kParams = 58884, kEps = 28210, kFactors = 1124;
constexpr int kLearner = 4 * kParams + 2 * kEps + 52;
static const mg_dqn_hyper kHyper = {0.001, 0.99, 0.9, 0.999, 1e-8, 1, 0};

struct Steps {  // T steps of n envs, exactly sized
  float *obs_first, *obs, *rew;
  int8_t* a1;
  uint8_t* done;
  mg_transitions X;
};
static Steps steps(int64_t n, int T) {
  Steps S{};
  S.obs_first = exact<float>(n * 10);
  S.obs = exact<float>(T * n * 10);
  S.rew = exact<float>(T * n * 2);
  S.a1 = exact<int8_t>(T * n);
  S.done = exact<uint8_t>(T * n);
  for (int64_t i = 0; i < n * 10; ++i) S.obs_first[i] = unit();
  for (int64_t i = 0; i < T * n * 10; ++i) S.obs[i] = unit();
  for (int64_t i = 0; i < T * n; ++i)
    S.rew[2 * i] = 3.0f * unit(), S.a1[i] = static_cast<int8_t>(i % 5), S.done[i] = static_cast<uint8_t>(i % 7 == 0);
  S.X.obs_first = S.obs_first, S.X.obs = S.obs, S.X.rew = S.rew, S.X.a1 = S.a1, S.X.done = S.done;
  return S;
}
static void release(Steps& S) {
  std::free(S.obs_first), std::free(S.obs), std::free(S.rew), std::free(S.a1), std::free(S.done);
}

// every inner node is the op of its children
static int consistent(const double* tree, int64_t C) {
  const double *sum = tree, *mn = tree + 2 * C;
  for (int64_t i = 1; i < C; ++i)
    if (sum[i] != sum[2 * i] + sum[2 * i + 1] || mn[i] != std::fmin(mn[2 * i], mn[2 * i + 1])) return 1;
  return 0;
}

// Stores that wrap and exceed the ring, samples and updates with duplicates and rejected entries, at
// capacities 1 (a tree of one leaf), 13 and 3000; then three prioritized updates of the learner.
static int host_run() {
  int bad = 0;
  for (int64_t cap : {int64_t{1}, int64_t{13}, int64_t{3000}}) {
    int64_t C = 1;
    while (C < cap) C *= 2;
    const size_t tb = mg_per_bytes(cap);
    if (tb != sizeof(double) * (4 * C + 2)) ++bad;
    double* tree = exact<double>(4 * C + 2);
    float* rows = exact<float>(cap * kRow);
    uint64_t* counter = exact<uint64_t>(1);
    if (mg_host_per_init(tree, tb, cap) != 0) ++bad;
    const int B = 33;
    int64_t* idx = exact<int64_t>(B);
    float* w = exact<float>(B);
    float* pr = exact<float>(B);
    if (mg_host_per_sample(tree, tb, counter, cap, 0.4, 1, 0, B, idx, w) != 0) ++bad;  // empty: slot 0, weight 1
    for (int b = 0; b < B; ++b)
      if (idx[b] != 0 || w[b] != 1.0f) ++bad;
    const int64_t ns[3] = {1, 5, cap + 7};
    for (int r = 0; r < 3; ++r) {
      Steps S = steps(ns[r], 3);
      if (mg_host_per_store(rows, counter, cap, &S.X, ns[r], 3, tree, tb, 0.6) != 0) {
        std::printf("FAIL: mg_host_per_store: %s\n", mg_last_error());
        ++bad;
      }
      release(S);
      bad += consistent(tree, C);
      for (int d = 0; d < 3; ++d) {
        if (mg_host_per_sample(tree, tb, counter, cap, 0.4, 7, 10 * r + d, B, idx, w) != 0) ++bad;
        for (int b = 0; b < B; ++b) {
          if (idx[b] < 0 || idx[b] >= cap || !(w[b] > 0.0f && w[b] <= 1.0f)) ++bad;
          pr[b] = 0.001f + 4.0f * std::fabs(unit());
        }
        pr[3] = 0.0f, pr[4] = NAN, idx[5] = -1, idx[6] = cap, idx[7] = int64_t{1} << 40;  // left out
        if (mg_host_per_update(tree, tb, counter, cap, 0.6, idx, pr, B) != 0) ++bad;
        bad += consistent(tree, C);
      }
    }
    double total = -1.0;
    if (mg_host_per_total(tree, tb, counter, cap, &total) != 0 || !(total >= 0.0)) ++bad;
    if (*counter != static_cast<uint64_t>(3 * (1 + 5 + cap + 7))) ++bad;
    for (void* p : {static_cast<void*>(tree), static_cast<void*>(rows), static_cast<void*>(counter),
                    static_cast<void*>(idx), static_cast<void*>(w), static_cast<void*>(pr)})
      std::free(p);
  }
  const double x[4] = {1e-5, 1.0, 3.5, 10.0}, y[4] = {0.6, -0.4, 1.0, -1.0};
  double out[4];
  if (mg_host_per_pow(x, y, out, 4) != 0) ++bad;
  for (int i = 0; i < 4; ++i)
    if (!(std::fabs(out[i] - std::pow(x[i], y[i])) <= 5e-15 * std::pow(x[i], y[i]))) ++bad;
  const double u = mg_host_per_uniform(3, 4, 5);
  if (!(u >= 0.0 && u < 1.0)) ++bad;

  // the learner: batch 33 on a partly filled ring of 48 slots, every optional output, then none
  const int B = 33, U = 3;
  const int64_t cap = 48;
  float* L = exact<float>(kLearner);
  for (int i = 0; i < 2 * kParams; ++i) L[i] = 0.1f * unit();
  std::memcpy(L + kParams, L, sizeof(float) * kParams);
  for (int i = 0; i < 2 * kEps; ++i) L[4 * kParams + i] = unit();
  for (int i = 0; i < 51; ++i) L[4 * kParams + 2 * kEps + i] = -10.0f + 0.4f * static_cast<float>(i);
  const size_t tb = mg_per_bytes(cap);
  double* tree = exact<double>(tb / sizeof(double));
  float* rows = exact<float>(cap * kRow);
  uint64_t* counter = exact<uint64_t>(1);
  if (mg_host_per_init(tree, tb, cap) != 0) ++bad;
  Steps S = steps(8, 5);
  if (mg_host_per_store(rows, counter, cap, &S.X, 8, 5, tree, tb, 0.6) != 0) ++bad;
  release(S);
  float* noise = exact<float>(U * 2 * kFactors);
  for (int i = 0; i < U * 2 * kFactors; ++i) noise[i] = unit();
  const size_t sb = mg_rainbow_learn_prioritized_scratch_bytes(B);
  char* scratch = exact<char>(sb);
  float* loss = exact<float>(U);
  float* orows = exact<float>(U * B * kRow);
  float* proj = exact<float>(U * B * 51);
  float* grads = exact<float>(static_cast<size_t>(U) * kParams);
  int64_t* idx = exact<int64_t>(U * B);
  float* w = exact<float>(U * B);
  if (mg_host_rainbow_learn_prioritized(L, rows, counter, cap, B, U, 0, 5, 0, &kHyper, noise, loss, orows, proj, grads,
                                        scratch, sb, tree, tb, 0.6, 0.4, 1e-5, idx, w) != 0) {
    std::printf("FAIL: mg_host_rainbow_learn_prioritized: %s\n", mg_last_error());
    ++bad;
  }
  for (int u = 0; u < U; ++u)
    if (!std::isfinite(loss[u])) ++bad;
  for (int i = 0; i < U * B; ++i)
    if (idx[i] < 0 || idx[i] >= 39 || !(w[i] > 0.0f && w[i] <= 1.0f)) ++bad;  // 40 stored: the newest is not drawn
  bad += consistent(tree, 64);
  if (mg_host_rainbow_learn_prioritized(L, rows, counter, cap, B, 1, 3, 5, 3, &kHyper, noise, nullptr, nullptr, nullptr,
                                        nullptr, scratch, sb, tree, tb, 0.6, 0.4, 1e-5, nullptr, nullptr) != 0)
    ++bad;
  for (void* p : {static_cast<void*>(L), static_cast<void*>(tree), static_cast<void*>(rows), static_cast<void*>(counter),
                  static_cast<void*>(noise), static_cast<void*>(scratch), static_cast<void*>(loss),
                  static_cast<void*>(orows), static_cast<void*>(proj), static_cast<void*>(grads),
                  static_cast<void*>(idx), static_cast<void*>(w)})
    std::free(p);
  return bad;
}

// The entry points refuse before anything is launched or read.
static int refusals() {
  int bad = 0;
  float* t = exact<float>(64);
  uint64_t* c = exact<uint64_t>(1);
  int64_t* idx = exact<int64_t>(8);
  const size_t tb = mg_per_bytes(13);
  double* tree = exact<double>(tb / sizeof(double));
  char* big = exact<char>(64);
  mg_transitions X{};
  X.obs_first = X.obs = X.rew = t;
  X.a1 = reinterpret_cast<const int8_t*>(t);
  bad += expect_error(mg_per_init(nullptr, tb, 13, nullptr), "NULL", "init: NULL");
  bad += expect_error(mg_per_init(tree, tb - 1, 13, nullptr), "smaller", "init: short");
  bad += expect_error(mg_per_init(tree + 1, tb, 13, nullptr), "aligned", "init: misaligned");
  bad += expect_error(mg_host_per_init(tree, tb, 0), "capacity", "init: capacity 0");
  bad += expect_error(mg_per_store(t, c, 13, &X, 4, 2, nullptr, tb, 0.6, nullptr), "NULL", "store: NULL tree");
  bad += expect_error(mg_per_store(nullptr, c, 13, &X, 4, 2, tree, tb, 0.6, nullptr), "NULL", "store: NULL rows");
  bad += expect_error(mg_per_store(t, c, 13, &X, 4, 2, tree, tb, 0.0, nullptr), "alpha", "store: alpha 0");
  bad += expect_error(mg_per_store(t, c, 13, &X, 4, 2, tree, tb - 8, 0.6, nullptr), "smaller", "store: short tree");
  bad += expect_error(mg_host_per_store(t, c, 13, &X, 4, -2, tree, tb, 0.6), "num_steps < 0", "store: num_steps < 0");
  bad += expect_error(mg_per_sample(tree, tb, c, 13, 0.0, 0, 0, 8, idx, t, nullptr), "beta", "sample: beta 0");
  bad += expect_error(mg_per_sample(tree, tb, c, 13, 0.4, 0, 0, 0, idx, t, nullptr), "batch", "sample: batch 0");
  bad += expect_error(mg_per_sample(tree, tb, c, 13, 0.4, 0, 0, 1025, idx, t, nullptr), "batch", "sample: batch 1025");
  bad += expect_error(mg_per_sample(tree, tb, nullptr, 13, 0.4, 0, 0, 8, idx, t, nullptr), "NULL", "sample: NULL counter");
  bad += expect_error(mg_host_per_sample(tree, tb, c, 13, 0.4, 0, 0, 8, nullptr, t), "NULL", "sample: NULL idx_out");
  bad += expect_error(mg_host_per_sample(tree, tb, c, 17, 0.4, 0, 0, 8, idx, t), "smaller", "sample: short tree");
  bad += expect_error(mg_per_update(tree, tb, c, 13, -0.6, idx, t, 8, nullptr), "alpha", "update: alpha < 0");
  bad += expect_error(mg_per_update(tree, tb, c, 13, 0.6, nullptr, t, 8, nullptr), "NULL", "update: NULL idx");
  bad += expect_error(mg_per_update(tree, tb, c, 13, 0.6, idx, t, 2000, nullptr), "batch", "update: batch 2000");
  bad += expect_error(mg_host_per_update(tree, tb, c, 13, 0.6, idx, reinterpret_cast<float*>(big + 2), 8), "aligned",
                      "update: priority misaligned");
  const size_t sb = mg_rainbow_learn_prioritized_scratch_bytes(32);
  auto learn = [&](int which, void* tr, size_t tbytes, double alpha, double beta, double eps, size_t sbytes) {
    return which ? mg_host_rainbow_learn_prioritized(t, t, c, 13, 32, 1, 0, 0, 0, &kHyper, t, nullptr, nullptr, nullptr,
                                                     nullptr, big, sbytes, tr, tbytes, alpha, beta, eps, nullptr, nullptr)
                 : mg_rainbow_learn_prioritized(t, t, c, 13, 32, 1, 0, 0, 0, &kHyper, t, nullptr, nullptr, nullptr, nullptr,
                                                nullptr, big, sbytes, tr, tbytes, alpha, beta, eps, nullptr, nullptr,
                                                nullptr);
  };
  for (int which = 0; which < 2; ++which) {
    bad += expect_error(learn(which, nullptr, tb, 0.6, 0.4, 1e-5, sb), "NULL", "learn: NULL tree");
    bad += expect_error(learn(which, tree, tb - 1, 0.6, 0.4, 1e-5, sb), "tree buffer smaller", "learn: short tree");
    bad += expect_error(learn(which, tree, tb, 0.0, 0.4, 1e-5, sb), "alpha", "learn: alpha 0");
    bad += expect_error(learn(which, tree, tb, 0.6, 0.0, 1e-5, sb), "beta > 0", "learn: beta 0");
    bad += expect_error(learn(which, tree, tb, 0.6, 0.4, -1.0, sb), "prio_eps", "learn: prio_eps < 0");
    bad += expect_error(learn(which, tree, tb, 0.6, 0.4, 1e-5, sb - 1), "scratch smaller", "learn: short scratch");
    bad += expect_error(learn(which, tree, tb, 0.6, 0.4, 1e-5, mg_rainbow_learn_scratch_bytes(32)), "prioritized_scratch",
                        "learn: the uniform learner's scratch");
  }
  if (mg_per_bytes(0) != 0 || mg_rainbow_learn_prioritized_scratch_bytes(0) != 0 ||
      mg_rainbow_learn_prioritized_scratch_bytes(1025) != 0)
    ++bad;
  std::free(t), std::free(c), std::free(idx), std::free(tree), std::free(big);
  return bad;
}

int main() {
  int bad = 0;
  if (mg_abi_version() != 21) ++bad;
  bad += host_run();
  bad += refusals();
  std::printf("prioritized replay sanitizer run: %d failures\n", bad);
  return bad ? 1 : 0;
}
