// Host sanitizer driver for the Rainbow learning entry points (test infrastructure):
// tests/test_rainbow_learn_sanitize.py compiles merging_hip.hip with -Xarch_host -fsanitize=address / undefined
// and links this file. mg_host_rainbow_learn, mg_host_rainbow_project and mg_host_rainbow_log run on exactly
// sized heap buffers, so the sanitizers see every access they make; the device entry points only get as far as
// their argument checks (nothing here launches a kernel). Any sanitizer report aborts the run.
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

static uint32_t g_lcg = 777u;
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

constexpr int kParams = 58884, kEps = 28210, kFactors = 1124, kAtoms = 51, kRow = 24;
constexpr int kLearner = 4 * kParams + 2 * kEps + 52;
static const mg_dqn_hyper kHyper = {0.001, 0.99, 0.9, 0.999, 1e-8, 1, 0};

// Two valid host updates (batch 33: not a multiple of anything) on a partly filled ring of 48 rows with every
// optional output, then one without any.
static int host_learn_run() {
  int bad = 0;
  const int B = 33, U = 2;
  const int64_t cap = 48;
  if (mg_rainbow_learner_bytes() != sizeof(float) * kLearner) ++bad;
  float* L = exact<float>(kLearner);
  for (int i = 0; i < 2 * kParams; ++i) L[i] = 0.1f * unit();
  std::memcpy(L + kParams, L, sizeof(float) * kParams);
  for (int i = 0; i < 2 * kEps; ++i) L[4 * kParams + i] = unit();
  for (int i = 0; i < kAtoms; ++i) L[4 * kParams + 2 * kEps + i] = -10.0f + 0.4f * static_cast<float>(i);
  float* ring = exact<float>(cap * kRow);
  for (int64_t r = 0; r < 40; ++r) {
    for (int k = 0; k < kRow; ++k) ring[r * kRow + k] = 3.0f * unit();
    ring[r * kRow + 10] = static_cast<float>(r % 7) - 1.0f;  // actions outside 0..4 are kept inside
    ring[r * kRow + 11] = r % 5 == 0 ? 10.0f : r % 5 == 1 ? -25.0f : 0.4f * static_cast<float>(r % 9);
    ring[r * kRow + 22] = static_cast<float>(r & 1);
    ring[r * kRow + 23] = 0.0f;
  }
  ring[3 * kRow + 10] = NAN;
  uint64_t* counter = exact<uint64_t>(1);
  *counter = 40;
  float* noise = exact<float>(U * 2 * kFactors);
  for (int i = 0; i < U * 2 * kFactors; ++i) noise[i] = unit();
  const size_t sbytes = mg_rainbow_learn_scratch_bytes(B);
  char* scratch = exact<char>(sbytes);
  float* loss = exact<float>(U);
  float* rows = exact<float>(U * B * kRow);
  float* proj = exact<float>(U * B * kAtoms);
  float* grads = exact<float>(static_cast<size_t>(U) * kParams);
  if (mg_host_rainbow_learn(L, ring, counter, cap, B, U, 0, 5, 0, &kHyper, noise, loss, rows, proj, grads, scratch,
                            sbytes) != 0) {
    std::printf("FAIL: mg_host_rainbow_learn: %s\n", mg_last_error());
    ++bad;
  }
  for (int u = 0; u < U; ++u)
    if (!std::isfinite(loss[u])) {
      std::printf("FAIL: loss[%d] = %g\n", u, loss[u]);
      ++bad;
    }
  if (mg_host_rainbow_learn(L, ring, counter, cap, B, 1, 2, 5, 2, &kHyper, noise, nullptr, nullptr, nullptr, nullptr,
                            scratch, sbytes) != 0)
    ++bad;
  if (mg_host_rainbow_learn(L, ring, counter, cap, B, 0, 3, 5, 3, &kHyper, nullptr, nullptr, nullptr, nullptr, nullptr,
                            scratch, sbytes) != 0)
    ++bad;  // no update: a no-op that needs no noise
  // the projection alone: rewards past both clamps, integral b, done both ways
  const int64_t n = 7;
  float* nd = exact<float>(n * kAtoms);
  float* r = exact<float>(n);
  float* d = exact<float>(n);
  float* pr = exact<float>(n * kAtoms);
  const float rs[7] = {-30.0f, 30.0f, 0.0f, 0.4f, 1.3f, 10.0f, -10.0f};
  for (int64_t i = 0; i < n; ++i) {
    r[i] = rs[i];
    d[i] = static_cast<float>(i & 1);
    for (int k = 0; k < kAtoms; ++k) nd[i * kAtoms + k] = unit();
  }
  if (mg_host_rainbow_project(nd, r, d, L + 4 * kParams + 2 * kEps, 0.99, pr, n) != 0) ++bad;
  if (mg_host_rainbow_project(nd, r, d, L + 4 * kParams + 2 * kEps, 0.99, pr, 0) != 0) ++bad;
  // the log on the clamp range and on what it refuses
  const int64_t m = 4096;
  float* x = exact<float>(m + 4);
  float* y = exact<float>(m + 4);
  for (int64_t i = 0; i < m; ++i) x[i] = 0.01f + 0.98f * static_cast<float>(i) / static_cast<float>(m - 1);
  x[m] = 0.0f, x[m + 1] = -1.0f, x[m + 2] = NAN, x[m + 3] = INFINITY;
  if (mg_host_rainbow_log(x, y, m + 4) != 0) ++bad;
  for (int64_t i = 0; i < m; ++i)
    if (!(std::fabs(y[i] - std::log(x[i])) <= 3e-7f * std::fabs(std::log(x[i])) + 1e-9f)) {
      std::printf("FAIL: log(%g) = %g\n", x[i], y[i]);
      ++bad;
      break;
    }
  for (int i = 0; i < 4; ++i)
    if (!std::isnan(y[m + i])) ++bad;
  for (void* p : {static_cast<void*>(L), static_cast<void*>(ring), static_cast<void*>(counter), static_cast<void*>(noise),
                  static_cast<void*>(scratch), static_cast<void*>(loss), static_cast<void*>(rows),
                  static_cast<void*>(proj), static_cast<void*>(grads), static_cast<void*>(nd), static_cast<void*>(r),
                  static_cast<void*>(d), static_cast<void*>(pr), static_cast<void*>(x), static_cast<void*>(y)})
    std::free(p);
  return bad;
}

// The entry points refuse before anything is launched or read.
static int refusals() {
  int bad = 0;
  float* t = exact<float>(64);
  uint64_t* c = exact<uint64_t>(1);
  char* big = exact<char>(64);
  const size_t sb = mg_rainbow_learn_scratch_bytes(32);
  mg_transitions X{};
  X.obs_first = X.obs = X.rew = t;
  X.a1 = reinterpret_cast<const int8_t*>(t);
  bad += expect_error(mg_rainbow_replay_store(nullptr, c, 10, &X, 4, 2, nullptr), "NULL", "store: NULL rows");
  bad += expect_error(mg_rainbow_replay_store(t, nullptr, 10, &X, 4, 2, nullptr), "NULL", "store: NULL counter");
  bad += expect_error(mg_rainbow_replay_store(t, c, 10, nullptr, 4, 2, nullptr), "NULL", "store: NULL tr");
  bad += expect_error(mg_rainbow_replay_store(t, c, 0, &X, 4, 2, nullptr), "capacity", "store: capacity 0");
  bad += expect_error(mg_rainbow_replay_store(t, c, 10, &X, -1, 2, nullptr), "n < 0", "store: n < 0");
  bad += expect_error(mg_rainbow_replay_store(t, c, 10, &X, 4, -2, nullptr), "num_steps < 0", "store: num_steps < 0");
  X.goal = t;
  bad += expect_error(mg_rainbow_replay_store(t, c, 10, &X, 4, 2, nullptr), "must be NULL", "store: goal set");
  X.goal = nullptr;
  X.rew = nullptr;
  bad += expect_error(mg_rainbow_replay_store(t, c, 10, &X, 4, 2, nullptr), "required", "store: rew NULL");
  X.rew = reinterpret_cast<const float*>(reinterpret_cast<const char*>(t) + 2);
  bad += expect_error(mg_rainbow_replay_store(t, c, 10, &X, 4, 2, nullptr), "aligned", "store: rew misaligned");
  X.rew = t;
  bad += expect_error(mg_rainbow_replay_store(t + 1, c, 10, &X, 4, 2, nullptr), "aligned", "store: rows misaligned");
  bad += expect_error(mg_rainbow_replay_store(t, c, 10, &X, int64_t{1} << 40, 2, nullptr), "grid", "store: too many");
  if (mg_rainbow_replay_store(t, c, 10, &X, 0, 2, nullptr) != 0) ++bad;  // no env: a no-op
  if (mg_rainbow_replay_store(t, c, 10, &X, 4, 0, nullptr) != 0) ++bad;  // no step: a no-op
  auto dev = [&](float* l, const float* rows, const uint64_t* cnt, int64_t cap, int b, int u, const mg_dqn_hyper* h,
                 const float* nz, void* packed, void* scr, size_t bytes) {
    return mg_rainbow_learn(l, rows, cnt, cap, b, u, 0, 0, 0, h, nz, nullptr, nullptr, nullptr, nullptr, packed, scr, bytes,
                            nullptr);
  };
  auto host = [&](float* l, const float* rows, const uint64_t* cnt, int64_t cap, int b, int u, const mg_dqn_hyper* h,
                  const float* nz, void*, void* scr, size_t bytes) {
    return mg_host_rainbow_learn(l, rows, cnt, cap, b, u, 0, 0, 0, h, nz, nullptr, nullptr, nullptr, nullptr, scr, bytes);
  };
  mg_dqn_hyper badh = kHyper;
  badh.beta2 = 1.0;
  for (int which = 0; which < 2; ++which) {
    auto call = [&](float* l, const float* rows, const uint64_t* cnt, int64_t cap, int b, int u, const mg_dqn_hyper* h,
                    const float* nz, void* packed, void* scr, size_t bytes) {
      return which ? host(l, rows, cnt, cap, b, u, h, nz, packed, scr, bytes)
                   : dev(l, rows, cnt, cap, b, u, h, nz, packed, scr, bytes);
    };
    bad += expect_error(call(nullptr, t, c, 10, 32, 1, &kHyper, t, nullptr, big, sb), "NULL", "learn: NULL learner");
    bad += expect_error(call(t, nullptr, c, 10, 32, 1, &kHyper, t, nullptr, big, sb), "NULL", "learn: NULL rows");
    bad += expect_error(call(t, t, nullptr, 10, 32, 1, &kHyper, t, nullptr, big, sb), "NULL", "learn: NULL counter");
    bad += expect_error(call(t, t, c, 10, 32, 1, nullptr, t, nullptr, big, sb), "NULL", "learn: NULL hyper");
    bad += expect_error(call(t, t, c, 10, 32, 1, &kHyper, t, nullptr, nullptr, sb), "NULL", "learn: NULL scratch");
    bad += expect_error(call(t, t, c, 10, 0, 1, &kHyper, t, nullptr, big, sb), "batch", "learn: batch 0");
    bad += expect_error(call(t, t, c, 10, 1025, 1, &kHyper, t, nullptr, big, sb), "batch", "learn: batch 1025");
    bad += expect_error(call(t, t, c, 0, 32, 1, &kHyper, t, nullptr, big, sb), "capacity", "learn: capacity 0");
    bad += expect_error(call(t, t, c, 10, 32, -1, &kHyper, t, nullptr, big, sb), "num_updates", "learn: -1 updates");
    bad += expect_error(call(t, t, c, 10, 32, 1, &kHyper, nullptr, nullptr, big, sb), "noise is NULL", "learn: no noise");
    bad += expect_error(call(t, t, c, 10, 32, 1, &badh, t, nullptr, big, sb), "beta", "learn: beta2 1");
    bad += expect_error(call(t + 1, t, c, 10, 32, 1, &kHyper, t, nullptr, big, sb), "aligned", "learn: learner misaligned");
    bad += expect_error(call(t, t, c, 10, 32, 1, &kHyper, t, nullptr, big, sb - 1), "scratch smaller", "learn: scratch short");
  }
  bad += expect_error(dev(t, t, c, 10, 32, 1, &kHyper, t, big + 8, big, sb), "aligned", "learn: packed_out misaligned");
  bad += expect_error(mg_host_rainbow_project(nullptr, t, t, t, 0.99, t, 1), "NULL", "project: NULL next_dist");
  bad += expect_error(mg_host_rainbow_project(t, t, t, t, 0.99, nullptr, 1), "NULL", "project: NULL proj");
  bad += expect_error(mg_host_rainbow_project(t, t, t, t, 0.99, t, -1), "n < 0", "project: n < 0");
  bad += expect_error(mg_host_rainbow_log(nullptr, t, 1), "NULL", "log: NULL x");
  bad += expect_error(mg_host_rainbow_log(t, t, -1), "n < 0", "log: n < 0");
  if (mg_rainbow_learn_scratch_bytes(0) != 0 || mg_rainbow_learn_scratch_bytes(1025) != 0) ++bad;
  std::free(t);
  std::free(c);
  std::free(big);
  return bad;
}

int main() {
  int bad = 0;
  if (mg_abi_version() != 21) ++bad;
  bad += host_learn_run();
  bad += refusals();
  std::printf("rainbow learn sanitizer run: %d failures\n", bad);
  return bad ? 1 : 0;
}
