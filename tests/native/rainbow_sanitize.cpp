// Host sanitizer driver for the Rainbow entry points (test infrastructure): tests/test_rainbow_sanitize.py
// compiles merging_hip.hip with -Xarch_host -fsanitize=address / undefined and links this file.
// mg_host_rainbow_head and mg_host_rainbow_exp run on exactly sized heap buffers, so the sanitizers see every
// access they make; the device entry points only get as far as their argument checks (nothing here launches
// a kernel). Any sanitizer report aborts the run.
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

constexpr int kLogits = 306, kActions = 5, kAtoms = 51;

// The head over rows of several scales: moderate logits, a spread far past the exp cut-off, huge and
// non-finite values (the int conversion inside exp must stay defined for every input it accepts).
static int host_head_run() {
  const int64_t n = 37;
  int bad = 0;
  float* z = exact<float>(kAtoms);
  for (int i = 0; i < kAtoms; ++i) z[i] = -10.0f + 0.4f * static_cast<float>(i);
  float* lg = exact<float>(n * kLogits);
  for (int64_t r = 0; r < n; ++r) {
    const float scale = r < 12 ? 2.0f : r < 24 ? 300.0f : 3.0e37f;
    for (int k = 0; k < kLogits; ++k) lg[r * kLogits + k] = scale * unit();
  }
  lg[30 * kLogits + 7] = INFINITY;
  lg[31 * kLogits + 60] = -INFINITY;
  lg[32 * kLogits + 100] = NAN;
  float* q = exact<float>(n * kActions);
  int8_t* a = exact<int8_t>(n);
  float* q2 = exact<float>(n * kActions);
  int8_t* a2 = exact<int8_t>(n);
  if (mg_host_rainbow_head(lg, z, q, a, n) != 0 || mg_host_rainbow_head(lg, z, q2, nullptr, n) != 0 ||
      mg_host_rainbow_head(lg, z, nullptr, a2, n) != 0) {
    std::printf("FAIL: mg_host_rainbow_head: %s\n", mg_last_error());
    ++bad;
  }
  if (std::memcmp(q, q2, n * kActions * sizeof(float)) != 0 || std::memcmp(a, a2, n) != 0) {
    std::printf("FAIL: the head's optional outputs differ\n");
    ++bad;
  }
  for (int64_t r = 0; r < 24; ++r) {  // the finite rows: q inside the support, an action in range
    for (int k = 0; k < kActions; ++k)
      if (!(q[r * kActions + k] >= -10.001f && q[r * kActions + k] <= 10.001f)) {
        std::printf("FAIL: q[%lld][%d] = %g outside the support\n", static_cast<long long>(r), k, q[r * kActions + k]);
        ++bad;
      }
  }
  for (int64_t r = 0; r < n; ++r)
    if (a[r] < 0 || a[r] >= kActions) ++bad;
  if (mg_host_rainbow_head(lg, z, q, a, 0) != 0) ++bad;  // an empty batch
  // exp on its whole accepted range and beyond
  const int64_t m = 4096;
  float* x = exact<float>(m + 6);
  float* y = exact<float>(m + 6);
  for (int64_t i = 0; i < m; ++i) x[i] = -87.0f * static_cast<float>(i) / static_cast<float>(m - 1);
  x[m] = -88.0f;
  x[m + 1] = -3.0e38f;
  x[m + 2] = -INFINITY;
  x[m + 3] = NAN;
  x[m + 4] = -0.0f;
  x[m + 5] = std::nextafterf(-87.0f, -100.0f);
  if (mg_host_rainbow_exp(x, y, m + 6) != 0) ++bad;
  for (int64_t i = 0; i < m; ++i)
    if (!(y[i] > 0.0f && y[i] <= 1.0f) || std::fabs(y[i] - std::exp(x[i])) > 3e-7f * std::exp(x[i])) {
      std::printf("FAIL: exp(%g) = %g\n", x[i], y[i]);
      ++bad;
      break;
    }
  if (y[m] != 0.0f || y[m + 1] != 0.0f || y[m + 2] != 0.0f || y[m + 3] != 0.0f || y[m + 4] != 1.0f || y[m + 5] != 0.0f)
    ++bad;
  std::free(z);
  std::free(lg);
  std::free(q);
  std::free(a);
  std::free(q2);
  std::free(a2);
  std::free(x);
  std::free(y);
  return bad;
}

// The entry points refuse before anything is launched or read.
static int refusals() {
  int bad = 0;
  float* t = exact<float>(64);
  char* packed = exact<char>(mg_rainbow_packed_bytes());
  auto pack = [&](const float* first, const float* support, int in, int h1, int h2, int hs, int na, int nz, void* p) {
    return mg_rainbow_pack(first, t, t, t, t, t, t, t, t, t, t, t, support, in, h1, h2, hs, na, nz, p, nullptr);
  };
  bad += expect_error(pack(nullptr, t, 10, 32, 64, 64, 5, 51, packed), "NULL", "pack: NULL tensor");
  bad += expect_error(pack(t, nullptr, 10, 32, 64, 64, 5, 51, packed), "NULL", "pack: NULL support");
  bad += expect_error(pack(t, t, 10, 32, 64, 64, 5, 51, nullptr), "NULL", "pack: NULL packed");
  bad += expect_error(pack(t, t, 11, 32, 64, 64, 5, 51, packed), "only RainbowDQN(10, 5)", "pack: in_dim 11");
  bad += expect_error(pack(t, t, 10, 200, 100, 64, 5, 51, packed), "only RainbowDQN(10, 5)", "pack: the DQN's widths");
  bad += expect_error(pack(t, t, 10, 32, 64, 64, 3, 51, packed), "only RainbowDQN(10, 5)", "pack: 3 actions");
  bad += expect_error(pack(t, t, 10, 32, 64, 64, 5, 21, packed), "only RainbowDQN(10, 5)", "pack: 21 atoms");
  bad += expect_error(pack(t, t, 10, 32, 64, 64, 5, 51, packed + 8), "16-byte", "pack: misaligned packed");
  bad += expect_error(pack(reinterpret_cast<const float*>(reinterpret_cast<const char*>(t) + 2), t, 10, 32, 64, 64, 5,
                           51, packed),
                      "4-byte", "pack: misaligned tensor");
  int8_t* act = exact<int8_t>(8);
  bad += expect_error(mg_rainbow_forward(packed, nullptr, 0, t, t, act, 4, nullptr), "obs is NULL", "forward: NULL obs");
  bad += expect_error(mg_rainbow_forward(nullptr, t, 0, t, t, act, 4, nullptr), "16-byte", "forward: NULL packed");
  bad += expect_error(mg_rainbow_forward(packed + 4, t, 0, t, t, act, 4, nullptr), "16-byte", "forward: misaligned");
  bad += expect_error(mg_rainbow_forward(packed, t, 10, t, t, act, 4, nullptr), "rotate", "forward: rotate 10");
  bad += expect_error(mg_rainbow_forward(packed, t, -1, t, t, act, 4, nullptr), "rotate", "forward: rotate -1");
  bad += expect_error(mg_rainbow_forward(packed, t, 3, t, t, act, -1, nullptr), "n < 0", "forward: n < 0");
  if (mg_rainbow_forward(packed, t, 3, nullptr, nullptr, nullptr, 0, nullptr) != 0) ++bad;  // an empty batch
  mg_params P;
  mg_params_default(&P);
  double* d = exact<double>(4);
  uint16_t* tf = exact<uint16_t>(4);
  mg_state S{};
  S.p1 = S.v1 = S.p2 = S.v2 = S.ret1 = S.ret2 = d;
  S.tf = tf;
  mg_traj T{};
  bad += expect_error(mg_rollout_rainbow(nullptr, &S, &T, nullptr, 4, 2, packed, 2, MG_AUTORESET, nullptr), "params",
                      "rollout: NULL params");
  bad += expect_error(mg_rollout_rainbow(&P, &S, nullptr, nullptr, 4, 2, packed, 2, MG_AUTORESET, nullptr), "traj is NULL",
                      "rollout: NULL traj");
  bad += expect_error(mg_rollout_rainbow(&P, &S, &T, nullptr, 4, 2, nullptr, 2, MG_AUTORESET, nullptr), "packed Rainbow net",
                      "rollout: NULL net");
  bad += expect_error(mg_rollout_rainbow(&P, &S, &T, nullptr, 4, 2, packed + 8, 0, MG_AUTORESET, nullptr),
                      "packed Rainbow net", "rollout: misaligned net");
  bad += expect_error(mg_rollout_rainbow(&P, &S, &T, nullptr, 4, -1, packed, 2, MG_AUTORESET, nullptr), "num_steps",
                      "rollout: num_steps -1");
  bad += expect_error(mg_rollout_rainbow(&P, &S, &T, nullptr, 4, 2, packed, 1, MG_AUTORESET, nullptr), "opponent_mode",
                      "rollout: mode 1");
  bad += expect_error(mg_rollout_rainbow(&P, &S, &T, nullptr, 4, 2, packed, 3, MG_AUTORESET, nullptr), "opponent_mode",
                      "rollout: mode 3");
  S.tf = nullptr;
  bad += expect_error(mg_rollout_rainbow(&P, &S, &T, nullptr, 4, 2, packed, 2, MG_AUTORESET, nullptr), "mg_state",
                      "rollout: NULL state array");
  S.tf = tf;
  if (mg_rollout_rainbow(&P, &S, &T, nullptr, 0, 2, packed, 2, MG_AUTORESET, nullptr) != 0) ++bad;  // no env: a no-op
  if (mg_rollout_rainbow(&P, &S, &T, nullptr, 4, 0, packed, 0, MG_AUTORESET, nullptr) != 0) ++bad;  // no step: a no-op
  bad += expect_error(mg_host_rainbow_head(nullptr, t, t, act, 1), "NULL", "head: NULL logits");
  bad += expect_error(mg_host_rainbow_head(t, nullptr, t, act, 1), "NULL", "head: NULL support");
  bad += expect_error(mg_host_rainbow_head(t, t, t, act, -1), "n < 0", "head: n < 0");
  bad += expect_error(mg_host_rainbow_exp(nullptr, t, 1), "NULL", "exp: NULL x");
  if (mg_rainbow_packed_bytes() != 74192) ++bad;
  std::free(t);
  std::free(packed);
  std::free(act);
  std::free(d);
  std::free(tf);
  return bad;
}

int main() {
  int bad = 0;
  if (mg_abi_version() != 21) ++bad;
  bad += host_head_run();
  bad += refusals();
  std::printf("rainbow sanitizer run: %d failures\n", bad);
  return bad ? 1 : 0;
}
