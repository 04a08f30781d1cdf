// Host sanitizer driver for DQN.learn's host code (test infrastructure): tests/test_learn_sanitize.py
// compiles merging_hip.hip with -Xarch_host -fsanitize=address / undefined and links this file.
// mg_host_dqn_learn runs on exactly sized heap buffers, so the sanitizers see every access the update
// makes; the device entry points only get as far as their argument checks (nothing here launches a
// kernel). Any sanitizer report aborts the run.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "merging_hip.h"

// `bytes` bytes at a 16-byte boundary, not one more (posix_memalign keeps the size exact for ASan).
template <class T>
static T* exact(size_t count) {
  void* p = nullptr;
  if (posix_memalign(&p, 16, count * sizeof(T)) != 0 || !p) std::abort();
  std::memset(p, 0, count * sizeof(T));
  return static_cast<T*>(p);
}

static uint32_t g_lcg = 12345u;
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

static int host_learn_run(int in, int out, int batch) {
  const int rf = 2 * in + 2, updates = 3;
  const int64_t cap = 300;
  const size_t P = mg_dqn_learner_bytes(in, out) / 16;
  const size_t sbytes = mg_dqn_learn_scratch_bytes(batch, in, out);
  int bad = 0;
  if (P != static_cast<size_t>(200 * in + 200 + 20000 + 100 + 100 * out + out) || sbytes == 0) ++bad;
  float* ring = exact<float>(cap * rf);
  for (int64_t r = 0; r < cap / 2; ++r) {  // a half-filled memory
    for (int k = 0; k < rf; ++k) ring[r * rf + k] = 10.0f * unit();
    ring[r * rf + in] = static_cast<float>(r % (out + 1));  // one action past the net's: kept inside
  }
  uint64_t* counter = exact<uint64_t>(1);
  *counter = static_cast<uint64_t>(cap / 2);
  float* first = nullptr;
  for (int run = 0; run < 2; ++run) {
    g_lcg = 777u;
    float* learner = exact<float>(4 * P);
    const float scale[6] = {0.3f, 0.3f, 0.07f, 0.07f, 0.1f, 0.1f};
    const size_t ends[6] = {200u * in, 200u * in + 200u, 200u * in + 20200u, 200u * in + 20300u,
                            200u * in + 20300u + 100u * out, P};
    for (size_t i = 0, t = 0; i < P; ++i) {
      while (i >= ends[t]) ++t;
      learner[i] = scale[t] * unit();
      learner[P + i] = 0.5f * learner[i];
    }
    float* loss = exact<float>(updates);
    float* rows_out = exact<float>(static_cast<size_t>(updates) * batch * rf);
    void* scratch = exact<char>(sbytes);
    const mg_dqn_hyper h{0.01, 0.9, 0.9, 0.999, 1e-8, 2, 0};
    for (int filled = 0; filled < 2; ++filled)
      if (mg_host_dqn_learn(learner, ring, counter, cap, rf, in, out, batch, updates, 1 + 3 * filled, 9, 4, filled, &h,
                            loss, rows_out, scratch, sbytes) != 0) {
        std::printf("FAIL: mg_host_dqn_learn(%d, %d, %d): %s\n", in, out, batch, mg_last_error());
        ++bad;
      }
    // the optional outputs may be absent, and counter is not read without filled_only
    if (mg_host_dqn_learn(learner, ring, nullptr, cap, rf, in, out, batch, 1, 7, 9, 4, 0, &h, nullptr, nullptr, scratch,
                          sbytes) != 0)
      ++bad;
    for (size_t i = 0; i < 4 * P; ++i)
      if (!std::isfinite(learner[i])) {
        std::printf("FAIL: learner[%zu] is not finite\n", i);
        ++bad;
        break;
      }
    for (int u = 0; u < updates; ++u)
      if (!std::isfinite(loss[u]) || loss[u] < 0.0f) ++bad;
    if (run == 0) {
      first = learner;
    } else {
      if (std::memcmp(first, learner, 4 * P * sizeof(float)) != 0) {
        std::printf("FAIL: two runs of (%d, %d, %d) differ\n", in, out, batch);
        ++bad;
      }
      std::free(learner);
    }
    std::free(loss);
    std::free(rows_out);
    std::free(scratch);
  }
  std::free(first);
  std::free(ring);
  std::free(counter);
  return bad;
}

// The device entry points refuse before anything is launched or read.
static int device_refusals() {
  const int in = 10, out = 5, batch = 96, rf = 22;
  const size_t P = mg_dqn_learner_bytes(in, out) / 16, sbytes = mg_dqn_learn_scratch_bytes(batch, in, out);
  float* learner = exact<float>(4 * P);
  float* ring = exact<float>(64 * rf);
  uint64_t* counter = exact<uint64_t>(1);
  char* scratch = exact<char>(sbytes);
  float* loss = exact<float>(1);
  mg_dqn_hyper h{0.01, 0.9, 0.9, 0.999, 1e-8, 100, 0};
  int bad = 0;
  auto learn = [&](float* l, const float* r, const uint64_t* c, int64_t cap, int rfl, int i, int o, int b, int nu, int fo,
                   const mg_dqn_hyper* hp, float* lo, void* packed, void* s, size_t sb) {
    return mg_dqn_learn(l, r, c, cap, rfl, i, o, b, nu, 0, 0, 0, fo, hp, lo, nullptr, packed, s, sb, nullptr);
  };
  bad += expect_error(learn(nullptr, ring, counter, 64, rf, in, out, batch, 1, 0, &h, loss, nullptr, scratch, sbytes),
                      "NULL", "NULL learner");
  bad += expect_error(learn(learner, nullptr, counter, 64, rf, in, out, batch, 1, 0, &h, loss, nullptr, scratch, sbytes),
                      "NULL", "NULL rows");
  bad += expect_error(learn(learner, ring, nullptr, 64, rf, in, out, batch, 1, 1, &h, loss, nullptr, scratch, sbytes),
                      "NULL", "filled_only without counter");
  bad += expect_error(learn(learner, ring, counter, 64, rf, in, out, batch, 1, 0, nullptr, loss, nullptr, scratch, sbytes),
                      "NULL", "NULL hyper");
  bad += expect_error(learn(learner, ring, counter, 64, rf, in, out, batch, 1, 0, &h, loss, nullptr, nullptr, sbytes),
                      "NULL", "NULL scratch");
  bad += expect_error(learn(learner, ring, counter, 64, rf, 14, out, batch, 1, 0, &h, loss, nullptr, scratch, sbytes),
                      "in_dim", "in_dim 14");
  bad += expect_error(learn(learner, ring, counter, 64, rf, in, 9, batch, 1, 0, &h, loss, nullptr, scratch, sbytes),
                      "out_dim", "out_dim 9");
  bad += expect_error(learn(learner, ring, counter, 64, 24, in, out, batch, 1, 0, &h, loss, nullptr, scratch, sbytes),
                      "row_floats", "row_floats 24 with in_dim 10");
  bad += expect_error(learn(learner, ring, counter, 64, rf, in, out, 0, 1, 0, &h, loss, nullptr, scratch, sbytes),
                      "batch", "batch 0");
  bad += expect_error(learn(learner, ring, counter, 64, rf, in, out, 1025, 1, 0, &h, loss, nullptr, scratch, sbytes),
                      "batch", "batch 1025");
  bad += expect_error(learn(learner, ring, counter, 0, rf, in, out, batch, 1, 0, &h, loss, nullptr, scratch, sbytes),
                      "capacity", "capacity 0");
  bad += expect_error(learn(learner, ring, counter, 64, rf, in, out, batch, -1, 0, &h, loss, nullptr, scratch, sbytes),
                      "num_updates", "num_updates -1");
  bad += expect_error(learn(learner, ring, counter, 64, rf, in, out, batch, 1, 0, &h, loss, nullptr, scratch, sbytes - 4),
                      "scratch", "short scratch");
  bad += expect_error(learn(learner + 1, ring, counter, 64, rf, in, out, batch, 1, 0, &h, loss, nullptr, scratch, sbytes),
                      "aligned", "misaligned learner");
  bad += expect_error(learn(learner, ring, counter, 64, rf, in, out, batch, 1, 0, &h, loss, scratch + 8, scratch, sbytes),
                      "aligned", "misaligned packed_out");
  h.target_period = 0;
  bad += expect_error(learn(learner, ring, counter, 64, rf, in, out, batch, 1, 0, &h, loss, nullptr, scratch, sbytes),
                      "target_period", "target_period 0");
  h.target_period = 100;
  h.beta2 = 1.0;
  bad += expect_error(learn(learner, ring, counter, 64, rf, in, out, batch, 1, 0, &h, loss, nullptr, scratch, sbytes),
                      "beta2", "beta2 1");
  h.beta2 = 0.999;
  if (learn(learner, ring, counter, 64, rf, in, out, batch, 0, 0, &h, loss, nullptr, scratch, sbytes) != 0) ++bad;  // no-op
  bad += expect_error(mg_dqn_learner_init(nullptr, ring, ring, ring, ring, ring, ring, in, out, nullptr), "NULL",
                      "init: NULL learner");
  bad += expect_error(mg_dqn_learner_init(learner, ring, ring, nullptr, ring, ring, ring, in, out, nullptr), "NULL",
                      "init: NULL tensor");
  bad += expect_error(mg_dqn_learner_init(learner, ring, ring, ring, ring, ring, ring, 0, out, nullptr), "in_dim",
                      "init: in_dim 0");
  bad += expect_error(mg_dqn_learner_init(learner + 2, ring, ring, ring, ring, ring, ring, in, out, nullptr), "aligned",
                      "init: misaligned learner");
  if (mg_dqn_learner_bytes(14, 5) != 0 || mg_dqn_learn_scratch_bytes(2000, 10, 5) != 0) ++bad;
  std::free(learner);
  std::free(ring);
  std::free(counter);
  std::free(scratch);
  std::free(loss);
  return bad;
}

int main() {
  int bad = 0;
  if (mg_abi_version() != 21) ++bad;
  bad += host_learn_run(10, 5, 96);
  bad += host_learn_run(11, 5, 32);
  bad += device_refusals();
  std::printf("learn sanitizer run: %d failures\n", bad);
  return bad ? 1 : 0;
}
