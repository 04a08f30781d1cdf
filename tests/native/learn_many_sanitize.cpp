// Host sanitizer driver for the DQN population's host code (test infrastructure): tests/test_learn_many_host.py
// compiles merging_hip.hip with -Xarch_host -fsanitize=address / undefined and links this file.
// mg_host_dqn_learn_many runs on exactly sized heap buffers -- the learners [M, 4 P], the scratch [M, one
// learner's], the outputs [U, M] and [U, M, B, rf], every member's own ring -- so the sanitizers see every access
// a member makes past its own slice; each member is compared with mg_host_dqn_learn on buffers of its own. The
// device entry points only get as far as their argument checks (nothing here launches a kernel). Any sanitizer
// report aborts the run.
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

static int host_population_run(int M, int in, int out, int batch) {
  const int rf = 2 * in + 2, updates = 3;
  const int64_t cap = 96;
  const size_t P = mg_dqn_learner_bytes(in, out) / 16;
  const size_t one = mg_dqn_learn_scratch_bytes(batch, in, out);
  int bad = 0;
  if (one == 0 || one % 16 != 0) ++bad;
  g_lcg = 4242u + static_cast<uint32_t>(M);
  mg_dqn_member* member = exact<mg_dqn_member>(M);
  float** ring = exact<float*>(M);
  uint64_t** counter = exact<uint64_t*>(M);
  for (int m = 0; m < M; ++m) {
    ring[m] = exact<float>(cap * rf);
    for (int64_t r = 0; r < cap / 2; ++r) {  // a half-filled memory
      for (int k = 0; k < rf; ++k) ring[m][r * rf + k] = 10.0f * unit();
      ring[m][r * rf + in] = static_cast<float>(r % (out + 1));  // one action past the net's: kept inside
    }
    counter[m] = exact<uint64_t>(1);
    *counter[m] = static_cast<uint64_t>(m % 3 == 0 ? 0 : cap / 2 - m % 5);  // a counter of 0 draws slot 0
    member[m].rows = ring[m];
    member[m].counter = counter[m];
    member[m].seed = 0x9E3779B97F4A7C15ull * static_cast<uint64_t>(m + 1);
    member[m].first_update = static_cast<uint64_t>(m);
    member[m].first_draw = static_cast<uint64_t>(5 + 3 * m);
    member[m].hyper = mg_dqn_hyper{0.01 * (1 + m % 4), 0.9 - 0.01 * (m % 6), 0.9 - 0.02 * (m % 3), 0.999 - 0.001 * (m % 2),
                                   1e-8 * (1 + m % 3), 1 + m % 3, 0};
  }
  float* learners = exact<float>(static_cast<size_t>(M) * 4 * P);
  for (size_t i = 0; i < static_cast<size_t>(M) * 4 * P; ++i)
    learners[i] = (i / P) % 4 < 2 ? 0.1f * unit() : 0.0f;  // eval, target; zero moments
  float* lone = exact<float>(static_cast<size_t>(M) * 4 * P);
  std::memcpy(lone, learners, static_cast<size_t>(M) * 4 * P * sizeof(float));
  float* loss = exact<float>(static_cast<size_t>(updates) * M);
  float* rows_out = exact<float>(static_cast<size_t>(updates) * M * batch * rf);
  void* scratch = exact<char>(one * M);
  for (int filled = 0; filled < 2; ++filled) {
    // the lone learners first: the population call advances the members' counters
    float* loss1 = exact<float>(updates);
    float* rows1 = exact<float>(static_cast<size_t>(updates) * batch * rf);
    void* scratch1 = exact<char>(one);
    float* want_loss = exact<float>(static_cast<size_t>(updates) * M);
    for (int m = 0; m < M; ++m) {
      if (mg_host_dqn_learn(lone + static_cast<size_t>(m) * 4 * P, ring[m], counter[m], cap, rf, in, out, batch, updates,
                            member[m].first_update, member[m].seed, member[m].first_draw, filled, &member[m].hyper,
                            loss1, rows1, scratch1, one) != 0)
        ++bad;
      for (int u = 0; u < updates; ++u) want_loss[u * M + m] = loss1[u];
    }
    const uint64_t before = member[M - 1].first_update;
    if (mg_host_dqn_learn_many(learners, member, M, cap, rf, in, out, batch, updates, filled, loss, rows_out, scratch,
                               one * M) != 0) {
      std::printf("FAIL: mg_host_dqn_learn_many(%d, %d, %d, %d): %s\n", M, in, out, batch, mg_last_error());
      ++bad;
    }
    if (member[M - 1].first_update != before + updates) ++bad;
    if (std::memcmp(learners, lone, static_cast<size_t>(M) * 4 * P * sizeof(float)) != 0) {
      std::printf("FAIL: population (%d, %d, %d, %d) differs from its lone learners\n", M, in, out, batch);
      ++bad;
    }
    if (std::memcmp(loss, want_loss, static_cast<size_t>(updates) * M * sizeof(float)) != 0) {
      std::printf("FAIL: losses of (%d, %d, %d, %d) differ from the lone learners'\n", M, in, out, batch);
      ++bad;
    }
    std::free(loss1);
    std::free(rows1);
    std::free(scratch1);
    std::free(want_loss);
  }
  // the optional outputs may be absent, and the counters are not read without filled_only
  for (int m = 0; m < M; ++m) member[m].counter = nullptr;
  if (mg_host_dqn_learn_many(learners, member, M, cap, rf, in, out, batch, 1, 0, nullptr, nullptr, scratch, one * M) != 0)
    ++bad;
  for (size_t i = 0; i < static_cast<size_t>(M) * 4 * P; ++i)
    if (!std::isfinite(learners[i])) {
      std::printf("FAIL: learners[%zu] is not finite\n", i);
      ++bad;
      break;
    }
  for (int m = 0; m < M; ++m) {
    std::free(ring[m]);
    std::free(counter[m]);
  }
  std::free(ring);
  std::free(counter);
  std::free(member);
  std::free(learners);
  std::free(lone);
  std::free(loss);
  std::free(rows_out);
  std::free(scratch);
  return bad;
}

// The device entry points refuse before anything is launched or read.
static int device_refusals() {
  const int in = 10, out = 5, batch = 8, rf = 22, M = 3;
  const size_t P = mg_dqn_learner_bytes(in, out) / 16, one = mg_dqn_learn_scratch_bytes(batch, in, out);
  const size_t tbytes = mg_dqn_learn_many_table_bytes(M);
  float* learners = exact<float>(M * 4 * P);
  float* ring = exact<float>(64 * rf);
  uint64_t* counter = exact<uint64_t>(1);
  char* scratch = exact<char>(one * M);
  char* table = exact<char>(tbytes);
  mg_dqn_member* member = exact<mg_dqn_member>(M);
  for (int m = 0; m < M; ++m) {
    member[m].rows = ring, member[m].counter = counter;
    member[m].hyper = mg_dqn_hyper{0.01, 0.9, 0.9, 0.999, 1e-8, 100, 0};
  }
  int bad = 0;
  auto learn = [&](float* l, void* t, size_t tb, mg_dqn_member* mem, int members, int nu, int fo, void* packed,
                   size_t stride, void* s, size_t sb) {
    return mg_dqn_learn_many(l, t, tb, mem, members, 64, rf, in, out, batch, nu, fo, nullptr, nullptr, packed, stride, s,
                             sb, nullptr);
  };
  bad += expect_error(learn(nullptr, table, tbytes, member, M, 1, 0, nullptr, 0, scratch, one * M), "NULL", "NULL learners");
  bad += expect_error(learn(learners, nullptr, tbytes, member, M, 1, 0, nullptr, 0, scratch, one * M), "NULL", "NULL table");
  bad += expect_error(learn(learners, table, tbytes, nullptr, M, 1, 0, nullptr, 0, scratch, one * M), "NULL", "NULL member");
  bad += expect_error(learn(learners, table, tbytes, member, 0, 1, 0, nullptr, 0, scratch, one * M), "members", "0 members");
  bad += expect_error(learn(learners, table, tbytes, member, 65, 1, 0, nullptr, 0, scratch, one * M), "members", "65 members");
  bad += expect_error(learn(learners, table, tbytes - 1, member, M, 1, 0, nullptr, 0, scratch, one * M), "table smaller",
                      "short table");
  bad += expect_error(learn(learners, table, tbytes, member, M, 1, 0, nullptr, 0, scratch, one * M - 4), "scratch smaller",
                      "short scratch");
  bad += expect_error(learn(learners + 1, table, tbytes, member, M, 1, 0, nullptr, 0, scratch, one * M), "aligned",
                      "misaligned learners");
  bad += expect_error(learn(learners, table, tbytes, member, M, 1, 0, scratch, 24, scratch, one * M), "packed_stride",
                      "packed_stride 24");
  member[2].hyper.target_period = 0;
  bad += expect_error(learn(learners, table, tbytes, member, M, 1, 0, nullptr, 0, scratch, one * M), "member 2: target_period",
                      "target_period 0");
  bad += expect_error(mg_dqn_learn_many_init(table, tbytes, member, M, nullptr), "member 2: target_period",
                      "init: target_period 0");
  member[2].hyper.target_period = 100;
  member[1].hyper.beta2 = 1.0;
  bad += expect_error(learn(learners, table, tbytes, member, M, 1, 0, nullptr, 0, scratch, one * M), "member 1: need 0 <= beta1",
                      "beta2 1");
  member[1].hyper.beta2 = 0.999;
  member[1].counter = nullptr;
  bad += expect_error(learn(learners, table, tbytes, member, M, 1, 1, nullptr, 0, scratch, one * M), "NULL",
                      "filled_only without a counter");
  member[1].counter = counter;
  if (learn(learners, table, tbytes, member, M, 0, 0, nullptr, 0, scratch, one * M) != 0) ++bad;  // no-op
  bad += expect_error(mg_dqn_learn_many_init(nullptr, tbytes, member, M, nullptr), "NULL", "init: NULL table");
  bad += expect_error(mg_dqn_learn_many_init(table, tbytes - 1, member, M, nullptr), "table smaller", "init: short table");
  if (mg_dqn_learn_many_table_bytes(0) != 0 || mg_dqn_learn_many_table_bytes(65) != 0 ||
      mg_dqn_learn_many_table_bytes(1) * 64 != mg_dqn_learn_many_table_bytes(64))
    ++bad;
  std::free(learners);
  std::free(ring);
  std::free(counter);
  std::free(scratch);
  std::free(table);
  std::free(member);
  return bad;
}

int main() {
  int bad = 0;
  if (mg_abi_version() != 21) ++bad;
  bad += host_population_run(3, 10, 5, 5);
  bad += host_population_run(64, 11, 5, 1);
  bad += device_refusals();
  std::printf("learn_many sanitizer run: %d failures\n", bad);
  return bad ? 1 : 0;
}
