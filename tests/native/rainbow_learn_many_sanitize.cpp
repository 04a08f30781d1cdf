// Host sanitizer driver for the Rainbow population's entry points (test infrastructure):
// tests/test_rainbow_learn_many_sanitize.py compiles merging_hip.hip with -Xarch_host -fsanitize=address /
// undefined and links this file. mg_host_rainbow_learn_many and mg_host_rainbow_noise_many run at batch 33 with
// three members on exactly sized heap buffers, so the sanitizers see every access they make -- a member stride
// that is not what rl_scratch rounds its sections to would run past the scratch; the device entry points only
// get as far as their argument checks (nothing here launches a kernel). Any sanitizer report aborts the run.
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

constexpr int kParams = 58884, kEps = 28210, kFactors = 1124, kAtoms = 51, kRow = 24;
constexpr int kLearner = 4 * kParams + 2 * kEps + 52;
constexpr int M = 3, B = 33, U = 2;
constexpr int64_t kCap = 48;

// Two updates of three members (two of them on one ring, one ring partly filled, one wrapped) with the population's
// own noise and every optional output, one more without any output, and the call without an update.
static int host_run() {
  int bad = 0;
  float* L = exact<float>(static_cast<size_t>(M) * kLearner);
  for (int m = 0; m < M; ++m) {
    float* l = L + static_cast<size_t>(m) * kLearner;
    for (int i = 0; i < kParams; ++i) l[i] = 0.1f * unit();
    std::memcpy(l + kParams, l, sizeof(float) * kParams);
    for (int i = 0; i < 2 * kEps; ++i) l[4 * kParams + i] = unit();
    for (int i = 0; i < kAtoms; ++i) l[4 * kParams + 2 * kEps + i] = -10.0f + 0.4f * static_cast<float>(i);
  }
  float* ring[2];
  uint64_t* counter[2];
  for (int r = 0; r < 2; ++r) {
    ring[r] = exact<float>(kCap * kRow);
    counter[r] = exact<uint64_t>(1);
    *counter[r] = r == 0 ? 40 : 200;
    for (int64_t i = 0; i < (r == 0 ? 40 : kCap); ++i) {
      for (int k = 0; k < kRow; ++k) ring[r][i * kRow + k] = 3.0f * unit();
      ring[r][i * kRow + 10] = static_cast<float>(i % 7) - 1.0f;  // actions outside 0..4 are kept inside
      ring[r][i * kRow + 11] = i % 5 == 0 ? 10.0f : i % 5 == 1 ? -25.0f : 0.4f * static_cast<float>(i % 9);
      ring[r][i * kRow + 22] = static_cast<float>(i & 1);
      ring[r][i * kRow + 23] = 0.0f;
    }
  }
  mg_dqn_member* member = exact<mg_dqn_member>(M);
  uint64_t* seeds = exact<uint64_t>(M);
  uint64_t* first = exact<uint64_t>(M);
  for (int m = 0; m < M; ++m) {
    member[m] = mg_dqn_member{ring[m == 1], counter[m == 1], 5u + 11u * m, static_cast<uint64_t>(3 * m),
                              static_cast<uint64_t>(m), {0.001 * (m + 1), 0.99 - 0.01 * m, 0.9, 0.999, 1e-8, 1, 0}};
    seeds[m] = m == 1 ? (uint64_t{1} << 63) + 9u : 77u + m;
    first[m] = m == 2 ? (uint64_t{1} << 32) + 1u : member[m].first_update;
  }
  float* noise = exact<float>(static_cast<size_t>(U) * M * 2 * kFactors);
  if (mg_host_rainbow_noise_many(seeds, first, M, U, noise) != 0) {
    std::printf("FAIL: mg_host_rainbow_noise_many: %s\n", mg_last_error());
    ++bad;
  }
  float* lone = exact<float>(static_cast<size_t>(U) * 2 * kFactors);
  for (int m = 0; m < M; ++m) {  // element (u, m, ...) is member m's lone stream
    if (mg_host_rainbow_noise(seeds[m], first[m], U, lone) != 0) ++bad;
    for (int u = 0; u < U; ++u)
      if (std::memcmp(lone + static_cast<size_t>(u) * 2 * kFactors,
                      noise + (static_cast<size_t>(u) * M + m) * 2 * kFactors, sizeof(float) * 2 * kFactors) != 0) {
        std::printf("FAIL: noise of member %d, update %d\n", m, u);
        ++bad;
      }
  }
  const size_t sbytes = static_cast<size_t>(M) * mg_rainbow_learn_scratch_bytes(B);
  char* scratch = exact<char>(sbytes);
  float* loss = exact<float>(U * M);
  float* rows = exact<float>(static_cast<size_t>(U) * M * B * kRow);
  float* proj = exact<float>(static_cast<size_t>(U) * M * B * kAtoms);
  float* grads = exact<float>(static_cast<size_t>(U) * M * kParams);
  if (mg_host_rainbow_learn_many(L, member, M, kCap, B, U, noise, loss, rows, proj, grads, scratch, sbytes) != 0) {
    std::printf("FAIL: mg_host_rainbow_learn_many: %s\n", mg_last_error());
    ++bad;
  }
  for (int i = 0; i < U * M; ++i)
    if (!std::isfinite(loss[i])) {
      std::printf("FAIL: loss[%d] = %g\n", i, loss[i]);
      ++bad;
    }
  for (int m = 0; m < M; ++m)
    if (member[m].first_update != static_cast<uint64_t>(3 * m + U) || member[m].first_draw != static_cast<uint64_t>(m + U))
      ++bad;
  if (mg_host_rainbow_learn_many(L, member, M, kCap, B, 1, noise, nullptr, nullptr, nullptr, nullptr, scratch, sbytes) != 0)
    ++bad;
  if (mg_host_rainbow_learn_many(L, member, M, kCap, B, 0, nullptr, nullptr, nullptr, nullptr, nullptr, scratch, sbytes) != 0)
    ++bad;  // no update: needs no noise, moves no counter
  if (member[0].first_update != static_cast<uint64_t>(U + 1)) ++bad;
  if (mg_host_rainbow_noise_many(seeds, first, M, 0, noise) != 0) ++bad;
  for (void* p : {static_cast<void*>(L), static_cast<void*>(ring[0]), static_cast<void*>(ring[1]),
                  static_cast<void*>(counter[0]), static_cast<void*>(counter[1]), static_cast<void*>(member),
                  static_cast<void*>(seeds), static_cast<void*>(first), static_cast<void*>(noise),
                  static_cast<void*>(lone), static_cast<void*>(scratch), static_cast<void*>(loss),
                  static_cast<void*>(rows), static_cast<void*>(proj), static_cast<void*>(grads)})
    std::free(p);
  return bad;
}

// The device entry points refuse before anything is launched or read; the host twins refuse the same.
static int refusals() {
  int bad = 0;
  float* t = exact<float>(64);
  uint64_t* c = exact<uint64_t>(8);
  char* big = exact<char>(256);
  const size_t sb = 2 * mg_rainbow_learn_scratch_bytes(32);
  const size_t tb = mg_rainbow_learn_many_table_bytes(2);
  const mg_dqn_hyper h = {0.001, 0.99, 0.9, 0.999, 1e-8, 1, 0};
  mg_dqn_member ok[2] = {{t, c, 1, 0, 0, h}, {t, c, 2, 0, 0, h}};
  mg_dqn_member nul[2] = {{t, c, 1, 0, 0, h}, {nullptr, c, 2, 0, 0, h}};
  mg_dqn_member beta[2] = {{t, c, 1, 0, 0, h}, {t, c, 2, 0, 0, h}};
  beta[1].hyper.beta2 = 1.0;
  mg_dqn_member odd[2] = {{t + 1, c, 1, 0, 0, h}, {t, c, 2, 0, 0, h}};
  auto dev = [&](float* l, mg_dqn_member* mem, int members, int b, int u, const float* nz, void* packed, size_t stride,
                 void* scr, size_t bytes, const void* table, size_t tbytes) {
    return mg_rainbow_learn_many(l, table, tbytes, mem, members, 10, b, u, nz, nullptr, nullptr, nullptr, nullptr, packed,
                                 stride, scr, bytes, nullptr);
  };
  auto host = [&](float* l, mg_dqn_member* mem, int members, int b, int u, const float* nz, void* scr, size_t bytes) {
    return mg_host_rainbow_learn_many(l, mem, members, 10, b, u, nz, nullptr, nullptr, nullptr, nullptr, scr, bytes);
  };
  for (int which = 0; which < 2; ++which) {
    auto call = [&](float* l, mg_dqn_member* mem, int members, int b, int u, const float* nz, void* scr, size_t bytes) {
      return which ? host(l, mem, members, b, u, nz, scr, bytes)
                   : dev(l, mem, members, b, u, nz, nullptr, 0, scr, bytes, big, tb);
    };
    bad += expect_error(call(t, ok, 0, 32, 1, t, big, sb), "members", "learn: 0 members");
    bad += expect_error(call(t, ok, 65, 32, 1, t, big, sb), "members", "learn: 65 members");
    bad += expect_error(call(nullptr, ok, 2, 32, 1, t, big, sb), "NULL", "learn: NULL learners");
    bad += expect_error(call(t, nullptr, 2, 32, 1, t, big, sb), "NULL", "learn: NULL member");
    bad += expect_error(call(t, ok, 2, 32, 1, t, nullptr, sb), "NULL", "learn: NULL scratch");
    bad += expect_error(call(t, nul, 2, 32, 1, t, big, sb), "member 1: NULL", "learn: member 1 NULL rows");
    bad += expect_error(call(t, ok, 2, 0, 1, t, big, sb), "batch", "learn: batch 0");
    bad += expect_error(call(t, ok, 2, 32, -1, t, big, sb), "num_updates", "learn: -1 updates");
    bad += expect_error(call(t, ok, 2, 32, 1, nullptr, big, sb), "noise is NULL", "learn: no noise");
    bad += expect_error(call(t, beta, 2, 32, 1, t, big, sb), "member 1: need 0 <= beta1", "learn: member 1 beta2 1");
    bad += expect_error(call(t + 1, ok, 2, 32, 1, t, big, sb), "aligned", "learn: learners misaligned");
    bad += expect_error(call(t, odd, 2, 32, 1, t, big, sb), "member 0: rows and counter", "learn: member 0 misaligned");
    bad += expect_error(call(t, ok, 2, 32, 1, t, big, sb - 1), "scratch smaller", "learn: scratch short");
  }
  bad += expect_error(dev(t, ok, 2, 32, 1, t, big + 8, 74192, big, sb, big, tb), "aligned", "learn: packed_out misaligned");
  bad += expect_error(dev(t, ok, 2, 32, 1, t, big, 74192 - 16, big, sb, big, tb), "packed_stride smaller", "learn: stride");
  bad += expect_error(dev(t, ok, 2, 32, 1, t, nullptr, 0, big, sb, nullptr, tb), "table is NULL", "learn: NULL table");
  bad += expect_error(dev(t, ok, 2, 32, 1, t, nullptr, 0, big, sb, big, tb - 1), "table smaller", "learn: table short");
  bad += expect_error(mg_rainbow_learn_many_init(big, tb, ok, 0, nullptr), "members", "init: 0 members");
  bad += expect_error(mg_rainbow_learn_many_init(nullptr, tb, ok, 2, nullptr), "table is NULL", "init: NULL table");
  bad += expect_error(mg_rainbow_learn_many_init(big, tb, nul, 2, nullptr), "member 1", "init: member 1 NULL rows");
  bad += expect_error(mg_rainbow_learn_many_init(big, tb - 1, ok, 2, nullptr), "table smaller", "init: table short");
  bad += expect_error(mg_rainbow_noise_many(c, c, 0, 1, t, nullptr), "members", "noise: 0 members");
  bad += expect_error(mg_rainbow_noise_many(nullptr, c, 2, 1, t, nullptr), "NULL", "noise: NULL seeds");
  bad += expect_error(mg_rainbow_noise_many(c, c, 2, -1, t, nullptr), "num_updates", "noise: -1 updates");
  bad += expect_error(mg_host_rainbow_noise_many(c, c, 65, 1, t), "members", "host noise: 65 members");
  bad += expect_error(mg_host_rainbow_noise_many(c, c, 2, 1, nullptr), "NULL", "host noise: NULL out");
  bad += expect_error(mg_rainbow_sync_target_many(nullptr, 2, 1, nullptr), "NULL", "sync: NULL learners");
  bad += expect_error(mg_rainbow_sync_target_many(t, 2, 4, nullptr), "mask", "sync: bit 2 of 2 members");
  bad += expect_error(mg_rainbow_sync_target_many(t, 65, 1, nullptr), "members", "sync: 65 members");
  for (int m = 0; m < 2; ++m)
    if (ok[m].first_update != 0 || ok[m].first_draw != 0) ++bad;  // a refused call moves no counter
  if (mg_rainbow_learn_many_table_bytes(0) != 0 || mg_rainbow_learn_many_table_bytes(65) != 0 ||
      mg_rainbow_learn_many_table_bytes(64) != 64 * 48)
    ++bad;
  std::free(t);
  std::free(c);
  std::free(big);
  return bad;
}

int main() {
  int bad = 0;
  if (mg_abi_version() != 21) ++bad;
  bad += host_run();
  bad += refusals();
  std::printf("rainbow learn many sanitizer run: %d failures\n", bad);
  return bad ? 1 : 0;
}
