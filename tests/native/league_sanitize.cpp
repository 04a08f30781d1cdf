// Host sanitizer driver for the league's entry points (test infrastructure): tests/test_league_sanitize.py
// compiles merging_hip.hip with -Xarch_host -fsanitize=address / undefined and links this file.
// mg_rollout_qnet_league reads a host array the caller sizes by `nets` -- the mg_league_net list -- so the list here
// is an exactly sized heap block of 1 and of 64 entries and the sanitizers see a read past entry nets - 1.
// mg_stats_reduce_many's scratch size is driven at the edges of its block count. Each argument check of both entry
// points is driven once; every call returns before anything is launched (nothing here touches a GPU), and the
// pointers that stand for device memory are never dereferenced. Any sanitizer report aborts the run.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "merging_hip.h"

template <class T>
static T* exact(size_t count) {
  void* p = nullptr;
  if (posix_memalign(&p, 16, count * sizeof(T)) != 0 || !p) std::abort();
  std::memset(p, 0, count * sizeof(T));
  return static_cast<T*>(p);
}

static int expect_error(int rc, const char* needle, const char* what) {
  if (rc == 0 || !std::strstr(mg_last_error(), needle)) {
    std::printf("FAIL: %s: rc %d, message '%s'\n", what, rc, mg_last_error());
    return 1;
  }
  return 0;
}

static int expect_ok(int rc, const char* what) {
  if (rc != 0) {
    std::printf("FAIL: %s: rc %d, message '%s'\n", what, rc, mg_last_error());
    return 1;
  }
  return 0;
}

static int expect_size(size_t got, size_t want, const char* what) {
  if (got != want) {
    std::printf("FAIL: %s: %zu, expected %zu\n", what, got, want);
    return 1;
  }
  return 0;
}

// stands for device memory: aligned, never dereferenced on the host
static char* const kDev = reinterpret_cast<char*>(uintptr_t{1} << 20);

static int rollout_checks(int K) {
  mg_params P;
  mg_params_default(&P);
  double* d = reinterpret_cast<double*>(kDev);
  mg_state S{d, d, d, d, d, d, reinterpret_cast<uint16_t*>(kDev)};
  mg_traj T;
  std::memset(&T, 0, sizeof(T));
  mg_league_net* league = exact<mg_league_net>(K);
  for (int k = 0; k < K; ++k) league[k] = mg_league_net{kDev + 4096 * k, 7u + k, uint64_t{1} << (20 + k % 12)};
  auto call = [&](const mg_params* p, const mg_state* s, const mg_traj* t, int64_t n_pair, int nets, int steps,
                  const mg_league_net* l, int out_dim) {
    return mg_rollout_qnet_league(p, s, t, nullptr, n_pair, nets, 0, 500, steps, l, out_dim, MG_AUTORESET, nullptr);
  };
  int bad = 0;
  bad += expect_error(call(&P, &S, &T, 64, 0, 4, league, 5), "1 <= nets <= 64", "0 nets");
  bad += expect_error(call(&P, &S, &T, 64, 65, 4, league, 5), "1 <= nets <= 64", "65 nets");
  bad += expect_error(call(&P, &S, &T, 64, -1, 4, league, 5), "1 <= nets <= 64", "-1 nets");
  bad += expect_error(call(&P, &S, &T, -64, K, 4, league, 5), "n_pair < 0", "negative n_pair");
  bad += expect_error(call(&P, &S, &T, 96, K, 4, league, 5), "multiple of 64", "n_pair 96");
  bad += expect_error(call(&P, &S, &T, 1, K, 4, league, 5), "multiple of 64", "n_pair 1");
  bad += expect_error(call(&P, &S, &T, int64_t{1} << 40, K, 4, league, 5), "grid limit", "n_pair 2^40");
  bad += expect_error(call(&P, &S, &T, INT64_MAX - 63, K, 4, league, 5), "grid limit", "the largest multiple of 64");
  bad += expect_error(call(nullptr, &S, &T, 64, K, 4, league, 5), "params is NULL", "NULL params");
  bad += expect_error(call(&P, nullptr, &T, 64, K, 4, league, 5), "NULL array", "NULL state");
  bad += expect_error(call(&P, &S, nullptr, 64, K, 4, league, 5), "traj is NULL", "NULL traj");
  bad += expect_error(call(&P, &S, &T, 64, K, 4, nullptr, 5), "league is NULL", "NULL league");
  bad += expect_error(call(&P, &S, &T, 64, K, -1, league, 5), "num_steps >= 0", "negative num_steps");
  bad += expect_error(call(&P, &S, &T, 64, K, 4, league, 0), "1 <= out_dim <= 8", "out_dim 0");
  bad += expect_error(call(&P, &S, &T, 64, K, 4, league, 9), "1 <= out_dim <= 8", "out_dim 9");
  char want[64];
  const int last = K - 1;
  league[last].net = nullptr;
  std::snprintf(want, sizeof(want), "net %d: net must be", last);
  bad += expect_error(call(&P, &S, &T, 64, K, 4, league, 5), want, "the last net NULL");
  league[last].net = kDev + 8;
  bad += expect_error(call(&P, &S, &T, 64, K, 4, league, 8), want, "the last net misaligned");
  bad += expect_error(call(&P, &S, &T, 0, K, 4, league, 5), want, "the last net misaligned, n_pair 0");
  league[last].net = kDev;
  T.obs = reinterpret_cast<float*>(kDev + 4);
  bad += expect_error(call(&P, &S, &T, 64, K, 4, league, 5), "traj.obs must be 16-byte", "misaligned traj.obs");
  T.obs = nullptr;
  bad += expect_ok(call(&P, &S, &T, 64, K, 0, league, 5), "num_steps 0");
  bad += expect_ok(call(&P, &S, &T, 0, K, 4, league, 8), "n_pair 0");
  P.timeout_steps = 0;
  bad += expect_error(call(&P, &S, &T, 64, K, 4, league, 5), "timeout_steps", "timeout_steps 0");
  std::free(league);
  return bad;
}

static int reduce_checks(int segments) {
  const mg_episode_stats* rec = reinterpret_cast<const mg_episode_stats*>(kDev);
  mg_stats_totals* tot = reinterpret_cast<mg_stats_totals*>(kDev + 8);
  const size_t one = sizeof(mg_stats_totals);
  int bad = 0;
  // the scratch at the edges of the block count: no record, one, a full block, one past it
  const size_t S = static_cast<size_t>(segments);
  bad += expect_size(mg_stats_reduce_many_scratch_bytes(0, segments), 0, "scratch(0)");
  bad += expect_size(mg_stats_reduce_many_scratch_bytes(-5, segments), 0, "scratch(-5)");
  bad += expect_size(mg_stats_reduce_many_scratch_bytes(1, segments), S * one, "scratch(1)");
  bad += expect_size(mg_stats_reduce_many_scratch_bytes(1024, segments), S * one, "scratch(1024)");
  bad += expect_size(mg_stats_reduce_many_scratch_bytes(1025, segments), 2 * S * one, "scratch(1025)");
  for (int64_t n : {int64_t{1}, int64_t{1024}, int64_t{1025}})
    bad += expect_size(mg_stats_reduce_many_scratch_bytes(n, segments), S * mg_stats_reduce_scratch_bytes(n),
                       "scratch = segments lone scratches");
  const size_t sb = mg_stats_reduce_many_scratch_bytes(1025, segments);
  auto call = [&](const mg_episode_stats* r, int64_t n, int s, mg_stats_totals* t, void* scratch, size_t bytes) {
    return mg_stats_reduce_many(r, n, s, t, scratch, bytes, nullptr);
  };
  bad += expect_error(call(rec, 1025, 0, tot, kDev, sb), "1 <= segments <= 4096", "0 segments");
  bad += expect_error(call(rec, 1025, 4097, tot, kDev, sb), "1 <= segments <= 4096", "4097 segments");
  bad += expect_error(call(rec, 1025, -1, tot, kDev, sb), "1 <= segments <= 4096", "-1 segments");
  bad += expect_error(call(rec, -1, segments, tot, kDev, sb), "n_segment < 0", "negative n_segment");
  bad += expect_error(call(rec, 1025, segments, nullptr, kDev, sb), "NULL pointer", "NULL totals");
  bad += expect_error(call(nullptr, 1025, segments, tot, kDev, sb), "NULL pointer", "NULL rec");
  bad += expect_error(call(nullptr, 0, segments, nullptr, nullptr, 0), "NULL pointer", "NULL totals, no records");
  bad += expect_error(call(reinterpret_cast<const mg_episode_stats*>(kDev + 8), 1025, segments, tot, kDev, sb),
                      "must be 16-byte", "misaligned rec");
  bad += expect_error(call(rec, 1025, segments, tot, kDev + 8, sb), "must be 16-byte", "misaligned scratch");
  bad += expect_error(call(rec, 1025, segments, reinterpret_cast<mg_stats_totals*>(kDev + 4), kDev, sb),
                      "must be 16-byte", "misaligned totals");
  bad += expect_error(call(rec, INT64_MAX, segments, tot, kDev, SIZE_MAX), "grid limit", "the largest n_segment");
  bad += expect_error(call(rec, (int64_t{0x7fffffff} << 10) + 1, segments, tot, kDev, SIZE_MAX), "grid limit",
                      "one record past the grid");
  bad += expect_error(call(rec, 1025, segments, tot, nullptr, sb), "scratch smaller", "NULL scratch");
  bad += expect_error(call(rec, 1025, segments, tot, kDev, sb - 8), "scratch smaller", "short scratch");
  bad += expect_error(call(rec, 1025, segments, tot, kDev, mg_stats_reduce_many_scratch_bytes(1024, segments)),
                      "scratch smaller", "scratch of one block per segment at 1,025 records");
  return bad;
}

int main() {
  int bad = 0;
  if (mg_abi_version() != 21) ++bad;
  if (sizeof(mg_league_net) != 24) ++bad;
  for (int K : {1, 64}) bad += rollout_checks(K);
  for (int segments : {1, 4096}) bad += reduce_checks(segments);
  bad += expect_size(mg_stats_reduce_many_scratch_bytes(1025, 0), 0, "scratch, 0 segments");
  bad += expect_size(mg_stats_reduce_many_scratch_bytes(1025, 4097), 0, "scratch, 4097 segments");
  std::printf("league sanitizer run: %d failures\n", bad);
  return bad ? 1 : 0;
}
