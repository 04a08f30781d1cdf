// Host sanitizer driver for the population's acting entry points (test infrastructure):
// tests/test_population_acting_host.py compiles merging_hip.hip with -Xarch_host -fsanitize=address / undefined and
// links this file. mg_rollout_qnet_many and mg_replay_store_many read host arrays the caller sizes by `members` --
// the mg_qnet_actor list, the rings' and counters' pointer lists -- so every list here is an exactly sized heap
// block and the sanitizers see a read past member members - 1. Each argument check is driven once; every call
// returns before anything is launched (nothing here touches a GPU), and the pointers that stand for device
// memory are never dereferenced. Any sanitizer report aborts the run.
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

// stands for device memory: aligned, never dereferenced on the host
static char* const kDev = reinterpret_cast<char*>(uintptr_t{1} << 20);

static int rollout_checks(int M) {
  mg_params P;
  mg_params_default(&P);
  double* d = reinterpret_cast<double*>(kDev);
  mg_state S{d, d, d, d, d, d, reinterpret_cast<uint16_t*>(kDev)};
  mg_traj T;
  std::memset(&T, 0, sizeof(T));
  mg_qnet_actor* actors = exact<mg_qnet_actor>(M);
  for (int m = 0; m < M; ++m) actors[m] = mg_qnet_actor{kDev + 4096 * m, kDev + 4096 * (M - 1 - m), 7u + m, 1u << 31, 1u << 30};
  auto call = [&](const mg_params* p, const mg_state* s, const mg_traj* t, int64_t n_member, int members, int steps,
                  const mg_qnet_actor* a, int out_dim, int mode) {
    return mg_rollout_qnet_many(p, s, t, nullptr, n_member, members, 0, 500, steps, a, out_dim, mode, MG_AUTORESET, nullptr);
  };
  int bad = 0;
  bad += expect_error(call(&P, &S, &T, 64, 0, 4, actors, 5, 0), "1 <= members <= 64", "0 members");
  bad += expect_error(call(&P, &S, &T, 64, 65, 4, actors, 5, 0), "1 <= members <= 64", "65 members");
  bad += expect_error(call(&P, &S, &T, 64, -1, 4, actors, 5, 0), "1 <= members <= 64", "-1 members");
  bad += expect_error(call(&P, &S, &T, -64, M, 4, actors, 5, 0), "n_member < 0", "negative n_member");
  bad += expect_error(call(&P, &S, &T, 96, M, 4, actors, 5, 0), "multiple of 64", "n_member 96");
  bad += expect_error(call(&P, &S, &T, 1, M, 4, actors, 5, 0), "multiple of 64", "n_member 1");
  bad += expect_error(call(&P, &S, &T, int64_t{1} << 40, M, 4, actors, 5, 0), "grid limit", "n_member 2^40");
  bad += expect_error(call(nullptr, &S, &T, 64, M, 4, actors, 5, 0), "params is NULL", "NULL params");
  bad += expect_error(call(&P, nullptr, &T, 64, M, 4, actors, 5, 0), "NULL array", "NULL state");
  bad += expect_error(call(&P, &S, nullptr, 64, M, 4, actors, 5, 0), "traj is NULL", "NULL traj");
  bad += expect_error(call(&P, &S, &T, 64, M, 4, nullptr, 5, 0), "actors is NULL", "NULL actors");
  bad += expect_error(call(&P, &S, &T, 64, M, -1, actors, 5, 0), "num_steps >= 0", "negative num_steps");
  bad += expect_error(call(&P, &S, &T, 64, M, 4, actors, 0, 0), "1 <= out_dim <= 8", "out_dim 0");
  bad += expect_error(call(&P, &S, &T, 64, M, 4, actors, 9, 0), "1 <= out_dim <= 8", "out_dim 9");
  bad += expect_error(call(&P, &S, &T, 64, M, 4, actors, 5, -1), "opponent_mode", "mode -1");
  bad += expect_error(call(&P, &S, &T, 64, M, 4, actors, 5, 4), "opponent_mode", "mode 4");
  char want[64];
  const int last = M - 1;
  actors[last].net = nullptr;
  std::snprintf(want, sizeof(want), "member %d: net", last);
  bad += expect_error(call(&P, &S, &T, 64, M, 4, actors, 5, 0), want, "the last member's net NULL");
  actors[last].net = kDev + 8;
  bad += expect_error(call(&P, &S, &T, 64, M, 4, actors, 5, 2), want, "the last member's net misaligned");
  actors[last].net = kDev;
  actors[last].opp_net = nullptr;
  std::snprintf(want, sizeof(want), "member %d: opponent_mode 3 needs opp_net", last);
  bad += expect_error(call(&P, &S, &T, 64, M, 4, actors, 5, 3), want, "mode 3 without the last member's opp_net");
  actors[last].opp_net = kDev + 4;
  bad += expect_error(call(&P, &S, &T, 64, M, 4, actors, 5, 3), want, "mode 3 with a misaligned opp_net");
  bad += expect_ok(call(&P, &S, &T, 0, M, 4, actors, 5, 2), "n_member 0 (opp_net unused in mode 2)");
  actors[last].opp_net = kDev;
  T.obs = reinterpret_cast<float*>(kDev + 4);
  bad += expect_error(call(&P, &S, &T, 64, M, 4, actors, 5, 3), "traj.obs must be 16-byte", "misaligned traj.obs");
  T.obs = nullptr;
  bad += expect_ok(call(&P, &S, &T, 64, M, 0, actors, 5, 3), "num_steps 0");
  bad += expect_ok(call(&P, &S, &T, 0, M, 4, actors, 5, 3), "n_member 0");
  P.timeout_steps = 0;
  bad += expect_error(call(&P, &S, &T, 64, M, 4, actors, 5, 0), "timeout_steps", "timeout_steps 0");
  std::free(actors);
  return bad;
}

static int store_checks(int M) {
  float** rows = exact<float*>(M);
  uint64_t** counters = exact<uint64_t*>(M);
  for (int m = 0; m < M; ++m) {
    rows[m] = reinterpret_cast<float*>(kDev + 65536 * (m + 1));
    counters[m] = reinterpret_cast<uint64_t*>(kDev + 8 * m);
  }
  mg_transitions X;
  std::memset(&X, 0, sizeof(X));
  const float* f = reinterpret_cast<const float*>(kDev);
  X.obs_first = X.obs = X.rew = X.final_obs = f;
  X.flags = reinterpret_cast<const uint8_t*>(kDev);
  X.won_mask = reinterpret_cast<const uint64_t*>(kDev);
  const size_t sb = mg_replay_scratch_many_bytes(320, 3, M);
  auto call = [&](float* const* r, uint64_t* const* c, int members, int64_t cap, int rf, const mg_transitions* t,
                  int64_t n_member, int steps, void* scratch, size_t bytes) {
    return mg_replay_store_many(r, c, members, cap, rf, t, n_member, steps, 1, scratch, bytes, nullptr);
  };
  int bad = 0;
  if (sb != static_cast<size_t>(M) * mg_replay_scratch_bytes(320, 3) || sb == 0 || sb % 8 != 0) {
    std::printf("FAIL: mg_replay_scratch_many_bytes(320, 3, %d) = %zu\n", M, sb);
    ++bad;
  }
  if (mg_replay_scratch_many_bytes(320, 3, 0) != 0 || mg_replay_scratch_many_bytes(320, 3, 65) != 0 ||
      mg_replay_scratch_many_bytes(0, 3, M) != 0 || mg_replay_scratch_many_bytes(320, 0, M) != 0)
    ++bad;
  bad += expect_error(call(rows, counters, 0, 2000, 22, &X, 320, 3, kDev, sb), "1 <= members <= 64", "0 members");
  bad += expect_error(call(rows, counters, 65, 2000, 22, &X, 320, 3, kDev, sb), "1 <= members <= 64", "65 members");
  bad += expect_error(call(nullptr, counters, M, 2000, 22, &X, 320, 3, kDev, sb), "NULL pointer", "NULL rows");
  bad += expect_error(call(rows, nullptr, M, 2000, 22, &X, 320, 3, kDev, sb), "NULL pointer", "NULL counters");
  bad += expect_error(call(rows, counters, M, 2000, 22, nullptr, 320, 3, kDev, sb), "NULL pointer", "NULL transitions");
  const int last = M - 1;
  float* keep_row = rows[last];
  uint64_t* keep_counter = counters[last];
  rows[last] = nullptr;
  bad += expect_error(call(rows, counters, M, 2000, 22, &X, 320, 3, kDev, sb), "NULL pointer", "the last member's rows NULL");
  rows[last] = reinterpret_cast<float*>(kDev + 4);
  bad += expect_error(call(rows, counters, M, 2000, 22, &X, 320, 3, kDev, sb), "8-byte aligned", "misaligned rows");
  rows[last] = keep_row;
  counters[last] = nullptr;
  bad += expect_error(call(rows, counters, M, 2000, 22, &X, 320, 3, kDev, sb), "NULL pointer", "the last member's counter NULL");
  counters[last] = keep_counter;
  if (M > 1) {
    rows[last] = rows[0];
    bad += expect_error(call(rows, counters, M, 2000, 22, &X, 320, 3, kDev, sb), "listed twice", "a ring twice");
    rows[last] = keep_row;
    counters[last] = counters[0];
    bad += expect_error(call(rows, counters, M, 2000, 22, &X, 320, 3, kDev, sb), "listed twice", "a counter twice");
    counters[last] = keep_counter;
  }
  bad += expect_error(call(rows, counters, M, 0, 22, &X, 320, 3, kDev, sb), "capacity < 1", "capacity 0");
  bad += expect_error(call(rows, counters, M, 2000, 24, &X, 320, 3, kDev, sb), "22-float rows only", "24-float rows");
  X.goal = f;
  bad += expect_error(call(rows, counters, M, 2000, 22, &X, 320, 3, kDev, sb), "22-float rows only", "goal set");
  X.goal = nullptr;
  X.next_goal = f;
  bad += expect_error(call(rows, counters, M, 2000, 22, &X, 320, 3, kDev, sb), "22-float rows only", "next_goal set");
  X.next_goal = nullptr;
  X.meta_goal = f;
  bad += expect_error(call(rows, counters, M, 2000, 22, &X, 320, 3, kDev, sb), "22-float rows only", "meta_goal set");
  X.meta_goal = nullptr;
  bad += expect_error(call(rows, counters, M, 2000, 22, &X, -64, 3, kDev, sb), "n_member < 0", "negative n_member");
  bad += expect_error(call(rows, counters, M, 2000, 22, &X, 320, -1, kDev, sb), "num_steps < 0", "negative num_steps");
  bad += expect_error(call(rows, counters, M, 2000, 22, &X, 100, 3, kDev, sb), "multiple of 64", "n_member 100");
  bad += expect_ok(call(rows, counters, M, 2000, 22, &X, 0, 3, nullptr, 0), "n_member 0");
  bad += expect_ok(call(rows, counters, M, 2000, 22, &X, 320, 0, nullptr, 0), "num_steps 0");
  X.obs = nullptr;
  bad += expect_error(call(rows, counters, M, 2000, 22, &X, 320, 3, kDev, sb), "are required", "obs NULL");
  X.obs = f;
  X.flags = nullptr;
  bad += expect_error(call(rows, counters, M, 2000, 22, &X, 320, 3, kDev, sb), "are required", "neither a1 nor flags");
  X.flags = reinterpret_cast<const uint8_t*>(kDev);
  X.rew = f + 1;
  bad += expect_error(call(rows, counters, M, 2000, 22, &X, 320, 3, kDev, sb), "8-byte aligned", "misaligned rew");
  X.rew = f;
  X.reward = reinterpret_cast<const float*>(kDev + 2);
  bad += expect_error(call(rows, counters, M, 2000, 22, &X, 320, 3, kDev, sb), "4-byte aligned", "misaligned reward");
  X.reward = nullptr;
  bad += expect_error(call(rows, counters, M, 2000, 22, &X, 320, 3, nullptr, sb), "scratch smaller", "NULL scratch");
  bad += expect_error(call(rows, counters, M, 2000, 22, &X, 320, 3, kDev, sb - 8), "scratch smaller", "short scratch");
  bad += expect_error(call(rows, counters, M, 2000, 22, &X, 320, 3, kDev + 4, sb), "8-byte aligned", "misaligned scratch");
  bad += expect_error(call(rows, counters, M, 2000, 22, &X, 64, 200000, kDev, mg_replay_scratch_many_bytes(64, 200000, M)),
                      "num_steps too large", "200,000 steps");
  std::free(rows);
  std::free(counters);
  return bad;
}

int main() {
  int bad = 0;
  if (mg_abi_version() != 21) ++bad;
  for (int M : {1, 3, 64}) {
    bad += rollout_checks(M);
    bad += store_checks(M);
  }
  std::printf("population_act sanitizer run: %d failures\n", bad);
  return bad ? 1 : 0;
}
