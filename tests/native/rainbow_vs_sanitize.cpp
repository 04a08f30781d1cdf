// Host sanitizer driver for the Rainbow rollouts against another net (test infrastructure):
// tests/test_rainbow_vs_sanitize.py compiles merging_hip.hip with -Xarch_host -fsanitize=address / undefined and links
// this file. mg_rollout_rainbow_vs_many reads two host arrays the caller sizes by `members` -- the members' nets and
// their opponents -- so both are exactly sized heap blocks of 1, 3 and 64 entries here and the sanitizers see a read
// past entry members - 1. Each argument check of mg_rollout_rainbow_vs and mg_rollout_rainbow_vs_many is driven once;
// every call returns before anything is launched (nothing here touches a GPU), and the pointers that stand for device
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

struct Batch {
  mg_params P;
  mg_state S;
  mg_traj T;
  Batch() {
    mg_params_default(&P);
    double* d = reinterpret_cast<double*>(kDev);
    S = mg_state{d, d, d, d, d, d, reinterpret_cast<uint16_t*>(kDev)};
    std::memset(&T, 0, sizeof(T));
  }
};

static int lone_checks() {
  Batch B;
  const void* net = kDev + 131072;
  const void* opp = kDev + 262144;
  auto call = [&](const mg_params* p, const mg_state* s, const mg_traj* t, int64_t n, int steps, const void* a,
                  const void* b) { return mg_rollout_rainbow_vs(p, s, t, nullptr, n, steps, a, b, MG_AUTORESET, nullptr); };
  int bad = 0;
  bad += expect_error(call(nullptr, &B.S, &B.T, 64, 4, net, opp), "params is NULL", "NULL params");
  bad += expect_error(call(&B.P, nullptr, &B.T, 64, 4, net, opp), "NULL array", "NULL state");
  bad += expect_error(call(&B.P, &B.S, nullptr, 64, 4, net, opp), "traj is NULL", "NULL traj");
  bad += expect_error(call(&B.P, &B.S, &B.T, -1, 4, net, opp), "n < 0", "negative n");
  bad += expect_error(call(&B.P, &B.S, &B.T, 64, 4, nullptr, opp), "mg_rollout_rainbow_vs: net must be", "NULL net");
  bad += expect_error(call(&B.P, &B.S, &B.T, 64, 4, kDev + 8, opp), "mg_rollout_rainbow_vs: net must be",
                      "misaligned net");
  bad += expect_error(call(&B.P, &B.S, &B.T, 64, 4, net, nullptr), "mg_rollout_rainbow_vs: opponent must be",
                      "NULL opponent");
  bad += expect_error(call(&B.P, &B.S, &B.T, 64, 4, net, kDev + 8), "mg_rollout_rainbow_vs: opponent must be",
                      "misaligned opponent");
  bad += expect_error(call(&B.P, &B.S, &B.T, 64, -1, net, opp), "mg_rollout_rainbow_vs: need 0 <= num_steps <= 65535",
                      "num_steps -1");
  bad += expect_error(call(&B.P, &B.S, &B.T, 64, 65536, net, opp),
                      "mg_rollout_rainbow_vs: need 0 <= num_steps <= 65535", "num_steps 65536");
  B.T.obs = reinterpret_cast<float*>(kDev + 4);
  bad += expect_error(call(&B.P, &B.S, &B.T, 64, 4, net, opp), "traj.obs must be 16-byte", "misaligned traj.obs");
  B.T.obs = nullptr;
  bad += expect_ok(call(&B.P, &B.S, &B.T, 64, 0, net, opp), "num_steps 0");
  bad += expect_ok(call(&B.P, &B.S, &B.T, 0, 4, net, net), "n 0, the net its own opponent");
  B.P.timeout_steps = 0;
  bad += expect_error(call(&B.P, &B.S, &B.T, 64, 4, net, opp), "timeout_steps", "timeout_steps 0");
  return bad;
}

static int member_checks(int M) {
  Batch B;
  const void** nets = exact<const void*>(M);
  const void** opps = exact<const void*>(M);
  for (int m = 0; m < M; ++m) {
    nets[m] = kDev + 131072 * (m + 1);
    opps[m] = kDev + 131072 * ((m + 1) % M + 1);  // the next member's net
  }
  auto call = [&](const mg_params* p, const mg_state* s, const mg_traj* t, int64_t n_member, int members, int steps,
                  const void* const* a, const void* const* b) {
    return mg_rollout_rainbow_vs_many(p, s, t, nullptr, n_member, members, steps, a, b, MG_AUTORESET, nullptr);
  };
  const char* const who = "mg_rollout_rainbow_vs_many: ";
  char want[96];
  auto text = [&](const char* tail) {
    std::snprintf(want, sizeof(want), "%s%s", who, tail);
    return want;
  };
  int bad = 0;
  bad += expect_error(call(&B.P, &B.S, &B.T, 64, 0, 4, nets, opps), text("need 1 <= members <= 64"), "members 0");
  bad += expect_error(call(&B.P, &B.S, &B.T, 64, 65, 4, nets, opps), text("need 1 <= members <= 64"), "members 65");
  bad += expect_error(call(&B.P, &B.S, &B.T, -64, M, 4, nets, opps), text("n_member < 0"), "negative n_member");
  bad += expect_error(call(&B.P, &B.S, &B.T, 96, M, 4, nets, opps), text("n_member must be a multiple of 64"),
                      "n_member 96");
  bad += expect_error(call(&B.P, &B.S, &B.T, int64_t{1} << 40, M, 4, nets, opps),
                      text("members * n_member exceeds the grid limit"), "n_member 2^40");
  bad += expect_error(call(&B.P, &B.S, &B.T, INT64_MAX - 63, M, 4, nets, opps),
                      text("members * n_member exceeds the grid limit"), "the largest multiple of 64");
  bad += expect_error(call(nullptr, &B.S, &B.T, 64, M, 4, nets, opps), "params is NULL", "NULL params");
  bad += expect_error(call(&B.P, nullptr, &B.T, 64, M, 4, nets, opps), "NULL array", "NULL state");
  bad += expect_error(call(&B.P, &B.S, nullptr, 64, M, 4, nets, opps), "traj is NULL", "NULL traj");
  bad += expect_error(call(&B.P, &B.S, &B.T, 64, M, 4, nullptr, opps), text("nets is NULL"), "NULL nets");
  bad += expect_error(call(&B.P, &B.S, &B.T, 64, M, 4, nets, nullptr), text("opponents is NULL"), "NULL opponents");
  const int last = M - 1;
  const void* keep = nets[last];
  std::snprintf(want, sizeof(want), "%smember %d: net must be a 16-byte aligned", who, last);
  nets[last] = nullptr;
  bad += expect_error(call(&B.P, &B.S, &B.T, 64, M, 4, nets, opps), want, "the last net NULL");
  nets[last] = kDev + 8;
  bad += expect_error(call(&B.P, &B.S, &B.T, 64, M, 4, nets, opps), want, "the last net misaligned");
  nets[last] = keep;
  keep = opps[last];
  std::snprintf(want, sizeof(want), "%smember %d: opponent must be a 16-byte aligned", who, last);
  opps[last] = nullptr;
  bad += expect_error(call(&B.P, &B.S, &B.T, 64, M, 4, nets, opps), want, "the last opponent NULL");
  opps[last] = kDev + 8;
  bad += expect_error(call(&B.P, &B.S, &B.T, 64, M, 4, nets, opps), want, "the last opponent misaligned");
  bad += expect_error(call(&B.P, &B.S, &B.T, 0, M, 4, nets, opps), want, "the last opponent misaligned, n_member 0");
  opps[0] = nullptr;  // the first offending member is the one named
  std::snprintf(want, sizeof(want), "%smember 0: opponent must be", who);
  bad += expect_error(call(&B.P, &B.S, &B.T, 64, M, 4, nets, opps), want, "the first of two bad opponents");
  opps[0] = nets[0];  // a member against itself
  opps[last] = keep;
  bad += expect_error(call(&B.P, &B.S, &B.T, 64, M, -1, nets, opps), text("need 0 <= num_steps <= 65535"),
                      "num_steps -1");
  bad += expect_error(call(&B.P, &B.S, &B.T, 64, M, 65536, nets, opps), text("need 0 <= num_steps <= 65535"),
                      "num_steps 65536");
  B.T.rew = reinterpret_cast<float*>(kDev + 4);
  bad += expect_error(call(&B.P, &B.S, &B.T, 64, M, 4, nets, opps), "traj.obs must be 16-byte", "misaligned traj.rew");
  B.T.rew = nullptr;
  bad += expect_ok(call(&B.P, &B.S, &B.T, 64, M, 0, nets, opps), "num_steps 0");
  bad += expect_ok(call(&B.P, &B.S, &B.T, 0, M, 4, nets, nets), "n_member 0, every member its own opponent");
  std::free(nets);
  std::free(opps);
  return bad;
}

int main() {
  int bad = 0;
  if (mg_abi_version() != 21) ++bad;
  bad += lone_checks();
  for (int M : {1, 3, 64}) bad += member_checks(M);
  std::printf("rainbow vs sanitizer run: %d failures\n", bad);
  return bad ? 1 : 0;
}
