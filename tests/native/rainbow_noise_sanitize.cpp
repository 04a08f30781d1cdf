// Host sanitizer driver for the device-noise entry points (test infrastructure):
// tests/test_rainbow_noise_sanitize.py links this file against merging_hip.hip compiled with -Xarch_host
// -fsanitize=address / undefined. The host twins mg_host_rainbow_noise and mg_host_rainbow_ndtri run on exactly
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

static int expect_error(int rc, const char* needle, const char* what) {
  if (rc == 0 || !std::strstr(mg_last_error(), needle)) {
    std::printf("FAIL: %s: rc %d, message '%s'\n", what, rc, mg_last_error());
    return 1;
  }
  return 0;
}

constexpr int kFactors = 1124;

// U = 0, 1, 3 and n = 0, 1, 65: every factor finite and nonzero, every z finite and odd about one half.
static int host_run() {
  int bad = 0;
  for (int U : {0, 1, 3}) {
    const size_t n = static_cast<size_t>(U) * 2 * kFactors;
    float* out = exact<float>(n);
    if (mg_host_rainbow_noise(0x8000000000000005ull, 0xffffffffull, U, out) != 0) {
      std::printf("FAIL: mg_host_rainbow_noise: %s\n", mg_last_error());
      ++bad;
    }
    for (size_t i = 0; i < n; ++i)
      if (!std::isfinite(out[i]) || out[i] == 0.0f) ++bad;
    std::free(out);
  }
  for (int n : {0, 1, 65}) {
    double* u = exact<double>(n);
    double* z = exact<double>(n);
    for (int i = 0; i < n; ++i) u[i] = std::ldexp(1.0, -53 + (i % 53)) * (i % 2 ? 1.0 : 1.5);  // all three branches
    if (n > 1) u[1] = 0.0, u[2] = 1.0;                                                           // NaN
    if (mg_host_rainbow_ndtri(u, z, n) != 0) {
      std::printf("FAIL: mg_host_rainbow_ndtri: %s\n", mg_last_error());
      ++bad;
    }
    for (int i = 0; i < n; ++i)
      if (std::isfinite(z[i]) != (u[i] > 0.0 && u[i] < 1.0)) ++bad;
    std::free(u), std::free(z);
  }
  return bad;
}

// The entry points refuse before anything is launched or read.
static int refusals() {
  int bad = 0;
  float* f = exact<float>(2 * kFactors);
  double* d = exact<double>(8);
  char* fb = reinterpret_cast<char*>(f);
  char* db = reinterpret_cast<char*>(d);
  bad += expect_error(mg_rainbow_noise(1, 0, 1, nullptr, nullptr), "mg_rainbow_noise: NULL", "noise: NULL");
  bad += expect_error(mg_rainbow_noise(1, 0, -1, f, nullptr), "num_updates < 0", "noise: U < 0");
  bad += expect_error(mg_rainbow_noise(1, 0, 1, reinterpret_cast<float*>(fb + 2), nullptr), "4-byte aligned",
                      "noise: misaligned");
  bad += expect_error(mg_host_rainbow_noise(1, 0, 1, nullptr), "mg_host_rainbow_noise: NULL", "host noise: NULL");
  bad += expect_error(mg_host_rainbow_noise(1, 0, -1, f), "num_updates < 0", "host noise: U < 0");
  bad += expect_error(mg_host_rainbow_noise(1, 0, 1, reinterpret_cast<float*>(fb + 1)), "4-byte aligned",
                      "host noise: misaligned");
  bad += expect_error(mg_rainbow_ndtri(nullptr, d, 4, nullptr), "mg_rainbow_ndtri: NULL", "ndtri: NULL u");
  bad += expect_error(mg_rainbow_ndtri(d, nullptr, 4, nullptr), "mg_rainbow_ndtri: NULL", "ndtri: NULL z");
  bad += expect_error(mg_rainbow_ndtri(d, d + 4, -1, nullptr), "n < 0", "ndtri: n < 0");
  bad += expect_error(mg_rainbow_ndtri(reinterpret_cast<double*>(db + 4), d + 4, 2, nullptr), "8-byte aligned",
                      "ndtri: misaligned u");
  bad += expect_error(mg_host_rainbow_ndtri(nullptr, d, 4), "mg_host_rainbow_ndtri: NULL", "host ndtri: NULL u");
  bad += expect_error(mg_host_rainbow_ndtri(d, d + 4, -1), "n < 0", "host ndtri: n < 0");
  bad += expect_error(mg_host_rainbow_ndtri(d, reinterpret_cast<double*>(db + 36), 2), "8-byte aligned",
                      "host ndtri: misaligned z");
  if (mg_rainbow_noise(1, 0, 0, f, nullptr) != 0 || mg_rainbow_ndtri(d, d + 4, 0, nullptr) != 0) ++bad;  // nothing to do
  std::free(f), std::free(d);
  return bad;
}

int main() {
  int bad = 0;
  if (mg_abi_version() != 21) ++bad;
  bad += host_run();
  bad += refusals();
  std::printf("rainbow noise sanitizer run: %d failures\n", bad);
  return bad ? 1 : 0;
}
