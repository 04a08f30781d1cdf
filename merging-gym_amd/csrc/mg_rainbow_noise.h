// mg_rainbow_noise.h -- the Rainbow learner's noisy-net factors drawn on the device: a counter-based stream
// keyed by (noise_seed, update, model, factor) -- Philox words, a 52-bit uniform, the inverse normal CDF in fp64
// (Wichura's AS 241, PPND16) and _scale_noise's sign(x) sqrt|x| -- with the per-element functions the host twin
// (mg_host_rainbow_noise) runs too, so both fill the same [U][2][kRlFactors] bits. The contract is in
// include/merging_hip.h at mg_rainbow_noise. A population's factors [U][M][2][kRlFactors] come from one launch
// of the same functions (mg_rainbow_noise_many).
// A part of the one translation unit merging_hip.hip (see its head comment).
#pragma once

#include "mg_common.h"
#include "mg_launch.h"
#include "mg_learn_core.h"
#include "mg_per.h"
#include "mg_rainbow_learn.h"

namespace {

// ---------------------------------------------------------------------------- per-element functions
// The uniform of factor f of model m at update t: 52 bits of learn_words' block at counter
// (2^63 | (m kRlFactors + f), t) -- the top bit keeps it apart from the minibatch draws (b < 1024) under the same
// key -- as (k + 0.5) 2^-52: exact, never 0, 0.5 or 1, and 1 - u is exact too.
MG_HD double rn_uniform(uint64_t noise_seed, uint64_t t, int m, int f) {
  uint32_t w0, w1;
  learn_words((uint64_t{1} << 63) | static_cast<uint64_t>(m * kRlFactors + f), t, noise_seed, w0, w1);
  const uint64_t k = (static_cast<uint64_t>(w0 >> 6) << 26) | static_cast<uint64_t>(w1 >> 6);
  return (static_cast<double>(k) + 0.5) * (1.0 / 4503599627370496.0);
}

// c[0] + r (c[1] + r (... + r c[7])), from c[7] down: acc = acc * r + c[i], two roundings a term.
MG_HD double rn_horner(const double (&c)[8], double r) {
  double acc = c[7];
#pragma unroll
  for (int i = 6; i >= 0; --i) acc = acc * r + c[i];
  return acc;
}

// Phi^-1(u), fp64, for a normal u in (0, 1) (NaN otherwise): AS 241's PPND16 with the coefficients as CPython's
// statistics.py writes them. q = u - 0.5; |q| <= 0.425: r = 0.180625 - q q, z = (q A(r)) / B(r). Else
// r = sqrt(-per_log(min(u, 1 - u))); r <= 5: z = C(r - 1.6) / D(r - 1.6), else z = E(r - 5) / F(r - 5); negated
// where q < 0. Every polynomial in Horner form from its highest coefficient, numerator then denominator then one
// division; every operation rounded once (no fma), the sqrt correctly rounded.
MG_HD double rn_ndtri(double u) {
  constexpr double A[8] = {3.3871328727963666080e+0, 1.3314166789178437745e+2, 1.9715909503065514427e+3,
                           1.3731693765509461125e+4, 4.5921953931549871457e+4, 6.7265770927008700853e+4,
                           3.3430575583588128105e+4, 2.5090809287301226727e+3};
  constexpr double B[8] = {1.0, 4.2313330701600911252e+1, 6.8718700749205790830e+2, 5.3941960214247511077e+3,
                           2.1213794301586595867e+4, 3.9307895800092710610e+4, 2.8729085735721942674e+4,
                           5.2264952788528545610e+3};
  constexpr double C[8] = {1.42343711074968357734e+0, 4.63033784615654529590e+0, 5.76949722146069140550e+0,
                           3.64784832476320460504e+0, 1.27045825245236838258e+0, 2.41780725177450611770e-1,
                           2.27238449892691845833e-2, 7.74545014278341407640e-4};
  constexpr double D[8] = {1.0, 2.05319162663775882187e+0, 1.67638483018380384940e+0, 6.89767334985100004550e-1,
                           1.48103976427480074590e-1, 1.51986665636164571966e-2, 5.47593808499534494600e-4,
                           1.05075007164441684324e-9};
  constexpr double E[8] = {6.65790464350110377720e+0, 5.46378491116411436990e+0, 1.78482653991729133580e+0,
                           2.96560571828504891230e-1, 2.65321895265761230930e-2, 1.24266094738807843860e-3,
                           2.71155556874348757815e-5, 2.01033439929228813265e-7};
  constexpr double F[8] = {1.0, 5.99832206555887937690e-1, 1.36929880922735805310e-1, 1.48753612908506148525e-2,
                           7.86869131145613259100e-4, 1.84631831751005468180e-5, 1.42151175831644588870e-7,
                           2.04426310338993978564e-15};
  if (!(u >= 2.2250738585072014e-308 && u < 1.0)) return NAN;
  const double q = u - 0.5;
  if (fabs(q) <= 0.425) {
    const double r = 0.180625 - q * q;
    return (rn_horner(A, r) * q) / rn_horner(B, r);
  }
  const double p = q < 0.0 ? u : 1.0 - u;
  double r = sqrt(-per_log(p));
  double z;
  if (r <= 5.0) {
    r = r - 1.6;
    z = rn_horner(C, r) / rn_horner(D, r);
  } else {
    r = r - 5.0;
    z = rn_horner(E, r) / rn_horner(F, r);
  }
  return q < 0.0 ? -z : z;
}

// The factor: x = fp32(z) rounded to nearest, then sign(x) sqrtf(|x|) (_scale_noise, :493-496). x is never 0.
MG_HD float rn_factor_at(uint64_t noise_seed, uint64_t t, int m, int f) {
  const float x = static_cast<float>(rn_ndtri(rn_uniform(noise_seed, t, m, f)));
  return x < 0.0f ? -sqrtf(-x) : sqrtf(x);
}

// Element i of [U][2][kRlFactors]: update first_update + u, model m, factor f.
MG_HD float rn_noise_at(uint64_t noise_seed, uint64_t first_update, int64_t i) {
  const int64_t u = i / (2 * kRlFactors);
  const int r = static_cast<int>(i - u * (2 * kRlFactors));
  return rn_factor_at(noise_seed, first_update + static_cast<uint64_t>(u), r / kRlFactors, r % kRlFactors);
}

// ---------------------------------------------------------------------------- kernels
// One thread per factor, consecutive threads consecutive floats. Six lanes in seven take the central branch.
__global__ __launch_bounds__(kBlock) void rainbow_noise_kernel(uint64_t noise_seed, uint64_t first_update, int64_t n,
                                                               float* out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i < n) out[i] = rn_noise_at(noise_seed, first_update, i);
}

// The inverse CDF alone, so a test reaches the far tail (u < e^-25), which no small stream hits.
__global__ __launch_bounds__(kBlock) void rainbow_ndtri_kernel(const double* u, double* z, int64_t n) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i < n) z[i] = rn_ndtri(u[i]);
}

// ---------------------------------------------------------------------------- host side of a call
MG_HD int64_t rn_noise_items(int32_t num_updates) { return static_cast<int64_t>(num_updates) * 2 * kRlFactors; }

int check_rainbow_noise(const char* what, int32_t num_updates, const float* noise_out) {
  if (!noise_out) return fail(hipErrorInvalidValue, "%s: NULL pointer", what);
  if (num_updates < 0) return fail(hipErrorInvalidValue, "%s: num_updates < 0", what);
  if (misaligned(noise_out, 3)) return fail(hipErrorInvalidValue, "%s: noise_out must be 4-byte aligned", what);
  if (rn_noise_items(num_updates) > static_cast<int64_t>(0x7fffffff) * kBlock)
    return fail(hipErrorInvalidValue, "%s: num_updates exceeds the grid limit", what);
  return 0;
}

int check_rainbow_ndtri(const char* what, const double* u, const double* z, int64_t n) {
  if (!u || !z) return fail(hipErrorInvalidValue, "%s: NULL pointer", what);
  if (n < 0) return fail(hipErrorInvalidValue, "%s: n < 0", what);
  if (misaligned(u, 7) || misaligned(z, 7)) return fail(hipErrorInvalidValue, "%s: u and z must be 8-byte aligned", what);
  if (n > static_cast<int64_t>(0x7fffffff) * kBlock) return fail(hipErrorInvalidValue, "%s: n exceeds the grid limit", what);
  return 0;
}

void launch_rainbow_noise(uint64_t noise_seed, uint64_t first_update, int32_t num_updates, float* out, hipStream_t st) {
  const int64_t n = rn_noise_items(num_updates);
  hipLaunchKernelGGL(rainbow_noise_kernel, dim3(grid_blocks(n)), dim3(kBlock), 0, st, noise_seed, first_update, n, out);
}
void host_rainbow_noise(uint64_t noise_seed, uint64_t first_update, int32_t num_updates, float* out) {
  for (int64_t i = 0; i < rn_noise_items(num_updates); ++i) out[i] = rn_noise_at(noise_seed, first_update, i);
}

// ---------------------------------------------------------------------------- a population's factors
// [U][M][2][kRlFactors] in one launch: element (u, m, model, f) = rn_factor_at(noise_seed[m], first_update[m] + u,
// model, f), what mg_rainbow_noise gives member m. The members' keys travel in the kernel argument (64 x 16 B).
// Each (u, m) takes kRnBlocks whole blocks, so a block's member is uniform and its key arrives by scalar loads.
struct RnMany {
  uint64_t noise_seed[kMaxMembers];
  uint64_t first_update[kMaxMembers];
  int32_t members;
};
static_assert(sizeof(RnMany) <= 1100, "the by-value kernel argument stays well inside HIP's 4096 bytes");
constexpr int kRnBlocks = (2 * kRlFactors + kBlock - 1) / kBlock;

MG_HD float rn_noise_many_at(const RnMany& R, int64_t um, int r) {
  const int m = static_cast<int>(um % R.members);
  return rn_factor_at(R.noise_seed[m], R.first_update[m] + static_cast<uint64_t>(um / R.members), r / kRlFactors,
                      r % kRlFactors);
}

__global__ __launch_bounds__(kBlock) void rainbow_noise_many_kernel(const RnMany R, float* out) {
  const int64_t um = blockIdx.x / kRnBlocks;
  const int r = static_cast<int>(blockIdx.x % kRnBlocks) * kBlock + threadIdx.x;
  if (r < 2 * kRlFactors) out[um * (2 * kRlFactors) + r] = rn_noise_many_at(R, um, r);
}

int check_rainbow_noise_many(const char* what, const uint64_t* noise_seed, const uint64_t* first_update,
                             int32_t members, int32_t num_updates, const float* noise_out) {
  if (!members_ok(members)) return fail(hipErrorInvalidValue, "%s: need 1 <= members <= 64", what);
  if (!noise_seed || !first_update || !noise_out) return fail(hipErrorInvalidValue, "%s: NULL pointer", what);
  if (num_updates < 0) return fail(hipErrorInvalidValue, "%s: num_updates < 0", what);
  if (misaligned(noise_out, 3)) return fail(hipErrorInvalidValue, "%s: noise_out must be 4-byte aligned", what);
  if (static_cast<int64_t>(num_updates) * members > static_cast<int64_t>(0x7fffffff) / kRnBlocks)
    return fail(hipErrorInvalidValue, "%s: num_updates * members exceeds the grid limit", what);
  return 0;
}

RnMany make_rainbow_noise_many(const uint64_t* noise_seed, const uint64_t* first_update, int32_t members) {
  RnMany R{};
  for (int m = 0; m < members; ++m) R.noise_seed[m] = noise_seed[m], R.first_update[m] = first_update[m];
  R.members = members;
  return R;
}
void launch_rainbow_noise_many(const RnMany& R, int32_t num_updates, float* out, hipStream_t st) {
  const int64_t um = static_cast<int64_t>(num_updates) * R.members;
  if (um == 0) return;
  hipLaunchKernelGGL(rainbow_noise_many_kernel, dim3(static_cast<unsigned>(um * kRnBlocks)), dim3(kBlock), 0, st, R,
                     out);
}
void host_rainbow_noise_many(const RnMany& R, int32_t num_updates, float* out) {
  for (int64_t um = 0; um < static_cast<int64_t>(num_updates) * R.members; ++um)
    for (int r = 0; r < 2 * kRlFactors; ++r) out[um * (2 * kRlFactors) + r] = rn_noise_many_at(R, um, r);
}

void launch_rainbow_ndtri(const double* u, double* z, int64_t n, hipStream_t st) {
  hipLaunchKernelGGL(rainbow_ndtri_kernel, dim3(grid_blocks(n)), dim3(kBlock), 0, st, u, z, n);
}
void host_rainbow_ndtri(const double* u, double* z, int64_t n) {
  for (int64_t i = 0; i < n; ++i) z[i] = rn_ndtri(u[i]);
}

}  // namespace
