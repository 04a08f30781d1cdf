/* Plain-C restatement of the Rainbow learner's device noise stream (include/merging_hip.h, mg_rainbow_noise),
 * written from the header's contract and sharing no code with the library: Philox4x32-10, the 52-bit uniform,
 * AS 241's PPND16 on fdlibm's log, and _scale_noise. tests/rainbow_noise_ref.py compiles it with the C compiler
 * (-O2 -ffp-contract=off) and loads it with ctypes. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define FACTORS 1124

/* Philox4x32-10 (Salmon et al. 2011): ten rounds, the key bumped by the Weyl constants between them. */
static void philox(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t c[4] = {ctr[0], ctr[1], ctr[2], ctr[3]};
  uint32_t k[2] = {key[0], key[1]};
  for (int round = 0; round < 10; ++round) {
    const uint64_t hi_lo_a = (uint64_t)0xD2511F53u * c[0];
    const uint64_t hi_lo_b = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n[4] = {(uint32_t)(hi_lo_b >> 32) ^ c[1] ^ k[0], (uint32_t)hi_lo_b,
                           (uint32_t)(hi_lo_a >> 32) ^ c[3] ^ k[1], (uint32_t)hi_lo_a};
    memcpy(c, n, sizeof(c));
    k[0] += 0x9E3779B9u;
    k[1] += 0xBB67AE85u;
  }
  memcpy(out, c, sizeof(c));
}

/* step 1 and 2: the uniform of (seed, update t, model m, factor f) */
static double uniform_ref(uint64_t seed, uint64_t t, int m, int f) {
  const uint64_t b = 0x8000000000000000ull | (uint64_t)(m * FACTORS + f);
  const uint32_t ctr[4] = {(uint32_t)b, (uint32_t)(b >> 32), (uint32_t)t, (uint32_t)(t >> 32)};
  const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  uint32_t w[4];
  philox(ctr, key, w);
  const uint64_t k = ((uint64_t)(w[0] >> 6) << 26) | (uint64_t)(w[1] >> 6);
  return ((double)k + 0.5) * 0x1p-52;
}

/* fdlibm e_log.c (Sun Microsystems, 1993) for a normal positive x, its special cases left out */
static double log_ref(double x) {
  static const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10,
                      Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01,
                      Lg4 = 2.222219843214978396e-01, Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
                      Lg7 = 1.479819860511658591e-01;
  uint64_t bits;
  memcpy(&bits, &x, 8);
  int32_t hx = (int32_t)(bits >> 32);
  const uint32_t lx = (uint32_t)bits;
  int k = (hx >> 20) - 1023;
  hx &= 0x000fffff;
  const int32_t i = (hx + 0x95f64) & 0x100000;
  hx |= i ^ 0x3ff00000; /* normalize x or x / 2 */
  k += i >> 20;
  bits = ((uint64_t)(uint32_t)hx << 32) | lx;
  double m;
  memcpy(&m, &bits, 8);
  const double f = m - 1.0;
  const double s = f / (2.0 + f);
  const double dk = (double)k;
  const double z = s * s;
  const double w = z * z;
  const double t1 = w * (Lg2 + w * (Lg4 + w * Lg6));
  const double t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)));
  const double R = t2 + t1;
  const double hfsq = 0.5 * f * f;
  return dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f);
}

/* step 3: AS 241, PPND16, as CPython's statistics.py writes it */
static double ndtri_one(double p) {
  if (!(p >= 0x1p-1022 && p < 1.0)) return NAN;
  const double q = p - 0.5;
  double r, num, den, x;
  if (fabs(q) <= 0.425) {
    r = 0.180625 - q * q;
    num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r +
               4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
            1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) * q;
    den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r +
               2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
            4.2313330701600911252e+1) * r + 1.0);
    return num / den;
  }
  r = q <= 0.0 ? p : 1.0 - p;
  r = sqrt(-log_ref(r));
  if (r <= 5.0) {
    r = r - 1.6;
    num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
               1.27045825245236838258e+0) * r + 3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r +
            4.63033784615654529590e+0) * r + 1.42343711074968357734e+0);
    den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
               1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r +
            2.05319162663775882187e+0) * r + 1.0);
  } else {
    r = r - 5.0;
    num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r +
               2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r +
            5.46378491116411436990e+0) * r + 6.65790464350110377720e+0);
    den = (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r +
               7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
            5.99832206555887937690e-1) * r + 1.0);
  }
  x = num / den;
  return q < 0.0 ? -x : x;
}

void ndtri_ref(const double* u, double* z, int64_t n) {
  for (int64_t i = 0; i < n; ++i) z[i] = ndtri_one(u[i]);
}

void uniform_ref_fill(uint64_t noise_seed, uint64_t first_update, int32_t U, double* out) {
  for (int32_t u = 0; u < U; ++u)
    for (int m = 0; m < 2; ++m)
      for (int f = 0; f < FACTORS; ++f)
        out[((int64_t)u * 2 + m) * FACTORS + f] = uniform_ref(noise_seed, first_update + (uint64_t)u, m, f);
}

/* step 4, over [U][2][1124] */
void noise_ref(uint64_t noise_seed, uint64_t first_update, int32_t U, float* out) {
  for (int32_t u = 0; u < U; ++u)
    for (int m = 0; m < 2; ++m)
      for (int f = 0; f < FACTORS; ++f) {
        const float x = (float)ndtri_one(uniform_ref(noise_seed, first_update + (uint64_t)u, m, f));
        const float a = sqrtf(fabsf(x));
        out[((int64_t)u * 2 + m) * FACTORS + f] = x > 0.0f ? a : x < 0.0f ? -a : 0.0f * x;
      }
}
