/* Plain-C restatement of the Rainbow head's contract (include/merging_hip.h, "Rainbow acting"), written from
 * that text alone: it shares no code with csrc/. Compiled by the tests with the C compiler
 * (-ffp-contract=off, no fast-math) and loaded with ctypes (tests/rainbow_ref.py).
 *
 *   rainbow_exp_ref(x, y, n)                      y[i] = the contract's exp(x[i])
 *   rainbow_head_ref(logits, z, q, action, n)     logits [n][306], z [51] -> q [n][5], action [n]
 */
#include <math.h>
#include <stdint.h>

#define ATOMS 51
#define ACTIONS 5
#define CHAIN 13 /* atoms per chain: four chains */

static float exp_ref(float x) {
  static const float coef[8] = {1.0f / 5040.0f, 1.0f / 720.0f, 1.0f / 120.0f, 1.0f / 24.0f,
                                1.0f / 6.0f,    0.5f,          1.0f,          1.0f};
  if (!(x >= -87.0f)) return 0.0f;
  const float k = nearbyintf(x * 1.44269504088896341f);
  const float r = fmaf(k, 2.12194440e-4f, fmaf(k, -0.693359375f, x));
  float p = coef[0];
  for (int c = 1; c < 8; ++c) p = fmaf(p, r, coef[c]);
  return ldexpf(p, (int)k); /* exact: every result here is a normal number */
}

void rainbow_exp_ref(const float* x, float* y, int64_t n) {
  for (int64_t i = 0; i < n; ++i) y[i] = exp_ref(x[i]);
}

void rainbow_head_ref(const float* logits, const float* z, float* q, int8_t* action, int64_t n) {
  for (int64_t row = 0; row < n; ++row) {
    const float* v = logits + row * (ATOMS * (1 + ACTIONS));
    const float* adv = v + ATOMS;
    float mean[ATOMS];
    for (int i = 0; i < ATOMS; ++i) {
      float s = adv[i] + adv[ATOMS + i];
      s = s + adv[2 * ATOMS + i];
      s = s + adv[3 * ATOMS + i];
      s = s + adv[4 * ATOMS + i];
      mean[i] = s / 5.0f;
    }
    int best = 0;
    float qbest = 0.0f;
    for (int a = 0; a < ACTIONS; ++a) {
      float x[ATOMS];
      float top = -INFINITY;
      for (int i = 0; i < ATOMS; ++i) {
        const float t = v[i] + adv[a * ATOMS + i];
        x[i] = t - mean[i];
        if (x[i] > top) top = x[i];
      }
      float den[4], num[4];
      for (int c = 0; c < 4; ++c) {
        den[c] = 0.0f;
        num[c] = 0.0f;
        for (int i = CHAIN * c; i < CHAIN * c + CHAIN && i < ATOMS; ++i) {
          const float e = exp_ref(x[i] - top);
          const float ez = e * z[i];
          den[c] = den[c] + e;
          num[c] = num[c] + ez;
        }
      }
      const float d01 = den[0] + den[1], d23 = den[2] + den[3];
      const float n01 = num[0] + num[1], n23 = num[2] + num[3];
      const float qa = (n01 + n23) / (d01 + d23);
      if (q) q[row * ACTIONS + a] = qa;
      if (a == 0 || qa > qbest) {
        qbest = qa;
        best = a;
      }
    }
    if (action) action[row] = (int8_t)best;
  }
}
