/* Plain-C restatement of one Rainbow update (scripts/ranbowdqn.py:554-609) in the operation order
 * include/merging_hip.h documents at mg_rainbow_learn. Test infrastructure: it shares no code with csrc/;
 * tests/rainbow_learn_ref.py compiles it with the C compiler at test time (-ffp-contract=off) and compares
 * mg_host_rainbow_learn and mg_rainbow_learn against it bit for bit. Everything is written as whole-array
 * loops over [batch][unit] tables, not per item. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { IN = 10, H1 = 32, H2 = 64, HS = 64, NA = 5, NZ = 51, NL = 306, ROW = 24 };
enum { NP = 58884, NE = 28210, NF = 1124, PLAIN = 2464 };
enum { OFF_W1 = 0, OFF_B1 = 320, OFF_W2 = 352, OFF_B2 = 2400 };
static const int OUT[4] = {64, 51, 64, 255};          /* value1, value2, advantage1, advantage2 */
static const int POFF[4] = {2464, 10784, 17414, 25734}; /* weight_mu of the layer in a parameter block */
static const int EOFF[4] = {0, 4160, 7475, 11635};      /* weight_epsilon of the layer in a noise block */
static const int FOFF[4] = {0, 192, 358, 550};          /* eps_in of the layer in a model's factors */

static uint32_t philox_x(uint64_t b, uint64_t draw, uint64_t seed) {
  uint32_t c[4] = {(uint32_t)b, (uint32_t)(b >> 32), (uint32_t)draw, (uint32_t)(draw >> 32)};
  uint32_t k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  for (int round = 0; round < 10; ++round) {
    const uint64_t a = (uint64_t)0xD2511F53u * c[0], d = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n[4] = {(uint32_t)(d >> 32) ^ c[1] ^ k[0], (uint32_t)d, (uint32_t)(a >> 32) ^ c[3] ^ k[1], (uint32_t)a};
    memcpy(c, n, sizeof n);
    k[0] += 0x9E3779B9u;
    k[1] += 0xBB67AE85u;
  }
  return c[0];
}

static float exp_ref(float x) { /* the library's exp for x <= 0 */
  if (!(x >= -87.0f)) return 0.0f;
  const float k = rintf(x * 1.44269504088896341f);
  float r = fmaf(k, -0.693359375f, x);
  r = fmaf(k, 2.12194440e-4f, r);
  const float c[8] = {1.0f / 5040.0f, 1.0f / 720.0f, 1.0f / 120.0f, 1.0f / 24.0f, 1.0f / 6.0f, 0.5f, 1.0f, 1.0f};
  float p = c[0];
  for (int i = 1; i < 8; ++i) p = fmaf(p, r, c[i]);
  return ldexpf(p, (int)k);
}

static float log_ref(float x) { /* the library's log for normal x > 0 */
  int e;
  float m = frexpf(x, &e); /* x = m 2^e, m in [0.5, 1) */
  union { float f; uint32_t u; } bits = {m};
  if (bits.u < 0x3f3504f3u) { /* below sqrt(1/2) as the bit pattern orders it */
    m = m * 2.0f;
    e = e - 1;
  }
  const float f = m - 1.0f, dk = (float)e;
  const float s = f / (2.0f + f);
  const float z = s * s, w = z * z;
  const float t1 = w * (0.40000972152f + w * 0.24279078841f);
  const float t2 = z * (0.66666662693f + w * 0.28498786688f);
  const float R = t2 + t1;
  const float h = (0.5f * f) * f;
  float y = s * (h + R) + dk * 9.0580006145e-06f;
  y = y - h;
  y = y + f;
  return y + dk * 6.9313812256e-01f;
}

float rainbow_log_ref(float x) { return log_ref(x); }

static float sum4(const float* v) {
  float c[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int i = 0; i < NZ; ++i) c[i / 13] = c[i / 13] + v[i];
  return (c[0] + c[1]) + (c[2] + c[3]);
}

static float relu(float y) { return y > 0.0f ? y : 0.0f; }

static float dot(float bias, const float* x, const float* w, int K) {
  float acc = bias;
  for (int k = 0; k < K; ++k) acc = fmaf(x[k], w[k], acc);
  return acc;
}

typedef struct {
  float h1[H1], h2[H2], hv[HS], ha[HS], prob[NA][NZ];
} Acts;

/* P: a parameter block; eff: that model's effective noisy weights in the noise block's layout */
static void forward(const float* P, const float* eff, const float* x, Acts* A) {
  float lg[NL];
  for (int j = 0; j < H1; ++j) A->h1[j] = relu(dot(P[OFF_B1 + j], x, P + OFF_W1 + j * IN, IN));
  for (int j = 0; j < H2; ++j) A->h2[j] = relu(dot(P[OFF_B2 + j], A->h1, P + OFF_W2 + j * H1, H1));
  for (int j = 0; j < HS; ++j) {
    A->hv[j] = relu(dot(eff[EOFF[0] + 64 * HS + j], A->h2, eff + EOFF[0] + j * H2, H2));
    A->ha[j] = relu(dot(eff[EOFF[2] + 64 * HS + j], A->h2, eff + EOFF[2] + j * H2, H2));
  }
  for (int j = 0; j < NZ; ++j) lg[j] = dot(eff[EOFF[1] + NZ * HS + j], A->hv, eff + EOFF[1] + j * HS, HS);
  for (int j = 0; j < NA * NZ; ++j) lg[NZ + j] = dot(eff[EOFF[3] + NA * NZ * HS + j], A->ha, eff + EOFF[3] + j * HS, HS);
  float mean[NZ];
  for (int i = 0; i < NZ; ++i) {
    float t = lg[NZ + i];
    for (int a = 1; a < NA; ++a) t = t + lg[NZ + a * NZ + i];
    mean[i] = t / 5.0f;
  }
  for (int a = 0; a < NA; ++a) {
    float x2[NZ], m = -INFINITY;
    for (int i = 0; i < NZ; ++i) {
      x2[i] = (lg[i] + lg[NZ + a * NZ + i]) - mean[i];
      if (x2[i] > m) m = x2[i];
    }
    for (int i = 0; i < NZ; ++i) x2[i] = exp_ref(x2[i] - m);
    const float S = sum4(x2);
    for (int i = 0; i < NZ; ++i) A->prob[a][i] = x2[i] / S;
  }
}

void rainbow_project_ref(const float* nd, float r, float done, float gamma, const float* z, float* proj) {
  float b[NZ];
  for (int i = 0; i < NZ; ++i) {
    float tz = r + ((1.0f - done) * gamma) * z[i];
    if (tz < -10.0f) tz = -10.0f;
    if (tz > 10.0f) tz = 10.0f;
    b[i] = (tz + 10.0f) / 0.4f;
    proj[i] = 0.0f;
  }
  for (int i = 0; i < NZ; ++i) proj[(int)floorf(b[i])] += nd[i] * (ceilf(b[i]) - b[i]);
  for (int i = 0; i < NZ; ++i) proj[(int)ceilf(b[i])] += nd[i] * (b[i] - floorf(b[i]));
}

/* g[j][k] = the fmaf chain over the batch of dy[b][j] x[b][k]; gb[j] = the sequential sum of dy[b][j] */
static void weight_grads(const float* dy, int sdy, const float* x, int sx, int B, int J, int K, float* gW, float* gb) {
  for (int j = 0; j < J; ++j) {
    for (int k = 0; k < K; ++k) {
      float acc = 0.0f;
      for (int b = 0; b < B; ++b) acc = fmaf(dy[b * sdy + j], x[b * sx + k], acc);
      gW[j * K + k] = acc;
    }
    float acc = 0.0f;
    for (int b = 0; b < B; ++b) acc = acc + dy[b * sdy + j];
    gb[j] = acc;
  }
}

/* dx[b][k] = the fmaf chain over j of dy[b][j] W[j][k] (no mask) */
static void input_grads(const float* dy, int sdy, const float* W, int B, int J, int K, float* dx) {
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < K; ++k) {
      float acc = 0.0f;
      for (int j = 0; j < J; ++j) acc = fmaf(dy[b * sdy + j], W[j * K + k], acc);
      dx[b * K + k] = acc;
    }
}

static void effective(const float* L, float* eff) { /* eff [2][NE] from both models' parameters and noise */
  for (int m = 0; m < 2; ++m)
    for (int l = 0; l < 4; ++l) {
      const int nw = OUT[l] * HS;
      const float* P = L + m * NP + POFF[l];
      const float* eps = L + 4 * NP + m * NE + EOFF[l];
      float* e = eff + m * NE + EOFF[l];
      for (int i = 0; i < nw; ++i) e[i] = P[i] + P[nw + i] * eps[i];
      for (int j = 0; j < OUT[l]; ++j) e[nw + j] = P[2 * nw + j] + P[2 * nw + OUT[l] + j] * eps[nw + j];
    }
}

int rainbow_learn_ref(float* L, const float* ring, uint64_t counter, int64_t cap, int32_t B, int32_t U,
                      uint64_t first_update, uint64_t seed, uint64_t first_draw, double lr, double gamma, double beta1,
                      double beta2, double eps, const float* noise, float* loss_out, float* rows_out, float* proj_out,
                      float* grads_out) {
  const float* z = L + 4 * NP + 2 * NE;
  float* eff = malloc(sizeof(float) * 2 * NE);
  float* geff = malloc(sizeof(float) * NE);
  float* g = malloc(sizeof(float) * NP);
  Acts* cur = malloc(sizeof(Acts) * B);
  float* rows = malloc(sizeof(float) * B * ROW);
  float* proj = malloc(sizeof(float) * B * NZ);
  float* dlog = malloc(sizeof(float) * B * NL);
  float* dhv = malloc(sizeof(float) * B * HS);
  float* dha = malloc(sizeof(float) * B * HS);
  float* dh2 = malloc(sizeof(float) * B * H2);
  float* dh2a = malloc(sizeof(float) * B * H2);
  float* dh1 = malloc(sizeof(float) * B * H1);
  float* act = malloc(sizeof(float) * B * (H1 + H2 + 2 * HS));
  float *h1 = act, *h2 = h1 + B * H1, *hv = h2 + B * H2, *ha = hv + B * HS;
  float* lossb = malloc(sizeof(float) * B);
  const float gam = (float)gamma, inv_b = (float)(1.0 / B);
  uint64_t live = counter < (uint64_t)cap ? counter : (uint64_t)cap;
  if (live == 0) live = 1;
  for (int u = 0; u < U; ++u) {
    effective(L, eff);
    for (int b = 0; b < B; ++b) {
      const uint64_t slot = ((uint64_t)philox_x((uint64_t)b, first_draw + u, seed) * live) >> 32;
      memcpy(rows + b * ROW, ring + slot * ROW, sizeof(float) * ROW);
    }
    if (rows_out) memcpy(rows_out + (size_t)u * B * ROW, rows, sizeof(float) * B * ROW);
    /* the target: projection of the target model's distribution at s' */
    for (int b = 0; b < B; ++b) {
      const float* row = rows + b * ROW;
      Acts T;
      forward(L + NP, eff + NE, row + 12, &T);
      float nd[NA][NZ], q[NA];
      int best = 0;
      for (int a = 0; a < NA; ++a) {
        for (int i = 0; i < NZ; ++i) nd[a][i] = T.prob[a][i] * z[i];
        q[a] = sum4(nd[a]);
        if (q[a] > q[best]) best = a;
      }
      rainbow_project_ref(nd[best], row[11], row[22], gam, z, proj + b * NZ);
    }
    if (proj_out) memcpy(proj_out + (size_t)u * B * NZ, proj, sizeof(float) * B * NZ);
    /* the current model at s: loss and the gradient at the logits */
    for (int b = 0; b < B; ++b) {
      const float* row = rows + b * ROW;
      forward(L, eff, row, &cur[b]);
      memcpy(h1 + b * H1, cur[b].h1, sizeof cur[b].h1);
      memcpy(h2 + b * H2, cur[b].h2, sizeof cur[b].h2);
      memcpy(hv + b * HS, cur[b].hv, sizeof cur[b].hv);
      memcpy(ha + b * HS, cur[b].ha, sizeof cur[b].ha);
      int a = !(row[10] >= 0.0f) ? 0 : row[10] >= 5.0f ? 4 : (int)row[10];
      const float* y = cur[b].prob[a];
      const float* pr = proj + b * NZ;
      float gl[NZ], acc = 0.0f, d = 0.0f;
      for (int i = 0; i < NZ; ++i) {
        const float c = y[i] < 0.01f ? 0.01f : y[i] > 0.99f ? 0.99f : y[i];
        acc = acc + pr[i] * log_ref(c);
        gl[i] = -(pr[i] / c) * inv_b;
        d = fmaf(gl[i], y[i], d);
      }
      lossb[b] = -acc;
      float* dl = dlog + b * NL;
      for (int i = 0; i < NZ; ++i) {
        const float dx = y[i] * (gl[i] - d), fifth = dx / 5.0f;
        dl[i] = dx;
        for (int a2 = 0; a2 < NA; ++a2) dl[NZ + a2 * NZ + i] = a2 == a ? dx - fifth : -fifth;
      }
    }
    /* backward */
    weight_grads(dlog, NL, hv, HS, B, NZ, HS, geff + EOFF[1], geff + EOFF[1] + NZ * HS);
    weight_grads(dlog + NZ, NL, ha, HS, B, NA * NZ, HS, geff + EOFF[3], geff + EOFF[3] + NA * NZ * HS);
    input_grads(dlog, NL, eff + EOFF[1], B, NZ, HS, dhv);
    input_grads(dlog + NZ, NL, eff + EOFF[3], B, NA * NZ, HS, dha);
    for (int i = 0; i < B * HS; ++i) {
      if (!(hv[i] > 0.0f)) dhv[i] = 0.0f;
      if (!(ha[i] > 0.0f)) dha[i] = 0.0f;
    }
    weight_grads(dhv, HS, h2, H2, B, HS, H2, geff + EOFF[0], geff + EOFF[0] + HS * H2);
    weight_grads(dha, HS, h2, H2, B, HS, H2, geff + EOFF[2], geff + EOFF[2] + HS * H2);
    input_grads(dhv, HS, eff + EOFF[0], B, HS, H2, dh2);
    input_grads(dha, HS, eff + EOFF[2], B, HS, H2, dh2a);
    for (int i = 0; i < B * H2; ++i) dh2[i] = h2[i] > 0.0f ? dh2[i] + dh2a[i] : 0.0f;
    weight_grads(dh2, H2, h1, H1, B, H2, H1, g + OFF_W2, g + OFF_B2);
    input_grads(dh2, H2, L + OFF_W2, B, H2, H1, dh1);
    for (int i = 0; i < B * H1; ++i)
      if (!(h1[i] > 0.0f)) dh1[i] = 0.0f;
    weight_grads(dh1, H1, rows, ROW, B, H1, IN, g + OFF_W1, g + OFF_B1);
    for (int l = 0; l < 4; ++l) { /* g_mu = g_w, g_sigma = g_w eps, weights then biases */
      const int nw = OUT[l] * HS;
      const float* ge = geff + EOFF[l];
      const float* ep = L + 4 * NP + EOFF[l];
      float* gp = g + POFF[l];
      for (int i = 0; i < nw; ++i) gp[i] = ge[i], gp[nw + i] = ge[i] * ep[i];
      for (int j = 0; j < OUT[l]; ++j) gp[2 * nw + j] = ge[nw + j], gp[2 * nw + OUT[l] + j] = ge[nw + j] * ep[nw + j];
    }
    if (grads_out) memcpy(grads_out + (size_t)u * NP, g, sizeof(float) * NP);
    /* Adam */
    const double step = (double)(first_update + u + 1);
    const float b1 = (float)beta1, omb1 = (float)(1.0 - beta1), b2 = (float)beta2, omb2 = (float)(1.0 - beta2);
    const float ss = (float)(lr / (1.0 - pow(beta1, step))), bc2 = (float)sqrt(1.0 - pow(beta2, step)), ep = (float)eps;
    float *m = L + 2 * NP, *v = L + 3 * NP;
    for (int i = 0; i < NP; ++i) {
      m[i] = fmaf(omb1, g[i], b1 * m[i]);
      v[i] = fmaf(omb2 * g[i], g[i], b2 * v[i]);
      const float den = sqrtf(v[i]) / bc2 + ep;
      L[i] = L[i] - ss * (m[i] / den);
    }
    if (loss_out) {
      float acc = 0.0f;
      for (int b = 0; b < B; ++b) acc = acc + lossb[b];
      loss_out[u] = acc * inv_b;
    }
    /* reset_noise of the current model, then the target's */
    for (int mdl = 0; mdl < 2; ++mdl)
      for (int l = 0; l < 4; ++l) {
        const float* F = noise + ((size_t)u * 2 + mdl) * NF + FOFF[l];
        float* ep2 = L + 4 * NP + mdl * NE + EOFF[l];
        for (int j = 0; j < OUT[l]; ++j) {
          for (int k = 0; k < HS; ++k) ep2[j * HS + k] = F[HS + j] * F[k];
          ep2[OUT[l] * HS + j] = F[HS + OUT[l] + j];
        }
      }
  }
  free(eff), free(geff), free(g), free(cur), free(rows), free(proj), free(dlog), free(dhv), free(dha), free(dh2);
  free(dh2a), free(dh1), free(act), free(lossb);
  return 0;
}

/* Every fp32 in [lo, hi] through `lib_log` (the library's mg_host_rainbow_log) in blocks: the largest distance
 * in units of the last place from libm's logf, and how many values differ from it or from log_ref above. */
int64_t rainbow_log_scan(int (*lib_log)(const float*, float*, int64_t), float lo, float hi, int64_t* count,
                         int64_t* off_libm, int64_t* off_ref) {
  enum { BLOCK = 1 << 16 };
  static float x[BLOCK], y[BLOCK];
  union { float f; uint32_t u; } a = {lo}, b = {hi};
  int64_t worst = 0;
  *count = *off_libm = *off_ref = 0;
  for (uint64_t first = a.u; first <= b.u; first += BLOCK) {
    const int64_t n = b.u - first + 1 < BLOCK ? (int64_t)(b.u - first + 1) : BLOCK;
    for (int64_t i = 0; i < n; ++i) {
      union { uint32_t u; float f; } v = {(uint32_t)(first + i)};
      x[i] = v.f;
    }
    if (lib_log(x, y, n) != 0) return -1;
    for (int64_t i = 0; i < n; ++i) {
      union { float f; int32_t s; } got = {y[i]}, want = {logf(x[i])}, ref = {log_ref(x[i])};
      const int64_t d = got.s > want.s ? (int64_t)got.s - want.s : (int64_t)want.s - got.s;
      if (d > worst) worst = d;
      *off_libm += d != 0;
      *off_ref += got.s != ref.s;
    }
    *count += n;
  }
  return worst;
}
