/* dqn_learn_ref.c -- DQN.learn restated in plain C, for the tests only.
 *
 * Written from the reference's learn() (scripts/main.py:122-157: Double-DQN target, nn.MSELoss,
 * torch.optim.Adam, the target copy every Q_NETWORK_ITERATION learns; Net main.py:30-47) and from the
 * operation order include/merging_hip.h documents at mg_dqn_learn. It shares no code with csrc/: whole
 * matrices in nested loops, one layer after another, every intermediate in its own malloc'd array.
 * Compile with -ffp-contract=off so that only the fmaf calls fuse. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define H1 200
#define H2 100

/* Philox4x32-10 (Salmon et al., SC'11), word 0 of the output. */
static uint32_t philox_word0(uint64_t ctr_lo, uint64_t ctr_hi, uint64_t key) {
  uint32_t c[4] = {(uint32_t)ctr_lo, (uint32_t)(ctr_lo >> 32), (uint32_t)ctr_hi, (uint32_t)(ctr_hi >> 32)};
  uint32_t k[2] = {(uint32_t)key, (uint32_t)(key >> 32)};
  for (int round = 0; round < 10; ++round) {
    const uint64_t a = (uint64_t)0xD2511F53u * c[0];
    const uint64_t b = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n[4] = {(uint32_t)(b >> 32) ^ c[1] ^ k[0], (uint32_t)b, (uint32_t)(a >> 32) ^ c[3] ^ k[1],
                           (uint32_t)a};
    memcpy(c, n, sizeof c);
    k[0] += 0x9E3779B9u;
    k[1] += 0xBB67AE85u;
  }
  return c[0];
}

/* y[B, J] = x[B, K] W[J, K]^T + bias, each element one fmaf chain over k from the bias; relu optional */
static void linear(const float* x, int B, int K, const float* W, const float* bias, int J, int relu, float* y) {
  for (int b = 0; b < B; ++b)
    for (int j = 0; j < J; ++j) {
      float s = bias[j];
      for (int k = 0; k < K; ++k) s = fmaf(x[b * K + k], W[j * K + k], s);
      y[b * J + j] = (relu && !(s > 0.0f)) ? 0.0f : s;
    }
}

typedef struct {
  const float *W1, *b1, *W2, *b2, *W3, *b3;
} net_t;

static net_t net_at(const float* p, int in, int out) {
  net_t n;
  n.W1 = p;
  n.b1 = n.W1 + H1 * in;
  n.W2 = n.b1 + H1;
  n.b2 = n.W2 + H2 * H1;
  n.W3 = n.b2 + H2;
  n.b3 = n.W3 + out * H2;
  return n;
}

static void forward(net_t n, const float* x, int B, int in, int out, float* a1, float* a2, float* q) {
  linear(x, B, in, n.W1, n.b1, H1, 1, a1);
  linear(a1, B, H1, n.W2, n.b2, H2, 1, a2);
  linear(a2, B, H2, n.W3, n.b3, out, 0, q);
}

int dqn_learn_params(int in, int out) { return H1 * in + H1 + H2 * H1 + H2 + out * H2 + out; }

/* learner: [4, P] eval, target, m, v. ring: [capacity, 2 in + 2]. counter: the ring's memory_counter.
 * loss_out [U], rows_out [U, B, 2 in + 2], grads_out [U, P]: optional. Returns 0, or -1 without memory. */
int dqn_learn_ref(float* learner, const float* ring, uint64_t counter, int64_t capacity, int in, int out, int B,
                  int num_updates, uint64_t first_update, uint64_t seed, uint64_t first_draw, int filled_only,
                  double lr, double gamma, double beta1, double beta2, double eps, int target_period,
                  float* loss_out, float* rows_out, float* grads_out) {
  const int P = dqn_learn_params(in, out), RF = 2 * in + 2;
  float *ev = learner, *tg = learner + P, *am = learner + 2 * P, *av = learner + 3 * P;
  float* mem = malloc(sizeof(float) * ((size_t)B * (RF + 2 * in + 3 * (H1 + H2 + out) + out + H2 + H1) + P));
  if (!mem) return -1;
  float* batch = mem;
  float* s = batch + B * RF;
  float* s2 = s + B * in;
  float* e1 = s2 + B * in; /* eval(s): hidden 1, hidden 2, q */
  float* e2 = e1 + B * H1;
  float* eq = e2 + B * H2;
  float* n1 = eq + B * out; /* eval(s') */
  float* n2 = n1 + B * H1;
  float* nq = n2 + B * H2;
  float* t1 = nq + B * out; /* target(s') */
  float* t2 = t1 + B * H1;
  float* tq = t2 + B * H2;
  float* dq = tq + B * out;
  float* d2 = dq + B * out;
  float* d1 = d2 + B * H2;
  float* g = d1 + B * H1;
  const float gam = (float)gamma, inv_b = (float)(1.0 / B), two_inv_b = (float)(2.0 / B);

  for (int u = 0; u < num_updates; ++u) {
    const uint64_t t = first_update + (uint64_t)u;
    if (t % (uint64_t)target_period == 0) memcpy(tg, ev, sizeof(float) * P); /* main.py:125-126 */

    /* main.py:130-135: the minibatch, drawn as mg_replay_sample draws it */
    uint64_t live = (uint64_t)capacity;
    if (filled_only) {
      if (counter < live) live = counter;
      if (live == 0) live = 1;
    }
    for (int b = 0; b < B; ++b) {
      const uint64_t slot = ((uint64_t)philox_word0((uint64_t)b, first_draw + (uint64_t)u, seed) * live) >> 32;
      memcpy(batch + b * RF, ring + slot * RF, sizeof(float) * RF);
      memcpy(s + b * in, batch + b * RF, sizeof(float) * in);
      memcpy(s2 + b * in, batch + b * RF + in + 2, sizeof(float) * in);
    }
    if (rows_out) memcpy(rows_out + (size_t)u * B * RF, batch, sizeof(float) * B * RF);

    /* main.py:144-146 */
    forward(net_at(ev, in, out), s, B, in, out, e1, e2, eq);
    forward(net_at(ev, in, out), s2, B, in, out, n1, n2, nq);
    forward(net_at(tg, in, out), s2, B, in, out, t1, t2, tq);

    /* main.py:149-153 and the loss's gradient */
    float loss = 0.0f;
    for (int b = 0; b < B; ++b) {
      const float af = batch[b * RF + in], r = batch[b * RF + in + 1];
      int a = 0;
      if (af >= 0.0f) a = af >= (float)out ? out - 1 : (int)af;
      int best = 0;
      for (int j = 1; j < out; ++j)
        if (nq[b * out + j] > nq[b * out + best]) best = j;
      const float prod = gam * tq[b * out + best];
      const float target = r + prod;
      const float d = eq[b * out + a] - target;
      const float sq = d * d;
      loss = loss + sq;
      for (int j = 0; j < out; ++j) dq[b * out + j] = 0.0f;
      dq[b * out + a] = d * two_inv_b;
    }
    loss = loss * inv_b;
    if (loss_out) loss_out[u] = loss;

    /* backward: out layer, fc2, fc1 */
    net_t E = net_at(ev, in, out);
    float* gW1 = g;
    float* gb1 = gW1 + H1 * in;
    float* gW2 = gb1 + H1;
    float* gb2 = gW2 + H2 * H1;
    float* gW3 = gb2 + H2;
    float* gb3 = gW3 + out * H2;
    for (int j = 0; j < out; ++j) {
      for (int k = 0; k < H2; ++k) {
        float acc = 0.0f;
        for (int b = 0; b < B; ++b) acc = fmaf(dq[b * out + j], e2[b * H2 + k], acc);
        gW3[j * H2 + k] = acc;
      }
      float acc = 0.0f;
      for (int b = 0; b < B; ++b) acc = acc + dq[b * out + j];
      gb3[j] = acc;
    }
    for (int b = 0; b < B; ++b)
      for (int k = 0; k < H2; ++k) {
        float acc = 0.0f;
        for (int j = 0; j < out; ++j) acc = fmaf(dq[b * out + j], E.W3[j * H2 + k], acc);
        d2[b * H2 + k] = e2[b * H2 + k] > 0.0f ? acc : 0.0f;
      }
    for (int j = 0; j < H2; ++j) {
      for (int k = 0; k < H1; ++k) {
        float acc = 0.0f;
        for (int b = 0; b < B; ++b) acc = fmaf(d2[b * H2 + j], e1[b * H1 + k], acc);
        gW2[j * H1 + k] = acc;
      }
      float acc = 0.0f;
      for (int b = 0; b < B; ++b) acc = acc + d2[b * H2 + j];
      gb2[j] = acc;
    }
    for (int b = 0; b < B; ++b)
      for (int k = 0; k < H1; ++k) {
        float acc = 0.0f;
        for (int j = 0; j < H2; ++j) acc = fmaf(d2[b * H2 + j], E.W2[j * H1 + k], acc);
        d1[b * H1 + k] = e1[b * H1 + k] > 0.0f ? acc : 0.0f;
      }
    for (int j = 0; j < H1; ++j) {
      for (int k = 0; k < in; ++k) {
        float acc = 0.0f;
        for (int b = 0; b < B; ++b) acc = fmaf(d1[b * H1 + j], s[b * in + k], acc);
        gW1[j * in + k] = acc;
      }
      float acc = 0.0f;
      for (int b = 0; b < B; ++b) acc = acc + d1[b * H1 + j];
      gb1[j] = acc;
    }
    if (grads_out) memcpy(grads_out + (size_t)u * P, g, sizeof(float) * P);

    /* torch.optim.Adam, single-tensor form; the bias corrections in double as Python computes them */
    const double step = (double)(t + 1);
    const float fb1 = (float)beta1, fomb1 = (float)(1.0 - beta1), fb2 = (float)beta2, fomb2 = (float)(1.0 - beta2);
    const float step_size = (float)(lr / (1.0 - pow(beta1, step)));
    const float bc2_sqrt = (float)sqrt(1.0 - pow(beta2, step));
    const float feps = (float)eps;
    for (int i = 0; i < P; ++i) {
      const float scaled_m = fb1 * am[i];
      am[i] = fmaf(fomb1, g[i], scaled_m);
      const float scaled_v = fb2 * av[i];
      const float og = fomb2 * g[i];
      av[i] = fmaf(og, g[i], scaled_v);
      const float root = sqrtf(av[i]);
      const float denom = root / bc2_sqrt + feps;
      const float ratio = am[i] / denom;
      ev[i] = ev[i] - step_size * ratio;
    }
  }
  free(mem);
  return 0;
}
