// mg_rainbow.h -- Rainbow's acting net: packed layout, pack kernel, the bf16 MFMA forward, the fp32 head.
// A part of the one translation unit merging_hip.hip (see its head comment).
#pragma once

#include "mg_common.h"
#include "mg_qnet.h"

namespace {

// ============================================================================ Rainbow acting net
// The reference's RainbowDQN (scripts/ranbowdqn.py:498-548) as its act() evaluates it (:543-548):
// Linear(10, 32) -> ReLU -> Linear(32, 64) -> ReLU, a value stream NoisyLinear(64, 64) -> ReLU ->
// NoisyLinear(64, 51) and an advantage stream NoisyLinear(64, 64) -> ReLU -> NoisyLinear(64, 5 * 51), the
// dueling combination per atom, a softmax over the 51 atoms of each action, q[a] = sum_i p[a][i] z[i] and the
// first maximum of q. The noisy layers arrive as their effective weights mu + sigma * epsilon (:468-470):
// between two reset_noise() calls the net is a fixed function.
//
// Matrix layers: bf16 operands on v_mfma_f32_16x16x32_bf16 with fp32 accumulation, transposed like qnet_mlp
// (units on tile rows, envs on tile columns). A wave forwards its 64 envs as four column tiles of 16, ONE
// COLUMN TILE AT A TIME through all six layers (a rolled loop): a 16x16 accumulator holds rows 4 g .. 4 g + 3
// of column c in lane l = 16 g + c, which is exactly the B operand's layout of the next layer when two row
// tiles sit side by side (k = 8 g + j: row tile 2 kb + (j >> 2), row 4 g + (j & 3) -- qnet_unit2's order, which
// the pack kernel gives every later layer's columns), so no activation goes through LDS or a lane exchange,
// and the whole head of a column tile -- 51 value and 255 advantage logits per env -- stays in 96 accumulator
// registers instead of the 320 that four column tiles at once would need. The price is that a weight fragment
// read from LDS feeds one MFMA instead of four (280 KB of LDS reads per 64-env forward); the forward is bound
// by the head's vector arithmetic, not by those reads.
//  * layer 1 (K = 10 of 32): the bias folded as three bf16 parts (hi + mid + lo == b1 exactly) in the padded
//    slots k = 10, 11, 12, whose inputs are 1.0; the accumulator starts at zero.
//  * every later layer (K = 32 or 64, no spare slot): the accumulator starts from the fp32 bias.
//  * hidden activations: one bf16 rounding (v_cvt_pk_bf16_f32), then ReLU (relu_pair).
// Head rows are packed so that the lane that holds an accumulator row also owns that atom: each of the six
// head streams (value, advantage of action 0..4) is 4 row tiles of its own, and row 16 m + 4 g + i of a stream
// is atom 13 g + 4 m + i (slot s = 4 m + i < 13; slots 13..15 and atom 51 are zero padding). Lane group g of a
// column tile therefore holds atoms 13 g .. 13 g + 12 of its env for all six streams, and the head runs on
// registers alone.
constexpr int kRbIn = 10, kRbH1 = 32, kRbH2 = 64, kRbHS = 64;  // ranbowdqn.py:508-515
constexpr int kRbActions = 5, kRbAtoms = 51;
constexpr int kRbLogits = kRbAtoms * (1 + kRbActions);  // 306: value [51], advantage [5][51]
constexpr int kRbBias1 = kRbIn;                         // layer-1 k slots 10..12: b1's three parts
constexpr int kRbSlots = 13;                            // atoms per lane group: 4 x 13 = 52 >= 51
static_assert(kRbIn == kObs && kRbActions == MG_NUM_ACTIONS, "the net acts on the env's observation");
static_assert(4 * kRbSlots >= kRbAtoms && kRbSlots <= 16, "four lane groups of a 64-row stream cover the atoms");

// The packed net: the forward's A fragments in the order it consumes them (each the 64 lanes' 16 bytes
// contiguous: a conflict-free ds_read_b128), every stream's fp32 bias in accumulator row order before its
// fragments, the support last. Fragment (m, kb) of a stream is at 1024 (nkb m + kb).
constexpr int kRbFrag = 1024, kRbBiasBytes = 64 * 4;
constexpr int kRbOffW1 = 0;                                   // 2 row tiles, K = 32
constexpr int kRbOffB2 = kRbOffW1 + 2 * kRbFrag;              // b2 [64]
constexpr int kRbOffW2 = kRbOffB2 + kRbBiasBytes;             // 4 row tiles, one k-block
constexpr int kRbOffBV1 = kRbOffW2 + 4 * kRbFrag;             // value stream, hidden: bias, 4 x 2 fragments
constexpr int kRbOffWV1 = kRbOffBV1 + kRbBiasBytes;
constexpr int kRbOffBA1 = kRbOffWV1 + 8 * kRbFrag;            // advantage stream, hidden
constexpr int kRbOffWA1 = kRbOffBA1 + kRbBiasBytes;
constexpr int kRbOffHead = kRbOffWA1 + 8 * kRbFrag;           // six head streams: value, action 0..4
constexpr int kRbHeadStride = kRbBiasBytes + 8 * kRbFrag;     // bias [64 rows], 4 x 2 fragments
constexpr int kRbOffZ = kRbOffHead + 6 * kRbHeadStride;       // support z[52] fp32 (z[51] = 0)
constexpr int kRbNetBytes = kRbOffZ + 4 * kRbSlots * 4;       // 74,192 B
static_assert(kRbNetBytes == 74192 && kRbNetBytes % 16 == 0 && kRbOffZ % 16 == 0, "16-byte sections");

// The atom of row `row` (0..63) of a head stream, or -1 for padding.
__host__ __device__ constexpr int rb_row_atom(int row) {
  const int m = row >> 4, g = (row >> 2) & 3, i = row & 3, s = 4 * m + i;
  return s < kRbSlots && kRbSlots * g + s < kRbAtoms ? kRbSlots * g + s : -1;
}

// The effective fp32 tensors of the six layers (torch Linear layout, row-major [out][in]) and the support.
struct RbTensors {
  const float *w1, *b1, *w2, *b2, *wv1, *bv1, *wv2, *bv2, *wa1, *ba1, *wa2, *ba2, *z;
};

// One thread per packed 4-byte word: two bf16 weights of a fragment, or one fp32 bias / support value.
__device__ inline void rainbow_pack_at(int w, const RbTensors& T, uint8_t* packed) {
  if (w >= kRbNetBytes / 4) return;
  const int off = 4 * w;
  // part p (0 hi, 1 mid, 2 lo) of the three-way bf16 split of b (hi + mid + lo == b)
  auto part = [](float b, int p) {
    const float hi = static_cast<float>(static_cast<__bf16>(b));
    const float r = b - hi;
    const float mid = static_cast<float>(static_cast<__bf16>(r));
    return p == 0 ? hi : p == 1 ? mid : r - mid;
  };
  // element (row, k) of a K-column fragment section that starts at `base`: fragment (m, kb), lane 16 g + c
  // holds row 16 m + c, k = 32 kb + 8 g + j
  auto frag_rk = [&](int base, int nkb, int& row, int& k) {
    const int rel = off - base, f = rel / kRbFrag, lane = (rel % kRbFrag) / 16, j = (rel % 16) / 2;
    row = 16 * (f / nkb) + (lane & 15);
    k = 32 * (f % nkb) + 8 * (lane >> 4) + j;
  };
  // hidden unit at k of a later layer: qnet_unit2's order within each k-block of 32
  auto unit = [](int k) { return qnet_unit2(k >> 5, (k >> 3) & 3, k & 7); };
  float v[2] = {0.f, 0.f};
  bool bf = true;
  int row, k;
  if (off < kRbOffB2) {  // W1: natural k order, b1's parts at 10..12
    frag_rk(kRbOffW1, 1, row, k);
    for (int e = 0; e < 2; ++e) {
      const int kk = k + e;
      v[e] = kk < kRbIn ? T.w1[row * kRbIn + kk] : kk < kRbBias1 + 3 ? part(T.b1[row], kk - kRbBias1) : 0.f;
    }
  } else if (off < kRbOffW2) {
    bf = false;
    v[0] = T.b2[(off - kRbOffB2) / 4];
  } else if (off < kRbOffBV1) {
    frag_rk(kRbOffW2, 1, row, k);
    for (int e = 0; e < 2; ++e) v[e] = T.w2[row * kRbH1 + unit(k + e)];
  } else if (off < kRbOffWV1) {
    bf = false;
    v[0] = T.bv1[(off - kRbOffBV1) / 4];
  } else if (off < kRbOffBA1) {
    frag_rk(kRbOffWV1, 2, row, k);
    for (int e = 0; e < 2; ++e) v[e] = T.wv1[row * kRbH2 + unit(k + e)];
  } else if (off < kRbOffWA1) {
    bf = false;
    v[0] = T.ba1[(off - kRbOffBA1) / 4];
  } else if (off < kRbOffHead) {
    frag_rk(kRbOffWA1, 2, row, k);
    for (int e = 0; e < 2; ++e) v[e] = T.wa1[row * kRbH2 + unit(k + e)];
  } else if (off < kRbOffZ) {  // head stream st: 0 the value, 1 + a the advantage of action a
    const int st = (off - kRbOffHead) / kRbHeadStride, base = kRbOffHead + st * kRbHeadStride;
    const float* W = st == 0 ? T.wv2 : T.wa2 + (st - 1) * kRbAtoms * kRbHS;
    const float* B = st == 0 ? T.bv2 : T.ba2 + (st - 1) * kRbAtoms;
    if (off < base + kRbBiasBytes) {
      bf = false;
      const int atom = rb_row_atom((off - base) / 4);
      v[0] = atom >= 0 ? B[atom] : 0.f;
    } else {
      frag_rk(base + kRbBiasBytes, 2, row, k);
      const int atom = rb_row_atom(row);
      for (int e = 0; e < 2; ++e) v[e] = atom >= 0 ? W[atom * kRbHS + unit(k + e)] : 0.f;
    }
  } else {
    bf = false;
    const int i = (off - kRbOffZ) / 4;
    v[0] = i < kRbAtoms ? T.z[i] : 0.f;
  }
  if (bf) {
    reinterpret_cast<__bf16*>(packed + off)[0] = static_cast<__bf16>(v[0]);
    reinterpret_cast<__bf16*>(packed + off)[1] = static_cast<__bf16>(v[1]);
  } else {
    *reinterpret_cast<float*>(packed + off) = v[0];
  }
}

__global__ void rainbow_pack_kernel(const RbTensors T, uint8_t* packed) {
  rainbow_pack_at(blockIdx.x * blockDim.x + threadIdx.x, T, packed);
}

// ---------------------------------------------------------------------------- the head, host and device
// exp(x) for x <= 0, the same bits on host and device: k = rint(x log2 e), r = x - k ln 2 in two fmaf steps
// (Cody-Waite: the high part has 9 significant bits, so k hi is exact), the degree-7 Taylor polynomial of
// exp(r) in Horner form with fmaf, scaled by 2^k through the exponent field. Below kRbExpCut (and for NaN) it
// returns +0: every result above is a normal number (exp(-87) = 1.6e-38 > FLT_MIN), so the scaling is exact
// and no subnormal is ever produced. Not the hardware v_exp_f32, which the host cannot reproduce.
constexpr float kRbExpCut = -87.0f;
MG_HD float rb_exp(float x) {
  if (!(x >= kRbExpCut)) return 0.0f;
  const float k = rintf(x * 1.44269504088896341f);
  float r = fmaf(k, -0.693359375f, x);
  r = fmaf(k, 2.12194440e-4f, r);
  float p = 1.0f / 5040.0f;
  p = fmaf(p, r, 1.0f / 720.0f);
  p = fmaf(p, r, 1.0f / 120.0f);
  p = fmaf(p, r, 1.0f / 24.0f);
  p = fmaf(p, r, 1.0f / 6.0f);
  p = fmaf(p, r, 0.5f);
  p = fmaf(p, r, 1.0f);
  p = fmaf(p, r, 1.0f);
  const uint32_t sb = static_cast<uint32_t>(static_cast<int>(k) + 127) << 23;
  return p * __builtin_bit_cast(float, sb);
}

// mean over the five actions of one atom's advantages: the left-to-right sum, one division
MG_HD float rb_mean(float a0, float a1, float a2, float a3, float a4) {
  return ((((a0 + a1) + a2) + a3) + a4) / 5.0f;
}
// the dueling combination of one (action, atom): (v + A) - mean
MG_HD float rb_duel(float v, float a, float mean) { return (v + a) - mean; }
// one atom's terms of the two sums: S += e, N += e z (the product rounded, then the sum)
MG_HD void rb_accumulate(float x, float m, float z, float& S, float& N) {
  const float e = rb_exp(x - m);
  S = S + e;
  N = N + e * z;
}
MG_HD int rb_argmax(const float (&q)[kRbActions]) {
  int best = 0;
  for (int a = 1; a < kRbActions; ++a)
    if (q[a] > q[best]) best = a;
  return best;
}

// The head of one env on host memory, in the device's order: logits [306] = value [51], advantage [5][51].
// The atoms are summed as four chains over 13 g .. 13 g + 12 (the lane groups), each from +0 in ascending
// order, combined as (c0 + c1) + (c2 + c3).
inline void host_rainbow_head_row(const float* lg, const float* z, float* q, int8_t* action) {
  float mean[kRbAtoms], qa[kRbActions];
  const float* A = lg + kRbAtoms;
  for (int i = 0; i < kRbAtoms; ++i)
    mean[i] = rb_mean(A[i], A[kRbAtoms + i], A[2 * kRbAtoms + i], A[3 * kRbAtoms + i], A[4 * kRbAtoms + i]);
  for (int a = 0; a < kRbActions; ++a) {
    float x[kRbAtoms], m = -INFINITY;
    for (int i = 0; i < kRbAtoms; ++i) {
      x[i] = rb_duel(lg[i], A[a * kRbAtoms + i], mean[i]);
      m = fmaxf(m, x[i]);
    }
    float S[4], N[4];
    for (int g = 0; g < 4; ++g) {
      S[g] = N[g] = 0.0f;
      for (int i = kRbSlots * g; i < kRbSlots * (g + 1) && i < kRbAtoms; ++i) rb_accumulate(x[i], m, z[i], S[g], N[g]);
    }
    qa[a] = ((N[0] + N[1]) + (N[2] + N[3])) / ((S[0] + S[1]) + (S[2] + S[3]));
    if (q) q[a] = qa[a];
  }
  if (action) *action = static_cast<int8_t>(rb_argmax(qa));
}

// ---------------------------------------------------------------------------- the forward
__device__ __forceinline__ bf16x8 rb_frag(const uint8_t* net, int off) {
  return *reinterpret_cast<const bf16x8*>(net + off + 16 * (threadIdx.x & 63));
}
// rows 4 g .. 4 g + 3 of row tile m of a stream's bias: the accumulator's initial value
__device__ __forceinline__ f32x4 rb_bias(const uint8_t* net, int off, int m) {
  return *reinterpret_cast<const f32x4*>(net + off + 4 * (16 * m + 4 * ((threadIdx.x & 63) >> 4)));
}
// B operand of k-block kb from the accumulators of row tiles 2 kb and 2 kb + 1: bf16 rounding, then ReLU
__device__ __forceinline__ bf16x8 rb_hidden(const f32x4& lo, const f32x4& hi) {
  return __builtin_bit_cast(bf16x8, u32x4{relu_pair(lo[0], lo[1]), relu_pair(lo[2], lo[3]), relu_pair(hi[0], hi[1]),
                                          relu_pair(hi[2], hi[3])});
}
// A 64-row stream over K = 64: acc[m] = bias + W(m, 0) b[0] + W(m, 1) b[1]
__device__ __forceinline__ void rb_stream(const uint8_t* net, int boff, int woff, const bf16x8 (&b)[2],
                                          f32x4 (&acc)[4]) {
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    acc[m] = rb_bias(net, boff, m);
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) acc[m] = mfma16(rb_frag(net, woff + kRbFrag * (2 * m + kb)), b[kb], acc[m]);
  }
}

// The forward of this wave's 64 envs from their fp32 observation rows wtile [64][10] in LDS. The packed net is
// named by two bases, each that of a whole packed net: `trunk` serves bytes [0, kRbOffBV1) (W1, b2, W2) and
// `streams` bytes [kRbOffBV1, kRbNetBytes) (the hidden streams, the head, the support). With the whole net in LDS
// both are that copy; a rollout against another net (rainbow_rollout_kernel<3>) keeps only the opponent's stream
// part in LDS and reads its 6,400-byte trunk from the packed net in global memory. rot: the view, input j =
// obs[(j + rot) % 10] (0 the ego's; 3 the opponent's state[3:] + state[:3] of ranbowdqn.py:669). On return lane l
// holds q[0..4] and the chosen action of env l. logits (global, [nrows][306] of this wave's envs, or NULL): the
// raw head outputs. Every lane of the wave must call it.
__device__ __forceinline__ void rainbow_forward_wave(const uint8_t* trunk_base, const uint8_t* streams_base,
                                                     const float* wtile, int rot, float (&q)[kRbActions], int& action,
                                                     float* logits, int nrows) {
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  action = 0;
#pragma unroll 1
  for (int t = 0; t < 4; ++t) {
    const int oz = opaque_zero();  // the fragment loads stay inside the loop
    const uint8_t* trunk = trunk_base + oz;
    const uint8_t* net = streams_base + oz;
    // layer-1 B operand: k = 8 g + j of env 16 t + c
    const float* row = wtile + (16 * t + c) * kObs;
    float xin[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = 8 * g + j;
      int src = k + rot;
      src = src >= kObs ? src - kObs : src;
      const float x = row[k < kRbIn ? src : 0];
      xin[j] = k < kRbIn ? x : (k < kRbBias1 + 3 ? 1.0f : 0.0f);
    }
    u32x4 xw;
#pragma unroll
    for (int d = 0; d < 4; ++d)
      xw[d] = __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{xin[2 * d], xin[2 * d + 1]}, bf16x2));
    const bf16x8 xb = __builtin_bit_cast(bf16x8, xw);
    const f32x4 z4 = {};
    // layer 1: 32 units, bias inside the K sum
    const f32x4 a10 = mfma16(rb_frag(trunk, kRbOffW1), xb, z4);
    const f32x4 a11 = mfma16(rb_frag(trunk, kRbOffW1 + kRbFrag), xb, z4);
    const bf16x8 h1 = rb_hidden(a10, a11);
    // layer 2: 64 units over one k-block
    f32x4 a2[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) a2[m] = mfma16(rb_frag(trunk, kRbOffW2 + kRbFrag * m), h1, rb_bias(trunk, kRbOffB2, m));
    const bf16x8 h2[2] = {rb_hidden(a2[0], a2[1]), rb_hidden(a2[2], a2[3])};
    // the two hidden streams
    f32x4 av[4], aa[4];
    rb_stream(net, kRbOffBV1, kRbOffWV1, h2, av);
    rb_stream(net, kRbOffBA1, kRbOffWA1, h2, aa);
    const bf16x8 hv[2] = {rb_hidden(av[0], av[1]), rb_hidden(av[2], av[3])};
    const bf16x8 ha[2] = {rb_hidden(aa[0], aa[1]), rb_hidden(aa[2], aa[3])};
    // the head: this lane's 13 atoms of the value and of the five advantages
    f32x4 V[4], A[kRbActions][4];
    rb_stream(net, kRbOffHead, kRbOffHead + kRbBiasBytes, hv, V);
#pragma unroll
    for (int a = 0; a < kRbActions; ++a)
      rb_stream(net, kRbOffHead + (1 + a) * kRbHeadStride, kRbOffHead + (1 + a) * kRbHeadStride + kRbBiasBytes, ha,
                A[a]);
    const int env = 16 * t + c;
    if (logits != nullptr && env < nrows) {
      float* lr = logits + static_cast<int64_t>(env) * kRbLogits + kRbSlots * g;
#pragma unroll
      for (int s = 0; s < kRbSlots; ++s) {
        if (kRbSlots * g + s >= kRbAtoms) continue;
        lr[s] = V[s >> 2][s & 3];
#pragma unroll
        for (int a = 0; a < kRbActions; ++a) lr[kRbAtoms * (1 + a) + s] = A[a][s >> 2][s & 3];
      }
    }
    float mean[kRbSlots], zz[kRbSlots];
#pragma unroll
    for (int s = 0; s < kRbSlots; ++s) {
      mean[s] = rb_mean(A[0][s >> 2][s & 3], A[1][s >> 2][s & 3], A[2][s >> 2][s & 3], A[3][s >> 2][s & 3],
                        A[4][s >> 2][s & 3]);
      zz[s] = reinterpret_cast<const float*>(net + kRbOffZ)[kRbSlots * g + s];
    }
    float qt[kRbActions];
#pragma unroll
    for (int a = 0; a < kRbActions; ++a) {
      float x[kRbSlots], m = -INFINITY;
#pragma unroll
      for (int s = 0; s < kRbSlots; ++s) {
        x[s] = rb_duel(V[s >> 2][s & 3], A[a][s >> 2][s & 3], mean[s]);
        if (kRbSlots * 3 + s >= kRbAtoms && g == 3) x[s] = -INFINITY;  // atom 51: padding
        m = fmaxf(m, x[s]);
      }
      m = fmaxf(m, __shfl_xor(m, 16));
      m = fmaxf(m, __shfl_xor(m, 32));
      float S = 0.0f, N = 0.0f;
#pragma unroll
      for (int s = 0; s < kRbSlots; ++s) rb_accumulate(x[s], m, zz[s], S, N);  // padding: e = +0, z = 0
      S = S + __shfl_xor(S, 16);
      N = N + __shfl_xor(N, 16);
      S = S + __shfl_xor(S, 32);
      N = N + __shfl_xor(N, 32);
      qt[a] = N / S;
    }
    // the four lane groups hold the same q of env 16 t + c: lane l keeps those of its own env l
    if (t == g) {
#pragma unroll
      for (int a = 0; a < kRbActions; ++a) q[a] = qt[a];
      action = rb_argmax(qt);
    }
  }
}

// Cooperative copy of a packed net, or of its first `bytes` (a multiple of 16) from `net` on, into LDS (all threads
// of the block; caller syncs).
__device__ __forceinline__ void rainbow_to_lds(const uint8_t* net, uint8_t* lds, int bytes = kRbNetBytes) {
  const f32x4* src = reinterpret_cast<const f32x4*>(net);
  f32x4* dst = reinterpret_cast<f32x4*>(lds);
  for (int j = threadIdx.x; j < bytes / 16; j += blockDim.x) dst[j] = src[j];
}

// Stand-alone forward (RainbowNet.forward / .act, and the test seam): obs [n][10] -> optional logits [n][306],
// q [n][5], action [n].
__global__ __launch_bounds__(kBlock) void rainbow_forward_kernel(const uint8_t* net, const float* obs, int rot,
                                                                 float* logits, float* qout, int8_t* action,
                                                                 int64_t n) {
  __shared__ __attribute__((aligned(16))) uint8_t lds_net[kRbNetBytes];
  __shared__ __attribute__((aligned(16))) float tile[kBlock * kObs];
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kBlock;
  rainbow_to_lds(net, lds_net);
  for (int j = threadIdx.x; j < kBlock * kObs; j += kBlock) {
    const int64_t i = base + j / kObs;
    tile[j] = i < n ? obs[base * kObs + j] : 0.f;
  }
  __syncthreads();
  const int64_t wbase = base + (threadIdx.x & ~63);
  const int64_t wrem = n - wbase;
  const int wrows = wrem <= 0 ? 0 : (wrem < 64 ? static_cast<int>(wrem) : 64);
  float q[kRbActions];
  int act;
  rainbow_forward_wave(lds_net, lds_net, tile + (threadIdx.x & ~63) * kObs, rot, q, act,
                       logits ? logits + wbase * kRbLogits : nullptr, wrows);
  const int64_t i = base + threadIdx.x;
  if (i < n) {
    if (qout) {
#pragma unroll
      for (int a = 0; a < kRbActions; ++a) qout[i * kRbActions + a] = q[a];
    }
    if (action) action[i] = static_cast<int8_t>(act);
  }
}

}  // namespace
