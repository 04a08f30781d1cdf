// mg_qnet.h -- the bf16 MFMA Q-net: weight layouts, pack kernels, both forwards, the stand-alone forward.
// A part of the one translation unit merging_hip.hip (see its head comment).
#pragma once

#include "mg_common.h"

namespace {

// ============================================================================ Q-net policy
// The reference's DQN Net (scripts/main.py:30-47, scripts/hdqn.py:38-55): Linear(in,200) ->
// ReLU -> Linear(200,100) -> ReLU -> Linear(100,out), and its epsilon-greedy choose_action
// (main.py:99-112: greedy argmax when np.random.randn() <= EPISILO, else uniform). Computed
// in bf16 on the matrix cores with fp32 accumulation, one wave per 64 envs, in the TRANSPOSED
// form  H1' = W1 X',  H2' = W2 H1',  Q' = W3 H2'  (hidden units on tile rows, envs on lanes):
//  * layer 1 (K = 16: up to 13 inputs and the 3 bias slots) on v_mfma_f32_32x32x16_bf16, 7 row
//    tiles of 32 units x 2 column tiles of 32 envs;
//  * layers 2 and 3 on v_mfma_f32_16x16x32_bf16: H2' in 7 row tiles of 16 units x 4 column tiles
//    of 16 envs over 7 k-blocks of 32 hidden-1 units, Q' in one row tile over 4 k-blocks of 32
//    hidden-2 units. Under load the chip holds a higher clock for the 16x16 shape at equal cycles
//    per FLOP (tools/micro/qfwd_probe.hip: 2.33-2.47 PF against 2.07 PF for 32x32x16, r03ab), and
//    16-row tiles pad hidden-2 to 112 units instead of 128: 14 x 32 + (196 + 16) x 16 = 3,840
//    matrix cycles per 64-env forward (round 3's all-32x32 forward: 132 x 32 = 4,224).
// No layer's output goes through LDS:
//  * a 32x32 layer-1 accumulator holds its 32 envs (lane & 31) in both lane halves. After ReLU +
//    bf16 packing, one v_permlane16_swap per pair of packed registers leaves envs 0..15 in every
//    16-lane row of the first register and envs 16..31 in the second: each is then the B operand
//    of a 16x16x32 MFMA (lane l: env column l & 15, k = 8 (l >> 4) + j), in the k order
//    qnet_unit1, which mg_qnet_pack gives W2's columns;
//  * a 16x16 accumulator holds rows 4 (l >> 4) .. + 3 of column l & 15, so two row tiles side by
//    side are the B operand of a layer-3 k-block (k order qnet_unit2, W3's columns);
//  * the Q tiles of the four column tiles reach one env per lane through two v_permlane32_swap and
//    one v_permlane16_swap per register (qnet_gather_q).
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short i16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr int kQH1Real = 200, kQH2Real = 100;  // main.py:30-47 Net widths
constexpr int kQT1 = 7;  // layer-1 row tiles of 32 units = layer-2 k-blocks (224 >= 203)
constexpr int kQT2 = 7;  // layer-2 row tiles of 16 units (112 >= 103)
constexpr int kQK3 = 4;  // layer-3 k-blocks of 32 hidden-2 units (two row tiles each)
// Biases are folded into the padded K slots: each bias b is split into three bf16 parts
// hi + mid + lo == b exactly (8 significant bits each, 24 = fp32's), stored as three weight
// columns whose inputs are 1.0 -- layer-1 inputs 13..15, hidden-1 units 200..202 and hidden-2
// units 100..102 (W1 / W2 rows that output exactly 1.0). The matrix cores add the fp32 bias
// inside the K sum, so there are no bias loads and every accumulator starts at an inline zero
// (a bias-initialised accumulator cost 4 ds_read_b128 per tile and the zeroing or bias moves;
// folding measured -5..8 % on the config-5 kernel). Summation order is the only difference.
constexpr int kQBiasIn = 13;       // first of the three layer-1 input slots holding 1.0
constexpr int kQOne1 = 200;        // hidden-1 units 200..202 = 1.0
constexpr int kQOne2 = 100;        // hidden-2 units 100..102 = 1.0
constexpr int kQMaxIn = kQBiasIn;  // widest net input: 13
constexpr int kLMaxOut = 8;        // widest net output (argmax_first's q[8], the learner's dq rows)
static_assert(32 * kQT1 >= kQOne1 + 3 && 32 * (kQT1 - 1) < kQH1Real && 16 * kQT2 >= kQOne2 + 3 &&
                  16 * (kQT2 - 1) < kQH2Real && 32 * kQK3 >= 16 * kQT2,
              "tile counts cover the hidden units and their 1.0 units, no tile is all padding");

// The packed net (mg_qnet_pack) is the forward's MFMA A operands in the order it consumes them,
// each fragment the 64 lanes' 16 bytes contiguous, so a wave's ds_read_b128 (LDS nets) or
// buffer_load_dwordx4 (nets read from L2) covers 1 KB of consecutive bytes: conflict-free in LDS,
// 8 cache lines from L2. Consumption order:
//   s = 0: W1(0); for k-block kb = 0..5: W1(kb + 1), then W2(t, kb) for row tiles t = 0..6;
//   kb = 6 interleaved with layer 3:  W2(0,6) W2(1,6) W2(2,6) W3(0) W2(3,6) W2(4,6) W3(1)
//                                     W2(5,6) W2(6,6) W3(2) W3(3)
// W1(m): lane l = 32 h + r holds W1[32 m + r][8 h .. 8 h + 7] (inputs in natural order, b1's parts
// at 13..15). W2(t, kb): lane l holds row 16 t + (l & 15), hidden-1 units qnet_unit1(kb, l >> 4,
// j = 0..7). W3(kb): 512 B -- output rows 0..7 only; lane l reads row l & 7, so rows 8..15 of the
// Q tile repeat rows 0..7 and are never read.
struct QFrag {
  int kind, tile, kb;  // kind 0: W1(tile), 1: W2(tile, kb), 2: W3(kb)
};
constexpr int kQFrags = 1 + 6 * 8 + 11;
// Closed forms (no loops or tables), so that every fragment offset of the unrolled forward folds
// to a constant. Last k-block: entry u = s - 49 is W3 at u = 3, 6, 9, 10, else W2 row tile u - u / 3.
__host__ __device__ constexpr QFrag qfrag(int s) {
  if (s == 0) return QFrag{0, 0, 0};
  if (s < 49) {
    const int u = s - 1, kb = u / 8, v = u % 8;
    return v == 0 ? QFrag{0, kb + 1, 0} : QFrag{1, v - 1, kb};
  }
  const int u = s - 49;
  if (u == 10) return QFrag{2, 0, 3};
  return u % 3 == 0 && u > 0 ? QFrag{2, 0, u / 3 - 1} : QFrag{1, u - u / 3, kQT1 - 1};
}
__host__ __device__ constexpr int qfrag_off(int s) {
  if (s <= 49) return 1024 * s;
  const int u = s - 49;
  return 1024 * s - 512 * ((u > 3) + (u > 6) + (u > 9) + (u > 10));
}
constexpr int kQNetBytes = qfrag_off(kQFrags);  // 59,392 B
static_assert(kQNetBytes == 56 * 1024 + 4 * 512, "7 W1 + 49 W2 fragments of 1 KB, 4 W3 of 512 B");

// hidden-1 unit at k = 8 g + j of layer-2 k-block kb: 32x32 accumulator register i = 2 q + e of
// lane half h holds row (i & 3) + 8 (i >> 2) + 4 h; after the swap, lane row g holds packed
// register q + 4 (g & 1) of half g >> 1 as its dword q
__host__ __device__ constexpr int qnet_unit1(int kb, int g, int j) {
  return 32 * kb + (j & 3) + 8 * (j >> 2) + 16 * (g & 1) + 4 * (g >> 1);
}
// hidden-2 unit at k = 8 g + j of layer-3 k-block kb: rows 4 g .. 4 g + 3 of row tiles 2 kb
// (j < 4) and 2 kb + 1 (j >= 4)
__host__ __device__ constexpr int qnet_unit2(int kb, int g, int j) {
  return 32 * kb + 16 * (j >> 2) + 4 * g + (j & 3);
}

// ReLU + bf16 pack of two accumulator values: one v_cvt_pk_bf16_f32 + one v_pk_max_i16
// (a 2-wide fptrunc selects ONE convert; scalar casts cost 2 converts + a perm). Rounded first,
// then max(x, 0) on the packed bf16 pairs as signed 16-bit integers: a bf16 with its sign bit set
// is a negative int16 (and -0.0 becomes +0.0), so max_i16(x, 0) is exactly ReLU.
__device__ __forceinline__ uint32_t relu_pair(float x, float y) {
  i16x2 v = __builtin_bit_cast(i16x2, __builtin_convertvector(f32x2{x, y}, bf16x2));
  const i16x2 zero = {0, 0};
  v = __builtin_elementwise_max(v, zero);
  return __builtin_bit_cast(uint32_t, v);
}

// Layer-1 B fragment of one env: features k = 8h .. 8h+7 of its observation row, in the
// swapped order state[5:] + state[:5] when swap (main.py:199); features 8..15 are x8, x9, 0, 0,
// 0, 1, 1, 1 (the 1.0 inputs of b1's three parts). The row is read with five unconditional
// ds_read_b64 and converted pairwise; the lane half picks its pairs with selects (per-element
// conditional loads cost a full LDS wait each).
__device__ __forceinline__ bf16x8 qnet_input(const float* row, bool swap, int h) {
  float v[kObs];
#pragma unroll
  for (int k = 0; k < kObs / 2; ++k) {
    const f32x2 t = reinterpret_cast<const f32x2*>(row)[k];
    v[2 * k] = t[0];
    v[2 * k + 1] = t[1];
  }
  uint32_t pr[kObs / 2];
#pragma unroll
  for (int k = 0; k < kObs / 2; ++k) {
    const int a = swap ? (2 * k + 5) % kObs : 2 * k, b = swap ? (2 * k + 6) % kObs : 2 * k + 1;
    pr[k] = __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{v[a], v[b]}, bf16x2));
  }
  static_assert(kQBiasIn == 13 && kObs == 10, "bias slots 13..15 follow the 10 features");
  const u32x4 w = h ? u32x4{pr[4], 0u, 0x3F800000u, 0x3F803F80u} : u32x4{pr[0], pr[1], pr[2], pr[3]};
  return __builtin_bit_cast(bf16x8, w);
}

// Layer-1 B fragment from a 16-float row (in_dim <= 13, zero padded, 1.0 at 13..15): features
// 8h .. 8h+7. The standalone forward takes any input width this way, e.g. hdqn.py's goal states
// [goal] + state (11 values, :291) for its lower-level Net(NUM_STATES + 1, NUM_ACTIONS) (:145).
__device__ __forceinline__ bf16x8 qnet_input_wide(const float* row16, int h) {
  const f32x4 lo = reinterpret_cast<const f32x4*>(row16 + 8 * h)[0];
  const f32x4 hi = reinterpret_cast<const f32x4*>(row16 + 8 * h)[1];
  const u32x4 w = {__builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{lo[0], lo[1]}, bf16x2)),
                   __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{lo[2], lo[3]}, bf16x2)),
                   __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{hi[0], hi[1]}, bf16x2)),
                   __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{hi[2], hi[3]}, bf16x2))};
  return __builtin_bit_cast(bf16x8, w);
}

__device__ __forceinline__ f32x16 mfma32(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// Packs fp32 torch Linear weights (row-major [out][in]) and biases into the fragment layout above:
// element e of (fragment, lane, element).
__device__ __forceinline__ void qnet_pack_at(int e, const float* w1, const float* b1, const float* w2, const float* b2,
                                             const float* w3, const float* b3, int in_dim, int out_dim,
                                             uint8_t* packed) {
  if (e >= kQFrags * 64 * 8) return;
  const int s = e >> 9, lane = (e >> 3) & 63, j = e & 7;
  const QFrag f = qfrag(s);
  // part p (0 hi, 1 mid, 2 lo) of the three-way bf16 split of b (hi + mid + lo == b)
  auto part = [](float b, int p) {
    const float hi = static_cast<float>(static_cast<__bf16>(b));
    const float r = b - hi;
    const float mid = static_cast<float>(static_cast<__bf16>(r));
    return p == 0 ? hi : p == 1 ? mid : r - mid;
  };
  float v = 0.f;
  int off = qfrag_off(s) + 16 * lane;
  if (f.kind == 0) {  // W1[m][k]: the input features, then b1's parts; hidden-1 units 200..202 = 1.0
    const int m = 32 * f.tile + (lane & 31), k = 8 * (lane >> 5) + j;
    if (m < kQH1Real && k < in_dim) v = w1[m * in_dim + k];
    else if (m < kQH1Real && k >= kQBiasIn && k < kQBiasIn + 3) v = part(b1[m], k - kQBiasIn);
    else if (m >= kQOne1 && m < kQOne1 + 3 && k == kQBiasIn) v = 1.f;
  } else if (f.kind == 1) {  // W2[m][u], u = qnet_unit1: then b2's parts; hidden-2 units 100..102 = 1.0
    const int m = 16 * f.tile + (lane & 15), u = qnet_unit1(f.kb, lane >> 4, j);
    if (m < kQH2Real && u < kQH1Real) v = w2[m * kQH1Real + u];
    else if (m < kQH2Real && u >= kQOne1 && u < kQOne1 + 3) v = part(b2[m], u - kQOne1);
    else if (m >= kQOne2 && m < kQOne2 + 3 && u == kQOne1) v = 1.f;
  } else {  // W3[m][u], u = qnet_unit2, then b3's parts; rows 0..7 of 16
    if ((lane & 15) >= 8) return;
    const int m = lane & 7, u = qnet_unit2(f.kb, lane >> 4, j);
    if (m < out_dim && u < kQH2Real) v = w3[m * kQH2Real + u];
    else if (m < out_dim && u >= kQOne2 && u < kQOne2 + 3) v = part(b3[m], u - kQOne2);
    off = qfrag_off(s) + 16 * (8 * (lane >> 4) + m);
  }
  reinterpret_cast<__bf16*>(packed + off)[j] = static_cast<__bf16>(v);
}

// One thread per (fragment, lane, element).
__global__ void qnet_pack_kernel(const float* w1, const float* b1, const float* w2, const float* b2,
                                 const float* w3, const float* b3, int in_dim, int out_dim,
                                 uint8_t* packed) {
  qnet_pack_at(blockIdx.x * blockDim.x + threadIdx.x, w1, b1, w2, b2, w3, b3, in_dim, out_dim, packed);
}

// A zero the compiler cannot see through. Added to the LDS addresses of loop-invariant
// weight loads so they are issued where they are used: hoisted out of the tile and time loops,
// they stay live across them and push the kernel into scratch.
__device__ __forceinline__ int opaque_zero() {
  int z = 0;
  asm volatile("" : "+v"(z));
  return z;
}

// Cooperative copy of a packed net into LDS (all threads of the block; caller syncs).
__device__ __forceinline__ void qnet_to_lds(const uint8_t* net, uint8_t* lds) {
  const f32x4* src = reinterpret_cast<const f32x4*>(net);
  f32x4* dst = reinterpret_cast<f32x4*>(lds);
  for (int j = threadIdx.x; j < kQNetBytes / 16; j += blockDim.x) dst[j] = src[j];
}

// Fragment s of a packed net for this lane: a net in LDS ...
struct QSrcLds {
  const uint8_t* net;  // + opaque zero: the loads stay where they are used
  int lo, lo3;         // lane byte offsets within a W1 / W2 fragment and within a W3 fragment
  __device__ __forceinline__ bf16x8 operator()(int s) const {
    return *reinterpret_cast<const bf16x8*>(net + qfrag_off(s) + (qfrag(s).kind == 2 ? lo3 : lo));
  }
};
// ... or in global memory (the h-DQN kernel's opponent from another checkpoint: four nets exceed
// one CU's LDS, so the opponent's two are read from L2), through a buffer resource: the lane offset
// in a VGPR, the fragment's offset a constant
struct QSrcGlobal {
  __amdgpu_buffer_rsrc_t rs;
  int lo, lo3;
  __device__ __forceinline__ bf16x8 operator()(int s) const {
    return __builtin_bit_cast(
        bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, qfrag(s).kind == 2 ? lo3 : lo, qfrag_off(s), 0));
  }
};
__device__ __forceinline__ int qnet_lane_off() { return 16 * (threadIdx.x & 63); }
__device__ __forceinline__ int qnet_lane_off3() {
  const int lane = threadIdx.x & 63;
  return 16 * (8 * (lane >> 4) + (lane & 7));
}
__device__ __forceinline__ QSrcLds qnet_lds(const uint8_t* net) {
  return QSrcLds{net + opaque_zero(), qnet_lane_off(), qnet_lane_off3()};
}
__device__ __forceinline__ QSrcGlobal qnet_global(const uint8_t* net) {
  // gfx9 buffer descriptor word 3 (raw untyped dword access), num_records = the packed net
  return QSrcGlobal{__builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(net), static_cast<short>(0), kQNetBytes,
                                                      0x00020000),
                    qnet_lane_off(), qnet_lane_off3()};
}
constexpr int kQLdsAhead = 2;     // fragments in flight, LDS nets
constexpr int kQGlobalAhead = 3;  // fragments in flight, nets read from L2 (five measured the same, r03e)

// (x, y) -> (x with y's lane rows swapped in as documented for the instruction, y likewise).
// Operands into locals and the result read as one 64-bit value: hipcc (ROCm 7.2) passed element 0
// for every j when the builtin's arguments were subscripts, and returned the first result for
// both subscripts of its 2-vector.
__device__ __forceinline__ void permlane16_swap(uint32_t& x, uint32_t& y) {
  const uint32_t a = x, b = y;
  const uint64_t sw = __builtin_bit_cast(uint64_t, __builtin_amdgcn_permlane16_swap(a, b, false, false));
  x = static_cast<uint32_t>(sw);
  y = static_cast<uint32_t>(sw >> 32);
}

// Q tile of column tile t: lane row g holds rows 4 g + i of env 16 t + (l & 15) in register i.
// Transposed over (g, t) so that lane l = 16 g + c ends with rows 0..7 of env 16 g + c = l:
// permlane32_swap of tiles (0, 2) and (1, 3) leaves rows 0-3 / 4-7 of tiles 0 and 2 (resp. 1, 3)
// in lane rows 0, 1, 2, 3 of the first register; permlane16_swap of those two registers then gives
// rows 0-3 of tile g in lane row g of the first and rows 4-7 in the second.
__device__ __forceinline__ void qnet_gather_q(const f32x4 (&acc3)[4], float (&q)[8]) {
  // Inline asm: with the builtins, hipcc (ROCm 7.2) computed register 0's swaps only and returned
  // them for all four registers. The compiler does not pad hazards inside inline asm, and the
  // operands come straight from the last layer-3 MFMAs (VGPR accumulators in the rollout kernels):
  // 16 wait states first cover the XDL-write -> VALU-read distance of a 16x16x32 result (and the
  // two a VALU write needs before a swap reads it), two more after the block.
  float x0[4], y0[4], x1[4], y1[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    x0[i] = acc3[0][i];
    y0[i] = acc3[2][i];
    x1[i] = acc3[1][i];
    y1[i] = acc3[3][i];
  }
  asm volatile(
      "s_nop 7\n\ts_nop 7\n\t"
      "v_permlane32_swap_b32 %0, %4\n\tv_permlane32_swap_b32 %8, %12\n\t"
      "v_permlane32_swap_b32 %1, %5\n\tv_permlane32_swap_b32 %9, %13\n\t"
      "v_permlane32_swap_b32 %2, %6\n\tv_permlane32_swap_b32 %10, %14\n\t"
      "v_permlane32_swap_b32 %3, %7\n\tv_permlane32_swap_b32 %11, %15\n\t"
      "s_nop 1\n\t"
      "v_permlane16_swap_b32 %0, %8\n\tv_permlane16_swap_b32 %1, %9\n\t"
      "v_permlane16_swap_b32 %2, %10\n\tv_permlane16_swap_b32 %3, %11\n\t"
      "s_nop 1"
      : "+v"(x0[0]), "+v"(x0[1]), "+v"(x0[2]), "+v"(x0[3]), "+v"(y0[0]), "+v"(y0[1]), "+v"(y0[2]), "+v"(y0[3]),
        "+v"(x1[0]), "+v"(x1[1]), "+v"(x1[2]), "+v"(x1[3]), "+v"(y1[0]), "+v"(y1[1]), "+v"(y1[2]), "+v"(y1[3]));
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    q[i] = x0[i];
    q[4 + i] = x1[i];
  }
}

// Q-values of this lane's env row0 + lane (rows 0..7) from the layer-1 B fragments of the wave's
// two 32-env column tiles (xb0: envs row0 + r, xb1: envs row0 + 32 + r, k-half h = lane >> 5),
// with the weight fragments from src, D in flight. Every lane of the wave must call it.
// Software-pipelined and fully unrolled: layer 1 of k-block kb + 1 is issued ahead of layer 2 of
// k-block kb, and its ReLU, packing and swaps are computed in pieces between kb's layer-2 MFMAs
// (each W2 fragment feeds the four column tiles' MFMAs); layer 3's k-blocks follow the last
// k-block's layer-2 row tiles they read. Unrolled, the first MFMA into each accumulator takes an
// inline zero and the next k-block's operands land in their final registers.
//
// NC (round 5): the number of 16-env column tiles computed, 1..4: lanes 16 NC .. 63 get no result.
// Column tiles are independent (each MFMA column is one env), so the envs computed get the same
// bits as in a full forward; a pass over a compacted list of the envs whose Q the reference
// evaluates (its greedy branch) skips the other tiles' MFMAs. NC <= 2 also skips the layer-1 half
// xb1 and its ReLU / swap work. A compile-time count (qnet_mlp_nc dispatches): guarding each MFMA
// with a runtime test put a scalar branch behind every MFMA and cost +66 % per h-DQN launch even
// where every tile ran (r05a).
template <int D, int NC = 4, class Src>
__device__ __forceinline__ void qnet_mlp(const Src& src, bf16x8 xb0, bf16x8 xb1, float (&q)[8]) {
  static_assert(NC >= 1 && NC <= 4, "1..4 column tiles");
  constexpr int nc = NC;
  static_assert(kQT1 == 7 && kQT2 == 7 && kQK3 == 4 && kQFrags == 60,
                "qfrag's consumption order assumes 7 k-blocks, 7 layer-2 row tiles and 4 layer-3 k-blocks");
  bf16x8 ring[D];
#pragma unroll
  for (int s = 0; s < D; ++s) ring[s] = src(s);
  auto take = [&](int s) __attribute__((always_inline)) {
    const bf16x8 f = ring[s % D];
    if (s + D < kQFrags) ring[s % D] = src(s + D);
    return f;
  };
  const f32x16 z16 = {};
  const f32x4 z4 = {};
  f32x16 c0, c1;
  constexpr bool hi = nc > 2;  // column tiles 2 and 3: the layer-1 half xb1
  auto layer1 = [&](int s) __attribute__((always_inline)) {
    const bf16x8 a1 = take(s);
    c0 = mfma32(a1, xb0, z16);
    if (hi) c1 = mfma32(a1, xb1, z16);
  };
  // packed ReLU pairs of c0 (d = 0..7) and c1 (d = 8..15)
  auto relu_d = [&](int d) __attribute__((always_inline)) {
    const f32x16& c = d < 8 ? c0 : c1;
    const int b = 2 * (d & 7);
    return relu_pair(c[b], c[b + 1]);
  };
  uint32_t nx[16];
  // swaps of column tile u's packed registers: afterwards nx[8u + q] is dword q of the B operand
  // of env tile 2u, nx[8u + 4 + q] that of env tile 2u + 1
  auto swap_u = [&](int u) __attribute__((always_inline)) {
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) permlane16_swap(nx[8 * u + qd], nx[8 * u + 4 + qd]);
  };
  auto operands = [&](bf16x8 (&hb)[4]) __attribute__((always_inline)) {
#pragma unroll
    for (int t = 0; t < 4; ++t) hb[t] = __builtin_bit_cast(bf16x8, u32x4{nx[4 * t], nx[4 * t + 1], nx[4 * t + 2], nx[4 * t + 3]});
  };
  layer1(0);
#pragma unroll
  for (int d = 0; d < 8; ++d) nx[d] = relu_d(d);
  if (hi) {
#pragma unroll
    for (int d = 8; d < 16; ++d) nx[d] = relu_d(d);
  }
  swap_u(0);
  if (hi) swap_u(1);
  bf16x8 hb[4];
  operands(hb);
  f32x4 acc2[kQT2][4];
  // One MFMA per slot and the vector work placed behind it, in source order (sched_barrier): a
  // 16x16x32 MFMA occupies the matrix pipe 16 cycles, room for one ReLU pair (v_cvt_pk + v_pk_max)
  // or one swap of the wave's own instruction stream; left to the scheduler, the four MFMAs of a
  // row tile went out back to back and the vector work behind them held the next row tile.
  auto slot = [&](f32x4& acc, const bf16x8& a, const bf16x8& b, bool zero) __attribute__((always_inline)) {
    __builtin_amdgcn_sched_barrier(0);
    acc = mfma16(a, b, zero ? z4 : acc);
  };
  int s = 1;
#pragma unroll
  for (int kb = 0; kb < kQT1 - 1; ++kb) {
    layer1(s++);
#pragma unroll
    for (int t2 = 0; t2 < kQT2; ++t2) {
      const bf16x8 a2 = take(s++);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (t < nc) slot(acc2[t2][t], a2, hb[t], kb == 0);
        // the next k-block's operands: ReLU pairs behind row tiles 1..4, swaps behind 5 and 6
        if (t2 >= 1 && t2 <= 4 && (t2 <= 2 || hi)) nx[4 * (t2 - 1) + t] = relu_d(4 * (t2 - 1) + t);
        if (t2 == 5) permlane16_swap(nx[t], nx[4 + t]);
        if (t2 == 6 && hi) permlane16_swap(nx[8 + t], nx[12 + t]);
      }
    }
    operands(hb);
  }
  // The last k-block with layer 3 interleaved. Layer-3 k-block k3 reads row tiles 2 k3 and 2 k3 + 1;
  // the ReLU pairs of its B operands are built in the slots after each row tile's MFMAs have issued
  // (two pairs per slot), into two buffers used alternately.
  f32x4 acc3[4] = {z4, z4, z4, z4};  // the tiles past nc stay zero (never read as results)
  uint32_t b3[2][4][4];
  auto pairs3 = [&](int t2, int t) __attribute__((always_inline)) {  // row tile t2 of env tile t
    const int buf = (t2 >> 1) & 1, d = 2 * (t2 & 1);
    b3[buf][t][d] = relu_pair(acc2[t2][t][0], acc2[t2][t][1]);
    b3[buf][t][d + 1] = relu_pair(acc2[t2][t][2], acc2[t2][t][3]);
  };
  // slots of layer-2 row tile t2, each followed by the pairs of row tile p (p < 0: none)
  auto layer2 = [&](int t2, int p) __attribute__((always_inline)) {
    const bf16x8 a2 = take(s++);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (t < nc) slot(acc2[t2][t], a2, hb[t], false);
      if (p >= 0 && t < nc) pairs3(p, t);
    }
  };
  auto layer3 = [&](int k3, int p) __attribute__((always_inline)) {
    const bf16x8 a3 = take(s++);
    const int buf = k3 & 1;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (2 * k3 + 1 >= kQT2) b3[buf][t][2] = b3[buf][t][3] = 0u;  // row tile 7 does not exist
      const bf16x8 b = __builtin_bit_cast(bf16x8, u32x4{b3[buf][t][0], b3[buf][t][1], b3[buf][t][2], b3[buf][t][3]});
      if (t < nc) slot(acc3[t], a3, b, k3 == 0);
      if (p >= 0 && t < nc) pairs3(p, t);
    }
  };
  static_assert(kQT2 == 7 && kQK3 == 4, "the tail below is written for 7 row tiles, 4 layer-3 k-blocks");
  layer2(0, -1);
  layer2(1, 0);
  layer2(2, 1);
  layer3(0, 2);
  layer2(3, -1);
  layer2(4, 3);
  layer3(1, 4);
  layer2(5, -1);
  layer2(6, 5);
  layer3(2, 6);
  layer3(3, -1);
  qnet_gather_q(acc3, q);
}

// qnet_mlp on nc (1..4, wave-uniform) column tiles: one instance per count. Every call site inlines
// all four, so the kernels keep one or two call sites (a pass loop), not one per pass. A weight
// fragment feeds nc MFMAs, so the fewer the column tiles the less of a fragment's load latency its
// MFMAs cover: the ring deepens as nc falls (D(nc) fragments in flight, D the full forward's; the
// fewer accumulators of a narrow instance leave the registers for it).
template <int D, class Src>
__device__ __forceinline__ void qnet_mlp_nc(const Src& src, bf16x8 xb0, bf16x8 xb1, float (&q)[8], int nc) {
  switch (nc) {
    case 1:
      qnet_mlp<4 * D, 1>(src, xb0, xb1, q);
      break;
    case 2:
      qnet_mlp<2 * D, 2>(src, xb0, xb1, q);
      break;
    case 3:
      qnet_mlp<D + D / 2, 3>(src, xb0, xb1, q);
      break;
    default:
      qnet_mlp<D, 4>(src, xb0, xb1, q);
  }
}

// the forward of a net in LDS
__device__ __forceinline__ void qnet_mlp_swp(const uint8_t* net, bf16x8 xb0, bf16x8 xb1, float (&q)[8]) {
  qnet_mlp<kQLdsAhead>(qnet_lds(net), xb0, xb1, q);
}
__device__ __forceinline__ void qnet_mlp_swp_nc(const uint8_t* net, bf16x8 xb0, bf16x8 xb1, float (&q)[8], int nc) {
  qnet_mlp_nc<kQLdsAhead>(qnet_lds(net), xb0, xb1, q, nc);
}

// Q-values of this lane's env (rows 0..7) from the block's f32 observation tile in LDS.
// row0 = tile row of this wave's lane 0. swap = the opponent's view state[5:] + state[:5]
// (scripts/main.py:199, human_player.py:40-41). Every lane of the wave must call it.
__device__ __forceinline__ void qnet_forward_swp(const uint8_t* net, const float* tile, int row0,
                                                 bool swap, float (&q)[8]) {
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  qnet_mlp_swp(net, qnet_input(tile + (row0 + r) * kObs, swap, h),
               qnet_input(tile + (row0 + 32 + r) * kObs, swap, h), q);
}

// ---------------------------------------------------------------------------- 32x32 forward
// The all-32x32x16 forward (rounds 1-3), kept for the config-5 instances without a net opponent
// (qnet_rollout_ws_kernel<0 / 1>). There the Q-net wave shares its SIMD's vector issue with an
// env wave that needs as much of it, and an MFMA holds the issue 8 cycles whatever its shape
// (MI355X_MICROARCH.md): 132 MFMAs per forward hold it 1,056 cycles, the 16x16 forward's 226 hold
// it 1,808. A/B at 2^20 envs, same process (profiles/r03/ab/qnet_16x16_ab_r03af.txt): ego-only
// 49.6 us/step with this forward, 53.2 with the 16x16 one; self-play 91.5 against 85.4.
// Its packed layout follows the 16x16 fragments in the same buffer (mg_qnet_pack writes both):
// W1 [204 x 24], W2 [104 x 232], W3 [9 x 136] bf16 rows (strides conflict-free for
// ds_read_b128), transposed as above with hidden units on the 32 rows of a tile; registers
// 8s..8s+7 of lane half h of a 32x32 accumulator hold rows 16s + 8(j>>2) + 4h + (j&3), and W2 / W3
// store each 16-column block in that k order, so an accumulator feeds the next MFMA directly.
constexpr int kQ32H1 = 224, kQ32H2 = 128;  // padded 200, 100
constexpr int kQ32S1 = 24, kQ32S2 = 232, kQ32S3 = 136;  // row strides (bf16)
// Stored rows: only up to the last row that can be non-zero plus one zero row (W1: units
// 0..202 + zero row 203; W2: 0..102 + zero row 103; W3: outputs 0..7 + zero row 8). A lane
// whose tile row lies past them reads the zero row instead (q32row*).
constexpr int kQ32R1 = 204, kQ32R2 = 104, kQ32R3 = 9;                    // stored rows per matrix
constexpr int kQ32OffW2 = kQ32R1 * kQ32S1 * 2;                           // ds_read_b128 lane group hits
constexpr int kQ32OffW3 = kQ32OffW2 + kQ32R2 * kQ32S2 * 2;                 // 16 distinct 4-bank slots
constexpr int kQ32NetBytes = kQ32OffW3 + kQ32R3 * kQ32S3 * 2;              // 60,496 B
static_assert(kQ32OffW2 % 16 == 0 && kQ32OffW3 % 16 == 0 && kQ32NetBytes % 16 == 0 && kQNetBytes % 16 == 0,
              "packed Q-net sections must stay 16-byte aligned");

__device__ __forceinline__ int q32row1(int m) { return m < kQ32R1 ? m : kQ32R1 - 1; }
__device__ __forceinline__ int q32row2(int m) { return m < kQ32R2 ? m : kQ32R2 - 1; }
__device__ __forceinline__ int q32row3(int m) { return m < kQ32R3 ? m : kQ32R3 - 1; }

// hardware k (0..15) within a 16-block -> hidden unit within that block (see above)
__host__ __device__ constexpr int q32_krow(int kk) {
  return 8 * ((kk & 7) >> 2) + 4 * (kk >> 3) + (kk & 3);
}

__device__ __forceinline__ bf16x8 relu_bf16(const f32x16& c, int s) {
  const int b = 8 * s;
  return __builtin_bit_cast(bf16x8, u32x4{relu_pair(c[b], c[b + 1]), relu_pair(c[b + 2], c[b + 3]),
                                          relu_pair(c[b + 4], c[b + 5]), relu_pair(c[b + 6], c[b + 7])});
}

// Packs fp32 torch Linear weights (row-major [out][in]) and biases into the kernel layout: element e.
__device__ __forceinline__ void qnet32_pack_at(int e, const float* w1, const float* b1, const float* w2,
                                               const float* b2, const float* w3, const float* b3, int in_dim,
                                               int out_dim, uint8_t* packed) {
  __bf16* pw1 = reinterpret_cast<__bf16*>(packed);
  __bf16* pw2 = reinterpret_cast<__bf16*>(packed + kQ32OffW2);
  __bf16* pw3 = reinterpret_cast<__bf16*>(packed + kQ32OffW3);
  // part p (0 hi, 1 mid, 2 lo) of the three-way bf16 split of b (hi + mid + lo == b)
  auto part = [](float b, int p) {
    const float hi = static_cast<float>(static_cast<__bf16>(b));
    const float r = b - hi;
    const float mid = static_cast<float>(static_cast<__bf16>(r));
    return p == 0 ? hi : p == 1 ? mid : r - mid;
  };
  if (e < kQ32R1 * kQ32S1) {  // W1[m][k]: natural k order (the input features), then b1's parts
    const int m = e / kQ32S1, k = e % kQ32S1;
    float v = 0.f;
    if (m < kQH1Real && k < in_dim) v = w1[m * in_dim + k];
    else if (m < kQH1Real && k >= kQBiasIn && k < kQBiasIn + 3) v = part(b1[m], k - kQBiasIn);
    else if (m >= kQOne1 && m < kQOne1 + 3 && k == kQBiasIn) v = 1.f;  // hidden-1 units = 1.0
    pw1[e] = static_cast<__bf16>(v);
    return;
  }
  e -= kQ32R1 * kQ32S1;
  if (e < kQ32R2 * kQ32S2) {  // W2[m][c]: columns in the accumulator's k order, then b2's parts
    const int m = e / kQ32S2, c = e % kQ32S2;
    const int src = 16 * (c / 16) + q32_krow(c % 16);
    float v = 0.f;
    if (c < kQ32H1) {
      if (m < kQH2Real && src < kQH1Real) v = w2[m * kQH1Real + src];
      else if (m < kQH2Real && src >= kQOne1 && src < kQOne1 + 3) v = part(b2[m], src - kQOne1);
      else if (m >= kQOne2 && m < kQOne2 + 3 && src == kQOne1) v = 1.f;  // hidden-2 units = 1.0
    }
    pw2[e] = static_cast<__bf16>(v);
    return;
  }
  e -= kQ32R2 * kQ32S2;
  if (e < kQ32R3 * kQ32S3) {  // W3[m][c], then b3's parts
    const int m = e / kQ32S3, c = e % kQ32S3;
    const int src = 16 * (c / 16) + q32_krow(c % 16);
    float v = 0.f;
    if (m < out_dim && c < kQ32H2) {
      if (src < kQH2Real) v = w3[m * kQH2Real + src];
      else if (src >= kQOne2 && src < kQOne2 + 3) v = part(b3[m], src - kQOne2);
    }
    pw3[e] = static_cast<__bf16>(v);
  }
}

__global__ void qnet32_pack_kernel(const float* w1, const float* b1, const float* w2, const float* b2,
                                 const float* w3, const float* b3, int in_dim, int out_dim,
                                 uint8_t* packed) {
  qnet32_pack_at(blockIdx.x * blockDim.x + threadIdx.x, w1, b1, w2, b2, w3, b3, in_dim, out_dim, packed);
}

// The grids of the two pack launches (mg_qnet_pack, the DQN learners' repack): one thread per packed element.
constexpr int kQPackBlock = 256;
constexpr unsigned kQPackBlocks = (kQFrags * 64 * 8 + kQPackBlock - 1) / kQPackBlock;  // (fragment, lane, element)
constexpr unsigned kQ32PackBlocks =
    (kQ32R1 * kQ32S1 + kQ32R2 * kQ32S2 + kQ32R3 * kQ32S3 + kQPackBlock - 1) / kQPackBlock;

// Rows 0-3 of the env of lane 32t + r sit in registers 0-3 of lane half 0 of column tile t,
// rows 4-7 in lane half 1. One v_permlane32_swap per register pair (gfx950) exchanges tile 0's
// upper half with tile 1's lower half: afterwards register j of the first operand holds row j and
// of the second row 4 + j of the lane's own env, in both lane halves (the ds_bpermute round trip
// plus selects it replaces sat between the forward's last MFMA and the argmax).
__device__ __forceinline__ void qnet32_gather_q(const f32x16& acc3_0, const f32x16& acc3_1, int h,
                                              float (&q)[8]) {
  (void)h;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    // operands into locals first and the result read as one 64-bit value: hipcc (ROCm 7.2)
    // passed element 0 for every j when the builtin's arguments were subscripts, and returned
    // the first result for both subscripts of its 2-vector
    const float a = acc3_0[j], b = acc3_1[j];
    const uint32_t x = __builtin_bit_cast(uint32_t, a), y = __builtin_bit_cast(uint32_t, b);
    const uint64_t sw = __builtin_bit_cast(uint64_t, __builtin_amdgcn_permlane32_swap(x, y, false, false));
    q[j] = __builtin_bit_cast(float, static_cast<uint32_t>(sw));
    q[4 + j] = __builtin_bit_cast(float, static_cast<uint32_t>(sw >> 32));
  }
}

__device__ __forceinline__ void qnet32_mlp(const uint8_t* net, bf16x8 xb0, bf16x8 xb1, float (&q)[8]) {
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int z = opaque_zero();
  const __bf16* W1 = reinterpret_cast<const __bf16*>(net) + z;
  const __bf16* W2 = reinterpret_cast<const __bf16*>(net + kQ32OffW2) + z;
  const __bf16* W3 = reinterpret_cast<const __bf16*>(net + kQ32OffW3) + z;
  f32x16 acc2a[4] = {}, acc2b[4] = {};
  const f32x16 zero = {};
  auto layer1 = [&](int mt, f32x16& c0, f32x16& c1) {
    const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(W1 + q32row1(32 * mt + r) * kQ32S1 + 8 * h);
    c0 = mfma32(a1, xb0, zero);
    c1 = mfma32(a1, xb1, zero);
  };
  f32x16 c0, c1;
  layer1(0, c0, c1);
  // hb[f]: f = 0, 1 -> column tile 0 k-steps 0, 1; f = 2, 3 -> column tile 1
  bf16x8 hb[4] = {relu_bf16(c0, 0), relu_bf16(c0, 1), relu_bf16(c1, 0), relu_bf16(c1, 1)};
  auto w2frag = [&](int mt, int j) {
    return *reinterpret_cast<const bf16x8*>(W2 + q32row2(32 * (j >> 1) + r) * kQ32S2 + 16 * (2 * mt + (j & 1)) + 8 * h);
  };
  // one hidden tile: its layer 2, with the next tile's layer 1 + ReLU folded in when `more`
  // (a constant at every call site). nk: 16-unit k-blocks of the tile that hold real units --
  // the last tile's second block (units 208-223) is all padding, so it is skipped.
  auto tile_step = [&](int mt, bool more, int nk) __attribute__((always_inline)) {
    bf16x8 a2n = w2frag(mt, 0);
    if (more) layer1(mt + 1, c0, c1);
    uint32_t nx[16];  // next tile's packed ReLU pairs, built between this tile's MFMAs
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int m2 = j >> 1, sk = j & 1;
      if (sk >= nk) continue;
      // one fragment ahead: the next load is in flight under this pair of MFMAs
      const bf16x8 a2 = a2n;
      const int jn = nk == 2 ? j + 1 : j + 2;
      if (jn < 8) a2n = w2frag(mt, jn);
      __builtin_amdgcn_sched_barrier(0);
      acc2a[m2] = mfma32(a2, hb[sk], acc2a[m2]);
      acc2b[m2] = mfma32(a2, hb[2 + sk], acc2b[m2]);
      if (more) {
#pragma unroll
        for (int pp = 2 * j; pp < 2 * j + 2; ++pp) {
          const int f = pp >> 2, b = 8 * (f & 1) + 2 * (pp & 3);
          const f32x16& c = f < 2 ? c0 : c1;
          nx[pp] = relu_pair(c[b], c[b + 1]);
        }
      }
    }
    if (more) {
#pragma unroll
      for (int f = 0; f < 4; ++f)
        hb[f] = __builtin_bit_cast(bf16x8, u32x4{nx[4 * f], nx[4 * f + 1], nx[4 * f + 2], nx[4 * f + 3]});
    }
  };
  constexpr int kLast = kQ32H1 / 32 - 1;
  static_assert(16 * (2 * kLast + 1) >= kQH1Real && 32 * kLast < kQH1Real,
                "only the last hidden tile's second k-block is padding");
#pragma unroll
  for (int mt = 0; mt < kLast; ++mt) tile_step(mt, true, 2);
  // The last hidden tile (its k-block 0 only) interleaved with layer 3, over the k-blocks holding
  // real units (96..111 carries units 100..102 = 1.0 too; 112..127 is padding). acc2a/b[m2] are
  // final once the tile's pair m2 has issued, so layer 3's k-blocks 2 m2 and 2 m2 + 1 -- their
  // ReLU and MFMAs, in the same order as before -- follow pair m2 + 1 instead of the whole tile:
  // the tile's MFMAs had no vector work beside them and layer 3 is mostly vector work. W2 and W3
  // fragments one ahead.
  f32x16 acc3_0 = {}, acc3_1 = {};
  auto w3frag = [&](int kb) { return *reinterpret_cast<const bf16x8*>(W3 + q32row3(r) * kQ32S3 + 16 * kb + 8 * h); };
  constexpr int kK3 = (kQH2Real + 15) / 16;
  static_assert(kK3 == 7 && kQ32H2 / 32 == 4, "layer 3 k-blocks 2 m2, 2 m2 + 1 follow layer-2 row tile m2");
  bf16x8 a3n = w3frag(0);
  auto layer3 = [&](int m2) __attribute__((always_inline)) {
#pragma unroll
    for (int sk = 0; sk < 2; ++sk) {
      const int kb = 2 * m2 + sk;
      if (kb >= kK3) continue;
      const bf16x8 a3 = a3n;
      if (kb + 1 < kK3) a3n = w3frag(kb + 1);
      acc3_0 = mfma32(a3, relu_bf16(acc2a[m2], sk), acc3_0);
      acc3_1 = mfma32(a3, relu_bf16(acc2b[m2], sk), acc3_1);
    }
  };
  bf16x8 a2n = w2frag(kLast, 0);
#pragma unroll
  for (int m2 = 0; m2 < kQ32H2 / 32; ++m2) {
    const bf16x8 a2 = a2n;
    if (m2 + 1 < kQ32H2 / 32) a2n = w2frag(kLast, 2 * (m2 + 1));
    __builtin_amdgcn_sched_barrier(0);
    acc2a[m2] = mfma32(a2, hb[0], acc2a[m2]);
    acc2b[m2] = mfma32(a2, hb[2], acc2b[m2]);
    if (m2 > 0) layer3(m2 - 1);
  }
  layer3(kQ32H2 / 32 - 1);
  qnet32_gather_q(acc3_0, acc3_1, h, q);
}

// the 32x32 forward of a net whose 32x32 layout is in LDS, from the block's observation tile
__device__ __forceinline__ void qnet32_forward(const uint8_t* net32, const float* tile, int row0, bool swap,
                                               float (&q)[8]) {
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  qnet32_mlp(net32, qnet_input(tile + (row0 + r) * kObs, swap, h), qnet_input(tile + (row0 + 32 + r) * kObs, swap, h), q);
}

// mg_qnet_fragments: the packed layout is fragment-major itself since ABI 19, so the "fragment
// copy" the h-DQN opponent is read from is a plain copy (kept so the ABI-18 callers run unchanged)
__global__ __launch_bounds__(64) void qnet_fragments_kernel(const uint8_t* packed, uint8_t* frags) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < kQNetBytes / 16) reinterpret_cast<u32x4*>(frags)[i] = reinterpret_cast<const u32x4*>(packed)[i];
}

// Standalone forward for tests / evaluation: q[i][0..7] for x[i][0..in_dim-1], staged in LDS as
// 16-float rows (swap, in_dim 10 only: the features in the order state[5:] + state[:5]).
__global__ __launch_bounds__(kBlock) void qnet_forward_kernel(const uint8_t* net, const float* x,
                                                              int in_dim, int swap, float* qout,
                                                              int64_t n) {
  __shared__ __attribute__((aligned(16))) uint8_t lds_net[kQNetBytes];
  __shared__ __attribute__((aligned(16))) float tile[kBlock * 16];
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kBlock;
  qnet_to_lds(net, lds_net);
  for (int j = threadIdx.x; j < kBlock * 16; j += kBlock) {
    const int64_t i = base + (j >> 4);
    const int k = j & 15;
    const int src = swap ? (k + kObs / 2) % kObs : k;
    tile[j] = (i < n && k < in_dim) ? x[i * in_dim + src]
              : (k >= kQBiasIn && k < kQBiasIn + 3) ? 1.f : 0.f;
  }
  __syncthreads();
  float q[8];
  {
    const int lane = threadIdx.x & 63, row0 = (threadIdx.x >> 6) * 64;
    qnet_mlp_swp(lds_net, qnet_input_wide(tile + (row0 + (lane & 31)) * 16, lane >> 5),
                 qnet_input_wide(tile + (row0 + 32 + (lane & 31)) * 16, lane >> 5), q);
  }
  const int64_t i = base + threadIdx.x;
  if (i < n) {
#pragma unroll
    for (int j = 0; j < 8; ++j) qout[i * 8 + j] = q[j];
  }
}

}  // namespace
