// The Checkers IAC / COMA baseline critics over TRANSITION rows (part of ABI 9, additive): the value networks
// networks.V_checkers_local (networks.py:415-435, IAC) and networks.V_checkers_global (:438-458), and the COMA critic
// networks.Q_coma_checkers (:293-306), at the widths alg_baseline_checkers.py:117-138 passes (config_checkers_stage2.json) -- the
// evaluations of alg_baseline_checkers.train_step that carry no gradient (V_target / V on the next-step columns :527, Q_target :572,
// Q :617).  No kernel takes a tiled feed: row r = b N + n is decoded with critic_rows::decode (form ROWS) and gathers its inputs from
// the batch's base columns (grid [B][54], agent state [B][N][4], goals [B][N], actions [B][N], windows [B][N][75], obs_self_v
// [B][N][4], obs_others [B][N][2(N-1)]); "others" run over the agents j != n in ascending order.  Input dtypes are those of
// k_critic_checkers_rows (critic_checkers.hip); everything is rounded to float32, as the reference's tf.float32 placeholders do.
//
// ---- the value networks (k_value_checkers_rows<N, KIND>, N = 1..8; stage 1 = N = 1: no second branch) -------------------------------
//   local:   conv = relu(conv2d SAME [3][3][3][6] over window[5][5][3])  -> 150   x1 = concat(conv, v_obs[4], goal[2])   [156]
//            x2 = obs_others [2(N-1)]
//   global:  conv = relu(conv2d SAME [3][5][2][4] over grid[3][9][2])    -> 108   x1 = concat(conv, s_n[4], g_n[2])      [114]
//            x2 = the states of the other agents [4(N-1)]
//   branch1 = relu(x1 . [K1][256] + b)     branch2 = relu(x2 . [K2][32] + b)
//   h2  = relu(branch1 . [256][256] + branch2 . [32][256])   (no bias)             out = h2 . [256][1] + bias
// ---- the COMA critic (k_coma_checkers_rows<N>, N = 2..8) ----------------------------------------------------------------------------
//   x = concat(conv_s(grid) [108], states of all agents [4N], one-hot actions of the others [5(N-1)], g_n [2], goals of the others
//              [2(N-1)], one-hot label of n [N], conv_o(window of n) [150], obs_self_v of n [4]),  K = 257 + 12N
//   h1 = relu(x . [K][256] + b)     h2 = relu(h1 . [256][256] + b)     q = h2 . [256][5] + b
//
// Mapping, that of k_critic_checkers_rows: 256 threads = 4 waves own 64 rows; every layer is ck_tiles.h's gemm_tiles on the exact-f32
// matrix instruction (v_mfma_f32_16x16x4_f32), B operands from packed per-lane tiles; the convolutions are Toeplitz matrices built by
// the pack kernels.  SUMMATION ORDER: every output element is ONE chain of fused multiply-adds that starts at 0 and runs over k in
// ascending order of the layer's tile columns -- in a convolution the NHWC-flattened input, in branch1 / h1 the tile layout below (the
// convolution outputs first, then the vector inputs), in the value networks' h2 branch1's 256 units and then branch2's 32 in the same
// chain; padding columns hold zero inputs and zero weights.  The bias is added to the finished chain in float32, then the ReLU.  A
// row's bits depend on neither its place in the workgroup nor the launch's row count; one-hot inputs are 0 / 1 inputs of the chains.
// LDS, value kernels: region A [64][260] (x1 = conv out | the 6 vector inputs, padded to 16; later h2) and region B [64][292] (the raw
//   input tile and x2; later hidden = concat(branch1[256], branch2[32])): 141 312 bytes, one workgroup per CU.
// LDS, COMA kernel: region A [64][112 + 160 + pad16(12N-1) + 4] (x1 = conv_s out | conv_o out | the 12N-1 vector inputs; later h2 at
//   stride 260) and region H [64][260] (the raw grid [64][68] and window [64][84] tiles until the convolutions are done; later h1):
//   161 792 bytes at N = 8, under the 163 840 a workgroup may declare (with the 512 bytes of row indices).
#include "ck_tiles.h"
#include "critic_rows.h"

namespace cm3 {
namespace ck_baseline {

using critic_rows::decode;
using critic_rows::kFormRows;
constexpr int kLocal = CM3_VALUE_LOCAL, kGlobal = CM3_VALUE_GLOBAL;
constexpr int kMaxAgents = 8;                                 // the Checkers range
constexpr int kH1 = 256, kH1B = 32, kH2 = 256;                // {V,Q}_n_h1_1, _n_h1_2, _n_h2 (config_checkers_stage2.json)
constexpr int kQU = 256;                                      // units of Q_coma_checkers
constexpr int kGrid = 54, kGridF = 4, kGridOut = 108;         // 3 x 9 x 2 -> 3 x 9 x 4
constexpr int kWin = 75, kWinF = 6, kWinOut = 150;            // 5 x 5 x 3 -> 5 x 5 x 6
constexpr int kKG = 64, kNG = 112, kKW = 80, kNW = 160;       // the Toeplitz matrices, padded to whole tiles
constexpr int kLdG = kKG + 4, kLdW = kKW + 4;
constexpr int kLdH = 256 + 4;                                 // row stride of a 256-wide hidden tile (4 mod 64 words)

constexpr int tiles(int k, int n) { return (n / 16) * (k / 16) * 256; }
constexpr int pad16(int k) { return (k + 15) / 16 * 16; }

// goal bit k of agent (flat index bn): one-hot int64 [..][2] or uint8 index
__device__ __forceinline__ float goal_bit(const void *goals, int onehot, size_t bn, int k) {
  if (onehot) return (float)reinterpret_cast<const int64_t *>(goals)[bn * 2 + k];
  const int gl = reinterpret_cast<const uint8_t *>(goals)[bn];
  return (gl == 0) == (k == 0) ? 1.0f : 0.0f;
}

__device__ __forceinline__ float narrow_at(const void *p, int f64, size_t at) {
  return f64 ? (float)reinterpret_cast<const double *>(p)[at] : (float)reinterpret_cast<const int8_t *>(p)[at];
}

// ================================================================================================================================
// the value networks
// ================================================================================================================================
template <int KIND> struct Geo {      // the network's one convolution: local the window, global the grid
  static constexpr bool kWindow = KIND == kLocal;
  static constexpr int kIn = kWindow ? kWin : kGrid, kOut = kWindow ? kWinOut : kGridOut, kF = kWindow ? kWinF : kGridF;
  static constexpr int kKC = kWindow ? kKW : kKG, kNC = kWindow ? kNW : kNG;
  static constexpr int kLdIn = kKC + 4;
  static constexpr int kK1 = kNC + 16;                        // x1: conv out | 4 state / v_obs values, 2 goal bits, 10 zeros
};

constexpr int kVLdA = kLdH, kVLdB = kH1 + kH1B + 4;           // regions A and B of the value kernels
constexpr int kVLdsFloats = 64 * (kVLdA + kVLdB);
static_assert(kVLdsFloats * 4 <= 2 * 64 * 292 * 4, "no more than the two [64][292] regions of k_critic_checkers_rows");
static_assert(Geo<kLocal>::kK1 + 4 <= kVLdA && Geo<kGlobal>::kK1 + 4 <= kVLdA, "x1 lies in region A");

template <int N, int KIND> struct ValueLayout {
  using G = Geo<KIND>;
  static constexpr bool kStage2 = N > 1;
  static constexpr int K2 = !kStage2 ? 0 : (KIND == kLocal ? 2 * (N - 1) : 4 * (N - 1));
  static constexpr int K2P = kStage2 ? pad16(K2) : 0;         // <= 32
  static constexpr int kLdX2 = K2P + 4;
  static constexpr int KH = kStage2 ? kH1 + kH1B : kH1;       // width of concat(branch1, branch2)
  // packed weights (floats): B tiles [col tile][k group][lane][4] (ck_tiles.h), each followed by its bias
  static constexpr int kPC = 0;
  static constexpr int kPCB = kPC + tiles(G::kKC, G::kNC);
  static constexpr int kP1 = kPCB + G::kNC;
  static constexpr int kP1B = kP1 + tiles(G::kK1, kH1);
  static constexpr int kP2 = kP1B + kH1;
  static constexpr int kP2B = kP2 + (kStage2 ? tiles(K2P, kH1B) : 0);
  static constexpr int kPH = kP2B + (kStage2 ? kH1B : 0);
  static constexpr int kPO = kPH + tiles(KH, kH2);
  static constexpr int kPOB = kPO + tiles(kH2, 16);
  static constexpr int kTotal = kPOB + 16;
  static_assert(64 * (G::kLdIn + kLdX2) <= 64 * kVLdB, "the input tiles must fit into region B");
  static_assert(KH + 4 <= kVLdB, "the hidden tile is region B");
};

struct ValuePackParams {
  const float *conv_w, *conv_b, *w_b1, *b_b1, *w_b1_h2, *w_b2, *b_b2, *w_b2_h2, *w_out, *b_out;
};

template <int N, int KIND> __global__ void __launch_bounds__(256) k_value_checkers_pack(const ValuePackParams p, float *out) {
  using L = ValueLayout<N, KIND>;
  using G = Geo<KIND>;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < L::kTotal; t += gridDim.x * 256) {
    int base, K, layer;
    if (t < L::kPCB) { base = L::kPC; K = G::kKC; layer = 0; }
    else if (t < L::kP1) { base = L::kPCB; K = 0; layer = 10; }
    else if (t < L::kP1B) { base = L::kP1; K = G::kK1; layer = 1; }
    else if (t < L::kP2) { base = L::kP1B; K = 0; layer = 11; }
    else if (t < L::kP2B) { base = L::kP2; K = L::K2P; layer = 2; }
    else if (t < L::kPH) { base = L::kP2B; K = 0; layer = 12; }
    else if (t < L::kPO) { base = L::kPH; K = L::KH; layer = 3; }
    else if (t < L::kPOB) { base = L::kPO; K = kH2; layer = 4; }
    else { base = L::kPOB; K = 0; layer = 14; }
    const int u = t - base;
    float v = 0.0f;
    if (layer < 10) {
      const int j = u & 3, lane = (u >> 2) & 63, gi = u >> 8, KG = K / 16, g = gi % KG, ct = gi / KG;
      const int k = 16 * g + 4 * (lane >> 4) + j, n = 16 * ct + (lane & 15);
      switch (layer) {
        case 0:
          if constexpr (G::kWindow) v = toeplitz<5, 5, 3, kWinF, 3, 3>(p.conv_w, k, n);
          else v = toeplitz<3, 9, 2, kGridF, 3, 5>(p.conv_w, k, n);
          break;
        case 1: {     // x1 column k: conv output k (k < kOut), or vector input k - kNC (6 of them, behind the conv outputs)
          const int kin = k < G::kNC ? (k < G::kOut ? k : -1) : (k - G::kNC < 6 ? G::kOut + (k - G::kNC) : -1);
          v = kin >= 0 ? p.w_b1[kin * kH1 + n] : 0.0f;
          break;
        }
        case 2: v = k < L::K2 ? p.w_b2[k * kH1B + n] : 0.0f; break;
        case 3:
          if (k < kH1) v = p.w_b1_h2[k * kH2 + n];
          else if constexpr (L::kStage2) v = p.w_b2_h2[(k - kH1) * kH2 + n];
          break;
        default: v = n == 0 ? p.w_out[k] : 0.0f; break;
      }
    } else {
      switch (layer) {
        case 10: v = u < G::kOut ? p.conv_b[u % G::kF] : 0.0f; break;
        case 11: v = p.b_b1[u]; break;
        case 12: v = p.b_b2[u]; break;
        default: v = u == 0 ? p.b_out[0] : 0.0f; break;
      }
    }
    out[t] = v;
  }
}

struct ValueParams {
  uint32_t n_rows;
  int grid_f64, windows_f64, goals_onehot, reward_f64;
  const void *grid;               // global: [B][54] int8 / float64
  const double *vec;              // global: [B][N][4]
  const void *goals;              // [B][N] uint8 index / [B][N][2] int64 one-hot
  const void *windows;            // local: [B][N][75] int8 / float64
  const double *obs_self_v;       // local: [B][N][4]
  const double *obs_others;       // local, stage 2: [B][N][2(N-1)]
  const void *reward;             // [B][N] float32 / float64 (td)
  const uint8_t *done;            // [B] (td)
  double gamma;
  float *v;                       // optional [n_rows]
  double *v64, *td;               // optional [n_rows]
  const float *packed;
};

// (the register budget and occupancy of k_critic_checkers_rows: one workgroup per CU, 1..2 waves per SIMD)
template <int N, int KIND>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) k_value_checkers_rows(const ValueParams p) {
  using L = ValueLayout<N, KIND>;
  using G = Geo<KIND>;
  __shared__ __attribute__((aligned(16))) float smem[kVLdsFloats];
  __shared__ uint32_t sB[64];
  __shared__ int sN[64];
  float *sA = smem, *sBk = smem + 64 * kVLdA;
  float *sIn = sBk, *sX2 = sBk + 64 * G::kLdIn;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t rows = p.n_rows;
  const uint32_t row_base = blockIdx.x * 64u;
  const float *pk = p.packed;

  // ---- the rows' indices, and the 6 inputs of x1 that are no convolution output (lane = row; a lane past the count reads the last row)
  if (w == 0) {
    const uint32_t r = row_base + lane;
    uint32_t b;
    int m, n, a;
    decode<N, kFormRows>(r < rows ? r : rows - 1, b, m, n, a);
    sB[lane] = b;
    sN[lane] = n;
    const size_t bn = (size_t)b * N + n;
    const double *st = G::kWindow ? p.obs_self_v : p.vec;
    float *x = sA + lane * kVLdA + G::kNC;
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = (float)st[bn * 4 + k];
    x[4] = goal_bit(p.goals, p.goals_onehot, bn, 0);
    x[5] = goal_bit(p.goals, p.goals_onehot, bn, 1);
#pragma unroll
    for (int k = 6; k < 16; ++k) x[k] = 0.0f;
  }
  float4 b_c[5];      // the convolution's first B operands: 5 column tiles per wave (window), 4 or 3 (grid)
  if constexpr (G::kWindow) {
    load_b0<5, G::kKC / 16>(pk + L::kPC, 5 * (w >> 1), lane, b_c);
  } else {
    float4 b4[4], b3[3];
    if ((w >> 1) == 0) {
      load_b0<4, G::kKC / 16>(pk + L::kPC, 0, lane, b4);
#pragma unroll
      for (int c = 0; c < 4; ++c) b_c[c] = b4[c];
    } else {
      load_b0<3, G::kKC / 16>(pk + L::kPC, 4, lane, b3);
#pragma unroll
      for (int c = 0; c < 3; ++c) b_c[c] = b3[c];
    }
  }
  __syncthreads();
  // ---- the input tiles: window [64][80] / grid [64][64], x2 [64][K2P] -------------------------------------------------------------
  for (int idx = tid; idx < 64 * G::kKC; idx += 256) {
    const int r = idx / G::kKC, k = idx - r * G::kKC;
    float v = 0.0f;
    if (k < G::kIn) {
      if constexpr (G::kWindow) v = narrow_at(p.windows, p.windows_f64, ((size_t)sB[r] * N + sN[r]) * kWin + k);
      else v = narrow_at(p.grid, p.grid_f64, (size_t)sB[r] * kGrid + k);
    }
    sIn[r * G::kLdIn + k] = v;
  }
  if constexpr (L::kStage2) {
    for (int idx = tid; idx < 64 * L::K2P; idx += 256) {
      const int r = idx / L::K2P, k = idx - r * L::K2P;
      const size_t base = (size_t)sB[r] * N;
      const int n = sN[r];
      float v = 0.0f;
      if (k < L::K2) {
        if constexpr (KIND == kLocal) {
          v = (float)p.obs_others[(base + n) * (2 * (N - 1)) + k];
        } else {
          const int u = k >> 2;
          v = (float)p.vec[(base + u + (u >= n ? 1 : 0)) * 4 + (k & 3)];
        }
      }
      sX2[r * L::kLdX2 + k] = v;
    }
  }
  __syncthreads();
  // ---- the convolution (Toeplitz) into x1, relu; branch2 into registers ------------------------------------------------------------
  f32x4 acc_b2[1][2];
  float bias_b2[2] = {0.0f, 0.0f};
  float4 b_1[4];
  {
    if constexpr (G::kWindow) {
      f32x4 acc[2][5];
      float bias[5];
      load_bias<5>(pk + L::kPCB, 5 * (w >> 1), lane, bias);
      zero_tiles(acc);
      gemm_tiles<2, 5, G::kKC / 16>(sIn, G::kLdIn, 2 * (w & 1), pk + L::kPC, 5 * (w >> 1), lane, b_c, acc);
      store_relu<2, 5>(sA, kVLdA, 2 * (w & 1), 5 * (w >> 1), bias, lane, acc);
    } else if ((w >> 1) == 0) {
      f32x4 acc[2][4];
      float bias[4];
      const float4 b4[4] = {b_c[0], b_c[1], b_c[2], b_c[3]};
      load_bias<4>(pk + L::kPCB, 0, lane, bias);
      zero_tiles(acc);
      gemm_tiles<2, 4, G::kKC / 16>(sIn, G::kLdIn, 2 * (w & 1), pk + L::kPC, 0, lane, b4, acc);
      store_relu<2, 4>(sA, kVLdA, 2 * (w & 1), 0, bias, lane, acc);
    } else {
      f32x4 acc[2][3];
      float bias[3];
      const float4 b3[3] = {b_c[0], b_c[1], b_c[2]};
      load_bias<3>(pk + L::kPCB, 4, lane, bias);
      zero_tiles(acc);
      gemm_tiles<2, 3, G::kKC / 16>(sIn, G::kLdIn, 2 * (w & 1), pk + L::kPC, 4, lane, b3, acc);
      store_relu<2, 3>(sA, kVLdA, 2 * (w & 1), 4, bias, lane, acc);
    }
    zero_tiles(acc_b2);
    if constexpr (L::kStage2) {   // wave w: row tile w, both column tiles
      float4 b_2[2];
      load_b0<2, L::K2P / 16>(pk + L::kP2, 0, lane, b_2);
      load_bias<2>(pk + L::kP2B, 0, lane, bias_b2);
      gemm_tiles<1, 2, L::K2P / 16>(sX2, L::kLdX2, w, pk + L::kP2, 0, lane, b_2, acc_b2);
    }
    load_b0<4, G::kK1 / 16>(pk + L::kP1, 4 * w, lane, b_1);
  }
  __syncthreads();   // x1 is complete, nobody reads the input tiles any more: region B becomes the hidden tile
  // ---- branch1: x1 -> hidden[:, 0:256], relu; wave w owns columns [64w, 64w + 64) from here on; branch2 -> hidden[:, 256:288] ------
  float4 b_h[4];
  {
    if constexpr (L::kStage2) store_relu<1, 2>(sBk + kH1, kVLdB, w, 0, bias_b2, lane, acc_b2);
    f32x4 acc[4][4];
    float bias[4];
    load_bias<4>(pk + L::kP1B, 4 * w, lane, bias);
    zero_tiles(acc);
    gemm_tiles<4, 4, G::kK1 / 16>(sA, kVLdA, 0, pk + L::kP1, 4 * w, lane, b_1, acc);
    load_b0<4, L::KH / 16>(pk + L::kPH, 4 * w, lane, b_h);
    store_relu<4, 4>(sBk, kVLdB, 0, 4 * w, bias, lane, acc);
  }
  __syncthreads();
  // ---- h2 = relu(ONE chain over concat(branch1, branch2)), no bias; into region A (x1 is dead) -------------------------------------
  float4 b_o[1];
  {
    f32x4 acc[4][4];
    const float bias[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    zero_tiles(acc);
    gemm_tiles<4, 4, L::KH / 16>(sBk, kVLdB, 0, pk + L::kPH, 4 * w, lane, b_h, acc);
    load_b0<1, kH2 / 16>(pk + L::kPO, 0, lane, b_o);
    store_relu<4, 4>(sA, kVLdA, 0, 4 * w, bias, lane, acc);
  }
  __syncthreads();
  // ---- out: wave w finishes rows [16w, 16w + 16); column 0 of the tile is V: lanes 0, 16, 32, 48 hold four rows each ---------------
  f32x4 acc[1][1];
  zero_tiles(acc);
  gemm_tiles<1, 1, kH2 / 16>(sA, kVLdA, w, pk + L::kPO, 0, lane, b_o, acc);
  if ((lane & 15) == 0) {
    const float bo = pk[L::kPOB];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int lr = 16 * w + 4 * (lane >> 4) + reg;
      const uint32_t hr = row_base + lr;
      if (hr >= rows) continue;
      const float v = acc[0][0][reg] + bo;
      if (p.v) p.v[hr] = v;
      if (p.v64) p.v64[hr] = (double)v;
      if (p.td) {
        // reward_local + gamma * v * not_done in the order of k_td_target (batch.hip) on the widened v; hr = b N + n indexes [B][N]
        const double rw = p.reward_f64 ? reinterpret_cast<const double *>(p.reward)[hr] : (double)reinterpret_cast<const float *>(p.reward)[hr];
        const double gv = p.gamma * (double)v;
        p.td[hr] = rw + gv * (double)(int64_t)(p.done[sB[lr]] ? 0 : 1);
      }
    }
  }
}

template <int N, int KIND> static int value_launch(const ValueParams &p, hipStream_t s) {
  const unsigned blocks = (p.n_rows + 63u) / 64u;
  note_variant("k_value_checkers_rows", (int)sizeof(float), N, 4, 0, 0, 0, 0, 0, 0, /* prec=f32 */ 0);
  note_tail(KIND == kLocal ? ",kind=local" : ",kind=global");
  hipLaunchKernelGGL((k_value_checkers_rows<N, KIND>), dim3(blocks), dim3(256), 0, s, p);
  CM3_HIP_CHECK(hipGetLastError());
  return CM3_OK;
}

template <int N, int KIND> static int value_pack_launch(const ValuePackParams &p, float *out, hipStream_t s) {
  hipLaunchKernelGGL((k_value_checkers_pack<N, KIND>), dim3(128), dim3(256), 0, s, p, out);
  CM3_HIP_CHECK(hipGetLastError());
  return CM3_OK;
}

template <typename F> static int agents_1_to_8(int n_agents, F &&f) { return agent_launch<1, 2, 3, 4, 5, 6, 7, 8>(n_agents, f); }

static size_t value_floats_for(int n, int kind) {
  bool hit;
  return agent_dispatch<1, 2, 3, 4, 5, 6, 7, 8>(n, hit, [&](auto k) {
    constexpr int N = k();
    if (kind == kLocal) return (size_t)ValueLayout<N, kLocal>::kTotal;
    if (kind == kGlobal) return (size_t)ValueLayout<N, kGlobal>::kTotal;
    return (size_t)0;
  });
}

static int value_check_desc(const cm3_value_checkers_desc *d) {
  CM3_REQUIRE(d, "null desc");
  CM3_REQUIRE(d->n_agents >= 1 && d->n_agents <= kMaxAgents, "n_agents must be in 1..%d", kMaxAgents);
  CM3_REQUIRE(d->kind == kLocal || d->kind == kGlobal, "kind must be CM3_VALUE_LOCAL (0) or CM3_VALUE_GLOBAL (1), got %d", d->kind);
  CM3_REQUIRE(d->stage == 1 || d->stage == 2, "stage must be 1 or 2, got %d", d->stage);
  CM3_REQUIRE((d->stage == 1) == (d->n_agents == 1), "%s runs at stage 1 with one agent and at stage 2 with more (n_agents %d, stage %d)",
              d->kind == kLocal ? "V_checkers_local" : "V_checkers_global", d->n_agents, d->stage);
  CM3_REQUIRE(d->n_h1_1 == kH1 && d->n_h1_2 == kH1B && d->n_h2 == kH2,
              "supported Checkers value-network widths are 256/32/256 (config_checkers_stage2.json); got %d/%d/%d", d->n_h1_1, d->n_h1_2,
              d->n_h2);
  return CM3_OK;
}

// ================================================================================================================================
// the COMA critic
// ================================================================================================================================
template <int N> struct ComaLayout {
  static_assert(N >= 2 && N <= kMaxAgents, "Q_coma_checkers exists with 2..8 agents");
  static constexpr int T = 12 * N - 1;                        // the vector inputs: states, others' actions, goals, label, v_obs
  static constexpr int TP = pad16(T);
  static constexpr int kTail = kNG + kNW;                     // x1: conv_s out | conv_o out | the T vector inputs
  static constexpr int K1 = kTail + TP;
  static constexpr int kLdX = K1 + 4;                         // row stride of region A (4 mod 16 words)
  static constexpr int kLdsFloats = 64 * (kLdX + kLdH);
  // offsets of the vector inputs in the tail, and of the network's input (the rows of h1/kernel)
  static constexpr int oAct = 4 * N, oGoal = oAct + kA * (N - 1), oGoalOthers = oGoal + 2, oLabel = oGoalOthers + 2 * (N - 1),
                       oObs = oLabel + N;                     // oObs = 12 N - 5: what lies between conv_s and conv_o
  static_assert(oObs + 4 == T, "T = 12 N - 1");
  static constexpr int K = kGridOut + T + kWinOut;            // 257 + 12 N
  // packed weights (floats): B tiles [col tile][k group][lane][4] (ck_tiles.h), each followed by its bias
  static constexpr int kPG = 0;
  static constexpr int kPGB = kPG + tiles(kKG, kNG);
  static constexpr int kPW = kPGB + kNG;
  static constexpr int kPWB = kPW + tiles(kKW, kNW);
  static constexpr int kP1 = kPWB + kNW;
  static constexpr int kP1B = kP1 + tiles(K1, kQU);
  static constexpr int kP2 = kP1B + kQU;
  static constexpr int kP2B = kP2 + tiles(kQU, kQU);
  static constexpr int kPO = kP2B + kQU;
  static constexpr int kPOB = kPO + tiles(kQU, 16);
  static constexpr int kTotal = kPOB + 16;
  static_assert(64 * (kLdG + kLdW) <= 64 * kLdH, "the raw grid and window tiles lie in the hidden tile's region");
  static_assert(kLdH <= kLdX, "h2 overwrites x1");
  static_assert(kLdsFloats * 4 + 512 <= 160 * 1024, "what a single workgroup may declare, with the row indices");
};
static_assert(ComaLayout<8>::kLdsFloats * 4 == 161792, "[64][372] + [64][260] floats at N = 8");

struct ComaPackParams {
  const float *conv_s_w, *conv_s_b, *conv_o_w, *conv_o_b, *w_h1, *b_h1, *w_h2, *b_h2, *w_out, *b_out;
};

// row of h1/kernel that column c of the x1 tile holds (-1: padding)
template <int N> __device__ __forceinline__ int coma_x1_input(int c) {
  using L = ComaLayout<N>;
  if (c < kNG) return c < kGridOut ? c : -1;                                            // conv_s
  if (c < L::kTail) return c - kNG < kWinOut ? kGridOut + L::oObs + (c - kNG) : -1;     // conv_o
  const int t = c - L::kTail;                                                           // states .. label | v_obs
  return t < L::oObs ? kGridOut + t : (t < L::T ? kGridOut + kWinOut + t : -1);
}

template <int N> __global__ void __launch_bounds__(256) k_coma_checkers_pack(const ComaPackParams p, float *out) {
  using L = ComaLayout<N>;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < L::kTotal; t += gridDim.x * 256) {
    int base, K, layer;
    if (t < L::kPGB) { base = L::kPG; K = kKG; layer = 0; }
    else if (t < L::kPW) { base = L::kPGB; K = 0; layer = 10; }
    else if (t < L::kPWB) { base = L::kPW; K = kKW; layer = 1; }
    else if (t < L::kP1) { base = L::kPWB; K = 0; layer = 11; }
    else if (t < L::kP1B) { base = L::kP1; K = L::K1; layer = 2; }
    else if (t < L::kP2) { base = L::kP1B; K = 0; layer = 12; }
    else if (t < L::kP2B) { base = L::kP2; K = kQU; layer = 3; }
    else if (t < L::kPO) { base = L::kP2B; K = 0; layer = 13; }
    else if (t < L::kPOB) { base = L::kPO; K = kQU; layer = 4; }
    else { base = L::kPOB; K = 0; layer = 14; }
    const int u = t - base;
    float v = 0.0f;
    if (layer < 10) {
      const int j = u & 3, lane = (u >> 2) & 63, gi = u >> 8, KG = K / 16, g = gi % KG, ct = gi / KG;
      const int k = 16 * g + 4 * (lane >> 4) + j, n = 16 * ct + (lane & 15);
      switch (layer) {
        case 0: v = toeplitz<3, 9, 2, kGridF, 3, 5>(p.conv_s_w, k, n); break;
        case 1: v = toeplitz<5, 5, 3, kWinF, 3, 3>(p.conv_o_w, k, n); break;
        case 2: {
          const int kin = coma_x1_input<N>(k);
          v = kin >= 0 ? p.w_h1[kin * kQU + n] : 0.0f;
          break;
        }
        case 3: v = p.w_h2[k * kQU + n]; break;
        default: v = n < kA ? p.w_out[k * kA + n] : 0.0f; break;
      }
    } else {
      switch (layer) {
        case 10: v = u < kGridOut ? p.conv_s_b[u % kGridF] : 0.0f; break;
        case 11: v = u < kWinOut ? p.conv_o_b[u % kWinF] : 0.0f; break;
        case 12: v = p.b_h1[u]; break;
        case 13: v = p.b_h2[u]; break;
        default: v = u < kA ? p.b_out[u] : 0.0f; break;
      }
    }
    out[t] = v;
  }
}

struct ComaParams {
  uint32_t n_rows;
  int grid_f64, windows_f64, goals_onehot, reward_f64;
  const void *grid;               // [B][54] int8 / float64
  const double *vec;              // [B][N][4]
  const void *goals;              // [B][N] uint8 index / [B][N][2] int64 one-hot
  const int32_t *actions;         // [B][N]: the others' one-hot actions
  const int32_t *own_actions;     // optional [B][N]: the row's own action (q_taken, q_taken64, td)
  const void *windows;            // [B][N][75] int8 / float64
  const double *obs_self_v;       // [B][N][4]
  const void *reward;             // [B] float32 / float64 (td): the GLOBAL reward
  const uint8_t *done;            // [B] (td)
  double gamma;
  float *q;                       // optional [n_rows][5]
  float *q_taken;                 // optional [n_rows]
  double *q_taken64, *td;         // optional [n_rows]
  const float *packed;
};

template <int N>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) k_coma_checkers_rows(const ComaParams p) {
  using L = ComaLayout<N>;
  __shared__ __attribute__((aligned(16))) float smem[L::kLdsFloats];
  __shared__ uint32_t sB[64];
  __shared__ int sN[64];
  float *sA = smem, *sH = smem + 64 * L::kLdX;
  float *sG = sH, *sW = sH + 64 * kLdG;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t rows = p.n_rows;
  const uint32_t row_base = blockIdx.x * 64u;
  const float *pk = p.packed;

  // ---- the rows' indices (lane = row; a lane past the count reads the last row's inputs) -------------------------------------------
  if (w == 0) {
    const uint32_t r = row_base + lane;
    uint32_t b;
    int m, n, a;
    decode<N, kFormRows>(r < rows ? r : rows - 1, b, m, n, a);
    sB[lane] = b;
    sN[lane] = n;
  }
  float4 b_g4[4], b_g3[3], b_w[5];
  if ((w >> 1) == 0) load_b0<4, kKG / 16>(pk + L::kPG, 0, lane, b_g4);
  else load_b0<3, kKG / 16>(pk + L::kPG, 4, lane, b_g3);
  load_b0<5, kKW / 16>(pk + L::kPW, 5 * (w >> 1), lane, b_w);
  __syncthreads();
  // ---- the input tiles: grid [64][64], window [64][80] (in the hidden tile's region), the TP vector inputs of x1 --------------------
  for (int idx = tid; idx < 64 * kKG; idx += 256) {
    const int r = idx >> 6, k = idx & 63;
    sG[r * kLdG + k] = k < kGrid ? narrow_at(p.grid, p.grid_f64, (size_t)sB[r] * kGrid + k) : 0.0f;
  }
  for (int idx = tid; idx < 64 * kKW; idx += 256) {
    const int r = idx / kKW, k = idx - r * kKW;
    sW[r * kLdW + k] = k < kWin ? narrow_at(p.windows, p.windows_f64, ((size_t)sB[r] * N + sN[r]) * kWin + k) : 0.0f;
  }
  for (int idx = tid; idx < 64 * L::TP; idx += 256) {
    const int r = idx / L::TP, t = idx - r * L::TP;
    const size_t base = (size_t)sB[r] * N;
    const int n = sN[r];
    float v = 0.0f;
    if (t < L::oAct) {                                    // the states of all agents
      v = (float)p.vec[base * 4 + t];
    } else if (t < L::oGoal) {                            // one-hot actions of the others
      const int u = (t - L::oAct) / kA, kk = (t - L::oAct) - kA * u;
      v = p.actions[base + u + (u >= n ? 1 : 0)] == kk ? 1.0f : 0.0f;
    } else if (t < L::oGoalOthers) {                      // g_n
      v = goal_bit(p.goals, p.goals_onehot, base + n, t - L::oGoal);
    } else if (t < L::oLabel) {                           // goals of the others
      const int u = (t - L::oGoalOthers) >> 1;
      v = goal_bit(p.goals, p.goals_onehot, base + u + (u >= n ? 1 : 0), (t - L::oGoalOthers) & 1);
    } else if (t < L::oObs) {                             // the label of n
      v = (t - L::oLabel) == n ? 1.0f : 0.0f;
    } else if (t < L::T) {                                // obs_self_v of n
      v = (float)p.obs_self_v[(base + n) * 4 + (t - L::oObs)];
    }
    sA[r * L::kLdX + L::kTail + t] = v;
  }
  __syncthreads();
  // ---- the two convolutions (Toeplitz) into x1, relu ----------------------------------------------------------------------------------
  float4 b_1[4];
  {
    if ((w >> 1) == 0) {
      f32x4 acc[2][4];
      float bias[4];
      load_bias<4>(pk + L::kPGB, 0, lane, bias);
      zero_tiles(acc);
      gemm_tiles<2, 4, kKG / 16>(sG, kLdG, 2 * (w & 1), pk + L::kPG, 0, lane, b_g4, acc);
      store_relu<2, 4>(sA, L::kLdX, 2 * (w & 1), 0, bias, lane, acc);
    } else {
      f32x4 acc[2][3];
      float bias[3];
      load_bias<3>(pk + L::kPGB, 4, lane, bias);
      zero_tiles(acc);
      gemm_tiles<2, 3, kKG / 16>(sG, kLdG, 2 * (w & 1), pk + L::kPG, 4, lane, b_g3, acc);
      store_relu<2, 3>(sA, L::kLdX, 2 * (w & 1), 4, bias, lane, acc);
    }
    {
      f32x4 acc[2][5];
      float bias[5];
      load_bias<5>(pk + L::kPWB, 5 * (w >> 1), lane, bias);
      zero_tiles(acc);
      gemm_tiles<2, 5, kKW / 16>(sW, kLdW, 2 * (w & 1), pk + L::kPW, 5 * (w >> 1), lane, b_w, acc);
      store_relu<2, 5>(sA + kNG, L::kLdX, 2 * (w & 1), 5 * (w >> 1), bias, lane, acc);
    }
    load_b0<4, L::K1 / 16>(pk + L::kP1, 4 * w, lane, b_1);
  }
  __syncthreads();   // x1 is complete, nobody reads the raw tiles any more: their region becomes h1
  // ---- h1: x1 [64][K1] -> h1 [64][256], relu; wave w owns columns [64w, 64w + 64) from here on --------------------------------------
  float4 b_2[4];
  {
    f32x4 acc[4][4];
    float bias[4];
    load_bias<4>(pk + L::kP1B, 4 * w, lane, bias);
    zero_tiles(acc);
    gemm_tiles<4, 4, L::K1 / 16>(sA, L::kLdX, 0, pk + L::kP1, 4 * w, lane, b_1, acc);
    load_b0<4, kQU / 16>(pk + L::kP2, 4 * w, lane, b_2);
    store_relu<4, 4>(sH, kLdH, 0, 4 * w, bias, lane, acc);
  }
  __syncthreads();
  // ---- h2 = relu(h1 . [256][256] + b) into region A at stride 260 (x1 is dead) --------------------------------------------------------
  float4 b_o[1];
  {
    f32x4 acc[4][4];
    float bias[4];
    load_bias<4>(pk + L::kP2B, 4 * w, lane, bias);
    zero_tiles(acc);
    gemm_tiles<4, 4, kQU / 16>(sH, kLdH, 0, pk + L::kP2, 4 * w, lane, b_2, acc);
    load_b0<1, kQU / 16>(pk + L::kPO, 0, lane, b_o);
    store_relu<4, 4>(sA, kLdH, 0, 4 * w, bias, lane, acc);
  }
  __syncthreads();
  // ---- out: wave w finishes rows [16w, 16w + 16); columns 0..4 of the tile are Q: lane (col, hi) holds unit col of rows 4 hi .. + 3 ---
  f32x4 acc[1][1];
  zero_tiles(acc);
  gemm_tiles<1, 1, kQU / 16>(sA, kLdH, w, pk + L::kPO, 0, lane, b_o, acc);
  const int col = lane & 15;
  if (col < kA) {
    const float bo = pk[L::kPOB + col];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int lr = 16 * w + 4 * (lane >> 4) + reg;
      const uint32_t hr = row_base + lr;
      if (hr >= rows) continue;
      const float q = acc[0][0][reg] + bo;
      if (p.q) p.q[(size_t)hr * kA + col] = q;
      if (p.own_actions && p.own_actions[hr] == col) {      // q[r][actions[b][n]] (hr = b N + n indexes [B][N]): this lane holds it
        if (p.q_taken) p.q_taken[hr] = q;
        if (p.q_taken64) p.q_taken64[hr] = (double)q;
        if (p.td) {
          // reward + gamma * q_taken * not_done in the order of k_td_target (batch.hip) on the widened value; the GLOBAL reward [B]
          const uint32_t b = sB[lr];
          const double rw = p.reward_f64 ? reinterpret_cast<const double *>(p.reward)[b] : (double)reinterpret_cast<const float *>(p.reward)[b];
          const double gq = p.gamma * (double)q;
          p.td[hr] = rw + gq * (double)(int64_t)(p.done[b] ? 0 : 1);
        }
      }
    }
  }
}

template <int N> static int coma_launch(const ComaParams &p, hipStream_t s) {
  if constexpr (N >= 2) {
    const unsigned blocks = (p.n_rows + 63u) / 64u;
    note_variant("k_coma_checkers_rows", (int)sizeof(float), N, 4, 0, 0, 0, 0, 0, 0, /* prec=f32 */ 0);
    hipLaunchKernelGGL((k_coma_checkers_rows<N>), dim3(blocks), dim3(256), 0, s, p);
    CM3_HIP_CHECK(hipGetLastError());
    return CM3_OK;
  } else {
    return fail(CM3_ERR_INVALID, "n_agents %d unsupported", N);
  }
}

template <int N> static int coma_pack_launch(const ComaPackParams &p, float *out, hipStream_t s) {
  if constexpr (N >= 2) {
    hipLaunchKernelGGL((k_coma_checkers_pack<N>), dim3(128), dim3(256), 0, s, p, out);
    CM3_HIP_CHECK(hipGetLastError());
    return CM3_OK;
  } else {
    return fail(CM3_ERR_INVALID, "n_agents %d unsupported", N);
  }
}

static size_t coma_floats_for(int n) {
  bool hit;
  return agent_dispatch<2, 3, 4, 5, 6, 7, 8>(n, hit, [&](auto k) { return (size_t)ComaLayout<k()>::kTotal; });
}

static int coma_check_desc(const cm3_coma_checkers_desc *d) {
  CM3_REQUIRE(d, "null desc");
  CM3_REQUIRE(d->n_agents >= 2 && d->n_agents <= kMaxAgents, "n_agents must be in 2..%d: Q_coma_checkers exists with more than one agent only",
              kMaxAgents);
  CM3_REQUIRE(d->units == kQU, "the supported Checkers COMA critic width is 256 (units of Q_coma_checkers); got %d", d->units);
  return CM3_OK;
}

// the row count of n_steps time steps of N agents, behind the checks on it (the order of critic_rows::check_rows)
static int row_count(int64_t n_steps, int N, uint32_t &n_rows) {
  CM3_REQUIRE(n_steps > 0, "n_steps must be positive");
  CM3_REQUIRE(n_steps <= (int64_t)0x7fffffff / N, "n_steps %lld gives more than 2^31 - 1 rows (%lld per time step)", (long long)n_steps,
              (long long)N);
  n_rows = (uint32_t)(n_steps * N);
  return CM3_OK;
}
}  // namespace ck_baseline
}  // namespace cm3

extern "C" size_t cm3_value_checkers_packed_bytes(int32_t n_agents, int32_t kind) {
  return cm3::ck_baseline::value_floats_for(n_agents, kind) * sizeof(float);
}

extern "C" int cm3_value_checkers_pack(const cm3_value_checkers_desc *d, const cm3_value_checkers_weights *wt, void *packed, void *stream) {
  using namespace cm3;
  using namespace cm3::ck_baseline;
  int rc = value_check_desc(d);
  if (rc != CM3_OK) return rc;
  CM3_REQUIRE(wt, "null weights");
  CM3_REQUIRE(packed, "packed is NULL: cm3_value_checkers_packed_bytes(n_agents, kind) bytes of device memory");
  CM3_REQUIRE(wt->conv_w && wt->conv_b && wt->w_b1 && wt->b_b1 && wt->w_b1_h2 && wt->w_out && wt->b_out,
              "missing weights: conv/Conv/weights, conv/Conv/biases, the branch-1 kernel and bias, W_self_h2 / W_branch1_h2, the output "
              "kernel and bias");
  CM3_REQUIRE(d->stage == 1 || (wt->w_b2 && wt->b_b2 && wt->w_b2_h2),
              "missing stage-2 weights: the branch-2 kernel and bias, stage-2/W_others_h2 / stage-2/W_branch2_h2");
  CM3_REQUIRE((uintptr_t)packed % 16 == 0, "misaligned packed: must be 16-byte aligned");
  const ValuePackParams p = {wt->conv_w, wt->conv_b, wt->w_b1, wt->b_b1, wt->w_b1_h2, wt->w_b2, wt->b_b2, wt->w_b2_h2, wt->w_out, wt->b_out};
  hipStream_t s = (hipStream_t)stream;
  const int kind = d->kind;
  return agents_1_to_8(d->n_agents, [&](auto n) {
    return kind == kLocal ? value_pack_launch<n(), kLocal>(p, (float *)packed, s) : value_pack_launch<n(), kGlobal>(p, (float *)packed, s);
  });
}

extern "C" int cm3_value_checkers_rows_f32(const cm3_value_checkers_desc *d, const cm3_value_checkers_weights *wt,
                                           const cm3_value_checkers_rows *r, void *stream) {
  using namespace cm3;
  using namespace cm3::ck_baseline;
  int rc = value_check_desc(d);
  if (rc != CM3_OK) return rc;
  CM3_REQUIRE(wt, "null weights");
  CM3_REQUIRE(r, "null rows");
  CM3_REQUIRE(wt->packed, "packed weights are NULL: run cm3_value_checkers_pack once per weight update");
  const int N = d->n_agents;
  const bool local = d->kind == kLocal, others = local && N > 1;
  uint32_t n_rows;
  rc = row_count(r->n_steps, N, n_rows);
  if (rc != CM3_OK) return rc;
  CM3_REQUIRE(r->goals && (local ? (r->windows && r->obs_self_v) : (r->grid && r->vec)),
              "missing inputs: goals, and windows and obs_self_v (V_checkers_local) or grid and vec (V_checkers_global), are required");
  CM3_REQUIRE(!others || r->obs_others, "missing input: V_checkers_local reads obs_others at stage 2");
  CM3_REQUIRE(r->v || r->v64 || r->td, "no output requested: set v, v64 or td");
  CM3_REQUIRE(!r->td || (r->reward && r->done), "missing inputs: td needs reward and done");
  CM3_REQUIRE((!r->goals_onehot || (uintptr_t)r->goals % 8 == 0) &&
                  (local ? ((uintptr_t)r->obs_self_v % 8 == 0 && (!r->windows_f64 || (uintptr_t)r->windows % 8 == 0) &&
                            (!others || (uintptr_t)r->obs_others % 8 == 0))
                         : ((uintptr_t)r->vec % 8 == 0 && (!r->grid_f64 || (uintptr_t)r->grid % 8 == 0))),
              "misaligned inputs: vec, obs_self_v, obs_others, float64 grids / windows and one-hot goals must be 8-byte aligned");
  CM3_REQUIRE(!r->td || (uintptr_t)r->reward % (r->reward_f64 ? 8 : 4) == 0, "misaligned reward");
  CM3_REQUIRE((uintptr_t)r->v % 4 == 0 && (uintptr_t)r->v64 % 8 == 0 && (uintptr_t)r->td % 8 == 0,
              "misaligned outputs: v must be 4-byte aligned, v64 and td 8-byte aligned");
  CM3_REQUIRE((uintptr_t)wt->packed % 16 == 0, "misaligned packed: must be 16-byte aligned");
  ValueParams p;
  memset(&p, 0, sizeof(p));
  p.n_rows = n_rows;
  p.grid_f64 = r->grid_f64;
  p.windows_f64 = r->windows_f64;
  p.goals_onehot = r->goals_onehot;
  p.reward_f64 = r->reward_f64;
  p.grid = r->grid;
  p.vec = r->vec;
  p.goals = r->goals;
  p.windows = r->windows;
  p.obs_self_v = r->obs_self_v;
  p.obs_others = r->obs_others;
  p.reward = r->reward;
  p.done = r->done;
  p.gamma = r->gamma;
  p.v = r->v;
  p.v64 = r->v64;
  p.td = r->td;
  p.packed = (const float *)wt->packed;
  hipStream_t s = (hipStream_t)stream;
  return agents_1_to_8(N, [&](auto n) { return local ? value_launch<n(), kLocal>(p, s) : value_launch<n(), kGlobal>(p, s); });
}

extern "C" size_t cm3_coma_checkers_packed_bytes(int32_t n_agents) { return cm3::ck_baseline::coma_floats_for(n_agents) * sizeof(float); }

extern "C" int cm3_coma_checkers_pack(const cm3_coma_checkers_desc *d, const cm3_coma_checkers_weights *wt, void *packed, void *stream) {
  using namespace cm3;
  using namespace cm3::ck_baseline;
  int rc = coma_check_desc(d);
  if (rc != CM3_OK) return rc;
  CM3_REQUIRE(wt, "null weights");
  CM3_REQUIRE(packed, "packed is NULL: cm3_coma_checkers_packed_bytes(n_agents) bytes of device memory");
  CM3_REQUIRE(wt->conv_s_w && wt->conv_s_b && wt->conv_o_w && wt->conv_o_b && wt->w_h1 && wt->b_h1 && wt->w_h2 && wt->b_h2 && wt->w_out &&
                  wt->b_out,
              "missing weights: conv_s/Conv/{weights,biases}, conv_o/Conv/{weights,biases}, stage-2/Q_coma_checkers/{h1,h2,out}/{kernel,bias}");
  CM3_REQUIRE((uintptr_t)packed % 16 == 0, "misaligned packed: must be 16-byte aligned");
  const ComaPackParams p = {wt->conv_s_w, wt->conv_s_b, wt->conv_o_w, wt->conv_o_b, wt->w_h1, wt->b_h1, wt->w_h2, wt->b_h2, wt->w_out, wt->b_out};
  hipStream_t s = (hipStream_t)stream;
  return agents_1_to_8(d->n_agents, [&](auto n) { return coma_pack_launch<n()>(p, (float *)packed, s); });
}

extern "C" int cm3_coma_checkers_rows_f32(const cm3_coma_checkers_desc *d, const cm3_coma_checkers_weights *wt,
                                          const cm3_coma_checkers_rows *r, void *stream) {
  using namespace cm3;
  using namespace cm3::ck_baseline;
  int rc = coma_check_desc(d);
  if (rc != CM3_OK) return rc;
  CM3_REQUIRE(wt, "null weights");
  CM3_REQUIRE(r, "null rows");
  CM3_REQUIRE(wt->packed, "packed weights are NULL: run cm3_coma_checkers_pack once per weight update");
  const int N = d->n_agents;
  uint32_t n_rows;
  rc = row_count(r->n_steps, N, n_rows);
  if (rc != CM3_OK) return rc;
  CM3_REQUIRE(r->grid && r->vec && r->goals && r->windows && r->obs_self_v,
              "missing inputs: grid, vec, goals, windows and obs_self_v are required");
  CM3_REQUIRE(r->actions, "missing input: Q_coma_checkers reads the actions of the others");
  CM3_REQUIRE(r->q || r->q_taken || r->q_taken64 || r->td, "no output requested: set q, q_taken, q_taken64 or td");
  CM3_REQUIRE(!(r->q_taken || r->q_taken64 || r->td) || r->own_actions, "missing input: q_taken, q_taken64 and td need own_actions");
  CM3_REQUIRE(!r->td || (r->reward && r->done), "missing inputs: td needs reward and done");
  CM3_REQUIRE((uintptr_t)r->vec % 8 == 0 && (uintptr_t)r->obs_self_v % 8 == 0 && (uintptr_t)r->actions % 4 == 0 &&
                  (uintptr_t)r->own_actions % 4 == 0 && (!r->grid_f64 || (uintptr_t)r->grid % 8 == 0) &&
                  (!r->windows_f64 || (uintptr_t)r->windows % 8 == 0) && (!r->goals_onehot || (uintptr_t)r->goals % 8 == 0),
              "misaligned inputs: vec, obs_self_v, float64 grids / windows and one-hot goals must be 8-byte aligned, actions and own_actions "
              "4-byte aligned");
  CM3_REQUIRE(!r->td || (uintptr_t)r->reward % (r->reward_f64 ? 8 : 4) == 0, "misaligned reward");
  CM3_REQUIRE((uintptr_t)r->q % 4 == 0 && (uintptr_t)r->q_taken % 4 == 0 && (uintptr_t)r->q_taken64 % 8 == 0 && (uintptr_t)r->td % 8 == 0,
              "misaligned outputs: q and q_taken must be 4-byte aligned, q_taken64 and td 8-byte aligned");
  CM3_REQUIRE((uintptr_t)wt->packed % 16 == 0, "misaligned packed: must be 16-byte aligned");
  ComaParams p;
  memset(&p, 0, sizeof(p));
  p.n_rows = n_rows;
  p.grid_f64 = r->grid_f64;
  p.windows_f64 = r->windows_f64;
  p.goals_onehot = r->goals_onehot;
  p.reward_f64 = r->reward_f64;
  p.grid = r->grid;
  p.vec = r->vec;
  p.goals = r->goals;
  p.actions = r->actions;
  p.own_actions = r->own_actions;
  p.windows = r->windows;
  p.obs_self_v = r->obs_self_v;
  p.reward = r->reward;
  p.done = r->done;
  p.gamma = r->gamma;
  p.q = r->q;
  p.q_taken = r->q_taken;
  p.q_taken64 = r->q_taken64;
  p.td = r->td;
  p.packed = (const float *)wt->packed;
  hipStream_t s = (hipStream_t)stream;
  return agents_1_to_8(N, [&](auto n) { return coma_launch<n()>(p, s); });
}
