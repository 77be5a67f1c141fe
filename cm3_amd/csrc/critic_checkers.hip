// CM3 Checkers critics over TRANSITION rows (part of ABI 9, additive): networks.Q_global_checkers (networks.py:155-183) and
// networks.Q_credit_checkers (:244-272) at the widths of config_checkers_stage{1,2}.json, the evaluations of
// alg_credit_checkers.train_step that carry no gradient -- Q_global_target (:558-569), Q_credit_target (:611-629), the counterfactual
// Q_credit over every action (:738-747), and at N = 1 the counterfactual Q_global of stage 1 (:704-713).
//   conv    = relu(conv2d SAME 3x5x2 -> 4 over grid[3][9][2])        -> 108  (NHWC flatten)
//   conv_o  = relu(conv2d SAME 3x3x3 -> 6 over window[5][5][3])      -> 150
//   branch1 = relu(concat(conv, s_n[4], g_n[2], a[5], conv_o, v_obs[4]) [273] . Q_branch1/kernel[273][256] + bias)
//   branch2 = relu(x2 . stage-2/Q_branch2/kernel[K2][32] + bias)                              (stage 2)
//     global: x2 = concat(s_others[4(N-1)], a_others[5(N-1)]), K2 = 9(N-1);  credit: x2 = concat(s_m[4], s_others[4(N-1)]), K2 = 4N
//   h2  = relu(branch1 . W_branch1_h2[256][256] + branch2 . stage-2/W_branch2_h2[32][256])   (no bias)
//   out = h2 . Q_out/kernel[256][1] + Q_out/bias[1]
// Like k_critic_particle_rows (critic.hip) the kernel takes NO tiled feed: a row's inputs are an index function of the batch's base
// columns (grid [B][54], agent state [B][N][4], goals [B][N], actions [B][N], windows [B][N][75], obs_self_v [B][N][4]):
//   ROWS  (global)             r = b N + n              a = onehot(actions[b][n]); window and v_obs of agent n
//   PAIRS (credit)             r = (b N + m) N + n      s_n, g_n, s_others of agent n; a = onehot(actions[b][m]), s_m = vec[b][m];
//                                                       window and v_obs of agent M (the reference repeats obs_self_t / obs_self_v
//                                                       "indexed by m", alg_credit_checkers.py:604-605, :637-638)
//   CF    (credit; global N=1) r = r' 5 + a             a = row a of eye(5); r' = the PAIRS index, or b
// Mapping: the Checkers actor's (actor_checkers.hip) -- 256 threads = 4 waves own 64 rows, every layer is ck_tiles.h's gemm_tiles on
// the exact-f32 matrix instruction (v_mfma_f32_16x16x4_f32) in a fixed k order, B operands from packed per-lane tiles; a row's bits
// depend on neither its place in the workgroup nor the launch's row count, and the one-hot inputs are 0 / 1 INPUTS of the same chains
// in every form.  Both convolutions are Toeplitz matrices (grid 54 -> 108 as [64 x 112], window 75 -> 150 as [80 x 160]).
// LDS: two [64][292] float regions, 149 504 bytes, one workgroup per CU:
//   region B: the input tiles grid [64][68], window [64][84], x2 [64][68]; later hidden = concat(branch1[256], branch2[32]) [64][292]
//   region A: x1 [64][292] = conv out (cols 0..111), conv_o out (112..271), s_n g_n a v_obs (272..286); later h2 [64][292]
// branch2 runs with the convolutions (its inputs sit in region B) and waits in 8 accumulator registers until region B is free.
#include "ck_tiles.h"
#include "critic_rows.h"

namespace cm3 {
namespace ck_critic {

using namespace critic_rows;   // (kinds, forms, form_exists, decode, form_dispatch, the entries' checks)
constexpr int kMaxAgents = 8;                                 // the Checkers actor's range
constexpr int kH1 = 256, kH1B = 32, kH2 = 256;                // Q_n_h1_1, Q_n_h1_2, Q_n_h2 (config_checkers_stage{1,2}.json)
constexpr int kGrid = 54, kGridF = 4, kGridOut = 108;         // 3 x 9 x 2 -> 3 x 9 x 4
constexpr int kWin = 75, kWinF = 6, kWinOut = 150;            // 5 x 5 x 3 -> 5 x 5 x 6
constexpr int kKG = 64, kNG = 112, kKW = 80, kNW = 160;       // the Toeplitz matrices, padded to whole tiles
constexpr int kK1 = 288, kTail = kNG + kNW;                   // x1 (273 inputs): conv | conv_o | tail of 15 (+ 1)
constexpr int kLd = kK1 + 4;                                  // row stride of regions A and B (4 mod 64 words)
constexpr int kLdG = kKG + 4, kLdW = kKW + 4, kLdX2 = 64 + 4;
constexpr int kLdsFloats = 2 * 64 * kLd;
static_assert(64 * (kLdG + kLdW + kLdX2) <= 64 * kLd, "the input tiles must fit into region B");
static_assert(kLdsFloats * 4 <= 160 * 1024, "the CU's LDS");

constexpr int tiles(int k, int n) { return (n / 16) * (k / 16) * 256; }

template <int N, int KIND> struct Layout {
  static constexpr bool kStage2 = N > 1;
  static constexpr int K2 = !kStage2 ? 0 : (KIND == kGlobal ? 9 * (N - 1) : 4 * N);
  static constexpr int K2P = (K2 + 15) / 16 * 16;             // <= 64
  static constexpr int KH = kStage2 ? kH1 + kH1B : kH1;       // width of concat(branch1, branch2)
  // packed weights (floats): B tiles [col tile][k group][lane][4] (ck_tiles.h), each followed by its bias
  static constexpr int kPG = 0;
  static constexpr int kPGB = kPG + tiles(kKG, kNG);
  static constexpr int kPW = kPGB + kNG;
  static constexpr int kPWB = kPW + tiles(kKW, kNW);
  static constexpr int kP1 = kPWB + kNW;
  static constexpr int kP1B = kP1 + tiles(kK1, kH1);
  static constexpr int kP2 = kP1B + kH1;
  static constexpr int kP2B = kP2 + (kStage2 ? tiles(K2P, kH1B) : 0);
  static constexpr int kPH = kP2B + (kStage2 ? kH1B : 0);
  static constexpr int kPO = kPH + tiles(KH, kH2);
  static constexpr int kPOB = kPO + tiles(kH2, 16);
  static constexpr int kTotal = kPOB + 16;
  static_assert(K2P <= 64, "x2 tile width");
};

struct PackParams {
  const float *conv_w, *conv_b, *conv_o_w, *conv_o_b, *w_b1, *b_b1, *w_b1_h2, *w_b2, *b_b2, *w_b2_h2, *w_out, *b_out;
};

// input of Q_branch1/kernel that column c of the x1 tile holds (-1: padding)
__device__ __forceinline__ int x1_input(int c) {
  if (c < kNG) return c < kGridOut ? c : -1;                                  // conv
  if (c < kTail) return c - kNG < kWinOut ? kGridOut + 11 + (c - kNG) : -1;   // conv_o
  const int t = c - kTail;                                                    // s_n[4] g_n[2] a[5] | v_obs[4]
  return t < 11 ? kGridOut + t : (t < 15 ? kGridOut + 11 + kWinOut + (t - 11) : -1);
}

template <int N, int KIND> __global__ void __launch_bounds__(256) k_critic_checkers_pack(const PackParams p, float *out) {
  using L = Layout<N, KIND>;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < L::kTotal; t += gridDim.x * 256) {
    int base, K, layer;
    if (t < L::kPGB) { base = L::kPG; K = kKG; layer = 0; }
    else if (t < L::kPW) { base = L::kPGB; K = 0; layer = 10; }
    else if (t < L::kPWB) { base = L::kPW; K = kKW; layer = 1; }
    else if (t < L::kP1) { base = L::kPWB; K = 0; layer = 11; }
    else if (t < L::kP1B) { base = L::kP1; K = kK1; layer = 2; }
    else if (t < L::kP2) { base = L::kP1B; K = 0; layer = 12; }
    else if (t < L::kP2B) { base = L::kP2; K = L::K2P; layer = 3; }
    else if (t < L::kPH) { base = L::kP2B; K = 0; layer = 13; }
    else if (t < L::kPO) { base = L::kPH; K = L::KH; layer = 4; }
    else if (t < L::kPOB) { base = L::kPO; K = kH2; layer = 5; }
    else { base = L::kPOB; K = 0; layer = 15; }
    const int u = t - base;
    float v = 0.0f;
    if (layer < 10) {
      const int j = u & 3, lane = (u >> 2) & 63, gi = u >> 8, KG = K / 16, g = gi % KG, ct = gi / KG;
      const int k = 16 * g + 4 * (lane >> 4) + j, n = 16 * ct + (lane & 15);
      switch (layer) {
        case 0: v = toeplitz<3, 9, 2, kGridF, 3, 5>(p.conv_w, k, n); break;
        case 1: v = toeplitz<5, 5, 3, kWinF, 3, 3>(p.conv_o_w, k, n); break;
        case 2: {
          const int kin = x1_input(k);
          v = kin >= 0 ? p.w_b1[kin * kH1 + n] : 0.0f;
          break;
        }
        case 3: v = k < L::K2 ? p.w_b2[k * kH1B + n] : 0.0f; break;
        case 4:
          if (k < kH1) v = p.w_b1_h2[k * kH2 + n];
          else if constexpr (L::kStage2) v = p.w_b2_h2[(k - kH1) * kH2 + n];
          break;
        default: v = n == 0 ? p.w_out[k] : 0.0f; break;
      }
    } else {
      switch (layer) {
        case 10: v = u < kGridOut ? p.conv_b[u % kGridF] : 0.0f; break;
        case 11: v = u < kWinOut ? p.conv_o_b[u % kWinF] : 0.0f; break;
        case 12: v = p.b_b1[u]; break;
        case 13: v = p.b_b2[u]; break;
        default: v = u == 0 ? p.b_out[0] : 0.0f; break;
      }
    }
    out[t] = v;
  }
}

struct Params {
  uint32_t n_rows;
  int grid_f64, windows_f64, goals_onehot, reward_f64;
  const void *grid;               // [B][54] int8 / float64
  const double *vec;              // [B][N][4]
  const void *goals;              // [B][N] uint8 index / [B][N][2] int64 one-hot
  const int32_t *actions;         // [B][N] (ROWS, PAIRS)
  const void *windows;            // [B][N][75] int8 / float64
  const double *obs_self_v;       // [B][N][4]
  const void *reward;             // [B][N] float32 / float64 (td)
  const uint8_t *done;            // [B] (td)
  double gamma;
  float *q;                       // optional [n_rows]
  double *q64, *td;               // optional [n_rows]
  const float *packed;
};

// (CM3_MATRIX_KERNEL's register budget -- 256 VGPRs, accumulators in architectural registers -- with the occupancy the LDS tile allows:
// one workgroup per CU, so the declared range is 1..2 waves per SIMD and not "at least 2")
template <int N, int KIND, int FORM>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) k_critic_checkers_rows(const Params p) {
  using L = Layout<N, KIND>;
  static_assert(form_exists(KIND, FORM, N), "forms: global ROWS (and CF at N = 1), credit PAIRS / CF at N > 1");
  __shared__ __attribute__((aligned(16))) float smem[kLdsFloats];
  __shared__ uint32_t sB[64];
  __shared__ int sMNA[64];
  float *sA = smem, *sBk = smem + 64 * kLd;
  float *sG = sBk, *sW = sBk + 64 * kLdG, *sX2 = sBk + 64 * (kLdG + kLdW);
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t rows = p.n_rows;
  const uint32_t row_base = blockIdx.x * 64u;
  const float *pk = p.packed;

  // ---- the rows' indices, and the 15 inputs of x1 that are no convolution output (lane = row) ------------------------------------
  if (w == 0) {
    const uint32_t r = row_base + lane;
    uint32_t b;
    int m, n, a;
    decode<N, FORM>(r < rows ? r : rows - 1, b, m, n, a);
    sB[lane] = b;
    sMNA[lane] = m | (n << 8);
    const size_t bn = (size_t)b * N + n, bm = (size_t)b * N + m;
    float *x = sA + lane * kLd + kTail;
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = (float)p.vec[bn * 4 + k];
    if (p.goals_onehot) {
      x[4] = (float)reinterpret_cast<const int64_t *>(p.goals)[bn * 2];
      x[5] = (float)reinterpret_cast<const int64_t *>(p.goals)[bn * 2 + 1];
    } else {
      const int gl = reinterpret_cast<const uint8_t *>(p.goals)[bn];
      x[4] = gl == 0 ? 1.0f : 0.0f;
      x[5] = gl == 0 ? 0.0f : 1.0f;
    }
    if constexpr (FORM != kFormCf) a = p.actions[bm];
#pragma unroll
    for (int k = 0; k < kA; ++k) x[6 + k] = a == k ? 1.0f : 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) x[11 + k] = (float)p.obs_self_v[bm * 4 + k];
    x[15] = 0.0f;
  }
  float4 b_g4[4], b_g3[3], b_w[5];
  if ((w >> 1) == 0) load_b0<4, kKG / 16>(pk + L::kPG, 0, lane, b_g4);
  else load_b0<3, kKG / 16>(pk + L::kPG, 4, lane, b_g3);
  load_b0<5, kKW / 16>(pk + L::kPW, 5 * (w >> 1), lane, b_w);
  __syncthreads();
  // ---- the input tiles: grid [64][64], window [64][80], x2 [64][K2P] ----------------------------------------------------------------
  for (int idx = tid; idx < 64 * kKG; idx += 256) {
    const int r = idx >> 6, k = idx & 63;
    const size_t at = (size_t)sB[r] * kGrid + k;
    float v = 0.0f;
    if (k < kGrid) v = p.grid_f64 ? (float)reinterpret_cast<const double *>(p.grid)[at] : (float)reinterpret_cast<const int8_t *>(p.grid)[at];
    sG[r * kLdG + k] = v;
  }
  for (int idx = tid; idx < 64 * kKW; idx += 256) {
    const int r = idx / kKW, k = idx - r * kKW;
    const size_t at = ((size_t)sB[r] * N + (sMNA[r] & 255)) * kWin + k;
    float v = 0.0f;
    if (k < kWin) v = p.windows_f64 ? (float)reinterpret_cast<const double *>(p.windows)[at] : (float)reinterpret_cast<const int8_t *>(p.windows)[at];
    sW[r * kLdW + k] = v;
  }
  if constexpr (L::kStage2) {
    for (int idx = tid; idx < 64 * L::K2P; idx += 256) {
      const int r = idx / L::K2P, k = idx - r * L::K2P;
      const size_t base = (size_t)sB[r] * N;
      const int m = sMNA[r] & 255, n = sMNA[r] >> 8;
      float v = 0.0f;
      if constexpr (KIND == kGlobal) {
        if (k < 4 * (N - 1)) {
          const int u = k >> 2;
          v = (float)p.vec[(base + u + (u >= n ? 1 : 0)) * 4 + (k & 3)];
        } else if (k < L::K2) {
          const int u = (k - 4 * (N - 1)) / kA, kk = (k - 4 * (N - 1)) - kA * u;
          v = p.actions[base + u + (u >= n ? 1 : 0)] == kk ? 1.0f : 0.0f;
        }
        (void)m;
      } else {
        if (k < 4) {
          v = (float)p.vec[(base + m) * 4 + k];
        } else if (k < L::K2) {
          const int u = (k >> 2) - 1;
          v = (float)p.vec[(base + u + (u >= n ? 1 : 0)) * 4 + (k & 3)];
        }
      }
      sX2[r * kLdX2 + k] = v;
    }
  }
  __syncthreads();
  // ---- the two convolutions (Toeplitz) into x1, relu; branch2 into registers --------------------------------------------------------
  f32x4 acc_b2[1][2];
  float bias_b2[2] = {0.0f, 0.0f};
  float4 b_1[4];
  {
    if ((w >> 1) == 0) {
      f32x4 acc[2][4];
      float bias[4];
      load_bias<4>(pk + L::kPGB, 0, lane, bias);
      zero_tiles(acc);
      gemm_tiles<2, 4, kKG / 16>(sG, kLdG, 2 * (w & 1), pk + L::kPG, 0, lane, b_g4, acc);
      store_relu<2, 4>(sA, kLd, 2 * (w & 1), 0, bias, lane, acc);
    } else {
      f32x4 acc[2][3];
      float bias[3];
      load_bias<3>(pk + L::kPGB, 4, lane, bias);
      zero_tiles(acc);
      gemm_tiles<2, 3, kKG / 16>(sG, kLdG, 2 * (w & 1), pk + L::kPG, 4, lane, b_g3, acc);
      store_relu<2, 3>(sA, kLd, 2 * (w & 1), 4, bias, lane, acc);
    }
    {
      f32x4 acc[2][5];
      float bias[5];
      load_bias<5>(pk + L::kPWB, 5 * (w >> 1), lane, bias);
      zero_tiles(acc);
      gemm_tiles<2, 5, kKW / 16>(sW, kLdW, 2 * (w & 1), pk + L::kPW, 5 * (w >> 1), lane, b_w, acc);
      store_relu<2, 5>(sA + kNG, kLd, 2 * (w & 1), 5 * (w >> 1), bias, lane, acc);
    }
    zero_tiles(acc_b2);
    if constexpr (L::kStage2) {   // wave w: row tile w, both column tiles
      float4 b_2[2];
      load_b0<2, L::K2P / 16>(pk + L::kP2, 0, lane, b_2);
      load_bias<2>(pk + L::kP2B, 0, lane, bias_b2);
      gemm_tiles<1, 2, L::K2P / 16>(sX2, kLdX2, w, pk + L::kP2, 0, lane, b_2, acc_b2);
    }
    load_b0<4, kK1 / 16>(pk + L::kP1, 4 * w, lane, b_1);
  }
  __syncthreads();   // x1 is complete, nobody reads the input tiles any more: region B becomes the hidden tile
  // ---- branch1: x1 [64][288] -> hidden[:, 0:256], relu; wave w owns columns [64w, 64w + 64) from here on; branch2 -> hidden[:, 256:288]
  float4 b_h[4];
  {
    if constexpr (L::kStage2) store_relu<1, 2>(sBk + kH1, kLd, w, 0, bias_b2, lane, acc_b2);
    f32x4 acc[4][4];
    float bias[4];
    load_bias<4>(pk + L::kP1B, 4 * w, lane, bias);
    zero_tiles(acc);
    gemm_tiles<4, 4, kK1 / 16>(sA, kLd, 0, pk + L::kP1, 4 * w, lane, b_1, acc);
    load_b0<4, L::KH / 16>(pk + L::kPH, 4 * w, lane, b_h);
    store_relu<4, 4>(sBk, kLd, 0, 4 * w, bias, lane, acc);
  }
  __syncthreads();
  // ---- h2 = relu(ONE chain over concat(branch1, branch2)), no bias; into region A (x1 is dead) ---------------------------------------
  float4 b_o[1];
  {
    f32x4 acc[4][4];
    const float bias[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    zero_tiles(acc);
    gemm_tiles<4, 4, L::KH / 16>(sBk, kLd, 0, pk + L::kPH, 4 * w, lane, b_h, acc);
    load_b0<1, kH2 / 16>(pk + L::kPO, 0, lane, b_o);
    store_relu<4, 4>(sA, kLd, 0, 4 * w, bias, lane, acc);
  }
  __syncthreads();
  // ---- out: wave w finishes rows [16w, 16w + 16); column 0 of the tile is Q: lanes 0, 16, 32, 48 hold four rows each ----------------
  f32x4 acc[1][1];
  zero_tiles(acc);
  gemm_tiles<1, 1, kH2 / 16>(sA, kLd, w, pk + L::kPO, 0, lane, b_o, acc);
  if ((lane & 15) == 0) {
    const float bo = pk[L::kPOB];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int lr = 16 * w + 4 * (lane >> 4) + reg;
      const uint32_t hr = row_base + lr;
      if (hr >= rows) continue;
      const float q = acc[0][0][reg] + bo;
      if (p.q) p.q[hr] = q;
      if (p.q64) p.q64[hr] = (double)q;
      if constexpr (FORM != kFormCf) {
        if (p.td) {
          // reward + gamma * q * not_done in the order of k_td_target (batch.hip) on the widened q
          const uint32_t b = sB[lr];
          const size_t bn = (size_t)b * N + (sMNA[lr] >> 8);
          const double rw = p.reward_f64 ? reinterpret_cast<const double *>(p.reward)[bn] : (double)reinterpret_cast<const float *>(p.reward)[bn];
          const double gq = p.gamma * (double)q;
          p.td[hr] = rw + gq * (double)(int64_t)(p.done[b] ? 0 : 1);
        }
      }
    }
  }
}

template <int N, int KIND, int FORM> static int launch(const Params &p, hipStream_t s) {
  const unsigned blocks = (p.n_rows + 63u) / 64u;
  note_variant("k_critic_checkers_rows", (int)sizeof(float), N, 4, 0, 0, 0, 0, 0, 0, /* prec=f32 */ 0);
  note_tail(variant_tail(KIND, FORM));
  hipLaunchKernelGGL((k_critic_checkers_rows<N, KIND, FORM>), dim3(blocks), dim3(256), 0, s, p);
  CM3_HIP_CHECK(hipGetLastError());
  return CM3_OK;
}

template <int N> static int launch_form(int kind, int form, const Params &p, hipStream_t s) {
  return form_dispatch<N>(kind, form, "Checkers critic", [&](auto k, auto f) { return launch<N, k(), f()>(p, s); });
}

template <int N> static int pack_launch(int kind, const PackParams &p, float *out, hipStream_t s) {
  if (kind == kGlobal) {
    hipLaunchKernelGGL((k_critic_checkers_pack<N, kGlobal>), dim3(128), dim3(256), 0, s, p, out);
  } else if constexpr (N > 1) {
    hipLaunchKernelGGL((k_critic_checkers_pack<N, kCredit>), dim3(128), dim3(256), 0, s, p, out);
  }
  CM3_HIP_CHECK(hipGetLastError());
  return CM3_OK;
}

template <typename F> static int agents_1_to_8(int n_agents, F &&f) { return agent_launch<1, 2, 3, 4, 5, 6, 7, 8>(n_agents, f); }

static int check_desc(const cm3_critic_checkers_desc *d) {
  CM3_REQUIRE(d, "null desc");
  CM3_REQUIRE(d->n_agents >= 1 && d->n_agents <= kMaxAgents, "n_agents must be in 1..%d", kMaxAgents);
  const int rc = check_kind_stage(d->kind, d->stage, d->n_agents, "Q_global_checkers", "Q_credit_checkers");
  if (rc != CM3_OK) return rc;
  CM3_REQUIRE(d->grid_h == 3 && d->grid_w == 9 && d->grid_c == 2 && d->win_h == 5 && d->win_w == 5 && d->win_c == 3,
              "supported geometry is a 3x9x2 grid and a 5x5x3 window; got %dx%dx%d and %dx%dx%d", d->grid_h, d->grid_w, d->grid_c,
              d->win_h, d->win_w, d->win_c);
  CM3_REQUIRE(d->n_h1_1 == kH1 && d->n_h1_2 == kH1B && d->n_h2 == kH2,
              "supported Checkers critic widths are 256/32/256 (config_checkers_stage{1,2}.json); got %d/%d/%d", d->n_h1_1, d->n_h1_2,
              d->n_h2);
  return CM3_OK;
}
}  // namespace ck_critic
}  // namespace cm3

extern "C" size_t cm3_critic_checkers_packed_bytes(int32_t n_agents, int32_t kind) {
  using namespace cm3::ck_critic;
  return floats_for<Layout, 1, 2, 3, 4, 5, 6, 7, 8>(n_agents, kind) * sizeof(float);
}

extern "C" int cm3_critic_checkers_pack(const cm3_critic_checkers_desc *d, const cm3_critic_checkers_weights *wt, void *packed,
                                        void *stream) {
  using namespace cm3;
  using namespace cm3::ck_critic;
  int rc = check_desc(d);
  if (rc != CM3_OK) return rc;
  CM3_REQUIRE(wt, "null weights");
  CM3_REQUIRE(packed, "packed is NULL: cm3_critic_checkers_packed_bytes(n_agents, kind) bytes of device memory");
  CM3_REQUIRE(wt->conv_w && wt->conv_b && wt->conv_o_w && wt->conv_o_b,
              "missing weights: conv/Conv/weights, conv/Conv/biases, conv_o/Conv/weights, conv_o/Conv/biases");
  CM3_REQUIRE(wt->w_b1 && wt->b_b1 && wt->w_b1_h2 && wt->w_out && wt->b_out,
              "missing weights: Q_branch1/kernel, Q_branch1/bias, W_branch1_h2, Q_out/kernel, Q_out/bias");
  CM3_REQUIRE(d->stage == 1 || (wt->w_b2 && wt->b_b2 && wt->w_b2_h2),
              "missing stage-2 weights: stage-2/Q_branch2/kernel, stage-2/Q_branch2/bias, stage-2/W_branch2_h2");
  CM3_REQUIRE((uintptr_t)packed % 16 == 0, "misaligned packed: must be 16-byte aligned");
  const PackParams p = {wt->conv_w, wt->conv_b, wt->conv_o_w, wt->conv_o_b, wt->w_b1, wt->b_b1, wt->w_b1_h2,
                        wt->w_b2,   wt->b_b2,   wt->w_b2_h2,  wt->w_out,    wt->b_out};
  hipStream_t s = (hipStream_t)stream;
  const int kind = d->kind;
  return agents_1_to_8(d->n_agents, [&](auto n) { return pack_launch<n()>(kind, p, (float *)packed, s); });
}

extern "C" int cm3_critic_checkers_rows_f32(const cm3_critic_checkers_desc *d, const cm3_critic_checkers_weights *wt,
                                            const cm3_critic_checkers_rows *r, void *stream) {
  using namespace cm3;
  using namespace cm3::ck_critic;
  int rc = check_desc(d);
  if (rc != CM3_OK) return rc;
  CM3_REQUIRE(wt, "null weights");
  CM3_REQUIRE(r, "null rows");
  CM3_REQUIRE(wt->packed, "packed weights are NULL: run cm3_critic_checkers_pack once per weight update");
  const int N = d->n_agents;
  uint32_t n_rows;
  rc = check_rows(r, wt->packed, d->kind, N, "Q_global_checkers", "Q_credit_checkers",
                  r->grid && r->vec && r->goals && r->windows && r->obs_self_v,
                  "missing inputs: grid, vec, goals, windows and obs_self_v are required",
                  (uintptr_t)r->vec % 8 == 0 && (uintptr_t)r->obs_self_v % 8 == 0 && (uintptr_t)r->actions % 4 == 0 &&
                      (!r->grid_f64 || (uintptr_t)r->grid % 8 == 0) && (!r->windows_f64 || (uintptr_t)r->windows % 8 == 0) &&
                      (!r->goals_onehot || (uintptr_t)r->goals % 8 == 0),
                  "misaligned inputs: vec, obs_self_v, float64 grids / windows and one-hot goals must be 8-byte aligned, actions 4-byte "
                  "aligned", n_rows);
  if (rc != CM3_OK) return rc;
  Params p;
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
  p.windows = r->windows;
  p.obs_self_v = r->obs_self_v;
  p.reward = r->reward;
  p.done = r->done;
  p.gamma = r->gamma;
  p.q = r->q;
  p.q64 = r->q64;
  p.td = r->td;
  p.packed = (const float *)wt->packed;
  hipStream_t s = (hipStream_t)stream;
  const int kind = d->kind, form = r->form;
  return agents_1_to_8(N, [&](auto n) { return launch_form<n()>(kind, form, p, s); });
}
