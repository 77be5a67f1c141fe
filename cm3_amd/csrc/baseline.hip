// The IAC / COMA baseline critics over TRANSITION rows (part of ABI 9, additive): the value networks networks.V_particle_local
// (networks.py:356-374, IAC) and networks.V_particle_global (:377-402), and the COMA critic networks.Q_global (:84-94) -- the
// evaluations of alg_baseline.train_step that carry no gradient (V_target / V on the next-step columns :534, Q_target :576, Q :616).
// No kernel takes a tiled feed: a lane decodes (b, n) from its row number r = b N + n (critic_rows::decode, form ROWS) and gathers
// its inputs from the batch's base columns; "others" run over the agents j != n in ascending order.
//
// ---- the value networks (k_value_particle_rows) --------------------------------------------------------------------------------
//   branch1 = relu(x1 . [6][64] + b)        local:  x1 = concat(v_obs[4], goal[2])      global: x1 = concat(state_n[4], goal_n[2])
//   branch2 = relu(x2 . [K2][128] + b)      local:  x2 = obs_others, K2 = 4(N-1)        global: x2 = concat(state of the others
//     (stage 2 = N > 1 only)                                                              [4(N-1)], goals of the others [2(N-1)]), K2 = 6(N-1)
//   h2  = relu(branch1 . [64][64] + branch2 . [128][64])   (no bias)                    out = h2 . [64][1]   (no bias)
// The body is that of k_critic_particle_rows (critic.hip) at K1 = 6, stated here: lifted into a shared header it moved the register
// counts of 13 of the 29 critic kernels (VGPRs by up to 5, SGPRs by up to 2), so critic.hip stays as it is.
// 256 threads = 4 waves own 64 rows; every layer on the exact-f32 matrix instruction (v_mfma_f32_16x16x4_f32, a k-ordered fmaf
// chain), so a row's bits depend on neither its place in the workgroup nor the launch's row count.
//   branch1 (K = 6 -> 8): transposed, C[unit][row]; wave w owns units [16w, 16w+16) of all 64 rows.
//   branch2 (K2 -> whole k-steps, up to 54 -> 56): transposed; wave w owns units [32w, 32w+32) as two 16-unit slices.
//   h2 (192 -> 64, ONE chain over concat(branch1, branch2)): wave w owns columns [16w, 16w+16).
//   out (64 -> 1): one 16 x 16 tile per wave, only output row 0 carries weights; lane l < 16 of wave w finishes row 16w + l.
// LDS: hidden [64][194] + inputs [64][9] + [64][K2P + 1]; h2 [64][66] reuses the input tiles.  N = 10 global: 66 560 bytes, two
// workgroups per CU; 64 rows per workgroup.
//
// ---- the COMA critic (k_coma_particle_rows) ------------------------------------------------------------------------------------
//   x = concat(state of all agents [4N], one-hot actions of the others [5(N-1)], goal_n [2], goals of the others [2(N-1)],
//              one-hot label of n [N], v_obs_n [4]),  K = 12N - 1 (23 .. 119)
//   h1 = relu(x . [K][256] + b)     h2 = relu(h1 . [256][256] + b)     q = h2 . [256][5] + b
// 256 threads = 4 waves own 64 rows.  All three layers transposed, C[unit][row], the weights the A operand and the bias the start
// value of the chain: in h1 and h2 wave w owns units [64w, 64w+64) of all 64 rows as four 16-unit slices (per slice: the lane's
// K / 4 weights in registers, four independent chains, one per 16-row tile); the output layer is ONE 16-unit tile (units 5..15 carry
// zero weights and are not stored), wave w finishing rows [16w, 16w+16).  256 -> 256 is 90 % (N = 2) .. 67 % (N = 10) of the FLOPs.
// LDS: h1 [64][258] + h2 [64][258]; the input tile [64][KP + 2] lies under h2 and is dead (a barrier) before h2 is written -- with a
// tile of its own the three would take 163 840 + bytes at N = 10.  132 096 bytes at every N: ONE workgroup of 64 rows per CU (32
// rows per workgroup would fit two, and read the 256 KiB of h2 weights twice as often).  Row strides = 2 mod 32 dwords: the 32
// lanes of a ds_read_b32 group (16 rows x 2 k) fall on 32 banks.  Plain launch bounds, not CM3_MATRIX_KERNEL: with one workgroup per
// CU its declared two waves per SIMD cannot be met; the compiler keeps the 16 accumulator registers in AGPRs (35 VGPRs, no scratch).
#include "critic_rows.h"

namespace cm3 {

using critic_rows::decode;
using critic_rows::kFormRows;
constexpr int kValueLocal = CM3_VALUE_LOCAL, kValueGlobal = CM3_VALUE_GLOBAL;
constexpr int kVH1 = 64, kVH2B = 128, kVH2 = 64;     // branch self / 1, V_n_others, V_n_h2 (config.json nn block)
constexpr int kQU = 256;                              // Q_units

// ================================================================================================================================
// the value networks
// ================================================================================================================================
template <int N, int KIND> struct ValueLayout {
  static constexpr bool kStage2 = N > 1;
  static constexpr int K1 = 6, S1 = 2, S1P = 4;
  static constexpr int K2 = !kStage2 ? 0 : (KIND == kValueLocal ? 4 * (N - 1) : 6 * (N - 1));
  static constexpr int K2P = (K2 + 3) / 4 * 4;
  static constexpr int S2 = K2P / 4;                          // branch-2 k-steps (up to 14)
  static constexpr int S2P = (S2 + 3) / 4 * 4;                // per-lane stride of the branch-2 operands (16-byte loads)
  static constexpr int HW = kStage2 ? kVH1 + kVH2B : kVH1;    // width of concat(branch1, branch2)
  static constexpr int SH = HW / 4;                           // k-steps of the h2 layer (48 / 16)
  static constexpr int HS = HW + 2, X1W = 9, X2W = K2P + 1, H2S = kVH2 + 2;     // LDS row strides
  static constexpr int kIn = 64 * X1W + (kStage2 ? 64 * X2W : 0);
  static constexpr int kLdsFloats = 64 * HS + (kIn > 64 * H2S ? kIn : 64 * H2S);
  // packed weights (floats)
  static constexpr int kW1 = 0;                               // [4 waves][64 lanes][S1P]      A operands of branch 1
  static constexpr int kB1 = kW1 + 4 * 64 * S1P;              // [64]
  static constexpr int kW2 = kB1 + kVH1;                      // [4 waves][2][64 lanes][S2P]   A operands of branch 2
  static constexpr int kB2 = kW2 + 4 * 2 * 64 * S2P;          // [128]
  static constexpr int kWh = kB2 + (kStage2 ? kVH2B : 0);     // [4 waves][64 lanes][SH]       B operands of h2
  static constexpr int kWo = kWh + 4 * 64 * SH;               // [64 lanes][16]                A operands of out (row 0 only)
  static constexpr int kTotal = kWo + 64 * 16;
};

struct ValuePackParams {
  const float *w_b1, *b_b1, *w_b1_h2, *w_b2, *b_b2, *w_b2_h2, *w_out;
};

template <int N, int KIND> __global__ void __launch_bounds__(256) k_value_pack(const ValuePackParams p, float *out) {
  using CL = ValueLayout<N, KIND>;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < CL::kTotal; t += gridDim.x * 256) {
    float v = 0.0f;
    if (t < CL::kB1) {
      const int s = t % CL::S1P, lane = (t / CL::S1P) & 63, w = t / CL::S1P / 64;
      const int k = 4 * s + (lane >> 4), j = 16 * w + (lane & 15);
      v = (s < CL::S1 && k < CL::K1) ? p.w_b1[k * kVH1 + j] : 0.0f;
    } else if (t < CL::kW2) {
      v = p.b_b1[t - CL::kB1];
    } else if (t < CL::kB2) {
      if constexpr (CL::kStage2) {
        const int u = t - CL::kW2, s = u % CL::S2P, lane = (u / CL::S2P) & 63, c = (u / CL::S2P / 64) & 1, w = u / CL::S2P / 128;
        const int k = 4 * s + (lane >> 4), j = 32 * w + 16 * c + (lane & 15);
        v = (s < CL::S2 && k < CL::K2) ? p.w_b2[k * kVH2B + j] : 0.0f;
      }
    } else if (t < CL::kWh) {
      if constexpr (CL::kStage2) v = p.b_b2[t - CL::kB2];
    } else if (t < CL::kWo) {
      const int u = t - CL::kWh, s = u % CL::SH, lane = (u / CL::SH) & 63, w = u / CL::SH / 64;
      const int k = 4 * s + (lane >> 4), j = 16 * w + (lane & 15);
      if (k < kVH1) {
        v = p.w_b1_h2[k * kVH2 + j];
      } else {
        if constexpr (CL::kStage2) v = p.w_b2_h2[(k - kVH1) * kVH2 + j];
      }
    } else {
      const int u = t - CL::kWo, s = u & 15, lane = u >> 4;
      v = (lane & 15) == 0 ? p.w_out[4 * s + (lane >> 4)] : 0.0f;
    }
    out[t] = v;
  }
}

struct ValueParams {
  uint32_t n_rows;
  const float *state, *obs_others, *goals;     // [B][N][4] (local: v_obs), [B][N][4(N-1)] (local), [B][N][2]
  const void *reward;                          // [B][N] float32 / float64 (td)
  int reward_f64;
  const uint8_t *done;                         // [B] (td)
  double gamma;
  float *v;                                    // optional [n_rows]
  double *v64, *td;                            // optional [n_rows]
  const float *packed;
};

template <int N, int KIND> __global__ void CM3_MATRIX_KERNEL k_value_particle_rows(const ValueParams p) {
  using CL = ValueLayout<N, KIND>;
  static_assert(CL::kLdsFloats * 4 <= 80 * 1024, "two workgroups per CU");
  __shared__ __attribute__((aligned(16))) float smem[CL::kLdsFloats];
  float(*hs)[CL::HS] = reinterpret_cast<float(*)[CL::HS]>(smem);
  float(*x1)[CL::X1W] = reinterpret_cast<float(*)[CL::X1W]>(smem + 64 * CL::HS);
  float(*x2)[CL::X2W] = reinterpret_cast<float(*)[CL::X2W]>(smem + 64 * CL::HS + 64 * CL::X1W);
  float(*h2s)[CL::H2S] = reinterpret_cast<float(*)[CL::H2S]>(smem + 64 * CL::HS);     // over x1 / x2, dead by then
  const int tid = threadIdx.x, lane = tid & 63, col = lane & 15, hi = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t rows = p.n_rows;
  const uint32_t row_base = blockIdx.x * 64u;

  // ---- staging: lane = row (a lane past the count reads the last row's inputs); wave 0 the branch-1 tile, the 4-float / 2-float
  // pieces of the branch-2 tile dealt round the waves ----
  {
    const uint32_t r = row_base + lane;
    uint32_t b;
    int m, n, a;
    decode<N, kFormRows>(r < rows ? r : rows - 1, b, m, n, a);
    const uint32_t base = b * (uint32_t)N;
    if (w == 0) {
      const float4 s = reinterpret_cast<const float4 *>(p.state)[base + n];
      const float2 g = reinterpret_cast<const float2 *>(p.goals)[base + n];
      x1[lane][0] = s.x; x1[lane][1] = s.y; x1[lane][2] = s.z; x1[lane][3] = s.w;
      x1[lane][4] = g.x; x1[lane][5] = g.y;
      x1[lane][6] = 0.0f; x1[lane][7] = 0.0f;
      if constexpr (CL::kStage2) {
#pragma unroll
        for (int k = CL::K2; k < CL::K2P; ++k) x2[lane][k] = 0.0f;
      }
    }
    if constexpr (CL::kStage2) {
      constexpr int kPieces = KIND == kValueLocal ? N - 1 : 2 * (N - 1);
      for (int u = w; u < kPieces; u += 4) {      // (u is wave-uniform)
        if (u < N - 1) {
          float4 s;
          if constexpr (KIND == kValueLocal) {
            s = reinterpret_cast<const float4 *>(p.obs_others)[(size_t)(base + n) * (N - 1) + u];
          } else {
            s = reinterpret_cast<const float4 *>(p.state)[base + u + (u >= n ? 1 : 0)];
          }
          x2[lane][4 * u + 0] = s.x; x2[lane][4 * u + 1] = s.y; x2[lane][4 * u + 2] = s.z; x2[lane][4 * u + 3] = s.w;
        } else {
          const int v = u - (N - 1);
          const float2 g = reinterpret_cast<const float2 *>(p.goals)[base + v + (v >= n ? 1 : 0)];
          x2[lane][4 * (N - 1) + 2 * v + 0] = g.x; x2[lane][4 * (N - 1) + 2 * v + 1] = g.y;
        }
      }
    }
  }
  __syncthreads();
  // ---- branch 1: units [16w, 16w+16) of all 64 rows, C[unit][row], bias as the start value ----------------------------------------
  {
    const float4 a1 = reinterpret_cast<const float4 *>(p.packed + CL::kW1)[w * 64 + lane];
    const float4 b1 = reinterpret_cast<const float4 *>(p.packed + CL::kB1)[4 * w + hi];
    const float a1s[2] = {a1.x, a1.y};
    f32x4 c[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) c[t] = f32x4{b1.x, b1.y, b1.z, b1.w};
#pragma unroll
    for (int s = 0; s < CL::S1; ++s)
#pragma unroll
      for (int t = 0; t < 4; ++t) c[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1s[s], x1[16 * t + col][4 * s + hi], c[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      *reinterpret_cast<float2 *>(&hs[16 * t + col][16 * w + 4 * hi]) = make_float2(relu_f32(c[t][0]), relu_f32(c[t][1]));
      *reinterpret_cast<float2 *>(&hs[16 * t + col][16 * w + 4 * hi + 2]) = make_float2(relu_f32(c[t][2]), relu_f32(c[t][3]));
    }
  }
  // ---- branch 2: units [32w, 32w+32) as two slices, the same form ----------------------------------------------------------------
  if constexpr (CL::kStage2) {
#pragma unroll
    for (int cs = 0; cs < 2; ++cs) {
      float a2[CL::S2P];
      const float4 *src = reinterpret_cast<const float4 *>(p.packed + CL::kW2) + (size_t)((w * 2 + cs) * 64 + lane) * (CL::S2P / 4);
#pragma unroll
      for (int s4 = 0; s4 < CL::S2P / 4; ++s4) {
        const float4 v = src[s4];
        a2[4 * s4 + 0] = v.x; a2[4 * s4 + 1] = v.y; a2[4 * s4 + 2] = v.z; a2[4 * s4 + 3] = v.w;
      }
      const float4 b2 = reinterpret_cast<const float4 *>(p.packed + CL::kB2)[8 * w + 4 * cs + hi];
      f32x4 c[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) c[t] = f32x4{b2.x, b2.y, b2.z, b2.w};
#pragma unroll
      for (int s = 0; s < CL::S2; ++s)
#pragma unroll
        for (int t = 0; t < 4; ++t) c[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[s], x2[16 * t + col][4 * s + hi], c[t], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        float *dst = &hs[16 * t + col][kVH1 + 32 * w + 16 * cs + 4 * hi];
        *reinterpret_cast<float2 *>(dst) = make_float2(relu_f32(c[t][0]), relu_f32(c[t][1]));
        *reinterpret_cast<float2 *>(dst + 2) = make_float2(relu_f32(c[t][2]), relu_f32(c[t][3]));
      }
    }
  }
  __syncthreads();
  // ---- h2: columns [16w, 16w+16), C[row][unit], one chain over concat(branch1, branch2) ------------------------------------------
  {
    float bw[CL::SH];
    const float4 *src = reinterpret_cast<const float4 *>(p.packed + CL::kWh) + (size_t)(w * 64 + lane) * (CL::SH / 4);
#pragma unroll
    for (int s4 = 0; s4 < CL::SH / 4; ++s4) {
      const float4 v = src[s4];
      bw[4 * s4 + 0] = v.x; bw[4 * s4 + 1] = v.y; bw[4 * s4 + 2] = v.z; bw[4 * s4 + 3] = v.w;
    }
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int s = 0; s < CL::SH; ++s)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(hs[16 * t + col][4 * s + hi], bw[s], acc[t], 0, 0, 0);
    // (h2s lies over the input tiles: every wave is past the barrier above, nobody reads them any more)
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) h2s[16 * t + 4 * hi + reg][16 * w + col] = relu_f32(acc[t][reg]);
  }
  __syncthreads();
  // ---- out: C[.][row] of rows [16w, 16w+16); output row 0 is V, in register 0 of lanes 0..15 -------------------------------------
  float wo[16];
  {
    const float4 *so = reinterpret_cast<const float4 *>(p.packed + CL::kWo) + (size_t)lane * 4;
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
      const float4 u = so[s4];
      wo[4 * s4 + 0] = u.x; wo[4 * s4 + 1] = u.y; wo[4 * s4 + 2] = u.z; wo[4 * s4 + 3] = u.w;
    }
  }
  f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int s = 0; s < kVH2 / 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wo[s], h2s[16 * w + col][4 * s + hi], acc, 0, 0, 0);
  const float v = acc[0];
  const uint32_t hr = row_base + 16 * w + col;
  if (hi == 0 && hr < rows) {
    if (p.v) p.v[hr] = v;
    if (p.v64) p.v64[hr] = (double)v;
    if (p.td) {
      // reward_local + gamma * v * not_done in the order of k_td_target (batch.hip) on the widened v; hr = b N + n indexes [B][N]
      const uint32_t b = hr / (uint32_t)N;
      const double rw = p.reward_f64 ? reinterpret_cast<const double *>(p.reward)[hr] : (double)reinterpret_cast<const float *>(p.reward)[hr];
      const double gv = p.gamma * (double)v;
      p.td[hr] = rw + gv * (double)(int64_t)(p.done[b] ? 0 : 1);
    }
  }
}

template <int N, int KIND> static int value_launch(const ValueParams &p, hipStream_t s) {
  const unsigned blocks = (p.n_rows + 63u) / 64u;
  note_variant("k_value_particle_rows", (int)sizeof(float), N, 4, 0, 0, 0, 0, 0, 0, /* prec=f32 */ 0);
  note_tail(KIND == kValueLocal ? ",kind=local" : ",kind=global");
  hipLaunchKernelGGL((k_value_particle_rows<N, KIND>), dim3(blocks), dim3(256), 0, s, p);
  CM3_HIP_CHECK(hipGetLastError());
  return CM3_OK;
}

template <int N, int KIND> static int value_pack_launch(const ValuePackParams &p, float *out, hipStream_t s) {
  hipLaunchKernelGGL((k_value_pack<N, KIND>), dim3(32), dim3(256), 0, s, p, out);
  CM3_HIP_CHECK(hipGetLastError());
  return CM3_OK;
}

static size_t value_floats_for(int n, int kind) {
  bool hit;
  return agent_dispatch_1_to_10(n, hit, [&](auto k) {
    constexpr int N = k();
    if (kind == kValueLocal) return (size_t)ValueLayout<N, kValueLocal>::kTotal;
    if (kind == kValueGlobal) return (size_t)ValueLayout<N, kValueGlobal>::kTotal;
    return (size_t)0;
  });
}

static int value_check_desc(const cm3_value_particle_desc *d) {
  CM3_REQUIRE(d, "null desc");
  CM3_REQUIRE(d->n_agents >= 1 && d->n_agents <= CM3_MAX_AGENTS, "n_agents must be in 1..%d", CM3_MAX_AGENTS);
  CM3_REQUIRE(d->kind == kValueLocal || d->kind == kValueGlobal, "kind must be CM3_VALUE_LOCAL (0) or CM3_VALUE_GLOBAL (1), got %d", d->kind);
  CM3_REQUIRE(d->stage == 1 || d->stage == 2, "stage must be 1 or 2, got %d", d->stage);
  CM3_REQUIRE((d->stage == 1) == (d->n_agents == 1), "%s runs at stage 1 with one agent and at stage 2 with more (n_agents %d, stage %d)",
              d->kind == kValueLocal ? "V_particle_local" : "V_particle_global", d->n_agents, d->stage);
  CM3_REQUIRE(d->n_h1 == kVH1 && d->n_others == kVH2B && d->n_h2 == kVH2,
              "supported value-network widths are 64/128/64 (config.json nn block); got %d/%d/%d", d->n_h1, d->n_others, d->n_h2);
  return CM3_OK;
}

// ================================================================================================================================
// the COMA critic
// ================================================================================================================================
template <int N> struct ComaLayout {
  static_assert(N >= 2, "Q_global exists with more than one agent only");
  static constexpr int K = 12 * N - 1;
  static constexpr int KP = (K + 3) / 4 * 4;
  static constexpr int S0 = KP / 4;                           // h1 k-steps (6 .. 30)
  static constexpr int S0P = (S0 + 3) / 4 * 4;                // per-lane stride of the h1 operands (16-byte loads)
  static constexpr int SU = kQU / 4;                          // k-steps of h2 and out (64)
  static constexpr int HS = kQU + 2, XW = KP + 2;             // LDS row strides (= 2 mod 4 dwords; HS = 2 mod 32)
  static constexpr int kLdsFloats = 2 * 64 * HS;              // h1 | h2, the input tile under h2
  static_assert(XW <= HS, "the input tile lies under h2");
  // offsets of the input's parts
  static constexpr int oAct = 4 * N, oGoal = oAct + kA * (N - 1), oGoalOthers = oGoal + 2, oLabel = oGoalOthers + 2 * (N - 1),
                       oObs = oLabel + N;
  static_assert(oObs + 4 == K, "K = 12 N - 1");
  // packed weights (floats)
  static constexpr int kW1 = 0;                               // [4 waves][4 slices][64 lanes][S0P]   A operands of h1
  static constexpr int kB1 = kW1 + 16 * 64 * S0P;             // [256]
  static constexpr int kW2 = kB1 + kQU;                       // [4 waves][4 slices][64 lanes][64]    A operands of h2
  static constexpr int kB2 = kW2 + 16 * 64 * SU;              // [256]
  static constexpr int kWo = kB2 + kQU;                       // [64 lanes][64]                       A operands of out (units 0..4)
  static constexpr int kBo = kWo + 64 * SU;                   // [16]                                 (5 biases, zeros)
  static constexpr int kTotal = kBo + 16;
};

struct ComaPackParams {
  const float *w_h1, *b_h1, *w_h2, *b_h2, *w_out, *b_out;
};

template <int N> __global__ void __launch_bounds__(256) k_coma_pack(const ComaPackParams p, float *out) {
  using CL = ComaLayout<N>;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < CL::kTotal; t += gridDim.x * 256) {
    float v = 0.0f;
    if (t < CL::kB1) {
      const int s = t % CL::S0P, lane = (t / CL::S0P) & 63, slice = t / CL::S0P / 64;      // slice = 4 w + c
      const int k = 4 * s + (lane >> 4), j = 16 * slice + (lane & 15);
      v = (s < CL::S0 && k < CL::K) ? p.w_h1[k * kQU + j] : 0.0f;
    } else if (t < CL::kW2) {
      v = p.b_h1[t - CL::kB1];
    } else if (t < CL::kB2) {
      const int u = t - CL::kW2, s = u % CL::SU, lane = (u / CL::SU) & 63, slice = u / CL::SU / 64;
      const int k = 4 * s + (lane >> 4), j = 16 * slice + (lane & 15);
      v = p.w_h2[k * kQU + j];
    } else if (t < CL::kWo) {
      v = p.b_h2[t - CL::kB2];
    } else if (t < CL::kBo) {
      const int u = t - CL::kWo, s = u % CL::SU, lane = u / CL::SU;
      const int k = 4 * s + (lane >> 4), j = lane & 15;
      v = j < kA ? p.w_out[k * kA + j] : 0.0f;
    } else {
      const int j = t - CL::kBo;
      v = j < kA ? p.b_out[j] : 0.0f;
    }
    out[t] = v;
  }
}

struct ComaParams {
  uint32_t n_rows;
  const float *state, *goals, *v_obs;     // [B][N][4], [B][N][2], [B][N][4]
  const int32_t *actions;                 // [B][N]: the others' one-hot actions
  const int32_t *own_actions;             // optional [B][N]: the row's own action (q_taken, q_taken64, td)
  const void *reward;                     // [B] float32 / float64 (td): the GLOBAL reward
  int reward_f64;
  const uint8_t *done;                    // [B] (td)
  double gamma;
  float *q;                               // optional [n_rows][5]
  float *q_taken;                         // optional [n_rows]
  double *q_taken64, *td;                 // optional [n_rows]
  const float *packed;
};

// one hidden layer of the COMA critic: units [64w, 64w+64) of all 64 rows as four 16-unit slices, C[unit][row], the bias as the
// start value; S k-steps over the rows of `in` (stride IS), relu into `out` (stride OS).  wt: this layer's A operands, bias: its 256
template <int S, int SP, int IS, int OS>
__device__ __forceinline__ void coma_hidden_layer(const float *wt, const float *bias, const float *in, float *out, int w, int lane) {
  const int col = lane & 15, hi = lane >> 4;
#pragma unroll 1
  for (int cs = 0; cs < 4; ++cs) {
    float a[SP];
    const float4 *src = reinterpret_cast<const float4 *>(wt) + (size_t)((w * 4 + cs) * 64 + lane) * (SP / 4);
#pragma unroll
    for (int s4 = 0; s4 < SP / 4; ++s4) {
      const float4 v = src[s4];
      a[4 * s4 + 0] = v.x; a[4 * s4 + 1] = v.y; a[4 * s4 + 2] = v.z; a[4 * s4 + 3] = v.w;
    }
    const float4 b = reinterpret_cast<const float4 *>(bias)[16 * w + 4 * cs + hi];
    f32x4 c[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) c[t] = f32x4{b.x, b.y, b.z, b.w};
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int t = 0; t < 4; ++t) c[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], in[(16 * t + col) * IS + 4 * s + hi], c[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      float *dst = out + (16 * t + col) * OS + 64 * w + 16 * cs + 4 * hi;
      *reinterpret_cast<float2 *>(dst) = make_float2(relu_f32(c[t][0]), relu_f32(c[t][1]));
      *reinterpret_cast<float2 *>(dst + 2) = make_float2(relu_f32(c[t][2]), relu_f32(c[t][3]));
    }
  }
}

template <int N> __global__ void __launch_bounds__(256) k_coma_particle_rows(const ComaParams p) {
  using CL = ComaLayout<N>;
  static_assert(CL::kLdsFloats * 4 <= 160 * 1024, "one workgroup per CU");
  __shared__ __attribute__((aligned(16))) float smem[CL::kLdsFloats];
  float *h1s = smem;                      // [64][HS]
  float *h2s = smem + 64 * CL::HS;        // [64][HS]
  float *xs = h2s;                        // [64][XW], dead before h2 is written
  const int tid = threadIdx.x, lane = tid & 63, col = lane & 15, hi = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t rows = p.n_rows;
  const uint32_t row_base = blockIdx.x * 64u;

  // ---- staging: lane = row (a lane past the count reads the last row's inputs); the 3 N + 1 pieces dealt round the waves:
  // N states, N - 1 one-hot actions, N goals (own first), the label, v_obs with the padding ----
  {
    const uint32_t r = row_base + lane;
    uint32_t b;
    int m, n, a;
    decode<N, kFormRows>(r < rows ? r : rows - 1, b, m, n, a);
    const uint32_t base = b * (uint32_t)N;
    float *x = xs + lane * CL::XW;
    for (int u = w; u < 3 * N + 1; u += 4) {      // (u is wave-uniform)
      if (u < N) {
        const float4 s = reinterpret_cast<const float4 *>(p.state)[base + u];
        x[4 * u + 0] = s.x; x[4 * u + 1] = s.y; x[4 * u + 2] = s.z; x[4 * u + 3] = s.w;
      } else if (u < 2 * N - 1) {
        const int v = u - N;
        const int act = p.actions[base + v + (v >= n ? 1 : 0)];
#pragma unroll
        for (int k = 0; k < kA; ++k) x[CL::oAct + kA * v + k] = act == k ? 1.0f : 0.0f;
      } else if (u < 3 * N - 1) {
        const int v = u - (2 * N - 1);            // 0: the row's own goal; v >= 1: the goal of the (v - 1)th other agent
        const int j = v == 0 ? n : (v - 1) + (v - 1 >= n ? 1 : 0);
        const float2 g = reinterpret_cast<const float2 *>(p.goals)[base + j];
        x[CL::oGoal + 2 * v + 0] = g.x; x[CL::oGoal + 2 * v + 1] = g.y;
      } else if (u == 3 * N - 1) {
#pragma unroll
        for (int k = 0; k < N; ++k) x[CL::oLabel + k] = n == k ? 1.0f : 0.0f;
      } else {
        const float4 s = reinterpret_cast<const float4 *>(p.v_obs)[base + n];
        x[CL::oObs + 0] = s.x; x[CL::oObs + 1] = s.y; x[CL::oObs + 2] = s.z; x[CL::oObs + 3] = s.w;
#pragma unroll
        for (int k = CL::K; k < CL::KP; ++k) x[k] = 0.0f;
      }
    }
  }
  __syncthreads();
  coma_hidden_layer<CL::S0, CL::S0P, CL::XW, CL::HS>(p.packed + CL::kW1, p.packed + CL::kB1, xs, h1s, w, lane);
  __syncthreads();      // (h2s lies over the input tile: every wave is past this barrier, nobody reads the inputs any more)
  coma_hidden_layer<CL::SU, CL::SU, CL::HS, CL::HS>(p.packed + CL::kW2, p.packed + CL::kB2, h1s, h2s, w, lane);
  __syncthreads();
  // ---- out: C[unit][row] of rows [16w, 16w+16), one chain of 64 k-steps; the lane (col, hi) ends with units 4 hi .. 4 hi + 3 of
  // row 16w + col: units 0..3 in the lanes with hi == 0, unit 4 in register 0 of those with hi == 1 --------------------------------
  f32x4 c;
  {
    float a[CL::SU];
    const float4 *src = reinterpret_cast<const float4 *>(p.packed + CL::kWo) + (size_t)lane * (CL::SU / 4);
#pragma unroll
    for (int s4 = 0; s4 < CL::SU / 4; ++s4) {
      const float4 v = src[s4];
      a[4 * s4 + 0] = v.x; a[4 * s4 + 1] = v.y; a[4 * s4 + 2] = v.z; a[4 * s4 + 3] = v.w;
    }
    const float4 bo = reinterpret_cast<const float4 *>(p.packed + CL::kBo)[hi];
    c = f32x4{bo.x, bo.y, bo.z, bo.w};
#pragma unroll
    for (int s = 0; s < CL::SU; ++s) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], h2s[(16 * w + col) * CL::HS + 4 * s + hi], c, 0, 0, 0);
  }
  const uint32_t hr = row_base + 16 * w + col;
  if (hi < 2 && hr < rows) {
    if (p.q) {
      float *q = p.q + (size_t)hr * kA;
      if (hi == 0) {
        q[0] = c[0]; q[1] = c[1]; q[2] = c[2]; q[3] = c[3];
      } else {
        q[4] = c[0];
      }
    }
    if (p.own_actions) {
      // q[r][actions[b][n]] (hr = b N + n indexes [B][N]): the lane that holds that unit finishes the row
      const int act = p.own_actions[hr];
      const bool mine = hi == 0 ? (act >= 0 && act < 4) : act == 4;
      if (mine) {
        const float qt = hi == 1 ? c[0] : (act == 0 ? c[0] : (act == 1 ? c[1] : (act == 2 ? c[2] : c[3])));
        if (p.q_taken) p.q_taken[hr] = qt;
        if (p.q_taken64) p.q_taken64[hr] = (double)qt;
        if (p.td) {
          // reward + gamma * q_taken * not_done in the order of k_td_target (batch.hip) on the widened value; the GLOBAL reward [B]
          const uint32_t b = hr / (uint32_t)N;
          const double rw = p.reward_f64 ? reinterpret_cast<const double *>(p.reward)[b] : (double)reinterpret_cast<const float *>(p.reward)[b];
          const double gq = p.gamma * (double)qt;
          p.td[hr] = rw + gq * (double)(int64_t)(p.done[b] ? 0 : 1);
        }
      }
    }
  }
}

template <int N> static int coma_launch(const ComaParams &p, hipStream_t s) {
  if constexpr (N >= 2) {
    const unsigned blocks = (p.n_rows + 63u) / 64u;
    note_variant("k_coma_particle_rows", (int)sizeof(float), N, 4, 0, 0, 0, 0, 0, 0, /* prec=f32 */ 0);
    hipLaunchKernelGGL((k_coma_particle_rows<N>), dim3(blocks), dim3(256), 0, s, p);
    CM3_HIP_CHECK(hipGetLastError());
    return CM3_OK;
  } else {
    return fail(CM3_ERR_INVALID, "n_agents %d unsupported", N);
  }
}

template <int N> static int coma_pack_launch(const ComaPackParams &p, float *out, hipStream_t s) {
  if constexpr (N >= 2) {
    hipLaunchKernelGGL((k_coma_pack<N>), dim3(64), dim3(256), 0, s, p, out);
    CM3_HIP_CHECK(hipGetLastError());
    return CM3_OK;
  } else {
    return fail(CM3_ERR_INVALID, "n_agents %d unsupported", N);
  }
}

static size_t coma_floats_for(int n) {
  bool hit;
  return agent_dispatch<2, 3, 4, 5, 6, 7, 8, 9, 10>(n, hit, [&](auto k) { return (size_t)ComaLayout<k()>::kTotal; });
}

static int coma_check_desc(const cm3_coma_particle_desc *d) {
  CM3_REQUIRE(d, "null desc");
  CM3_REQUIRE(d->n_agents >= 2 && d->n_agents <= CM3_MAX_AGENTS, "n_agents must be in 2..%d: Q_global exists with more than one agent only",
              CM3_MAX_AGENTS);
  CM3_REQUIRE(d->units == kQU, "the supported COMA critic width is 256 (config.json nn block, Q_units); got %d", d->units);
  return CM3_OK;
}

// the row count of n_steps time steps of N agents, behind the checks on it (the order of critic_rows::check_rows)
static int baseline_row_count(int64_t n_steps, int N, uint32_t &n_rows) {
  CM3_REQUIRE(n_steps > 0, "n_steps must be positive");
  CM3_REQUIRE(n_steps <= (int64_t)0x7fffffff / N, "n_steps %lld gives more than 2^31 - 1 rows (%lld per time step)", (long long)n_steps,
              (long long)N);
  n_rows = (uint32_t)(n_steps * N);
  return CM3_OK;
}
}  // namespace cm3

extern "C" size_t cm3_value_particle_packed_bytes(int32_t n_agents, int32_t kind) {
  return cm3::value_floats_for(n_agents, kind) * sizeof(float);
}

extern "C" int cm3_value_particle_pack(const cm3_value_particle_desc *d, const cm3_value_particle_weights *wt, void *packed, void *stream) {
  using namespace cm3;
  int rc = value_check_desc(d);
  if (rc != CM3_OK) return rc;
  CM3_REQUIRE(wt, "null weights");
  CM3_REQUIRE(packed, "packed is NULL: cm3_value_particle_packed_bytes(n_agents, kind) bytes of device memory");
  CM3_REQUIRE(wt->w_b1 && wt->b_b1 && wt->w_b1_h2 && wt->w_out,
              "missing weights: the branch-1 kernel and bias, W_branch_self_out / W_branch1_h2, V_particle_out/kernel");
  CM3_REQUIRE(d->stage == 1 || (wt->w_b2 && wt->b_b2 && wt->w_b2_h2),
              "missing stage-2 weights: the branch-2 kernel and bias, stage-2/W_others_out / stage-2/W_branch2_h2");
  CM3_REQUIRE((uintptr_t)packed % 16 == 0, "misaligned packed: must be 16-byte aligned");
  const ValuePackParams p = {wt->w_b1, wt->b_b1, wt->w_b1_h2, wt->w_b2, wt->b_b2, wt->w_b2_h2, wt->w_out};
  hipStream_t s = (hipStream_t)stream;
  const int kind = d->kind;
  return agent_launch_1_to_10(d->n_agents, [&](auto n) {
    return kind == kValueLocal ? value_pack_launch<n(), kValueLocal>(p, (float *)packed, s)
                               : value_pack_launch<n(), kValueGlobal>(p, (float *)packed, s);
  });
}

extern "C" int cm3_value_particle_rows_f32(const cm3_value_particle_desc *d, const cm3_value_particle_weights *wt, const cm3_value_rows *r,
                                           void *stream) {
  using namespace cm3;
  int rc = value_check_desc(d);
  if (rc != CM3_OK) return rc;
  CM3_REQUIRE(wt, "null weights");
  CM3_REQUIRE(r, "null rows");
  CM3_REQUIRE(wt->packed, "packed weights are NULL: run cm3_value_particle_pack once per weight update");
  const int N = d->n_agents;
  const bool others = d->kind == kValueLocal && N > 1;
  uint32_t n_rows;
  rc = baseline_row_count(r->n_steps, N, n_rows);
  if (rc != CM3_OK) return rc;
  CM3_REQUIRE(r->state && r->goals, "missing inputs: state and goals are required");
  CM3_REQUIRE(!others || r->obs_others, "missing input: V_particle_local reads obs_others at stage 2");
  CM3_REQUIRE(r->v || r->v64 || r->td, "no output requested: set v, v64 or td");
  CM3_REQUIRE(!r->td || (r->reward && r->done), "missing inputs: td needs reward and done");
  CM3_REQUIRE((uintptr_t)r->state % 16 == 0 && (uintptr_t)r->goals % 8 == 0 && (!others || (uintptr_t)r->obs_others % 16 == 0),
              "misaligned inputs: state and obs_others must be 16-byte aligned, goals 8-byte aligned");
  CM3_REQUIRE(!r->td || (uintptr_t)r->reward % (r->reward_f64 ? 8 : 4) == 0, "misaligned reward");
  CM3_REQUIRE((uintptr_t)r->v % 4 == 0 && (uintptr_t)r->v64 % 8 == 0 && (uintptr_t)r->td % 8 == 0,
              "misaligned outputs: v must be 4-byte aligned, v64 and td 8-byte aligned");
  CM3_REQUIRE((uintptr_t)wt->packed % 16 == 0, "misaligned packed: must be 16-byte aligned");
  ValueParams p;
  memset(&p, 0, sizeof(p));
  p.n_rows = n_rows;
  p.state = r->state;
  p.obs_others = r->obs_others;
  p.goals = r->goals;
  p.reward = r->reward;
  p.reward_f64 = r->reward_f64;
  p.done = r->done;
  p.gamma = r->gamma;
  p.v = r->v;
  p.v64 = r->v64;
  p.td = r->td;
  p.packed = (const float *)wt->packed;
  hipStream_t s = (hipStream_t)stream;
  const int kind = d->kind;
  return agent_launch_1_to_10(N, [&](auto n) {
    return kind == kValueLocal ? value_launch<n(), kValueLocal>(p, s) : value_launch<n(), kValueGlobal>(p, s);
  });
}

extern "C" size_t cm3_coma_particle_packed_bytes(int32_t n_agents) { return cm3::coma_floats_for(n_agents) * sizeof(float); }

extern "C" int cm3_coma_particle_pack(const cm3_coma_particle_desc *d, const cm3_coma_particle_weights *wt, void *packed, void *stream) {
  using namespace cm3;
  int rc = coma_check_desc(d);
  if (rc != CM3_OK) return rc;
  CM3_REQUIRE(wt, "null weights");
  CM3_REQUIRE(packed, "packed is NULL: cm3_coma_particle_packed_bytes(n_agents) bytes of device memory");
  CM3_REQUIRE(wt->w_h1 && wt->b_h1 && wt->w_h2 && wt->b_h2 && wt->w_out && wt->b_out,
              "missing weights: stage-2/Q_goals/{h1,h2,out}/{kernel,bias}");
  CM3_REQUIRE((uintptr_t)packed % 16 == 0, "misaligned packed: must be 16-byte aligned");
  const ComaPackParams p = {wt->w_h1, wt->b_h1, wt->w_h2, wt->b_h2, wt->w_out, wt->b_out};
  hipStream_t s = (hipStream_t)stream;
  return agent_launch_1_to_10(d->n_agents, [&](auto n) { return coma_pack_launch<n()>(p, (float *)packed, s); });
}

extern "C" int cm3_coma_particle_rows_f32(const cm3_coma_particle_desc *d, const cm3_coma_particle_weights *wt, const cm3_coma_rows *r,
                                          void *stream) {
  using namespace cm3;
  int rc = coma_check_desc(d);
  if (rc != CM3_OK) return rc;
  CM3_REQUIRE(wt, "null weights");
  CM3_REQUIRE(r, "null rows");
  CM3_REQUIRE(wt->packed, "packed weights are NULL: run cm3_coma_particle_pack once per weight update");
  const int N = d->n_agents;
  uint32_t n_rows;
  rc = baseline_row_count(r->n_steps, N, n_rows);
  if (rc != CM3_OK) return rc;
  CM3_REQUIRE(r->state && r->goals && r->v_obs, "missing inputs: state, goals and v_obs are required");
  CM3_REQUIRE(r->actions, "missing input: Q_global reads the actions of the others");
  CM3_REQUIRE(r->q || r->q_taken || r->q_taken64 || r->td, "no output requested: set q, q_taken, q_taken64 or td");
  CM3_REQUIRE(!(r->q_taken || r->q_taken64 || r->td) || r->own_actions, "missing input: q_taken, q_taken64 and td need own_actions");
  CM3_REQUIRE(!r->td || (r->reward && r->done), "missing inputs: td needs reward and done");
  CM3_REQUIRE((uintptr_t)r->state % 16 == 0 && (uintptr_t)r->v_obs % 16 == 0 && (uintptr_t)r->goals % 8 == 0 &&
                  (uintptr_t)r->actions % 4 == 0 && (uintptr_t)r->own_actions % 4 == 0,
              "misaligned inputs: state and v_obs must be 16-byte aligned, goals 8-byte aligned, actions and own_actions 4-byte aligned");
  CM3_REQUIRE(!r->td || (uintptr_t)r->reward % (r->reward_f64 ? 8 : 4) == 0, "misaligned reward");
  CM3_REQUIRE((uintptr_t)r->q % 4 == 0 && (uintptr_t)r->q_taken % 4 == 0 && (uintptr_t)r->q_taken64 % 8 == 0 && (uintptr_t)r->td % 8 == 0,
              "misaligned outputs: q and q_taken must be 4-byte aligned, q_taken64 and td 8-byte aligned");
  CM3_REQUIRE((uintptr_t)wt->packed % 16 == 0, "misaligned packed: must be 16-byte aligned");
  ComaParams p;
  memset(&p, 0, sizeof(p));
  p.n_rows = n_rows;
  p.state = r->state;
  p.goals = r->goals;
  p.v_obs = r->v_obs;
  p.actions = r->actions;
  p.own_actions = r->own_actions;
  p.reward = r->reward;
  p.reward_f64 = r->reward_f64;
  p.done = r->done;
  p.gamma = r->gamma;
  p.q = r->q;
  p.q_taken = r->q_taken;
  p.q_taken64 = r->q_taken64;
  p.td = r->td;
  p.packed = (const float *)wt->packed;
  hipStream_t s = (hipStream_t)stream;
  return agent_launch_1_to_10(N, [&](auto n) { return coma_launch<n()>(p, s); });
}
