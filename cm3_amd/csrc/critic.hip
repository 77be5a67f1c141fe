// CM3 particle critics over TRANSITION rows (part of ABI 9, additive): networks.Q_global_1output (networks.py:97-122) and
// networks.Q_credit (:186-211), the evaluations of alg_credit.train_step that carry no gradient -- Q_global_target, Q_credit_target,
// the counterfactual Q_credit over every action, and at N = 1 the counterfactual Q_global of stage 1.
//   branch1 = relu(concat(s_n[4], g_n[2], a[5]) . Q_branch1/kernel[11][64] + bias)
//   branch2 = relu(x2 . stage-2/Q_branch2/kernel[K2][128] + bias)                          (N > 1)
//     global: x2 = concat(s_others[4(N-1)], a_others[5(N-1)]), K2 = 9(N-1);  credit: x2 = concat(s_m[4], s_others[4(N-1)]), K2 = 4N
//   h2  = relu(branch1 . W_branch1_h2[64][64] + branch2 . stage-2/W_branch2_h2[128][64])    (no bias)
//   out = h2 . Q_out/kernel[64][1]                                                          (no bias)
// The kernel takes NO tiled feed: every row of the n x n x 5 tilings of train_step is an index function of the batch's base columns
// (state [B][N][4], goals [B][N][2], actions [B][N]), so a lane decodes (b, m, n, a) from its row number and gathers ~100 bytes.
//   ROWS  (global)            r = b N + n              a = onehot(actions[b][n])
//   PAIRS (credit)            r = (b N + m) N + n      a = onehot(actions[b][m]), s_m = state[b][m]; s_n, g_n, s_others those of n
//   CF    (credit; global N=1) r = r' 5 + a            a = row a of eye(5); r' = the PAIRS index, or b
// s_others / a_others run over the agents j != n in ascending order (batch.process_global_state / process_actions).
// Mapping as qmix_forward (actor.hip): 256 threads = 4 waves own 64 rows; every layer on the exact-f32 matrix instruction
// (v_mfma_f32_16x16x4_f32, a k-ordered fmaf chain), so a row's bits depend on neither its place in the workgroup nor the launch's
// row count.  The one-hot inputs are 0 / 1 INPUTS of the same chains in every form: equal inputs give equal bits.
//   branch1 (K = 11 -> 12): transposed, C[unit][row]; wave w owns units [16w, 16w+16) of all 64 rows.
//   branch2 (K2 -> whole k-steps, up to 84): transposed; wave w owns units [32w, 32w+32) as two 16-unit slices.
//   h2 (192 -> 64, ONE chain over concat(branch1, branch2): 51 % .. 83 % of the FLOPs): wave w owns columns [16w, 16w+16).
//   out (64 -> 1): one 16 x 16 tile per wave, only output row 0 carries weights; lane l < 16 of wave w finishes row 16w + l.
// LDS: hidden [64][194] + inputs [64][13] + [64][K2P + 1]; h2 [64][66] reuses the input tiles.  N = 10 global: 74 752 bytes.
#include "critic_rows.h"

namespace cm3 {

using namespace critic_rows;   // (kinds, forms, form_exists, decode, form_dispatch, the entries' checks)
constexpr int kCriticGlobal = kGlobal, kCriticCredit = kCredit;
constexpr int kCH1 = 64, kCH2B = 128, kCH2 = 64;     // n_h1_1, n_h1_2, n_h2 (config.json nn block)

template <int N, int KIND> struct CriticLayout {
  static constexpr bool kStage2 = N > 1;
  static constexpr int K1 = 11, S1 = 3, S1P = 4;
  static constexpr int K2 = !kStage2 ? 0 : (KIND == kCriticGlobal ? 9 * (N - 1) : 4 * N);
  static constexpr int K2P = (K2 + 3) / 4 * 4;
  static constexpr int S2 = K2P / 4;                          // branch-2 k-steps (up to 21)
  static constexpr int S2P = (S2 + 3) / 4 * 4;                // per-lane stride of the branch-2 operands (16-byte loads)
  static constexpr int HW = kStage2 ? kCH1 + kCH2B : kCH1;    // width of concat(branch1, branch2)
  static constexpr int SH = HW / 4;                           // k-steps of the h2 layer (48 / 16)
  static constexpr int HS = HW + 2, X1W = 13, X2W = K2P + 1, H2S = kCH2 + 2;     // LDS row strides
  static constexpr int kIn = 64 * X1W + (kStage2 ? 64 * X2W : 0);
  static constexpr int kLdsFloats = 64 * HS + (kIn > 64 * H2S ? kIn : 64 * H2S);
  // packed weights (floats)
  static constexpr int kW1 = 0;                               // [4 waves][64 lanes][S1P]      A operands of branch 1
  static constexpr int kB1 = kW1 + 4 * 64 * S1P;              // [64]
  static constexpr int kW2 = kB1 + kCH1;                      // [4 waves][2][64 lanes][S2P]   A operands of branch 2
  static constexpr int kB2 = kW2 + 4 * 2 * 64 * S2P;          // [128]
  static constexpr int kWh = kB2 + (kStage2 ? kCH2B : 0);     // [4 waves][64 lanes][SH]       B operands of h2
  static constexpr int kWo = kWh + 4 * 64 * SH;               // [64 lanes][16]                A operands of out (row 0 only)
  static constexpr int kTotal = kWo + 64 * 16;
};

struct CriticPackParams {
  const float *w_b1, *b_b1, *w_b1_h2, *w_b2, *b_b2, *w_b2_h2, *w_out;
};

template <int N, int KIND> __global__ void __launch_bounds__(256) k_critic_pack(const CriticPackParams p, float *out) {
  using CL = CriticLayout<N, KIND>;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < CL::kTotal; t += gridDim.x * 256) {
    float v = 0.0f;
    if (t < CL::kB1) {
      const int s = t % CL::S1P, lane = (t / CL::S1P) & 63, w = t / CL::S1P / 64;
      const int k = 4 * s + (lane >> 4), j = 16 * w + (lane & 15);
      v = (s < CL::S1 && k < CL::K1) ? p.w_b1[k * kCH1 + j] : 0.0f;
    } else if (t < CL::kW2) {
      v = p.b_b1[t - CL::kB1];
    } else if (t < CL::kB2) {
      if constexpr (CL::kStage2) {
        const int u = t - CL::kW2, s = u % CL::S2P, lane = (u / CL::S2P) & 63, c = (u / CL::S2P / 64) & 1, w = u / CL::S2P / 128;
        const int k = 4 * s + (lane >> 4), j = 32 * w + 16 * c + (lane & 15);
        v = (s < CL::S2 && k < CL::K2) ? p.w_b2[k * kCH2B + j] : 0.0f;
      }
    } else if (t < CL::kWh) {
      if constexpr (CL::kStage2) v = p.b_b2[t - CL::kB2];
    } else if (t < CL::kWo) {
      const int u = t - CL::kWh, s = u % CL::SH, lane = (u / CL::SH) & 63, w = u / CL::SH / 64;
      const int k = 4 * s + (lane >> 4), j = 16 * w + (lane & 15);
      if (k < kCH1) {
        v = p.w_b1_h2[k * kCH2 + j];
      } else {
        if constexpr (CL::kStage2) v = p.w_b2_h2[(k - kCH1) * kCH2 + j];
      }
    } else {
      const int u = t - CL::kWo, s = u & 15, lane = u >> 4;
      v = (lane & 15) == 0 ? p.w_out[4 * s + (lane >> 4)] : 0.0f;
    }
    out[t] = v;
  }
}

struct CriticParams {
  uint32_t n_rows;
  const float *state, *goals;     // [B][N][4], [B][N][2]
  const int32_t *actions;         // [B][N] (ROWS, PAIRS)
  const void *reward;             // [B][N] float32 / float64 (td)
  int reward_f64;
  const uint8_t *done;            // [B] (td)
  double gamma;
  float *q;                       // optional [n_rows]
  double *q64, *td;               // optional [n_rows]
  const float *packed;
};

template <int N, int KIND, int FORM> __global__ void CM3_MATRIX_KERNEL k_critic_particle_rows(const CriticParams p) {
  using CL = CriticLayout<N, KIND>;
  static_assert(form_exists(KIND, FORM, N), "forms: global ROWS (and CF at N = 1), credit PAIRS / CF at N > 1");
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

  // ---- staging: lane = row; wave 0 the branch-1 tile, the 4-float / 5-float pieces of the branch-2 tile dealt round the waves ----
  {
    const uint32_t r = row_base + lane;
    uint32_t b;
    int m, n, a;
    decode<N, FORM>(r < rows ? r : rows - 1, b, m, n, a);
    const uint32_t base = b * (uint32_t)N;
    if (w == 0) {
      const float4 s = reinterpret_cast<const float4 *>(p.state)[base + n];
      const float2 g = reinterpret_cast<const float2 *>(p.goals)[base + n];
      if constexpr (FORM != kFormCf) a = p.actions[base + m];
      x1[lane][0] = s.x; x1[lane][1] = s.y; x1[lane][2] = s.z; x1[lane][3] = s.w;
      x1[lane][4] = g.x; x1[lane][5] = g.y;
#pragma unroll
      for (int k = 0; k < kA; ++k) x1[lane][6 + k] = a == k ? 1.0f : 0.0f;
      x1[lane][11] = 0.0f;
      if constexpr (CL::kStage2) {
#pragma unroll
        for (int k = CL::K2; k < CL::K2P; ++k) x2[lane][k] = 0.0f;
      }
    }
    if constexpr (CL::kStage2) {
      constexpr int kStatePieces = KIND == kCriticGlobal ? N - 1 : N;
      constexpr int kPieces = KIND == kCriticGlobal ? 2 * (N - 1) : N;
      for (int u = w; u < kPieces; u += 4) {      // (u is wave-uniform)
        if (u < kStatePieces) {
          int j;
          if constexpr (KIND == kCriticCredit) {
            const int v = u - 1;
            j = u == 0 ? m : v + (v >= n ? 1 : 0);
          } else {
            j = u + (u >= n ? 1 : 0);
          }
          const float4 s = reinterpret_cast<const float4 *>(p.state)[base + j];
          x2[lane][4 * u + 0] = s.x; x2[lane][4 * u + 1] = s.y; x2[lane][4 * u + 2] = s.z; x2[lane][4 * u + 3] = s.w;
        } else {
          const int v = u - kStatePieces;
          const int act = p.actions[base + v + (v >= n ? 1 : 0)];
#pragma unroll
          for (int k = 0; k < kA; ++k) x2[lane][4 * (N - 1) + kA * v + k] = act == k ? 1.0f : 0.0f;
        }
      }
    }
  }
  __syncthreads();
  // ---- branch 1: units [16w, 16w+16) of all 64 rows, C[unit][row], bias as the start value ----------------------------------------
  {
    const float4 a1 = reinterpret_cast<const float4 *>(p.packed + CL::kW1)[w * 64 + lane];
    const float4 b1 = reinterpret_cast<const float4 *>(p.packed + CL::kB1)[4 * w + hi];
    const float a1s[3] = {a1.x, a1.y, a1.z};
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
        float *dst = &hs[16 * t + col][kCH1 + 32 * w + 16 * cs + 4 * hi];
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
  // ---- out: C[.][row] of rows [16w, 16w+16); output row 0 is Q, in register 0 of lanes 0..15 -------------------------------------
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
  for (int s = 0; s < kCH2 / 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wo[s], h2s[16 * w + col][4 * s + hi], acc, 0, 0, 0);
  const float q = acc[0];
  const uint32_t hr = row_base + 16 * w + col;
  if (hi == 0 && hr < rows) {
    if (p.q) p.q[hr] = q;
    if (p.q64) p.q64[hr] = (double)q;
    if constexpr (FORM != kFormCf) {
      if (p.td) {
        // reward + gamma * q * not_done in the order of k_td_target (batch.hip) on the widened q
        uint32_t b;
        int m, n, a;
        decode<N, FORM>(hr, b, m, n, a);
        const size_t bn = (size_t)b * N + n;
        const double rw = p.reward_f64 ? reinterpret_cast<const double *>(p.reward)[bn] : (double)reinterpret_cast<const float *>(p.reward)[bn];
        const double gq = p.gamma * (double)q;
        p.td[hr] = rw + gq * (double)(int64_t)(p.done[b] ? 0 : 1);
      }
    }
  }
}

template <int N, int KIND, int FORM> static int critic_launch(const CriticParams &p, hipStream_t s) {
  const unsigned blocks = (p.n_rows + 63u) / 64u;
  note_variant("k_critic_particle_rows", (int)sizeof(float), N, 4, 0, 0, 0, 0, 0, 0, /* prec=f32 */ 0);
  note_tail(variant_tail(KIND, FORM));
  hipLaunchKernelGGL((k_critic_particle_rows<N, KIND, FORM>), dim3(blocks), dim3(256), 0, s, p);
  CM3_HIP_CHECK(hipGetLastError());
  return CM3_OK;
}

template <int N> static int critic_launch_form(int kind, int form, const CriticParams &p, hipStream_t s) {
  return form_dispatch<N>(kind, form, "critic", [&](auto k, auto f) { return critic_launch<N, k(), f()>(p, s); });
}

template <int N> static int critic_pack_launch(int kind, const CriticPackParams &p, float *out, hipStream_t s) {
  if (kind == kCriticGlobal) {
    hipLaunchKernelGGL((k_critic_pack<N, kCriticGlobal>), dim3(32), dim3(256), 0, s, p, out);
  } else if constexpr (N > 1) {
    hipLaunchKernelGGL((k_critic_pack<N, kCriticCredit>), dim3(32), dim3(256), 0, s, p, out);
  }
  CM3_HIP_CHECK(hipGetLastError());
  return CM3_OK;
}

static size_t critic_floats_for(int n, int kind) { return floats_for<CriticLayout, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10>(n, kind); }

static int critic_check_desc(const cm3_critic_particle_desc *d) {
  CM3_REQUIRE(d, "null desc");
  CM3_REQUIRE(d->n_agents >= 1 && d->n_agents <= CM3_MAX_AGENTS, "n_agents must be in 1..%d", CM3_MAX_AGENTS);
  const int rc = check_kind_stage(d->kind, d->stage, d->n_agents, "Q_global_1output", "Q_credit");
  if (rc != CM3_OK) return rc;
  CM3_REQUIRE(d->n_h1_1 == kCH1 && d->n_h1_2 == kCH2B && d->n_h2 == kCH2,
              "supported critic widths are 64/128/64 (config.json nn block); got %d/%d/%d", d->n_h1_1, d->n_h1_2, d->n_h2);
  return CM3_OK;
}
}  // namespace cm3

extern "C" size_t cm3_critic_particle_packed_bytes(int32_t n_agents, int32_t kind) {
  return cm3::critic_floats_for(n_agents, kind) * sizeof(float);
}

extern "C" int cm3_critic_particle_pack(const cm3_critic_particle_desc *d, const cm3_critic_particle_weights *wt, void *packed,
                                        void *stream) {
  using namespace cm3;
  int rc = critic_check_desc(d);
  if (rc != CM3_OK) return rc;
  CM3_REQUIRE(wt, "null weights");
  CM3_REQUIRE(packed, "packed is NULL: cm3_critic_particle_packed_bytes(n_agents, kind) bytes of device memory");
  CM3_REQUIRE(wt->w_b1 && wt->b_b1 && wt->w_b1_h2 && wt->w_out, "missing weights: Q_branch1/kernel, Q_branch1/bias, W_branch1_h2, Q_out/kernel");
  CM3_REQUIRE(d->stage == 1 || (wt->w_b2 && wt->b_b2 && wt->w_b2_h2),
              "missing stage-2 weights: stage-2/Q_branch2/kernel, stage-2/Q_branch2/bias, stage-2/W_branch2_h2");
  CM3_REQUIRE((uintptr_t)packed % 16 == 0, "misaligned packed: must be 16-byte aligned");
  const CriticPackParams p = {wt->w_b1, wt->b_b1, wt->w_b1_h2, wt->w_b2, wt->b_b2, wt->w_b2_h2, wt->w_out};
  hipStream_t s = (hipStream_t)stream;
  const int kind = d->kind;
  return agent_launch_1_to_10(d->n_agents, [&](auto n) { return critic_pack_launch<n()>(kind, p, (float *)packed, s); });
}

extern "C" int cm3_critic_particle_rows_f32(const cm3_critic_particle_desc *d, const cm3_critic_particle_weights *wt,
                                            const cm3_critic_rows *r, void *stream) {
  using namespace cm3;
  int rc = critic_check_desc(d);
  if (rc != CM3_OK) return rc;
  CM3_REQUIRE(wt, "null weights");
  CM3_REQUIRE(r, "null rows");
  CM3_REQUIRE(wt->packed, "packed weights are NULL: run cm3_critic_particle_pack once per weight update");
  const int N = d->n_agents;
  uint32_t n_rows;
  rc = check_rows(r, wt->packed, d->kind, N, "Q_global", "Q_credit", r->state && r->goals, "missing inputs: state and goals are required",
                  (uintptr_t)r->state % 16 == 0 && (uintptr_t)r->goals % 8 == 0 && (uintptr_t)r->actions % 4 == 0,
                  "misaligned inputs: state must be 16-byte aligned, goals 8-byte aligned, actions 4-byte aligned", n_rows);
  if (rc != CM3_OK) return rc;
  CriticParams p;
  memset(&p, 0, sizeof(p));
  p.n_rows = n_rows;
  p.state = r->state;
  p.goals = r->goals;
  p.actions = r->actions;
  p.reward = r->reward;
  p.reward_f64 = r->reward_f64;
  p.done = r->done;
  p.gamma = r->gamma;
  p.q = r->q;
  p.q64 = r->q64;
  p.td = r->td;
  p.packed = (const float *)wt->packed;
  hipStream_t s = (hipStream_t)stream;
  const int kind = d->kind, form = r->form;
  return agent_launch_1_to_10(N, [&](auto n) { return critic_launch_form<n()>(kind, form, p, s); });
}
