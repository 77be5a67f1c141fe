// The particle QMIX learner (part of ABI 9, additive): mixer_op of alg_qmix.py:186-192, 371-378 -- loss, dense gradients of the eleven
// trainable variables, and tf.train.AdamOptimizer's step -- in float32, for 1..10 agents.
//   agent rows r = (b, n), R = B N     x = concat(o_others[L], o_self[4], goal[2]), K1 = L + 6           (networks.py:581-594)
//     h1 = relu(x . h/kernel + h/bias)   h2 = relu(h1 . h2/kernel + h2/bias)   Q = h2 . out/kernel + out/bias   q_sel = Q[action[r]]
//   transitions b                      xm = concat(v_global[b] [4N], goals[b] [2N]), KM = 6N              (networks.py:640-685)
//     q_tot = Qmix_mixer(q_sel[b][0..N), xm)        loss = mean_b((float32(td[b]) - q_tot[b])^2)
// cm3_qmix_learner_particle_grad_f32 is FIVE launches on one stream, every one capturable; all scratch is the caller's workspace
// (cm3_qmix_learner_particle_workspace_bytes).  Every matrix product is on the exact-f32 matrix instruction
// (v_mfma_f32_16x16x4_f32, a k-ordered fmaf chain); the unit is built with -ffp-contract=off.  The weights are read as TensorFlow
// shapes them ([in][out]); the launches read no packed copy, so they follow the tensors as they are at launch.
//
// 1. k_learner_agent_fwd   256 threads = 4 waves own 64 agent rows.  The forward pass in the operand order of k_qmix_particle_rows
//    (actor.hip), so Q has the bits greedy_rows computes:
//      h    C[unit][row], wave w units [16w, 16w + 16): chain over k = 0 .. K1 + 1 (two zero pads) started by the bias
//      h2   C[row][unit], wave w units [16w, 16w + 16): chain over k = 0 .. 63 from zero, + bias
//      out  C[action][row], wave w rows [16w, 16w + 16): chain over k = 0 .. 63 started by the bias
//    Leaves x (padded to K1 + 2), h1, h2 (after relu) and q_sel in the workspace.  An action outside 0..4 selects nothing: q_sel 0.
//    LDS: x [64][K1 + 3] + h1, h2 [64][66]: 45 312 bytes at N = 10.
// 2. k_learner_mixer       256 threads = 4 waves own 16 transitions; wave w owns the embedding units e in [16w, 16w + 16), lane
//    (hi, col) rows 4 hi + 0..3 at e = 16w + col.  The forward pass is the text of k_qmix_mixer_rows (mixer.hip) on q_sel, so q_tot has
//    the bits ParticleQmixMixer.q_tot computes from the same agent_qs; the pre-activations stay in registers.  Then, per row,
//      dq = (2 (q_tot - td)) / B                                         err2 = (td - q_tot)^2
//      d l1_pre = l1_pre > 0 ? dq hyper_b_final[e] : 0                   (ReluGrad)        p_bf = dq l1[e]
//      d wf_pre = dq hidden[e] sign(wf_pre[e])                           (sign(0) = 0)
//      dh = dq |wf_pre[e]| (h > 0 ? 1 : hidden[e] + 1)                   (EluGrad: elu + 1 below zero)      d b1_pre = dh
//      d w1_pre[n][e] = dh q_sel[n] sign(w1_pre[n][e])                   d q_sel[n] = sum_e dh[e] |w1_pre[n][e]|
//    The sum over e is the forward's tree: pairwise inside every 16 units by DPP moves, then the four waves through LDS in wave order
//    ((s0 + s1) + s2) + s3.  Leaves xm (padded to whole k-steps), the delta rows [B][64 (N + 4)] -- N blocks d w1_pre, d b1_pre,
//    d wf_pre, d l1_pre, p_bf --, d q_sel, q_tot and err2.  LDS at N = 10: 7 744 bytes.
// 3. k_learner_agent_bwd   256 threads own 64 agent rows.  d Q = d q_sel at the taken action, so
//      d h2_pre[u] = h2[u] > 0 ? d q_sel out/kernel[u][action] : 0       (one product: exact)
//      d h1_pre[u] = h1[u] > 0 ? sum_v d h2_pre[v] h2/kernel[u][v] : 0   C[row][u], chain over v = 0 .. 63 from zero
//    Leaves d Q padded to 16 columns, d h2_pre and d h1_pre.  LDS: [64][66] floats, 16 896 bytes.
// 4. k_learner_xtd<4>      (learner_common.h) the weight gradients X^T . Delta with the ROW index as the contraction, four jobs in one launch:
//      h/kernel, h/bias     X = x,  Delta = d h1_pre        h2/kernel, h2/bias   X = h1, Delta = d h2_pre
//      out/kernel, out/bias X = h2, Delta = d Q             the mixer's five     X = xm, Delta = the delta rows
//    One wave per 16 x 16 output tile and per CHUNK of 256 consecutive rows: A[i][k] = X[row k][16 kt + i], B[k][j] =
//    Delta[row k][16 mt + j], one chain from zero over the chunk's rows in ascending order, four rows per instruction.  A bias gradient
//    (and hyper_b_final's, the column sums of p_bf) is one more row tile whose A operand is 1 in row 0: the same chain.  The chunk's
//    tile goes to the workspace.  No LDS.
// 5. k_learner_reduce<4>   (learner_common.h) one thread per gradient element: the chunks' partial sums added in ascending chunk order, from the first,
//    and stored TF-shaped.  Its last workgroup sums err2: thread t the rows t, t + 256, ... in ascending order from zero, then the 256
//    partial sums by a halving tree in LDS (t with t + 128, then + 64, ...); loss = sum / B.
// No floating-point atomics anywhere.  Chunks are cut by the row count alone, so every sum's order depends on the batch and on nothing
// of the launch: two launches on the same inputs give the same bits.
//
// cm3_adam_step_f32 (k_adam_step) knows nothing of QMIX: one launch over a device table of (var, grad, m, v, count) segments applies
//   lr_t = lr sqrt(1 - beta2_power) / (1 - beta1_power);  m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g g;
//   var = var - (lr_t m) / (sqrt(v) + epsilon)
// as tf.train.AdamOptimizer does (epsilon outside the bias correction), every product and sum a float32 operation of its own.  The two
// powers live in device memory as ONE 64-bit object next to an arrival counter ({beta1_power, beta2_power, arrivals, 0}); thread 0 of
// every workgroup reads them and then takes a ticket, and the workgroup with the last ticket stores the powers
// multiplied by beta1 / beta2 and resets the counter (the mechanism of rows_draw_arrive, actor_common.h; the ticket is an acq_rel
// agent-scope add, so the store comes after every read).  A replayed graph therefore takes the next step.  Launches that share a state
// must be ordered on the device.
#include "actor_common.h"
#include "learner_common.h"

namespace cm3 {
namespace learner {

constexpr int kH = 64;          // both hidden widths of Qmix_single_particle
constexpr int kE = 64;          // embed_dim of Qmix_mixer

template <int N> struct LL {
  static constexpr int L = 4 * (N > 1 ? N - 1 : 1);
  static constexpr int K1 = L + 6, K1P = L + 8, S1 = K1P / 4, XW = K1P + 1, HS = kH + 2;
  static constexpr int KM = 6 * N, KMP = (KM + 3) / 4 * 4, SM = KMP / 4, XMW = KMP + 1;
  static constexpr int NB = N + 4;          // delta blocks: d w1_pre[0..N), d b1_pre, d wf_pre, d l1_pre, p_bf
  static constexpr int MD = kE * NB;
  static constexpr int KT1 = (K1 + 15) / 16, KTM = (KM + 15) / 16;
};

// the workspace, in floats; every part starts at a multiple of four
struct Ws {
  size_t xa, h1, h2, qsel, dqs, dq16, dh2, dh1, xm, dhy, err2, p1, p2, po, ph, total;
  size_t chunks_a, chunks_m;
};
static inline size_t up4(size_t x) { return (x + 3) / 4 * 4; }
template <int N> static Ws ws_layout(size_t B) {
  using T = LL<N>;
  const size_t R = B * N;
  Ws w;
  w.chunks_a = (R + kChunk - 1) / kChunk;
  w.chunks_m = (B + kChunk - 1) / kChunk;
  size_t o = 0;
  w.xa = o;   o += up4(R * T::K1P);
  w.h1 = o;   o += R * kH;
  w.h2 = o;   o += R * kH;
  w.qsel = o; o += up4(R);
  w.dqs = o;  o += up4(R);
  w.dq16 = o; o += R * 16;
  w.dh2 = o;  o += R * kH;
  w.dh1 = o;  o += R * kH;
  w.xm = o;   o += B * T::KMP;
  w.dhy = o;  o += B * T::MD;
  w.err2 = o; o += up4(B);
  w.p1 = o;   o += w.chunks_a * (size_t)((T::KT1 + 1) * 16 * kH);
  w.p2 = o;   o += w.chunks_a * (size_t)((kH / 16 + 1) * 16 * kH);
  w.po = o;   o += w.chunks_a * (size_t)((kH / 16 + 1) * 16 * 16);
  w.ph = o;   o += w.chunks_m * (size_t)((T::KTM + 1) * 16 * T::MD);
  w.total = o;
  return w;
}

// ---- 1. the agent network over the rows, keeping what the backward pass reads ------------------------------------------------------
struct AgentFwdParams {
  size_t n_rows;
  const float *obs_others, *v_obs, *goals;   // [R][L], [R][4], [R][2]
  const int32_t *actions;                    // [R]
  const float *w1, *b1, *w2, *b2, *wo, *bo;  // h/kernel [K1][64], h/bias, h2/kernel [64][64], h2/bias, out/kernel [64][5], out/bias
  float *xa, *h1, *h2, *qsel;                // [R][K1P], [R][64], [R][64], [R]
};

template <int N> __global__ void CM3_MATRIX_KERNEL k_learner_agent_fwd(const AgentFwdParams p) {
  using T = LL<N>;
  constexpr int L = T::L, S1 = T::S1;
  __shared__ float xs[64][T::XW];
  __shared__ __attribute__((aligned(16))) float h1s[64][T::HS];
  __shared__ float h2s[64][T::HS];
  const int tid = threadIdx.x, lane = tid & 63, col = lane & 15, hi = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const size_t rows = p.n_rows;
  const size_t row_base = (size_t)blockIdx.x * 64;

  if (w == 0) {
    // concat(o_others, o_self, goal) (networks.py:583), two zero pads; rows past the count repeat the last one
    const size_t r = row_base + lane;
    const size_t rc = r < rows ? r : rows - 1;
    const float4 *o4 = reinterpret_cast<const float4 *>(p.obs_others + rc * L);
#pragma unroll
    for (int k = 0; k < L / 4; ++k) {
      const float4 v = o4[k];
      xs[lane][4 * k + 0] = v.x; xs[lane][4 * k + 1] = v.y; xs[lane][4 * k + 2] = v.z; xs[lane][4 * k + 3] = v.w;
    }
    const float4 s = reinterpret_cast<const float4 *>(p.v_obs)[rc];
    const float2 g = reinterpret_cast<const float2 *>(p.goals)[rc];
    xs[lane][L + 0] = s.x; xs[lane][L + 1] = s.y; xs[lane][L + 2] = s.z; xs[lane][L + 3] = s.w;
    xs[lane][L + 4] = g.x; xs[lane][L + 5] = g.y;
    xs[lane][L + 6] = 0.0f; xs[lane][L + 7] = 0.0f;
  }
  // this lane's operands: A of layer h (W[k = 4 s + hi][unit 16 w + col]), B of layer h2, A of the head (0 for actions >= 5)
  float a1[S1], bw[kH / 4], wo[kH / 4];
#pragma unroll
  for (int s = 0; s < S1; ++s) {
    const int k = 4 * s + hi;
    a1[s] = k < T::K1 ? p.w1[k * kH + 16 * w + col] : 0.0f;
  }
#pragma unroll
  for (int s = 0; s < kH / 4; ++s) {
    const int k = 4 * s + hi;
    bw[s] = p.w2[k * kH + 16 * w + col];
    wo[s] = col < kA ? p.wo[k * kA + col] : 0.0f;
  }
  float b1[4], bo[4];
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    b1[reg] = p.b1[16 * w + 4 * hi + reg];
    bo[reg] = 4 * hi + reg < kA ? p.bo[4 * hi + reg] : 0.0f;
  }
  const float b2 = p.b2[16 * w + col];
  __syncthreads();
  // ---- layer "h": units [16w, 16w + 16) for all 64 rows, C[unit][row] ----
  {
    f32x4 c[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) c[t] = f32x4{b1[0], b1[1], b1[2], b1[3]};
#pragma unroll
    for (int s = 0; s < S1; ++s)
#pragma unroll
      for (int t = 0; t < 4; ++t) c[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[s], xs[16 * t + col][4 * s + hi], c[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      *reinterpret_cast<float2 *>(&h1s[16 * t + col][16 * w + 4 * hi]) = make_float2(relu_f32(c[t][0]), relu_f32(c[t][1]));
      *reinterpret_cast<float2 *>(&h1s[16 * t + col][16 * w + 4 * hi + 2]) = make_float2(relu_f32(c[t][2]), relu_f32(c[t][3]));
    }
  }
  __syncthreads();
  // ---- layer "h2": columns [16w, 16w + 16), C[row][unit] ----
  {
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int s = 0; s < kH / 4; ++s)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(h1s[16 * t + col][4 * s + hi], bw[s], acc[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) h2s[16 * t + 4 * hi + reg][16 * w + col] = relu_f32(acc[t][reg] + b2);
  }
  __syncthreads();
  // ---- head "out": C[action][row] of rows [16w, 16w + 16), bias as the start value; the lane that holds the taken action stores it ----
  {
    f32x4 acc = f32x4{bo[0], bo[1], bo[2], bo[3]};
#pragma unroll
    for (int s = 0; s < kH / 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wo[s], h2s[16 * w + col][4 * s + hi], acc, 0, 0, 0);
    const size_t hr = row_base + 16 * w + col;
    if (hr < rows) {
      const int act = p.actions[hr];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        if (4 * hi + reg == act) p.qsel[hr] = acc[reg];
      if (hi == 2 && (act < 0 || act >= kA)) p.qsel[hr] = 0.0f;
    }
  }
  // ---- what the backward pass reads ----
  for (int idx = tid; idx < 64 * kH; idx += 256) {
    const int r = idx >> 6, u = idx & 63;
    const size_t gr = row_base + r;
    if (gr < rows) {
      p.h1[gr * kH + u] = h1s[r][u];
      p.h2[gr * kH + u] = h2s[r][u];
    }
  }
  for (int idx = tid; idx < 64 * T::K1P; idx += 256) {
    const int r = idx / T::K1P, k = idx - r * T::K1P;
    const size_t gr = row_base + r;
    if (gr < rows) p.xa[gr * T::K1P + k] = xs[r][k];
  }
}

// ---- 2. the mixer: forward as k_qmix_mixer_rows, the loss terms, the deltas of the hyper-network and of q_sel -----------------------
struct MixParams {
  uint32_t B;
  int td_f64;
  const float *state, *goals, *qsel;            // [B][N][4], [B][N][2], [B][N]
  const void *td;                               // [B] float64 / float32
  const float *w1, *wf, *b1, *bfl1, *bf;        // hyper_w_1 [KM][64 N], hyper_w_final, hyper_b_1, hyper_b_final_l1/kernel [KM][64], [64]
  float *q_tot, *err2, *xm, *dhy, *dqs;         // [B], [B], [B][KMP], [B][MD], [B][N]
};


// x . W[:, c0 + e] for this lane's e and four rows: one k-ordered chain from zero over the KMP inputs (zero operands past KM)
template <int N> __device__ __forceinline__ f32x4 hyper_block(const float *W, int ld, int ce, int hi, const float (&xa)[LL<N>::SM]) {
  using T = LL<N>;
  float bw[T::SM];
#pragma unroll
  for (int s = 0; s < T::SM; ++s) {
    const int k = 4 * s + hi;
    bw[s] = k < T::KM ? W[k * ld + ce] : 0.0f;
  }
  f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int s = 0; s < T::SM; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[s], bw[s], acc, 0, 0, 0);
  return acc;
}

template <int N> __global__ void CM3_MATRIX_KERNEL k_learner_mixer(const MixParams p) {
  using T = LL<N>;
  constexpr int kRows = 16;
  __shared__ float xs[kRows][T::XMW];
  __shared__ float qs[kRows][N];
  __shared__ float part[4][kRows][2];
  __shared__ float partq[4][kRows][N];
  __shared__ float qrow[kRows], tds[kRows];
  const int tid = threadIdx.x, lane = tid & 63, col = lane & 15, hi = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t rows = p.B;
  const uint32_t row_base = blockIdx.x * (uint32_t)kRows;

  // ---- staging: thread u = (row, agent) brings one agent's state, goal and Q; rows past the count repeat the last one ----
  if (tid < kRows * N) {
    const int r = tid / N, n = tid - r * N;
    const uint32_t hr = row_base + r;
    const size_t bn = (size_t)(hr < rows ? hr : rows - 1) * N + n;
    const float4 s = reinterpret_cast<const float4 *>(p.state)[bn];
    const float2 g = reinterpret_cast<const float2 *>(p.goals)[bn];
    xs[r][4 * n + 0] = s.x; xs[r][4 * n + 1] = s.y; xs[r][4 * n + 2] = s.z; xs[r][4 * n + 3] = s.w;
    xs[r][4 * N + 2 * n + 0] = g.x; xs[r][4 * N + 2 * n + 1] = g.y;
    qs[r][n] = p.qsel[bn];
  } else if (tid >= 192 && tid < 192 + kRows) {
#pragma unroll
    for (int k = T::KM; k < T::KMP; ++k) xs[tid - 192][k] = 0.0f;
  } else if (tid >= 224 && tid < 224 + kRows) {
    // the td_target placeholder is tf.float32: a float64 target is rounded as it is read
    const uint32_t hr = row_base + (tid - 224);
    const size_t b = hr < rows ? hr : rows - 1;
    tds[tid - 224] = p.td_f64 ? (float)reinterpret_cast<const double *>(p.td)[b] : reinterpret_cast<const float *>(p.td)[b];
  }
  __syncthreads();

  float xa[T::SM];                      // A operands: x[row = col][k = 4 s + hi], the same for every column block
#pragma unroll
  for (int s = 0; s < T::SM; ++s) xa[s] = xs[col][4 * s + hi];
  float qv[4][N];                       // q_sel of this lane's four rows
#pragma unroll
  for (int reg = 0; reg < 4; ++reg)
#pragma unroll
    for (int n = 0; n < N; ++n) qv[reg][n] = qs[4 * hi + reg][n];

  const int e = 16 * w + col;
  // the chain over agents: |w1_pre[n][e]| ascending, started by the product for n = 0 (mixer.hip)
  f32x4 a[N];
  float t[4];
#pragma unroll
  for (int n = 0; n < N; ++n) {
    a[n] = hyper_block<N>(p.w1, kE * N, kE * n + e, hi, xa);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const float term = qv[reg][n] * __builtin_fabsf(a[n][reg]);
      t[reg] = n == 0 ? term : t[reg] + term;
    }
  }
  const f32x4 b1 = hyper_block<N>(p.b1, kE, e, hi, xa), wf = hyper_block<N>(p.wf, kE, e, hi, xa), l1 = hyper_block<N>(p.bfl1, kE, e, hi, xa);
  const float bf = p.bf[e];
  float h[4], hidden[4];
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    h[reg] = t[reg] + b1[reg];
    hidden[reg] = h[reg] > 0.0f ? h[reg] : expm1f(h[reg]);
    const float pe = hidden[reg] * __builtin_fabsf(wf[reg]);
    const float ce = relu_f32(l1[reg]) * bf;
    const float sp = lrn_sum16(pe), sc = lrn_sum16(ce);
    if (col == 0) {
      part[w][4 * hi + reg][0] = sp;
      part[w][4 * hi + reg][1] = sc;
    }
  }
  __syncthreads();
  if (tid < kRows) {
    const float sp = ((part[0][tid][0] + part[1][tid][0]) + part[2][tid][0]) + part[3][tid][0];
    const float sc = ((part[0][tid][1] + part[1][tid][1]) + part[2][tid][1]) + part[3][tid][1];
    const float q = sp + sc;
    qrow[tid] = q;
    const uint32_t hr = row_base + tid;
    if (hr < rows) {
      const float d = tds[tid] - q;
      p.q_tot[hr] = q;
      p.err2[hr] = d * d;
    }
  }
  __syncthreads();
  // ---- backward: this lane's e of its four rows ----
  const float batch = (float)rows;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int r = 4 * hi + reg;
    const uint32_t hr = row_base + r;
    const bool live = hr < rows;
    const float dq = (2.0f * (qrow[r] - tds[r])) / batch;
    const float l1r = relu_f32(l1[reg]);
    const float d_l1 = l1[reg] > 0.0f ? dq * bf : 0.0f;
    const float p_bf = dq * l1r;
    const float d_wf = (dq * hidden[reg]) * sign_f32(wf[reg]);
    const float dhid = dq * __builtin_fabsf(wf[reg]);
    const float dh = h[reg] > 0.0f ? dhid : dhid * (hidden[reg] + 1.0f);
    float *out = p.dhy + (size_t)(live ? hr : 0) * T::MD + e;
#pragma unroll
    for (int n = 0; n < N; ++n) {
      const float d_w1 = (dh * qv[reg][n]) * sign_f32(a[n][reg]);
      if (live) out[kE * n] = d_w1;
      const float sq = lrn_sum16(dh * __builtin_fabsf(a[n][reg]));
      if (col == 0) partq[w][r][n] = sq;
    }
    if (live) {
      out[kE * N] = dh;
      out[kE * (N + 1)] = d_wf;
      out[kE * (N + 2)] = d_l1;
      out[kE * (N + 3)] = p_bf;
    }
  }
  __syncthreads();
  if (tid < kRows * N) {
    const int r = tid / N, n = tid - r * N;
    const uint32_t hr = row_base + r;
    if (hr < rows) p.dqs[(size_t)hr * N + n] = ((partq[0][r][n] + partq[1][r][n]) + partq[2][r][n]) + partq[3][r][n];
  }
  for (int idx = tid; idx < kRows * T::KMP; idx += 256) {
    const int r = idx / T::KMP, k = idx - r * T::KMP;
    const uint32_t hr = row_base + r;
    if (hr < rows) p.xm[(size_t)hr * T::KMP + k] = xs[r][k];
  }
}

// ---- 3. the agent network's deltas ------------------------------------------------------------------------------------------------
struct AgentBwdParams {
  size_t n_rows;
  const int32_t *actions;
  const float *dqs, *h1, *h2, *w2, *wo;
  float *dq16, *dh2, *dh1;                 // [R][16], [R][64], [R][64]
};

__global__ void CM3_MATRIX_KERNEL k_learner_agent_bwd(const AgentBwdParams p) {
  constexpr int HS = kH + 2;
  __shared__ float d2s[64][HS];
  const int tid = threadIdx.x, lane = tid & 63, col = lane & 15, hi = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const size_t rows = p.n_rows;
  const size_t row_base = (size_t)blockIdx.x * 64;
  float bw[kH / 4];                        // B[k = v][j = u] = h2/kernel[u = 16 w + col][v = 4 s + hi]
#pragma unroll
  for (int s = 0; s < kH / 4; ++s) bw[s] = p.w2[(16 * w + col) * kH + 4 * s + hi];
  for (int idx = tid; idx < 64 * kH; idx += 256) {
    const int r = idx >> 6, u = idx & 63;
    const size_t gr = row_base + r;
    const size_t rc = gr < rows ? gr : rows - 1;
    const int act = p.actions[rc];
    const bool ok = gr < rows && act >= 0 && act < kA;
    const float g = p.dqs[rc], hv = p.h2[rc * kH + u];
    const float v = (ok && hv > 0.0f) ? g * p.wo[u * kA + (ok ? act : 0)] : 0.0f;
    d2s[r][u] = v;
    if (gr < rows) p.dh2[gr * kH + u] = v;
  }
  for (int idx = tid; idx < 64 * 16; idx += 256) {
    const int r = idx >> 4, j = idx & 15;
    const size_t gr = row_base + r;
    if (gr < rows) p.dq16[gr * 16 + j] = p.actions[gr] == j ? p.dqs[gr] : 0.0f;
  }
  __syncthreads();
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int s = 0; s < kH / 4; ++s)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(d2s[16 * t + col][4 * s + hi], bw[s], acc[t], 0, 0, 0);
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const size_t gr = row_base + 16 * t + 4 * hi + reg;
      if (gr < rows) {
        const size_t at = gr * kH + 16 * w + col;
        p.dh1[at] = p.h1[at] > 0.0f ? acc[t][reg] : 0.0f;
      }
    }
}

template <int N> static int grad_launch(const cm3_qmix_learner_tensors *wt, const cm3_qmix_learner_tensors *g, const cm3_qmix_learner_rows *r,
                                        float *ws, hipStream_t s) {
  using T = LL<N>;
  const size_t B = (size_t)r->n_steps, R = B * N;
  const Ws o = ws_layout<N>(B);
  const unsigned row_blocks = (unsigned)((R + 63) / 64);
  {
    AgentFwdParams p = {R, r->obs_others, r->v_obs, r->goals, r->actions, wt->h_kernel, wt->h_bias, wt->h2_kernel, wt->h2_bias, wt->out_kernel,
                        wt->out_bias, ws + o.xa, ws + o.h1, ws + o.h2, ws + o.qsel};
    hipLaunchKernelGGL((k_learner_agent_fwd<N>), dim3(row_blocks), dim3(256), 0, s, p);
  }
  {
    MixParams p = {(uint32_t)B, r->td_f64, r->state, r->goals, ws + o.qsel, r->td, wt->hyper_w_1, wt->hyper_w_final, wt->hyper_b_1,
                   wt->hyper_b_final_l1, wt->hyper_b_final, r->q_tot, ws + o.err2, ws + o.xm, ws + o.dhy, ws + o.dqs};
    hipLaunchKernelGGL((k_learner_mixer<N>), dim3((unsigned)((B + 15) / 16)), dim3(256), 0, s, p);
  }
  {
    AgentBwdParams p = {R, r->actions, ws + o.dqs, ws + o.h1, ws + o.h2, wt->h2_kernel, wt->out_kernel, ws + o.dq16, ws + o.dh2, ws + o.dh1};
    hipLaunchKernelGGL(k_learner_agent_bwd, dim3(row_blocks), dim3(256), 0, s, p);
  }
  XtdParams<4> x;
  RedParams<4> d;
  memset(&x, 0, sizeof(x));
  memset(&d, 0, sizeof(d));
  unsigned blocks = 0, elems = 0;
  auto job = [&](int i, const float *X, int ldx, int Kx, const float *D, int ldd, size_t rows, size_t chunks, float *P) {
    learner_job(x.job[i], d.job[i], blocks, elems, X, ldx, Kx, D, ldd, rows, chunks, P);
  };
  job(0, ws + o.xa, T::K1P, T::K1, ws + o.dh1, kH, R, o.chunks_a, ws + o.p1);
  job(1, ws + o.h1, kH, kH, ws + o.dh2, kH, R, o.chunks_a, ws + o.p2);
  job(2, ws + o.h2, kH, kH, ws + o.dq16, 16, R, o.chunks_a, ws + o.po);
  job(3, ws + o.xm, T::KMP, T::KM, ws + o.dhy, T::MD, B, o.chunks_m, ws + o.ph);
  d.job[0].nseg = 1; d.job[0].seg[0] = RedSeg{0, kH, g->h_kernel, g->h_bias};
  d.job[1].nseg = 1; d.job[1].seg[0] = RedSeg{0, kH, g->h2_kernel, g->h2_bias};
  d.job[2].nseg = 1; d.job[2].seg[0] = RedSeg{0, kA, g->out_kernel, g->out_bias};
  d.job[3].nseg = 5;
  d.job[3].seg[0] = RedSeg{0, kE * N, g->hyper_w_1, nullptr};
  d.job[3].seg[1] = RedSeg{kE * N, kE, g->hyper_b_1, nullptr};
  d.job[3].seg[2] = RedSeg{kE * (N + 1), kE, g->hyper_w_final, nullptr};
  d.job[3].seg[3] = RedSeg{kE * (N + 2), kE, g->hyper_b_final_l1, nullptr};
  d.job[3].seg[4] = RedSeg{kE * (N + 3), kE, nullptr, g->hyper_b_final};
  d.total = elems;
  d.B = (uint32_t)B;
  d.err2 = ws + o.err2;
  d.loss = r->loss;
  hipLaunchKernelGGL(k_learner_xtd<4>, dim3(blocks), dim3(256), 0, s, x);
  note_variant("k_qmix_learner_reduce", (int)sizeof(float), N, 4, 0, 0, 0, 0, 0, 0, /* prec=f32 */ 0);
  note_tail(",after=fwd+mixer+bwd+xtd");   // (the four launches before it: k_learner_agent_fwd, _mixer, _agent_bwd, _xtd)
  hipLaunchKernelGGL(k_learner_reduce<4>, dim3((elems + 255u) / 256u + 1u), dim3(256), 0, s, d);
  CM3_HIP_CHECK(hipGetLastError());
  return CM3_OK;
}

static size_t ws_floats_for(int n, int64_t n_steps) {   // (0 for an agent count outside 1..10 or a batch out of range)
  if (n_steps <= 0 || n_steps > (int64_t)0x7fffffff / CM3_MAX_AGENTS) return 0;
  bool hit;
  return agent_dispatch_1_to_10(n, hit, [&](auto k) { return ws_layout<k()>((size_t)n_steps).total; });
}

static bool all_set(const cm3_qmix_learner_tensors *t) {
  return t->h_kernel && t->h_bias && t->h2_kernel && t->h2_bias && t->out_kernel && t->out_bias && t->hyper_w_1 && t->hyper_w_final &&
         t->hyper_b_1 && t->hyper_b_final_l1 && t->hyper_b_final;
}

// ---- Adam ------------------------------------------------------------------------------------------------------------------------
struct AdamParams {
  float lr, beta1, beta2, epsilon;
  int n_segments;
  uint32_t *state;                // {beta1_power, beta2_power, arrivals, 0}
};

__global__ void __launch_bounds__(256) k_adam_step(const AdamParams p, const cm3_adam_segment *segs) {
  __shared__ float pw[2];
  const int tid = threadIdx.x;
  unsigned long long *both = reinterpret_cast<unsigned long long *>(p.state);
  if (tid == 0) {
    const unsigned long long v = __hip_atomic_load(both, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    pw[0] = __builtin_bit_cast(float, (uint32_t)v);
    pw[1] = __builtin_bit_cast(float, (uint32_t)(v >> 32));
  }
  __syncthreads();
  const float b1p = pw[0], b2p = pw[1];
  const float lr_t = (p.lr * sqrtf(1.0f - b2p)) / (1.0f - b1p);
  const float c1 = 1.0f - p.beta1, c2 = 1.0f - p.beta2;
  for (int s = 0; s < p.n_segments; ++s) {
    const cm3_adam_segment g = segs[s];
    for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < g.count; i += (int64_t)gridDim.x * 256) {
      const float gr = g.grad[i];
      const float m = p.beta1 * g.m[i] + c1 * gr;
      const float v = p.beta2 * g.v[i] + c2 * (gr * gr);
      g.m[i] = m;
      g.v[i] = v;
      g.var[i] = g.var[i] - (lr_t * m) / (sqrtf(v) + p.epsilon);
    }
  }
  if (tid == 0) {
    const uint32_t old = __hip_atomic_fetch_add(p.state + 2, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (old == gridDim.x - 1) {
      const unsigned long long nv = (unsigned long long)__builtin_bit_cast(uint32_t, b1p * p.beta1) |
                                    ((unsigned long long)__builtin_bit_cast(uint32_t, b2p * p.beta2) << 32);
      __hip_atomic_store(both, nv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(p.state + 2, 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

}  // namespace learner
}  // namespace cm3

extern "C" size_t cm3_qmix_learner_particle_workspace_bytes(int32_t n_agents, int64_t n_steps) {
  return cm3::learner::ws_floats_for(n_agents, n_steps) * sizeof(float);
}

extern "C" int cm3_qmix_learner_particle_grad_f32(const cm3_qmix_learner_particle_desc *d, const cm3_qmix_learner_tensors *weights,
                                                  const cm3_qmix_learner_tensors *grads, const cm3_qmix_learner_rows *r, void *workspace,
                                                  size_t workspace_bytes, void *stream) {
  using namespace cm3;
  using namespace cm3::learner;
  CM3_REQUIRE(d, "null desc");
  CM3_REQUIRE(d->n_agents >= 1 && d->n_agents <= CM3_MAX_AGENTS, "n_agents must be in 1..%d", CM3_MAX_AGENTS);
  CM3_REQUIRE(d->n_h == kH && d->n_actions == kA, "the QMIX agent network is 64/64/5 (networks.Qmix_single_particle): n_h, n_actions; got %d/%d",
              d->n_h, d->n_actions);
  CM3_REQUIRE(d->embed_dim == kE, "the supported embedding width of Qmix_mixer is %d (networks.py:650); got %d", kE, d->embed_dim);
  CM3_REQUIRE(weights, "null weights");
  CM3_REQUIRE(grads, "null grads");
  CM3_REQUIRE(r, "null rows");
  CM3_REQUIRE(all_set(weights), "missing weights: the six Agent_main and five Mixer_main tensors are all required");
  CM3_REQUIRE(all_set(grads), "missing gradients: one tensor per weight is required");
  CM3_REQUIRE(r->obs_others && r->v_obs && r->goals && r->actions && r->state && r->td,
              "missing inputs: obs_others, v_obs, goals, actions, state and td are all required");
  CM3_REQUIRE(r->loss && r->q_tot, "missing outputs: loss and q_tot are required");
  CM3_REQUIRE(workspace, "workspace is NULL: cm3_qmix_learner_particle_workspace_bytes(n_agents, n_steps) bytes of device memory");
  CM3_REQUIRE((uintptr_t)r->obs_others % 16 == 0 && (uintptr_t)r->v_obs % 16 == 0 && (uintptr_t)r->state % 16 == 0 &&
                  (uintptr_t)r->goals % 8 == 0 && (uintptr_t)r->actions % 4 == 0 && (uintptr_t)r->td % (r->td_f64 ? 8 : 4) == 0,
              "misaligned inputs: obs_others, v_obs and state must be 16-byte aligned, goals 8-byte aligned, actions 4-byte, td as its type");
  CM3_REQUIRE((uintptr_t)r->loss % 4 == 0 && (uintptr_t)r->q_tot % 4 == 0, "misaligned outputs: loss and q_tot must be 4-byte aligned");
  CM3_REQUIRE((uintptr_t)workspace % 16 == 0, "misaligned workspace: must be 16-byte aligned");
  CM3_REQUIRE(r->n_steps > 0, "n_steps must be positive");
  CM3_REQUIRE(r->n_steps <= (int64_t)0x7fffffff / CM3_MAX_AGENTS, "n_steps %lld is more than (2^31 - 1) / %d", (long long)r->n_steps,
              CM3_MAX_AGENTS);
  const size_t need = ws_floats_for(d->n_agents, r->n_steps) * sizeof(float);
  CM3_REQUIRE(workspace_bytes >= need, "workspace of %zu bytes is too small: %d agents and %lld steps take %zu", workspace_bytes, d->n_agents,
              (long long)r->n_steps, need);
  hipStream_t s = (hipStream_t)stream;
  return agent_launch_1_to_10(d->n_agents, [&](auto n) { return grad_launch<n()>(weights, grads, r, (float *)workspace, s); });
}

extern "C" int cm3_adam_step_f32(const cm3_adam_desc *d, const cm3_adam_segment *segments, void *state, void *stream) {
  using namespace cm3;
  using namespace cm3::learner;
  CM3_REQUIRE(d, "null desc");
  CM3_REQUIRE(d->lr == d->lr && d->beta1 >= 0.0f && d->beta1 < 1.0f && d->beta2 >= 0.0f && d->beta2 < 1.0f && d->epsilon > 0.0f,
              "Adam takes a learning rate that is a number, beta1 and beta2 in [0, 1) and a positive epsilon; got %g, %g, %g, %g", (double)d->lr,
              (double)d->beta1, (double)d->beta2, (double)d->epsilon);
  CM3_REQUIRE(d->n_segments >= 1, "n_segments must be positive");
  CM3_REQUIRE(segments, "segments is NULL: a device array of n_segments cm3_adam_segment");
  CM3_REQUIRE(state, "state is NULL: 16 bytes of device memory {beta1_power, beta2_power, 0, 0}");
  CM3_REQUIRE((uintptr_t)segments % 8 == 0 && (uintptr_t)state % 8 == 0, "misaligned segments or state: must be 8-byte aligned");
  CM3_REQUIRE(d->total > 0, "total must be positive: the sum of the segments' counts");
  const int64_t want = (d->total + 255) / 256;
  const unsigned blocks = (unsigned)(want < 1024 ? want : 1024);
  const AdamParams p = {d->lr, d->beta1, d->beta2, d->epsilon, d->n_segments, (uint32_t *)state};
  note_variant("k_adam_step", (int)sizeof(float), 0, 4, 0, 0, 0, 0, 0, 0, /* prec=f32 */ 0);
  hipLaunchKernelGGL(k_adam_step, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, segments);
  CM3_HIP_CHECK(hipGetLastError());
  return CM3_OK;
}
