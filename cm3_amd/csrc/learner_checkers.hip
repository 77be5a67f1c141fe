// The Checkers QMIX learner (part of ABI 9, additive): mixer_op of alg_qmix_checkers.py:184-190, 381-391 -- the loss and the dense
// float32 gradients of the thirteen Agent_main and the seven Mixer_main variables -- for 1..8 agents.  cm3_adam_step_f32 (learner.hip)
// applies them over a 20-segment table.
//   agent rows r = (b, n), R = B N     networks.Qmix_single_checkers (networks.py:617-637)
//     c1 = relu(conv3x3 SAME(window) + b) [150]   lin = relu(c1 . conv_linear + b) [32]   xs = concat(lin, obs_self_v, 1hot(a_prev), goal) [43]
//     hs = relu(xs . branch_self + b)   ho = relu(obs_others . branch_others + b)   h2 = relu(hs . W_self_h2 + ho . W_others_h2 + b)
//     Q = h2 . Qmix_single_out + b   q_sel = Q[action[r]]
//   transitions b                      networks.Qmix_mixer_checkers (networks.py:688-734)
//     xm = concat(relu(conv3x5 SAME(grid) + b) [108], vec [4N], goals [2N])   q_tot = mixer(q_sel[b][0..N), xm)
//     loss = mean_b((float32(td[b]) - q_tot[b])^2)
// cm3_qmix_learner_checkers_grad_f32 is FOURTEEN launches on one stream, every one capturable; all scratch is the caller's workspace
// (cm3_qmix_learner_checkers_workspace_bytes).  Every matrix product is k_lck_gemm, one wave per 16 x 16 output tile on the exact-f32
// matrix instruction (v_mfma_f32_16x16x4_f32); the unit is built with -ffp-contract=off.  The weights are read as TensorFlow shapes
// them, the convolutions as Toeplitz matrices made on the fly (ck_tiles.h: toeplitz); no packed copy is read, so the launches follow
// the tensors as they are at launch.  A forward product issues the instructions of gemm_tiles (ck_tiles.h) on the same operands --
// a chain from zero over k groups of 16, instruction j of a group contracting inputs {16 g + 4 h + j : h = 0..3}, the bias added
// after the chain -- so q_sel has the bits of k_ck_actor's rows form at precision f32 and q_tot those of k_ck_qmix_mixer_rows.
//    1. k_lck_stage     the columns as float32 in the workspace (each value rounded as it is read): windows [R][80], their 3 x 3 patches
//                       [25 R][27], the concat tail, obs_others [R][16], grids [B][64], their 3 x 5 patches [27 B][30], vec and goals in xm;
//                       zeros for every pad and for the two convolution delta arrays
//    2. k_lck_gemm      both convolutions: c1 [R][160], xm[:, 0:108]
//    3. k_lck_gemm      conv_linear -> xs[:, 0:32]
//    4. k_lck_gemm      branch_self -> hs, branch_others -> ho (input k of the others group sits at position 4 (k & 3) + (k >> 2), as in the
//                       rows kernel: instruction j contracts inputs 4 j .. 4 j + 3)
//    5. k_lck_gemm      h2: one chain over hs . W_self_h2 then ho . W_others_h2, + b
//    6. k_lck_gemm      Qmix_single_out -> Q [R][16] (columns 5..15 zero)
//    7. k_lck_gemm      the hyper-network: xm . (hyper_w_1 | hyper_b_1 | hyper_w_final | hyper_b_final_l1) -> hy [B][128 (N + 3)]
//    8. k_lck_mixer     128 threads per transition, thread e one embedding unit: the sums after the hyper-network in the order of
//                       k_ck_qmix_mixer_rows (the chain over agents; over e pairwise inside every 16 units by DPP moves, then the eight
//                       sixteens left to right), q_tot, err2, and per row
//                         dq = (2 (q_tot - td)) / B
//                         d l1_pre = l1_pre > 0 ? dq hyper_b_final[e] : 0    (ReluGrad)      p_bf = dq l1[e]
//                         d wf_pre = dq hidden[e] sign(wf_pre[e])            (sign(0) = 0)
//                         dh = dq |wf_pre[e]| (h > 0 ? 1 : hidden[e] + 1)    (EluGrad: elu + 1 below zero)
//                         d w1_pre[n][e] = dh q_sel[n] sign(w1_pre[n][e])    d q_sel[n] = sum_e dh[e] |w1_pre[n][e]|  (the same tree)
//                       -> the delta rows dhy [B][128 (N + 4)] and d Q [R][16] (d q_sel at the taken action)
//    9. k_lck_gemm      d conv_m = [xm > 0] dhy . (the four hyper matrices)^T -> [27 B][16] (4 filters per position);
//                       d h2_pre = [h2 > 0] d Q . out^T
//   10. k_lck_gemm      d hs_pre = [hs > 0] d h2_pre . W_self_h2^T;   d ho_pre = [ho > 0] d h2_pre . W_others_h2^T
//   11. k_lck_gemm      d lin_pre = [lin > 0] d hs_pre . branch_self^T (the first 32 inputs)
//   12. k_lck_gemm      d c1_pre = [c1 > 0] d lin_pre . conv_linear^T -> [25 R][16] (6 filters per position)
//   13. k_learner_xtd<9> (learner_common.h) the weight gradients X^T . Delta per chunk of 256 rows, nine jobs: the agent convolution
//                       (patches x d c1_pre, contracted over (row, position)), conv_linear, branch_self, branch_others, W_self_h2 (+ b),
//                       W_others_h2, Qmix_single_out, the mixer convolution (patches x d conv_m), the hyper-network (xm x dhy)
//   14. k_learner_reduce<9> the chunks in ascending order, stored TF-shaped; the loss
// [x > 0] passes where the stored activation is > 0, which is where the pre-activation is (ReluGrad: exactly 0 passes nothing).  No
// floating-point atomics anywhere; tiles and chunks are cut by the row count alone, so two calls on the same inputs give the same bits.
#include "actor_common.h"
#include "agent_dispatch.h"
#include "ck_tiles.h"
#include "learner_common.h"

namespace cm3 {
namespace lck {

using namespace cm3::learner;

constexpr int kMaxAgents = 8;
constexpr int kObs = 75, kX0 = 80, kC1 = 160, kC1R = 150, kLin = 32, kXs = 48, kCat = 43, kXo = 16, kH = 256, kQ = 16;
constexpr int kPatA = 27, kPosA = 25, kFA = 6;          // agent convolution: 27 inputs per position, 25 positions, 6 filters
constexpr int kGrid = 54, kGm = 64, kConvM = 108, kPatM = 30, kPosM = 27, kFM = 4, kE = 128;
constexpr int64_t kMaxSteps = (int64_t)0x7fffffff / (kMaxAgents * kPosM);   // every row index of every array stays in int32

static inline size_t up4(size_t x) { return (x + 3) / 4 * 4; }
static inline int kp_of(int N) { return (kConvM + 6 * N + 15) / 16 * 16; }

// the workspace, in floats; every part starts at a multiple of four
struct Ws {
  size_t x0, pa, c1, xs, xo, hs, ho, h2, q, dq, dh2, dhs, dho, dlin, dca, gm, pm, xm, hy, dhy, dcm, err2, part[9], total;
  size_t chunks_r, chunks_ra, chunks_b, chunks_bm;
};
static Ws ws_layout(int N, size_t B) {
  const size_t R = B * N;
  const int KP = kp_of(N), KM = kConvM + 6 * N, Lo = 2 * (N > 1 ? N - 1 : 1);
  Ws w;
  w.chunks_r = (R + kChunk - 1) / kChunk;
  w.chunks_ra = (R * kPosA + kChunk - 1) / kChunk;
  w.chunks_b = (B + kChunk - 1) / kChunk;
  w.chunks_bm = (B * kPosM + kChunk - 1) / kChunk;
  size_t o = 0;
  auto take = [&](size_t n) { const size_t at = o; o += up4(n); return at; };
  w.x0 = take(R * kX0);
  w.pa = take(R * kPosA * kPatA);
  w.c1 = take(R * kC1);
  w.xs = take(R * kXs);
  w.xo = take(R * kXo);
  w.hs = take(R * kH);
  w.ho = take(R * kH);
  w.h2 = take(R * kH);
  w.q = take(R * kQ);
  w.dq = take(R * kQ);
  w.dh2 = take(R * kH);
  w.dhs = take(R * kH);
  w.dho = take(R * kH);
  w.dlin = take(R * kLin);
  w.dca = take(R * kPosA * 16);
  w.gm = take(B * kGm);
  w.pm = take(B * kPosM * kPatM);
  w.xm = take(B * KP);
  w.hy = take(B * (size_t)(kE * (N + 3)));
  w.dhy = take(B * (size_t)(kE * (N + 4)));
  w.dcm = take(B * kPosM * 16);
  w.err2 = take(B);
  w.part[0] = take(learner_partial_floats(w.chunks_ra, kPatA, 16));
  w.part[1] = take(learner_partial_floats(w.chunks_r, kC1R, kLin));
  w.part[2] = take(learner_partial_floats(w.chunks_r, kCat, kH));
  w.part[3] = take(learner_partial_floats(w.chunks_r, Lo, kH));
  w.part[4] = take(learner_partial_floats(w.chunks_r, kH, kH));
  w.part[5] = take(learner_partial_floats(w.chunks_r, kH, kH));
  w.part[6] = take(learner_partial_floats(w.chunks_r, kH, kQ));
  w.part[7] = take(learner_partial_floats(w.chunks_bm, kPatM, 16));
  w.part[8] = take(learner_partial_floats(w.chunks_b, KM, kE * (N + 4)));
  w.total = o;
  return w;
}

// ---- 1. the columns as float32 ------------------------------------------------------------------------------------------------------
struct StageParams {
  size_t R, B;
  int N, Lo, KP, t_f64, g_f64, goals_onehot;
  const void *obs_self_t, *grid, *goals;
  const double *obs_self_v, *obs_others, *vec;
  const int32_t *actions_prev;
  float *x0, *pa, *xs, *xo, *gm, *pm, *xm, *dca, *dcm;
};

__device__ __forceinline__ float lck_cell(const void *p, int f64, size_t at) {
  return f64 ? (float)reinterpret_cast<const double *>(p)[at] : (float)reinterpret_cast<const int8_t *>(p)[at];
}
__device__ __forceinline__ float lck_goal(const void *p, int onehot, size_t row, int k) {
  if (onehot) return (float)reinterpret_cast<const int64_t *>(p)[row * 2 + k];
  const int gl = reinterpret_cast<const uint8_t *>(p)[row];
  return (gl == 0) == (k == 0) ? 1.0f : 0.0f;
}

__global__ void __launch_bounds__(256) k_lck_stage(const StageParams p) {
  const size_t t0 = (size_t)blockIdx.x * 256 + threadIdx.x, step = (size_t)gridDim.x * 256;
  const size_t R = p.R, B = p.B;
  const int N = p.N;
  for (size_t i = t0; i < R * kX0; i += step) {
    const size_t r = i / kX0;
    const int k = (int)(i - r * kX0);
    p.x0[i] = k < kObs ? lck_cell(p.obs_self_t, p.t_f64, r * kObs + k) : 0.0f;
  }
  for (size_t i = t0; i < R * kPosA * kPatA; i += step) {      // patch (row, position (ro, co)), input (dr, dc, ch): SAME zero padding
    const size_t rp = i / kPatA, r = rp / kPosA;
    const int k = (int)(i - rp * kPatA), pos = (int)(rp - r * kPosA);
    const int ch = k % 3, dc = (k / 3) % 3, dr = k / 9, ri = pos / 5 + dr - 1, ci = pos % 5 + dc - 1;
    p.pa[i] = (ri >= 0 && ri < 5 && ci >= 0 && ci < 5) ? lck_cell(p.obs_self_t, p.t_f64, r * kObs + (ri * 5 + ci) * 3 + ch) : 0.0f;
  }
  for (size_t i = t0; i < R * (kXs - kLin); i += step) {        // concat tail: v_obs_self (4), a_prev one-hot (5), v_goal (2), pad (5)
    const size_t r = i / (kXs - kLin);
    const int k = (int)(i - r * (kXs - kLin));
    float v = 0.0f;
    if (k < 4) v = (float)p.obs_self_v[r * 4 + k];
    else if (k < 9) v = p.actions_prev[r] == k - 4 ? 1.0f : 0.0f;
    else if (k < 11) v = lck_goal(p.goals, p.goals_onehot, r, k - 9);
    p.xs[r * kXs + kLin + k] = v;
  }
  for (size_t i = t0; i < R * kXo; i += step) {
    const size_t r = i / kXo;
    const int k = (int)(i - r * kXo);
    p.xo[i] = k < p.Lo ? (float)p.obs_others[r * p.Lo + k] : 0.0f;
  }
  for (size_t i = t0; i < B * kGm; i += step) {
    const size_t b = i / kGm;
    const int k = (int)(i - b * kGm);
    p.gm[i] = k < kGrid ? lck_cell(p.grid, p.g_f64, b * kGrid + k) : 0.0f;
  }
  for (size_t i = t0; i < B * kPosM * kPatM; i += step) {      // 3 x 5 patches of the 3 x 9 x 2 grid
    const size_t bp = i / kPatM, b = bp / kPosM;
    const int k = (int)(i - bp * kPatM), pos = (int)(bp - b * kPosM);
    const int ch = k % 2, dc = (k / 2) % 5, dr = k / 10, ri = pos / 9 + dr - 1, ci = pos % 9 + dc - 2;
    p.pm[i] = (ri >= 0 && ri < 3 && ci >= 0 && ci < 9) ? lck_cell(p.grid, p.g_f64, b * kGrid + (ri * 9 + ci) * 2 + ch) : 0.0f;
  }
  const int tail = p.KP - kConvM;
  for (size_t i = t0; i < B * tail; i += step) {                // xm behind the convolution: vec [4N], goals [2N], pad
    const size_t b = i / tail;
    const int k = (int)(i - b * tail);
    float v = 0.0f;
    if (k < 4 * N) v = (float)p.vec[b * 4 * N + k];
    else if (k < 6 * N) v = lck_goal(p.goals, p.goals_onehot, b * N + ((k - 4 * N) >> 1), (k - 4 * N) & 1);
    p.xm[b * p.KP + kConvM + k] = v;
  }
  for (size_t i = t0; i < R * kPosA * 16; i += step) p.dca[i] = 0.0f;
  for (size_t i = t0; i < B * kPosM * 16; i += step) p.dcm[i] = 0.0f;
}

// ---- the matrix product of every layer, forward and backward ------------------------------------------------------------------------
// C[row][n] = epilogue(sum over the job's segments, in order, of A[row][k] B[k][n]): one wave per 16 x 16 tile, the chain of gemm_tiles.
enum { kBPlain = 0, kBTrans = 1, kBConvA = 2, kBConvM = 3 };
enum { kActNone = 0, kActRelu = 1, kActMask = 2 };
struct GemmSeg {
  const float *A, *Bm;
  int lda, ldb, K, KG;            // A and B are read for k < K (zero operands past it); KG groups of 16 are issued
  int bmode, perm;                // B[k][n]: Bm[k ldb + n] / Bm[n ldb + k] / a Toeplitz element;  perm: position 4 h + j holds input 4 j + h
};
struct GemmJob {
  GemmSeg seg[4];
  int nseg, Nreal, CT, act, ldm, ldc, cf, bias_mod;   // columns n < Nreal are real (others: zero operands, zero bias) and stored ...
  int Nstore;                                         // ... together with the pad columns up to Nstore
  size_t rows;
  const float *bias, *M;          // optional bias[n] (bias[n % bias_mod] with bias_mod > 0); kActMask passes where M[row ldm + n] > 0
  float *C;                       // C[row ldc + n], or with cf > 0 the convolution's rows: C[(row (Nreal / cf) + n / cf) 16 + n % cf]
  unsigned block0;
};
template <int NJ> struct GemmParams {
  GemmJob job[NJ];
};

template <int NJ> __global__ void CM3_MATRIX_KERNEL k_lck_gemm(const GemmParams<NJ> p) {
  const int tid = threadIdx.x, lane = tid & 63, col = lane & 15, hi = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int ji = 0;
#pragma unroll
  for (int i = 1; i < NJ; ++i) ji = blockIdx.x >= p.job[i].block0 ? i : ji;
  const GemmJob &J = p.job[ji];
  const unsigned tile = (blockIdx.x - J.block0) * 4u + (unsigned)w;
  const unsigned row_tiles = (unsigned)((J.rows + 15) / 16);
  if (tile >= row_tiles * (unsigned)J.CT) return;
  const unsigned rt = tile / (unsigned)J.CT;
  const int ct = (int)(tile - rt * (unsigned)J.CT);
  const int n = 16 * ct + col;
  const bool n_ok = n < J.Nreal;
  const size_t arow = (size_t)rt * 16 + col;
  const size_t arc = arow < J.rows ? arow : J.rows - 1;         // rows past the count repeat the last one; nothing of them is stored
  f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  for (int s = 0; s < J.nseg; ++s) {
    const GemmSeg &S = J.seg[s];
    const float *a = S.A + arc * (size_t)S.lda;
    for (int g = 0; g < S.KG; ++g) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = 16 * g + (S.perm ? 4 * j + hi : 4 * hi + j);
        const bool k_ok = k < S.K;
        const float av = k_ok ? a[k] : 0.0f;
        float bv = 0.0f;
        if (k_ok && n_ok) {
          if (S.bmode == kBPlain) bv = S.Bm[(size_t)k * S.ldb + n];
          else if (S.bmode == kBTrans) bv = S.Bm[(size_t)n * S.ldb + k];
          else if (S.bmode == kBConvA) bv = toeplitz<5, 5, 3, kFA, 3, 3>(S.Bm, k, n);
          else bv = toeplitz<3, 9, 2, kFM, 3, 5>(S.Bm, k, n);
        }
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
      }
    }
  }
  if (n >= J.Nstore) return;
  const float bias = (J.bias != nullptr && n_ok) ? J.bias[J.bias_mod > 0 ? n % J.bias_mod : n] : 0.0f;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const size_t row = (size_t)rt * 16 + 4 * hi + reg;
    if (row >= J.rows) continue;
    float v = acc[reg] + bias;
    if (J.act == kActRelu) v = fmaxf(v, 0.0f);
    else if (J.act == kActMask) v = J.M[row * (size_t)J.ldm + n] > 0.0f ? v : 0.0f;
    if (J.cf > 0) {
      if (n_ok) J.C[(row * (size_t)(J.Nreal / J.cf) + (size_t)(n / J.cf)) * 16 + n % J.cf] = v;
    } else {
      J.C[row * (size_t)J.ldc + n] = v;
    }
  }
}

// ---- 8. the mixer behind the hyper-network: forward sums, loss terms, deltas --------------------------------------------------------
struct MixParams {
  uint32_t B;
  int td_f64;
  const float *hy, *q, *bf;          // [B][128 (N + 3)] pre-activations, Q [R][16], hyper_b_final/kernel [128]
  const int32_t *actions;
  const void *td;
  float *q_tot, *err2, *dhy, *dq;    // [B], [B], [B][128 (N + 4)], [R][16]
};

// the sum over the 128 units of thread e's value: the tree of k_ck_qmix_mixer_rows.  Every thread returns the sum.
__device__ __forceinline__ float lck_sum128(float v, float *part, int e) {
  const float s16 = lrn_sum16(v);
  __syncthreads();                   // (the previous sum's readers are done with part)
  if ((e & 15) == 0) part[e >> 4] = s16;
  __syncthreads();
  float s = part[0] + part[1];
#pragma unroll
  for (int j = 2; j < 8; ++j) s = s + part[j];
  return s;
}

template <int N> __global__ void __launch_bounds__(128) k_lck_mixer(const MixParams p) {
  __shared__ float part[8];
  __shared__ float qs[N];
  __shared__ int acts[N];
  const int e = threadIdx.x;
  const size_t b = blockIdx.x;
  if (e < N) {
    const int act = p.actions[b * N + e];
    const bool ok = act >= 0 && act < kA;
    acts[e] = ok ? act : -1;
    qs[e] = ok ? p.q[(b * N + e) * kQ + act] : 0.0f;     // an action outside 0..4 selects nothing
  }
  __syncthreads();
  const float *hy = p.hy + b * (size_t)(kE * (N + 3));
  float a[N], t = 0.0f;
#pragma unroll
  for (int n = 0; n < N; ++n) {
    a[n] = hy[kE * n + e];
    const float term = qs[n] * __builtin_fabsf(a[n]);
    t = n == 0 ? term : t + term;
  }
  const float b1 = hy[kE * N + e], wf = hy[kE * (N + 1) + e], l1 = hy[kE * (N + 2) + e], bf = p.bf[e];
  const float h = t + b1;
  const float hidden = h > 0.0f ? h : expm1f(h);
  const float sp = lck_sum128(hidden * __builtin_fabsf(wf), part, e);
  const float sc = lck_sum128(relu_f32(l1) * bf, part, e);
  const float q = sp + sc;
  // the td_target placeholder is tf.float32: a float64 target is rounded as it is read
  const float td = p.td_f64 ? (float)reinterpret_cast<const double *>(p.td)[b] : reinterpret_cast<const float *>(p.td)[b];
  if (e == 0) {
    const float d = td - q;
    p.q_tot[b] = q;
    p.err2[b] = d * d;
  }
  const float dq = (2.0f * (q - td)) / (float)p.B;
  const float d_l1 = l1 > 0.0f ? dq * bf : 0.0f;
  const float p_bf = dq * relu_f32(l1);
  const float d_wf = (dq * hidden) * sign_f32(wf);
  const float dhid = dq * __builtin_fabsf(wf);
  const float dh = h > 0.0f ? dhid : dhid * (hidden + 1.0f);
  float *out = p.dhy + b * (size_t)(kE * (N + 4)) + e;
  float dqs[N];
#pragma unroll
  for (int n = 0; n < N; ++n) {
    out[kE * n] = (dh * qs[n]) * sign_f32(a[n]);
    dqs[n] = lck_sum128(dh * __builtin_fabsf(a[n]), part, e);
  }
  out[kE * N] = dh;
  out[kE * (N + 1)] = d_wf;
  out[kE * (N + 2)] = d_l1;
  out[kE * (N + 3)] = p_bf;
  // d Q of the N agent rows: d q_sel at the taken action, zero elsewhere; thread (n, j) = (e >> 4, e & 15)
#pragma unroll
  for (int n = 0; n < N; ++n)
    if ((e >> 4) == n) p.dq[(b * N + n) * kQ + (e & 15)] = (e & 15) == acts[n] ? dqs[n] : 0.0f;
}

// ---- the launches ---------------------------------------------------------------------------------------------------------------------
static GemmSeg seg(const float *A, int lda, const float *Bm, int ldb, int K, int bmode, int perm = 0) {
  GemmSeg s;
  s.A = A; s.Bm = Bm; s.lda = lda; s.ldb = ldb; s.K = K; s.KG = (K + 15) / 16; s.bmode = bmode; s.perm = perm;
  return s;
}
static GemmJob gjob(size_t rows, int Nreal, int Nstore, const float *bias, int bias_mod, int act, const float *M, int ldm, float *C, int ldc,
                    int cf, GemmSeg s0) {
  GemmJob j;
  memset(&j, 0, sizeof(j));
  j.seg[0] = s0; j.nseg = 1; j.Nreal = Nreal; j.Nstore = Nstore; j.CT = ((Nstore > Nreal ? Nstore : Nreal) + 15) / 16; j.act = act; j.ldm = ldm;
  j.ldc = ldc; j.cf = cf; j.bias_mod = bias_mod; j.rows = rows; j.bias = bias; j.M = M; j.C = C;
  return j;
}
template <int NJ> static void gemm_launch(GemmParams<NJ> &g, hipStream_t s) {
  unsigned blocks = 0;
  for (int i = 0; i < NJ; ++i) {
    g.job[i].block0 = blocks;
    blocks += (unsigned)(((g.job[i].rows + 15) / 16 * (size_t)g.job[i].CT + 3) / 4);
  }
  hipLaunchKernelGGL((k_lck_gemm<NJ>), dim3(blocks), dim3(256), 0, s, g);
}

template <int N> static int grad_launch(const cm3_actor_checkers_weights *aw, const cm3_qmix_mixer_checkers_weights *mw,
                                        const cm3_actor_checkers_weights *ag, const cm3_qmix_mixer_checkers_weights *mg,
                                        const cm3_qmix_learner_checkers_rows *r, float *ws, hipStream_t s) {
  const size_t B = (size_t)r->n_steps, R = B * N;
  const int Lo = 2 * (N > 1 ? N - 1 : 1), KP = kp_of(N), KM = kConvM + 6 * N, NH = kE * (N + 3), MD = kE * (N + 4);
  const Ws o = ws_layout(N, B);
  auto G = [](const float *q) { return const_cast<float *>(q); };
  {
    StageParams p = {R, B, N, Lo, KP, r->obs_self_t_f64, r->grid_f64, r->goals_onehot, r->obs_self_t, r->grid, r->goals, r->obs_self_v,
                     r->obs_others, r->vec, r->actions_prev, ws + o.x0, ws + o.pa, ws + o.xs, ws + o.xo, ws + o.gm, ws + o.pm, ws + o.xm,
                     ws + o.dca, ws + o.dcm};
    const size_t want = (R * kPosA * kPatA + 255) / 256;
    hipLaunchKernelGGL(k_lck_stage, dim3((unsigned)(want < 2048 ? want : 2048)), dim3(256), 0, s, p);
  }
  {  // 2. both convolutions
    GemmParams<2> g;
    g.job[0] = gjob(R, kC1R, kC1, aw->conv_b, kFA, kActRelu, nullptr, 0, ws + o.c1, kC1, 0, seg(ws + o.x0, kX0, aw->conv_w, 0, kObs, kBConvA));
    g.job[1] = gjob(B, kConvM, kConvM, mw->conv_b, kFM, kActRelu, nullptr, 0, ws + o.xm, KP, 0, seg(ws + o.gm, kGm, mw->conv_w, 0, kGrid, kBConvM));
    gemm_launch(g, s);
  }
  {  // 3. conv_linear
    GemmParams<1> g;
    g.job[0] = gjob(R, kLin, kLin, aw->lin_b, 0, kActRelu, nullptr, 0, ws + o.xs, kXs, 0, seg(ws + o.c1, kC1, aw->lin_w, kLin, kC1R, kBPlain));
    gemm_launch(g, s);
  }
  {  // 4. branch_self, branch_others
    GemmParams<2> g;
    g.job[0] = gjob(R, kH, kH, aw->self_b, 0, kActRelu, nullptr, 0, ws + o.hs, kH, 0, seg(ws + o.xs, kXs, aw->self_w, kH, kCat, kBPlain));
    g.job[1] = gjob(R, kH, kH, aw->others_b, 0, kActRelu, nullptr, 0, ws + o.ho, kH, 0, seg(ws + o.xo, kXo, aw->others_w, kH, Lo, kBPlain, 1));
    gemm_launch(g, s);
  }
  {  // 5. h2
    GemmParams<1> g;
    g.job[0] = gjob(R, kH, kH, aw->b_h2, 0, kActRelu, nullptr, 0, ws + o.h2, kH, 0, seg(ws + o.hs, kH, aw->w_self_h2, kH, kH, kBPlain));
    g.job[0].seg[1] = seg(ws + o.ho, kH, aw->w_others_h2, kH, kH, kBPlain);
    g.job[0].nseg = 2;
    gemm_launch(g, s);
  }
  {  // 6. Qmix_single_out
    GemmParams<1> g;
    g.job[0] = gjob(R, kA, kQ, aw->out_b, 0, kActNone, nullptr, 0, ws + o.q, kQ, 0, seg(ws + o.h2, kH, aw->out_w, kA, kH, kBPlain));
    gemm_launch(g, s);
  }
  {  // 7. the hyper-network
    GemmParams<4> g;
    const float *W[4] = {mw->hyper_w_1, mw->hyper_b_1, mw->hyper_w_final, mw->hyper_b_final_l1};
    for (int i = 0; i < 4; ++i) {
      const int nc = i == 0 ? kE * N : kE, c0 = i == 0 ? 0 : kE * (N + i - 1);
      g.job[i] = gjob(B, nc, nc, nullptr, 0, kActNone, nullptr, 0, ws + o.hy + c0, NH, 0, seg(ws + o.xm, KP, W[i], nc, KM, kBPlain));
    }
    gemm_launch(g, s);
  }
  {  // 8. the mixer
    MixParams p = {(uint32_t)B, r->td_f64, ws + o.hy, ws + o.q, mw->hyper_b_final, r->actions, r->td, r->q_tot, ws + o.err2, ws + o.dhy, ws + o.dq};
    hipLaunchKernelGGL((k_lck_mixer<N>), dim3((unsigned)B), dim3(128), 0, s, p);
  }
  {  // 9. d conv_m, d h2_pre
    GemmParams<2> g;
    g.job[0] = gjob(B, kConvM, kConvM, nullptr, 0, kActMask, ws + o.xm, KP, ws + o.dcm, 0, kFM,
                    seg(ws + o.dhy, MD, mw->hyper_w_1, kE * N, kE * N, kBTrans));
    g.job[0].seg[1] = seg(ws + o.dhy + kE * N, MD, mw->hyper_b_1, kE, kE, kBTrans);
    g.job[0].seg[2] = seg(ws + o.dhy + kE * (N + 1), MD, mw->hyper_w_final, kE, kE, kBTrans);
    g.job[0].seg[3] = seg(ws + o.dhy + kE * (N + 2), MD, mw->hyper_b_final_l1, kE, kE, kBTrans);
    g.job[0].nseg = 4;
    g.job[1] = gjob(R, kH, kH, nullptr, 0, kActMask, ws + o.h2, kH, ws + o.dh2, kH, 0, seg(ws + o.dq, kQ, aw->out_w, kA, kA, kBTrans));
    gemm_launch(g, s);
  }
  {  // 10. d hs_pre, d ho_pre
    GemmParams<2> g;
    g.job[0] = gjob(R, kH, kH, nullptr, 0, kActMask, ws + o.hs, kH, ws + o.dhs, kH, 0, seg(ws + o.dh2, kH, aw->w_self_h2, kH, kH, kBTrans));
    g.job[1] = gjob(R, kH, kH, nullptr, 0, kActMask, ws + o.ho, kH, ws + o.dho, kH, 0, seg(ws + o.dh2, kH, aw->w_others_h2, kH, kH, kBTrans));
    gemm_launch(g, s);
  }
  {  // 11. d lin_pre
    GemmParams<1> g;
    g.job[0] = gjob(R, kLin, kLin, nullptr, 0, kActMask, ws + o.xs, kXs, ws + o.dlin, kLin, 0, seg(ws + o.dhs, kH, aw->self_w, kH, kH, kBTrans));
    gemm_launch(g, s);
  }
  {  // 12. d c1_pre
    GemmParams<1> g;
    g.job[0] = gjob(R, kC1R, kC1R, nullptr, 0, kActMask, ws + o.c1, kC1, ws + o.dca, 0, kFA, seg(ws + o.dlin, kLin, aw->lin_w, kLin, kLin, kBTrans));
    gemm_launch(g, s);
  }
  XtdParams<9> x;
  RedParams<9> d;
  memset(&x, 0, sizeof(x));
  memset(&d, 0, sizeof(d));
  unsigned blocks = 0, elems = 0;
  auto job = [&](int i, const float *X, int ldx, int Kx, const float *D, int ldd, size_t rows, size_t chunks, RedSeg sg) {
    learner_job(x.job[i], d.job[i], blocks, elems, X, ldx, Kx, D, ldd, rows, chunks, ws + o.part[i]);
    d.job[i].nseg = 1;
    d.job[i].seg[0] = sg;
  };
  job(0, ws + o.pa, kPatA, kPatA, ws + o.dca, 16, R * kPosA, o.chunks_ra, RedSeg{0, kFA, G(ag->conv_w), G(ag->conv_b)});
  job(1, ws + o.c1, kC1, kC1R, ws + o.dlin, kLin, R, o.chunks_r, RedSeg{0, kLin, G(ag->lin_w), G(ag->lin_b)});
  job(2, ws + o.xs, kXs, kCat, ws + o.dhs, kH, R, o.chunks_r, RedSeg{0, kH, G(ag->self_w), G(ag->self_b)});
  job(3, ws + o.xo, kXo, Lo, ws + o.dho, kH, R, o.chunks_r, RedSeg{0, kH, G(ag->others_w), G(ag->others_b)});
  job(4, ws + o.hs, kH, kH, ws + o.dh2, kH, R, o.chunks_r, RedSeg{0, kH, G(ag->w_self_h2), G(ag->b_h2)});
  job(5, ws + o.ho, kH, kH, ws + o.dh2, kH, R, o.chunks_r, RedSeg{0, kH, G(ag->w_others_h2), nullptr});
  job(6, ws + o.h2, kH, kH, ws + o.dq, kQ, R, o.chunks_r, RedSeg{0, kA, G(ag->out_w), G(ag->out_b)});
  job(7, ws + o.pm, kPatM, kPatM, ws + o.dcm, 16, B * kPosM, o.chunks_bm, RedSeg{0, kFM, G(mg->conv_w), G(mg->conv_b)});
  job(8, ws + o.xm, KP, KM, ws + o.dhy, MD, B, o.chunks_b, RedSeg{0, kE * N, G(mg->hyper_w_1), nullptr});
  d.job[8].nseg = 5;
  d.job[8].seg[1] = RedSeg{kE * N, kE, G(mg->hyper_b_1), nullptr};
  d.job[8].seg[2] = RedSeg{kE * (N + 1), kE, G(mg->hyper_w_final), nullptr};
  d.job[8].seg[3] = RedSeg{kE * (N + 2), kE, G(mg->hyper_b_final_l1), nullptr};
  d.job[8].seg[4] = RedSeg{kE * (N + 3), kE, nullptr, G(mg->hyper_b_final)};
  d.total = elems;
  d.B = (uint32_t)B;
  d.err2 = ws + o.err2;
  d.loss = r->loss;
  hipLaunchKernelGGL(k_learner_xtd<9>, dim3(blocks), dim3(256), 0, s, x);
  note_variant("k_qmix_learner_checkers_reduce", (int)sizeof(float), N, 4, 0, 0, 0, 0, 0, 0, /* prec=f32 */ 0);
  note_tail(",after=stage+6gemm+mixer+4gemm+xtd");   // (the thirteen launches before it, see the head of this file)
  hipLaunchKernelGGL(k_learner_reduce<9>, dim3((elems + 255u) / 256u + 1u), dim3(256), 0, s, d);
  CM3_HIP_CHECK(hipGetLastError());
  return CM3_OK;
}

static size_t ws_floats_for(int n, int64_t n_steps) {   // (0 for an agent count outside 1..8 or a batch out of range)
  if (n < 1 || n > kMaxAgents || n_steps <= 0 || n_steps > kMaxSteps) return 0;
  return ws_layout(n, (size_t)n_steps).total;
}

static bool agent_set(const cm3_actor_checkers_weights *t) {
  return t->conv_w && t->conv_b && t->lin_w && t->lin_b && t->self_w && t->self_b && t->w_self_h2 && t->others_w && t->others_b &&
         t->w_others_h2 && t->b_h2 && t->out_w && t->out_b;
}
static bool mixer_set(const cm3_qmix_mixer_checkers_weights *t) {
  return t->conv_w && t->conv_b && t->hyper_w_1 && t->hyper_w_final && t->hyper_b_1 && t->hyper_b_final_l1 && t->hyper_b_final;
}
static bool agent_aligned(const cm3_actor_checkers_weights *t) {
  const uintptr_t all = (uintptr_t)t->conv_w | (uintptr_t)t->conv_b | (uintptr_t)t->lin_w | (uintptr_t)t->lin_b | (uintptr_t)t->self_w |
                        (uintptr_t)t->self_b | (uintptr_t)t->w_self_h2 | (uintptr_t)t->others_w | (uintptr_t)t->others_b |
                        (uintptr_t)t->w_others_h2 | (uintptr_t)t->b_h2 | (uintptr_t)t->out_w | (uintptr_t)t->out_b;
  return all % 4 == 0;
}
static bool mixer_aligned(const cm3_qmix_mixer_checkers_weights *t) {
  const uintptr_t all = (uintptr_t)t->conv_w | (uintptr_t)t->conv_b | (uintptr_t)t->hyper_w_1 | (uintptr_t)t->hyper_w_final |
                        (uintptr_t)t->hyper_b_1 | (uintptr_t)t->hyper_b_final_l1 | (uintptr_t)t->hyper_b_final;
  return all % 4 == 0;
}

}  // namespace lck
}  // namespace cm3

extern "C" size_t cm3_qmix_learner_checkers_workspace_bytes(int32_t n_agents, int64_t n_steps) {
  return cm3::lck::ws_floats_for(n_agents, n_steps) * sizeof(float);
}

extern "C" int cm3_qmix_learner_checkers_grad_f32(const cm3_qmix_learner_checkers_desc *d, const cm3_actor_checkers_weights *agent_weights,
                                                  const cm3_qmix_mixer_checkers_weights *mixer_weights,
                                                  const cm3_actor_checkers_weights *agent_grads,
                                                  const cm3_qmix_mixer_checkers_weights *mixer_grads,
                                                  const cm3_qmix_learner_checkers_rows *r, void *workspace, size_t workspace_bytes,
                                                  void *stream) {
  using namespace cm3;
  using namespace cm3::lck;
  CM3_REQUIRE(d, "null desc");
  CM3_REQUIRE(d->n_agents >= 1 && d->n_agents <= kMaxAgents, "n_agents must be in 1..%d", kMaxAgents);
  CM3_REQUIRE(d->conv_f == kFA && d->n_conv_linear == kLin && d->n_h1 == kH && d->n_h2 == kH && d->n_actions == kA,
              "the Checkers QMIX agent network is 6/32/256/256/5 (networks.Qmix_single_checkers): conv_f, n_conv_linear, n_h1, n_h2, "
              "n_actions; got %d/%d/%d/%d/%d", d->conv_f, d->n_conv_linear, d->n_h1, d->n_h2, d->n_actions);
  CM3_REQUIRE(d->embed_dim == kE && d->mixer_conv_f == kFM,
              "the supported Qmix_mixer_checkers has embedding width %d and %d filters of 3x5; got %d and %d", kE, kFM, d->embed_dim,
              d->mixer_conv_f);
  CM3_REQUIRE(agent_weights && mixer_weights, "null weights");
  CM3_REQUIRE(agent_grads && mixer_grads, "null grads");
  CM3_REQUIRE(r, "null rows");
  CM3_REQUIRE(agent_set(agent_weights) && mixer_set(mixer_weights),
              "missing weights: the thirteen Agent_main and seven Mixer_main tensors are all required");
  CM3_REQUIRE(agent_set(agent_grads) && mixer_set(mixer_grads), "missing gradients: one tensor per weight is required");
  CM3_REQUIRE(r->obs_self_t && r->obs_self_v && r->obs_others && r->actions_prev && r->actions && r->goals && r->grid && r->vec && r->td,
              "missing inputs: obs_self_t, obs_self_v, obs_others, actions_prev, actions, goals, grid, vec and td are all required");
  CM3_REQUIRE(r->loss && r->q_tot, "missing outputs: loss and q_tot are required");
  CM3_REQUIRE(workspace, "workspace is NULL: cm3_qmix_learner_checkers_workspace_bytes(n_agents, n_steps) bytes of device memory");
  CM3_REQUIRE(agent_aligned(agent_weights) && mixer_aligned(mixer_weights) && agent_aligned(agent_grads) && mixer_aligned(mixer_grads),
              "misaligned weights or gradients: every tensor must be 4-byte aligned");
  CM3_REQUIRE((uintptr_t)r->obs_self_v % 8 == 0 && (uintptr_t)r->obs_others % 8 == 0 && (uintptr_t)r->vec % 8 == 0 &&
                  (uintptr_t)r->actions_prev % 4 == 0 && (uintptr_t)r->actions % 4 == 0 &&
                  (!r->obs_self_t_f64 || (uintptr_t)r->obs_self_t % 8 == 0) && (!r->grid_f64 || (uintptr_t)r->grid % 8 == 0) &&
                  (!r->goals_onehot || (uintptr_t)r->goals % 8 == 0) && (uintptr_t)r->td % (r->td_f64 ? 8 : 4) == 0,
              "misaligned inputs: obs_self_v, obs_others, vec, float64 windows and grids and one-hot goals must be 8-byte aligned, the "
              "actions 4-byte aligned, td as its type");
  CM3_REQUIRE((uintptr_t)r->loss % 4 == 0 && (uintptr_t)r->q_tot % 4 == 0, "misaligned outputs: loss and q_tot must be 4-byte aligned");
  CM3_REQUIRE((uintptr_t)workspace % 16 == 0, "misaligned workspace: must be 16-byte aligned");
  CM3_REQUIRE(r->n_steps > 0, "n_steps must be positive");
  CM3_REQUIRE(r->n_steps <= kMaxSteps, "n_steps %lld is more than (2^31 - 1) / %d", (long long)r->n_steps, kMaxAgents * kPosM);
  const size_t need = ws_floats_for(d->n_agents, r->n_steps) * sizeof(float);
  CM3_REQUIRE(workspace_bytes >= need, "workspace of %zu bytes is too small: %d agents and %lld steps take %zu", workspace_bytes, d->n_agents,
              (long long)r->n_steps, need);
  hipStream_t s = (hipStream_t)stream;
  return agent_launch<1, 2, 3, 4, 5, 6, 7, 8>(d->n_agents, [&](auto n) {
    return grad_launch<n()>(agent_weights, mixer_weights, agent_grads, mixer_grads, r, (float *)workspace, s);
  });
}
