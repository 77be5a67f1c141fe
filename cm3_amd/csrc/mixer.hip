// The particle QMIX mixer over TRANSITION rows (part of ABI 9, additive): networks.Qmix_mixer (networks.py:640-685), the evaluation
// mixer_target of alg_qmix.train_step (alg_qmix.py:358-369) that carries no gradient, with the TD target that follows it.
// Per transition b, x = concat(state[b] [4N], goals[b] [2N]), K = 6N:
//   l1      = relu(x . hyper_b_final_l1/kernel[K][64])                  b_final = l1 . hyper_b_final/kernel[64][1]      (no biases)
//   w1      = |x . hyper_w_1[K][64 N]| viewed [N][64]                    b1      = x . hyper_b_1[K][64]
//   hidden  = elu(agent_qs[b][0..N) . w1 + b1)  [64]                     w_final = |x . hyper_w_final[K][64]|
//   q_tot   = hidden . w_final + b_final
// The hyper-network is ONE [rows][K] x [K][64 (N + 3)] product: the N column blocks of hyper_w_1, then hyper_b_1, hyper_w_final,
// hyper_b_final_l1, on the exact-f32 matrix instruction (v_mfma_f32_16x16x4_f32, a k-ordered fmaf chain); K is zero-padded to whole
// k-steps (6N = 2 mod 4 for odd N) by the pack kernel and the staging.
// Mapping: 256 threads = 4 waves own 16 rows (a batch of 128 is eight workgroups on eight CUs).  Wave w owns the
// embedding columns e in [16w, 16w + 16) of every column block, C[row][e]: lane (hi, col) holds rows 4 hi + 0..3 at e = 16w + col.
// The column blocks are streamed one after the other -- the packed weights (213 KB at N = 10) never sit in LDS -- and each is folded
// into four registers per lane as soon as it is through, so a lane finishes its e of its four rows without any exchange.
// Order of every sum, in the source as it is evaluated (-ffp-contract=off): a row's bits depend on neither its place in the
// workgroup nor n_steps.
//   over agents   t = q[0] |w1[0][e]|;  t = t + q[n] |w1[n][e]| for n = 1 .. N-1;  h = t + b1[e]     (tf.matmul([1,N] x [N,64]) + b1)
//   elu           h > 0 ? h : expm1f(h)
//   over e        p[e] = hidden[e] |w_final[e]| and c[e] = l1[e] hyper_b_final[e] are summed SEPARATELY, each as
//                 a pairwise tree inside every 16 columns -- ((e0 + e1) + (e2 + e3)) + ((e4 + e5) + (e6 + e7)), the same for
//                 e8..e15, then the two halves -- by DPP moves inside the 16-lane row, then across the four waves through LDS in
//                 wave order ((s0 + s1) + s2) + s3;  q_tot = sum p + sum c
// LDS: x [16][KP + 1] + agent_qs [16][N] + partials [4][16][2]: 5 056 bytes at N = 10.
#include "ck_tiles.h"

namespace cm3 {

constexpr int kME = 64;      // embed_dim of Qmix_mixer
constexpr int kMixerRows = 16;

template <int N> struct MixerLayout {
  static constexpr int K = 6 * N, KP = (K + 3) / 4 * 4;
  static constexpr int S = KP / 4;                    // k-steps (2 .. 15)
  static constexpr int SP = (S + 3) / 4 * 4;          // per-lane stride of a block's operands (16-byte loads)
  static constexpr int NB = N + 3;                    // column blocks: w1[0..N), b1, w_final, b_final_l1
  static constexpr int XW = KP + 1;                   // LDS row stride of x
  // packed weights (floats)
  static constexpr int kW = 0;                        // [NB blocks][4 waves][64 lanes][SP]   B operands
  static constexpr int kBf = kW + NB * 4 * 64 * SP;   // [64]                                 hyper_b_final/kernel
  static constexpr int kTotal = kBf + kME;
};

struct MixerPackParams {
  const float *w1, *w_final, *b1, *b_final_l1, *b_final;
};

template <int N> __global__ void __launch_bounds__(256) k_qmix_mixer_pack(const MixerPackParams p, float *out) {
  using ML = MixerLayout<N>;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < ML::kTotal; t += gridDim.x * 256) {
    float v = 0.0f;
    if (t < ML::kBf) {
      const int s = t % ML::SP, lane = (t / ML::SP) & 63, w = (t / ML::SP / 64) & 3, c = t / ML::SP / 256;
      const int k = 4 * s + (lane >> 4), e = 16 * w + (lane & 15);
      if (s < ML::S && k < ML::K) {
        if (c < N) v = p.w1[k * (kME * N) + kME * c + e];
        else if (c == N) v = p.b1[k * kME + e];
        else if (c == N + 1) v = p.w_final[k * kME + e];
        else v = p.b_final_l1[k * kME + e];
      }
    } else {
      v = p.b_final[t - ML::kBf];
    }
    out[t] = v;
  }
}

struct MixerParams {
  uint32_t n_steps;
  const float *state, *goals, *agent_qs;     // [B][N][4], [B][N][2], [B][N]
  const void *reward;                        // [B][N] float32 / float64 (td)
  int reward_f64;
  const uint8_t *done;                       // [B] (td)
  double gamma;
  float *q_tot;                              // optional [B]
  double *q_tot64, *td;                      // optional [B]
  const float *packed;
};

// moves inside a 16-lane DPP row: lane ^ 1, lane ^ 2 (inside each quad), i <-> 7 - i (inside each 8 lanes), i <-> 15 - i
constexpr int kMixDppXor1 = 0xB1, kMixDppXor2 = 0x4E, kMixDppHalfMirror = 0x141, kMixDppMirror = 0x140;
template <int CTRL> __device__ __forceinline__ float mix_dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
// the pairwise tree over the 16 columns of a row tile; every lane of the row ends with the same bits (a + b == b + a)
__device__ __forceinline__ float mix_sum16(float v) {
  v = v + mix_dpp<kMixDppXor1>(v);
  v = v + mix_dpp<kMixDppXor2>(v);
  v = v + mix_dpp<kMixDppHalfMirror>(v);
  v = v + mix_dpp<kMixDppMirror>(v);
  return v;
}

// sum(reward_local[b][0..N)) in float64 in np.sum's order, as k_qmix_td_target (batch.hip)
template <int N, typename RR> __device__ __forceinline__ double mixer_reward_sum(const RR *r) {
  double sum;
  int i;
  if constexpr (N < 8) {
    sum = (double)r[0];
    i = 1;
  } else {
    sum = (((double)r[0] + (double)r[1]) + ((double)r[2] + (double)r[3])) + (((double)r[4] + (double)r[5]) + ((double)r[6] + (double)r[7]));
    i = 8;
  }
  for (; i < N; ++i) sum += (double)r[i];
  return sum;
}

// x . (column block c) for this lane's e and four rows: the block's S operands of the lane (lane_w: the lane's operands of block 0),
// then one k-ordered chain from zero
template <int N> __device__ __forceinline__ f32x4 mixer_block(const float *lane_w, int c, const float (&xa)[MixerLayout<N>::S]) {
  using ML = MixerLayout<N>;
  float bw[ML::SP];
  const float4 *src = reinterpret_cast<const float4 *>(lane_w + (size_t)c * (4 * 64 * ML::SP));
#pragma unroll
  for (int s4 = 0; s4 < ML::SP / 4; ++s4) {
    const float4 v = src[s4];
    bw[4 * s4 + 0] = v.x; bw[4 * s4 + 1] = v.y; bw[4 * s4 + 2] = v.z; bw[4 * s4 + 3] = v.w;
  }
  f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int s = 0; s < ML::S; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[s], bw[s], acc, 0, 0, 0);
  return acc;
}

template <int N> __global__ void CM3_MATRIX_KERNEL k_qmix_mixer_rows(const MixerParams p) {
  using ML = MixerLayout<N>;
  __shared__ float xs[kMixerRows][ML::XW];
  __shared__ float qs[kMixerRows][N];
  __shared__ float part[4][kMixerRows][2];
  const int tid = threadIdx.x, lane = tid & 63, col = lane & 15, hi = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t rows = p.n_steps;
  const uint32_t row_base = blockIdx.x * (uint32_t)kMixerRows;

  // ---- staging: thread u = (row, agent) brings one agent's state, goal and Q; rows past the count repeat the last one ----
  if (tid < kMixerRows * N) {
    const int r = tid / N, n = tid - r * N;
    const uint32_t hr = row_base + r;
    const size_t bn = (size_t)(hr < rows ? hr : rows - 1) * N + n;
    const float4 s = reinterpret_cast<const float4 *>(p.state)[bn];
    const float2 g = reinterpret_cast<const float2 *>(p.goals)[bn];
    xs[r][4 * n + 0] = s.x; xs[r][4 * n + 1] = s.y; xs[r][4 * n + 2] = s.z; xs[r][4 * n + 3] = s.w;
    xs[r][4 * N + 2 * n + 0] = g.x; xs[r][4 * N + 2 * n + 1] = g.y;
    qs[r][n] = p.agent_qs[bn];
  } else if (tid >= 192 && tid < 192 + kMixerRows) {
#pragma unroll
    for (int k = ML::K; k < ML::KP; ++k) xs[tid - 192][k] = 0.0f;
  }
  __syncthreads();

  float xa[ML::S];                      // A operands: x[row = col][k = 4 s + hi], the same for every column block
#pragma unroll
  for (int s = 0; s < ML::S; ++s) xa[s] = xs[col][4 * s + hi];
  float qv[4][N];                       // agent_qs of this lane's four rows
#pragma unroll
  for (int reg = 0; reg < 4; ++reg)
#pragma unroll
    for (int n = 0; n < N; ++n) qv[reg][n] = qs[4 * hi + reg][n];

  const float *wave_w = p.packed + ML::kW + (size_t)(w * 64 + lane) * ML::SP;
  // the chain over agents: |w1[n][e]| of column block n, ascending, started by the product for n = 0
  float t[4];
  {
    const f32x4 a = mixer_block<N>(wave_w, 0, xa);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) t[reg] = qv[reg][0] * __builtin_fabsf(a[reg]);
  }
#pragma unroll
  for (int n = 1; n < N; ++n) {
    const f32x4 a = mixer_block<N>(wave_w, n, xa);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) t[reg] = t[reg] + qv[reg][n] * __builtin_fabsf(a[reg]);
  }
  float pe[4], ce[4];
  {
    const f32x4 b1 = mixer_block<N>(wave_w, N, xa), wf = mixer_block<N>(wave_w, N + 1, xa), l1 = mixer_block<N>(wave_w, N + 2, xa);
    const float bf = p.packed[ML::kBf + 16 * w + col];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const float h = t[reg] + b1[reg];
      const float hidden = h > 0.0f ? h : expm1f(h);
      pe[reg] = hidden * __builtin_fabsf(wf[reg]);
      ce[reg] = relu_f32(l1[reg]) * bf;
    }
  }
  // ---- over e: inside the wave's 16 columns, then across the waves in wave order ----
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const float sp = mix_sum16(pe[reg]), sc = mix_sum16(ce[reg]);
    if (col == 0) {
      part[w][4 * hi + reg][0] = sp;
      part[w][4 * hi + reg][1] = sc;
    }
  }
  __syncthreads();
  const uint32_t hr = row_base + tid;
  if (tid < kMixerRows && hr < rows) {
    const float sp = ((part[0][tid][0] + part[1][tid][0]) + part[2][tid][0]) + part[3][tid][0];
    const float sc = ((part[0][tid][1] + part[1][tid][1]) + part[2][tid][1]) + part[3][tid][1];
    const float q = sp + sc;
    if (p.q_tot) p.q_tot[hr] = q;
    if (p.q_tot64) p.q_tot64[hr] = (double)q;
    if (p.td) {
      // sum(reward_local[b]) + float32(gamma) * q * not_done, in the order and types of k_qmix_td_target (batch.hip) on a float32 q_tot
      const size_t b0 = (size_t)hr * N;
      const double sum = p.reward_f64 ? mixer_reward_sum<N>(reinterpret_cast<const double *>(p.reward) + b0)
                                      : mixer_reward_sum<N>(reinterpret_cast<const float *>(p.reward) + b0);
      const float gq = (float)p.gamma * q;
      p.td[hr] = sum + (double)gq * (double)(p.done[hr] ? 0 : 1);
    }
  }
}

template <int N> static int mixer_launch(const MixerParams &p, hipStream_t s) {
  const unsigned blocks = (p.n_steps + (uint32_t)kMixerRows - 1u) / (uint32_t)kMixerRows;
  note_variant("k_qmix_mixer_rows", (int)sizeof(float), N, 4, 0, 0, 0, 0, 0, 0, /* prec=f32 */ 0);
  hipLaunchKernelGGL((k_qmix_mixer_rows<N>), dim3(blocks), dim3(256), 0, s, p);
  CM3_HIP_CHECK(hipGetLastError());
  return CM3_OK;
}

template <int N> static int mixer_pack_launch(const MixerPackParams &p, float *out, hipStream_t s) {
  hipLaunchKernelGGL((k_qmix_mixer_pack<N>), dim3(32), dim3(256), 0, s, p, out);
  CM3_HIP_CHECK(hipGetLastError());
  return CM3_OK;
}

static size_t mixer_floats_for(int n) {   // (0 for an agent count outside 1..10)
  bool hit;
  return agent_dispatch_1_to_10(n, hit, [&](auto k) { return (size_t)MixerLayout<k()>::kTotal; });
}

static int mixer_check_desc(const cm3_qmix_mixer_particle_desc *d) {
  CM3_REQUIRE(d, "null desc");
  CM3_REQUIRE(d->n_agents >= 1 && d->n_agents <= CM3_MAX_AGENTS, "n_agents must be in 1..%d", CM3_MAX_AGENTS);
  CM3_REQUIRE(d->embed_dim == kME, "the supported embedding width of Qmix_mixer is %d (networks.py:650); got %d", kME, d->embed_dim);
  return CM3_OK;
}

// ---- Checkers -------------------------------------------------------------------------------------------------------------------------
// The Checkers QMIX mixer over TRANSITION rows (part of ABI 9, additive): networks.Qmix_mixer_checkers (networks.py:688-734) at the
// widths of config_checkers_stage{1,2}.json, mixer_target of alg_qmix_checkers.train_step (alg_qmix_checkers.py:364-375) with the TD
// target that follows it (:377-379).  Per transition b:
//   conv    = relu(conv2d SAME 3x5x2 -> 4 over grid[b] [3][9][2] + bias)  -> 108 (NHWC flatten)
//   x       = concat(conv [108], state[b] [4N], goals[b] [2N]), K = 108 + 6N; the rest is the particle mixer at embed_dim 128
// The convolution is the critic's Toeplitz matrix (ck_tiles.h: toeplitz<3, 9, 2, 4, 3, 5>, here [64 x 128]: 108 outputs padded to two
// column tiles per wave); the hyper-network is ONE [rows][KP] x [KP][128 (N + 3)] product -- the N column blocks of hyper_w_1, then
// hyper_b_1, hyper_w_final, hyper_b_final_l1 -- and both run through ck_tiles.h's gemm_tiles on the exact-f32 matrix instruction
// (v_mfma_f32_16x16x4_f32), B operands from packed per-lane tiles [col tile][k group][lane][4].  K is zero-padded to whole k groups of
// the tile loop (KP = 128 at N <= 3, 144 at N <= 6, 160 above) by the pack kernel and the staging.
// Mapping: 256 threads = 4 waves own 16 rows (a batch of 128 is eight workgroups on eight CUs).  Wave w owns the embedding
// units e in [32w, 32w + 32) of every column block -- column tiles 2w and 2w + 1, C[row][e]: lane (hi, col) holds rows 4 hi + 0..3 at
// e = 32w + 16c + col.  The column blocks are streamed one after the other -- the packed weights (361 KB at N = 2, 935 KB at N = 8)
// never sit in LDS; the first operands of block c + 1 are requested before the matrix instructions of block c -- and each is folded
// into registers as soon as it is through, so a lane finishes its two e of its four rows without any exchange.
// Order of every sum, in the source as it is evaluated (-ffp-contract=off): a row's bits depend on neither its place in the workgroup
// nor n_steps.
//   conv, hyper   one chain per output from zero in the tile loop's k order: k groups of 16 ascending; inside a group the four matrix
//                 instructions j = 0..3, each over k = 16g + j, 16g + 4 + j, 16g + 8 + j, 16g + 12 + j; conv: + bias, relu
//   over agents   t = q[0] |w1[0][e]|;  t = t + q[n] |w1[n][e]| for n = 1 .. N-1;  h = t + b1[e]    (tf.matmul([1,N] x [N,128]) + b1)
//   elu           h > 0 ? h : expm1f(h)
//   over e        p[e] = hidden[e] |w_final[e]| and c[e] = l1[e] hyper_b_final[e] are summed SEPARATELY, each as a pairwise tree
//                 inside every 16 units (mix_sum16 above: DPP moves inside the 16-lane row), then the eight sixteens left to right
//                 through LDS, ((((((s0 + s1) + s2) + s3) + s4) + s5) + s6) + s7;  q_tot = sum p + sum c
// Inputs in the forms the Checkers columns have (no staging copy): grid int8 / float64, vec float64, goals uint8 index / int64 one-hot;
// float64 values are rounded to float32 as they are staged, as a tf.float32 placeholder rounds its feed.
// LDS at N = 8: x [16][164] + grid [16][68] + agent_qs [16][8] + partials [8][16][2]: 16 384 bytes.
namespace ck_mixer {

constexpr int kE = 128;                                       // embed_dim of Qmix_mixer_checkers
constexpr int kRows = 16;
constexpr int kMaxAgents = 8;                                 // the Checkers actor's and critics' range
constexpr int kGrid = 54, kGridF = 4, kConv = 108;            // 3 x 9 x 2 -> 3 x 9 x 4
constexpr int kKG = 64, kNG = 128, kLdG = kKG + 4;            // the Toeplitz matrix, padded to two column tiles per wave
constexpr int kCT = kE / 16;                                  // column tiles of a column block

template <int N> struct Layout {
  static constexpr int K = kConv + 6 * N, KP = (K + 15) / 16 * 16;
  static constexpr int KG = KP / 16;                          // k groups (8 .. 10)
  static constexpr int NB = N + 3;                            // column blocks: w1[0..N), b1, w_final, b_final_l1
  static constexpr int Ld = KP + 4;                           // LDS row stride of x (4 mod 32 words)
  // packed weights (floats): B tiles [col tile][k group][lane][4] (ck_tiles.h)
  static constexpr int kPG = 0;                               // the Toeplitz matrix [8 tiles][4 groups]
  static constexpr int kPGB = kPG + (kNG / 16) * (kKG / 16) * 256;   // [128] the conv bias per output column
  static constexpr int kPH = kPGB + kNG;                      // the hyper-network [NB blocks][8 tiles][KG groups]
  static constexpr int kBf = kPH + NB * kCT * KG * 256;       // [128] hyper_b_final/kernel
  static constexpr int kTotal = kBf + kE;
};

struct PackParams {
  const float *conv_w, *conv_b, *w1, *w_final, *b1, *b_final_l1, *b_final;
};

template <int N> __global__ void __launch_bounds__(256) k_ck_qmix_mixer_pack(const PackParams p, float *out) {
  using L = Layout<N>;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < L::kTotal; t += gridDim.x * 256) {
    float v = 0.0f;
    if (t < L::kPGB) {
      const int u = t - L::kPG, j = u & 3, lane = (u >> 2) & 63, gi = u >> 8, g = gi % (kKG / 16), ct = gi / (kKG / 16);
      v = toeplitz<3, 9, 2, kGridF, 3, 5>(p.conv_w, 16 * g + 4 * (lane >> 4) + j, 16 * ct + (lane & 15));
    } else if (t < L::kPH) {
      const int u = t - L::kPGB;
      v = u < kConv ? p.conv_b[u % kGridF] : 0.0f;
    } else if (t < L::kBf) {
      const int u = t - L::kPH, j = u & 3, lane = (u >> 2) & 63, gi = u >> 8, g = gi % L::KG, tile = gi / L::KG;
      const int c = tile / kCT, k = 16 * g + 4 * (lane >> 4) + j, e = 16 * (tile - kCT * c) + (lane & 15);
      if (k < L::K) {
        if (c < N) v = p.w1[k * (kE * N) + kE * c + e];
        else if (c == N) v = p.b1[k * kE + e];
        else if (c == N + 1) v = p.w_final[k * kE + e];
        else v = p.b_final_l1[k * kE + e];
      }
    } else {
      v = p.b_final[t - L::kBf];
    }
    out[t] = v;
  }
}

struct Params {
  uint32_t n_steps;
  int grid_f64, goals_onehot, reward_f64;
  const void *grid;               // [B][54] int8 / float64
  const double *vec;              // [B][N][4]
  const void *goals;              // [B][N] uint8 index / [B][N][2] int64 one-hot
  const float *agent_qs;          // [B][N]
  const void *reward;             // [B][N] float32 / float64 (td)
  const uint8_t *done;            // [B] (td)
  double gamma;
  float *q_tot;                   // optional [B]
  double *q_tot64, *td;           // optional [B]
  const float *packed;
};

// x . (column block blk) for this wave's two column tiles of the 16 rows.  b: in, the first operands of block blk; out, those of block
// blk + 1, requested before the matrix instructions of this block issue
template <int N>
__device__ __forceinline__ void ck_block(const float *xs, const float *ph, int blk, int w, int lane, float4 (&b)[2], f32x4 (&acc)[1][2]) {
  using L = Layout<N>;
  float4 next[2];
  if (blk + 1 < L::NB) load_b0<2, L::KG>(ph, kCT * (blk + 1) + 2 * w, lane, next);
  zero_tiles(acc);
  gemm_tiles<1, 2, L::KG>(xs, L::Ld, 0, ph, kCT * blk + 2 * w, lane, b, acc);
  if (blk + 1 < L::NB) {
    b[0] = next[0];
    b[1] = next[1];
  }
}

template <int N> __global__ void CM3_MATRIX_KERNEL k_ck_qmix_mixer_rows(const Params p) {
  using L = Layout<N>;
  __shared__ __attribute__((aligned(16))) float xs[kRows * L::Ld];
  __shared__ __attribute__((aligned(16))) float gs[kRows * kLdG];
  __shared__ float qs[kRows][N];
  __shared__ float part[kCT][kRows][2];
  const int tid = threadIdx.x, lane = tid & 63, col = lane & 15, hi = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t rows = p.n_steps;
  const uint32_t row_base = blockIdx.x * (uint32_t)kRows;
  const float *pk = p.packed, *ph = p.packed + L::kPH;

  float4 b_g[2], b_h[2];
  load_b0<2, kKG / 16>(pk + L::kPG, 2 * w, lane, b_g);
  // ---- staging: thread u = (row, agent) brings one agent's state, goal and Q; the grid tile [16][64]; rows past the count repeat
  // the last one ----
  if (tid < kRows * N) {
    const int r = tid / N, n = tid - r * N;
    const uint32_t hr = row_base + r;
    const size_t bn = (size_t)(hr < rows ? hr : rows - 1) * N + n;
    float *x = xs + r * L::Ld + kConv;
#pragma unroll
    for (int k = 0; k < 4; ++k) x[4 * n + k] = (float)p.vec[bn * 4 + k];
    if (p.goals_onehot) {
      x[4 * N + 2 * n + 0] = (float)reinterpret_cast<const int64_t *>(p.goals)[bn * 2];
      x[4 * N + 2 * n + 1] = (float)reinterpret_cast<const int64_t *>(p.goals)[bn * 2 + 1];
    } else {
      const int gl = reinterpret_cast<const uint8_t *>(p.goals)[bn];
      x[4 * N + 2 * n + 0] = gl == 0 ? 1.0f : 0.0f;
      x[4 * N + 2 * n + 1] = gl == 0 ? 0.0f : 1.0f;
    }
    qs[r][n] = p.agent_qs[bn];
  } else if (tid >= 192 && tid < 192 + kRows) {
#pragma unroll
    for (int k = L::K; k < L::KP; ++k) xs[(tid - 192) * L::Ld + k] = 0.0f;
  }
  for (int idx = tid; idx < kRows * kKG; idx += 256) {
    const int r = idx >> 6, k = idx & 63;
    const uint32_t hr = row_base + r;
    const size_t at = (size_t)(hr < rows ? hr : rows - 1) * kGrid + k;
    float v = 0.0f;
    if (k < kGrid) v = p.grid_f64 ? (float)reinterpret_cast<const double *>(p.grid)[at] : (float)reinterpret_cast<const int8_t *>(p.grid)[at];
    gs[r * kLdG + k] = v;
  }
  __syncthreads();
  // ---- the convolution (Toeplitz) into x[:, 0:108], relu; wave w: column tiles 2w, 2w + 1 ----
  {
    f32x4 acc[1][2];
    float bias[2];
    load_bias<2>(pk + L::kPGB, 2 * w, lane, bias);
    zero_tiles(acc);
    gemm_tiles<1, 2, kKG / 16>(gs, kLdG, 0, pk + L::kPG, 2 * w, lane, b_g, acc);
    load_b0<2, L::KG>(ph, 2 * w, lane, b_h);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int n = 16 * (2 * w + c) + col;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        if (n < kConv) xs[(4 * hi + reg) * L::Ld + n] = fmaxf(acc[0][c][reg] + bias[c], 0.0f);
    }
  }
  __syncthreads();

  float qv[4][N];                       // agent_qs of this lane's four rows
#pragma unroll
  for (int reg = 0; reg < 4; ++reg)
#pragma unroll
    for (int n = 0; n < N; ++n) qv[reg][n] = qs[4 * hi + reg][n];
  // ---- the hyper-network, block by block.  The chain over agents: |w1[n][e]| of column block n, ascending, started by the product
  // for n = 0 ----
  float t[2][4];
  {
    f32x4 a[1][2];
    ck_block<N>(xs, ph, 0, w, lane, b_h, a);
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) t[c][reg] = qv[reg][0] * __builtin_fabsf(a[0][c][reg]);
  }
#pragma unroll
  for (int n = 1; n < N; ++n) {
    f32x4 a[1][2];
    ck_block<N>(xs, ph, n, w, lane, b_h, a);
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) t[c][reg] = t[c][reg] + qv[reg][n] * __builtin_fabsf(a[0][c][reg]);
  }
  float pe[2][4], ce[2][4];
  {
    f32x4 b1[1][2], wf[1][2], l1[1][2];
    ck_block<N>(xs, ph, N, w, lane, b_h, b1);
    ck_block<N>(xs, ph, N + 1, w, lane, b_h, wf);
    ck_block<N>(xs, ph, N + 2, w, lane, b_h, l1);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const float bf = pk[L::kBf + 32 * w + 16 * c + col];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const float h = t[c][reg] + b1[0][c][reg];
        const float hidden = h > 0.0f ? h : expm1f(h);
        pe[c][reg] = hidden * __builtin_fabsf(wf[0][c][reg]);
        ce[c][reg] = relu_f32(l1[0][c][reg]) * bf;
      }
    }
  }
  // ---- over e: inside each sixteen, then the eight sixteens left to right ----
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const float sp = mix_sum16(pe[c][reg]), sc = mix_sum16(ce[c][reg]);
      if (col == 0) {
        part[2 * w + c][4 * hi + reg][0] = sp;
        part[2 * w + c][4 * hi + reg][1] = sc;
      }
    }
  __syncthreads();
  const uint32_t hr = row_base + tid;
  if (tid < kRows && hr < rows) {
    float sp = part[0][tid][0] + part[1][tid][0], sc = part[0][tid][1] + part[1][tid][1];
#pragma unroll
    for (int j = 2; j < kCT; ++j) {
      sp = sp + part[j][tid][0];
      sc = sc + part[j][tid][1];
    }
    const float q = sp + sc;
    if (p.q_tot) p.q_tot[hr] = q;
    if (p.q_tot64) p.q_tot64[hr] = (double)q;
    if (p.td) {
      // sum(local_rewards[b]) + float32(gamma) * q * not_done, in the order and types of k_qmix_td_target (batch.hip) on a float32 q_tot
      const size_t b0 = (size_t)hr * N;
      const double sum = p.reward_f64 ? mixer_reward_sum<N>(reinterpret_cast<const double *>(p.reward) + b0)
                                      : mixer_reward_sum<N>(reinterpret_cast<const float *>(p.reward) + b0);
      const float gq = (float)p.gamma * q;
      p.td[hr] = sum + (double)gq * (double)(p.done[hr] ? 0 : 1);
    }
  }
}

template <int N> static int launch(const Params &p, hipStream_t s) {
  const unsigned blocks = (p.n_steps + (uint32_t)kRows - 1u) / (uint32_t)kRows;
  note_variant("k_ck_qmix_mixer_rows", (int)sizeof(float), N, 4, 0, 0, 0, 0, 0, 0, /* prec=f32 */ 0);
  hipLaunchKernelGGL((k_ck_qmix_mixer_rows<N>), dim3(blocks), dim3(256), 0, s, p);
  CM3_HIP_CHECK(hipGetLastError());
  return CM3_OK;
}

template <int N> static int pack_launch(const PackParams &p, float *out, hipStream_t s) {
  hipLaunchKernelGGL((k_ck_qmix_mixer_pack<N>), dim3(128), dim3(256), 0, s, p, out);
  CM3_HIP_CHECK(hipGetLastError());
  return CM3_OK;
}

template <typename F> static int agents_1_to_8(int n_agents, F &&f) { return agent_launch<1, 2, 3, 4, 5, 6, 7, 8>(n_agents, f); }

static size_t floats_for(int n) {   // (0 for an agent count outside 1..8)
  bool hit;
  return agent_dispatch<1, 2, 3, 4, 5, 6, 7, 8>(n, hit, [&](auto k) { return (size_t)Layout<k()>::kTotal; });
}

static int check_desc(const cm3_qmix_mixer_checkers_desc *d) {
  CM3_REQUIRE(d, "null desc");
  CM3_REQUIRE(d->n_agents >= 1 && d->n_agents <= kMaxAgents, "n_agents must be in 1..%d", kMaxAgents);
  CM3_REQUIRE(d->embed_dim == kE, "the supported embedding width of Qmix_mixer_checkers is %d (networks.py:699); got %d", kE, d->embed_dim);
  CM3_REQUIRE(d->grid_h == 3 && d->grid_w == 9 && d->grid_c == 2, "supported geometry is a 3x9x2 grid; got %dx%dx%d", d->grid_h, d->grid_w,
              d->grid_c);
  CM3_REQUIRE(d->conv_f == kGridF && d->conv_kh == 3 && d->conv_kw == 5,
              "the supported convolution is 4 filters of 3x5 (Q_conv_f, Q_conv_k of config_checkers_stage{1,2}.json); got %d of %dx%d", d->conv_f,
              d->conv_kh, d->conv_kw);
  return CM3_OK;
}
}  // namespace ck_mixer
}  // namespace cm3

extern "C" size_t cm3_qmix_mixer_particle_packed_bytes(int32_t n_agents) { return cm3::mixer_floats_for(n_agents) * sizeof(float); }

extern "C" int cm3_qmix_mixer_particle_pack(const cm3_qmix_mixer_particle_desc *d, const cm3_qmix_mixer_particle_weights *wt, void *packed,
                                            void *stream) {
  using namespace cm3;
  int rc = mixer_check_desc(d);
  if (rc != CM3_OK) return rc;
  CM3_REQUIRE(wt, "null weights");
  CM3_REQUIRE(packed, "packed is NULL: cm3_qmix_mixer_particle_packed_bytes(n_agents) bytes of device memory");
  CM3_REQUIRE(wt->hyper_w_1 && wt->hyper_w_final && wt->hyper_b_1 && wt->hyper_b_final_l1 && wt->hyper_b_final,
              "missing weights: hyper_w_1, hyper_w_final, hyper_b_1, hyper_b_final_l1/kernel, hyper_b_final/kernel");
  CM3_REQUIRE((uintptr_t)packed % 16 == 0, "misaligned packed: must be 16-byte aligned");
  const MixerPackParams p = {wt->hyper_w_1, wt->hyper_w_final, wt->hyper_b_1, wt->hyper_b_final_l1, wt->hyper_b_final};
  hipStream_t s = (hipStream_t)stream;
  return agent_launch_1_to_10(d->n_agents, [&](auto n) { return mixer_pack_launch<n()>(p, (float *)packed, s); });
}

extern "C" int cm3_qmix_mixer_particle_rows_f32(const cm3_qmix_mixer_particle_desc *d, const cm3_qmix_mixer_particle_weights *wt,
                                                const cm3_qmix_mixer_rows *r, void *stream) {
  using namespace cm3;
  int rc = mixer_check_desc(d);
  if (rc != CM3_OK) return rc;
  CM3_REQUIRE(wt, "null weights");
  CM3_REQUIRE(r, "null rows");
  CM3_REQUIRE(wt->packed, "packed weights are NULL: run cm3_qmix_mixer_particle_pack once per weight update");
  CM3_REQUIRE(r->n_steps > 0, "n_steps must be positive");
  CM3_REQUIRE(r->n_steps <= (int64_t)0x7fffffff, "n_steps %lld is more than 2^31 - 1", (long long)r->n_steps);
  CM3_REQUIRE(r->state && r->goals && r->agent_qs, "missing inputs: state, goals and agent_qs are required");
  CM3_REQUIRE(r->q_tot || r->q_tot64 || r->td, "no output requested: set q_tot, q_tot64 or td");
  CM3_REQUIRE(!r->td || (r->reward && r->done), "missing inputs: td needs reward and done");
  CM3_REQUIRE((uintptr_t)r->state % 16 == 0 && (uintptr_t)r->goals % 8 == 0 && (uintptr_t)r->agent_qs % 4 == 0,
              "misaligned inputs: state must be 16-byte aligned, goals 8-byte aligned, agent_qs 4-byte aligned");
  CM3_REQUIRE(!r->td || (uintptr_t)r->reward % (r->reward_f64 ? 8 : 4) == 0, "misaligned reward");
  CM3_REQUIRE((uintptr_t)r->q_tot % 4 == 0 && (uintptr_t)r->q_tot64 % 8 == 0 && (uintptr_t)r->td % 8 == 0,
              "misaligned outputs: q_tot must be 4-byte aligned, q_tot64 and td 8-byte aligned");
  CM3_REQUIRE((uintptr_t)wt->packed % 16 == 0, "misaligned packed: must be 16-byte aligned");
  MixerParams p;
  memset(&p, 0, sizeof(p));
  p.n_steps = (uint32_t)r->n_steps;
  p.state = r->state;
  p.goals = r->goals;
  p.agent_qs = r->agent_qs;
  p.reward = r->reward;
  p.reward_f64 = r->reward_f64;
  p.done = r->done;
  p.gamma = r->gamma;
  p.q_tot = r->q_tot;
  p.q_tot64 = r->q_tot64;
  p.td = r->td;
  p.packed = (const float *)wt->packed;
  hipStream_t s = (hipStream_t)stream;
  return agent_launch_1_to_10(d->n_agents, [&](auto n) { return mixer_launch<n()>(p, s); });
}

extern "C" size_t cm3_qmix_mixer_checkers_packed_bytes(int32_t n_agents) { return cm3::ck_mixer::floats_for(n_agents) * sizeof(float); }

extern "C" int cm3_qmix_mixer_checkers_pack(const cm3_qmix_mixer_checkers_desc *d, const cm3_qmix_mixer_checkers_weights *wt, void *packed,
                                            void *stream) {
  using namespace cm3;
  using namespace cm3::ck_mixer;
  int rc = check_desc(d);
  if (rc != CM3_OK) return rc;
  CM3_REQUIRE(wt, "null weights");
  CM3_REQUIRE(packed, "packed is NULL: cm3_qmix_mixer_checkers_packed_bytes(n_agents) bytes of device memory");
  CM3_REQUIRE(wt->conv_w && wt->conv_b && wt->hyper_w_1 && wt->hyper_w_final && wt->hyper_b_1 && wt->hyper_b_final_l1 && wt->hyper_b_final,
              "missing weights: conv/Conv/weights, conv/Conv/biases, hyper_w_1, hyper_w_final, hyper_b_1, hyper_b_final_l1/kernel, "
              "hyper_b_final/kernel");
  CM3_REQUIRE((uintptr_t)packed % 16 == 0, "misaligned packed: must be 16-byte aligned");
  const PackParams p = {wt->conv_w, wt->conv_b, wt->hyper_w_1, wt->hyper_w_final, wt->hyper_b_1, wt->hyper_b_final_l1, wt->hyper_b_final};
  hipStream_t s = (hipStream_t)stream;
  return agents_1_to_8(d->n_agents, [&](auto n) { return pack_launch<n()>(p, (float *)packed, s); });
}

extern "C" int cm3_qmix_mixer_checkers_rows_f32(const cm3_qmix_mixer_checkers_desc *d, const cm3_qmix_mixer_checkers_weights *wt,
                                                const cm3_qmix_mixer_checkers_rows *r, void *stream) {
  using namespace cm3;
  using namespace cm3::ck_mixer;
  int rc = check_desc(d);
  if (rc != CM3_OK) return rc;
  CM3_REQUIRE(wt, "null weights");
  CM3_REQUIRE(r, "null rows");
  CM3_REQUIRE(wt->packed, "packed weights are NULL: run cm3_qmix_mixer_checkers_pack once per weight update");
  CM3_REQUIRE(r->n_steps > 0, "n_steps must be positive");
  CM3_REQUIRE(r->n_steps <= (int64_t)0x7fffffff, "n_steps %lld is more than 2^31 - 1", (long long)r->n_steps);
  CM3_REQUIRE(r->grid && r->vec && r->goals && r->agent_qs, "missing inputs: grid, vec, goals and agent_qs are required");
  CM3_REQUIRE(r->q_tot || r->q_tot64 || r->td, "no output requested: set q_tot, q_tot64 or td");
  CM3_REQUIRE(!r->td || (r->reward && r->done), "missing inputs: td needs reward and done");
  CM3_REQUIRE((uintptr_t)r->vec % 8 == 0 && (uintptr_t)r->agent_qs % 4 == 0 && (!r->grid_f64 || (uintptr_t)r->grid % 8 == 0) &&
                  (!r->goals_onehot || (uintptr_t)r->goals % 8 == 0),
              "misaligned inputs: vec, a float64 grid and one-hot goals must be 8-byte aligned, agent_qs 4-byte aligned");
  CM3_REQUIRE(!r->td || (uintptr_t)r->reward % (r->reward_f64 ? 8 : 4) == 0, "misaligned reward");
  CM3_REQUIRE((uintptr_t)r->q_tot % 4 == 0 && (uintptr_t)r->q_tot64 % 8 == 0 && (uintptr_t)r->td % 8 == 0,
              "misaligned outputs: q_tot must be 4-byte aligned, q_tot64 and td 8-byte aligned");
  CM3_REQUIRE((uintptr_t)wt->packed % 16 == 0, "misaligned packed: must be 16-byte aligned");
  Params p;
  memset(&p, 0, sizeof(p));
  p.n_steps = (uint32_t)r->n_steps;
  p.grid_f64 = r->grid_f64;
  p.goals_onehot = r->goals_onehot;
  p.reward_f64 = r->reward_f64;
  p.grid = r->grid;
  p.vec = r->vec;
  p.goals = r->goals;
  p.agent_qs = r->agent_qs;
  p.reward = r->reward;
  p.done = r->done;
  p.gamma = r->gamma;
  p.q_tot = r->q_tot;
  p.q_tot64 = r->q_tot64;
  p.td = r->td;
  p.packed = (const float *)wt->packed;
  hipStream_t s = (hipStream_t)stream;
  return agents_1_to_8(d->n_agents, [&](auto n) { return launch<n()>(p, s); });
}
