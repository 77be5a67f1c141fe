// A whole POLICY-DRIVEN episode in one launch: actor forward pass (matrix cores) + epsilon-mixed sampling + physics
// step + observation, tick after tick, with the network weights, the input tile and the env state resident in
// LDS / registers.
//
// Reference loop being replaced (alg/train_onpolicy.py:302-350, the branch taken for 49 950 of its 50 000 episodes):
//     actions = alg.run_actor(local_others, local_self, goals, epsilon, sess)      :313   (alg_credit.py:249-270)
//     next_... = env.step(actions)                                                 :323   (environment.py:81-123)
//     buf.add(transition) ; roll state forward                                     :338-347
// The unfused device path (ParticleRollout.collect(policy=actor)) alternates k_actor_particle and
// k_particle_step_pairs launches inside a hipGraph: 12.9 us per tick at 4096 envs x 4 agents, of which ~3.8k cycles
// re-stage the weights, ~3 us are launch boundaries and ~2 us re-load state/observations.  Here a workgroup owns
// 64 agent rows = 64/N whole envs for all T ticks:
//   * weights: first-layer tables + output layer in LDS, W2 B-operands in VGPRs -- staged ONCE per launch;
//   * per tick: actor_mlp (phase A / phase B on the matrix cores, 2 or 3 barriers) -> head: probabilities + action of row
//     16w + (l&15) in the 16 "part 0" lanes of wave w -> the same lanes advance their agent: own-side contact forces
//     against the other agents of the env (positions read from the LDS input tile), integration, reward / collision /
//     reached, per-env reductions with wave shuffles, optional same-tick re-initialisation, and the next observation is
//     written both to the trajectory (global) and back into the LDS tile that feeds the next tick's phase A.
// Arithmetic per agent is the reference's operation order, so trajectories are bit-identical to the unfused path
// (tests/test_gpu_actor.py::test_fused_policy_rollout_equals_launch_per_tick).
//
// Agent counts: a wave's 16-row tile holds 16 / N whole envs (policy_tiles.h).  N in {1, 2, 4, 8} fill it; N in {3, 5, 6, 7, 9, 10}
// leave pad rows that nobody owns -- float32 envs and the CM3 actor only, built in a translation unit of their own (build.sh compiles
// this file a third time with -DCM3_POLICY_PARTIAL_TILES; see policy_partial_launch).  Same bits as the launch pairs
// (tests/test_gpu_policy_partial_tiles.py).
//
// float64 envs (VecParticleEnv(dtype=torch.float64), the reference-precision mode): build.sh compiles this file twice, with
// -DCM3_PARTICLE_F32 and -DCM3_PARTICLE_F64, and PolicyReal below is the real of the env side -- state, contact chain,
// integration, reward / collision / reached, re-initialisation and every trajectory store.  The network is float32 in both (the
// reference feeds its float64 observations into tf.float32 placeholders, alg_credit.py:96-111): the next tick's observation is
// rounded into the float32 input tile on the way in, exactly as k_actor_particle<., ., double> stages it from the env's buffers.
// What the physics reads back is never that rounded tile: in float64 the rows' pre-step state lives in the double exchange slots
// `ns` and their goals in `gd` (see the kernel), so an f64 episode is bit-identical to alternating cm3_actor_particle_f64 and
// cm3_particle_step_f64 launches.
//
// QMIX mode (k_policy_rollout<N, kPrecF32, 4, float, true>, float32 build only; cm3_policy_rollout_qmix_f32): the QMIX baseline's
// agent network (networks.Qmix_single_particle, k_qmix_particle in actor.hip) and its epsilon-greedy choice in the CM3 actor's
// place; everything from "physics of agent i" to the closing barrier is the same text.  What differs:
//   * LDS: qmix_forward's tiles xs[64][K1+1], h1s[64][66], h2s[64][66] (QmixLayout<N>) instead of the actor's tables, 38 - 43 KB;
//   * row tiles: RT = 4 only -- 64 rows per workgroup, wave w owns rows 16w .. 16w+15, part 0 (lanes 0..15) writes;
//     cm3_policy_force_row_tiles does not apply (no 32- or 16-row build of this mode exists);
//   * weights: every lane's operands of the three layers (cm3_qmix_particle_pack's buffer) are loaded ONCE per launch and stay in
//     registers for all ticks, ~55 VGPRs next to the 16 accumulators;
//   * per tick: the three layers of qmix_forward -- the same matrix instruction, k grouping and start values, so every Q value
//     is the same k-ordered chain and the same bits as k_qmix_particle's -- then epsilon-greedy on the exploration words of
//     (seed, global env id, the row's episode, its pre-step steps, agent): what k_qmix_particle reads from meta / episode at that
//     tick, also after a same-tick reset.  Three barriers per tick: after "h", after "h2", the closing one;
//   * the input tile's columns: concat(others[L], self[4], goal[2], 0, 0) instead of self, goal, others -- the env phase reaches
//     the tile through three column offsets (kXSelf / kXGoal / kXOth); the two zero pads are written once per launch;
//   * q.probs receives the raw Q values, epsilon comes from q.eps_dev when given (read once at entry).
// Bit-identical to alternating cm3_qmix_particle_f32 and cm3_particle_step_f32 launches (tests/test_gpu_qmix_particle_episode.py).
#define CM3_NO_ENTRY_POINTS 1
#if !defined(CM3_PARTICLE_F32) && !defined(CM3_PARTICLE_F64)
#define CM3_PARTICLE_F32 1
#endif
#if defined(CM3_PARTICLE_F32) && !defined(CM3_POLICY_PARTIAL_TILES)
#define CM3_POLICY_ENTRY_F32 1   // the translation unit that holds the float32 entry points (see policy_partial_launch)
#endif
#include "particle.hip"
#include "actor.hip"
#include "policy_tiles.h"
#include <stdlib.h>
#include <atomic>

namespace cm3 {

#ifdef CM3_PARTICLE_F64
using PolicyReal = double;
#else
using PolicyReal = float;
#endif

struct PolicyParams {
  ParticleParams p;  // trajectory pointers/strides of the fused rollout (state_in = slot 0, *_out = slot 1 ...)
  const void *obs_in;   // obs_others slot 0 (PolicyReal)
  const float *packed;
  float *probs;         // optional [T][E][N][5]
  size_t st_probs;
  float eps;
  int stage;
  const float *eps_dev;   // QMIX mode, optional: epsilon read at entry instead of eps
};

// ---- QMIX mode: the three layers of qmix_forward (actor.hip) once more, as device functions of this kernel.  A COPY, not a shared
// text: with the layers of qmix_forward moved into these functions, every k_qmix_particle / k_qmix_particle_rows build came out with
// another instruction schedule (up to 12 instructions more, 650 - 1060 differing lines per kernel), so qmix_forward keeps its text and
// the rollout has its own.  What must stay equal between the two is what the bits rest on: v_mfma_f32_16x16x4_f32, k = 4s .. 4s+3
// per step in ascending s, and the start values (bias as C for "h" and "out", zero then + b2 for "h2").
template <int N> struct QmixW {
  float a1[QmixLayout<N>::S1P], bw[16], wo[16];   // layer-1 A operands, layer-2 B operands, the head's A operands of this lane
  float4 b1;                                      // units 16w + 4 (l>>4) + 0..3
  float b2;                                       // unit 16w + (l&15)
  float4 bo;                                      // actions 4 (l>>4) + 0..3
};
template <int N> __device__ __forceinline__ void qmix_load_w(const float *packed, int w, int lane, QmixW<N> &k) {
  using QL = QmixLayout<N>;
  const int col = lane & 15, hi = lane >> 4;
  const float4 *src = reinterpret_cast<const float4 *>(packed + QL::kW1) + (size_t)(w * 64 + lane) * (QL::S1P / 4);
#pragma unroll
  for (int s4 = 0; s4 < QL::S1P / 4; ++s4) {
    const float4 v = src[s4];
    k.a1[4 * s4 + 0] = v.x; k.a1[4 * s4 + 1] = v.y; k.a1[4 * s4 + 2] = v.z; k.a1[4 * s4 + 3] = v.w;
  }
  const float4 *s2 = reinterpret_cast<const float4 *>(packed + QL::kW2) + (size_t)(w * 64 + lane) * 4;
  const float4 *so = reinterpret_cast<const float4 *>(packed + QL::kWo) + (size_t)lane * 4;
#pragma unroll
  for (int s4 = 0; s4 < 4; ++s4) {
    const float4 v = s2[s4], u = so[s4];
    k.bw[4 * s4 + 0] = v.x; k.bw[4 * s4 + 1] = v.y; k.bw[4 * s4 + 2] = v.z; k.bw[4 * s4 + 3] = v.w;
    k.wo[4 * s4 + 0] = u.x; k.wo[4 * s4 + 1] = u.y; k.wo[4 * s4 + 2] = u.z; k.wo[4 * s4 + 3] = u.w;
  }
  k.b1 = reinterpret_cast<const float4 *>(packed + QL::kB1)[4 * w + hi];
  k.b2 = packed[QL::kB2 + 16 * w + col];
  k.bo = reinterpret_cast<const float4 *>(packed + QL::kBo)[hi];
}
// layer "h": units [16w, 16w+16) for all 64 rows, C[unit][row]
template <int N> __device__ __forceinline__ void qmix_layer_h(const QmixW<N> &k, const float (*xs)[QmixLayout<N>::XW],
                                                              float (*h1s)[QmixLayout<N>::HS], int w, int lane) {
  const int col = lane & 15, hi = lane >> 4;
  f32x4 c[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) c[t] = f32x4{k.b1.x, k.b1.y, k.b1.z, k.b1.w};
#pragma unroll
  for (int s = 0; s < QmixLayout<N>::S1; ++s)
#pragma unroll
    for (int t = 0; t < 4; ++t) c[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(k.a1[s], xs[16 * t + col][4 * s + hi], c[t], 0, 0, 0);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    *reinterpret_cast<float2 *>(&h1s[16 * t + col][16 * w + 4 * hi]) = make_float2(relu_f32(c[t][0]), relu_f32(c[t][1]));
    *reinterpret_cast<float2 *>(&h1s[16 * t + col][16 * w + 4 * hi + 2]) = make_float2(relu_f32(c[t][2]), relu_f32(c[t][3]));
  }
}
// layer "h2": columns [16w, 16w+16), C[row][unit]
template <int N> __device__ __forceinline__ void qmix_layer_h2(const QmixW<N> &k, const float (*h1s)[QmixLayout<N>::HS],
                                                               float (*h2s)[QmixLayout<N>::HS], int w, int lane) {
  const int col = lane & 15, hi = lane >> 4;
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int s = 0; s < kQH / 4; ++s)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(h1s[16 * t + col][4 * s + hi], k.bw[s], acc[t], 0, 0, 0);
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) h2s[16 * t + 4 * hi + reg][16 * w + col] = relu_f32(acc[t][reg] + k.b2);
}
// head "out": C[action][row] of rows [16w, 16w+16), one k-ordered chain; lanes 0..15 end with all five Q values of their row
template <int N> __device__ __forceinline__ void qmix_head_q(const QmixW<N> &k, const float (*h2s)[QmixLayout<N>::HS], int w, int lane,
                                                             float (&q)[kA]) {
  const int col = lane & 15, hi = lane >> 4;
  float hx[kQH / 4];
#pragma unroll
  for (int s = 0; s < kQH / 4; ++s) hx[s] = h2s[16 * w + col][4 * s + hi];
  f32x4 acc = f32x4{k.bo.x, k.bo.y, k.bo.z, k.bo.w};
#pragma unroll
  for (int s = 0; s < kQH / 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(k.wo[s], hx[s], acc, 0, 0, 0);
#pragma unroll
  for (int a = 0; a < 4; ++a) q[a] = acc[a];
  // action 4 of the row sits in register 0 of the lane 16 further on (see actor_head_probs)
  uint32_t x;
  __builtin_memcpy(&x, &q[0], 4);
  const auto sw = __builtin_amdgcn_permlane16_swap(x, x, false, false);
  const uint32_t y = sw[1];
  __builtin_memcpy(&q[4], &y, 4);
}

// RT = 16-row tiles per workgroup: 4 (64 agent rows) where that already gives every CU several workgroups; 2 or 1 for smaller
// batches, so that two or more workgroups share a CU and one's matrix-core phases run under the other's physics / LDS staging
// (round 4: the per-env chain actor -> physics -> observation is serial, and at one wave per SIMD the tick was latency-bound:
// ~1 us of matrix time inside 5.0 us).  Waves w >= RT take part in the layers (every wave owns 16 columns of all row tiles) and
// in the barriers, but have no rows of their own in the head and the physics.
// R = the env's real (PolicyReal of the translation unit).  R = double: the physics reads its own and the other agents' pre-step
// state from `ns` (double, written at the end of every tick) and the goals from `gd`, never from the float32 input tile; the
// wave's post-step exchange goes through the same `ns` slots.  +3 KB of LDS at 64 rows, the per-env reductions by shuffles.
// Element [r][c] of the rollout's input tile: the actor's (lds.xs) or the QMIX mode's (q_xs), whose rows differ in width.  A function
// of the two declarations, called where the tile is touched -- not a pointer variable set once, not a lambda: with either, the float32
// actor builds of two, four and eight agents came out with permuted registers or a commuted operand.
template <bool QMIX, typename A, typename B> __device__ __forceinline__ float &policy_tile(A actor_xs, B &qmix_xs, int r, int c) {
  if constexpr (QMIX) return qmix_xs[r][c];
  else return actor_xs[r][c];
}
#define XS(r, c) policy_tile<QMIX>(lds.xs, q_xs, r, c)   // (inside k_policy_rollout only; undefined after it)
// QMIX: the QMIX agent's network and epsilon-greedy choice instead of the CM3 actor (see the head of this file)
template <int N, int BF16, int RT, typename R, bool QMIX = false> __global__ void CM3_MATRIX_KERNEL k_policy_rollout(const PolicyParams q) {
  using G = ActorGeom<N, BF16, RT>;
  using QL = QmixLayout<N>;
  using V4 = typename Vec<R>::v4;
  using V2 = typename Vec<R>::v2;
  constexpr bool F64 = sizeof(R) == 8;
  static_assert(!QMIX || (RT == 4 && !F64 && BF16 == kPrecF32), "QMIX mode: 64-row workgroups, float32 env, float32 network");
  constexpr int L = G::L, NO = N > 1 ? N - 1 : 1;
  // the input tile's columns: the actor reads (self, goal, others), the QMIX agent concat(others, self, goal, 0, 0)
  constexpr int kXSelf = QMIX ? L : 0, kXGoal = kXSelf + 4, kXOth = QMIX ? 0 : 6;
  const ParticleParams &p = q.p;
  // (every mode declares both sets of LDS arrays and uses one: an array without a use is not allocated -- see the LDS sizes in
  // policy.resource_usage.txt, 38 - 43 KB per workgroup in QMIX mode)
  CM3_ACTOR_LDS_RT(N, BF16, RT, lds);
  __shared__ float q_xs[64][QL::XW];
  __shared__ __attribute__((aligned(16))) float q_h1s[64][QL::HS];
  __shared__ float q_h2s[64][QL::HS];
  __shared__ __attribute__((aligned(16))) V4 ns[16 * RT];  // post-step (vx, vy, px, py) of every row, exchanged inside a wave
  __shared__ __attribute__((aligned(16))) V2 gd[F64 ? 16 * RT : 1];   // float64: the rows' goals (float32 reads them from the tile)
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const size_t E = (size_t)p.E;
  const size_t rows = E * N;
  const size_t row_base = (size_t)blockIdx.x * (16 * RT);
  CM3_STAMP(13, false);   // kernel entry (probes only)

  // the row this lane owns in the head and in the physics: rl = 16w + (l&15); only part 0 (l < 16) of the waves w < RT writes
  // Which waves own rows: w < RT -- and, for two-tile workgroups, waves 2, 3 in every other group of 256 workgroups.  Wave w of a
  // workgroup runs on SIMD w of its CU, and two such workgroups share a CU once a batch has more than 256 of them (workgroup b and
  // b + 256, as the dispatcher fills the chip): the head and the physics of both would otherwise pile up on SIMDs 0 and 1 while
  // SIMDs 2 and 3 idle for 60 % of every tick (stamped build, profiles/r04_policy_row_tiles.txt).  Speed only: results do not
  // depend on the placement.
  const int wr = RT == 2 ? ((w + 2 * (int)((blockIdx.x >> 8) & 1u)) & 3) : w;
  const bool row_wave = wr < RT;
  // N in {1, 2, 4, 8}: a tile is 16 / N whole envs, no row is padded, and a row behind the batch repeats the last one.
  // Other N (policy_tiles.h): a tile holds 16 / N whole envs in its first rows_used rows; a lane whose row is a pad row, or whose
  // env lies behind the batch, owns nothing (row_ok false) and MIRRORS ROW 0 OF ITS TILE as lanes 16..63 mirror lane l & 15 --
  // rl, i and env_lane0 are row 0's, so every row it reads (rl - i + j, the per-env shuffles) is a row of its own tile, and
  // (e, i) is a pair of the batch for its entry loads.  `tile_store` guards every LDS store of a row: pad lanes store nothing.
  int rl_, i_, env_lane0_;
  size_t r_, e_;
  bool row_ok_, part0_;
  if constexpr (policy_tile_is_dense(N)) {
    rl_ = row_wave ? 16 * wr + (lane & 15) : (lane & 15);
    part0_ = (lane >> 4) == 0 && row_wave;
    r_ = row_base + rl_;
    row_ok_ = r_ < rows;
    r_ = row_ok_ ? r_ : rows - 1;
    e_ = r_ / N;
    i_ = (int)(r_ - e_ * N);
    env_lane0_ = (lane & 15) - i_;  // lane (within the wave's part 0) of agent 0 of this env
  } else {
    (void)rows;
    (void)row_base;
    part0_ = (lane >> 4) == 0 && row_wave;
    const int wt = row_wave ? wr : 0;
    const PolicyTileRow tr = policy_tile_row(policy_tile_of(blockIdx.x, wt, RT), lane & 15, N, E);
    rl_ = 16 * wt + tr.local_row;
    row_ok_ = tr.owns;
    e_ = tr.env;
    i_ = tr.agent;
    r_ = e_ * N + (size_t)i_;
    env_lane0_ = tr.local_row - tr.agent;
  }
  const int rl = rl_, i = i_, env_lane0 = env_lane0_;
  const size_t r = r_, e = e_;
  const bool row_ok = row_ok_, part0 = part0_;
  const uint64_t genv = (uint64_t)(p.env_id_base + (int64_t)e);
  const bool writer = row_ok && part0;
  const bool head_lane = writer && i == 0;
  bool tile_store_ = part0;   // who stores row rl of `ns` and of the input tile
  if constexpr (!policy_tile_is_dense(N)) tile_store_ = writer;
  const bool tile_store = tile_store_;

  // ---- once per launch: weights, live counters, the input tile ---------------------------------------------------------
  // every global request of the entry first (tables, the wave's W2 slice, counters, the rows' state / goals / observation), the
  // sampling key's Philox block while they are in flight, then the LDS stores: one memory round trip before the barrier
  // (the W2 slice first: it keeps its registers for the whole launch, and requested after the table copy the register allocator
  // parked the copy in those very registers -- a wait for the tables, a move, and only then the slice's requests)
  ActorB<N, BF16> b;
  ActorTabRegs<N> tab;
  QmixW<N> qw;
  if constexpr (QMIX) {
    qmix_load_w<N>(q.packed, w, lane, qw);   // the lane's operands of all three layers, for the whole launch
  } else {
    actor_load_b<N, BF16>(q.packed, w, lane, b);
    actor_tables_fetch<N>(q.packed, tid, tab);
  }
  const int2 meta = reinterpret_cast<const int2 *>(p.meta_in)[e];
  const bool auto_reset = (p.flags & CM3_FLAG_AUTO_RESET) != 0;
  uint32_t episode = (uint32_t)p.episode[e];
  V4 s0, o0[L / 4];   // (every lane requests its row -- lanes outside part 0 repeat one of part 0's -- rather than branch)
  V2 g0;
  {
    s0 = reinterpret_cast<const V4 *>(p.state_in)[(size_t)i * E + e];
    g0 = reinterpret_cast<const V2 *>(p.goals_in)[(size_t)i * E + e];
    const V4 *o4 = reinterpret_cast<const V4 *>(reinterpret_cast<const R *>(q.obs_in) + r * L);
#pragma unroll
    for (int k = 0; k < L / 4; ++k) o0[k] = o4[k];
  }
  // stage 1 of the actor's sampling uniforms, once per launch (actor_common.h); QMIX mode: epsilon, read once
  uint32_t ublock = 0;
  uint2 xblock = make_uint2(0u, 0u);
  float q_eps = 0.0f;
  if constexpr (QMIX) {
    q_eps = q.eps_dev ? *q.eps_dev : q.eps;
  } else {
    ublock = actor_block_word(p.seed, genv, i);
  }
  int steps = meta.x, collisions = meta.y;
  const uint32_t episode_in = episode;
  if constexpr (!QMIX) actor_tables_store<N, BF16, RT>(lds, tid, tab);
  if constexpr (!policy_tile_is_dense(N)) {
    // the rows nobody owns: zeros once per launch, in the input tile and in `ns`, so that the hidden planes of the pad rows and what
    // a pad lane of an empty tile computes never depend on what the LDS held before (no owned row's value depends on them either
    // way: the rows of a matrix product are independent)
    if (part0 && !row_ok) {
      const int pad = 16 * wr + (lane & 15);
#pragma unroll
      for (int c = 0; c < 6 + L; ++c) XS(pad, c) = 0.0f;
      V4 zero;
      zero.x = zero.y = zero.z = zero.w = R(0);
      ns[pad] = zero;
    }
  }
  if (tile_store) {
    XS(rl, kXSelf + 0) = (float)s0.x; XS(rl, kXSelf + 1) = (float)s0.y; XS(rl, kXSelf + 2) = (float)s0.z; XS(rl, kXSelf + 3) = (float)s0.w;
    XS(rl, kXGoal + 0) = (float)g0.x; XS(rl, kXGoal + 1) = (float)g0.y;
#pragma unroll
    for (int k = 0; k < L / 4; ++k) {
      XS(rl, kXOth + 4 * k + 0) = (float)o0[k].x; XS(rl, kXOth + 4 * k + 1) = (float)o0[k].y;
      XS(rl, kXOth + 4 * k + 2) = (float)o0[k].z; XS(rl, kXOth + 4 * k + 3) = (float)o0[k].w;
    }
    if constexpr (QMIX) {   // the two zero pads of the last k-step: once per launch, the env phase never writes them
      XS(rl, L + 6) = 0.0f;
      XS(rl, L + 7) = 0.0f;
    }
    if constexpr (F64) {
      ns[rl] = s0;
      gd[rl] = g0;
    }
  }
  __syncthreads();
  CM3_STAMP(14, true);    // tables, weights and the input tile are in
  // QMIX mode draws stage 1 of its exploration words here, behind the barrier (drawn ahead of it, next to the entry's loads, the
  // one-agent build reserved 52 bytes of scratch per lane that no instruction touched)
  if constexpr (QMIX) xblock = explore_block_words(p.seed, genv, i);
  ActorHeadB hb;
  ActorFirstB<N> f1;
  if constexpr (!F64 && !QMIX) {
    actor_head_load(lds.wout, lane, hb);      // output-layer operands of this lane, once per launch
    actor_first_b<N, float>(&lds.ws_self[0][0], &lds.ws_oth[0][0], w, lane, q.stage > 1, f1);  // ... and its first-layer operands
                                              // (round 4: they were re-read from LDS every tick)
  }

  const R kDt = R(0.1), kKeep = R(1) - R(0.25);
#pragma unroll 1
  for (int t = 0; t < p.n_ticks; ++t) {
    // ---- policy: forward pass, probabilities and the sampled action of row rl (alg_credit.py:113-122) -----------------
    CM3_STAMP(0, false);
    // float64: the operands of the first layer and the head are read from the LDS tables every tick (the float32 build holds them
    // for the whole launch): their 40 (N = 4) to 56 (N = 8) registers are what the double physics and the re-initialisation's
    // double transcendentals need -- held, every f64 build spilled (20 - 340 bytes of scratch per lane)
    if constexpr (QMIX) {
      qmix_layer_h<N>(qw, q_xs, q_h1s, w, lane);
      __syncthreads();
      qmix_layer_h2<N>(qw, q_h1s, q_h2s, w, lane);
      __syncthreads();
    } else {
      if constexpr (F64) actor_first_b<N, float>(&lds.ws_self[0][0], &lds.ws_oth[0][0], w, lane, q.stage > 1, f1);
      actor_mlp<N, BF16, RT>(lds, b, f1, w, lane, q.stage > 1);
    }
    if (row_wave) {   // (wave-uniform; no workgroup barrier inside)
    // The head, the physics and the stores of the rows are the part of the tick only this wave can do while its workgroup waits at
    // the closing barrier: it goes first on its SIMD, ahead of the matrix phases of the workgroup that shares the CU (measured,
    // same box, three alternating rounds: 4.31 -> 4.15 us per tick at 4 096 x 4, 45.1 -> 44.6 at 65 536 x 4; levels 1, 2, 3 are
    // the same, raising the priority for the WHOLE tick loses the gain; profiles/r04_policy_head.txt)
    __builtin_amdgcn_s_setprio(2);
    float pr[kA];   // the row's probabilities; QMIX mode: its raw Q values
    int act;
    // (either head leaves the row's values in lanes 0..15 only; lanes 16..63 repeat the physics of lane l & 15 and get its
    // action so that they take the same branches -- nothing they compute is stored: see the exchange slot below)
    if constexpr (QMIX) {
      // exploration words first: the Philox mixing is VALU work that issues between the head's dependent matrix instructions
      uint32_t w_explore, w_action;
      explore_words_from(xblock, episode, (uint32_t)steps, w_explore, w_action);
      qmix_head_q<N>(qw, q_h2s, wr, lane, pr);
      act = bcast_row0(epsilon_greedy(pr, q_eps, w_explore, w_action));
    } else {
      const float u = actor_uniform_from(ublock, episode, steps);
      if constexpr (F64) actor_head_load(lds.wout, lane, hb);
      actor_head_probs(lds.h2s, hb, wr, lane, q.eps, pr);
      act = bcast_row0(actor_pick(pr, u));
    }
    CM3_STAMP(7, false);

    // ---- physics of agent i (environment.py:81-123), lanes of part 0 ------------------------------------------------------
    V4 si;
    V2 gl;
    if constexpr (F64) {
      si = ns[rl];
      gl = gd[rl];
    } else {
      si.x = XS(rl, kXSelf + 0); si.y = XS(rl, kXSelf + 1); si.z = XS(rl, kXSelf + 2); si.w = XS(rl, kXSelf + 3);
      gl.x = XS(rl, kXGoal + 0); gl.y = XS(rl, kXGoal + 1);
    }
    R ux = R(0), uy = R(0);
    if (act == 1) ux = R(-1);
    if (act == 2) ux = R(+1);
    if (act == 3) uy = R(-1);
    if (act == 4) uy = R(+1);
    R Fx = ux * R(5.0) + R(0.0), Fy = uy * R(5.0) + R(0.0);
#pragma unroll
    for (int k = 0; k < N - 1; ++k) {  // the reference's accumulation order: other agents ascending (core.py:145-155)
      const int j = k < i ? k : k + 1;
      const int rj = rl - i + j;
      R f_x, f_y;
      if constexpr (F64)
        contact_force<R>(si.z - ns[rj].z, si.w - ns[rj].w, f_x, f_y);
      else
        contact_force<R>(si.z - XS(rj, kXSelf + 2), si.w - XS(rj, kXSelf + 3), f_x, f_y);
      Fx = f_x + Fx;
      Fy = f_y + Fy;
    }
    si.x = si.x * kKeep;
    si.y = si.y * kKeep;
    si.x = si.x + (Fx / R(1.0)) * kDt;
    si.y = si.y + (Fy / R(1.0)) * kDt;
    si.z = si.z + si.x * kDt;
    si.w = si.w + si.y * kDt;
    steps += 1;
    // (one 16-byte LDS store; the other agents' rows come back as 16-byte reads, once, for collisions AND observation.  Lanes 0..15
    // only: lanes 16..63 repeat their physics and used to store their copy into the same slot -- the same value by the code,
    // but this way nothing a copy computes is ever stored.  Round 5 found what made copies differ: a packed multiply of the contact
    // chain returning a wrong low half in lanes 48..63 under a co-resident matrix wave, profiles/r05_policy_fault.txt)
    if constexpr (F64) wave_lds_sync();   // float64: every lane has read the pre-step rows from `ns` before they are overwritten
    if (tile_store) ns[rl] = si;
    wave_lds_sync();  // the other agents of this env live in the same wave
    V4 oth[NO];
    if constexpr (!F64) {
#pragma unroll
      for (int k = 0; k < NO; ++k) {
        const int j = (N > 1) ? (k < i ? k : k + 1) : 0;
        oth[k] = ns[rl - i + j];
      }
    }
    // the post-step state of the k-th other agent: float64 reads it from `ns` where it is used (seven double4 held from here to the
    // observation stores are 56 registers at N = 8); `ns` holds the reset states once a re-initialisation has written them
    auto other = [&](int k) -> V4 {
      if constexpr (F64) {
        const int j = (N > 1) ? (k < i ? k : k + 1) : 0;
        return ns[rl - i + j];
      } else {
        return oth[k];
      }
    };

    CM3_STAMP(8, false);
    // ---- reward / reached / collisions (multi-goal_spread.py:114-143) ----------------------------------------------------------
    R rew;
    bool reached;
    {
      const R dx = si.z - gl.x, dy = si.w - gl.y;
      const R d2 = dx * dx + dy * dy;
      rew = R(0) - Math<R>::sqrt(d2);
      reached = d2 < Thresh<R>::kReach2;  // rew >= -0.05 (thresholds.h)
    }
    int hits = 0;
#pragma unroll
    for (int k = 0; k < N - 1; ++k) {
      const V4 ok = other(k);
      if (is_collision<R>(ok.z - si.z, ok.w - si.w)) {  // is_collision(a = j, agent = i)
        rew = rew - R(1);
        hits += 1;
      }
    }
    R rews[N];
    int hit_sum = 0;
    bool all_reached = true;
    if constexpr (N == 4 && !F64) {  // the env's four agents are one DPP quad: broadcasts and sums without the LDS crossbar
      rews[0] = dpp_f32<0x00>(rew);
      rews[1] = dpp_f32<0x55>(rew);
      rews[2] = dpp_f32<0xAA>(rew);
      rews[3] = dpp_f32<0xFF>(rew);
      hit_sum = hits + dpp_i32<kDppXor1>(hits);
      hit_sum += dpp_i32<kDppXor2>(hit_sum);
      int r4 = (int)reached;
      r4 &= dpp_i32<kDppXor1>(r4);
      r4 &= dpp_i32<kDppXor2>(r4);
      all_reached = r4 != 0;
    } else if constexpr (N == 8 && !F64) {  // an env is half a DPP row: sums over its 8 lanes by xor 1, xor 2, half mirror (lane i <-> 7 - i)
      hit_sum = hits + dpp_i32<kDppXor1>(hits);
      hit_sum += dpp_i32<kDppXor2>(hit_sum);
      hit_sum += dpp_i32<kDppHalfMirror>(hit_sum);
      int r8 = (int)reached;
      r8 &= dpp_i32<kDppXor1>(r8);
      r8 &= dpp_i32<kDppXor2>(r8);
      r8 &= dpp_i32<kDppHalfMirror>(r8);
      all_reached = r8 != 0;
    } else {
#pragma unroll
      for (int a = 0; a < N; ++a) {  // per-env reductions over the N part-0 lanes of this env
        rews[a] = __shfl(rew, env_lane0 + a, 64);
        hit_sum += __shfl(hits, env_lane0 + a, 64);
        all_reached = all_reached && (__shfl((int)reached, env_lane0 + a, 64) != 0);
      }
    }
    collisions += hit_sum;
    R reward;
    if constexpr (N == 8 && !F64) {
      // NumPy's pairwise tree for 8 values, ((v0+v1)+(v2+v3)) + ((v4+v5)+(v6+v7)) (sum_agents), by the same three DPP steps: every
      // partial sum meets its partner with the operands possibly swapped, and float addition is commutative bit for bit
      float tsum = rew + dpp_f32<kDppXor1>(rew);
      tsum = tsum + dpp_f32<kDppXor2>(tsum);
      reward = tsum + dpp_f32<kDppHalfMirror>(tsum);
    } else {
      reward = sum_agents<R, N>(rews);
    }
    const bool done = (steps == p.max_steps) || all_reached;
    if (head_lane) {
      reinterpret_cast<R *>(tick_ptr(p.reward, p.st_reward, t))[e] = reward;
      tick_ptr(p.done, p.st_done, t)[e] = done ? 1 : 0;
      if (p.collisions_tick) tick_ptr(p.collisions_tick, p.st_coll, t)[e] = collisions;
    }

    CM3_STAMP(9, false);
    // ---- same-tick re-initialisation of finished episodes (CM3_FLAG_AUTO_RESET) ------------------------------------------------
    bool was_reset = false;
    if (auto_reset && done) {
      void *term_state = tick_ptr(p.term_state, p.st_term_state, t);
      void *term_obs = tick_ptr(p.term_obs_others, p.st_term_obs, t);
      if (writer && term_state) reinterpret_cast<V4 *>(term_state)[(size_t)i * E + e] = si;
      if (writer && term_obs) {
        V4 *o = reinterpret_cast<V4 *>(term_obs) + r * NO;
#pragma unroll
        for (int k = 0; k < NO; ++k) {
          const int j = (N > 1) ? (k < i ? k : k + 1) : 0;
          (void)j;
          o[k] = sub4<R, V4>(other(k), si);
        }
      }
      wave_lds_sync();  // every lane of the env has read the terminal states before they are overwritten
      episode += 1;
      const bool rnd = episode_is_random(p, genv, episode);
      static_assert(offsetof(PolicyParams, p) == 0, "preset_table(0): the ParticleParams lead the kernel's only argument");
      init_agent<R, N, true>(p, genv, episode, rnd, i, si, gl, preset_table(0));
      steps = 0;
      collisions = 0;
      was_reset = true;
      if (tile_store) ns[rl] = si;
      wave_lds_sync();
    }
    if (!F64 && auto_reset && __any(done)) {  // fresh episodes in this wave: the observation is that of the reset states
#pragma unroll
      for (int k = 0; k < NO; ++k) {
        const int j = (N > 1) ? (k < i ? k : k + 1) : 0;
        oth[k] = ns[rl - i + j];
      }
    }

    CM3_STAMP(10, false);
    // ---- trajectory stores + the LDS tile of the next tick ---------------------------------------------------------------------
    if (tile_store) {
      if (row_ok) {   // every per-row store of the tick in ONE exec region (the action, its probabilities and the reward used to have
                      // regions of their own further up: ~6 scalar instructions and a branch each on the row waves' path)
        tick_ptr(p.actions, p.st_actions, t)[r] = act;
        if (q.probs) {
          float *pt = tick_ptr(q.probs, q.st_probs, t) + r * kA;
#pragma unroll
          for (int a = 0; a < kA; ++a) pt[a] = pr[a];
        }
        reinterpret_cast<R *>(tick_ptr(p.reward_n, p.st_reward_n, t))[r] = rew;
        reinterpret_cast<V4 *>(tick_ptr(p.state_out, p.st_state, t))[(size_t)i * E + e] = si;
        if (p.goals_out != p.goals_in || was_reset)
          reinterpret_cast<V2 *>(tick_ptr(p.goals_out, p.st_goals, t))[(size_t)i * E + e] = gl;
      }
      V4 *o = reinterpret_cast<V4 *>(tick_ptr(p.obs_others, p.st_obs, t)) + r * NO;
#pragma unroll
      for (int k = 0; k < NO; ++k) {  // observation (multi-goal_spread.py:145-154)
        const int j = (N > 1) ? (k < i ? k : k + 1) : 0;
        (void)j;
        const V4 d = sub4<R, V4>(other(k), si);
        if (row_ok) o[k] = d;
        XS(rl, kXOth + 4 * k + 0) = (float)d.x; XS(rl, kXOth + 4 * k + 1) = (float)d.y;
        XS(rl, kXOth + 4 * k + 2) = (float)d.z; XS(rl, kXOth + 4 * k + 3) = (float)d.w;
      }
      XS(rl, kXSelf + 0) = (float)si.x; XS(rl, kXSelf + 1) = (float)si.y; XS(rl, kXSelf + 2) = (float)si.z; XS(rl, kXSelf + 3) = (float)si.w;
      XS(rl, kXGoal + 0) = (float)gl.x; XS(rl, kXGoal + 1) = (float)gl.y;
      if constexpr (F64) gd[rl] = gl;   // (ns[rl] already holds si: the post-step store above, or the reset's)
    }
    CM3_STAMP(11, false);
    __builtin_amdgcn_s_setprio(0);
    }  // row_wave
    __syncthreads();  // the tile (and the h1/h2 storage) is free for the next tick's phase A
    CM3_STAMP(12, false);
  }

  if (head_lane) {
    int2 m;
    m.x = steps;
    m.y = collisions;
    reinterpret_cast<int2 *>(p.meta_out)[e] = m;
    if (episode != episode_in) p.episode[e] = (int32_t)episode;
  }
  CM3_STAMP(15, true);    // last store acknowledged
}
#undef XS

template <int N, int RT> static int policy_launch_rt(const PolicyParams &q, int prec, hipStream_t s) {
  using R = PolicyReal;
  const unsigned blocks = policy_blocks((size_t)q.p.E, N, RT);   // (N in {1, 2, 4, 8}: ceil(E N / (16 RT)), as ever)
  note_variant("k_policy_rollout", (int)sizeof(R), N, 4, q.p.n_ticks > 1, prec, 0, 0, 0, RT);
  if (prec == kPrecF16x3)
    hipLaunchKernelGGL((k_policy_rollout<N, kPrecF16x3, RT, R>), dim3(blocks), dim3(256), 0, s, q);
  else if (prec == kPrecBf16)
    hipLaunchKernelGGL((k_policy_rollout<N, kPrecBf16, RT, R>), dim3(blocks), dim3(256), 0, s, q);
  else
    hipLaunchKernelGGL((k_policy_rollout<N, kPrecF32, RT, R>), dim3(blocks), dim3(256), 0, s, q);
  CM3_HIP_CHECK(hipGetLastError());
  return CM3_OK;
}

// Row tiles per workgroup from the batch (measured on MI355X with the final kernel, f16x3, us per tick at RT = 4 / 2 / 1 --
// profiles/r04_policy_row_tiles.txt, re-swept after the accumulators moved to architectural VGPRs):  N = 4: 2048 envs 4.17 / 3.05 /
// 2.86, 4096 envs (C2) 4.32 / 3.97 / 5.12, 8192 envs 6.00 / 7.21 / 9.68, 65536 envs 43.3 / 54.0 / 73.8;  N = 8: 512 envs 5.38 /
// 3.94 / 3.23, 1024 envs 5.43 / 4.06 / 3.84, 2048 envs 5.63 / 5.37 / 6.99, 4096 envs 8.09 / 9.91 / 13.4, 8192 envs 15.2 / 19.4 /
// 26.4;  N = 2 at 8192 envs 3.85 / 3.62 / 4.72;  N = 1 at 16384 envs 3.58 / 3.36 / 4.43.  A lone workgroup per CU is latency-bound
// and the smaller one is faster (fewer matrix instructions per wave and tick); once a CU holds several, the 64-row workgroup does
// the most work per instruction issued.  So: 64-row workgroups when they already give every CU more than one, 32-row ones down to
// half a workgroup per CU, 16-row ones below -- for every N (N = 8 had a rule of its own while its 32-row build needed 261
// registers, one wave per SIMD; every build is under 256 now).  cm3_policy_force_row_tiles(1 | 2 | 4) overrides the choice (tests and
// measurements; its initial value is the environment's CM3_POLICY_RT, read ONCE -- not per launch).
constexpr size_t kPolicyCus = 256;
// (one knob for both translation units of this file: an inline variable is one object in the library)
inline std::atomic<int> g_policy_rt_override{-1};   // -1: not initialised, 0: the rule decides
static int policy_rt_override() {
  int v = g_policy_rt_override.load(std::memory_order_relaxed);
  if (v < 0) {
    const char *e = getenv("CM3_POLICY_RT");
    v = e ? atoi(e) : 0;
    if (v != 1 && v != 2 && v != 4) v = 0;
    int expected = -1;
    g_policy_rt_override.compare_exchange_strong(expected, v);
    v = g_policy_rt_override.load(std::memory_order_relaxed);
  }
  return v;
}
template <int N> static int policy_launch(const PolicyParams &q, int prec, hipStream_t s) {
  // (counted in tiles: ceil(tiles / 4) 64-row workgroups, which is ceil(E N / 64) where no row is padded.  The thresholds below were
  // measured at N in {1, 2, 4, 8}; the other agent counts inherit them untuned, with the one exception further down -- profiles/r21_policy_partial_tiles.txt)
  const size_t wg64 = (policy_tiles((size_t)q.p.E, N) + 3) / 4;
  int rt = wg64 > kPolicyCus ? 4 : (wg64 > kPolicyCus / 2 ? 2 : 1);
  // One or two ticks per launch (the launch-per-tick mode): the entry -- 58 KB of tables and weight slice per workgroup through the
  // CU's L1 path -- is as long as the tick, so the larger workgroup wins one step earlier (N = 4, one tick per launch, RT = 4 / 2 / 1:
  // 1024 envs 8.34 / 7.50 / 6.75, 2048 envs 8.46 / 7.43 / 8.47, 4096 envs 8.72 / 9.71 / 14.2, 8192 envs 11.8 / 16.6 / 24.5 us;
  // tools/probes/policy_tick_tiles.sh, profiles/r04_policy_head.txt)
  if (q.p.n_ticks <= 2) rt = wg64 >= kPolicyCus ? 4 : (wg64 >= kPolicyCus / 2 ? 2 : 1);
  // Nine and ten agents at f16x3: the 64-row build needs 80 - 88 KB of LDS and 256 registers, ONE workgroup per CU at one wave per
  // SIMD, and two 32-row workgroups per CU beat it at every size swept -- us per tick at RT = 4 / 2, slowest round of RT = 2 below
  // the fastest of RT = 4 in each: N = 9 at 4096 envs 19.6 / 18.1, at 16384 envs 77.8 / 69.9; N = 10 at 4096 envs 24.0 / 21.7, at
  // 16384 envs 94.7 / 84.0 (profiles/r21_policy_partial_tiles.txt).  Only what was swept: float32 / bf16 and the one-tick launches
  // of these agent counts keep the inherited rule.
  if (N >= 9 && prec == kPrecF16x3 && q.p.n_ticks > 2 && rt == 4) rt = 2;
  if (const int v = policy_rt_override()) rt = v;
  switch (rt) {
    case 1: return policy_launch_rt<N, 1>(q, prec, s);
    case 2: return policy_launch_rt<N, 2>(q, prec, s);
  }
  return policy_launch_rt<N, 4>(q, prec, s);
}

// The agent counts whose tiles are padded -- 3, 5, 6, 7, 9, 10; float32 envs and the CM3 actor only: 6 x 3 precisions x 3 row-tile
// counts = 54 builds of the kernel -- are a translation unit of their own, so that they compile beside the others instead of
// behind them: build.sh compiles this file once more with -DCM3_POLICY_PARTIAL_TILES, which emits this one function and nothing else.
int policy_partial_launch(int n_agents, const PolicyParams &q, int prec, hipStream_t s);
#ifdef CM3_POLICY_PARTIAL_TILES
int policy_partial_launch(int n_agents, const PolicyParams &q, int prec, hipStream_t s) {
  bool hit;
  const int rc = agent_dispatch<3, 5, 6, 7, 9, 10>(n_agents, hit, [&](auto n) { return policy_launch<n()>(q, prec, s); });
  return hit ? rc : fail(CM3_ERR_INVALID, "n_agents %d has no padded-tile build", n_agents);
}
#endif

#ifdef CM3_POLICY_ENTRY_F32
// QMIX mode: 64-row workgroups at every batch size (the only build; cm3_policy_force_row_tiles is not consulted)
template <int N> static int policy_qmix_launch(const PolicyParams &q, hipStream_t s) {
  const size_t rows = (size_t)q.p.E * N;
  const unsigned blocks = (unsigned)((rows + 63) / 64);
  note_variant("k_policy_rollout_qmix", (int)sizeof(float), N, 4, q.p.n_ticks > 1, kPrecF32, 0, 0, 0, 4);
  hipLaunchKernelGGL((k_policy_rollout<N, kPrecF32, 4, float, true>), dim3(blocks), dim3(256), 0, s, q);
  CM3_HIP_CHECK(hipGetLastError());
  return CM3_OK;
}
#endif

}  // namespace cm3

#ifndef CM3_POLICY_PARTIAL_TILES   // (every entry point below: the other two translation units of this file)
#ifdef CM3_POLICY_ENTRY_F32
extern "C" int cm3_policy_force_row_tiles(int32_t row_tiles) {
  using namespace cm3;
  CM3_REQUIRE(row_tiles == 0 || row_tiles == 1 || row_tiles == 2 || row_tiles == 4, "row_tiles must be 0 (rule), 1, 2 or 4; got %d", row_tiles);
  g_policy_rt_override.store(row_tiles, std::memory_order_relaxed);
  return CM3_OK;
}
#endif

namespace cm3 {
// the checks on the env descriptor, the tick count and the two descriptors' agreement that every entry point of this file makes first
// padded_tiles: the entry has the builds whose 16-row tiles hold 16 / n_agents whole envs and pad rows (cm3_policy_rollout_f32)
static int policy_check_env(const cm3_particle_desc *d, const cm3_actor_particle_desc *ad, int32_t n_ticks, bool padded_tiles) {
  CM3_REQUIRE(n_ticks >= 1, "n_ticks must be >= 1");
  if (padded_tiles)
    CM3_REQUIRE(d->n_agents >= 1 && d->n_agents <= CM3_MAX_AGENTS,
                "the fused policy rollout needs n_agents in 1..%d (16 / n_agents whole envs per 16-row wave tile); got %d",
                CM3_MAX_AGENTS, d->n_agents);
  else
    CM3_REQUIRE(d->n_agents == 1 || d->n_agents == 2 || d->n_agents == 4 || d->n_agents == 8,
                "the fused policy rollout needs n_agents in {1, 2, 4, 8} (whole envs per 16-row wave tile); got %d",
                d->n_agents);
  CM3_REQUIRE(ad->n_agents == d->n_agents && ad->n_envs == d->n_envs, "actor / env descriptors disagree");
  CM3_REQUIRE(!(d->flags & CM3_FLAG_GEN_ACTIONS), "the policy draws the actions: CM3_FLAG_GEN_ACTIONS is meaningless here");
  return CM3_OK;
}

// the trajectory checks and the parameter fill every entry point of this file shares: q.p, the strides, q.obs_in
static int policy_fill(const cm3_particle_desc *d, const cm3_particle_traj *t, int32_t n_ticks, PolicyParams &q) {
  CM3_REQUIRE(t->state && t->goals && t->obs_others && t->actions && t->reward_n && t->reward && t->done && t->meta &&
                  t->episode,
              "trajectory base pointers are required");
  auto at = [](void *base, size_t stride, int k) -> void * {
    return base ? (void *)((char *)base + stride * (size_t)k) : nullptr;
  };
  cm3_particle_bufs b;
  memset(&b, 0, sizeof(b));
  b.state_in = t->state;
  b.state_out = at(t->state, t->state_stride, 1);
  b.goals_in = t->goals;
  b.goals_out = at(t->goals, t->goals_stride, 1);
  b.meta_in = b.meta_out = t->meta;
  b.episode = t->episode;
  b.actions = t->actions;
  b.obs_others = at(t->obs_others, t->obs_others_stride, 1);
  b.reward_n = t->reward_n;
  b.reward = t->reward;
  b.done = t->done;
  b.term_state = t->term_state;
  b.term_obs_others = t->term_obs_others;
  b.collisions_tick = t->collisions;
  CM3_REQUIRE(d->env_offset == 0 && d->env_count == 0, "the fused policy rollout covers the whole batch");
  cm3_particle_desc dd = *d;
  dd.flags &= CM3_FLAG_AUTO_RESET;
  memset(&q, 0, sizeof(q));
  int rc = fill_params(&dd, &b, kStep, nullptr, q.p);
  if (rc != CM3_OK) return rc;
  q.p.n_ticks = n_ticks;
  q.p.st_state = t->state_stride;
  q.p.st_goals = t->goals_stride;
  q.p.st_obs = t->obs_others_stride;
  q.p.st_actions = t->actions_stride;
  q.p.st_reward_n = t->reward_n_stride;
  q.p.st_reward = t->reward_stride;
  q.p.st_done = t->done_stride;
  q.p.st_term_state = t->term_state_stride;
  q.p.st_term_obs = t->term_obs_others_stride;
  q.p.st_coll = t->collisions_stride;
  q.obs_in = t->obs_others;
  return CM3_OK;
}

// cm3_policy_rollout_f32 / _f64: the same validation and launch, PolicyReal of this translation unit
static int policy_rollout_call(const cm3_particle_desc *d, const cm3_particle_traj *t, const cm3_actor_particle_desc *ad,
                               const cm3_actor_particle_weights *wt, float *probs, size_t probs_stride, int32_t n_ticks,
                               void *stream) {
  CM3_REQUIRE(d && t && ad && wt, "null argument");
  constexpr bool kPadded = sizeof(PolicyReal) == 4;   // float32 envs: every n_agents; float64: the dense tiles only
  int rc = policy_check_env(d, ad, n_ticks, kPadded);
  if (rc != CM3_OK) return rc;
  rc = actor_check_desc(ad);
  if (rc != CM3_OK) return rc;
  CM3_REQUIRE(ad->seed == d->seed && ad->env_id_base == d->env_id_base,
              "actor and env must share seed and env_id_base (one Philox key; the streams differ by purpose bits)");
  CM3_REQUIRE(ad->epsilon >= 0.0f && ad->epsilon <= 1.0f, "epsilon must be in [0,1]");
  CM3_REQUIRE(wt->packed, "weights->packed is NULL: run cm3_actor_particle_pack once per weight update");
  PolicyParams q;
  rc = policy_fill(d, t, n_ticks, q);
  if (rc != CM3_OK) return rc;
  q.packed = (const float *)wt->packed;
  q.probs = probs;
  q.st_probs = probs_stride;
  q.eps = ad->epsilon;
  q.stage = ad->stage;
  hipStream_t s = (hipStream_t)stream;
  CM3_REQUIRE(ad->precision >= 0 && ad->precision <= 2, "precision must be 0, 1 or 2");
  const int bf16 = ad->precision;
  bool hit;
  rc = agent_dispatch<1, 2, 4, 8>(d->n_agents, hit, [&](auto n) { return policy_launch<n()>(q, bf16, s); });
  if (hit) return rc;
  if constexpr (kPadded) return policy_partial_launch(d->n_agents, q, bf16, s);   // 3, 5, 6, 7, 9, 10: their own translation unit
  return fail(CM3_ERR_INVALID, "n_agents %d unsupported", d->n_agents);
}
}  // namespace cm3

#ifdef CM3_POLICY_ENTRY_F32
extern "C" int cm3_policy_rollout_f32(const cm3_particle_desc *d, const cm3_particle_traj *t,
                                      const cm3_actor_particle_desc *ad, const cm3_actor_particle_weights *wt,
                                      float *probs, size_t probs_stride, int32_t n_ticks, void *stream) {
  return cm3::policy_rollout_call(d, t, ad, wt, probs, probs_stride, n_ticks, stream);
}
#endif
#ifdef CM3_POLICY_ENTRY_F32
// The QMIX agent's one-launch rollout: desc / traj / n_ticks checked as cm3_policy_rollout_f32 checks them, the agent as
// cm3_qmix_particle_f32 checks it; every failure returns before anything touches the device.
extern "C" int cm3_policy_rollout_qmix_f32(const cm3_particle_desc *d, const cm3_particle_traj *t, const cm3_actor_particle_desc *ad,
                                           const void *packed, float *q_values, size_t q_stride, const float *epsilon_dev,
                                           int32_t n_ticks, void *stream) {
  using namespace cm3;
  CM3_REQUIRE(d && t && ad, "null argument");
  int rc = policy_check_env(d, ad, n_ticks, false);
  if (rc != CM3_OK) return rc;
  rc = qmix_check_desc(ad);
  if (rc != CM3_OK) return rc;
  CM3_REQUIRE(ad->seed == d->seed && ad->env_id_base == d->env_id_base,
              "agent and env must share seed and env_id_base (one Philox key; the streams differ by purpose bits)");
  CM3_REQUIRE(ad->epsilon >= 0.0f && ad->epsilon <= 1.0f, "epsilon must be in [0,1]");
  CM3_REQUIRE(packed, "packed weights are NULL: run cm3_qmix_particle_pack once per weight update");
  PolicyParams q;
  rc = policy_fill(d, t, n_ticks, q);
  if (rc != CM3_OK) return rc;
  q.packed = (const float *)packed;
  q.probs = q_values;
  q.st_probs = q_stride;
  q.eps = ad->epsilon;
  q.eps_dev = epsilon_dev;
  hipStream_t s = (hipStream_t)stream;
  return agent_launch<1, 2, 4, 8>(d->n_agents, [&](auto n) { return policy_qmix_launch<n()>(q, s); });
}
#endif
#ifdef CM3_PARTICLE_F64
extern "C" int cm3_policy_rollout_f64(const cm3_particle_desc *d, const cm3_particle_traj *t,
                                      const cm3_actor_particle_desc *ad, const cm3_actor_particle_weights *wt,
                                      float *probs, size_t probs_stride, int32_t n_ticks, void *stream) {
  return cm3::policy_rollout_call(d, t, ad, wt, probs, probs_stride, n_ticks, stream);
}
#endif
#endif   // !CM3_POLICY_PARTIAL_TILES
