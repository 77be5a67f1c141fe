// Pieces shared by the particle actor (actor.hip, policy.hip) and the Checkers actor (actor_checkers.hip).
#pragma once
#include "agent_dispatch.h"
#include "common.h"
#include "philox.h"

namespace cm3 {

constexpr int kA = 5;  // l_action
constexpr uint32_t kPurposePolicy = 0x40000000u;

// An entry point's launch by agent count: f(std::integral_constant<int, N>) for the N of the list that equals n_agents
// (agent_dispatch.h), the entry points' one refusal otherwise -- fail() runs only on a miss.
template <int... Ns, typename F> static int agent_launch(int n_agents, F &&f) {
  bool hit;
  const int rc = agent_dispatch<Ns...>(n_agents, hit, f);
  return hit ? rc : fail(CM3_ERR_INVALID, "n_agents %d unsupported", n_agents);
}
template <typename F> static int agent_launch_1_to_10(int n_agents, F &&f) {
  return agent_launch<1, 2, 3, 4, 5, 6, 7, 8, 9, 10>(n_agents, f);
}

// The matrix kernels are built for TWO waves per SIMD.  With that as the declared minimum occupancy the register budget is 256 and
// the compiler's default selection keeps the matrix accumulators in architectural VGPRs (no v_accvgpr_read per value in the
// epilogues) -- round 4 forced the same code with the experimental -amdgpu-mfma-vgpr-form=1; round 5 showed that the attribute
// gives it by the standard path (profiles/r05_policy_fault.txt, variant agpr2w) and dropped the flag.  Consequence that
// stays: NO inline assembly may read a matrix instruction's result (the hazard recogniser does not see into asm statements).
#define CM3_MATRIX_KERNEL __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// relu as ONE instruction: fmaxf(x, 0) first canonicalises x (a second v_max_f32 x, x) because the build honours signalling NaNs
// (v_med3_f32 against 0 and +inf is folded back into the same pair).  On the bit patterns it is a signed-integer maximum: a float
// with the sign bit set is a negative integer (-0.0 included, a NaN with the sign bit too; a positive NaN stays what it is), every
// other float is its own non-negative integer.  Plain C rather than inline assembly: the compiler's hazard recogniser does not look
// into an asm statement, and with the accumulators in architectural VGPRs (build.sh) the operand is the matrix instruction's own
// destination -- an opaque "v_max_f32" read it before the passes were through (caught by tests/test_gpu_actor.py on the first
// build with that flag).
__device__ __forceinline__ float relu_f32(float x) {
  const int xi = __builtin_bit_cast(int, x);
  return __builtin_bit_cast(float, xi > 0 ? xi : 0);
}

// action ~ multinomial(probs) (alg_credit.py:120): inverse CDF in action order, one uniform per (seed, global env id, episode,
// step, agent) from the two-stage stream of philox.h -- stage 1 (actor_block_word: the agent's word of the env's Philox block with
// the policy purpose bit) depends on nothing loaded or computed, so a kernel draws it once, ahead of time (the fused policy rollout:
// once per LAUNCH, for all its ticks); stage 2 (actor_uniform_from) mixes the episode / step counters in, ~10 instructions.
__device__ __forceinline__ uint32_t actor_block_word(uint64_t seed, uint64_t genv, int agent) {
  u32x4 ctr;
  ctr.x = (uint32_t)genv;
  ctr.y = (uint32_t)(genv >> 32);
  ctr.z = 0u;
  ctr.w = kPurposePolicy | ((uint32_t)(agent >> 2) << 24);
  const u32x4 wd = philox4x32_10(ctr, (uint32_t)seed, (uint32_t)(seed >> 32));
  const int q = agent & 3;
  return q == 0 ? wd.x : (q == 1 ? wd.y : (q == 2 ? wd.z : wd.w));
}
__device__ __forceinline__ float actor_uniform_from(uint32_t block_word, uint32_t episode, int steps) {
  return (float)u01(action_word(block_word, episode, (uint32_t)steps));
}
__device__ __forceinline__ float actor_uniform(uint64_t seed, uint64_t genv, uint32_t episode, int steps, int agent) {
  return actor_uniform_from(actor_block_word(seed, genv, agent), episode, steps);
}

__device__ __forceinline__ int actor_pick(const float (&pr)[kA], float u) {
  // first action whose cumulative probability exceeds u, the last one otherwise.  The running sum never decreases (pr >= 0), so
  // the comparisons that fail form a prefix and the index is their count: no branches (the if-chain compiled to four exec-mask
  // regions on the path of every tick)
  int act = 0;
  float cdf = 0.0f;
#pragma unroll
  for (int a = 0; a < kA - 1; ++a) {
    cdf += pr[a];
    act += (u < cdf) ? 0 : 1;
  }
  return act;
}

__device__ __forceinline__ int actor_sample(const float (&pr)[kA], uint64_t seed, uint64_t genv, uint32_t episode,
                                            int steps, int agent) {
  return actor_pick(pr, actor_uniform(seed, genv, episode, steps, agent));
}

// ---- the QMIX agents' epsilon-greedy choice (k_qmix_particle in actor.hip, k_ck_actor<.., true> / k_ck_actor_x3<true> in
// actor_checkers.hip): ONE exploration stream for both.  Two independent words per (seed, global env id, episode, step, agent) --
// "explore?" and the uniform action -- from a Philox block of their own purpose: words 2 (agent & 1) and 2 (agent & 1) + 1 of the
// block (env id lo, env id hi, 0, kPurposeExplore | (agent >> 1) << 24), each mixed with the episode / step counters (action_word).
// Callers issue it before their head's dependent matrix work: the Philox rounds are VALU work that fills the matrix waits.
constexpr uint32_t kPurposeExplore = 0x20000000u;   // distinct from kAction (0), kReset (bit 31), kPolicy (bit 30)

// Two stages, like the actor's uniform: stage 1 (explore_block_words: the agent's two words of the env's block) depends on nothing
// loaded or computed, so the whole-episode Checkers kernel draws it once per LAUNCH; stage 2 (explore_words_from) mixes the
// episode / step counters in.
__device__ __forceinline__ uint2 explore_block_words(uint64_t seed, uint64_t genv, int agent) {
  u32x4 ctr;
  ctr.x = (uint32_t)genv;
  ctr.y = (uint32_t)(genv >> 32);
  ctr.z = 0u;
  ctr.w = kPurposeExplore | ((uint32_t)(agent >> 1) << 24);
  const u32x4 wd = philox4x32_10(ctr, (uint32_t)seed, (uint32_t)(seed >> 32));
  const bool odd = (agent & 1) != 0;
  return make_uint2(odd ? wd.z : wd.x, odd ? wd.w : wd.y);
}
__device__ __forceinline__ void explore_words_from(uint2 block_words, uint32_t episode, uint32_t steps, uint32_t &w_explore,
                                                   uint32_t &w_action) {
  w_explore = action_word(block_words.x, episode, steps);
  w_action = action_word(block_words.y, episode, steps);
}
__device__ __forceinline__ void explore_words(uint64_t seed, uint64_t genv, uint32_t episode, uint32_t steps, int agent,
                                              uint32_t &w_explore, uint32_t &w_action) {
  explore_words_from(explore_block_words(seed, genv, agent), episode, steps, w_explore, w_action);
}

// ---- the draw of the actor over TRANSITION rows (k_actor_particle<.., ROWS = true> in actor.hip): a sampled batch has no env, episode or step
// behind it, so its uniforms come from a Philox block of their own purpose, keyed by the row alone: counter (row id lo, row id hi,
// draw, kPurposeRows), key = seed, word .x -- row id = the caller's 64-bit row_id_base + the row's index, draw = a 32-bit counter the
// caller advances once per launch.  ONE stage (no action_word mix): nothing of the counter is loaded, all of it is known at entry.
// kPurposeRows is bit 28 of counter word 3 and nothing else.  No other stream can produce that word: the reset stream always sets
// bit 31, the policy stream bit 30, the exploration stream bit 29, and what they and the action stream (purpose 0) OR in below is
// `call << 24` with call = agent >> 2 (action, policy: at most 2 with CM3_MAX_AGENTS = 10, bits 24..25) or agent >> 1 (explore: at
// most 4, bits 24..26): bit 28 would take 64 (32) agents.
constexpr uint32_t kPurposeRows = 0x10000000u;
__device__ __forceinline__ float rows_uniform(uint64_t seed, uint64_t row_id, uint32_t draw) {
  u32x4 ctr;
  ctr.x = (uint32_t)row_id;
  ctr.y = (uint32_t)(row_id >> 32);
  ctr.z = draw;
  ctr.w = kPurposeRows;
  return (float)u01(philox4x32_10(ctr, (uint32_t)seed, (uint32_t)(seed >> 32)).x);
}

// ---- a rows launch that keeps its OWN draw counter (the *_rows_counted entries): two uint32 words in device memory, 8-byte aligned,
// {draw, arrivals}, set up once by the caller with arrivals = 0.  A host-side `draw` is baked into a captured launch, so every replay
// of a hipGraph would draw the same uniforms; a counted launch reads word 0 for itself -- every row of the launch draws at that
// value -- and leaves word 0 + 1 (mod 2^32) behind, in the same launch: no node more per evaluation.  The mechanism is
// k_returns_moments' (advantage.hip): once every wave of a workgroup has its value (the barrier), the workgroup takes a ticket from
// `arrivals`; the workgroup whose ticket is gridDim.x - 1 knows every other one has read, writes the advanced value and resets
// `arrivals`.  Nothing waits for another workgroup, so a grid of more workgroups than the chip holds at once is no different.
// Ordering: the two words are ONE 64-bit atomic object (why they are 8-byte aligned; word 0 is its low half), and every access --
// the read, the ticket, the write -- is a relaxed agent-scope atomic on it (never served by an XCD's own L2 copy).  A wave's read
// happens before its workgroup's ticket (the barrier); the ticket modifies the object, so by the coherence of a single atomic object
// the read took its value from before that ticket in the object's modification order; the write comes after the last ticket, hence
// after every ticket, in that order: no read can see the advanced value, on whichever XCD it ran.  No release fence is involved: an
// agent-scope release makes the workgroup write its XCD's L2 back first (measured with the ticket as a 32-bit acq_rel add on
// word 1: +5.1 .. +6.2 us per launch at 16 384 rows; this form +3.2 .. +3.8, profiles/r23_rows_counter.txt).  Launches that share
// a counter must be ordered on the device (one stream, or graph dependencies): two of them in flight at once would count each
// other's arrivals.
__device__ __forceinline__ uint32_t rows_draw_read(const uint32_t *state) {
  return (uint32_t)__hip_atomic_load(reinterpret_cast<const unsigned long long *>(state), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// called by EVERY thread of the workgroup (it holds a barrier), after the thread's last rows_draw_read
__device__ __forceinline__ void rows_draw_arrive(uint32_t *state, int tid) {
  __syncthreads();
  if (tid == 0) {
    unsigned long long *both = reinterpret_cast<unsigned long long *>(state);
    const unsigned long long old = __hip_atomic_fetch_add(both, 1ull << 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // (low half: the draw every row of this launch used; high half: how many workgroups took a ticket before this one)
    if ((uint32_t)(old >> 32) == gridDim.x - 1)
      __hip_atomic_store(both, (unsigned long long)((uint32_t)old + 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // {draw + 1, 0}
  }
}

// One row of an int64 [rows][5] one-hot array (the reference's np.zeros(dtype=int) forms: actions_target_1hot, action_one):
// 40 bytes per row from a 16-byte aligned base -- an even row is 16 | 16 | 8 bytes, an odd one 8 | 16 | 16
__device__ __forceinline__ void onehot_row_store(int64_t *onehot, size_t hr, int act) {
  typedef long long i64x2 __attribute__((ext_vector_type(2)));
  int64_t *row = onehot + hr * kA;
  const int k0 = (int)(hr & 1), k1 = k0 ? 0 : 4;
  *reinterpret_cast<i64x2 *>(row + k0) = i64x2{act == k0, act == k0 + 1};
  *reinterpret_cast<i64x2 *>(row + k0 + 2) = i64x2{act == k0 + 2, act == k0 + 3};
  row[k1] = act == k1;
}

// argmax Q with the first index on ties (tf.argmax) and the value there: the greedy half of epsilon_greedy below, on its own
__device__ __forceinline__ void greedy_argmax(const float (&q)[kA], int &greedy, float &best) {
  greedy = 0;
  best = q[0];
#pragma unroll
  for (int a = 1; a < kA; ++a) {
    const bool gt = q[a] > best;
    greedy = gt ? a : greedy;
    best = gt ? q[a] : best;
  }
}

// argmax Q with the first index on ties (tf.argmax), replaced with probability eps by a uniform action (alg_qmix.py:177-182,
// alg_qmix_checkers.py:176-181).  eps is compared in double: eps = 1 always explores.
__device__ __forceinline__ int epsilon_greedy(const float (&q)[kA], float eps, uint32_t w_explore, uint32_t w_action) {
  int greedy = 0;
  float best = q[0];
#pragma unroll
  for (int a = 1; a < kA; ++a) {
    const bool gt = q[a] > best;
    greedy = gt ? a : greedy;
    best = gt ? q[a] : best;
  }
  const bool explore = u01(w_explore) < (double)eps;
  return explore ? rand5(w_action) : greedy;
}

}  // namespace cm3
