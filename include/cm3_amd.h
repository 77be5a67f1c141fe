/*
 * cm3_amd.h -- C ABI of libcm3_hip.so: the MI355X (gfx950) vectorised rollout engine for the
 * CM3 hot path (cooperative-navigation particle env, Checkers env, trajectory collection).
 *
 * The reference (011235813/cm3) is pure Python and has no FFI of its own; the interface the
 * hot path sits behind is the Python env protocol (reset()/step()) used by
 * alg/train_onpolicy.py:119,126,282,294,321,323.  Each entry point below names the reference
 * function(s) it replaces for E environments at once.  INTEGRATION.md shows the ctypes stub a
 * reference maintainer would add.
 *
 * Conventions
 *   - Plain pointers and sizes only; no torch / HIP types in signatures (`stream` is a
 *     hipStream_t passed as void*, NULL = the default stream).
 *   - Every pointer is a DEVICE pointer owned by the caller unless stated otherwise.  The
 *     library allocates nothing persistent, keeps no pointer after return, and only ENQUEUES
 *     work on `stream` (asynchronous).
 *   - Return value: 0 (CM3_OK) or a negative CM3_ERR_* code; cm3_last_error() returns a
 *     thread-local message for the last failure on the calling thread.
 *   - E = environments in this launch (this rank's shard), N = agents per environment.
 *
 * Device layouts (particle; `real` = float for *_f32, double for *_f64)
 *   state       real [N][E][4]   (vx, vy, px, py) of agent i in env e at [i][e]: one 16/32-byte
 *                                vector per lane, unit-stride over e (coalesced).  The
 *                                reference's global_state[N,4] (environment.py:113-116) and
 *                                obs_self (multi-goal_spread.py:154) for env e are the rows
 *                                state[:, e, :].
 *   goals       real [N][E][2]   landmark positions (train_onpolicy.py:283-285)
 *   meta        int32 [E][2]     {steps, collisions}   (environment.py:93; multi-goal_spread.py:93,137).  As in the
 *                                reference, an env that is stepped after its episode ended keeps counting both
 *                                (MultiAgentEnv.step never looks at a previous `done`); the COLLECTOR stops using it
 *                                (train_onpolicy.py:302) -- see cm3_particle_traj.collisions for the per-episode value.
 *   episode     int32 [E]        episodes started so far by env e (RNG key; touched on reset only)
 *   actions     int32 [E][N]     discrete actions 0..4 (environment.py:197-200)
 *   obs_others  real [E][N][L]   L = 4*max(N-1,1)  (multi-goal_spread.py:145-154)
 *   reward_n    real [E][N]      (multi-goal_spread.py:121-138)
 *   reward      real [E]         np.sum(reward_n) (environment.py:107)
 *   done        uint8 [E]        (environment.py:118-121)
 */
#ifndef CM3_AMD_H
#define CM3_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CM3_ABI_VERSION 9   /* 9: ADDED cm3_qmix_particle_packed_bytes / _pack / _f32 / _f64 (the QMIX agent network; additive).
                                  Also part of 9, additive: cm3_qmix_checkers_pack / _f32 (the Checkers QMIX agent network);
                                  cm3_policy_rollout_qmix_f32 (the one-launch particle rollout driven by the particle QMIX agent);
                                  cm3_policy_rollout_checkers_qmix (the one-launch Checkers rollout driven by that agent; cm3_qmix_checkers_pack
                                  now also writes the others-branch table behind the packed weights, inside the same allocation);
                                  cm3_checkers_transitions_gather (the Checkers transition export in one launch);
                                  cm3_checkers_transitions_pack / cm3_checkers_ring_expand (the compact Checkers replay ring);
                                  cm3_particle_traj.live_record (appended; NULL = as before) and cm3_particle_live_record_applies.
                                  NOTE: sizeof(cm3_particle_traj) GREW by 8 bytes (192 -> 200) without a version step: a caller compiled
                                  against the shorter struct must be recompiled, or the library reads 8 bytes past its struct as
                                  live_record.  The in-tree binding mirrors the new size (tests/test_abi.py compares every offset).
                                  cm3_qmix_particle_rows_f32 (the QMIX agent network over transition rows, argmax head) and
                                  cm3_qmix_td_target_f64 (the QMIX TD target): the data side of alg_qmix.train_step; additive.
                                  cm3_qmix_checkers_rows_f32 (the Checkers QMIX agent network over transition rows, argmax head): the
                                  data side of alg_qmix_checkers.train_step; additive.
                                  cm3_critic_particle_packed_bytes / _pack / _rows_f32 (the CM3 particle critics Q_global_1output and
                                  Q_credit over transition rows decoded from a batch's base columns, with the TD target): the critic
                                  evaluations of alg_credit.train_step that carry no gradient; additive.
                                  cm3_critic_checkers_packed_bytes / _pack / _rows_f32 (the CM3 Checkers critics Q_global_checkers and
                                  Q_credit_checkers over transition rows decoded from a batch's base columns, with the TD target): the
                                  critic evaluations of alg_credit_checkers.train_step that carry no gradient; additive.
                                  cm3_qmix_mixer_particle_packed_bytes / _pack / _rows_f32 (the particle QMIX mixer over transition rows
                                  with the TD target: mixer_target of alg_qmix.train_step, the last evaluation without a gradient);
                                  additive.
                                  cm3_qmix_mixer_checkers_packed_bytes / _pack / _rows_f32 (the Checkers QMIX mixer over transition rows
                                  with the TD target: mixer_target of alg_qmix_checkers.train_step); additive.
                                  cm3_qmix_learner_particle_workspace_bytes / _grad_f32 (loss and the eleven dense gradients of mixer_op of
                                  alg_qmix.train_step) and cm3_adam_step_f32 (tf.train.AdamOptimizer's step over a table of tensors, its
                                  two powers kept on the device): the first train step that needs no session; additive.
                                  cm3_qmix_learner_checkers_workspace_bytes / _grad_f32 (loss and the twenty dense gradients of mixer_op
                                  of alg_qmix_checkers.train_step, applied by cm3_adam_step_f32): additive.
                                  cm3_value_particle_packed_bytes / _pack / _rows_f32 and cm3_coma_particle_packed_bytes / _pack /
                                  _rows_f32 (the IAC / COMA baseline critics V_particle_local, V_particle_global and Q_global over
                                  transition rows, with the TD targets: the evaluations of alg_baseline.train_step that carry no
                                  gradient); additive.
                                  cm3_value_checkers_packed_bytes / _pack / _rows_f32 and cm3_coma_checkers_packed_bytes / _pack /
                                  _rows_f32 (the Checkers IAC / COMA baseline critics V_checkers_local, V_checkers_global and
                                  Q_coma_checkers over transition rows, with the TD targets: the evaluations of
                                  alg_baseline_checkers.train_step that carry no gradient); additive.
                                  cm3_actor_particle_rows_f32 (the CM3 particle actor over transition rows: probabilities and sampled
                                  actions, the two actor evaluations of alg_credit.train_step); additive.
                                  cm3_actor_checkers_rows_f32 (the CM3 Checkers actor over transition rows: the two actor evaluations of
                                  alg_credit_checkers.train_step); additive.
                                  cm3_actor_particle_rows_counted_f32 / cm3_actor_checkers_rows_counted_f32 (the two actor rows launches
                                  with a draw counter in device memory that the launch reads and advances itself, so a captured launch
                                  draws afresh on every replay); additive.
                                  cm3_rows_force_index_width / cm3_rows_last_index_width (the 64-bit index builds of the row, export
                                  and tiling kernels at any size: tests); additive.
                               8: ADDED cm3_actor_particle_f64, cm3_policy_rollout_f64 (policy-driven collection on float64 envs; additive).
                               7 (round 6): REMOVED cm3_particle_rollout_chains_f32 / _f64 (sub-batch chains on several streams: a tested,
                               measured regression since round 2 -- profiles/r02_chains_diag.txt; tools/chains_diag.py reproduces it
                               with desc->env_offset / env_count).  ADDED cm3_td_target_f64, cm3_policy_rollout_checkers; cm3_actor_checkers_packed_bytes grew by the others-branch table; the
                               precision-2 Checkers actor adds branch_others W_others_h2 to h2's accumulators BEFORE branch_self
                               W_self_h2 (probabilities move in the last bits).
                               6: cm3_policy_force_row_tiles, cm3_rows_scatter / cm3_rows_gather / cm3_rows_tile / cm3_transitions_gather_f32 (round 5).
                               5: the in-kernel ACTION STREAM of the particle kernels and the actors' sampling uniforms became two stages
                               (Philox4x32-10 block per (seed, global env id, call) + fmix32((word ^ step) + episode * 0x9E3779B1);
                               csrc/philox.h, oracle/philox.py; since ABI 6 the Checkers kernels too) -- a given (seed, env, episode, step, agent) draws a DIFFERENT action
                               than under ABI 4, whose counter layout masked `step & 0x00FFFFFF` into one Philox call (Checkers kept
                               that one-stage draw until ABI 6).  Also 5: cm3_last_kernel_variant; cm3_returns_moments_* takes a zero-initialised-once scratch (see there);
                               cm3_returns_normalize_*, cm3_copy_shift, cm3_source_id, actor precision 2 (all added under 4) */
#define CM3_MAX_AGENTS 10   /* the reference's make_world takes up to ten agents (its colour table, multi-goal_spread.py:7-16);
                              8 until ABI 5.  Checkers, the lane-per-pair mapping and the fused policy rollout stay at <= 8 */

#define CM3_OK 0
#define CM3_ERR_INVALID (-1)     /* bad argument / unsupported configuration */
#define CM3_ERR_HIP (-2)         /* a HIP runtime call failed */
#define CM3_ERR_STATE (-3)       /* call sequence error (graph capture etc.) */

/* cm3_*_desc.flags */
#define CM3_FLAG_AUTO_RESET 1u   /* an env whose episode ends is re-initialised inside the same launch:
                                    its reward/done outputs are the terminal ones, its state/obs outputs are
                                    those of the fresh episode (train_onpolicy.py:282 folded into :321) and
                                    the true terminal next-state goes to term_* when those are non-NULL */
#define CM3_FLAG_GEN_ACTIONS 2u  /* actions are drawn in-kernel, uniform on {0..4} (train_onpolicy.py:305-307),
                                    Philox4x32-10 keyed (seed, global env id, episode, step), and WRITTEN to
                                    `actions` */

#define CM3_FLAG_FUSED_TICKS 0x400u  /* cm3_particle_rollout_* only: run all n_ticks ticks in ONE launch with the
                                       state in registers (identical results).  Needs CM3_FLAG_GEN_ACTIONS or one
                                       pre-filled action slot per tick: nothing can act between the ticks */
#define CM3_FLAG_KERNEL_LANE_PER_ENV 0x100u  /* particle step: force the one-lane-per-env mapping   */
#define CM3_FLAG_KERNEL_LANE_PER_PAIR 0x200u /* particle step: force the one-lane-per-agent-pair mapping
                                                (default: chosen from n_envs; both give identical results) */
#define CM3_FLAG_KERNEL_LANE_PER_AGENT 0x800u /* particle step: force the one-lane-per-agent mapping (n_agents >= 2) */
/* The two shared-env mappings index with 32-bit byte offsets: every per-tick array (the largest is obs_others,
   n_envs * N * (N-1) * 4 reals) must stay below 4 GiB.  The default choice respects that; a FORCED mapping beyond it returns
   CM3_ERR_INVALID.  (N = 8, float32: 4.79 M envs.) */

int cm3_abi_version(void);
/* First 16 hex digits of the SHA-256 over the library's sources (the .hip and .h files of csrc/ in byte order of their names,
 * then this header), baked in by csrc/build.sh.  The Python binding compares it with the sources next to it and refuses a stale build. */
const char *cm3_source_id(void);
const char *cm3_last_error(void);
/* Debug / test query (ABI 5): the kernel instantiation that the most recent cm3_particle_* / cm3_checkers_* call ON THE CALLING
 * THREAD launched last, e.g. "k_particle_step_pairs<f32,N=4,waves=4,fused=0,sp=nt,live=1,early=0,g=0,tu=ilp>" -- the launchers
 * choose among size-gated builds of one template (mapping, waves per workgroup, observation store policy plain / nt / wt, the
 * live-state variant, the max-ILP translation unit); tests/test_gpu_dispatch_sizes.py asserts which build it checked.
 * Thread-local storage, valid until the next call on the thread.  No reference counterpart. */
const char *cm3_last_kernel_variant(void);
/* Number of visible HIP devices (0 when none); fills name (<= len bytes) of device `dev` if name != NULL. */
int cm3_device_count(void);
int cm3_device_name(int dev, char *name, int len);

/* ------------------------------------------------------------------------------------------
 * Particle env: MultiAgentEnv + multi-goal_spread scenario
 * ---------------------------------------------------------------------------------------- */
typedef struct cm3_particle_desc {
  int32_t n_envs;      /* E */
  int32_t n_agents;    /* N, 1..CM3_MAX_AGENTS */
  int32_t max_steps;   /* config.json:61 */
  uint32_t flags;      /* CM3_FLAG_* */
  int32_t env_offset;  /* launch only envs [env_offset, env_offset + env_count) of the E-extent arrays (a sub-batch; the */
  int32_t env_count;   /* arrays and RNG keys are untouched by the split).  env_count == 0 (with offset 0) = all E envs */
  int64_t env_id_base; /* global id of local env 0: RNG is keyed by GLOBAL env id, so results do not
                          depend on how envs are sharded over GPUs */
  uint64_t seed;
  double prob_random;  /* multi-goal_spread.py:75 */
  double initial_std;  /* multi-goal_spread.py:80-81 */
  double agents_x[CM3_MAX_AGENTS], agents_y[CM3_MAX_AGENTS];       /* config_particle_*.json */
  double landmarks_x[CM3_MAX_AGENTS], landmarks_y[CM3_MAX_AGENTS];
} cm3_particle_desc;

typedef struct cm3_particle_bufs {
  const void *state_in; /* real [N][E][4] pre-step state */
  void *state_out;      /* real [N][E][4] post-step state; may alias state_in */
  const void *goals_in; /* real [N][E][2] */
  void *goals_out;      /* real [N][E][2]; may alias goals_in (then only re-initialised envs are written) */
  const int32_t *meta_in; /* int32 [E][2] */
  int32_t *meta_out;      /* may alias meta_in */
  int32_t *episode;     /* int32 [E], in/out */
  int32_t *actions;     /* int32 [E][N]; input, or output under CM3_FLAG_GEN_ACTIONS */
  void *obs_others;     /* real [E][N][L] out */
  void *reward_n;       /* real [E][N] out */
  void *reward;         /* real [E] out */
  uint8_t *done;        /* uint8 [E] out */
  void *term_state;      /* optional real [N][E][4]: written only for envs re-initialised by AUTO_RESET */
  void *term_obs_others; /* optional real [E][N][L]: same */
  int32_t *collisions_tick; /* optional int32 [E] out, written for EVERY env: scenario.collisions (multi-goal_spread.py:137)
                               after this tick and before any same-launch re-initialisation.  At the tick that ends an
                               episode it is that episode's count, whose `!= 0` is the reference's is_bad flag of the dual
                               replay buffer (train_onpolicy.py:356): AUTO_RESET zeroes the live counter in the same launch,
                               and without it the live counter keeps counting if the env is stepped further */
} cm3_particle_bufs;

/* One tick for E envs in ONE kernel launch: replaces MultiAgentEnv.step (environment.py:81-123) =
 * _set_action (:177-225) + World.step (core.py:117-131) + Scenario.observation/reward/done
 * (multi-goal_spread.py:121-154). */
int cm3_particle_step_f32(const cm3_particle_desc *desc, const cm3_particle_bufs *bufs, void *stream);
int cm3_particle_step_f64(const cm3_particle_desc *desc, const cm3_particle_bufs *bufs, void *stream);

/* (Re)initialise envs: replaces MultiAgentEnv.reset (environment.py:125-149) +
 * Scenario.reset_world (multi-goal_spread.py:65-93).  Uses state_out, goals_out, meta_out, episode,
 * obs_others of `bufs`; `mask` (uint8 [E], optional) selects the envs to reset (NULL = all).
 * The build's own counter-based RNG reproduces the reference's DISTRIBUTIONS (one Bernoulli(prob_random)
 * per episode shared by agents and landmarks; U(-1,1)^2, or preset + N(0, initial_std) on agents only). */
int cm3_particle_reset_f32(const cm3_particle_desc *desc, const cm3_particle_bufs *bufs, const uint8_t *mask,
                           void *stream);
int cm3_particle_reset_f64(const cm3_particle_desc *desc, const cm3_particle_bufs *bufs, const uint8_t *mask,
                           void *stream);

/* Observation only (no dynamics): obs_others from state_in.  Replaces Scenario.observation
 * (multi-goal_spread.py:145-154) after a state injection. */
int cm3_particle_observe_f32(const cm3_particle_desc *desc, const cm3_particle_bufs *bufs, void *stream);
int cm3_particle_observe_f64(const cm3_particle_desc *desc, const cm3_particle_bufs *bufs, void *stream);

/* Trajectory collection (train_onpolicy.py:302-350): n_ticks launches of the step kernel over a
 * time-major trajectory.  Slot t of each array is base + t*stride (strides in BYTES).  state/obs_others/
 * goals have n_ticks+1 slots (slot t = before tick t, slot t+1 = after); the per-tick outputs have
 * n_ticks slots.  meta/episode are live (in place).  goals_stride == 0 keeps one live goals array.
 * term_* are optional (n_ticks slots).  All strides 0 = every tick overwrites the same live buffers.
 * With CM3_FLAG_GEN_ACTIONS every launch draws its own actions and writes them to its action slot. */
typedef struct cm3_particle_traj {
  void *state;        size_t state_stride;
  void *goals;        size_t goals_stride;
  void *obs_others;   size_t obs_others_stride;
  int32_t *actions;   size_t actions_stride;
  void *reward_n;     size_t reward_n_stride;
  void *reward;       size_t reward_stride;
  uint8_t *done;      size_t done_stride;
  int32_t *meta;      /* int32 [E][2], live */
  int32_t *episode;   /* int32 [E], live */
  void *term_state;      size_t term_state_stride;
  void *term_obs_others; size_t term_obs_others_stride;
  int32_t *collisions;  size_t collisions_stride; /* optional, n_ticks slots of int32 [E]: cm3_particle_bufs.collisions_tick */
  /* optional (ABI 4), both or neither; per-tick launches only (ignored with CM3_FLAG_FUSED_TICKS, where the state never leaves
     the registers): LIVE state real [N][E][4] / goals real [N][E][2].  When given, every tick reads and overwrites the live
     buffers IN PLACE (they hold the current state on entry and the final state on return) and writes its post-step state ALSO to
     slot k + 1 of `state` (slot 0 is neither read nor written: the caller keeps the initial state there if it wants it).  The
     GOALS slots are sparse from ABI 5 on (see goals_live below): slot k + 1 of `goals` is written only for the envs that restart
     at tick k -- landmarks do not move otherwise.  Values are identical either way; what changes is where a tick LOADS from -- lines its predecessor read and
     overwrote stay resident, lines of a fresh slot that was only ever written do not: measured 0.19 us of 2.83 us per tick at
     4096 envs x 4 agents (tools/trajectory_gap.py). */
  void *state_live;
  void *goals_live;
  /* goals_live WITHOUT state_live (ABI 5): SPARSE goal slots.  Landmarks move only when an episode starts (multi-goal_spread.py:
     88-91), yet a slot trajectory wrote all of them every tick: 8 N of the ~450 bytes a tick moves per env at streaming sizes, where
     the launch runs at the chip's copy rate (profiles/r04_trajectory_stream.txt).  Here the goals live in goals_live (read and, on a
     restart, updated in place) and slot k + 1 of `goals` is written ONLY for the envs re-initialised at tick k: the goals in effect
     at slot t are those of the last written slot <= t (slot 0 is the caller's).  Per-tick launches only. */
  void *live_record;
  /* optional, with state_live / goals_live: PACKED LIVE RECORDS, n_envs x 128 bytes, 128-byte aligned, scratch owned by the caller
     (contents are undefined between calls).  The live state of an env is otherwise spread over five arrays (state, goals, meta,
     episode and the action stream's per-env block, which every launch recomputes): a wave of the lane-per-pair kernel opens a cold
     line in each of them at the start of every tick.  With live_record a rollout call packs the live buffers of its envs into one
     record per env before its first tick, every tick loads from and stores its live state back into that ONE line, and the call
     unpacks the records into state_live / goals_live / meta / episode after its last tick: the caller's buffers are current after the
     call exactly as without it, and every trajectory slot gets the same values at the same addresses.  Layout of a record:
         bytes   0 ..  63   state (vx, vy, px, py) of agents 0..3, 16 bytes each (agents >= n_agents: zero)
                64 ..  95   goals (x, y) of agents 0..3, 8 bytes each
                96 ..  99   steps          100 .. 103   collisions          104 .. 107   episode          108 .. 111   zero
               112 .. 127   the four stage-1 words of the env's action stream (Philox block (seed, global env id, call 0); a constant
                            of the env: a same-launch reset leaves it alone)
     Only for descriptors for which cm3_particle_live_record_applies() returns 1 (CM3_ERR_INVALID otherwise). */
} cm3_particle_traj;

int cm3_particle_rollout_f32(const cm3_particle_desc *desc, const cm3_particle_traj *traj, int32_t n_ticks,
                             void *stream);
int cm3_particle_rollout_f64(const cm3_particle_desc *desc, const cm3_particle_traj *traj, int32_t n_ticks,
                             void *stream);
/* 1 when a cm3_particle_rollout_* call of this descriptor (flags, n_envs and n_agents as they will be passed) can step on packed
 * live records (cm3_particle_traj.live_record): float32 (real_bytes == 4), CM3_FLAG_GEN_ACTIONS without CM3_FLAG_FUSED_TICKS,
 * n_agents in 2..4, and a batch that the lane-per-pair kernel steps (forced, or chosen from n_envs).  0 otherwise. */
int cm3_particle_live_record_applies(const cm3_particle_desc *desc, int32_t real_bytes);


/* ------------------------------------------------------------------------------------------
 * Checkers env (env/checkers.py).  Compact live state, reference-shaped outputs.
 *   mask     uint64 [E]      bit (k*n_columns + j) set <=> reward cell (row k, col j) collected
 *   agents   uint32 [N][E]   r | c<<8 | n_green<<16 | n_orange<<24   (expanded-grid coordinates)
 *   steps    int32  [E]
 *   goals    uint8  [E][N]   index of the colour the agent wants (0 green, 1 orange): argmax of the
 *                            reference's one-hot goals (checkers.py:234)
 *   actions  int32  [E][N]
 * Outputs (values identical to the reference's float64 arrays; integer-valued ones are stored as
 * integers):
 *   grid        int8   [E][n_rows][n_columns+1][2]        get_valid_grid (checkers.py:66-76); env records may be
 *                                                         padded, see grid_stride / obs_self_t_stride
 *   vec         int32  [E][N][4]                          (r, c, n_green, n_orange) (:79-94)
 *   obs_others  double [E][N][2*max(N-1,1)]               (:128-154, normalize :112-125)
 *   obs_self_t  int8   [E][N][2*n_obs+1][2*n_obs+1][3]    get_obs (:97-109)
 *   obs_self_v  double [E][N][4]
 *   local_rewards double [E][N]; reward double [E]; done uint8 [E]   (:228-262)
 * ---------------------------------------------------------------------------------------- */
typedef struct cm3_checkers_desc {
  int32_t n_envs;
  int32_t n_agents;   /* 1..CM3_MAX_AGENTS */
  int32_t n_rows;     /* odd  (checkers.py:16) */
  int32_t n_columns;  /* even (checkers.py:17); n_rows*n_columns <= 64 */
  int32_t n_obs;
  int32_t max_steps;
  uint32_t flags;     /* CM3_FLAG_AUTO_RESET, CM3_FLAG_GEN_ACTIONS */
  int32_t grid_stride;       /* bytes between consecutive envs' grid records; 0 = packed (n_rows*(n_columns+1)*2) */
  int32_t obs_self_t_stride; /* bytes between consecutive envs' obs_self_t records; 0 = packed (N*K*K*3).
                                Records padded to a multiple of 4 bytes (56 / 152 for the reference geometry with
                                N = 2) enable the multi-lane fast kernel, which writes each record up to its payload
                                rounded up to 4 bytes (the rounding bytes as 0; bytes of a LARGER stride beyond that are
                                left untouched) and indexes with 32-bit byte offsets: n_envs times the widest per-env record
                                of any per-tick array -- max(obs_self_t_stride, grid_stride, 32 N, 16 N max(N-1, 1)) bytes
                                (obs_others is the widest from N = 6 on: 896 B at N = 8) -- must stay below 4 GiB, else
                                CM3_ERR_INVALID */
  int32_t _pad;
  int64_t env_id_base;
  uint64_t seed;
  int32_t agents_r[CM3_MAX_AGENTS]; /* before expansion, as in config_checkers_*.json */
  int32_t agents_c[CM3_MAX_AGENTS];
} cm3_checkers_desc;

typedef struct cm3_checkers_bufs {
  uint64_t *mask;      /* in/out */
  uint32_t *agents;    /* in/out */
  int32_t *steps;      /* in/out */
  int32_t *episode;    /* in/out (RNG key for GEN_ACTIONS) */
  uint8_t *goals;      /* in; rewritten only for N == 1 under AUTO_RESET (train_onpolicy.py:288-291) */
  int32_t *actions;    /* in, or out under GEN_ACTIONS */
  int8_t *grid;
  int32_t *vec;
  double *obs_others;
  int8_t *obs_self_t;
  double *obs_self_v;
  double *local_rewards;
  double *reward;
  uint8_t *done;
  /* optional, all five or none: written ONLY for envs re-initialised by CM3_FLAG_AUTO_RESET in this launch -- their TRUE
     post-step observation, i.e. the next_* columns of the terminal transition, which the reference stores before it resets
     (train_onpolicy.py:336-347; checkers.py:246-262).  Same layouts / record strides as the five arrays above. */
  int8_t *term_grid;
  int32_t *term_vec;
  double *term_obs_others;
  int8_t *term_obs_self_t;
  double *term_obs_self_v;
  uint8_t *goals_next; /* optional uint8 [E][N]: the goals in effect AFTER this tick -- the goals column of the NEXT
                          transition (they change only when a single-agent env restarts, train_onpolicy.py:288-291) */
  const uint32_t *action_block; /* optional (ABI 6), uint32 [E][4], 16-byte aligned, filled ONCE per (seed, env_id_base) by
                          cm3_checkers_action_blocks: stage 1 of the in-kernel action stream (CM3_FLAG_GEN_ACTIONS), a constant per env.
                          With it a step launch loads the block with its state instead of running ten Philox rounds behind the
                          loads; NULL: the kernel computes the same block itself (identical actions). */
} cm3_checkers_bufs;

/* Trajectory collection for Checkers (train_onpolicy.py:302-350, 16-column transitions): n_ticks step launches over
 * a time-major trajectory, or ONE launch with CM3_FLAG_FUSED_TICKS (fast kernel only).  Observation arrays have
 * n_ticks+1 slots (slot t = before tick t); per-tick outputs n_ticks slots; strides in BYTES between slots.
 * With CM3_FLAG_AUTO_RESET (continuous collection) slot t+1 of an env whose episode ended at tick t holds the FRESH
 * episode's observation (what the policy acts on next) and the terminal next_* go to the term_* slots of tick t. */
typedef struct cm3_checkers_traj {
  uint64_t *mask; uint32_t *agents; int32_t *steps; int32_t *episode; uint8_t *goals; /* live, in place */
  int32_t *actions;      size_t actions_stride;
  int8_t *grid;          size_t grid_slot_stride;
  int32_t *vec;          size_t vec_stride;
  double *obs_others;    size_t obs_others_stride;
  int8_t *obs_self_t;    size_t obs_self_t_slot_stride;
  double *obs_self_v;    size_t obs_self_v_stride;
  double *local_rewards; size_t local_rewards_stride;
  double *reward;        size_t reward_stride;
  uint8_t *done;         size_t done_stride;
  /* optional terminal capture (see cm3_checkers_bufs), n_ticks slots each */
  int8_t *term_grid;        size_t term_grid_slot_stride;
  int32_t *term_vec;        size_t term_vec_stride;
  double *term_obs_others;  size_t term_obs_others_stride;
  int8_t *term_obs_self_t;  size_t term_obs_self_t_slot_stride;
  double *term_obs_self_v;  size_t term_obs_self_v_stride;
  uint8_t *goals_slots;     size_t goals_slots_stride; /* optional, n_ticks+1 slots of uint8 [E][N]; slot 0 is the caller's,
                                                          tick t writes slot t+1 (cm3_checkers_bufs.goals_next) */
  const uint32_t *action_block;  /* optional (ABI 6): see cm3_checkers_bufs.action_block */
} cm3_checkers_traj;

int cm3_checkers_rollout(const cm3_checkers_desc *desc, const cm3_checkers_traj *traj, int32_t n_ticks, void *stream);

/* Stage 1 of the in-kernel action stream for every env of `desc` (seed, env_id_base, n_envs): out = uint32 [E][4], the Philox block
 * action_block(seed, global env id, 0) of csrc/philox.h.  Once per env object (ABI 6; since round 5 the Checkers kernels draw with
 * the particle kernels' two-stage stream: action = rand5(fmix32((word ^ step) + episode * 0x9E3779B1))). */
int cm3_checkers_action_blocks(const cm3_checkers_desc *desc, uint32_t *out, void *stream);
/* SCOPE of that table: it holds Philox call 0 = the words of agents 0..3; with 5..8 agents the second block (agents
 * 4..7) is still computed in every step launch, so the round-5 gain applies to n_agents <= 4.  The table is a function of
 * (desc->seed, desc->env_id_base, n_envs): REBUILD it whenever one of them changes -- a step launch cannot check, a stale table
 * silently draws another action stream (cm3_amd.checkers.VecCheckersEnv builds it once per env object, whose seed and base are fixed). */
/* Replaces Checkers.step (checkers.py:228-262): agents act sequentially in index order inside one lane. */
int cm3_checkers_step(const cm3_checkers_desc *desc, const cm3_checkers_bufs *bufs, void *stream);
/* Replaces Checkers.reset (checkers.py:265-291) for the envs selected by mask (NULL = all). */
int cm3_checkers_reset(const cm3_checkers_desc *desc, const cm3_checkers_bufs *bufs, const uint8_t *mask,
                       void *stream);

/* ------------------------------------------------------------------------------------------
 * On-device particle actor: networks.actor_particle (networks.py:517-538) + the epsilon-mixed categorical
 * sampling of alg_credit.py:119-120 / run_actor :249-270, for all E*N agent rows in one launch.
 * Weights are float32, row-major [in][out] exactly as the TF variables are shaped:
 *   w_self [6][64] + b_self [64]            "actor_branch_self" (input = concat(v_obs[4], v_goal[2]))
 *   w_self_h2 [64][64]                      "W_branch_self_h2"
 *   w_others [L][128] + b_others [128]      "stage-2/actor_others"    (stage > 1 only; L = 4*max(N-1,1))
 *   w_others_h2 [128][64]                   "stage-2/W_others_h2"
 *   b_h2 [64]                               "b"
 *   w_out [64][5] + b_out [5]               "actor_out"
 * Inputs are the env's own buffers (obs_others [E][N][L], state [N][E][4], goals [N][E][2], meta, episode) -- float32 for
 * cm3_actor_particle_f32, float64 for cm3_actor_particle_f64, which rounds them to float32 (to nearest even) as it stages them,
 * as the reference's tf.float32 placeholders do with its float64 observations; the network is float32 either way;
 * outputs actions int32 [E][N] (what cm3_particle_step_* consumes) and optionally the mixed probabilities
 * float [E][N][5].  Sampling inverts the CDF in action order with one uniform per agent-step from the Philox
 * stream keyed (seed, global env id, episode, step).
 * ---------------------------------------------------------------------------------------- */
typedef struct cm3_actor_particle_desc {
  int32_t n_envs, n_agents;
  int32_t stage;       /* 1: self branch only; 2: + others branch */
  int32_t n_h1_self, n_h1_others, n_h2, n_actions; /* 64, 128, 64, 5 */
  float epsilon;
  int32_t precision;   /* 0: float32 throughout (exact-f32 MFMA: a k-ordered fmaf chain).  1: second layer on the bf16
                          matrix cores with float32 accumulation (activations and W2 rounded to bf16; probabilities move
                          by up to ~1e-2).  2: SPLIT float16 -- activations and W2 as hi + lo float16 pairs, three f16 MFMA
                          passes (hi hi + hi lo + lo hi), float32 accumulation (22 of 24 significand bits per factor):
                          probabilities within the 2e-5 of the float64 oracle that precision 0 is held to, ~5x fewer
                          matrix-core cycles; first-layer activations must stay below 65504.  With 16..32 others inputs (5..9
                          agents) actor_others runs in the same split float16 (inputs and weights split alike; inputs below
                          65504 too: they are relative positions / velocities) */
  int32_t _pad;
  int64_t env_id_base;
  uint64_t seed;
} cm3_actor_particle_desc;

typedef struct cm3_actor_particle_weights {
  const float *w_self, *b_self, *w_self_h2, *w_others, *b_others, *w_others_h2, *b_h2, *w_out, *b_out;
  const void *packed; /* kernel-layout copy written by cm3_actor_particle_pack (cm3_actor_particle_packed_bytes()
                         bytes); the forward launch reads ONLY this buffer, re-pack after every weight update */
} cm3_actor_particle_weights;

typedef struct cm3_actor_particle_bufs {
  const void *obs_others;
  const void *state;
  const void *goals;
  const int32_t *meta;
  const int32_t *episode;
  int32_t *actions;
  float *probs; /* optional */
  const float *epsilon_dev; /* optional device float: read at launch INSTEAD of desc->epsilon, so a captured hipGraph
                               follows the epsilon annealing of train_onpolicy.py:369 without being re-captured */
} cm3_actor_particle_bufs;

size_t cm3_actor_particle_packed_bytes(int32_t n_agents);
/* Re-arranges the TensorFlow-shaped weights into the forward kernel's layout (unit-major first-layer tables, per-lane
 * MFMA B operands in f32 and bf16) -- one small launch per weight update; only desc->n_agents / stage are read. */
int cm3_actor_particle_pack(const cm3_actor_particle_desc *desc, const cm3_actor_particle_weights *weights,
                            void *packed, void *stream);
int cm3_actor_particle_f32(const cm3_actor_particle_desc *desc, const cm3_actor_particle_weights *weights,
                           const cm3_actor_particle_bufs *bufs, void *stream);
/* The same actor on a float64 env's buffers (ABI 8): actions and probabilities bit-identical to cm3_actor_particle_f32 on the
 * float32 roundings of those buffers.  probs stays float32. */
int cm3_actor_particle_f64(const cm3_actor_particle_desc *desc, const cm3_actor_particle_weights *weights,
                           const cm3_actor_particle_bufs *bufs, void *stream);

/* The same actor over TRANSITION rows (part of ABI 9, additive): what alg_credit.train_step evaluates twice per minibatch -- the
 * Policy_target weights with sampling (action_samples_target, alg_credit.py:128, run_actor_target :272-287) on obs_others_next /
 * v_local_next / goals, and the Policy_main weights forward only (probs, :121) on obs_others / v_local / goals.  Row r comes from
 * three row-major float32 arrays -- the batch columns viewed as [B * N, .] -- and n_rows is any positive count (not a multiple of
 * n_agents).  A row's mixed probabilities are, bit for bit, those cm3_actor_particle_f32 computes for the same L + 6 inputs at the
 * same stage and precision.  Every output is optional, at least one is required:
 *   probs    the mixed probabilities (1 - eps) softmax + eps / 5
 *   actions  the sampled action: the inverse CDF in action order, as cm3_actor_particle_f32 picks, at the row's uniform
 *   onehot   the sampled action as int64 one-hot rows, the form of cm3_qmix_rows.onehot
 * The uniform of row r is (float)((word + 0.5) 2^-32) of word .x of the Philox4x32-10 block with counter (row id lo, row id hi, draw,
 * 0x10000000) and key seed, where row id = row_id_base + r (64 bit): a purpose of its own in counter word 3, so these draws meet no
 * other stream of the build.  The caller advances `draw` once per launch; equal (seed, row id, draw) reproduce a draw.  With actions
 * and onehot both NULL nothing is drawn.  (Anonymous struct tag, like cm3_qmix_rows.) */
typedef struct {
  const float *obs_others;  /* [n_rows][4*max(N-1,1)], 16-byte aligned */
  const float *v_obs;       /* [n_rows][4], 16-byte aligned */
  const float *goals;       /* [n_rows][2],  8-byte aligned */
  float   *probs;           /* optional [n_rows][5] */
  int32_t *actions;         /* optional [n_rows] */
  int64_t *onehot;          /* optional [n_rows][5], 16-byte aligned */
  const float *epsilon_dev; /* optional device float: read at launch INSTEAD of desc->epsilon */
  int64_t  n_rows;
  int64_t  row_id_base;
  uint32_t draw;
  uint32_t _pad;
} cm3_actor_rows;
/* desc is validated as for cm3_actor_particle_f32 (n_agents 1..10, the widths 64/128/64/5, precision 0..2, epsilon in [0,1]); stage
 * and seed are read, n_envs and env_id_base are not.  CM3_ERR_INVALID before any launch: null desc / weights / rows, weights->packed
 * NULL, a missing input, no output requested, n_rows <= 0 or more than 64 * (2^31 - 1), a misaligned input or onehot pointer.
 * cm3_last_kernel_variant() names the launch k_actor_particle_rows<f32,N=..,...>. */
int cm3_actor_particle_rows_f32(const cm3_actor_particle_desc *desc, const cm3_actor_particle_weights *weights,
                                const cm3_actor_rows *rows, void *stream);
/* The same launch with a draw counter it keeps ITSELF (part of ABI 9, additive), for launches captured into a hipGraph: a captured
 * cm3_actor_particle_rows_f32 bakes rows->draw in, so every replay would draw the same uniforms.  draw_state: two uint32 words in
 * device memory, 8-byte aligned, {draw, arrivals}; the caller initialises them once, with arrivals = 0.  The launch draws every row
 * at draw = word 0 -- the actions are those of cm3_actor_particle_rows_f32 at rows->draw = word 0, the probabilities the same bits
 * -- and leaves word 0 + 1 (mod 2^32) in word 0 and arrivals = 0, within the same launch (no node more in a captured graph; each
 * workgroup takes a ticket from `arrivals` once it has read word 0, the last one writes; nothing waits).  rows->draw is ignored.  A
 * launch that draws nothing (actions and onehot both NULL) neither reads nor advances the counter.  Launches that share a counter
 * MUST be ordered on the device -- one stream, or graph dependencies: two in flight at once would count each other's arrivals.
 * Validation: every check of cm3_actor_particle_rows_f32 first, in its order and with its messages; then CM3_ERR_INVALID for
 * draw_state == NULL, then for a draw_state that is not 8-byte aligned; all before any launch.  cm3_last_kernel_variant() names the
 * kernel of the uncounted launch with a ",counted" suffix: k_actor_particle_rows<f32,N=..,...,counted>. */
int cm3_actor_particle_rows_counted_f32(const cm3_actor_particle_desc *desc, const cm3_actor_particle_weights *weights,
                                        const cm3_actor_rows *rows, uint32_t *draw_state, void *stream);

/* ------------------------------------------------------------------------------------------
 * On-device QMIX agent (ABI 9): networks.Qmix_single_particle (networks.py:581-594) + the epsilon-greedy choice of
 * alg_qmix.run_actor (alg_qmix.py:160-184), for all E*N agent rows in one launch.  Float32 weights, row-major [in][out] as
 * the TF variables "Agent_main/..." are shaped (L = 4*max(N-1,1)):
 *   tensors[0] h/kernel [L+6][64]    tensors[1] h/bias [64]     (input = concat(o_others[L], o_self[4], goal[2]))
 *   tensors[2] h2/kernel [64][64]    tensors[3] h2/bias [64]
 *   tensors[4] out/kernel [64][5]    tensors[5] out/bias [5]    (Q values, no softmax)
 * The descriptor and buffers are the particle actor's: n_agents 1..10, n_envs >= 1, n_h1_self = n_h2 = 64, n_actions = 5,
 * precision 0 (float32 throughout; n_h1_others and stage are not read), epsilon in [0,1] (or bufs->epsilon_dev, read at launch).
 * Inputs as for cm3_actor_particle_f32 / _f64 (float64 envs are rounded to float32 as the inputs are staged).  Outputs:
 * actions int32 [E][N] -- argmax Q (the first index on ties), replaced with probability epsilon by a uniform action -- and, when
 * bufs->probs is set, the Q values float [E][N][5].  The two exploration draws per agent-step ("explore?", the uniform action)
 * come from the build's Philox stream with a purpose of their own, keyed (seed, global env id, episode, step, agent).
 * ---------------------------------------------------------------------------------------- */
size_t cm3_qmix_particle_packed_bytes(int32_t n_agents);
/* Re-arranges the six TensorFlow-shaped tensors into the forward kernel's layout; one small launch per weight update.
 * Only desc->n_agents and the widths are read. */
int cm3_qmix_particle_pack(const cm3_actor_particle_desc *desc, const float *const *tensors, void *packed, void *stream);
int cm3_qmix_particle_f32(const cm3_actor_particle_desc *desc, const void *packed, const cm3_actor_particle_bufs *bufs,
                          void *stream);
int cm3_qmix_particle_f64(const cm3_actor_particle_desc *desc, const void *packed, const cm3_actor_particle_bufs *bufs,
                          void *stream);

/* The same network over TRANSITION rows (part of ABI 9, additive): what alg_qmix.train_step evaluates with the Agent_target weights
 * (argmax_Q_target, alg_qmix.py:349-356) on the next observation of every sampled agent row.  Row r comes from three row-major
 * float32 arrays -- the columns obs_others_next / v_local_next / goals of a sampled batch viewed as [B * N, .] -- and n_rows is any
 * positive count (not a multiple of n_agents).  The head is a pure argmax (the first index on ties); nothing is drawn.  A row's Q values
 * are, bit for bit, those cm3_qmix_particle_f32 computes for the same L + 6 inputs.  Every output is optional, at least one is required:
 *   q       the Q values                                  argmax  the greedy action
 *   onehot  the reference's actions_target_1hot (int64)     q_max   Q of the greedy action
 * (Anonymous struct tag, like cm3_episode_route_desc.) */
typedef struct {
  const float *obs_others;  /* [n_rows][4*max(N-1,1)], 16-byte aligned */
  const float *v_obs;       /* [n_rows][4], 16-byte aligned */
  const float *goals;       /* [n_rows][2],  8-byte aligned */
  float   *q;               /* optional [n_rows][5] */
  int32_t *argmax;          /* optional [n_rows] */
  int64_t *onehot;          /* optional [n_rows][5], 16-byte aligned */
  float   *q_max;           /* optional [n_rows] */
  int64_t  n_rows;
} cm3_qmix_rows;
/* desc: n_agents 1..10, the widths 64/64/5 and precision 0 are validated; n_envs, epsilon, seed and env_id_base are not read.
 * packed: from cm3_qmix_particle_pack.  CM3_ERR_INVALID before any launch: null desc / packed / rows, a missing input, no output
 * requested, n_rows <= 0 or more than 64 * (2^31 - 1), a misaligned input or onehot pointer.  cm3_last_kernel_variant() names the
 * launch k_qmix_particle_rows<f32,N=..>. */
int cm3_qmix_particle_rows_f32(const cm3_actor_particle_desc *desc, const void *packed, const cm3_qmix_rows *rows, void *stream);

/* ------------------------------------------------------------------------------------------
 * CM3 particle critics over TRANSITION rows (part of ABI 9, additive): networks.Q_global_1output (networks.py:97-122) and
 * networks.Q_credit (:186-211) -- the evaluations of alg_credit.train_step that carry no gradient (Q_global_target :597,
 * Q_credit_target :620-640, the counterfactual Q_credit over every action :730-751, at one agent the counterfactual Q_global).
 * Float32 weights, row-major [in][out] as the TF variables of a scope "Q_global_main/..." / "Q_credit_target/..." are shaped:
 *   w_b1    Q_branch1/kernel [11][64]           b_b1  Q_branch1/bias [64]          (input = concat(s_n[4], g_n[2], a[5]))
 *   w_b1_h2 W_branch1_h2 [64][64]
 *   w_b2    stage-2/Q_branch2/kernel [K2][128]  b_b2  stage-2/Q_branch2/bias [128]  w_b2_h2 stage-2/W_branch2_h2 [128][64]
 *             global: K2 = 9 (N-1), input concat(s_others[4(N-1)], a_others[5(N-1)]); credit: K2 = 4 N, concat(s_m[4], s_others)
 *   w_out   Q_out/kernel [64][1]                (h2 and out have no bias)
 * The three stage-2 tensors are read at stage 2 only.  kind global: stage 1 with one agent, stage 2 with more; kind credit: stage 2
 * with more than one agent.
 * ---------------------------------------------------------------------------------------- */
#define CM3_CRITIC_GLOBAL 0
#define CM3_CRITIC_CREDIT 1
typedef struct {
  int32_t n_agents;              /* 1..CM3_MAX_AGENTS */
  int32_t stage;                 /* 1 / 2 */
  int32_t kind;                  /* CM3_CRITIC_GLOBAL / CM3_CRITIC_CREDIT */
  int32_t n_h1_1, n_h1_2, n_h2;  /* 64 / 128 / 64 */
} cm3_critic_particle_desc;

typedef struct {
  const float *w_b1, *b_b1, *w_b1_h2, *w_b2, *b_b2, *w_b2_h2, *w_out;
  const void *packed; /* kernel-layout copy written by cm3_critic_particle_pack (cm3_critic_particle_packed_bytes() bytes, 16-byte
                         aligned); the rows launch reads ONLY this buffer, re-pack after every weight update */
} cm3_critic_particle_weights;

/* The launch takes NO tiled feed: its inputs are the base columns of a batch of n_steps transitions, and a row's inputs are decoded
 * from the row number by `form` (s_others / a_others run over the agents j != n in ascending order):
 *   CM3_CRITIC_ROWS  (global)  r = b N + n             s_n, g_n of (b, n); a = onehot(actions[b][n])
 *   CM3_CRITIC_PAIRS (credit)  r = (b N + m) N + n     s_n, g_n, s_others of n; a = onehot(actions[b][m]), s_m = state[b][m]
 *   CM3_CRITIC_CF              r = r' 5 + a            a = row a of eye(5), no action array read; credit: r' = the PAIRS index;
 *                                                      global with one agent: r' = b
 * Every output is optional, at least one is required; rows at or past the row count n_steps * N (* N) (* 5) are not written:
 *   q    float32 [R]     q64  float64 [R], the same value widened
 *   td   float64 [R] = reward[b][n] + gamma * q * (1 - done[b]), in the order and bits of cm3_td_target_f64 applied to q64 (ROWS and
 *        PAIRS only)
 * Every contraction is k-ordered: a row's bits depend on neither its place in a workgroup nor the row count, and a PAIRS row equals
 * the CF row of the same (b, m, n) at a = actions[b][m].  (Anonymous struct tags, like cm3_qmix_rows.) */
#define CM3_CRITIC_ROWS 0
#define CM3_CRITIC_PAIRS 1
#define CM3_CRITIC_CF 2
typedef struct {
  int32_t form;             /* CM3_CRITIC_ROWS / _PAIRS / _CF */
  int32_t reward_f64;       /* reward holds float64 (else float32) */
  const float *state;       /* [n_steps][N][4], 16-byte aligned */
  const float *goals;       /* [n_steps][N][2],  8-byte aligned */
  const int32_t *actions;   /* [n_steps][N], values 0..4 (ROWS, PAIRS) */
  const void *reward;       /* [n_steps][N] (td) */
  const uint8_t *done;      /* [n_steps], 0 / 1 (td) */
  double gamma;
  float *q;
  double *q64;
  double *td;
  int64_t n_steps;
} cm3_critic_rows;

/* 0 for an agent count outside 1..10, an unknown kind, and kind credit with one agent */
size_t cm3_critic_particle_packed_bytes(int32_t n_agents, int32_t kind);
/* Re-arranges the TensorFlow-shaped weights into the rows kernel's per-lane operand order: one small launch per weight update, on
 * persistent tensors (capturable).  CM3_ERR_INVALID: the descriptor checks below, null weights / packed, a missing tensor. */
int cm3_critic_particle_pack(const cm3_critic_particle_desc *desc, const cm3_critic_particle_weights *weights, void *packed,
                             void *stream);
/* CM3_ERR_INVALID with a readable cm3_last_error() before anything touches the device: null desc / weights / rows,
 * weights->packed NULL, n_agents outside 1..10, an unknown kind or stage, kind credit with one agent or stage 1, kind global with a
 * stage that does not go with the agent count, other widths than 64/128/64, a form the kind does not have, n_steps <= 0 or a row
 * count above 2^31 - 1, a missing input the form needs (state, goals; actions for ROWS / PAIRS; reward and done with td), no
 * output requested, td with CF, a misaligned pointer.  cm3_last_kernel_variant() names the launch
 * k_critic_particle_rows<f32,N=..,...,kind=..,form=..>. */
int cm3_critic_particle_rows_f32(const cm3_critic_particle_desc *desc, const cm3_critic_particle_weights *weights,
                                 const cm3_critic_rows *rows, void *stream);

/* ------------------------------------------------------------------------------------------
 * The IAC / COMA baseline critics over TRANSITION rows (part of ABI 9, additive; particle env): the value networks
 * networks.V_particle_local (networks.py:356-374, IAC) and networks.V_particle_global (:377-402), and the COMA critic
 * networks.Q_global (:84-94) -- the evaluations of alg_baseline.train_step that carry no gradient (V_target / V on the next-step
 * columns :534, Q_target :576, Q :616).  Float32 weights, row-major [in][out] as the TF variables of the scopes "V_main/...",
 * "V_target/...", "Q_main/...", "Q_target/..." are shaped.  One form: row r = b N + n, decoded from the base columns; "others" run
 * over the agents j != n in ascending order.
 *
 * Value networks (widths 64 / 128 / 64: the branch-self default, V_n_others, V_n_h2 of config.json):
 *   w_b1    local: V_particle_branch_self/kernel [6][64], input concat(v_obs[4], goal[2]);  global: V_particle_branch1/kernel [6][64],
 *           input concat(state_n[4], goal_n[2]);  b_b1 its bias [64]
 *   w_b1_h2 local: W_branch_self_out [64][64];  global: W_branch1_h2 [64][64]
 *   w_b2    local: stage-2/V_local_others/kernel [4(N-1)][128], input obs_others;  global: stage-2/V_particle_branch2/kernel
 *           [6(N-1)][128], input concat(state of the others [4(N-1)], goals of the others [2(N-1)]);  b_b2 its bias [128]
 *   w_b2_h2 local: stage-2/W_others_out [128][64];  global: stage-2/W_branch2_h2 [128][64]
 *   w_out   V_particle_out/kernel [64][1]          (h2 and out have no bias)
 * The three stage-2 tensors are read at stage 2 only; stage 1 with one agent, stage 2 with more.
 * ---------------------------------------------------------------------------------------- */
#define CM3_VALUE_LOCAL 0
#define CM3_VALUE_GLOBAL 1
typedef struct {
  int32_t n_agents;              /* 1..CM3_MAX_AGENTS */
  int32_t stage;                 /* 1 / 2 */
  int32_t kind;                  /* CM3_VALUE_LOCAL / CM3_VALUE_GLOBAL */
  int32_t n_h1, n_others, n_h2;  /* 64 / 128 / 64 */
} cm3_value_particle_desc;

typedef struct {
  const float *w_b1, *b_b1, *w_b1_h2, *w_b2, *b_b2, *w_b2_h2, *w_out;
  const void *packed; /* kernel-layout copy written by cm3_value_particle_pack (cm3_value_particle_packed_bytes() bytes, 16-byte
                         aligned); the rows launch reads ONLY this buffer, re-pack after every weight update */
} cm3_value_particle_weights;

/* Every output is optional, at least one is required; rows at or past the row count n_steps * N are not written:
 *   v    float32 [R]     v64  float64 [R], the same value widened
 *   td   float64 [R] = reward[b][n] + gamma * v * (1 - done[b]), in the order and bits of cm3_td_target_f64 applied to v64 */
typedef struct {
  int32_t reward_f64;       /* reward holds float64 (else float32) */
  int32_t reserved;
  const float *state;       /* global: v_global [n_steps][N][4]; local: v_obs [n_steps][N][4]; 16-byte aligned */
  const float *obs_others;  /* local at stage 2: [n_steps][N][4(N-1)], 16-byte aligned */
  const float *goals;       /* [n_steps][N][2], 8-byte aligned */
  const void *reward;       /* the LOCAL reward [n_steps][N] (td) */
  const uint8_t *done;      /* [n_steps], 0 / 1 (td) */
  double gamma;
  float *v;
  double *v64;
  double *td;
  int64_t n_steps;
} cm3_value_rows;

/* 0 for an agent count outside 1..10 and an unknown kind */
size_t cm3_value_particle_packed_bytes(int32_t n_agents, int32_t kind);
/* One small launch per weight update, on persistent tensors (capturable).  CM3_ERR_INVALID: the descriptor checks below, null
 * weights / packed, a missing tensor. */
int cm3_value_particle_pack(const cm3_value_particle_desc *desc, const cm3_value_particle_weights *weights, void *packed, void *stream);
/* CM3_ERR_INVALID with a readable cm3_last_error() before anything touches the device, in this order: null desc, n_agents outside
 * 1..10, an unknown kind or stage, a stage that does not go with the agent count, other widths than 64/128/64; null weights / rows,
 * weights->packed NULL; n_steps <= 0 or a row count above 2^31 - 1; a missing input (state, goals; obs_others for a local network at
 * stage 2); no output requested; td without reward and done; a misaligned input, reward, output, packed.
 * cm3_last_kernel_variant() names the launch k_value_particle_rows<f32,N=..,...,kind=local|global>. */
int cm3_value_particle_rows_f32(const cm3_value_particle_desc *desc, const cm3_value_particle_weights *weights,
                                const cm3_value_rows *rows, void *stream);

/* The COMA critic, fc3 K -> 256 -> 256 -> 5 (ReLU on both hidden layers, biases on all three), N = 2..10:
 *   input = concat(state of all agents [4N], one-hot actions of the others [5(N-1)], goal_n [2], goals of the others [2(N-1)],
 *                  one-hot label of n [N], v_obs_n [4]),  K = 12 N - 1
 *   w_h1 stage-2/Q_goals/h1/kernel [K][256]   b_h1 .../h1/bias [256]      w_h2 .../h2/kernel [256][256]   b_h2 .../h2/bias [256]
 *   w_out .../out/kernel [256][5]             b_out .../out/bias [5] */
typedef struct {
  int32_t n_agents;   /* 2..CM3_MAX_AGENTS */
  int32_t units;      /* 256 (Q_units) */
} cm3_coma_particle_desc;

typedef struct {
  const float *w_h1, *b_h1, *w_h2, *b_h2, *w_out, *b_out;
  const void *packed; /* written by cm3_coma_particle_pack (cm3_coma_particle_packed_bytes() bytes, 16-byte aligned) */
} cm3_coma_particle_weights;

/* Every output is optional, at least one is required; rows at or past the row count n_steps * N are not written:
 *   q          float32 [R][5]
 *   q_taken    float32 [R] = q[r][own_actions[b][n]] (np.sum(Q * actions_self_1hot, axis=1), alg_baseline.py:577); q_taken64 the same
 *              value widened; an own action outside 0..4 leaves the row's q_taken, q_taken64 and td unwritten
 *   td         float64 [R] = reward[b] + gamma * q_taken * (1 - done[b]) with the GLOBAL reward [n_steps] (:581), in the order and
 *              bits of cm3_td_target_f64 applied to q_taken64 */
typedef struct {
  int32_t reward_f64;          /* reward holds float64 (else float32) */
  int32_t reserved;
  const float *state;          /* v_global [n_steps][N][4], 16-byte aligned */
  const float *goals;          /* [n_steps][N][2], 8-byte aligned */
  const float *v_obs;          /* v_local [n_steps][N][4], 16-byte aligned */
  const int32_t *actions;      /* [n_steps][N], values 0..4: a row reads those of the OTHER agents */
  const int32_t *own_actions;  /* optional [n_steps][N], values 0..4: the row's own action (q_taken, q_taken64, td) */
  const void *reward;          /* the GLOBAL reward [n_steps] (td) */
  const uint8_t *done;         /* [n_steps], 0 / 1 (td) */
  double gamma;
  float *q;
  float *q_taken;
  double *q_taken64;
  double *td;
  int64_t n_steps;
} cm3_coma_rows;

/* 0 for an agent count outside 2..10 */
size_t cm3_coma_particle_packed_bytes(int32_t n_agents);
int cm3_coma_particle_pack(const cm3_coma_particle_desc *desc, const cm3_coma_particle_weights *weights, void *packed, void *stream);
/* CM3_ERR_INVALID before anything touches the device, in this order: null desc, n_agents outside 2..10, another width than 256; null
 * weights / rows, weights->packed NULL; n_steps <= 0 or a row count above 2^31 - 1; a missing input (state, goals, v_obs; actions);
 * no output requested; q_taken / q_taken64 / td without own_actions; td without reward and done; a misaligned input, reward,
 * output, packed.  cm3_last_kernel_variant() names the launch k_coma_particle_rows<f32,N=..,...>. */
int cm3_coma_particle_rows_f32(const cm3_coma_particle_desc *desc, const cm3_coma_particle_weights *weights, const cm3_coma_rows *rows,
                               void *stream);

/* ------------------------------------------------------------------------------------------
 * The Checkers IAC / COMA baseline critics over TRANSITION rows (part of ABI 9, additive): networks.V_checkers_local
 * (networks.py:415-435), networks.V_checkers_global (:438-458) and networks.Q_coma_checkers (:293-306) at the widths
 * alg_baseline_checkers.py:117-138 passes -- the evaluations of alg_baseline_checkers.train_step that carry no gradient (V_target /
 * V :527, Q_target :572, Q :617).  One form: row r = b N + n, decoded from the base columns of a Checkers batch (dtypes as in
 * cm3_critic_checkers_rows below: int8 or float64 grids and windows, float64 vectors, uint8 index or int64 one-hot goals; all
 * rounded to float32 in the kernel); "others" run over the agents j != n in ascending order.  Agent counts 1..8 (COMA: 2..8).
 * CM3_VALUE_LOCAL / CM3_VALUE_GLOBAL are those of the particle value networks.  Float32 weights as the TF variables of a scope
 * "V_main/...", "V_target/...", "Q_main/...", "Q_target/..." are shaped:
 *
 * Value networks (widths 256 / 32 / 256):
 *   conv_w   conv/Conv/weights: local [3][3][3][6] over the window [5][5][3] -> 150; global [3][5][2][4] over the grid [3][9][2] ->
 *            108 (SAME, NHWC flatten);  conv_b conv/Conv/biases [6] / [4]
 *   w_b1     local: branch_self/kernel [156][256], input concat(conv, obs_self_v[4], goal[2]);  global: V_branch1/kernel [114][256],
 *            input concat(conv, s_n[4], g_n[2]);  b_b1 its bias [256]
 *   w_b1_h2  local: W_self_h2 [256][256];  global: W_branch1_h2 [256][256]
 *   w_b2     local: stage-2/branch_others/kernel [2(N-1)][32], input obs_others;  global: stage-2/V_branch2/kernel [4(N-1)][32],
 *            input the states of the other agents;  b_b2 its bias [32]
 *   w_b2_h2  local: stage-2/W_others_h2 [32][256];  global: stage-2/W_branch2_h2 [32][256]
 *   w_out    local: V_checkers_out/kernel [256][1];  global: V_out/kernel [256][1];  b_out its bias [1]     (h2 has no bias)
 * The three stage-2 tensors are read at stage 2 only; stage 1 with one agent, stage 2 with more.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int32_t n_agents;               /* 1..8 */
  int32_t stage;                  /* 1 / 2 */
  int32_t kind;                   /* CM3_VALUE_LOCAL / CM3_VALUE_GLOBAL */
  int32_t n_h1_1, n_h1_2, n_h2;   /* 256 / 32 / 256 */
} cm3_value_checkers_desc;

typedef struct {
  const float *conv_w, *conv_b;
  const float *w_b1, *b_b1, *w_b1_h2, *w_b2, *b_b2, *w_b2_h2, *w_out, *b_out;
  const void *packed; /* kernel-layout copy written by cm3_value_checkers_pack (cm3_value_checkers_packed_bytes() bytes, 16-byte
                         aligned); the rows launch reads ONLY this buffer, re-pack after every weight update */
} cm3_value_checkers_weights;

/* A local network reads windows, obs_self_v, goals (and obs_others at stage 2); a global one grid, vec, goals.  Outputs as in
 * cm3_value_rows: v float32 [R], v64 the same value widened, td float64 [R] = reward[b][n] + gamma * v * (1 - done[b]) in the bits
 * of cm3_td_target_f64 applied to v64; at least one is required; rows past the row count are not written. */
typedef struct {
  int32_t reward_f64;       /* reward holds float64 (else float32) */
  int32_t grid_f64;         /* grid holds float64 (else int8) */
  int32_t windows_f64;      /* windows holds float64 (else int8) */
  int32_t goals_onehot;     /* goals holds int64 one-hot [n_steps][N][2] (else uint8 indices [n_steps][N]) */
  const void *grid;         /* global: [n_steps][3][9][2] */
  const double *vec;        /* global: [n_steps][N][4] agent state */
  const void *goals;
  const void *windows;      /* local: [n_steps][N][75] (obs_self_t) */
  const double *obs_self_v; /* local: [n_steps][N][4] */
  const double *obs_others; /* local at stage 2: [n_steps][N][2(N-1)] */
  const void *reward;       /* the LOCAL reward [n_steps][N] (td) */
  const uint8_t *done;      /* [n_steps], 0 / 1 (td) */
  double gamma;
  float *v;
  double *v64;
  double *td;
  int64_t n_steps;
} cm3_value_checkers_rows;

/* 0 for an agent count outside 1..8 and an unknown kind */
size_t cm3_value_checkers_packed_bytes(int32_t n_agents, int32_t kind);
/* Re-arranges the TensorFlow-shaped weights into the rows kernel's per-lane operand order, the convolution as a Toeplitz matrix: one
 * launch per weight update, on persistent tensors (capturable). */
int cm3_value_checkers_pack(const cm3_value_checkers_desc *desc, const cm3_value_checkers_weights *weights, void *packed, void *stream);
/* CM3_ERR_INVALID with a readable cm3_last_error() before anything touches the device, in this order: null desc, n_agents outside
 * 1..8, an unknown kind or stage, a stage that does not go with the agent count, other widths than 256/32/256; null weights / rows,
 * weights->packed NULL; n_steps <= 0 or a row count above 2^31 - 1; a missing input (obs_others for a local network at stage 2
 * after the others); no output requested; td without reward and done; a misaligned input, reward, output, packed.
 * cm3_last_kernel_variant() names the launch k_value_checkers_rows<f32,N=..,...,kind=local|global>. */
int cm3_value_checkers_rows_f32(const cm3_value_checkers_desc *desc, const cm3_value_checkers_weights *weights,
                                const cm3_value_checkers_rows *rows, void *stream);

/* The Checkers COMA critic, N = 2..8: fc3 K -> 256 -> 256 -> 5 (ReLU on both hidden layers, biases on all three) on
 *   input = concat(conv_s(grid) [108], states of all agents [4N], one-hot actions of the others [5(N-1)], g_n [2], goals of the
 *                  others [2(N-1)], one-hot label of n [N], conv_o(window of n) [150], obs_self_v of n [4]),  K = 257 + 12 N
 *   conv_s_w conv_s/Conv/weights [3][5][2][4]   conv_s_b conv_s/Conv/biases [4]   conv_o_w conv_o/Conv/weights [3][3][3][6]
 *   conv_o_b conv_o/Conv/biases [6]             w_h1 stage-2/Q_coma_checkers/h1/kernel [K][256]   b_h1 .../h1/bias [256]
 *   w_h2 .../h2/kernel [256][256]   b_h2 .../h2/bias [256]   w_out .../out/kernel [256][5]   b_out .../out/bias [5] */
typedef struct {
  int32_t n_agents;   /* 2..8 */
  int32_t units;      /* 256 */
} cm3_coma_checkers_desc;

typedef struct {
  const float *conv_s_w, *conv_s_b, *conv_o_w, *conv_o_b;
  const float *w_h1, *b_h1, *w_h2, *b_h2, *w_out, *b_out;
  const void *packed; /* written by cm3_coma_checkers_pack (cm3_coma_checkers_packed_bytes() bytes, 16-byte aligned) */
} cm3_coma_checkers_weights;

/* Outputs as in cm3_coma_rows: q float32 [R][5]; q_taken float32 [R] = q[r][own_actions[b][n]], q_taken64 the same value widened (an
 * own action outside 0..4 leaves the row's q_taken, q_taken64 and td unwritten); td float64 [R] = reward[b] + gamma * q_taken *
 * (1 - done[b]) with the GLOBAL reward [n_steps], in the bits of cm3_td_target_f64 applied to q_taken64. */
typedef struct {
  int32_t reward_f64;          /* reward holds float64 (else float32) */
  int32_t grid_f64;            /* grid holds float64 (else int8) */
  int32_t windows_f64;         /* windows holds float64 (else int8) */
  int32_t goals_onehot;        /* goals holds int64 one-hot [n_steps][N][2] (else uint8 indices [n_steps][N]) */
  const void *grid;            /* [n_steps][3][9][2] */
  const double *vec;           /* [n_steps][N][4] agent state */
  const void *goals;
  const int32_t *actions;      /* [n_steps][N], values 0..4: a row reads those of the OTHER agents */
  const int32_t *own_actions;  /* optional [n_steps][N], values 0..4: the row's own action (q_taken, q_taken64, td) */
  const void *windows;         /* [n_steps][N][75] (obs_self_t) */
  const double *obs_self_v;    /* [n_steps][N][4] */
  const void *reward;          /* the GLOBAL reward [n_steps] (td) */
  const uint8_t *done;         /* [n_steps], 0 / 1 (td) */
  double gamma;
  float *q;
  float *q_taken;
  double *q_taken64;
  double *td;
  int64_t n_steps;
} cm3_coma_checkers_rows;

/* 0 for an agent count outside 2..8 */
size_t cm3_coma_checkers_packed_bytes(int32_t n_agents);
int cm3_coma_checkers_pack(const cm3_coma_checkers_desc *desc, const cm3_coma_checkers_weights *weights, void *packed, void *stream);
/* CM3_ERR_INVALID before anything touches the device, in this order: null desc, n_agents outside 2..8, another width than 256; null
 * weights / rows, weights->packed NULL; n_steps <= 0 or a row count above 2^31 - 1; a missing input (grid, vec, goals, windows,
 * obs_self_v; actions); no output requested; q_taken / q_taken64 / td without own_actions; td without reward and done; a misaligned
 * input, reward, output, packed.  cm3_last_kernel_variant() names the launch k_coma_checkers_rows<f32,N=..,...>. */
int cm3_coma_checkers_rows_f32(const cm3_coma_checkers_desc *desc, const cm3_coma_checkers_weights *weights,
                               const cm3_coma_checkers_rows *rows, void *stream);

/* ------------------------------------------------------------------------------------------
 * CM3 Checkers critics over TRANSITION rows (part of ABI 9, additive): networks.Q_global_checkers (networks.py:155-183) and
 * networks.Q_credit_checkers (:244-272) at the widths of config_checkers_stage{1,2}.json -- the evaluations of
 * alg_credit_checkers.train_step that carry no gradient (Q_global_target :558-569, Q_credit_target :611-629, the counterfactual
 * Q_credit over every action :738-747, at one agent the counterfactual Q_global :704-713).
 * Float32 weights as the TF variables of a scope "Q_global_main/..." / "Q_credit_target/..." are shaped:
 *   conv_w   conv/Conv/weights [3][5][2][4]      conv_b   conv/Conv/biases [4]      (SAME, over the grid [3][9][2])
 *   conv_o_w conv_o/Conv/weights [3][3][3][6]    conv_o_b conv_o/Conv/biases [6]    (SAME, over the window [5][5][3])
 *   w_b1     Q_branch1/kernel [273][256]         b_b1     Q_branch1/bias [256]
 *              (input = concat(conv[108], s_n[4], g_n[2], a[5], conv_o[150], v_obs[4]), convolution outputs flattened NHWC)
 *   w_b1_h2  W_branch1_h2 [256][256]
 *   w_b2     stage-2/Q_branch2/kernel [K2][32]   b_b2     stage-2/Q_branch2/bias [32]   w_b2_h2 stage-2/W_branch2_h2 [32][256]
 *              global: K2 = 9 (N-1), input concat(s_others[4(N-1)], a_others[5(N-1)]); credit: K2 = 4 N, concat(s_m[4], s_others)
 *   w_out    Q_out/kernel [256][1]               b_out    Q_out/bias [1]            (h2 has no bias)
 * The three stage-2 tensors are read at stage 2 only.  kind global: stage 1 with one agent, stage 2 with more; kind credit: stage 2
 * with more than one agent.  Agent counts 1..8 (the Checkers actor's range).  CM3_CRITIC_GLOBAL / _CREDIT and CM3_CRITIC_ROWS /
 * _PAIRS / _CF are those of the particle critics above.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int32_t n_agents;                 /* 1..8 */
  int32_t stage;                    /* 1 / 2 */
  int32_t kind;                     /* CM3_CRITIC_GLOBAL / CM3_CRITIC_CREDIT */
  int32_t grid_h, grid_w, grid_c;   /* 3 / 9 / 2 */
  int32_t win_h, win_w, win_c;      /* 5 / 5 / 3 */
  int32_t n_h1_1, n_h1_2, n_h2;     /* 256 / 32 / 256 */
} cm3_critic_checkers_desc;

typedef struct {
  const float *conv_w, *conv_b, *conv_o_w, *conv_o_b;
  const float *w_b1, *b_b1, *w_b1_h2, *w_b2, *b_b2, *w_b2_h2, *w_out, *b_out;
  const void *packed; /* kernel-layout copy written by cm3_critic_checkers_pack (cm3_critic_checkers_packed_bytes() bytes, 16-byte
                         aligned); the rows launch reads ONLY this buffer, re-pack after every weight update */
} cm3_critic_checkers_weights;

/* The launch takes NO tiled feed: its inputs are the base columns of a batch of n_steps transitions, and a row's inputs are decoded
 * from the row number by `form` (s_others / a_others run over the agents j != n in ascending order; the grid is that of step b):
 *   CM3_CRITIC_ROWS  (global)  r = b N + n             s_n, g_n, window, v_obs of (b, n); a = onehot(actions[b][n])
 *   CM3_CRITIC_PAIRS (credit)  r = (b N + m) N + n     s_n, g_n, s_others of n; a = onehot(actions[b][m]), s_m = vec[b][m]; the
 *                                                      window and v_obs are those of agent M (the reference repeats obs_self_t /
 *                                                      obs_self_v "indexed by m")
 *   CM3_CRITIC_CF              r = r' 5 + a            a = row a of eye(5), no action array read; credit: r' = the PAIRS index;
 *                                                      global with one agent: r' = b
 * float64 inputs are rounded to float32 in the kernel, as the reference's tf.float32 placeholders do.  Outputs as in
 * cm3_critic_rows: q float32 [R], q64 the same value widened, td float64 [R] = reward[b][n] + gamma * q * (1 - done[b]) in the bits
 * of cm3_td_target_f64 applied to q64 (ROWS and PAIRS only); at least one is required; rows past the row count are not written.
 * Every contraction is k-ordered: a row's bits depend on neither its place in a workgroup nor the row count, and a PAIRS row equals
 * the CF row of the same (b, m, n) at a = actions[b][m]. */
typedef struct {
  int32_t form;             /* CM3_CRITIC_ROWS / _PAIRS / _CF */
  int32_t reward_f64;       /* reward holds float64 (else float32) */
  int32_t grid_f64;         /* grid holds float64 (else int8) */
  int32_t windows_f64;      /* windows holds float64 (else int8) */
  int32_t goals_onehot;     /* goals holds int64 one-hot [n_steps][N][2] (else uint8 indices [n_steps][N]) */
  int32_t reserved;         /* 0 */
  const void *grid;         /* [n_steps][3][9][2] */
  const double *vec;        /* [n_steps][N][4] agent state */
  const void *goals;
  const int32_t *actions;   /* [n_steps][N], values 0..4 (ROWS, PAIRS) */
  const void *windows;      /* [n_steps][N][75] (obs_self_t) */
  const double *obs_self_v; /* [n_steps][N][4] */
  const void *reward;       /* [n_steps][N] (td) */
  const uint8_t *done;      /* [n_steps], 0 / 1 (td) */
  double gamma;
  float *q;
  double *q64;
  double *td;
  int64_t n_steps;
} cm3_critic_checkers_rows;

/* 0 for an agent count outside 1..8, an unknown kind, and kind credit with one agent */
size_t cm3_critic_checkers_packed_bytes(int32_t n_agents, int32_t kind);
/* Re-arranges the TensorFlow-shaped weights into the rows kernel's per-lane operand order, the two convolutions as Toeplitz
 * matrices: one launch per weight update, on persistent tensors (capturable).  CM3_ERR_INVALID: the descriptor checks below, null
 * weights / packed, a missing tensor. */
int cm3_critic_checkers_pack(const cm3_critic_checkers_desc *desc, const cm3_critic_checkers_weights *weights, void *packed,
                             void *stream);
/* CM3_ERR_INVALID with a readable cm3_last_error() before anything touches the device: null desc / weights / rows,
 * weights->packed NULL, n_agents outside 1..8, an unknown kind or stage, kind credit with one agent or stage 1, kind global with a
 * stage that does not go with the agent count, another geometry than 3x9x2 / 5x5x3, other widths than 256/32/256, a form the kind
 * does not have, n_steps <= 0 or a row count above 2^31 - 1, a missing input the form needs (grid, vec, goals, windows, obs_self_v;
 * actions for ROWS / PAIRS; reward and done with td), no output requested, td with CF, a misaligned pointer.
 * cm3_last_kernel_variant() names the launch k_critic_checkers_rows<f32,N=..,...,kind=..,form=..>. */
int cm3_critic_checkers_rows_f32(const cm3_critic_checkers_desc *desc, const cm3_critic_checkers_weights *weights,
                                 const cm3_critic_checkers_rows *rows, void *stream);

/* ------------------------------------------------------------------------------------------
 * The particle QMIX mixer over TRANSITION rows (part of ABI 9, additive): networks.Qmix_mixer (networks.py:640-685) -- mixer_target
 * of alg_qmix.train_step (alg_qmix.py:358-365), the one evaluation of the mixer that carries no gradient -- and the TD target that
 * follows it (:367-369).  Per transition b, x = concat(state[b] [4N], goals[b] [2N]), K = 6N.  Float32 weights, row-major [in][out]
 * as the TF variables of a scope "Mixer_main/..." / "Mixer_target/..." are shaped:
 *   hyper_w_1        hyper_w_1 [K][64 N]                 w1 = |x . hyper_w_1| viewed [N][64]
 *   hyper_w_final    hyper_w_final [K][64]               w_final = |x . hyper_w_final|
 *   hyper_b_1        hyper_b_1 [K][64]                   b1 = x . hyper_b_1
 *   hyper_b_final_l1 hyper_b_final_l1/kernel [K][64]     l1 = relu(x . kernel)                    (no bias)
 *   hyper_b_final    hyper_b_final/kernel [64][1]        b_final = l1 . kernel                    (no bias)
 *   hidden = elu(agent_qs[b][0..N) . w1 + b1),  q_tot = hidden . w_final + b_final
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int32_t n_agents;   /* 1..CM3_MAX_AGENTS */
  int32_t embed_dim;  /* 64 */
} cm3_qmix_mixer_particle_desc;

typedef struct {
  const float *hyper_w_1, *hyper_w_final, *hyper_b_1, *hyper_b_final_l1, *hyper_b_final;
  const void *packed; /* kernel-layout copy written by cm3_qmix_mixer_particle_pack (cm3_qmix_mixer_particle_packed_bytes() bytes,
                         16-byte aligned); the rows launch reads ONLY this buffer, re-pack after every weight update */
} cm3_qmix_mixer_particle_weights;

/* The base columns of a batch of n_steps transitions and the optional outputs, at least one required; nothing is written at or past
 * n_steps:
 *   q_tot    float32 [n_steps]    q_tot64  float64 [n_steps], the same value widened
 *   td       float64 [n_steps] = sum(reward[b][0..N)) + gamma * q_tot * (1 - done[b]), the bits cm3_qmix_td_target_f64 produces from
 *            this launch's float32 q_tot (np.sum's order in float64, gamma * q_tot in float32)
 * The sum over agents is a chain in ascending n started by the product for n = 0, b1 added last; the sum over the 64 embedding
 * units is a fixed tree (csrc/mixer.hip): a row's bits depend on neither its place in a workgroup nor n_steps.  (Anonymous struct
 * tags, like cm3_qmix_rows.) */
typedef struct {
  int32_t reward_f64;       /* reward holds float64 (else float32) */
  int32_t reserved;         /* 0 */
  const float *state;       /* [n_steps][N][4], 16-byte aligned */
  const float *goals;       /* [n_steps][N][2],  8-byte aligned */
  const float *agent_qs;    /* [n_steps][N]: the target agents' Q at their argmax (cm3_qmix_rows.q_max) */
  const void *reward;       /* [n_steps][N] reward_local (td) */
  const uint8_t *done;      /* [n_steps], 0 / 1 (td) */
  double gamma;
  float *q_tot;
  double *q_tot64;
  double *td;
  int64_t n_steps;
} cm3_qmix_mixer_rows;

/* 0 for an agent count outside 1..10 */
size_t cm3_qmix_mixer_particle_packed_bytes(int32_t n_agents);
/* Re-arranges the TensorFlow-shaped weights into the rows kernel's per-lane operand order, K zero-padded to whole k-steps: one small
 * launch per weight update, on persistent tensors (capturable).  CM3_ERR_INVALID: the descriptor checks below, null weights /
 * packed, a missing tensor, a misaligned packed. */
int cm3_qmix_mixer_particle_pack(const cm3_qmix_mixer_particle_desc *desc, const cm3_qmix_mixer_particle_weights *weights, void *packed,
                                 void *stream);
/* CM3_ERR_INVALID with a readable cm3_last_error() before anything touches the device: null desc / weights / rows,
 * weights->packed NULL, n_agents outside 1..10, another embedding width than 64, n_steps <= 0 or above 2^31 - 1, a missing input
 * (state, goals, agent_qs; reward and done with td), no output requested, a misaligned pointer.  cm3_last_kernel_variant() names the
 * launch k_qmix_mixer_rows<f32,N=..>. */
int cm3_qmix_mixer_particle_rows_f32(const cm3_qmix_mixer_particle_desc *desc, const cm3_qmix_mixer_particle_weights *weights,
                                     const cm3_qmix_mixer_rows *rows, void *stream);

/* ------------------------------------------------------------------------------------------
 * The particle QMIX learner (part of ABI 9, additive): mixer_op of alg_qmix.train_step (alg_qmix.py:186-192, 371-378) -- the loss
 * mean((float32(td_target) - q_tot)^2) and its dense gradients for the six variables of Agent_main (networks.Qmix_single_particle,
 * shared by the agents: their gradient sums over the B N agent rows) and the five of Mixer_main (networks.Qmix_mixer), in float32,
 * with TensorFlow's conventions at the kinks (ReluGrad passes where the input is > 0, d|x|/dx = sign(x) with 0 at 0, EluGrad below
 * zero is elu + 1).  Five launches on the given stream, every one capturable; no floating-point atomics: every output element is
 * summed in an order fixed by the row count alone (csrc/learner.hip), so two calls on the same inputs give the same bits.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int32_t n_agents;   /* 1..CM3_MAX_AGENTS */
  int32_t n_h;        /* 64: both hidden widths of Qmix_single_particle */
  int32_t n_actions;  /* 5 */
  int32_t embed_dim;  /* 64 */
} cm3_qmix_learner_particle_desc;

/* The eleven tensors, float32 row-major as the TF variables are shaped -- the weights read, or the gradients written (dense, every
 * element).  With L = 4 max(N - 1, 1), K = 6 N: */
typedef struct {
  float *h_kernel;          /* Agent_main/h/kernel    [L + 6][64] */
  float *h_bias;            /* Agent_main/h/bias      [64] */
  float *h2_kernel;         /* Agent_main/h2/kernel   [64][64] */
  float *h2_bias;           /* Agent_main/h2/bias     [64] */
  float *out_kernel;        /* Agent_main/out/kernel  [64][5] */
  float *out_bias;          /* Agent_main/out/bias    [5] */
  float *hyper_w_1;         /* Mixer_main/hyper_w_1   [K][64 N] */
  float *hyper_w_final;     /* Mixer_main/hyper_w_final            [K][64] */
  float *hyper_b_1;         /* Mixer_main/hyper_b_1                [K][64] */
  float *hyper_b_final_l1;  /* Mixer_main/hyper_b_final_l1/kernel  [K][64] */
  float *hyper_b_final;     /* Mixer_main/hyper_b_final/kernel     [64][1] */
} cm3_qmix_learner_tensors;

/* The columns of a batch of n_steps transitions (B) of N agents, and the two outputs beside the gradients.  The agent rows are the
 * columns viewed [B N, .]; an action outside 0..4 selects no Q value (q_selected 0, no gradient into that row). */
typedef struct {
  int32_t td_f64;           /* td holds float64 (rounded to float32 as it is read: the td_target placeholder is tf.float32), else float32 */
  int32_t reserved;         /* 0 */
  const float *obs_others;  /* [B][N][L], 16-byte aligned */
  const float *v_obs;       /* [B][N][4] v_local, 16-byte aligned */
  const float *goals;       /* [B][N][2],  8-byte aligned: the agents' goal and the mixer's goals_all */
  const int32_t *actions;   /* [B][N] the actions taken */
  const float *state;       /* [B][N][4] v_global, 16-byte aligned */
  const void *td;           /* [B] the TD target */
  float *loss;              /* [1] */
  float *q_tot;             /* [B]: the bits cm3_qmix_mixer_particle_rows_f32 computes from the same weights and Q values */
  int64_t n_steps;
} cm3_qmix_learner_rows;

/* Bytes of scratch cm3_qmix_learner_particle_grad_f32 takes for this agent count and batch (csrc/learner.hip: the inputs and
 * activations of the rows, the deltas, one partial gradient per 256 rows); grows with n_steps.  0 for an agent count outside 1..10
 * or n_steps outside 1..(2^31 - 1) / 10. */
size_t cm3_qmix_learner_particle_workspace_bytes(int32_t n_agents, int64_t n_steps);
/* CM3_ERR_INVALID with a readable cm3_last_error() before anything touches the device, in this order: null desc, n_agents outside
 * 1..10, other widths than 64 / 5 / 64; null weights / grads / rows, a missing tensor, input, output or workspace, a misaligned
 * pointer; n_steps <= 0 or above (2^31 - 1) / 10, a workspace smaller than cm3_qmix_learner_particle_workspace_bytes().  Changes
 * nothing but grads, loss, q_tot and the workspace.  cm3_last_kernel_variant() names the last launch, k_qmix_learner_reduce<f32,N=..,after=fwd+mixer+bwd+xtd>,
 * and so the four before it. */
int cm3_qmix_learner_particle_grad_f32(const cm3_qmix_learner_particle_desc *desc, const cm3_qmix_learner_tensors *weights,
                                       const cm3_qmix_learner_tensors *grads, const cm3_qmix_learner_rows *rows, void *workspace,
                                       size_t workspace_bytes, void *stream);

/* tf.train.AdamOptimizer's step (TF1: epsilon OUTSIDE the bias correction -- not torch.optim.Adam's formula) in float32 over a table
 * of tensors, ONE launch:
 *   lr_t = lr sqrt(1 - beta2_power) / (1 - beta1_power);  m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g g;
 *   var = var - lr_t m / (sqrt(v) + epsilon)
 * state: 16 bytes of device memory, 8-byte aligned, {float beta1_power, float beta2_power, uint32 0, uint32 0}, set up once with the
 * powers at beta1 and beta2 (as TF initialises beta1_power / beta2_power).  The launch reads the powers and leaves them multiplied by
 * beta1 / beta2, so a replayed hipGraph takes the next step.  Launches that share a state must be ordered on the device. */
typedef struct {
  float *var;         /* updated in place */
  const float *grad;
  float *m, *v;       /* the two moments, updated in place (zeros before the first step) */
  int64_t count;      /* elements */
} cm3_adam_segment;

typedef struct {
  float lr, beta1, beta2, epsilon;
  int32_t n_segments;
  int32_t reserved;   /* 0 */
  int64_t total;      /* the sum of the segments' counts: sizes the grid */
} cm3_adam_desc;

/* segments: a DEVICE array of desc->n_segments cm3_adam_segment, 8-byte aligned.  CM3_ERR_INVALID before anything touches the device,
 * in this order: null desc, a learning rate that is no number, a beta outside [0, 1), epsilon <= 0, n_segments < 1; null segments /
 * state, a misaligned pointer; total < 1.  cm3_last_kernel_variant() names the launch k_adam_step<f32,..>. */
int cm3_adam_step_f32(const cm3_adam_desc *desc, const cm3_adam_segment *segments, void *state, void *stream);

/* ------------------------------------------------------------------------------------------
 * The Checkers QMIX mixer over TRANSITION rows (part of ABI 9, additive): networks.Qmix_mixer_checkers (networks.py:688-734) at the
 * widths of config_checkers_stage{1,2}.json -- mixer_target of alg_qmix_checkers.train_step (alg_qmix_checkers.py:364-375) -- and the
 * TD target that follows it (:377-379).  Per transition b, conv = relu(conv2d SAME 3x5x2 -> 4 over grid[b] [3][9][2] + biases)
 * flattened NHWC to 108, x = concat(conv, state[b] [4N], goals[b] [2N]), K = 108 + 6N; the rest is the particle mixer above at
 * embed_dim 128.  Float32 weights as the TF variables of a scope "Mixer_main/..." / "Mixer_target/..." are shaped:
 *   conv_w           conv/Conv/weights [3][5][2][4]      conv_b   conv/Conv/biases [4]
 *   hyper_w_1        hyper_w_1 [K][128 N]                w1 = |x . hyper_w_1| viewed [N][128]
 *   hyper_w_final    hyper_w_final [K][128]              w_final = |x . hyper_w_final|
 *   hyper_b_1        hyper_b_1 [K][128]                  b1 = x . hyper_b_1
 *   hyper_b_final_l1 hyper_b_final_l1/kernel [K][128]    l1 = relu(x . kernel)                    (no bias)
 *   hyper_b_final    hyper_b_final/kernel [128][1]       b_final = l1 . kernel                    (no bias)
 *   hidden = elu(agent_qs[b][0..N) . w1 + b1),  q_tot = hidden . w_final + b_final
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int32_t n_agents;                  /* 1..8 */
  int32_t embed_dim;                 /* 128 */
  int32_t grid_h, grid_w, grid_c;    /* 3, 9, 2 */
  int32_t conv_f, conv_kh, conv_kw;  /* 4, 3, 5 (Q_conv_f, Q_conv_k) */
} cm3_qmix_mixer_checkers_desc;

typedef struct {
  const float *conv_w, *conv_b, *hyper_w_1, *hyper_w_final, *hyper_b_1, *hyper_b_final_l1, *hyper_b_final;
  const void *packed; /* kernel-layout copy written by cm3_qmix_mixer_checkers_pack (cm3_qmix_mixer_checkers_packed_bytes() bytes,
                         16-byte aligned); the rows launch reads ONLY this buffer, re-pack after every weight update */
} cm3_qmix_mixer_checkers_weights;

/* The base columns of a batch of n_steps transitions in the forms the Checkers columns have, and the optional outputs (those of
 * cm3_qmix_mixer_rows, at least one required; nothing is written at or past n_steps).  Float64 values are rounded to float32 as they
 * are read, as a tf.float32 placeholder rounds its feed.  td = sum(reward[b][0..N)) + gamma * q_tot * (1 - done[b]), the bits
 * cm3_qmix_td_target_f64 produces from this launch's float32 q_tot.  Every sum has a fixed order (csrc/mixer.hip): a row's bits depend
 * on neither its place in a workgroup nor n_steps.  (Anonymous struct tags, like cm3_qmix_rows.) */
typedef struct {
  int32_t grid_f64;         /* grid holds float64 [n_steps][54] (else int8) */
  int32_t goals_onehot;     /* goals holds int64 one-hot [n_steps][N][2] (else uint8 index [n_steps][N]) */
  int32_t reward_f64;       /* reward holds float64 (else float32) */
  int32_t reserved;         /* 0 */
  const void *grid;         /* [n_steps][3][9][2]; float64: 8-byte aligned */
  const double *vec;        /* [n_steps][N][4] the agents' states */
  const void *goals;        /* one-hot: 8-byte aligned */
  const float *agent_qs;    /* [n_steps][N]: the target agents' Q at their argmax (cm3_qmix_checkers_rows.q_max) */
  const void *reward;       /* [n_steps][N] local_rewards (td) */
  const uint8_t *done;      /* [n_steps], 0 / 1 (td) */
  double gamma;
  float *q_tot;
  double *q_tot64;
  double *td;
  int64_t n_steps;
} cm3_qmix_mixer_checkers_rows;

/* 0 for an agent count outside 1..8 */
size_t cm3_qmix_mixer_checkers_packed_bytes(int32_t n_agents);
/* Re-arranges the TensorFlow-shaped weights into the rows kernel's tiles -- the convolution as a Toeplitz matrix, K zero-padded to
 * whole k groups: one small launch per weight update, on persistent tensors (capturable).  CM3_ERR_INVALID: the descriptor checks
 * below, null weights / packed, a missing tensor, a misaligned packed. */
int cm3_qmix_mixer_checkers_pack(const cm3_qmix_mixer_checkers_desc *desc, const cm3_qmix_mixer_checkers_weights *weights, void *packed,
                                 void *stream);
/* CM3_ERR_INVALID with a readable cm3_last_error() before anything touches the device: null desc / weights / rows,
 * weights->packed NULL, n_agents outside 1..8, another embedding width than 128, another grid than 3x9x2 or convolution than 4 filters
 * of 3x5, n_steps <= 0 or above 2^31 - 1, a missing input (grid, vec, goals, agent_qs; reward and done with td), no output requested,
 * a misaligned pointer.  cm3_last_kernel_variant() names the launch k_ck_qmix_mixer_rows<f32,N=..>. */
int cm3_qmix_mixer_checkers_rows_f32(const cm3_qmix_mixer_checkers_desc *desc, const cm3_qmix_mixer_checkers_weights *weights,
                                     const cm3_qmix_mixer_checkers_rows *rows, void *stream);

/* A whole policy-driven episode in ONE launch: for every tick, actor forward pass + sampling (as cm3_actor_particle_f32)
 * followed by the env step (as cm3_particle_step_f32), with the network weights, the observation tile and the env
 * state resident in LDS / registers.  Same trajectory layout and flags as cm3_particle_rollout_f32 (AUTO_RESET honoured;
 * GEN_ACTIONS rejected: the policy draws the actions, written to traj->actions).  probs (optional) receives the mixed
 * probabilities per tick, float [n_ticks][E][N][5] with probs_stride bytes between ticks.  n_agents 1..10: a wave owns a 16-row
 * tile that holds 16 / n_agents whole envs, so n_agents in {3,5,6,7,9,10} leave 1 .. 7 rows of every tile unused (builds of their
 * own; same results, fewer envs per workgroup).  actor_desc and desc must agree on n_envs / n_agents / seed / env_id_base.
 * Bit-identical to alternating cm3_actor_particle_f32 and cm3_particle_step_f32 launches.  cm3_last_kernel_variant() names the
 * launch k_policy_rollout<f32,N=..,..g=<row tiles per workgroup>..>. */
int cm3_policy_rollout_f32(const cm3_particle_desc *desc, const cm3_particle_traj *traj,
                           const cm3_actor_particle_desc *actor_desc, const cm3_actor_particle_weights *weights,
                           float *probs, size_t probs_stride, int32_t n_ticks, void *stream);
/* The same one-launch episode on a float64 env (ABI 8): trajectory arrays float64 as for cm3_particle_rollout_f64, the physics,
 * rewards and re-initialisation in float64 (the operation order and contact-skip threshold of cm3_particle_step_f64), the network
 * float32 on the float32 roundings of each tick's observation.  probs stays float32.  Same validation as the _f32 entry, except
 * n_agents in {1,2,4,8}: the padded-tile builds exist for float32 envs only.
 * Bit-identical to alternating cm3_actor_particle_f64 and cm3_particle_step_f64 launches. */
int cm3_policy_rollout_f64(const cm3_particle_desc *desc, const cm3_particle_traj *traj,
                           const cm3_actor_particle_desc *actor_desc, const cm3_actor_particle_weights *weights,
                           float *probs, size_t probs_stride, int32_t n_ticks, void *stream);
/* The same one-launch rollout driven by the QMIX agent (part of ABI 9, additive; float32 envs): for every tick the agent network and
 * its epsilon-greedy choice (as cm3_qmix_particle_f32) followed by the env step (as cm3_particle_step_f32).  CONTRACT: every output --
 * the trajectory slots, actions, rewards, done, per-tick collisions, the terminal captures, meta / episode, and q_values -- equals,
 * bit for bit, what n_ticks x (cm3_qmix_particle_f32, cm3_particle_step_f32) write.
 *   desc, traj, n_ticks   validated as cm3_policy_rollout_f32 validates them (AUTO_RESET honoured, GEN_ACTIONS rejected)
 *   agent                 validated as cm3_qmix_particle_f32 validates it (64/64/5, precision 0; n_h1_others and stage are not read);
 *                         n_agents equal in both descriptors and in {1,2,4,8}; agent->seed == desc->seed and agent->env_id_base ==
 *                         desc->env_id_base (policy and env draw under one Philox key)
 *   packed                from cm3_qmix_particle_pack, non-NULL
 *   q_values              optional: the raw Q values per tick, float [n_ticks][E][N][5], q_stride bytes between ticks (the unit of
 *                         probs_stride)
 *   epsilon_dev           optional device float, read once at launch INSTEAD of agent->epsilon
 * Every failure returns CM3_ERR_INVALID with a readable cm3_last_error() before anything touches the device.  Workgroups are 64 rows
 * at every batch size: cm3_policy_force_row_tiles does not apply.  cm3_last_kernel_variant() names the launch
 * k_policy_rollout_qmix<f32,N=..>. */
int cm3_policy_rollout_qmix_f32(const cm3_particle_desc *desc, const cm3_particle_traj *traj,
                                const cm3_actor_particle_desc *agent, const void *packed,
                                float *q_values, size_t q_stride, const float *epsilon_dev,
                                int32_t n_ticks, void *stream);
/* Test / measurement knob (ABI 6): 16-row tiles per workgroup of cm3_policy_rollout_f32 and _f64 -- 1, 2 or 4 forces that build of the
 * kernel for every later launch of the process, 0 gives the choice back to the library's rule (by batch size).  Results do not
 * depend on it (tests/test_gpu_actor.py forces each build on one batch).  Initial value: the environment's CM3_POLICY_RT, read
 * once at the first launch. */
int cm3_policy_force_row_tiles(int32_t row_tiles);

/* ------------------------------------------------------------------------------------------
 * On-device Checkers actor: networks.convnet_1 + networks.actor_checkers (networks.py:67-75, :549-578) + the
 * epsilon-mixed categorical sampling of alg_credit_checkers.py:107-113 / run_actor :229-253, for all E*N agent rows in
 * one launch; every layer on the matrix cores (exact-f32 MFMA).  Weights are float32, shaped as the TF variables:
 *   conv_w [3][3][3][6] + conv_b [6]        "conv/Conv/weights", "conv/Conv/biases"  (3x3, stride 1, SAME, relu; NHWC)
 *   lin_w [150][32] + lin_b [32]            "conv_linear"
 *   self_w [43][256] + self_b [256]         "branch_self"  (input = concat(conv_linear 32, v_obs_self 4, a_prev 5, goal 2))
 *   w_self_h2 [256][256]                    "W_self_h2"
 *   others_w [2(N-1)][256] + others_b       "stage-2/branch_others"   (stage > 1 only)
 *   w_others_h2 [256][256]                  "stage-2/W_others_h2"
 *   b_h2 [256]                              "b"
 *   out_w [256][5] + out_b [5]              "actor_out"
 * Inputs are the env's own output buffers: obs_self_t int8 (env records of obs_self_t_stride bytes, agent i at byte
 * 75 i), obs_self_v double [E][N][4], obs_others double [E][N][2 max(N-1,1)] (cast to float32 like a TF feed), goals uint8
 * [E][N] (0 green / 1 orange -> one-hot), actions_prev int32 [E][N] (NULL = zeros, train_onpolicy.py:295), steps, episode.
 * Outputs: actions int32 [E][N] (what cm3_checkers_step consumes), optional mixed probabilities float [E][N][5].
 * ---------------------------------------------------------------------------------------- */
typedef struct cm3_actor_checkers_desc {
  int32_t n_envs, n_agents;
  int32_t stage;  /* 1: self branch only; 2: + others branch */
  int32_t n_obs;  /* 2 (5x5 window) */
  int32_t conv_f, n_conv_linear, n_h1, n_h2, n_actions; /* 6, 32, 256, 256, 5 */
  float epsilon;
  int32_t precision;         /* 0: float32 throughout (parity path).  1: the two 256x256 layers on the bf16 matrix cores with
                                float32 accumulation (first-layer activations and those weights rounded to bf16; probabilities
                                move by up to ~1e-2).  2: EVERY layer in split float16 -- activations and weights as float16
                                hi + lo, hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_f16, float32 accumulation: a parity
                                path (held to the 2e-5 of precision 0) in about half the time of precision 0 */
  int32_t obs_self_t_stride; /* bytes between env records of obs_self_t (cm3_checkers_desc.obs_self_t_stride) */
  int64_t env_id_base;
  uint64_t seed;
} cm3_actor_checkers_desc;

typedef struct cm3_actor_checkers_weights {
  const float *conv_w, *conv_b, *lin_w, *lin_b, *self_w, *self_b, *w_self_h2, *others_w, *others_b, *w_others_h2, *b_h2,
      *out_w, *out_b;
  const void *packed; /* written by cm3_actor_checkers_pack (cm3_actor_checkers_packed_bytes() bytes); the forward launch
                         reads ONLY this buffer */
} cm3_actor_checkers_weights;

typedef struct cm3_actor_checkers_bufs {
  const int8_t *obs_self_t;
  const double *obs_self_v;
  const double *obs_others;
  const uint8_t *goals;
  const int32_t *actions_prev; /* optional */
  const int32_t *steps;
  const int32_t *episode;
  int32_t *actions;
  float *probs; /* optional */
  const uint8_t *prev_done;  /* optional uint8 [E]: envs whose previous tick ended an episode (continuous collection with
                                CM3_FLAG_AUTO_RESET) feed actions_prev = zeros, as a fresh episode does (train_onpolicy.py:295) */
  const float *epsilon_dev;  /* optional device float read at launch instead of desc->epsilon (see cm3_actor_particle_bufs) */
} cm3_actor_checkers_bufs;

size_t cm3_actor_checkers_packed_bytes(void);
int cm3_actor_checkers_pack(const cm3_actor_checkers_desc *desc, const cm3_actor_checkers_weights *weights, void *packed,
                            void *stream);
int cm3_actor_checkers_f32(const cm3_actor_checkers_desc *desc, const cm3_actor_checkers_weights *weights,
                           const cm3_actor_checkers_bufs *bufs, void *stream);

/* ------------------------------------------------------------------------------------------
 * The Checkers QMIX learner (part of ABI 9, additive): mixer_op of alg_qmix_checkers.train_step (alg_qmix_checkers.py:184-190,
 * 381-391) -- the loss mean((float32(td_target) - q_tot)^2) and its dense float32 gradients for the thirteen variables of Agent_main
 * (networks.Qmix_single_checkers, shared by the agents: their gradient sums over the B N agent rows) and the seven of Mixer_main
 * (networks.Qmix_mixer_checkers), with TensorFlow's conventions at the kinks (ReluGrad passes where the input is > 0, d|x|/dx =
 * sign(x) with 0 at 0, EluGrad below zero is elu + 1).  Fourteen launches on the given stream (csrc/learner_checkers.hip), every one
 * capturable; no floating-point atomics: every sum's order is fixed by the row count alone, so two calls on the same inputs give the
 * same bits.  Weights and gradients go in as cm3_actor_checkers_weights / cm3_qmix_mixer_checkers_weights (TF-shaped tensors; `packed`
 * is not read: the launches follow the tensors as they are); the gradient structs name the tensors WRITTEN, dense, every element.
 * cm3_adam_step_f32 over a table of the twenty tensors applies them.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int32_t n_agents;                               /* 1..8 */
  int32_t conv_f, n_conv_linear, n_h1, n_h2;      /* 6, 32, 256, 256 */
  int32_t n_actions;                              /* 5 */
  int32_t embed_dim;                              /* 128 */
  int32_t mixer_conv_f;                           /* 4 */
} cm3_qmix_learner_checkers_desc;

/* The columns of a batch of n_steps transitions (B) of N agents in the forms the rows kernels read (cm3_qmix_checkers_rows,
 * cm3_qmix_mixer_checkers_rows), each value rounded to float32 as it is read, and the two outputs beside the gradients.  The agent
 * rows are the columns viewed [B N, .]; Lo = 2 max(N - 1, 1).  An action outside 0..4 selects no Q value (q_selected 0, no gradient
 * into that row). */
typedef struct {
  int32_t obs_self_t_f64;     /* obs_self_t holds float64 (else int8) */
  int32_t grid_f64;           /* grid holds float64 (else int8) */
  int32_t goals_onehot;       /* goals holds int64 one-hot [B][N][2] (else the uint8 index [B][N]) */
  int32_t td_f64;             /* td holds float64 (the td_target placeholder is tf.float32), else float32 */
  const void *obs_self_t;     /* [B][N][75]; float64: 8-byte aligned */
  const double *obs_self_v;   /* [B][N][4] */
  const double *obs_others;   /* [B][N][Lo] */
  const int32_t *actions_prev;/* [B][N], 0..4 */
  const int32_t *actions;     /* [B][N] the actions taken */
  const void *goals;          /* the agents' goal and the mixer's goals_all; one-hot: 8-byte aligned */
  const void *grid;           /* [B][3][9][2]; float64: 8-byte aligned */
  const double *vec;          /* [B][N][4] the agents' states */
  const void *td;             /* [B] the TD target */
  float *loss;                /* [1] */
  float *q_tot;               /* [B]: the bits cm3_qmix_mixer_checkers_rows_f32 computes from the same weights and Q values */
  int64_t n_steps;
} cm3_qmix_learner_checkers_rows;

/* Bytes of scratch cm3_qmix_learner_checkers_grad_f32 takes for this agent count and batch; grows with n_steps.  0 for an agent
 * count outside 1..8 or n_steps outside 1..(2^31 - 1) / 216 (every row index of the launches -- 27 grid positions per transition, 25
 * window positions per agent row -- stays in int32). */
size_t cm3_qmix_learner_checkers_workspace_bytes(int32_t n_agents, int64_t n_steps);
/* CM3_ERR_INVALID with a readable cm3_last_error() before anything touches the device, in this order: null desc, n_agents outside
 * 1..8, other widths than 6 / 32 / 256 / 256 / 5 and 128 / 4; null weights / grads / rows, a missing tensor, input, output or
 * workspace, a misaligned pointer; n_steps <= 0 or above (2^31 - 1) / 216, a workspace smaller than
 * cm3_qmix_learner_checkers_workspace_bytes().  Changes nothing but the gradients, loss, q_tot and the workspace.
 * cm3_last_kernel_variant() names the last launch, k_qmix_learner_checkers_reduce<f32,N=..,after=stage+6gemm+mixer+4gemm+xtd>, and so the
 * thirteen before it. */
int cm3_qmix_learner_checkers_grad_f32(const cm3_qmix_learner_checkers_desc *desc, const cm3_actor_checkers_weights *agent_weights,
                                       const cm3_qmix_mixer_checkers_weights *mixer_weights,
                                       const cm3_actor_checkers_weights *agent_grads, const cm3_qmix_mixer_checkers_weights *mixer_grads,
                                       const cm3_qmix_learner_checkers_rows *rows, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * On-device Checkers QMIX agent (part of ABI 9, additive): networks.Qmix_single_checkers (networks.py:617-637) + the
 * epsilon-greedy choice of alg_qmix_checkers.run_actor (alg_qmix_checkers.py:153-182), for all E*N agent rows in one launch.
 * The network is the actor's above with three differences: the others branch exists at every agent count (N = 1 included: its
 * input is the agent's own normalised position, 2 values), the output layer ("Qmix_single_out") gives Q values (no softmax),
 * and the head takes argmax Q (the first index on ties), replaced with probability epsilon by a uniform action.  Same structs:
 * weights under the names "conv/Conv/...", "conv_linear", "branch_self", "W_self_h2", "branch_others", "W_others_h2", "b",
 * "Qmix_single_out" (out_w / out_b), all thirteen required; desc->stage is not read; precision 0 (float32) or 2 (split
 * float16) -- 1 (bf16) is refused; epsilon from desc->epsilon or bufs->epsilon_dev.  Outputs: actions int32 [E][N] and, when
 * bufs->probs is set, the raw Q values float [E][N][5].  The two exploration draws per agent-step come from the stream of the
 * particle QMIX agent (cm3_qmix_particle_f32), keyed (seed, global env id, episode, step, agent).
 * ---------------------------------------------------------------------------------------- */
/* Packs into cm3_actor_checkers_packed_bytes() bytes; one small launch per weight update. */
int cm3_qmix_checkers_pack(const cm3_actor_checkers_desc *desc, const cm3_actor_checkers_weights *weights, void *packed,
                           void *stream);
/* Reads ONLY weights->packed (written by cm3_qmix_checkers_pack). */
int cm3_qmix_checkers_f32(const cm3_actor_checkers_desc *desc, const cm3_actor_checkers_weights *weights,
                          const cm3_actor_checkers_bufs *bufs, void *stream);

/* The same network over TRANSITION rows (part of ABI 9, additive): what alg_qmix_checkers.train_step evaluates with the Agent_target
 * weights (argmax_Q_target, alg_qmix_checkers.py:353-359) on every sampled agent row.  Row r comes from five row-major arrays over
 * n_rows rows -- the columns next_obs_self_t / next_obs_self_v / next_obs_others / actions / goals of a sampled batch viewed as
 * [B * N, .] (the reference feeds the action just taken as actions_prev there) -- and n_rows is any positive count (not a multiple of
 * n_agents).  The head is a pure argmax (the first index on ties); nothing is drawn: no steps, episode, prev_done, epsilon or seed.
 * A row's Q values are, bit for bit, those cm3_qmix_checkers_f32 computes for the same inputs at the same precision.
 *   obs_self_t   obs_self_t_f64 = 0: int8 [n_rows][75] (what the trajectory and the compact ring keep);
 *                obs_self_t_f64 = 1: float64 [n_rows][75] (what sample_batch of either ring returns), rounded to float32 as a
 *                tf.float32 placeholder rounds a fed array.  At precision 2 the window plane is ONE float16 plane, as in the collection
 *                kernel: float64 windows must then hold float16-exact values (the env's are -1 / 0 / 1).
 *   goals        goals_onehot = 0: the uint8 index [n_rows] (0 or 1); goals_onehot = 1: the int64 one-hot pair [n_rows][2], each of
 *                its two values converted to float as it is.
 * Alignment the staging relies on (checked): obs_self_t (both forms), obs_self_v, obs_others, one-hot goals and onehot 16 bytes;
 * actions_prev, q, argmax and q_max 4 bytes; index goals none.  No load touches a byte past n_rows rows of any input.
 * Every output is optional, at least one is required:
 *   q       the Q values                                  argmax  the greedy action
 *   onehot  the reference's actions_target_1hot (int64)     q_max   Q of the greedy action
 * Rows at or past n_rows are not written.  (Anonymous struct tag, like cm3_qmix_rows.) */
typedef struct {
  const void    *obs_self_t;    /* [n_rows][75] int8 or float64 (obs_self_t_f64), 16-byte aligned */
  const double  *obs_self_v;    /* [n_rows][4], 16-byte aligned */
  const double  *obs_others;    /* [n_rows][2*max(N-1,1)], 16-byte aligned */
  const int32_t *actions_prev;  /* [n_rows], 0..4 */
  const void    *goals;         /* [n_rows] uint8, or [n_rows][2] int64 (goals_onehot; then 16-byte aligned) */
  int32_t  obs_self_t_f64;      /* 0 / 1 */
  int32_t  goals_onehot;        /* 0 / 1 */
  float   *q;                   /* optional [n_rows][5] */
  int32_t *argmax;              /* optional [n_rows] */
  int64_t *onehot;              /* optional [n_rows][5], 16-byte aligned */
  float   *q_max;               /* optional [n_rows] */
  int64_t  n_rows;
} cm3_qmix_checkers_rows;
/* desc: validated like cm3_qmix_checkers_f32's (n_agents 1..8, the widths, n_obs 2) plus precision 0 or 2; n_envs, epsilon, seed,
 * env_id_base, stage and obs_self_t_stride are not read.  Reads ONLY weights->packed (cm3_qmix_checkers_pack).  CM3_ERR_INVALID before
 * any launch: null desc / weights / rows / weights->packed, a missing input, no output requested, n_rows <= 0 or more than
 * 64 * (2^31 - 1), a form flag other than 0 / 1, a misaligned pointer.  cm3_last_kernel_variant() names the launch
 * k_ck_qmix_rows<f32,N=..,g=F,..> or k_ck_qmix_rows_x3<..> with F = obs_self_t_f64 + 2 * goals_onehot. */
int cm3_qmix_checkers_rows_f32(const cm3_actor_checkers_desc *desc, const cm3_actor_checkers_weights *weights,
                               const cm3_qmix_checkers_rows *rows, void *stream);

/* The Checkers ACTOR over TRANSITION rows (part of ABI 9, additive): what alg_credit_checkers.train_step evaluates twice per
 * minibatch -- the Policy_target weights with sampling (action_samples_target, alg_credit_checkers.py:551, run_actor_target) on
 * next_obs_self_t / next_obs_self_v / next_obs_others / actions / goals (the reference feeds the action just taken as actions_prev
 * there), and the Policy_main weights forward only (probs, :107-113) on obs_self_t / obs_self_v / obs_others / actions_prev / goals.
 * The five inputs, the two form flags and the alignment rules are those of cm3_qmix_checkers_rows above (at precision 2 float64
 * windows must hold float16-exact values); n_rows is any positive count; no load touches a byte past n_rows rows of any input.
 * The network is cm3_actor_checkers_f32's: desc->stage IS read (1: no others branch, obs_others is staged but not contracted; 2: the
 * others branch at every agent count, N = 1 with its 2 values included), weights->packed comes from cm3_actor_checkers_pack, precision
 * 0, 1 or 2.  A row's mixed probabilities are, bit for bit, those cm3_actor_checkers_f32 computes for the same inputs at the same
 * stage and precision with prev_done = NULL.  Every output is optional, at least one is required:
 *   probs    the mixed probabilities (1 - eps) softmax + eps / 5
 *   actions  the sampled action: the inverse CDF in action order, as cm3_actor_checkers_f32 picks, at the row's uniform
 *   onehot   the sampled action as int64 one-hot rows, the form of cm3_qmix_checkers_rows.onehot
 * The uniform of row r is that of cm3_actor_rows: word .x of the Philox4x32-10 block with counter (row id lo, row id hi, draw,
 * 0x10000000) and key desc->seed, row id = row_id_base + r (64 bit).  The caller advances `draw` once per launch; equal (seed, row id,
 * draw) reproduce a draw.  With actions and onehot both NULL nothing is drawn.  Rows at or past n_rows are not written.
 * (Anonymous struct tag, like cm3_qmix_checkers_rows.) */
typedef struct {
  const void    *obs_self_t;    /* [n_rows][75] int8 or float64 (obs_self_t_f64), 16-byte aligned */
  const double  *obs_self_v;    /* [n_rows][4], 16-byte aligned */
  const double  *obs_others;    /* [n_rows][2*max(N-1,1)], 16-byte aligned */
  const int32_t *actions_prev;  /* [n_rows], 0..4 */
  const void    *goals;         /* [n_rows] uint8, or [n_rows][2] int64 (goals_onehot; then 16-byte aligned) */
  int32_t  obs_self_t_f64;      /* 0 / 1 */
  int32_t  goals_onehot;        /* 0 / 1 */
  float   *probs;               /* optional [n_rows][5] */
  int32_t *actions;             /* optional [n_rows] */
  int64_t *onehot;              /* optional [n_rows][5], 16-byte aligned */
  const float *epsilon_dev;     /* optional device float: read at launch INSTEAD of desc->epsilon */
  int64_t  n_rows;
  uint64_t row_id_base;
  uint32_t draw;
  uint32_t _pad;
} cm3_actor_checkers_rows;
/* desc: validated like cm3_actor_checkers_f32's (n_agents 1..8, the widths, n_obs 2, epsilon in [0,1]) plus precision 0 / 1 / 2 and
 * stage 1 / 2; stage, epsilon and seed are read, n_envs, env_id_base and obs_self_t_stride are not.  CM3_ERR_INVALID before any launch:
 * null desc / weights / rows / weights->packed, a missing input, no output requested, n_rows <= 0 or more than 64 * (2^31 - 1), a
 * form flag other than 0 / 1, a misaligned pointer (inputs as above; onehot 16 bytes, probs and actions 4).
 * cm3_last_kernel_variant() names the launch k_ck_actor_rows<f32,N=..,g=F,..,prec=P> or k_ck_actor_rows_x3<..> with
 * F = obs_self_t_f64 + 2 * goals_onehot. */
int cm3_actor_checkers_rows_f32(const cm3_actor_checkers_desc *desc, const cm3_actor_checkers_weights *weights,
                                const cm3_actor_checkers_rows *rows, void *stream);
/* The same launch with a draw counter it keeps itself (part of ABI 9, additive): draw_state, its two words, what the launch leaves
 * in them, the ordering rule for launches that share a counter and the validation order (every check of
 * cm3_actor_checkers_rows_f32 first, then NULL, then 8-byte alignment of draw_state) are those of
 * cm3_actor_particle_rows_counted_f32.  rows->draw is ignored; a probs-only launch neither reads nor advances the counter.
 * cm3_last_kernel_variant(): k_ck_actor_rows<..,counted> / k_ck_actor_rows_x3<..,counted>. */
int cm3_actor_checkers_rows_counted_f32(const cm3_actor_checkers_desc *desc, const cm3_actor_checkers_weights *weights,
                                        const cm3_actor_checkers_rows *rows, uint32_t *draw_state, void *stream);

/* A whole POLICY-DRIVEN Checkers rollout in ONE launch (ABI 7; csrc/policy_checkers.hip): per tick the actor above (precision 2),
 * epsilon-mixed sampling and Checkers.step with the actions just drawn -- train_onpolicy.py:309-347 / train_offpolicy.py:309-368 without
 * leaving the kernel; env state in registers, the network's inputs written straight into LDS, the others branch of the two-agent
 * network read from a table that cm3_actor_checkers_pack builds with the forward pass's own code.  `traj` as for
 * cm3_checkers_rollout (slot 0 of the observation arrays = the caller's current observation is NOT read: the live state is);
 * actions_prev0: optional int32 [E][N], actions_prev of tick 0 (NULL = zeros, train_onpolicy.py:295); later ticks use the actions just
 * taken, zeros after a tick that ended an episode under CM3_FLAG_AUTO_RESET; actions_prev_next: optional int32 [E][N] output, the
 * actions_prev of the NEXT rollout's first tick (a different buffer); probs: optional float [n_ticks][E][N][5] with
 * probs_stride BYTES between ticks; epsilon_dev: optional device float read at launch instead of actor->epsilon.
 * One or two agents (config_checkers_stage1 / stage2; actor->stage = n_agents), reference geometry, 4-byte padded records.
 * Every output equals, bit for bit, what n_ticks x (cm3_actor_checkers_f32, cm3_checkers_step) write. */
int cm3_policy_rollout_checkers(const cm3_checkers_desc *desc, const cm3_checkers_traj *traj, const cm3_actor_checkers_desc *actor,
                                const cm3_actor_checkers_weights *weights, const int32_t *actions_prev0, int32_t *actions_prev_next, float *probs,
                                size_t probs_stride, const float *epsilon_dev, const cm3_checkers_bufs *final_obs,
                                int32_t n_ticks, void *stream);

/* The same rollout driven by the Checkers QMIX agent (part of ABI 9, additive): per tick networks.Qmix_single_checkers (precision 2),
 * argmax Q + the epsilon-greedy choice of cm3_qmix_checkers_f32, and Checkers.step -- the QMIX collection loop of
 * train_offpolicy.py:309-368 without leaving the kernel.  Arguments as for cm3_policy_rollout_checkers, with these differences:
 * `agent` is validated like cm3_qmix_checkers_f32's descriptor (agent->stage is not read); weights->packed comes from
 * cm3_qmix_checkers_pack, which for one or two agents also builds the others-branch table (N = 1: a row per cell of the agent
 * itself, what the env's obs_others holds there); n_agents 1 or 2; precision 2 only -- precision 0 stays on alternating
 * cm3_qmix_checkers_f32 / cm3_checkers_step launches; agent and env must share seed and env_id_base; q_values: optional float
 * [n_ticks][E][N][5], the raw Q values, q_stride BYTES between ticks.  Every output equals, bit for bit, what n_ticks x
 * (cm3_qmix_checkers_f32, cm3_checkers_step) write.  cm3_last_kernel_variant() names it k_ck_policy_rollout_qmix. */
int cm3_policy_rollout_checkers_qmix(const cm3_checkers_desc *desc, const cm3_checkers_traj *traj, const cm3_actor_checkers_desc *agent,
                                     const cm3_actor_checkers_weights *weights, const int32_t *actions_prev0, int32_t *actions_prev_next,
                                     float *q_values, size_t q_stride, const float *epsilon_dev, const cm3_checkers_bufs *final_obs,
                                     int32_t n_ticks, void *stream);

/* ------------------------------------------------------------------------------------------
 * Advantage normalisation (build-defined; the reference's advantage, alg_credit.py:334-357, is not normalised).
 * Discounted return-to-go over a time-major trajectory, G[t] = x[t] + gamma * (1 - done[t]) * G[t+1], G[T] = 0:
 *   x, out  real [T][E][C]   (C = N for reward_n, 1 for the team reward); out may alias x
 *   done    uint8 [T][E];  valid uint8 [T][E] optional (invalid entries: out = 0, excluded from the moments)
 *   scratch >= cm3_returns_scratch_bytes() bytes, ZERO-INITIALISED ONCE by the caller (per-block partials + an arrival
 *   counter; the last block to arrive folds the partials in block order and resets the counter for the
 *   next call on the same stream -- no memset launch per call);
 *   moments double[3] = (sum, sum of squares, count) of this rank's valid returns, computed deterministically.
 *   The host all-gathers the three numbers over the ranks (RCCL); cm3_normalize_* sums the n_parts triples in rank order
 *   and applies x = (x - (real)mean) / (real)(std + eps) with the GLOBAL moments (x real [n_elem], n_elem a multiple of C,
 *   valid indexed by element / C; the same expression as the host helper cm3_amd.shard.normalize_advantages, bit for bit);
 *   stats (optional) receives (mean, std, count); apply = 0 only computes stats.
 * ---------------------------------------------------------------------------------------- */
size_t cm3_returns_scratch_bytes(void);
/* NOTE (scratch layout): cm3_returns_moments_* keeps its arrival ticket BEHIND 3 * 1024 partial slots of `scratch`;
 * cm3_returns_normalize_segments_* with n_segments >= 2 uses that range for partials.  Give the two entry-point families SEPARATE
 * scratch buffers (cm3_returns_scratch_bytes / cm3_returns_segments_scratch_bytes): a shared one leaves a garbage ticket and the
 * moments silently stale. */
int cm3_returns_moments_f32(const void *x, const uint8_t *done, const uint8_t *valid, void *out, void *scratch,
                            double *moments, int32_t T, int32_t E, int32_t C, double gamma, void *stream);
int cm3_returns_moments_f64(const void *x, const uint8_t *done, const uint8_t *valid, void *out, void *scratch,
                            double *moments, int32_t T, int32_t E, int32_t C, double gamma, void *stream);
int cm3_normalize_f32(void *x, const uint8_t *valid, const double *parts, int32_t n_parts, double *stats, size_t n_elem,
                      int32_t C, double eps, int32_t apply, void *stream);
int cm3_normalize_f64(void *x, const uint8_t *valid, const double *parts, int32_t n_parts, double *stats, size_t n_elem,
                      int32_t C, double eps, int32_t apply, void *stream);
/* ONE rank's whole advantage step (the all-gather is the identity) as TWO launches: cm3_returns_moments_* + cm3_normalize_* with
 * n_parts = 1 on its own moments, bit for bit.  Launch A computes the returns and per-block partial moments (short trajectories,
 * T <= 40: the whole column in one memory round trip), launch B folds the partials in block order in every block -- the fold of
 * cm3_returns_moments_*, so `moments` receives the same bits -- and normalises; no atomics, no arrival counter.
 * cm3_last_kernel_variant() then names launch A's build (k_returns_partials_keep: T <= 40 and <= 1024 column blocks, else
 * k_returns_partials) with N = its number of partial blocks.
 * `shift` (optional) adds the slot bookkeeping of the rollout whose rewards these are to launch A, element by element:
 * first_dst[r] <- mid[r], then mid[r] <- last_src[r] (r < n <= 4; 16-byte aligned pointers and sizes).  With mid = the env's live
 * buffers, first_dst = slot 0 and last_src = slot T of a trajectory whose first tick READ the live buffers, this records the
 * initial state into slot 0 and leaves the final state in the live buffers (train_onpolicy.py:340-343 "state = next_state" across
 * rollouts) without launches of its own: a 33-tick rollout is a chain of dependent launches of ~2.6 us each, and its tail was four. */
typedef struct cm3_copy_shift {
  int32_t n;
  int32_t _pad;
  void *first_dst[4];
  void *mid[4];
  const void *last_src[4];
  size_t bytes[4];
} cm3_copy_shift;
int cm3_returns_normalize_f32(const void *x, const uint8_t *done, const uint8_t *valid, void *out, void *scratch,
                              double *moments, double *stats, int32_t T, int32_t E, int32_t C, double gamma, double eps,
                              int32_t apply, const cm3_copy_shift *shift, void *stream);
int cm3_returns_normalize_f64(const void *x, const uint8_t *done, const uint8_t *valid, void *out, void *scratch,
                              double *moments, double *stats, int32_t T, int32_t E, int32_t C, double gamma, double eps,
                              int32_t apply, const cm3_copy_shift *shift, void *stream);
/* The same two launches for n_segments consecutive rollouts of ONE collection phase (ABI 5; train_onpolicy.py:359: episodes_per_train
 * rollouts between two training steps): x / out are time-major over n_segments * T ticks, done / valid likewise; segment k = ticks
 * [k T, (k + 1) T) has its own returns (G = 0 beyond its last tick), moments[k][3] and stats[k][3] and is normalised with its own
 * statistics -- bit for bit what n_segments calls of cm3_returns_normalize_* on the slices give.  A phase of K rollouts is then ONE
 * chain of K T step launches + 2, and one hipGraph replay, instead of K chains of T + 2 and K replay boundaries.
 * scratch >= cm3_returns_segments_scratch_bytes(n_segments); `shift` is applied once (by segment 0's blocks).
 * apply = 0 leaves the raw returns in `out` and only fills moments / stats: the multi-rank form, followed by ONE all-gather of every
 * rank's moments[n_segments][3] and cm3_normalize_segments_* with parts = [n_parts ranks][n_segments][3]. */
size_t cm3_returns_segments_scratch_bytes(int32_t n_segments);
int cm3_returns_normalize_segments_f32(const void *x, const uint8_t *done, const uint8_t *valid, void *out, void *scratch,
                                       double *moments, double *stats, int32_t T, int32_t n_segments, int32_t E, int32_t C,
                                       double gamma, double eps, int32_t apply, const cm3_copy_shift *shift, void *stream);
int cm3_returns_normalize_segments_f64(const void *x, const uint8_t *done, const uint8_t *valid, void *out, void *scratch,
                                       double *moments, double *stats, int32_t T, int32_t n_segments, int32_t E, int32_t C,
                                       double gamma, double eps, int32_t apply, const cm3_copy_shift *shift, void *stream);
/* x: n_segments slabs of n_elem elements; parts [n_parts][n_segments][3]; stats (optional) [n_segments][3]. */
int cm3_normalize_segments_f32(void *x, const uint8_t *valid, const double *parts, int32_t n_parts, int32_t n_segments, double *stats,
                               size_t n_elem, int32_t C, double eps, int32_t apply, void *stream);
int cm3_normalize_segments_f64(void *x, const uint8_t *valid, const double *parts, int32_t n_parts, int32_t n_segments, double *stats,
                               size_t n_elem, int32_t C, double eps, int32_t apply, void *stream);
/* Up to 8 device-to-device copies (16-byte aligned pointers and sizes) in ONE launch: trajectory slot <-> live env buffers
 * of the collection loop (train_onpolicy.py:340-343 "state = next_state" across rollouts). */
int cm3_copy_list(int32_t n, void *const *dst, const void *const *src, const size_t *bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Transition export and replay rings as single launches (ABI 6)
 * ---------------------------------------------------------------------------------------- */
/* The nine distinct columns of the reference's 11-field particle transition (alg/train_onpolicy.py:338; v_global == v_local ==
 * state, alg_credit.py:458-470), each contiguous over the B gathered transitions. */
typedef struct cm3_transition_cols {
  void *state;            /* float [B][N][4]            global_state / local_self */
  void *obs_others;       /* float [B][N][4 max(N-1,1)] */
  int32_t *actions;       /* int32 [B][N] */
  void *reward;           /* float [B] */
  void *reward_n;         /* float [B][N] */
  void *next_state;       /* float [B][N][4]   slot t + 1, or the captured terminal state where the env restarted in that launch */
  void *next_obs_others;  /* float [B][N][L]   likewise */
  uint8_t *done;          /* uint8 [B] */
  void *goals;            /* float [B][N][2] */
  int64_t ring_start;     /* ring_size > 0: the columns are REPLAY RINGS of ring_size rows and transition b is written to row */
  int64_t ring_size;      /* (ring_start + b) mod ring_size -- export and replay_buffer.add in one launch; 0: row b */
} cm3_transition_cols;
/* The 16 columns of the reference's Checkers transition (alg/train_onpolicy.py:336, consumed by alg_credit_checkers.process_batch,
 * alg_credit_checkers.py:427-444), each contiguous over the B gathered transitions and 16-byte aligned (obs_self_t at odd N: 8).
 * The reference keeps every observation as float64: the int8 / int32 records of the trajectory are converted (exactly) on the way.
 * R = n_rows, C = n_columns, K = 2 n_obs + 1, Lo = 2 max(N-1, 1).  Field order = CheckersRollout.ORDER.
 * (An untagged struct: tests/test_abi.py enumerates the tagged ones against a fixed list; the layout of this one is checked by
 * tests/test_checkers_export_abi.py the same way.) */
typedef struct {
  double *grid;             /* [B][R][C+1][2]   from int8, padding bytes of a strided record skipped */
  double *vec;              /* [B][N][4]        from int32 */
  double *obs_others;       /* [B][N][Lo] */
  double *obs_self_t;       /* [B][N][K][K][3]  from int8 */
  double *obs_self_v;       /* [B][N][4] */
  int32_t *actions_prev;    /* [B][N]   t = 0: prev0[e]; else actions[t-1][e], zeros where the trajectory has terminal capture and
                                        done[t-1][e] (a fresh episode starts from zeros, train_onpolicy.py:295,345) */
  int32_t *actions;         /* [B][N] */
  double *reward;           /* [B] */
  double *local_rewards;    /* [B][N] */
  double *next_grid;        /* next_*: slot t + 1, or term_*[t] where the trajectory has terminal capture and done[t][e] */
  double *next_vec;
  double *next_obs_others;
  double *next_obs_self_t;
  double *next_obs_self_v;
  uint8_t *done;            /* [B]  0 / 1 (a torch.bool column) */
  int64_t *goals;           /* [B][N][2] one-hot of the goal byte: goals_slots[t][e][n] where the trajectory records goal slots,
                                         else the live goals[e][n] */
  int64_t ring_start;       /* ring_size > 0: the columns are REPLAY RINGS of ring_size rows and transition b is written to row */
  int64_t ring_size;        /* (ring_start + b) mod ring_size -- export and replay_buffer.add in one launch; 0: row b */
} cm3_checkers_transition_cols;
/* INDEX CONTRACT of cm3_rows_scatter / cm3_rows_gather / cm3_transitions_gather_f32 / cm3_checkers_transitions_gather: row indices
 * (dst_row, src_row, tt, ee) are
 * NOT bounds-checked by the launches -- an index outside its array is an out-of-bounds device access.  The host classes that call
 * them (cm3_amd/replay.py RingIndex, rollout.py) derive every index from sizes they own; a caller of the C ABI must do the same.
 * n == 0 (or zero rows) returns CM3_OK without touching any pointer. */
/* Gathers transitions (tt[b], ee[b]), b < n, out of a time-major trajectory (the cm3_particle_traj the collector wrote: state
 * [T+1][N][E][4], obs_others [T+1][E][N][L], actions / reward_n [T][E][N], reward / done [T][E], optional term_* [T][...]) in ONE
 * launch.  goals: traj->goals with goals_stride bytes per slot (stride 0: one live array); goal_slot (optional, int32 with
 * goal_slot_stride bytes per tick, [T+1][E]) names the slot that holds the goals in effect at (t, e) -- sparse goal slots; NULL:
 * slot t itself.  tt == ee == NULL: ALL transitions of ticks [0, n / E) in time-major order (b = t E + e).  desc supplies n_envs /
 * n_agents only.  Replaces alg/replay_buffer.py's list-of-arrays + np.stack(batch[:, k]). */
int cm3_transitions_gather_f32(const cm3_particle_desc *desc, const cm3_particle_traj *traj, const int32_t *goal_slot,
                               size_t goal_slot_stride, const int64_t *tt, const int64_t *ee, int64_t n,
                               const cm3_transition_cols *out, void *stream);
/* The same for Checkers (additive in ABI 9): transitions (tt[b], ee[b]), b < n -- or, with tt == ee == NULL, ALL transitions of
 * ticks [0, n / E) in time-major order (b = t E + e) -- out of the cm3_checkers_traj the collector wrote, into the 16 columns of
 * `out`, in ONE launch.  prev0: int32 [E][N], the actions_prev of slot 0.  desc supplies n_envs, n_agents, the geometry and the two
 * record strides; any geometry and agent count cm3_checkers_step accepts, padded or unpadded records.  Every value is a copy or an
 * exact integer -> double conversion.  Validation precedes the launch: null desc / traj / out, tt without ee, n < 0, a ring that
 * does not hold n rows, a missing column are CM3_ERR_INVALID; n == 0 returns CM3_OK without touching a pointer. */
int cm3_checkers_transitions_gather(const cm3_checkers_desc *desc, const cm3_checkers_traj *traj, const int32_t *prev0,
                                    const int64_t *tt, const int64_t *ee, int64_t n, const cm3_checkers_transition_cols *out,
                                    void *stream);

/* The COMPACT Checkers replay ring (additive in ABI 9): the same 16 columns, each with the dtype the trajectory keeps and DENSE rows
 * (no padding) -- 707 B per transition at the reference geometry with N = 2 instead of the 3657 B of cm3_checkers_transition_cols.
 * Field order = CheckersRollout.ORDER.  Every column holds ring_size rows and is 16-byte aligned.  (Untagged, as the struct above;
 * its layout is checked by tests/test_checkers_compact_abi.py.) */
typedef struct {
  int8_t *grid;             /* [ring_size][R][C+1][2] */
  int32_t *vec;             /* [ring_size][N][4] */
  double *obs_others;       /* [ring_size][N][Lo] */
  int8_t *obs_self_t;       /* [ring_size][N][K][K][3] */
  double *obs_self_v;       /* [ring_size][N][4] */
  int32_t *actions_prev;    /* [ring_size][N]  final values: prev0 / zeros behind a done already applied */
  int32_t *actions;         /* [ring_size][N] */
  double *reward;           /* [ring_size] */
  double *local_rewards;    /* [ring_size][N] */
  int8_t *next_grid;
  int32_t *next_vec;
  double *next_obs_others;
  int8_t *next_obs_self_t;
  double *next_obs_self_v;
  uint8_t *done;            /* [ring_size]  0 / 1 */
  uint8_t *goals;           /* [ring_size][N]  the goal INDEX; the one-hot pair is made by cm3_checkers_ring_expand */
  int64_t ring_start;       /* cm3_checkers_transitions_pack writes transition b to row (ring_start + b) mod ring_size */
  int64_t ring_size;        /* rows of every column, >= 1 */
} cm3_checkers_compact_cols;
/* ALL transitions of ticks [0, n / E) of a continuous-collection trajectory, time-major (b = t E + e), into rows (ring_start + b) mod
 * ring_size of the compact columns, in ONE launch that converts nothing.  Same semantics as cm3_checkers_transitions_gather with
 * tt == ee == NULL: next_* from the term_* slot where done[t][e], actions_prev = prev0 at t = 0 and zeros behind a done under terminal
 * capture, goals from goals_slots[t] where recorded; padded and unpadded records, any record stride.  Validation precedes the launch
 * (CM3_ERR_INVALID): null desc / traj / out, n < 0, ring_start / ring_size out of range, n > ring_size, a missing or misaligned column
 * (by name), n_agents outside 1..8, record strides; n == 0 returns CM3_OK without touching a pointer. */
int cm3_checkers_transitions_pack(const cm3_checkers_desc *desc, const cm3_checkers_traj *traj, const int32_t *prev0, int64_t n,
                                  const cm3_checkers_compact_cols *out, void *stream);
/* Row b < n of the 16 reference columns of `out` (float64 / int32 / bool / int64 one-hot, as cm3_checkers_transitions_gather writes
 * them) from compact ring row index[b] (int64 on the device, NOT bounds-checked: see the index contract above); index == NULL: rows
 * 0 .. n - 1.  ONE launch of the export kernel with a ring row as its source; every conversion is exact.  desc supplies n_agents
 * and the geometry.  The same validation as above, for both column sets. */
int cm3_checkers_ring_expand(const cm3_checkers_desc *desc, const cm3_checkers_compact_cols *ring, const int64_t *index, int64_t n,
                             const cm3_checkers_transition_cols *out, void *stream);

/* Up to 16 columns of row-major records (row_bytes[k] bytes per row of column k), moved together. */
typedef struct cm3_row_cols {
  int32_t n_cols;
  int32_t reserved;
  void *dst[16];
  const void *src[16];
  uint32_t row_bytes[16];
} cm3_row_cols;
/* dst[k][row(b)] = src[k][b] for b < n_rows, every column in ONE launch.  row(b) = dst_row[b] when dst_row is given (a negative
 * entry skips the row: the two rings of replay_buffer_dual.py:12-38 take the same batch with complementary index arrays), else the
 * ring position (ring_start + b) mod ring_size (replay_buffer.py:11-16: overwrite the oldest; n_rows <= ring_size). */
int cm3_rows_scatter(const cm3_row_cols *cols, int64_t n_rows, const int64_t *dst_row, int64_t ring_start, int64_t ring_size,
                     void *stream);
/* dst[k][b] = src[k][src_row[b]] (replay_buffer.py:28-37 sample_batch: the sampled transitions as contiguous columns). */
int cm3_rows_gather(const cm3_row_cols *cols, int64_t n_rows, const int64_t *src_row, void *stream);
/* Index width of the data-movement kernels that exist in two: cm3_rows_scatter / cm3_rows_gather, cm3_rows_tile,
 * cm3_checkers_transitions_gather / cm3_checkers_ring_expand, cm3_checkers_transitions_pack, cm3_transitions_gather_f32 /
 * cm3_transitions_route_f32.  Each launcher takes 32-bit unit arithmetic while every index a lane forms stays below 2^32 (the rules:
 * csrc/rows_index_width.h), else its 64-bit build.  bits = 64: every such launch takes the 64-bit build whatever its size (tests run
 * the wide instantiations at small shapes; results are identical, the launch is slower); bits = 0, the initial value: the rule
 * decides.  Anything else is CM3_ERR_INVALID -- 32 on purpose: a narrow build above its limit would write out of range.
 * Process-wide (one relaxed atomic load per launch). */
int cm3_rows_force_index_width(int32_t bits);
/* 32 or 64: what the most recent of those launches of THIS thread took; 0 before any.  (Not part of cm3_last_kernel_variant(), which
 * these launchers leave alone.) */
int cm3_rows_last_index_width(void);

/* ------------------------------------------------------------------------------------------
 * Whole episodes into the dual replay buffer (additive in ABI 9; replay_buffer_dual.py:13-37 fed as train_onpolicy.py:300-356 feeds it)
 * ---------------------------------------------------------------------------------------- */
/* A collection of n_ticks ticks over n_envs envs.  Episodes are ordered by (end tick, env index) -- the order in which a host walking
 * `for t: for e:` meets the done bytes.  The episode that ends at (t, e) is added whole and oldest first, the transitions an earlier
 * call left in the PENDING STORE in front of this call's, to ring 0 (bad) when collisions[t][e] != 0, else to ring 1 (good); every
 * transition is one sequential add: row (ring_idx + rank) mod ring_size, rank counted over all adds of the call to that ring, and a
 * rank below counts - ring_size is skipped (the call itself overwrites it).  synchronous == 0 (continuous collection): the
 * transitions behind an env's last done wait in the pending store (row k * n_envs + e for transition k of the running episode) and
 * pend_len[e] counts them.  synchronous != 0: only transitions with valid[t][e] != 0 exist, an episode still open at the last tick
 * ends there with collisions[n_ticks - 1][e], nothing pends (pend_len, flush_row and pending_depth may be NULL / 0).
 * (Untagged, as the column structs above; its layout is checked by tests/test_episode_route_abi.py.) */
typedef struct {
  const uint8_t *done;          /* uint8 [n_ticks][n_envs], done_stride bytes per tick */
  const int32_t *collisions;    /* int32 [n_ticks][n_envs], collisions_stride bytes per tick */
  const uint8_t *valid;         /* optional uint8 [n_ticks][n_envs], valid_stride bytes per tick; NULL: every transition exists */
  size_t done_stride, collisions_stride, valid_stride;
  int32_t n_ticks, n_envs;
  int32_t pending_depth;        /* P: rows per env of the pending store; the caller keeps it >= the longest episode (max_steps) --
                                   a running episode that outgrows it is NOT kept whole: pend_len saturates at P, the newest
                                   transitions of the tail take rows P - 1 downwards and the older ones are dropped (sel 255);
                                   no row >= P is ever named */
  int32_t synchronous;
  int64_t ring_idx[2];          /* [0] the bad ring, [1] the good ring: where its next add goes */
  int64_t ring_size[2];
} cm3_episode_route_desc;
#define CM3_ROUTE_BAD 0         /* values of sel */
#define CM3_ROUTE_GOOD 1
#define CM3_ROUTE_PENDING 2
#define CM3_ROUTE_SKIP 255      /* no such transition (valid == 0), or the call itself overwrites it */
/* Bytes of device scratch cm3_episode_route_plan needs (8-byte aligned); 0 for a shape it refuses. */
size_t cm3_episode_route_scratch_bytes(int32_t n_ticks, int32_t n_envs);
/* The routing plan, on the device, in five fixed-shape launches (no host read, no atomics, no workgroup waits for another):
 *   sel uint8 [T E], row int64 [T E]   transition b = t E + e goes to row[b] of column set sel[b] (ring 0, ring 1, the pending store)
 *   flush_row int64 [2][P E]           pending row k E + e goes to flush_row[c][k E + e] of ring c; -1: it stays, or is overwritten
 *   counts int64 [2]                   sequential adds per ring, pending prefixes included: what the caller advances its rings by
 *   pend_in / pend_out int32 [E]       transitions of each env's running episode in the pending store before / after (may alias)
 * CM3_ERR_INVALID: null desc / done / collisions / outputs, a shape with (n_ticks + pending_depth) * n_envs >= 2^31, strides smaller
 * than a row, ring_idx outside [0, ring_size), scratch too small.  Enqueue the two flushes (cm3_rows_scatter with flush_row[c]) BEFORE
 * cm3_transitions_route_f32: the export may overwrite pending rows of an env whose next episode starts in this chunk. */
int cm3_episode_route_plan(const cm3_episode_route_desc *desc, const int32_t *pend_in, int32_t *pend_out, uint8_t *sel, int64_t *row,
                           int64_t *flush_row, int64_t *counts, void *scratch, size_t scratch_bytes, void *stream);
/* The same plan computed sequentially on the host from HOST arrays (the one arithmetic, csrc/episode_route.h): same validation, same
 * outputs element for element. */
int cm3_episode_route_plan_host(const cm3_episode_route_desc *desc, const int32_t *pend_in, int32_t *pend_out, uint8_t *sel,
                                int64_t *row, int64_t *flush_row, int64_t *counts);
/* cm3_transitions_gather_f32 with tt == ee == NULL (ALL transitions of ticks [0, n / E), b = t E + e, sparse goal slots included),
 * routed: ONE launch reads every transition once and writes it to row row[b] of sets[sel[b]]; sel[b] == CM3_ROUTE_SKIP (or any value
 * >= n_sets) writes nothing.  sets: n_sets (1..3) column sets, ring_start / ring_size unused.  row is NOT bounds-checked (the index
 * contract above): the caller derives it from sizes it owns, cm3_episode_route_plan does. */
int cm3_transitions_route_f32(const cm3_particle_desc *desc, const cm3_particle_traj *traj, const int32_t *goal_slot,
                              size_t goal_slot_stride, int64_t n, const uint8_t *sel, const int64_t *row,
                              const cm3_transition_cols *sets, int32_t n_sets, void *stream);

/* Tiling of per-agent rows into the feeds of the reference's train_step (ABI 6): process_actions / process_global_state
 * (alg/alg_credit.py:406-443, :528-557), the n x n credit repeats (:614-658) and the n x n x l_action counterfactual tiling
 * (:730-751).  Every output column is "destination row r <- source row f(r)":
 *   others_n == 0:  f(r) = ((r / div[0]) % mod[0]) * mul[0] + ((r / div[1]) % mod[1]) * mul[1]      (mod 0 = no remainder taken)
 *   others_n == N:  f(r) = (r / others_divq) * N + j,  j = k + (k >= n),  k = r % (N - 1),  n = (r / others_divn) % N
 *                   (the reference's `x[:, np.arange(N) != n]` selections, whatever repeats sit around them)
 * and what is written per element depends on `kind`.  Up to 16 columns in ONE launch.  CM3_TILE_COPY columns with rows of at least
 * 64 bytes in whole 8-byte units, between 16-byte aligned dst and src, are moved row by row (a group of lanes per row, f(r) once per
 * row, 16-byte units; 8-byte units where the row size is no multiple of 16: the Checkers feeds, 432 and 600 bytes per row); every
 * other column element by element.  Same results either way. */
#define CM3_TILE_COPY 0         /* elements of elem_bytes (1, 4, 8) copied */
#define CM3_TILE_F32_TO_F64 1   /* float -> double (the reference's float64 np.zeros targets) */
#define CM3_TILE_ONEHOT_I64 2   /* source rows are ONE int32 each; destination rows elems_per_row int64: 1 at the value's index */
#define CM3_TILE_ONEHOT_F64 3   /* ... as double */
#define CM3_TILE_EYE_F64 4      /* np.tile(np.eye(elems_per_row)): row r has its 1.0 at r % elems_per_row (src unused) */
#define CM3_TILE_NOT_I64 5      /* int64 1 - (byte != 0):  -(done.astype(int) - 1), alg_credit.py:590 */
typedef struct cm3_tile_col {
  void *dst;
  const void *src;
  int64_t n_rows;           /* destination rows */
  uint32_t elems_per_row;   /* destination (= source, except the one-hot / eye kinds) elements per row */
  uint32_t kind;            /* CM3_TILE_* */
  uint32_t elem_bytes;      /* CM3_TILE_COPY only */
  uint32_t others_n, others_divq, others_divn;
  uint32_t div[2], mod[2], mul[2];
} cm3_tile_col;
int cm3_rows_tile(const cm3_tile_col *cols, int32_t n_cols, void *stream);
/* out[i] = (double)reward[i] + (gamma * q[i]) * (double)multiplier[i]  (ABI 7): the TD targets of the reference's train_step
 * (alg_credit.py:594, :640, :684: reward + gamma * Q_target * done_multiplier), NumPy's evaluation order, no contraction.
 * reward float32 (reward_is_f64 = 0) or float64 [n], q float64 [n], multiplier int64 [n] (0 / 1), out float64 [n]. */
int cm3_td_target_f64(const void *reward, int32_t reward_is_f64, const double *q, const int64_t *multiplier, double gamma, double *out,
                      int64_t n, void *stream);
/* out[b] = sum_i reward_local[b][i] + (gamma * q_tot[b]) * (1 - done[b])  (part of ABI 9, additive): the TD target of the QMIX
 * train_step (alg_qmix.py:367-369), in the order and types NumPy evaluates it with.  The row sum runs in float64 after widening: left
 * to right for n_agents < 8, NumPy's eight-accumulator tree over the first 8 values and then the rest one by one from 8 on.
 * gamma * q_tot is computed in the type of q_tot (float32: q_is_f64 = 0, gamma rounded to float32 first -- what a TF session's
 * float32 result gives; float64: q_is_f64 = 1), widened to float64, multiplied by 1 - done (done: one byte per transition, 0 / 1)
 * and added.  reward_local float32 (reward_is_f64 = 0) or float64 [n][n_agents], out float64 [n].  One launch, no atomics.
 * CM3_ERR_INVALID: n < 0, n_agents outside 1..10, a null pointer with n > 0. */
int cm3_qmix_td_target_f64(const void *reward_local, int32_t reward_is_f64, int32_t n_agents, const void *q_tot, int32_t q_is_f64,
                           const uint8_t *done, double gamma, double *out, int64_t n, void *stream);

/* ------------------------------------------------------------------------------------------
 * Measurement and launch plumbing
 * ---------------------------------------------------------------------------------------- */
/* Launch-structure floor probe: `blocks` x `threads` lanes read read_bytes (16-byte vectors, all loads first), then write
 * write_bytes whose value depends on what was read -- the load -> store skeleton of a step launch with no arithmetic. */
int cm3_traffic_floor_bench(const void *src, size_t read_bytes, void *dst, size_t write_bytes, int32_t blocks,
                            int32_t threads, void *stream);
/* Streaming 16-byte-per-lane read of `bytes` bytes (multiple of 16); writes one checksum word per
 * workgroup to sink (>= 4*cm3_hbm_bench_sink_words() bytes).  The measured read-bandwidth roofline. */
int cm3_hbm_read_bench(const void *buf, size_t bytes, void *sink, void *stream);
int cm3_hbm_bench_sink_words(void);
/* The same probe with an explicit configuration (independent 16-byte loads in flight per lane: 1/2/4/8/16; workgroups of
 * 256 lanes per CU: 1..32; nt != 0: non-temporal loads) -- tools/hbm_probe_sweep.py picks cm3_hbm_read_bench's. */
int cm3_hbm_read_bench_cfg(const void *buf, size_t bytes, void *sink, int32_t unroll, int32_t wg_per_cu, int32_t nt,
                           void *stream);
/* Streaming 16-byte-per-lane copy of `bytes` bytes (the pattern behind the guide's 6.29 TB/s "float4 copy" figure);
 * the bandwidth is 2 * bytes / time.  unroll 1/2/4/8. */
int cm3_hbm_copy_bench(void *dst, const void *src, size_t bytes, void *stream);
int cm3_hbm_copy_bench_cfg(void *dst, const void *src, size_t bytes, int32_t unroll, int32_t wg_per_cu, int32_t nt,
                           void *stream);

/* hipGraph capture of whatever is enqueued on `stream` between begin and end (launch-bound inner
 * loops: 33 ticks per replay). */
int cm3_graph_begin(void *stream);
int cm3_graph_end(void *stream, void **graph_exec);
int cm3_graph_launch(void *graph_exec, void *stream);
int cm3_graph_destroy(void *graph_exec);

/* HIP events on the caller's stream (bench.py times the kernel on the stream it is launched on). */
int cm3_event_create(void **event);
int cm3_event_record(void *event, void *stream);
int cm3_event_synchronize(void *event);
int cm3_event_elapsed_ms(void *start, void *stop, float *ms);
int cm3_event_destroy(void *event);
int cm3_stream_synchronize(void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CM3_AMD_H */
