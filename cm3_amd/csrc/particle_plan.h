// Which build of the particle step kernels one launch runs, as a pure function of a handful of integers.  Plain C++17, no HIP:
// tests/test_particle_step_plan.py compiles this header alone and walks it on a machine without a GPU.
//   StepShape            what a launch looks like from outside
//   plan_step()          the one place that decides: mapping, waves per workgroup, store policy, live / record / early, translation
//                        unit, grid -- or why the launch is refused
//   step_variant_exists  the set of template instantiations the library contains; particle.hip instantiates exactly these
// The measurements behind the numbers, round by round: DESIGN.md section 4.2c.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/cm3_amd.h"
#include "xcd_grid.h"

namespace cm3 {

constexpr uint32_t kFlagObsStoreNt = 0x100000u;   // internal launch flag, set by particle_rollout only: the observation slots are a stream
constexpr int kSpPlain = 0, kSpNt = 1, kSpWt = 2;  // store policy of the observation rows (what each is for: particle.hip, store_obs_vec)
enum StepMap : int { kMapEnv = 0, kMapPairs = 1, kMapAgents = 2, kMapAgents2 = 3 };   // lane per env / per pair / per agent / two lanes per agent

struct StepShape {
  int real_bytes;     // 4 / 8
  int n_agents;
  int E, E0, EN;      // extent of the env axis of the arrays; the launch covers envs [E0, EN)
  int n_ticks;        // > 1: the tick loop runs inside one launch
  uint32_t flags;     // CM3_FLAG_* of the descriptor | kFlagObsStoreNt
  bool slot_copy;     // ParticleParams.state_copy != nullptr (cm3_particle_traj.state_live)
  bool live_record;   // ParticleParams.live_record != nullptr
};

struct StepPlan {
  int map;            // StepMap
  int waves;          // per workgroup
  int fused, sp, live, rec, early;   // the template arguments beside (real, N, waves)
  int ilp;            // 1: the build of the max-ILP translation unit
  unsigned raw_blocks, grid_blocks;  // workgroups the batch needs; launched (cm3_xcd_grid)
  uint32_t xcd_flags;                // or-ed into the kernel's leading `flags` argument (cm3_xcd_flags)
};

enum StepRefusal : int {
  kPlanOk = 0,
  kRefuseAgentCount,        // n_agents outside 1..CM3_MAX_AGENTS
  kRefusePairAgents,        // lane per pair with n_agents outside 2..8 (N (N - 1) pair lanes must fit a wave)
  kRefuseAgentAgents,       // lane per agent with n_agents < 2
  kRefusePair4GiB,          // the shared-env kernels index with 32-bit byte offsets: obs_others of one tick stays below 4 GiB
  kRefuseAgent4GiB,
  kRefuseRecordMapping,     // live record, and the launch does not go to the lane-per-pair kernel
  kRefuseRecordConditions,  // live record outside per-tick float32 live-state launches with in-kernel actions, n_agents 2..4
};

// ---- geometry of the mappings as functions of n ------------------------------------------------------------------
// (PairGeom / AgentGeom / ObsGeom of particle.hip take their values from these)
constexpr int pow2ceil(int v) {
  int r = 1;
  while (r < v) r <<= 1;
  return r;
}
// lane per pair: lanes per agent = its n - 1 pair lanes, padded to a power of two where that keeps the group size (n = 3, 4, 5)
constexpr int pair_lanes_per_agent(int n) { return (n >= 3 && n <= 5) ? (n == 3 ? 2 : 4) : n - 1; }
constexpr int pair_group_lanes(int n) { return pow2ceil(n * pair_lanes_per_agent(n)); }
constexpr int pair_envs_per_wave(int n) { return 64 / pair_group_lanes(n); }       // (n <= 8)
constexpr int agent_envs_per_wave(int n) { return 64 / pow2ceil(n); }
constexpr int kAgents2EnvsPerWave = 4;                                              // n = 8, two lanes per agent
// reals of obs_others per env: lane per env (n == 1 stores self) and the shared-env mappings (n >= 2)
constexpr int env_obs_reals(int n) { return n * (n > 1 ? n - 1 : 1) * 4; }
constexpr int shared_obs_reals(int n) { return n * (n - 1) * 4; }
constexpr uint32_t kRecBytes = 128;   // one packed live record (layout: particle.hip, kRec*)

// ---- the crossover table ---------------------------------------------------------------------------------------
// Per agent count 1..10: lane per pair up to pair_max envs, lane per agent from agent_lo to agent_hi, lane per env elsewhere.
constexpr size_t kNever = ~(size_t)0;
struct Crossover { size_t pair_max, agent_lo, agent_hi; };
//   pair_max: profiles/r02_mapping_sweep_final_build.txt, r02_mapping_sweep_after_path_shortening.txt (0 for n > 8: no pair mapping)
//   agent_lo: profiles/r03_mapping_sweep_xcd.txt, r03_xcd_block_order.txt (n = 9, 10: r04_mapping_sweep.txt)
//   agent_hi: profiles/r03_mapping_sweep_large.txt (n = 4, 5: r02_mapping_sweep_after_path_shortening.txt)
constexpr Crossover kCrossover[CM3_MAX_AGENTS] = {
    {0, kNever, 0},        {32768, kNever, 0},     {24576, kNever, 0},    {12288, 12289, 40960},  {16384, 10240, 40960},
    {16384, 8192, 1572864}, {16384, 6144, 786432}, {16384, 4096, 786432}, {0, 1024, 786432},      {0, 1024, 786432}};
static_assert(CM3_MAX_AGENTS == 10, "one row per agent count");
constexpr size_t kIlpMaxWaves = 16384;        // max-ILP unit up to this many waves per launch (profiles/r02_sched_strategy_max_ilp.txt)
constexpr int kSharedEnvWaves = 4;            // waves per workgroup of the shared-env mappings ... (profiles/r02_f32_softplus_hw.txt, g.)
constexpr size_t kSharedEnvOneWaveBelow = 256;   // ... from this many waves per launch; below, single-wave workgroups reach more CUs
constexpr size_t kEnvOneWaveMaxEnvs = (size_t)128 * 1024;   // lane per env: one wave per workgroup up to here, 4 above (11.27 vs 11.43 us at 2^17, N = 4)
constexpr int kEnvWaves = 4;
constexpr size_t kWtMinObsBytes = (size_t)3 << 20;   // write-through rows from this many bytes per launch (profiles/r03_obs_store_write_through.txt)
constexpr size_t kAgents2MaxEnvs = 32768;            // n = 8: two lanes per agent up to here (profiles/r03_two_lanes_per_agent.txt) ...
constexpr size_t kAgents2EarlyMaxEnvs = 16384;       // ... with its write-through stores ahead of the reward work up to here (r03_early_wt_stores.txt)
constexpr size_t k4GiB = (size_t)1 << 32;

// what a packed live record needs of a launch beside the lane-per-pair mapping
inline bool record_fits(const StepShape &s) {
  return s.real_bytes == 4 && s.n_agents >= 2 && s.n_agents <= 4 && s.slot_copy && s.n_ticks == 1 && (s.flags & CM3_FLAG_GEN_ACTIONS) &&
         (size_t)s.E * kRecBytes < k4GiB;
}

// The flags, the grid and the refusals of one launch whose mapping and waves per workgroup are given (plan_step below chooses them;
// the probes under tools/probes fix them).  kMapAgents becomes kMapAgents2 where that build applies.
inline int plan_launch(const StepShape &s, int map, int waves, StepPlan &pl) {
  const int n = s.n_agents;
  const size_t E = (size_t)s.E, envs = (size_t)(s.EN - s.E0), rb = (size_t)s.real_bytes;
  const bool f32 = s.real_bytes == 4, nt = f32 && (s.flags & kFlagObsStoreNt), fused = s.n_ticks > 1, copy = s.slot_copy;
  bool wt = false;
  size_t envs_per_wave = 64;
  pl = StepPlan{map, waves, fused, kSpPlain, map != kMapEnv && !fused && copy, 0, 0, 0, 0u, 0u, 0u};   // (lane per env: live is no template argument)
  if (map == kMapEnv) {
    wt = f32 && envs * env_obs_reals(n) * rb >= kWtMinObsBytes && !copy;   // lane per env: not beside a slot copy
  } else if (map == kMapPairs) {
    if (n < 2 || n > 8) return kRefusePairAgents;
    if (E * shared_obs_reals(n) * rb >= k4GiB) return kRefusePair4GiB;
    if (s.live_record && !record_fits(s)) return kRefuseRecordConditions;
    envs_per_wave = pair_envs_per_wave(n);
    pl.rec = s.live_record;   // lane per pair: no write-through build
  } else {
    if (n < 2) return kRefuseAgentAgents;
    if (E * shared_obs_reals(n) * rb >= k4GiB) return kRefuseAgent4GiB;
    wt = f32 && envs * shared_obs_reals(n) * rb >= kWtMinObsBytes;        // lane per agent: a slot copy does not stop it
    envs_per_wave = agent_envs_per_wave(n);
    if (n == 8 && f32 && !fused && envs <= kAgents2MaxEnvs) {
      pl.map = kMapAgents2;
      envs_per_wave = kAgents2EnvsPerWave;
      pl.early = wt && envs <= kAgents2EarlyMaxEnvs;
    }
  }
  pl.sp = !fused && wt ? kSpWt : (nt ? kSpNt : kSpPlain);   // write-through: per-tick launches only
  const size_t per_block = (size_t)waves * envs_per_wave;
  pl.raw_blocks = (unsigned)((envs + per_block - 1) / per_block);
  pl.grid_blocks = map == kMapEnv ? pl.raw_blocks : cm3_xcd_grid(pl.raw_blocks);   // XCD-aware block order: the shared-env kernels
  pl.xcd_flags = map == kMapEnv ? 0u : cm3_xcd_flags(pl.raw_blocks);
  return kPlanOk;
}

// waves per workgroup and translation unit of a shared-env launch: both gates count the waves of the whole ARRAY (E, not EN - E0)
inline int plan_shared(const StepShape &s, int map, StepPlan &pl) {
  const size_t envs_per_wave = map == kMapPairs ? pair_envs_per_wave(s.n_agents) : agent_envs_per_wave(s.n_agents);
  const size_t waves = ((size_t)s.E + envs_per_wave - 1) / envs_per_wave;
  const int rc = plan_launch(s, map, waves < kSharedEnvOneWaveBelow ? 1 : kSharedEnvWaves, pl);
  pl.ilp = s.real_bytes == 4 && waves <= kIlpMaxWaves;
  return rc;
}

// The build one step launch runs, or why it is refused (StepRefusal; the checks in the order the callers have always seen them).
inline int plan_step(const StepShape &s, StepPlan &pl) {
  const int n = s.n_agents;
  if (n < 1 || n > CM3_MAX_AGENTS) return kRefuseAgentCount;
  const Crossover &x = kCrossover[n - 1];
  const size_t E = (size_t)s.E;
  bool pairs = n >= 2 && E <= x.pair_max;
  bool agents = n >= 4 && E >= x.agent_lo && E <= x.agent_hi;
  // beyond 4 GiB of obs_others per tick only a forced choice reaches the shared-env mappings (and is refused by plan_launch)
  if (E * shared_obs_reals(n) * (size_t)s.real_bytes >= k4GiB) pairs = agents = false;
  if (s.flags & CM3_FLAG_KERNEL_LANE_PER_ENV) pairs = agents = false;
  if (s.flags & CM3_FLAG_KERNEL_LANE_PER_PAIR) { pairs = true; agents = false; }
  if (n > 8 && pairs) return kRefusePairAgents;
  if (s.flags & CM3_FLAG_KERNEL_LANE_PER_AGENT) agents = true;
  if (s.live_record && (agents || !pairs)) return kRefuseRecordMapping;
  if (agents) return plan_shared(s, kMapAgents, pl);   // (n = 1 reaches the two only when forced: refused by plan_launch)
  if (pairs) return plan_shared(s, kMapPairs, pl);
  return plan_launch(s, kMapEnv, E <= kEnvOneWaveMaxEnvs ? 1 : kEnvWaves, pl);
}

// Do the per-tick launches of a rollout of this shape (slot copy and record present) step on the record?  Where plan_step plans them
// -- and where a forced pair mapping beyond 4 GiB is the ONLY obstacle: such a call has always got as far as the launch that names
// the limit.  (plan_launch tests the limit before the record, as the launcher always has, so the record is asked about again here.)
inline bool plan_takes_record(const StepShape &s) {
  StepPlan pl;
  const int why = plan_step(s, pl);
  return why == kPlanOk || (why == kRefusePair4GiB && record_fits(s));
}

// The instantiations of the step kernels the library contains -- exactly what plan_step can ask for.
constexpr bool step_variant_exists(int map, int real_bytes, int n, int waves, bool fused, int sp, bool live, bool rec, bool early) {
  const bool f32 = real_bytes == 4;
  if (!f32 && real_bytes != 8) return false;
  if (waves != 1 && waves != 4) return false;
  if (sp != kSpPlain && !(f32 && (sp == kSpNt || sp == kSpWt))) return false;   // nt and wt: float32 only
  if (fused && (live || sp == kSpWt)) return false;                              // the tick loop: no slot copies, no write-through
  if (rec && !(map == kMapPairs && f32 && n <= 4 && live)) return false;         // (live excludes fused)
  if (early && !(map == kMapAgents2 && sp == kSpWt)) return false;
  switch (map) {
    case kMapEnv: return n >= 1 && n <= CM3_MAX_AGENTS && !live;                 // (a slot copy is not a template argument there)
    case kMapPairs: return n >= 2 && n <= 8 && sp != kSpWt;
    case kMapAgents: return n >= 2 && n <= CM3_MAX_AGENTS;
    case kMapAgents2: return f32 && n == 8 && !fused;
  }
  return false;
}

}  // namespace cm3
