// Data movement of the rows SURVEY.md section 8(f2) / (f4) as single launches (round 5):
//   cm3_transitions_gather_f32   every column of the reference's 11-field transition (alg/train_onpolicy.py:338, consumed by
//                                alg_credit.process_batch, alg_credit.py:458-470) for a list of (tick, env) pairs, straight out of the
//                                time-major trajectory: next_* = slot t + 1 or the captured terminal values where the env restarted
//                                in the same launch, goals from the slot that last wrote them (sparse goal slots) -- ONE launch
//                                instead of the ~25 indexing / where launches of the torch composition;
//   cm3_rows_scatter             the columns of a batch of transitions into ring positions (replay_buffer.py:11-16 `add`, and the
//                                dual buffer's two rings, replay_buffer_dual.py:12-38) -- all columns in one launch;
//   cm3_rows_gather              the columns of sampled transitions out of a ring (replay_buffer.py:28-37) -- all columns in one launch.
// Pure byte movement: HBM-bound, no arithmetic, no matrix cores.  A wave copies whole rows with 16-byte (or 8- / 4- / 1-byte, by the
// row size) units, consecutive lanes on consecutive units, so that the side with contiguous rows is fully coalesced.
#include <atomic>

#include "common.h"
#include "rows_index_width.h"

namespace cm3 {

constexpr int kMaxRowCols = 16;

// The index width of the five kernels that exist in two (rows_index_width.h).  cm3_rows_force_index_width(64) sends every launch to the
// wide build (tests: the wide instantiations at small shapes); each launcher records what it chose for cm3_rows_last_index_width().
// A thread-local of its own: cm3_last_kernel_variant() must not change across calls that export.
static std::atomic<int> g_rows_force_bits{0};       // 0: the rule decides; 64: wide
static thread_local int t_rows_last_bits = 0;
static bool rows_forced_wide() { return g_rows_force_bits.load(std::memory_order_relaxed) == 64; }
static bool rows_take_narrow(bool rule_narrow) {
  const bool narrow = rule_narrow && !rows_forced_wide();
  t_rows_last_bits = narrow ? 32 : 64;
  return narrow;
}

struct RowCols {
  int n;
  void *dst[kMaxRowCols];
  const void *src[kMaxRowCols];
  uint32_t row_bytes[kMaxRowCols];
  uint32_t unit[kMaxRowCols];   // bytes per lane: 16, 8, 4 or 1 (largest that divides the row size and both base addresses)
};

// (I = uint32_t whenever the unit count fits: a 64-bit division per unit costs more than the copy)
template <typename U, typename I> __device__ __forceinline__ void copy_units(void *dst, const void *src, size_t n_rows, uint32_t units_per_row,
                                                                             const int64_t *dst_row, const int64_t *src_row,
                                                                             int64_t ring_start, int64_t ring_size) {
  const I total = (I)(n_rows * units_per_row), stride = (I)((size_t)gridDim.x * blockDim.x);
  for (I g = (I)((size_t)blockIdx.x * blockDim.x + threadIdx.x); g < total; g += stride) {
    const I b = g / (I)units_per_row;
    const uint32_t u = (uint32_t)(g - b * (I)units_per_row);
    int64_t d = (int64_t)b, s = (int64_t)b;
    if (dst_row) {
      d = dst_row[b];
    } else if (ring_size > 0) {
      d = ring_start + (int64_t)b;
      d = d >= ring_size ? d - ring_size : d;
    }
    if (src_row) s = src_row[b];
    if (d < 0 || s < 0) continue;     // (a negative row index = skip: how the dual buffer's two rings share one flag pass)
    reinterpret_cast<U *>(dst)[(size_t)d * units_per_row + u] = reinterpret_cast<const U *>(src)[(size_t)s * units_per_row + u];
  }
}

template <typename I> __global__ void __launch_bounds__(256) k_rows_copy(const RowCols c, size_t n_rows, const int64_t *dst_row,
                                                                         const int64_t *src_row, int64_t ring_start, int64_t ring_size) {
  const int col = blockIdx.y;
  const uint32_t unit = c.unit[col], upr = c.row_bytes[col] / unit;
  if (unit == 16)
    copy_units<uint4, I>(c.dst[col], c.src[col], n_rows, upr, dst_row, src_row, ring_start, ring_size);
  else if (unit == 8)
    copy_units<uint2, I>(c.dst[col], c.src[col], n_rows, upr, dst_row, src_row, ring_start, ring_size);
  else if (unit == 4)
    copy_units<uint32_t, I>(c.dst[col], c.src[col], n_rows, upr, dst_row, src_row, ring_start, ring_size);
  else
    copy_units<uint8_t, I>(c.dst[col], c.src[col], n_rows, upr, dst_row, src_row, ring_start, ring_size);
}

static int rows_copy(const cm3_row_cols *cols, int64_t n_rows, const int64_t *dst_row, const int64_t *src_row, int64_t ring_start,
                     int64_t ring_size, hipStream_t s) {
  CM3_REQUIRE(cols && cols->n_cols >= 1 && cols->n_cols <= kMaxRowCols, "row columns: 1..%d columns", kMaxRowCols);
  CM3_REQUIRE(n_rows >= 0, "n_rows must be >= 0");
  if (n_rows == 0) return CM3_OK;
  RowCols c;
  memset(&c, 0, sizeof(c));
  c.n = cols->n_cols;
  size_t most = 0;
  for (int k = 0; k < c.n; ++k) {
    CM3_REQUIRE(cols->dst[k] && cols->src[k] && cols->row_bytes[k] > 0, "row columns: column %d is null / empty", k);
    c.dst[k] = cols->dst[k];
    c.src[k] = cols->src[k];
    c.row_bytes[k] = cols->row_bytes[k];
    const uintptr_t a = (uintptr_t)cols->dst[k] | (uintptr_t)cols->src[k] | (uintptr_t)cols->row_bytes[k];
    c.unit[k] = (a % 16 == 0) ? 16u : (a % 8 == 0) ? 8u : (a % 4 == 0) ? 4u : 1u;
    const size_t units = (size_t)n_rows * (c.row_bytes[k] / c.unit[k]);
    most = units > most ? units : most;
  }
  const size_t blocks = rows_copy_blocks(most);
  if (rows_take_narrow(rows_stride_index_narrow(most, blocks)))
    hipLaunchKernelGGL(k_rows_copy<uint32_t>, dim3((unsigned)blocks, (unsigned)c.n), dim3(256), 0, s, c, (size_t)n_rows, dst_row, src_row,
                       ring_start, ring_size);
  else
    hipLaunchKernelGGL(k_rows_copy<size_t>, dim3((unsigned)blocks, (unsigned)c.n), dim3(256), 0, s, c, (size_t)n_rows, dst_row, src_row,
                       ring_start, ring_size);
  CM3_HIP_CHECK(hipGetLastError());
  return CM3_OK;
}

// ---- the reference's transition, gathered from the trajectory ---------------------------------------------------------------------
struct TransParams {
  const float *state, *obs, *reward_n, *reward, *term_state, *term_obs, *goals;
  const int32_t *actions, *goal_slot;
  const uint8_t *done;
  size_t st_state, st_obs, st_actions, st_reward_n, st_reward, st_done, st_term_state, st_term_obs, st_goals, st_goal_slot;   // bytes per tick
  const int64_t *tt, *ee;
  float *o_state, *o_obs, *o_reward_n, *o_reward, *o_next_state, *o_next_obs, *o_goals;
  int32_t *o_actions;
  uint8_t *o_done;
  size_t n, E;
  size_t ring_start, ring_size;   // ring_size > 0: transition b goes to output row (ring_start + b) mod ring_size (a replay ring), else to row b
  int N, L;
  static constexpr bool kRouted = false;
};
// The ROUTED whole-trajectory export (cm3_transitions_route_f32): transition b goes to row row[b] of column set sel[b] -- the two rings
// and the pending store of the dual replay buffer -- or nowhere (sel[b] >= n_sets).  A second parameter struct, so that the plain
// export keeps its kernel arguments, and with them its instruction stream, as they were.
struct TransOut {
  float *state, *obs, *reward_n, *reward, *next_state, *next_obs, *goals;
  int32_t *actions;
  uint8_t *done;
};
struct RouteParams : TransParams {
  const uint8_t *sel;
  const int64_t *row;
  TransOut set[3];
  uint32_t n_sets;
  static constexpr const int64_t *tt = nullptr, *ee = nullptr;   // (hides TransParams': the routed export is a whole-trajectory one)
  static constexpr bool kRouted = true;
};

template <typename T> __device__ __forceinline__ const T *tick_of(const T *base, size_t stride, int64_t t) {
  return reinterpret_cast<const T *>(reinterpret_cast<const char *>(base) + stride * (size_t)t);
}

// A lane per (transition, unit): unit u of transition b's record is
//   [0, N)                state row of agent u          16 B      state[t][u][e]            -> o_state[b][u]
//   [N, 2N)               next state                    16 B      done ? term_state[t] : state[t + 1]
//   [2N, 2N + NV)         obs_others, NV = N L / 4      16 B      obs[t][e][...]            -> o_obs[b][...]   (contiguous both sides)
//   [.., + NV)            next obs_others               16 B      done ? term_obs[t] : obs[t + 1]
//   then N goal pairs (8 B), N actions, N local rewards (4 B), the reward (4 B) and done (1 B)
// (round 5, first form: a wave per transition looping over its units -- 46 of 64 lanes busy at N = 4 and one dependent chain of
// index -> done -> data loads per wave at a time: 1.23 ms for the 1.35 M transitions of a C2 phase, hardly faster than the torch
// composition; flattened, every lane has its own chain in flight)
// (second form: each lane carries FOUR units at once -- their `done` bytes are requested together, then their data, then the stores:
// a unit is two dependent memory round trips, and with one unit per lane in flight the export ran at 2 TB/s)
struct TransUnit {
  const void *src;
  const void *alt;   // next_* units under terminal capture: the source when the env restarted at this tick (needs the done byte); else NULL
  void *dst;
  int bytes;   // 16, 8, 4, 1 (the done byte: written from the value already loaded), 0 (nothing: past the end)
};
// u.dst: `plain` (the launch's one output column) as the plain export always computed it -- the statement the routed build discards
// is the only one the plain build sees, which keeps its instruction stream -- or `routed`, from the column of the set the
// transition's sel byte s names
#define CM3_TRANS_DST(plain, routed) \
  do { if constexpr (P::kRouted) u.dst = (routed); else u.dst = (plain); } while (0)
#define CM3_TRANS_SET(field) (s == 0u ? p.set[0].field : s == 1u ? p.set[1].field : p.set[2].field)
template <typename P> __device__ __forceinline__ TransUnit trans_unit(const P &p, size_t b_in, int v, int64_t t, size_t e, int N, int NV,
                                                                      uint32_t s = 0u) {
  TransUnit u;
  u.alt = nullptr;
  size_t b = b_in;                // output row (routed: row[b] already)
  if constexpr (!P::kRouted) {
    if (p.ring_size) {
      b = p.ring_start + b_in;
      b = b >= p.ring_size ? b - p.ring_size : b;
    }
  }
  if (v < 2 * N) {
    const bool nxt = v >= N;
    const int i = nxt ? v - N : v;
    const float *src = nxt ? tick_of(p.state, p.st_state, t + 1) : tick_of(p.state, p.st_state, t);
    u.src = reinterpret_cast<const float4 *>(src) + ((size_t)i * p.E + e);
    if (nxt && p.term_state) u.alt = reinterpret_cast<const float4 *>(tick_of(p.term_state, p.st_term_state, t)) + ((size_t)i * p.E + e);
    CM3_TRANS_DST(reinterpret_cast<float4 *>(nxt ? p.o_next_state : p.o_state) + (b * N + i),
                  reinterpret_cast<float4 *>(nxt ? CM3_TRANS_SET(next_state) : CM3_TRANS_SET(state)) + (b * N + i));
    u.bytes = 16;
    return u;
  }
  v -= 2 * N;
  if (v < 2 * NV) {
    const bool nxt = v >= NV;
    const int k = nxt ? v - NV : v;
    const float *src = nxt ? tick_of(p.obs, p.st_obs, t + 1) : tick_of(p.obs, p.st_obs, t);
    u.src = reinterpret_cast<const float4 *>(src) + (e * NV + k);
    if (nxt && p.term_obs) u.alt = reinterpret_cast<const float4 *>(tick_of(p.term_obs, p.st_term_obs, t)) + (e * NV + k);
    CM3_TRANS_DST(reinterpret_cast<float4 *>(nxt ? p.o_next_obs : p.o_obs) + (b * NV + k),
                  reinterpret_cast<float4 *>(nxt ? CM3_TRANS_SET(next_obs) : CM3_TRANS_SET(obs)) + (b * NV + k));
    u.bytes = 16;
    return u;
  }
  v -= 2 * NV;
  if (v < N) {   // goals [slot][N][E][2]: the slot that last wrote this env's landmarks (goal_slot), or the only one (stride 0)
    const int64_t gs = p.goal_slot ? (int64_t)tick_of(p.goal_slot, p.st_goal_slot, t)[e] : t;
    u.src = reinterpret_cast<const float2 *>(tick_of(p.goals, p.st_goals, gs)) + ((size_t)v * p.E + e);
    CM3_TRANS_DST(reinterpret_cast<float2 *>(p.o_goals) + (b * N + v), reinterpret_cast<float2 *>(CM3_TRANS_SET(goals)) + (b * N + v));
    u.bytes = 8;
    return u;
  }
  v -= N;
  if (v < N) {
    u.src = tick_of(p.actions, p.st_actions, t) + (e * N + v);
    CM3_TRANS_DST(p.o_actions + (b * N + v), CM3_TRANS_SET(actions) + (b * N + v));
    u.bytes = 4;
    return u;
  }
  v -= N;
  if (v < N) {
    u.src = tick_of(p.reward_n, p.st_reward_n, t) + (e * N + v);
    CM3_TRANS_DST(p.o_reward_n + (b * N + v), CM3_TRANS_SET(reward_n) + (b * N + v));
    u.bytes = 4;
    return u;
  }
  v -= N;
  if (v == 0) {
    u.src = tick_of(p.reward, p.st_reward, t) + e;
    CM3_TRANS_DST(p.o_reward + b, CM3_TRANS_SET(reward) + b);
    u.bytes = 4;
    return u;
  }
  u.src = nullptr;
  CM3_TRANS_DST(p.o_done + b, CM3_TRANS_SET(done) + b);
  u.bytes = 1;
  return u;
}
#undef CM3_TRANS_DST
#undef CM3_TRANS_SET

// (WIDE: `small` is a compile-time false -- the 64-bit divisions at any size, launched only under cm3_rows_force_index_width(64))
template <typename P, bool WIDE = false> __global__ void __launch_bounds__(256) k_transitions_gather(const P p) {
  constexpr int K = kTransUnitsPerLane;
  const int N = p.N, NV = N * p.L / 4;
  const uint32_t U = (uint32_t)(2 * N + 2 * NV + 3 * N + 2);
  const size_t total = p.n * U, stride = (size_t)gridDim.x * blockDim.x;
  const bool small = WIDE ? false : trans_index_small(total, stride);
  for (size_t g0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g0 < total; g0 += (size_t)K * stride) {
    size_t bb[K], ee[K];
    int64_t tt[K];
    int vv[K];
    uint8_t dd[K];
    [[maybe_unused]] int64_t rr[K];      // routed: the transition's output row and its column set
    [[maybe_unused]] uint32_t ss[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const size_t g = g0 + (size_t)k * stride, gc = g < total ? g : total - 1;
      size_t b;
      int v;
      if (p.tt) {   // an indexed gather: a transition's units on consecutive lanes
        b = small ? (size_t)((uint32_t)gc / U) : gc / U;
        v = (int)(gc - b * U);
      } else {
        // the whole trajectory in order (b = t E + e): the units whose SOURCE rows lie along the env index -- state, next state and
        // goals are [slot][N][E][..] -- take consecutive lanes on consecutive ENVS (whole lines read; the 16- / 8-byte pieces a
        // lane writes meet their neighbours of the same output line in the L2), the others stay transition-major.  With every
        // lane of a transition reading its own state row the export read 4 lines for 64 bytes of them and ran at 2.4 TB/s.
        const size_t nA = p.n * (size_t)(3 * N);
        if (gc < nA) {
          const size_t c = small ? (size_t)((uint32_t)gc / (uint32_t)p.n) : gc / p.n;
          b = gc - c * p.n;
          v = c < (size_t)(2 * N) ? (int)c : (int)c + 2 * NV;           // goals follow the observation units in the unit order
        } else {
          const size_t g2 = gc - nA;
          const uint32_t UB = (uint32_t)(2 * NV + 2 * N + 2);
          b = small ? (size_t)((uint32_t)g2 / UB) : g2 / UB;
          const int w2 = (int)(g2 - b * UB);
          v = w2 < 2 * NV ? 2 * N + w2 : w2 + 3 * N;                     // (2N + 2NV + N) + (w2 - 2NV)
        }
      }
      bb[k] = b;
      vv[k] = g < total ? v : -1;
      // (tt == NULL: every transition of the trajectory in time-major order, b = t E + e -- no index arrays to build or read)
      tt[k] = p.tt ? p.tt[b] : (int64_t)(small ? (size_t)((uint32_t)b / (uint32_t)p.E) : b / p.E);
      ee[k] = p.tt ? (size_t)p.ee[b] : b - (size_t)tt[k] * p.E;
      if constexpr (P::kRouted) {   // (requested with everything else of the unit: only the STORE waits for them)
        rr[k] = p.row[b];
        ss[k] = p.sel[b];
      }
    }
    TransUnit u[K];
    uint4 val[K];
    // Only the next_* units of a trajectory with terminal capture (and the done column itself) need the env's done byte before
    // their data can be requested: the byte is requested for those alone, every other unit's data in the same round trip
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if constexpr (P::kRouted) {
        u[k] = trans_unit(p, (size_t)rr[k], vv[k] < 0 ? 0 : vv[k], tt[k], ee[k], N, NV, ss[k]);
        if (ss[k] >= p.n_sets) { u[k].bytes = 0; u[k].alt = nullptr; }     // skipped: nothing loaded, nothing stored
      } else {
        u[k] = trans_unit(p, bb[k], vv[k] < 0 ? 0 : vv[k], tt[k], ee[k], N, NV);
      }
      if (vv[k] < 0) u[k].bytes = 0;
      dd[k] = 0;
      if (u[k].alt || u[k].bytes == 1) dd[k] = tick_of(p.done, p.st_done, tt[k])[ee[k]];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      val[k] = uint4{0u, 0u, 0u, 0u};
      if (!u[k].alt) {
        if (u[k].bytes == 16) val[k] = *reinterpret_cast<const uint4 *>(u[k].src);
        else if (u[k].bytes == 8) { const uint2 w = *reinterpret_cast<const uint2 *>(u[k].src); val[k].x = w.x; val[k].y = w.y; }
        else if (u[k].bytes == 4) val[k].x = *reinterpret_cast<const uint32_t *>(u[k].src);
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
      if (u[k].alt) val[k] = *reinterpret_cast<const uint4 *>(dd[k] ? u[k].alt : u[k].src);      // (next state / next observation rows: 16 bytes)
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (u[k].bytes == 16) *reinterpret_cast<uint4 *>(u[k].dst) = val[k];
      else if (u[k].bytes == 8) *reinterpret_cast<uint2 *>(u[k].dst) = uint2{val[k].x, val[k].y};
      else if (u[k].bytes == 4) *reinterpret_cast<uint32_t *>(u[k].dst) = val[k].x;
      else if (u[k].bytes == 1) *reinterpret_cast<uint8_t *>(u[k].dst) = dd[k] ? 1 : 0;
    }
  }
}

// ---- the reference's 16-column Checkers transition, gathered from the trajectory ---------------------------------------------------
// (alg_credit_checkers.py:427-444: float64 throughout, while the trajectory keeps grid / obs_self_t as int8 and vec as int32 -- the
// export EXPANDS: at the reference geometry with N = 2 a transition reads ~0.7 KB and writes 3.65 KB, so the kernel is store-bound.)
// A lane per (transition, output unit), the units of ONE column per workgroup: column c owns the blocks [blk_end[c - 1], blk_end[c])
// and block j of it the units [1024 j, 1024 (j + 1)) of the column in row-major order, unit g = b * units_per_row + u.  Consecutive
// lanes therefore write consecutive 16-byte (8- / 4- / 1-byte) pieces of the column: a wave's store is one contiguous KiB whatever the
// row size (432 B for grid, 1200 B for obs_self_t at N = 2), and because every source is [slot][env][record] the loads of a
// whole-trajectory export are contiguous too.  The column -- and with it the unit kind, the need for the done byte and every table
// entry -- is uniform over the workgroup: scalar loads from the kernel arguments, no per-lane table lookup (which would go through
// scratch) and no divergent kind switch.
// A 16-byte unit of grid / obs_self_t is two doubles made from two source BYTES: one 2-byte load where every record starts on an even
// address (padded records; unpadded ones with an even record size), else two byte loads (75 N-byte records at odd N > 1 -- at N = 1
// the row is 75 doubles, not a multiple of 16 bytes, and the column takes 8-byte units of one source byte each).
// As in k_transitions_gather every lane carries FOUR units: their (tt, ee), then their done bytes, then their data are requested
// together, and only next_* under terminal capture, actions_prev and the done column ask for a done byte at all.
enum CkUnitKind : uint32_t {
  CKU_I8X2,     // 2 int8 -> 2 doubles (16 B)
  CKU_I8,       // 1 int8 -> 1 double (8 B)
  CKU_I32X2,    // 2 int32 -> 2 doubles (16 B)
  CKU_COPY16,
  CKU_COPY8,
  CKU_COPY4,
  CKU_PREV,     // actions_prev: actions[t - 1] (zeros behind a done under terminal capture), prev0 at t = 0 (4 B)
  CKU_DONE,     // done[t][e] != 0 (1 B)
  CKU_GOAL      // goal byte -> int64 one-hot pair (16 B)
};
constexpr int kCkCols = 16;

struct CkCol {
  const char *src;      // slot 0 of the source array
  const char *alt;      // next_* under terminal capture: the term_* array (slot t, taken where done[t][e]); else NULL
  char *dst;
  size_t slot_stride, alt_stride;   // bytes between slots
  uint32_t env_stride;  // bytes between the env records of a slot
  uint32_t upr;         // units per output row
  uint32_t kind;
  uint32_t next;        // 1: the source slot is t + 1
};
struct CkTransParams {
  CkCol col[kCkCols];
  uint32_t blk_end[kCkCols];
  const uint8_t *done;
  const int32_t *prev0;
  const int64_t *tt, *ee;
  size_t st_done;
  size_t n, E;
  size_t ring_start, ring_size;
  int term;             // the trajectory has terminal capture
  int pair16;           // every int8 record starts on an even address
};

__device__ __forceinline__ uint32_t ck_src_bytes(uint32_t kind) {
  return kind == CKU_I8X2 ? 2u : kind == CKU_I8 || kind == CKU_GOAL ? 1u : kind == CKU_COPY16 ? 16u
       : kind == CKU_I32X2 || kind == CKU_COPY8 ? 8u : kind == CKU_DONE ? 0u : 4u;
}
__device__ __host__ __forceinline__ uint32_t ck_dst_bytes(uint32_t kind) {
  return kind == CKU_I8 || kind == CKU_COPY8 ? 8u : kind == CKU_COPY4 || kind == CKU_PREV ? 4u : kind == CKU_DONE ? 1u : 16u;
}

template <typename I> __global__ void __launch_bounds__(256) k_ck_transitions_gather(const CkTransParams p) {
  constexpr int K = kCkUnitsPerLane;
  int c = 0;
  uint32_t first = 0;
#pragma unroll
  for (int k = 0; k < kCkCols - 1; ++k)
    if (blockIdx.x >= p.blk_end[k]) { c = k + 1; first = p.blk_end[k]; }
  const CkCol &C = p.col[c];
  const uint32_t kind = C.kind, upr = C.upr, sb = ck_src_bytes(kind), db = ck_dst_bytes(kind);
  const I total = (I)(p.n * upr);
  const I g0 = (I)(blockIdx.x - first) * (I)(K * 256) + (I)threadIdx.x;
  size_t bb[K], ee[K];
  int64_t tt[K];
  uint32_t uu[K];
  bool live[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const I g = g0 + (I)(k * 256);
    live[k] = g < total;
    const I gc = live[k] ? g : total - 1;      // (lanes past the end repeat the last unit's loads and store nothing)
    const I b = gc / (I)upr;
    uu[k] = (uint32_t)(gc - b * (I)upr);
    bb[k] = (size_t)b;
    if (p.ee) {                                // (ee without tt: slot 0 throughout -- the rows of a compact ring, cm3_checkers_ring_expand)
      tt[k] = p.tt ? p.tt[b] : 0;
      ee[k] = (size_t)p.ee[b];
    } else {                                   // the whole trajectory in time-major order: b = t E + e
      const I t = b / (I)p.E;
      tt[k] = (int64_t)t;
      ee[k] = (size_t)(b - t * (I)p.E);
    }
  }
  uint8_t dd[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    dd[k] = 0;
    if (kind == CKU_PREV) {
      if (p.term && tt[k] > 0) dd[k] = tick_of(p.done, p.st_done, tt[k] - 1)[ee[k]];
    } else if (C.alt || kind == CKU_DONE) {
      dd[k] = tick_of(p.done, p.st_done, tt[k])[ee[k]];
    }
  }
  uint4 val[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const size_t off = ee[k] * C.env_stride + (size_t)uu[k] * sb;
    const char *s;
    if (kind == CKU_PREV)
      s = tt[k] > 0 ? C.src + C.slot_stride * (size_t)(tt[k] - 1) + off : reinterpret_cast<const char *>(p.prev0) + off;
    else if (C.alt && dd[k])
      s = C.alt + C.alt_stride * (size_t)tt[k] + off;
    else
      s = C.src + C.slot_stride * (size_t)(tt[k] + C.next) + off;
    val[k] = uint4{0u, 0u, 0u, 0u};
    if (kind == CKU_COPY16) {
      val[k] = *reinterpret_cast<const uint4 *>(s);
    } else if (kind == CKU_I32X2 || kind == CKU_COPY8) {
      const uint2 w = *reinterpret_cast<const uint2 *>(s);
      val[k].x = w.x;
      val[k].y = w.y;
    } else if (kind == CKU_COPY4 || kind == CKU_PREV) {
      val[k].x = *reinterpret_cast<const uint32_t *>(s);
    } else if (kind == CKU_I8X2) {
      if (p.pair16) {
        val[k].x = *reinterpret_cast<const uint16_t *>(s);
      } else {
        val[k].x = (uint32_t)reinterpret_cast<const uint8_t *>(s)[0] | ((uint32_t)reinterpret_cast<const uint8_t *>(s)[1] << 8);
      }
    } else if (kind != CKU_DONE) {             // CKU_I8, CKU_GOAL
      val[k].x = *reinterpret_cast<const uint8_t *>(s);
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if (!live[k]) continue;
    size_t row = bb[k];
    if (p.ring_size) {
      row += p.ring_start;
      row = row >= p.ring_size ? row - p.ring_size : row;
    }
    char *d = C.dst + (row * upr + uu[k]) * db;
    const uint32_t x = val[k].x;
    if (kind == CKU_I8X2) {
      *reinterpret_cast<double2 *>(d) = double2{(double)(int8_t)(x & 0xffu), (double)(int8_t)(x >> 8)};
    } else if (kind == CKU_I8) {
      *reinterpret_cast<double *>(d) = (double)(int8_t)x;
    } else if (kind == CKU_I32X2) {
      *reinterpret_cast<double2 *>(d) = double2{(double)(int32_t)x, (double)(int32_t)val[k].y};
    } else if (kind == CKU_COPY16) {
      *reinterpret_cast<uint4 *>(d) = val[k];
    } else if (kind == CKU_COPY8) {
      *reinterpret_cast<uint2 *>(d) = uint2{x, val[k].y};
    } else if (kind == CKU_COPY4) {
      *reinterpret_cast<uint32_t *>(d) = x;
    } else if (kind == CKU_PREV) {
      *reinterpret_cast<uint32_t *>(d) = dd[k] ? 0u : x;
    } else if (kind == CKU_DONE) {
      *reinterpret_cast<uint8_t *>(d) = dd[k] ? 1 : 0;
    } else {                                   // CKU_GOAL: one_hot(g, 2) as int64
      *reinterpret_cast<uint4 *>(d) = uint4{x == 0u ? 1u : 0u, 0u, x == 1u ? 1u : 0u, 0u};
    }
  }
}

// ---- the compact Checkers replay ring: the same 16 columns with the dtypes the trajectory keeps ------------------------------------
// (cm3_checkers_transitions_pack: 707 B per transition at the reference geometry with N = 2 instead of the 3657 B of the float64
// columns; nothing is converted -- cm3_checkers_ring_expand widens the rows a learner samples, through k_ck_transitions_gather with a
// ring row as its source.)  Rows are dense: 54-byte grid and 150-byte obs_self_t rows are no multiple of 16 bytes, so a column is
// addressed as ONE flat byte array and a lane owns an aligned 16-byte PIECE of it, whatever rows the piece lies in: consecutive lanes
// store consecutive pieces, a wave's store is one contiguous KiB as in the wide export.  The chunk covers the bytes [lo_a, hi_a) of the
// column and, where it wraps, [0, hi_b); the first and last piece of either range may be partly outside it and are written granule by
// granule, every other piece with one 16-byte store.
// A piece is assembled from GRANULES of `gran` bytes: the largest power of two (<= 16) that divides the row size, every source stride
// and every base address, so that a granule lies in one row and is one naturally aligned load (2 bytes for grid / obs_self_t records
// on even strides, 1 byte on odd ones, 16 for the float64 and vec rows, the row itself for the narrow columns).  Rows of 16 bytes or
// more put at most two rows into a piece: their (tick, env), done bytes and source rows are resolved once per piece, four pieces per
// lane in flight as in k_ck_transitions_gather.  Narrower rows (done, goals, actions, reward: 27 of the 707 bytes) resolve every
// granule on its own.  The column is uniform over the workgroup, as above: no per-lane table lookup, nothing in scratch.
enum PkKind : uint32_t {
  PK_COPY,      // the record bytes as they are (next_*: slot t + 1, or the term_* slot where done[t][e])
  PK_PREV,      // actions_prev: actions[t - 1] (zeros behind a done under terminal capture), prev0 at t = 0
  PK_DONE       // done[t][e] != 0
};

struct PkCol {
  const char *src, *alt;
  char *dst;
  size_t slot_stride, alt_stride;
  size_t lo_a, hi_a, hi_b;   // bytes of the flat column this chunk covers: [lo_a, hi_a), then [0, hi_b) past the wrap
  uint32_t env_stride, rb;   // bytes between the env records of a slot; bytes per ring row
  uint32_t gran, kind, next;
};
struct PkParams {
  PkCol col[kCkCols];
  uint32_t blk_end[kCkCols];
  const uint8_t *done;
  const char *prev0;
  size_t st_done, E, ring_start, ring_size;
  int term;
};

template <int G> __device__ __forceinline__ void pk_fetch(uint32_t (&w)[4], int i, const char *s, bool zero, bool norm) {
  if constexpr (G == 16) {
    const uint4 v = *reinterpret_cast<const uint4 *>(s);
    w[0] = zero ? 0u : v.x; w[1] = zero ? 0u : v.y; w[2] = zero ? 0u : v.z; w[3] = zero ? 0u : v.w;
  } else if constexpr (G == 8) {
    const uint2 v = *reinterpret_cast<const uint2 *>(s);
    w[2 * i] = zero ? 0u : v.x; w[2 * i + 1] = zero ? 0u : v.y;
  } else if constexpr (G == 4) {
    const uint32_t v = *reinterpret_cast<const uint32_t *>(s);
    w[i] = zero ? 0u : v;
  } else if constexpr (G == 2) {
    const uint32_t v = *reinterpret_cast<const uint16_t *>(s);
    w[i / 2] |= (zero ? 0u : v) << (16 * (i & 1));
  } else {
    uint32_t v = *reinterpret_cast<const uint8_t *>(s);
    if (norm) v = v ? 1u : 0u;
    w[i / 4] |= (zero ? 0u : v) << (8 * (i & 3));
  }
}
template <int G> __device__ __forceinline__ void pk_store(char *d, const uint32_t (&w)[4], int i) {   // granule i of the piece at d
  if constexpr (G == 16) *reinterpret_cast<uint4 *>(d) = uint4{w[0], w[1], w[2], w[3]};
  else if constexpr (G == 8) *reinterpret_cast<uint2 *>(d + 8 * i) = uint2{w[2 * i], w[2 * i + 1]};
  else if constexpr (G == 4) *reinterpret_cast<uint32_t *>(d + 4 * i) = w[i];
  else if constexpr (G == 2) *reinterpret_cast<uint16_t *>(d + 2 * i) = (uint16_t)(w[i / 2] >> (16 * (i & 1)));
  else *reinterpret_cast<uint8_t *>(d + i) = (uint8_t)(w[i / 4] >> (8 * (i & 3)));
}
// the done byte a ring row's source depends on (0 where it depends on none), and the source of the row's first byte
__device__ __forceinline__ uint32_t pk_row_done(const PkParams &p, const PkCol &C, size_t t, size_t e) {
  if (C.kind == PK_PREV) return (p.term && t > 0) ? (uint32_t)tick_of(p.done, p.st_done, (int64_t)t - 1)[e] : 0u;
  return C.alt ? (uint32_t)tick_of(p.done, p.st_done, (int64_t)t)[e] : 0u;
}
__device__ __forceinline__ const char *pk_row_src(const PkParams &p, const PkCol &C, size_t t, size_t e, uint32_t d) {
  const size_t off = e * C.env_stride;
  if (C.kind == PK_PREV) return t > 0 ? C.src + C.slot_stride * (t - 1) + off : p.prev0 + off;
  if (C.alt && d) return C.alt + C.alt_stride * t + off;
  return C.src + C.slot_stride * (t + C.next) + off;
}
// piece g of the column -> the range it belongs to ([lo, hi) bytes, `wrapped`: the one past the wrap) and its first byte
template <typename I> __device__ __forceinline__ I pk_piece(const PkCol &C, I g, I nA, I &lo, I &hi, bool &wrapped) {
  wrapped = g >= nA;
  lo = wrapped ? (I)0 : (I)C.lo_a;
  hi = wrapped ? (I)C.hi_b : (I)C.hi_a;
  return (wrapped ? g - nA : (I)(C.lo_a / 16) + g) * (I)16;
}
// ring row -> (tick, env) of the transition it takes
template <typename I> __device__ __forceinline__ void pk_row_te(const PkParams &p, I row, bool wrapped, I &t, I &e) {
  const I b = wrapped ? row + (I)(p.ring_size - p.ring_start) : row - (I)p.ring_start;
  t = b / (I)p.E;
  e = b - t * (I)p.E;
}

template <int G, typename I> __device__ __forceinline__ void pk_wide(const PkParams &p, const PkCol &C, I g0) {   // rows of >= 16 bytes
  // (K pieces in flight per lane: all four where a piece is one or two loads, two where it is eight or sixteen)
  constexpr int K = G >= 8 ? kPkPiecesPerLane : 2, NG = 16 / G;
  const uint32_t rb = C.rb;
  const I nA = (I)((C.hi_a + 15) / 16 - C.lo_a / 16), total = nA + (I)((C.hi_b + 15) / 16);
  const bool prev = C.kind == PK_PREV;
#pragma unroll 1
  for (int k0 = 0; k0 < kPkPiecesPerLane; k0 += K) {
  I first[K], tA[K], eA[K], tB[K], eB[K];
  uint32_t c0[K], c1[K], u0[K], dA[K], dB[K];
  bool live[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const I g = g0 + (I)((k0 + k) * 256);
    live[k] = g < total;
    I lo, hi;
    bool wrapped;
    first[k] = pk_piece<I>(C, live[k] ? g : total - 1, nA, lo, hi, wrapped);      // (lanes past the end repeat the last piece's loads)
    const I start = first[k] > lo ? first[k] : lo, end = first[k] + 16 < hi ? first[k] + 16 : hi;
    c0[k] = (uint32_t)(start - first[k]);      // the bytes [c0, c1) of the piece belong to the chunk
    c1[k] = (uint32_t)(end - first[k]);
    const I row = start / (I)rb;
    u0[k] = (uint32_t)(start - row * (I)rb);
    pk_row_te<I>(p, row, wrapped, tA[k], eA[k]);
    tB[k] = tA[k];
    eB[k] = eA[k];
    if (u0[k] + (c1[k] - c0[k]) > rb) {        // the piece runs on into the next row: the next transition
      eB[k] = eA[k] + 1;
      if (eB[k] == (I)p.E) { eB[k] = 0; tB[k] = tA[k] + 1; }
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    dA[k] = pk_row_done(p, C, tA[k], eA[k]);
    dB[k] = pk_row_done(p, C, tB[k], eB[k]);
  }
  uint32_t w[K][4];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const char *sA = pk_row_src(p, C, tA[k], eA[k], dA[k]), *sB = pk_row_src(p, C, tB[k], eB[k], dB[k]);
    w[k][0] = w[k][1] = w[k][2] = w[k][3] = 0u;
#pragma unroll
    for (int i = 0; i < NG; ++i) {
      const uint32_t at = (uint32_t)(i * G);
      const bool in = at >= c0[k] && at < c1[k];
      const uint32_t pos = in ? u0[k] + at - c0[k] : u0[k];       // (a granule outside the chunk loads the first one inside it)
      const bool second = pos >= rb;
      pk_fetch<G>(w[k], i, second ? sB + (pos - rb) : sA + pos, prev && (second ? dB[k] : dA[k]) != 0u, false);
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if (!live[k]) continue;
    char *d = C.dst + (size_t)first[k];
    if (c0[k] == 0u && c1[k] == 16u) {
      *reinterpret_cast<uint4 *>(d) = uint4{w[k][0], w[k][1], w[k][2], w[k][3]};
    } else {
#pragma unroll
      for (int i = 0; i < NG; ++i)
        if ((uint32_t)(i * G) >= c0[k] && (uint32_t)(i * G) < c1[k]) pk_store<G>(d, w[k], i);
    }
  }
  }
}

template <int G, typename I> __device__ __forceinline__ void pk_narrow(const PkParams &p, const PkCol &C, I g0) {   // rows of < 16 bytes
  constexpr int K = kPkPiecesPerLane, NG = 16 / G;
  const uint32_t rb = C.rb;
  const I nA = (I)((C.hi_a + 15) / 16 - C.lo_a / 16), total = nA + (I)((C.hi_b + 15) / 16);
#pragma unroll 1
  for (int k = 0; k < K; ++k) {
    const I g = g0 + (I)(k * 256);
    if (g >= total) break;
    I lo, hi;
    bool wrapped;
    const I first = pk_piece<I>(C, g, nA, lo, hi, wrapped);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < NG; ++i) {
      const I at = first + (I)(i * G);
      if (at < lo || at >= hi) continue;
      const I row = at / (I)rb;
      I t, e;
      pk_row_te<I>(p, row, wrapped, t, e);
      const uint32_t d = pk_row_done(p, C, t, e);
      pk_fetch<G>(w, i, pk_row_src(p, C, t, e, d) + (uint32_t)(at - row * (I)rb), C.kind == PK_PREV && d != 0u, C.kind == PK_DONE);
    }
    char *dst = C.dst + (size_t)first;
    if (first >= lo && first + 16 <= hi) {
      *reinterpret_cast<uint4 *>(dst) = uint4{w[0], w[1], w[2], w[3]};
    } else {
#pragma unroll
      for (int i = 0; i < NG; ++i)
        if (first + (I)(i * G) >= lo && first + (I)(i * G) < hi) pk_store<G>(dst, w, i);
    }
  }
}

template <typename I> __global__ void __launch_bounds__(256) k_ck_transitions_pack(const PkParams p) {
  int c = 0;
  uint32_t first = 0;
#pragma unroll
  for (int k = 0; k < kCkCols - 1; ++k)
    if (blockIdx.x >= p.blk_end[k]) { c = k + 1; first = p.blk_end[k]; }
  const PkCol &C = p.col[c];
  const I g0 = (I)(blockIdx.x - first) * (I)(kPkPiecesPerLane * 256) + (I)threadIdx.x;
  const uint32_t G = C.gran;
  if (C.rb >= 16u) {
    if (G == 16u) pk_wide<16, I>(p, C, g0);
    else if (G == 8u) pk_wide<8, I>(p, C, g0);
    else if (G == 4u) pk_wide<4, I>(p, C, g0);
    else if (G == 2u) pk_wide<2, I>(p, C, g0);
    else pk_wide<1, I>(p, C, g0);
  } else {
    if (G == 8u) pk_narrow<8, I>(p, C, g0);
    else if (G == 4u) pk_narrow<4, I>(p, C, g0);
    else if (G == 2u) pk_narrow<2, I>(p, C, g0);
    else pk_narrow<1, I>(p, C, g0);
  }
}

// ---- tiling: the n x n credit repeats and the n x n x l_action counterfactual tiling of train_step ------------------------------
// (alg_credit.py:614-658 `np.repeat(np.reshape(x, [n_steps, n, d]), n, axis=0)` / `np.repeat(x, n, axis=0)`; :730-751 the same
// repeated l_action times against np.tile(np.eye(l_action)); process_actions / process_global_state :406-443, :528-557 with their
// `np.arange(N) != n` selections.)  Every output is "destination row r <- source row f(r)", f built from divisions and remainders of
// r; up to 16 outputs per launch.  The Checkers twin (alg_credit_checkers.py:536-780) repeats the same way rows of 432 and 600 bytes
// (state_env, obs_self_t): those take the row-granular path below (tile_rows), narrow rows and the computed kinds the element loop.
struct TileCol {
  void *dst;
  const void *src;
  unsigned long long n_rows;      // destination rows
  uint32_t epr;                   // elements per row
  uint32_t kind;                  // CM3_TILE_*
  uint32_t es;                    // bytes per SOURCE element for CM3_TILE_COPY (1, 4, 8)
  uint32_t div0, mod0, mul0, div1, mod1, mul1;   // source row = ((r / div0) % mod0) * mul0 + ((r / div1) % mod1) * mul1   (mod 0: no remainder)
  uint32_t oth_n, oth_divq, oth_divn;            // oth_n = N > 0: source row = (r / divq) * N + j, j = k + (k >= n), k = r % (N - 1), n = (r / divn) % N
};
struct TileCols {
  int n;
  TileCol c[kMaxRowCols];
};

// source row f(r) of destination row r, as the element loop of k_rows_tile forms it
template <typename I> __device__ __forceinline__ I tile_src_row(const TileCol &c, I r) {
  if (c.oth_n) {
    const uint32_t k = (uint32_t)(r % (I)(c.oth_n - 1)), n = (uint32_t)((r / (I)c.oth_divn) % (I)c.oth_n);
    return (r / (I)c.oth_divq) * (I)c.oth_n + k + (k >= n ? 1u : 0u);
  }
  I q0 = r / (I)c.div0, q1 = r / (I)c.div1;
  if (c.mod0) q0 %= c.mod0;
  if (c.mod1) q1 %= c.mod1;
  return q0 * c.mul0 + q1 * c.mul1;
}

// The row-granular path of CM3_TILE_COPY columns with wide rows (Checkers: state_env 432 B, obs_self_t 600 B, repeated N, N^2 and
// N^2 l_action times): a power-of-two group of lanes serves one destination row, f(r) is formed once per row instead of once per
// 8-byte element, and every lane moves 16-byte units (8-byte ones where the row size is an odd number of 8-byte units: rows then
// alternate between the two alignments).  Taken from kTileRowMinBytes per row, for rows of whole 8-byte units between 16-byte
// aligned views; everything else -- narrower rows, an 8-byte aligned source view, other kinds -- stays on the element path below.
// Block-uniform (blockIdx.y selects the column), plain stores (the networks read the feeds next).  The path lives in a build of the
// kernel of its own, k_rows_tile<I, true>, which the launcher takes when a column of the launch qualifies: a launch without one (every
// particle feed: rows of 16 .. 48 bytes) runs k_rows_tile<I, false>, the element loop alone -- with the row path compiled in, that
// loop's launches were 0.3 us slower (profiles/r21_checkers_phase.txt, 4.).
constexpr uint32_t kTileRowMinBytes = 64;   // row path from this many bytes per row (profiles/r21_checkers_phase.txt, 4.)
// bytes per unit of the row path (16 / 8), 0: the element path
__host__ __device__ __forceinline__ uint32_t tile_row_unit(const TileCol &c) {
  const size_t rb = (size_t)c.epr * c.es;
  if (c.kind != CM3_TILE_COPY || rb < kTileRowMinBytes || rb > 0x7fffffffu || (rb & 7u)) return 0;
  if ((reinterpret_cast<uintptr_t>(c.dst) | reinterpret_cast<uintptr_t>(c.src)) & 15u) return 0;
  return (rb & 15u) ? 8u : 16u;
}
// log2 of the lanes that serve one row of `units` units: about four units per lane (f(r) is then formed once per four units and a
// wave holds several rows), at least one 128-byte line per group and pass, at most one wave
__device__ __forceinline__ uint32_t tile_row_lanes_log2(uint32_t units, uint32_t unit_bytes) {
  const uint32_t line = 128u / unit_bytes, least = units < line ? units : line, want = (units + 3u) / 4u;
  const uint32_t v = want > least ? want : least;
  const uint32_t lg = v <= 1u ? 0u : 32u - (uint32_t)__builtin_clz(v - 1u);
  return lg > 6u ? 6u : lg;
}
template <typename I, typename V> __device__ __forceinline__ void tile_rows(const TileCol &c) {
  const uint32_t rb = c.epr * c.es, units = rb / (uint32_t)sizeof(V), lg = tile_row_lanes_log2(units, (uint32_t)sizeof(V));
  const uint32_t G = 1u << lg, lane = threadIdx.x & (G - 1u);
  const I n_rows = (I)c.n_rows, stride = (I)(((size_t)gridDim.x * 256) >> lg);     // (n_rows <= elements: within the launcher's rule)
  for (I r = (I)(((size_t)blockIdx.x * 256 + threadIdx.x) >> lg); r < n_rows; r += stride) {
    const I s = tile_src_row<I>(c, r);
    const V *sp = reinterpret_cast<const V *>(static_cast<const char *>(c.src) + (size_t)s * rb);
    V *dp = reinterpret_cast<V *>(static_cast<char *>(c.dst) + (size_t)r * rb);
    for (uint32_t u = lane; u < units; u += 4u * G) {       // four loads in flight per lane, then their stores
      const uint32_t u1 = u + G, u2 = u + 2u * G, u3 = u + 3u * G;
      V v0 = sp[u], v1 = v0, v2 = v0, v3 = v0;
      if (u1 < units) v1 = sp[u1];
      if (u2 < units) v2 = sp[u2];
      if (u3 < units) v3 = sp[u3];
      dp[u] = v0;
      if (u1 < units) dp[u1] = v1;
      if (u2 < units) dp[u2] = v2;
      if (u3 < units) dp[u3] = v3;
    }
  }
}

template <typename I, bool ROWS> __global__ void __launch_bounds__(256) k_rows_tile(const TileCols a) {
  const TileCol &c = a.c[blockIdx.y];
  if constexpr (ROWS) {
    const uint32_t row_unit = tile_row_unit(c);
    if (row_unit) {
      if (row_unit == 16u) tile_rows<I, uint4>(c);
      else tile_rows<I, uint2>(c);
      return;
    }
  }
  const I total = (I)((size_t)c.n_rows * c.epr), stride = (I)((size_t)gridDim.x * blockDim.x);
  for (I g = (I)((size_t)blockIdx.x * blockDim.x + threadIdx.x); g < total; g += stride) {
    const I r = g / (I)c.epr;
    const uint32_t e = (uint32_t)(g - r * (I)c.epr);
    I s;
    if (c.oth_n) {
      const uint32_t k = (uint32_t)(r % (I)(c.oth_n - 1)), n = (uint32_t)((r / (I)c.oth_divn) % (I)c.oth_n);
      s = (r / (I)c.oth_divq) * (I)c.oth_n + k + (k >= n ? 1u : 0u);
    } else {
      I q0 = r / (I)c.div0, q1 = r / (I)c.div1;
      if (c.mod0) q0 %= c.mod0;
      if (c.mod1) q1 %= c.mod1;
      s = q0 * c.mul0 + q1 * c.mul1;
    }
    switch (c.kind) {
      case CM3_TILE_COPY:
        if (c.es == 4)
          reinterpret_cast<uint32_t *>(c.dst)[g] = reinterpret_cast<const uint32_t *>(c.src)[s * c.epr + e];
        else if (c.es == 8)
          reinterpret_cast<uint64_t *>(c.dst)[g] = reinterpret_cast<const uint64_t *>(c.src)[s * c.epr + e];
        else
          reinterpret_cast<uint8_t *>(c.dst)[g] = reinterpret_cast<const uint8_t *>(c.src)[s * c.epr + e];
        break;
      case CM3_TILE_F32_TO_F64:
        reinterpret_cast<double *>(c.dst)[g] = (double)reinterpret_cast<const float *>(c.src)[s * c.epr + e];
        break;
      case CM3_TILE_ONEHOT_I64:
        reinterpret_cast<int64_t *>(c.dst)[g] = reinterpret_cast<const int32_t *>(c.src)[s] == (int32_t)e ? 1 : 0;
        break;
      case CM3_TILE_ONEHOT_F64:
        reinterpret_cast<double *>(c.dst)[g] = reinterpret_cast<const int32_t *>(c.src)[s] == (int32_t)e ? 1.0 : 0.0;
        break;
      case CM3_TILE_EYE_F64:
        reinterpret_cast<double *>(c.dst)[g] = (uint32_t)(r % c.epr) == e ? 1.0 : 0.0;
        break;
      default:   // CM3_TILE_NOT_I64: 1 - (byte != 0)   ("if true, then 0, else 1", alg_credit.py:590)
        reinterpret_cast<int64_t *>(c.dst)[g] = reinterpret_cast<const uint8_t *>(c.src)[s * c.epr + e] ? 0 : 1;
        break;
    }
  }
}

// TD target of the reference's train_step (alg_credit.py:594, :640, :684): reward + gamma * Q_target * done_multiplier, evaluated in
// NumPy's order -- (gamma * q) first, times the 0 / 1 multiplier, plus the float64 reward -- with no contraction (the library is built
// with -ffp-contract=off): the same bits as the torch composition in cm3_amd/batch.py, ONE launch instead of four
template <typename R> __global__ void __launch_bounds__(256) k_td_target(const R *reward, const double *q, const int64_t *mult, double gamma,
                                                                         double *out, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const double gq = gamma * q[i];
    out[i] = (double)reward[i] + gq * (double)mult[i];
  }
}

// The QMIX TD target (alg_qmix.py:367-369): np.sum(reward_local.reshape(n, N), axis=1) + gamma * q_tot * (-(done - 1)).  One thread
// per transition.  np.sum over a contiguous last axis of N float64 values: left to right below 8 values, from 8 on the pairwise
// kernel's eight accumulators over the first 8, combined as ((r0+r1)+(r2+r3)) + ((r4+r5)+(r6+r7)), then the tail one by one.
template <typename RR, typename RQ> __global__ void __launch_bounds__(256) k_qmix_td_target(const RR *reward, int N, const RQ *q, const uint8_t *done,
                                                                                             double gamma, double *out, size_t n) {
  for (size_t b = (size_t)blockIdx.x * 256 + threadIdx.x; b < n; b += (size_t)gridDim.x * 256) {
    const RR *r = reward + b * (size_t)N;
    double sum;
    int i;
    if (N < 8) {
      sum = (double)r[0];
      i = 1;
    } else {
      sum = (((double)r[0] + (double)r[1]) + ((double)r[2] + (double)r[3])) + (((double)r[4] + (double)r[5]) + ((double)r[6] + (double)r[7]));
      i = 8;
    }
    for (; i < N; ++i) sum += (double)r[i];
    const RQ gq = (RQ)gamma * q[b];                    // in q's type: float32(gamma) * float32, or float64
    out[b] = sum + (double)gq * (double)(done[b] ? 0 : 1);
  }
}

// ---- host side shared by the Checkers export, the compact ring's pack and its expansion --------------------------------------------
struct CkGeom {
  uint32_t N, Lo, grid_rec, obst_rec, grid_stride, obst_stride;   // record sizes and strides in bytes
};
static int ck_geometry(const cm3_checkers_desc *desc, bool need_envs, CkGeom &g) {
  CM3_REQUIRE(!need_envs || desc->n_envs > 0, "n_envs must be positive");
  CM3_REQUIRE(desc->n_agents >= 1 && desc->n_agents <= 8, "Checkers: n_agents must be in 1..8");
  CM3_REQUIRE(desc->n_rows >= 1 && desc->n_columns >= 2 && desc->n_rows * desc->n_columns <= 64, "n_rows / n_columns out of range");
  CM3_REQUIRE(desc->n_obs >= 0 && desc->n_obs <= 8, "n_obs out of range");
  const uint32_t Kw = 2u * (uint32_t)desc->n_obs + 1u;
  g.N = (uint32_t)desc->n_agents;
  g.Lo = 2u * (g.N > 1 ? g.N - 1 : 1);
  g.grid_rec = (uint32_t)desc->n_rows * (uint32_t)(desc->n_columns + 1) * 2u;
  g.obst_rec = g.N * Kw * Kw * 3u;
  g.grid_stride = desc->grid_stride ? (uint32_t)desc->grid_stride : g.grid_rec;
  g.obst_stride = desc->obs_self_t_stride ? (uint32_t)desc->obs_self_t_stride : g.obst_rec;
  CM3_REQUIRE(desc->grid_stride >= 0 && desc->obs_self_t_stride >= 0 && g.grid_stride >= g.grid_rec && g.obst_stride >= g.obst_rec,
              "record strides smaller than the records");
  return CM3_OK;
}

// what both whole-trajectory readers require of the trajectory: prev0, the base pointers, terminal capture all or none
static int ck_traj_check(const char *entry, const cm3_checkers_traj *traj, const int32_t *prev0, bool &term) {
  CM3_REQUIRE(prev0, "%s: prev0 (actions_prev of slot 0) is required", entry);
  CM3_REQUIRE(traj->actions && traj->grid && traj->vec && traj->obs_others && traj->obs_self_t && traj->obs_self_v &&
                  traj->local_rewards && traj->reward && traj->done && (traj->goals_slots || traj->goals),
              "trajectory base pointers are required");
  const int n_term = (traj->term_grid != nullptr) + (traj->term_vec != nullptr) + (traj->term_obs_others != nullptr) +
                     (traj->term_obs_self_t != nullptr) + (traj->term_obs_self_v != nullptr);
  CM3_REQUIRE(n_term == 0 || n_term == 5, "terminal capture: all five term_* arrays or none");
  term = n_term == 5;
  return CM3_OK;
}

// ---- the 16 columns, ONE table: cm3_checkers_transitions_gather, cm3_checkers_transitions_pack and cm3_checkers_ring_expand all read it --
enum CkRec : uint8_t {   // the record of the trajectory a column carries
  CKR_GRID, CKR_VEC, CKR_OBS_OTHERS, CKR_OBS_SELF_T, CKR_OBS_SELF_V, CKR_ACTIONS, CKR_REWARD, CKR_LOCAL_REWARDS, CKR_DONE, CKR_GOALS
};
// X(field, record, next, prev) in header order.  next: the next_* form (slot t + 1, or the term_* slot behind a done); prev:
// actions_prev, the actions record one tick back.  (done and goals are their own records: the record is their role.)
#define CM3_CK_COLUMNS(X)                                                                                                                 \
  X(grid, CKR_GRID, 0, 0) X(vec, CKR_VEC, 0, 0) X(obs_others, CKR_OBS_OTHERS, 0, 0) X(obs_self_t, CKR_OBS_SELF_T, 0, 0)                   \
  X(obs_self_v, CKR_OBS_SELF_V, 0, 0) X(actions_prev, CKR_ACTIONS, 0, 1) X(actions, CKR_ACTIONS, 0, 0) X(reward, CKR_REWARD, 0, 0)        \
  X(local_rewards, CKR_LOCAL_REWARDS, 0, 0) X(next_grid, CKR_GRID, 1, 0) X(next_vec, CKR_VEC, 1, 0) X(next_obs_others, CKR_OBS_OTHERS, 1, 0) \
  X(next_obs_self_t, CKR_OBS_SELF_T, 1, 0) X(next_obs_self_v, CKR_OBS_SELF_V, 1, 0) X(done, CKR_DONE, 0, 0) X(goals, CKR_GOALS, 0, 0)
struct CkColumn {
  const char *name; CkRec rec; bool next, prev;
  size_t off;           // of the pointer inside cm3_checkers_transition_cols AND cm3_checkers_compact_cols
};
#define X(f, rec, next, prev) {#f, rec, next != 0, prev != 0, offsetof(cm3_checkers_transition_cols, f)},
static const CkColumn kCkColumns[kCkCols] = {CM3_CK_COLUMNS(X)};
#undef X
#define X(f, rec, next, prev) && offsetof(cm3_checkers_compact_cols, f) == offsetof(cm3_checkers_transition_cols, f)
static_assert(sizeof(cm3_checkers_compact_cols) == sizeof(cm3_checkers_transition_cols) CM3_CK_COLUMNS(X) &&
                  offsetof(cm3_checkers_compact_cols, ring_start) == offsetof(cm3_checkers_transition_cols, ring_start) &&
                  offsetof(cm3_checkers_compact_cols, ring_size) == offsetof(cm3_checkers_transition_cols, ring_size),
              "cm3_checkers_compact_cols and cm3_checkers_transition_cols must lay their fields out alike");
#undef X
static void *ck_field(const void *cols, const CkColumn &col) {   // the column's pointer in either struct
  void *p;
  memcpy(&p, static_cast<const char *>(cols) + col.off, sizeof(p));
  return p;
}

// (geometry, record) -> bytes between the env records of a slot, bytes of a dense ring row, the wide export's unit kind and units per row
struct CkRecord { uint32_t env_stride, row_bytes, kind, upr; };
static CkRecord ck_record(const CkGeom &g, CkRec rec) {
  const uint32_t N = g.N;
  switch (rec) {
    case CKR_GRID: return {g.grid_stride, g.grid_rec, CKU_I8X2, g.grid_rec / 2};
    case CKR_VEC: return {16 * N, 16 * N, CKU_I32X2, 2 * N};
    case CKR_OBS_OTHERS: return {8 * N * g.Lo, 8 * N * g.Lo, CKU_COPY16, N * g.Lo / 2};
    case CKR_OBS_SELF_T:   // (a row of 75 N doubles at odd N: 8-byte units)
      return {g.obst_stride, g.obst_rec, (g.obst_rec & 1u) ? CKU_I8 : CKU_I8X2, (g.obst_rec & 1u) ? g.obst_rec : g.obst_rec / 2};
    case CKR_OBS_SELF_V: return {32 * N, 32 * N, CKU_COPY16, 2 * N};
    case CKR_ACTIONS: return {4 * N, 4 * N, CKU_COPY4, N};
    case CKR_REWARD: return {8, 8, CKU_COPY8, 1};
    case CKR_LOCAL_REWARDS: return {8 * N, 8 * N, CKU_COPY8, N};
    case CKR_DONE: return {1, 1, CKU_DONE, 1};
    default: return {N, N, CKU_GOAL, N};   // CKR_GOALS
  }
}

// what a launch needs to know of one column (upr / the CKU_* kinds: the wide export; row_bytes / the PK_* kinds: the pack)
struct CkSpec {
  const char *name; void *dst;
  const void *src, *alt;
  size_t slot_stride, alt_stride;
  uint32_t env_stride, row_bytes, upr, kind, next;
};
// (trajectory, record, next) -> where the export and the pack read a column: slot 0 with its slot stride and, for next_*, the term_*
// array with its own.  Everything else of the spec is the record's; the caller sets the kind where it differs.
static CkSpec ck_traj_spec(const cm3_checkers_traj *t, const CkColumn &col, const CkRecord &r, void *dst) {
  CkSpec s = {col.name, dst, nullptr, nullptr, 0, 0, r.env_stride, r.row_bytes, r.upr, r.kind, col.next ? 1u : 0u};
  auto from = [&](const void *src, size_t stride, const void *alt = nullptr, size_t alt_stride = 0) {
    s.src = src; s.slot_stride = stride;
    if (col.next) { s.alt = alt; s.alt_stride = alt_stride; }
  };
  switch (col.rec) {
    case CKR_GRID: from(t->grid, t->grid_slot_stride, t->term_grid, t->term_grid_slot_stride); break;
    case CKR_VEC: from(t->vec, t->vec_stride, t->term_vec, t->term_vec_stride); break;
    case CKR_OBS_OTHERS: from(t->obs_others, t->obs_others_stride, t->term_obs_others, t->term_obs_others_stride); break;
    case CKR_OBS_SELF_T: from(t->obs_self_t, t->obs_self_t_slot_stride, t->term_obs_self_t, t->term_obs_self_t_slot_stride); break;
    case CKR_OBS_SELF_V: from(t->obs_self_v, t->obs_self_v_stride, t->term_obs_self_v, t->term_obs_self_v_stride); break;
    case CKR_ACTIONS: from(t->actions, t->actions_stride); break;
    case CKR_REWARD: from(t->reward, t->reward_stride); break;
    case CKR_LOCAL_REWARDS: from(t->local_rewards, t->local_rewards_stride); break;
    case CKR_DONE: from(t->done, t->done_stride); break;
    default:   // CKR_GOALS: the slot's goal bytes where the trajectory records them, else the live array (stride 0: every tick the same)
      from(t->goals_slots ? t->goals_slots : t->goals, t->goals_slots ? t->goals_slots_stride : 0);
  }
  return s;
}

// What CkCol and PkCol share, filled from a spec (C = either), behind the check that the column is there ...
template <typename C> static int ck_col_fill(C &c, const CkSpec &s, bool term, const char *cols_what) {
  CM3_REQUIRE(s.dst, "%s: column %s is missing", cols_what, s.name);
  c.src = (const char *)s.src; c.slot_stride = s.slot_stride;
  c.alt = term ? (const char *)s.alt : nullptr; c.alt_stride = c.alt ? s.alt_stride : 0;
  c.dst = (char *)s.dst; c.env_stride = s.env_stride; c.kind = s.kind; c.next = s.next;
  return CM3_OK;
}
// ... and, behind the kernel's own alignment checks, the column's workgroups: `work` units (pieces) at per_block of them each
static int ck_col_blocks(const char *entry, size_t work, size_t per_block, size_t &blocks, uint32_t &blk_end) {
  blocks += (work + per_block - 1) / per_block;
  CM3_REQUIRE(blocks < ((size_t)1 << 31), "%s: too many transitions for one launch", entry);
  blk_end = (uint32_t)blocks;
  return CM3_OK;
}

// the ring a column struct names: one that takes the n rows, or (optional) none -- ring_size 0: transition b goes to row b
static int ring_required(const char *what, int64_t start, int64_t size, int64_t n) {
  CM3_REQUIRE(size >= 1 && start >= 0 && start < size && n <= size,
              "%s: ring_start / ring_size out of range (0 <= ring_start < ring_size, n <= ring_size)", what);
  return CM3_OK;
}
static int ring_optional(const char *what, int64_t start, int64_t size, int64_t n) {
  return size == 0 && start >= 0 ? CM3_OK : ring_required(what, start, size, n);
}

// One k_ck_transitions_gather launch over the 16 columns of `specs`: `cols_what` / `src_what` name the destination and the source in
// the error texts.  check_small_copies: the sources of the 8- / 4-byte copy units are checked for the alignment of their loads too (a
// caller's ring columns; the trajectory export keeps the checks it always had).
static int ck_gather_launch(const char *entry, const char *cols_what, const char *src_what, bool check_small_copies,
                            const CkSpec (&specs)[kCkCols], bool term, const uint8_t *done,
                            size_t st_done, const int32_t *prev0, const int64_t *tt, const int64_t *ee, size_t n, size_t E,
                            int64_t ring_start, int64_t ring_size, hipStream_t stream) {
  CkTransParams p;
  memset(&p, 0, sizeof(p));
  size_t blocks = 0, most = 0;
  bool even = true;
  for (int k = 0; k < kCkCols; ++k) {
    const CkSpec &s = specs[k];
    CkCol &c = p.col[k];
    if (int rc = ck_col_fill(c, s, term, cols_what)) return rc;
    c.upr = s.upr;
    CM3_REQUIRE((uintptr_t)s.dst % ck_dst_bytes(s.kind) == 0, "%s: column %s is not aligned to its %u-byte units", cols_what, s.name,
                ck_dst_bytes(s.kind));
    if (s.kind == CKU_COPY16 || s.kind == CKU_I32X2)
      CM3_REQUIRE(((uintptr_t)c.src | (uintptr_t)c.alt | c.slot_stride | c.alt_stride) % (s.kind == CKU_COPY16 ? 16 : 8) == 0,
                  "%s: %s is not aligned to the loads of its units", src_what, s.name);
    if (check_small_copies && (s.kind == CKU_COPY8 || s.kind == CKU_COPY4))
      CM3_REQUIRE(((uintptr_t)c.src | c.slot_stride) % (s.kind == CKU_COPY8 ? 8 : 4) == 0,
                  "%s: %s is not aligned to the loads of its units", src_what, s.name);
    if (s.kind == CKU_I8X2) even = even && (((uintptr_t)c.src | (uintptr_t)c.alt | c.slot_stride | c.alt_stride | c.env_stride) & 1u) == 0;
    const size_t units = n * s.upr;
    most = units > most ? units : most;
    if (int rc = ck_col_blocks(entry, units, kCkUnitsPerLane * 256, blocks, p.blk_end[k])) return rc;
  }
  p.done = done;
  p.st_done = st_done;
  p.prev0 = prev0;
  p.tt = tt;
  p.ee = ee;
  p.n = n;
  p.E = E;
  p.ring_start = (size_t)ring_start;
  p.ring_size = (size_t)ring_size;
  p.term = term ? 1 : 0;
  p.pair16 = even ? 1 : 0;
  if (rows_take_narrow(ck_gather_index_narrow(most)))     // (32-bit unit arithmetic: a 64-bit division per unit costs more than the copy)
    hipLaunchKernelGGL(k_ck_transitions_gather<uint32_t>, dim3((unsigned)blocks), dim3(256), 0, stream, p);
  else
    hipLaunchKernelGGL(k_ck_transitions_gather<size_t>, dim3((unsigned)blocks), dim3(256), 0, stream, p);
  CM3_HIP_CHECK(hipGetLastError());
  return CM3_OK;
}

// ---- host side shared by cm3_transitions_gather_f32 and cm3_transitions_route_f32 --------------------------------------------------
static int trans_check(const cm3_particle_desc *desc, const cm3_particle_traj *traj) {
  CM3_REQUIRE(desc->n_agents >= 1 && desc->n_agents <= CM3_MAX_AGENTS, "n_agents out of range");
  CM3_REQUIRE(traj->state && traj->obs_others && traj->actions && traj->reward_n && traj->reward && traj->done && traj->goals,
              "trajectory base pointers are required");
  CM3_REQUIRE((traj->term_state == nullptr) == (traj->term_obs_others == nullptr), "term_state and term_obs_others: both or neither");
  return CM3_OK;
}
static void trans_sources(TransParams &p, const cm3_particle_desc *desc, const cm3_particle_traj *traj, const int32_t *goal_slot,
                          size_t goal_slot_stride, int64_t n) {
  p.state = (const float *)traj->state;             p.st_state = traj->state_stride;
  p.obs = (const float *)traj->obs_others;          p.st_obs = traj->obs_others_stride;
  p.actions = traj->actions;                        p.st_actions = traj->actions_stride;
  p.reward_n = (const float *)traj->reward_n;       p.st_reward_n = traj->reward_n_stride;
  p.reward = (const float *)traj->reward;           p.st_reward = traj->reward_stride;
  p.done = traj->done;                              p.st_done = traj->done_stride;
  p.term_state = (const float *)traj->term_state;   p.st_term_state = traj->term_state_stride;
  p.term_obs = (const float *)traj->term_obs_others; p.st_term_obs = traj->term_obs_others_stride;
  p.goals = (const float *)traj->goals;             p.st_goals = traj->goals_stride;
  p.goal_slot = goal_slot;                          p.st_goal_slot = goal_slot_stride;
  p.n = (size_t)n;
  p.E = (size_t)desc->n_envs;
  p.N = desc->n_agents;
  p.L = 4 * (desc->n_agents > 1 ? desc->n_agents - 1 : 1);
}
static size_t trans_units(const TransParams &p) { return p.n * (size_t)(2 * p.N + 2 * (p.N * p.L / 4) + 3 * p.N + 2); }
// One k_transitions_gather launch, four units per lane: the build whose `small` the kernel decides, or the wide one when forced
template <typename P> static void trans_launch(const P &p, hipStream_t stream) {
  const size_t units = trans_units(p), blocks = trans_blocks_for(units);
  if (rows_forced_wide()) {
    rows_take_narrow(false);
    hipLaunchKernelGGL((k_transitions_gather<P, true>), dim3((unsigned)blocks), dim3(256), 0, stream, p);
  } else {
    rows_take_narrow(trans_index_small(units, blocks * kRowsLanes));      // (what every lane of the launch will find)
    hipLaunchKernelGGL((k_transitions_gather<P>), dim3((unsigned)blocks), dim3(256), 0, stream, p);
  }
}

}  // namespace cm3

extern "C" {
int cm3_rows_force_index_width(int32_t bits) {
  using namespace cm3;
  // (32 is refused on purpose: a narrow build above its limit would write out of range)
  CM3_REQUIRE(bits == 0 || bits == 64, "rows_force_index_width: 0 (the rule decides) or 64; got %d", (int)bits);
  g_rows_force_bits.store(bits, std::memory_order_relaxed);
  return CM3_OK;
}

int cm3_rows_last_index_width(void) { return cm3::t_rows_last_bits; }

int cm3_td_target_f64(const void *reward, int32_t reward_is_f64, const double *q, const int64_t *multiplier, double gamma, double *out,
                      int64_t n, void *stream) {
  using namespace cm3;
  CM3_REQUIRE(n >= 0, "n must be >= 0");
  if (n == 0) return CM3_OK;
  CM3_REQUIRE(reward && q && multiplier && out, "td_target: null argument");
  size_t blocks = ((size_t)n + 255) / 256;
  blocks = blocks > 2048 ? 2048 : blocks;
  if (reward_is_f64)
    hipLaunchKernelGGL(k_td_target<double>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const double *)reward, q, multiplier,
                       gamma, out, (size_t)n);
  else
    hipLaunchKernelGGL(k_td_target<float>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const float *)reward, q, multiplier,
                       gamma, out, (size_t)n);
  CM3_HIP_CHECK(hipGetLastError());
  return CM3_OK;
}

int cm3_qmix_td_target_f64(const void *reward_local, int32_t reward_is_f64, int32_t n_agents, const void *q_tot, int32_t q_is_f64,
                           const uint8_t *done, double gamma, double *out, int64_t n, void *stream) {
  using namespace cm3;
  CM3_REQUIRE(n >= 0, "n must be >= 0");
  CM3_REQUIRE(n_agents >= 1 && n_agents <= CM3_MAX_AGENTS, "n_agents must be in 1..%d", CM3_MAX_AGENTS);
  if (n == 0) return CM3_OK;
  CM3_REQUIRE(reward_local && q_tot && done && out, "qmix_td_target: null argument");
  size_t blocks = ((size_t)n + 255) / 256;
  blocks = blocks > 2048 ? 2048 : blocks;
  const dim3 grid((unsigned)blocks), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (reward_is_f64 && q_is_f64)
    hipLaunchKernelGGL((k_qmix_td_target<double, double>), grid, block, 0, s, (const double *)reward_local, n_agents, (const double *)q_tot, done, gamma, out, (size_t)n);
  else if (reward_is_f64)
    hipLaunchKernelGGL((k_qmix_td_target<double, float>), grid, block, 0, s, (const double *)reward_local, n_agents, (const float *)q_tot, done, gamma, out, (size_t)n);
  else if (q_is_f64)
    hipLaunchKernelGGL((k_qmix_td_target<float, double>), grid, block, 0, s, (const float *)reward_local, n_agents, (const double *)q_tot, done, gamma, out, (size_t)n);
  else
    hipLaunchKernelGGL((k_qmix_td_target<float, float>), grid, block, 0, s, (const float *)reward_local, n_agents, (const float *)q_tot, done, gamma, out, (size_t)n);
  CM3_HIP_CHECK(hipGetLastError());
  return CM3_OK;
}

int cm3_rows_tile(const cm3_tile_col *cols, int32_t n_cols, void *stream) {
  using namespace cm3;
  CM3_REQUIRE(cols && n_cols >= 1 && n_cols <= kMaxRowCols, "rows_tile: 1..%d columns", kMaxRowCols);
  TileCols a;
  memset(&a, 0, sizeof(a));
  a.n = n_cols;
  size_t most = 0;
  bool rows = false;      // a column of the launch takes the row-granular path
  for (int k = 0; k < n_cols; ++k) {
    const cm3_tile_col &q = cols[k];
    // (an EMPTY column may come with null pointers: torch.empty(0).data_ptr() is 0 -- ADVICE r5)
    CM3_REQUIRE(q.n_rows == 0 || (q.dst && (q.src || q.kind == CM3_TILE_EYE_F64)), "rows_tile: column %d is null", k);
    CM3_REQUIRE(q.kind >= CM3_TILE_COPY && q.kind <= CM3_TILE_NOT_I64, "rows_tile: column %d: unknown kind %d", k, (int)q.kind);
    CM3_REQUIRE(q.elems_per_row >= 1 && q.n_rows >= 0, "rows_tile: column %d: empty rows", k);
    CM3_REQUIRE(q.kind != CM3_TILE_COPY || q.elem_bytes == 1 || q.elem_bytes == 4 || q.elem_bytes == 8,
                "rows_tile: column %d: elem_bytes must be 1, 4 or 8", k);
    CM3_REQUIRE(q.others_n == 0 || (q.others_n >= 2 && q.others_divq >= 1 && q.others_divn >= 1), "rows_tile: column %d: bad others spec", k);
    CM3_REQUIRE(q.others_n != 0 || (q.div[0] >= 1 && q.div[1] >= 1), "rows_tile: column %d: divisors must be >= 1", k);
    TileCol &c = a.c[k];
    c.dst = q.dst;
    c.src = q.src;
    c.n_rows = (unsigned long long)q.n_rows;
    c.epr = q.elems_per_row;
    c.kind = q.kind;
    c.es = q.elem_bytes;
    c.div0 = q.div[0]; c.mod0 = q.mod[0]; c.mul0 = q.mul[0];
    c.div1 = q.div[1]; c.mod1 = q.mod[1]; c.mul1 = q.mul[1];
    c.oth_n = q.others_n; c.oth_divq = q.others_divq; c.oth_divn = q.others_divn;
    const size_t total = (size_t)q.n_rows * q.elems_per_row;
    most = total > most ? total : most;
    rows = rows || (total != 0 && tile_row_unit(c) != 0);
  }
  if (most == 0) return CM3_OK;
  const size_t blocks = rows_tile_blocks(most);
  const dim3 grid((unsigned)blocks, (unsigned)n_cols), block(256);
  const bool narrow = rows_take_narrow(rows_stride_index_narrow(most, blocks));
  if (narrow && rows) hipLaunchKernelGGL((k_rows_tile<uint32_t, true>), grid, block, 0, (hipStream_t)stream, a);
  else if (narrow) hipLaunchKernelGGL((k_rows_tile<uint32_t, false>), grid, block, 0, (hipStream_t)stream, a);
  else if (rows) hipLaunchKernelGGL((k_rows_tile<size_t, true>), grid, block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((k_rows_tile<size_t, false>), grid, block, 0, (hipStream_t)stream, a);
  CM3_HIP_CHECK(hipGetLastError());
  return CM3_OK;
}

int cm3_rows_scatter(const cm3_row_cols *cols, int64_t n_rows, const int64_t *dst_row, int64_t ring_start, int64_t ring_size,
                     void *stream) {
  using namespace cm3;
  CM3_REQUIRE(dst_row || (ring_size > 0 && ring_start >= 0 && ring_start < ring_size && n_rows <= ring_size),
              "rows_scatter: either dst_row or a ring (0 <= ring_start < ring_size, n_rows <= ring_size)");
  return rows_copy(cols, n_rows, dst_row, nullptr, ring_start, dst_row ? 0 : ring_size, (hipStream_t)stream);
}

int cm3_rows_gather(const cm3_row_cols *cols, int64_t n_rows, const int64_t *src_row, void *stream) {
  using namespace cm3;
  CM3_REQUIRE(src_row, "rows_gather: src_row is NULL");
  return rows_copy(cols, n_rows, nullptr, src_row, 0, 0, (hipStream_t)stream);
}

int cm3_transitions_gather_f32(const cm3_particle_desc *desc, const cm3_particle_traj *traj, const int32_t *goal_slot,
                               size_t goal_slot_stride, const int64_t *tt, const int64_t *ee, int64_t n,
                               const cm3_transition_cols *out, void *stream) {
  using namespace cm3;
  CM3_REQUIRE(desc && traj && out && ((tt == nullptr) == (ee == nullptr)), "null argument (tt and ee: both or neither)");
  CM3_REQUIRE(n >= 0, "n must be >= 0");
  if (n == 0) return CM3_OK;      // (before the pointer checks: the columns of an empty batch are null -- ADVICE r5)
  if (int rc = trans_check(desc, traj)) return rc;
  CM3_REQUIRE(out->state && out->obs_others && out->actions && out->reward && out->reward_n && out->next_state && out->next_obs_others &&
                  out->done && out->goals,
              "output columns are required");
  TransParams p;
  memset(&p, 0, sizeof(p));
  trans_sources(p, desc, traj, goal_slot, goal_slot_stride, n);
  p.tt = tt;
  p.ee = ee;
  p.o_state = (float *)out->state;
  p.o_obs = (float *)out->obs_others;
  p.o_actions = out->actions;
  p.o_reward = (float *)out->reward;
  p.o_reward_n = (float *)out->reward_n;
  p.o_next_state = (float *)out->next_state;
  p.o_next_obs = (float *)out->next_obs_others;
  p.o_done = out->done;
  p.o_goals = (float *)out->goals;
  if (int rc = ring_optional("transition columns", out->ring_start, out->ring_size, n)) return rc;
  p.ring_start = (size_t)out->ring_start;
  p.ring_size = (size_t)out->ring_size;
  trans_launch(p, (hipStream_t)stream);
  CM3_HIP_CHECK(hipGetLastError());
  return CM3_OK;
}

int cm3_transitions_route_f32(const cm3_particle_desc *desc, const cm3_particle_traj *traj, const int32_t *goal_slot,
                              size_t goal_slot_stride, int64_t n, const uint8_t *sel, const int64_t *row,
                              const cm3_transition_cols *sets, int32_t n_sets, void *stream) {
  using namespace cm3;
  CM3_REQUIRE(desc && traj && sets, "transitions_route: null argument");
  CM3_REQUIRE(n >= 0, "n must be >= 0");
  CM3_REQUIRE(n_sets >= 1 && n_sets <= 3, "transitions_route: 1..3 column sets");
  if (n == 0) return CM3_OK;
  CM3_REQUIRE(sel && row, "transitions_route: sel and row are required");
  if (int rc = trans_check(desc, traj)) return rc;
  CM3_REQUIRE(desc->n_envs >= 1 && n % desc->n_envs == 0, "transitions_route: n must be whole ticks (a multiple of n_envs)");
  RouteParams p;
  memset(&p, 0, sizeof(p));
  trans_sources(p, desc, traj, goal_slot, goal_slot_stride, n);
  p.sel = sel;
  p.row = row;
  p.n_sets = (uint32_t)n_sets;
  for (int k = 0; k < n_sets; ++k) {
    const cm3_transition_cols &o = sets[k];
    CM3_REQUIRE(o.state && o.obs_others && o.actions && o.reward && o.reward_n && o.next_state && o.next_obs_others && o.done && o.goals,
                "transitions_route: column set %d: output columns are required", k);
    CM3_REQUIRE(((uintptr_t)o.state | (uintptr_t)o.obs_others | (uintptr_t)o.next_state | (uintptr_t)o.next_obs_others) % 16 == 0 &&
                    (uintptr_t)o.goals % 8 == 0 && ((uintptr_t)o.actions | (uintptr_t)o.reward | (uintptr_t)o.reward_n) % 4 == 0,
                "transitions_route: column set %d is not aligned to the units the kernel stores", k);
    TransOut &t = p.set[k];
    t.state = (float *)o.state; t.obs = (float *)o.obs_others; t.actions = o.actions; t.reward = (float *)o.reward;
    t.reward_n = (float *)o.reward_n; t.next_state = (float *)o.next_state; t.next_obs = (float *)o.next_obs_others; t.done = o.done;
    t.goals = (float *)o.goals;
  }
  trans_launch(p, (hipStream_t)stream);
  CM3_HIP_CHECK(hipGetLastError());
  return CM3_OK;
}

int cm3_checkers_transitions_gather(const cm3_checkers_desc *desc, const cm3_checkers_traj *traj, const int32_t *prev0,
                                    const int64_t *tt, const int64_t *ee, int64_t n, const cm3_checkers_transition_cols *out,
                                    void *stream) {
  using namespace cm3;
  CM3_REQUIRE(desc, "checkers_transitions_gather: null desc");
  CM3_REQUIRE(traj, "checkers_transitions_gather: null traj");
  CM3_REQUIRE(out, "checkers_transitions_gather: null out");
  CM3_REQUIRE((tt == nullptr) == (ee == nullptr), "checkers_transitions_gather: tt and ee: both or neither");
  CM3_REQUIRE(n >= 0, "n must be >= 0");
  if (int rc = ring_optional("checkers transition columns", out->ring_start, out->ring_size, n)) return rc;
  if (n == 0) return CM3_OK;      // (before the pointer checks: the columns of an empty batch are null)
  CkGeom geo;
  if (int rc = ck_geometry(desc, true, geo)) return rc;
  bool term = false;
  if (int rc = ck_traj_check("checkers_transitions_gather", traj, prev0, term)) return rc;
  CkSpec specs[kCkCols];
  for (int k = 0; k < kCkCols; ++k) {
    const CkColumn &col = kCkColumns[k];
    specs[k] = ck_traj_spec(traj, col, ck_record(geo, col.rec), ck_field(out, col));
    if (col.prev) specs[k].kind = CKU_PREV;
  }
  return ck_gather_launch("checkers_transitions_gather", "checkers transition columns", "checkers trajectory", false, specs, term, traj->done, traj->done_stride, prev0, tt, ee,
                          (size_t)n, (size_t)desc->n_envs, out->ring_start, out->ring_size, (hipStream_t)stream);
}

int cm3_checkers_transitions_pack(const cm3_checkers_desc *desc, const cm3_checkers_traj *traj, const int32_t *prev0, int64_t n,
                                  const cm3_checkers_compact_cols *out, void *stream) {
  using namespace cm3;
  CM3_REQUIRE(desc, "checkers_transitions_pack: null desc");
  CM3_REQUIRE(traj, "checkers_transitions_pack: null traj");
  CM3_REQUIRE(out, "checkers_transitions_pack: null compact columns");
  CM3_REQUIRE(n >= 0, "n must be >= 0");
  if (int rc = ring_required("compact checkers columns", out->ring_start, out->ring_size, n)) return rc;
  if (n == 0) return CM3_OK;      // (before the pointer checks: nothing is touched)
  CkGeom geo;
  if (int rc = ck_geometry(desc, true, geo)) return rc;
  bool term = false;
  if (int rc = ck_traj_check("checkers_transitions_pack", traj, prev0, term)) return rc;
  PkParams p;
  memset(&p, 0, sizeof(p));
  const size_t start = (size_t)out->ring_start, size = (size_t)out->ring_size;
  const size_t rows_a = start + (size_t)n <= size ? (size_t)n : size - start, rows_b = (size_t)n - rows_a;   // before / past the wrap
  size_t blocks = 0, most = 0;
  for (int k = 0; k < kCkCols; ++k) {
    const CkColumn &col = kCkColumns[k];
    CkSpec s = ck_traj_spec(traj, col, ck_record(geo, col.rec), ck_field(out, col));
    s.kind = col.prev ? PK_PREV : col.rec == CKR_DONE ? PK_DONE : PK_COPY;
    PkCol &c = p.col[k];
    if (int rc = ck_col_fill(c, s, term, "compact checkers columns")) return rc;
    CM3_REQUIRE((uintptr_t)s.dst % 16 == 0, "compact checkers columns: column %s is not aligned to the 16-byte pieces the kernel stores",
                s.name);
    c.rb = s.row_bytes;
    c.lo_a = start * s.row_bytes;
    c.hi_a = (start + rows_a) * s.row_bytes;
    c.hi_b = rows_b * s.row_bytes;
    // the granule: what divides the row, every stride and every base (a granule is one naturally aligned load inside one row)
    uintptr_t a = (uintptr_t)c.src | (uintptr_t)c.alt | c.slot_stride | c.alt_stride | c.env_stride | c.rb;
    if (s.kind == PK_PREV) a |= (uintptr_t)prev0;
    c.gran = a % 16 == 0 ? 16u : a % 8 == 0 ? 8u : a % 4 == 0 ? 4u : a % 2 == 0 ? 2u : 1u;
    const size_t pieces = (c.hi_a + 15) / 16 - c.lo_a / 16 + (c.hi_b + 15) / 16;
    const size_t bytes = size * s.row_bytes;
    most = bytes > most ? bytes : most;
    if (int rc = ck_col_blocks("checkers_transitions_pack", pieces, kPkPiecesPerLane * 256, blocks, p.blk_end[k])) return rc;
  }
  p.done = traj->done;
  p.st_done = traj->done_stride;
  p.prev0 = (const char *)prev0;
  p.E = (size_t)desc->n_envs;
  p.ring_start = start;
  p.ring_size = size;
  p.term = term ? 1 : 0;
  // (32-bit byte offsets into a ring column whenever the largest column fits, the slack of a last workgroup included)
  if (rows_take_narrow(ck_pack_index_narrow(most, size)))
    hipLaunchKernelGGL(k_ck_transitions_pack<uint32_t>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(k_ck_transitions_pack<size_t>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
  CM3_HIP_CHECK(hipGetLastError());
  return CM3_OK;
}

int cm3_checkers_ring_expand(const cm3_checkers_desc *desc, const cm3_checkers_compact_cols *ring, const int64_t *index, int64_t n,
                             const cm3_checkers_transition_cols *out, void *stream) {
  using namespace cm3;
  CM3_REQUIRE(desc, "checkers_ring_expand: null desc");
  CM3_REQUIRE(ring, "checkers_ring_expand: null compact columns");
  CM3_REQUIRE(out, "checkers_ring_expand: null out");
  CM3_REQUIRE(n >= 0, "n must be >= 0");
  if (int rc = ring_required("compact checkers columns", ring->ring_start, ring->ring_size, n)) return rc;
  if (int rc = ring_optional("checkers transition columns", out->ring_start, out->ring_size, n)) return rc;
  if (n == 0) return CM3_OK;      // (before the pointer checks: the columns of an empty batch are null)
  CkGeom geo;
  if (int rc = ck_geometry(desc, false, geo)) return rc;
  // the unit kinds of the export with ONE slot (stride 0) of dense ring rows as their source: row index[b] is the "env", the
  // actions_prev and done a row holds are final (plain copies -- CKU_DONE reads p.done, here the ring's own column)
  CkSpec specs[kCkCols];
  for (int k = 0; k < kCkCols; ++k) {
    const CkColumn &col = kCkColumns[k];
    const CkRecord r = ck_record(geo, col.rec);
    const void *src = ck_field(ring, col);
    CM3_REQUIRE(src, "compact checkers columns: column %s is missing", col.name);
    specs[k] = {col.name, ck_field(out, col), src, nullptr, 0, 0, r.row_bytes, r.row_bytes, r.upr, r.kind, 0};
  }
  // index NULL: rows 0 .. n - 1 -- the whole-trajectory order b = t E + e with E = n is tick 0, env b
  return ck_gather_launch("checkers_ring_expand", "checkers transition columns", "compact checkers columns", true, specs, false, ring->done, 0, nullptr, nullptr, index,
                          (size_t)n, (size_t)n, out->ring_start, out->ring_size, (hipStream_t)stream);
}
}
