// Which (env, agent) a lane of the one-launch policy rollout (k_policy_rollout, policy.hip) owns, and how many 16-row tiles and
// workgroups a batch needs, as pure functions of a handful of integers.  Plain C++17, no HIP: the kernel, its launcher and
// tests/test_policy_tiles.py (which compiles this header alone and walks it on a machine without a GPU) share this one definition.
//
// A wave owns one 16-row tile of the actor's input and exchanges env state inside the wave, so a tile holds WHOLE envs:
// 16 / N of them (integer division), in rows 0 .. rows_used - 1; the remaining rows of the tile are pad rows that belong to nobody.
//   N               1   2   3   4   5   6   7   8   9   10
//   envs per tile   16  8   5   4   3   2   2   2   1   1
//   rows used       16  16  15  16  15  12  14  16  9   10
// Tile k of a batch holds envs [k * envs_per_tile, (k + 1) * envs_per_tile); workgroup b of a launch with RT row tiles per
// workgroup holds tiles b * RT .. b * RT + RT - 1.  For N in {1, 2, 4, 8} nothing is padded and the map is the dense one the
// kernel has always had: row r = 16 * tile + (lane & 15), env r / N, agent r % N.
#pragma once
#include <stddef.h>

namespace cm3 {

constexpr int kPolicyTileRows = 16;
constexpr int policy_envs_per_tile(int n) { return kPolicyTileRows / n; }
constexpr int policy_rows_used(int n) { return policy_envs_per_tile(n) * n; }
constexpr bool policy_tile_is_dense(int n) { return kPolicyTileRows % n == 0; }
constexpr size_t policy_tiles(size_t E, int n) { return (E + policy_envs_per_tile(n) - 1) / policy_envs_per_tile(n); }
constexpr unsigned policy_blocks(size_t E, int n, int rt) { return (unsigned)((policy_tiles(E, n) + rt - 1) / rt); }
// the tile that wave `w` (< rt) of workgroup `block` owns
constexpr size_t policy_tile_of(size_t block, int w, int rt) { return block * rt + w; }

// What lane `lane16` = lane & 15 of the wave that owns `tile` works on.  owns: the lane's row exists -- it is one of the tile's used
// rows and its env is inside the batch; only such a lane stores anything.  A lane that owns nothing (a pad lane) mirrors row 0 of
// its tile, as lanes 16 .. 63 of the wave mirror lane l & 15: local_row is the row OF THE TILE whose state the lane reads, and
// (env, agent) is a valid pair of the batch for every lane -- row 0's, or, in a tile that lies wholly behind the batch (the last
// workgroup of a launch with RT > 1), agent 0 of the last env.
struct PolicyTileRow {
  size_t env;
  int agent;
  int local_row;   // 0 .. rows_used - 1
  bool owns;
};
constexpr PolicyTileRow policy_tile_row(size_t tile, int lane16, int n, size_t E) {
  const size_t env0 = tile * policy_envs_per_tile(n);
  const int slot = lane16 / n;
  const size_t env = env0 + slot;
  if (lane16 < policy_rows_used(n) && env < E) return PolicyTileRow{env, lane16 - slot * n, lane16, true};
  return PolicyTileRow{env0 < E ? env0 : E - 1, 0, 0, false};
}

}  // namespace cm3
