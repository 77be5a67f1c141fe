"""CPU: the tile geometry of the one-launch policy rollout (csrc/policy_tiles.h) and what rests on it without a GPU.

A wave of k_policy_rollout owns a 16-row tile that holds 16 // N whole envs; for N in {3, 5, 6, 7, 9, 10} the remaining rows are
pad rows.  The row <-> (env, agent) map, the tile count and the grid are pure functions in a header that needs no HIP, so a small
program with its own main() -- written here, compiled with the host compiler under AddressSanitizer and UBSan -- prints the map of
every (N, E, RT) it reads and the properties are checked on what it printed.  Then, through the loaded library: which entry points
accept which agent counts (nothing here launches), and that ParticleRollout takes the opt-in keyword.
"""
import ctypes
import inspect
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cm3_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
AGENTS = list(range(1, 11))
ENVS = [1, 2, 5, 16, 37, 600]
ROW_TILES = [1, 2, 4]
ENVS_PER_TILE = {1: 16, 2: 8, 3: 5, 4: 4, 5: 3, 6: 2, 7: 2, 8: 2, 9: 1, 10: 1}      # the issue's table, restated by hand
FAKE = 0x1000                                   # never dereferenced: validation fails first

PROGRAM = r"""
#include <stdio.h>
#include "policy_tiles.h"
static_assert(cm3::policy_envs_per_tile(3) == 5 && cm3::policy_rows_used(3) == 15 && cm3::policy_tiles(37, 3) == 8 &&
              cm3::policy_blocks(37, 3, 4) == 2 && cm3::policy_tile_is_dense(8) && !cm3::policy_tile_is_dense(10),
              "the geometry is usable in constant expressions (the kernel's if constexpr)");
int main() {
  int n, rt;
  unsigned long E;
  while (scanf("%d %lu %d", &n, &E, &rt) == 3) {
    const unsigned blocks = cm3::policy_blocks(E, n, rt);
    printf("H %d %d %lu %u\n", cm3::policy_envs_per_tile(n), cm3::policy_rows_used(n), (unsigned long)cm3::policy_tiles(E, n), blocks);
    for (unsigned b = 0; b < blocks; ++b)
      for (int w = 0; w < rt; ++w)
        for (int l = 0; l < 16; ++l) {
          const cm3::PolicyTileRow r = cm3::policy_tile_row(cm3::policy_tile_of(b, w, rt), l, n, E);
          printf("R %u %d %d %lu %d %d %d\n", b, w, l, (unsigned long)r.env, r.agent, r.local_row, (int)r.owns);
        }
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def tile_maps(tmp_path_factory):
    """{(N, E, RT): (header, rows)}: header = (envs_per_tile, rows_used, tiles, blocks), rows = [(block, wave, lane, env, agent,
    local_row, owns)] for every lane < 16 of every wave < RT of every workgroup of the launch."""
    tmp = tmp_path_factory.mktemp("policy_tiles")
    src, exe = tmp / "tiles.cpp", tmp / "tiles"
    src.write_text(PROGRAM)
    san = ["-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe)]
    if shutil.which("g++"):
        subprocess.check_call(["g++"] + san + [str(src)])
    elif os.path.exists(HIPCC):
        subprocess.check_call([HIPCC, "-x", "c++"] + san + [str(src)])      # host only: the header holds no device code
    else:
        pytest.skip("no host C++ compiler")
    cases = [(n, e, rt) for n in AGENTS for e in ENVS for rt in ROW_TILES]
    out = subprocess.run([str(exe)], input="".join("%d %d %d\n" % c for c in cases), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr              # (a sanitizer report ends the program with a non-zero status)
    maps, cur = {}, None
    for line in out.stdout.splitlines():
        tag, *v = line.split()
        if tag == "H":
            cur = (tuple(map(int, v)), [])
            maps[cases[len(maps)]] = cur
        else:
            cur[1].append(tuple(map(int, v)))
    assert len(maps) == len(cases)
    return maps


def test_every_env_agent_pair_has_exactly_one_owner_and_pad_lanes_own_nothing(tile_maps):
    for (n, E, rt), ((ept, used, tiles, blocks), rows) in tile_maps.items():
        assert ept == ENVS_PER_TILE[n] == 16 // n and used == ept * n, (n, ept, used)
        owned = [(env, agent) for _, _, _, env, agent, _, owns in rows if owns]
        assert sorted(owned) == [(e, a) for e in range(E) for a in range(n)], (n, E, rt)     # each pair once, none behind the batch
        for b, w, l, env, agent, local, owns in rows:
            tile = b * rt + w
            first = tile * ept
            pad = l >= used or first + l // n >= E
            assert owns == (not pad), (n, E, rt, b, w, l)
            # every lane, owner or not, holds a pair of the batch (its entry loads) and a used row of its own tile (its LDS reads)
            assert 0 <= env < E and 0 <= agent < n and 0 <= local < used, (n, E, rt, b, w, l)
            if owns:
                assert (env, agent, local) == (first + l // n, l % n, l), (n, E, rt, b, w, l)
                assert first <= env < first + ept                              # whole envs: all agents of an env in one tile
            else:
                assert (agent, local) == (0, 0) and env == min(first, E - 1), (n, E, rt, b, w, l)   # mirrors row 0 of its tile


def test_grid_covers_every_tile_and_no_workgroup_is_empty(tile_maps):
    for (n, E, rt), ((ept, used, tiles, blocks), rows) in tile_maps.items():
        assert tiles == -(-E // ept) and blocks == -(-tiles // rt), (n, E, rt)
        assert blocks * rt >= tiles > (blocks - 1) * rt
        owners = {}
        for b, w, l, env, agent, local, owns in rows:
            owners[b] = owners.get(b, 0) + owns
        assert sorted(owners) == list(range(blocks)) and min(owners.values()) > 0, (n, E, rt)
        assert sum(owners.values()) == E * n


@pytest.mark.parametrize("n", [1, 2, 4, 8])
def test_dense_agent_counts_keep_the_old_formula(tile_maps, n):
    """r = block * 16 * RT + 16 * w + (lane & 15), e = r // N, i = r % N, owned iff r < E * N; grid = ceil(E N / (16 RT)), and the
    row-tile rule's count of 64-row workgroups, ceil(tiles / 4), is ceil(E N / 64)."""
    for E in ENVS:
        for rt in ROW_TILES:
            (ept, used, tiles, blocks), rows = tile_maps[(n, E, rt)]
            assert used == 16 and blocks == -(-(E * n) // (16 * rt)) and -(-tiles // 4) == -(-(E * n) // 64)
            for b, w, l, env, agent, local, owns in rows:
                r = b * 16 * rt + 16 * w + l
                assert owns == (r < E * n)
                if owns:
                    assert (env, agent, local) == (r // n, r % n, l)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from cm3_amd import _lib
    return _lib


def _descs(built, n):
    d = built.ParticleDesc()
    d.n_envs, d.n_agents, d.max_steps, d.flags = 16, n, 33, 0
    d.seed, d.env_id_base, d.prob_random = 7, 0, 0.2
    a = built.ActorParticleDesc()
    a.n_envs, a.n_agents, a.stage = 16, n, 2
    a.n_h1_self, a.n_h1_others, a.n_h2, a.n_actions = 64, 0, 64, 5
    a.epsilon, a.precision = 0.1, 0
    a.seed, a.env_id_base = 7, 0
    t = built.ParticleTraj()
    for name, ctype in t._fields_:
        if ctype is ctypes.c_void_p and name not in ("state_live", "goals_live", "live_record"):
            setattr(t, name, FAKE)
    return d, t, a


def test_float64_and_qmix_entries_still_refuse_three_agents(built):
    handle = built.lib()
    d, t, a = _descs(built, 3)
    wt = built.ActorParticleWeights()
    rc = handle.cm3_policy_rollout_f64(ctypes.byref(d), ctypes.byref(t), ctypes.byref(a), ctypes.byref(wt), None, 0, 4, None)
    msg = handle.cm3_last_error()
    assert rc == -1 and b"{1, 2, 4, 8}" in msg and b"got 3" in msg, msg
    rc = handle.cm3_policy_rollout_qmix_f32(ctypes.byref(d), ctypes.byref(t), ctypes.byref(a), FAKE, None, 0, None, 4, None)
    msg = handle.cm3_last_error()
    assert rc == -1 and b"{1, 2, 4, 8}" in msg and b"got 3" in msg, msg


@pytest.mark.parametrize("n", [0, 11])
def test_float32_entry_refuses_agent_counts_outside_one_to_ten(built, n):
    """(an accepted count is never tried here: with these fake pointers it would launch)"""
    handle = built.lib()
    d, t, a = _descs(built, n)
    wt = built.ActorParticleWeights()
    rc = handle.cm3_policy_rollout_f32(ctypes.byref(d), ctypes.byref(t), ctypes.byref(a), ctypes.byref(wt), None, 0, 4, None)
    msg = handle.cm3_last_error()
    assert rc == -1 and b"1..10" in msg and (b"got %d" % n) in msg, msg
    assert built.ABI_VERSION == 9 and handle.cm3_abi_version() == 9          # no new export: the ABI does not move


def test_rollout_takes_the_keyword_and_carries_the_auto_table():
    from cm3_amd import rollout
    sig = inspect.signature(rollout.ParticleRollout.__init__)
    assert sig.parameters["partial_tiles"].default is False
    assert sorted(rollout.PARTIAL_TILES_AUTO) == [3, 5, 6, 7, 9, 10]
    for n, bound in rollout.PARTIAL_TILES_AUTO.items():          # "auto": the one launch up to `bound` envs, launch pairs beyond
        assert isinstance(bound, int) and bound >= 0
        assert rollout.partial_tiles_auto(n, bound + 1) is False and rollout.partial_tiles_auto(n, max(bound, 1)) is (bound > 0)
    assert rollout.partial_tiles_auto(4, 1) is False             # (the dense agent counts are not this table's business)
