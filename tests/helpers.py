"""Shared helpers for the parity tests (test infrastructure)."""
import glob
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CFG_DIR = os.path.join(ROOT, "cm3_amd", "configs")


def golden_names(prefix):
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, prefix + "*.npz")))


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(str(d["meta"]))
    return d


def load_cfg(name):
    with open(os.path.join(CFG_DIR, name)) as f:
        return json.load(f)


def band_init(n_agents, seed=None):
    """The reference geometry (3 x 8 band, n_obs 2) with ``n_agents`` distinct start cells: the first cells of a seeded
    permutation of the 27 cells of band plus start column (column 8), or, with no seed, the start column top to bottom."""
    if seed is None:
        assert n_agents <= 3
        cells = [8 + 9 * r for r in range(n_agents)]
    else:
        cells = np.random.default_rng(seed).permutation(27)[:n_agents]
    return dict(n_rows=3, n_columns=8, n_obs=2, agents_r=[int(c) // 9 for c in cells], agents_c=[int(c) % 9 for c in cells])


def left_biased_actions(rng, shape, lo=-1, hi=7, p_left=0.3):
    """Actions in lo..hi-1 (out-of-range ones included), 30 % overwritten with "left" so that episodes collect many cells."""
    acts = rng.integers(lo, hi, shape)
    return np.where(rng.random(shape) < p_left, 3, acts)


def particle_transition_columns(g, ep):
    """The reference's 11 transition columns of episode ``ep`` of a particle golden fixture -> (columns, T, N)."""
    T = int(g["ep_len"][ep])
    N = g["meta"]["n_agents"]
    gs = np.concatenate([g["init_gs"][ep][None], g["gs"][ep, :T]])
    oo = np.concatenate([g["init_obs_others"][ep][None], g["obs_others"][ep, :T]])
    goals = np.repeat(g["landmarks"][ep][None], T, axis=0)
    return dict(v_global=gs[:-1], obs_others=oo[:-1], v_local=gs[:-1], actions=g["actions"][ep, :T],
                reward=g["reward"][ep, :T], reward_local=g["reward_n"][ep, :T], v_global_next=gs[1:],
                obs_others_next=oo[1:], v_local_next=gs[1:], done=g["done"][ep, :T], goals=goals), T, N


def checkers_transition_columns(g, ep):
    """The reference's 16 transition columns of episode ``ep`` of a Checkers golden fixture -> (columns, T, N)."""
    T, N = int(g["ep_len"][ep]), g["meta"]["n_agents"]

    def seq(init, per_tick):
        return np.concatenate([g[init][ep][None], g[per_tick][ep, :T]])
    grid, vec = seq("init_grid", "grid"), seq("init_vec", "vec")
    oo, ot, ov = seq("init_obs_others", "obs_others"), seq("init_obs_self_t", "obs_self_t"), seq("init_obs_self_v", "obs_self_v")
    acts = g["actions"][ep, :T]
    prev = np.concatenate([np.zeros((1, N), acts.dtype), acts[:-1]])
    return dict(grid=grid[:-1], vec=vec[:-1], obs_others=oo[:-1], obs_self_t=ot[:-1], obs_self_v=ov[:-1],
                actions_prev=prev, actions=acts, reward=g["reward"][ep, :T], local_rewards=g["local_rewards"][ep, :T],
                next_grid=grid[1:], next_vec=vec[1:], next_obs_others=oo[1:], next_obs_self_t=ot[1:],
                next_obs_self_v=ov[1:], done=g["done"][ep, :T],
                goals=np.repeat(g["goals"][ep][None], T, axis=0).astype(float)), T, N
