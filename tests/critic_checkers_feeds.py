"""TEST INFRASTRUCTURE ONLY -- Checkers batches, the tiled critic feeds of the torch composition, and the Checkers critics' reference
on them (helper of tests/test_gpu_critic_checkers_rows.py and tests/test_gpu_critic_checkers_train_feeds.py; not a test module)."""
import numpy as np
import torch

from tests import critic_checkers_ref as CR
from tests.critic_feeds import BOUND, CRITIC_OPS, rows_of, within  # noqa: F401  (the project's bound and its report)

WEIGHT_SCALE = 1.5                 # init_weights(scale=...): |Q| reaches several units (tests/test_gpu_critic_checkers_rows.py)


def make_cols(B, N, seed, device="cpu", reward_dtype=torch.float64):
    """The 16 columns of a sampled Checkers batch (CheckersRollout.as_reference_batch(numpy=False)): wide columns float64, grids 0 / 1,
    windows -1 / 0 / 1 (what the env emits), agent states uniform in +-2, goals one-hot int64."""
    rng = np.random.default_rng(seed)
    Lo = 2 * max(N - 1, 1)
    u = lambda lo, *s: torch.as_tensor(rng.uniform(-lo, lo, s))      # noqa: E731
    grid = lambda: torch.as_tensor(rng.integers(0, 2, (B, 3, 9, 2)).astype(np.float64))      # noqa: E731
    win = lambda: torch.as_tensor(rng.integers(-1, 2, (B, N, 5, 5, 3)).astype(np.float64))      # noqa: E731
    cols = {"grid": grid(), "vec": u(2, B, N, 4), "obs_others": u(1, B, N, Lo), "obs_self_t": win(), "obs_self_v": u(1, B, N, 4),
            "actions_prev": torch.as_tensor(rng.integers(0, 5, (B, N)).astype(np.int32)),
            "actions": torch.as_tensor(rng.integers(0, 5, (B, N)).astype(np.int32)), "reward": u(1, B),
            "local_rewards": u(1, B, N).to(reward_dtype), "next_grid": grid(), "next_vec": u(2, B, N, 4),
            "next_obs_others": u(1, B, N, Lo), "next_obs_self_t": win(), "next_obs_self_v": u(1, B, N, 4),
            "done": torch.as_tensor(rng.random(B) < 0.4), "goals": torch.as_tensor(np.eye(2, dtype=np.int64)[rng.integers(0, 2, (B, N))])}
    return {k: v.to(device) for k, v in cols.items()}


def composition_run(acts, seen, dev):
    """a `run` that records the feeds of the critic evaluations without a gradient and answers every op with zeros"""
    def run(ops, feed):
        if ops in CRITIC_OPS:
            seen[ops[0]] = feed
        if ops == ["action_samples_target"]:
            return [acts.to(dev)]
        if ops == ["probs"]:
            return [torch.full((rows_of(feed), 5), 0.2, dtype=torch.float64, device=dev)]
        return [None if (op.endswith("_op") or op == "list_update_target_ops") else torch.zeros(rows_of(feed), 1, dtype=torch.float64, device=dev)
                for op in ops]
    return run


def tiled_feeds(cols, acts):
    """{op name: feed} of the critic evaluations without a gradient, built by the torch composition of
    train_step_feeds(env="checkers", device_tiling=False) with `acts` [B * N] as the target actor's samples."""
    from cm3_amd.batch import train_step_feeds
    N = cols["vec"].shape[1]
    seen = {}
    train_step_feeds(cols, composition_run(acts, seen, cols["vec"].device), 0.99, 0.1, env="checkers", use_V=False, device_tiling=False)
    assert sorted(seen) == (["Q_global", "Q_global_target"] if N == 1 else ["Q_credit", "Q_credit_target", "Q_global_target"])
    return seen


def ref_on_feed(w, feed, kind, n, dtype):
    """critic_checkers_ref on a tiled feed (the reference's placeholder names) -> [rows] in `dtype`"""
    return CR.q_from_feed(w, kind, {k: v for k, v in feed.items() if torch.is_tensor(v)}, stage=1 if n == 1 else 2, dtype=dtype).reshape(-1)


# ---- the cases of the GPU tests, built once and left unchanged (tests/test_critic_checkers_oracle.py checks on the CPU how much of the
# bound the float32 restatement alone uses on them) ---------------------------------------------------------------------------------------
AGENTS = (1, 2, 3, 8)
BATCHES = (1, 3, 13)
_CACHE = {}


def weights(N):
    """(Q_global_target weights, Q_credit_main weights or None) of the GPU tests' critics for N agents"""
    if ("w", N) not in _CACHE:
        rng = np.random.default_rng(500 + N)
        wg = CR.init_weights(rng, N, "global", scale=WEIGHT_SCALE, scope="Q_global_target")
        wc = CR.init_weights(rng, N, "credit", scale=WEIGHT_SCALE, scope="Q_credit_main") if N > 1 else None
        _CACHE[("w", N)] = (wg, wc)
    return _CACHE[("w", N)]


def case(N, B):
    """(host columns, target actions [B * N], the composition's tiled feeds) of the GPU tests' batch of B time steps, N agents"""
    if ("case", N, B) not in _CACHE:
        cols = make_cols(B, N, 7000 + 31 * N + B)
        acts = torch.as_tensor(np.random.default_rng(N * 100 + B).integers(0, 5, B * N))
        _CACHE[("case", N, B)] = (cols, acts, tiled_feeds(cols, acts))
    return _CACHE[("case", N, B)]


def refs(N, B, dtype=np.float64):
    """{op name: the restatement on the composition's feed, [rows]} for the critics of weights(N)"""
    key = ("ref", N, B, np.dtype(dtype).name)
    if key not in _CACHE:
        wg, wc = weights(N)
        _, _, feeds = case(N, B)
        _CACHE[key] = {op: ref_on_feed(wc if "credit" in op else wg, f, "credit" if "credit" in op else "global", N, dtype)
                       for op, f in feeds.items()}
    return _CACHE[key]
