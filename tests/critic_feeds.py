"""TEST INFRASTRUCTURE ONLY -- batches, the tiled critic feeds of the torch composition, and the critics' reference on them (helper
of tests/test_gpu_critic_rows.py and tests/test_gpu_critic_train_feeds.py; not a test module)."""
import numpy as np
import torch

from tests import critic_ref as CR

BOUND = 2e-5                       # the project's float32-network bound: BOUND * max(1, |ref|) per row (tests/test_gpu_qmix_rows.py)
CRITIC_OPS = (["Q_global_target"], ["Q_credit_target"], ["Q_credit"], ["Q_global"])


def make_cols(B, N, seed, device="cpu", reward_dtype=torch.float32):
    """The columns of a sampled particle batch (ParticleRollout.as_reference_batch(numpy=False)): float32, states uniform in +-2."""
    rng = np.random.default_rng(seed)
    L = 4 * max(N - 1, 1)
    u = lambda lo, *s: torch.as_tensor(rng.uniform(-lo, lo, s).astype(np.float32))      # noqa: E731
    cols = {"v_global": u(2, B, N, 4), "obs_others": u(2, B, N, L), "v_local": u(2, B, N, 4),
            "actions": torch.as_tensor(rng.integers(0, 5, (B, N))), "reward": u(1, B), "reward_local": u(1, B, N).to(reward_dtype),
            "v_global_next": u(2, B, N, 4), "obs_others_next": u(2, B, N, L), "v_local_next": u(2, B, N, 4),
            "done": torch.as_tensor(rng.random(B) < 0.4), "goals": u(1, B, N, 2)}
    return {k: v.to(device) for k, v in cols.items()}


def rows_of(feed):
    return max([v.shape[0] for v in feed.values() if torch.is_tensor(v) and v.dim() > 0] or [1])


def tiled_feeds(cols, acts):
    """{op name: feed} of the critic evaluations without a gradient, built by the torch composition of train_step_feeds (static=None,
    device_tiling=False) with `acts` [B * N] as the target actor's samples."""
    from cm3_amd.batch import train_step_feeds
    N = cols["v_global"].shape[1]
    dev = cols["v_global"].device
    seen = {}

    def run(ops, feed):
        if ops in CRITIC_OPS:
            seen[ops[0]] = feed
        if ops == ["action_samples_target"]:
            return [acts.to(dev)]
        if ops == ["probs"]:
            return [torch.full((rows_of(feed), 5), 0.2, dtype=torch.float64, device=dev)]
        return [None if (op.endswith("_op") or op == "list_update_target_ops") else torch.zeros(rows_of(feed), 1, dtype=torch.float64, device=dev)
                for op in ops]
    train_step_feeds(cols, run, 0.99, 0.1, use_V=False, device_tiling=False)
    assert sorted(seen) == (["Q_global", "Q_global_target"] if N == 1 else ["Q_credit", "Q_credit_target", "Q_global_target"])
    return seen


def ref_on_feed(w, feed, kind, n, dtype):
    """critic_ref on a tiled feed (the reference's placeholder names) -> [rows] in `dtype`"""
    f = {k: v.detach().cpu().numpy() for k, v in feed.items() if torch.is_tensor(v)}
    if kind == "global":
        q = CR.q_global(w, f["v_state_one_agent"], f["v_goal"], f["action_one"], f["v_state_other_agents"], f["action_others"],
                        stage=1 if n == 1 else 2, dtype=dtype)
    else:
        q = CR.q_credit(w, f["v_state_one_agent"], f["v_goal"], f["action_one"], f["v_state_m"], f["v_state_other_agents"], dtype=dtype)
    return q.reshape(-1)


def within(got, ref, scale=1.0, what=""):
    """prints the largest share of the bound used, then asserts it"""
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    used = np.abs(got - ref) / (scale * BOUND * np.maximum(1.0, np.abs(ref)))
    print("%s: max |q| %.3f, share of the bound used %.3f" % (what, float(np.abs(ref).max()), float(used.max())))
    assert used.max() <= 1.0, (what, float(used.max()))
