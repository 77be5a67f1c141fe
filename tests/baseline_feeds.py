"""TEST INFRASTRUCTURE ONLY -- the tiled feeds of the baseline critics as the torch composition of
cm3_amd.batch.baseline_train_step_feeds builds them, and tests/baseline_ref.py on them (helper of tests/test_gpu_baseline_rows.py and
tests/test_gpu_baseline_train_feeds.py; not a test module).  Batches and the bound are tests/critic_feeds.py's."""
import numpy as np
import torch

from tests import baseline_ref as BR
from tests.critic_feeds import make_cols, rows_of, within  # noqa: F401

VALUE_OPS, Q_TARGET_OPS, Q_OPS = ["V_target", "V"], ["Q_target"], ["Q", "probs"]


def blank_run(acts, seen=None, dev="cpu"):
    """a `run` that answers every op with zeros of the right shape (the samples with `acts`) and notes the feeds of the evaluations
    without a gradient in `seen`"""
    def run(ops, feed):
        if seen is not None and ops in (VALUE_OPS, Q_TARGET_OPS, Q_OPS):
            seen[ops[0]] = feed
        out = []
        for op in ops:
            if op.endswith("_op") or op == "list_update_target_ops":
                out.append(None)
            elif op == "action_samples_target":
                out.append(acts.to(dev))
            elif op == "probs":
                out.append(torch.full((rows_of(feed), 5), 0.2, dtype=torch.float64, device=dev))
            elif op in ("Q_target", "Q"):
                out.append(torch.zeros(rows_of(feed), 5, dtype=torch.float32, device=dev))
            else:
                out.append(torch.zeros(rows_of(feed), 1, dtype=torch.float32, device=dev))
        return out
    return run


def tiled_feeds(cols, acts, IAC):
    """{"V_target": feed on the next-step columns, "Q_target": ..., "Q": ...} (the COMA feeds with more than one agent only), built by
    the torch composition with `acts` [B * N] as the target actor's samples"""
    from cm3_amd.batch import baseline_train_step_feeds
    N = cols["v_global"].shape[1]
    seen = {}
    baseline_train_step_feeds(cols, blank_run(acts, seen, cols["v_global"].device), 0.99, 0.1, IAC=IAC, use_Q=0 if IAC else 1, use_V=1)
    assert sorted(seen) == (["V_target"] if (IAC or N == 1) else ["Q", "Q_target", "V_target"])
    return seen


def value_ref_on_feed(w, feed, kind, n, dtype):
    """baseline_ref on a tiled value feed (the reference's placeholder names) -> [rows] in `dtype`"""
    f = {k: v.detach().cpu().numpy() for k, v in feed.items() if torch.is_tensor(v)}
    stage = 1 if n == 1 else 2
    if kind == "local":
        return BR.v_local(w, f["obs_others"], f["v_obs"], f["v_goal"], stage=stage, dtype=dtype).reshape(-1)
    return BR.v_global(w, f["v_state_one_agent"], f["v_goal"], f["v_state_other_agents"], f["v_goal_others"], stage=stage,
                       dtype=dtype).reshape(-1)


def coma_ref_on_feed(w, feed, dtype):
    """baseline_ref on a tiled COMA feed -> [rows, 5] in `dtype`"""
    f = {k: v.detach().cpu().numpy() for k, v in feed.items() if torch.is_tensor(v)}
    return BR.q_coma(w, f["v_state"], f["action_others"], f["v_goal"], f["v_goal_others"], f["v_labels"], f["v_obs"], dtype=dtype)


def chain_f32(x, w, b=None):
    """x . w (+ b as the start value) in float32 as ONE sequential k-ordered chain of fused multiply-adds per output, the order of
    the exact-f32 matrix instruction: each step is computed in float64 (exact for float32 products) and rounded to float32 once"""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    acc = np.zeros((x.shape[0], w.shape[1]), np.float32) if b is None else np.broadcast_to(np.asarray(b, np.float32), (x.shape[0], w.shape[1])).copy()
    for k in range(x.shape[1]):
        acc = (acc.astype(np.float64) + x[:, k:k + 1].astype(np.float64) * w[k:k + 1].astype(np.float64)).astype(np.float32)
    return acc
