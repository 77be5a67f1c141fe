"""GPU: what a captured train_step_feeds launch reads or writes outlives the capture.  process_actions_device hands the int32 form
of the sampled actions to the caller's keep list, and OnPolicyPhasePlan holds it (and issues no torch.eye on the static path), so a
replay touches no block the allocator may have given to someone else."""
import pytest
import torch

from tests.helpers import load_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_process_actions_device_hands_its_int32_temporary_to_keep():
    from cm3_amd import batch as BR
    B, N = 3, 3
    acts = (torch.arange(B * N, device=DEV) * 7 + 3) % 5                            # int64 [B * N]
    keep = []
    one, others, rep = BR.process_actions_device(acts, B, N, rep_m=True, keep=keep)
    torch.cuda.synchronize()
    assert len(keep) == 1 and keep[0].dtype == torch.int32 and keep[0].numel() == B * N and keep[0].is_cuda
    assert torch.equal(keep[0].long(), acts)
    want_one, want_others = BR.process_actions(acts.reshape(B, N))
    assert one.dtype == want_one.dtype and others.dtype == want_others.dtype
    assert torch.equal(one, want_one) and torch.equal(others, want_others) and torch.equal(rep, BR.rep_rows(want_one, N))
    # int32 input: no temporary -- the list receives the input itself (or nothing)
    keep32, a32 = [], acts.to(torch.int32)
    one32, others32, none = BR.process_actions_device(a32, B, N, keep=keep32)
    torch.cuda.synchronize()
    assert none is None and all(t.data_ptr() == a32.data_ptr() for t in keep32) and len(keep32) <= 1
    assert torch.equal(one32, want_one) and torch.equal(others32, want_others)
    assert BR.process_actions_device(acts, B, N)[2] is None                         # (keep is optional)


def test_plan_replay_leaves_blocks_of_freed_temporaries_alone():
    """A plan whose `run` returns int64 actions, both steps captured; then tensors of the sizes of the two temporaries the capture used
    to free -- the int32 actions (B * N elements) and the 5 x 5 float64 identity -- are allocated and filled with a sentinel, the
    graphs are replayed, and the replayed feeds must equal the use_graph=False plan's and the sentinels must be untouched.
    A regression guard, not a proof: the sentinel assertion fails on the code of before only if the allocator hands one of the freed
    blocks to a sentinel tensor, and passes trivially if it does not."""
    from cm3_amd import batch as BR
    from cm3_amd.particle import VecParticleEnv
    from cm3_amd.rollout import ParticleRollout
    N, M, K = 2, 2, 4
    R = K * N
    env = VecParticleEnv(load_cfg("particle_stage2_merge.json"), N, 0.2, 33, 8, device=DEV, dtype=torch.float32, auto_reset=True, seed=8)
    env.reset()
    ro = ParticleRollout(env, n_ticks=33, use_graph=False)
    ro.collect()
    g = torch.Generator(device=DEV).manual_seed(9)
    bufs = {"acts": torch.randint(0, 5, (R,), generator=g, device=DEV),            # int64: process_actions_device converts
            "probs": torch.rand(R, 5, generator=g, device=DEV, dtype=torch.float64),
            "q": torch.rand(R * N * 5, generator=g, device=DEV, dtype=torch.float64)}
    assert bufs["acts"].dtype == torch.int64

    def run(ops, feed):
        rows = max([v.shape[0] for v in feed.values() if torch.is_tensor(v) and v.dim() > 0] or [1])
        answer = {"action_samples_target": bufs["acts"], "probs": bufs["probs"]}
        return [None if (op.endswith("_op") or op == "list_update_target_ops") else answer.get(op, bufs["q"][:rows]) for op in ops]

    plan_g = BR.OnPolicyPhasePlan(ro, run, 0.99, 0.1, epochs=M, batch_size=K, use_graph=True)
    plan_e = BR.OnPolicyPhasePlan(ro, run, 0.99, 0.1, epochs=M, batch_size=K, use_graph=False)
    plan_g.refresh(torch.Generator(device=DEV).manual_seed(4))
    plan_e.refresh(torch.Generator(device=DEV).manual_seed(4))
    for k in range(M):                                                              # capture both steps
        plan_g.step(k)
    torch.cuda.synchronize()
    assert len(plan_g._graphs) == M
    for k in range(M):      # held next to the calls: the int32 actions, and nothing of another kind
        held = [t for t in plan_g._keep[k] if torch.is_tensor(t)]
        assert held and all(t.dtype == torch.int32 and t.numel() == R for t in held), k
    SENTINEL = 0x5A5A5A5A
    sent_i = [torch.full((R,), SENTINEL, dtype=torch.int32, device=DEV) for _ in range(6)]
    sent_f = [torch.full((5, 5), -7.25, dtype=torch.float64, device=DEV) for _ in range(6)]
    torch.cuda.synchronize()
    checked = 0
    for k in range(M):
        cg, ce = plan_g.step(k), plan_e.step(k)                                     # a replay; the eager specification
        torch.cuda.synchronize()
        assert [ops for ops, _ in cg] == [ops for ops, _ in ce]
        for (ops, fa), (_, fb) in zip(cg, ce):
            assert sorted(fa) == sorted(fb), (k, ops)
            for name in fb:
                if torch.is_tensor(fb[name]):
                    assert fa[name].dtype == fb[name].dtype and fa[name].shape == fb[name].shape, (k, ops, name)
                    assert torch.equal(fa[name], fb[name]), (k, ops, name)
                    checked += 1
    assert checked == M * 48                                                        # every tensor feed of the eleven calls
    assert all(bool((t == SENTINEL).all()) for t in sent_i) and all(bool((t == -7.25).all()) for t in sent_f)
    plan_g.close()
    plan_e.close()
    ro.close()
