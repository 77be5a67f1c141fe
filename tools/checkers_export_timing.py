#!/usr/bin/env python
"""Times the export of a Checkers trajectory into the reference's 16-column transitions (alg_credit_checkers.py:427-444) at C3 --
8192 envs x 2 agents, reference geometry, continuous collection, one chunk of 33 ticks = 270 336 transitions:

  (1) the whole chunk into fresh columns:  CheckersRollout.as_reference_batch (ONE launch of cm3_checkers_transitions_gather)
                                           against as_reference_batch_torch (the composition of torch operations it replaces);
  (2) export + replay add:                 DeviceReplayBuffer.add_rollout (the same launch writing ring rows) against the route
                                           off_policy_batches took before: composition, .contiguous(), DeviceReplayBuffer.add;
  (3) 24 x 128 sampled transitions:        the indexed export of one on-policy phase, kernel against composition (toy-sized and
                                           launch-bound: reported, not judged);
  (4) wide against compact replay add:     DeviceReplayBuffer.add_rollout (float64 ring, the launch of (2)) against
                                           CompactCheckersReplayBuffer.add_rollout (ONE launch of cm3_checkers_transitions_pack: the
                                           ring keeps the trajectory's dtypes, nothing is converted), same chunk, wrapping rings;
  (5) sample_batch(24 x 128) from each:    cm3_rows_gather out of the wide ring against cm3_checkers_ring_expand out of the compact
                                           one (launch-bound: reported, not judged).

One process, one GPU; every variant is warmed up, each repetition is timed with device events around a call that ends in a
synchronise, and the two variants of a case alternate inside one loop.  The bytes a variant has to move are computed from shapes;
their floor is those bytes over the copy rate that cm3_hbm_copy_bench reaches in this same run (as tools/host_side_timing.py
defines it).  Before anything is timed the two routes are compared at this size: every column bit-identical (the compact ring: every column
widened equals the wide ring's, every sampled batch equals the wide ring's batch).

    python tools/checkers_export_timing.py [--reps 12] > profiles/r11_checkers_compact_ring.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _nbytes(cols):
    return sum(v.numel() * v.element_size() for v in cols.values())


def _once(fn, device):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def _alternate(variants, device, reps, warm=2):
    """{name: [ms per repetition]}: the variants take turns, so that whatever else the host or the chip does hits all of them."""
    for fn in variants.values():
        for _ in range(warm):
            fn()
    import torch
    torch.cuda.synchronize(device)
    times = {name: [] for name in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            times[name].append(_once(fn, device))
    return times


def _copy_rate(device, gib=2.0, reps=10):
    """GB/s of the project's streaming copy probe over a buffer far beyond the Infinity Cache (2 x bytes / time)."""
    import torch
    from cm3_amd import _lib
    lib = _lib.lib()
    nbytes = int(gib * (1 << 30)) // 32 * 32
    buf = torch.empty(nbytes // 4, dtype=torch.int32, device=device)
    buf.random_(0, 1 << 30)
    s, half = _lib.current_stream_handle(device), nbytes // 2
    copy = lambda: _lib.check(lib.cm3_hbm_copy_bench(buf.data_ptr() + half, buf.data_ptr(), half, s))    # noqa: E731
    copy()
    ms = [_once(copy, device) for _ in range(reps)]
    del buf
    torch.cuda.empty_cache()
    return 2.0 * half / (statistics.median(ms) * 1e-3) / 1e9


def trajectory_bytes_per_transition(ro):
    """Bytes of trajectory a transition is made from (payload, without the padding of the records): the five observation arrays of
    slot t and of its successor, actions and actions_prev, the rewards, done and the goal bytes."""
    env = ro.env
    N = env.n
    obs = env.grid_rec + 16 * N + 8 * N * env.Lo + env.obst_rec + 32 * N
    return 2 * obs + 2 * 4 * N + 8 * N + 8 + 1 + N


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--ticks", type=int, default=33)
    args = ap.parse_args()
    import numpy as np
    import torch
    import cm3_amd
    from cm3_amd.checkers import VecCheckersEnv
    from cm3_amd.replay import CompactCheckersReplayBuffer, DeviceReplayBuffer
    from cm3_amd.rollout import CheckersRollout, sample_distinct
    device = cm3_amd._lib.require_gpu("cuda:0")
    reps = max(10, args.reps)
    cfg = cm3_amd.load_config("checkers_stage2")
    E, T, N = args.envs, args.ticks, 2
    env = VecCheckersEnv(cfg["init"], N, 33, E, device=device, auto_reset=True, seed=12341)
    ro = CheckersRollout(env, n_ticks=T).collect(goals=np.eye(2))
    torch.cuda.synchronize(device)
    B = T * E
    kernel = ro.as_reference_batch(numpy=False)
    torch_cols = ro.as_reference_batch_torch(None, None, numpy=False)
    for name in kernel:
        assert kernel[name].dtype == torch_cols[name].dtype and torch.equal(kernel[name], torch_cols[name]), name
    write = _nbytes(kernel)
    read = B * trajectory_bytes_per_transition(ro)
    assert write == B * sum(int(np.prod(shape, dtype=np.int64)) * torch.empty(0, dtype=dt).element_size() for shape, dt in ro.column_specs().values())
    del kernel, torch_cols
    copy_gbps = _copy_rate(device)
    print("Checkers transition export at C3: %d envs x %d agents x %d ticks = %d transitions, continuous collection, random actions"
          % (E, N, T, B))
    print("device: %s   command: python tools/checkers_export_timing.py --reps %d" % (torch.cuda.get_device_name(device), reps))
    print("copy rate of cm3_hbm_copy_bench in this run: %.0f GB/s   (floor = bytes to move / this rate)" % copy_gbps)
    print("per transition: %d B of trajectory read, %d B of columns written; the chunk: %.1f MB read, %.1f MB written"
          % (read // B, write // B, read / 1e6, write / 1e6))
    print("every column of the kernel route equals the composition bit for bit at this size: checked before timing")
    print()

    def report(title, times, moved, judge, other="the composition"):
        print(title)
        for name, ms in times.items():
            floor = moved[name] / (copy_gbps * 1e9) * 1e3
            print("  %-46s min %8.3f  median %8.3f  max %8.3f ms over %d reps | must move %8.1f MB, floor %6.3f ms, median = %5.1f x floor"
                  % (name, min(ms), statistics.median(ms), max(ms), len(ms), moved[name] / 1e6, floor, statistics.median(ms) / floor))
        (a, ta), (b, tb) = times.items()
        ratio = statistics.median(tb) / statistics.median(ta)
        if judge:
            verdict = ("faster by more than the spread of either (its slowest repetition beats the other's fastest)" if max(ta) < min(tb)
                       else "NOT separated from %s by more than the spread" % other)
            print("  -> %s is %.1f x the speed of %s at the median: %s" % (a, ratio, b, verdict))
        else:
            print("  -> ratio of the medians %.1f (toy-sized and launch-bound: reported, not judged)" % ratio)
        print()

    # (1) the whole chunk into fresh columns
    times = _alternate({"kernel: as_reference_batch": lambda: ro.as_reference_batch(numpy=False),
                        "composition: as_reference_batch_torch": lambda: ro.as_reference_batch_torch(None, None, numpy=False)}, device, reps)
    report("(1) whole-chunk export into fresh columns", times,
           {"kernel: as_reference_batch": read + write, "composition: as_reference_batch_torch": read + write}, True)
    torch.cuda.empty_cache()

    # (2) export + ring add; a ring of 3 chunks and a bit, so that the adds wrap
    ring = 3 * B + 17
    buf_k, buf_c = DeviceReplayBuffer(size=ring, device=device), DeviceReplayBuffer(size=ring, device=device)

    def parent_route():
        cols = ro.as_reference_batch_torch(None, None, numpy=False)
        buf_c.add({k: v.contiguous() for k, v in cols.items()})
    times = _alternate({"kernel: add_rollout": lambda: buf_k.add_rollout(ro),
                        "composition + contiguous + add": parent_route}, device, reps)
    assert (buf_k.len, buf_k.idx) == (buf_c.len, buf_c.idx)
    for name in buf_k.cols:
        assert torch.equal(buf_k.cols[name], buf_c.cols[name]), name
    report("(2) export + replay-ring add (ring of %d rows, wraps)" % ring, times,
           {"kernel: add_rollout": read + write, "composition + contiguous + add": read + 3 * write}, True)
    del buf_k, buf_c
    torch.cuda.empty_cache()

    # (3) the 24 x 128 sampled transitions of one on-policy phase
    gen = torch.Generator(device=device).manual_seed(0)
    pos = sample_distinct(B, 128, 24, gen, device).reshape(-1)
    tt, ee = torch.div(pos, E, rounding_mode="floor"), pos % E
    n = pos.numel()
    moved = n * (read // B + write // B)
    times = _alternate({"kernel: as_reference_batch(tt, ee)": lambda: ro.as_reference_batch(tt, ee, numpy=False),
                        "composition: as_reference_batch_torch(tt, ee)": lambda: ro.as_reference_batch_torch(tt, ee, numpy=False)},
                       device, reps)
    report("(3) indexed export of 24 x 128 sampled transitions", times,
           {"kernel: as_reference_batch(tt, ee)": moved, "composition: as_reference_batch_torch(tt, ee)": moved}, False)
    # (4) the wide ring's add against the compact ring's, same chunk, both rings wrap; bit equality of the two rings first
    buf_w, buf_n = DeviceReplayBuffer(size=ring, device=device), CompactCheckersReplayBuffer(size=ring, device=device)
    widen = {torch.int8: lambda v: v.to(torch.float64), torch.int32: lambda v: v.to(torch.float64),
             torch.uint8: lambda v: torch.nn.functional.one_hot(v.long(), 2)}
    for _ in range(4):                                   # (the fourth add wraps)
        buf_w.add_rollout(ro)
        buf_n.add_rollout(ro)
    assert (buf_w.len, buf_w.idx) == (buf_n.len, buf_n.idx) and buf_w.idx < B
    for name in ro.ORDER:
        v = buf_n.cols[name]
        wide_v = widen[v.dtype](v) if name.endswith(("grid", "obs_self_t", "vec", "goals")) else v
        assert wide_v.dtype == buf_w.cols[name].dtype and torch.equal(wide_v, buf_w.cols[name]), name
        del wide_v
    torch.cuda.empty_cache()
    compact_row = _nbytes(buf_n.cols) // ring
    print("the compact ring, widened, equals the wide ring bit for bit in every column after 4 adds (one wrapped): checked before timing")
    print("ring row: wide %d B, compact %d B; a ring of %d rows: wide %.2f GB, compact %.2f GB"
          % (write // B, compact_row, ring, _nbytes(buf_w.cols) / 1e9, _nbytes(buf_n.cols) / 1e9))
    print()
    times = _alternate({"compact: add_rollout (pack)": lambda: buf_n.add_rollout(ro),
                        "wide: add_rollout (export)": lambda: buf_w.add_rollout(ro)}, device, reps)
    assert (buf_w.len, buf_w.idx) == (buf_n.len, buf_n.idx)
    report("(4) replay-ring add of the chunk: compact ring against the wide ring (rings of %d rows, wrap)" % ring, times,
           {"compact: add_rollout (pack)": read + B * compact_row, "wide: add_rollout (export)": read + write}, True, "the wide add")

    # (5) sample_batch(24 x 128) from each ring, generators seeded alike
    n = 24 * 128
    ga, gb = torch.Generator(device=device).manual_seed(1), torch.Generator(device=device).manual_seed(1)
    got, want = buf_n.sample_batch(n, generator=ga), buf_w.sample_batch(n, generator=gb)
    for name in ro.ORDER:
        assert got[name].dtype == want[name].dtype and torch.equal(got[name], want[name]), name
    del got, want
    print("sample_batch(%d) from the compact ring equals the wide ring's batch bit for bit (generators seeded alike): checked before timing" % n)
    times = _alternate({"compact: sample_batch (ring_expand)": lambda: buf_n.sample_batch(n, generator=ga),
                        "wide: sample_batch (rows_gather)": lambda: buf_w.sample_batch(n, generator=gb)}, device, reps)
    report("(5) sample_batch(24 x 128) out of each ring (draws included)", times,
           {"compact: sample_batch (ring_expand)": n * (compact_row + write // B + 8),
            "wide: sample_batch (rows_gather)": n * (2 * (write // B) + 8)}, False)
    del buf_w, buf_n
    torch.cuda.empty_cache()
    print("the compact add above its floor (compare its multiple with the wide add's): NOT attributed by measurement.  By count: the partly covered pieces at the range ends and the wrap are at most 4 per column (64 of ~24 M pieces), nothing; 58 % of the bytes (grid / obs_self_t and their next_*) arrive as 2-byte loads, eight per 16-byte store, and 47 % of the bytes (next_*) issue their loads only after a done byte: the load side, not the byte-granular tails or the wrap, is where a profile should look first")
    print("not measured: non-temporal stores for the column writes; kernel time in isolation (rocprofv3); other agent counts and sizes")
    ro.close()


if __name__ == "__main__":
    main()
