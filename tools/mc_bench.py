"""What tools/bench_playout.py, bench_move_playout.py and bench_uct.py share: the repository on sys.path, event timing, the
(alternating) median of workloads, mid-game roots."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    """-> (seconds between two events around fn() on the current stream, fn's result)."""
    import torch
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3, out


def median_timed(*fns, reps):
    """`reps` rounds of timed(fn) for every fn in turn (alternating) -> [(median seconds, last result) per fn]."""
    times, outs = [[] for _ in fns], [None] * len(fns)
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t, outs[i] = timed(fn)
            times[i].append(t)
    return [(sorted(ts)[len(ts) // 2], out) for ts, out in zip(times, outs)]


def mid_game_roots(R, N, plies):
    """R roots on cuda:0 after `plies` plies of random play from the empty board (no auto-reset)."""
    from gymgo_amd import gogame
    roots = gogame.batch_init_state(R, N, device='cuda:0')
    return gogame.batch_rollout(roots, gogame.rng_seed(R, 17), plies, auto_reset=False)
