"""Flat Monte Carlo (gogame.batch_move_playouts) against batch_playouts on pre-built children; prints one JSON line.

  python tools/bench_move_playout.py [--roots 256] [--k 16] [--size 19] [--plies 120] [--slots S] [--reps 3]

Workload: R mid-game roots (random play from the empty board, `--plies` plies) x K playouts after every legal first move,
komi 7.5, default slot count.  In one process, alternating, median of `--reps` runs each:
  (a) batch_move_playouts(roots, K);
  (b) batch_playouts over the padded children (batch_children, built once, not timed; its build time is reported apart)
      with first_root = 0, so that child a of root r is job row r A + a - the same numbering as (a).  Only the legal slots
      are played: every illegal slot is marked as a finished game, so it plays no ply and is harvested at once.
Both play identical playouts: the legal rows of (b) must equal (a) field for field (asserted).  Plies are the plies the
playouts played after the first move (plies_sum).  For the split of device time between the rollout chunks and the
harvest launches, run this once under `rocprofv3 --kernel-trace --stats -- python tools/bench_move_playout.py --reps 1`
(k_rollout* vs k_po_harvest<..., MpArgs>).
"""
import argparse
import json
import time

from mc_bench import median_timed, mid_game_roots   # (puts the repository on sys.path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--roots', type=int, default=256)
    ap.add_argument('--k', type=int, default=16)
    ap.add_argument('--size', type=int, default=19)
    ap.add_argument('--plies', type=int, default=120)
    ap.add_argument('--slots', type=int, default=None)
    ap.add_argument('--reps', type=int, default=3)
    args = ap.parse_args()

    import torch
    from gymgo_amd import gogame, govars, _lib
    torch.cuda.set_device(0)
    N, R, K = args.size, args.roots, args.k
    A = N * N + 1
    roots = mid_game_roots(R, N, args.plies)
    kw = dict(komi=7.5, seed=1, slots=args.slots)

    # (b)'s input: the padded children, illegal slots (all-zero boards) marked as finished games
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    kids = gogame.batch_children(roots).reshape(R * A, 6, N, N)
    ended = roots[:, govars.DONE_CHNL].reshape(R, -1).any(dim=1).bool()   # (any() of uint8 is uint8)
    legal = ((gogame.batch_valid_moves(roots) != 0) & ~ended[:, None]).reshape(-1)
    kids[~legal, govars.DONE_CHNL] = 1
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    children_bytes = R * A * 6 * N * N

    run_a = lambda: gogame.batch_move_playouts(roots, K, **kw)
    run_b = lambda: gogame.batch_playouts(kids, K, **kw)
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ref_a = run_a()   # warm-up, and (a)'s peak extra device memory (its outputs included)
    peak_a = torch.cuda.max_memory_allocated() - base
    ref_b = run_b()
    assert bool((ref_a.legal.reshape(-1) == legal).all()), 'legal mask'
    for k in ('black_wins', 'white_wins', 'draws', 'unfinished', 'margin_sum', 'plies_sum'):
        ga, gb = getattr(ref_a, k).reshape(-1), getattr(ref_b, k)
        assert bool((ga[legal] == gb[legal]).all()) and not bool(ga[~legal].any()), k
    plies = int(ref_a.plies_sum.sum())
    assert plies == int(ref_b.plies_sum[legal].sum()) == int(ref_b.plies_sum.sum())

    (sa, _), (sb, _) = median_timed(run_a, run_b, reps=args.reps)
    T = int(legal.sum())
    res = {'metric': 'move_playout_plies_per_s', 'size': N, 'roots': R, 'k': K, 'root_plies': args.plies,
           'legal_pairs': T, 'padded_pairs': R * A, 'playouts': T * K, 'cus': int(_lib.lib().gg_device_cus()),
           'mean_plies': plies / (T * K), 'seconds_move_playouts': sa, 'seconds_children_playouts': sb,
           'plies_per_s_move_playouts': plies / sa, 'plies_per_s_children_playouts': plies / sb,
           'ratio': sb / sa, 'children_build_seconds': build_s, 'children_bytes': children_bytes,
           'move_playouts_peak_extra_bytes': int(peak_a), 'outputs_equal': True, 'reps': args.reps}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
