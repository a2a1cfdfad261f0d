"""UCT tree search with several leaves per root and round (gogame.batch_uct(leaves=L)) against the one-leaf search of the same
build at the same leaf budget; prints one JSON line per (mode, root count, L).

  python tools/bench_uct_leaves.py [--roots 1 16 256 1024] [--leaves 1 4 16 64] [--budget 64] [--k 256] [--size 19]
                                   [--plies 120] [--reps 3] [--modes plain prior]

Workload: R mid-game roots (random play from the empty board, `--plies` plies), komi 7.5, default slot count, K playouts per
leaf, a fixed budget of `--budget` leaves per root: budget / L rounds of L slots.  Modes: plain, and RAVE with priors
(rave_equiv 300, prior=True).  In one process, alternating, median of `--reps` runs each:
  (a) batch_uct(roots, budget, K)                       one leaf per root and iteration;
  (b) batch_uct(roots, budget / L, K, leaves=L).
time_ratio = seconds of (a) / seconds of (b): what a caller gains at the same budget of leaves.  plies_per_s counts the plies of
the playouts that reached a tree (plies_sum): the playouts of empty slots - a collision leaves its slot and the later ones of
the root empty - are run and thrown away.  live_slots = the mean number of non-empty slots per round; ratio = plies_per_s of
(b) / of (a).  The two sides grow different trees, so their playouts differ in length (mean_plies, mean_plies_one_leaf: plies
per playout that reached a tree) and ratio differs from time_ratio by that much.  For the device-time split of
k_uct_select<RAVE, true> and k_uct_backup<RAVE, true> (side (a): <RAVE, false>), run once under `rocprofv3 --kernel-trace --stats -- python
tools/bench_uct_leaves.py --reps 1`.
"""
import argparse
import json

from mc_bench import median_timed, mid_game_roots   # (puts the repository on sys.path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--roots', type=int, nargs='+', default=[1, 16, 256, 1024])
    ap.add_argument('--leaves', type=int, nargs='+', default=[1, 4, 16, 64])
    ap.add_argument('--budget', type=int, default=64)
    ap.add_argument('--k', type=int, default=256)
    ap.add_argument('--size', type=int, default=19)
    ap.add_argument('--plies', type=int, default=120)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--modes', nargs='+', default=['plain', 'prior'], choices=['plain', 'prior'])
    args = ap.parse_args()

    import torch
    from gymgo_amd import gogame, _lib
    torch.cuda.set_device(0)
    N, K, C = args.size, args.k, args.budget
    for mode in args.modes:
        kw = dict(komi=7.5, seed=1)
        if mode == 'prior':
            kw.update(rave_equiv=300.0, prior=True)
        for R in args.roots:
            roots = mid_game_roots(R, N, args.plies)
            for L in args.leaves:
                if C % L:
                    raise SystemExit('--budget must be a multiple of every --leaves')
                T = C // L

                def run_a():
                    return gogame.batch_uct(roots, C, K, **kw)

                def run_b():
                    return gogame.batch_uct(roots, T, K, leaves=L, **kw)

                run_a()   # warm-up
                run_b()
                (sa, a), (sb, b) = median_timed(run_a, run_b, reps=args.reps)
                plies_a, plies_b = int(a.plies_sum.sum()), int(b.plies_sum.sum())
                leaves_b = int(b.root_visits.sum()) // K
                print(json.dumps({
                    'metric': 'uct_leaves_plies_per_s', 'mode': mode, 'size': N, 'roots': R, 'k': K, 'budget': C, 'leaves': L, 'rounds': T,
                    'root_plies': args.plies, 'cus': int(_lib.lib().gg_device_cus()), 'seconds_one_leaf': sa, 'seconds_leaves': sb,
                    'time_ratio': sa / sb, 'plies_per_s_one_leaf': plies_a / sa, 'plies_per_s': plies_b / sb,
                    'ratio': (plies_b / sb) / (plies_a / sa), 'mean_plies_one_leaf': plies_a / (int(a.root_visits.sum()) or 1),
                    'mean_plies': plies_b / (leaves_b * K or 1),
                    'live_slots': leaves_b / (R * T), 'evaluated_leaves': leaves_b, 'queued_rows': R * T * L,
                    'mean_nodes': float(b.nodes.float().mean()), 'mean_nodes_one_leaf': float(a.nodes.float().mean()), 'reps': args.reps}),
                    flush=True)


if __name__ == '__main__':
    main()
