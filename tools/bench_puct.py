"""PUCT tree search (gogame.batch_puct): the cost of the tree per iteration, and the search with the playout evaluator against
batch_uct at the same R, I, K; prints one JSON line per configuration.

  python tools/bench_puct.py --evaluator null [--roots 1024 16384] [--iters 64 800] [--size 19] [--plies 120] [--reps 3]
  python tools/bench_puct.py --evaluator playouts [--roots 256 1024] [--k 256] [--iters 64] ...

Workload: R mid-game roots (random play from the empty board, `--plies` plies), komi 7.5.
  null:      the evaluator returns the same preallocated priors (1 / A everywhere) and values (0) every time - no evaluator
             work, so an iteration is k_puct_select, the one-move step, untrack, the legality mask (a few torch kernels) and
             k_puct_backup plus the host loop around them.  us_per_iteration is wall time (events on the stream) of
             batch_puct / I, gg_puct_begin's memsets included (begin_ms: measured on its own); median of `--reps` runs.
             For the device time per kernel run it once under `rocprofv3 --kernel-trace --stats -- python
             tools/bench_puct.py --evaluator null --reps 1 --roots R --iters I`.
  playouts:  batch_puct with gogame.playout_evaluator(K) and batch_uct(roots, I, K) alternate in one process, median of
             `--reps` runs each; ratio = PUCT iterations/s over UCT iterations/s.  The two searches grow different trees, so
             plies/s of both are reported too.
"""
import argparse
import json

from mc_bench import median_timed, mid_game_roots, timed   # (puts the repository on sys.path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--evaluator', choices=['null', 'playouts'], default='null')
    ap.add_argument('--roots', type=int, nargs='+', default=None)
    ap.add_argument('--iters', type=int, nargs='+', default=None)
    ap.add_argument('--k', type=int, default=256)
    ap.add_argument('--size', type=int, default=19)
    ap.add_argument('--plies', type=int, default=120)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--c', type=float, default=1.25)
    args = ap.parse_args()

    import torch
    from gymgo_amd import gogame, _lib
    torch.cuda.set_device(0)
    N, K, A = args.size, args.k, args.size * args.size + 1
    null = args.evaluator == 'null'
    for R in args.roots or ([1024, 16384] if null else [256, 1024]):
        roots = mid_game_roots(R, N, args.plies)
        for I in args.iters or ([64, 800] if null else [64]):
            base = {'size': N, 'roots': R, 'iterations': I, 'root_plies': args.plies, 'c': args.c,
                    'cus': int(_lib.lib().gg_device_cus()), 'reps': args.reps}
            if null:
                priors = torch.full((R, A), 1.0 / A, dtype=torch.float32, device='cuda:0')
                values = torch.zeros(R, dtype=torch.float32, device='cuda:0')
                run = lambda: gogame.batch_puct(roots, I, lambda states, legal: (priors, values), c=args.c, komi=7.5, tree=True)
                ref = run()   # warm-up
                assert bool((ref.root_visits == I).all())
                (s, out), = median_timed(run, reps=args.reps)
                sb, _ = timed(lambda: gogame.PuctSearch(roots, I, c=args.c, komi=7.5))
                depth = _mean_leaf_depth(out.tree.parent, out.nodes)
                res = dict(base, metric='puct_wall_us_per_iteration', evaluator='null', seconds=s, begin_ms=sb * 1e3,
                           us_per_iteration=s / I * 1e6, us_per_iteration_without_begin=(s - sb) / I * 1e6,
                           mean_nodes=float(out.nodes.float().mean()), mean_node_depth=depth,
                           tree_bytes=R * (I + 1) * (4 * (5 * N + 1) + 8 * A + 24))
            else:
                kw = dict(komi=7.5)
                evs = []

                def run_a():
                    evs.append(gogame.playout_evaluator(K, seed=1, **kw))
                    return gogame.batch_puct(roots, I, evs[-1], c=args.c, **kw)

                def run_b():
                    return gogame.batch_uct(roots, I, K, seed=1, **kw)

                ref = run_a()   # warm-up
                run_b()
                assert bool((ref.root_visits == I).all())
                (sa, pa), (sb, ub) = median_timed(run_a, run_b, reps=args.reps)
                plies_a, plies_b = int(evs[-1].plies_sum), int(ub.plies_sum.sum())
                P = R * K * I
                res = dict(base, metric='puct_iterations_per_s', evaluator='playouts', k=K, playouts=P,
                           jobs_per_slot=R * K / (256 * base['cus']), seconds_puct=sa, seconds_uct=sb,
                           iterations_per_s=I / sa, iterations_per_s_uct=I / sb, ratio=sb / sa,
                           plies_per_s=plies_a / sa, plies_per_s_uct=plies_b / sb, ratio_plies=(plies_a / sa) / (plies_b / sb),
                           mean_plies_puct=plies_a / P, mean_plies_uct=plies_b / P,
                           mean_nodes=float(pa.nodes.float().mean()), mean_nodes_uct=float(ub.nodes.float().mean()))
            print(json.dumps(res), flush=True)


def _mean_leaf_depth(parent, nodes):
    """Mean depth of the nodes in use (the root at 0), from the parent links: how deep the walks of the search went."""
    import torch
    R, NN = parent.shape
    depth = torch.zeros((R, NN), dtype=torch.int64, device=parent.device)
    for x in range(1, NN):   # (parents have smaller ids)
        depth[:, x] = torch.gather(depth, 1, parent[:, x].clamp(min=0).long()[:, None])[:, 0] + 1
    used = torch.arange(NN, device=parent.device)[None, :] < nodes[:, None]
    return float((depth * used).sum() / used.sum().clamp(min=1))


if __name__ == '__main__':
    main()
