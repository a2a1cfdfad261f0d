"""UCT tree search (gogame.batch_uct) against I back-to-back batch_playouts calls of the same R and K; prints one JSON line per
root count.

  python tools/bench_uct.py [--roots 256 1024] [--k 256] [--iters 64] [--size 19] [--plies 120] [--reps 3]

Workload: R mid-game roots (random play from the empty board, `--plies` plies), komi 7.5, default slot count, I iterations
of K playouts per leaf.  In one process, alternating, median of `--reps` runs each:
  (a) batch_uct(roots, I, K);
  (b) I calls of batch_playouts(roots, K, seed=i): the same playout volume with no tree (the roots as leaves).
ratio = time (b) / time (a) per playout: what the select, one-move step and backup launches - and the host loop around
them - cost on top of the playouts (1.0: nothing).  Both drain the playout queue once per iteration.  Plies are the plies
the playouts played (plies_sum).  For the device-time split of k_uct_select<RAVE, false>, the one-move step
(k_play_moves*) and k_uct_backup<RAVE, false>, run once under `rocprofv3 --kernel-trace --stats -- python tools/bench_uct.py --reps 1`.
--rave-equiv K: a third side in the same alternation, (c) batch_uct(roots, I, K, rave_equiv=K) - keys with the suffix _rave,
rave_ratio = iterations/s with RAVE / plain, and the mean depth of the deepest node per tree on both sides.
"""
import argparse
import json

from mc_bench import median_timed, mid_game_roots   # (puts the repository on sys.path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--roots', type=int, nargs='+', default=[256, 1024])
    ap.add_argument('--k', type=int, default=256)
    ap.add_argument('--iters', type=int, default=64)
    ap.add_argument('--size', type=int, default=19)
    ap.add_argument('--plies', type=int, default=120)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--rave-equiv', type=float, default=None)
    args = ap.parse_args()

    import torch
    from gymgo_amd import gogame, _lib
    torch.cuda.set_device(0)
    N, K, I = args.size, args.k, args.iters
    for R in args.roots:
        roots = mid_game_roots(R, N, args.plies)
        kw = dict(komi=7.5)

        def run_a():
            return gogame.batch_uct(roots, I, K, seed=1, **kw)

        def run_b():
            return [gogame.batch_playouts(roots, K, seed=i, **kw) for i in range(I)]

        ref = run_a()   # warm-up
        run_b()
        assert bool((ref.root_visits == I * K).all())
        plies_a = int(ref.plies_sum.sum())
        (sa, _), (sb, outs) = median_timed(run_a, run_b, reps=args.reps)
        plies_b = sum(int(o.plies_sum.sum()) for o in outs)
        P = R * K * I
        res = {'metric': 'uct_playouts_per_s', 'size': N, 'roots': R, 'k': K, 'iterations': I, 'root_plies': args.plies,
               'playouts': P, 'cus': int(_lib.lib().gg_device_cus()), 'jobs_per_slot': R * K / (256 * int(_lib.lib().gg_device_cus())),
               'seconds_uct': sa, 'seconds_playouts': sb, 'iterations_per_s': I / sa, 'playouts_per_s': P / sa,
               'plies_per_s': plies_a / sa, 'mean_plies_uct': plies_a / P, 'playouts_per_s_plain': P / sb,
               'plies_per_s_plain': plies_b / sb, 'mean_plies_plain': plies_b / P,
               'ratio': (P / sa) / (P / sb), 'ratio_plies': (plies_a / sa) / (plies_b / sb),
               'mean_nodes': float(ref.nodes.float().mean()), 'reps': args.reps}
        if args.rave_equiv is not None:
            def run_c():
                return gogame.batch_uct(roots, I, K, seed=1, rave_equiv=args.rave_equiv, **kw)

            def depth(parent):   # the deepest node of every tree: parents have smaller ids
                d = torch.zeros_like(parent)
                for x in range(1, parent.shape[1]):
                    p = parent[:, x]
                    d[:, x] = torch.where(p >= 0, torch.gather(d, 1, p.clamp(min=0).long()[:, None])[:, 0] + 1, torch.zeros_like(p))
                return float(d.max(dim=1).values.float().mean())

            rv = run_c()   # warm-up
            assert bool((rv.root_visits == I * K).all())
            (sa2, _), (sc, out_c) = median_timed(run_a, run_c, reps=args.reps)
            res.update(rave_equiv=args.rave_equiv, seconds_uct_alt=sa2, seconds_rave=sc, iterations_per_s_rave=I / sc,
                       playouts_per_s_rave=P / sc, rave_ratio=sa2 / sc, mean_nodes_rave=float(out_c.nodes.float().mean()),
                       mean_plies_rave=int(out_c.plies_sum.sum()) / P,
                       mean_depth=depth(gogame.batch_uct(roots, I, K, seed=1, tree=True, **kw).tree.parent),
                       mean_depth_rave=depth(gogame.batch_uct(roots, I, K, seed=1, tree=True, rave_equiv=args.rave_equiv, **kw).tree.parent))
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
