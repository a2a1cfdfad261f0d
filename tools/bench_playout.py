"""Batched Monte Carlo playouts (gogame.batch_playouts) against the tracked rollout they are built on; prints one JSON line.

  python tools/bench_playout.py [--roots 32768] [--k 16] [--size 19] [--slots S] [--reps 3] [--policy no_eye_fill | tactical]

Workload: R empty roots x K playouts to the end of the game (komi 7.5, default slot count: 256 per CU), without and with
ownership.  Ceiling, in the same process: gg_batch_rollout_tracked on S boards x 256 plies with auto-reset (the rollout
kernel the playouts run on, at the same batch size).  Plies are the plies the playouts actually played (plies_sum).
For the split of device time between the rollout chunks and the harvest launches, run this once under
`rocprofv3 --kernel-trace --stats -- python tools/bench_playout.py --reps 1` (k_rollout* vs k_po_harvest).
--policy no_eye_fill / tactical: the playouts (without ownership) under that policy NEXT TO the uniform ones in the same run, the two
sides alternating (keys with the suffix _policy; policy_ratio_* = policy / uniform), and the tracked rollout under the policy.
"""
import argparse
import json

from mc_bench import median_timed   # (puts the repository on sys.path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--roots', type=int, default=32768)
    ap.add_argument('--k', type=int, default=16)
    ap.add_argument('--size', type=int, default=19)
    ap.add_argument('--slots', type=int, default=None)
    ap.add_argument('--chunk', type=int, default=32)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--policy', default='uniform', choices=sorted(('uniform', 'no_eye_fill', 'tactical')))
    args = ap.parse_args()

    import torch
    from gymgo_amd import gogame, _lib
    torch.cuda.set_device(0)
    N, R, K = args.size, args.roots, args.k
    cus = int(_lib.lib().gg_device_cus())
    S = min(args.slots or 256 * cus, R * K)
    roots = gogame.batch_init_state(R, N, device='cuda:0')

    # ceiling: the tracked rollout on S boards, 256 plies per launch, auto-reset
    tracked = gogame.batch_track(gogame.batch_init_state(S, N, device='cuda:0'))
    rng = gogame.rng_seed(S, 3)
    gogame.batch_rollout_tracked(tracked, rng, 256)   # warm-up (and mid-game boards)
    (t_roll, _), = median_timed(lambda: gogame.batch_rollout_tracked(tracked, rng, 256), reps=args.reps)
    ceiling = S * 256 / t_roll

    res = {'metric': 'playout_plies_per_s', 'size': N, 'roots': R, 'k': K, 'slots': S, 'chunk_plies': args.chunk, 'cus': cus,
           'tracked_rollout_plies_per_s': ceiling}
    for own in (False, True):
        run = lambda: gogame.batch_playouts(roots, K, komi=7.5, seed=1, slots=S, chunk_plies=args.chunk, ownership=own)
        run()   # warm-up
        (t, out), = median_timed(run, reps=args.reps)
        plies = int(out.plies_sum.sum())
        tag = '_own' if own else ''
        res['seconds' + tag] = t
        res['playouts_per_s' + tag] = R * K / t
        res['plies_per_s' + tag] = plies / t
        res['ratio_to_tracked' + tag] = plies / t / ceiling
        if not own:
            res['mean_plies'] = plies / (R * K)
            res['unfinished'] = int(out.unfinished.sum())
            res['black_win_rate'] = int(out.black_wins.sum()) / (R * K)
    if args.policy != 'uniform':
        pol = args.policy
        res['policy'] = pol
        gogame.batch_rollout_tracked(tracked, rng, 256, policy=pol)
        (t_pol, _), = median_timed(lambda: gogame.batch_rollout_tracked(tracked, rng, 256, policy=pol), reps=args.reps)
        res['tracked_rollout_plies_per_s_policy'] = S * 256 / t_pol
        runs = {'': lambda: gogame.batch_playouts(roots, K, komi=7.5, seed=1, slots=S, chunk_plies=args.chunk),
                '_policy': lambda: gogame.batch_playouts(roots, K, komi=7.5, seed=1, slots=S, chunk_plies=args.chunk, policy=pol)}
        runs['_policy']()   # warm-up
        timed = dict(zip(runs, median_timed(*runs.values(), reps=args.reps)))   # the two sides alternating
        for k, (t, out) in timed.items():
            plies = int(out.plies_sum.sum())
            res['alt_seconds' + k] = t
            res['alt_playouts_per_s' + k] = R * K / t
            res['alt_plies_per_s' + k] = plies / t
            res['alt_mean_plies' + k] = plies / (R * K)
            res['alt_unfinished' + k] = int(out.unfinished.sum())
        res['black_win_rate_policy'] = int(timed['_policy'][1].black_wins.sum()) / (R * K)
        res['policy_ratio_plies_per_s'] = res['alt_plies_per_s_policy'] / res['alt_plies_per_s']
        res['policy_ratio_playouts_per_s'] = res['alt_playouts_per_s_policy'] / res['alt_playouts_per_s']
    print(json.dumps(res))


if __name__ == '__main__':
    main()
