"""Batched Monte Carlo playouts (gogame.batch_playouts) against the tracked rollout they are built on; prints one JSON line.

  python tools/bench_playout.py [--roots 32768] [--k 16] [--size 19] [--slots S] [--reps 3] [--policy no_eye_fill | tactical | pattern]

Workload: R empty roots x K playouts to the end of the game (komi 7.5, default slot count: 256 per CU), without and with
ownership.  Ceiling, in the same process: gg_batch_rollout_tracked on S boards x 256 plies with auto-reset (the rollout
kernel the playouts run on, at the same batch size).  Plies are the plies the playouts actually played (plies_sum).
For the split of device time between the rollout chunks and the harvest launches, run this once under
`rocprofv3 --kernel-trace --stats -- python tools/bench_playout.py --reps 1` (k_rollout* vs k_po_harvest).
--policy no_eye_fill / tactical / pattern: the playouts (without ownership) under that policy NEXT TO the uniform ones in the same run, the two
sides alternating (keys with the suffix _policy; policy_ratio_* = policy / uniform), and the tracked rollout under the policy.
--amaf: under --policy (uniform included), the tracked rollout WITHOUT auto-reset from the same boards with and without the move log
(gg_batch_rollout_tracked_log against gg_batch_rollout_tracked_policy2, 256 plies, the two sides alternating from copies:
log_plies_per_s / nolog_plies_per_s, log_ratio = with / without) and batch_playouts with amaf=True next to the plain call, alternating
(amaf_* keys; amaf_ratio_playouts_per_s = with / without).  Device-time split of the AMAF harvest: run once under
`rocprofv3 --kernel-trace --stats -- python tools/bench_playout.py --amaf --reps 1` (k_po_harvest<.., AmafArgs>).
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
    ap.add_argument('--policy', default='uniform', choices=sorted(('uniform', 'no_eye_fill', 'tactical', 'pattern')))
    ap.add_argument('--amaf', action='store_true')
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
    if args.amaf:
        pol = args.policy
        res['amaf_policy'] = pol
        # the cost of the log: 256 plies without auto-reset from the same mid-game boards (copies: the launch is in place)
        base = gogame.batch_track(gogame.batch_init_state(S, N, device='cuda:0'))
        gogame.batch_rollout_tracked(base, gogame.rng_seed(S, 5), 64, False)
        rng0 = gogame.rng_seed(S, 6)
        log = torch.empty((S, 256), dtype=torch.int16, device='cuda:0')
        steps = torch.zeros(S, dtype=torch.int64, device='cuda:0')

        def timed_launch(with_log):
            tr, rg = base.clone(), rng0.clone()
            steps.zero_()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if with_log:
                gogame.batch_rollout_tracked_log(tr, rg, 256, log, None, steps, policy=pol)
            else:
                gogame.batch_rollout_tracked(tr, rg, 256, False, None, steps, policy=pol)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e-3, int(steps.sum())

        timed_launch(True), timed_launch(False)   # warm-up
        ts = {True: [], False: []}
        for _ in range(max(3, args.reps)):
            for w in (False, True):
                ts[w].append(timed_launch(w))
        for w, tag in ((False, 'nolog'), (True, 'log')):
            t = sorted(x[0] for x in ts[w])[len(ts[w]) // 2]
            res[tag + '_seconds'] = t
            res[tag + '_plies_per_s'] = ts[w][0][1] / t
        assert ts[True][0][1] == ts[False][0][1]
        res['log_ratio'] = res['log_plies_per_s'] / res['nolog_plies_per_s']
        runs = {'plain': lambda: gogame.batch_playouts(roots, K, komi=7.5, seed=1, slots=S, chunk_plies=args.chunk, policy=pol),
                'amaf': lambda: gogame.batch_playouts(roots, K, komi=7.5, seed=1, slots=S, chunk_plies=args.chunk, policy=pol, amaf=True)}
        runs['amaf']()   # warm-up
        timed = dict(zip(runs, median_timed(*runs.values(), reps=args.reps)))   # the two sides alternating
        for k, (t, out) in timed.items():
            res['amaf_alt_seconds_' + k] = t
            res['amaf_alt_playouts_per_s_' + k] = R * K / t
            res['amaf_alt_plies_per_s_' + k] = int(out.plies_sum.sum()) / t
        assert bool((timed['plain'][1].plies_sum == timed['amaf'][1].plies_sum).all())
        res['amaf_ratio_playouts_per_s'] = res['amaf_alt_playouts_per_s_amaf'] / res['amaf_alt_playouts_per_s_plain']
        res['amaf_first_plays'] = int(timed['amaf'][1].amaf[:, :, 0].sum())
    print(json.dumps(res))


if __name__ == '__main__':
    main()
