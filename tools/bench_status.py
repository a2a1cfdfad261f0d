"""The status launches (gogame.batch_stone_status / batch_stone_status_tracked: k_status of gg_status.h) on positions of the
no_eye_fill policy with the ownership counts of their own playouts; prints one JSON line per configuration.

  python tools/bench_status.py [--launches 30] [--warmup 5] [--sample 8] [--boards 8192] [--plies 180] [--playouts 16]

Shapes and protocol: tools/bench_area.py's - 19x19, `--plies` plies into batch_rollout_tracked(policy='no_eye_fill', auto_reset
off) from the empty board, 8 192 boards by default, own = batch_playouts(..., `--playouts`, ownership=True,
policy='no_eye_fill') of those boards; `--warmup` launches, then `--launches` (>= 5) launches each between two events of its
own on the stream; median, min and max of the device time per launch and boards per second at the median.  Rows:
  status         per input form (byte planes, tracked boards) x dtype (uint8, float16) x plain / oriented x without / with
                 counts, into a preallocated out, threshold (2, 3)
  next to, on the same boards in the same process: batch_features[_tracked] (float16: the same chain rounds without the sums)
  and batch_area_planes[_tracked] (uint8: the same final floods without the rounds) - `ratio_to_features`, `ratio_to_area` and
  `ratio_to_both` (their sum)
There is no target: the medians and the ratios are the result.  With --sample S > 0 (needs the repository's tests/ on the
path: the expectation) the first S boards are held against tests/status_expect.py.
"""
import argparse
import json
import os
import sys

from mc_bench import ROOT   # noqa: F401  (puts the repository on sys.path)
from bench_features import per_launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--sample', type=int, default=8)
    ap.add_argument('--boards', type=int, default=8192)
    ap.add_argument('--plies', type=int, default=180)
    ap.add_argument('--playouts', type=int, default=16)
    args = ap.parse_args()
    if args.launches < 5:
        ap.error('need at least 5 timed launches')
    import torch
    from gymgo_amd import gogame, _lib
    torch.cuda.set_device(0)
    cus = int(_lib.lib().gg_device_cus())
    B, N, K, thr = args.boards, 19, args.playouts, (2, 3)
    tracked = gogame.batch_track(gogame.batch_init_state(B, N, device='cuda:0'))
    rng = gogame.rng_seed(B, 17)
    gogame.batch_rollout_tracked(tracked, rng, args.plies, auto_reset=False, policy='no_eye_fill')
    st = gogame.batch_untrack(tracked)
    own = gogame.batch_playouts(st, K, ownership=True, policy='no_eye_fill').ownership
    black_view = torch.zeros(B, dtype=torch.uint8, device='cuda:0')
    ref, ref_counts = gogame.batch_stone_status(st, own, K, thr, side=black_view, counts=True)
    stones = (st[:, 0] | st[:, 1]) != 0
    assert bool((ref[:, :6].sum(dim=1) == stones).all()) and bool((ref[:, 6:].sum(dim=1) == 1).all())
    assert bool((ref[:, 6].sum(dim=(1, 2)) == ref_counts[:, 0]).all()) and bool((ref[:, 4].sum(dim=(1, 2)) == ref_counts[:, 3]).all())
    if args.sample > 0:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import status_expect as se
        S = args.sample
        want, want_counts = se.batch_status(st[:S].cpu().numpy(), own[:S].cpu().numpy(), K, thr[0], thr[1], side=0)
        assert (want == ref[:S].cpu().numpy()).all() and (want_counts == ref_counts[:S].cpu().numpy()).all()
    orient = (torch.arange(B, device='cuda:0', dtype=torch.int32) * 3 + 1) % 8
    common = dict(size=N, boards=B, root_plies=args.plies, playouts=K, launches=args.launches, cus=cus)
    chains = lambda lo, hi: float(ref[:, lo:hi].sum()) / B
    print(json.dumps(dict(metric='status_boards', **common, mean_stones=float(stones.sum()) / B, mean_alive=chains(0, 1) + chains(3, 4),
                          mean_dead=chains(1, 2) + chains(4, 5), mean_unsettled=chains(2, 3) + chains(5, 6),
                          mean_black=float(ref_counts[:, 0].sum()) / B, mean_white=float(ref_counts[:, 1].sum()) / B,
                          mean_neutral=chains(8, 9))), flush=True)
    for form, x, status, feat, area in (('bytes', st, gogame.batch_stone_status, gogame.batch_features, gogame.batch_area_planes),
                                        ('tracked', tracked, gogame.batch_stone_status_tracked, gogame.batch_features_tracked,
                                         gogame.batch_area_planes_tracked)):
        out = torch.empty((B, 16, N, N), dtype=torch.float16, device='cuda:0')
        t = per_launch(lambda: feat(x, out=out), args.launches, args.warmup)
        feat_us = t['median_us']
        print(json.dumps(dict(metric='features_us_per_launch', input=form, dtype='float16', **common, **t,
                              boards_per_s=B / (t['median_us'] * 1e-6))), flush=True)
        out = torch.empty((B, 3, N, N), dtype=torch.uint8, device='cuda:0')
        t = per_launch(lambda: area(x, out=out), args.launches, args.warmup)
        area_us = t['median_us']
        print(json.dumps(dict(metric='area_us_per_launch', input=form, dtype='uint8', **common, **t,
                              boards_per_s=B / (t['median_us'] * 1e-6))), flush=True)
        for dt in (torch.uint8, torch.float16):
            out = torch.empty((B, 9, N, N), dtype=dt, device='cuda:0')
            cnt = torch.empty((B, 4), dtype=torch.int32, device='cuda:0')
            for o in (None, orient):
                for counts in (False, cnt):
                    t = per_launch(lambda: status(x, own, K, thr, dtype=dt, out=out, orient=o, counts=counts), args.launches, args.warmup)
                    print(json.dumps(dict(metric='status_us_per_launch', input=form, dtype=str(dt).split('.')[-1],
                                          oriented=o is not None, counts=counts is not False, **common, **t,
                                          boards_per_s=B / (t['median_us'] * 1e-6), ratio_to_features=t['median_us'] / feat_us,
                                          ratio_to_area=t['median_us'] / area_us, ratio_to_both=t['median_us'] / (feat_us + area_us))),
                          flush=True)
        del out


if __name__ == '__main__':
    main()
