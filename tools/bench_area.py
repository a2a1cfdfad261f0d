"""The area launches (gogame.batch_area_planes / batch_area_planes_tracked: k_area of gg_area.h) on positions of the
no_eye_fill policy; prints one JSON line per configuration.

  python tools/bench_area.py [--launches 30] [--warmup 5] [--sample 8] [--boards 8192]

Shapes and protocol: tools/bench_hash.py's - 19x19, N^2 / 2 plies (mid-game) into batch_rollout_tracked(policy='no_eye_fill',
auto_reset off) from the empty board, 8 192 boards by default; `--warmup` launches, then `--launches` (>= 5) launches each
between two events of its own on the stream; median, min and max of the device time per launch and boards per second at the
median.  Rows:
  area           per input form (byte planes, tracked boards) x dtype (uint8, float16) x plain / oriented x without / with
                 counts, into a preallocated out
  next to, on the same boards in the same process: batch_life[_tracked] (uint8), batch_features[_tracked] (float16) and
  gg_batch_areas (the two sums alone, from byte planes)
  puct_round     one PuctSearch round (select + backup, leaves=8, 1 024 roots, features float16, a constant evaluator) without
                 and with area=True (`ratio_to_plain`)
There is no target: the medians and the ratios are the result.  With --sample S > 0 (needs the repository's tests/ on the
path: the expectation) the first S boards are held against tests/area_expect.py.
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
    args = ap.parse_args()
    if args.launches < 5:
        ap.error('need at least 5 timed launches')
    import torch
    from gymgo_amd import gogame, _lib
    torch.cuda.set_device(0)
    cus = int(_lib.lib().gg_device_cus())
    B, N = args.boards, 19
    tracked = gogame.batch_track(gogame.batch_init_state(B, N, device='cuda:0'))
    rng = gogame.rng_seed(B, 17)
    plies = N * N // 2
    gogame.batch_rollout_tracked(tracked, rng, plies, auto_reset=False, policy='no_eye_fill')
    st = gogame.batch_untrack(tracked)
    ref, ref_counts = gogame.batch_area_planes(st, side=torch.zeros(B, dtype=torch.uint8, device='cuda:0'), counts=True)
    black, white = gogame.batch_areas(st)
    assert bool((ref_counts[:, 0] == black).all()) and bool((ref_counts[:, 1] == white).all())
    assert bool((ref.sum(dim=1) == 1).all())
    if args.sample > 0:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import area_expect as ae
        assert (ae.batch_area_planes(st[:args.sample].cpu().numpy(), 0) == ref[:args.sample].cpu().numpy()).all()
    orient = (torch.arange(B, device='cuda:0', dtype=torch.int32) * 3 + 1) % 8
    common = dict(size=N, boards=B, root_plies=plies, launches=args.launches, cus=cus)
    neutral = float(ref[:, 2].sum()) / B
    print(json.dumps(dict(metric='area_boards', **common, mean_black=float(black.sum()) / B, mean_white=float(white.sum()) / B,
                          mean_neutral=neutral)), flush=True)
    t = per_launch(lambda: gogame.batch_areas(st, out=(black, white)), args.launches, args.warmup)
    sums_us = t['median_us']
    print(json.dumps(dict(metric='areas_us_per_launch', input='bytes', **common, **t, boards_per_s=B / (t['median_us'] * 1e-6))),
          flush=True)
    for form, x, area, life, feat in (('bytes', st, gogame.batch_area_planes, gogame.batch_life, gogame.batch_features),
                                      ('tracked', tracked, gogame.batch_area_planes_tracked, gogame.batch_life_tracked,
                                       gogame.batch_features_tracked)):
        out = torch.empty((B, 4, N, N), dtype=torch.uint8, device='cuda:0')
        t = per_launch(lambda: life(x, out=out), args.launches, args.warmup)
        life_us = t['median_us']
        print(json.dumps(dict(metric='life_us_per_launch', input=form, dtype='uint8', **common, **t,
                              boards_per_s=B / (t['median_us'] * 1e-6))), flush=True)
        out = torch.empty((B, 16, N, N), dtype=torch.float16, device='cuda:0')
        t = per_launch(lambda: feat(x, out=out), args.launches, args.warmup)
        feat_us = t['median_us']
        print(json.dumps(dict(metric='features_us_per_launch', input=form, dtype='float16', **common, **t,
                              boards_per_s=B / (t['median_us'] * 1e-6))), flush=True)
        for dt in (torch.uint8, torch.float16):
            out = torch.empty((B, 3, N, N), dtype=dt, device='cuda:0')
            cnt = torch.empty((B, 2), dtype=torch.int32, device='cuda:0')
            for o in (None, orient):
                for counts in (False, cnt):
                    t = per_launch(lambda: area(x, dtype=dt, out=out, orient=o, counts=counts), args.launches, args.warmup)
                    print(json.dumps(dict(metric='area_us_per_launch', input=form, dtype=str(dt).split('.')[-1],
                                          oriented=o is not None, counts=counts is not False, **common, **t,
                                          boards_per_s=B / (t['median_us'] * 1e-6), ratio_to_life=t['median_us'] / life_us,
                                          ratio_to_features=t['median_us'] / feat_us, ratio_to_areas=t['median_us'] / sums_us)),
                          flush=True)
        del out
    R, L, A = min(1024, B), 8, N * N + 1
    rounds = args.launches + args.warmup
    priors = torch.full((R * L, A), 1.0 / A, dtype=torch.float32, device='cuda:0')
    values = torch.zeros(R * L, dtype=torch.float32, device='cuda:0')
    plain = None
    for with_area in (False, True):
        search = gogame.PuctSearch(st[:R], rounds + 1, leaves=L, features=torch.float16, area=with_area)
        search.select()
        search.backup(priors, values)               # round 0 hands out the roots alone

        def one_round():
            search.select()
            search.backup(priors, values)

        t = per_launch(one_round, args.launches, args.warmup)
        plain = t['median_us'] if plain is None else plain
        print(json.dumps(dict(metric='puct_round_us', area=with_area, roots=R, leaves=L, **dict(common, boards=R * L), **t,
                              ratio_to_plain=t['median_us'] / plain)), flush=True)
        del search
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
