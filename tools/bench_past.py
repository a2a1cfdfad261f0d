"""The history-plane launches (gogame.batch_past_planes / batch_past_planes_tracked, StoneHistory.push: k_past and k_past_push
of gg_past.h; gg_puct_past inside a PuctSearch round) on positions of the no_eye_fill policy; prints one JSON line per
configuration.

  python tools/bench_past.py [--launches 30] [--warmup 5] [--sample 8] [--boards 8192]

Shapes and protocol: tools/bench_area.py's - 19x19, N^2 / 2 plies (mid-game) of batch_rollout_tracked(policy='no_eye_fill',
auto_reset off) from the empty board, 8 192 boards by default; the last seven plies are played one at a time with a
StoneHistory.push_tracked in front of each, so every ring holds the board's true last seven positions.  `--warmup` launches,
then `--launches` (>= 5) launches each between two events of its own on the stream; median, min and max of the device time
per launch and boards per second at the median.  Rows:
  past           T = 8 without / with moves (16 / 23 planes) x input form (byte planes, tracked boards) x dtype (uint8,
                 float16) x plain / oriented, into a preallocated out
  push           one push of the current positions, per input form
  next to, on the same boards in the same process: batch_features[_tracked] (float16)
  puct_round     one PuctSearch round (select + backup, leaves=8, 1 024 roots, features float16, a constant evaluator) without
                 and with past= (`ratio_to_plain`)
There is no target: the medians and the ratios are the result.  With --sample S > 0 (needs the repository's tests/ on the
path: the expectation) the first S boards are held against tests/past_expect.py.
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
    B, N, T = args.boards, 19, gogame.PAST_MAX_POSITIONS
    tracked = gogame.batch_track(gogame.batch_init_state(B, N, device='cuda:0'))
    rng = gogame.rng_seed(B, 17)
    plies = N * N // 2
    gogame.batch_rollout_tracked(tracked, rng, plies - (T - 1), auto_reset=False, policy='no_eye_fill')
    hist = {moves: gogame.StoneHistory(B, N, T, moves, device='cuda:0') for moves in (False, True)}
    earlier = []
    for _ in range(T - 1):
        earlier.append(gogame.batch_untrack(tracked[:max(args.sample, 1)]).cpu().numpy())
        for h in hist.values():
            h.push_tracked(tracked)
        gogame.batch_rollout_tracked(tracked, rng, 1, auto_reset=False, policy='no_eye_fill')
    st = gogame.batch_untrack(tracked)
    ref = gogame.batch_past_planes(st, hist[True])
    assert bool((ref == gogame.batch_past_planes_tracked(tracked, hist[True])).all())
    assert bool((ref[:, 2 * T:].sum(dim=(2, 3)) <= 1).all())            # a move plane holds one point, or none for a pass
    if args.sample > 0:
        import numpy as np
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import past_expect as pe
        now = st[:args.sample].cpu().numpy()
        for b in range(args.sample):
            seq = np.stack([e[b] for e in earlier] + [now[b]])
            assert (pe.planes(seq, T, True) == ref[b].cpu().numpy()).all(), b
    orient = (torch.arange(B, device='cuda:0', dtype=torch.int32) * 3 + 1) % 8
    common = dict(size=N, boards=B, root_plies=plies, launches=args.launches, cus=cus)
    print(json.dumps(dict(metric='past_boards', **common, positions=T,
                          mean_moves_on_board=float(ref[:, 2 * T:].sum()) / B)), flush=True)
    for form, x, past, feat in (('bytes', st, gogame.batch_past_planes, gogame.batch_features),
                                ('tracked', tracked, gogame.batch_past_planes_tracked, gogame.batch_features_tracked)):
        out = torch.empty((B, 16, N, N), dtype=torch.float16, device='cuda:0')
        t = per_launch(lambda: feat(x, out=out), args.launches, args.warmup)
        feat_us = t['median_us']
        print(json.dumps(dict(metric='features_us_per_launch', input=form, dtype='float16', **common, **t,
                              boards_per_s=B / (t['median_us'] * 1e-6))), flush=True)
        scratch = gogame.StoneHistory(B, N, T, False, device='cuda:0')
        push = scratch.push_tracked if form == 'tracked' else scratch.push
        t = per_launch(lambda: push(x), args.launches, args.warmup)
        print(json.dumps(dict(metric='past_push_us_per_launch', input=form, **common, **t,
                              boards_per_s=B / (t['median_us'] * 1e-6))), flush=True)
        for moves in (False, True):
            for dt in (torch.uint8, torch.float16):
                out = torch.empty((B, hist[moves].planes, N, N), dtype=dt, device='cuda:0')
                for o in (None, orient):
                    t = per_launch(lambda: past(x, hist[moves], dtype=dt, out=out, orient=o), args.launches, args.warmup)
                    print(json.dumps(dict(metric='past_us_per_launch', input=form, positions=T, moves=moves, planes=hist[moves].planes,
                                          dtype=str(dt).split('.')[-1], oriented=o is not None, **common, **t,
                                          boards_per_s=B / (t['median_us'] * 1e-6), ratio_to_features=t['median_us'] / feat_us)),
                          flush=True)
        del out
    R, L, A = min(1024, B), 8, N * N + 1
    rounds = args.launches + args.warmup
    priors = torch.full((R * L, A), 1.0 / A, dtype=torch.float32, device='cuda:0')
    values = torch.zeros(R * L, dtype=torch.float32, device='cuda:0')
    plain = None
    for with_past in (False, True):
        roots_past = None
        if with_past:
            roots_past = gogame.StoneHistory(R, N, T, True, device='cuda:0')
            roots_past.rows.copy_(hist[True].rows[:R])
            roots_past.count.copy_(hist[True].count[:R])
        search = gogame.PuctSearch(st[:R], rounds + 1, leaves=L, features=torch.float16, past=roots_past)
        search.select()
        search.backup(priors, values)               # round 0 hands out the roots alone

        def one_round():
            search.select()
            search.backup(priors, values)

        t = per_launch(one_round, args.launches, args.warmup)
        plain = t['median_us'] if plain is None else plain
        print(json.dumps(dict(metric='puct_round_us', past=with_past, roots=R, leaves=L, **dict(common, boards=R * L), **t,
                              ratio_to_plain=t['median_us'] / plain)), flush=True)
        del search
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
