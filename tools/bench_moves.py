"""The move-outcome launches (gogame.batch_move_planes / batch_move_planes_tracked / batch_move_counts: k_moves of gg_moves.h)
on positions of the no_eye_fill policy; prints one JSON line per configuration.

  python tools/bench_moves.py [--launches 30] [--warmup 5] [--sample 16]
  LIB=tools/exp/libgymgo_ab.so python tools/bench_moves.py      # another build of the library (make ab), for an A/B

Shapes and protocol: tools/bench_ladder.py's - 19x19 and 9x9 at 65 536 boards; dtypes uint8 and float16; tracked and
byte-plane input; N^2 / 2 (mid-game) and N^2 plies into batch_rollout_tracked(policy='no_eye_fill', auto_reset off) from the
empty board; `--warmup` launches, then `--launches` (>= 5) launches each between two events of its own on the stream;
median, min and max of the device time per launch and boards per second at the median.  Next to it, on the same boards in
the same process:
  features_us   gg_batch_features_tracked (float16) - the launch the search queues before this one
  ladder_us     gg_batch_ladder_tracked (uint8)
  groups_us     gg_batch_group_liberties - one flood pair per group: the group rounds this launch starts with
There is no target: the medians and the ratios are the result.  `candidates` / `exact` are the per-board means of the
candidate points and of those among them that capture or join two own chains (the points that take the flood per
candidate), from the launch's own counts and feature planes.  With --sample S > 0 (needs the repository's tests/ on the
path: the expectation) the first S boards are held against tests/outcome_expect.py.
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
    ap.add_argument('--sample', type=int, default=16)
    ap.add_argument('--boards', type=int, default=65536)
    args = ap.parse_args()
    if args.launches < 5:
        ap.error('need at least 5 timed launches')
    import torch
    from gymgo_amd import gogame, _lib
    if os.environ.get('LIB'):
        _lib.LIB_PATH = os.path.join(ROOT, os.environ['LIB'])
    torch.cuda.set_device(0)
    cus = int(_lib.lib().gg_device_cus())
    if args.sample > 0:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import outcome_expect as oe
    B = args.boards
    for N in (19, 9):
        tracked = gogame.batch_track(gogame.batch_init_state(B, N, device='cuda:0'))
        rng = gogame.rng_seed(B, 17)
        done = 0
        for plies in (N * N // 2, N * N):
            gogame.batch_rollout_tracked(tracked, rng, plies - done, auto_reset=False, policy='no_eye_fill')
            done = plies
            st = gogame.batch_untrack(tracked)
            ref8 = gogame.batch_move_planes(st)
            counts = gogame.batch_move_counts(st)
            feats = gogame.batch_features(st, dtype=torch.uint8)
            assert bool((gogame.batch_move_planes_tracked(tracked) == ref8).all())
            assert bool(((counts[:, 1] > 0) == (feats[:, 12] != 0)).all())
            candidates = float(feats[:, 10].sum()) / B
            if args.sample > 0:
                sub = st[:args.sample].cpu().numpy()
                raw = oe.batch_outcome(sub)
                assert (oe.planes_of(raw) == ref8[:args.sample].cpu().numpy()).all()
                assert (oe.counts_of(raw) == counts[:args.sample].cpu().numpy()).all()
                exact = float(((raw[:, 3] >= 2) | (raw[:, 1] > 0)).sum()) / len(raw)
            else:
                exact = None
            groups = per_launch(lambda: gogame.batch_group_liberties(st), args.launches, args.warmup)
            fout = torch.empty((B, 16, N, N), dtype=torch.float16, device='cuda:0')
            features = per_launch(lambda: gogame.batch_features_tracked(tracked, dtype=torch.float16, out=fout), args.launches, args.warmup)
            del fout
            ladder = per_launch(lambda: gogame.batch_ladder_tracked(tracked), args.launches, args.warmup)
            t = per_launch(lambda: gogame.batch_move_counts(st), args.launches, args.warmup)
            print(json.dumps(dict(metric='move_counts_us_per_launch', size=N, boards=B, root_plies=plies, launches=args.launches,
                                  cus=cus, **t, boards_per_s=B / (t['median_us'] * 1e-6))), flush=True)
            for dtype in (torch.uint8, torch.float16):
                out = torch.empty((B, 12, N, N), dtype=dtype, device='cuda:0')
                for form, fn in (('tracked', lambda: gogame.batch_move_planes_tracked(tracked, dtype=dtype, out=out)),
                                 ('bytes', lambda: gogame.batch_move_planes(st, dtype=dtype, out=out))):
                    t = per_launch(fn, args.launches, args.warmup)
                    assert bool((out.to(torch.uint8) == ref8).all())
                    print(json.dumps(dict(metric='move_planes_us_per_launch', size=N, boards=B, root_plies=plies,
                                          dtype=str(dtype).split('.')[-1], input=form, launches=args.launches, cus=cus, **t,
                                          boards_per_s=B / (t['median_us'] * 1e-6), candidates=candidates, exact=exact,
                                          features_us=features['median_us'], ratio_to_features=t['median_us'] / features['median_us'],
                                          ladder_us=ladder['median_us'], ratio_to_ladder=t['median_us'] / ladder['median_us'],
                                          groups_us=groups['median_us'], ratio_to_groups=t['median_us'] / groups['median_us'])),
                          flush=True)
                del out


if __name__ == '__main__':
    main()
