"""The ladder launches (gogame.batch_ladder / batch_ladder_tracked: k_ladder of gg_ladder.h) on positions of the no_eye_fill
policy; prints one JSON line per configuration.

  python tools/bench_ladder.py [--launches 30] [--warmup 5] [--sample 64]

Shapes, boards and protocol: tools/bench_life.py's - 19x19 at 8 192 and 65 536 boards, 9x9 at 65 536 boards; dtypes uint8 and
float16; tracked and byte-plane input; N^2 and 2 N^2 plies into batch_rollout_tracked(policy='no_eye_fill', auto_reset off)
from the empty board; `--warmup` launches, then `--launches` (>= 20) launches each between two events of its own on the
stream; median, min and max of the device time per launch.  Next to it, on the same boards:
  life_us     gg_batch_life_tracked (uint8) - the launch the search queues next to this one
  groups_us   gg_batch_group_liberties - one flood pair per group, the analysis this launch starts with
There is no target: the medians, ratio_to_life and ratio_to_groups are the result.  `laddered_boards` / `aborted_queries`
say what the board set holds (from the launch itself).  With --sample S > 0 (needs the repository's tests/ on the path: the
expectation) the per-board means of root queries, nodes and aborted queries of the first S boards, counted by
tests/ladder_expect.py on the host, are printed next to each board set.
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
    ap.add_argument('--sample', type=int, default=64)
    args = ap.parse_args()
    if args.launches < 20:
        ap.error('need at least 20 timed launches')
    import torch
    from gymgo_amd import gogame, _lib
    torch.cuda.set_device(0)
    cus = int(_lib.lib().gg_device_cus())
    if args.sample > 0:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import ladder_expect as le
    for N, B in ((19, 8192), (19, 65536), (9, 65536)):
        tracked = gogame.batch_track(gogame.batch_init_state(B, N, device='cuda:0'))
        rng = gogame.rng_seed(B, 17)
        for plies in (N * N, 2 * N * N):
            gogame.batch_rollout_tracked(tracked, rng, N * N, auto_reset=False, policy='no_eye_fill')
            st = gogame.batch_untrack(tracked)
            ref8, ab = gogame.batch_ladder(st, aborted=True)
            laddered = int((ref8[:, 0] | ref8[:, 1]).flatten(1).any(dim=1).sum())
            if args.sample > 0:
                sub = st[:args.sample].cpu().numpy()
                want, wab, stats = le.batch_ladder(sub, stats=True)
                assert (want == ref8[:args.sample].cpu().numpy()).all() and (wab == ab[:args.sample].cpu().numpy()).all()
                mean = lambda k: sum(x[k] for x in stats) / len(stats)
                print(json.dumps(dict(metric='ladder_work_per_board', size=N, root_plies=plies, sample=len(stats),
                                      queries=mean('queries'), nodes=mean('nodes'), aborts=mean('aborts'),
                                      max_depth=max(x['depth'] for x in stats))), flush=True)
            groups = per_launch(lambda: gogame.batch_group_liberties(st), args.launches, args.warmup)
            life = per_launch(lambda: gogame.batch_life_tracked(tracked), args.launches, args.warmup)
            for dtype in (torch.uint8, torch.float16):
                out = torch.empty((B, 4, N, N), dtype=dtype, device='cuda:0')
                for form, fn in (('tracked', lambda: gogame.batch_ladder_tracked(tracked, dtype=dtype, out=out)),
                                 ('bytes', lambda: gogame.batch_ladder(st, dtype=dtype, out=out))):
                    t = per_launch(fn, args.launches, args.warmup)
                    assert bool((out.to(torch.uint8) == ref8).all())
                    print(json.dumps(dict(metric='ladder_us_per_launch', size=N, boards=B, root_plies=plies,
                                          dtype=str(dtype).split('.')[-1], input=form, launches=args.launches, cus=cus, **t,
                                          laddered_boards=laddered, aborted_queries=int(ab.sum()),
                                          life_us=life['median_us'], life_min_us=life['min_us'], life_max_us=life['max_us'],
                                          ratio_to_life=t['median_us'] / life['median_us'],
                                          groups_us=groups['median_us'], groups_min_us=groups['min_us'], groups_max_us=groups['max_us'],
                                          ratio_to_groups=t['median_us'] / groups['median_us'])), flush=True)


if __name__ == '__main__':
    main()
