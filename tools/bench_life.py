"""The pass-alive life launches (gogame.batch_life / batch_life_tracked: k_life of gg_life.h) on positions of the no_eye_fill
policy; prints one JSON line per configuration.

  python tools/bench_life.py [--launches 30] [--warmup 5]

Shapes: 19x19 at 8 192 and 65 536 boards, 9x9 at 65 536 boards; dtypes uint8 and float16; tracked and byte-plane input.
Boards: N^2 and 2 N^2 plies into batch_rollout_tracked(policy='no_eye_fill', auto_reset off) from the empty board - an open
board set (few alive chains, no settled board) and a settled one; `alive_boards` and `settled_boards` say what each set
holds.  Per configuration: `--warmup` launches, then `--launches` (>= 20) launches each between two events of its own on
the stream; median, min and max of the device time per launch.  Next to it, on the same boards:
  groups_us   gg_batch_group_liberties - the closest launch the library had before: the same layout, one flood pair per
              group where the life launch runs one per region and per candidate chain, pass after pass
  copy_us     a device-to-device copy of a buffer of the output's size (torch's copy_, the same event timing)
There is no target: ratio_to_groups on the two board sets is the result.
"""
import argparse
import json

from mc_bench import ROOT   # noqa: F401  (puts the repository on sys.path)
from bench_features import per_launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    if args.launches < 20:
        ap.error('need at least 20 timed launches')
    import torch
    from gymgo_amd import gogame, _lib
    torch.cuda.set_device(0)
    cus = int(_lib.lib().gg_device_cus())
    for N, B in ((19, 8192), (19, 65536), (9, 65536)):
        tracked = gogame.batch_track(gogame.batch_init_state(B, N, device='cuda:0'))
        rng = gogame.rng_seed(B, 17)
        for plies in (N * N, 2 * N * N):
            gogame.batch_rollout_tracked(tracked, rng, N * N, auto_reset=False, policy='no_eye_fill')
            st = gogame.batch_untrack(tracked)
            ref8, flags = gogame.batch_life(st, settled=True)
            alive = int((ref8[:, 0] | ref8[:, 1]).flatten(1).any(dim=1).sum())
            groups = per_launch(lambda: gogame.batch_group_liberties(st), args.launches, args.warmup)
            for dtype in (torch.uint8, torch.float16):
                out = torch.empty((B, 4, N, N), dtype=dtype, device='cuda:0')
                src = torch.ones_like(out)
                nbytes = out.numel() * out.element_size()
                copy = per_launch(lambda: out.copy_(src), args.launches, args.warmup)
                for form, fn in (('tracked', lambda: gogame.batch_life_tracked(tracked, dtype=dtype, out=out)),
                                 ('bytes', lambda: gogame.batch_life(st, dtype=dtype, out=out))):
                    t = per_launch(fn, args.launches, args.warmup)
                    assert bool((out.to(torch.uint8) == ref8).all())
                    print(json.dumps(dict(metric='life_us_per_launch', size=N, boards=B, root_plies=plies,
                                          dtype=str(dtype).split('.')[-1], input=form, launches=args.launches, cus=cus, **t,
                                          alive_boards=alive, settled_boards=int(flags.sum()), bytes_written=nbytes,
                                          groups_us=groups['median_us'], groups_min_us=groups['min_us'], groups_max_us=groups['max_us'],
                                          ratio_to_groups=t['median_us'] / groups['median_us'], copy_us=copy['median_us'],
                                          copy_min_us=copy['min_us'], copy_max_us=copy['max_us'])), flush=True)


if __name__ == '__main__':
    main()
