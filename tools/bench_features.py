"""The feature-plane launches (gogame.batch_features / batch_features_tracked: k_features of gg_feat.h) on mid-game positions;
prints one JSON line per configuration.

  python tools/bench_features.py [--launches 30] [--warmup 5]

Shapes: 19x19 at 8 192 and 65 536 boards (120 plies of random play in), 9x9 at 65 536 boards (40 plies in); dtypes uint8 and
float16; tracked and byte-plane input.  Per configuration: `--warmup` launches, then `--launches` (>= 20) launches each
between two events of its own on the stream; median, min and max of the device time per launch.  Next to it, on the same
boards:
  untrack_us      gg_batch_untrack_states of the tracked boards - the launch the leaves=L path of PuctSearch gives up for
                  the feature launch, i.e. the parent's cost at that point of a round
  copy_GBps       bytes written per second by a device-to-device copy (torch's copy_ of a buffer of the output's size, the
                  same event timing): this box's own copy rate, the yardstick of written_GBps / frac_of_copy
  groups_only_us  the analysis without the emission is not a launch of its own; gg_batch_group_liberties (the same floods,
                  N^2 bytes out per board instead of 16 N^2 elements) stands in for it
"""
import argparse
import json

from mc_bench import ROOT   # noqa: F401  (puts the repository on sys.path)


def per_launch(fn, launches, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return {'median_us': ts[len(ts) // 2], 'min_us': ts[0], 'max_us': ts[-1]}


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
    for N, B, plies in ((19, 8192, 120), (19, 65536, 120), (9, 65536, 40)):
        st = gogame.batch_init_state(B, N, device='cuda:0')
        gogame.batch_rollout(st, gogame.rng_seed(B, 17), plies, auto_reset=False)
        tracked = gogame.batch_track(st)
        states_out = torch.empty_like(st)
        untrack = per_launch(lambda: gogame.batch_untrack(tracked, out=states_out), args.launches, args.warmup)
        groups = per_launch(lambda: gogame.batch_group_liberties(st), args.launches, args.warmup)
        for dtype in (torch.uint8, torch.float16):
            out = torch.empty((B, 16, N, N), dtype=dtype, device='cuda:0')
            src = torch.ones_like(out)
            nbytes = out.numel() * out.element_size()
            copy = per_launch(lambda: out.copy_(src), args.launches, args.warmup)
            ref = gogame.batch_features(st, dtype=dtype)
            for form, fn in (('tracked', lambda: gogame.batch_features_tracked(tracked, dtype=dtype, out=out)),
                             ('bytes', lambda: gogame.batch_features(st, dtype=dtype, out=out))):
                t = per_launch(fn, args.launches, args.warmup)
                assert bool((out == ref).all())
                gbps = nbytes / t['median_us'] * 1e-3
                copy_gbps = nbytes / copy['median_us'] * 1e-3
                print(json.dumps(dict(metric='features_us_per_launch', size=N, boards=B, root_plies=plies, dtype=str(dtype).split('.')[-1],
                                      input=form, launches=args.launches, cus=int(_lib.lib().gg_device_cus()), **t,
                                      bytes_written=nbytes, written_GBps=gbps, copy_us=copy['median_us'], copy_GBps=copy_gbps,
                                      frac_of_copy=gbps / copy_gbps, untrack_us=untrack['median_us'],
                                      groups_only_us=groups['median_us'])), flush=True)


if __name__ == '__main__':
    main()
