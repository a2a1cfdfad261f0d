"""The feature-plane launches (gogame.batch_features / batch_features_tracked: k_features of gg_feat.h) on mid-game positions;
prints one JSON line per configuration.

  python tools/bench_features.py [--launches 30] [--warmup 5] [--orient]

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

--orient: the symmetry-aware launches instead, same shapes, same event protocol, orientations from batch_draw_orient:
  oriented_features_us_per_launch   gg_batch_features_tracked_oriented (one launch) beside what a caller could do without
                  it - two_launch_*: gg_batch_symmetry_rows into a second board buffer, then gg_batch_features_tracked, both
                  between the same pair of events - and beside the unoriented launch (plain_us)
  policy_turn_us_per_launch         gg_batch_symmetry_policy on [B, N^2 + 1] rows of float32 and of bool, forward and
                  inverse, beside a device-to-device copy of the same bytes (copy_us; moved_GBps counts bytes read + written)
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


def main_orient(args):
    import torch
    from gymgo_amd import gogame, _lib
    torch.cuda.set_device(0)
    lib, cus = _lib.lib(), int(_lib.lib().gg_device_cus())
    I32, U8 = torch.int32, torch.uint8
    for N, B, plies in ((19, 8192, 120), (19, 65536, 120), (9, 65536, 40)):
        st = gogame.batch_init_state(B, N, device='cuda:0')
        gogame.batch_rollout(st, gogame.rng_seed(B, 17), plies, auto_reset=False)
        tracked = gogame.batch_track(st)
        turned = torch.empty_like(tracked)
        orient = gogame.batch_draw_orient(gogame.rng_seed(B, 23))
        stream = _lib.stream_ptr(st.device)
        tp, up, op = _lib.dev_ptr(tracked, I32, 'tracked'), _lib.dev_ptr(turned, I32, 'turned'), _lib.dev_ptr(orient, I32, 'orient')
        for dtype in (torch.uint8, torch.float16):
            code = gogame.FEATURE_DTYPES[dtype]
            out = torch.empty((B, 16, N, N), dtype=dtype, device='cuda:0')
            pp = _lib.dev_ptr(out, dtype, 'out')
            nbytes = out.numel() * out.element_size()

            def two_launches():
                _lib.check(lib.gg_batch_symmetry_rows(tp, 5, op, up, B, N, stream), 'gg_batch_symmetry_rows')
                _lib.check(lib.gg_batch_features_tracked(up, pp, code, B, N, stream), 'gg_batch_features_tracked')

            two = per_launch(two_launches, args.launches, args.warmup)
            ref = out.clone()
            plain = per_launch(lambda: _lib.check(lib.gg_batch_features_tracked(tp, pp, code, B, N, stream), 'gg_batch_features_tracked'),
                               args.launches, args.warmup)
            t = per_launch(lambda: _lib.check(lib.gg_batch_features_tracked_oriented(tp, op, pp, code, B, N, stream),
                                              'gg_batch_features_tracked_oriented'), args.launches, args.warmup)
            assert bool((out == ref).all())
            print(json.dumps(dict(metric='oriented_features_us_per_launch', size=N, boards=B, root_plies=plies,
                                  dtype=str(dtype).split('.')[-1], input='tracked', launches=args.launches, cus=cus, **t,
                                  bytes_written=nbytes, two_launch_median_us=two['median_us'], two_launch_min_us=two['min_us'],
                                  two_launch_max_us=two['max_us'], frac_of_two_launch=t['median_us'] / two['median_us'],
                                  plain_us=plain['median_us'])), flush=True)
        A = N * N + 1
        for dtype in (torch.float32, torch.bool):
            src = (torch.rand((B, A), device='cuda:0') < 0.5) if dtype == torch.bool else torch.rand((B, A), device='cuda:0')
            dst = torch.empty_like(src)
            es = src.element_size()
            sp, dp = _lib.dev_ptr(src, dtype, 'in'), _lib.dev_ptr(dst, dtype, 'out')
            copy = per_launch(lambda: dst.copy_(src), args.launches, args.warmup)
            for inverse in (0, 1):
                t = per_launch(lambda: _lib.check(lib.gg_batch_symmetry_policy(sp, op, dp, es, inverse, B, N, stream),
                                                  'gg_batch_symmetry_policy'), args.launches, args.warmup)
                moved = 2 * src.numel() * es
                print(json.dumps(dict(metric='policy_turn_us_per_launch', size=N, boards=B, dtype=str(dtype).split('.')[-1],
                                      inverse=bool(inverse), launches=args.launches, cus=cus, **t, bytes_moved=moved,
                                      moved_GBps=moved / t['median_us'] * 1e-3, copy_us=copy['median_us'], copy_min_us=copy['min_us'],
                                      copy_max_us=copy['max_us'], copy_GBps=moved / copy['median_us'] * 1e-3,
                                      frac_of_copy=copy['median_us'] / t['median_us'])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--orient', action='store_true', help='the oriented launches and the policy turn beside their baselines')
    args = ap.parse_args()
    if args.launches < 20:
        ap.error('need at least 20 timed launches')
    if args.orient:
        return main_orient(args)
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
