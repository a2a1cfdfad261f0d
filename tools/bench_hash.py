"""The hash launches (gogame.batch_move_hashes / batch_move_hashes_tracked / batch_superko_moves[_tracked]: k_move_hashes of
gg_hash.h) on positions of the no_eye_fill policy; prints one JSON line per configuration.

  python tools/bench_hash.py [--launches 30] [--warmup 5] [--sample 8] [--boards 65536] [--history 256]

Shapes and protocol: tools/bench_moves.py's - 19x19 at 65 536 boards, N^2 / 2 plies (mid-game) into
batch_rollout_tracked(policy='no_eye_fill', auto_reset off) from the empty board; `--warmup` launches, then `--launches`
(>= 5) launches each between two events of its own on the stream; median, min and max of the device time per launch and
boards per second at the median.  Per input form (byte planes, tracked boards):
  move_hashes    the hashes int64 [B, N^2 + 1] alone
  superko        the repeat bytes alone, against a history of `--history` entries per board, all valid (random words: the
                 worst case, every candidate is compared with every entry)
next to batch_move_counts and batch_hash on the same boards in the same process (`ratio_to_counts`).  There is no target: the
medians and the ratios are the result.  With --sample S > 0 (needs the repository's tests/ on the path: the expectation) the
first S boards are held against tests/hash_expect.py.
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
    ap.add_argument('--boards', type=int, default=65536)
    ap.add_argument('--history', type=int, default=256)
    args = ap.parse_args()
    if args.launches < 5:
        ap.error('need at least 5 timed launches')
    import torch
    from gymgo_amd import gogame, _lib
    torch.cuda.set_device(0)
    cus = int(_lib.lib().gg_device_cus())
    B, N, H = args.boards, 19, args.history
    tracked = gogame.batch_track(gogame.batch_init_state(B, N, device='cuda:0'))
    rng = gogame.rng_seed(B, 17)
    plies = N * N // 2
    gogame.batch_rollout_tracked(tracked, rng, plies, auto_reset=False, policy='no_eye_fill')
    st = gogame.batch_untrack(tracked)
    ref = gogame.batch_move_hashes(st)
    assert bool((gogame.batch_move_hashes_tracked(tracked) == ref).all())
    assert bool((gogame.batch_hash(st) == ref[:, N * N]).all()) and bool((gogame.batch_hash_tracked(tracked) == ref[:, N * N]).all())
    if args.sample > 0:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import hash_expect as he
        assert (he.batch_move_hashes(st[:args.sample].cpu().numpy()) == ref[:args.sample].cpu().numpy()).all()
    history = gogame.PositionHistory(B, H)
    history.hashes.random_()
    history.count.fill_(H)
    history.hashes[:, H // 2] = ref[:, 0]          # (one entry that can match: the move at point 0, or the board itself)
    rep = gogame.batch_superko_moves(st, history)
    assert bool((gogame.batch_superko_moves_tracked(tracked, history) == rep).all())
    counts = per_launch(lambda: gogame.batch_move_counts(st), args.launches, args.warmup)
    common = dict(size=N, boards=B, root_plies=plies, launches=args.launches, cus=cus)
    print(json.dumps(dict(metric='move_counts_us_per_launch', **common, **counts, boards_per_s=B / (counts['median_us'] * 1e-6))),
          flush=True)
    for form, x, base, moves, superko in (('bytes', st, gogame.batch_hash, gogame.batch_move_hashes, gogame.batch_superko_moves),
                                          ('tracked', tracked, gogame.batch_hash_tracked, gogame.batch_move_hashes_tracked,
                                           gogame.batch_superko_moves_tracked)):
        t = per_launch(lambda: base(x), args.launches, args.warmup)
        print(json.dumps(dict(metric='hash_us_per_launch', input=form, **common, **t, boards_per_s=B / (t['median_us'] * 1e-6))),
              flush=True)
        out = torch.empty((B, N * N + 1), dtype=torch.int64, device='cuda:0')
        t = per_launch(lambda: moves(x, out=out), args.launches, args.warmup)
        assert bool((out == ref).all())
        print(json.dumps(dict(metric='move_hashes_us_per_launch', input=form, **common, **t, boards_per_s=B / (t['median_us'] * 1e-6),
                              counts_us=counts['median_us'], ratio_to_counts=t['median_us'] / counts['median_us'])), flush=True)
        del out
        t = per_launch(lambda: superko(x, history), args.launches, args.warmup)
        print(json.dumps(dict(metric='superko_us_per_launch', input=form, history=H, **common, **t,
                              boards_per_s=B / (t['median_us'] * 1e-6), counts_us=counts['median_us'],
                              ratio_to_counts=t['median_us'] / counts['median_us'])), flush=True)


if __name__ == '__main__':
    main()
