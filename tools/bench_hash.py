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

The tree's rule (gg_puct_superko: k_puct_superko of gg_hash.h), on the same positions:
  puct_superko   one launch on the first 8 192 boards as the leaves of 8 192 roots (L = 1), links and node_hash built as chains
                 of `depth` = 8 / 32 / 128 ancestors (random words: every candidate is compared with every ancestor), without
                 a history (H = 0) and with `--history` valid entries; next to gg_batch_move_hashes_tracked(rows=) on the same
                 boards with the same history in the same process (`ratio_to_rows`) - the nearest launch without a chain
  puct_round     one PuctSearch round (select + backup, leaves=8, 1 024 roots, features float16, a constant evaluator) with
                 superko=None and with superko=history (`ratio_to_plain`)
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
    tree_rows(args, tracked, st, common)


def tree_rows(args, tracked, st, common):
    """The rows of gg_puct_superko and of a search round with it (the module's text)."""
    import torch
    from gymgo_amd import gogame, _lib
    N, H, dev = 19, args.history, tracked.device
    Bt, C = min(8192, tracked.shape[0]), 128
    leaf0 = tracked[:Bt].contiguous()
    history = gogame.PositionHistory(Bt, H)
    history.hashes.random_()
    history.count.fill_(H)
    rows = per_launch(lambda: gogame._move_hashes(leaf0, True, history, rows=True), args.launches, args.warmup)
    tree = dict(common, boards=Bt)
    print(json.dumps(dict(metric='superko_rows_us_per_launch', input='tracked', history=H, **tree, **rows)), flush=True)
    links = torch.full((Bt, C + 1, 2), -1, dtype=torch.int32, device=dev)
    links[:, 1:, 0] = torch.arange(C, dtype=torch.int32, device=dev)[None, :]       # node x hangs under x - 1
    node_hash = torch.empty((Bt, C + 1), dtype=torch.int64, device=dev).random_()
    move = torch.zeros(Bt, dtype=torch.int32, device=dev)
    stream = _lib.stream_ptr(dev)
    for depth in (8, 32, 128):
        leaf_id = torch.full((Bt,), depth, dtype=torch.int32, device=dev)
        for hist in (None, history):
            leaf = leaf0.clone()
            hp, cp, h = (None, None, 0) if hist is None else (hist.hashes, hist.count, H)
            t = per_launch(lambda: _lib.call('gg_puct_superko', Bt, N, C, 1, links, node_hash, hp, cp, h, leaf, move, leaf_id, stream),
                           args.launches, args.warmup)
            assert bool((leaf == leaf0).all())      # (random words: nothing is hit, the boards stay what they were)
            print(json.dumps(dict(metric='puct_superko_us_per_launch', depth=depth, history=h, **tree, **t,
                                  boards_per_s=Bt / (t['median_us'] * 1e-6), rows_us=rows['median_us'],
                                  ratio_to_rows=t['median_us'] / rows['median_us'])), flush=True)
    R, L, A = min(1024, st.shape[0]), 8, N * N + 1
    rounds = args.launches + args.warmup
    priors = torch.full((R * L, A), 1.0 / A, dtype=torch.float32, device=dev)
    values = torch.zeros(R * L, dtype=torch.float32, device=dev)
    plain = None
    for mode in ('none', 'history'):
        hist = None
        if mode == 'history':
            hist = gogame.PositionHistory(R, H)
            hist.hashes.random_()
            hist.count.fill_(H - 1)
            hist.push(gogame.batch_hash(st[:R]))
        search = gogame.PuctSearch(st[:R], rounds + 1, leaves=L, features=torch.float16, superko=hist)
        search.select()
        search.backup(priors, values)               # round 0 hands out the roots alone

        def one_round():
            search.select()
            search.backup(priors, values)

        t = per_launch(one_round, args.launches, args.warmup)
        plain = t['median_us'] if plain is None else plain
        print(json.dumps(dict(metric='puct_round_us', superko=mode, roots=R, leaves=L, history=H if hist is not None else 0,
                              **dict(common, boards=R * L), **t, ratio_to_plain=t['median_us'] / plain)), flush=True)
        del search
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
