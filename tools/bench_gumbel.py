"""One PuctSearch round under the Gumbel root rule next to the plain round (gg_gumbel_select_leaves in place of
gg_puct_select_leaves), and gg_gumbel_root / gg_gumbel_begin alone; prints one JSON line per row.

  python tools/bench_gumbel.py [--launches 30] [--warmup 5] [--roots 1024] [--repo PATH]

Shape: `--roots` roots of 19x19 after N^2 / 2 plies of batch_rollout_tracked(policy='no_eye_fill', auto_reset off) from the
empty board, leaves=8, features float16, a constant evaluator (uniform priors, value 0), so a round is the library's own
share.  Two searches on the same roots, gumbel=None and gumbel=16 (g from gumbel_noise, seeded), each given round 0 (the
roots alone); then `--warmup` + `--launches` turns, each turn ONE round of the plain search and ONE round of the Gumbel
search, every round between two events of its own on the stream: the two rows alternate on one lease.  Median, min and max
of the device time per round.  Then, on the Gumbel search after its rounds: gg_gumbel_root alone (preallocated outputs, with
q / visits / value), PuctSearch.gumbel_root() as a whole (the launch and the torch softmax) and gg_gumbel_begin alone.

--repo PATH imports gymgo_amd from another checkout (its own built library): a checkout without the Gumbel rule - the parent
commit - gives the plain row alone, which is the yardstick for both rows of this one.  There is no target.
"""
import argparse
import json
import os
import sys


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def stats(ts):
    ts = sorted(ts)
    return {'median_us': ts[len(ts) // 2], 'min_us': ts[0], 'max_us': ts[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--roots', type=int, default=1024)
    ap.add_argument('--repo', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    if args.launches < 5:
        ap.error('need at least 5 timed launches')
    sys.path.insert(0, os.path.abspath(args.repo))
    import torch
    from gymgo_amd import gogame, _lib
    torch.cuda.set_device(0)
    cus = int(_lib.lib().gg_device_cus())
    has_gumbel = hasattr(gogame, 'Gumbel')
    R, N, L, m = args.roots, 19, 8, 16
    A = N * N + 1
    tracked = gogame.batch_track(gogame.batch_init_state(R, N, device='cuda:0'))
    gogame.batch_rollout_tracked(tracked, gogame.rng_seed(R, 17), N * N // 2, auto_reset=False, policy='no_eye_fill')
    st = gogame.batch_untrack(tracked)
    rounds = args.launches + args.warmup
    priors = torch.full((R * L, A), 1.0 / A, dtype=torch.float32, device='cuda:0')
    values = torch.zeros(R * L, dtype=torch.float32, device='cuda:0')
    searches = {'plain': gogame.PuctSearch(st, rounds + 1, leaves=L, features=torch.float16)}
    if has_gumbel:
        searches['gumbel'] = gogame.PuctSearch(st, rounds + 1, leaves=L, features=torch.float16, gumbel=m)
        draws = gogame.gumbel_noise(torch.Generator(device='cuda:0').manual_seed(5))
        searches['gumbel'].set_gumbel(draws(0, searches['gumbel']._legal_roots))
    for s in searches.values():
        s.select()
        s.backup(priors, values)                  # round 0 hands out the roots alone
    times = {k: [] for k in searches}
    for i in range(rounds):
        for k, s in searches.items():             # one round of each, in turn

            def one_round():
                s.select()
                s.backup(priors, values)

            t = timed(one_round)
            if i >= args.warmup:
                times[k].append(t)
    common = dict(size=N, roots=R, leaves=L, boards=R * L, launches=args.launches, cus=cus, repo=os.path.abspath(args.repo))
    plain = stats(times['plain'])['median_us']
    for k, s in searches.items():   # (live_slots: the slots of the last round that hold a leaf - the work a round does)
        t = stats(times[k])
        print(json.dumps(dict(metric='puct_round_us', rule=k, considered=m if k == 'gumbel' else None, **common, **t,
                              ratio_to_plain=t['median_us'] / plain, live_slots=int((s._leaf_id >= 0).sum()),
                              nodes_per_root=float(s._nodes.float().mean()))), flush=True)
    if not has_gumbel:
        return
    s = searches['gumbel']
    print(json.dumps(dict(metric='gumbel_schedule', simulations=s._gumbel.simulations,
                          done_min=int(s._sims.min()), done_max=int(s._sims.max()))), flush=True)
    acts = torch.empty(R, dtype=torch.int32, device='cuda:0')
    q = torch.empty((R, A), dtype=torch.float32, device='cuda:0')
    n = torch.empty((R, A), dtype=torch.int32, device='cuda:0')
    v = torch.empty(R, dtype=torch.float32, device='cuda:0')
    boards, child, _, _, st_, nodes = s._tree
    stream = _lib.current_raw_stream(torch.device('cuda:0'))
    root = lambda: _lib.call('gg_gumbel_root', R, N, s._C, boards, child, st_, nodes, s.base, s._seen, s._gumbel.c_visit,
                             s._gumbel.c_scale, acts, q, n, v, stream)
    rows = (('gumbel_root_us_per_launch', root), ('gumbel_root_with_policy_us', lambda: s._gumbel_root(pi=True)),
            ('gumbel_begin_us_per_launch', s._gumbel_begin))
    for name, fn in rows:
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        print(json.dumps(dict(metric=name, **common, **stats([timed(fn) for _ in range(args.launches)]))), flush=True)


if __name__ == '__main__':
    main()
