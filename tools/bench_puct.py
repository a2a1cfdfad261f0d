"""PUCT tree search (gogame.batch_puct): the cost of the tree per iteration, and the search with the playout evaluator against
batch_uct at the same R, I, K; prints one JSON line per configuration.

  python tools/bench_puct.py --evaluator null [--roots 1024 16384] [--iters 64 800] [--size 19] [--plies 120] [--reps 3]
  python tools/bench_puct.py --evaluator playouts [--roots 256 1024] [--k 256] [--iters 64] ...

Workload: R mid-game roots (random play from the empty board, `--plies` plies), komi 7.5.
  null:      the evaluator returns the same preallocated priors (1 / A everywhere) and values (0) every time - no evaluator
             work, so an iteration is k_puct_select, the one-move step, untrack, the legality mask (k_puct_legal) and
             k_puct_backup plus the host loop around them.  us_per_iteration is wall time (events on the stream) of
             batch_puct / I, gg_puct_begin's memsets included (begin_ms: measured on its own); median of `--reps` runs.
             For the device time per kernel run it once under `rocprofv3 --kernel-trace --stats -- python
             tools/bench_puct.py --evaluator null --reps 1 --roots R --iters I`.
  playouts:  batch_puct with gogame.playout_evaluator(K) and batch_uct(roots, I, K) alternate in one process, median of
             `--reps` runs each; ratio = PUCT iterations/s over UCT iterations/s.  The two searches grow different trees, so
             plies/s of both are reported too.

  --leaves L [L ...]: several leaves per root per round (batch_puct(.., leaves=L)) against leaves=None at the same total leaf
  budget: `--iters` is the budget I, the search with L leaves runs I // L rounds in a tree of the same size.
  null:      batch_puct(.., leaves=L) and batch_puct(..) alternate in one process, median of `--reps`; us_per_leaf is wall time
             over the leaves that were evaluated per root (the non-empty slots: mean root_visits), ratio = us_per_leaf of
             leaves=None over that of leaves=L.
  playouts:  plies/s of the search with playout_evaluator(K) for leaves=L against leaves=None at the same R, and against
             leaves=None at `--ref-roots` (the batch size the drain argument compares with), all alternating in one process.

  --moves M [--reuse | --no-reuse] [--capacity-factor F]: M moves in a row (search `--iters` rounds, play the most-visited
  child, PuctSearch.advance), the tree with room for F * (the default) nodes.  Per move: wall ms of the search, of advance()
  and of constructing a fresh PuctSearch of the same capacity on R roots (what a caller did before advance existed;
  alternating with advance, median of `--reps`), the mean share of nodes and of root visits that advance kept, and the mean
  root visits after the move's search.  --no-reuse starts every move from a new PuctSearch (the same rounds per move).
  --evaluator peaked: fixed preallocated priors that fall geometrically with the action index (ratio 1/2), values 0.
  For the kernel's device time: `rocprofv3 --kernel-trace --stats -- python tools/bench_puct.py --moves M --reps 1 ...`.

  --features (null evaluator, with or without --leaves): the search hands out float16 feature planes (batch_puct(..,
  features=torch.float16): gg_batch_features_tracked in the round) instead of byte-plane states; the evaluator ignores them.

  --selfplay --moves M [--leaves L] [--alpha 0.03] [--eps 0.25]: gogame.puct_selfplay (the kept tree with room for
  `--capacity-factor` times the default, Dirichlet noise by add_root_noise, every move drawn from the visit counts, the
  records on the device, no synchronisation) against what a caller could do without it: a new PuctSearch per move
  (puct_play's reuse=False loop), the same noise mixed into the priors by the evaluator on its first call of every move,
  result() read back per move, pi and the draw on the host.  Null evaluator, `--iters` rounds per move; both alternate in
  one process, wall seconds (host clock around the call and a synchronisation) as the median of `--reps`.  The two play
  different games (kept trees, other generators): the figure is the cost of a move, not a strength.  For the device time
  of k_puct_root_noise / k_puct_root_policy: `rocprofv3 --kernel-trace --stats -- python tools/bench_puct.py --selfplay
  --moves M --reps 1 ...`.
"""
import argparse
import json
import time

from mc_bench import median_timed, mid_game_roots, timed   # (puts the repository on sys.path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--evaluator', choices=['null', 'playouts', 'peaked'], default='null')
    ap.add_argument('--roots', type=int, nargs='+', default=None)
    ap.add_argument('--iters', type=int, nargs='+', default=None)
    ap.add_argument('--k', type=int, default=256)
    ap.add_argument('--size', type=int, default=19)
    ap.add_argument('--plies', type=int, default=120)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--c', type=float, default=1.25)
    ap.add_argument('--leaves', type=int, nargs='+', default=None)
    ap.add_argument('--ref-roots', type=int, default=1024)
    ap.add_argument('--moves', type=int, default=None)
    ap.add_argument('--reuse', dest='reuse', action='store_true', default=True)
    ap.add_argument('--no-reuse', dest='reuse', action='store_false')
    ap.add_argument('--capacity-factor', type=int, default=2)
    ap.add_argument('--selfplay', action='store_true')
    ap.add_argument('--alpha', type=float, default=0.03)
    ap.add_argument('--eps', type=float, default=0.25)
    ap.add_argument('--features', action='store_true')
    args = ap.parse_args()
    if args.evaluator == 'peaked' and args.moves is None:
        ap.error('--evaluator peaked needs --moves')
    if args.selfplay and (args.moves is None or args.evaluator != 'null'):
        ap.error('--selfplay needs --moves and the null evaluator')

    import torch
    from gymgo_amd import gogame, _lib
    torch.cuda.set_device(0)
    N, K, A = args.size, args.k, args.size * args.size + 1
    null = args.evaluator == 'null'
    for R in args.roots or ([1024, 16384] if null else [256, 1024]):
        roots = mid_game_roots(R, N, args.plies)
        for I in args.iters or ([64, 800] if null else [64]):
            base = {'size': N, 'roots': R, 'iterations': I, 'root_plies': args.plies, 'c': args.c,
                    'cus': int(_lib.lib().gg_device_cus()), 'reps': args.reps}
            if args.selfplay:
                for L in args.leaves or [None]:
                    print(json.dumps(_selfplay(args, gogame, torch, roots, base, L)), flush=True)
                continue
            if args.moves is not None:
                for L in args.leaves or [None]:
                    for res in _moves(args, gogame, torch, roots, base, L):
                        print(json.dumps(res), flush=True)
                continue
            if args.leaves:
                for res in _leaves(args, gogame, torch, roots, base, null):
                    print(json.dumps(res), flush=True)
                continue
            if null:
                priors = torch.full((R, A), 1.0 / A, dtype=torch.float32, device='cuda:0')
                values = torch.zeros(R, dtype=torch.float32, device='cuda:0')
                run = lambda: gogame.batch_puct(roots, I, lambda states, legal: (priors, values), c=args.c, komi=7.5, tree=True,
                                                features=torch.float16 if args.features else None)
                ref = run()   # warm-up
                assert bool((ref.root_visits == I).all())
                (s, out), = median_timed(run, reps=args.reps)
                sb, _ = timed(lambda: gogame.PuctSearch(roots, I, c=args.c, komi=7.5))
                depth = _mean_leaf_depth(out.tree.parent, out.nodes)
                res = dict(base, metric='puct_wall_us_per_iteration', evaluator='null', seconds=s, begin_ms=sb * 1e3,
                           us_per_iteration=s / I * 1e6, us_per_iteration_without_begin=(s - sb) / I * 1e6,
                           mean_nodes=float(out.nodes.float().mean()), mean_node_depth=depth,
                           tree_bytes=R * (I + 1) * (4 * (5 * N + 1) + 8 * A + 24))
            else:
                kw = dict(komi=7.5)
                evs = []

                def run_a():
                    evs.append(gogame.playout_evaluator(K, seed=1, **kw))
                    return gogame.batch_puct(roots, I, evs[-1], c=args.c, **kw)

                def run_b():
                    return gogame.batch_uct(roots, I, K, seed=1, **kw)

                ref = run_a()   # warm-up
                run_b()
                assert bool((ref.root_visits == I).all())
                (sa, pa), (sb, ub) = median_timed(run_a, run_b, reps=args.reps)
                plies_a, plies_b = int(evs[-1].plies_sum), int(ub.plies_sum.sum())
                P = R * K * I
                res = dict(base, metric='puct_iterations_per_s', evaluator='playouts', k=K, playouts=P,
                           jobs_per_slot=R * K / (256 * base['cus']), seconds_puct=sa, seconds_uct=sb,
                           iterations_per_s=I / sa, iterations_per_s_uct=I / sb, ratio=sb / sa,
                           plies_per_s=plies_a / sa, plies_per_s_uct=plies_b / sb, ratio_plies=(plies_a / sa) / (plies_b / sb),
                           mean_plies_puct=plies_a / P, mean_plies_uct=plies_b / P,
                           mean_nodes=float(pa.nodes.float().mean()), mean_nodes_uct=float(ub.nodes.float().mean()))
            print(json.dumps(res), flush=True)


def _leaves(args, gogame, torch, roots, base, null):
    """The --leaves comparison: one result per L, each against leaves=None in alternation."""
    R, N, I, K = base['roots'], base['size'], base['iterations'], args.k
    A = N * N + 1
    if null:
        for L in args.leaves:
            T = I // L
            priors = torch.full((R * L, A), 1.0 / A, dtype=torch.float32, device='cuda:0')
            values = torch.zeros(R * L, dtype=torch.float32, device='cuda:0')
            ev_l = lambda states, legal: (priors, values)
            ev_1 = lambda states, legal: (priors[:R], values[:R])
            run_l = lambda: gogame.batch_puct(roots, T, ev_l, c=args.c, komi=7.5, tree=True, leaves=L,
                                              features=torch.float16 if args.features else None)
            run_1 = lambda: gogame.batch_puct(roots, I, ev_1, c=args.c, komi=7.5, tree=True)
            run_l(), run_1()   # warm-up
            (sl, ol), (s1, o1) = median_timed(run_l, run_1, reps=args.reps)
            done = float(ol.root_visits.double().mean())
            assert bool((o1.root_visits == I).all())
            us_l, us_1 = sl / done * 1e6, s1 / I * 1e6
            yield dict(base, metric='puct_leaves_wall_us_per_leaf', evaluator='null', leaves=L, rounds=T, seconds=sl,
                       seconds_one_leaf=s1, leaves_evaluated_per_root=done, live_slots_per_round=done / T,
                       us_per_leaf=us_l, us_per_leaf_one_leaf=us_1, ratio=us_1 / us_l, us_per_round=sl / T * 1e6,
                       mean_nodes=float(ol.nodes.float().mean()), mean_nodes_one_leaf=float(o1.nodes.float().mean()),
                       mean_node_depth=_mean_leaf_depth(ol.tree.parent, ol.nodes))
        return
    kw = dict(komi=7.5)
    ref_roots = mid_game_roots(args.ref_roots, N, args.plies)
    evs = {}

    def runner(key, rts, rounds, L):
        def run():
            evs[key] = gogame.playout_evaluator(K, seed=1, **kw)
            return gogame.batch_puct(rts, rounds, evs[key], c=args.c, leaves=L, **kw)
        return run

    runs = [('none', runner('none', roots, I, None)), ('ref', runner('ref', ref_roots, I, None))]
    runs += [(L, runner(L, roots, I // L, L)) for L in args.leaves]
    for _, fn in runs:
        fn()   # warm-up
    timed_runs = median_timed(*[fn for _, fn in runs], reps=args.reps)
    rate = {key: int(evs[key].plies_sum) / s for (key, _), (s, _) in zip(runs, timed_runs)}
    for (key, _), (s, out) in zip(runs, timed_runs):
        L = None if key in ('none', 'ref') else key
        rr = args.ref_roots if key == 'ref' else R
        rounds = I if L is None else I // L
        done = float(out.root_visits.double().mean())
        yield dict(base, metric='puct_leaves_plies_per_s', evaluator='playouts', k=K, roots=rr, leaves=L, rounds=rounds,
                   seconds=s, plies=int(evs[key].plies_sum), plies_per_s=rate[key], ratio_to_one_leaf=rate[key] / rate['none'],
                   ratio_to_ref_roots=rate[key] / rate['ref'], ref_roots=args.ref_roots,
                   leaves_evaluated_per_root=done, live_slots_per_round=done / rounds,
                   jobs_per_slot=rr * (L or 1) * K / (256 * base['cus']))


def _moves(args, gogame, torch, roots, base, L):
    """The --moves loop: one result per move."""
    R, N, I, K = base['roots'], base['size'], base['iterations'], args.k
    A, B = N * N + 1, R * (L or 1)
    T = I // (L or 1)
    capacity = args.capacity_factor * T * (L or 1) + 1
    if args.evaluator == 'playouts':
        ev = gogame.playout_evaluator(K, seed=1, komi=7.5)
    else:
        row = torch.full((A,), 1.0 / A) if args.evaluator == 'null' else 0.5 ** torch.arange(1, A + 1, dtype=torch.float64)
        priors = row.to(torch.float32).to('cuda:0')[None, :].expand(B, A).contiguous()
        values = torch.zeros(B, dtype=torch.float32, device='cuda:0')
        ev = lambda states, legal: (priors, values)

    def rounds(search):
        for _ in range(T):
            search.backup(*ev(*search.select()))

    search = gogame.PuctSearch(roots, T, c=args.c, komi=7.5, leaves=L, capacity=capacity)
    for mv in range(args.moves):
        s_search, _ = timed(lambda: rounds(search))
        res = search._result()
        visits_before, nodes_before = res.root_visits.double().clone(), res.nodes.double().clone()
        acts = gogame._best_legal(gogame._ON_DEVICE, res.legal, res.visits.long())
        best = res.visits.gather(1, acts.clamp(min=0)[:, None])[:, 0].double()
        # advance on copies of the tree (alternating with the construction of a fresh search), then once for real
        names = ('_boards', '_child', '_prior', '_links', '_stats', '_nodes')
        saved = [getattr(search, n).clone() for n in names]

        def advance():
            for n, t in zip(names, saved):
                getattr(search, n).copy_(t)
            torch.cuda.synchronize()
            return timed(lambda: search.advance(acts, check=False))[0]

        nxt = search.root_states()   # (a fresh search costs the same on any R boards)
        fresh = lambda: timed(lambda: gogame.PuctSearch(nxt, T, c=args.c, komi=7.5, leaves=L, capacity=capacity))[0]
        adv, new = [], []
        for _ in range(args.reps):
            adv.append(advance())
            new.append(fresh())
        med = lambda ts: sorted(ts)[len(ts) // 2]
        kept = search._kept.double()
        if not args.reuse:
            search = gogame.PuctSearch(search.root_states(), T, c=args.c, komi=7.5, leaves=L, capacity=capacity)
        yield dict(base, metric='puct_advance_per_move', evaluator=args.evaluator, leaves=L, rounds=T, move=mv, reuse=args.reuse,
                   capacity=capacity, search_ms=s_search * 1e3, advance_ms=med(adv) * 1e3, fresh_search_ms=med(new) * 1e3,
                   ratio_fresh_over_advance=med(new) / med(adv), root_visits_after_search=float(visits_before.mean()),
                   nodes_before=float(nodes_before.mean()), kept_nodes=float(kept.mean()),
                   share_nodes_kept=float((kept / nodes_before).mean()), share_visits_kept=float((best / visits_before).mean()),
                   kept_visits=float(best.mean()), tree_full=float((nodes_before >= capacity).double().mean()))


def _selfplay(args, gogame, torch, roots, base, L):
    """The --selfplay comparison: one result."""
    import numpy as np
    R, N, T, M = base['roots'], base['size'], base['iterations'], args.moves
    A, B = N * N + 1, R * (L or 1)
    capacity = args.capacity_factor * T * (L or 1) + 1
    priors = torch.full((B, A), 1.0 / A, dtype=torch.float32, device='cuda:0')
    values = torch.zeros(B, dtype=torch.float32, device='cuda:0')
    null = lambda states, legal: (priors, values)
    noise = gogame.dirichlet_noise(args.alpha)

    def ours():
        return gogame.puct_selfplay(roots, M, T, null, c=args.c, komi=7.5, leaves=L, capacity=capacity, noise=noise, eps=args.eps,
                                    sample_moves=M)

    def theirs():
        states, host_rng = roots, np.random.default_rng(1)
        acts, pis = np.zeros((R, M), np.int64), np.zeros((R, M, A), np.float32)
        for mv in range(M):
            search = gogame.PuctSearch(states, T, c=args.c, komi=7.5, leaves=L)
            for t in range(T):
                st, legal = search.select()
                p = priors
                if t == 0:   # round 0 hands out the roots (slot 0 of every root): the only place noise can go
                    rows = slice(None, None, L or 1)
                    p = priors.clone()
                    p[rows] = (1 - args.eps) * p[rows] + args.eps * noise(mv, legal[rows])
                search.backup(p, values)
            visits = search.result().visits.cpu().numpy().astype(np.float64)   # (the synchronisation)
            total = visits.sum(axis=1, keepdims=True)
            pi = np.divide(visits, total, out=np.zeros_like(visits), where=total > 0)
            pis[:, mv] = pi
            cum = np.cumsum(pi, axis=1)
            draw = (cum < host_rng.random((R, 1))).sum(axis=1).clip(max=A - 1)
            acts[:, mv] = np.where(total[:, 0] > 0, draw, -1)
            states = search._played_states(torch.from_numpy(acts[:, mv]).to('cuda:0'))
        return acts, pis, states

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    wall(ours), wall(theirs)   # warm-up
    ta, tb = [], []
    for _ in range(args.reps):
        ta.append(wall(ours))
        tb.append(wall(theirs))
    med = lambda ts: sorted(t for t, _ in ts)[len(ts) // 2]
    rec = ta[-1][1]
    return dict(base, metric='puct_selfplay_wall_s', evaluator='null', leaves=L, rounds=T, moves=M, capacity=capacity,
                alpha=args.alpha, eps=args.eps, seconds_selfplay=med(ta), seconds_fresh_search_host_pi=med(tb),
                ratio=med(tb) / med(ta), ms_per_move_selfplay=med(ta) / M * 1e3, ms_per_move_fresh=med(tb) / M * 1e3,
                mean_length=float(rec.lengths.double().mean()), pi_bytes=4 * R * M * A)


def _mean_leaf_depth(parent, nodes):
    """Mean depth of the nodes in use (the root at 0), from the parent links: how deep the walks of the search went."""
    import torch
    R, NN = parent.shape
    depth = torch.zeros((R, NN), dtype=torch.int64, device=parent.device)
    for x in range(1, NN):   # (parents have smaller ids)
        depth[:, x] = torch.gather(depth, 1, parent[:, x].clamp(min=0).long()[:, None])[:, 0] + 1
    used = torch.arange(NN, device=parent.device)[None, :] < nodes[:, None]
    return float((depth * used).sum() / used.sum().clamp(min=1))


if __name__ == '__main__':
    main()
