"""Games of flat Monte Carlo under one playout policy against flat Monte Carlo under another; prints one JSON line.

  python tools/playout_strength.py [--games 500] [--k 8] [--size 9] [--komi 7.5] [--policy tactical | pattern] [--against no_eye_fill | tactical]

`--games` games with `--policy` as black and as many with it as white, from the empty board: every move is
gogame.flat_mc_actions(states, k, komi, policy=the mover's policy) - equal playouts per candidate move on either side -, the games
of a half move in lockstep (game g differs from the others through its job numbers: the root index enters every playout's
seed; the seed changes with the ply), each game to two passes or 8 N^2 plies, scored by area against komi as it stands.
win_share = the policy's wins / decided games, ci95 its normal-approximation binomial interval.  For the record only
(DESIGN 34): one opponent, flat Monte Carlo, no claim beyond the line it prints.

  python tools/playout_strength.py --rave-equiv 50 [--iters 64] [--k 4] [--games 200] [--policy uniform]

RAVE against plain UCT: every move of one side is gogame.uct_actions(states, iters, k, rave_equiv=...), of the other
gogame.uct_actions(states, iters, k) - equal iterations and playouts, the same playout policy (--policy) on both sides; win_share is
the RAVE side's (--rave-c: its exploration constant, where it is to differ from the plain side's sqrt(2)).  The same lockstep
games, colours, cap, scoring and interval."""
import argparse
import json
import math
import time

import mc_bench   # (puts the repository on sys.path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--games', type=int, default=500)
    ap.add_argument('--k', type=int, default=8)
    ap.add_argument('--size', type=int, default=9)
    ap.add_argument('--komi', type=float, default=7.5)
    ap.add_argument('--policy', default='tactical')
    ap.add_argument('--against', default='no_eye_fill')
    ap.add_argument('--rave-equiv', type=float, default=None)
    ap.add_argument('--iters', type=int, default=64)
    ap.add_argument('--rave-c', type=float, default=None, help="exploration constant of the RAVE side (default: batch_uct's, as the plain side)")
    args = ap.parse_args()

    import torch
    from gymgo_amd import gogame
    N, K, half, cap = args.size, args.k, args.games, 8 * args.size * args.size
    res = {'size': N, 'komi': args.komi, 'playouts_per_move': K, 'games_per_colour': half, 'ply_cap': cap, 'policy': args.policy,
           'against': args.against}
    rave = args.rave_equiv is not None
    if rave:
        res.update(mode='rave_vs_uct', rave_equiv=args.rave_equiv, iterations=args.iters, against='plain uct', rave_c=args.rave_c)
    t0 = time.time()
    wins, unfinished = [0, 0], 0
    for as_black in (True, False):
        st = gogame.batch_init_state(half, N, device='cuda')
        for ply in range(cap):
            live = torch.nonzero(gogame.batch_game_ended(st) == 0)[:, 0]
            if live.numel() == 0:
                break
            pol = args.policy if (ply % 2 == 0) == as_black else args.against
            sub = st[live].contiguous()
            seed = 1000 * ply + (7 if as_black else 13)
            if rave:
                mine = (ply % 2 == 0) == as_black
                kw = {'c': args.rave_c} if mine and args.rave_c is not None else {}
                act = gogame.uct_actions(sub, args.iters, K, komi=args.komi, seed=seed, policy=args.policy,
                                         rave_equiv=args.rave_equiv if mine else None, **kw)
            else:
                act = gogame.flat_mc_actions(sub, K, komi=args.komi, seed=seed, policy=pol)
            st[live] = gogame.batch_next_states(sub, act.to(torch.int32))
        unfinished += int((gogame.batch_game_ended(st) == 0).sum())
        w = gogame.batch_winning(st, args.komi)
        b, wh = int((w > 0).sum()), int((w < 0).sum())
        wins[0] += b if as_black else wh
        wins[1] += wh if as_black else b
        res['black_wins_as_black' if as_black else 'black_wins_as_white'] = b
    n = wins[0] + wins[1]
    p = wins[0] / n
    hw = 1.96 * math.sqrt(p * (1 - p) / n)
    res.update(wins=wins[0], losses=wins[1], games=n, unfinished=unfinished, win_share=p, ci95=[p - hw, p + hw],
               seconds=time.time() - t0)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
