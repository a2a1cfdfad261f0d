"""CPU: the premises of tests/test_gpu_amaf.py, asserted on the expectations of tests/mc_amaf_expect.py - the playout cases hold
replayed captures, early passes and cut-off playouts; the expectation without its amaf IS mc_expect's; the RAVE searches go
deep, meet the exclusion of the tree moves and differ from the plain search; the value and U at hand-computed points; and the
binding table of the family (_lib.ABI_AMAF) against include/gymgo_amd_amaf.h."""
import ctypes
import math
import os

import numpy as np
import pytest

import mc_amaf_expect as ma
import mc_expect as mc
import mc_policy_expect as mp
import mc_tactics_expect as mt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_first_play_map_by_hand():
    # 3x3, black starts: B 4, W 0, B pass, W 4 (a later play at 4: nothing), B 0 (nothing), W 8
    acts = np.array([[4, 0, 9, 4, 0, 8, -1, -1]], np.int32)
    m = ma.first_play_maps(acts, np.array([False]), 3)
    assert np.flatnonzero(m[0, 0]).tolist() == [4] and np.flatnonzero(m[0, 1]).tolist() == [0, 8]
    # white starts: the colours swap; the pass flips the colour like any ply
    m = ma.first_play_maps(acts, np.array([True]), 3)
    assert np.flatnonzero(m[0, 1]).tolist() == [4] and np.flatnonzero(m[0, 0]).tolist() == [0, 8]
    acts = np.array([[9, 2, 9, -1]], np.int32)           # pass, then WHITE plays 2
    assert np.flatnonzero(ma.first_play_maps(acts, np.array([False]), 3)[0, 1]).tolist() == [2]
    replay, early = ma.sequence_facts(np.array([[4, 0, 9, 4, 0, 8, -1, -1], [1, 2, 3, 9, 9, -1, -1, -1]], np.int32), np.array([False, False]), 3)
    assert replay.tolist() == [True, False] and early.tolist() == [True, False]


def test_playout_cases_hold_what_the_device_test_relies_on():
    replayed = early = cut = 0
    for N, policy, is_cut in ma.all_playout_cases():
        e = ma.playout_case(N, policy, is_cut)
        roots = ma.playout_roots(N)
        assert roots[0].sum() == 0 and roots[2, 5].all() and not roots[1, 5].any() and roots[1, :2].any()
        r, p = ma.sequence_facts(e['sequences'], e['start_white'], N)
        replayed += int(r.sum())
        early += int(p.sum())
        cut += int(e['unfinished'].sum()) if is_cut else 0
        # without its amaf the expectation is the one the existing tests use
        cap = ma.PO_CUT[N] if is_cut else ma.cs.full_cap(N)
        plain = (mc.expected_playouts, mp.expected_playouts_policy, mt.expected_playouts_tactical)[policy](
            roots, ma.PO_K, cap, komi=ma.PO_KOMI, base_seed=ma.PO_SEED + N, with_ownership=True)
        for k in mc.KEYS + ('ownership',):
            assert np.array_equal(e[k], plain[k]) and e[k].dtype == plain[k].dtype, (N, policy, is_cut, k)
        # the sum over the points = the distinct points each colour played first, over the playouts; a point has one owner
        maps = e['maps']
        assert not (maps[:, 0] & maps[:, 1]).any()
        for c in (0, 1):
            distinct = 0
            for b, row in enumerate(e['sequences']):
                seen = {}
                for t, a in enumerate(row[row >= 0]):
                    if a < N * N:
                        seen.setdefault(int(a), bool(e['start_white'][b]) ^ bool(t & 1))
                distinct += sum(1 for v in seen.values() if int(v) == c)
            assert int(e['amaf'][:, c, 0].sum()) == distinct, (N, policy, is_cut, c)
        assert (e['amaf'][:, :, 1] + e['amaf'][:, :, 2] <= e['amaf'][:, :, 0]).all()
        assert not e['amaf'][2].any()                     # the finished root plays nothing
    assert replayed > 0 and early > 0 and cut > 0, (replayed, early, cut)


def test_log_cases_have_mid_game_and_ended_boards():
    for N in ma.SIZES:
        st = ma.log_boards(N)
        ended = st[:, 5, 0, 0] != 0
        assert len(st) == ma.LOG_B and 3 <= ended.sum() <= 30 and (st[:, :2].reshape(len(st), -1).any(axis=1) & ~ended).sum() >= ma.LOG_B // 4
    states, rng, acts = ma.log_case(5, 0)
    assert acts.shape == (ma.LOG_B, 33) and (acts[states[:, 5, 0, 0] != 0] == -1).all() and (acts[:, 0] >= 0).sum() >= 60
    assert ((acts >= 0).sum(axis=1) < 33).sum() > (states[:, 5, 0, 0] != 0).sum()       # some game ends inside the launch


def test_rave_cases_go_deep_meet_the_exclusion_and_differ_from_the_plain_search():
    deep = met = differ = False
    for N in ma.RAVE_SIZES:
        roots = ma.rave_roots(N)
        assert roots[3, 5].all() and not roots[:3, 5].any()
        for c in ma.RAVE_CS:
            e, p = ma.rave_case(N, c), ma.plain_case(N, c)
            deep = deep or max(t.max_depth for t in e['trees']) >= 3
            met = met or bool(e['replayed'].any())
            differ = differ or not np.array_equal(mc.most_visited(e), mc.most_visited(p))
            assert (e['root_visits'] == ma.RAVE_I * ma.RAVE_K).all()
            # the plain search at these sizes is one ply deep wherever the root has more than I actions
            if N >= 5:
                assert all(cs_deep == 0 for cs_deep in (int((t.parent[:len(t.boards)] > 0).sum()) for t in p['trees'][2:3]))
            # a node's pair never counts more simulations than went through the node
            for t in e['trees']:
                n = len(t.boards)
                assert (t.node_amaf[:n, :, 0] <= t.stats[:n, 0][:, None]).all() and (t.node_amaf[:n, :, 1] <= 2 * t.node_amaf[:n, :, 0]).all()
                assert not t.node_amaf[n:].any()
    assert deep and met and differ
    e = ma.past_capacity_case()
    assert (e['nodes'][:3] == ma.PAST_I + 1).all() and (e['root_visits'] == (ma.PAST_I + ma.PAST_EXTRA) * ma.RAVE_K).all()


def test_value_and_u_at_hand_computed_points():
    k, fpu = 50.0, 1.0
    # both counts positive: n = 10, s = 12 -> q = 0.6; n~ = 40, s~ = 20 -> q~ = 0.25; beta = 40 / (10 + 40 + 400 / 50) = 40 / 58
    beta = 40.0 / 58.0
    v = (1.0 - beta) * 0.6 + beta * 0.25
    assert ma.rave_value(10, 12, 40, 20, k, fpu) == v
    assert abs(v - (18 * 0.6 + 40 * 0.25) / 58) < 1e-15
    L = math.log(100.0)
    assert ma.rave_u(10, 12, 40, 20, L, 0.5, k, fpu) == v + 0.5 * math.sqrt(L / 10.0)
    assert ma.rave_u(10, 12, 40, 20, L, 0.0, k, fpu) == v
    # one count positive
    assert ma.rave_value(8, 12, 0, 0, k, fpu) == 0.75 and ma.rave_u(8, 12, 0, 0, L, 1.0, k, fpu) == 0.75 + math.sqrt(L / 8.0)
    assert ma.rave_value(0, 0, 16, 8, k, fpu) == 0.25 and ma.rave_u(0, 0, 16, 8, L, 1.0, k, fpu) == 0.25     # n = 0: no exploration term
    # neither: the first-play urgency
    assert ma.rave_value(0, 0, 0, 0, k, 0.55) == 0.55 and ma.rave_u(0, 0, 0, 0, L, 3.0, k, 0.55) == 0.55
    # beta falls from 1 towards 0 as n grows, and is n~ / (n + n~) for a huge k
    b = lambda n, nt, kk: float(nt) / (float(n) + float(nt) + (float(n) * float(nt)) / kk)
    assert b(1, 40, k) > b(10, 40, k) > b(1000, 40, k) and abs(b(10, 40, 1e300) - 0.8) < 1e-15
    # no fused multiply-add hides in the restatement: the value is the two rounded products' rounded sum
    n, s, nt, st = 7, 9, 13, 11
    q, qt = 9.0 / 14.0, 11.0 / 26.0
    bb = 13.0 / (7.0 + 13.0 + (7.0 * 13.0) / 50.0)
    assert ma.rave_value(n, s, nt, st, k, fpu) == (1.0 - bb) * q + bb * qt


def test_binding_table_matches_the_header(native_built, monkeypatch):
    import torch
    import test_host_abi as tha
    from gymgo_amd import _lib
    decls = tha.header_declarations('gymgo_amd_amaf.h')
    assert list(decls) == ['gg_batch_rollout_tracked_log', 'gg_playouts_advance_amaf', 'gg_uct_select_rave', 'gg_uct_backup_rave']
    monkeypatch.setitem(tha._POINTEES, 'uint16_t', 'int16')      # the move log: uint16_t * is an int16 tensor
    assert tha._abi_mismatches(decls, _lib.ABI_AMAF) == []
    assert _lib.EXPORTS_AMAF == tuple(decls) and not set(decls) & set(_lib.EXPORTS)
    f = 'gg_uct_select_rave'
    dropped = dict(_lib.ABI_AMAF, **{f: _lib.ABI_AMAF[f][:5] + _lib.ABI_AMAF[f][6:]})
    assert any('18 parameters in the header, 17 in the table' in b for b in tha._abi_mismatches(decls, dropped))   # the comparison can fail
    # the two calls that extend an existing one take its parameter list and add to it
    names = lambda ps: [p.name for p in ps]
    assert names(_lib.ABI_AMAF['gg_playouts_advance_amaf'])[:-5] == names(_lib.ABI_TACTICS['gg_playouts_advance_policy2'])[:-1]
    assert names(_lib.ABI_AMAF['gg_playouts_advance_amaf'])[-5:] == ['log', 'first', 'mark', 'amaf', 'hip_stream']
    for f, (argtypes, restype) in _lib._SIGNATURES_AMAF.items():
        assert restype is ctypes.c_int32
        assert argtypes == [p.kind if isinstance(p.kind, type) else ctypes.c_void_p for p in _lib.ABI_AMAF[f]]
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in decls:
        assert hasattr(L, name), name
    assert native_built.gg_version() == _lib.ABI_VERSION == 5
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in list(decls) + ['gymgo_amd_amaf.h']:
        assert name in doc, name


def test_argument_checks_before_any_device_work(native_built):
    """The checks of the C entry points that come before any pointer is looked at, in the order the header gives."""
    L = native_built
    BADSIZE, NULLPTR, BADARG = -1, -2, -3
    log = lambda B, N, plies, policy: L.gg_batch_rollout_tracked_log(None, None, None, None, B, N, plies, policy, None, None)
    assert log(4, 9, 4097, 0) == BADARG and log(4, 9, -1, 0) == BADARG and log(4, 9, 8, 3) == BADARG and log(4, 9, 8, -1) == BADARG
    assert log(4, 20, 8, 0) == BADSIZE and log(4, 1, 8, 2) == BADSIZE and log(-1, 9, 8, 0) == BADSIZE
    assert log(4, 20, 4097, 0) == BADARG                                                         # arguments before sizes, as _policy2
    assert log(0, 9, 8, 0) == 0                                                                   # B = 0: no work
    assert log(4, 9, 4096, 2) == NULLPTR
    adv = lambda chunk, max_plies, policy, chunks=1: L.gg_playouts_advance_amaf(None, 2, 9, 3, 0, 1, max_plies, chunk, 0.0, chunks, policy, None,
                                                                                None, None, None, 4, None, None, None, None, None, None, None, None, None)
    assert adv(32, 64, 0) == NULLPTR and adv(32, 65, 0) == BADARG
    sel = lambda I, K, k, fpu, c=1.0, N=9: L.gg_uct_select_rave(1, N, I, K, c, k, fpu, None, None, None, None, None, None, None, None, None,
                                                                None, None)
    assert sel(4, 2, 50.0, 1.0) == NULLPTR                                                        # every check passed: the NULL pointers
    assert sel(1 << 20, 1 << 10, 50.0, 1.0) == BADSIZE and sel((1 << 20) - 1, 1 << 10, 50.0, 1.0) == NULLPTR     # 2 I K = 2^31 / below it
    for k, fpu in ((0.0, 1.0), (-1.0, 1.0), (math.inf, 1.0), (math.nan, 1.0), (50.0, math.inf), (50.0, math.nan)):
        assert sel(4, 2, k, fpu) == BADARG, (k, fpu)
    assert sel(4, 2, 50.0, 1.0, c=-1.0) == BADARG and sel(4, 2, 50.0, 1.0, N=20) == BADSIZE and sel(0, 2, 50.0, 1.0) == BADARG
    back = lambda I, K: L.gg_uct_backup_rave(1, 9, I, K, None, None, None, None, None, None, None, None, None, None, None, None)
    assert back(1 << 20, 1 << 10) == BADSIZE and back(4, 2) == NULLPTR and back(0, 2) == BADARG
