"""-m gpu: gg_batch_rollout_ws - the fused rollout with a caller-owned workspace (include/gymgo_amd.h) - against its twin
gg_batch_rollout on a copy and the pinned C oracle.  The byte-plane load of k_rollout5 (gymgo_amd/csrc/gg_v5_kernel.h) takes the
liberty classes of a board from the workspace when its stones stand there exactly and analyses it otherwise; states, generator
states, last actions and step counters must not depend on what the workspace holds.

The library is sized for FOUR compute units (GYMGO_AMD_CUS=4, read once per process: one child process runs every case and
reports per case), so k_rollout5 serves 19x19 launches of >= 8 plies from 513 games on and 9x9 / 13x13 from 637 on
(gg_kernels.hip: use_rollout5, 4 * 32 and 5 * 32 - 1 games per CU).  Whether the load really skipped an analysis cannot be seen
from here: the -DGG_AB_WS counter build says (docs/history/r09.md).
Reference loop: gym_go/envs/go_env.py:49-81 over gym_go/gogame.py:34-87.
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r'''
import gc, os, sys, traceback
sys.path.insert(0, %r)
import numpy as np
import torch
from gymgo_amd import gogame, _lib
from oracle import c_oracle
L = _lib.lib()
CUS = 4
assert L.gg_device_cus() == CUS
DEV = 'cuda'
I32, I64, U8 = torch.int32, torch.int64, torch.uint8


def raw(st, rng, la, sd, ws, F, auto_reset):
    """One launch through the C-ABI: gg_batch_rollout_ws with a workspace, gg_batch_rollout without."""
    B, N = st.shape[0], st.shape[2]
    p = lambda t, d, n: _lib.dev_ptr(t, d, n)
    if ws is None:
        code = L.gg_batch_rollout(p(st, U8, 'st'), p(rng, I64, 'rng'), p(la, I32, 'la'), p(sd, I64, 'sd'), B, N, F, int(auto_reset),
                                  _lib.stream_ptr(st.device))
    else:
        code = L.gg_batch_rollout_ws(p(st, U8, 'st'), p(rng, I64, 'rng'), p(la, I32, 'la'), p(sd, I64, 'sd'), p(ws, I32, 'ws'),
                                     B, N, F, int(auto_reset), _lib.stream_ptr(st.device))
    assert code == 0, code


def midgame(B, N, plies, seed, auto_reset=True):
    st = gogame.batch_init_state(B, N, device=DEV)
    rng = gogame.rng_seed(B, seed, 0, DEV)
    raw(st, rng, None, None, None, plies, auto_reset)
    return st, rng


class Twin:
    """The same games twice: `a` goes through gg_batch_rollout_ws, `b` through gg_batch_rollout."""

    def __init__(self, st, rng, ws=None):
        B, N = st.shape[0], st.shape[2]
        self.B, self.N = B, N
        self.a, self.b = (st.clone(), rng.clone()), (st.clone(), rng.clone())
        self.la = [torch.full((B,), -9, dtype=I32, device=DEV) for _ in range(2)]
        self.sd = [torch.zeros(B, dtype=I64, device=DEV) for _ in range(2)]
        self.ws = torch.zeros((B, 5 * N + 1), dtype=I32, device=DEV) if ws is None else ws

    def launch(self, F, auto_reset, what=''):
        for la in self.la:
            la.fill_(-9)
        raw(self.a[0], self.a[1], self.la[0], self.sd[0], self.ws, F, auto_reset)
        raw(self.b[0], self.b[1], self.la[1], self.sd[1], None, F, auto_reset)
        bad = torch.nonzero((self.a[0] != self.b[0]).reshape(self.B, -1).any(dim=1)).flatten()
        assert bad.numel() == 0, (what, 'states', bad[:8].tolist())
        assert torch.equal(self.a[1], self.b[1]), (what, 'rng')
        assert torch.equal(self.la[0], self.la[1]), (what, 'last_actions')
        assert torch.equal(self.sd[0], self.sd[1]), (what, 'steps_done')

    def edit(self, fn):
        for st, _ in (self.a, self.b):
            fn(st)


def case_twin_runs_and_oracle():
    B, N = 641, 19      # odd: a ragged last wave and a half-filled last pair
    st, rng = midgame(B, N, 150, 11)
    t = Twin(st, rng)
    for k in range(3):
        if k == 2:
            h_st, h_rng = t.b[0][::8].contiguous().cpu().numpy(), t.b[1][::8].contiguous().cpu().numpy().view(np.uint64).copy()
        t.launch(8, True, 'launch %%d' %% k)
    assert int(t.ws.ne(0).sum()) > 0      # the launches did leave something behind
    want, want_rng, want_last = c_oracle.batch_rollout_mt(h_st, h_rng, 8, True)
    assert np.array_equal(t.a[0][::8].contiguous().cpu().numpy(), want)
    assert np.array_equal(t.a[1][::8].contiguous().cpu().numpy().view(np.uint64), want_rng)
    assert np.array_equal(t.la[0][::8].contiguous().cpu().numpy(), want_last)
    assert np.array_equal(t.sd[0].cpu().numpy(), np.full(B, 24, np.int64))


def case_external_edits():
    B, N = 641, 19
    st, rng = midgame(B, N, 150, 12)
    other, _ = midgame(B, N, 210, 13)
    t = Twin(st, rng)
    t.launch(8, True, 'launch 1')
    cur = t.b[0].cpu().numpy()
    one = cur[100].copy()                      # board 100: the workspace entry with ONE stone taken off, the mask recomputed
    r, c = np.argwhere(one[0] == 1)[0]
    one[0, r, c] = 0
    one[3] = c_oracle.compute_invalid_moves(one, 1 - int(one[2, 0, 0]))
    one = torch.from_numpy(one).to(DEV)

    def edits(s):
        s[0:50] = other[0:50]                  # whole boards replaced by other positions
        s[100] = one
        s[200] = other[200]                    # only board 2i of a pair
        s[301] = other[301]                    # only board 2i + 1 of a pair
        s[400] = 0                             # a board set to empty
        s[640] = other[640]                    # the single board of the half-filled last pair
    t.edit(edits)
    t.launch(8, True, 'launch 2 after edits')
    t.launch(8, True, 'launch 3')
    # a workspace taken from a different batch: every board mismatches
    ws_other = Twin(other, rng)
    ws_other.launch(8, True, 'other batch')
    t2 = Twin(st, rng, ws=ws_other.ws)
    t2.launch(8, True, 'foreign workspace')
    t2.launch(8, True, 'foreign workspace, launch 2')


def case_frozen_games():
    B, N = 641, 19
    st, rng = midgame(B, N, 640, 14, auto_reset=False)      # about half of the games have ended: frozen boards in every wave
    done = st[:, 5, 0, 0] != 0
    assert 50 < int(done.sum()) < B - 50, int(done.sum())
    t = Twin(st, rng)
    t.launch(8, False, 'frozen 1')
    assert torch.equal(t.a[0][done], st[done])                # untouched boards are not rewritten ...
    t.launch(8, False, 'frozen 2')                            # ... and are still right on the next launch
    t.launch(8, True, 'frozen boards reset')


def case_resetting_games():
    B, N = 641, 19
    st, rng = midgame(B, N, 600, 15, auto_reset=False)       # many games a few plies before their end, some over
    before = (st[:, 0] | st[:, 1]).reshape(B, -1).sum(dim=1)
    t = Twin(st, rng)
    t.launch(8, True, 'reset 1')
    t.launch(8, True, 'reset 2')
    after = (t.a[0][:, 0] | t.a[0][:, 1]).reshape(B, -1).sum(dim=1)
    assert int((after + 100 < before).sum()) > 0              # boards were reset inside the launches
    mid = t.a[0].clone()
    for _ in range(6):                                        # games that end INSIDE a launch, with a workspace that knows them
        t.launch(8, True, 'reset later')
    assert not torch.equal(mid, t.a[0])


def case_small_boards():
    B = CUS * (5 * 32 - 1) + 1      # 637: just above the take-over of 9x9 / 13x13 (use_rollout5), odd
    for N in (9, 13):               # (13x13: the row stride of 20 words)
        st, rng = midgame(B, N, 40, 16 + N)
        t = Twin(st, rng)
        for k in range(3):
            t.launch(8, True, '%%dx%%d launch %%d' %% (N, N, k))
        assert int(t.ws.ne(0).sum()) > 0
        h_st, h_rng = t.b[0][::8].contiguous().cpu().numpy(), t.b[1][::8].contiguous().cpu().numpy().view(np.uint64).copy()
        t.launch(9, True, '%%dx%%d launch 3' %% (N, N))
        want, want_rng, want_last = c_oracle.batch_rollout_mt(h_st, h_rng, 9, True)
        assert np.array_equal(t.a[0][::8].contiguous().cpu().numpy(), want) and np.array_equal(t.la[0][::8].contiguous().cpu().numpy(), want_last)


def case_other_dispatch_targets():
    N = 19
    # (B, plies): k_rollout4 (32 .. 128 games per CU), k_rollout_lat (<= 31 games per CU, >= 8 plies), k_rollout5's batch on a
    # launch too short for it
    for B, F in ((300, 8), (100, 8), (641, 7)):
        st, rng = midgame(B, N, 60, 20 + B)
        fill = torch.arange(B * (5 * N + 1), dtype=I32, device=DEV).reshape(B, 5 * N + 1) * 2654435 + 7
        t = Twin(st, rng, ws=fill.clone())
        t.launch(F, True, 'B %%d F %%d' %% (B, F))
        t.launch(F, False, 'B %%d F %%d' %% (B, F))
        assert torch.equal(t.ws, fill), (B, F)      # not this kernel's business: the bytes stay


def case_python_attachment():
    B, N = 641, 19
    st0, rng0 = midgame(B, N, 150, 31)
    other, _ = midgame(B, N, 210, 32)
    table = gogame._ROLLOUT_WS
    table.clear()
    st, rng = st0.clone(), rng0.clone()
    ref = Twin(st0, rng0)
    gogame.batch_rollout(st, rng, 8, True)
    ref.launch(8, True)
    assert [e[1] for e in table.values()] == [None]                # recorded, nothing allocated
    gogame.batch_rollout(st, rng, 8, True)
    ref.launch(8, True)
    assert len(table) == 1 and tuple(table[id(st)][1].shape) == (B, 5 * N + 1)
    ws = table[id(st)][1]
    gogame.batch_rollout(st, rng, 8, True)
    ref.launch(8, True)
    assert torch.equal(st, ref.b[0]) and torch.equal(rng, ref.b[1])
    assert table[id(st)][1] is ws and int(ws.ne(0).sum()) > 0      # the third call used it
    gogame.batch_rollout(st[64:], rng[64:], 8, True)               # a slice never gets a workspace
    raw(ref.b[0][64:], ref.b[1][64:], None, None, None, 8, True)
    gc.collect()
    assert len(table) == 1
    st.copy_(other)                                                # other positions in place between calls
    ref.b[0].copy_(other)
    gogame.batch_rollout(st, rng, 8, True)
    raw(ref.b[0], ref.b[1], None, None, None, 8, True)
    assert torch.equal(st, ref.b[0]) and torch.equal(rng, ref.b[1])
    mine = torch.zeros((B, 5 * N + 1), dtype=I32, device=DEV)      # the caller's own workspace
    gogame.batch_rollout(st, rng, 8, True, workspace=mine)
    raw(ref.b[0], ref.b[1], None, None, None, 8, True)
    assert torch.equal(st, ref.b[0]) and int(mine.ne(0).sum()) > 0
    try:
        gogame.batch_rollout(st, rng, 8, True, workspace=mine[:, :5])
        raise SystemError('a workspace of the wrong shape was accepted')
    except ValueError:
        pass
    del st, ws
    gc.collect()
    assert len(table) == 0                                         # the entry leaves with its tensor
    os.environ['GYMGO_AMD_ROLLOUT_WS'] = '0'
    try:
        st, rng = st0.clone(), rng0.clone()
        for _ in range(3):
            gogame.batch_rollout(st, rng, 8, True)
        assert len(table) == 0
    finally:
        del os.environ['GYMGO_AMD_ROLLOUT_WS']
    ref2 = Twin(st0, rng0)
    for _ in range(3):
        ref2.launch(8, True)
    assert torch.equal(st, ref2.b[0]) and torch.equal(rng, ref2.b[1])


def case_symbol_and_arguments():
    import ctypes
    assert 'gg_batch_rollout_ws' in _lib.EXPORTS and hasattr(ctypes.CDLL(_lib.LIB_PATH), 'gg_batch_rollout_ws')
    f = L.gg_batch_rollout_ws
    st, rng = midgame(8, 9, 4, 40)
    ws = torch.zeros((8, 46), dtype=I32, device=DEV)
    sp, rp, wp = st.data_ptr(), rng.data_ptr(), ws.data_ptr()
    assert f(sp, rp, None, None, None, 8, 9, 4, 1, None) == -2      # GG_E_NULLPTR: no workspace
    assert f(None, rp, None, None, wp, 8, 9, 4, 1, None) == -2
    assert f(sp, None, None, None, wp, 8, 9, 4, 1, None) == -2
    assert f(sp, rp, None, None, wp, 8, 9, -1, 1, None) == -3       # GG_E_BADARG, as gg_batch_rollout
    assert f(sp, rp, None, None, wp, 8, 20, 4, 1, None) == -1       # GG_E_BADSIZE
    assert f(sp, rp, None, None, wp, -1, 9, 4, 1, None) == -1
    assert f(None, None, None, None, None, 0, 9, 4, 1, None) == 0   # an empty batch is no work
    assert f(sp, rp, None, None, wp, 8, 9, 0, 1, None) == 0         # nor are zero plies
    torch.cuda.synchronize()


for name, fn in sorted(globals().items()):
    if name.startswith('case_'):
        try:
            fn()
            torch.cuda.synchronize()
            print('CASE %%s OK' %% name[5:], flush=True)
        except Exception:
            print('CASE %%s FAIL %%s' %% (name[5:], traceback.format_exc()[-1800:].replace('\n', ' | ')), flush=True)
''' % ROOT


@pytest.fixture(scope='module')
def cases():
    env = dict(os.environ)
    env['GYMGO_AMD_CUS'] = '4'
    env.pop('GYMGO_AMD_ROLLOUT_WS', None)
    p = subprocess.run([sys.executable, '-c', SCRIPT], env=env, capture_output=True, text=True, timeout=600)
    out = {}
    for line in p.stdout.splitlines():
        if line.startswith('CASE '):
            _, name, rest = line.split(' ', 2)
            out[name] = rest
    assert p.returncode == 0 and out, (p.stdout[-1500:], p.stderr[-3000:])
    return out


def _ok(cases, name):
    assert cases.get(name) == 'OK', cases.get(name, 'the case did not run')


def test_ws_twin_runs_three_launches_and_the_oracle(cases):
    _ok(cases, 'twin_runs_and_oracle')


def test_ws_external_edits_between_launches_and_a_foreign_workspace(cases):
    _ok(cases, 'external_edits')


def test_ws_frozen_games_are_not_rewritten_and_stay_right(cases):
    _ok(cases, 'frozen_games')


def test_ws_games_that_reset_inside_the_launch(cases):
    _ok(cases, 'resetting_games')


def test_ws_9x9_and_13x13_just_above_their_take_over(cases):
    _ok(cases, 'small_boards')


def test_ws_other_dispatch_targets_leave_the_workspace_alone(cases):
    _ok(cases, 'other_dispatch_targets')


def test_ws_python_attachment_table(cases):
    _ok(cases, 'python_attachment')


def test_ws_symbol_resolves_and_bad_arguments_are_refused(cases):
    _ok(cases, 'symbol_and_arguments')
