"""The plane of M of k_rollout5<19, ..> against the registers it mirrors, on a -DGG_AB_MCHECK build
(make -C gymgo_amd/csrc ab EXTRA=-DGG_AB_MCHECK): every row a job lane reads out of the plane is compared with the row the board's
lanes hold, over launches that load from byte planes (without a workspace, with one that misses, with one that hits) and from tracked
boards, from empty and from mid-game boards, with resets inside the launch and with ragged waves.  Prints rows that differ / compared;
exits 1 if any differ.
    LIB=tools/exp/libgymgo_ab.so python tools/exp/r5_mplane_check.py"""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
from gymgo_amd import _lib
_lib.LIB_PATH = os.path.join(ROOT, os.environ.get('LIB', 'tools/exp/libgymgo_ab.so'))
from gymgo_amd import gogame
L = ctypes.CDLL(_lib.LIB_PATH)
L.gg_ab_mcheck_read_r5.argtypes = [ctypes.c_void_p]; L.gg_ab_mcheck_read_r5.restype = ctypes.c_int32
buf = (ctypes.c_ulonglong * 2)()
assert L.gg_ab_mcheck_read_r5(buf) == 0
bad = 0
for B in (65536, 65536 - 37):
    st = gogame.batch_init_state(B, 19, device='cuda'); rng = gogame.rng_seed(B, 2900 + B)
    ch = B // 16
    for g in range(1, 16):      # a stationary mix of game ages, finished games among them
        gogame.batch_rollout(st[g * ch:(g + 1) * ch], rng[g * ch:(g + 1) * ch], g * 40, True)
    assert L.gg_ab_mcheck_read_r5(buf) == 0
    ws = torch.zeros((B, 5 * 19 + 1), dtype=torch.int32, device='cuda')
    for name, launch in (('byte planes, no workspace', lambda: gogame.batch_rollout(st.clone(), rng.clone(), 256, True)),
                         ('byte planes, workspace misses then hits', lambda: [gogame.batch_rollout(st, rng, 64, True, workspace=ws) for _ in range(3)]),
                         ('byte planes, frozen games', lambda: gogame.batch_rollout(st.clone(), rng.clone(), 256, False)),
                         ('tracked boards', lambda: gogame.batch_rollout_tracked(gogame.batch_track(st), rng.clone(), 256, True))):
        launch()
        assert L.gg_ab_mcheck_read_r5(buf) == 0
        print('%6d games, %-42s rows that differ %d of %d' % (B, name + ':', buf[0], buf[1]))
        assert buf[1] > 0
        bad += buf[0]
sys.exit(1 if bad else 0)
