"""The parts of the byte-plane load of k_rollout5 (A/B build with -DGG_AB_LOADSPLIT: gg_v5.h, gg_lsplit) on the stationary mix of
65 536 19x19 games, launches of 8 / 32 / 256 plies, without and with the rollout workspace.
   LIB=<A/B library> python tools/exp/r5_load_split.py"""
import os, sys, ctypes
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
from gymgo_amd import _lib
_lib.LIB_PATH = os.path.join(ROOT, os.environ['LIB'])
from gymgo_amd import gogame
L = ctypes.CDLL(_lib.LIB_PATH)
rd = L.gg_ab_load_split_read_r5; rd.argtypes = [ctypes.c_void_p]; rd.restype = ctypes.c_int32
N, B = 19, 65536
st = gogame.batch_init_state(B, N, device='cuda'); rng = gogame.rng_seed(B, 20260927)
ch = B // 16
for g in range(1, 16):
    gogame.batch_rollout(st[g*ch:(g+1)*ch], rng[g*ch:(g+1)*ch], g * 40, True)
buf = (ctypes.c_ulonglong * 4)()
names = ['staging + bytes -> rows', 'analysis / workspace compare', 'hand-over of mask and M']
for ws_on in ('0', '1'):
    os.environ['GYMGO_AMD_ROLLOUT_WS'] = ws_on
    for F in (8, 32, 256):
        for _ in range(4): gogame.batch_rollout(st, rng, F, True)
        rd(buf)
        reps = 20
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps): gogame.batch_rollout(st, rng, F, True)
        b.record(); torch.cuda.synchronize()
        rd(buf)
        v = list(buf)
        print('workspace %s, 65536 x %3d plies: %.1f us per launch (instrumented), %d groups' % (ws_on, F, a.elapsed_time(b) / reps * 1e3, v[3] // reps))
        for n, x in zip(names, v[:3]):
            print('  %-30s %9.0f cycles per wave and launch (%4.1f %% of the three)' % (n, x / max(1, v[3]), 100.0 * x / max(1, sum(v[:3]))), flush=True)
