"""Flood batches of k_rollout5 on the stationary mix (A/B build with -DGG_AB_SWEEPS: make ab EXTRA=-DGG_AB_SWEEPS; add
-DGG_AB_FLOODK=3 for the three-sweep schedule at 19x19): sweeps up to the weak closure of the G lanes, the share of batches that
leave a lane unsettled there, the sweeps those batches run on until every lane is settled, and what the unsettled lanes flood.
    LIB=ab_tmp/libgg_sweeps.so python tools/exp/r5_sweeps.py"""
import os, sys, ctypes
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
from gymgo_amd import _lib
_lib.LIB_PATH = os.path.join(ROOT, os.environ.get('LIB', 'ab_tmp/libgg_sweeps.so'))
from gymgo_amd import gogame
L = ctypes.CDLL(_lib.LIB_PATH)
L.gg_ab_sweeps_read_r5.argtypes = [ctypes.c_void_p]; L.gg_ab_sweeps_read_r5.restype = ctypes.c_int32
N, F, B = 19, 256, 65536
st = gogame.batch_init_state(B, N, device='cuda'); rng = gogame.rng_seed(B, 20260927)
ch = B // 16
for g in range(1, 16):
    gogame.batch_rollout(st[g*ch:(g+1)*ch], rng[g*ch:(g+1)*ch], g * 40, True)
gogame.batch_rollout(st, rng, 4 * F, True)
buf = (ctypes.c_ulonglong * 10)()
L.gg_ab_sweeps_read_r5(buf)
for _ in range(4): gogame.batch_rollout(st, rng, F, True)
L.gg_ab_sweeps_read_r5(buf)
c = list(buf)
nb, nu = c[1], max(c[2], 1)
print('%s: %d flood batches (%.4f per wave-ply)' % (os.environ.get('LIB', 'ab_tmp/libgg_sweeps.so'), nb, nb / (B / 32 * F * 4)))
print('a. sweeps to the weak closure of the G lanes      %.3f per batch' % (c[0] / nb))
print('b. batches that leave a lane unsettled there      %.2f %%' % (100.0 * c[2] / nb))
print('c. sweeps those batches run on: 1: %.2f %%  2: %.2f %%  3: %.2f %%  4+: %.2f %%  (mean %.3f; %.3f per batch of all)'
      % tuple([100.0 * c[3 + i] / nu for i in range(4)] + [c[9] / nu, c[9] / nb]))
print('d. unsettled lanes: G %.1f %%  opponent %.1f %%  (%.2f per unsettled batch)'
      % (100.0 * c[7] / max(c[7] + c[8], 1), 100.0 * c[8] / max(c[7] + c[8], 1), (c[7] + c[8]) / nu))
print('   sweeps per batch in all                        %.3f' % ((c[0] + c[9]) / nb))
