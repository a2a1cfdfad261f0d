"""Pairs of boards whose analysis the byte-plane load of k_rollout5 skipped / ran, per launch, over the sequence bench.py runs
(A/B build with -DGG_AB_WS: gg_v5.h, gg_wsc): de-synchronising slices, burn-in, settle windows, restore, warm-up, timed launches.
   LIB=<A/B library> python tools/exp/r5_ws_counts.py"""
import os, sys, ctypes
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
from gymgo_amd import _lib
_lib.LIB_PATH = os.path.join(ROOT, os.environ['LIB'])
import bench
L = ctypes.CDLL(_lib.LIB_PATH)
rd = L.gg_ab_ws_read_r5; rd.argtypes = [ctypes.c_void_p]; rd.restype = ctypes.c_int32
buf = (ctypes.c_ulonglong * 2)()
N, B, F = 19, 65536, 256
back = bench.HipBackend(torch.device('cuda', 0))
back.setup(B, N, 0)
def launch(tag, **kw):
    back.rollout(F, **kw)
    rd(buf)
    print('%-28s skipped %6d  analysed %6d' % (tag, buf[0], buf[1]), flush=True)
chunk = B // 16
for g in range(1, 16):
    back.rollout(g * 640 // 16, g * chunk, (g + 1) * chunk)
rd(buf)
print('%-28s skipped %6d  analysed %6d   (slices: no workspace)' % ('de-synchronising slices', buf[0], buf[1]))
launch('burn-in 0 (first call: recorded)', count_steps=False)
snap = back.snapshot()
for k in range(8): launch('settle %d' % k, count_steps=False)
back.restore(snap)
for k in range(5): launch('warm-up %d (0: after restore)' % k, count_steps=False)
for k in range(20): launch('timed %d' % k)
