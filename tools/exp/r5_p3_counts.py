"""How often the wave takes each wave-wide branch of k_rollout5's phase 3 (class patch, captures, ko, atari-join) on the
stationary mix of 65 536 games of 19x19, and the trip count of the atari-join loop (A/B build with -DGG_AB_P3:
make -C gymgo_amd/csrc ab EXTRA=-DGG_AB_P3).  Also reads the live-prefix / played invariant counter (built in with -DGG_AB_P3 or -DGG_AB_LIVE).
    LIB=ab_tmp/libgg_p3.so python tools/exp/r5_p3_counts.py"""
import os, sys, ctypes
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
from gymgo_amd import _lib
_lib.LIB_PATH = os.path.join(ROOT, os.environ.get('LIB', 'ab_tmp/libgg_p3.so'))
from gymgo_amd import gogame
L = ctypes.CDLL(_lib.LIB_PATH)
L.gg_ab_p3_read_r5.argtypes = [ctypes.c_void_p]; L.gg_ab_p3_read_r5.restype = ctypes.c_int32
L.gg_ab_live_bad_r5.argtypes = [ctypes.c_void_p]; L.gg_ab_live_bad_r5.restype = ctypes.c_int32
N, F, B = 19, 256, 65536
st = gogame.batch_init_state(B, N, device='cuda'); rng = gogame.rng_seed(B, 20260927)
ch = B // 16
for g in range(1, 16):
    gogame.batch_rollout(st[g*ch:(g+1)*ch], rng[g*ch:(g+1)*ch], g * 40, True)
gogame.batch_rollout(st, rng, 4 * F, True)
buf = (ctypes.c_ulonglong * 10)()
assert L.gg_ab_p3_read_r5(buf) == 0
for _ in range(4): gogame.batch_rollout(st, rng, F, True)
assert L.gg_ab_p3_read_r5(buf) == 0
wp = buf[0]
print('k_rollout5 phase 3, 65 536 games x 4 launches x 256 plies: %d wave-plies (%.4f of B / 32 x plies)' % (wp, wp / (B / 32 * F * 4)))
for k, name in ((1, 'capt_m (a capture on some board)'), (2, 'ncapn == 1 && libsG == 0'), (3, 'ko1'),
                (4, 'anya && capt_m'), (5, 'anyf (atari-join loop entered)')):
    print('  %-34s %.4f of the wave-plies' % (name, buf[k] / wp))
print('  atari-join trips: %.3f per wave-ply that enters it, %.3f per wave-ply, at most %d' %
      (buf[6] / max(buf[5], 1), buf[6] / wp, buf[7]))
print('  boards that capture: %.4f per moving board (%.3f per wave-ply)' % (buf[8] / max(buf[9], 1), buf[8] / wp))
bad = (ctypes.c_ulonglong * 1)()
assert L.gg_ab_live_bad_r5(bad) == 0
print('live-prefix / played invariant: %d violations' % bad[0])
