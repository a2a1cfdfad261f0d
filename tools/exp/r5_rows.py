"""The rows of profiles/r12_ab_rows.txt / r17_ab_rows.txt for ONE library: ms per launch and a digest (sha256 over states, generator
states, last actions and step counters after 3 + reps launches) per shape on the stationary mix of tools/exp/ab_rollout.py.
  LIB=<library relative to the repository> python tools/exp/r5_rows.py      (default: the shipped library)
One block per process; run parent and change alternately and compare the digests shape by shape."""
import hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
from gymgo_amd import _lib
if os.environ.get('LIB'):
    _lib.LIB_PATH = os.path.join(ROOT, os.environ['LIB'])
from gymgo_amd import gogame


def row(N, B, F, tracked=False, policy='uniform', reps=6):
    st = gogame.batch_init_state(B, N, device='cuda'); rng = gogame.rng_seed(B, 20260927)
    ch = B // 16
    for g in range(1, 16):
        gogame.batch_rollout(st[g * ch:(g + 1) * ch], rng[g * ch:(g + 1) * ch], g * (40 if N == 19 else 12), True)
    la = torch.full((B,), -9, dtype=torch.int32, device='cuda')
    sd = torch.zeros((B,), dtype=torch.int64, device='cuda')
    tr = gogame.batch_track(st) if tracked else None
    def launch():
        if tracked: gogame.batch_rollout_tracked(tr, rng, F, True, la, sd, policy=policy)
        else: gogame.batch_rollout(st, rng, F, True, la, sd)
    for _ in range(3): launch()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps): launch()
    b.record(); torch.cuda.synchronize()
    ms = a.elapsed_time(b) / reps
    h = hashlib.sha256()
    for t in ((gogame.batch_untrack(tr) if tracked else st), rng, la, sd):
        h.update(t.cpu().numpy().tobytes())
    print('N %2d B %6d F %3d %-7s %-11s ms/launch %.4f steps/s %.3e digest %s' % (
        N, B, F, 'tracked' if tracked else 'bytes', policy, ms, B * F / ms * 1e3, h.hexdigest()[:12]), flush=True)


row(19, 65536, 256); row(19, 65536, 32, reps=20); row(19, 65536, 8, reps=40)
row(19, 131072, 256, reps=3)
row(19, 65536, 256, tracked=True); row(19, 65536, 8, tracked=True, reps=40)
row(19, 65536, 256, tracked=True, policy='no_eye_fill')
row(13, 65536, 256); row(9, 65536, 256)
