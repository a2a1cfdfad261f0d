"""ms per launch and state digests of the fused byte-plane rollout at the shapes of docs/history/r09.md, for ONE source tree
(GG_TREE = its root, default this one: a parent checkout built in place measures the parent) through the product path
gogame.batch_rollout; GYMGO_AMD_ROLLOUT_WS=0 measures this tree's launch without a workspace."""
import os, sys, hashlib
ROOT = os.path.abspath(os.environ.get('GG_TREE') or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)
import torch
from gymgo_amd import gogame
tag = '%s ws=%s' % (os.path.basename(ROOT), os.environ.get('GYMGO_AMD_ROLLOUT_WS', '1'))
def run(N, B, F, reps):
    st = gogame.batch_init_state(B, N, device='cuda'); rng = gogame.rng_seed(B, 20260927)
    ch = B // 16
    for g in range(1, 16):
        gogame.batch_rollout(st[g*ch:(g+1)*ch], rng[g*ch:(g+1)*ch], g * (40 if N == 19 else 8), True)
    for _ in range(3): gogame.batch_rollout(st, rng, F, True)
    torch.cuda.synchronize()
    best = None
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps): gogame.batch_rollout(st, rng, F, True)
        b.record(); torch.cuda.synchronize()
        ms = a.elapsed_time(b) / reps
        best = ms if best is None or ms < best else best
    h = hashlib.sha256(st.cpu().numpy().tobytes()).hexdigest()[:12]
    print('%-22s N %2d B %6d F %3d  ms/launch %.4f (best of 3 x %d)  digest %s' % (tag, N, B, F, best, reps, h), flush=True)
run(19, 65536, 256, 10); run(19, 65536, 256, 10)      # (the first shape twice: the clock ramps during the first)
run(19, 65536, 8, 100); run(19, 65536, 32, 50); run(19, 131072, 256, 5); run(9, 65536, 256, 10); run(13, 65536, 256, 10)
