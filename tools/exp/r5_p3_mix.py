"""Static VALU instructions between consecutive GGMARK markers of k_rollout5<19, 0> in a -DGG_AB_MARK listing (gg_v5.h: the
phase markers 0 - 7 and the phase-3 branch markers 10 - 20), in listing order, priced as tools/isa_mix.py prices them
(2 / 4 issue cycles).  Loop bodies count once: weight them with the trip counts of tools/exp/r5_p3_counts.py.
    hipcc -O3 -std=c++17 --offload-arch=gfx950 -Iinclude -DGG_AB_MARK -S --cuda-device-only -o /tmp/gg5.s gymgo_amd/csrc/gg_r5.hip
    python tools/exp/r5_p3_mix.py /tmp/gg5.s"""
import os
import re
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isa_mix import FAST

KERNEL = '_ZN2gg10k_rollout5ILi19ELi0E'
text = open(sys.argv[1]).read().split('\n')
start = next(i for i, l in enumerate(text) if l.startswith(KERNEL))
end = next(i for i in range(start, len(text)) if 's_endpgm' in text[i])
cur, counts, order = None, {}, []
for l in text[start:end]:
    m = re.search(r'GGMARK (\d+)', l)
    if m:
        nxt = int(m.group(1))
        key = (cur, nxt)
        cur = nxt
        continue
    s = l.strip()
    if cur is None or not s or s[0] in '.;' or s.endswith(':') or not s.startswith('v_'):
        continue
    op = re.sub(r'_e(32|64)$', '', s.split()[0])
    fast = op in FAST and 'dpp' not in s
    c = counts.setdefault(cur, [0, 0])
    if cur not in order:
        order.append(cur)
    c[0] += 1
    c[1] += 2 if fast else 4
print('static VALU after each marker up to the next one in listing order (%s)' % sys.argv[1])
for k in order:
    print('  after GGMARK %2d: %4d VALU, %5d issue cycles' % (k, counts[k][0], counts[k][1]))
