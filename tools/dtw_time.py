"""Times afx_dtw_batch (host to host, device synchronised on return): python tools/dtw_time.py [pairs N M dim metric]
Defaults: 1000 pairs of 862 x 862 frames (ten-second utterances at hop 256), dim 39, euclidean.  Prints one line per mode
(without / with back-tracking) with the cell-update rate.  Per-kernel times: run it under rocprofv3 --kernel-trace --stats."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from audio_feature_extraction_amd import _native as N

a = sys.argv[1:]
P, n, m, dim = (int(a[0]), int(a[1]), int(a[2]), int(a[3])) if len(a) >= 4 else (1000, 862, 862, 39)
metric = a[4] if len(a) >= 5 else "euclidean"
reps = 5
rng = np.random.default_rng(0)
feats = rng.standard_normal((P * (n + m), dim)).astype(np.float32)
xo = np.arange(P, dtype=np.int64) * (n + m)
yo = xo + n
xl, yl = np.full(P, n, np.int64), np.full(P, m, np.int64)
ctx = N.Context(0)
cells = float(P) * n * m
res = {}
for bt in (False, True):
    ctx.dtw_batch(feats, xo, xl, yo, yl, None, metric, backtrack=bt)       # workspace allocation, first touch
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = ctx.dtw_batch(feats, xo, xl, yo, yl, None, metric, backtrack=bt)
        ts.append(time.perf_counter() - t0)
    dt = min(ts)
    res[bt] = dt
    assert (out["status"] == 0).all()
    print(f"dtw_batch {P} pairs {n}x{m} dim {dim} {metric} backtrack={int(bt)}: {dt * 1e3:.2f} ms (median "
          f"{np.median(ts) * 1e3:.2f}) {cells / dt:.3e} cells/s  mean cost {out['cost'].mean():.4f}")
print(f"backtrack / no backtrack time: {res[True] / res[False]:.3f}")
ctx.close()
