"""Times afx_dtw_steps_batch (host to host, device synchronised on return):
    python tools/dtw_steps_time.py [--steps 1,1,1,2,2,1] [--subseq] [--default] [pairs N M dim metric]
Defaults: 1000 pairs of 862 x 862 frames (ten-second utterances at hop 256), dim 39, euclidean -- tools/dtw_time.py's
shapes -- with the slope-limited list (1,1), (1,2), (2,1).  --steps takes di,dj,di,dj,...; --default runs the default
steps with unit weights through the general kernel (tools/dtw_time.py times them on k_dtw).  Prints one line per mode
(without / with back-tracking) with the cell-update rate.  Per-kernel times: run it under rocprofv3 --kernel-trace --stats."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from audio_feature_extraction_amd import _native as N

a = sys.argv[1:]
steps = np.array([[1, 1], [1, 2], [2, 1]], np.int32)
subseq = False
while a and a[0].startswith("--"):
    flag = a.pop(0)
    if flag == "--steps":
        steps = np.array([int(v) for v in a.pop(0).split(",")], np.int32).reshape(-1, 2)
    elif flag == "--subseq":
        subseq = True
    elif flag == "--default":
        steps = None
    else:
        raise SystemExit(f"unknown option {flag}")
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
name = "default" if steps is None else "".join("(%d,%d)" % tuple(s) for s in steps)
res = {}
for bt in (False, True):
    run = lambda: ctx.dtw_steps_batch(feats, xo, xl, yo, yl, None, metric, backtrack=bt, steps=steps, subseq=subseq)
    run()                                                                  # workspace allocation, first touch
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = run()
        ts.append(time.perf_counter() - t0)
    dt = min(ts)
    res[bt] = dt
    assert (out["status"] == 0).all()
    print(f"dtw_steps_batch {P} pairs {n}x{m} dim {dim} {metric} steps {name} subseq={int(subseq)} backtrack={int(bt)}: "
          f"{dt * 1e3:.2f} ms (median {np.median(ts) * 1e3:.2f}) {cells / dt:.3e} cells/s  mean cost {out['cost'].mean():.4f}")
print(f"backtrack / no backtrack time: {res[True] / res[False]:.3f}")
ctx.close()
