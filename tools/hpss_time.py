"""Times afx_hpss_batch (host to host, device synchronised on return): python tools/hpss_time.py [clips seconds sr]
Defaults: 1000 ten-second clips at 22050 Hz.  Prints one line per mode: the harmonic features alone (stats), and the
harmonic signal as well (stats + out_harm).  Per-kernel times: run it under rocprofv3 --kernel-trace --stats.
``--cpu`` also times the float32 restatement of tests/hpss_ref.py on one clip on one core, for comparison."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from audio_feature_extraction_amd import _native as N
from audio_feature_extraction_amd.synth import make_clip

a = [x for x in sys.argv[1:] if not x.startswith("--")]
P, sec, sr = (int(a[0]), float(a[1]), int(a[2])) if len(a) >= 3 else (1000, 10.0, 22050)
reps = 5
base = [make_clip(i, sr, sec, speechy=bool(i % 2)) for i in range(8)]
y = np.concatenate([base[i % 8] for i in range(P)]).astype(np.float32)
ln = np.full(P, base[0].size, np.int64)
off = np.arange(P, dtype=np.int64) * base[0].size
plan = N.Plan(N.Context(0), N.make_params(sr, 2048, 512, 13, 128, "hann"))
for harm in (False, True):
    plan.hpss_batch(y, off, ln, want_harm=harm)           # workspace allocation, first touch
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = plan.hpss_batch(y, off, ln, want_harm=harm)
        ts.append(time.perf_counter() - t0)
    assert (out["status"] == 0).all()
    print(f"hpss_batch {P} clips x {sec:g} s at {sr} Hz, out_harm={int(harm)}: {min(ts) * 1e3:.2f} ms (median "
          f"{np.median(ts) * 1e3:.2f})  mean harmonic_ratio {np.mean(out['stats'][:, 0] / out['stats'][:, 1]):.4f}")
if "--cpu" in sys.argv:
    from tests import hpss_ref as R
    t0 = time.perf_counter()
    R.hpss(base[0], f32=True)
    dt = time.perf_counter() - t0
    print(f"float32 restatement (numpy, one core), one clip: {dt * 1e3:.1f} ms -> {dt * P:.1f} s per {P} clips")
plan.close()
