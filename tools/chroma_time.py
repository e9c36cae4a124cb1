"""Times afx_chroma_batch (host to host, device synchronised on return): python tools/chroma_time.py [clips seconds sr]
Defaults: 1000 ten-second clips at 22050 Hz.  Prints one line per mode: the timbre statistics alone (tuning estimated, mel
and chroma reduced on the device), and with the chroma and mel matrices copied out as well.  Per-kernel times: run it under
rocprofv3 --kernel-trace --stats (``--hpss`` adds one afx_hpss_batch call over the same batch, so that the trace holds the
complex-output k_hpss_stft as the yardstick).  ``--cpu`` also times tests/chroma_ref.timbre_features on one clip on one core."""
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
frames = int((1 + ln // 512).sum())
print(f"{P} clips x {sec:g} s at {sr} Hz: {frames} frames, one pass over S = {frames * 4100 / 1e9:.3f} GB")
for mats in (False, True):
    plan.chroma_batch(y, off, ln, want_chroma=mats, want_mel=mats)           # workspace allocation, tables, first touch
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = plan.chroma_batch(y, off, ln, want_chroma=mats, want_mel=mats)
        ts.append(time.perf_counter() - t0)
    assert (out["status"] == 0).all()
    print(f"chroma_batch, matrices out={int(mats)}: {min(ts) * 1e3:.2f} ms (median {np.median(ts) * 1e3:.2f})  "
          f"mean chroma_mean {np.mean(out['stats'][:, 2]):.4f}  tunings {np.unique(out['tuning']).size} distinct")
if "--hpss" in sys.argv:
    plan.hpss_batch(y, off, ln, want_harm=False)
if "--cpu" in sys.argv:
    from tests import chroma_ref as R
    t0 = time.perf_counter()
    R.timbre_features(base[0], sr)
    dt = time.perf_counter() - t0
    print(f"restatement timbre_features (numpy, one core), one clip: {dt * 1e3:.1f} ms -> {dt * P:.1f} s per {P} clips")
plan.close()
