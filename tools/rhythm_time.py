"""Times afx_rhythm_batch (host to host, device synchronised on return): python tools/rhythm_time.py [clips seconds sr]
Defaults: 1000 ten-second clips at 22050 Hz.  Prints one line per mode: tempo and the envelope statistics alone, and with the
onset envelopes copied out as well.  Per-kernel times: run it under rocprofv3 --kernel-trace --stats in a run of its own (no
counters); k_hpss_stft<true>, the front end of the same batch, is the yardstick in that trace.  ``--cpu`` also times
tests/rhythm_ref.rhythm_features on one clip on one core."""
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
win = N.tempo_table(sr)["win"]
print(f"{P} clips x {sec:g} s at {sr} Hz: {frames} frames, window {win} lags, {frames * win * win / 2e9:.1f} G multiply-adds in the tempogram")
for env in (False, True):
    plan.rhythm_batch(y, off, ln, want_env=env)                               # workspace allocation, tables, first touch
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = plan.rhythm_batch(y, off, ln, want_env=env)
        ts.append(time.perf_counter() - t0)
    assert (out["status"] == 0).all()
    print(f"rhythm_batch, envelopes out={int(env)}: {min(ts) * 1e3:.2f} ms (median {np.median(ts) * 1e3:.2f})  "
          f"mean tempo {np.mean(out['tempo']):.3f}  mean onset strength {np.mean(out['stats'][:, 0]):.4f}")
if "--cpu" in sys.argv:
    from tests import rhythm_ref as R
    t0 = time.perf_counter()
    R.rhythm_features(base[0], sr)
    dt = time.perf_counter() - t0
    print(f"restatement rhythm_features (numpy / scipy.fft, one core), one clip: {dt * 1e3:.1f} ms -> {dt * P:.1f} s per {P} clips")
plan.close()
