"""Times afx_beat_batch beside afx_rhythm_batch (host to host, device synchronised on return):
python tools/beat_time.py [clips seconds sr] [--host] [--trace]
Defaults: 1000 ten-second clips at 22050 Hz.  The two entry points share their front end, so their difference is what the
beat kernels and the copy of the flags add; they are interleaved in one process, seven rounds after one warm-up, and the
median, the minimum and the spread (max - min) of each are printed.  ``--host`` also times afx_beat_track_host on the same
envelopes and tempi over 16 threads (the CPU comparison).  ``--trace`` runs three calls of afx_beat_batch and nothing else:
the run to put under rocprofv3 --kernel-trace --stats, on its own and without counters; k_hpss_stft<true>, the front end of
the same batch, is the yardstick in that trace."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from audio_feature_extraction_amd import _native as N
from tests.rhythm_ref import clicks

a = [x for x in sys.argv[1:] if not x.startswith("--")]
P, sec, sr = (int(a[0]), float(a[1]), int(a[2])) if len(a) >= 3 else (1000, 10.0, 22050)
rounds = 7
base = [clicks(sr, bpm, seconds=sec, seed=bpm) for bpm in (72, 90, 100, 110, 120, 132, 150, 168)]
y = np.concatenate([base[i % 8] for i in range(P)]).astype(np.float32)
ln = np.full(P, base[0].size, np.int64)
off = np.arange(P, dtype=np.int64) * base[0].size
plan = N.Plan(N.Context(0), N.make_params(sr, 2048, 512, 13, 128, "hann"))
frames = int((1 + ln // 512).sum())
print(f"{P} clips x {sec:g} s at {sr} Hz: {frames} frames")
if "--trace" in sys.argv:
    for _ in range(3):
        out = plan.beat_batch(y, off, ln)
    print(f"beats per clip: mean {np.mean(out['n_beats']):.2f}")
    plan.close()
    sys.exit(0)
calls = {"rhythm_batch": lambda: plan.rhythm_batch(y, off, ln, want_env=False),
         "beat_batch": lambda: plan.beat_batch(y, off, ln)}
ts = {k: [] for k in calls}
for r in range(rounds + 1):                                                       # round 0: allocation, tables, first touch
    for k, f in calls.items():
        t0 = time.perf_counter()
        out = f()
        dt = time.perf_counter() - t0
        assert (out["status"] == 0).all()
        if r:
            ts[k].append(dt)
for k, v in ts.items():
    v = np.array(v) * 1e3
    print(f"{k}: median {np.median(v):.2f} ms  min {v.min():.2f} ms  spread {v.max() - v.min():.2f} ms  ({rounds} rounds)")
print(f"beat_batch - rhythm_batch, medians: {(np.median(ts['beat_batch']) - np.median(ts['rhythm_batch'])) * 1e3:.2f} ms; "
      f"beats per clip: mean {np.mean(out['n_beats']):.2f}, fpb {sorted(set(out['fpb'].tolist()))}")
if "--host" in sys.argv:
    from concurrent.futures import ThreadPoolExecutor
    full = plan.beat_batch(y, off, ln, want_env=True)
    fps = sr / 512.0
    def one(i):
        return N.beat_track_host(full["env"][i], fps, float(full["tempo"][i]))["beats"]
    with ThreadPoolExecutor(16) as pool:
        list(pool.map(one, range(16)))
        t0 = time.perf_counter()
        got = list(pool.map(one, range(P)))
        dt = time.perf_counter() - t0
    same = sum(np.array_equal(g, b) for g, b in zip(got, full["beats"]))
    print(f"afx_beat_track_host on the same {P} envelopes, 16 threads: {dt * 1e3:.1f} ms ({same} of {P} clips give the device's beats)")
plan.close()
