"""Times the recording screen and the compare sums: python tools/assess_time.py [clips seconds sr] [--files N]
Defaults: 1000 ten-second clips at 22050 Hz (the batch of tools/denoise_time.py), float32, resident in device memory.
  afx_assess_batch / afx_compare_batch   one warm call, five timed calls taking turns, host clock around the call (it returns
        behind a device synchronise): min, median, every time; the bytes each must read (4 per sample, 8 per sample of a
        pair) over the minimum, beside the HBM peak bench.py --full reports its roofline against.  A call is two launches,
        one upload of the records and one download of the results: at this size those are a visible share of it.  The
        kernels' own times: run this file under rocprofv3 --kernel-trace --stats, in a run of its own.
  quality.assess_files                   N PCM16 files of the same clips (default 200) written to a temporary directory,
        one warm pass, three timed: files per second, probe + read + decode + screen.
  tests/assess_ref.py                    the numpy restatement (float32 flow, one core) over the first 100 clips after a
        warm-up of 5, scaled to the batch.
A machine without a GPU fails here: nothing falls back."""
import os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from audio_feature_extraction_amd import _native as N
from audio_feature_extraction_amd import quality, wavio
from audio_feature_extraction_amd.synth import make_clip
from tests import assess_ref as R

HBM_PEAK_GBS = 8000.0                                      # bench.py's roofline peak
a = [x for x in sys.argv[1:] if not x.startswith("--")]
P, sec, sr = (int(a[0]), float(a[1]), int(a[2])) if len(a) >= 3 else (1000, 10.0, 22050)
n_files = int(sys.argv[sys.argv.index("--files") + 1]) if "--files" in sys.argv else 200
if N.device_count() < 1:
    raise SystemExit("assess_time.py needs a GPU")
reps = 5
base = [make_clip(i, sr, sec, speechy=bool(i % 2)) for i in range(8)]
L = base[0].size
y = np.concatenate([base[i % 8] for i in range(P)]).astype(np.float32)
ln = np.full(P, L, np.int64)
off = np.arange(P, dtype=np.int64) * L
fs, fl = quality.frame_lengths(sr)
fsa, fla = np.full(P, fs, np.int32), np.full(P, fl, np.int32)
ctx = N.Context(0)
dev = N.DeviceBuffer(ctx, 2 * y.nbytes)                    # the clips, then the clips scaled: the degraded side of the pairs
dev.upload(y)
dev.upload((y * np.float32(0.9)), y.nbytes)
calls = (
    ("assess_batch", 4 * P * L, lambda: ctx.assess_batch(dev, off, ln, fsa, fla, fmt=N.FMT_F32)),
    ("compare_batch", 8 * P * L, lambda: ctx.compare_batch(dev, off, ln, dev, off + P * L, ln, fmt=N.FMT_F32)),
)
for _, _, call in calls:
    call()                                                # workspace allocation, first touch
ts = {name: [] for name, _, _ in calls}
for _ in range(reps):
    for name, _, call in calls:
        t0 = time.perf_counter()
        out = call()
        ts[name].append(time.perf_counter() - t0)
        assert (out["status"] == 0).all()
for name, nbytes, _ in calls:
    best = min(ts[name])
    print(f"{name} {P} clips x {sec:g} s at {sr} Hz, device-resident float32: {best * 1e3:.3f} ms per call (median "
          f"{np.median(ts[name]) * 1e3:.3f}) = {best * 1e3 * 1000 / P:.3f} ms per 1000 clips; {nbytes / 1e6:.0f} MB read -> "
          f"{nbytes / best / 1e9:.0f} GB/s, {nbytes / best / 1e9 / HBM_PEAK_GBS:.3f} of the {HBM_PEAK_GBS:.0f} GB/s HBM peak  ["
          + " ".join(f"{t * 1e3:.3f}" for t in ts[name]) + "]")
dev.free()

with tempfile.TemporaryDirectory() as d:
    paths = []
    for i in range(n_files):
        paths.append(os.path.join(d, f"clip{i:04d}.wav"))
        wavio.write_wav_pcm16(paths[-1], base[i % 8], sr)
    quality.assess_files(paths)
    tf = []
    for _ in range(3):
        t0 = time.perf_counter()
        res = quality.assess_files(paths)
        tf.append(time.perf_counter() - t0)
        assert all("error" not in r for r in res)
    print(f"assess_files {n_files} PCM16 files x {sec:g} s at {sr} Hz: {n_files / min(tf):.0f} files/s (min of 3: "
          + " ".join(f"{t * 1e3:.1f}" for t in tf) + " ms)")

m = min(100, P)
for i in range(5):
    R.assess(base[i % 8], sr, f32=True)
t0 = time.perf_counter()
for i in range(m):
    R.assess(base[i % 8], sr, f32=True)
tr = time.perf_counter() - t0
print(f"tests/assess_ref.py, one core, float32 flow: {tr / m * 1e3:.2f} ms per clip over {m} clips = {tr / m * 1000 * 1e3:.0f} ms per 1000 clips")
ctx.close()
