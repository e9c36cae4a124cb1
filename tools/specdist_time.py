"""Times the whole-clip DFT behind the PESQ-like score: python tools/specdist_time.py [pairs seconds sr]
Defaults: 1000 pairs of ten-second clips at 22050 Hz (220500 = 2^2 3^2 5^3 7^2 samples: M = 2^19), float32, resident in
device memory -- the batch of tools/assess_time.py.
  afx_specdist_batch   one warm call, five timed calls, host clock around the call (it returns behind a device synchronise):
        min, median, every time, and the chunks the default budget cuts the batch into (afx_specdist_cost).  Beside it the
        traffic estimate: a transform of M points is three passes that each read and write 16 M bytes (the first reads the
        samples instead, the last keeps N points) and the middle pass reads the filter spectrum as well: about
        (2 + 3 + 1.5) x 16 M bytes per pair, over the minimum, beside the HBM peak bench.py --full reports its roofline
        against.  The kernels' own times: run this file under rocprofv3 --kernel-trace --stats, in a run of its own.
  numpy                np.fft.fft of both float64 signals of a pair, |.|, the distance: one core, over 20 pairs after a
        warm-up of 3, scaled to the batch.
A machine without a GPU fails here: nothing falls back."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from audio_feature_extraction_amd import _native as N
from audio_feature_extraction_amd.synth import make_clip
from tests import spectrum_ref as S

HBM_PEAK_GBS = 8000.0                                      # bench.py's roofline peak
a = [x for x in sys.argv[1:] if not x.startswith("--")]
P, sec, sr = (int(a[0]), float(a[1]), int(a[2])) if len(a) >= 3 else (1000, 10.0, 22050)
if N.device_count() < 1:
    raise SystemExit("specdist_time.py needs a GPU")
reps = 5
base = [make_clip(i, sr, sec, speechy=bool(i % 2)) for i in range(8)]
L = base[0].size
y = np.concatenate([base[i % 8] for i in range(P)]).astype(np.float32)
noise = (0.01 * np.random.default_rng(5).standard_normal(y.size)).astype(np.float32)
ln = np.full(P, L, np.int64)
off = np.arange(P, dtype=np.int64) * L
ctx = N.Context(0)
dev = N.DeviceBuffer(ctx, 2 * y.nbytes)                    # the clips, then the clips with noise: the degraded side of the pairs
dev.upload(y)
dev.upload(y + noise, y.nbytes)
call = lambda: ctx.specdist_batch(dev, off, ln, dev, off + P * L, ln, fmt=N.FMT_F32)
out = call()                                               # workspace allocation, first touch, the twiddle table
ts = []
for _ in range(reps):
    t0 = time.perf_counter()
    out = call()
    ts.append(time.perf_counter() - t0)
    assert (out["status"] == 0).all()
M = 1
while M < 2 * L - 1:
    M *= 2
chunks = int(N.stft_chunks(ln, N.specdist_cost(N.FMT_F32, N.MEM_DEVICE), 2 << 30).max()) + 1
nbytes = 6.5 * 16 * M * P
best = min(ts)
print(f"specdist_batch {P} pairs x {sec:g} s at {sr} Hz (N = {L}, M = {M}), device-resident float32, {chunks} chunk(s): "
      f"{best * 1e3:.3f} ms per call (median {np.median(ts) * 1e3:.3f}) = {best * 1e3 * 1000 / P:.3f} ms per 1000 pairs; about "
      f"{nbytes / 1e9:.1f} GB moved by the estimate -> {nbytes / best / 1e9:.0f} GB/s, {nbytes / best / 1e9 / HBM_PEAK_GBS:.3f} of the "
      f"{HBM_PEAK_GBS:.0f} GB/s HBM peak  [" + " ".join(f"{t * 1e3:.3f}" for t in ts) + "]")
want = S.spec_dist(base[0], base[0] + noise[:L])
print(f"pair 0: device {out['rec'][0][1] / L:.15f}  numpy {want:.15f}")
dev.free()

m = min(20, P)
for i in range(3):
    S.spec_dist(base[i % 8], base[i % 8] + noise[:L])
t0 = time.perf_counter()
for i in range(m):
    S.spec_dist(base[i % 8], base[i % 8] + noise[:L])
tr = time.perf_counter() - t0
print(f"numpy np.fft.fft of both sides in float64, one core: {tr / m * 1e3:.2f} ms per pair over {m} pairs = {tr / m * 1000 * 1e3:.0f} ms per 1000 pairs")
ctx.close()
