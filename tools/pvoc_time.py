"""Times afx_time_stretch_batch beside the same stretch through the three public calls with the spectra going home and back:
python tools/pvoc_time.py [clips seconds sr] [--fused-only]
Defaults: 1000 ten-second clips at 22050 Hz, 2048 / 512 (periodic Hann, center, constant padding), rates 0.8 and 1.25.
Per rate, taking turns in the same process:
  fused d2d    afx_time_stretch_batch, samples in device memory, the result left there
  fused h2h    the same call on host samples, the result brought home
  three calls  afx_stft_batch (host in, complex64 home), afx_pvoc_batch (host in, host out), afx_istft_batch (host in, samples
               home): what a caller had to do before -- the yardstick, which the fused call is no part of
One warm round, then two timed rounds; every wall time per line with min .. max (each call ends in a stream synchronise).
The three-call path holds two spectra of the batch in host memory (about 8 GB at the defaults).  ``--fused-only`` leaves it
out, for a kernel trace: run that under rocprofv3 --kernel-trace --stats, in a run of its own (k_hpss_prep, k_stft_frames,
k_pvoc_prep, k_pvoc_tiles, k_pvoc_carry, k_pvoc_apply, k_istft_frames, k_istft_ola)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.signal
from audio_feature_extraction_amd import _native as N
from tests import stft_ref as R

a = [x for x in sys.argv[1:] if not x.startswith("--")]
fused_only = "--fused-only" in sys.argv
P, sec, sr = (int(a[0]), float(a[1]), int(a[2])) if len(a) >= 3 else (1000, 10.0, 22050)
warm, reps = 1, 2
n, hop = 2048, 512
bins = n // 2 + 1
L = int(round(sec * sr))
base = [R.make_clip(L, seed=i, sr=sr) for i in range(8)]
y = np.concatenate([base[i % 8] for i in range(P)])
ln = np.full(P, L, np.int64)
off = np.arange(P, dtype=np.int64) * L
ctx = N.Context(0)
o = N.stft_opts(n, hop)
w = scipy.signal.get_window("hann", n).astype(np.float32)
d_in = N.DeviceBuffer(ctx, y.nbytes)
d_in.upload(y)


def three_calls(rates, n_out):
    s = ctx.stft_batch(y, off, ln, o, w)
    v = ctx.pvoc_batch(s["out"], s["offsets"], s["frames"], rates, n, hop)
    return ctx.istft_batch(v["out"], v["offsets"], v["frames"], o, w, lengths=n_out)


calls = []
for rate in (0.8, 1.25):
    rates = np.full(P, rate, np.float64)
    T, T_out, n_out, _ = N.time_stretch_samples(o, L, rate)
    ooff = N.packed_offsets(np.full(P, n_out, np.int64), 4)
    d_out = N.DeviceBuffer(ctx, 4 * int(ooff[-1] + n_out + 4))
    what = f"rate {rate}: {P * T} frames in, {P * T_out} out"
    calls.append((f"fused d2d, {what}", lambda rates=rates, d=d_out, ooff=ooff: ctx.time_stretch_batch(
        d_in, off, ln, rates, o, w, fmt=N.FMT_F32, out=d, out_offsets=ooff)))
    calls.append((f"fused h2h, {what}", lambda rates=rates: ctx.time_stretch_batch(y, off, ln, rates, o, w)))
    if not fused_only:
        calls.append((f"three calls, {what}", lambda rates=rates, m=n_out: three_calls(rates, np.full(P, m, np.int64))))
for _ in range(warm):
    for c in calls:
        c[1]()
ts = {c[0]: [] for c in calls}
for _ in range(reps):
    for name, call in calls:
        out = None                                       # the last result is freed outside the timed span
        t0 = time.perf_counter()
        out = call()
        ts[name].append(time.perf_counter() - t0)
        assert (out["status"] == 0).all()
for name, _ in calls:
    t = ts[name]
    print(f"{name}, {P} clips x {sec:g} s at {sr} Hz: {min(t) * 1e3:.1f} .. {max(t) * 1e3:.1f} ms  [" + " ".join(f"{x * 1e3:.1f}" for x in t) + "]")
