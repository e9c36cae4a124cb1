"""Times afx_gate_batch (spectral gating, both modes) beside the nearest existing call, afx_denoise_batch's Wiener filter (one
FFT pair per frame, no statistics pass), on the same batch in the same process: python tools/gate_time.py [clips seconds sr]
Defaults: 1000 ten-second clips at 16000 Hz, n_fft 1024 / hop 256 (the reference's "wiener" branch).  The samples are device
resident.  afx_gate_batch is timed device to device and device to host; afx_denoise_batch writes to host memory only, so its
figure holds the download and belongs beside the device-to-host one.  Two warm calls, seven timed calls, the calls taking
turns round by round; min..max and every time per line.  Last, the float64 numpy oracle (tests/gate_ref.py) on one clip and
one core.  Per-kernel times: run it under rocprofv3 --kernel-trace --stats, in a run of its own."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from audio_feature_extraction_amd import _native as N
from tests import gate_ref as G

a = [x for x in sys.argv[1:] if not x.startswith("--")]
P, sec, sr = (int(a[0]), float(a[1]), int(a[2])) if len(a) >= 3 else (1000, 10.0, 16000)
warm, reps = 2, 7
base = [G.make_clip(sr, sec, seed=i) for i in range(8)]
L = base[0].size
y = np.concatenate([base[i % 8] for i in range(P)])
ln = np.full(P, L, np.int64)
off = np.arange(P, dtype=np.int64) * L
ctx = N.Context(0)
plan = N.Plan(ctx, N.make_params(sr, 2048, 512, 13, 128, "hann"))
d_in, d_out = N.DeviceBuffer(ctx, y.nbytes), N.DeviceBuffer(ctx, y.nbytes)
d_in.upload(y)
h_out = np.zeros(y.size, np.float32)
stat = N.gate_opts(sr, stationary=True, prop_decrease=0.95)
nonstat = N.gate_opts(sr)
calls = (
    ("gate stationary, device to device", lambda: ctx.gate_batch(d_in, off, ln, stat, fmt=N.FMT_F32, out=d_out, out_offsets=off)),
    ("gate non-stationary, device to device", lambda: ctx.gate_batch(d_in, off, ln, nonstat, fmt=N.FMT_F32, out=d_out, out_offsets=off)),
    ("gate stationary, device to host", lambda: ctx.gate_batch(d_in, off, ln, stat, fmt=N.FMT_F32, out=h_out, out_offsets=off)),
    ("gate non-stationary, device to host", lambda: ctx.gate_batch(d_in, off, ln, nonstat, fmt=N.FMT_F32, out=h_out, out_offsets=off)),
    ("denoise wiener 2048 / 512, device to host", lambda: plan.denoise_batch(d_in, off, ln, mode=N.DENOISE_WIENER, mem=N.MEM_DEVICE)),
)
for _ in range(warm):
    for _, call in calls:
        call()
ts = {name: [] for name, _ in calls}
for _ in range(reps):
    for name, call in calls:
        out = None
        t0 = time.perf_counter()
        out = call()
        ts[name].append(time.perf_counter() - t0)
        assert (out["status"] == 0).all()
for name, _ in calls:
    print(f"{name}, {P} clips x {sec:g} s at {sr} Hz: {min(ts[name]) * 1e3:.2f} .. {max(ts[name]) * 1e3:.2f} ms  ["
          + " ".join(f"{t * 1e3:.1f}" for t in ts[name]) + "]")
for name, kw in (("stationary", dict(stationary=True, prop_decrease=0.95)), ("non-stationary", {})):
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        G.reduce_noise(base[0], sr, **kw)
        t.append(time.perf_counter() - t0)
    print(f"numpy oracle {name}, one clip x {sec:g} s, one core: {min(t) * 1e3:.1f} ms ({min(t) * P:.1f} s for {P} clips)")
plan.close()
