"""Times afx_stft_batch and afx_istft_batch, device to device, beside afx_hpss_batch on the same batch in the same process:
python tools/stft_time.py [clips seconds sr]
Defaults: 1000 ten-second clips at 22050 Hz.  The calls: stft at 2048 / 512 and at 1024 / 256 (periodic Hann, center,
constant padding, complex64 out), the |D| kind at 2048 / 512, istft of both spectra back to the clips' lengths, and
afx_hpss_batch (harmonic out, no statistics), whose first kernel k_hpss_stft<false> is the same transform on the same
frames and is untouched by this code.  Two warm rounds, then three timed rounds with the calls taking turns; every wall
time per line with min .. max, and the bytes the call moves per second of its fastest run.  Per-kernel times (k_stft_frames
beside k_hpss_stft, k_istft_frames, k_istft_ola): run it under rocprofv3 --kernel-trace --stats, in a run of its own."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.signal
from audio_feature_extraction_amd import _native as N
from tests import stft_ref as R

a = [x for x in sys.argv[1:] if not x.startswith("--")]
P, sec, sr = (int(a[0]), float(a[1]), int(a[2])) if len(a) >= 3 else (1000, 10.0, 22050)
warm, reps = 2, 3
L = int(round(sec * sr))
base = [R.make_clip(L, seed=i, sr=sr) for i in range(8)]
y = np.concatenate([base[i % 8] for i in range(P)])
ln = np.full(P, L, np.int64)
off = np.arange(P, dtype=np.int64) * L
ctx = N.Context(0)
plan = N.Plan(ctx, N.make_params(sr, 2048, 512, 13, 128, "hann"))
d_in, d_sig = N.DeviceBuffer(ctx, y.nbytes), N.DeviceBuffer(ctx, y.nbytes)
d_in.upload(y)
cfg, calls = {}, []
for n, hop in ((2048, 512), (1024, 256)):
    o = N.stft_opts(n, hop)
    T = N.stft_frames(o, L)[0]
    bins = n // 2 + 1
    soff = np.arange(P, dtype=np.int64) * T * bins
    d_spec = N.DeviceBuffer(ctx, 8 * P * T * bins)
    w = scipy.signal.get_window("hann", n).astype(np.float32)
    cfg[n] = (o, T, bins, soff, d_spec, w)
    fr = np.full(P, T, np.int64)
    calls.append((f"stft {n}/{hop} complex", 4 * y.size + 8 * P * T * bins, P * T,
                  lambda o=o, soff=soff, d=d_spec, w=w: ctx.stft_batch(d_in, off, ln, o, w, fmt=N.FMT_F32, out=d, out_offsets=soff)))
    if n == 2048:
        om = N.stft_opts(n, hop, out_kind=N.STFT_MAG)
        calls.append((f"stft {n}/{hop} |D|", 4 * y.size + 4 * P * T * bins, P * T,
                      lambda om=om, soff=soff, d=d_spec, w=w: ctx.stft_batch(d_in, off, ln, om, w, fmt=N.FMT_F32, out=d, out_offsets=soff)))
    calls.append((f"istft {n}/{hop}", 8 * P * T * bins + 2 * 4 * P * T * n + 4 * y.size, P * T,
                  lambda o=o, soff=soff, d=d_spec, w=w, fr=fr: ctx.istft_batch(d, soff, fr, o, w, lengths=ln, out=d_sig, out_offsets=off)))
calls.append(("hpss 2048/512 (k_hpss_stft<false> first)", 0, P * (1 + L // 512),
              lambda: plan.hpss_batch(d_in.ptr, off, ln, mem=N.MEM_DEVICE, want_stats=False)))
for _ in range(warm):
    for c in calls:
        c[3]()
ts = {c[0]: [] for c in calls}
for _ in range(reps):
    for name, _, _, call in calls:
        out = None                                       # the last result is freed outside the timed span
        t0 = time.perf_counter()
        out = call()
        ts[name].append(time.perf_counter() - t0)
        assert (out["status"] == 0).all()
for name, nbytes, frames, _ in calls:
    t = ts[name]
    rate = f", {nbytes / min(t) / 1e9:.1f} GB/s moved" if nbytes else ""
    print(f"{name}, {P} clips x {sec:g} s at {sr} Hz, {frames} frames: {min(t) * 1e3:.2f} .. {max(t) * 1e3:.2f} ms  ["
          + " ".join(f"{x * 1e3:.1f}" for x in t) + f"]{rate}")
plan.close()
