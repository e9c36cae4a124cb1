"""Times afx_sosfiltfilt_batch (host to host and device to device, synchronised on return):
python tools/filtfilt_time.py [clips seconds sr].  Defaults: 1000 ten-second clips at 22050 Hz, the experiment extractor's
filter (5th-order Butterworth high-pass at 200 Hz, padlen 18).  Prints one line per mode and memory kind.  Per-kernel times:
run it under rocprofv3 --kernel-trace --stats.  ``--cpu`` also times scipy.signal.filtfilt on the same clips on one core and
on a pool of 15 processes, for comparison."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from audio_feature_extraction_amd import _native as N
from audio_feature_extraction_amd.synth import make_clip

a = [x for x in sys.argv[1:] if not x.startswith("--")]
P, sec, sr = (int(a[0]), float(a[1]), int(a[2])) if len(a) >= 3 else (1000, 10.0, 22050)
reps = 5
base = [make_clip(i, sr, sec, speechy=bool(i % 2)) for i in range(8)]


def _scipy_clip(i):
    import scipy.signal
    b, a_ = scipy.signal.butter(5, 200 / (sr / 2), btype="high")
    return float(np.abs(scipy.signal.filtfilt(b, a_, base[i % 8])).max())


if __name__ == "__main__":
    y = np.concatenate([base[i % 8] for i in range(P)]).astype(np.float32)
    n = base[0].size
    ln = np.full(P, n, np.int64)
    off = np.arange(P, dtype=np.int64) * n
    sos = N.butter_sos(5, 200 / (sr / 2), True)
    ctx = N.Context(0)
    d_in, d_out = N.DeviceBuffer(ctx, y.nbytes), N.DeviceBuffer(ctx, y.nbytes)
    d_in.upload(y)
    out = np.zeros(y.size, np.float32)
    for mode, name in ((N.FILT_PLAIN, "plain"), (N.FILT_EXPERIMENT, "experiment")):
        for kind, src, dst in (("host -> host", y, out), ("device -> device", d_in, d_out)):
            kw = dict(mode=mode, preemph=0.98, fmt=N.FMT_F32, out=dst, out_offsets=off)
            ctx.sosfiltfilt_batch(src, off, ln, sos, 18, **kw)          # workspace allocation, first touch
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                r = ctx.sosfiltfilt_batch(src, off, ln, sos, 18, **kw)
                ts.append(time.perf_counter() - t0)
            assert (r["status"] == 0).all()
            print(f"sosfiltfilt_batch {name}, {kind}: {P} clips x {sec:g} s at {sr} Hz: {min(ts) * 1e3:.2f} ms (median "
                  f"{np.median(ts) * 1e3:.2f}), {min(ts) * 1e9 / (P * n):.3f} ns per sample")
    if "--cpu" in sys.argv:
        import multiprocessing as mp
        _scipy_clip(0)                                                   # the import, the design
        t0 = time.perf_counter()
        for i in range(16):
            _scipy_clip(i)
        dt = (time.perf_counter() - t0) / 16
        print(f"scipy.signal.filtfilt, one core: {dt * 1e3:.2f} ms per clip -> {dt * P:.2f} s per {P} clips")
        with mp.get_context("spawn").Pool(15) as pool:
            pool.map(_scipy_clip, range(30))                             # start the workers
            t0 = time.perf_counter()
            pool.map(_scipy_clip, range(P), chunksize=8)
            dt = time.perf_counter() - t0
        print(f"scipy.signal.filtfilt, pool of 15 processes: {dt:.2f} s per {P} clips")
    ctx.close()
