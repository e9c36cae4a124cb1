"""Times the experiment extractor's energy and ZCR groups: python tools/smooth_time.py [clips seconds sr].  Defaults: 1000
ten-second clips at 22050 Hz, seven rounds after one warm-up, the four modes interleaved in one process:
  (a) the reference's own routine on the CPU: preprocess_audio, medfilt(3), savgol_filter(11, 3), the rms and zero-crossing
      statistics through scipy / numpy, in a pool of 15 processes;
  (b) the composition of the separate device calls, host to host: sosfiltfilt_batch, medfilt_batch, savgol_batch (the
      statistics are not computed: what remains is the part the fused call would otherwise also do on the host);
  (c) energy_zcr_batch, host to host;
  (d) energy_zcr_batch on device-resident input.
Prints the median and the spread (max - min) of every mode, the ratios, and whether (c) is below (a) by more than the larger
of the two spreads.  ``--no-cpu`` leaves (a) out (for a kernel trace: run that under rocprofv3 --kernel-trace --stats)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

a = [x for x in sys.argv[1:] if not x.startswith("--")]
P, sec, sr = (int(a[0]), float(a[1]), int(a[2])) if len(a) >= 3 else (1000, 10.0, 22050)
ROUNDS = 7
FL, HOP = 2048, 512


def _base():
    from audio_feature_extraction_amd.synth import make_clip
    return [make_clip(i, sr, sec, speechy=bool(i % 2)) for i in range(8)]


_clips = None


def _reference_clip(i):
    """what extract_energy and extract_zcr compute from one loaded signal (the preprocess once: it is the same in both)"""
    global _clips
    import scipy.signal
    if _clips is None:
        _clips = _base()
    from tests import filt_ref as F
    from tests import smooth_ref as S
    y = F.preprocess_experiment(_clips[i % 8], sr).astype(np.float32)
    r = S.group_record(y, FL, HOP)
    return r["energy_mean"] + r["zcr_mean"]


if __name__ == "__main__":
    from audio_feature_extraction_amd import _native as N
    base = _base()
    y = np.concatenate([base[i % 8] for i in range(P)]).astype(np.float32)
    n = base[0].size
    ln = np.full(P, n, np.int64)
    off = np.arange(P, dtype=np.int64) * n
    sos = N.butter_sos(5, 200 / (sr / 2), True)
    ctx = N.Context(0)
    d_in = N.DeviceBuffer(ctx, y.nbytes)
    d_in.upload(y)
    full = N.EZ_PREPROCESS | N.EZ_ENERGY | N.EZ_ZCR
    buf = [np.zeros(y.size, np.float32) for _ in range(3)]

    def composition():
        p = ctx.sosfiltfilt_batch(y, off, ln, sos, 18, mode=N.FILT_EXPERIMENT, preemph=0.98, out=buf[0], out_offsets=off)
        m = ctx.medfilt_batch(p["out"], off, ln, 3, out=buf[1], out_offsets=off)
        return ctx.savgol_batch(m["out"], off, ln, 11, 3, out=buf[2], out_offsets=off)

    modes = {"b": composition,
             "c": lambda: ctx.energy_zcr_batch(y, off, ln, sr, FL, HOP, full),
             "d": lambda: ctx.energy_zcr_batch(d_in, off, ln, sr, FL, HOP, full, fmt=N.FMT_F32)}
    pool = None
    if "--no-cpu" not in sys.argv:
        import multiprocessing as mp
        pool = mp.get_context("spawn").Pool(15)
        pool.map(_reference_clip, range(30))                             # start the workers
        modes = {"a": lambda: pool.map(_reference_clip, range(P), chunksize=8), **modes}
    ts = {k: [] for k in modes}
    for rnd in range(ROUNDS + 1):
        for k, fn in modes.items():
            t0 = time.perf_counter()
            r = fn()
            dt = time.perf_counter() - t0
            if rnd:
                ts[k].append(dt)
    assert (modes["c"]()["status"] == 0).all()
    names = {"a": "(a) scipy chain, pool of 15 processes", "b": "(b) composition of the device calls, host to host",
             "c": "(c) energy_zcr_batch, host to host", "d": "(d) energy_zcr_batch, device-resident input"}
    med = {k: float(np.median(v)) for k, v in ts.items()}
    spread = {k: float(max(v) - min(v)) for k, v in ts.items()}
    print(f"{P} clips x {sec:g} s at {sr} Hz, {ROUNDS} rounds after one warm-up, modes interleaved")
    for k in ts:
        print(f"{names[k]}: median {med[k] * 1e3:.2f} ms, spread {spread[k] * 1e3:.2f} ms, {med[k] * 1e9 / (P * n):.3f} ns per sample")
    print(f"(b) / (c) = {med['b'] / med['c']:.2f}, (c) / (d) = {med['c'] / med['d']:.2f}")
    if pool is not None:
        pool.close()
        gap, need = med["a"] - med["c"], max(spread["a"], spread["c"])
        print(f"(a) / (c) = {med['a'] / med['c']:.1f}; (a) - (c) = {gap * 1e3:.1f} ms against a largest spread of {need * 1e3:.1f} ms: "
              f"{'holds' if gap > need else 'DOES NOT HOLD'}")
    ctx.close()
