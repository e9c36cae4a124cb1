"""Times the experiment extractor's preprocess and its spectral, harmonic, timbre and rhythm groups three ways, host to host,
device synchronised on return: python tools/groups_time.py [clips seconds sr]   (defaults: 1000 ten-second clips at 22050 Hz)
  (a) the chain of existing calls on host arrays: afx_sosfiltfilt_batch, afx_spectral_batch, afx_hpss_batch,
      afx_chroma_batch plus the extract pass its MFCC statistics come from, afx_rhythm_batch
  (b) the same chain with the preprocess output kept on the device
  (c) afx_groups_batch with AFX_GROUPS_PREPROCESS
All three run in this process, interleaved, after a warm-up round; each is repeated and reported as minimum, median and
spread (max - min).  The gate of DESIGN.md 18: the median of (c) lies below the median of (b) by more than (b)'s spread.
Per-kernel times: run it under rocprofv3 --kernel-trace --stats in a run of its own (no counters)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from audio_feature_extraction_amd import _native as N
from audio_feature_extraction_amd.synth import make_clip

a = [x for x in sys.argv[1:] if not x.startswith("--")]
P, sec, sr = (int(a[0]), float(a[1]), int(a[2])) if len(a) >= 3 else (1000, 10.0, 22050)
reps = 7
rng = np.random.default_rng(0)
base = [(make_clip(i, sr, sec, speechy=bool(i % 2)) + 1e-3 * rng.standard_normal(int(round(sr * sec)))).astype(np.float32) for i in range(8)]
y = np.concatenate([base[i % 8] for i in range(P)]).astype(np.float32)
ln = np.full(P, base[0].size, np.int64)
off = np.arange(P, dtype=np.int64) * base[0].size
ctx = N.Context(0)
plan = N.Plan(ctx, N.make_params(sr, 2048, 512, 13, 128, "hann"))
sos = N.butter_sos(5, 200 / (sr / 2), True)
T = 1 + ln // 512
doff = N.packed_offsets(17 * T)
desc = np.zeros(int(17 * T.sum()), np.float32)
dstat = np.zeros(P, np.int32)
dev = N.DeviceBuffer(ctx, 4 * y.size + 64)
pre_host = np.zeros(y.size, np.float32)


def spectral(src, mem):
    ptr = src.ctypes.data if mem == N.MEM_HOST else src.ptr
    N._check(N.lib().afx_spectral_batch(plan.handle, ptr, N.FMT_F32, mem, off.ctypes.data, ln.ctypes.data, P, 0,
                                        desc.ctypes.data, doff.ctypes.data, dstat.ctypes.data), "afx_spectral_batch")


def groups_of(src, mem):
    spectral(src, mem)
    h = plan.hpss_batch(src, off, ln, mem=mem, want_harm=False)
    c = plan.chroma_batch(src, off, ln, mem=mem, want_chroma=False)
    m = plan.extract_batch(src, off, ln, flags=0)
    r = plan.rhythm_batch(src, off, ln, mem=mem, want_env=False)
    return h, c, m, r


def chain_host():
    f = ctx.sosfiltfilt_batch(y, off, ln, sos, 18, mode=N.FILT_EXPERIMENT, preemph=0.98, out=pre_host, out_offsets=off)
    return f, groups_of(pre_host, N.MEM_HOST)


def chain_device():
    f = ctx.sosfiltfilt_batch(y, off, ln, sos, 18, mode=N.FILT_EXPERIMENT, preemph=0.98, out=dev, out_offsets=off)
    return f, groups_of(dev, N.MEM_DEVICE)


def fused():
    return plan.groups_batch(y, off, ln, preprocess=True)


modes = (("(a) five calls, host arrays", chain_host), ("(b) five calls, preprocess output on the device", chain_device),
         ("(c) afx_groups_batch", fused))
frames = int(T.sum())
print(f"{P} clips x {sec:g} s at {sr} Hz: {frames} frames, {y.size * 4 / 1e6:.0f} MB of samples; {reps} repetitions each, interleaved")
for _, fn in modes:                                                  # workspace allocation, tables, first touch
    fn()
ts = {name: [] for name, _ in modes}
for _ in range(reps):
    for name, fn in modes:
        t0 = time.perf_counter()
        out = fn()
        ts[name].append(time.perf_counter() - t0)
for name, _ in modes:
    v = np.array(ts[name]) * 1e3
    print(f"{name}: min {v.min():.2f} ms  median {np.median(v):.2f} ms  spread {v.max() - v.min():.2f} ms")
assert (out["status"] == 0).all()
b, c = np.array(ts[modes[1][0]]) * 1e3, np.array(ts[modes[2][0]]) * 1e3
gain = np.median(b) - np.median(c)
print(f"gate: median (b) - median (c) = {gain:.2f} ms against (b)'s spread {b.max() - b.min():.2f} ms: "
      f"{'holds' if gain > b.max() - b.min() else 'DOES NOT HOLD'}")
s = out["stats"]
print(f"mean tempo {np.mean(s[:, 18]):.3f}  mean centroid {np.mean(s[:, 0]):.2f}  mean mfcc {np.mean(s[:, 16]):.4f}")
dev.free()
plan.close()
