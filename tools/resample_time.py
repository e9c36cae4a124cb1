"""Timing of the device resampler.  Needs a GPU.

  python tools/resample_time.py kernel                    afx_resample_batch, 1000 ten-second int16 clips, device-resident
  python tools/resample_time.py files --rate 44100        batch_process files/s over 2048 ten-second 16-bit mono files
      [--tree PATH]   import the package from another checkout (the parent commit) for an A/B on the same files
      [--dir DIR]     keep / reuse the generated files
"""
import argparse
import os
import sys
import time

import numpy as np

CU, SIMD, F64_LANES, GHZ = 256, 4, 16, 2.4           # v_fma_f64: 16 lanes per SIMD and clock


def kernel(args):
    from audio_feature_extraction_amd import _native as N
    ctx = N.Context(0)
    rng = np.random.default_rng(0)
    print(f"{'pair':>14} {'taps/out':>8} {'median ms':>10} {'min':>8} {'max':>8} {'fma bound ms':>12} {'fraction':>8}")
    for sr_in, sr_out in [(44100, 22050), (48000, 22050), (16000, 22050), (48000, 16000)]:
        d = N.resample_design(sr_in, sr_out)
        n_clips, n = args.clips, 10 * sr_in
        lens = np.full(n_clips, n, np.int64)
        offs = np.arange(n_clips, dtype=np.int64) * n
        one = rng.integers(-20000, 20000, size=n * 8).astype(np.int16)
        src = N.DeviceBuffer(ctx, 2 * n * n_clips)
        for k in range(0, n_clips, 8):
            src.upload(one[: n * min(8, n_clips - k)], byte_offset=2 * n * k)
        olen = N.resample_lengths(lens, sr_in, sr_out)
        dst = N.DeviceBuffer(ctx, 4 * int(((olen + 3) // 4 * 4).sum()))
        ts = []
        for r in range(args.warmup + args.runs):
            t0 = time.perf_counter()
            ctx.resample_batch(src, offs, lens, sr_in, sr_out, fmt=N.FMT_S16, out=dst)     # synchronous on return
            if r >= args.warmup:
                ts.append(1e3 * (time.perf_counter() - t0))
        per_out = -(-d["n_taps"] // d["up"])
        fma = float(olen.sum()) * d["n_taps"] / d["up"]
        bound = 1e3 * fma / (CU * SIMD * F64_LANES * GHZ * 1e9)
        ts = np.array(ts) * (1000.0 / n_clips)
        bound *= 1000.0 / n_clips
        print(f"{sr_in:>7}->{sr_out:<5} {per_out:>8} {np.median(ts):>10.2f} {ts.min():>8.2f} {ts.max():>8.2f} {bound:>12.2f} "
              f"{bound / np.median(ts):>8.2f}")
        src.free(); dst.free()
    print("ms per 1000 ten-second clips: host clock around the synchronous call (clip records, launch, kernel)")
    ctx.close()


def make_files(d, rate, n_files):
    from audio_feature_extraction_amd import wavio
    from audio_feature_extraction_amd.synth import make_clip
    os.makedirs(d, exist_ok=True)
    base = [make_clip(k, rate, 10.0, speechy=True) for k in range(8)]
    files = []
    for i in range(n_files):
        p = os.path.join(d, f"f{i:05d}.wav")
        if not os.path.exists(p):
            wavio.write_wav_pcm16(p, base[i % 8] * (0.5 + 0.5 * (i % 7) / 7.0), rate)
        files.append(p)
    return files


def files(args):
    if args.tree:
        sys.path.insert(0, os.path.abspath(args.tree))
    else:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import audio_feature_extraction_amd as pkg
    from audio_feature_extraction_amd import parallel
    from audio_feature_extraction_amd.core.feature_extractor import AudioFeatureExtractor
    import tempfile
    d = args.dir or tempfile.mkdtemp(prefix="afx_rs_")
    fl = make_files(os.path.join(d, str(args.rate)), args.rate, args.files)
    ex = AudioFeatureExtractor(sr=22050)
    ex.logger.setLevel("CRITICAL")
    feats = None if args.features == "all" else ["mfcc", "energy"]
    rates = []
    for r in range(args.warmup + args.runs):
        t0 = time.perf_counter()
        res = parallel.process_files(ex, fl, features_to_extract=feats)
        dt = time.perf_counter() - t0
        assert len(res) == len(fl), (len(res), len(fl))
        if r >= args.warmup:
            rates.append(len(fl) / dt)
    rates = np.array(rates)
    print(f"files tree={os.path.dirname(os.path.dirname(pkg.__file__))} rate={args.rate} features={args.features} n={len(fl)} "
          f"files/s median {np.median(rates):.0f} min {rates.min():.0f} max {rates.max():.0f} runs {[round(x) for x in rates]}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "files"])
    ap.add_argument("--clips", type=int, default=1000)
    ap.add_argument("--files", type=int, default=2048)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--features", choices=["all", "nof0"], default="all")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tree", default=None)
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    if a.mode == "kernel":
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        kernel(a)
    else:
        files(a)
