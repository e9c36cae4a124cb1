"""Timing of the native ingest of every WAVE layout.  Needs a GPU.

  python tools/ingest_time.py kernel                     afx_decode_batch alone: 1000 ten-second clips, device-resident, input
                                                         bytes per second against a device-to-device copy of the same bytes
  python tools/ingest_time.py files --corpus s16x2_44100  batch_process files/s over 2048 ten-second files of one layout
      corpora: s16x2_44100 (16-bit stereo 44.1 kHz), s24x1_22050 (24-bit mono 22.05 kHz), s16x1_22050 (the 16-bit mono class)
      [--tree PATH]   import the package from another checkout (the parent commit) for an A/B on the same files
      [--dir DIR]     keep / reuse the generated files
  python tools/ingest_time.py make --corpus ... --dir DIR  only write the files (before a --tree run)
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORPORA = {"s16x2_44100": ("s16", 2, 44100), "s24x1_22050": ("s24", 1, 22050), "s16x1_22050": ("s16", 1, 22050)}


def kernel(args):
    import torch
    from audio_feature_extraction_amd import _native as N
    ctx = N.Context(0)
    rng = np.random.default_rng(0)
    print(f"{'layout':>10} {'MB in':>8} {'median ms':>10} {'min':>8} {'max':>8} {'GB/s in':>8} {'copy ms':>8} {'copy GB/s':>9} {'decode/copy':>11} {'copy ev ms':>10}")
    for name, kind, ch, rate in [("s16 x 2", N.SMP_S16, 2, 44100), ("s24 x 1", N.SMP_S24, 1, 44100), ("f32 x 2", N.SMP_F32, 2, 44100),
                                 ("f64 x 7", N.SMP_F64, 7, 8000)]:
        n_clips, n = args.clips, 10 * rate
        per = int(n * ch * N.SMP_BYTES[kind] + 15) // 16 * 16
        frames = np.full(n_clips, n, np.int64)
        boffs = np.arange(n_clips, dtype=np.int64) * per
        one = rng.integers(0, 256, size=per * 8, dtype=np.uint8)
        if kind >= N.SMP_F32:                                # no NaN / inf patterns: the top byte of every sample kept small
            one[N.SMP_BYTES[kind] - 1::N.SMP_BYTES[kind]] &= 0x3F
        src = N.DeviceBuffer(ctx, per * n_clips)
        for k in range(0, n_clips, 8):
            src.upload(one[: per * min(8, n_clips - k)], byte_offset=per * k)
        dst = N.DeviceBuffer(ctx, 4 * ((n + 3) // 4 * 4) * n_clips)
        kinds, chans = np.full(n_clips, kind, np.int32), np.full(n_clips, ch, np.int32)
        ts = []
        for r in range(args.warmup + args.runs):
            t0 = time.perf_counter()
            ctx.decode_batch(src, boffs, frames, kinds, chans, out=dst)          # synchronous on return
            if r >= args.warmup:
                ts.append(1e3 * (time.perf_counter() - t0))
        src.free(); dst.free()
        # the yardstick: a device-to-device copy of as many bytes (reads and writes them once), timed with device events
        nbytes = per * n_clips
        a = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        b = torch.empty_like(a)
        cs, ch_ = [], []
        for r in range(args.warmup + args.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(); b.copy_(a); e1.record(); e1.synchronize()
            if r >= args.warmup:
                ch_.append(1e3 * (time.perf_counter() - t0))
                cs.append(e0.elapsed_time(e1))
        del a, b
        ts, cm, chm = np.array(ts), float(np.median(cs)), float(np.median(ch_))
        print(f"{name:>10} {nbytes / 1e6:>8.0f} {np.median(ts):>10.3f} {ts.min():>8.3f} {ts.max():>8.3f} "
              f"{nbytes / np.median(ts) / 1e6:>8.0f} {chm:>8.3f} {nbytes / chm / 1e6:>9.0f} {np.median(ts) / chm:>11.2f} {cm:>10.3f}")
    print("decode and copy (one device-to-device copy of the input bytes) both by the host clock around a call that ends in a")
    print("synchronise: each carries its fixed host share (decode: clip records, their upload, the launch).  copy ev: the same")
    print("copy by device events.  The decoder writes 4 bytes per frame on top of the bytes it reads; the copy writes what it reads.")
    ctx.close()


def make_files(d, corpus, n_files):
    """The corpus' files in d (written where missing, by this tree's helpers: with --tree, generate them first with `make`)."""
    files = [os.path.join(d, f"f{i:05d}.wav") for i in range(n_files)]
    if all(os.path.exists(p) for p in files):
        return files
    sys.path.insert(0, ROOT)
    from audio_feature_extraction_amd.synth import make_clip
    from tests.wavfiles import quantize, write_wav
    kind, ch, rate = CORPORA[corpus]
    os.makedirs(d, exist_ok=True)
    base = [make_clip(k, rate, 10.0, speechy=True) for k in range(8)]
    first = {}                                   # 56 different contents: the others are copies
    for i, p in enumerate(files):
        if (i % 8, i % 7) not in first:
            write_wav(p, quantize(base[i % 8] * (0.5 + 0.5 * (i % 7) / 7.0), kind, ch), rate, kind)
            first[(i % 8, i % 7)] = open(p, "rb").read()
        elif not os.path.exists(p):
            with open(p, "wb") as f:
                f.write(first[(i % 8, i % 7)])
    return files


def files(args):
    import tempfile
    d = args.dir or tempfile.mkdtemp(prefix="afx_ingest_")
    fl = make_files(os.path.join(d, args.corpus), args.corpus, args.files)
    if args.mode == "make":
        return
    assert not args.tree or "audio_feature_extraction_amd" not in sys.modules, "--tree: generate the files first (mode `make`)"
    sys.path.insert(0, os.path.abspath(args.tree) if args.tree else ROOT)
    import audio_feature_extraction_amd as pkg
    from audio_feature_extraction_amd import parallel
    from audio_feature_extraction_amd.core.feature_extractor import AudioFeatureExtractor
    ex = AudioFeatureExtractor(sr=22050)
    ex.logger.setLevel("CRITICAL")
    for features in args.features.split(","):
        feats = None if features == "all" else ["mfcc", "energy"]
        rates, waits = [], []
        for r in range(args.warmup + args.runs):
            t0 = time.perf_counter()
            res = parallel.process_files(ex, fl, features_to_extract=feats)
            dt = time.perf_counter() - t0
            assert len(res) == len(fl), (len(res), len(fl))
            if r >= args.warmup:
                rates.append(len(fl) / dt)
                waits.append((parallel.LAST_TIMING["decode_wait"], parallel.LAST_TIMING["device"]))
        rates, w = np.array(rates), np.median(np.array(waits), axis=0)
        print(f"files tree={os.path.dirname(os.path.dirname(pkg.__file__))} corpus={args.corpus} features={features} n={len(fl)} "
              f"files/s median {np.median(rates):.0f} min {rates.min():.0f} max {rates.max():.0f} runs {[round(x) for x in rates]} "
              f"decode_wait {w[0]:.2f} s device {w[1]:.2f} s (summed over workers) ingest {parallel.LAST_TIMING.get('ingest')}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "files", "make"])
    ap.add_argument("--clips", type=int, default=1000)
    ap.add_argument("--files", type=int, default=2048)
    ap.add_argument("--corpus", choices=sorted(CORPORA), default="s16x2_44100")
    ap.add_argument("--features", default="nof0,all", help="comma-separated: nof0 (mfcc + energy), all")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tree", default=None)
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    if a.mode == "kernel":
        sys.path.insert(0, ROOT)
        kernel(a)
    else:
        files(a)
