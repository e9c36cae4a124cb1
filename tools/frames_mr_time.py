#!/usr/bin/env python
"""Frame-kernel time of the 400 / 160 speech framing (k_frames_mr) against the generic k_frames<512> at 512 / 128 on the
same clips, through the plan's own timing interface (afx_plan_set_timing(plan, 2): events around the frame kernel only).

  python tools/frames_mr_time.py [--clips 1000] [--seconds 10] [--runs 7] [--warmup 2] [--out profiles/frames_mr_time.txt]

Workload: 16 kHz clips from synth.make_clip (50 distinct ones, repeated), device-resident float32, K = 13.  The comparator
runs in a child process of its own with AFX_NO_FRAMES3D=1 (the developer switch that turns the wave-level 512 / 128 kernel
off; the library reads it once per process), so both sides go through trim -> frame kernel -> DCT -> statistics and only
the frame kernel differs.  Prints one JSON line per side and writes the summary."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(a):
    import numpy as np
    from audio_feature_extraction_amd import _native as N
    from audio_feature_extraction_amd.synth import make_clip
    n = int(round(16000 * a.seconds))
    base = [make_clip(i, 16000, a.seconds) for i in range(min(50, a.clips))]
    buf = np.concatenate([base[i % len(base)] for i in range(a.clips)])
    offsets = np.arange(a.clips, dtype=np.int64) * n
    lengths = np.full(a.clips, n, np.int64)
    ctx = N.Context(0)
    plan = N.Plan(ctx, N.make_params(16000, a.n_fft, a.hop, 13, a.n_mels))
    d = N.DeviceBuffer(ctx, buf.nbytes)
    d.upload(buf)
    for _ in range(a.warmup):
        plan.extract_batch(d, offsets, lengths)
    plan.set_timing(True, frames_only=True)
    ms = []
    for _ in range(a.runs):
        plan.timings(reset=True)
        out = plan.extract_batch(d, offsets, lengths)
        t = plan.timings()
        assert t["frames"][1] == 1 and (out["status"] == 0).all()
        ms.append(t["frames"][0])
    frames = int(out["nframes"].sum())
    plan.set_timing(False)
    d.free()
    plan.close()
    ctx.close()
    med = float(np.median(ms))
    print(json.dumps({"n_fft": a.n_fft, "hop": a.hop, "n_mels": a.n_mels, "clips": a.clips, "frames": frames,
                      "ms_runs": [round(float(v), 4) for v in ms], "ms_median": round(med, 4),
                      "ns_per_frame": round(1e6 * med / frames, 3)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1000)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--n-fft", dest="n_fft", type=int, default=400)
    ap.add_argument("--hop", type=int, default=160)
    ap.add_argument("--n-mels", dest="n_mels", type=int, default=40)
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = []
    for n_fft, hop, n_mels, env in ((400, 160, 40, {}), (512, 128, 128, {"AFX_NO_FRAMES3D": "1"})):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--clips", str(a.clips), "--seconds", str(a.seconds),
               "--runs", str(a.runs), "--warmup", str(a.warmup), "--n-fft", str(n_fft), "--hop", str(hop), "--n-mels", str(n_mels)]
        line = subprocess.run(cmd, env={**os.environ, **env}, check=True, stdout=subprocess.PIPE, text=True,
                              timeout=600).stdout.strip().splitlines()[-1]
        print(line)
        res.append(json.loads(line))
    mr, gen = res
    ratio = mr["ns_per_frame"] / gen["ns_per_frame"]
    text = ("Frame kernel alone (afx_plan_set_timing(plan, 2)), %d clips of %g s at 16 kHz, K = 13, device-resident float32,\n"
            "%d runs after %d warm-ups, median.  tools/frames_mr_time.py.\n\n"
            "k_frames_mr   400 / 160, n_mels  40: %9.4f ms for %d frames = %8.3f ns per frame   runs %s\n"
            "k_frames<512> 512 / 128, n_mels 128: %9.4f ms for %d frames = %8.3f ns per frame   runs %s\n"
            "ratio (ns per frame, 400 / 160 over 512 / 128): %.3f\n"
            % (a.clips, a.seconds, a.runs, a.warmup, mr["ms_median"], mr["frames"], mr["ns_per_frame"], mr["ms_runs"],
               gen["ms_median"], gen["frames"], gen["ns_per_frame"], gen["ms_runs"], ratio))
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
