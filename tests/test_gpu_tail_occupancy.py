"""k_tail's one-slot form (AFX_TAIL_MODE=5, and 6 with nt DMA pieces: one 8 KB LDS-DMA slot per wave, the DCT images in
registers, four workgroups per CU) against the 4 x 2 ring form it replaces as the default for up to 16 coefficients (AFX_TAIL_MODE=4), against the
two-kernel tail, and against the oracle, at 22050 / 1024 / 256 / 13.

The developer switches are read once per process, so every mode runs in a child process of its own; the children run once
per session and the tests share what they wrote.

Two batches.  "many": more clips than workgroups can be resident (4 per CU; the CU count is asked of the device), so that
workgroups walk a second clip.  "few": fewer than 32 clips.  Both hold the same special clips -- "many" at its start and
again behind the last resident workgroup:
  9 and 10 frames (one tile, the delta's minimum), 16 and 17 (tile boundary), 64 and 65 (one tile per wave / wave 0 gets a
  second), clips with leading silence (the trimmed frame offset is > 0 and the tiles start off the 16-frame grid of the
  spill), a last tile that runs past the last frame (every frame count that is no multiple of 16), fewer than 9 frames
  (energy only), a non-finite sample."""
import os
import subprocess
import sys

import numpy as np
import pytest

from audio_feature_extraction_amd.synth import make_clip

SR, N_FFT, HOP, K = 22050, 1024, 256, 13
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECIAL_FRAMES = (9, 10, 16, 17, 64, 65)
I_SILENCE = (6, 7, 8)            # leading and trailing silence, three lengths
I_SHORT, I_NONFINITE = 9, 10
N_SPECIAL = 11


def special_clips():
    """The eleven special clips.  A clip of n hop - 1 samples has n frames (1 + len // hop)."""
    clips = [make_clip(900 + i, SR, 1.0)[: n * HOP - 1].copy() for i, n in enumerate(SPECIAL_FRAMES)]
    clips += [make_clip(910 + i, SR, s, speechy=True) for i, s in enumerate((0.9, 1.0, 1.13))]
    clips.append(make_clip(920, SR, 1.0)[: 5 * HOP].copy())                  # 6 frames: MFCC fails, energy stays
    bad = make_clip(921, SR, 0.5).copy()
    bad[777] = np.inf
    clips.append(bad)
    return clips


def batches(n_cu):
    """{name: list of clips}.  Fillers: 0.1 s (9 frames) .. 0.3 s, 24 distinct ones repeated."""
    fill = [make_clip(1000 + i, SR, 0.1 + 0.01 * (i % 21)) for i in range(24)]
    sp = special_clips()
    n_many = max(1100, 4 * n_cu + 76)
    many = sp + [fill[i % len(fill)] for i in range(n_many - 2 * len(sp))] + sp
    few = sp + fill[:9]
    return {"many": many, "few": few}


def pack(clips):
    lens = np.array([c.size for c in clips], np.int64)
    offs = np.zeros(len(clips), np.int64)
    offs[1:] = np.cumsum((lens + 3) // 4 * 4)[:-1]
    buf = np.zeros(int(offs[-1] + lens[-1]) + 8, np.float32)
    for c, o in zip(clips, offs):
        buf[o:o + c.size] = c
    return buf, offs, lens


_CHILD = r"""
import sys
sys.path.insert(0, {root!r})
import numpy as np
import torch
from audio_feature_extraction_amd import _native as N
from tests.test_gpu_tail_occupancy import SR, N_FFT, HOP, K, batches, pack
n_cu = torch.cuda.get_device_properties(0).multi_processor_count
out = {{"n_cu": np.array(n_cu)}}
ctx = N.Context(0)
plan = N.Plan(ctx, N.make_params(SR, N_FFT, HOP, K))
for name, clips in batches(n_cu).items():
    buf, offs, lens = pack(clips)
    for tag, res in (("one", plan.extract_batch(buf, offs, lens)),) + \
                    ((("two", plan.extract_batch(buf, offs, lens, want_frames=True)),) if {two!r} else ()):
        for key in ("status", "trim", "nframes", "stats"):
            out["%s_%s_%s" % (name, tag, key)] = np.asarray(res[key])
plan.close()
ctx.close()
np.savez({path!r}, **out)
print("ok")
"""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{mode: arrays of the child that ran with AFX_TAIL_MODE=mode}; "default": the variable unset (that child also runs
    the two-kernel tail)."""
    tmp = tmp_path_factory.mktemp("tail_modes")
    procs = {}
    for mode in ("default", "5", "6", "4"):                  # side by side: four processes on the GPU
        path = str(tmp / ("mode_%s.npz" % mode))
        env = {k: v for k, v in os.environ.items() if k not in ("AFX_TAIL_MODE", "AFX_NO_FUSED_TAIL")}
        if mode != "default":
            env["AFX_TAIL_MODE"] = mode
        procs[mode] = (path, subprocess.Popen([sys.executable, "-c", _CHILD.format(root=ROOT, path=path, two=(mode == "default"))],
                                              env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    res = {}
    for mode, (path, proc) in procs.items():
        out, err = proc.communicate(timeout=300)
        assert proc.returncode == 0 and out.strip().endswith("ok"), (mode, out[-1500:], err[-3000:])
        with np.load(path) as z:
            res[mode] = {k: z[k] for k in z.files}
    return res


def special_positions(name, n):
    return list(range(N_SPECIAL)) + ([] if name == "few" else list(range(n - N_SPECIAL, n)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["many", "few"])
def test_batches_hold_the_cases_they_are_meant_to(runs, name):
    """Frame counts, trims and statuses of the special clips are what the cases above say, and "many" is larger than the
    number of workgroups the chip holds."""
    from audio_feature_extraction_amd import _native as N
    d = runs["default"]
    status, trim, nframes = d[name + "_one_status"], d[name + "_one_trim"], d[name + "_one_nframes"]
    n = status.shape[0]
    if name == "many":
        assert n > 4 * int(d["n_cu"])
    else:
        assert n < 32
    for base in special_positions(name, n)[::N_SPECIAL]:
        assert [int(v) for v in nframes[base:base + len(SPECIAL_FRAMES)]] == list(SPECIAL_FRAMES)
        assert (status[base:base + len(SPECIAL_FRAMES)] == 0).all()
        offgrid = 0
        for i in I_SILENCE:
            start = int(np.asarray(trim[base + i]).reshape(-1)[0])
            assert status[base + i] == 0 and start > 0
            offgrid += (start // HOP) % 16 != 0
        assert offgrid >= 1
        assert any(int(nframes[base + i]) % 16 != 0 for i in I_SILENCE)
        assert status[base + I_SHORT] == N.CLIP_TOO_SHORT and status[base + I_NONFINITE] == N.CLIP_NONFINITE
        assert d[name + "_one_stats"][base + I_SHORT][4 * K] > 0.0 and not d[name + "_one_stats"][base + I_SHORT][:4 * K].any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["many", "few"])
@pytest.mark.parametrize("mode", ["5", "6", "default"])
def test_one_slot_tail_equals_the_ring_tail_bit_for_bit(runs, name, mode):
    """Same tile -> wave assignment, same MFMA order, same float64 sums: statuses, trims, frame counts and statistics of the
    one-slot form (asked for by number with either cache policy, and as the default) are the bits of AFX_TAIL_MODE=4."""
    a, b = runs[mode], runs["4"]
    for key in ("status", "trim", "nframes"):
        assert np.array_equal(a["%s_one_%s" % (name, key)], b["%s_one_%s" % (name, key)]), key
    sa, sb = a[name + "_one_stats"], b[name + "_one_stats"]
    assert sa.dtype == np.float32 and sa.shape == sb.shape
    diff = np.nonzero((sa.view(np.uint32) != sb.view(np.uint32)).any(axis=1))[0]
    assert diff.size == 0, ("clips whose statistics differ", diff[:20])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["many", "few"])
@pytest.mark.parametrize("mode", ["5", "6"])
def test_one_slot_tail_equals_the_two_kernel_tail(runs, name, mode):
    """Against k_dct16* + k_stats (a batch with per-frame output): the bound of test_fused_tail_equals_the_two_kernel_tail,
    2e-5 on each value's own scale, floored at 1e-2 of the clip's largest coefficient mean."""
    d, o = runs["default"], runs[mode]
    for key in ("status", "trim", "nframes"):
        assert np.array_equal(o["%s_one_%s" % (name, key)], d["%s_two_%s" % (name, key)]), key
    one, two, status = o[name + "_one_stats"], d[name + "_two_stats"], o[name + "_one_status"]
    worst = 0.0
    for i in range(status.shape[0]):
        a, b = one[i].astype(np.float64), two[i].astype(np.float64)
        if status[i] == 0:
            scale = np.maximum(np.abs(b), 1e-2 * np.abs(b[:K]).max())
            worst = max(worst, float((np.abs(a - b) / scale).max()))
            assert (np.abs(a - b) <= 2e-5 * scale).all(), (i, np.abs(a - b).max())
        else:
            assert np.array_equal(a, b), i
    print("%s: largest own-scale difference to the two-kernel tail %.3g" % (name, worst))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["5", "6"])
def test_one_slot_tail_matches_the_oracle(runs, mode):
    """A handful of clips of "many" -- the special ones of the second round and two fillers -- through the parity gate (1e-4)."""
    from tests.parity import check_stats, oracle_stats
    d = runs[mode]
    clips = batches(int(d["n_cu"]))["many"]
    n = len(clips)
    for i in [n - N_SPECIAL + j for j in (0, 1, 3, 5, 6, 8)] + [N_SPECIAL + 3, n - N_SPECIAL - 1]:
        assert d["many_one_status"][i] == 0
        check_stats(d["many_one_stats"][i], oracle_stats(clips[i], SR, N_FFT, HOP, K), K, "one-slot tail clip %d" % i)
