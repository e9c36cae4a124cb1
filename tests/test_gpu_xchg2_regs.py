"""The second FFT exchange of k_frames3 (1024 / 256) and k_frames3s (2048 / 512): the half that butterfly ja reads goes from
pass 2 to pass 3 by lane swaps (a transpose between lane rows and registers) instead of through the LDS image.  The change
moves data and does no arithmetic, so every result is the bits of the all-LDS form, which AFX_F3_XCHG2=lds selects.

The switch is read once per process, so each form runs in a child process of its own: AFX_F3_XCHG2 unset (the default) and
=lds, each under nothing, AFX_F3_WAVES=12 and AFX_F3_GENERIC_MEL=1 -- six processes, side by side, once per session.  Both
shapes that hold the exchange take the swap form by default (afx_frames3.hip: f3_xchg2_swap), so the unset children run it.

Batches (tests/test_gpu_spare_cus.py builds them): at 22050 / 1024 / 256 / 13 (bench configuration 2) the 40 ragged clips of
0.3 .. 3 s, at 44100 / 2048 / 512 / 20 (5) the first 16 of them; the first four are a 9-frame clip (a last odd pair), a clip
trimmed at both ends (the redo launch), an all-zero clip and a non-finite clip; the others reach the first block of a run,
chained blocks and clip edges.  16000 / 512 / 128 / 40 (3), whose kernel is untouched, runs in the pair without other
switches as a control.  That pair also feeds the batches of 2 and 5 as int16 samples (the non-finite clip, which int16
cannot hold, as its finite samples).  Each batch goes through extract_batch once and through four extract_submit /
extract_collect steps on two plans."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_spare_cus import CONFIGS, I_NINE, I_NONFINITE, I_SPEECHY, I_ZERO, clips_of, pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 4
KEYS = ("stats", "status", "trim", "nframes")
CHANGED = (2, 5)                          # configurations whose frame kernel holds the exchange
VARIANTS = {"plain": {}, "waves12": {"AFX_F3_WAVES": "12"}, "generic_mel": {"AFX_F3_GENERIC_MEL": "1"}}
FORMS = ("default", "lds")


def pack_s16(clips):
    """The same layout as pack(), the samples as int16 (x 32767, rounded; a non-finite sample becomes 0)."""
    buf, offs, lens = pack(clips)
    return np.round(np.nan_to_num(buf, nan=0.0, posinf=0.0, neginf=0.0) * 32767.0).astype(np.int16), offs, lens


_CHILD = r"""
import sys
sys.path.insert(0, {root!r})
import numpy as np
from audio_feature_extraction_amd import _native as N
from tests.test_gpu_spare_cus import CONFIGS, clips_of, pack
from tests.test_gpu_xchg2_regs import KEYS, STEPS, pack_s16
out = {{}}
for tag in {tags!r}:
    cfg, s16 = int(tag[1]), tag.endswith("s16")
    sr, n_fft, hop, k, _ = CONFIGS[cfg]
    buf, offs, lens = (pack_s16 if s16 else pack)(clips_of(cfg))
    fmt = N.FMT_S16 if s16 else N.FMT_F32
    ctxs = [N.Context(0), N.Context(0)]
    plans = [N.Plan(c, N.make_params(sr, n_fft, hop, k)) for c in ctxs]
    res = plans[0].extract_batch(buf, offs, lens, fmt=fmt)
    for key in KEYS:
        out["%s_batch_%s" % (tag, key)] = np.asarray(res[key]).copy()
    busy, step_of, done = [False, False], [0, 0], {{}}
    for i in range(STEPS):
        p = i % 2
        if busy[p]:
            done[step_of[p]] = plans[p].extract_collect()
        plans[p].extract_submit(buf, offs, lens, fmt=fmt)
        busy[p], step_of[p] = True, i
    for p in (0, 1):
        if busy[p]:
            done[step_of[p]] = plans[p].extract_collect()
    for i, res in done.items():
        for key in KEYS:
            out["%s_step%d_%s" % (tag, i, key)] = np.asarray(res[key]).copy()
    for p in plans:
        p.close()
    for c in ctxs:
        c.close()
np.savez({path!r}, **out)
print("ok")
"""


def tags_of(variant):
    """What a child of the variant runs: "c<cfg>" float32 batches, "c<cfg>s16" int16 ones."""
    tags = ["c%d" % cfg for cfg in CHANGED]
    if variant == "plain":
        tags += ["c3"] + ["c%ds16" % cfg for cfg in CHANGED]
    return tags


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{(variant, form): arrays of the child that ran with the variant's switches and AFX_F3_XCHG2 unset / =lds}."""
    tmp = tmp_path_factory.mktemp("xchg2")
    base = {k: v for k, v in os.environ.items() if k not in ("AFX_F3_XCHG2", "AFX_F3_WAVES", "AFX_F3_GENERIC_MEL")}
    procs = {}
    for variant, extra in VARIANTS.items():                   # side by side: six processes on the GPU
        for form in FORMS:
            path = str(tmp / ("%s_%s.npz" % (variant, form)))
            env = dict(base, **extra)
            if form != "default":
                env["AFX_F3_XCHG2"] = form
            code = _CHILD.format(root=ROOT, path=path, tags=tags_of(variant))
            procs[variant, form] = (path, subprocess.Popen([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE,
                                                           stderr=subprocess.PIPE, text=True))
    res = {}
    for key, (path, proc) in procs.items():
        out, err = proc.communicate(timeout=300)
        assert proc.returncode == 0 and out.strip().endswith("ok"), (key, out[-1500:], err[-3000:])
        with np.load(path) as z:
            res[key] = {k: z[k] for k in z.files}
    return res


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_same_as_lds(runs, variant, tag):
    got_all, want_all = runs[variant, "default"], runs[variant, "lds"]
    for what in ["batch"] + ["step%d" % i for i in range(STEPS)]:
        for key in KEYS:
            got, want = got_all["%s_%s_%s" % (tag, what, key)], want_all["%s_%s_%s" % (tag, what, key)]
            assert got.shape == want.shape and got.dtype == want.dtype, (what, key)
            a, b = got.reshape(got.shape[0], -1), want.reshape(want.shape[0], -1)
            diff = np.nonzero([x.tobytes() != y.tobytes() for x, y in zip(a, b)])[0]
            assert diff.size == 0, ("clips whose %s differ from the all-LDS form" % key, variant, tag, what, diff[:20])
            assert same_bits(got, want), (what, key)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CHANGED)
def test_batches_hold_the_cases_they_are_meant_to(runs, cfg):
    from audio_feature_extraction_amd import _native as N
    d = runs["plain", "lds"]
    n = CONFIGS[cfg][4]
    status, trim, nframes = d["c%d_batch_status" % cfg], d["c%d_batch_trim" % cfg], d["c%d_batch_nframes" % cfg]
    assert status.shape[0] == n
    assert status[I_NINE] == 0 and nframes[I_NINE] == 9                                    # a last pair with one frame
    clip = clips_of(cfg)[I_SPEECHY]
    assert status[I_SPEECHY] == 0 and trim[I_SPEECHY][0] > 0 and trim[I_SPEECHY][1] < clip.size       # cut at both ends: redo
    assert status[I_NONFINITE] == N.CLIP_NONFINITE
    assert not clips_of(cfg)[I_ZERO].any()
    assert (np.delete(status, [I_ZERO, I_NONFINITE]) == 0).all()
    # chained blocks (more than 16 frames in a clip) and clips that end in an odd and in an even number of frames
    assert nframes.max() > 32 and (nframes[status == 0] % 2 == 1).any() and (nframes[status == 0] % 2 == 0).any()
    # the int16 batch holds the same clips; its non-finite clip is finite
    s = runs["plain", "lds"]["c%ds16_batch_status" % cfg]
    assert s.shape[0] == n and s[I_NINE] == 0 and s[I_SPEECHY] == 0 and s[I_NONFINITE] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CHANGED)
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_every_result_is_the_all_lds_form_bit_for_bit(runs, variant, cfg):
    assert_same_as_lds(runs, variant, "c%d" % cfg)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CHANGED)
def test_int16_samples_bit_for_bit(runs, cfg):
    assert_same_as_lds(runs, "plain", "c%ds16" % cfg)


@pytest.mark.gpu
def test_the_untouched_kernel_is_a_control(runs):
    assert_same_as_lds(runs, "plain", "c3")
