"""GPU checks of afx_denoise_batch / effects.spectral_subtraction / wiener_filter / preprocess_alignment against the oracle
(tests/denoise_ref.py).

The bound on a signal is the one tests/test_gpu_hpss.py uses for the same chain (forward FFT, a gain <= 1 per bin, inverse
FFT, overlap-add): max|gpu - ref64| <= 4 max(max|ref32 - ref64|, ulp32(max|input to the STFT|)), ref32 being the oracle's
restatement in the reference's own dtypes."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import denoise_ref as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (("specsub", 0.01), ("specsub", 1.0), ("wiener", 0.0))


@pytest.fixture(scope="module")
def N():
    from audio_feature_extraction_amd import _native
    if _native.device_count() < 1:
        pytest.fail("no GPU visible")
    return _native


@pytest.fixture(scope="module")
def plan(N):
    return N.Plan(N.Context(0), N.make_params(22050, 2048, 512, 13, 128, "hann"))


def _pack(sigs):
    lengths = np.array([s.size for s in sigs], np.int64)
    offsets = np.zeros(len(sigs), np.int64)
    offsets[1:] = np.cumsum(lengths)[:-1]
    return np.concatenate(sigs).astype(np.float32), offsets, lengths


def _run(N, plan, sigs, mode, beta=0.01, **kw):
    y, off, ln = _pack(sigs)
    return plan.denoise_batch(y, off, ln, mode=N.DENOISE_WIENER if mode == "wiener" else N.DENOISE_SPECSUB, beta=beta, **kw)


@functools.lru_cache(maxsize=None)
def _cases():
    """nine clips of about 2 s: (name, sr, float32 signal)"""
    from audio_feature_extraction_amd.synth import make_clip
    out = []
    for sr in (16000, 22050, 44100):
        rng = np.random.default_rng(sr)
        lead = 0.02 * rng.standard_normal(int(0.4 * sr) + int(round(1.6 * sr)))
        body = make_clip(sr + 3, sr, 1.6).astype(np.float64)
        noise_led = lead.copy()
        noise_led[int(0.4 * sr):] += body
        n = 2 * sr + 333
        t = np.arange(n) / sr
        gate = (np.floor(t / 0.2) % 2 == 0).astype(np.float64)
        bursts = 0.4 * gate * np.sin(2 * np.pi * 300.0 * t) + 0.01 * rng.standard_normal(n)
        out += [(f"noise_led{sr}", sr, noise_led.astype(np.float32)),
                (f"speechy{sr}", sr, make_clip(sr + 1, sr, 1.7, speechy=True)),
                (f"bursts{sr}", sr, bursts.astype(np.float32))]
    return tuple(out)


def _ref(s, mode, beta, noise_frames=10, f32=False):
    return D.wiener(s, noise_frames, f32) if mode == "wiener" else D.spectral_subtraction(s, beta, noise_frames, f32)


@functools.lru_cache(maxsize=None)
def _oracle(i, mode, beta):
    """(ref64, bound, ulp) of case i, computed once"""
    s = _cases()[i][2]
    r64, r32 = _ref(s, mode, beta), _ref(s, mode, beta, f32=True)
    ulp = float(np.spacing(np.float32(np.max(np.abs(s)))))
    return r64, 4.0 * max(float(np.max(np.abs(r32 - r64))), ulp), ulp


def _check_signal(name, got, r64, bound, ulp):
    n, Lp = got.size, D.kept(got.size)
    assert got.dtype == np.float32 and r64.shape == (n,)
    assert np.isfinite(got).all(), name
    assert not got[Lp:].any(), name                                      # exact zeros behind L'
    err = float(np.max(np.abs(got - r64))) if n else 0.0
    assert err <= bound, (name, "error / ulp", err / ulp, "bound / ulp", bound / ulp)


@pytest.mark.parametrize("mode,beta", MODES)
def test_signals_match_the_oracle(N, plan, mode, beta):
    cases = _cases()
    out = _run(N, plan, [c[2] for c in cases], mode, beta)
    assert (out["status"] == 0).all()
    np.testing.assert_array_equal(out["info"], np.tile([1.0, np.nan, 0.0, 0.0], (len(cases), 1)))
    for i, (name, _, s) in enumerate(cases):
        r64, bound, ulp = _oracle(i, mode, beta)
        _check_signal(f"{name} {mode} {beta}", out["out"][i], r64, bound, ulp)
        if name.startswith("speechy") and not name.endswith("16000"):
            # a silent lead of ten frames: the profile is exactly zero, |X| = 0 occurs, and the clip comes back as it was
            assert not np.abs(D.stft(s))[:, :10].any()
            assert np.max(np.abs(out["out"][i][:D.kept(s.size)] - s[:D.kept(s.size)])) <= bound, name


SHORT = (300, 700, 1500, 4607, 4608, 5119, 5120, 5632, 8192, 8193, 40001)


def test_short_and_boundary_lengths(N, plan):
    rng = np.random.default_rng(21)
    sigs = [(0.3 * rng.standard_normal(n) * (0.2 + 0.8 * (np.arange(n) > n // 3))).astype(np.float32) for n in SHORT]
    for mode, beta in (("specsub", 1.0), ("wiener", 0.0)):
        out = _run(N, plan, sigs, mode, beta, noise_frames=10)
        assert (out["status"] == 0).all()
        for s, got in zip(sigs, out["out"]):
            r64, r32 = _ref(s, mode, beta), _ref(s, mode, beta, f32=True)
            ulp = float(np.spacing(np.float32(np.max(np.abs(s)))))
            _check_signal(f"{mode} length {s.size}", got, r64, 4.0 * max(float(np.max(np.abs(r32 - r64))), ulp), ulp)
        assert not out["out"][0].any()                                   # 300 samples: no hop fits, all zero, status OK
        for nf in (1, 64):
            got = _run(N, plan, [sigs[-1]], mode, beta, noise_frames=nf)["out"][0]
            r64, r32 = _ref(sigs[-1], mode, beta, nf), _ref(sigs[-1], mode, beta, nf, f32=True)
            ulp = float(np.spacing(np.float32(np.max(np.abs(sigs[-1])))))
            _check_signal(f"{mode} noise_frames {nf}", got, r64, 4.0 * max(float(np.max(np.abs(r32 - r64))), ulp), ulp)


def test_aligner_preprocess_matches_the_oracle(N):
    from audio_feature_extraction_amd import effects
    cases = _cases()
    for sr in (16000, 22050, 44100):
        mine = [c for c in cases if c[1] == sr]
        pl = N.Plan(N.Context(0), N.make_params(sr, 2048, 512, 13, 128, "hann"))
        out = _run(N, pl, [c[2] for c in mine], "specsub", 1.0, noise_frames=10, rms_gain=True, vad=True)
        assert (out["status"] == 0).all()
        for (name, _, s), got, info in zip(mine, out["out"], out["info"]):
            p, q = D.preprocess_alignment(s, sr), D.preprocess_alignment(s, sr, f32=True)
            Lp, F = D.kept(s.size), p["e"].size
            gain, thr, n_speech, n_frames = info
            assert abs(gain - p["gain"]) <= 1e-6 * p["gain"], (name, gain, p["gain"])
            assert abs(thr - p["thr"]) <= 1e-5 * p["thr"], (name, thr, p["thr"])
            assert n_frames == F and n_speech == int(p["speech"].sum()), (name, info, F, int(p["speech"].sum()))
            # samples whose mask hangs on a frame within 1e-3 of the threshold may go either way: at most 1 % of the frames
            close = np.flatnonzero(np.abs(p["e"] - p["thr"]) < 1e-3 * p["thr"])
            assert close.size <= 0.01 * F, (name, close.size, F)
            sure = np.ones(Lp, bool)
            for i in close:
                sure[i * p["hop"]:i * p["hop"] + p["fl"]] = False
            assert got.shape == s.shape and not got[Lp:].any() and np.isfinite(got).all(), name
            off = sure & ~p["mask"]
            assert not got[:Lp][off].any(), name                         # exactly 0.0 where the mask is off
            ulp = float(np.spacing(np.float32(np.max(np.abs(p["scaled"])))))
            bound = 4.0 * max(float(np.max(np.abs(q["d"] - p["d"]))), ulp)
            on = sure & p["mask"]
            assert on.any(), name
            err = float(np.max(np.abs(got[:Lp][on] - p["d"][on])))
            assert err <= bound, (name, "error / ulp", err / ulp, "bound / ulp", bound / ulp)
        one = effects.preprocess_alignment(mine[0][2], sr)
        assert one.dtype == np.float32 and one.shape == (D.kept(mine[0][2].size),)
        np.testing.assert_array_equal(one, out["out"][0][:one.size])
        pl.close()


def _batch50():
    from audio_feature_extraction_amd.synth import make_clip
    sigs = [make_clip(i, 22050, 0.3 + 0.05 * (i % 7), speechy=bool(i % 2)) for i in range(50)]
    sigs[20] = sigs[20].copy()
    sigs[20][777] = np.nan
    sigs[30] = np.zeros(0, np.float32)
    return sigs


# (mode, beta, rms_gain, vad): both reducers and the aligner's preprocess
_VARIANTS = (("specsub", 0.01, False, False), ("wiener", 0.0, False, False), ("specsub", 1.0, True, True))


def _all_variants(N, plan, sigs, **kw):
    y, off, ln = _pack(sigs)
    return [plan.denoise_batch(y if "samples" not in kw else kw["samples"], kw.get("offsets", off), ln,
                               mode=N.DENOISE_WIENER if m == "wiener" else N.DENOISE_SPECSUB, beta=b, rms_gain=g, vad=v,
                               **{k: x for k, x in kw.items() if k not in ("samples", "offsets")})
            for m, b, g, v in _VARIANTS]


def _assert_same(a, b, what):
    np.testing.assert_array_equal(a["status"], b["status"], err_msg=what)
    np.testing.assert_array_equal(a["info"], b["info"], err_msg=what)
    for i, (u, v) in enumerate(zip(a["out"], b["out"])):
        np.testing.assert_array_equal(u, v, err_msg=f"{what} clip {i}")


def test_failed_clips_are_isolated_and_runs_are_deterministic(N, plan):
    sigs = _batch50()
    a, b = _all_variants(N, plan, sigs), _all_variants(N, plan, sigs)
    for k, (ra, rb) in enumerate(zip(a, b)):
        assert ra["status"][20] == N.CLIP_NONFINITE and ra["status"][30] == N.CLIP_TOO_SHORT
        assert (np.delete(ra["status"], [20, 30]) == 0).all()
        assert np.isnan(ra["info"][20]).all() and np.isnan(ra["info"][30]).all()
        assert ra["out"][20].shape == sigs[20].shape and not ra["out"][20].any() and ra["out"][30].size == 0
        assert np.isfinite(np.concatenate(ra["out"])).all()
        _assert_same(ra, rb, f"variant {k}, second run")
    for i in (0, 19, 21, 29, 31, 49):
        solo = _all_variants(N, plan, [sigs[i]])
        for k in range(len(_VARIANTS)):
            np.testing.assert_array_equal(solo[k]["out"][0], a[k]["out"][i], err_msg=f"variant {k} clip {i}")
            np.testing.assert_array_equal(solo[k]["info"][0], a[k]["info"][i], err_msg=f"variant {k} clip {i}")
    # the VAD refuses what has no hop to frame: fewer than 512 samples is too short there, and only there
    short = [sigs[0][:511], sigs[1][:512]]
    plain, pre = _all_variants(N, plan, short)[0], _all_variants(N, plan, short)[2]
    assert plain["status"].tolist() == [0, 0] and pre["status"].tolist() == [N.CLIP_TOO_SHORT, 0]
    assert not pre["out"][0].any() and np.isnan(pre["info"][0]).all() and pre["info"][1][3] == D.vad_frames(512, 22050)[2]


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_denoise import _all_variants, _batch50
from audio_feature_extraction_amd import _native as N
plan = N.Plan(N.Context(0), N.make_params(22050, 2048, 512, 13, 128, "hann"))
res = _all_variants(N, plan, _batch50())
np.savez(sys.argv[2], **{"%s%d" % (k, i): (np.concatenate(r["out"]) if k == "out" else r[k])
                         for i, r in enumerate(res) for k in ("out", "info", "status")})
"""


def test_chunked_batch_equals_one_chunk(N, plan, tmp_path):
    sigs = _batch50()
    lengths = [s.size for s in sigs]
    budget = 2000000
    for flags in (0, N.DENOISE_RMS_GAIN | N.DENOISE_VAD):
        assert N.stft_chunks(lengths, N.denoise_cost(flags), budget).max() + 1 >= 4
        assert N.stft_chunks(lengths, N.denoise_cost(flags), 2 << 30).max() == 0
    ref = _all_variants(N, plan, sigs)
    env = dict(os.environ, AFX_TEST_HPSS_BUDGET=str(budget))
    dst = str(tmp_path / "chunked.npz")
    subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _CHILD, ROOT, dst], env=env, check=True, timeout=150)
    z = np.load(dst)
    for i, r in enumerate(ref):
        np.testing.assert_array_equal(z[f"status{i}"], r["status"], err_msg=f"variant {i}")
        np.testing.assert_array_equal(z[f"info{i}"], r["info"], err_msg=f"variant {i}")
        np.testing.assert_array_equal(z[f"out{i}"], np.concatenate(r["out"]), err_msg=f"variant {i}")


_LAYOUTS_LENGTHS = (5000, 12345, 700, 9000, 3000, 7000)


def _layouts(N, plan):
    """s16, device-resident and reverse-ordered (NaN-filled gaps) inputs against the packed host float32 batch"""
    rng = np.random.default_rng(4)
    q = [rng.integers(-20000, 20000, n).astype(np.int16) for n in _LAYOUTS_LENGTHS]
    f = [x.astype(np.float32) / 32768.0 for x in q]
    y, off, ln = _pack(f)
    ref = _all_variants(N, plan, f)
    assert all((r["status"] == 0).all() for r in ref)
    s16 = _all_variants(N, plan, f, samples=np.concatenate(q), fmt=N.FMT_S16)
    dev = plan.device_buffer(y.nbytes)
    dev.upload(y)
    d = _all_variants(N, plan, f, samples=dev.ptr, mem=N.MEM_DEVICE)
    dev.free()
    roff = np.zeros(len(f), np.int64)                      # the last clip first, 37 samples between neighbours
    for i in range(len(f) - 2, -1, -1):
        roff[i] = roff[i + 1] + ln[i + 1] + 37
    ry = np.full(int(roff[0] + ln[0]), np.nan, np.float32)           # a gap that is read would poison its clip
    for s, o in zip(f, roff):
        ry[o:o + s.size] = s
    r = _all_variants(N, plan, f, samples=ry, offsets=roff)
    for name, o in (("s16", s16), ("device", d), ("reversed", r)):
        for k in range(len(_VARIANTS)):
            _assert_same(o[k], ref[k], f"{name} variant {k}")


def test_s16_device_and_scattered_inputs_match_host_f32(N, plan):
    _layouts(N, plan)


_LAYOUTS_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_denoise import _layouts
from audio_feature_extraction_amd import _native as N
_layouts(N, N.Plan(N.Context(0), N.make_params(22050, 2048, 512, 13, 128, "hann")))
"""


def test_chunked_layouts_equal_the_packed_host_batch(N):
    """the same comparison with every call cut into chunks: chunks behind the first read device input at offsets that
    are not rebased, and clips laid out in reverse order take the per-clip copy of the output"""
    for flags, fmt, mem in ((0, N.FMT_F32, N.MEM_HOST), (N.DENOISE_VAD, N.FMT_S16, N.MEM_HOST), (0, N.FMT_F32, N.MEM_DEVICE)):
        assert N.stft_chunks(_LAYOUTS_LENGTHS, N.denoise_cost(flags, fmt, mem), 400000).max() + 1 >= 3
    env = dict(os.environ, AFX_TEST_HPSS_BUDGET="400000")
    subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _LAYOUTS_CHILD, ROOT], env=env, check=True, timeout=150)


def test_effects_and_extractor_api(N):
    from audio_feature_extraction_amd import AudioFeatureExtractor, effects
    name, sr, y = _cases()[3]                                            # noise_led22050
    a = effects.spectral_subtraction(y, sr)
    w = effects.wiener_filter(y, sr)
    assert a.dtype == w.dtype == np.float32 and a.shape == w.shape == y.shape
    r64, bound, ulp = _oracle(3, "specsub", 0.01)
    _check_signal("effects.spectral_subtraction", a, r64, bound, ulp)
    r64, bound, ulp = _oracle(3, "wiener", 0.0)
    _check_signal("effects.wiener_filter", w, r64, bound, ulp)
    both = effects.spectral_subtraction_batch([y, y[:1000], y[:300]], sr)
    np.testing.assert_array_equal(both[0], a)
    assert both[1].shape == (1000,) and both[2].shape == (300,) and not both[2].any()
    wb = effects.wiener_filter_batch([y[:5000], y], sr, noise_frames=10)
    np.testing.assert_array_equal(wb[1], w)
    np.testing.assert_array_equal(effects.spectral_subtraction(y.astype(np.float64), sr, beta=1.0),
                                  effects.spectral_subtraction_batch([y], sr, beta=1.0)[0])
    with pytest.raises(NotImplementedError):
        effects.spectral_subtraction(y, sr, frame_length=1024)
    with pytest.raises(NotImplementedError):
        effects.wiener_filter(y, sr, frame_length=1024, hop_length=256)
    bad = y.copy()
    bad[100] = np.inf
    with pytest.raises(ValueError):
        effects.spectral_subtraction(bad, sr)
    with pytest.raises(ValueError):
        effects.wiener_filter_batch([y, bad], sr)
    with pytest.raises(ValueError):
        effects.preprocess_alignment(bad, sr)
    with pytest.raises(ValueError):
        effects.preprocess_alignment(y[:400], sr)
    fx = AudioFeatureExtractor(sr=sr)
    p = fx.preprocess_alignment(y)
    assert p.dtype == np.float32 and p.shape == (D.kept(y.size),)
    np.testing.assert_array_equal(p, effects.preprocess_alignment(y, sr))
    res = fx.preprocess_alignment_batch([y, bad, y[:400], y[:6000]])
    assert res[1] is None and res[2] is None and res[3].shape == (D.kept(6000),)
    np.testing.assert_array_equal(res[0], p)
    assert fx.preprocess_alignment_batch([]) == []
