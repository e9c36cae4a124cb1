"""GPU tests of afx_gate_batch (spectral-gating noise reduction, noisereduce's reduce_noise) and of effects.reduce_noise /
AudioFeatureExtractor.apply_noise_reduction / process_recordings_batch against the float64 oracle of tests/gate_ref.py.

Clips: 2 s of a gated two-tone plus white noise (gate_ref.make_clip), one with its first eighth zeroed, one with a separate
noise clip, one of 3000 samples, at 16000 and 22050 Hz and n_fft 1024 and 2048, in both modes; and the lengths at which the
framing can go wrong.

Tolerances are multiples of what the oracle's float32-faithful form (f32=True) loses against its float64 form on these same
clips -- the yardsticks, computed here from the oracle alone, never from the device:
  thresholds   |thr_device - thr_64| <= 4 x the largest |thr_32 - thr_64|, dB
  hard mask    against the oracle's decision taken with the *device's* thresholds; a bin may differ only where |X_64| lies
               within kappa max_b |X_64[b, t]| of the threshold amplitude, kappa = 4 x the largest | |X_32| - |X_64| | /
               max_b |X_64[b, t]|, and at most 1e-4 of a clip's bins may differ at all
  signal       against the oracle evaluated with the device's hard mask (stationary) or as it is (non-stationary), relative to
               max|y|: 4 x the float32-faithful form's largest error, per mode
The clips of the length test are test clips too: where the float32 form loses more on one of them than on the clips above (a
clip of 1023 samples has two noise frames at n_fft 2048, and a threshold from two values moves with either), that clip's own
figure is its yardstick.
Measured 2026-10-21 (yardstick -> bound; observed on an MI355X):
  thresholds   1.22e-4 dB -> 4.9e-4 dB; device up to 2.4e-4 dB; the 1023-sample clip 3.8e-4 -> 1.5e-3 dB, device 1.1e-3 dB
  kappa        6.6e-8 -> 2.6e-7; no bin of any test clip differed
  signal       stationary 1.21e-7 -> 4.8e-7, device up to 1.8e-7; non-stationary 1.88e-7 -> 7.5e-7, device up to 3.1e-7
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import gate_ref as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(16000, 1024), (16000, 2048), (22050, 1024), (22050, 2048)]
STAT_KW = dict(stationary=True, prop_decrease=0.95)           # config/experiment_config.yaml's values
NONSTAT_KW = dict(stationary=False)


@pytest.fixture(scope="module")
def N():
    from audio_feature_extraction_amd import _native
    if _native.device_count() < 1:
        pytest.fail("no GPU visible")
    return _native


@pytest.fixture(scope="module")
def ctx(N):
    return N.Context(0)


def _kw(stationary, n_fft):
    return dict(STAT_KW if stationary else NONSTAT_KW, n_fft=n_fft)


@functools.lru_cache(maxsize=None)
def _clips(sr):
    """name -> (clip, noise clip or None); read-only"""
    y = G.make_clip(sr)
    out = {"plain": (y, None), "silence": (G.make_clip(sr, silence=True, seed=1), None), "noise": (y, G.noise_clip(sr)),
           "short": (y[:3000].copy(), None)}
    for a, b in out.values():
        a.setflags(write=False)
        if b is not None:
            b.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _oracle(sr, n_fft, stationary, name, f32):
    """(out, parts) of the oracle on a named test clip; computed once and shared"""
    y, noise = _clips(sr)[name]
    parts = {}
    out = G.reduce_noise(y, sr, y_noise=noise if stationary else None, f32=f32, parts=parts, **_kw(stationary, n_fft))
    return out, parts


@functools.lru_cache(maxsize=None)
def _yard():
    """The yardsticks over every test clip and configuration: thr (dB), kappa, signal error per mode (of max|y|)."""
    thr = kap = 0.0
    sig = {True: 0.0, False: 0.0}
    for sr, n_fft in CONFIGS:
        for name, (y, noise) in _clips(sr).items():
            for stationary in (True, False):
                if noise is not None and not stationary:
                    continue
                a, p64 = _oracle(sr, n_fft, stationary, name, False)
                b, p32 = _oracle(sr, n_fft, stationary, name, True)
                sig[stationary] = max(sig[stationary], float(np.abs(a.astype(np.float64) - b).max() / np.abs(y).max()))
                if stationary:
                    assert np.array_equal(p64["hard"], p32["hard"]), "choose clips the float32 form itself does not flip"
                    thr = max(thr, float(np.abs(p64["thr"] - p32["thr"]).max()))
                    A64, A32 = np.abs(p64["X"]), np.abs(p32["X"])
                    top = np.maximum(A64.max(axis=0, keepdims=True), np.finfo(np.float64).tiny)
                    kap = max(kap, float((np.abs(A32 - A64) / top).max()))
    return {"thr": thr, "kappa": kap, "sig": sig}


def _pack(N, clips):
    lengths = np.array([c.size for c in clips], np.int64)
    offsets = N.packed_offsets(lengths, 4)
    buf = np.zeros(int((offsets + lengths).max()), clips[0].dtype)
    for o, c in zip(offsets, clips):
        buf[o:o + c.size] = c
    return buf, offsets, lengths


def _gate(N, ctx, clips, sr, kw, noise=None, **more):
    """clips (and one noise clip each) through afx_gate_batch from a packed host buffer -> (list of outputs, result)"""
    parts = list(clips) + (list(noise) if noise is not None else [])
    buf, offsets, lengths = _pack(N, parts)
    n = len(clips)
    r = ctx.gate_batch(buf, offsets[:n], lengths[:n], N.gate_opts(sr, **kw),
                       noise_offsets=offsets[n:] if noise is not None else None,
                       noise_lengths=lengths[n:] if noise is not None else None, **more)
    return [r["out"][o:o + l] for o, l in zip(r["offsets"], lengths[:n])], r


def _check_stationary(name, y, noise, sr, kw, dev, thr, mask, bound, thr_yard=0.0):
    """thresholds, the decision and the signal of one stationary clip against the oracle; thr_yard: the float32 form's own
    threshold deviation on this clip, where the clip is not one of _yard()'s"""
    yd = dict(_yard())
    yd["thr"] = max(yd["thr"], thr_yard)
    p64 = {}
    G.reduce_noise(y, sr, y_noise=noise, parts=p64, **kw)
    thr_err = float(np.abs(thr - p64["thr"]).max())
    # the oracle's decision with the device's thresholds
    pd = {}
    ref = G.reduce_noise(y, sr, y_noise=noise, thresh=thr, parts=pd, **kw)
    diff = mask != pd["hard"]
    print(f"{name}: thr err {thr_err:.3g} dB (bound {4 * yd['thr']:.3g}), bins that differ {int(diff.sum())} of {diff.size}")
    assert thr_err <= 4 * yd["thr"], name
    assert diff.sum() <= 1e-4 * diff.size, name
    if diff.any():
        A = np.abs(pd["X"])
        margin = np.abs(A + G.EPS - 10.0 ** (thr[:, None] / 20.0))
        allowed = margin <= 4 * yd["kappa"] * A.max(axis=0, keepdims=True)
        assert np.all(allowed[diff]), f"{name}: a bin far from its threshold was decided differently"
        ref = G.reduce_noise(y, sr, y_noise=noise, hard_mask=mask, **kw)
    err = float(np.abs(dev.astype(np.float64) - ref).max() / np.abs(y).max())
    print(f"{name}: signal err {err:.3g} of max|y| (bound {bound:.3g})")
    assert err <= bound, name


@pytest.mark.parametrize("sr,n_fft", CONFIGS)
def test_stationary_against_the_oracle(N, ctx, sr, n_fft):
    kw = _kw(True, n_fft)
    bound = 4 * _yard()["sig"][True]
    names = ["plain", "silence", "short"]
    outs, r = _gate(N, ctx, [_clips(sr)[k][0] for k in names], sr, kw, want_thresh=True, want_mask=True)
    assert list(r["status"]) == [N.CLIP_OK] * 3
    for i, k in enumerate(names):
        assert outs[i].dtype == np.float32 and r["mask"][i].shape == (n_fft // 2 + 1, G.n_frames(outs[i].size, n_fft // 4))
        _check_stationary(f"{sr}/{n_fft}/{k}", _clips(sr)[k][0], None, sr, kw, outs[i], r["thresh"][i], r["mask"][i], bound)
    y, noise = _clips(sr)["noise"]
    outs, r = _gate(N, ctx, [y], sr, kw, noise=[noise], want_thresh=True, want_mask=True)
    assert list(r["status"]) == [N.CLIP_OK]
    _check_stationary(f"{sr}/{n_fft}/noise", y, noise, sr, kw, outs[0], r["thresh"][0], r["mask"][0], bound)


@pytest.mark.parametrize("sr,n_fft", CONFIGS)
def test_nonstationary_against_the_oracle(N, ctx, sr, n_fft):
    kw = _kw(False, n_fft)
    bound = 4 * _yard()["sig"][False]
    names = ["plain", "silence", "short"]
    outs, r = _gate(N, ctx, [_clips(sr)[k][0] for k in names], sr, kw)
    assert list(r["status"]) == [N.CLIP_OK] * 3
    for i, k in enumerate(names):
        y = _clips(sr)[k][0]
        err = float(np.abs(outs[i].astype(np.float64) - _oracle(sr, n_fft, False, k, False)[0]).max() / np.abs(y).max())
        print(f"{sr}/{n_fft}/{k}: signal err {err:.3g} of max|y| (bound {bound:.3g})")
        assert err <= bound, k


@pytest.mark.parametrize("stationary", [True, False])
@pytest.mark.parametrize("n_fft", [1024, 2048])
def test_lengths_at_which_the_framing_can_go_wrong(N, ctx, stationary, n_fft):
    """1 sample, n_fft / 2 -+ 1, hop k -+ 1, a whole number of hops with the padding ((L + 60000) % hop == 0), and one more"""
    sr, hop = 16000, n_fft // 4
    whole = hop * (60000 // hop + 5) - 60000
    lengths = [1, n_fft // 2 - 1, n_fft // 2 + 1, 3 * hop - 1, 3 * hop + 1, whole, whole + 1]
    assert (whole + 60000) % hop == 0 and 60000 % hop != 0
    clips = [G.make_clip(sr, seed=10 + i, length=L) for i, L in enumerate(lengths)]
    kw = _kw(stationary, n_fft)
    outs, r = _gate(N, ctx, clips, sr, kw, want_thresh=True, want_mask=True)
    assert list(r["status"]) == [N.CLIP_OK] * len(clips)
    yard = _yard()["sig"][stationary]
    for i, y in enumerate(clips):
        assert outs[i].shape == y.shape
        p64, p32 = {}, {}
        f64 = G.reduce_noise(y, sr, parts=p64, **kw).astype(np.float64)
        own = float(np.abs(G.reduce_noise(y, sr, f32=True, parts=p32, **kw) - f64).max() / np.abs(y).max())
        bound = 4 * max(yard, own)                                   # these clips are test clips too: their yardsticks count
        if stationary:
            assert np.array_equal(p64["hard"], p32["hard"])
            _check_stationary(f"{n_fft}/L={y.size}", y, None, sr, kw, outs[i], r["thresh"][i], r["mask"][i], bound,
                              thr_yard=float(np.abs(p64["thr"] - p32["thr"]).max()))
        else:
            err = float(np.abs(outs[i] - f64).max() / np.abs(y).max())
            print(f"{n_fft}/L={y.size}: signal err {err:.3g} of max|y| (bound {bound:.3g})")
            assert err <= bound, y.size


@pytest.mark.parametrize("stationary", [True, False])
def test_a_clip_of_chunk_size_passes_and_one_more_sample_fails(N, ctx, stationary):
    sr = 16000
    y = G.make_clip(sr, seed=3, length=600001)
    kw = _kw(stationary, 1024)
    sentinel = np.float32(1234.5)
    buf, offsets, lengths = _pack(N, [y[:600000], y])
    out = np.full(int((offsets + lengths).max()), sentinel, np.float32)
    r = ctx.gate_batch(buf, offsets, lengths, N.gate_opts(sr, **kw), out=out, out_offsets=offsets, want_mask=True)
    assert list(r["status"]) == [N.CLIP_OK, N.CLIP_TOO_LONG]
    assert np.all(out[offsets[1]:] == sentinel)                       # a failed clip's range is not written
    assert not stationary or r["mask"][1] is None
    dev = out[:600000]
    ref = G.reduce_noise(y[:600000], sr, hard_mask=r["mask"][0] if stationary else None, **kw)
    err = float(np.abs(dev.astype(np.float64) - ref).max() / np.abs(y).max())
    print(f"600000 samples, stationary={stationary}: signal err {err:.3g} (bound {4 * _yard()['sig'][stationary]:.3g})")
    assert err <= 4 * _yard()["sig"][stationary]


@pytest.mark.parametrize("stationary", [True, False])
def test_ragged_batch_with_a_failed_clip_in_the_middle(N, ctx, stationary):
    """a NaN clip gives zeros and its status, an empty clip its status, and neither touches another clip: every other output
    is bit for bit what the clip gives alone; a second run repeats the first bit for bit"""
    sr = 22050
    kw = _kw(stationary, 1024)
    bad = G.make_clip(sr, seed=5, length=5000)
    bad[2500] = np.nan
    clips = [_clips(sr)["plain"][0], bad, G.make_clip(sr, seed=6, length=777), np.zeros(0, np.float32), _clips(sr)["short"][0]]
    outs, r = _gate(N, ctx, clips, sr, kw)
    assert list(r["status"]) == [N.CLIP_OK, N.CLIP_NONFINITE, N.CLIP_OK, N.CLIP_TOO_SHORT, N.CLIP_OK]
    assert not outs[1].any() and outs[1].size == 5000
    for i in (0, 2, 4):
        alone, ra = _gate(N, ctx, [clips[i]], sr, kw)
        assert list(ra["status"]) == [N.CLIP_OK]
        np.testing.assert_array_equal(outs[i], alone[0], err_msg=f"clip {i}")
    again, _ = _gate(N, ctx, clips, sr, kw)
    for a, b in zip(outs, again):
        np.testing.assert_array_equal(a, b)
    if stationary:                                                    # a NaN in the noise clip fails the clip it belongs to
        noise = [G.noise_clip(sr), G.noise_clip(sr, seed=101)]
        noise[0][7] = np.inf
        outs, r = _gate(N, ctx, [clips[0], clips[2]], sr, kw, noise=noise)
        assert list(r["status"]) == [N.CLIP_NONFINITE, N.CLIP_OK] and not outs[0].any() and outs[1].any()


@pytest.mark.parametrize("stationary", [True, False])
def test_zeros_and_no_reduction(N, ctx, stationary):
    sr = 16000
    outs, r = _gate(N, ctx, [np.zeros(3000, np.float32)], sr, _kw(stationary, 1024))
    assert list(r["status"]) == [N.CLIP_OK] and not outs[0].any()
    if not stationary:                                                # p = 0: the mask is 1 exactly, y comes back to rounding
        y = _clips(sr)["plain"][0]
        outs, _ = _gate(N, ctx, [y], sr, dict(stationary=False, prop_decrease=0.0))
        assert np.abs(outs[0] - y).max() / np.abs(y).max() <= 4 * _yard()["sig"][False]


_LAYOUT_LENGTHS = (32000, 700, 5000, 1, 12345)


def _layout_clips(sr=16000):
    return [G.make_clip(sr, seed=20 + i, length=L) for i, L in enumerate(_LAYOUT_LENGTHS)]


def test_input_layouts_equal_the_packed_host_batch(N, ctx):
    """int16 on the host, float32 in device memory (output there too), and clips scattered in reverse order with gaps, all
    bit for bit the packed host float32 batch"""
    sr = 16000
    q = [np.round(c * 32767.0).astype(np.int16) for c in _layout_clips()]
    clips = [(c.astype(np.float32) / np.float32(32768.0)) for c in q]         # what the int16 samples are taken to be
    n = len(clips)
    for stationary in (True, False):
        opts = N.gate_opts(sr, **_kw(stationary, 1024))
        want, r0 = _gate(N, ctx, clips, sr, _kw(stationary, 1024))
        assert list(r0["status"]) == [N.CLIP_OK] * n
        buf16, offsets, lengths = _pack(N, q)
        r = ctx.gate_batch(buf16, offsets, lengths, opts)
        for i in range(n):
            np.testing.assert_array_equal(r["out"][r["offsets"][i]:r["offsets"][i] + lengths[i]], want[i], err_msg=f"int16 {i}")
        # scattered: reverse order, a gap of 37 samples in front of every clip
        soff = np.zeros(n, np.int64)
        pos = 0
        for i in reversed(range(n)):
            soff[i] = pos + 37
            pos = soff[i] + lengths[i]
        sbuf = np.full(pos + 5, 9.0e9, np.float32)
        for i in range(n):
            sbuf[soff[i]:soff[i] + lengths[i]] = clips[i]
        r = ctx.gate_batch(sbuf, soff, lengths, opts)
        for i in range(n):
            np.testing.assert_array_equal(r["out"][r["offsets"][i]:r["offsets"][i] + lengths[i]], want[i], err_msg=f"scattered {i}")
        # device in, device out, at the scattered offsets
        d_in, d_out = N.DeviceBuffer(ctx, sbuf.nbytes), N.DeviceBuffer(ctx, sbuf.nbytes)
        d_in.upload(sbuf)
        d_out.upload(np.full(sbuf.size, 77.0, np.float32))
        r = ctx.gate_batch(d_in, soff, lengths, opts, fmt=N.FMT_F32, out=d_out, out_offsets=soff)
        assert list(r["status"]) == [N.CLIP_OK] * n
        back = np.zeros(sbuf.size, np.float32)
        d_out.download(back)
        keep = np.ones(sbuf.size, bool)
        for i in range(n):
            np.testing.assert_array_equal(back[soff[i]:soff[i] + lengths[i]], want[i], err_msg=f"device {i}")
            keep[soff[i]:soff[i] + lengths[i]] = False
        assert np.all(back[keep] == 77.0)                                 # nothing outside the clips' ranges is written
        d_in.free()
        d_out.free()


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from audio_feature_extraction_amd import _native as N
from tests import test_gpu_gate as T
ctx = N.Context(0)
res = {}
for stationary in (True, False):
    outs, r = T._gate(N, ctx, T._layout_clips(), 16000, T._kw(stationary, 1024), want_thresh=stationary)
    res[f"out{int(stationary)}"] = np.concatenate(outs)
    res[f"status{int(stationary)}"] = r["status"]
    if stationary:
        res["thresh"] = r["thresh"]
np.savez(sys.argv[2], **res)
"""


def test_chunked_equals_unchunked(N, ctx, tmp_path):
    """the same batch cut into chunks by a small workspace budget, in a child process (the budget is read once per process)"""
    budget = 6000000
    for stationary in (True, False):
        cost = N.gate_cost(N.gate_opts(16000, **_kw(stationary, 1024)))
        assert N.stft_chunks(_LAYOUT_LENGTHS, cost, budget).max() + 1 >= 3
        assert N.stft_chunks(_LAYOUT_LENGTHS, cost, 2 << 30).max() == 0
    dst = str(tmp_path / "chunked.npz")
    env = dict(os.environ, AFX_TEST_GATE_BUDGET=str(budget))
    subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _CHILD, ROOT, dst], env=env, check=True, timeout=150)
    z = np.load(dst)
    for stationary in (True, False):
        outs, r = _gate(N, ctx, _layout_clips(), 16000, _kw(stationary, 1024), want_thresh=stationary)
        np.testing.assert_array_equal(z[f"status{int(stationary)}"], r["status"])
        np.testing.assert_array_equal(z[f"out{int(stationary)}"], np.concatenate(outs))
        if stationary:
            np.testing.assert_array_equal(z["thresh"], r["thresh"])


def test_effects_and_extractor_api(N, ctx):
    from audio_feature_extraction_amd import AudioFeatureExtractor, effects
    sr = 16000
    y, noise = _clips(sr)["noise"]
    short = _clips(sr)["short"][0]
    a = effects.reduce_noise(y, sr)
    assert a.dtype == np.float32 and a.shape == y.shape
    np.testing.assert_array_equal(a, _gate(N, ctx, [y], sr, NONSTAT_KW)[0][0])
    b = effects.reduce_noise(y=y, sr=sr, stationary=True, y_noise=noise, prop_decrease=0.95, n_jobs=1, use_tqdm=False)
    np.testing.assert_array_equal(b, _gate(N, ctx, [y], sr, STAT_KW, noise=[noise])[0][0])
    both = effects.reduce_noise_batch([y, short], sr, y_noise=noise, stationary=True, prop_decrease=0.95)
    np.testing.assert_array_equal(both[0], b)
    assert both[1].shape == short.shape
    nan = short.copy()
    nan[3] = np.nan
    assert not effects.reduce_noise(nan, sr).any()
    ex = AudioFeatureExtractor(sr=sr)
    w = ex.apply_noise_reduction(y)                                   # "wiener": stationary, prop_decrease 0.95, 1024 / 256
    np.testing.assert_array_equal(w, effects.reduce_noise(y, sr, stationary=True, prop_decrease=0.95))
    s = ex.apply_noise_reduction(y, method="spectral")                # non-stationary at 2048 / 2048 / 512
    np.testing.assert_array_equal(s, effects.reduce_noise(y, sr, n_fft=2048, win_length=2048, hop_length=512))
    assert not np.array_equal(w, s)
    many = ex.apply_noise_reduction_batch([y, short], method="spectral")
    np.testing.assert_array_equal(many[0], s)
    ref = G.reduce_noise(y, sr, n_fft=2048)
    assert np.abs(s - ref).max() / np.abs(y).max() <= 4 * _yard()["sig"][False]


def test_process_recordings_batch_equals_the_two_calls(N):
    """normalise -> denoise with the samples staying on the device equals the two extractor calls made one after the other,
    bit for bit; the loudness is the normalised signal's, None where the reference's meter raises"""
    from audio_feature_extraction_amd import AudioFeatureExtractor, loudness
    sr = 16000
    ex = AudioFeatureExtractor(sr=sr)
    sigs = [_clips(sr)["plain"][0], _clips(sr)["short"][0], _clips(sr)["silence"][0], np.zeros(8000, np.float32)]
    for method in ("wiener", "spectral"):
        ys, ls = ex.process_recordings_batch(sigs, method=method)
        norm = ex.normalize_volume_batch(sigs)
        want = ex.apply_noise_reduction_batch(norm, method=method)
        for i, (a, b) in enumerate(zip(ys, want)):
            np.testing.assert_array_equal(a, b, err_msg=f"{method} {i}")
        meas = loudness.integrated_loudness_batch(norm, sr)
        assert ls == meas
        assert ls[1] is None and abs(ls[0] + 23.0) < 1e-3 and ls[3] == -np.inf        # 3000 samples: shorter than a block
