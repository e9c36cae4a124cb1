"""GPU tests of afx_pvoc_batch / afx_time_stretch_batch (librosa-style phase_vocoder and effects.time_stretch) and of their
Python front ends against the oracle of tests/pvoc_ref.py.

The vocoder: n_fft 16 (9 bins, less than a wave; a random complex64 array with two zero columns), 1024 and 2048 (the
oracle's float32 stft of tests/stft_ref.make_clip, cut to T columns); rates 1, 0.5, 2, 0.8, 1.25, 3.7 and 1/3; T = 1, 2,
PVOC_TILE - 1, PVOC_TILE, PVOC_TILE + 1 and 81, so that T_out covers 1, 2, the three lengths around a tile and more than two
tiles (asserted).  time_stretch: 1024 / 256 and 2048 / 441, reflect and constant padding, rates 0.8, 1.25 and 2, clips of
9000 .. 9003 samples (round(len / rate) meets its ties at 9002 / 0.8 and at odd lengths / 2).

Tolerances are multiples of what the oracle's device-faithful form (float32 magnitudes, float64 phases) loses against its
float64 form on the same input -- the yardsticks, computed here from the oracle alone, never from the device:
  vocoder       per (n_fft, rate), the largest |P_32 - P_64| / max_b |P_64[b, t]| over the T of the configuration; the device
                must stay within 4 x that against P_64 (a column that is zero in float64 must be zero on the device)
  time_stretch  per (n_fft, hop, pad_mode, rate), the largest |x_32 - x_64| / max |y| of the float32-form composition against
                the float64 one; the device within 4 x that against x_64
The clips have noise in every bin: a bin that is silent at first carries an arbitrary phase forward (the angle of a rounding
residue), on which the float32 and float64 forms disagree at order 1 as soon as the bin sounds -- nothing a tolerance can
measure.  Each test prints yardstick -> bound; device, and DESIGN.md section 27 has the table.
Measured 2026-10-21 on an MI355X, over the printed lines (yardstick -> bound; device):
  vocoder       16 / 4: 1.09e-7 .. 1.65e-7 -> 4.4e-7 .. 6.6e-7; 1024 / 256: 8.1e-8 .. 1.61e-7 -> 3.2e-7 .. 6.4e-7; 2048 / 512:
                9.7e-8 .. 1.78e-7 -> 3.9e-7 .. 7.1e-7; the device prints the yardstick's own three digits in all 21 lines
  rate 1        against D itself: 1.05e-7 .. 1.17e-7 -> 4.2e-7 .. 4.7e-7; device the same three digits
  time_stretch  1024 / 256 reflect 1.6e-6 .. 4.3e-6 -> 6.4e-6 .. 1.7e-5, device 2.2e-6 .. 4.4e-6; constant 1.2e-6 .. 1.5e-6 ->
                4.8e-6 .. 6.0e-6, device 2.2e-6 .. 2.8e-6 (at most 1.9 x its yardstick, rate 2); 2048 / 441 reflect
                1.06e-6 .. 3.2e-6 -> 4.2e-6 .. 1.3e-5, device 1.09e-6 .. 2.6e-6; constant 8.4e-7 .. 1.96e-6 -> 3.4e-6 .. 7.9e-6,
                device 7.8e-7 .. 1.54e-6
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import pvoc_ref as P
from tests import stft_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY64 = np.finfo(np.float64).tiny
RATES = (1.0, 0.5, 2.0, 0.8, 1.25, 3.7, 1.0 / 3.0)
SHAPES = ((16, 4), (1024, 256), (2048, 512))


@pytest.fixture(scope="module")
def N():
    from audio_feature_extraction_amd import _native
    if _native.device_count() < 1:
        pytest.fail("no GPU visible")
    return _native


@pytest.fixture(scope="module")
def ctx(N):
    return N.Context(0)


@functools.lru_cache(maxsize=None)
def _spectrum(n, hop, seed=0):
    """[bins, 81] complex64, read-only: random with two zero columns at n_fft 16, else the oracle's float32 stft of make_clip"""
    if n == 16:
        rng = np.random.default_rng(seed + 16)
        D = (rng.standard_normal((9, 81)) + 1j * rng.standard_normal((9, 81))).astype(np.complex64)
        D[:, 11] = 0
        D[:, 12] = 0
    else:
        D = np.ascontiguousarray(R.stft(R.make_clip(80 * hop, seed=seed + n), n, hop, f32=True))
    assert D.shape == (n // 2 + 1, 81) and D.dtype == np.complex64
    D.setflags(write=False)
    return D


def _pvoc(N, ctx, specs, rates, n, hop, **kw):
    """specs: [bins, T] arrays -> the result of Context.pvoc_batch from packed host memory"""
    bins = n // 2 + 1
    frames = np.array([D.shape[1] for D in specs], np.int64)
    offsets = N.packed_offsets(frames * bins)
    buf = np.zeros(max(int(frames.sum()) * bins, 1), np.complex64)
    for o, D in zip(offsets, specs):
        buf[o:o + D.size] = np.asarray(D, np.complex64).ravel(order="F")
    return ctx.pvoc_batch(buf, offsets, frames, rates, n, hop, **kw)


def _rel(A, B):
    """largest |A - B| / max_b |B[b, t]|; a column that is zero in B must be zero in A"""
    top = np.abs(B).max(axis=0, keepdims=True)
    err = np.abs(A - B)
    assert not err[:, top[0] == 0].any()
    return float((err / np.maximum(top, TINY64)).max())


def _Ts(N):
    return (1, 2, N.PVOC_TILE - 1, N.PVOC_TILE, N.PVOC_TILE + 1, 81)


@pytest.mark.parametrize("n,hop", SHAPES)
def test_vocoder_against_the_oracle(N, ctx, n, hop):
    D = _spectrum(n, hop)
    Ts = _Ts(N)
    specs = [D[:, :T] for _ in RATES for T in Ts]
    rates = [r for r in RATES for _ in Ts]
    res = _pvoc(N, ctx, specs, rates, n, hop)                        # one call: 42 clips, every one with its own rate
    assert list(res["status"]) == [N.CLIP_OK] * len(specs)
    seen = set()
    k = 0
    for rate in RATES:
        yard = dev = 0.0
        for T in Ts:
            got = res["spec"][k]
            k += 1
            P64 = P.phase_vocoder(D[:, :T], rate=rate, hop_length=hop, n_fft=n, exact=True)
            assert got.shape == P64.shape and got.dtype == np.complex64 and got.flags.f_contiguous
            seen.add(got.shape[1])
            yard = max(yard, _rel(P.phase_vocoder(D[:, :T], rate=rate, hop_length=hop, n_fft=n, f32=True), P64))
            dev = max(dev, _rel(got, P64))
        print(f"pvoc {n}/{hop} rate {rate:.4g}: yardstick {yard:.3g} -> bound {4 * yard:.3g}; device {dev:.3g}")
        assert yard > 0 and dev <= 4 * yard, f"{n}/{hop} rate {rate}: device {dev:.3g}, yardstick {yard:.3g}"
    tile = N.PVOC_TILE
    assert {1, 2, tile - 1, tile, tile + 1} <= seen and max(seen) > 2 * tile, sorted(seen)
    if n == 16:                                                      # steps 22 .. 24 at rate 0.5 mix the zero columns only
        assert not res["spec"][1 * len(Ts) + 5][:, 22:25].any()


@pytest.mark.parametrize("n,hop", SHAPES)
def test_rate_one_returns_the_input(N, ctx, n, hop):
    D = _spectrum(n, hop, seed=1)
    got = _pvoc(N, ctx, [D], [1.0], n, hop)["spec"][0]
    P64 = P.phase_vocoder(D, rate=1.0, hop_length=hop, n_fft=n, exact=True)
    yard = _rel(P.phase_vocoder(D, rate=1.0, hop_length=hop, n_fft=n, f32=True), P64)
    dev = _rel(got, D.astype(np.complex128))
    print(f"pvoc {n}/{hop} rate 1 against D: yardstick {yard:.3g} -> bound {4 * yard:.3g}; device {dev:.3g}")
    assert got.shape == D.shape and yard > 0 and dev <= 4 * yard


# ---- the ragged batch ------------------------------------------------------------------------------------------------------
_BATCH = ((16, 4), (2048, 512))
_BATCH_T = (40, 0, 33, 7, 64, 81, 2)
_BATCH_RATES = (0.8, 1.0, 1.25, 3.7, 0.5, 1.0 / 3.0, 2.0)
_BATCH_NAN = 2
_BATCH_GOOD = (0, 3, 4, 5, 6)


def _batch_specs(n, hop):
    """seven spectra, ragged: one without frames, one with a NaN bin in the middle of the batch"""
    specs = [np.array(_batch_columns(n, hop, i)) for i in range(len(_BATCH_T))]
    specs[_BATCH_NAN][n // 4, 17] = complex(0.5, np.nan)
    return specs


def _batch_columns(n, hop, i):
    T = _BATCH_T[i]
    a = i % 3 if T + i % 3 <= 81 else 0
    return _spectrum(n, hop, seed=2)[:, a:a + T]


def _batch_run(N, ctx, n, hop):
    return _pvoc(N, ctx, _batch_specs(n, hop), _BATCH_RATES, n, hop)


_STRETCH = (1024, 256, "reflect")
_STRETCH_RATES = (0.8, 1.25, 2.0, 0.5, 1.25)


def _stretch_clips():
    """five clips: a NaN sample in the second, the third too short for reflect padding"""
    clips = [R.make_clip(L, seed=20 + i) for i, L in enumerate((9000, 9001, 512, 40000, 9003))]
    clips[1][4000] = np.nan
    return clips


def _pack(N, clips):
    lengths = np.array([c.size for c in clips], np.int64)
    offsets = N.packed_offsets(lengths, 4)
    buf = np.zeros(max(int((offsets + lengths).max()), 1), np.float32)
    for o, c in zip(offsets, clips):
        buf[o:o + c.size] = c
    return buf, offsets, lengths


def _stretch_run(N, ctx):
    n, hop, pad = _STRETCH
    buf, offsets, lengths = _pack(N, _stretch_clips())
    r = ctx.time_stretch_batch(buf, offsets, lengths, _STRETCH_RATES, N.stft_opts(n, hop, True, pad),
                               R.get_window("hann", n, n).astype(np.float32))
    return [r["out"][o:o + m] for o, m in zip(r["offsets"], r["samples"])], r["status"]


@pytest.mark.parametrize("n,hop", _BATCH)
def test_ragged_batch_layouts_and_order_are_bit_identical(N, ctx, n, hop):
    bins = n // 2 + 1
    specs = _batch_specs(n, hop)
    m = len(specs)
    res = _batch_run(N, ctx, n, hop)
    want_status = [N.CLIP_OK] * m
    want_status[1], want_status[_BATCH_NAN] = N.CLIP_TOO_SHORT, N.CLIP_NONFINITE
    assert list(res["status"]) == want_status
    assert list(res["frames"]) == [P.steps(T, r)[0] if T else 0 for T, r in zip(_BATCH_T, _BATCH_RATES)]
    assert res["spec"][1] is None and res["spec"][_BATCH_NAN] is None
    o, T = res["offsets"][_BATCH_NAN], res["frames"][_BATCH_NAN]
    assert T > 0 and not res["out"][o:o + T * bins].any()            # the NaN clip: zeros
    spec = res["spec"]
    clean = list(specs)                                              # the NaN clip's neighbours are what they are without it
    clean[_BATCH_NAN] = np.array(_batch_columns(n, hop, _BATCH_NAN))
    r = _pvoc(N, ctx, clean, _BATCH_RATES, n, hop)
    assert r["status"][_BATCH_NAN] == N.CLIP_OK
    for i in _BATCH_GOOD:
        np.testing.assert_array_equal(r["spec"][i], spec[i], err_msg=f"clean {i}")
    for i in _BATCH_GOOD:                                            # alone
        r = _pvoc(N, ctx, [specs[i]], [_BATCH_RATES[i]], n, hop)
        np.testing.assert_array_equal(r["spec"][0], spec[i], err_msg=f"alone {i}")
    order = [4, 2, 6, 0, 1, 5, 3]                                     # another order
    r = _pvoc(N, ctx, [specs[i] for i in order], [_BATCH_RATES[i] for i in order], n, hop)
    for k, i in enumerate(order):
        assert r["status"][k] == want_status[i]
        if i in _BATCH_GOOD:
            np.testing.assert_array_equal(r["spec"][k], spec[i], err_msg=f"order {i}")
    # device in, device out, scattered with gaps in reverse order; nothing outside the rows is written
    frames_in, frames = np.array(_BATCH_T, np.int64), res["frames"]
    soff, pos = np.zeros(m, np.int64), 0
    for i in reversed(range(m)):
        soff[i] = pos + 5
        pos = soff[i] + frames_in[i] * bins
    sbuf = np.full(pos + 3, 9.0e9, np.complex64)
    for i in range(m):
        sbuf[soff[i]:soff[i] + specs[i].size] = specs[i].ravel(order="F")
    ooff, opos = np.zeros(m, np.int64), 0
    for i in reversed(range(m)):
        ooff[i] = opos + 3
        opos = ooff[i] + frames[i] * bins
    d_in, d_out = N.DeviceBuffer(ctx, sbuf.nbytes), N.DeviceBuffer(ctx, 8 * (opos + 2))
    d_in.upload(sbuf)
    d_out.upload(np.full(opos + 2, 77.0, np.complex64))
    r = ctx.pvoc_batch(d_in, soff, frames_in, _BATCH_RATES, n, hop, out=d_out, out_offsets=ooff)
    assert list(r["status"]) == want_status and "spec" not in r
    back = np.zeros(opos + 2, np.complex64)
    d_out.download(back)
    keep = np.ones(back.size, bool)
    for i in range(m):
        rows = back[ooff[i]:ooff[i] + frames[i] * bins]
        keep[ooff[i]:ooff[i] + frames[i] * bins] = False
        if i in _BATCH_GOOD:
            np.testing.assert_array_equal(rows.reshape(frames[i], bins).T, spec[i], err_msg=f"device {i}")
    assert not back[ooff[_BATCH_NAN]:ooff[_BATCH_NAN] + frames[_BATCH_NAN] * bins].any()
    assert np.all(back[keep] == 77.0)
    d_in.free()
    d_out.free()
    again = _batch_run(N, ctx, n, hop)                               # a second run repeats the first bit for bit
    for i in _BATCH_GOOD:
        np.testing.assert_array_equal(again["spec"][i], spec[i])


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from audio_feature_extraction_amd import _native as N
from tests import test_gpu_pvoc as T
ctx = N.Context(0)
res = {}
for n, hop in T._BATCH:
    r = T._batch_run(N, ctx, n, hop)
    for i in T._BATCH_GOOD:
        res[f"spec{n}_{i}"] = np.ascontiguousarray(r["spec"][i])
    res[f"status{n}"] = r["status"]
outs, status = T._stretch_run(N, ctx)
for i, x in enumerate(outs):
    res[f"sig{i}"] = x
res["sig_status"] = status
np.savez(sys.argv[2], **res)
"""


def test_chunked_equals_unchunked(N, ctx, tmp_path):
    """the ragged batches cut into chunks by a small workspace budget, in a child process (the budget is read once per process)"""
    budget = 4000000
    n, hop = _BATCH[1]
    w = [T + N.pvoc_frames(n, hop, T, r)[0] if T else 0 for T, r in zip(_BATCH_T, _BATCH_RATES)]
    assert N.stft_chunks(w, N.pvoc_cost(n), budget).max() + 1 >= 3
    assert N.stft_chunks(w, N.pvoc_cost(n), 2 << 30).max() == 0
    sn, shop, pad = _STRETCH
    o = N.stft_opts(sn, shop, True, pad)
    w = []
    for c, r in zip(_stretch_clips(), _STRETCH_RATES):
        T, T_out, n_out, st = N.time_stretch_samples(o, c.size, r)
        w.append(T + T_out + -(-c.size // shop) + -(-n_out // shop) if st == N.CLIP_OK else 0)
    assert N.stft_chunks(w, N.time_stretch_cost(o), budget).max() + 1 >= 3
    assert N.stft_chunks(w, N.time_stretch_cost(o), 2 << 30).max() == 0
    dst = str(tmp_path / "chunked.npz")
    env = dict(os.environ, AFX_TEST_STFT_BUDGET=str(budget))
    subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _CHILD, ROOT, dst], env=env, check=True, timeout=150)
    z = np.load(dst)
    for n, hop in _BATCH:
        r = _batch_run(N, ctx, n, hop)
        np.testing.assert_array_equal(z[f"status{n}"], r["status"])
        for i in _BATCH_GOOD:
            np.testing.assert_array_equal(z[f"spec{n}_{i}"], r["spec"][i])
    outs, status = _stretch_run(N, ctx)
    np.testing.assert_array_equal(z["sig_status"], status)
    assert list(status) == [N.CLIP_OK, N.CLIP_NONFINITE, N.CLIP_TOO_SHORT, N.CLIP_OK, N.CLIP_OK]
    for i in (0, 3, 4):
        np.testing.assert_array_equal(z[f"sig{i}"], outs[i])
    assert not outs[1].any() and outs[1].size == round(9001 / 1.25)   # the NaN clip: zeros


# ---- time_stretch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,hop", [(1024, 256), (2048, 441)])
@pytest.mark.parametrize("pad_mode", ["reflect", "constant"])
def test_time_stretch_fused_against_the_three_calls_and_the_oracle(N, ctx, n, hop, pad_mode):
    import audio_feature_extraction_amd as pkg
    from audio_feature_extraction_amd import effects
    clips = [R.make_clip(L, seed=40 + L) for L in (9000, 9001, 9002, 9003)]
    kw = dict(n_fft=n, hop_length=hop, pad_mode=pad_mode)
    ties = 0
    for rate in (0.8, 1.25, 2.0):
        fused = effects.time_stretch_batch(clips, rate, **kw)
        yard = dev = 0.0
        for y, x in zip(clips, fused):
            L_out = round(y.size / rate)
            ties += (y.size / rate) % 1 == 0.5
            assert x.dtype == np.float32 and x.size == L_out
            D = pkg.stft(y, **kw)                                     # the three public calls, the spectra going home
            three = pkg.istft(pkg.phase_vocoder(D, rate=rate, hop_length=hop, n_fft=n), hop_length=hop, n_fft=n, length=L_out)
            np.testing.assert_array_equal(x, three, err_msg=f"{n}/{hop}/{pad_mode} rate {rate} len {y.size}")
            x64 = P.time_stretch(y, rate=rate, **kw)
            top = float(np.abs(y).max())
            yard = max(yard, float(np.abs(P.time_stretch(y, rate=rate, f32=True, **kw) - x64).max()) / top)
            dev = max(dev, float(np.abs(x.astype(np.float64) - x64).max()) / top)
        print(f"time_stretch {n}/{hop}/{pad_mode} rate {rate}: yardstick {yard:.3g} -> bound {4 * yard:.3g}; device {dev:.3g}")
        assert yard > 0 and dev <= 4 * yard
    assert ties >= 2                                                 # 9002 / 0.8, and the odd lengths / 2
    np.testing.assert_array_equal(effects.time_stretch(clips[0], rate=0.8, **kw), effects.time_stretch_batch(clips[:1], [0.8], **kw)[0])


def test_time_stretch_front_end(N, ctx):
    import audio_feature_extraction_amd as pkg
    from audio_feature_extraction_amd import effects
    y = R.make_clip(9000, seed=7)
    y2 = effects.time_stretch(y, rate=0.8)                            # the README's line
    assert y2.dtype == np.float32 and y2.size == 11250 and np.all(np.isfinite(y2))
    q = np.round(y * 32767.0).astype(np.int16)
    np.testing.assert_array_equal(effects.time_stretch(q, rate=1.25), effects.time_stretch(q.astype(np.float32) / np.float32(32768.0), rate=1.25))
    bad = y.copy()
    bad[77] = np.inf
    for clip, kw in ((bad, {}), (y[:0], {}), (y[:1024], dict(pad_mode="reflect"))):   # n_fft / 2 samples under reflect padding
        with pytest.raises(ValueError):
            effects.time_stretch(clip, rate=0.8, **kw)
    many = effects.time_stretch_batch([y, bad, y[:1024], y[:3000]], [0.8, 0.8, 2.0, 1.25], pad_mode="reflect")
    assert many[1] is None and many[2] is None and many[3].size == 2400
    np.testing.assert_array_equal(many[0], effects.time_stretch(y, rate=0.8, pad_mode="reflect"))
    assert effects.time_stretch(y[:1], rate=3.0).size == 0           # round(1 / 3) = 0 samples: nothing to write
    D = pkg.stft(y)
    with pytest.raises(ValueError):
        pkg.phase_vocoder(D[:, :0], rate=1.0)
    Dn = D.copy()
    Dn[3, 3] = np.nan
    with pytest.raises(ValueError):
        pkg.phase_vocoder(Dn, rate=1.0)
    from audio_feature_extraction_amd.core import spectrum as S
    both = S.phase_vocoder_batch([D, Dn, D[:, :5]], 2.0)
    assert both[1] is None and both[2].shape == (1025, 3)
    np.testing.assert_array_equal(both[0], pkg.phase_vocoder(np.ascontiguousarray(D), rate=2.0))


def test_stretch_to_length_is_exact(N, ctx):
    import audio_feature_extraction_amd as pkg
    ex = pkg.AudioFeatureExtractor()
    y = R.make_clip(9000, seed=8)
    for n in (9000, 7001, 11113, 4500, 18001, 1):
        x = ex.stretch_to_length(y, n)
        assert x.dtype == np.float32 and x.size == n and np.all(np.isfinite(x)), n
    outs = ex.stretch_to_length_batch([y, y[:5000], y[:0]], [8000, 8000, 8000])
    assert outs[0].size == 8000 and outs[1].size == 8000 and outs[2] is None
    np.testing.assert_array_equal(outs[0], ex.stretch_to_length(y, 8000))
