"""GPU tests of afx_stft_batch / afx_istft_batch (librosa-style stft / istft at n_fft 1024 and 2048) and of
audio_feature_extraction_amd.core.spectrum against the oracle of tests/stft_ref.py.

The grid: n_fft 1024 and 2048; hop n/4, n/2, n, 160, 441, n/16; the windows hann, hamming, boxcar, an array and hann of
win_length 400; center on (constant and reflect padding) and off.  The clips are short (tests/stft_ref.make_clip): with
center 1, n/2, n/2 + 1, n - 1, n, n + 1, 3 hop - 1, 3 hop, 3 hop + 1, 4 hop (an odd frame count) and 5 hop (an even one);
without it n - 1, n, n + hop - 1, n + hop, n + 2 hop.  Every clip is either compared or has the status the oracle predicts.

Tolerances are multiples of what the oracle's float32-faithful form (f32=True) loses against its float64 form on these same
clips -- the yardsticks, computed here from the oracle alone, never from the device:
  spectrum   per configuration, the largest |D_32 - D_64| / max_b |D_64[b, t]| over the configuration's clips and frames; the
             device must stay within 4 x that against D_64 (a frame that is zero in float64 must be zero on the device)
  kinds      the same with | |D_32| - |D_64| | and, relative to max_b |D_64|^2, | |D_32|^2 - |D_64|^2 |
  istft      on the float64 spectra rounded to complex64, per configuration, the largest |x_32 - x_64| / max |y| over the
             configuration's clips and lengths; the device within 4 x that against x_64
  round trip 4 x the error of the float32 form's own istft(stft(y)) against y, relative to max |y|
Measured 2026-10-21 on an MI355X; each test prints, per (n_fft, hop), the configuration that came closest to its bound
(yardstick -> bound; device), and DESIGN.md section 26 has the table.  Over those lines:
  spectrum   5.9e-8 .. 1.15e-7 -> 2.4e-7 .. 4.6e-7; device 8.2e-8 .. 2.0e-7, at most 2.2 x its yardstick (1024 / 441, array window)
  kinds      |D| 8.2e-8 .. 2.0e-7 -> 3.3e-7 .. 8.2e-7, device 6.0e-8 .. 1.8e-7; |D|^2 1.5e-7 .. 4.1e-7 -> 6.0e-7 .. 1.6e-6, device
             1.2e-7 .. 3.2e-7
  istft      1024 / 160 (hamming): 9.5e-7 -> 3.8e-6, device 1.1e-6.  Everywhere else a Hann window was closest (hann, or hann
             of 400): it reaches wss of a few 1e-6 beside the samples where it is zero, and acc / wss magnifies the transform's
             rounding there in the float32 form and on the device alike: 2.1e-4 .. 5.3e-3 -> 8.6e-4 .. 2.1e-2, device
             2.9e-4 .. 7.6e-3, at most 2.6 x its yardstick (1024 / 512, hann).  Hann at hop n: 5.1e-3 / 2.2e-2, device 5.7e-3 / 1.4e-2
  round trip 2.5e-7 -> 9.9e-7, device 2.5e-7
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import stft_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY64 = np.finfo(np.float64).tiny
PADS = [(True, "constant"), (True, "reflect"), (False, "constant")]


@pytest.fixture(scope="module")
def N():
    from audio_feature_extraction_amd import _native
    if _native.device_count() < 1:
        pytest.fail("no GPU visible")
    return _native


@pytest.fixture(scope="module")
def ctx(N):
    return N.Context(0)


def _hops(n):
    return [n // 4, n // 2, n, 160, 441, n // 16]


@functools.lru_cache(maxsize=None)
def _array_window(n):
    rng = np.random.default_rng(n)
    w = (0.2 + rng.random(n)).astype(np.float32)
    w.setflags(write=False)
    return w


def _windows(n):
    """name -> (window, win_length)"""
    return {"hann": ("hann", n), "hamming": ("hamming", n), "boxcar": ("boxcar", n), "array": (_array_window(n), n),
            "hann400": ("hann", 400)}


def _table(n, window, win_length):
    return R.get_window(window, win_length, n).astype(np.float32)


def _lengths(n, hop, center):
    if center:
        ls = [1, n // 2, n // 2 + 1, n - 1, n, n + 1, 3 * hop - 1, 3 * hop, 3 * hop + 1, 4 * hop, 5 * hop]
    else:
        ls = [n - 1, n, n + hop - 1, n + hop, n + 2 * hop]
    return sorted(set(ls))


@functools.lru_cache(maxsize=None)
def _clip(length, seed=0):
    y = R.make_clip(length, seed=seed + length)
    y.setflags(write=False)
    return y


def _pack(N, clips):
    lengths = np.array([c.size for c in clips], np.int64)
    offsets = N.packed_offsets(lengths, 4)
    buf = np.zeros(max(int((offsets + lengths).max()), 1) if len(clips) else 1, clips[0].dtype)
    for o, c in zip(offsets, clips):
        buf[o:o + c.size] = c
    return buf, offsets, lengths


def _stft(N, ctx, clips, n, hop, table, center=True, pad_mode="constant", kind=0):
    buf, offsets, lengths = _pack(N, clips)
    return ctx.stft_batch(buf, offsets, lengths, N.stft_opts(n, hop, center, pad_mode, kind), table)


def _istft(N, ctx, specs, n, hop, table, center=True, lengths=None):
    """specs: [bins, T] arrays -> list of float32 outputs (None for a failed clip), result"""
    bins = n // 2 + 1
    frames = np.array([D.shape[1] for D in specs], np.int64)
    offsets = N.packed_offsets(frames * bins)
    buf = np.zeros(max(int(frames.sum()) * bins, 1), np.complex64)
    for o, D in zip(offsets, specs):
        buf[o:o + D.size] = np.asarray(D, np.complex64).ravel(order="F")
    want = None if lengths is None else np.array([-1 if l is None else l for l in lengths], np.int64)
    r = ctx.istft_batch(buf, offsets, frames, N.stft_opts(n, hop, center), table, lengths=want)
    return [r["out"][o:o + m] if st == N.CLIP_OK else None for o, m, st in zip(r["offsets"], r["samples"], r["status"])], r


def _rel(D, D64):
    """largest |D - D64| / max_b |D64[b, t]|; a frame that is zero in float64 must be zero in D"""
    top = np.abs(D64).max(axis=0, keepdims=True)
    err = np.abs(D - D64)
    assert not err[:, top[0] == 0].any()
    return float((err / np.maximum(top, TINY64)).max())


@pytest.mark.parametrize("n", [1024, 2048])
@pytest.mark.parametrize("hop_i", range(6))
def test_spectrum_against_the_oracle(N, ctx, n, hop_i):
    hop = _hops(n)[hop_i]
    worst = (0.0, 0.0, "")
    for center, pad_mode in PADS:
        clips = [_clip(L) for L in _lengths(n, hop, center)]
        for name, (window, win_length) in _windows(n).items():
            kw = dict(n_fft=n, hop_length=hop, win_length=win_length, window=window, center=center, pad_mode=pad_mode)
            r = _stft(N, ctx, clips, n, hop, _table(n, window, win_length), center, pad_mode)
            yard, dev, compared = 0.0, 0.0, 0
            for y, D, T, st in zip(clips, r["spec"], r["frames"], r["status"]):
                want_T = R.n_frames(y.size, n, hop, center, pad_mode)
                if want_T is None:
                    assert st == N.CLIP_TOO_SHORT and T == 0 and D is None, (kw, y.size)
                    continue
                assert st == N.CLIP_OK and T == want_T, (kw, y.size)
                D64 = R.stft(y, **kw)
                assert D.shape == D64.shape and D.dtype == np.complex64 and D.flags.f_contiguous
                yard = max(yard, _rel(R.stft(y, f32=True, **kw), D64))
                dev = max(dev, _rel(D, D64))
                compared += 1
            assert compared >= 4 and yard > 0
            assert dev <= 4 * yard, f"{n}/{hop}/{name}/{center}/{pad_mode}: device {dev:.3g}, yardstick {yard:.3g}"
            if dev / yard > worst[0] / max(worst[1], 1e-30) or worst[1] == 0:
                worst = (dev, yard, f"{name}/{center}/{pad_mode}")
    print(f"stft {n}/{hop}: closest to its bound {worst[2]}: device {worst[0]:.3g}, yardstick {worst[1]:.3g} -> bound {4 * worst[1]:.3g}")


@pytest.mark.parametrize("n", [1024, 2048])
def test_magnitude_and_power_kinds(N, ctx, n):
    for hop in (n // 4, 441):
        for center, pad_mode in PADS:
            clips = [_clip(L) for L in _lengths(n, hop, center)]
            ok = [y for y in clips if R.n_frames(y.size, n, hop, center, pad_mode) is not None]
            kw = dict(n_fft=n, hop_length=hop, center=center, pad_mode=pad_mode)
            D64 = [R.stft(y, **kw) for y in ok]
            D32 = [R.stft(y, f32=True, **kw) for y in ok]
            for kind, p in ((N.STFT_MAG, 1), (N.STFT_POWER, 2)):
                r = _stft(N, ctx, ok, n, hop, _table(n, "hann", n), center, pad_mode, kind)
                assert list(r["status"]) == [N.CLIP_OK] * len(ok)
                yard = dev = 0.0
                for S, a, b in zip(r["spec"], D64, D32):
                    assert S.dtype == np.float32 and S.shape == a.shape and S.flags.f_contiguous
                    top = np.maximum(np.abs(a).max(axis=0, keepdims=True) ** p, TINY64)
                    yard = max(yard, float((np.abs(np.abs(b).astype(np.float64) ** p - np.abs(a) ** p) / top).max()))
                    dev = max(dev, float((np.abs(S.astype(np.float64) - np.abs(a) ** p) / top).max()))
                print(f"kind {kind} {n}/{hop}/{center}/{pad_mode}: device {dev:.3g}, yardstick {yard:.3g} -> bound {4 * yard:.3g}")
                assert dev <= 4 * yard


def _spectra(n, hop, window, win_length, center):
    """the oracle's float64 spectra of a few clips of the grid, rounded to complex64, with the clips they came from"""
    ls = _lengths(n, hop, center)
    pick = [ls[0], ls[len(ls) // 2], ls[-2], ls[-1]] if center else ls[1:]
    clips = [_clip(L) for L in sorted(set(pick))]
    return clips, [R.stft(y, n, hop, win_length, window, center).astype(np.complex64) for y in clips]


@pytest.mark.parametrize("n", [1024, 2048])
@pytest.mark.parametrize("hop_i", range(6))
def test_istft_against_the_oracle(N, ctx, n, hop_i):
    hop = _hops(n)[hop_i]
    worst = (0.0, 0.0, "")
    for center in (True, False):
        s = n // 2 if center else 0
        for name, (window, win_length) in _windows(n).items():
            clips, specs = _spectra(n, hop, window, win_length, center)
            table = _table(n, window, win_length)
            kw = dict(hop_length=hop, win_length=win_length, window=window, center=center)
            yard = dev = 0.0
            for mode in ("none", "shorter", "longer"):
                fulls = [n + hop * (D.shape[1] - 1) for D in specs]
                if mode == "none":
                    lengths = [None] * len(specs)
                elif mode == "shorter":
                    lengths = [max((f - 2 * s) // 2, 1) for f in fulls]
                else:
                    lengths = [f - 2 * s + n + 77 for f in fulls]
                outs, r = _istft(N, ctx, specs, n, hop, table, center, lengths)
                assert list(r["status"]) == [N.CLIP_OK] * len(specs)
                for y, D, L, x in zip(clips, specs, lengths, outs):
                    x64 = R.istft(D, length=L, **kw)
                    x32 = R.istft(D, length=L, f32=True, **kw)
                    assert x.dtype == np.float32 and x.shape == x64.shape, (name, mode, y.size)
                    if x.size == 0:
                        continue
                    top = float(np.abs(y).max())
                    yard = max(yard, float(np.abs(x32 - x64).max()) / top)
                    dev = max(dev, float(np.abs(x.astype(np.float64) - x64).max()) / top)
                    if mode == "longer":
                        assert not x[max(n + hop * (D.shape[1] - 1) - s, 0):].any()
            assert yard > 0
            assert dev <= 4 * yard, f"{n}/{hop}/{name}/{center}: device {dev:.3g}, yardstick {yard:.3g}"
            if worst[1] == 0 or dev / yard > worst[0] / worst[1]:
                worst = (dev, yard, f"{name}/{center}")
    print(f"istft {n}/{hop}: closest to its bound {worst[2]}: device {worst[0]:.3g}, yardstick {worst[1]:.3g} -> bound {4 * worst[1]:.3g}")


@pytest.mark.parametrize("n", [1024, 2048])
def test_istft_of_one_frame_and_of_hann_at_hop_n(N, ctx, n):
    y = _clip(4 * n)
    table = _table(n, "hann", n)
    D = R.stft(y, n, n).astype(np.complex64)                       # hann at hop = n_fft: wss = 0 where the frames join
    (x,), r = _istft(N, ctx, [D], n, n, table, True, [y.size])
    x64, x32 = R.istft(D, n, length=y.size), R.istft(D, n, length=y.size, f32=True)
    assert np.all(np.isfinite(x)) and not x[np.arange(n // 2, y.size, n)].any()
    yard = float(np.abs(x32 - x64).max()) / float(np.abs(y).max())
    dev = float(np.abs(x - x64).max()) / float(np.abs(y).max())
    print(f"hann at hop n, {n}: device {dev:.3g}, yardstick {yard:.3g} -> bound {4 * yard:.3g}")
    assert dev <= 4 * yard
    for center in (True, False):                                   # T = 1
        D1 = D[:, :1]
        outs, r = _istft(N, ctx, [D1, D1], n, n // 4, table, center, [None, 700])
        assert list(r["status"]) == [N.CLIP_OK] * 2 and list(r["samples"]) == [0 if center else n, 700]
        for xo, L in zip(outs, (None, 700)):
            ref = R.istft(D1, n // 4, center=center, length=L)
            assert xo.shape == ref.shape
            if xo.size:
                bound = 4 * float(np.abs(R.istft(D1, n // 4, center=center, length=L, f32=True) - ref).max())
                assert float(np.abs(xo - ref).max()) <= bound
    outs, r = _istft(N, ctx, [D[:, :0], D], n, n, table)            # no frames: its status, and the neighbour untouched
    assert list(r["status"]) == [N.CLIP_TOO_SHORT, N.CLIP_OK] and outs[0] is None
    np.testing.assert_array_equal(outs[1], _istft(N, ctx, [D], n, n, table)[0][0])


@pytest.mark.parametrize("n", [1024, 2048])
def test_a_nan_frame_reaches_only_its_own_samples(N, ctx, n):
    hop = n // 4
    y = _clip(12 * hop)
    table = _table(n, "hann", n)
    D = R.stft(y, n, hop).astype(np.complex64)
    x64 = R.istft(D, hop)
    bound = 4 * float(np.abs(R.istft(D, hop, f32=True) - x64).max())
    for t0, b in ((4, 17), (7, 0), (D.shape[1] - 1, n // 2)):       # an even and an odd frame (the pair packing at 1024), the last
        Dn = D.copy()
        Dn[b, t0] = complex(np.nan, 0.0 if b in (0, n // 2) else np.nan)
        (x,), r = _istft(N, ctx, [Dn], n, hop, table)
        m = np.arange(x.size) + n // 2
        covered = (m >= t0 * hop) & (m < t0 * hop + n)
        assert np.array_equal(np.isnan(R.istft(Dn, hop)), covered)  # what the oracle predicts
        assert np.array_equal(np.isnan(x), covered), t0
        # (not bit for bit the clean run: at 1024 the frame packed with t0 is transformed beside zeros instead)
        assert float(np.abs(x[~covered] - x64[~covered]).max()) <= bound, t0
    Dn = D.copy()
    Dn[0, 3] = complex(1.0, np.nan)                                # the imaginary parts of bins 0 and n / 2 are ignored
    Dn[n // 2, 4] = complex(Dn[n // 2, 4].real, np.inf)
    (x,), _ = _istft(N, ctx, [Dn], n, hop, table)
    assert np.all(np.isfinite(x))
    ref = D.copy()
    ref[0, 3] = 1.0
    np.testing.assert_array_equal(x, _istft(N, ctx, [ref], n, hop, table)[0][0])


_BATCH = ((1024, 256), (2048, 441))


def _batch_clips(n):
    """five clips, ragged: a NaN clip and a clip too short for reflect padding in the middle; int16-exact values"""
    q = [np.round(_clip(L, seed=9) * 32767.0).astype(np.int16) for L in (3 * n + 5, 2000 + n, n // 2, 7 * n // 4, n + 1)]
    clips = [c.astype(np.float32) / np.float32(32768.0) for c in q]
    clips[1][n] = np.nan
    return q, clips


def _batch_run(N, ctx, n, hop):
    """forward (reflect) and inverse of the batch from packed host memory -> (spectra, frames, status, signals)"""
    _, clips = _batch_clips(n)
    table = _table(n, "hann", n)
    r = _stft(N, ctx, clips, n, hop, table, True, "reflect")
    specs = [D if D is not None else np.zeros((n // 2 + 1, 0), np.complex64) for D in r["spec"]]
    outs, ri = _istft(N, ctx, specs, n, hop, table, True, [c.size for c in clips])
    return r["spec"], r["frames"], r["status"], outs, ri["status"]


@pytest.mark.parametrize("n,hop", _BATCH)
def test_ragged_batch_layouts_and_order_are_bit_identical(N, ctx, n, hop):
    q, clips = _batch_clips(n)
    table = _table(n, "hann", n)
    bins = n // 2 + 1
    spec, frames, status, sigs, ist = _batch_run(N, ctx, n, hop)
    assert list(status) == [N.CLIP_OK, N.CLIP_NONFINITE, N.CLIP_TOO_SHORT, N.CLIP_OK, N.CLIP_OK]
    assert list(ist) == [N.CLIP_OK, N.CLIP_TOO_SHORT, N.CLIP_TOO_SHORT, N.CLIP_OK, N.CLIP_OK]   # no rows came of clips 1 and 2
    assert spec[1] is None and spec[2] is None and frames[1] == 1 + clips[1].size // hop and frames[2] == 0
    good = (0, 3, 4)
    for i in good:                                                  # alone
        r = _stft(N, ctx, [clips[i]], n, hop, table, True, "reflect")
        np.testing.assert_array_equal(r["spec"][0], spec[i], err_msg=f"alone {i}")
        x, _ = _istft(N, ctx, [spec[i]], n, hop, table, True, [clips[i].size])
        np.testing.assert_array_equal(x[0], sigs[i], err_msg=f"alone {i}")
    order = [4, 2, 0, 1, 3]                                          # another order
    r = _stft(N, ctx, [clips[i] for i in order], n, hop, table, True, "reflect")
    for k, i in enumerate(order):
        assert r["status"][k] == status[i]
        if i in good:
            np.testing.assert_array_equal(r["spec"][k], spec[i], err_msg=f"order {i}")
    buf16, offsets, lengths = _pack(N, [c for k, c in enumerate(q) if k != 1])   # int16 (it has no NaN to give)
    r = ctx.stft_batch(buf16, offsets, lengths, N.stft_opts(n, hop, True, "reflect"), table)
    for k, i in enumerate((0, 2, 3, 4)):
        assert r["status"][k] == status[i]
        if i in good:
            np.testing.assert_array_equal(r["spec"][k], spec[i], err_msg=f"int16 {i}")
    # device in, device out, scattered with gaps in reverse order; nothing outside the rows is written
    m = len(clips)
    soff, pos = np.zeros(m, np.int64), 0
    for i in reversed(range(m)):
        soff[i] = pos + 37
        pos = soff[i] + clips[i].size
    sbuf = np.full(pos + 5, 9.0e9, np.float32)
    for i in range(m):
        sbuf[soff[i]:soff[i] + clips[i].size] = clips[i]
    ooff, opos = np.zeros(m, np.int64), 0
    for i in reversed(range(m)):
        ooff[i] = opos + 3
        opos = ooff[i] + frames[i] * bins
    d_in, d_out = N.DeviceBuffer(ctx, sbuf.nbytes), N.DeviceBuffer(ctx, 8 * (opos + 2))
    d_in.upload(sbuf)
    d_out.upload(np.full(opos + 2, 77.0, np.complex64))
    lengths = np.array([c.size for c in clips], np.int64)
    r = ctx.stft_batch(d_in, soff, lengths, N.stft_opts(n, hop, True, "reflect"), table, fmt=N.FMT_F32, out=d_out, out_offsets=ooff)
    assert list(r["status"]) == list(status) and "spec" not in r
    back = np.zeros(opos + 2, np.complex64)
    d_out.download(back)
    keep = np.ones(back.size, bool)
    for i in range(m):
        rows = back[ooff[i]:ooff[i] + frames[i] * bins]
        keep[ooff[i]:ooff[i] + frames[i] * bins] = False
        if i in good:
            np.testing.assert_array_equal(rows.reshape(frames[i], bins).T, spec[i], err_msg=f"device {i}")
    assert not back[ooff[1]:ooff[1] + frames[1] * bins].any()        # the NaN clip: zeros
    assert np.all(back[keep] == 77.0)
    # the inverse from those rows in device memory to device memory
    xoff = N.packed_offsets(lengths, 4) + 11
    d_sig = N.DeviceBuffer(ctx, 4 * int(xoff[-1] + lengths[-1] + 3))
    d_sig.upload(np.full(d_sig.nbytes // 4, 55.0, np.float32))
    nf = np.where(status == N.CLIP_OK, frames, 0)
    r = ctx.istft_batch(d_out, ooff, nf, N.stft_opts(n, hop, True), table, lengths=lengths, out=d_sig, out_offsets=xoff)
    assert list(r["status"]) == list(ist)
    xb = np.zeros(d_sig.nbytes // 4, np.float32)
    d_sig.download(xb)
    keep = np.ones(xb.size, bool)
    for i in good:
        np.testing.assert_array_equal(xb[xoff[i]:xoff[i] + lengths[i]], sigs[i], err_msg=f"device istft {i}")
        keep[xoff[i]:xoff[i] + lengths[i]] = False
    assert np.all(xb[keep] == 55.0)
    for d in (d_in, d_out, d_sig):
        d.free()
    again = _batch_run(N, ctx, n, hop)                               # a second run repeats the first bit for bit
    for i in good:
        np.testing.assert_array_equal(again[0][i], spec[i])
        np.testing.assert_array_equal(again[3][i], sigs[i])


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from audio_feature_extraction_amd import _native as N
from tests import test_gpu_stft as T
ctx = N.Context(0)
res = {}
for n, hop in T._BATCH:
    spec, frames, status, sigs, ist = T._batch_run(N, ctx, n, hop)
    for i in (0, 3, 4):
        res[f"spec{n}_{i}"] = np.ascontiguousarray(spec[i])
        res[f"sig{n}_{i}"] = sigs[i]
    res[f"status{n}"] = np.concatenate([status, ist])
np.savez(sys.argv[2], **res)
"""


def test_chunked_equals_unchunked(N, ctx, tmp_path):
    """the same batches cut into chunks by a small workspace budget, in a child process (the budget is read once per process)"""
    budget = 120000
    for n, hop in _BATCH:
        _, clips = _batch_clips(n)
        o = N.stft_opts(n, hop, True, "reflect")
        eff = [c.size if N.stft_frames(o, c.size)[1] == N.CLIP_OK else 0 for c in clips]
        assert N.stft_chunks(eff, N.stft_cost(o), budget).max() + 1 >= 3
        assert N.stft_chunks(eff, N.stft_cost(o), 2 << 30).max() == 0
        w = [N.istft_samples(o, N.stft_frames(o, L)[0], L)[0] + -(-L // hop) if L else 0 for L in eff]
        assert N.stft_chunks(w, N.stft_cost(o, inverse=True), budget).max() + 1 >= 3
    dst = str(tmp_path / "chunked.npz")
    env = dict(os.environ, AFX_TEST_STFT_BUDGET=str(budget))
    subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _CHILD, ROOT, dst], env=env, check=True, timeout=150)
    z = np.load(dst)
    for n, hop in _BATCH:
        spec, frames, status, sigs, ist = _batch_run(N, ctx, n, hop)
        np.testing.assert_array_equal(z[f"status{n}"], np.concatenate([status, ist]))
        for i in (0, 3, 4):
            np.testing.assert_array_equal(z[f"spec{n}_{i}"], spec[i])
            np.testing.assert_array_equal(z[f"sig{n}_{i}"], sigs[i])


def test_python_front_end_and_round_trip(N, ctx):
    import audio_feature_extraction_amd as pkg
    from audio_feature_extraction_amd.core import spectrum as S
    y = _clip(9000, seed=3)
    for n, hop, window, pad_mode in ((2048, None, "hann", "constant"), (1024, 256, "hamming", "reflect"), (2048, 441, "hann", "reflect")):
        D = pkg.stft(y, n_fft=n, hop_length=hop, window=window, pad_mode=pad_mode)
        h = n // 4 if hop is None else hop
        assert D.dtype == np.complex64 and D.shape == (n // 2 + 1, 1 + y.size // h) and D.flags.f_contiguous
        np.testing.assert_array_equal(D, _stft(N, ctx, [y], n, h, _table(n, window, n), True, pad_mode)["spec"][0])
        x = pkg.istft(D, hop_length=hop, window=window, length=y.size)
        assert x.dtype == np.float32 and x.shape == y.shape
        np.testing.assert_array_equal(x, pkg.istft(np.ascontiguousarray(D), hop_length=hop, window=window, length=y.size))
        kw = dict(hop_length=h, window=window)
        rt32 = R.istft(R.stft(y, n, pad_mode=pad_mode, f32=True, **kw), length=y.size, f32=True, **kw)
        yard = float(np.abs(rt32 - y).max() / np.abs(y).max())
        dev = float(np.abs(x.astype(np.float64) - y).max() / np.abs(y).max())
        print(f"round trip {n}/{h}/{window}: device {dev:.3g}, yardstick {yard:.3g} -> bound {4 * yard:.3g}")
        assert dev <= 4 * yard
        assert pkg.istft(D, hop_length=hop, window=window).size == h * (D.shape[1] - 1)
    D = S.stft(y)
    np.testing.assert_array_equal(S.spectrogram(y), _stft(N, ctx, [y], 2048, 512, _table(2048, "hann", 2048), kind=N.STFT_MAG)["spec"][0])
    P = S.spectrogram(y, power=2)
    assert P.dtype == np.float32 and np.abs(P - np.abs(D).astype(np.float64) ** 2).max() <= 1e-5 * P.max()
    db = pkg.amplitude_to_db(np.abs(D), ref=np.max)                  # visualization.py:194-208
    assert db.shape == D.shape and db.max() == 0.0 and db.min() >= -80.0
    q = np.round(y * 32767.0).astype(np.int16)
    np.testing.assert_array_equal(S.stft(q), S.stft(q.astype(np.float32) / np.float32(32768.0)))
    bad = y.copy()
    bad[5] = np.inf
    for clip, kw in ((bad, {}), (y[:0], {}), (y[:1000], dict(center=False)), (y[:1024], dict(pad_mode="reflect"))):
        with pytest.raises(ValueError):
            S.stft(clip, **kw)
    with pytest.raises(ValueError):
        S.istft(D[:, :0])
    many = S.stft_batch([y, bad, y[:1024], y[:3000]], pad_mode="reflect")
    assert many[1] is None and many[2] is None
    np.testing.assert_array_equal(many[0], S.stft(y, pad_mode="reflect"))
    back = S.istft_batch([many[0], D[:, :0], many[3]], length=[y.size, None, 3000])
    assert back[1] is None and back[0].size == y.size and back[2].size == 3000
    np.testing.assert_array_equal(back[2], S.istft(many[3], length=3000))
