"""GPU tests of afx_sosfiltfilt_batch (zero-phase IIR filtering and the experiment extractor's preprocess_audio), of
audio_feature_extraction_amd.filters and of AudioFeatureExtractor.preprocess_experiment against the restatement
tests/filt_ref.py, whose docstring derives the tolerance:  |got - ref| <= 2^-23 + 4 conditioning(case)  on outputs scaled to
a reference peak of 1, conditioning(case) <= 2^-20 asserted for every case.

One ragged batch per rate holds the nine boundary lengths of the block decomposition (filt_ref.shape_lengths: the shortest
clips, either side of one block, two blocks and one tile of the extended signal, and more than three tiles), a clip of
length 0, one of padlen samples, an all-zero clip and a clip with one NaN.  A batch has one sample format, so the S16 clips
travel in a batch of their own: the same clips quantised."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import filt_ref as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = np.float32(1234.5)
I_EMPTY, I_SHORT, I_ZERO, I_NAN = 9, 10, 11, 12        # behind the nine shape clips


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
def _clips(sr):
    from audio_feature_extraction_amd import _native
    g = _native.filtfilt_geometry()
    clips = [F.signal(n, sr, 100 + k) for k, n in enumerate(F.shape_lengths(g["block"], g["tile"]))]
    clips += [np.zeros(0, np.float32), F.signal(F.PADLEN, sr, 50), np.zeros(1000, np.float32), F.signal(500, sr, 51)]
    clips[I_NAN][250] = np.nan
    for c in clips:
        c.setflags(write=False)
    return tuple(clips)


def _pack(clips, dtype=np.float32):
    lengths = np.array([c.size for c in clips], np.int64)
    offsets = np.zeros(len(clips), np.int64)
    offsets[1:] = np.cumsum(lengths)[:-1]
    return np.concatenate(clips).astype(dtype), offsets, lengths


def _sos(sr):
    from audio_feature_extraction_amd import _native
    return _native.butter_sos(5, 200 / (sr / 2), True)


def _run(ctx, sr, mode, clips, dtype=np.float32):
    """the batch into a sentinel-filled host array at 4-aligned packed offsets"""
    from audio_feature_extraction_amd import _native
    y, off, ln = _pack(clips, dtype)
    oo = _native.packed_offsets(ln, 4)
    out = np.full(int(oo[-1] + ln[-1]) + 8, SENTINEL, np.float32)
    r = ctx.sosfiltfilt_batch(y, off, ln, _sos(sr), F.PADLEN, mode=mode, preemph=F.COEF, out=out, out_offsets=oo)
    assert r["out"] is out
    return r


@pytest.fixture(scope="module")
def runs(ctx, N):
    return {(sr, mode): _run(ctx, sr, mode, _clips(sr)) for sr in F.RATES for mode in (N.FILT_PLAIN, N.FILT_EXPERIMENT)}


@functools.lru_cache(maxsize=None)
def _ref(sr, i, mode, s16=False):
    """(reference, filter input) of clip i: computed once, shared, never modified"""
    y = _clips(sr)[i]
    if s16:
        y = F.to_s16(y).astype(np.float32) / np.float32(32768.0)
    ref, u = (F.highpass(y, sr), y) if mode == 0 else (F.preprocess_experiment(y, sr), F.filter_input(y))
    ref.setflags(write=False)
    return ref, u


@pytest.mark.parametrize("sr", F.RATES)
def test_both_modes_match_the_restatement(runs, N, sr):
    worst = [0.0, 0.0]
    for mode in (N.FILT_PLAIN, N.FILT_EXPERIMENT):
        r = runs[(sr, mode)]
        for i in range(9):
            n = _clips(sr)[i].size
            ref, u = _ref(sr, i, mode)
            got = r["out"][int(r["offsets"][i]):int(r["offsets"][i]) + n]
            ratio = F.error_ratio(got, ref, u, sr)
            print(f"sr {sr} mode {mode} n {n}: {ratio:.3f} of the bound (conditioning {F.conditioning(u, sr):.2e})")
            assert ratio <= 1.0, (sr, mode, n, ratio)
            worst[mode] = max(worst[mode], ratio)
            assert r["peak"][i][0] == np.max(np.abs(_clips(sr)[i]))
            if mode == N.FILT_EXPERIMENT:
                assert np.max(np.abs(got)) == 1.0
            else:
                assert r["peak"][i][1] == pytest.approx(np.max(np.abs(ref)), rel=1e-6)
    print(f"sr {sr}: largest ratios to the bound (plain, experiment): {worst[0]:.3f} {worst[1]:.3f}")


@pytest.mark.parametrize("sr", F.RATES)
def test_statuses_and_untouched_ranges(runs, N, sr):
    for mode in (N.FILT_PLAIN, N.FILT_EXPERIMENT):
        r = runs[(sr, mode)]
        st = r["status"]
        assert st[I_EMPTY] == st[I_SHORT] == N.CLIP_TOO_SHORT and st[I_NAN] == N.CLIP_NONFINITE and st[I_ZERO] == N.CLIP_OK
        assert (np.delete(st, [I_EMPTY, I_SHORT, I_NAN]) == N.CLIP_OK).all()
        clips = _clips(sr)
        written = np.zeros(r["out"].size, bool)
        for i, c in enumerate(clips):
            if st[i] == N.CLIP_OK:
                written[int(r["offsets"][i]):int(r["offsets"][i]) + c.size] = True
        assert (r["out"][~written] == SENTINEL).all()                 # failed clips, the alignment gaps, the tail
        assert np.isfinite(r["out"][written]).all() and (r["out"][written] != SENTINEL).all()
        o = int(r["offsets"][I_ZERO])
        assert not r["out"][o:o + 1000].any()                         # digital silence: zeros, not NaN
        assert not r["peak"][[I_EMPTY, I_SHORT, I_ZERO, I_NAN]].any()


@pytest.mark.parametrize("sr", F.RATES)
def test_kernels_equal_the_host_executor_bit_for_bit(runs, N, sr):
    """afx_sosfiltfilt_host is the kernels' specification: the same tables and the same fused operations in the same order"""
    for mode in (N.FILT_PLAIN, N.FILT_EXPERIMENT):
        r = runs[(sr, mode)]
        for i, c in enumerate(_clips(sr)):
            h = N.sosfiltfilt_host(c, _sos(sr), F.PADLEN, mode, F.COEF)
            assert h["status"] == r["status"][i]
            if h["status"] == N.CLIP_OK:
                got = r["out"][int(r["offsets"][i]):int(r["offsets"][i]) + c.size]
                np.testing.assert_array_equal(got.view(np.uint32), h["out"].view(np.uint32), err_msg=f"mode {mode} clip {i}")
                np.testing.assert_array_equal(r["peak"][i], h["peak"])


def test_a_clip_alone_equals_its_rows_in_the_batch(runs, ctx, N):
    sr = 22050
    for mode in (N.FILT_PLAIN, N.FILT_EXPERIMENT):
        r = runs[(sr, mode)]
        for i, c in enumerate(_clips(sr)):
            solo = _run(ctx, sr, mode, [c])
            assert solo["status"][0] == r["status"][i]
            np.testing.assert_array_equal(solo["out"][:c.size], r["out"][int(r["offsets"][i]):int(r["offsets"][i]) + c.size],
                                          err_msg=f"mode {mode} clip {i}")
            np.testing.assert_array_equal(solo["peak"][0], r["peak"][i])
        again = _run(ctx, sr, mode, _clips(sr))                        # and the batch is reproducible
        np.testing.assert_array_equal(again["out"], r["out"])


def test_s16_batch(ctx, N):
    sr = 22050
    clips = [F.to_s16(c) for i, c in enumerate(_clips(sr)) if i != I_NAN]
    for mode in (N.FILT_PLAIN, N.FILT_EXPERIMENT):
        r = _run(ctx, sr, mode, clips, np.int16)
        f = _run(ctx, sr, mode, [c.astype(np.float32) / np.float32(32768.0) for c in clips])
        np.testing.assert_array_equal(r["out"], f["out"])              # S16 is value / 32768 in float32, exactly
        np.testing.assert_array_equal(r["status"], f["status"])
        for i in range(9):
            ref, u = _ref(sr, i, mode, True)
            got = r["out"][int(r["offsets"][i]):int(r["offsets"][i]) + clips[i].size]
            assert F.error_ratio(got, ref, u, sr) <= 1.0, (mode, i)


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_filtfilt import _clips, _run
from audio_feature_extraction_amd import _native as N
ctx = N.Context(0)
res = {}
for mode in (N.FILT_PLAIN, N.FILT_EXPERIMENT):
    r = _run(ctx, 22050, mode, _clips(22050))
    res.update({f"out{mode}": r["out"], f"status{mode}": r["status"], f"peak{mode}": r["peak"]})
np.savez(sys.argv[2], **res)
"""


def test_chunked_batch_equals_one_chunk(runs, N, tmp_path):
    """a tile costs 36 872 bytes of workspace and a host clip 8 bytes per sample: at a budget of 100 000 bytes a chunk holds
    two of the one-tile clips, and the four-tile clip (246 000 bytes) goes alone -- the eleven filtered clips take at least
    five chunks"""
    env = dict(os.environ, AFX_TEST_FILT_BUDGET="100000")
    dst = str(tmp_path / "chunked.npz")
    subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _CHILD, ROOT, dst], env=env, check=True, timeout=150)
    z = np.load(dst)
    for mode in (N.FILT_PLAIN, N.FILT_EXPERIMENT):
        r = runs[(22050, mode)]
        np.testing.assert_array_equal(z[f"out{mode}"], r["out"])
        np.testing.assert_array_equal(z[f"status{mode}"], r["status"])
        np.testing.assert_array_equal(z[f"peak{mode}"], r["peak"])


def test_device_path_equals_host_path(runs, ctx, N):
    sr = 22050
    y, off, ln = _pack(_clips(sr))
    d_in = N.DeviceBuffer(ctx, y.nbytes)
    d_in.upload(y)
    for mode in (N.FILT_PLAIN, N.FILT_EXPERIMENT):
        r = runs[(sr, mode)]
        d_out = N.DeviceBuffer(ctx, r["out"].nbytes)
        d_out.upload(np.full(r["out"].size, SENTINEL, np.float32))
        d = ctx.sosfiltfilt_batch(d_in, off, ln, _sos(sr), F.PADLEN, mode=mode, preemph=F.COEF, fmt=N.FMT_F32, out=d_out,
                                  out_offsets=r["offsets"])
        got = np.zeros(r["out"].size, np.float32)
        d_out.download(got)
        np.testing.assert_array_equal(got, r["out"])
        np.testing.assert_array_equal(d["status"], r["status"])
        np.testing.assert_array_equal(d["peak"], r["peak"])
        d_out.free()
    d_in.free()


def test_public_python_entry_points(runs, N):
    from audio_feature_extraction_amd import AudioFeatureExtractor, filters
    sr = 22050
    clips = _clips(sr)
    ex = AudioFeatureExtractor(sr=sr, device=0)
    batch = ex.preprocess_experiment_batch(clips)
    r = runs[(sr, N.FILT_EXPERIMENT)]
    assert [b is None for b in batch] == [i in (I_EMPTY, I_SHORT, I_NAN) for i in range(len(clips))]
    for i, b in enumerate(batch):
        if b is None:
            continue
        assert b.dtype == np.float32 and b.shape == clips[i].shape
        np.testing.assert_array_equal(b, r["out"][int(r["offsets"][i]):int(r["offsets"][i]) + clips[i].size])
        if i < 9:
            ref, u = _ref(sr, i, N.FILT_EXPERIMENT)
            assert F.error_ratio(b, ref, u, sr) <= 1.0
    np.testing.assert_array_equal(ex.preprocess_experiment(clips[3]), batch[3])
    for i in (I_SHORT, I_NAN):
        with pytest.raises(ValueError):
            ex.preprocess_experiment(clips[i])
    assert not ex.preprocess_experiment(clips[I_ZERO]).any()
    # the plain filter: our own sections, scipy's sections of the same filter, and (b, a) through tf2sos
    import scipy.signal
    b, a = F.butter_ba(sr)
    rp = runs[(sr, N.FILT_PLAIN)]
    for i in (0, 4, 8):
        ref, u = _ref(sr, i, N.FILT_PLAIN)
        own = filters.sosfiltfilt(_sos(sr), clips[i])
        np.testing.assert_array_equal(own, rp["out"][int(rp["offsets"][i]):int(rp["offsets"][i]) + clips[i].size])
        for got in (own, filters.sosfiltfilt(scipy.signal.tf2sos(b, a), clips[i], padlen=F.PADLEN), filters.filtfilt(b, a, clips[i])):
            assert got.dtype == np.float32 and F.error_ratio(got, ref, u, sr) <= 1.0, i
    many = filters.sosfiltfilt_batch(_sos(sr), clips)
    assert [m is None for m in many] == [i in (I_EMPTY, I_SHORT, I_NAN) for i in range(len(clips))]
    np.testing.assert_array_equal(many[8], rp["out"][int(rp["offsets"][8]):int(rp["offsets"][8]) + clips[8].size])
    with pytest.raises(ValueError, match="infs or NaNs"):
        filters.sosfiltfilt(_sos(sr), clips[I_NAN])
