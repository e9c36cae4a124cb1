"""GPU checks of afx_resample_batch / wavio.resample_batch against wavio.resample (scipy.signal.resample_poly with the
engine's own Kaiser filter, float64): every sample within one float32 ulp, at most 1 in 10^5 differing at all."""
from math import gcd

import numpy as np
import pytest

from audio_feature_extraction_amd import wavio

pytestmark = pytest.mark.gpu

PAIRS = [(44100, 22050), (48000, 22050), (16000, 22050), (48000, 16000), (44100, 16000),
         (22050, 44100), (44100, 48000), (11025, 22050), (8000, 22050), (22050, 16000)]


@pytest.fixture(scope="module")
def ctx():
    from audio_feature_extraction_amd import _native
    if _native.device_count() < 1:
        pytest.fail("no GPU visible")
    c = _native.Context(0)
    yield c
    c.close()


def _ulp_diff(a, b):
    """distance in float32 ulps (order-preserving integer image of the bit patterns)"""
    def key(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def _compare(got, ref, what, tally=None):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not ref.size:
        return 0
    d = _ulp_diff(np.ascontiguousarray(got), np.ascontiguousarray(ref))
    nd = int((d > 0).sum())
    if tally is not None:
        tally[0] += nd
        tally[1] += ref.size
    assert int(d.max()) <= 1, f"{what}: {int((d > 1).sum())} samples beyond one ulp (max {int(d.max())})"
    return nd


def _clips(rng, lens, dtype):
    if dtype == np.int16:
        return [rng.integers(-20000, 20000, size=n).astype(np.int16) for n in lens]
    return [(rng.standard_normal(n) * 0.25).astype(np.float32) for n in lens]


def _ref(c, sr_in, sr_out):
    y = c.astype(np.float32) * np.float32(1.0 / 32768.0) if c.dtype == np.int16 else c
    return wavio.resample(y, sr_in, sr_out)


def _run(ctx, clips, sr_in, sr_out, dev_in=False, dev_out=False, unaligned=False):
    """-> list of resampled clips through Context.resample_batch with the requested memory kinds"""
    from audio_feature_extraction_amd import _native
    dt = clips[0].dtype
    lens = np.array([c.size for c in clips], np.int64)
    step = lens if unaligned else (lens + 3) // 4 * 4
    offs = np.zeros(len(clips), np.int64)
    offs[1:] = np.cumsum(step)[:-1]
    if unaligned:
        offs += 1
    buf = np.zeros(int(offs[-1] + lens[-1]) + 3, dt)
    for o, c in zip(offs, clips):
        buf[o:o + c.size] = c
    olen = _native.resample_lengths(lens, sr_in, sr_out)
    ooffs = None
    if unaligned:
        ooffs = np.zeros(len(clips), np.int64)
        ooffs[1:] = np.cumsum(olen)[:-1]
        ooffs += 3
    need = int(((olen + 3) // 4 * 4).sum()) + 8
    fmt = _native.FMT_S16 if dt == np.int16 else _native.FMT_F32
    src = buf
    if dev_in:
        src = _native.DeviceBuffer(ctx, max(buf.nbytes, 16))
        src.upload(buf)
    dst = _native.DeviceBuffer(ctx, 4 * need) if dev_out else None
    r = ctx.resample_batch(src, offs, lens, sr_in, sr_out, fmt=fmt, out=dst, out_offsets=ooffs)
    assert r["lengths"].tolist() == olen.tolist()
    if dev_out:
        host = np.zeros(need, np.float32)
        assert _native.lib().afx_memcpy_d2h(ctx.handle, host.ctypes.data, dst.ptr, host.nbytes) == 0
        dst.free()
    else:
        host = r["out"]
    if dev_in:
        src.free()
    return [host[o:o + n].copy() for o, n in zip(r["offsets"], r["lengths"])]


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d-%d" % p)
def test_pairs_and_edge_lengths(ctx, pair):
    from audio_feature_extraction_amd import _native
    sr_in, sr_out = pair
    d = _native.resample_design(sr_in, sr_out)
    hd = d["half"] // d["down"]
    lens = [0, 1, 2, 7, max(hd - 1, 0), hd, hd + 1, 1000, 1001, 4096, sr_in // 2 + 3, 0, 5]
    rng = np.random.default_rng(sr_in + sr_out)
    tally = [0, 0]
    for dt in (np.float32, np.int16):
        clips = _clips(rng, lens, dt)
        refs = [_ref(c, sr_in, sr_out) for c in clips]
        for dev_in, dev_out, unaligned in [(False, False, False), (True, True, False), (False, True, True), (True, False, True)]:
            got = _run(ctx, clips, sr_in, sr_out, dev_in, dev_out, unaligned)
            for k, (g, r) in enumerate(zip(got, refs)):
                _compare(g, r, f"{pair} {np.dtype(dt).name} len {lens[k]} dev_in={dev_in} dev_out={dev_out} unaligned={unaligned}", tally)
    print(f"resample {sr_in}->{sr_out}: {tally[0]} of {tally[1]} samples differ from wavio.resample")
    assert tally[0] <= max(1, tally[1] // 100000)


def test_thirty_second_clip(ctx):
    rng = np.random.default_rng(30)
    tally = [0, 0]
    for sr_in, dt in [(44100, np.int16), (48000, np.float32)]:
        clips = _clips(rng, [30 * sr_in], dt)
        got = _run(ctx, clips, sr_in, 22050, dev_in=True, dev_out=True)
        _compare(got[0], _ref(clips[0], sr_in, 22050), f"30 s at {sr_in}", tally)
    print(f"30 s clips: {tally[0]} of {tally[1]} samples differ")
    assert tally[0] <= max(1, tally[1] // 100000)


def test_ragged_batch_of_300_clips(ctx):
    rng = np.random.default_rng(300)
    lens = rng.integers(0, 12000, size=300).tolist()
    tally = [0, 0]
    for (sr_in, sr_out), dt in [((48000, 22050), np.int16), ((16000, 22050), np.float32), ((44100, 22050), np.int16)]:
        clips = _clips(rng, lens, dt)
        got = _run(ctx, clips, sr_in, sr_out, dev_in=True, dev_out=True)
        for k, c in enumerate(clips):
            _compare(got[k], _ref(c, sr_in, sr_out), f"ragged {sr_in}->{sr_out} clip {k} len {lens[k]}", tally)
    print(f"ragged batches: {tally[0]} of {tally[1]} samples differ")
    assert tally[0] <= max(1, tally[1] // 100000)


@pytest.mark.parametrize("pair", [(44100, 22050), (48000, 22050), (8000, 22050)], ids=lambda p: "%d-%d" % p)
def test_no_bleed_from_full_scale_neighbours(ctx, pair):
    sr_in, sr_out = pair
    rng = np.random.default_rng(7)
    loud = lambda n: np.where(rng.integers(0, 2, size=n) > 0, 32767, -32768).astype(np.int16)
    quiet = rng.integers(-3, 4, size=2001).astype(np.int16)
    clips = [loud(3000), quiet, loud(3001)]
    got = _run(ctx, clips, sr_in, sr_out, dev_in=True, dev_out=True, unaligned=True)      # clips touch: no padding between
    ref = _ref(quiet, sr_in, sr_out)
    _compare(got[1], ref, "quiet clip between full-scale neighbours")
    assert float(np.abs(got[1]).max()) < 1e-3
    alone = _run(ctx, [quiet], sr_in, sr_out)[0]
    assert np.array_equal(alone.view(np.int32), got[1].view(np.int32))


def test_nan_clip_leaves_its_neighbours_alone(ctx):
    rng = np.random.default_rng(9)
    clips = _clips(rng, [5000, 4000, 6000], np.float32)
    clips[1][1234] = np.nan
    clips[1][17] = np.inf
    for sr_in, sr_out in [(44100, 22050), (48000, 22050)]:
        got = _run(ctx, clips, sr_in, sr_out, unaligned=True)
        for k in (0, 2):
            _compare(got[k], _ref(clips[k], sr_in, sr_out), f"clean clip {k} beside a NaN clip")
        assert not np.isfinite(got[1]).all()                      # the NaN / inf propagate, as on the host
        for i in (17, 1234):                                      # the output nearest a bad sample has it in its span
            assert not np.isfinite(got[1][i * sr_out // sr_in])


def test_same_call_twice_gives_identical_bits(ctx):
    rng = np.random.default_rng(2)
    clips = _clips(rng, rng.integers(1, 30000, size=40).tolist(), np.int16)
    for sr_in, sr_out in [(48000, 22050), (44100, 22050), (16000, 22050)]:
        a = _run(ctx, clips, sr_in, sr_out, dev_in=True, dev_out=True)
        b = _run(ctx, clips, sr_in, sr_out, dev_in=True, dev_out=True)
        assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


def test_equal_rates_convert_and_unsupported_pairs_say_so(ctx):
    rng = np.random.default_rng(4)
    for dt in (np.int16, np.float32):
        clips = _clips(rng, [0, 1, 4097, 10000], dt)
        got = _run(ctx, clips, 22050, 22050, dev_in=True, dev_out=True)
        for g, c in zip(got, clips):
            assert np.array_equal(g, _ref(c, 22050, 22050))
    with pytest.raises(NotImplementedError):
        _run(ctx, _clips(rng, [100], np.float32), 22051, 22050)
    with pytest.raises(ValueError):
        ctx.resample_batch(np.zeros(8, np.float32), [0], [-1], 44100, 22050)
    with pytest.raises(ValueError):
        ctx.resample_batch(np.zeros(8, np.float32), [0], [8], 0, 22050)


def test_caller_supplied_taps(ctx):
    rng = np.random.default_rng(5)
    clips = _clips(rng, [3000, 17], np.float32)
    g = gcd(44100, 22050)
    h = wavio._resample_filter(22050 // g, 44100 // g)
    from audio_feature_extraction_amd import _native
    lens = np.array([c.size for c in clips], np.int64)
    offs = np.array([0, 3000], np.int64)
    r = ctx.resample_batch(np.concatenate(clips), offs, lens, 44100, 22050, taps=h)
    for k, c in enumerate(clips):
        o, n = int(r["offsets"][k]), int(r["lengths"][k])
        _compare(r["out"][o:o + n], _ref(c, 44100, 22050), "caller-supplied taps")
    with pytest.raises(ValueError):
        ctx.resample_batch(np.concatenate(clips), offs, lens, 44100, 22050, taps=h[:-1])   # even tap count


def test_wavio_resample_batch(ctx):
    rng = np.random.default_rng(6)
    clips = _clips(rng, [100, 0, 5000], np.float32) + _clips(rng, [777, 12000], np.int16)
    got = wavio.resample_batch(clips, 48000, 22050)
    assert len(got) == 5 and all(g.dtype == np.float32 for g in got)
    for g, c in zip(got, clips):
        _compare(g, _ref(c, 48000, 22050), "wavio.resample_batch")
    host = wavio.resample_batch(clips[:1], 22051, 22050)                                   # no device table: the host path
    assert np.array_equal(host[0], wavio.resample(clips[0], 22051, 22050))
