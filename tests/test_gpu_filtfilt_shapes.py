"""GPU tests of afx_sosfiltfilt_batch at every section count (the kernels are templated on it: S = 1 .. 4) and at the padding
lengths where an index of theirs changes path: none, 1, the default 18, either side of one block, half a tile, and either
side of a whole tile of extension (filt_ref.SHAPE_FILTERS x SHAPE_PADLENS x shape_lengths_general).  The filters pass DC
as well as block it, and half of them are not the project's own sections: scipy's Butterworth, elliptic, Chebyshev and
band-pass sections, gain-only sections and a first-order one.

afx_sosfiltfilt_host is the kernels' specification (tests/test_filt_host.py holds it to scipy on the same cases, on the CPU):
the kernels must equal it bit for bit.  Against scipy.signal.sosfiltfilt the tolerance is the one tests/filt_ref.py derives,
|got - ref| <= 2^-23 + 4 conditioning(case) on outputs scaled to a reference peak of 1, with the conditioning of general
sections taken between the cascade and its reverse.

One batch per (filter, padlen): the lengths of shape_lengths_general, a clip of exactly padlen samples (too short) and a clip
with one NaN.  The NaN clip has 500 samples where the filter takes 500 samples (padlen < 500) and padlen + 500 otherwise, so
that it is refused for the NaN at every padlen."""
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
PAIRS = [(name, p) for name in F.SHAPE_FILTER_SECTIONS for p in F.SHAPE_PADLENS]
PAIR_IDS = [f"{name}-S{F.SHAPE_FILTER_SECTIONS[name]}-pad{p}" for name, p in PAIRS]
FOUR, FOUR_PAD = "lp8_0.05", 4096                      # the register-heavy instantiations, a first tile of extension only
CHUNK_BUDGET = 200000
TILE_BYTES = 4096 * 8 + 64 * 8 * 8 + 8                 # a tile's float64 workspace, the carries of its blocks, its maximum


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
def _lengths(p):
    from audio_feature_extraction_amd import _native
    g = _native.filtfilt_geometry()
    return F.shape_lengths_general(g["block"], g["tile"], p)


@functools.lru_cache(maxsize=None)
def _clips(name, p):
    """the shape clips, then the too-short one and the one with a NaN"""
    clips = [F.shape_clip(name, p, n) for n in _lengths(p)]
    bad = F.signal(500 if p < 500 else p + 500, F.SHAPE_SR, 51)
    bad[250] = np.nan
    clips += [F.signal(p, F.SHAPE_SR, 50), bad]
    for c in clips:
        c.setflags(write=False)
    return tuple(clips)


def _pack(clips, dtype=np.float32):
    lengths = np.array([c.size for c in clips], np.int64)
    offsets = np.zeros(len(clips), np.int64)
    offsets[1:] = np.cumsum(lengths)[:-1]
    return np.concatenate(clips).astype(dtype), offsets, lengths


def _run(ctx, name, p, clips, mode=0, dtype=np.float32):
    """the batch into a sentinel-filled host array at 4-aligned packed offsets"""
    from audio_feature_extraction_amd import _native
    y, off, ln = _pack(clips, dtype)
    oo = _native.packed_offsets(ln, 4)
    out = np.full(int(oo[-1] + ln[-1]) + 8, SENTINEL, np.float32)
    r = ctx.sosfiltfilt_batch(y, off, ln, F.SHAPE_FILTERS[name], p, mode=mode, preemph=F.COEF, out=out, out_offsets=oo)
    assert r["out"] is out
    return r


_batches = {}


def _batch(ctx, name, p):
    """the plain batch of a (filter, padlen): run once, shared, never modified"""
    if (name, p) not in _batches:
        r = _run(ctx, name, p, _clips(name, p))
        for v in r.values():
            v.setflags(write=False)
        _batches[(name, p)] = r
    return _batches[(name, p)]


def _rows(r, i, n):
    return r["out"][int(r["offsets"][i]):int(r["offsets"][i]) + n]


def _assert_equals_host(N, r, clips, sos, p, mode, what):
    for i, c in enumerate(clips):
        h = N.sosfiltfilt_host(c, sos, p, mode, F.COEF)
        assert h["status"] == r["status"][i], (what, i, c.size)
        if h["status"] == N.CLIP_OK:
            np.testing.assert_array_equal(_rows(r, i, c.size).view(np.uint32), h["out"].view(np.uint32),
                                          err_msg=f"{what} clip {i} n {c.size}")
            np.testing.assert_array_equal(r["peak"][i], h["peak"], err_msg=f"{what} clip {i} n {c.size}")


@pytest.mark.parametrize("name,p", PAIRS, ids=PAIR_IDS)
def test_kernels_equal_the_host_executor_bit_for_bit(ctx, N, name, p):
    """the gate for a divergence that only one section count or one padding length shows"""
    clips = _clips(name, p)
    r = _batch(ctx, name, p)
    assert (r["status"][:len(clips) - 2] == N.CLIP_OK).all()
    _assert_equals_host(N, r, clips, F.SHAPE_FILTERS[name], p, N.FILT_PLAIN, f"{name} padlen {p}")


@pytest.mark.parametrize("name", list(F.SHAPE_FILTER_SECTIONS))
def test_results_match_scipy(ctx, N, name):
    worst = 0.0
    for p in F.SHAPE_PADLENS:
        r = _batch(ctx, name, p)
        for i, n in enumerate(_lengths(p)):
            assert r["status"][i] == N.CLIP_OK
            ref, bnd = F.shape_case(name, p, n)
            ratio = F.sos_error_ratio(_rows(r, i, n), ref, bnd)
            assert ratio <= 1.0, (name, p, n, ratio)
            worst = max(worst, ratio)
    print(f"{name} (S = {F.SHAPE_FILTER_SECTIONS[name]}): largest ratio to the bound {worst:.3f}")


@pytest.mark.parametrize("name,p", PAIRS, ids=PAIR_IDS)
def test_untouched_ranges_and_statuses(ctx, N, name, p):
    clips = _clips(name, p)
    r = _batch(ctx, name, p)
    st = r["status"]
    assert st.tolist() == [N.CLIP_OK] * (len(clips) - 2) + [N.CLIP_TOO_SHORT, N.CLIP_NONFINITE]
    written = np.zeros(r["out"].size, bool)
    for i, c in enumerate(clips[:-2]):
        written[int(r["offsets"][i]):int(r["offsets"][i]) + c.size] = True
    assert (r["out"][~written] == SENTINEL).all()                     # failed clips, the alignment gaps, the tail
    assert np.isfinite(r["out"][written]).all() and (r["out"][written] != SENTINEL).all()
    assert not r["peak"][-2:].any()
    tiles = [(c.size + 2 * p + 4095) // 4096 for c in clips[:-2]]
    i = int(np.argmax(tiles))                                         # a clip alone equals its rows in the batch
    solo = _run(ctx, name, p, [clips[i]])
    assert solo["status"][0] == N.CLIP_OK
    np.testing.assert_array_equal(solo["out"][:clips[i].size].view(np.uint32), _rows(r, i, clips[i].size).view(np.uint32))
    np.testing.assert_array_equal(solo["peak"][0], r["peak"][i])
    assert (solo["out"][clips[i].size:] == SENTINEL).all()


@pytest.mark.parametrize("name,p", F.EXPERIMENT_PAIRS)
def test_experiment_mode_on_other_filters(ctx, N, name, p):
    """k_filt_scale and the pre-emphasised input with S = 1 and S = 4; at padlen 4096 the clip's samples begin in the
    second tile, and the first tile's maximum must come out 0 whatever the workspace held: a loud clip without padding
    goes first and leaves a large maximum in every tile slot the batch uses"""
    clips = _clips(name, p)
    loud = _run(ctx, name, 0, [8.0 * F.signal(24 * 4096, F.SHAPE_SR, 52)])
    assert loud["status"][0] == N.CLIP_OK and loud["peak"][0][0] > 8.0
    r = _run(ctx, name, p, clips, N.FILT_EXPERIMENT)
    _assert_equals_host(N, r, clips, F.SHAPE_FILTERS[name], p, N.FILT_EXPERIMENT, f"experiment {name} padlen {p}")
    for i, c in enumerate(clips[:-2]):
        assert r["status"][i] == N.CLIP_OK and np.max(np.abs(_rows(r, i, c.size))) == 1.0, (name, p, c.size)
    written = np.zeros(r["out"].size, bool)
    for i, c in enumerate(clips[:-2]):
        written[int(r["offsets"][i]):int(r["offsets"][i]) + c.size] = True
    assert (r["out"][~written] == SENTINEL).all()


def test_s16_and_device_paths_with_four_sections(ctx, N):
    sos = F.SHAPE_FILTERS[FOUR]
    clips = _clips(FOUR, FOUR_PAD)
    ref = _batch(ctx, FOUR, FOUR_PAD)
    # S16 is value / 32768 in float32, exactly
    q = [F.to_s16(c) for c in clips[:-1]]
    r = _run(ctx, FOUR, FOUR_PAD, q, dtype=np.int16)
    f = _run(ctx, FOUR, FOUR_PAD, [c.astype(np.float32) / np.float32(32768.0) for c in q])
    np.testing.assert_array_equal(r["out"].view(np.uint32), f["out"].view(np.uint32))
    np.testing.assert_array_equal(r["status"], f["status"])
    np.testing.assert_array_equal(r["peak"], f["peak"])
    assert r["status"].tolist() == [N.CLIP_OK] * (len(q) - 1) + [N.CLIP_TOO_SHORT]
    for i, n in enumerate(_lengths(FOUR_PAD)):
        u = q[i].astype(np.float32) / np.float32(32768.0)
        want = F.sos_reference(sos, u, FOUR_PAD)
        assert F.sos_error_ratio(_rows(r, i, n), want, F.sos_bound(sos, u, FOUR_PAD)) <= 1.0, n
    # device input and device output, every clip at an odd offset with gaps of its own on both sides
    ln = np.array([c.size for c in clips], np.int64)
    in_off = np.cumsum(ln + 2 * np.arange(len(clips)) + 3) - ln
    out_off = np.cumsum(ln + 2 * np.arange(len(clips))[::-1] + 5) - ln
    assert (in_off % 4 != 0).any() and (out_off % 4 != 0).any() and (in_off % 2 == 1).any()
    y = np.full(int(in_off[-1] + ln[-1]) + 9, np.nan, np.float32)     # a neighbour read by mistake would poison the result
    for o, c in zip(in_off, clips):
        y[int(o):int(o) + c.size] = c
    total = int(out_off[-1] + ln[-1]) + 9
    d_in, d_out = N.DeviceBuffer(ctx, y.nbytes), N.DeviceBuffer(ctx, 4 * total)
    try:
        d_in.upload(y)
        d_out.upload(np.full(total, SENTINEL, np.float32))
        d = ctx.sosfiltfilt_batch(d_in, in_off, ln, sos, FOUR_PAD, fmt=N.FMT_F32, out=d_out, out_offsets=out_off)
        got = np.zeros(total, np.float32)
        d_out.download(got)
    finally:
        d_in.free()
        d_out.free()
    np.testing.assert_array_equal(d["status"], ref["status"])
    np.testing.assert_array_equal(d["peak"], ref["peak"])
    gaps = np.ones(total, bool)
    for i, c in enumerate(clips):
        if ref["status"][i] == N.CLIP_OK:
            o = int(out_off[i])
            np.testing.assert_array_equal(got[o:o + c.size].view(np.uint32), _rows(ref, i, c.size).view(np.uint32), err_msg=str(i))
            gaps[o:o + c.size] = False
    assert (got[gaps] == SENTINEL).all()


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_filtfilt_shapes import FOUR, FOUR_PAD, _clips, _run
from audio_feature_extraction_amd import _native as N
ctx = N.Context(0)
res = {}
for mode in (N.FILT_PLAIN, N.FILT_EXPERIMENT):
    r = _run(ctx, FOUR, FOUR_PAD, _clips(FOUR, FOUR_PAD), mode)
    res.update({f"out{mode}": r["out"], f"status{mode}": r["status"], f"peak{mode}": r["peak"]})
np.savez(sys.argv[2], **res)
"""


def test_chunked_batch_equals_one_chunk(ctx, N, tmp_path):
    """four sections, padlen 4096: every clip costs at least three tiles of workspace.  The chunk helper is given a cost
    that is no more than the filter's for every clip here (three tiles and the record per clip, the staged input and output
    per sample), so it cuts no more chunks than the filter does: at least 3 at the small budget, one at the default."""
    clips = _clips(FOUR, FOUR_PAD)
    live = [c.size for c in clips if c.size > FOUR_PAD]
    assert all((n + 2 * FOUR_PAD + 4095) // 4096 >= 3 for n in live)
    cost = [0, 0, 8, 3 * TILE_BYTES + 48, 1, 1 << 24]
    assert N.stft_chunks(live, cost, CHUNK_BUDGET).max() + 1 >= 3
    assert N.stft_chunks(live, cost, 2 << 30).max() == 0
    env = dict(os.environ, AFX_TEST_FILT_BUDGET=str(CHUNK_BUDGET))
    dst = str(tmp_path / "chunked.npz")
    subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _CHILD, ROOT, dst], env=env, check=True, timeout=150)
    z = np.load(dst)
    for mode in (N.FILT_PLAIN, N.FILT_EXPERIMENT):
        r = _batch(ctx, FOUR, FOUR_PAD) if mode == N.FILT_PLAIN else _run(ctx, FOUR, FOUR_PAD, clips, mode)
        np.testing.assert_array_equal(z[f"out{mode}"].view(np.uint32), r["out"].view(np.uint32))
        np.testing.assert_array_equal(z[f"status{mode}"], r["status"])
        np.testing.assert_array_equal(z[f"peak{mode}"], r["peak"])


@pytest.mark.parametrize("btype", ["low", "high"])
def test_python_entry_points_on_every_order(N, btype):
    """Wn = 0.1 at every order: scipy's filtfilt and sosfiltfilt stay within the conditioning cap of each other there
    (5e-10 at most, order 8 low-pass), so no order needs an easier cut-off"""
    import scipy.signal
    from audio_feature_extraction_amd import filters
    x = F.signal(3000, F.SHAPE_SR, 77)
    worst = [0.0, 0.0]
    for order in range(1, 9):
        ref_sos = scipy.signal.butter(order, 0.1, btype, output="sos")
        ref = scipy.signal.sosfiltfilt(ref_sos, x)
        got = filters.sosfiltfilt(filters.butter_sos(order, 0.1, btype), x)
        assert got.dtype == np.float32 and got.shape == x.shape
        r0 = F.sos_error_ratio(got, ref, F.sos_bound(ref_sos, x, 3 * (order + 1)))
        b, a = scipy.signal.butter(order, 0.1, btype)
        ref_ba = scipy.signal.filtfilt(b, a, x)
        peak = float(np.max(np.abs(ref_ba)))
        cond = float(np.max(np.abs(scipy.signal.sosfiltfilt(scipy.signal.tf2sos(b, a), x, padlen=3 * (order + 1)) - ref_ba))) / peak
        assert peak > 0 and cond <= F.MAX_CONDITIONING, (order, btype, cond)
        r1 = F.sos_error_ratio(filters.filtfilt(b, a, x), ref_ba, F.EPS32 + 4.0 * cond)
        print(f"order {order} {btype}: sosfiltfilt {r0:.3f} filtfilt {r1:.3f} of the bound (conditioning {cond:.2e})")
        assert r0 <= 1.0 and r1 <= 1.0, (order, btype, r0, r1)
        worst = [max(worst[0], r0), max(worst[1], r1)]
    print(f"{btype}: largest ratios to the bound (sosfiltfilt, filtfilt): {worst[0]:.3f} {worst[1]:.3f}")


def test_bounds_are_refused_before_any_launch(ctx, N):
    x = F.signal(6000, F.SHAPE_SR, 78)
    off, ln = np.zeros(1, np.int64), np.array([x.size], np.int64)
    sos = F.SHAPE_FILTERS[FOUR]
    for bad_sos, bad_pad in ((sos, 4097), (np.tile(sos[:1], (5, 1)), 18)):
        out = np.full(x.size + 8, SENTINEL, np.float32)
        with pytest.raises(NotImplementedError, match="not supported"):
            ctx.sosfiltfilt_batch(x, off, ln, bad_sos, bad_pad, out=out, out_offsets=off)
        assert (out == SENTINEL).all()
    ok = ctx.sosfiltfilt_batch(x, off, ln, sos, 4096, out=np.full(x.size + 8, SENTINEL, np.float32), out_offsets=off)
    assert ok["status"][0] == N.CLIP_OK and (ok["out"][x.size:] == SENTINEL).all()
