"""GPU tests of afx_loudness_batch and of audio_feature_extraction_amd.loudness / AudioFeatureExtractor.normalize_volume,
bit for bit against the host executor (afx_loudness_host, the kernels' specification) and, within the bound derived in
tests/loudness_ref.py, against its float64 oracle.

One batch (loudness_ref.gpu_batch) mixes the rates 8000, 11025, 16000, 44100 and 48000 and holds, per rate, the lengths
B - 1 (refused), B, B + 1 (B = ceil(0.4 rate)), both sides of the first two flips of the block count's rounding (the second
leaves a partial last block), a whole number of the kernels' tiles - 1, + 0, + 1, and more than two and more than three
tiles beyond; every such clip lies between a clip of +1e30 and one of -1e30 in device memory with nothing between them, so
a read across a clip boundary changes a sum.  The batch also holds an empty clip, a clip with a NaN, an all-zero clip (it
reads -inf and comes back unchanged) and the gating clip that both gates cut.  Outputs go into sentinel-filled arrays whose
gaps, and the ranges of the refused clips, must stay untouched.

Re-measured levels.  The gain is applied as a float32 (the reference's arithmetic), so a normalised clip sits at
input + 20 log10(applied gain), up to 20 log10(1 + 2^-24) = 5.2e-7 dB from the target before anything is measured; the
re-measured level is held to the measuring bound (TOL_DB = 8e-8 dB) around that figure, and that figure to the float32
rounding of the gain around -23.0."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from tests import loudness_ref as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = np.float32(1234.5)
CHUNK_BUDGET = 150000
TARGET = -23.0


@pytest.fixture(scope="module")
def N():
    from audio_feature_extraction_amd import _native
    if _native.device_count() < 1:
        pytest.fail("no GPU visible")
    return _native


@pytest.fixture(scope="module")
def ctx(N):
    return N.Context(0)


def _run(N, ctx, samples, b, mode, target=TARGET, fmt=None):
    ooff, size = L.out_layout(b["lengths"])
    out = np.full(size, SENTINEL, np.float32) if mode != N.LOUD_MEASURE else None
    return ctx.loudness_batch(samples, b["offsets"], b["lengths"], b["rates"], 0.4, mode, target, want_blocks=True, fmt=fmt,
                              out=out, out_offsets=ooff if out is not None else None)


@pytest.fixture(scope="module")
def dev_run(N, ctx):
    """the batch from device memory (the flanks lie next to the clips), normalised to -23 LUFS into a host array"""
    b = L.gpu_batch()
    d = N.DeviceBuffer(ctx, b["buf"].nbytes)
    d.upload(b["buf"])
    r = _run(N, ctx, d, b, N.LOUD_NORM_LOUDNESS, fmt=N.FMT_F32)
    d.free()
    return r


@pytest.fixture(scope="module")
def host_exec(N):
    """afx_loudness_host of every clip, once"""
    b = L.gpu_batch()
    return [N.loudness_host(b["buf"][o:o + n], int(r), mode=N.LOUD_NORM_LOUDNESS, target=TARGET)
            for o, n, r in zip(b["offsets"], b["lengths"], b["rates"])]


def _live(b):
    return [i for i in b["shape"] if b["lengths"][i] >= 0.4 * b["rates"][i]] + [b["zero"], b["gating"]]


def test_statuses(N, dev_run):
    b = L.gpu_batch()
    st = dev_run["status"]
    live = _live(b)
    assert len(live) == len(b["shape"]) - len(L.RATES) + 2
    for i in range(len(st)):
        want = N.CLIP_OK if i in live else N.CLIP_NONFINITE if i == b["nan"] else N.CLIP_TOO_SHORT
        assert st[i] == want, i
    assert np.isnan(dev_run["rec"][st != N.CLIP_OK]).all()


def test_device_equals_host_executor_bit_for_bit(N, dev_run, host_exec):
    b = L.gpu_batch()
    for i in _live(b):
        h = host_exec[i]
        assert h["status"] == N.CLIP_OK
        assert dev_run["rec"][i].tobytes() == h["rec"].tobytes(), (i, dev_run["rec"][i], h["rec"])     # LUFS, counts, means, gain
        zo, zc = dev_run["z_offsets"][i], dev_run["z_counts"][i]
        assert zc == h["z"].size and dev_run["z"][zo:zo + zc].tobytes() == h["z"].tobytes(), i
        o, n = dev_run["offsets"][i], b["lengths"][i]
        assert dev_run["out"][o:o + n].tobytes() == h["out"].tobytes(), i


def test_outputs_leave_gaps_and_refused_clips_untouched(N, dev_run):
    b = L.gpu_batch()
    mask = np.ones(dev_run["out"].size, bool)
    for i in _live(b):
        mask[dev_run["offsets"][i]:dev_run["offsets"][i] + b["lengths"][i]] = False
    assert (dev_run["out"][mask] == SENTINEL).all()
    o = dev_run["offsets"][b["zero"]]
    assert not dev_run["out"][o:o + b["lengths"][b["zero"]]].any()               # silence: -inf, unchanged, gain 1
    rz = dict(zip(N.LOUD_FIELDS, dev_run["rec"][b["zero"]]))
    assert rz["lufs"] == -np.inf and rz["gain"] == 1.0 and rz["n1"] == 0 and rz["n2"] == 0


def test_loudness_against_the_float64_oracle(N, dev_run):
    b = L.gpu_batch()
    worst = 0.0
    for k, i in enumerate(b["shape"]):
        m = L.oracle(k)
        if m is None:
            continue
        rec = dict(zip(N.LOUD_FIELDS, dev_run["rec"][i]))
        assert (rec["blocks"], rec["n1"], rec["n2"]) == (len(m["z"]), m["n1"], m["n2"]), i
        worst = max(worst, abs(rec["lufs"] - m["lufs"]))
    m = L.oracle(-1)
    rec = dict(zip(N.LOUD_FIELDS, dev_run["rec"][b["gating"]]))
    assert (rec["blocks"], rec["n1"], rec["n2"]) == (67, m["n1"], m["n2"]) and rec["n1"] < 67 and rec["n2"] < rec["n1"]
    worst = max(worst, abs(rec["lufs"] - m["lufs"]))
    print("largest |device - float64 oracle| = %.3g dB; bound %.3g dB" % (worst, L.TOL_DB))
    assert worst <= L.TOL_DB


def test_host_memory_and_measure_only_give_the_same_bits(N, ctx, dev_run):
    b = L.gpu_batch()
    r = _run(N, ctx, b["buf"], b, N.LOUD_MEASURE)
    assert "out" not in r
    np.testing.assert_array_equal(r["status"], dev_run["status"])
    assert r["z"].tobytes() == dev_run["z"].tobytes()
    keep = [k for k, f in enumerate(N.LOUD_FIELDS) if f not in ("gain", "peak_out")]
    ok = r["status"] == N.CLIP_OK
    assert r["rec"][ok][:, keep].tobytes() == dev_run["rec"][ok][:, keep].tobytes()
    assert np.isnan(r["rec"][ok][:, [7, 8]]).all()


def test_int16_input_is_value_over_32768(N, ctx):
    b = L.gpu_batch()
    xi = np.round(np.nan_to_num(np.clip(b["buf"], -1.0, 1.0)) * 32767.0).astype(np.int16)
    a = _run(N, ctx, xi, b, N.LOUD_NORM_LOUDNESS)
    f = _run(N, ctx, xi.astype(np.float32) / np.float32(32768.0), b, N.LOUD_NORM_LOUDNESS)
    np.testing.assert_array_equal(a["status"], f["status"])
    assert (a["status"] == N.CLIP_OK).sum() >= len(_live(b))
    assert a["rec"].tobytes() == f["rec"].tobytes() and a["z"].tobytes() == f["z"].tobytes() and a["out"].tobytes() == f["out"].tobytes()


def test_peak_mode_equals_host_executor(N, ctx):
    b = L.gpu_batch()
    r = _run(N, ctx, b["buf"], b, N.LOUD_NORM_PEAK, target=-1.0)
    for i in range(len(b["lengths"])):
        o, n = b["offsets"][i], b["lengths"][i]
        if i in (b["empty"], b["nan"]):
            assert r["status"][i] == (N.CLIP_TOO_SHORT if i == b["empty"] else N.CLIP_NONFINITE)
            continue
        if i % 7 and i not in (b["zero"], b["gating"]):                  # every seventh clip, flanks and refused ones among them
            continue
        h = N.loudness_host(b["buf"][o:o + n], int(b["rates"][i]), mode=N.LOUD_NORM_PEAK, target=-1.0)
        assert r["status"][i] == N.CLIP_OK and h["status"] == N.CLIP_OK
        assert r["rec"][i].tobytes() == h["rec"].tobytes(), i
        assert r["out"][r["offsets"][i]:r["offsets"][i] + n].tobytes() == h["out"].tobytes(), i


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from audio_feature_extraction_amd import _native as N
from tests import loudness_ref as L
b = L.gpu_batch()
ooff, size = L.out_layout(b["lengths"])
out = np.full(size, np.float32(1234.5), np.float32)
assert N.stft_chunks(b["lengths"], N.loudness_cost(N.FMT_F32, N.MEM_HOST, N.MEM_HOST, N.LOUD_NORM_LOUDNESS), int(sys.argv[3])).max() + 1 >= 20
ctx = N.Context(0)
r = ctx.loudness_batch(b["buf"], b["offsets"], b["lengths"], b["rates"], 0.4, N.LOUD_NORM_LOUDNESS, -23.0, want_blocks=True,
                       out=out, out_offsets=ooff)
np.savez(sys.argv[2], rec=r["rec"], z=r["z"], out=r["out"], status=r["status"])
"""


def test_chunked_batch_equals_one_chunk(N, dev_run, tmp_path):
    """a host-to-host clip costs 8 bytes per sample and 64 per block: at a budget of 150 000 bytes the longer clips go alone
    and the batch takes at least twenty chunks"""
    b = L.gpu_batch()
    assert N.stft_chunks(b["lengths"], N.loudness_cost(N.FMT_F32, N.MEM_HOST, N.MEM_HOST, N.LOUD_NORM_LOUDNESS), 2 << 30).max() == 0
    env = dict(os.environ, AFX_TEST_LOUD_BUDGET=str(CHUNK_BUDGET))
    dst = str(tmp_path / "chunked.npz")
    subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _CHILD, ROOT, dst, str(CHUNK_BUDGET)], env=env, check=True, timeout=150)
    z = np.load(dst)
    np.testing.assert_array_equal(z["status"], dev_run["status"])
    assert z["rec"].tobytes() == dev_run["rec"].tobytes() and z["z"].tobytes() == dev_run["z"].tobytes()
    assert z["out"].tobytes() == dev_run["out"].tobytes()


def test_more_than_sixteen_rates_are_refused(N, ctx):
    n = 17
    x = np.zeros(n * 8, np.float32)
    with pytest.raises(NotImplementedError):
        ctx.loudness_batch(x, np.arange(n) * 8, np.full(n, 8), 8000 + np.arange(n), 0.4, N.LOUD_MEASURE)
    with pytest.raises(NotImplementedError):
        ctx.loudness_batch(x, np.arange(n) * 8, np.full(n, 8), 2000, 0.4, N.LOUD_MEASURE)


def test_normalize_batch_remeasures_at_the_target():
    from audio_feature_extraction_amd import loudness
    picks = [1, 5, 6, 10, 23, 30, 47, 59]                                  # B, both flips, tiles, every rate
    clips = [L.shape_clips()[k][1] for k in picks] + [L.gating_clip()[1], np.zeros(8000, np.float32), L.noise(100, 3)]
    rates = [L.shape_clips()[k][0] for k in picks] + [16000, 16000, 16000]
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                     # nothing here comes near full scale
        ys, ls = loudness.normalize_batch(clips, rates, TARGET)
    again = loudness.integrated_loudness_batch(ys, rates)
    for k in range(len(picks) + 1):
        m = L.oracle(picks[k] if k < len(picks) else -1)
        assert abs(ls[k] - m["lufs"]) <= L.TOL_DB
        g = float(np.float32(10.0 ** ((TARGET - ls[k]) / 20.0)))
        assert ys[k].tobytes() == (np.float32(g) * clips[k]).tobytes()
        assert abs(ls[k] + 20.0 * np.log10(g) - TARGET) <= L.GAIN_ROUND_DB
        print("clip %d: re-measured %.9f, %.3g dB from the level the applied gain sets" % (k, again[k], again[k] - (ls[k] + 20.0 * np.log10(g))))
        assert abs(again[k] - (ls[k] + 20.0 * np.log10(g))) <= L.TOL_DB
        assert abs(again[k] - TARGET) <= L.TOL_DB + L.GAIN_ROUND_DB
    assert ls[-2] == -np.inf and not ys[-2].any() and again[-2] == -np.inf   # silence comes back unchanged
    assert ls[-1] is None and ys[-1].tobytes() == clips[-1].tobytes() and again[-1] is None     # too short: unchanged


def test_meter_block_loudness_and_the_extractor():
    from audio_feature_extraction_amd import AudioFeatureExtractor, loudness
    rate, x = L.gating_clip()
    m = L.oracle(-1)
    assert abs(loudness.Meter(rate).integrated_loudness(x) - m["lufs"]) <= L.TOL_DB
    assert abs(loudness.integrated_loudness(x.astype(np.float64), rate) - m["lufs"]) <= L.TOL_DB
    lj = loudness.block_loudness(x, rate)
    fin = np.isfinite(m["l"])
    assert lj.shape == m["l"].shape and np.array_equal(np.isfinite(lj), fin)
    gated = m["l"] > -70.0               # z_j holds to 1e-10 of the largest block: 1e-5 of one 50 dB below it, 4.3e-5 dB
    assert gated.sum() == m["n1"] and np.all(np.abs(lj[gated] - m["l"][gated]) <= 1e-4)
    bad = x.copy()
    bad[5] = np.inf
    with pytest.raises(ValueError):
        loudness.integrated_loudness(bad, rate)
    ex = AudioFeatureExtractor(sr=rate, device=0)
    y = ex.normalize_volume(x)
    assert y.tobytes() == L.normalize_loudness(x, loudness.integrated_loudness(x, rate), TARGET).tobytes()
    short = L.noise(6399, 9)
    assert ex.normalize_volume(short).tobytes() == short.tobytes()         # process_audio.py:143-147
    with pytest.warns(UserWarning, match="clipped"):
        loudness.normalize_peak(x, 0.5)
    p = loudness.normalize_peak(x, -1.0)
    assert p.tobytes() == L.normalize_peak(x, -1.0).tobytes()
