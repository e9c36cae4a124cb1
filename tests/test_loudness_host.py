"""Host-side tests of the loudness meter: the K-weighting design against its formulas, the block count, the host executor
(afx_loudness_host, the kernels' specification) against the float64 oracle of tests/loudness_ref.py, the ABI's new symbols,
the Python refusals, the extractor's "too short: unchanged", and the stand-alone sanitizer program.  CPU only."""
import os
import re
import subprocess
import warnings

import numpy as np
import pytest

from tests import loudness_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio_feature_extraction_amd", "csrc")
NAMES_HOST = ("afx_kweight_sos", "afx_loudness_geometry", "afx_loudness_blocks", "afx_loudness_cost", "afx_loudness_host")
NAMES_DEVICE = ("afx_loudness_batch",)


@pytest.fixture(scope="module")
def N():
    from audio_feature_extraction_amd import _native
    return _native


def test_symbols_are_declared_bound_and_stubbed(N):
    header = open(os.path.join(ROOT, "include", "afx.h")).read()
    for name in NAMES_HOST + NAMES_DEVICE:
        assert name in N.SYMBOLS
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert hasattr(N.lib(), name)
    assert re.search(r"#define\s+AFX_VERSION\s+107\b", header)                  # found by their presence
    stubs = open(os.path.join(CSRC, "afx_host_stubs.cpp")).read()
    for name in NAMES_DEVICE:
        assert re.search(r"\bint\s+" + name + r"\s*\(", stubs), name
    for name in NAMES_HOST:                                                     # real in the host build
        assert not re.search(r"\bint\s+" + name + r"\s*\(", stubs), name
    mk = open(os.path.join(CSRC, "Makefile")).read()
    asan_srcs = re.search(r"^ASAN_SRCS := (.*)$", mk, re.M).group(1)
    assert "afx_loudness_host.cpp" in asan_srcs and "afx_loudness.hip" not in asan_srcs
    assert "afx_loudness.o" in mk and "afx_loudness_host.o" in mk and "loudness-check:" in mk
    for i, f in enumerate(N.LOUD_FIELDS):                                       # the record's slots as the header names them
        assert re.search(r"\bAFX_LOUD_%s = %d\b" % (f.upper(), i), header), f
    assert re.search(r"\bAFX_LOUD_N = %d\b" % N.LOUD_N, header) and len(N.LOUD_FIELDS) == N.LOUD_N


def test_module_is_exposed_like_quality():
    import audio_feature_extraction_amd as A
    import audio_feature_extraction_toolkit as T
    from audio_feature_extraction_amd import loudness
    assert A.loudness is loudness and T.loudness is loudness
    assert A.__all__ == ["AudioFeatureExtractor", "FeatureEvaluator"]


@pytest.mark.parametrize("rate", [8000, 16000, 22050, 44100, 48000, 192000])
def test_kweight_sos_against_the_formulas(N, rate):
    sos = N.kweight_sos(rate)
    for row, (b, a) in zip(sos, L.kweight(rate)):
        want = np.concatenate([b, a])
        assert np.all(np.abs(row - want) <= 1e-15 * np.abs(want)), (row, want)


def test_geometry_and_refusals(N):
    g = N.loudness_geometry()
    assert g == {"block": 64, "tile_blocks": 64, "tile": L.TILE, "min_rate": 4000, "max_rate": 192000, "max_rates": 16}
    for rate in (3999, 192001, 0):
        with pytest.raises(ValueError):
            N.kweight_sos(rate)
    with pytest.raises(NotImplementedError):
        N.loudness_blocks(1000, 2000)
    with pytest.raises(NotImplementedError):
        N.loudness_blocks(1000, 8000, 0.03)                                     # a segment of 60 samples
    with pytest.raises(ValueError):
        N.loudness_blocks(1000, 8000, 0.0)
    with pytest.raises(ValueError):
        N.loudness_host(np.zeros(8000, np.float32), 16000, mode=3)
    with pytest.raises(ValueError):
        N.loudness_host(np.zeros(8000, np.float64), 16000)
    cost = N.loudness_cost(N.FMT_S16, N.MEM_HOST, N.MEM_HOST, N.LOUD_NORM_LOUDNESS)
    assert cost.tolist() == [512, 8, 2 + 4, 3648, 8, 1 << 24]
    assert N.loudness_cost(N.FMT_F32, N.MEM_DEVICE, N.MEM_HOST, N.LOUD_MEASURE)[2] == 0


def test_block_count_is_numpys_round(N):
    for rate in L.RATES + (12345, 22050):
        B = int(np.ceil(0.4 * rate))
        assert N.loudness_blocks(B - 1, rate) == 0
        for n in range(B, B + 3 * B // 4):
            assert N.loudness_blocks(n, rate) == L.n_blocks(n, rate), (rate, n)
    assert [N.loudness_blocks(n, 16000) for n in (6400, 7199, 7200, 7201, 8799, 8800)] == [1, 1, 1, 2, 2, 3]


def _check_against_oracle(N, h, m):
    rec = dict(zip(N.LOUD_FIELDS, h["rec"]))
    assert h["status"] == N.CLIP_OK
    assert (rec["blocks"], rec["n1"], rec["n2"]) == (len(m["z"]), m["n1"], m["n2"])
    assert abs(rec["lufs"] - m["lufs"]) <= L.TOL_DB
    assert abs(rec["gamma_r"] - m["gamma_r"]) <= L.TOL_DB
    # float64 rounding through the high pass (poles at radius 0.99 and more): three decades above 1e-13 of the largest block
    assert np.all(np.abs(h["z"] - m["z"]) <= 1e-10 * m["z"].max())
    return rec


def test_host_executor_against_the_oracle(N):
    for i, (rate, x) in enumerate(L.shape_clips()):
        m = L.oracle(i)
        h = N.loudness_host(x, rate)
        if m is None:
            assert h["status"] == N.CLIP_TOO_SHORT and np.isnan(h["rec"]).all()
            continue
        rec = _check_against_oracle(N, h, m)
        assert rec["peak"] == float(np.abs(x).max()) and np.isnan(rec["gain"]) and h["out"] is None


def test_host_executor_gates_and_normalises(N):
    rate, x = L.gating_clip()
    m = L.oracle(-1)
    h = N.loudness_host(x, rate, mode=N.LOUD_NORM_LOUDNESS, target=-23.0)
    rec = _check_against_oracle(N, h, m)
    assert rec["blocks"] == 67 and rec["n1"] < 67 and rec["n2"] < rec["n1"]
    g = np.float32(10.0 ** ((-23.0 - rec["lufs"]) / 20.0))
    assert rec["gain"] == float(g) and h["out"].tobytes() == (g * x).tobytes()
    assert rec["peak_out"] == float(np.abs(h["out"]).max())
    assert abs(rec["lufs"] + 20.0 * np.log10(rec["gain"]) + 23.0) <= L.GAIN_ROUND_DB
    assert abs(L.measure(h["out"], rate)["lufs"] - (rec["lufs"] + 20.0 * np.log10(rec["gain"]))) <= L.TOL_DB
    p = N.loudness_host(x, rate, mode=N.LOUD_NORM_PEAK, target=-1.0)
    assert p["out"].tobytes() == L.normalize_peak(x, -1.0).tobytes()
    # int16 samples are value / 32768
    xi = np.round(x * 32767.0).astype(np.int16)
    a, b = N.loudness_host(xi, rate, mode=N.LOUD_NORM_LOUDNESS), N.loudness_host(xi.astype(np.float32) / np.float32(32768.0), rate, mode=N.LOUD_NORM_LOUDNESS)
    assert a["rec"].tobytes() == b["rec"].tobytes() and a["z"].tobytes() == b["z"].tobytes() and a["out"].tobytes() == b["out"].tobytes()


def test_host_executor_edge_clips(N):
    z = N.loudness_host(np.zeros(8000, np.float32), 16000, mode=N.LOUD_NORM_LOUDNESS)
    assert z["status"] == N.CLIP_OK and z["rec"][0] == -np.inf and z["rec"][7] == 1.0 and not z["out"].any()
    x = L.noise(8000, 1).copy()
    x[777] = np.nan
    bad = N.loudness_host(x, 16000, mode=N.LOUD_NORM_PEAK)
    assert bad["status"] == N.CLIP_NONFINITE and np.isnan(bad["rec"]).all()
    short = N.loudness_host(L.noise(100, 2), 16000, mode=N.LOUD_NORM_PEAK, target=-3.0)     # the peak form needs no block
    assert short["status"] == N.CLIP_OK and np.isnan(short["rec"][0])
    assert abs(20.0 * np.log10(float(np.abs(short["out"]).max())) + 3.0) <= 2 * L.GAIN_ROUND_DB


def test_python_refusals_need_no_device():
    from audio_feature_extraction_amd import loudness
    with pytest.raises(NotImplementedError):
        loudness.integrated_loudness(np.zeros((8000, 2), np.float32), 16000)
    with pytest.raises(ValueError):
        loudness.integrated_loudness(np.zeros(6399, np.float32), 16000)
    with pytest.raises(ValueError):
        loudness.Meter(16000).integrated_loudness(np.zeros(100, np.float32))
    with pytest.raises(ValueError):
        loudness.block_loudness(np.zeros(100, np.float32), 16000)
    with pytest.raises(ValueError):
        loudness.integrated_loudness(np.zeros(8000, np.int16), 16000)           # pyloudnorm: data must be floating point
    with pytest.raises(NotImplementedError):
        loudness.Meter(2000)
    with pytest.raises(NotImplementedError):
        loudness.Meter(16000, filter_class="DeMan")
    with pytest.raises(ValueError):
        loudness.Meter(16000, block_size=0.0)
    assert loudness.integrated_loudness_batch([], 16000) == [] and loudness.normalize_batch([], 16000) == ([], [])


def test_normalize_loudness_is_pyloudnorms_product():
    from audio_feature_extraction_amd import loudness
    x = L.noise(1000, 4)
    y = loudness.normalize_loudness(x, -18.0, -23.0)
    assert y.dtype == np.float32 and y.tobytes() == L.normalize_loudness(x, -18.0, -23.0).tobytes()
    with pytest.warns(UserWarning, match="clipped"):
        loudness.normalize_loudness(x, -40.0, -3.0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        loudness.normalize_loudness(x, -18.0, -23.0)


def test_extractor_returns_too_short_audio_unchanged(monkeypatch):
    """process_audio.py:143-147: pyloudnorm raises for audio shorter than a block and the audio is kept; the native call
    reports such a clip without touching a device buffer, so the rule is checked here with the device call replaced by the
    host build's answer for a batch of short clips"""
    from audio_feature_extraction_amd import AudioFeatureExtractor, _native, loudness

    class ShortOnly:
        def loudness_batch(self, samples, offsets, lengths, rates, block_size, mode, target, want_blocks=False):
            assert all(_native.loudness_blocks(int(n), int(r), block_size) == 0 for n, r in zip(lengths, rates))
            return {"rec": np.full((len(lengths), _native.LOUD_N), np.nan), "status": np.full(len(lengths), _native.CLIP_TOO_SHORT, np.int32),
                    "out": np.zeros(samples.size, np.float32), "offsets": np.asarray(offsets)}

    monkeypatch.setattr(loudness, "_ctx", lambda device: ShortOnly())
    ex = AudioFeatureExtractor(sr=16000)
    monkeypatch.setattr(ex, "_devices", lambda: [0])
    x = L.noise(6399, 9)
    y = ex.normalize_volume(x)
    assert y.dtype == np.float32 and y.tobytes() == x.tobytes()
    ys = ex.normalize_volume_batch([x, x[:10]], reference_level=-20.0)
    assert [v.tobytes() for v in ys] == [x.tobytes(), x[:10].tobytes()]


def test_loudness_check_program_is_clean():
    """the host executor and the design under AddressSanitizer + UBSan: a stand-alone program, nothing preloaded"""
    r = subprocess.run(["make", "-C", CSRC, "loudness-check"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "loudness_check: ok" in r.stdout
