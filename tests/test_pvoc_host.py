"""Host-side tests of phase_vocoder / time_stretch: afx_pvoc_frames, afx_time_stretch_samples, the cost records and
afx_pvoc_host through ctypes against the oracle (tests/pvoc_ref.py), the ABI's new symbols, and the argument errors of the
Python front end, which are raised before any device work.  CPU only.

afx_pvoc_host against the float64 truth, bounded at 4 x the oracle's own float32-magnitude form (the rule of the GPU test),
over the seven rates as yardstick -> bound; host (libm agrees with numpy to the three digits printed):
  16 / 4 random          9.5e-8 .. 1.5e-7 -> 3.8e-7 .. 6.1e-7; host 9.5e-8 .. 1.5e-7
  1024 / 256 make_clip   8.2e-8 .. 1.4e-7 -> 3.3e-7 .. 5.7e-7; host 8.2e-8 .. 1.4e-7
"""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import pvoc_ref as P
from tests import stft_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio_feature_extraction_amd", "csrc")
HOST_ONLY = ("afx_pvoc_frames", "afx_time_stretch_samples", "afx_pvoc_cost", "afx_time_stretch_cost", "afx_pvoc_host")
DEVICE = ("afx_pvoc_batch", "afx_time_stretch_batch")
RATES = (1.0, 0.5, 2.0, 0.8, 1.25, 3.7, 1.0 / 3.0)
TINY64 = np.finfo(np.float64).tiny


@pytest.fixture(scope="module")
def N():
    from audio_feature_extraction_amd import _native
    return _native


def test_symbols_are_declared_bound_and_stubbed(N):
    header = open(os.path.join(ROOT, "include", "afx.h")).read()
    stubs = open(os.path.join(CSRC, "afx_host_stubs.cpp")).read()
    for name in HOST_ONLY + DEVICE:
        assert name in N.SYMBOLS
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert hasattr(N.lib(), name)
        assert bool(re.search(r"\bint\s+" + name + r"\s*\(", stubs)) == (name in DEVICE), name
    assert re.search(r"#define\s+AFX_VERSION\s+107\b", header)                  # found by their presence
    assert re.search(r"AFX_PVOC_TILE = %d\b" % N.PVOC_TILE, header)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    asan_srcs = re.search(r"^ASAN_SRCS := (.*)$", mk, re.M).group(1)
    assert "afx_pvoc_host.cpp" in asan_srcs and "afx_pvoc.hip" not in asan_srcs
    assert "afx_pvoc.o" in mk and "afx_pvoc_host.o" in mk and "pvoc-check:" in mk


def test_frames_and_lengths_against_numpy_and_round(N):
    for rate in RATES + (0.1, 7.0):
        for T in list(range(0, 70)) + [199, 1000]:
            T_out, st = N.pvoc_frames(16, 4, T, rate)
            if T == 0:
                assert (T_out, st) == (0, N.CLIP_TOO_SHORT)
            else:
                assert (T_out, st) == (np.arange(0, T, rate).size, N.CLIP_OK), (T, rate)
    assert N.pvoc_frames(2048, 512, 44, 0.8) == (55, N.CLIP_OK)
    for n, hop, center, pad_mode in ((2048, 512, True, "constant"), (1024, 256, True, "reflect"), (2048, 441, False, "constant")):
        o = N.stft_opts(n, hop, center, pad_mode)
        for L in (0, 1, 3, 5, 7, n // 2, n // 2 + 1, n - 1, n, 9000, 22050):
            for rate in RATES:
                T, T_out, n_out, st = N.time_stretch_samples(o, L, rate)
                want_T = R.n_frames(L, n, hop, center, pad_mode)
                if want_T is None:
                    assert (T, T_out, n_out, st) == (0, 0, 0, N.CLIP_TOO_SHORT)
                    continue
                assert st == N.CLIP_OK and T == want_T and T_out == P.steps(T, rate)[0]
                assert n_out == round(L / rate) == P.stretch_length(L, rate), (L, rate)
    o = N.stft_opts(2048, 512)
    assert [N.time_stretch_samples(o, L, 2.0)[2] for L in (1, 3, 5, 7)] == [0, 2, 2, 4]      # the ties go to even


def _rel(A, B):
    top = np.abs(B).max(axis=0, keepdims=True)
    err = np.abs(A - B)
    assert not err[:, top[0] == 0].any()
    return float((err / np.maximum(top, TINY64)).max())


@pytest.mark.parametrize("n,hop", [(16, 4), (1024, 256)])
def test_pvoc_host_against_the_oracle(N, n, hop):
    if n == 16:
        rng = np.random.default_rng(3)
        D = (rng.standard_normal((9, 70)) + 1j * rng.standard_normal((9, 70))).astype(np.complex64)
        D[:, 20] = 0                                                          # a zero column: zeros out where both are
        D[:, 21] = 0
    else:
        D = R.stft(R.make_clip(7000, seed=2), n, hop, f32=True)
    for rate in RATES:
        out, st = N.pvoc_host(D, rate, hop, n)
        assert st == N.CLIP_OK and out.dtype == np.complex64 and out.flags.f_contiguous
        P64 = P.phase_vocoder(D, rate=rate, hop_length=hop, n_fft=n, exact=True)
        assert out.shape == P64.shape
        yard = _rel(P.phase_vocoder(D, rate=rate, hop_length=hop, n_fft=n, f32=True), P64)
        host = _rel(out, P64)
        print(f"pvoc_host {n}/{hop} rate {rate:.3g}: yardstick {yard:.3g} -> bound {4 * yard:.3g}; host {host:.3g}")
        assert yard > 0 and host <= 4 * yard
    if n == 16:
        assert not N.pvoc_host(D, 0.5, hop, n)[0][:, 40:43].any()             # steps 40 .. 42 mix columns 20 and 21 only


def test_statuses(N):
    D = np.ones((9, 6), np.complex64)
    out, st = N.pvoc_host(D[:, :0], 1.0, 4, 16)
    assert out is None and st == N.CLIP_TOO_SHORT
    bad = D.copy()
    bad[4, 5] = complex(0.0, np.nan)
    out, st = N.pvoc_host(bad, 0.5, 4, 16)
    assert st == N.CLIP_NONFINITE and out.shape == (9, 12) and not out.any()
    bad[4, 5] = complex(np.inf, 0.0)
    assert N.pvoc_host(bad, 2.0, 4, 16)[1] == N.CLIP_NONFINITE
    o = N.stft_opts(2048, 512, True, "reflect")
    assert N.time_stretch_samples(o, 1024, 0.8)[3] == N.CLIP_TOO_SHORT        # n_fft / 2 samples under reflect padding
    assert N.time_stretch_samples(o, 1025, 0.8)[3] == N.CLIP_OK


def test_unsupported_shapes_and_invalid_arguments(N):
    for rate in (0.0, -1.0, np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError):
            N.pvoc_frames(16, 4, 10, rate)
        with pytest.raises(ValueError):
            N.time_stretch_samples(N.stft_opts(2048, 512), 5000, rate)
        with pytest.raises(ValueError):
            N.pvoc_host(np.ones((9, 3), np.complex64), rate, 4, 16)
    for n, hop in ((15, 4), (0, 1), (4098, 1024), (16, 0), (16, 17)):
        with pytest.raises(NotImplementedError):
            N.pvoc_frames(n, hop, 10, 1.0)
    with pytest.raises(NotImplementedError):
        N.pvoc_cost(4098)
    with pytest.raises(NotImplementedError):
        N.pvoc_frames(4096, 1024, 1 << 31, 1.0)                                # T_out x bins >= 2^31
    with pytest.raises(NotImplementedError):
        N.pvoc_frames(16, 4, 1000, 1e-9)
    with pytest.raises(NotImplementedError):
        N.time_stretch_samples(N.stft_opts(512, 128), 5000, 1.0)
    with pytest.raises(NotImplementedError):
        N.time_stretch_cost(N.stft_opts(512, 128))
    with pytest.raises(ValueError):
        N.pvoc_cost(16, mem=7)
    with pytest.raises(ValueError):
        N.pvoc_frames(16, 4, -1, 1.0)


def test_costs_cover_the_workspace_and_cut_chunks(N):
    for n in (16, 1024, 2048):
        bins = n // 2 + 1
        cost = N.pvoc_cost(n)                                                  # host in, host out
        assert cost[0] == 0 and cost[1] == 0
        for T, T_out in ((1, 1), (10, 30), (100, 27), (33, 33)):
            w = T + T_out
            tiles = -(-T_out // N.PVOC_TILE)
            assert w * cost[2] + cost[3] >= T * bins * (8 + 12) + T_out * bins * 8 + tiles * bins * 8, (n, T, T_out)
        assert N.pvoc_cost(n, N.MEM_DEVICE, N.MEM_DEVICE)[2] == cost[2] - 16 * bins
    for n, hop in ((1024, 256), (2048, 441)):
        o = N.stft_opts(n, hop)
        bins = n // 2 + 1
        cost = N.time_stretch_cost(o)
        for L in (1, n, 9000, 40000):
            for rate in (0.5, 0.8, 2.0):
                T, T_out, n_out, _ = N.time_stretch_samples(o, L, rate)
                w = T + T_out + -(-L // hop) + -(-n_out // hop)
                tiles = -(-T_out // N.PVOC_TILE)
                need = 8 * L + T * bins * 20 + T_out * (bins * 8 + n * 4) + tiles * bins * 8 + 8 * (n_out + 3)
                assert w * cost[2] + cost[3] >= need, (n, L, rate)
    cost = N.pvoc_cost(16)
    w = [100, 1, 0, 50, 100, 7]
    clip = [int(x * cost[2] + cost[3]) for x in w]
    assert list(N.stft_chunks(w, cost, 2 << 30)) == [0, 0, -1, 0, 0, 0]
    assert list(N.stft_chunks(w, cost, clip[0])) == [0, 1, -1, 1, 2, 3]


def test_front_end_errors_come_before_any_device_work():
    """None of these reaches a device: the suite's CPU half has none to reach."""
    import audio_feature_extraction_amd as pkg
    from audio_feature_extraction_amd import effects
    from audio_feature_extraction_amd.core import spectrum as S
    assert pkg.phase_vocoder is S.phase_vocoder
    assert pkg.__all__ == ["AudioFeatureExtractor", "FeatureEvaluator"]
    D = np.ones((1025, 4), np.complex64)
    y = np.zeros(4096, np.float32)
    for rate in (0, -2.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="rate"):
            S.phase_vocoder(D, rate=rate)
        with pytest.raises(ValueError, match="rate"):
            effects.time_stretch(y, rate=rate)
        with pytest.raises(ValueError, match="rate"):
            S.phase_vocoder_batch([D, D], [1.0, rate])
        with pytest.raises(ValueError, match="rate"):
            effects.time_stretch_batch([y, y], [rate, 1.0])
    with pytest.raises(NotImplementedError):
        S.phase_vocoder(D, rate=1.0, n_fft=2047)                                # odd n_fft
    with pytest.raises(NotImplementedError):
        S.phase_vocoder(np.ones((8, 4), np.complex64), rate=1.0, n_fft=15)
    with pytest.raises(NotImplementedError):
        S.phase_vocoder(D, rate=1.0, hop_length=0)
    with pytest.raises(NotImplementedError):
        S.phase_vocoder(D, rate=1.0, hop_length=2049)
    with pytest.raises(NotImplementedError):
        S.phase_vocoder(np.ones((4097, 2), np.complex64), rate=1.0)             # n_fft 8192
    with pytest.raises(NotImplementedError, match="mono"):
        S.phase_vocoder(np.ones((2, 1025, 4), np.complex64), rate=1.0)
    with pytest.raises(ValueError):
        S.phase_vocoder(D, rate=1.0, n_fft=1024)                                # 1025 rows are not 513
    with pytest.raises(ValueError):
        S.phase_vocoder_batch([D, D], [1.0])
    with pytest.raises(NotImplementedError):
        effects.time_stretch(y, rate=0.8, n_fft=512)
    with pytest.raises(NotImplementedError):
        effects.time_stretch(y, rate=0.8, hop_length=0)
    with pytest.raises(ValueError):
        effects.time_stretch(y, rate=0.8, pad_mode="wrap")
    with pytest.raises(NotImplementedError, match="mono"):
        effects.time_stretch(np.zeros((2, 4096), np.float32), rate=0.8)
    with pytest.raises(ValueError):
        effects.time_stretch_batch([y, y], [0.8])
    ex = pkg.AudioFeatureExtractor()
    for n in (0, -5):
        with pytest.raises(ValueError):
            ex.stretch_to_length(y, n)
    assert S.phase_vocoder_batch([], []) == [] and effects.time_stretch_batch([], []) == []


def test_pvoc_check_program_is_clean():
    """the frame and length rules, the cost records and one clip through afx_pvoc_host under AddressSanitizer + UBSan: a
    stand-alone program, nothing preloaded"""
    r = subprocess.run(["make", "-C", CSRC, "pvoc-check"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "pvoc_check: ok" in r.stdout
