"""Host-side tests of spectral gating: afx_gate_params and afx_gate_cost through ctypes against the numbers of the float64
oracle (tests/gate_ref.py), the ABI's new symbols, and the argument errors of the Python front ends, which are raised before
any device work.  CPU only."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import gate_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio_feature_extraction_amd", "csrc")


@pytest.fixture(scope="module")
def N():
    from audio_feature_extraction_amd import _native
    return _native


def test_symbols_are_declared_bound_and_stubbed(N):
    header = open(os.path.join(ROOT, "include", "afx.h")).read()
    stubs = open(os.path.join(CSRC, "afx_host_stubs.cpp")).read()
    for name in ("afx_gate_params", "afx_gate_cost", "afx_gate_batch"):
        assert name in N.SYMBOLS
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert hasattr(N.lib(), name)
        assert bool(re.search(r"\bint\s+" + name + r"\s*\(", stubs)) == (name == "afx_gate_batch"), name
    assert re.search(r"#define\s+AFX_VERSION\s+107\b", header)                  # found by their presence
    assert re.search(r"\bAFX_CLIP_TOO_LONG = %d\b" % N.CLIP_TOO_LONG, header)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    asan_srcs = re.search(r"^ASAN_SRCS := (.*)$", mk, re.M).group(1)
    assert "afx_gate_host.cpp" in asan_srcs and "afx_gate.hip" not in asan_srcs
    assert "afx_gate.o" in mk and "afx_gate_host.o" in mk and "gate-check:" in mk


@pytest.mark.parametrize("sr", [16000, 22050, 44100])
@pytest.mark.parametrize("n_fft", [1024, 2048])
def test_params_against_the_oracle(N, sr, n_fft):
    hop = n_fft // 4
    o = N.gate_opts(sr, n_fft=n_fft)
    p = N.gate_params(o, 32000)
    n_f, n_t = G.smooth_sizes(sr, n_fft, hop)
    assert (p["n_f"], p["n_t"], p["smooth"]) == (n_f, n_t, True)
    assert abs(p["beta"] - G.beta(sr, hop)) <= 1e-15 * G.beta(sr, hop)
    F = G.smoothing_filter(n_f, n_t)
    assert p["taps_f"].shape == (2 * n_f + 1,) and p["taps_t"].shape == (2 * n_t + 1,)
    assert np.abs(np.outer(p["taps_f"], p["taps_t"]) - F).max() <= 4e-16 * F.max()
    for length in (0, 1, hop - 1, hop, 32000, 600000, (1 << 20) - 60000):
        assert N.gate_params(o, length)["frames"] == G.n_frames(length, hop)
    assert N.gate_params(N.gate_opts(sr, n_fft=n_fft, padding=0), 1000)["frames"] == 1 + 1000 // hop
    assert N.gate_params(N.gate_opts(sr, n_fft=n_fft, time_constant_s=0.5), 0)["beta"] == pytest.approx(G.beta(sr, hop, 0.5), rel=1e-15)


def test_known_filter_sizes(N):
    assert [(N.gate_params(N.gate_opts(sr, n_fft=n))["n_f"], N.gate_params(N.gate_opts(sr, n_fft=n))["n_t"])
            for sr, n in ((16000, 1024), (16000, 2048), (22050, 1024))] == [(16, 3), (32, 1), (11, 4)]
    p = N.gate_params(N.gate_opts(16000, freq_mask_smooth_hz=31.25, time_mask_smooth_ms=16.0))
    assert (p["n_f"], p["n_t"], p["smooth"]) == (1, 1, False)
    p = N.gate_params(N.gate_opts(16000, n_fft=512, hop_length=100))          # any framing: the numbers need no kernel
    assert (p["n_f"], p["n_t"]) == G.smooth_sizes(16000, 512, 100)


def test_invalid_and_unsupported_arguments(N):
    for kw in (dict(sr=8000, n_fft=2048),                                       # a frame lasts 64 ms: n_t = 0
               dict(sr=16000, freq_mask_smooth_hz=31.0), dict(sr=16000, time_mask_smooth_ms=15.9),
               dict(sr=16000, prop_decrease=1.5), dict(sr=16000, prop_decrease=-0.1), dict(sr=16000, prop_decrease=float("nan")),
               dict(sr=16000, time_constant_s=0.0), dict(sr=0), dict(sr=16000, padding=-1), dict(sr=16000, chunk_size=0),
               dict(sr=16000, n_std_thresh_stationary=float("inf")), dict(sr=16000, n_fft=1023)):
        with pytest.raises(ValueError):
            N.gate_params(N.gate_opts(**kw))
    for kw in (dict(sr=16000, win_length=512), dict(sr=16000, freq_mask_smooth_hz=5000.0), dict(sr=16000, padding=(1 << 20) + 1),
               dict(sr=16000, chunk_size=(1 << 24) + 1)):
        with pytest.raises(NotImplementedError):
            N.gate_params(N.gate_opts(**kw))
    with pytest.raises(NotImplementedError):
        N.gate_cost(N.gate_opts(16000, n_fft=512))
    with pytest.raises(ValueError):
        N.gate_cost(N.gate_opts(16000), fmt=7)


@pytest.mark.parametrize("n_fft,stationary", [(1024, True), (1024, False), (2048, True), (2048, False)])
def test_cost_covers_the_workspace_and_cuts_chunks(N, n_fft, stationary):
    o = N.gate_opts(16000, n_fft=n_fft, stationary=stationary)
    cost = N.gate_cost(o)
    hop, pitch, words = n_fft // 4, (n_fft // 2 + 1 + 15) // 16 * 16, (n_fft // 2 + 1 + 31) // 32
    frame = 8 * pitch + (4 * pitch + 4 * words if stationary else 8 * pitch) + 4 * n_fft
    for L in (1, 255, 512, 32000, 600000):
        T = G.n_frames(L, hop)
        assert (1 + L // 512) * cost[0] + cost[3] >= T * frame, L              # every frame of the grid is paid for
    assert cost[2] == 12 and N.gate_cost(o, N.FMT_S16, N.MEM_HOST, N.MEM_DEVICE, True)[2] == 12
    assert N.gate_cost(o, N.FMT_F32, N.MEM_DEVICE, N.MEM_DEVICE)[2] == 4
    lengths = [32000, 1, 0, 5000, 32000, 700]
    clip = [int((1 + L // 512) * cost[0] + L * cost[2] + cost[3]) for L in lengths]

    def cut(budget):                                                           # the rule of afx_stft_chunks, restated
        out, chunk, used = [], 0, 0
        for L, b in zip(lengths, clip):
            if L == 0:
                out.append(-1)
                continue
            if used and used + b > budget:
                chunk, used = chunk + 1, 0
            out.append(chunk)
            used += b
        return out

    assert list(N.stft_chunks(lengths, cost, 2 << 30)) == [0, 0, -1, 0, 0, 0]
    assert list(N.stft_chunks(lengths, cost, clip[0])) == cut(clip[0]) == [0, 1, -1, 2, 3, 4]   # the padding's frames weigh most
    for budget in (clip[0] + clip[1], 3 * clip[0]):
        assert list(N.stft_chunks(lengths, cost, budget)) == cut(budget)
    assert cut(3 * clip[0])[-1] >= 1


def test_front_end_errors_come_before_any_device_work():
    """None of these reaches a device: the suite's CPU half has none to reach."""
    from audio_feature_extraction_amd import AudioFeatureExtractor, effects
    y = np.zeros(1000, np.float32)
    for kw, word in ((dict(use_torch=True), "use_torch"), (dict(n_jobs=2), "n_jobs"), (dict(tmp_folder="/x"), "tmp_folder"),
                     (dict(win_length=512), "win_length"), (dict(n_fft=512), "n_fft"), (dict(n_fft=1024, hop_length=128), "hop_length")):
        with pytest.raises(NotImplementedError, match=word):
            effects.reduce_noise(y, 16000, **kw)
    with pytest.raises(NotImplementedError, match="chunk_size"):
        effects.reduce_noise(np.zeros(600001, np.float32), 16000)
    with pytest.raises(NotImplementedError, match="mono"):
        effects.reduce_noise(np.zeros((2, 100), np.float32), 16000)
    with pytest.raises(ValueError):
        effects.reduce_noise(y, 8000, n_fft=2048)
    with pytest.raises(ValueError):
        effects.reduce_noise(np.zeros(0, np.float32), 16000)
    with pytest.raises(ValueError):
        effects.reduce_noise(y, 16000, y_noise=np.zeros(0, np.float32), stationary=True)
    with pytest.raises(TypeError):
        effects.reduce_noise(y, 16000, no_such_keyword=1)
    assert effects.reduce_noise_batch([], 16000) == []
    ex = AudioFeatureExtractor(sr=16000)
    with pytest.raises(ValueError, match="method"):
        ex.apply_noise_reduction(y, method="median")
    with pytest.raises(NotImplementedError, match="chunk_size"):
        ex.process_recordings_batch([np.zeros(600001, np.float32)])
    with pytest.raises(ValueError):
        AudioFeatureExtractor(sr=8000).apply_noise_reduction(y, method="spectral")
    assert ex.process_recordings_batch([]) == ([], [])


def test_gate_check_program_is_clean():
    """the derived parameters and the cost record under AddressSanitizer + UBSan: a stand-alone program, nothing preloaded"""
    r = subprocess.run(["make", "-C", CSRC, "gate-check"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "gate_check: ok" in r.stdout
