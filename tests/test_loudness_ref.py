"""The restatement tests/loudness_ref.py against the standard it restates (ITU-R BS.1770-4) and against the block and gating
rules of pyloudnorm it spells out, and the conditions the GPU tests rely on: the measured distance between its two forms (the
basis of the engine's tolerance) and the distance of every test clip's blocks from the gates.  CPU only; numpy and scipy."""
import numpy as np
import pytest

from tests import loudness_ref as L


def _tone(rate, seconds=5.0, freq=997.0):
    return np.sin(2.0 * np.pi * freq * np.arange(int(seconds * rate)) / rate).astype(np.float32)


def test_full_scale_997_hz_sine_reads_minus_3_01_lkfs():
    """BS.1770-4's compliance signal, within BS.1771's +-0.1 LU (the RBJ sections read -3.05 at 48 kHz, -3.08 at 16 kHz)"""
    for rate in (48000, 16000):
        assert abs(L.measure(_tone(rate), rate)["lufs"] - (-3.01)) <= 0.1, rate
    assert abs(L.measure(_tone(48000), 48000)["lufs"] - (-3.052)) < 1e-3


def test_scaling_by_minus_20_db_lowers_the_reading_by_20_db():
    x = L.noise(3 * 16000, 5).astype(np.float64)
    a, b = L.measure(x, 16000)["lufs"], L.measure(x * 10.0 ** (-20.0 / 20.0), 16000)["lufs"]
    assert abs((a - b) - 20.0) <= 1e-9


@pytest.mark.parametrize("n, blocks, end", [(6400, 1, 6400), (7199, 1, 6400), (7200, 1, 6400), (7201, 2, 8000), (8799, 2, 8000),
                                            (8800, 3, 9600)])
def test_block_count_and_last_block_end_at_16_khz(n, blocks, end):
    assert L.n_blocks(n, 16000) == blocks
    assert L.block_slices(n, 16000)[-1][1] == end
    assert len(L.measure(L.noise(n, 3), 16000)["z"]) == blocks          # a partial last block is still a block


def test_too_short_audio_raises():
    with pytest.raises(ValueError):
        L.measure(np.zeros(6399, np.float32), 16000)


def test_segment_boundaries_are_truncated_not_evenly_spaced():
    assert L.bounds(8, 11025) == [0, 1102, 2205, 3307, 4410, 5512, 6615, 7717]
    for rate in (8000, 11025, 12345, 16000, 22050, 44100, 48000):       # a block is four consecutive segments
        b = L.bounds(2004, rate)
        for j in range(2000):
            assert (int(0.4 * (j * 0.25) * rate), int(0.4 * (j * 0.25 + 1) * rate)) == (b[j], b[j + 4])


def test_gating_case():
    """2 s at sigma 0.1, 2 s of zeros, 1 s at 0.003, 2 s at 0.05: the absolute gate drops the blocks inside the silence,
    the relative gate those of the quiet second as well; the level is that of the blocks left"""
    rate, x = L.gating_clip()
    m = L.oracle(-1)
    assert len(m["z"]) == 67 and m["n1"] < 67 and m["n2"] < m["n1"]
    assert abs(m["lufs"] - (-19.73)) < 0.05
    # by hand: the blocks that lie wholly inside the silence (samples 32000 .. 64000), less the high pass's ringing
    silent = [j for j, (l, u) in enumerate(L.block_slices(x.size, rate)) if l >= 32000 + 1600 and u <= 64000]
    assert len(silent) >= 10 and all(m["l"][j] < -70.0 for j in silent)
    quiet = [j for j, (l, u) in enumerate(L.block_slices(x.size, rate)) if l >= 64000 and u <= 80000]
    assert quiet and all(-70.0 < m["l"][j] < m["gamma_r"] for j in quiet)
    kept = (m["l"] > m["gamma_r"]) & (m["l"] > -70.0)
    assert abs(m["lufs"] - (-0.691 + 10.0 * np.log10(m["z"][kept].mean()))) < 1e-12


def test_both_forms_agree_and_the_bound_is_four_times_their_distance():
    """the float32-faithful form (the reference's own arithmetic) against the float64 truth on every test clip"""
    worst = 0.0
    clips = list(L.shape_clips()) + [L.gating_clip()]
    for i, (rate, x) in enumerate(clips):
        m = L.oracle(i if i < len(clips) - 1 else -1)
        if m is None:
            assert x.size < 0.4 * rate
            continue
        f = L.measure(x, rate, faithful=True)
        assert (f["n1"], f["n2"]) == (m["n1"], m["n2"])
        worst = max(worst, abs(f["lufs"] - m["lufs"]))
    print("largest |faithful - float64| = %.3g dB; bound %.3g dB" % (worst, L.TOL_DB))
    assert 0.0 < worst <= L.BOUND_BASIS_DB and L.TOL_DB == 4 * L.BOUND_BASIS_DB


def test_every_test_clip_keeps_its_blocks_away_from_the_gates():
    n = len(L.shape_clips())
    both = 0
    for i in list(range(n)) + [-1]:
        m = L.oracle(i)
        if m is None:
            continue
        assert L.gate_margin(m) >= 1e-6, i
        both += m["n1"] < len(m["z"]) and m["n2"] < m["n1"]
    assert both >= 1                                                     # both gates are exercised
    refused = [i for i in range(n) if L.oracle(i) is None]
    assert len(refused) == len(L.RATES)                                  # the B - 1 clip of every rate


def test_normalised_clip_sits_at_the_target_to_the_rounding_of_the_gain():
    rate, x = L.shape_clips()[10]
    m = L.oracle(10)
    y = L.normalize_loudness(x, m["lufs"], -23.0)
    assert y.dtype == np.float32
    g = np.float32(10.0 ** ((-23.0 - m["lufs"]) / 20.0))
    assert abs(m["lufs"] + 20.0 * np.log10(float(g)) + 23.0) <= L.GAIN_ROUND_DB
    assert abs(L.measure(y, rate)["lufs"] - (m["lufs"] + 20.0 * np.log10(float(g)))) <= L.TOL_DB
    p = L.normalize_peak(x, -1.0)
    assert abs(20.0 * np.log10(float(np.abs(p).max())) + 1.0) <= 2 * L.GAIN_ROUND_DB
