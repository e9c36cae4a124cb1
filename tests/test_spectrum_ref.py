"""Known answers for the numpy restatement of calculate_pesq_alternative (tests/spectrum_ref.py) and for its yardsticks.
CPU only."""
import numpy as np

from tests import spectrum_ref as S


def test_identical_signals():
    y = (0.1 * np.random.default_rng(1).standard_normal(3001)).astype(np.float32)
    got = S.pesq_like(y, y)
    assert got["spec_dist"] == 0 and got["snr"] == 100 and got["pesq"] == 4.5


def test_an_impulse_has_a_flat_spectrum():
    """|fft(delta)| = 1 in every bin: against a silent signal every bin's term is 1 / (1 + 1e-10), against itself
    doubled it is 1 / (1 + 1e-10) too"""
    n = 97
    imp = np.zeros(n, np.float32)
    imp[13] = 1.0
    assert np.allclose(np.abs(np.fft.fft(imp.astype(np.float64))), 1.0, atol=1e-15)
    assert abs(S.spec_dist(imp, np.zeros(n, np.float32)) - 1 / (1 + 1e-10)) <= 1e-15
    assert abs(S.spec_dist(imp, 2 * imp) - 1 / (1 + 1e-10)) <= 1e-15


def test_a_bin_centred_tone_against_itself_scaled():
    """cos(2 pi j / 4) = 1, 0, -1, 0, ... has only the values 0 and +-1, so its DFT is exact: n / 2 in the two tone bins and
    exactly 0 elsewhere (a zero bin adds 0 / 1e-10 = 0).  Against itself scaled by g the two tone bins give
    (1 - g) (n / 2) / (n / 2 + 1e-10) each."""
    g = 0.75
    for n in (4, 8, 64):
        t = np.tile(np.array([1.0, 0.0, -1.0, 0.0], np.float32), n // 4)
        R = np.abs(np.fft.fft(t.astype(np.float64)))
        assert R[n // 4] == n / 2 and R[n - n // 4] == n / 2 and np.count_nonzero(R) == 2
        want = 2 * (1 - g) * (n / 2) / (n / 2 + 1e-10) / n
        assert abs(S.spec_dist(t, np.float32(g) * t) - want) <= 1e-16
    # a constant signal: bin 0 only
    assert abs(S.spec_dist(np.ones(64, np.float32), np.full(64, g, np.float32)) - (1 - g) * 64 / (64 + 1e-10) / 64) <= 1e-16


def test_a_constant_reference_is_nan():
    c = np.full(500, 0.25, np.float32)
    y = (0.1 * np.random.default_rng(2).standard_normal(500)).astype(np.float32)
    got = S.pesq_like(c, y)
    assert np.isnan(got["correlation"]) and np.isnan(got["pesq"])
    assert np.isnan(S.pesq_score(20.0, float("nan"), 0.3)) and np.isnan(S.pesq_score(20.0, 0.5, float("nan")))
    assert S.pesq_score(100, 1.0, 0.0) == 4.5 and S.pesq_score(-3.0, -0.2, 7.0) == 1.0


def test_the_yardsticks():
    assert S.LENGTHS == (1, 2, 3, 5, 97, 2048, 2049, 4096, 4097, 8000, 22050, 65537, 220500)
    assert set(S.MEASURED_E_REF) == set(S.LENGTHS)
    P = S.pairs()
    assert [p["n"] for p in P] == list(S.LENGTHS)
    for p in P:
        assert p["r"].dtype == p["d"].dtype == np.float32 and p["r"].size == p["n"]
        assert p["bound"] == 8 * max(S.e_ref_table()[p["n"]], 2.0 ** -52) and p["bound"] <= 8e-15
        assert 0 < p["tol"] <= S.CONDITION_CAP and 0.05 < p["spec_dist"] < 0.5
        # the restatement itself (float64 pocketfft) lies within its own yardstick of the truth
        assert abs(S.spec_dist(p["r"], p["d"]) - p["spec_dist"]) <= p["tol"]
    if S.HAS_LONGDOUBLE:                                 # the committed table is what this generator measures
        for n, e in S.e_ref_table().items():
            assert e <= 4 * max(S.MEASURED_E_REF[n], 2.0 ** -53), (n, e)
