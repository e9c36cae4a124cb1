"""What the whole-clip DFT and the PESQ-like score are checked against: the numpy restatement of the reference's
``calculate_pesq_alternative`` (audio_quality_assessment.py:150-201), the pairs the tests run, and the yardsticks.

Truth.  ``scipy.fft.fft`` of the signal as ``np.longdouble`` (the 80-bit format where numpy has it: eps 1.1e-19).
Yardstick e_ref(N): the relative L2 error of ``np.fft.fft(x.astype(float64))`` -- what the reference itself runs --
against that truth, measured at import for every length below; where ``np.longdouble`` is no wider than float64 the
values measured on an x86-64 machine (MEASURED_E_REF) stand in, and the float64 transform is the truth.

Transform bound.  bound(N) = 8 max(e_ref(N), 2^-52): Bluestein does three transforms of M >= 2 N - 1 points and three
chirp products where pocketfft does one transform of N points -- about four times the rounding steps per output -- with
a factor of two to spare.

spec_dist tolerance.  bound(N) kappa with kappa = mean_k[(|R|_2 + |D|_2 + |R|_2 |R_k - D_k| / (R_k + 1e-10)) / (R_k + 1e-10)]
from the truth: the first-order effect of an error of bound(N) |.|_2 in every bin.  Every pair handed out satisfies
bound(N) kappa <= 1e-9 (asserted in ``pairs``), so an ill-conditioned pair cannot widen its own tolerance."""
import functools

import numpy as np
import scipy.fft

LENGTHS = (1, 2, 3, 5, 97, 2048, 2049, 4096, 4097, 8000, 22050, 65537, 220500)
SEED = 22
CONDITION_CAP = 1e-9
HAS_LONGDOUBLE = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
# e_ref of the reference clips below, measured with numpy 2.2 (pocketfft) against the 80-bit truth on x86-64
MEASURED_E_REF = {1: 0.0, 2: 0.0, 3: 5.6e-17, 5: 4.4e-17, 97: 2.1e-16, 2048: 2.1e-16, 2049: 5.4e-16, 4096: 2.4e-16, 4097: 5.4e-16,
                  8000: 2.7e-16, 22050: 3.2e-16, 65537: 9.8e-16, 220500: 3.5e-16}


# ---- the restatement of :150-201 ----
def spec_dist(reference, degraded) -> float:
    n = min(len(reference), len(degraded))
    reference, degraded = np.asarray(reference)[:n], np.asarray(degraded)[:n]
    ref_spec = np.abs(np.fft.fft(reference.astype(np.float64)))         # numpy 1.x: a float32 input is transformed in float64
    deg_spec = np.abs(np.fft.fft(degraded.astype(np.float64)))
    return np.mean(np.abs(ref_spec - deg_spec) / (ref_spec + 1e-10))


def pesq_score(snr, correlation, dist):
    """:186-199, with Python's min and max as there"""
    snr_score = min(max((snr - 5) / 35, 0), 1)
    corr_score = max(correlation, 0)
    spec_score = 1 - min(dist, 1)
    return 1.0 + 3.5 * (0.4 * snr_score + 0.4 * corr_score + 0.2 * spec_score)


def pesq_like(reference, degraded) -> dict:
    """calculate_pesq_alternative on the signals as they are (float32 arithmetic where numpy's is)"""
    n = min(len(reference), len(degraded))
    reference, degraded = np.asarray(reference)[:n], np.asarray(degraded)[:n]
    noise = degraded - reference
    signal_power, noise_power = np.mean(reference ** 2), np.mean(noise ** 2)
    snr = 10 * np.log10(signal_power / noise_power) if noise_power > 0 else 100
    with np.errstate(all="ignore"):
        correlation = np.corrcoef(reference, degraded)[0, 1]
    dist = spec_dist(reference, degraded)
    return {"snr": snr, "correlation": correlation, "spec_dist": dist, "pesq": pesq_score(snr, correlation, dist)}


# ---- the truth and the yardsticks ----
def truth_fft(x) -> np.ndarray:
    """the DFT of a real signal as exactly as this machine's numpy can"""
    if HAS_LONGDOUBLE:
        return scipy.fft.fft(np.asarray(x).astype(np.longdouble))
    return np.fft.fft(np.asarray(x).astype(np.float64))


def rel_l2(got, want) -> float:
    want = np.asarray(want)
    den = np.sqrt(np.sum(np.abs(want) ** 2))
    num = np.sqrt(np.sum(np.abs(np.asarray(got).astype(want.dtype) - want) ** 2))
    return float(num / den) if den else float(num)


@functools.lru_cache(maxsize=None)
def _generated():
    rng = np.random.default_rng(SEED)
    out = []
    for n in LENGTHS:
        r = (0.1 * rng.standard_normal(n)).astype(np.float32)
        d = (r + 0.02 * rng.standard_normal(n)).astype(np.float32)
        out.append((r, d))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _truths():
    return tuple((truth_fft(r), truth_fft(d)) for r, d in _generated())


@functools.lru_cache(maxsize=None)
def e_ref_table() -> dict:
    if not HAS_LONGDOUBLE:
        return dict(MEASURED_E_REF)
    return {n: rel_l2(np.fft.fft(r.astype(np.float64)), R) for n, (r, _), (R, _) in zip(LENGTHS, _generated(), _truths())}


def bound(n: int) -> float:
    return 8.0 * max(e_ref_table()[n], 2.0 ** -52)


def bound_for(x) -> float:
    """the transform bound of a clip that is not one of LENGTHS' own: from its own e_ref, measured here; without a wider
    longdouble, from the largest e_ref of the table"""
    if not HAS_LONGDOUBLE:
        return 8.0 * max(MEASURED_E_REF.values())
    x = np.asarray(x)
    return 8.0 * max(rel_l2(np.fft.fft(x.astype(np.float64)), truth_fft(x)), 2.0 ** -52)


def kappa(R, D) -> float:
    """the conditioning of spec_dist against a per-bin error relative to the spectrum's L2 norm, from the true spectra"""
    R, D = np.abs(R), np.abs(D)
    nr, nd = np.sqrt(np.sum(R * R)), np.sqrt(np.sum(D * D))
    return float(np.mean((nr + nd + nr * np.abs(R - D) / (R + 1e-10)) / (R + 1e-10)))


@functools.lru_cache(maxsize=None)
def pairs():
    """One dict per length: n, r, d (float32), R, D (the true spectra), bound, spec_dist (from the truth), tol."""
    out = []
    for n, (r, d), (R, D) in zip(LENGTHS, _generated(), _truths()):
        aR, aD = np.abs(R), np.abs(D)
        tol = bound(n) * kappa(R, D)
        assert tol <= CONDITION_CAP, (n, tol)
        out.append({"n": n, "r": r, "d": d, "R": R, "D": D, "bound": bound(n), "tol": tol,
                    "spec_dist": float(np.mean(np.abs(aR - aD) / (aR + 1e-10)))})
    return tuple(out)


def pesq_exact(reference, degraded, dist) -> float:
    """The restatement's weighting (pesq_score) of the pair's exactly evaluated terms: snr and correlation as
    tests/assess_ref.pair_exact forms them (math.fsum over the float32 inputs, the difference in float32 as numpy's is)
    and ``dist``, the spectral distance from the truth.  This is what the device's score is held to: numpy's own float32
    means lie 1e-7 from these, which is no property of the score."""
    from tests import assess_ref
    ex = assess_ref.pair_exact(reference, degraded)
    return pesq_score(ex["snr"], ex["correlation"], dist)


def as_s16(y) -> np.ndarray:
    return np.clip(np.round(np.asarray(y, np.float64) * 32768.0), -32768, 32767).astype(np.int16)
