"""numpy restatement of the recording screen and the denoising scores of the reference, the oracle of afx_assess_batch /
afx_compare_batch and of audio_feature_extraction_amd.quality:

  00_audio_data_collection_experiment/audio_format_assessment.py:143-300   detect_silence, check_volume_levels,
                                                                           check_amplitude_stability, estimate_snr
  00_audio_data_collection_experiment/audio_quality_assessment.py:93-116   estimate_snr
                                                               :235-280   calculate_stoi_alternative

Every function has two flows.  ``f32=True`` is librosa's own: a float32 signal gives float32 frame RMS values
(librosa.feature.rms returns the signal's type) and a float32 dB scale (librosa.amplitude_to_db keeps it), numpy's float32
means.  ``f32=False`` is the float64 truth the device is held to: the same expressions on the samples taken as float64.
The two can decide a frame differently only within rounding of the threshold; ``silence_is_robust`` says when they cannot."""
import math

import numpy as np

from oracle.cpu_ref import rms

AMIN = 1e-5                    # librosa.amplitude_to_db's amin
TOP_DB = 80.0
NOISE_CAP = 2000
RECORD = ("n_short", "silent", "longest_run", "max_rms_short", "mean_square", "peak", "noise_mean_square", "n_long",
          "rms_long_mean", "rms_long_std")


def _signal(y, f32):
    y = np.asarray(y)
    if y.dtype == np.int16:
        y = y.astype(np.float32) * np.float32(1.0 / 32768.0)          # wavio.to_float32
    return np.ascontiguousarray(y, np.float32 if f32 else np.float64)


def frame_lengths(sr: int):
    """(10 ms, 100 ms) frames of the screen at ``sr``: int(sr * 0.01), int(sr * 0.1)."""
    return int(sr * 0.01), int(sr * 0.1)


def frame_rms(y, frame_length: int, f32=False) -> np.ndarray:
    """librosa.feature.rms(y=y, frame_length=fl, hop_length=fl)[0]: 1 + (len + 2 (fl // 2) - fl) // fl centred frames, zero padding."""
    return rms(_signal(y, f32), frame_length, frame_length)[0]


def amplitude_to_db(S, top_db=TOP_DB) -> np.ndarray:
    """librosa.amplitude_to_db(S, ref=np.max): power_to_db(S**2, ref=max(S)**2, amin=AMIN**2, top_db) in S's type."""
    mag = np.abs(S)
    ref = np.max(mag) ** 2
    amin = AMIN ** 2
    log_spec = 10.0 * np.log10(np.maximum(amin, mag ** 2))
    log_spec = log_spec - 10.0 * np.log10(np.maximum(amin, ref))
    if top_db is not None:
        log_spec = np.maximum(log_spec, log_spec.max() - top_db)
    return log_spec


def silence_frames(y, sr: int, threshold_db=-40.0, f32=False) -> np.ndarray:
    return amplitude_to_db(frame_rms(y, frame_lengths(sr)[0], f32)) < threshold_db


def longest_run(flags) -> int:
    """The reference's scan (:172-193) in frames: a run that reaches the last frame counts."""
    best = run = 0
    for f in flags:
        run = run + 1 if f else 0
        best = max(best, run)
    return best


def detect_silence(y, sr: int, threshold_db=-40.0, f32=False) -> dict:
    fl = frame_lengths(sr)[0]
    s = silence_frames(y, sr, threshold_db, f32)
    ratio = np.mean(s)
    run = longest_run(s)
    dur = run * fl / sr if run else 0
    return {"silence_ratio": ratio, "max_silence_duration": dur, "silence_ok": bool(ratio < 0.3 and dur < 1.0),
            "n_short": int(s.size), "silent": int(s.sum()), "longest_run": run}


def check_volume_levels(y, f32=False) -> dict:
    y = _signal(y, f32)
    r = np.sqrt(np.mean(y ** 2))
    rms_dbfs = 20 * np.log10(r) if r > 0 else -100
    peak = np.max(np.abs(y))
    peak_dbfs = 20 * np.log10(peak) if peak > 0 else -100
    return {"rms_dbfs": rms_dbfs, "peak_dbfs": peak_dbfs, "volume_ok": bool(rms_dbfs > -30 and peak_dbfs < 0)}


def check_amplitude_stability(y, sr: int, f32=False) -> dict:
    r = frame_rms(y, frame_lengths(sr)[1], f32)
    std, mean = np.std(r), np.mean(r)
    cv = std / mean if mean > 0 else 0
    return {"rms_std": std, "rms_cv": cv, "stability_ok": bool(cv < 0.5)}


def snr_powers(y, f32=False):
    """(noise_power, signal_power) of estimate_snr; the noise power is NaN for fewer than 10 samples (an empty mean)."""
    y = _signal(y, f32)
    nw = min(int(len(y) * 0.1), NOISE_CAP)
    with np.errstate(all="ignore"):
        noise = np.mean(y[:nw] ** 2) if nw else np.float64(np.nan)
    return noise, np.mean(y ** 2)


def estimate_snr(y, f32=False) -> dict:
    noise, signal = snr_powers(y, f32)
    snr = 10 * np.log10((signal - noise) / noise) if noise > 0 and signal > noise else 0
    return {"snr": snr, "snr_ok": bool(snr >= 20)}


def assess(y, sr: int, threshold_db=-40.0, f32=False) -> dict:
    """The four checks' keys in quality.assess's order."""
    out = {}
    d = detect_silence(y, sr, threshold_db, f32)
    out.update({k: d[k] for k in ("silence_ratio", "max_silence_duration", "silence_ok")})
    out.update(check_volume_levels(y, f32))
    out.update(check_amplitude_stability(y, sr, f32))
    out.update(estimate_snr(y, f32))
    return out


def record(y, frame_short: int, frame_long: int, threshold_db=-40.0, noise_cap=NOISE_CAP) -> np.ndarray:
    """The AFX_ASSESS_N values of afx_assess_batch for one clip in the float64 truth (RECORD names them)."""
    y = _signal(y, False)
    rs, rl = frame_rms(y, frame_short), frame_rms(y, frame_long)
    s = amplitude_to_db(rs) < threshold_db
    nw = min(int(len(y) * 0.1), noise_cap)
    return np.array([rs.size, s.sum(), longest_run(s), rs.max(), np.mean(y ** 2), np.max(np.abs(y)),
                     np.mean(y[:nw] ** 2) if nw else np.nan, rl.size, np.mean(rl), np.std(rl)], np.float64)


def silence_is_robust(y, sr: int, threshold_db=-40.0, margin_db=0.01) -> bool:
    """True when, in the float64 truth, no frame lies within ``margin_db`` of the threshold and the clip's loudest frame is
    not within it of amin (where the reference level itself switches): the silence counts are then the same in every flow
    and are asserted exactly.  Every clip the tests use satisfies it."""
    r = frame_rms(y, frame_lengths(sr)[0])
    db = amplitude_to_db(r, top_db=None)
    if np.any(np.abs(db - threshold_db) <= margin_db):
        return False
    top = r.max()
    return top == 0 or abs(20 * math.log10(top) - 20 * math.log10(AMIN)) > margin_db


def snr_is_robust(y) -> bool:
    """True when estimate_snr's branch and its logarithm are well conditioned: the signal power is at least twice the noise
    power, or not above it (where the answer is 0 whatever the last bits say).  ``snr`` is asserted on such clips only: a
    steady tone, whose leading window has the clip's own power, is not one."""
    noise, signal = snr_powers(y)
    if not noise > 0:
        return True                                     # an empty or an all-zero window: snr = 0 in every flow
    return bool(signal >= 2 * noise or signal <= noise * (1 - 1e-6))


# ---- the scores of a reference / degraded pair ----
def pair_stats(reference, degraded, f32=False) -> dict:
    """correlation (np.corrcoef), mse and the SNR of the difference of calculate_stoi_alternative, over the shorter length."""
    r, d = _signal(reference, True), _signal(degraded, True)
    n = min(len(r), len(d))
    r, d = r[:n], d[:n]
    noise = d - r                                       # in float32, as the reference's arrays are
    e = r - d
    if not f32:
        r, d, noise, e = (a.astype(np.float64) for a in (r, d, noise, e))
    with np.errstate(all="ignore"):
        corr = np.corrcoef(r, d)[0, 1]
    mse = np.mean(e ** 2)
    sp, npow = np.mean(r ** 2), np.mean(noise ** 2)
    snr = 10 * np.log10(sp / npow) if npow > 0 else 100
    return {"correlation": corr, "mse": mse, "snr": snr}


def stoi_score(correlation, mse, snr):
    """The weighting of :267-278, with Python's max / min (max(nan, 0) is nan)."""
    corr_score = max(correlation, 0)
    mse_score = max(1 - mse * 10, 0)
    snr_score = min(max((snr - 5) / 35, 0), 1)
    return 0.5 * corr_score + 0.3 * mse_score + 0.2 * snr_score


def stoi_like(reference, degraded, f32=False):
    s = pair_stats(reference, degraded, f32)
    return stoi_score(s["correlation"], s["mse"], s["snr"])


def pair_exact(reference, degraded) -> dict:
    """pair_stats with every sum exact (math.fsum over the float32 inputs' float64 values; the last operations in
    longdouble): what numpy's own float64 error is measured against."""
    r, d = _signal(reference, True), _signal(degraded, True)
    n = min(len(r), len(d))
    r, d = r[:n], d[:n]
    e = (d - r).astype(np.float64)
    r, d = r.astype(np.float64), d.astype(np.float64)
    L = np.longdouble
    mr, md = L(math.fsum(r)) / n, L(math.fsum(d)) / n
    xr, xd = r.astype(L) - mr, d.astype(L) - md
    m2r, m2d, m2 = math.fsum(xr * xr), math.fsum(xd * xd), math.fsum(xr * xd)
    with np.errstate(all="ignore"):
        corr = float(L(m2) / np.sqrt(L(m2r)) / np.sqrt(L(m2d))) if m2r > 0 and m2d > 0 else float("nan")
    mse = float(L(math.fsum(e * e)) / n)
    sp = float(L(math.fsum(r * r)) / n)
    return {"correlation": corr, "mse": mse, "snr": 10 * math.log10(sp / mse) if mse > 0 else 100, "signal_power": sp}
