"""Restatement and case lists for the sample-domain smoothers (afx_medfilt_batch, afx_savgol_batch) and the experiment
extractor's energy and ZCR groups (afx_energy_zcr_batch; 04_feature_extraction_experiment/feature_extractor.py:341-483).

The reference is scipy / numpy on ``x.astype(float64)`` of the same float32 clip.
  medfilt   value-exact: ``array_equal``.
  savgol    ``|got - ref| <= 2^-24 |ref| + 4 conditioning(case) max|x|``: one rounding to float32 of a float64 value that is
            itself only defined to the distance between two float64 evaluations of the same filter -- scipy's own and the
            centred pseudo-inverse through numpy (``savgol_second``).  The conditioning is asserted to be <= 1e-10: a
            condition on the inputs, not a tolerance.
  groups    scalars to rtol 1e-12 (absolute 1e-12 for the ZCR statistics: their values are sums of multiples of 1 / fl)
            against the numpy restatement below on the same float32 signal; crossing counts are equal on inputs for which
            ``zcr_is_robust`` holds.
No GPU and no native code is used here."""
import numpy as np
import scipy.signal

EPS24 = 2.0 ** -24
MAX_CONDITIONING = 1e-10

MED_KERNELS = (1, 3, 5, 25, 31)
SAVGOL_CASES = ((11, 3, 0), (5, 0, 0), (3, 2, 0), (9, 1, 1), (9, 2, 2), (31, 5, 0), (31, 5, 2))

GROUP_RATES = (22050, 16000)
GROUP_LENGTHS_PRE = (19, 63, 64, 65, 2047, 2048, 2049, 9 * 512 - 1, 9 * 512, 10 * 512, 16 * 512, 70 * 512 + 1)
GROUP_LENGTHS_RAW = (5, 11, 12)
FRAME_LENGTH, HOP_LENGTH = 2048, 512
REC_FIELDS = ("T", "fl", "hop", "energy_mean", "energy_std", "energy_p10", "zcr_mean", "zcr_std", "zcr_local_stability",
              "peak_smooth", "peak_in", "peak_filt")
FLAG_MARGIN = 1e-6


def _unique(ns):
    out = []
    for n in ns:
        if n >= 1 and n not in out:
            out.append(int(n))
    return tuple(out)


def med_lengths(K: int, tile: int):
    """the shortest clips, either side of the half window and of the window, either side of one tile, a halo past it, more
    than two and more than three tiles"""
    h = K // 2
    return _unique((1, 2, h, h + 1, K, tile - 1, tile, tile + 1, tile + h, 2 * tile + 1, 3 * tile + 17))


def savgol_lengths(W: int, tile: int):
    """the window itself (edges only), one interior output, the two edge fits just apart, and the tile lengths of
    med_lengths; W - 1 is refused and tested apart"""
    h = W // 2
    return _unique((W, W + 1, 2 * W - 1, tile - 1, tile, tile + 1, tile + h, 2 * tile + 1, 3 * tile + 17))


def signal(n: int, seed: int) -> np.ndarray:
    """white noise of unit variance with isolated spikes (what a median filter exists for), float32"""
    rng = np.random.default_rng(seed)
    y = rng.standard_normal(n)
    y[rng.random(n) < 0.02] *= 25.0
    return y.astype(np.float32)


def quadratic(n: int) -> np.ndarray:
    """0.25 - 0.5 t + 3 t^2 on t = i / n: every Savitzky-Golay fit of order >= 2 reproduces it, edges included"""
    t = np.arange(n, dtype=np.float64) / max(n, 1)
    return (0.25 - 0.5 * t + 3.0 * t * t).astype(np.float32)


def to_s16(y: np.ndarray) -> np.ndarray:
    return np.clip(np.round(y * 1024.0), -32768, 32767).astype(np.int16)


def medfilt_ref(x: np.ndarray, K: int) -> np.ndarray:
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)     # "kernel_size exceeds volume extent": legal, zero padded
        return scipy.signal.medfilt(x.astype(np.float64), K)


def savgol_ref(x: np.ndarray, W: int, P: int, deriv: int = 0, delta: float = 1.0) -> np.ndarray:
    return scipy.signal.savgol_filter(x.astype(np.float64), W, P, deriv=deriv, delta=delta, mode="interp")


def _centred_rows(W: int, P: int, deriv: int, delta: float, positions) -> np.ndarray:
    """weights over W samples of the deriv-th derivative of the least-squares polynomial at sample positions: the
    pseudo-inverse of the Vandermonde matrix of the centred abscissa"""
    import math
    h = W // 2
    t = np.arange(W, dtype=np.float64) - h
    pinv = np.linalg.pinv(np.vander(t, P + 1, increasing=True))          # [P + 1, W]
    rows = np.zeros((len(positions), W))
    for r, pos in enumerate(positions):
        u = float(pos - h)
        for j in range(deriv, P + 1):
            rows[r] += math.factorial(j) / math.factorial(j - deriv) * u ** (j - deriv) * pinv[j]
    return rows / delta ** deriv


def savgol_second(x: np.ndarray, W: int, P: int, deriv: int = 0, delta: float = 1.0) -> np.ndarray:
    """a second float64 evaluation of savgol_ref through numpy alone"""
    x = x.astype(np.float64)
    n, h = x.size, W // 2
    assert n >= W
    out = np.correlate(x, _centred_rows(W, P, deriv, delta, [h])[0], mode="same")
    out[:h] = _centred_rows(W, P, deriv, delta, range(h)) @ x[:W]
    out[n - h:] = _centred_rows(W, P, deriv, delta, range(h + 1, W)) @ x[n - W:]
    return out


def savgol_conditioning(x: np.ndarray, ref: np.ndarray, W: int, P: int, deriv: int = 0, delta: float = 1.0) -> float:
    """the largest distance between the two float64 evaluations, relative to max|x|"""
    peak = float(np.max(np.abs(x)))
    if peak == 0.0:
        return 0.0
    c = float(np.max(np.abs(ref - savgol_second(x, W, P, deriv, delta)))) / peak
    assert c <= MAX_CONDITIONING, (W, P, deriv, x.size, c)
    return c


def savgol_ratio(got: np.ndarray, x: np.ndarray, W: int, P: int, deriv: int = 0, delta: float = 1.0):
    """(largest |got - ref| as a fraction of its bound, the case's conditioning)"""
    ref = savgol_ref(x, W, P, deriv, delta)
    c = savgol_conditioning(x, ref, W, P, deriv, delta)
    bound = EPS24 * np.abs(ref) + 4.0 * c * float(np.max(np.abs(x)))
    err = np.abs(got.astype(np.float64) - ref)
    if not (err[bound == 0] == 0).all():
        return float("inf"), c
    live = bound > 0
    return (float(np.max(err[live] / bound[live])) if live.any() else 0.0), c


# ---- the energy and ZCR groups ----

def group_signal(n: int, sr: int, seed: int) -> np.ndarray:
    """white noise + 0.5 DC + a 50 Hz tone: the filter tests' signal"""
    from tests import filt_ref
    return filt_ref.signal(n, sr, seed)


def framing(n: int, frame_length: int = FRAME_LENGTH, hop_length: int = HOP_LENGTH):
    """_adjust_frame_length (:42-60) and the hop of :353: (fl, hop, T)"""
    fl = frame_length
    if n < frame_length:
        fl = max(64, 2 ** int(np.log2(n)))
    hop = min(hop_length, fl // 4)
    return fl, hop, 1 + n // hop


def _frames(ypad: np.ndarray, fl: int, hop: int) -> np.ndarray:
    return np.lib.stride_tricks.sliding_window_view(ypad, fl)[::hop]


def energy_frames(y: np.ndarray, fl: int, hop: int) -> np.ndarray:
    """librosa.feature.rms(y=y, frame_length=fl, hop_length=hop, center=True) with zero padding, in float64"""
    ypad = np.pad(y.astype(np.float64), fl // 2)
    return np.sqrt(np.mean(_frames(ypad, fl, hop) ** 2, axis=1))


def smoothed(y: np.ndarray) -> np.ndarray:
    """the extra ZCR pre-step (:424-430), float32 between the stages"""
    assert y.dtype == np.float32
    m = medfilt_ref(y, 3).astype(np.float32)
    if m.size > 11:
        m = savgol_ref(m, 11, 3).astype(np.float32)
    return m


def zcr_is_robust(s: np.ndarray) -> bool:
    """no smoothed sample within 1e-9 of the peak of zero other than exact zeros: the sign decisions then survive a last-bit
    difference of the smoothed signal"""
    peak = float(np.max(np.abs(s))) if s.size else 0.0
    if peak < np.finfo(np.float32).tiny:
        return True
    r = np.abs(s.astype(np.float64)) / peak
    return not bool(((r > 0) & (r < 1e-9)).any())


def zcr_counts(s: np.ndarray, fl: int, hop: int) -> np.ndarray:
    """crossings per frame of librosa.feature.zero_crossing_rate(center=True) (edge padding) of librosa.util.normalize(s)"""
    peak = float(np.max(np.abs(s)))
    z = s.astype(np.float64)
    if peak >= np.finfo(np.float32).tiny:
        z = z / peak
    z[np.abs(z) <= 1e-10] = 0.0
    neg = np.signbit(z)
    f = _frames(np.pad(neg, fl // 2, mode="edge"), fl, hop)
    return np.sum(f[:, 1:] != f[:, :-1], axis=1)


def local_stability(rates: np.ndarray) -> float:
    w = min(10, rates.size)
    if w > 1:
        return float(np.mean([np.std(rates[i:i + w]) for i in range(0, rates.size - w + 1)]))
    return float(np.std(rates))


def group_record(y: np.ndarray, frame_length: int = FRAME_LENGTH, hop_length: int = HOP_LENGTH) -> dict:
    """both groups of one float32 signal (already preprocessed) as the record's fields, and the crossing counts"""
    assert y.dtype == np.float32 and y.size > 0
    fl, hop, T = framing(y.size, frame_length, hop_length)
    e = energy_frames(y, fl, hop)
    s = smoothed(y)
    counts = zcr_counts(s, fl, hop)
    rates = counts / float(fl)
    assert e.size == T == rates.size
    return {"T": T, "fl": fl, "hop": hop, "energy_mean": float(np.mean(e)), "energy_std": float(np.std(e)),
            "energy_p10": float(np.percentile(e, 10)), "zcr_mean": float(np.mean(rates)), "zcr_std": float(np.std(rates)),
            "zcr_local_stability": local_stability(rates), "peak_smooth": float(np.max(np.abs(s))), "counts": counts,
            "robust": zcr_is_robust(s)}


def check_record(rec: np.ndarray, ref: dict, what) -> None:
    """a record of the native code against group_record: the framing exactly, the scalars to rtol 1e-12 (absolute 1e-12 on
    the ZCR statistics, which presumes equal crossing counts: the input must be robust), the smoothed peak to one float32
    rounding"""
    f = REC_FIELDS.index
    assert (rec[f("T")], rec[f("fl")], rec[f("hop")]) == (ref["T"], ref["fl"], ref["hop"]), what
    for k in ("energy_mean", "energy_std", "energy_p10"):
        assert abs(rec[f(k)] - ref[k]) <= 1e-12 * abs(ref[k]), (what, k, rec[f(k)], ref[k])
    assert ref["robust"], what
    for k in ("zcr_mean", "zcr_std", "zcr_local_stability"):
        assert abs(rec[f(k)] - ref[k]) <= 1e-12, (what, k, rec[f(k)], ref[k])
    assert abs(rec[f("peak_smooth")] - ref["peak_smooth"]) <= 2.0 ** -23 * ref["peak_smooth"], what


def energy_dict(r: dict) -> dict:
    """:367-399 on the restated scalars"""
    mean, std, floor = r["energy_mean"], r["energy_std"], r["energy_p10"]
    cv = std / mean if mean != 0 else float("inf")
    snr = 20 * np.log10(mean / floor) if floor > 0 else 0
    d = {"energy_mean": mean, "energy_std": std, "energy_cv": cv, "energy_snr": float(snr),
         "energy_range_valid": bool((mean >= 5.67e-03) and (mean <= 2.62e+00)), "energy_stability": bool(cv <= 0.3),
         "energy_snr_valid": bool(snr >= 20)}
    score = 1.0
    for k in ("energy_range_valid", "energy_stability", "energy_snr_valid"):
        if not d[k]:
            score -= 0.3
    d["energy_quality_score"] = max(0.0, score)
    return d


def zcr_dict(r: dict) -> dict:
    """:444-480 on the restated scalars"""
    mean, std, local = r["zcr_mean"], r["zcr_std"], r["zcr_local_stability"]
    cv = std / mean if mean != 0 else float("inf")
    d = {"zcr_mean": mean, "zcr_std": std, "zcr_cv": cv, "zcr_local_stability": local,
         "zcr_range_valid": bool((mean >= 0.034) and (mean <= 0.491)), "zcr_stability": bool(cv <= 0.35),
         "zcr_local_stable": bool(local <= 0.1)}
    score = 1.0
    for k, cost in (("zcr_range_valid", 0.4), ("zcr_stability", 0.3), ("zcr_local_stable", 0.3)):
        if not d[k]:
            score -= cost
    d["zcr_quality_score"] = max(0.0, score)
    return d


def flag_margins(d: dict) -> dict:
    """flag -> True when the scalar behind it lies at least FLAG_MARGIN (relative) away from every threshold it is compared
    with; only such flags (and a score all of whose flags are such) are compared"""
    def far(v, *thresholds):
        return all(np.isinf(v) or abs(v - t) >= FLAG_MARGIN * abs(t) for t in thresholds)
    out = {}
    if "energy_mean" in d:
        out["energy_range_valid"] = far(d["energy_mean"], 5.67e-03, 2.62e+00)
        out["energy_stability"] = far(d["energy_cv"], 0.3)
        out["energy_snr_valid"] = far(d["energy_snr"], 20.0)
        out["energy_quality_score"] = all(out[k] for k in ("energy_range_valid", "energy_stability", "energy_snr_valid"))
    if "zcr_mean" in d:
        out["zcr_range_valid"] = far(d["zcr_mean"], 0.034, 0.491)
        out["zcr_stability"] = far(d["zcr_cv"], 0.35)
        out["zcr_local_stable"] = far(d["zcr_local_stability"], 0.1)
        out["zcr_quality_score"] = all(out[k] for k in ("zcr_range_valid", "zcr_stability", "zcr_local_stable"))
    return out
