"""Restatement of librosa.beat.beat_track(onset_envelope=env, sr=sr) at its defaults (hop 512, tightness 100, trim=True)
for a given tempo -- the second half of the rhythm group of 04_feature_extraction_experiment/feature_extractor.py:604-607,
whose first half (the envelope and the tempo) is tests/rhythm_ref.py -- written out with numpy alone.  librosa is not
installed where this runs, so this file is the spec of afx_beat_batch and afx_beat_track_host; parity with librosa itself
is unpinned, as for tests/rhythm_ref.py.

The tracker is Ellis's dynamic programme: the envelope over its standard deviation, smoothed by a Gaussian of the beat
period (the local score); per frame the best predecessor half to two periods back under a log-squared penalty; the last
beat is the last local maximum of the cumulative score that reaches half the median of the local maxima; backtrack; trim.
The trim is the beat-indexed rule of Ellis's tracker (the local score at the beats smoothed by a 5-point Hann window, cut
at half its root mean square).  librosa's releases differ in this step (0.10 and later pad and threshold differently from
0.9), which is one more reason parity with a particular release is not claimed.

Where librosa is undefined this file decides: one frame (std with ddof 1 of one value) has no beats; a cumulative score
without a local maximum has no beats.

dtype "f64": every array in float64 (the oracle).  "f32": every array in float32, as librosa holds them for a float32
envelope; scalars (the penalty, the thresholds) stay Python floats, as they do there."""
import numpy as np

MAX_FPB = 768                                  # frames per beat the kernels hold (the tempogram window's bound)
HOP = 512
HANN5 = np.array([0.0, 0.5, 1.0, 0.5, 0.0])    # scipy.signal.windows.hann(5)


def round_half_even(v) -> int:
    return int(np.round(v))


def frames_per_beat(fps, bpm) -> int:
    """round(fps * 60 / bpm), half to even; bpm > 0"""
    return round_half_even(float(fps) * 60.0 / float(bpm))


def beat_window(fpb, dt=np.float64) -> np.ndarray:
    """exp(-0.5 ((k - fpb) 32 / fpb)^2), k = 0 .. 2 fpb"""
    return np.exp(-0.5 * (np.arange(-fpb, fpb + 1) * 32.0 / fpb) ** 2).astype(dt)


def local_score(x, fpb) -> np.ndarray:
    """np.convolve(x, window, "same") by its definition: localscore[i] = sum_k window[k] x[i + fpb - k]"""
    dt = x.dtype.type
    w = beat_window(fpb, dt)
    T = x.shape[0]
    out = np.zeros(T, dt)
    for i in range(T):
        k0, k1 = max(0, i + fpb - (T - 1)), min(2 * fpb, i + fpb)
        k = np.arange(k0, k1 + 1)
        out[i] = np.sum(w[k] * x[i + fpb - k], dtype=dt) if k.size else dt(0)
    return out


def dp(localscore, fpb, tightness):
    """(cumscore, backlink) of the dynamic programme"""
    T = localscore.shape[0]
    cumscore = np.zeros(T, localscore.dtype)
    backlink = np.full(T, -1, np.int32)
    thresh = 0.01 * float(localscore.max())
    lo = round_half_even(fpb / 2.0)
    d = np.arange(lo, 2 * fpb + 1, dtype=np.float64)
    pen = tightness * (np.log(d) - np.log(float(fpb))) ** 2          # by distance i - loc, nearest first
    first = True
    for i in range(T):
        best, arg = -np.inf, -1
        n = min(2 * fpb, i) - lo + 1                                  # candidates loc = i - lo, i - lo - 1, ... >= 0
        if n > 0:
            score = cumscore[i - lo - n + 1:i - lo + 1][::-1].astype(np.float64) - pen[:n]
            j = int(np.argmax(score))                                 # the first maximum: the nearest predecessor wins a tie
            if score[j] > best:
                best, arg = float(score[j]), i - lo - j
        cumscore[i] = float(localscore[i]) + best if arg >= 0 else localscore[i]
        if first and float(localscore[i]) < thresh:
            backlink[i] = -1
        else:
            backlink[i] = arg
            first = False
    return cumscore, backlink


def local_max_mask(c) -> np.ndarray:
    T = c.shape[0]
    i = np.arange(T)
    return (c > c[np.maximum(i - 1, 0)]) & (c >= c[np.minimum(i + 1, T - 1)])


def last_beat(cumscore) -> int:
    """the largest local maximum that reaches half the median of the local maxima; -1 without a local maximum"""
    mask = local_max_mask(cumscore)
    if not mask.any():
        return -1
    med = np.median(cumscore[mask])
    ok = np.flatnonzero(mask & (cumscore >= 0.5 * med))
    return int(ok[-1]) if ok.size else -1


def trim_smooth(s) -> np.ndarray:
    """0.5 s[j-1] + s[j] + 0.5 s[j+1], out-of-range terms zero (float64)"""
    s = np.asarray(s, np.float64)
    p = np.concatenate([[0.0], s, [0.0]])
    return 0.5 * p[:-2] + p[1:-1] + 0.5 * p[2:]


def trim_beats(beats, localscore) -> np.ndarray:
    beats = np.asarray(beats, np.int64)
    if beats.size == 0:
        return beats
    smooth = trim_smooth(np.asarray(localscore, np.float64)[beats])
    th = 0.5 * np.sqrt(np.mean(smooth ** 2))
    keep = np.flatnonzero(smooth > th)
    if keep.size == 0:
        return beats[:0]
    return beats[keep[0]:keep[-1] + 1]


def beat_track(env, fps, bpm, tightness=100.0, trim=True, dtype="f64") -> dict:
    """-> beats (int64 frames, ascending), fpb, localscore, cumscore, backlink (None where there are no beats by rule 1)"""
    dt = {"f64": np.float64, "f32": np.float32}[dtype]
    env = np.asarray(env, dt)
    T = env.shape[0]
    none = {"beats": np.zeros(0, np.int64), "fpb": 0, "localscore": None, "cumscore": None, "backlink": None}
    if bpm < 0 or not np.isfinite(bpm):
        raise ValueError("bpm must be finite and >= 0")
    if bpm > 0:
        fpb = frames_per_beat(fps, bpm)
        if not 1 <= fpb <= MAX_FPB:
            raise ValueError("frames per beat outside [1, 768]")
        none["fpb"] = fpb
    if T < 2 or not np.any(env) or bpm == 0:
        return none
    x = env / (np.std(env, ddof=1, dtype=dt) + np.finfo(dt).tiny)
    assert x.dtype == dt
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):   # fpb 1: lo = 0 and log(0) = -inf never wins
        localscore = local_score(x, fpb)
        cumscore, backlink = dp(localscore, fpb, float(tightness))
        tail = last_beat(cumscore)
    beats = []
    n = tail
    while n >= 0:
        beats.append(n)
        n = int(backlink[n])
    beats = np.array(beats[::-1], np.int64)
    if trim:
        with np.errstate(over="ignore", invalid="ignore"):
            beats = trim_beats(beats, localscore)
    return {"beats": beats, "fpb": fpb, "localscore": localscore, "cumscore": cumscore, "backlink": backlink}


def beats_are_robust(env, fps, bpm, tightness=100.0, trim=True) -> bool:
    """True when the beats of env may be pinned exactly: the float64 run, the float32 run and eight float64 runs on
    env (1 + 1e-5 randn) (fixed seeds) give the same beats.  A condition on test inputs, not a measurement."""
    env = np.asarray(env, np.float64)
    ref = beat_track(env, fps, bpm, tightness, trim)["beats"]
    runs = [beat_track(env.astype(np.float32), fps, bpm, tightness, trim, "f32")["beats"]]
    for seed in range(8):
        noisy = env * (1.0 + 1e-5 * np.random.default_rng(3000 + seed).standard_normal(env.shape))
        runs.append(beat_track(noisy, fps, bpm, tightness, trim)["beats"])
    return all(np.array_equal(ref, b) for b in runs)


def beat_stats(beats, fps):
    """(count, mean, std (ddof 0) of the inter-beat interval in seconds); NaN below two beats"""
    beats = np.asarray(beats, np.float64)
    if beats.size < 2:
        return int(beats.size), float("nan"), float("nan")
    d = np.diff(beats) / float(fps)
    return int(beats.size), float(np.mean(d)), float(np.std(d))


def impulse_train(T, p, first=None) -> np.ndarray:
    """float32 envelope of T frames, 1 at first, first + p, ... (first defaults to p), 0 elsewhere"""
    e = np.zeros(T, np.float32)
    e[(p if first is None else first)::p] = 1.0
    return e
