"""The two steps the reference puts around its feature extraction, on the GPU.

The screen that decides which recordings enter the corpus (00_audio_data_collection_experiment/audio_format_assessment.py:
``detect_silence``, ``check_volume_levels``, ``check_amplitude_stability``, ``estimate_snr``, ``assess_audio_file``,
``batch_assess_audio``): ``assess``, ``assess_batch``, ``assess_files``.  The per-clip reductions run in ``libafx.so``
(``afx_assess_batch``) at each clip's own rate -- a batch may mix rates -- and the reference's own expressions and
constants turn the device record into its keys on the host.  ``assess_files`` follows ``wavio.load_batch``: headers and
data chunks are read natively, decoded and mixed down on the device, and the decoded buffer goes straight into the screen.

The scores that judge a noise reducer (audio_quality_assessment.py: ``estimate_snr`` and the ``*_alternative`` scores the
reference falls back to without pypesq / pystoi): ``estimate_snr``, ``stoi_like``, ``compare_batch``,
``evaluate_noise_reduction``, from the sums of ``afx_compare_batch``; ``pesq_like``, ``spec_dist`` and their ``_batch``
forms, whose spectral term is a float64 DFT of the whole clip at whatever length it has (``afx_specdist_batch``: Bluestein's
algorithm over a power of two).  ``clip_rfft`` / ``clip_rfft_batch`` hand that transform out as ``np.fft.rfft``.

With no GPU visible every function runs libafx's host executors (``afx_assess_host`` / ``afx_compare_host`` /
``afx_specdist_host`` / ``afx_clip_fft_host``), the same definitions in plain C++; so does a clip longer than the device
transforms (2^21 samples).  Not here: the real pesq / stoi packages, WebM input, plots and reports."""
from __future__ import annotations

import os
import threading
from typing import List, Optional, Sequence

import numpy as np

from . import _native, wavio

NOISE_CAP = 2000                       # estimate_snr: at most this many leading samples are the noise estimate
# the reference's standard for a teacher recording (check_audio_format): 16 kHz, 32-bit PCM, mono
TEACHER_FORMAT = {"sample_rate": 16000, "subtype": "PCM_32", "channels": 1}
ASSESS_KEYS = ("silence_ratio", "max_silence_duration", "silence_ok", "rms_dbfs", "peak_dbfs", "volume_ok", "rms_std", "rms_cv",
               "stability_ok", "snr", "snr_ok")
_SUBTYPES = {(1, 8): "PCM_U8", (1, 16): "PCM_16", (1, 24): "PCM_24", (1, 32): "PCM_32", (3, 32): "FLOAT", (3, 64): "DOUBLE"}
_UNREADABLE = "無法讀取音頻文件"      # the reference's message for a file whose format cannot be read


def _on_gpu() -> bool:
    try:
        return _native.device_count() > 0 and hasattr(_native.lib(), "afx_assess_batch")
    except (_native.AfxError, OSError):
        return False


def _ctx(device):
    dev = int(device or 0)
    if dev not in wavio._BATCH_CTX:
        wavio._BATCH_CTX[dev] = (threading.Lock(), _native.Context(dev))
    return wavio._BATCH_CTX[dev]


def frame_lengths(sr: int):
    """The screen's two frame lengths at ``sr``: int(sr * 0.01) (silence) and int(sr * 0.1) (stability)."""
    fs, fl = int(sr * 0.01), int(sr * 0.1)
    if fs < 1:
        raise ValueError(f"sr={sr!r}: the 10 ms frame of the screen needs a sample rate of at least 100 Hz")
    return fs, fl


def _clips(signals) -> List[np.ndarray]:
    out = []
    for i, y in enumerate(signals):
        y = np.asarray(y)
        if y.ndim != 1:
            raise ValueError(f"signal {i} must be 1-D (mono), got shape {y.shape}")
        out.append(np.ascontiguousarray(y, np.int16 if y.dtype == np.int16 else np.float32))
    return out


def _raise_status(who: str, status) -> None:
    bad = np.flatnonzero(np.asarray(status) != _native.CLIP_OK)
    if bad.size:
        what = "is empty" if status[bad[0]] == _native.CLIP_TOO_SHORT else "is not finite everywhere"
        raise ValueError(f"{who}: signal {int(bad[0])} {what}")


def _records(clips: List[np.ndarray], fs, fl, threshold_db: float, device) -> tuple:
    """(rec [n, ASSESS_N], status [n]) of host clips: one device call per sample type, or the host executor per clip."""
    n = len(clips)
    rec = np.full((n, _native.ASSESS_N), np.nan, np.float64)
    status = np.zeros(n, np.int32)
    if not _on_gpu():
        for i, y in enumerate(clips):
            r = _native.assess_host(y, fs[i], fl[i], threshold_db, NOISE_CAP)
            rec[i], status[i] = r["rec"], r["status"]
        return rec, status
    lock, ctx = _ctx(device)
    with lock:
        for dt in (np.int16, np.float32):
            idx = [i for i, c in enumerate(clips) if c.dtype == dt]
            if not idx:
                continue
            lens = np.array([clips[i].size for i in idx], np.int64)
            buf = np.concatenate([clips[i] for i in idx]) if lens.sum() else np.zeros(1, dt)
            r = ctx.assess_batch(buf, _native.packed_offsets(lens), lens, fs[idx], fl[idx], threshold_db, NOISE_CAP)
            rec[idx], status[idx] = r["rec"], r["status"]
    return rec, status


def _from_record(rec, sr: int, fs: int) -> dict:
    """The reference's keys from one device record, with its expressions and constants (:169-300)."""
    n_short, silent, run, _, mean_square, peak, noise_power, _, rl_mean, rl_std = (float(v) for v in rec)
    silence_ratio = silent / n_short
    max_silence_duration = run * fs / sr if run else 0
    rms = np.sqrt(mean_square)
    rms_dbfs = 20 * np.log10(rms) if rms > 0 else -100
    peak_dbfs = 20 * np.log10(peak) if peak > 0 else -100
    rms_cv = rl_std / rl_mean if rl_mean > 0 else 0
    snr = 10 * np.log10((mean_square - noise_power) / noise_power) if noise_power > 0 and mean_square > noise_power else 0
    return {"silence_ratio": silence_ratio, "max_silence_duration": max_silence_duration,
            "silence_ok": bool(silence_ratio < 0.3 and max_silence_duration < 1.0),
            "rms_dbfs": rms_dbfs, "peak_dbfs": peak_dbfs, "volume_ok": bool(rms_dbfs > -30 and peak_dbfs < 0),
            "rms_std": rl_std, "rms_cv": rms_cv, "stability_ok": bool(rms_cv < 0.5),
            "snr": snr, "snr_ok": bool(snr >= 20)}


def assess_batch(signals: Sequence[np.ndarray], rates, *, threshold_db: float = -40, device: int = 0) -> List[dict]:
    """``assess`` of many mono signals (float32, or int16 taken as value / 32768) in one device pass.  ``rates``: one sample
    rate for all, or one per signal -- each clip is framed at its own."""
    clips = _clips(signals)
    rates = np.broadcast_to(np.asarray(rates, np.int64), (len(clips),)) if np.ndim(rates) == 0 else np.asarray(rates, np.int64)
    if rates.shape != (len(clips),):
        raise ValueError("rates must be one value or one per signal")
    if not np.isfinite(threshold_db):
        raise ValueError("threshold_db must be finite")
    frames = [frame_lengths(int(r)) for r in rates]
    fs = np.array([f[0] for f in frames], np.int32)
    fl = np.array([f[1] for f in frames], np.int32)
    if not clips:
        return []
    rec, status = _records(clips, fs, fl, float(threshold_db), device)
    _raise_status("assess", status)
    return [_from_record(rec[i], int(rates[i]), int(fs[i])) for i in range(len(clips))]


def assess(y, sr: int, *, threshold_db: float = -40, device: int = 0) -> dict:
    """The reference's four checks of one recording: ``detect_silence`` (10 ms frames, dB relative to the loudest frame,
    ``threshold_db``), ``check_volume_levels``, ``check_amplitude_stability`` (100 ms frames) and ``estimate_snr``, with its
    keys: silence_ratio, max_silence_duration, silence_ok, rms_dbfs, peak_dbfs, volume_ok, rms_std, rms_cv, stability_ok,
    snr, snr_ok."""
    return assess_batch([y], sr, threshold_db=threshold_db, device=device)[0]


# ---- files ----
def _format_info(rate: int, subtype: str, channels: int, frames: int, expected: dict) -> dict:
    """check_audio_format's WAV branch (:108-131) against ``expected``."""
    depth_ok = subtype == expected["subtype"]
    ok = rate == expected["sample_rate"] and depth_ok and channels == expected["channels"]
    bits = "".join(ch for ch in expected["subtype"] if ch.isdigit())
    return {"sample_rate": int(rate), "bit_depth": (bits + "-bit") if depth_ok and bits else subtype, "channels": int(channels),
            "duration": frames / rate, "format_ok": bool(ok)}


def _file_record(path: str, fmt: dict, a: dict) -> dict:
    """The record of assess_audio_file (:349-368): its keys, in its order."""
    ok = fmt["format_ok"] and a["silence_ok"] and a["volume_ok"] and a["stability_ok"] and a["snr_ok"]
    return {"file_path": path, "file_name": os.path.basename(path), "sample_rate": fmt["sample_rate"],
            "bit_depth": fmt["bit_depth"], "channels": fmt["channels"], "duration": fmt["duration"],
            "silence_ratio": a["silence_ratio"], "max_silence_duration": a["max_silence_duration"], "rms_dbfs": a["rms_dbfs"],
            "peak_dbfs": a["peak_dbfs"], "rms_cv": a["rms_cv"], "snr": a["snr"], "format_ok": fmt["format_ok"],
            "silence_ok": a["silence_ok"], "volume_ok": a["volume_ok"], "stability_ok": a["stability_ok"], "snr_ok": a["snr_ok"],
            "assessment_ok": bool(ok)}


def _error_record(path: str, error: str) -> dict:
    return {"file_path": path, "file_name": os.path.basename(path), "assessment_ok": False, "error": error}


def _assess_loaded(path: str, expected: dict, threshold_db: float, device) -> dict:
    """One file through ``wavio`` on the host and the same device call: what the native path does not take."""
    try:
        a, rate, kind = wavio.read_wav_raw(path)
    except (OSError, wavio.WavError, ValueError):
        return _error_record(path, _UNREADABLE)
    try:
        y = wavio.to_mono(wavio.to_float32(a, kind))
        subtype = {"u8": "PCM_U8", "s16": "PCM_16", "s24": "PCM_24", "s32": "PCM_32", "f32": "FLOAT", "f64": "DOUBLE"}[kind]
        fmt = _format_info(rate, subtype, a.shape[1], a.shape[0], expected)
        return _file_record(path, fmt, assess(y, rate, threshold_db=threshold_db, device=device))
    except Exception as e:                              # the reference's own catch-all (:371-378)
        return _error_record(path, str(e))


def assess_files(paths: Sequence[str], expected: Optional[dict] = None, *, threshold_db: float = -40, device: int = 0) -> List[dict]:
    """``assess_audio_file`` of every path (``batch_assess_audio`` without the CSV): one record per file with the
    reference's keys in its order -- file_path, file_name, sample_rate, bit_depth, channels, duration, silence_ratio,
    max_silence_duration, rms_dbfs, peak_dbfs, rms_cv, snr, format_ok, silence_ok, volume_ok, stability_ok, snr_ok,
    assessment_ok.  ``format_ok`` compares the header with ``expected`` (sample_rate, subtype as soundfile names it, channels;
    default: the reference's teacher standard, 16 kHz PCM_32 mono).  A file that cannot be read or is not RIFF/WAVE gives
    the reference's error record (file_path, file_name, assessment_ok False, error).

    With a GPU visible the files are probed and read natively, decoded and mixed down on the device at their own rates (no
    resampling), and the decoded buffer is screened where it lies: the samples never come back to the host.  Files the
    native path does not take (8 or more channels, other sample widths) are decoded by ``wavio`` on the host and go through
    the same device call."""
    expected = dict(TEACHER_FORMAT if expected is None else expected)
    paths = [str(p) for p in paths]
    out: List[Optional[dict]] = [None] * len(paths)
    if _on_gpu() and hasattr(_native.lib(), "afx_decode_batch") and paths:
        pr = _native.wav_probe(paths)
        kinds = _native.wav_sample_kinds(pr)
        todo = np.nonzero((kinds >= 0) & (pr["frames"] > 0))[0]
        nbytes = pr["frames"] * _native.SMP_BYTES[np.maximum(kinds, 0)] * pr["channels"]
        lock, ctx = _ctx(device)
        pos = 0
        while pos < todo.size:                          # chunks of bounded size, each a run of whole files
            end, tot = pos + 1, int(nbytes[todo[pos]])
            while end < todo.size and tot + int(nbytes[todo[end]]) <= wavio._LOAD_BATCH_BYTES:
                tot += int(nbytes[todo[end]])
                end += 1
            sel, pos = todo[pos:end], end
            boffs = _native.packed_offsets(nbytes[sel], 16)
            raw = np.empty(max(int(boffs[-1] + nbytes[sel[-1]]), 1), np.uint8)
            st = _native.wav_read_raw([paths[j] for j in sel], pr["data_off"][sel], nbytes[sel], raw, boffs)
            sel, boffs = sel[st == 0], boffs[st == 0]
            if not sel.size:
                continue
            frames, rates = pr["frames"][sel].astype(np.int64), pr["rate"][sel]
            fr = [frame_lengths(int(r)) if r >= 100 else None for r in rates]
            keep = np.array([f is not None for f in fr], bool)
            sel, boffs, frames, rates = sel[keep], boffs[keep], frames[keep], rates[keep]
            fr = [f for f in fr if f is not None]
            if not sel.size:
                continue
            offs = _native.packed_offsets(frames, 4)
            total = int(offs[-1] + (frames[-1] + 3) // 4 * 4)
            with lock:
                dbuf = _native.DeviceBuffer(ctx, max(4 * total, 16))
                try:
                    ctx.decode_batch(raw, boffs, frames, kinds[sel], pr["channels"][sel], out=dbuf, out_offsets=offs)
                    r = ctx.assess_batch(dbuf, offs, frames, [f[0] for f in fr], [f[1] for f in fr], float(threshold_db),
                                         NOISE_CAP, fmt=_native.FMT_F32)
                finally:
                    dbuf.free()
            for k, j in enumerate(sel):
                if r["status"][k] != _native.CLIP_OK:
                    out[j] = _error_record(paths[j], "Audio buffer is not finite everywhere")
                    continue
                subtype = _SUBTYPES[(int(pr["tag"][j]), int(pr["bits"][j]))]
                fmt = _format_info(int(rates[k]), subtype, int(pr["channels"][j]), int(frames[k]), expected)
                out[j] = _file_record(paths[j], fmt, _from_record(r["rec"][k], int(rates[k]), fr[k][0]))
    for j, p in enumerate(paths):
        if out[j] is None:
            out[j] = _assess_loaded(p, expected, threshold_db, device)
    return out


# ---- the scores of a reference / degraded pair ----
def _pair_from_record(rec) -> dict:
    """correlation, mse, snr and the STOI-like score of calculate_stoi_alternative (:246-280) from one compare record."""
    n, _, _, srr, _, _, see, m2r, m2d, m2 = (float(v) for v in rec)
    with np.errstate(all="ignore"):
        corr = float(np.clip(np.float64(m2) / np.sqrt(np.float64(m2r)) / np.sqrt(np.float64(m2d)), -1.0, 1.0))   # np.corrcoef
    mse = see / n
    signal_power, noise_power = srr / n, see / n
    snr = 10 * np.log10(signal_power / noise_power) if noise_power > 0 else 100
    corr_score = max(corr, 0)                           # Python's max: a NaN correlation (a constant input) stays NaN
    mse_score = max(1 - mse * 10, 0)
    snr_score = min(max((snr - 5) / 35, 0), 1)
    return {"correlation": corr, "mse": mse, "snr": snr, "stoi": 0.5 * corr_score + 0.3 * mse_score + 0.2 * snr_score}


def compare_batch(pairs: Sequence, *, device: int = 0) -> List[dict]:
    """For every (reference, degraded) pair of mono signals, over the shorter length of the two: correlation (np.corrcoef),
    mse (mean squared difference), snr (10 log10 of reference power over the power of degraded - reference; 100 when they
    are equal) and stoi, the reference's STOI-like weighting of the three.  One device pass."""
    refs = _clips([p[0] for p in pairs])
    degs = _clips([p[1] for p in pairs])
    refs = [wavio.to_float32(r, "s16") if r.dtype == np.int16 else r for r in refs]
    degs = [wavio.to_float32(d, "s16") if d.dtype == np.int16 else d for d in degs]
    n = len(refs)
    if not n:
        return []
    rec = np.full((n, _native.COMPARE_N), np.nan, np.float64)
    status = np.zeros(n, np.int32)
    if not _on_gpu():
        for i in range(n):
            r = _native.compare_host(refs[i], degs[i])
            rec[i], status[i] = r["rec"], r["status"]
    else:
        rl = np.array([r.size for r in refs], np.int64)
        dl = np.array([d.size for d in degs], np.int64)
        both = np.concatenate(refs + degs) if rl.sum() + dl.sum() else np.zeros(1, np.float32)
        offs = _native.packed_offsets(np.concatenate([rl, dl]))
        lock, ctx = _ctx(device)
        with lock:
            r = ctx.compare_batch(both, offs[:n], rl, both, offs[n:], dl)
        rec, status = r["rec"], r["status"]
    _raise_status("compare_batch", status)
    return [_pair_from_record(rec[i]) for i in range(n)]


def stoi_like(reference, degraded, *, device: int = 0) -> float:
    """The reference's ``calculate_stoi_alternative``: 0.5 max(correlation, 0) + 0.3 max(1 - 10 mse, 0) + 0.2 of the SNR of
    the difference mapped from 5 .. 40 dB to 0 .. 1.  NaN for a constant input, as the reference's is."""
    return compare_batch([(reference, degraded)], device=device)[0]["stoi"]


def estimate_snr(y, *, device: int = 0):
    """The reference's ``estimate_snr``: the first min(10 %, 2000 samples) of the clip are the noise estimate;
    10 log10((signal - noise) / noise), 0 when the signal power does not exceed the noise power."""
    return assess(y, 16000, device=device)["snr"]       # the noise window does not depend on the rate


def _pair_clips(pairs, who: str):
    """The two sides of every pair as float32 (int16 taken as value / 32768), with ``compare_batch``'s refusals: 1-D
    only, and the two sides of a pair of one sample type."""
    refs = _clips([p[0] for p in pairs])
    degs = _clips([p[1] for p in pairs])
    for i, (r, d) in enumerate(zip(refs, degs)):
        if r.dtype != d.dtype:
            raise ValueError(f"{who}: pair {i} mixes int16 and float32")
    refs = [wavio.to_float32(r, "s16") if r.dtype == np.int16 else r for r in refs]
    degs = [wavio.to_float32(d, "s16") if d.dtype == np.int16 else d for d in degs]
    return refs, degs


def _specdist_records(refs, degs, device) -> tuple:
    """(rec [n, SPECDIST_N], status [n]) of float32 pairs: one device call for the pairs the device takes, the host
    executor for the others (over ``_native.CFFT_MAX_N`` samples) and for all of them when no GPU is visible."""
    n = len(refs)
    rec = np.full((n, _native.SPECDIST_N), np.nan, np.float64)
    status = np.zeros(n, np.int32)
    gpu = _on_gpu() and hasattr(_native.lib(), "afx_specdist_batch")
    dev = [i for i in range(n) if gpu and min(refs[i].size, degs[i].size) <= _native.CFFT_MAX_N]
    for i in sorted(set(range(n)) - set(dev)):
        r = _native.specdist_host(refs[i], degs[i])
        rec[i], status[i] = r["rec"], r["status"]
    if dev:
        m = [min(refs[i].size, degs[i].size) for i in dev]             # only the common part is sent
        lens = np.array(m + m, np.int64)
        both = np.concatenate([refs[i][:k] for i, k in zip(dev, m)] + [degs[i][:k] for i, k in zip(dev, m)]) if sum(m) else np.zeros(1, np.float32)
        offs = _native.packed_offsets(lens)
        lock, ctx = _ctx(device)
        with lock:
            r = ctx.specdist_batch(both, offs[:len(dev)], lens[:len(dev)], both, offs[len(dev):], lens[len(dev):])
        rec[dev], status[dev] = r["rec"], r["status"]
    return rec, status


def spec_dist_batch(pairs: Sequence, *, device: int = 0) -> List[float]:
    """For every (reference, degraded) pair of mono signals, over the shorter length n of the two, the spectral term of the
    reference's ``calculate_pesq_alternative``: mean over all n bins of ||fft(ref)| - |fft(deg)|| / (|fft(ref)| + 1e-10),
    the DFTs of the whole clips in float64, whatever n is.  One device pass."""
    refs, degs = _pair_clips(pairs, "spec_dist_batch")
    if not refs:
        return []
    rec, status = _specdist_records(refs, degs, device)
    _raise_status("spec_dist_batch", status)
    return [float(rec[i][1] / rec[i][0]) for i in range(len(refs))]


def spec_dist(reference, degraded, *, device: int = 0) -> float:
    """``spec_dist_batch`` of one pair."""
    return spec_dist_batch([(reference, degraded)], device=device)[0]


def _pesq_from(corr: float, snr, dist: float) -> float:
    """calculate_pesq_alternative's weighting (:186-199), with Python's min and max as there: a NaN term stays NaN."""
    snr_score = min(max((snr - 5) / 35, 0), 1)
    corr_score = max(corr, 0)
    spec_score = 1 - min(dist, 1)
    return 1 + 3.5 * (0.4 * snr_score + 0.4 * corr_score + 0.2 * spec_score)


def pesq_like_batch(pairs: Sequence, *, device: int = 0) -> List[dict]:
    """The reference's ``calculate_pesq_alternative`` (what ``calculate_pesq`` computes without the pypesq package, on the
    signals as they are) for every (reference, degraded) pair, over the shorter length of the two: snr (of the difference;
    100 when it is zero), correlation, spec_dist and pesq = 1 + 3.5 (0.4 clip((snr - 5) / 35, 0, 1) + 0.4 max(correlation, 0)
    + 0.2 (1 - min(spec_dist, 1))), in 1 .. 4.5; NaN for a constant input, as the reference's is.  One compare record and
    one spectral record per pair."""
    refs, degs = _pair_clips(pairs, "pesq_like_batch")
    if not refs:
        return []
    cmp = compare_batch(list(zip(refs, degs)), device=device)
    rec, status = _specdist_records(refs, degs, device)
    _raise_status("pesq_like_batch", status)
    out = []
    for i, c in enumerate(cmp):
        dist = float(rec[i][1] / rec[i][0])
        out.append({"snr": c["snr"], "correlation": c["correlation"], "spec_dist": dist,
                    "pesq": _pesq_from(c["correlation"], c["snr"], dist)})
    return out


def pesq_like(reference, degraded, *, device: int = 0) -> float:
    """The PESQ-like score of one pair (``pesq_like_batch``)."""
    return pesq_like_batch([(reference, degraded)], device=device)[0]["pesq"]


def clip_rfft_batch(clips: Sequence, *, device: int = 0) -> List[np.ndarray]:
    """``np.fft.rfft`` of every mono clip (float32, or int16 taken as value / 32768) in float64, whatever its length -- a
    prime, 220500 = 2^2 3^2 5^3 7^2 -- as complex128 arrays of len // 2 + 1 bins (no bins for an empty clip).  One device
    pass; clips over ``_native.CFFT_MAX_N`` samples go through the host executor."""
    clips = _clips(clips)
    n = len(clips)
    out: List[Optional[np.ndarray]] = [None] * n
    status = np.zeros(n, np.int32)
    gpu = _on_gpu() and hasattr(_native.lib(), "afx_clip_fft_batch")
    for i, c in enumerate(clips):
        if not gpu or c.size > _native.CFFT_MAX_N:
            r = _native.clip_fft_host(c)
            out[i], status[i] = r["bins"], r["status"]
    if gpu:
        lock, ctx = _ctx(device)
        for dt in (np.int16, np.float32):
            idx = [i for i, c in enumerate(clips) if c.dtype == dt and out[i] is None]
            if not idx:
                continue
            lens = np.array([clips[i].size for i in idx], np.int64)
            buf = np.concatenate([clips[i] for i in idx]) if lens.sum() else np.zeros(1, dt)
            with lock:
                r = ctx.clip_fft_batch(buf, _native.packed_offsets(lens), lens)
            for k, i in enumerate(idx):
                out[i] = r["bins"][r["offsets"][k]:r["offsets"][k] + r["counts"][k]].copy()
                status[i] = r["status"][k]
    bad = np.flatnonzero(status == _native.CLIP_NONFINITE)
    if bad.size:
        raise ValueError(f"clip_rfft_batch: signal {int(bad[0])} is not finite everywhere")
    return out


def clip_rfft(y, *, device: int = 0) -> np.ndarray:
    """``np.fft.rfft(y)`` of one whole clip in float64 (``clip_rfft_batch``)."""
    return clip_rfft_batch([y], device=device)[0]


def evaluate_noise_reduction(y, sr: int, reference=None, *, pesq: bool = False, device: int = 0) -> dict:
    """The reference's ``evaluate_audio_quality`` on an in-memory signal: ``effects.spectral_subtraction`` and
    ``effects.wiener_filter`` at their defaults, then {original, spectral_subtraction, wiener_filter} x {snr, stoi}, each
    STOI-like score against ``reference`` (default: the original itself, as the reference does without a teacher file).
    ``pesq=True``: each entry is the reference's {snr, pesq, stoi}, pesq the PESQ-like score (``pesq_like``) against the
    same reference; the three pairs have one length, so their transforms share one filter spectrum."""
    from . import effects
    y = np.ascontiguousarray(y, np.float32)
    ref = y if reference is None else np.ascontiguousarray(reference, np.float32)
    outs = {"original": y, "spectral_subtraction": effects.spectral_subtraction(y, sr, device=device),
            "wiener_filter": effects.wiener_filter(y, sr, device=device)}
    names = list(outs)
    snr = assess_batch([outs[k] for k in names], sr, device=device)
    sc = compare_batch([(ref, outs[k]) for k in names], device=device)
    if not pesq:
        return {k: {"snr": snr[i]["snr"], "stoi": sc[i]["stoi"]} for i, k in enumerate(names)}
    pq = pesq_like_batch([(ref, outs[k]) for k in names], device=device)
    return {k: {"snr": snr[i]["snr"], "pesq": pq[i]["pesq"], "stoi": sc[i]["stoi"]} for i, k in enumerate(names)}
