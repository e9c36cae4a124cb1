"""RIFF/WAVE decode for ``AudioFeatureExtractor.load_audio`` -- the decode+mono
half of ``librosa.load`` (reference: core/feature_extractor.py:52), restated
without soundfile: PCM 8/16/24/32-bit and IEEE float 32/64, any channel count,
scaled exactly as libsndfile scales to float32 (int16 / 32768, int24 / 2**23,
int32 / 2**31, (uint8 - 128) / 128), channels averaged in float32.

Resampling (librosa's ``soxr_hq`` when the file rate differs from ``sr``) is an
ingest step outside the GPU hot path; ``resample`` below uses scipy's polyphase
filter and is NOT bit-compatible with soxr."""
from __future__ import annotations

import struct
from math import gcd

import numpy as np

_FMT_PCM, _FMT_FLOAT, _FMT_EXT = 1, 3, 0xFFFE


class WavError(ValueError):
    pass


def _parse(buf: bytes):
    if len(buf) < 12 or buf[0:4] != b"RIFF" or buf[8:12] != b"WAVE":
        raise WavError("not a RIFF/WAVE file")
    pos, fmt, data = 12, None, None
    while pos + 8 <= len(buf):
        cid = buf[pos:pos + 4]
        size = struct.unpack_from("<I", buf, pos + 4)[0]
        body = pos + 8
        if cid == b"fmt ":
            if size < 16:
                raise WavError("short fmt chunk")
            tag, ch, rate, _, align, bits = struct.unpack_from("<HHIIHH", buf, body)
            if tag == _FMT_EXT and size >= 40:
                tag = struct.unpack_from("<H", buf, body + 24)[0]
            fmt = (tag, ch, rate, align, bits)
        elif cid == b"data":
            data = (body, min(size, len(buf) - body))
            break
        pos = body + size + (size & 1)
    if fmt is None or data is None:
        raise WavError("missing fmt or data chunk")
    return fmt, data


def read_wav_raw(path: str):
    """Returns (array [frames, channels] in the file's sample type, rate, kind) with
    kind in {'s16', 'u8', 's24', 's32', 'f32', 'f64'}; 's24' comes back as int32."""
    with open(path, "rb") as f:
        buf = f.read()
    (tag, ch, rate, align, bits), (off, size) = _parse(buf)
    if ch < 1:
        raise WavError("no channels")
    bps = bits // 8
    if bps * ch == 0:
        raise WavError("bad sample size")
    n = size // (bps * ch)
    raw = memoryview(buf)[off: off + n * bps * ch]
    if tag == _FMT_PCM:
        if bits == 16:
            a, kind = np.frombuffer(raw, "<i2"), "s16"
        elif bits == 8:
            a, kind = np.frombuffer(raw, np.uint8), "u8"
        elif bits == 32:
            a, kind = np.frombuffer(raw, "<i4"), "s32"
        elif bits == 24:
            b = np.frombuffer(raw, np.uint8).reshape(-1, 3).astype(np.int32)
            a = (b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16))
            a = np.where(a & 0x800000, a - 0x1000000, a).astype(np.int32)
            kind = "s24"
        else:
            raise WavError(f"unsupported PCM width {bits}")
    elif tag == _FMT_FLOAT:
        if bits == 32:
            a, kind = np.frombuffer(raw, "<f4"), "f32"
        elif bits == 64:
            a, kind = np.frombuffer(raw, "<f8"), "f64"
        else:
            raise WavError(f"unsupported float width {bits}")
    else:
        raise WavError(f"unsupported WAVE format tag {tag}")
    return a.reshape(n, ch), int(rate), kind


def to_float32(a: np.ndarray, kind: str) -> np.ndarray:
    if kind == "s16":
        return a.astype(np.float32) * np.float32(1.0 / 32768.0)
    if kind == "u8":
        return (a.astype(np.int32) - 128).astype(np.float32) * np.float32(1.0 / 128.0)
    if kind == "s24":
        return a.astype(np.float32) * np.float32(1.0 / 8388608.0)
    if kind == "s32":
        return a.astype(np.float32) * np.float32(1.0 / 2147483648.0)
    return a.astype(np.float32)


def to_mono(y: np.ndarray) -> np.ndarray:
    """[frames, channels] float32 -> [frames] float32 (librosa.to_mono = np.mean over channels)."""
    if y.shape[1] == 1:
        return np.ascontiguousarray(y[:, 0])
    return np.mean(y.T, axis=0, dtype=np.float32)


# Resampling policy (librosa.load(path, sr=...) at feature_extractor.py:52 resamples with
# soxr_hq).  soxr is not available here and bit parity with it is not a goal -- "parity unpinned" -- so this states
# what the engine's own resampler guarantees instead, and tests/test_wavio.py holds it to that:
#   * output length ceil(n * sr_out / sr_in), librosa's rule (it fixes the length after any resampler);
#   * a linear-phase Kaiser-windowed sinc low-pass (beta 12.98, ~125 dB) evaluated as a polyphase filter
#     (scipy.signal.resample_poly with explicit taps), transition band 0.913 .. 1.0 of the lower rate's Nyquist -- the
#     band edges soxr documents for its HQ recipe;
#   * pass band (up to 0.9 x that Nyquist): gain within 1e-4 of unity; stop band (at and above it): below -100 dB;
#   * float64 arithmetic, float32 result (librosa returns float32).
_RESAMPLE_TAPS = {}


def _resample_filter(up: int, down: int) -> np.ndarray:
    key = (up, down)
    h = _RESAMPLE_TAPS.get(key)
    if h is None:
        import scipy.signal
        fs = float(up)                                      # internal rate in units of sr_in
        nyq_low = 0.5 * min(1.0, up / down)                 # the lower of the two Nyquist frequencies, same units
        width = (1.0 - 0.913) * nyq_low
        numtaps, beta = scipy.signal.kaiserord(125.0, width / (0.5 * fs))
        numtaps |= 1
        h = scipy.signal.firwin(numtaps, 0.5 * (0.913 + 1.0) * nyq_low, window=("kaiser", beta), fs=fs)   # unity DC gain: resample_poly scales by up
        _RESAMPLE_TAPS[key] = h
    return h


def resample(y: np.ndarray, sr_in: int, sr_out: int) -> np.ndarray:
    """y at sr_in -> float32 at sr_out, ceil(n * sr_out / sr_in) samples (policy above)."""
    import scipy.signal
    if int(sr_in) == int(sr_out):
        return np.asarray(y, np.float32)
    g = gcd(int(sr_in), int(sr_out))
    up, down = int(sr_out) // g, int(sr_in) // g
    out = scipy.signal.resample_poly(np.asarray(y, np.float64), up, down, window=_resample_filter(up, down))
    n = int(np.ceil(y.shape[-1] * sr_out / sr_in))     # librosa fixes the length to ceil(n * ratio)
    out = out[:n] if out.shape[-1] >= n else np.pad(out, (0, n - out.shape[-1]))
    return out.astype(np.float32)


_BATCH_CTX = {}          # device -> (lock, _native.Context) of resample_batch and load_batch


def resample_batch(clips, sr_in: int, sr_out: int, device=None):
    """``resample`` of a list of mono clips (float32 or int16, int16 taken as value / 32768) -> list of float32 arrays.
    With a GPU visible the batch runs through afx_resample_batch on ``device`` (default 0): the same filter and float64
    arithmetic, within one float32 ulp of ``resample``.  Without one, or for a rate pair whose filter table the device
    resampler does not hold, every clip goes through ``resample`` on the host."""
    import threading
    from . import _native
    clips = [np.ascontiguousarray(c) for c in clips]
    for c in clips:
        if c.ndim != 1 or c.dtype not in (np.float32, np.int16):
            raise ValueError("resample_batch takes one-dimensional float32 or int16 clips")

    def host(c):
        return resample(to_float32(c, "s16") if c.dtype == np.int16 else c, sr_in, sr_out)

    try:
        on_gpu = _native.device_count() > 0
    except (_native.AfxError, OSError):
        on_gpu = False
    if not on_gpu or not clips:
        return [host(c) for c in clips]
    dev = int(device or 0)
    if dev not in _BATCH_CTX:
        _BATCH_CTX[dev] = (threading.Lock(), _native.Context(dev))
    lock, ctx = _BATCH_CTX[dev]
    out = [None] * len(clips)
    with lock:
        for dt in (np.int16, np.float32):                 # one call per sample type
            idx = [i for i, c in enumerate(clips) if c.dtype == dt]
            if not idx:
                continue
            lens = np.array([clips[i].size for i in idx], np.int64)
            offs = _native.packed_offsets(lens)
            buf = np.concatenate([clips[i] for i in idx]) if lens.sum() else np.zeros(1, dt)
            try:
                r = ctx.resample_batch(buf, offs, lens, sr_in, sr_out)
            except NotImplementedError:
                for i in idx:
                    out[i] = host(clips[i])
                continue
            for k, i in enumerate(idx):
                o, n = int(r["offsets"][k]), int(r["lengths"][k])
                out[i] = r["out"][o:o + n].copy()
    return out


_LOAD_BATCH_BYTES = 1 << 28     # raw bytes per device round trip of load_batch


def load_batch(paths, sr: int | None = None, device=None):
    """``load`` of many files -> list of (float32 mono samples, rate).  With a GPU visible, libafx parses the headers and
    reads the data chunks natively (afx_wav_probe / afx_wav_read_raw), the bytes are converted and mixed down on ``device``
    (default 0; afx_decode_batch, bit for bit ``to_mono(to_float32(...))``) and, where ``sr`` differs from a file's rate and
    the device resampler holds the rate pair, resampled there (within one float32 ulp of ``resample``).  With ``sr`` None or
    equal to the file's rate the samples are bit-identical to ``load``.  A file the native path does not take (8 or more
    channels, other sample widths or format tags), a file it cannot read, and every file when no GPU is visible goes through
    ``load`` -- which also raises what a bad file raises.  The bytes pass through ordinary (pageable) host memory here and
    are staged once more inside afx_decode_batch; the page-locked, uploaded-once path is batch_process's."""
    import threading
    from . import _native
    paths = [str(p) for p in paths]
    out = [None] * len(paths)
    try:
        on_gpu = _native.device_count() > 0 and hasattr(_native.lib(), "afx_decode_batch")
    except (_native.AfxError, OSError):
        on_gpu = False
    todo = np.zeros(0, np.int64)
    if on_gpu and paths:
        pr = _native.wav_probe(paths)
        kinds = _native.wav_sample_kinds(pr)
        todo = np.nonzero(kinds >= 0)[0]
        nbytes = pr["frames"] * _native.SMP_BYTES[np.maximum(kinds, 0)] * pr["channels"]
        dev = int(device or 0)
        if dev not in _BATCH_CTX:
            _BATCH_CTX[dev] = (threading.Lock(), _native.Context(dev))
        lock, ctx = _BATCH_CTX[dev]
    pos = 0
    while pos < todo.size:                                   # chunks of bounded size, each a run of whole files
        end, tot = pos + 1, int(nbytes[todo[pos]])
        while end < todo.size and tot + int(nbytes[todo[end]]) <= _LOAD_BATCH_BYTES:
            tot += int(nbytes[todo[end]])
            end += 1
        sel, pos = todo[pos:end], end
        boffs = _native.packed_offsets(nbytes[sel], 16)
        raw = np.empty(max(int(boffs[-1] + nbytes[sel[-1]]), 1), np.uint8)
        st = _native.wav_read_raw([paths[j] for j in sel], pr["data_off"][sel], nbytes[sel], raw, boffs)
        good = st == 0
        sel, boffs = sel[good], boffs[good]
        if not sel.size:
            continue
        frames, rates = pr["frames"][sel].astype(np.int64), pr["rate"][sel]
        offs = _native.packed_offsets(frames, 4)
        total = int(offs[-1] + (frames[-1] + 3) // 4 * 4)
        with lock:
            dbuf = _native.DeviceBuffer(ctx, max(4 * total, 16))
            try:
                ctx.decode_batch(raw, boffs, frames, kinds[sel], pr["channels"][sel], out=dbuf, out_offsets=offs)
                y = np.empty(total, np.float32)
                dbuf.download(y)
                for k, j in enumerate(sel):
                    if sr is None or int(rates[k]) == int(sr):
                        out[j] = (y[offs[k]:offs[k] + frames[k]].copy(), int(rates[k]))
                for rate in [] if sr is None else sorted({int(r) for r in rates} - {int(sr)}):
                    ks = np.nonzero(rates == rate)[0]
                    try:
                        r = ctx.resample_batch(dbuf, offs[ks], frames[ks], rate, int(sr), fmt=_native.FMT_F32)
                    except NotImplementedError:                  # no device table for this rate pair
                        for k in ks:
                            out[sel[k]] = (resample(y[offs[k]:offs[k] + frames[k]], rate, int(sr)), int(sr))
                        continue
                    for q, k in enumerate(ks):
                        o, n = int(r["offsets"][q]), int(r["lengths"][q])
                        out[sel[k]] = (r["out"][o:o + n].copy(), int(sr))
            finally:
                dbuf.free()
    for j, p in enumerate(paths):
        if out[j] is None:
            out[j] = load(p, sr)
    return out


def load(path: str, sr: int | None):
    """librosa.load(path, sr=sr): float32 mono, resampled to sr when it differs."""
    a, rate, kind = read_wav_raw(path)
    y = to_mono(to_float32(a, kind))
    if sr is not None and rate != sr:
        y = resample(y, rate, sr)
        rate = sr
    return y, rate


def write_wav_pcm16(path: str, y: np.ndarray, sr: int):
    """Test/bench helper: mono PCM16 writer (round-to-nearest of y * 32768, clipped)."""
    q = np.clip(np.rint(np.asarray(y, np.float64) * 32768.0), -32768, 32767).astype("<i2")
    data = q.tobytes()
    hdr = b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE" + b"fmt " + struct.pack(
        "<IHHIIHH", 16, 1, 1, int(sr), int(sr) * 2, 2, 16) + b"data" + struct.pack("<I", len(data))
    with open(path, "wb") as f:
        f.write(hdr + data)
