"""RIFF/WAVE files of every sample layout the engine reads, for the ingest tests (values in, bytes out: no scaling)."""
import struct

import numpy as np

KINDS = ("u8", "s16", "s24", "s32", "f32", "f64")
FORMAT = {"u8": (1, 8), "s16": (1, 16), "s24": (1, 24), "s32": (1, 32), "f32": (3, 32), "f64": (3, 64)}      # (tag, bits)
DTYPE = {"u8": np.uint8, "s16": "<i2", "s24": "<i4", "s32": "<i4", "f32": "<f4", "f64": "<f8"}


def sample_bytes(a, kind: str) -> bytes:
    """The data-chunk bytes of the sample values ``a`` ([frames, channels], the kind's own type; s24 as int32)."""
    a = np.ascontiguousarray(a, DTYPE[kind])
    if kind == "s24":
        return a.view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    return a.tobytes()


def header(tag: int, channels: int, rate: int, bits: int, data_len: int) -> bytes:
    bps = bits // 8
    return b"RIFF" + struct.pack("<I", 36 + data_len) + b"WAVE" + b"fmt " + struct.pack(
        "<IHHIIHH", 16, tag, channels, int(rate), int(rate) * bps * channels, bps * channels, bits) + b"data" + struct.pack("<I", data_len)


def write_wav(path, a, rate: int, kind: str) -> bytes:
    """Writes ``a`` ([frames, channels]) as a file of ``kind``; -> its data-chunk bytes."""
    a = np.asarray(a)
    data = sample_bytes(a, kind)
    tag, bits = FORMAT[kind]
    with open(path, "wb") as f:
        f.write(header(tag, a.shape[1], rate, bits, len(data)) + data)
    return data


def quantize(y, kind: str, channels: int = 1):
    """A float signal in [-1, 1) -> [frames, channels] sample values of ``kind`` (channel c scaled by 0.5 + 0.5 c / channels)."""
    y = np.asarray(y, np.float64)
    y = np.stack([y * (0.5 + 0.5 * c / channels) for c in range(channels)], axis=1)
    if kind == "u8":
        return np.clip(np.rint(y * 128.0) + 128, 0, 255).astype(np.uint8)
    if kind in ("s16", "s24", "s32"):
        full = {"s16": 2.0 ** 15, "s24": 2.0 ** 23, "s32": 2.0 ** 31}[kind]
        return np.clip(np.rint(y * full), -full, full - 1).astype(np.int64).astype(DTYPE[kind])
    return y.astype(DTYPE[kind])
