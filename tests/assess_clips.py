"""The clips of the assess tests (CPU and GPU), built once.  Loud is a 220 Hz tone of amplitude 0.3, quiet the same tone
80 dB down: every 10 ms frame lies at least 3 dB from the -40 dB threshold (a frame with a few loud samples in it is loud;
the segmented clips change level on frame edges), which ``assess_ref.silence_is_robust`` confirms for every clip when this
module is imported -- the silence counts of these clips are asserted exactly."""
import numpy as np

from tests import assess_ref as R

RATES = (8000, 16000, 22050, 44100)
LOUD, QUIET = 0.3, 0.3e-4


def tone(sr: int, n: int, amp: float = LOUD, start: int = 0) -> np.ndarray:
    t = (np.arange(n, dtype=np.float64) + start) / sr
    return (amp * np.sin(2 * np.pi * 220.0 * t + 0.7)).astype(np.float32)


def lead_in(sr: int, n: int, seed: int = 0) -> np.ndarray:
    """``n`` samples of a tone behind 2000 samples of noise 46 dB down: a clip whose SNR estimate is well conditioned."""
    y = tone(sr, n)
    m = min(2000, n)
    y[:m] = (1e-3 * np.random.default_rng(seed).standard_normal(m)).astype(np.float32)
    return y


def segmented(sr: int, segments) -> np.ndarray:
    """Segments of (loud, frames) whose levels change on the edges of the centred 10 ms frames: segment k is frames
    sum(frames[:k]) .. of the clip, so the clip has sum(frames) frames (the first segment is half a frame short)."""
    fl = R.frame_lengths(sr)[0]
    n = sum(f for _, f in segments) * fl - fl // 2
    y = tone(sr, n)
    pos = -(fl // 2)
    for loud, f in segments:
        if not loud:
            y[max(pos, 0):pos + f * fl] *= np.float32(QUIET / LOUD)
        pos += f * fl
    return y


# 0.3 s tone, 1.2 s quiet, 0.3 s tone, 0.3 s quiet, 0.3 s tone, 0.5 s quiet to the end: 290 frames, 200 silent, run 120
SEG_A = ((True, 30), (False, 120), (True, 30), (False, 30), (True, 30), (False, 50))
# starts and ends quiet; the run that reaches the last frame is the longest
SEG_B = ((False, 20), (True, 30), (False, 50))
SEGMENTED = {(name, sr): segmented(sr, seg) for name, seg in (("a", SEG_A), ("b", SEG_B)) for sr in RATES}
SEG_COUNTS = {"a": (290, 200, 120), "b": (100, 70, 50)}      # frames, silent, longest run


def _mixed():
    """One batch at four rates: lengths 0, 1, 9, frame - 1, frame, 2.3 s and about 40 000 samples (ten 4096-sample spans
    and, at every rate, 100 ms frame edges inside them)."""
    out = []
    for k, sr in enumerate(RATES):
        fs = R.frame_lengths(sr)[0]
        for n in (0, 1, 9, fs - 1, fs):
            out.append((f"{sr}/{n}", tone(sr, n), sr))
        out.append((f"{sr}/2.3s", lead_in(sr, int(2.3 * sr), seed=k), sr))
        out.append((f"{sr}/40k", lead_in(sr, 40000 + 37 * k, seed=10 + k), sr))
    return out


MIXED = _mixed()


def as_s16(y) -> np.ndarray:
    return np.clip(np.rint(np.asarray(y, np.float64) * 32768.0), -32768, 32767).astype(np.int16)


def every_clip():
    for name, y, sr in MIXED:
        yield name, y, sr
    for (name, sr), y in SEGMENTED.items():
        yield f"seg {name}/{sr}", y, sr


# the condition the exact assertions rest on, float32 and int16 alike
for _name, _y, _sr in every_clip():
    for _v in (_y, as_s16(_y)):
        assert _v.size == 0 or R.silence_is_robust(_v, _sr), _name
