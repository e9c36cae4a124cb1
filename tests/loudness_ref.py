"""A numpy / scipy restatement of pyloudnorm 0.1.x ``Meter(rate).integrated_loudness`` and ``normalize.loudness`` /
``normalize.peak`` for mono audio with K-weighting -- the oracle of tests/test_loudness_*.py and tests/test_gpu_loudness.py.
pyloudnorm itself is not a dependency; parity with it is by construction, statement by statement:

K-weighting (``pyloudnorm.IIRfilter``, 'high_shelf' and 'high_pass', the RBJ cookbook forms).  With A = 10^(G/40),
w0 = 2 pi fc / rate, alpha = sin w0 / (2 Q):
  stage 1, high shelf, G = 4.0 dB, Q = 1/sqrt 2, fc = 1500 Hz:
    b0 = A[(A+1) + (A-1) cos w0 + 2 sqrt A alpha]    a0 = (A+1) - (A-1) cos w0 + 2 sqrt A alpha
    b1 = -2A[(A-1) + (A+1) cos w0]                   a1 = 2[(A-1) - (A+1) cos w0]
    b2 = A[(A+1) + (A-1) cos w0 - 2 sqrt A alpha]    a2 = (A+1) - (A-1) cos w0 - 2 sqrt A alpha
  stage 2, high pass, Q = 0.5, fc = 38 Hz:  b = (1 + cos w0) [1/2, -1, 1/2],  a = [1 + alpha, -2 cos w0, 1 - alpha];
  both divided through by a0 and applied with ``scipy.signal.lfilter(b, a, x)`` (zero initial state), stage 1 then stage 2.

Blocks (``Meter.integrated_loudness``).  T_g = block_size, step = 0.25, T = n / rate,
numBlocks = int(np.round((T - T_g) / (T_g step)) + 1) -- np.round rounds half to even, so at 16 kHz n = 7200 still has one
block and n = 8800 has three, the third ending at 9600 > n --; block j is the slice
[int(T_g (j step) rate), int(T_g (j step + 1) rate)) of the filtered signal (numpy cuts it at n), the products taken left to
right in double; z_j = sum y^2 / (T_g rate), the divisor the same for a partial block.  Since j 0.25 + 1 == (j + 4) 0.25
exactly, a block is four consecutive segments with boundaries b_k = int(T_g (k 0.25) rate) (`bounds`): at 11025 Hz they are
0, 1102, 2205, 3307, 4410 .. -- truncated, not evenly spaced.

Gating.  l_j = -0.691 + 10 log10 z_j; first set l_j >= -70; Gamma_r = -0.691 + 10 log10(mean z over it) - 10; second set
l_j > Gamma_r and l_j > -70; LUFS = -0.691 + 10 log10(mean z over it); the mean of an empty set is taken as 0
(np.nan_to_num), so the result is -inf.  Audio with n < block_size * rate raises ValueError (``util.valid_audio``).

Normalising.  gain = 10^((target - loudness) / 20), or 10^(target / 20) / max|x|; under numpy 1.24 a float32 array times a
float64 scalar stays float32: the gain is rounded to float32 and every sample is one rounded float32 product.

Two forms.  `measure(x, rate)` is the float64 truth: the float32 samples widened, both stages and the sums in float64.
`measure(x, rate, faithful=True)` is pyloudnorm's own arithmetic on a float32 (``librosa.load``) array as far as it differs
in kind: each stage's output is written back into the float32 copy, i.e. rounded to float32; the sums stay float64.

The engine's tolerance.  The engine filters in float64 without the rounding between the stages, so it may differ from
pyloudnorm by the rounding noise pyloudnorm adds.  For every clip of `shape_clips()` and for `gating_clip()` the two forms
above were compared: |faithful - float64| lay between 3.1e-11 and 1.9e-8 dB (BOUND_BASIS_DB = 2e-8; test_loudness_ref.py
asserts the distances stay at or under it), and the engine's bound is four times that, TOL_DB = 8e-8 dB -- the project's
usual margin over the reference's own error.  (The host executor was within 1.1e-14 dB of the float64 form on every clip.)
The gain is another matter of number formats: it is applied as a float32, so a normalised clip sits at
input + 20 log10(float32(gain)) and misses the target by up to GAIN_ROUND_DB = 20 log10(1 + 2^-24) = 5.2e-7 dB in the
reference as in the engine (0.97e-9 .. 4.1e-7 dB on these clips); a re-measured level is therefore held to TOL_DB around
input + 20 log10(applied gain), and that figure to GAIN_ROUND_DB around the target.
A block within rounding of a gate could fall on either side in two correct implementations, so every test clip keeps
|l_j + 70| and |l_j - Gamma_r| at or above 1e-6 dB (`gate_margin`, asserted in test_loudness_ref.py; the smallest here is
0.19 dB); the seeds below were picked for that.
"""
import functools

import numpy as np
import scipy.signal

STEP = 0.25
BOUND_BASIS_DB = 2e-8
TOL_DB = 4 * BOUND_BASIS_DB
GAIN_ROUND_DB = 20.0 * np.log10(1.0 + 2.0 ** -24)
TILE = 4096
RATES = (8000, 11025, 16000, 44100, 48000)


def kweight(rate):
    """[(b, a), (b, a)]: the two stages, float64, divided through by a0"""
    G, Q, fc = 4.0, 1.0 / np.sqrt(2.0), 1500.0
    A = 10.0 ** (G / 40.0)
    w0 = 2.0 * np.pi * (fc / rate)
    al = np.sin(w0) / (2.0 * Q)
    c = np.cos(w0)
    b = np.array([A * ((A + 1) + (A - 1) * c + 2 * np.sqrt(A) * al), -2 * A * ((A - 1) + (A + 1) * c),
                  A * ((A + 1) + (A - 1) * c - 2 * np.sqrt(A) * al)])
    a = np.array([(A + 1) - (A - 1) * c + 2 * np.sqrt(A) * al, 2 * ((A - 1) - (A + 1) * c), (A + 1) - (A - 1) * c - 2 * np.sqrt(A) * al])
    s1 = (b / a[0], a / a[0])
    Q, fc = 0.5, 38.0
    w0 = 2.0 * np.pi * (fc / rate)
    al = np.sin(w0) / (2.0 * Q)
    c = np.cos(w0)
    b = np.array([(1 + c) / 2, -(1 + c), (1 + c) / 2])
    a = np.array([1 + al, -2 * c, 1 - al])
    return [s1, (b / a[0], a / a[0])]


def n_blocks(n, rate, block_size=0.4):
    T = n / rate
    return int(np.round((T - block_size) / (block_size * STEP)) + 1)


def block_slices(n, rate, block_size=0.4):
    """[(l, u)] of every block, u not yet cut at n"""
    return [(int(block_size * (j * STEP) * rate), int(block_size * (j * STEP + 1) * rate)) for j in range(n_blocks(n, rate, block_size))]


def bounds(count, rate, block_size=0.4):
    return [int(block_size * (k * STEP) * rate) for k in range(count)]


def measure(x, rate, block_size=0.4, faithful=False):
    """-> dict(lufs, z, l, n1, n2, gamma_r, mean1, mean2); ValueError for audio shorter than a block"""
    x = np.asarray(x)
    if x.shape[0] < block_size * rate:
        raise ValueError("Audio must have length greater than the block size.")
    y = x.astype(np.float32) if faithful else x.astype(np.float64)
    for b, a in kweight(rate):
        y = scipy.signal.lfilter(b, a, y)            # float64 out for float64 coefficients
        if faithful:
            y = y.astype(np.float32)
    y = y.astype(np.float64)
    z = np.array([np.sum(np.square(y[l:u])) / (block_size * rate) for l, u in block_slices(x.shape[0], rate, block_size)])
    with np.errstate(divide="ignore", invalid="ignore"):
        l = -0.691 + 10.0 * np.log10(z)
        first = l >= -70.0
        mean1 = float(np.nan_to_num(np.mean(z[first]))) if first.any() else 0.0
        gamma_r = -0.691 + 10.0 * np.log10(mean1) - 10.0
        second = (l > gamma_r) & (l > -70.0)
        mean2 = float(np.mean(z[second])) if second.any() else 0.0
        lufs = -0.691 + 10.0 * np.log10(mean2)
    return {"lufs": float(lufs), "z": z, "l": l, "n1": int(first.sum()), "n2": int(second.sum()), "gamma_r": float(gamma_r),
            "mean1": mean1, "mean2": mean2}


def gate_margin(m):
    """the smallest distance in dB of a block from either gate (silent blocks, at -inf, are on one side exactly)"""
    l = m["l"][np.isfinite(m["l"])]
    if l.size == 0:
        return np.inf
    d = np.abs(l + 70.0).min()
    if np.isfinite(m["gamma_r"]):
        d = min(d, np.abs(l - m["gamma_r"]).min())
    return float(d)


def normalize_loudness(x, loudness, target):
    gain = np.power(10.0, (target - loudness) / 20.0)
    return np.float32(gain) * np.asarray(x, np.float32)


def normalize_peak(x, target):
    x = np.asarray(x, np.float32)
    gain = np.power(10.0, target / 20.0) / np.float64(np.max(np.abs(x)))
    return np.float32(gain) * x


def noise(n, seed, sigma=0.1):
    return (sigma * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def first_length_with(rate, blocks, block_size=0.4):
    """the smallest n with `blocks` gating blocks"""
    n = int(np.ceil(block_size * rate))
    while n_blocks(n, rate, block_size) < blocks:
        n += 1
    return n


def shape_lengths(rate, block_size=0.4):
    """B - 1 (refused), B, B + 1; both sides of the first two flips of np.round (the second leaves a partial last block);
    a whole number of tiles - 1, + 0, + 1; more than two and more than three tiles beyond the shortest clip"""
    B = int(np.ceil(block_size * rate))
    f2, f3 = first_length_with(rate, 2, block_size), first_length_with(rate, 3, block_size)
    kt = (B + 1 + TILE - 1) // TILE * TILE
    return [B - 1, B, B + 1, f2 - 1, f2, f3 - 1, f3, kt - 1, kt, kt + 1, kt + 2 * TILE + 77, kt + 3 * TILE + 1234]


@functools.lru_cache(maxsize=None)
def shape_clips():
    """((rate, clip), ..): read-only float32 noise at sigma 0.1 with a quieter last third, every length of shape_lengths
    at every rate of RATES"""
    out = []
    for r, rate in enumerate(RATES):
        for k, n in enumerate(shape_lengths(rate)):
            x = noise(n, 1000 * r + k)
            x[2 * n // 3:] *= np.float32(0.25)
            x.setflags(write=False)
            out.append((rate, x))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def gating_clip():
    """(16000, clip): 2 s at sigma 0.1, 2 s of zeros, 1 s at 0.003, 2 s at 0.05 -- 67 blocks; the absolute gate drops the
    silent blocks, the relative gate the quiet second as well"""
    rate = 16000
    x = np.concatenate([noise(2 * rate, 11, 0.1), np.zeros(2 * rate, np.float32), noise(rate, 12, 0.003), noise(2 * rate, 13, 0.05)])
    x.setflags(write=False)
    return rate, x


@functools.lru_cache(maxsize=None)
def oracle(i):
    """the float64 measure of clip i of shape_clips() (None for the refused one); i == -1: the gating clip"""
    rate, x = gating_clip() if i < 0 else shape_clips()[i]
    try:
        return measure(x, rate)
    except ValueError:
        return None


FLANK = 37


@functools.lru_cache(maxsize=None)
def gpu_batch():
    """The batch of tests/test_gpu_loudness.py: every clip of shape_clips() between a clip of +1e30 and one of -1e30 (too
    short to be measured themselves; a read across a clip boundary changes a sum), then an empty clip, a clip with a NaN, an
    all-zero clip and the gating clip.  -> dict(buf, offsets, lengths, rates, shape, empty, nan, zero, gating): one float32
    buffer with the clips one after another, nothing between them, and the indices of the clips by kind"""
    clips, rates, shape = [], [], []
    for rate, x in shape_clips():
        clips += [np.full(FLANK, 1e30, np.float32), x, np.full(FLANK, -1e30, np.float32)]
        rates += [rate] * 3
        shape.append(len(clips) - 2)
    bad = noise(8000, 77).copy()
    bad[4321] = np.nan
    grate, g = gating_clip()
    clips += [np.zeros(0, np.float32), bad, np.zeros(8000, np.float32), g]
    rates += [16000, 16000, 16000, grate]
    lengths = np.array([c.size for c in clips], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
    buf = np.concatenate(clips)
    for a in (buf, offsets, lengths):
        a.setflags(write=False)
    n = len(clips)
    return {"buf": buf, "offsets": offsets, "lengths": lengths, "rates": np.array(rates, np.int32), "shape": tuple(shape),
            "empty": n - 4, "nan": n - 3, "zero": n - 2, "gating": n - 1}


def out_layout(lengths, gap=8):
    """output offsets (multiples of 4) that leave `gap` untouched elements after every clip, and the array size"""
    lengths = np.asarray(lengths, np.int64)
    step = (lengths + 3) // 4 * 4 + gap
    offs = np.concatenate([[0], np.cumsum(step)[:-1]]).astype(np.int64)
    return offs, int(step.sum())
