"""afx_decode_batch: sample conversion and channel mix-down on the device against wavio.to_mono(wavio.to_float32(...)),
bit for bit, for every sample kind, 1 to 7 channels and clip lengths around the 4-frame lane group, the wave and the
workgroup, with clips of different layouts side by side in one batch."""
import numpy as np
import pytest

from tests.wavfiles import DTYPE, KINDS, sample_bytes

pytestmark = pytest.mark.gpu

CHANNELS = (1, 2, 3, 5, 7)
FRAMES = (0, 1, 3, 4, 5, 63, 64, 65, 257, 4099)
SENTINEL = np.float32(-1234.5)

SPECIAL = {
    "u8": [0, 255, 128, 127, 129],
    "s16": [-32768, 32767, 0, -1, 1],
    "s24": [-(1 << 23), (1 << 23) - 1, 0, -1, 1, 0x7FFF00, -0x7FFF01],
    "s32": [-(1 << 31), (1 << 31) - 1, (1 << 24) + 1, -(1 << 24) - 1, (1 << 24) + 3, (1 << 31) - 129, (1 << 31) - 128, (1 << 25) + 2, 0, -1],
    # float32: largest / smallest normal, denormals, signed zero, inf and NaN
    "f32": [3.4028235e38, -3.4028235e38, 1.17549435e-38, 1e-45, -1e-45, 5e-42, 7e-42, -0.0, np.inf, -np.inf, np.nan],
    # float64: beyond float32's range, its largest value and the tie above it, below its normal range, below its
    # smallest denormal, ties of the 24-bit significand
    "f64": [1e39, -1e39, 3.4028234663852886e38, 3.4028235677973366e38, 1e-40, -1e-40, 1e-46, 7.006492321624085e-46,
            1.0 + 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50, 1.0 + 3 * 2.0 ** -24, np.inf, np.nan, 1.7976931348623157e308],
}


def _values(rng, kind, n, ch):
    """[n, ch] sample values: random over the whole range of the type, the first frames overwritten with SPECIAL."""
    m = n * ch
    if kind == "u8":
        a = rng.integers(0, 256, m).astype(np.uint8)
    elif kind == "s16":
        a = rng.integers(-(1 << 15), 1 << 15, m).astype("<i2")
    elif kind == "s24":
        a = rng.integers(-(1 << 23), 1 << 23, m).astype("<i4")
    elif kind == "s32":
        a = rng.integers(-(1 << 31), 1 << 31, m).astype("<i4")
    elif kind == "f32":                                        # half audio-like, half arbitrary bit patterns
        a = np.where(rng.random(m) < 0.5, rng.uniform(-1, 1, m).astype("<f4"), rng.integers(0, 1 << 32, m).astype("<u4").view("<f4"))
    else:
        a = np.where(rng.random(m) < 0.5, rng.uniform(-1, 1, m) * 10.0 ** rng.integers(-48, 40, m),
                     rng.integers(0, 1 << 63, m).astype("<u8").view("<f8"))
    a = a.astype(DTYPE[kind])
    sp = np.array(SPECIAL[kind]).astype(DTYPE[kind])
    k = min(m, sp.size)
    a[:k] = sp[:k]
    if kind == "f32" and ch == 2 and n >= 5:                    # denormals met in the channel sum and the division
        a[2 * ch: 5 * ch] = np.array([1e-45, 3e-45, 5e-42, -7e-42, 1.17549435e-38, -1e-45], "<f4")
    return a.reshape(n, ch)


@pytest.fixture(scope="module")
def batch():
    """Every kind x channels x frames case as one batch in a seeded random order, with its reference (computed once)."""
    from audio_feature_extraction_amd import _native as N, wavio
    if N.device_count() < 1:
        pytest.fail("no GPU visible")
    rng = np.random.default_rng(11)
    cases = [(kind, ch, n) for kind in KINDS for ch in CHANNELS for n in FRAMES]
    cases = [cases[i] for i in rng.permutation(len(cases))]
    raws, refs = [], []
    with np.errstate(over="ignore", invalid="ignore"):
        for kind, ch, n in cases:
            a = _values(rng, kind, n, ch)
            raws.append(sample_bytes(a, kind))
            refs.append(wavio.to_mono(wavio.to_float32(a, kind)) if n else np.zeros(0, np.float32))
    nbytes = np.array([len(r) for r in raws], np.int64)
    gaps = 16 * (np.arange(len(cases)) % 2)                     # some clips further apart than the alignment asks
    boffs = N.packed_offsets(nbytes + gaps, 16)
    raw = np.full(int(boffs[-1] + nbytes[-1] + 15) // 16 * 16, 0xC3, np.uint8)
    for o, r in zip(boffs, raws):
        raw[o:o + len(r)] = np.frombuffer(r, np.uint8)
    frames = np.array([c[2] for c in cases], np.int64)
    ooffs = N.packed_offsets(frames + 4 * (np.arange(len(cases)) % 3), 4)
    size = int(ooffs[-1] + frames[-1] + 3) // 4 * 4 + 8
    ctx = N.Context(0)
    yield {"ctx": ctx, "cases": cases, "raw": raw, "boffs": boffs, "frames": frames, "ooffs": ooffs, "size": size, "refs": refs,
           "kinds": np.array([N.SMP_KINDS[c[0]] for c in cases], np.int32), "chans": np.array([c[1] for c in cases], np.int32)}
    ctx.close()


def _run(b, raw_on_device, out_on_device):
    from audio_feature_extraction_amd import _native as N
    ctx = b["ctx"]
    out = np.full(b["size"], SENTINEL, np.float32)
    raw = b["raw"]
    if raw_on_device:
        raw = N.DeviceBuffer(ctx, b["raw"].nbytes)
        raw.upload(b["raw"])
    if out_on_device:
        dout = N.DeviceBuffer(ctx, out.nbytes)
        dout.upload(out)
        ctx.decode_batch(raw, b["boffs"], b["frames"], b["kinds"], b["chans"], out=dout, out_offsets=b["ooffs"])
        dout.download(out)
        dout.free()
    else:
        ctx.decode_batch(raw, b["boffs"], b["frames"], b["kinds"], b["chans"], out=out, out_offsets=b["ooffs"])
    if raw_on_device:
        raw.free()
    return out


@pytest.mark.parametrize("raw_on_device", [False, True], ids=["host-raw", "device-raw"])
@pytest.mark.parametrize("out_on_device", [False, True], ids=["host-out", "device-out"])
def test_decode_matches_wavio_bit_for_bit(batch, raw_on_device, out_on_device):
    out = _run(batch, raw_on_device, out_on_device)
    written = np.zeros(out.size, bool)
    bad = []
    for case, o, n, ref in zip(batch["cases"], batch["ooffs"], batch["frames"], batch["refs"]):
        got = out[o:o + n]
        nan = np.isnan(ref)
        same = (got.view(np.uint32) == ref.view(np.uint32)) | (nan & np.isnan(got))     # NaN payloads through a sum are not pinned
        if not same.all():
            k = int(np.nonzero(~same)[0][0])
            bad.append((case, int((~same).sum()), k, float(got[k]), float(ref[k])))
        pad = (n + 3) // 4 * 4
        assert (out[o + n:o + pad].view(np.uint32) == 0).all(), case            # zeros up to the 4-aligned end
        written[o:o + pad] = True
    assert not bad, bad[:10]
    assert (out[~written] == SENTINEL).all()                                        # nothing else is written
    # the cases the values were chosen for did occur
    refs = dict(zip(batch["cases"], batch["refs"]))
    f64 = refs[("f64", 1, 4099)]
    assert np.isinf(f64[:2]).all() and f64[4] != 0 and abs(f64[4]) < np.finfo(np.float32).tiny and f64[6] == 0
    den = refs[("f32", 2, 4099)][2:5]
    assert (den != 0).all() and (np.abs(den) < np.finfo(np.float32).tiny).any()
    assert refs[("s32", 1, 4099)][2] == np.float32(2.0 ** -7)                       # (2^24 + 1) / 2^31: rounded to even


def test_decode_is_reproducible(batch):
    a, b = _run(batch, True, True), _run(batch, True, True)
    assert (a.view(np.uint32) == b.view(np.uint32)).all()


def test_decode_rejects_what_it_does_not_take(batch):
    from audio_feature_extraction_amd import _native as N
    ctx = batch["ctx"]
    raw = np.zeros(4096, np.uint8)
    out = np.full(256, SENTINEL, np.float32)

    def call(boffs=(0, 512), frames=(8, 8), kinds=(N.SMP_S16, N.SMP_F32), chans=(2, 3), ooffs=(0, 8)):
        return ctx.decode_batch(raw, boffs, frames, kinds, chans, out=out, out_offsets=ooffs)

    with pytest.raises(NotImplementedError):
        call(chans=(2, 8))
    for kw in (dict(boffs=(0, 520)), dict(ooffs=(0, 10)), dict(kinds=(N.SMP_S16, 6)), dict(kinds=(-1, N.SMP_F32)),
               dict(chans=(0, 3)), dict(frames=(8, -1)), dict(boffs=(-16, 512)), dict(ooffs=(0, 4)), dict(ooffs=(8, 4), frames=(8, 5))):
        with pytest.raises(ValueError):
            call(**kw)
    assert (out == SENTINEL).all()
    call()                                                                          # and the valid call goes through
    assert (out[:16] == 0).all() and (out[16:] == SENTINEL).all()
    assert ctx.decode_batch(raw, [], [], [], [], out=out, out_offsets=[])["lengths"].size == 0


def test_decode_offsets_beyond_32_bits(batch):
    """A clip that starts behind byte 2^31 of the raw buffer (the byte index of a lane no longer fits 32 bits)."""
    from audio_feature_extraction_amd import _native as N, wavio
    ctx = batch["ctx"]
    rng = np.random.default_rng(5)
    a = rng.integers(-(1 << 23), 1 << 23, (1027, 3)).astype("<i4")
    data = np.frombuffer(sample_bytes(a, "s24"), np.uint8)
    boff, ooff = (1 << 31) + 48, 8
    raw = N.DeviceBuffer(ctx, boff + 12 * 1024)
    out = N.DeviceBuffer(ctx, 4 * 1040)
    try:
        raw.upload(np.concatenate([data, np.zeros(1, np.uint8)]), byte_offset=boff)
        fill = np.full(1040, SENTINEL, np.float32)
        out.upload(fill)
        ctx.decode_batch(raw, [boff], [1027], [N.SMP_S24], [3], out=out, out_offsets=[ooff])
        out.download(fill)
    finally:
        raw.free()
        out.free()
    ref = wavio.to_mono(wavio.to_float32(a, "s24"))
    assert (fill[ooff:ooff + 1027].view(np.uint32) == ref.view(np.uint32)).all()
    assert (fill[:ooff] == SENTINEL).all() and fill[ooff + 1027] == 0 and (fill[ooff + 1028:] == SENTINEL).all()
