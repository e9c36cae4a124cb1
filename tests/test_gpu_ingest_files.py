"""batch_process over a directory of every WAVE layout: files the device decodes (afx_wav_read_raw + afx_decode_batch, then
the device resampler) against extract_features(path) of the same file (the host decoder and resampler), within the
tolerances of tests/parity.py; which ingest path took which file; wavio.load_batch against wavio.load."""
import os

import numpy as np
import pytest

from tests.test_gpu_resample_files import _check
from tests.wavfiles import header, quantize, write_wav

pytestmark = pytest.mark.gpu

SR = 22050
# name, rate, kind, channels; the ingest path each must take
SPECS = [("a00", SR, "s16", 1, "native_s16"), ("a01", SR, "s16", 2, "native_raw"), ("a02", 44100, "s16", 2, "native_raw"),
         ("a03", 16000, "s24", 1, "native_raw"), ("a04", 44100, "s24", 2, "native_raw"), ("a05", SR, "u8", 1, "native_raw"),
         ("a06", 8000, "s32", 2, "native_raw"), ("a07", 48000, "f32", 3, "native_raw"), ("a08", SR, "f64", 1, "native_raw"),
         ("a09", SR, "s16", 8, "python"), ("a10", 16000, "s16", 1, "native_s16"), ("a11", SR, "s24", 7, "native_raw")]
BAD = {"b00_12bit.wav": "python", "b01_nan.wav": "native_raw", "b02_broken.wav": "python"}


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    from audio_feature_extraction_amd import _native
    from audio_feature_extraction_amd.synth import make_clip
    if _native.device_count() < 1:
        pytest.fail("no GPU visible")
    d = tmp_path_factory.mktemp("layouts")
    for k, (name, sr, kind, ch, _) in enumerate(SPECS):
        write_wav(d / f"{name}.wav", quantize(make_clip(k, sr, 1.5 + 0.25 * (k % 4), speechy=True), kind, ch), sr, kind)
    y = make_clip(40, SR, 1.5, speechy=True)
    data = quantize(y, "s16").tobytes()
    (d / "b00_12bit.wav").write_bytes(header(1, 1, SR, 12, len(data)) + data)           # a PCM width nobody decodes
    bad = quantize(make_clip(41, 16000, 1.5, speechy=True), "f32")
    bad[4000] = np.nan
    write_wav(d / "b01_nan.wav", bad, 16000, "f32")
    (d / "b02_broken.wav").write_bytes(b"RIFF\x00\x00\x00\x00WAVEjunk")                # truncated RIFF
    return d


@pytest.mark.parametrize("features", [None, ["mfcc", "energy"]], ids=["all", "mfcc-energy"])
@pytest.mark.parametrize("budget", [80 * 1024 * 1024, 60000], ids=["one-window", "small-budget"])
def test_every_layout_matches_single_file_extraction(corpus, features, budget):
    from audio_feature_extraction_amd import parallel, wavio
    from audio_feature_extraction_amd.core.feature_extractor import AudioFeatureExtractor
    ex = AudioFeatureExtractor(sr=SR)
    files = sorted(corpus.glob("*.wav"))
    calls = []
    real = wavio.resample
    wavio.resample = lambda *a, **k: (calls.append(a[1:]), real(*a, **k))[1]
    try:
        res = parallel.process_files(ex, files, max_batch_samples=budget, features_to_extract=features)
    finally:
        wavio.resample = real
    assert not calls, f"the host resampled {calls}"                       # every rate here has a device table
    paths = dict(BAD, **{f"{s[0]}.wav": s[4] for s in SPECS})
    want_ingest = {k: sum(1 for v in paths.values() if v == k) for k in ("native_s16", "native_raw", "python")}
    assert parallel.LAST_TIMING["ingest"] == want_ingest and want_ingest["python"] == 3
    got = [os.path.basename(r["file_path"]) for r in res]
    kw = {} if features is None else {"features_to_extract": features}
    want, refs = [], {}
    for f in files:
        try:
            refs[f.name] = ex.extract_features(str(f), **kw)
            want.append(f.name)
        except Exception:
            pass                                                           # dropped there: must be dropped here
    assert got == want                                                     # same files delivered / dropped, glob order
    assert got == [f"{s[0]}.wav" for s in SPECS]
    for r in res:
        ref = refs[os.path.basename(r["file_path"])]
        assert set(r) == set(ref)
        _check(r, ref, os.path.basename(r["file_path"]))


def test_load_batch_matches_load(corpus):
    from audio_feature_extraction_amd import wavio
    files = [str(corpus / f"{s[0]}.wav") for s in SPECS] + [str(corpus / "b01_nan.wav")]
    got = wavio.load_batch(files, sr=None)
    for f, (y, rate) in zip(files, got):
        ref, ref_rate = wavio.load(f, None)
        assert rate == ref_rate and y.dtype == np.float32 and y.shape == ref.shape, f
        assert ((y.view(np.uint32) == ref.view(np.uint32)) | np.isnan(ref)).all(), f
    # at one rate: files already there stay bit-identical, the others come from the device resampler, which is within
    # one float32 ulp of wavio.resample (an ulp is at most 2^-23 of the value)
    for f, (y, rate) in zip(files[:-1], wavio.load_batch(files[:-1], sr=SR)):
        ref, _ = wavio.load(f, SR)
        assert rate == SR and y.shape == ref.shape, f
        assert np.abs(y - ref).max() <= 2.0 ** -23 * np.abs(ref).max(), f
        if wavio.load(f, None)[1] == SR:
            assert (y.view(np.uint32) == ref.view(np.uint32)).all(), f
    with pytest.raises(wavio.WavError):                                    # what load raises for the file
        wavio.load_batch([files[0], str(corpus / "b00_12bit.wav")], sr=None)
