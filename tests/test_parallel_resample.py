"""process_files with files at another sample rate than the extractor's, on fake plans (no GPU, no libafx device code): who
resamples what, how the sub-batches are cut and laid out, and what happens when the device resampler is absent or fails."""
import os
import struct

import numpy as np

from audio_feature_extraction_amd import _native, parallel, wavio
from tests.test_parallel import _FakeBuf, _FakePlan

SR = 8000
REAL_RESAMPLE = wavio.resample


class _RsPlan(_FakePlan):
    """A fake plan with the device resampler: computes what wavio.resample computes, and records every call."""

    def __init__(self, device, lane, calls, rs_calls, fail_rs=False, unsupported=()):
        super().__init__(device, lane, calls)
        self.rs_calls, self.fail_rs, self.unsupported = rs_calls, fail_rs, set(unsupported)

    def resample_batch(self, samples, offsets, lengths, sr_in, sr_out, fmt=None, taps=None, out=None, out_offsets=None):
        if sr_in in self.unsupported:
            raise NotImplementedError(f"no table for {sr_in} -> {sr_out}")
        if self.fail_rs:
            raise RuntimeError(f"resampler on device {self.device} fell over")
        assert isinstance(samples, _FakeBuf) and isinstance(out, _FakeBuf)
        assert samples.data.dtype == (np.int16 if fmt == _native.FMT_S16 else np.float32)
        olen = _native.resample_lengths(lengths, sr_in, sr_out)
        res = np.zeros(int(out_offsets[-1] + olen[-1]) + 4, np.float32)
        for o, n, oo, on in zip(offsets, lengths, out_offsets, olen):
            y = samples.data[o:o + n].astype(np.float32)
            if fmt == _native.FMT_S16:
                y = y * np.float32(1.0 / 32768.0)
            r = REAL_RESAMPLE(y, sr_in, sr_out)
            assert r.size == on
            res[oo:oo + on] = r
        out.data = res
        self.rs_calls.append({"device": self.device, "sr_in": int(sr_in), "sr_out": int(sr_out), "fmt": int(fmt),
                              "lengths": np.array(lengths), "out_offsets": np.array(out_offsets), "out_lengths": olen})
        return {"out": out, "offsets": out_offsets, "lengths": olen}


def _extractor(n_dev, calls, make_plan):
    import logging
    from audio_feature_extraction_amd.core.feature_extractor import AudioFeatureExtractor
    ex = AudioFeatureExtractor.__new__(AudioFeatureExtractor)
    ex.sr, ex.n_mfcc, ex.f0_min, ex.f0_max = SR, 13, 65.4, 2093.0
    ex.logger = logging.getLogger("fake")
    plans = {}

    def _plan(device=None, lane=0):
        if (device, lane) not in plans:
            plans[(device, lane)] = make_plan(device, lane)
        return plans[(device, lane)]
    ex._devices = lambda: list(range(n_dev))
    ex._plan = _plan
    return ex


def _write_f32(path, y, sr):
    data = np.asarray(y, "<f4").tobytes()
    hdr = b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE" + b"fmt " + struct.pack(
        "<IHHIIHH", 16, 3, 1, int(sr), int(sr) * 4, 4, 32) + b"data" + struct.pack("<I", len(data))
    with open(path, "wb") as f:
        f.write(hdr + data)


def _corpus(tmp_path, n, rates=(8000, 16000, 11025), float_every=0):
    """n files cycling through `rates`; every `float_every`-th one is a float32 file.  -> files, per file the sum of
    the samples wavio.resample gives (the fake plans' mfcc_mean[0]), per file (rate, is_float)"""
    rng = np.random.default_rng(11)
    files, sums, kinds = [], [], []
    for i in range(n):
        rate = rates[i % len(rates)]
        m = int(rng.integers(3000, 9000)) * rate // 8000
        y = (rng.standard_normal(m) * 0.1).astype(np.float32)
        p = tmp_path / f"c{i:03d}.wav"
        is_f = bool(float_every) and i % float_every == float_every - 1
        if is_f:
            _write_f32(str(p), y, rate)
            q = y
        else:
            wavio.write_wav_pcm16(str(p), y, rate)
            q = (np.clip(np.round(y.astype(np.float64) * 32768.0), -32768, 32767).astype(np.float32) * np.float32(1.0 / 32768.0))
        r = REAL_RESAMPLE(q, rate, SR) if rate != SR else q
        files.append(p)
        sums.append(float(r.astype(np.float64).sum()))
        kinds.append((rate, is_f))
    return files, np.array(sums), kinds


def _check_values(res, sums):
    for r in res:
        i = int(os.path.basename(r["file_path"])[1:4])
        assert abs(r["mfcc_mean"][0] - sums[i]) < 1e-3 * max(1.0, abs(sums[i])), (i, r["mfcc_mean"][0], sums[i])


def test_without_a_device_resampler_the_host_resamples(tmp_path):
    files, sums, _ = _corpus(tmp_path, 24)
    calls = []
    ex = _extractor(2, calls, lambda d, l: _FakePlan(d, l, calls))
    res = parallel.process_files(ex, files)
    assert [os.path.basename(r["file_path"]) for r in res] == [f.name for f in files]
    _check_values(res, sums)


def test_off_rate_files_are_resampled_on_the_device(tmp_path, monkeypatch):
    files, sums, kinds = _corpus(tmp_path, 60, float_every=7)
    (tmp_path / "c013.wav").write_bytes(b"not a wav file")
    calls, rs_calls = [], []
    ex = _extractor(2, calls, lambda d, l: _RsPlan(d, l, calls, rs_calls))

    def boom(*a, **k):
        raise AssertionError("wavio.resample called: the host resampled a file the device should have")
    monkeypatch.setattr(wavio, "resample", boom)
    budget = 20000
    res = parallel.process_files(ex, files, max_batch_samples=budget)
    assert [os.path.basename(r["file_path"]) for r in res] == [f.name for i, f in enumerate(files) if i != 13]
    _check_values(res, sums)
    assert rs_calls
    n_off = sum(1 for i, (rate, _) in enumerate(kinds) if rate != SR and i != 13)
    assert sum(len(c["lengths"]) for c in rs_calls) == n_off                    # every off-rate file, once
    assert any(c["fmt"] == _native.FMT_S16 for c in rs_calls)                    # 16-bit mono files went up as int16
    assert any(c["fmt"] == _native.FMT_F32 for c in rs_calls)                    # decoded (float) files as float32
    for c in rs_calls:
        assert c["sr_in"] != SR and c["sr_out"] == SR                           # one file rate per call
        assert (c["out_offsets"] % 4 == 0).all()
        g = np.gcd(c["sr_in"], SR)
        up, down = SR // g, c["sr_in"] // g
        assert (c["out_lengths"] == -(-c["lengths"] * up // down)).all()        # the ceil rule
        assert (np.diff(c["out_offsets"]) >= c["out_lengths"][:-1]).all()       # clips do not overlap
        assert len(c["lengths"]) == 1 or int(c["out_lengths"].sum()) <= budget  # the budget counts resampled samples
        assert len(c["lengths"]) == 1 or int(c["lengths"].sum()) <= budget      # ... and what is uploaded
    assert {c["sr_in"] for c in rs_calls} == {16000, 11025}


def test_upsampled_files_are_budgeted_by_their_output(tmp_path, monkeypatch):
    files, sums, _ = _corpus(tmp_path, 20, rates=(4000,))                        # 4 kHz -> 8 kHz doubles every clip
    calls, rs_calls = [], []
    ex = _extractor(1, calls, lambda d, l: _RsPlan(d, l, calls, rs_calls))
    budget = 30000
    res = parallel.process_files(ex, files, max_batch_samples=budget)
    assert len(res) == 20
    _check_values(res, sums)
    assert len(rs_calls) > 1
    for c in rs_calls:
        assert len(c["lengths"]) == 1 or int(c["out_lengths"].sum()) <= budget


def test_a_failing_resampler_drops_only_its_files(tmp_path):
    files, sums, kinds = _corpus(tmp_path, 48)
    calls, rs_calls = [], []
    ex = _extractor(4, calls, lambda d, l: _RsPlan(d, l, calls, rs_calls, fail_rs=(d == 2)))
    res = parallel.process_files(ex, files)
    names = [os.path.basename(r["file_path"]) for r in res]
    assert names == sorted(names) and 0 < len(res) < 48
    assert len(res) >= 48 - 16                                                   # at most device 2's share is gone
    assert all(c["device"] != 2 for c in rs_calls)
    _check_values(res, sums)


def test_an_unsupported_rate_pair_takes_the_host_path(tmp_path):
    files, sums, _ = _corpus(tmp_path, 30)
    calls, rs_calls = [], []
    ex = _extractor(2, calls, lambda d, l: _RsPlan(d, l, calls, rs_calls, unsupported=(11025,)))
    res = parallel.process_files(ex, files)
    assert [os.path.basename(r["file_path"]) for r in res] == [f.name for f in files]
    _check_values(res, sums)
    assert {c["sr_in"] for c in rs_calls} == {16000}
