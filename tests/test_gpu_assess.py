"""GPU checks of afx_assess_batch / afx_compare_batch and audio_feature_extraction_amd.quality against the numpy
restatement (tests/assess_ref.py), on the smallest shapes where the kernels can go wrong: four rates in one batch, lengths
around the frame and the noise window, a clip of ten workgroups, int16 and float32 from host and device memory.

Tolerances.  Counts and the peak are exact (every clip satisfies assess_ref.silence_is_robust, tests/assess_clips.py).  Mean
squares and RMS values: rtol 1e-5 of the float64 truth, the project's RMS tolerance; the deviation of the long frames'
RMS: 1e-5 of their mean (tests/test_assess_host.py check_record / check_keys).  The scores of a pair: see COMPARE_FLOOR."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import assess_clips as K
from tests import assess_ref as R
from tests import wavfiles as W
from tests.test_assess_host import FILE_KEYS, RTOL, check_keys, check_record

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK_BUDGET = 200000
# The device's correlation, mse and snr of a pair may lie 1000 x as far from the exact value (math.fsum / longdouble over the
# same float32 inputs, assess_ref.pair_exact) as numpy's own float64 evaluation does (np.corrcoef, np.mean): the order of
# summation differs and the clips are short.  Floored at 1e-12 relative.  numpy's measured relative distances on the pairs
# below (correlation, mse, snr; 0: numpy's value is the exact one rounded):
#   unequal    3.3e-16  0  0      identical  1.1e-16  0  0      negated  1.1e-16  0  0
#   dc offset  2.3e-16  0  0      constant   NaN on both sides, 0, 0              wiener   4.5e-16  0  0  (needs the device)
# so 1000 x the distance is at most 4.5e-13 and the floor decides everywhere: 1e-12.  The test prints all three per pair.
COMPARE_FLOOR = 1e-12


@pytest.fixture(scope="module")
def N():
    from audio_feature_extraction_amd import _native
    if _native.device_count() < 1:
        pytest.fail("no GPU visible")
    return _native


@pytest.fixture(scope="module")
def ctx(N):
    return N.Context(0)


def _frames(rates):
    fr = [R.frame_lengths(sr) for sr in rates]
    return np.array([f[0] for f in fr], np.int32), np.array([f[1] for f in fr], np.int32)


def _assess(N, ctx, clips, rates, dtype=np.float32, device=False, order=None, gap=0, **kw):
    """records and statuses of ``clips`` (float32) as ``dtype``, laid out in ``order`` with ``gap`` elements between
    neighbours (NaN / a poison value in the gaps), from host memory or from a device buffer; results in the clips' order"""
    conv = [K.as_s16(c) if dtype == np.int16 else np.ascontiguousarray(c, np.float32) for c in clips]
    n = len(conv)
    order = list(range(n)) if order is None else list(order)
    offs = np.zeros(n, np.int64)
    pos = 0
    for i in order:
        offs[i] = pos
        pos += conv[i].size + gap
    buf = np.full(max(pos, 1), -32768 if dtype == np.int16 else np.nan, dtype)
    for i in order:
        buf[offs[i]:offs[i] + conv[i].size] = conv[i]
    lens = np.array([c.size for c in conv], np.int64)
    fs, fl = _frames(rates)
    if device:
        dev = N.DeviceBuffer(ctx, buf.nbytes)
        dev.upload(buf)
        try:
            return ctx.assess_batch(dev, offs, lens, fs, fl, fmt=N.FMT_S16 if dtype == np.int16 else N.FMT_F32, **kw)
        finally:
            dev.free()
    return ctx.assess_batch(buf, offs, lens, fs, fl, **kw)


@functools.lru_cache(maxsize=None)
def _mixed():
    return [y for _, y, _ in K.MIXED], [sr for _, _, sr in K.MIXED]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("dtype", [np.float32, np.int16], ids=["f32", "s16"])
def test_mixed_rates_in_one_batch(N, ctx, dtype, device):
    clips, rates = _mixed()
    assert sorted(set(rates)) == list(K.RATES) and max(c.size for c in clips) > 9 * 4096
    r = _assess(N, ctx, clips, rates, dtype, device, gap=3 if device else 0)     # device clips at every alignment
    for i, (name, y, sr) in enumerate(K.MIXED):
        v = K.as_s16(y) if dtype == np.int16 else y
        if y.size == 0:
            assert r["status"][i] == N.CLIP_TOO_SHORT and np.isnan(r["rec"][i]).all(), name
            continue
        assert r["status"][i] == N.CLIP_OK, name
        check_record(r["rec"][i], v, *R.frame_lengths(sr), f"{name} {np.dtype(dtype).name} {'device' if device else 'host'}")


def test_segmented_clips_count_exactly(N, ctx):
    keys = list(K.SEGMENTED)
    clips, rates = [K.SEGMENTED[k] for k in keys], [sr for _, sr in keys]
    for dtype in (np.float32, np.int16):
        r = _assess(N, ctx, clips, rates, dtype)
        assert (r["status"] == 0).all()
        for i, (name, sr) in enumerate(keys):
            fs, fl = R.frame_lengths(sr)
            assert tuple(r["rec"][i][:3]) == K.SEG_COUNTS[name], (name, sr)
            assert r["rec"][i][7] == R.frame_rms(clips[i], fl).size, (name, sr)
            check_record(r["rec"][i], K.as_s16(clips[i]) if dtype == np.int16 else clips[i], fs, fl, f"seg {name}/{sr}")
    # another threshold, the clamp at -80 dB, another cap of the noise window
    y = K.SEGMENTED[("a", 16000)]
    check_record(_assess(N, ctx, [y], [16000], threshold_db=-70.0)["rec"][0], y, 160, 1600, "-70 dB", -70.0)
    assert _assess(N, ctx, [y], [16000], threshold_db=-85.0)["rec"][0][1] == 0
    got = _assess(N, ctx, [y], [16000], noise_cap=100)["rec"][0][6]
    assert abs(got - np.mean(y[:100].astype(np.float64) ** 2)) <= RTOL * got
    # frame lengths on the three summing routes of a piece (a lane, a wave, the workgroup) and longer than the clip
    z = K.lead_in(16000, 30011, seed=3)
    for fs, fl in ((1, 63), (2, 64), (3, 1023), (64, 1024), (1024, 5000), (4096, 40000), (441, 2205)):
        rec = ctx.assess_batch(z, [0], [z.size], [fs], [fl])["rec"][0]
        ref = R.record(z, fs, fl)
        for k in (0, 5, 7):
            assert rec[k] == ref[k], (fs, fl, k)
        for k in (3, 4, 6, 8):
            assert abs(rec[k] - ref[k]) <= RTOL * abs(ref[k]), (fs, fl, k, rec[k], ref[k])
        assert abs(rec[9] - ref[9]) <= RTOL * ref[8], (fs, fl)


def test_a_nan_clip_fails_alone(N, ctx):
    clips, rates = _mixed()
    clips, rates = list(clips), list(rates)
    bad = K.lead_in(22050, 20000, seed=9)
    bad[12345] = np.nan
    mid = len(clips) // 2
    with_bad = clips[:mid] + [bad] + clips[mid:]
    for device in (False, True):
        ref = _assess(N, ctx, clips, rates, device=device)
        r = _assess(N, ctx, with_bad, rates[:mid] + [22050] + rates[mid:], device=device)
        assert r["status"][mid] == N.CLIP_NONFINITE and np.isnan(r["rec"][mid]).all()
        np.testing.assert_array_equal(np.delete(r["status"], mid), ref["status"])
        np.testing.assert_array_equal(np.delete(r["rec"], mid, axis=0), ref["rec"])          # bit-identical, NaN rows alike
    inf = bad.copy()
    inf[12345] = -np.inf
    assert _assess(N, ctx, [inf], [22050])["status"][0] == N.CLIP_NONFINITE


def test_records_do_not_depend_on_the_batch(N, ctx):
    clips, rates = _mixed()
    n = len(clips)
    ref = _assess(N, ctx, clips, rates)
    again = _assess(N, ctx, clips, rates)
    np.testing.assert_array_equal(again["rec"], ref["rec"])
    for name, r in (("reversed", _assess(N, ctx, clips, rates, order=range(n - 1, -1, -1), gap=5)),
                    ("device", _assess(N, ctx, clips, rates, device=True)),
                    ("device, unaligned", _assess(N, ctx, clips, rates, device=True, order=range(n - 1, -1, -1), gap=1))):
        np.testing.assert_array_equal(r["status"], ref["status"], err_msg=name)
        np.testing.assert_array_equal(r["rec"], ref["rec"], err_msg=name)
    for i in range(n):
        if clips[i].size:
            solo = _assess(N, ctx, [clips[i]], [rates[i]])
            np.testing.assert_array_equal(solo["rec"][0], ref["rec"][i], err_msg=K.MIXED[i][0])
    # the same clips in another order are the same records in that order
    perm = np.random.default_rng(1).permutation(n)
    r = _assess(N, ctx, [clips[i] for i in perm], [rates[i] for i in perm])
    np.testing.assert_array_equal(r["rec"], ref["rec"][perm])


def _pairs():
    y = K.lead_in(16000, 20000, seed=4)
    t = np.arange(20000) * 0.05
    dc, dc2 = (0.5 + 1e-3 * np.sin(t)).astype(np.float32), (0.5 + 1e-3 * np.sin(t + 0.3)).astype(np.float32)
    return [("unequal", y, (y[:7001] * np.float32(0.8) + np.float32(0.01))), ("identical", y, y.copy()), ("negated", y, -y),
            ("dc offset", dc, dc2), ("constant", np.full(5000, 0.25, np.float32), y[:5000].copy())]


def _compare(N, ctx, pairs, device=False, fmt16=False):
    conv = (lambda a: K.as_s16(a)) if fmt16 else (lambda a: np.ascontiguousarray(a, np.float32))
    refs, degs = [conv(p[1]) for p in pairs], [conv(p[2]) for p in pairs]
    rl, dl = np.array([r.size for r in refs], np.int64), np.array([d.size for d in degs], np.int64)
    both = np.concatenate(refs + degs)
    offs = N.packed_offsets(np.concatenate([rl, dl]))
    m = len(pairs)
    if device:
        dev = N.DeviceBuffer(ctx, both.nbytes)
        dev.upload(both)
        try:
            return ctx.compare_batch(dev, offs[:m], rl, dev, offs[m:], dl, fmt=N.FMT_S16 if fmt16 else N.FMT_F32)
        finally:
            dev.free()
    return ctx.compare_batch(both, offs[:m], rl, both, offs[m:], dl)


def _check_pair(got, r, d, what):
    """quality's scores of a pair against the exact evaluation, within 1000 x numpy's own distance from it"""
    ex, st = R.pair_exact(r, d), R.pair_stats(r, d)
    for k in ("correlation", "mse", "snr"):
        if np.isnan(ex[k]):
            assert np.isnan(got[k]) and np.isnan(st[k]), (what, k)
            continue
        dist = abs(st[k] - ex[k]) / abs(ex[k]) if ex[k] else abs(st[k])
        tol = max(1000 * dist, COMPARE_FLOOR)
        print(f"{what:12s} {k:12s} numpy {dist:.2e}  device {abs(got[k] - ex[k]) / (abs(ex[k]) or 1):.2e}  allowed {tol:.2e}")
        assert abs(got[k] - ex[k]) <= tol * (abs(ex[k]) or 1), (what, k, got[k], ex[k], tol)
    want = R.stoi_score(ex["correlation"], ex["mse"], ex["snr"])
    assert (np.isnan(want) and np.isnan(got["stoi"])) or abs(got["stoi"] - want) <= 1e-11, (what, got["stoi"], want)


def test_compare_batch(N, ctx):
    from audio_feature_extraction_amd import effects, quality
    pairs = _pairs()
    noisy = K.lead_in(22050, 30000, seed=6) + (0.01 * np.random.default_rng(7).standard_normal(30000)).astype(np.float32)
    pairs.append(("wiener", noisy, effects.wiener_filter(noisy, 22050)))
    got = quality.compare_batch([(r, d) for _, r, d in pairs])
    for (name, r, d), g in zip(pairs, got):
        _check_pair(g, r, d, name)
    assert got[1]["snr"] == 100 and got[1]["mse"] == 0 and got[1]["stoi"] == 1.0          # identical: no noise at all
    assert got[2]["correlation"] == pytest.approx(-1.0, abs=1e-12) and got[0]["correlation"] > 0.99
    assert np.isnan(got[4]["correlation"]) and np.isnan(got[4]["stoi"])                  # a constant reference
    assert quality.stoi_like(pairs[3][1], pairs[3][2]) == got[3]["stoi"]
    # the record itself: n and status, every layout bit-identical, a pair alone as in the batch
    ref = _compare(N, ctx, pairs)
    assert ref["rec"][:, 0].tolist() == [min(r.size, d.size) for _, r, d in pairs] and (ref["status"] == 0).all()
    np.testing.assert_array_equal(_compare(N, ctx, pairs, device=True)["rec"], ref["rec"])
    np.testing.assert_array_equal(_compare(N, ctx, pairs[::-1])["rec"], ref["rec"][::-1])
    for i, p in enumerate(pairs):
        np.testing.assert_array_equal(_compare(N, ctx, [p])["rec"][0], ref["rec"][i], err_msg=p[0])
    s16 = _compare(N, ctx, pairs, fmt16=True)
    np.testing.assert_array_equal(_compare(N, ctx, pairs, device=True, fmt16=True)["rec"], s16["rec"])
    for i, (name, r, d) in enumerate(pairs):
        host = N.compare_host(K.as_s16(r), K.as_s16(d))["rec"]
        np.testing.assert_allclose(s16["rec"][i], host, rtol=1e-9, atol=1e-9, err_msg=name)
    # a pair with nothing in common, a NaN on one side
    bad = pairs[0][2].copy()
    bad[5000] = np.nan
    r = _compare(N, ctx, [pairs[0], ("empty", pairs[0][1], np.zeros(0, np.float32)), ("nan", pairs[0][1], bad), pairs[1]])
    assert r["status"].tolist() == [0, N.CLIP_TOO_SHORT, N.CLIP_NONFINITE, 0] and np.isnan(r["rec"][1:3]).all()
    np.testing.assert_array_equal(r["rec"][[0, 3]], ref["rec"][[0, 1]])


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_assess import _assess, _compare, _mixed, _pairs
from audio_feature_extraction_amd import _native as N
ctx = N.Context(0)
clips, rates = _mixed()
out = {}
for name, dtype, device in (("f32", np.float32, False), ("s16", np.int16, False), ("dev", np.float32, True)):
    r = _assess(N, ctx, clips, rates, dtype, device)
    out["rec_" + name], out["status_" + name] = r["rec"], r["status"]
c = _compare(N, ctx, _pairs())
out["cmp"], out["cmp_status"] = c["rec"], c["status"]
np.savez(sys.argv[2], **out)
"""


def test_chunked_batch_equals_one_chunk(N, ctx, tmp_path):
    clips, rates = _mixed()
    lengths = [c.size for c in clips]
    for fmt, mem in ((N.FMT_F32, N.MEM_HOST), (N.FMT_S16, N.MEM_HOST), (N.FMT_F32, N.MEM_DEVICE)):
        assert N.stft_chunks(lengths, N.assess_cost(N.COST_ASSESS, fmt, mem), CHUNK_BUDGET).max() + 1 >= 3
        assert N.stft_chunks(lengths, N.assess_cost(N.COST_ASSESS, fmt, mem), 2 << 30).max() == 0
    pairs = _pairs()
    assert N.stft_chunks([min(r.size, d.size) for _, r, d in pairs], N.assess_cost(N.COST_COMPARE), CHUNK_BUDGET).max() + 1 >= 3
    dst = str(tmp_path / "chunked.npz")
    env = dict(os.environ, AFX_TEST_ASSESS_BUDGET=str(CHUNK_BUDGET))
    subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _CHILD, ROOT, dst], env=env, check=True, timeout=150)
    z = np.load(dst)
    for name, dtype, device in (("f32", np.float32, False), ("s16", np.int16, False), ("dev", np.float32, True)):
        r = _assess(N, ctx, clips, rates, dtype, device)
        np.testing.assert_array_equal(z["status_" + name], r["status"], err_msg=name)
        np.testing.assert_array_equal(z["rec_" + name], r["rec"], err_msg=name)
    c = _compare(N, ctx, pairs)
    np.testing.assert_array_equal(z["cmp"], c["rec"])
    np.testing.assert_array_equal(z["cmp_status"], c["status"])


def test_assess_files(N, tmp_path):
    from audio_feature_extraction_amd import quality, wavio
    specs = (("teacher.wav", 16000, "s32", 1, K.lead_in(16000, 24000, seed=1)),
             ("cd.wav", 22050, "s16", 1, K.SEGMENTED[("a", 22050)]),
             ("stereo24.wav", 44100, "s24", 2, K.lead_in(44100, 50000, seed=2)))
    paths = []
    for name, sr, kind, ch, y in specs:
        p = str(tmp_path / name)
        W.write_wav(p, W.quantize(y, kind, ch), sr, kind)
        paths.append(p)
    cut = str(tmp_path / "cut.wav")
    blob = open(paths[1], "rb").read()
    open(cut, "wb").write(blob[:44 + 2 * 30001 + 1])                 # the header still promises the whole clip
    webm, missing = str(tmp_path / "student.webm"), str(tmp_path / "absent.wav")
    open(webm, "wb").write(b"\x1a\x45\xdf\xa3" + bytes(300))
    every = paths + [cut, webm, missing]
    res = quality.assess_files(every)
    err_keys = ["file_path", "file_name", "assessment_ok", "error"]
    assert [list(r) for r in res] == [FILE_KEYS] * 4 + [err_keys] * 2
    for r, p in zip(res, every):
        assert r["file_path"] == p and r["file_name"] == os.path.basename(p)
    assert not res[4]["assessment_ok"] and not res[5]["assessment_ok"] and res[4]["error"] and res[5]["error"]
    want_fmt = ((16000, "32-bit", 1, 1.5, True), (22050, "PCM_16", 1, K.SEGMENTED[("a", 22050)].size / 22050, False),
                (44100, "PCM_24", 2, 50000 / 44100, False), (22050, "PCM_16", 1, 30001 / 22050, False))
    for r, p, f in zip(res, paths + [cut], want_fmt):
        assert (r["sample_rate"], r["bit_depth"], r["channels"], r["duration"], r["format_ok"]) == f, p
        y, sr = wavio.load(p, None)
        a = quality.assess(y, sr)
        for k in a:                                                  # key for key: the same kernel on the same samples
            if k != "rms_std":
                assert r[k] == a[k], (p, k, r[k], a[k])
        check_keys({k: (a[k] if k == "rms_std" else r[k]) for k in a}, y, sr, p)
        assert r["assessment_ok"] == all(r[k] for k in ("format_ok", "silence_ok", "volume_ok", "stability_ok", "snr_ok"))
    assert tuple(R.record(wavio.load(cut, None)[0], 220, 2205)[:1]) == (1 + 30001 // 220,)
    assert quality.assess_files([paths[2]], expected={"sample_rate": 44100, "subtype": "PCM_24", "channels": 2})[0]["format_ok"] is True
    assert quality.assess_files([]) == []


def test_evaluate_noise_reduction(N):
    from audio_feature_extraction_amd import effects, quality
    sr = 22050
    rng = np.random.default_rng(11)
    n = 3 * sr
    y = (0.02 * rng.standard_normal(n)).astype(np.float32)                      # noise throughout, a tone behind a 0.4 s lead-in
    y[int(0.4 * sr):] += K.tone(sr, n - int(0.4 * sr))
    got = quality.evaluate_noise_reduction(y, sr)
    assert list(got) == ["original", "spectral_subtraction", "wiener_filter"] and all(list(v) == ["snr", "stoi"] for v in got.values())
    outs = {"original": y, "spectral_subtraction": effects.spectral_subtraction(y, sr), "wiener_filter": effects.wiener_filter(y, sr)}
    for k, d in outs.items():
        assert R.snr_is_robust(d), k
        want = R.estimate_snr(d)["snr"]
        assert abs(got[k]["snr"] - want) <= RTOL * abs(want), (k, got[k]["snr"], want)
        ex = R.pair_exact(y, d)
        assert abs(got[k]["stoi"] - R.stoi_score(ex["correlation"], ex["mse"], ex["snr"])) <= 1e-11, k
    assert got["original"]["stoi"] == 1.0
    assert got["wiener_filter"]["snr"] > got["original"]["snr"]                  # the lead-in is what the filter removes
    # a reference of its own, shorter than the signal
    clean = np.zeros(n, np.float32)
    clean[int(0.4 * sr):] = K.tone(sr, n - int(0.4 * sr))
    g2 = quality.evaluate_noise_reduction(y, sr, reference=clean[:2 * sr])
    ex = R.pair_exact(clean[:2 * sr], outs["wiener_filter"])
    assert abs(g2["wiener_filter"]["stoi"] - R.stoi_score(ex["correlation"], ex["mse"], ex["snr"])) <= 1e-11
    assert g2["original"]["snr"] == got["original"]["snr"]
