"""Frame lengths that are not powers of two on the GPU (k_frames_mr): 400 / 160 at 16 kHz -- the 25 ms / 10 ms speech
front end of the reference's experiment extractors -- and one shape per radix mix, against the CPU oracle through
tests/parity.py, plus everything that rides on such a plan (ZCR, pYIN, the class API, batch_process)."""
import numpy as np
import pytest

from audio_feature_extraction_amd import _native as N
from audio_feature_extraction_amd import wavio
from audio_feature_extraction_amd.synth import make_clip
from oracle import cpu_ref as R
from oracle import pyin_ref as P
from tests.f0_shapes import voiced_tone
from tests.parity import check_frames, check_stats

pytestmark = pytest.mark.gpu

# name -> sr, n_fft, hop, n_mfcc, n_mels; the N2 = n_fft / 2 schedule each one walks
SHAPES = {
    "400-40": (16000, 400, 160, 13, 40),       # 5 5 8: 40 and 25 butterflies per pass, fewer than the 64 lanes
    "400-128": (16000, 400, 160, 13, 128),     # the same with librosa's default filter count: single-tap filters
    "320": (16000, 320, 160, 13, 128),         # 5 4 8
    "384": (22050, 384, 96, 13, 128),          # 3 8 8
    "1200": (48000, 1200, 480, 20, 128),       # 3 5 5 8: more butterflies than lanes (200 > 64, 120 > 64)
    "480": (16000, 480, 160, 13, 128),         # 3 5 4 4, hop is not n_fft / 4
}


@pytest.fixture(scope="module")
def ctx():
    c = N.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def plans(ctx):
    cache = {}

    def get(name):
        if name not in cache:
            sr, n_fft, hop, K, M = SHAPES[name]
            cache[name] = N.Plan(ctx, N.make_params(sr, n_fft, hop, K, M, "hamming", 0.97))
        return cache[name]
    yield get
    for p in cache.values():
        p.close()


def oracle(y, name, dtype=np.float32):
    sr, n_fft, hop, K, M = SHAPES[name]
    return R.extract_stats(y, sr=sr, frame_length=n_fft, hop_length=hop, n_mfcc=K, n_mels=M, dtype=dtype, return_frames=True)


def pack(clips, dtype=np.float32):
    lengths = np.array([c.size for c in clips], np.int64)
    pad = (lengths + 3) // 4 * 4
    offsets = np.concatenate([[0], np.cumsum(pad)[:-1]]).astype(np.int64)
    buf = np.zeros(int(pad.sum()), dtype)
    for c, o in zip(clips, offsets):
        buf[o:o + c.size] = c
    return buf, offsets, lengths


def run_one(plan, y, **kw):
    return plan.extract_batch(np.ascontiguousarray(y, np.float32), np.zeros(1, np.int64), np.array([y.size], np.int64),
                              want_frames=True, **kw)


@pytest.mark.parametrize("name", list(SHAPES))
def test_per_frame_and_stats_parity(plans, name):
    sr, n_fft, hop, K, M = SHAPES[name]
    plan = plans(name)
    for idx, speechy, secs in ((3, False, 0.45), (8, True, 0.6)):
        y = make_clip(idx, sr, secs, speechy=speechy)
        out = run_one(plan, y)
        assert out["status"][0] == 0
        ref = oracle(y, name)
        assert tuple(out["trim"][0]) == ref["trim"]
        assert out["nframes"][0] == ref["mfcc"].shape[1]
        what = f"{name} clip{idx}"
        check_frames(out["frames"][0], ref, what)
        check_stats(out["stats"][0], ref, K, what)
        # the float64 truth adjudicates: the GPU must be as close to it as the f32 oracle is (x4)
        truth = oracle(y, name, dtype=np.float64)
        sc = np.abs(truth["mfcc"]).max(axis=1, keepdims=True)
        e_gpu = (np.abs(out["frames"][0]["mfcc"] - truth["mfcc"]) / sc).max()
        e_ref = (np.abs(ref["mfcc"] - truth["mfcc"]) / sc).max()
        print(f"{what}: gpu-to-f64 {e_gpu:.2e}, oracle-f32-to-f64 {e_ref:.2e}")
        assert e_gpu <= max(4 * e_ref, 2e-5), f"{what}: gpu {e_gpu:.2e} vs oracle-f32 {e_ref:.2e}"


def test_filter_groups_without_a_bin(ctx):
    """64 filters between 1000 and 1100 Hz against the 40 Hz bins of 16000 / 400: two of the four 16-filter groups have no
    bin under any filter (tests/test_mixed_radix_host.py shows their empty block lists).  Their log-mel rows are
    10 log10(amin) and nothing is read for them; the MFCCs keep the parity of every other shape."""
    sr, n_fft, hop, K, M = 16000, 400, 160, 13, 64
    plan = N.Plan(ctx, N.make_params(sr, n_fft, hop, K, M, "hamming", 0.97, fmin=1000.0, fmax=1100.0))
    try:
        for idx, speechy in ((5, False), (6, True)):
            y = make_clip(idx, sr, 0.5, speechy=speechy)
            out = run_one(plan, y)
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                ref = R.extract_stats(y, sr=sr, frame_length=n_fft, hop_length=hop, n_mfcc=K, n_mels=M, return_frames=True,
                                      fmin=1000.0, fmax=1100.0)
            assert out["status"][0] == 0 and tuple(out["trim"][0]) == ref["trim"]
            check_frames(out["frames"][0], ref, f"empty groups clip{idx}")
            check_stats(out["stats"][0], ref, K, f"empty groups clip{idx}")
    finally:
        plan.close()


def test_preprocess_bit_exact_and_trim_index(plans):
    plan = plans("400-40")
    for idx, speechy in ((0, False), (1, True)):
        y = make_clip(idx, 16000, 0.6, speechy=speechy)
        y_pre, s, e, st = plan.preprocess(y)
        ref_pre = R.preemphasis(y, 0.97)
        _, (rs, re) = R.trim(ref_pre)
        assert st == 0
        np.testing.assert_array_equal(y_pre, ref_pre)          # float32 bit-exact
        assert (s, e) == (rs, re)


def test_edge_clips_in_one_batch(plans):
    """Nine frames, eight frames (TOO_SHORT, RMS statistics still there), less than one frame, digital silence, and a NaN
    clip between two good ones."""
    sr, n_fft, hop, K, M = SHAPES["400-40"]
    plan = plans("400-40")
    nine = make_clip(11, sr, 0.5)[:8 * hop + 37]                   # T = 1 + 1317 // 160 = 9
    eight = make_clip(12, sr, 0.5)[:7 * hop + 150]                 # T = 8
    tiny = make_clip(13, sr, 0.5)[:300]                            # shorter than one frame: T = 2
    good_a, good_b = make_clip(14, sr, 0.5), make_clip(15, sr, 0.45, speechy=True)
    bad = make_clip(16, sr, 0.5).copy()
    bad[777] = np.nan
    clips = [nine, eight, tiny, np.zeros(sr // 2, np.float32), good_a, bad, good_b]
    out = plan.extract_batch(*pack(clips), want_frames=True)
    assert out["status"].tolist() == [0, N.CLIP_TOO_SHORT, N.CLIP_TOO_SHORT, 0, 0, N.CLIP_NONFINITE, 0]
    ref9 = oracle(nine, "400-40")
    assert out["nframes"][0] == 9 == ref9["mfcc"].shape[1]
    for i in (0, 3, 4, 6):
        ref = oracle(clips[i], "400-40")
        assert tuple(out["trim"][i]) == ref["trim"]
        check_frames(out["frames"][i], ref, f"edge{i}")
        check_stats(out["stats"][i], ref, K, f"edge{i}")
    assert out["stats"][3][0] == pytest.approx(-100.0 * np.sqrt(M), rel=1e-5)       # silence: every log-mel is 10 log10(amin)
    for i in (1, 2):
        with pytest.raises(ValueError):
            oracle(clips[i], "400-40")
        yp, _ = R.preprocess_audio(clips[i])
        e = R.extract_energy(yp, n_fft, hop)
        assert out["nframes"][i] == 1 + yp.size // hop < 9
        np.testing.assert_allclose(out["stats"][i][4 * K:4 * K + 3], [e["energy_mean"], e["energy_std"], e["energy_range"]],
                                   rtol=1e-5, atol=1e-8)
    # the NaN clip's neighbours: what they give alone, bit for bit
    for i in (4, 6):
        alone = run_one(plan, clips[i])
        np.testing.assert_array_equal(alone["stats"][0], out["stats"][i])
        np.testing.assert_array_equal(alone["frames"][0]["mfcc"], out["frames"][i]["mfcc"])


def test_ragged_mixed_format_batch_equals_single_clips(plans):
    """24 clips of unequal length in one batch give, clip by clip, what each gives alone: statistics, frame counts, trim
    indices and every per-frame row, bit for bit.  A batch holds one sample format, so "mixed S16 / F32" is the same 24
    clips once as an F32 batch and once as an S16 batch (their values agree exactly: / 32768 is exact), plus an F32 batch
    packed at odd addresses."""
    sr, n_fft, hop, K, M = SHAPES["400-40"]
    plan = plans("400-40")
    rng = np.random.default_rng(7)
    clips = [make_clip(100 + i, sr, 0.4 + 0.2 * float(rng.random()), speechy=bool(i % 3 == 1))[:int(rng.integers(6400, 9600))]
             for i in range(24)]
    q = [np.clip(np.rint(c.astype(np.float64) * 32768), -32768, 32767).astype(np.int16) for c in clips]
    qf = [a.astype(np.float32) / np.float32(32768.0) for a in q]
    f32 = plan.extract_batch(*pack(qf), want_frames=True)
    s16 = plan.extract_batch(*pack(q, np.int16), fmt=N.FMT_S16, want_frames=True)
    assert (f32["status"] == 0).all() and (s16["status"] == 0).all()
    np.testing.assert_array_equal(f32["stats"], s16["stats"])          # / 32768 is exact
    # unaligned packing: every block takes the clamped loads at odd addresses
    offs2 = np.concatenate([[1], 1 + np.cumsum([c.size + 1 for c in qf])[:-1]]).astype(np.int64)
    buf2 = np.zeros(int(offs2[-1] + qf[-1].size + 8), np.float32)
    for c, o in zip(qf, offs2):
        buf2[o:o + c.size] = c
    un = plan.extract_batch(buf2, offs2, np.array([c.size for c in qf], np.int64))
    np.testing.assert_array_equal(un["stats"], f32["stats"])
    for i in range(24):
        one = run_one(plan, qf[i])
        for batch in (f32, s16):
            np.testing.assert_array_equal(one["stats"][0], batch["stats"][i])
            assert one["nframes"][0] == batch["nframes"][i] and tuple(one["trim"][0]) == tuple(batch["trim"][i])
            assert set(one["frames"][0]) == set(batch["frames"][i])
            for k, rows in one["frames"][0].items():
                np.testing.assert_array_equal(rows, batch["frames"][i][k], err_msg=f"clip {i} {k}")
    for i in (0, 1):
        ref = oracle(qf[i], "400-40")
        check_stats(f32["stats"][i], ref, K, f"ragged{i}")


def test_extract_frame_features_at_400_160(tmp_path):
    """The npz layout of 04_feature_extraction_experiment/feature_extraction.py at its own 400 / 160 framing: shapes,
    ZCR exactly, the pYIN track frame for frame on a single-source clip (the criterion of tests/test_gpu_f0.py)."""
    from audio_feature_extraction_amd import AudioFeatureExtractor
    sr = 16000
    sil = np.zeros(int(0.15 * sr), np.float32)
    y = np.concatenate([sil, voiced_tone(sr, 196.0, 0.6, vib=0.015, seed=4), sil])
    p = str(tmp_path / "tone.wav")
    wavio.write_wav_pcm16(p, y, sr)
    yd = wavio.load(p, sr)[0]
    ex = AudioFeatureExtractor(sr=sr, frame_length=400, hop_length=160, n_mels=40, device=0)
    fr = ex.extract_frame_features(p)
    yp, _ = R.preprocess_audio(yd)
    T = 1 + yp.size // 160
    assert fr["mfcc"].shape == (39, T) and fr["f0"].shape == (T,) and fr["energy"].shape == (T,) and fr["zcr"].shape == (T,)
    np.testing.assert_array_equal(fr["zcr"], R.zero_crossing_rate(yp, 400, 160))
    ref = R.extract_stats(yd, sr=sr, frame_length=400, hop_length=160, n_mfcc=13, n_mels=40, return_frames=True)
    got = {"mfcc": fr["mfcc"][:13], "mfcc_delta": fr["mfcc"][13:26], "mfcc_delta2": fr["mfcc"][26:], "rms": fr["energy"][None, :]}
    check_frames(got, ref, "frame features")
    f0_ref, _, _ = P.pyin(yp, sr=sr, frame_length=400, hop_length=160)
    assert fr["f0"].shape == f0_ref.shape
    same = np.isnan(fr["f0"]) == np.isnan(f0_ref)
    v = ~np.isnan(f0_ref) & ~np.isnan(fr["f0"])
    same[v] &= np.abs(fr["f0"][v] - f0_ref[v]) <= 1e-9 * f0_ref[v]
    print(f"[f0 400/160] {int((~same).sum())} of {same.size} frames differ; voiced {int(v.sum())}")
    assert v.sum() > T // 3 and same.all(), np.flatnonzero(~same)[:10]
    s = ex.extract_f0(yp)
    rf = P.extract_f0(yp, sr=sr, frame_length=400, hop_length=160)
    np.testing.assert_allclose([s["f0_mean"], s["f0_std"], s["f0_missing_rate"], s["f0_quality"]],
                               [rf["f0_mean"], rf["f0_std"], rf["f0_missing_rate"], rf["f0_quality"]], rtol=1e-10, atol=1e-12)
    # save / align: the consumers of this layout
    ex.save_frame_features(fr, str(tmp_path / "tone.npz"))
    assert np.load(str(tmp_path / "tone.npz"))["mfcc"].shape == (39, T)
    al = ex.align_files(p, p)
    assert al["dtw_distance"] == pytest.approx(0.0, abs=1e-6) and len(al["path"]) == T


def test_batch_process_equals_extract_features(tmp_path):
    from audio_feature_extraction_amd import AudioFeatureExtractor
    sr = 16000
    for i in range(6):
        wavio.write_wav_pcm16(str(tmp_path / f"c{i}.wav"), make_clip(40 + i, sr, 0.4 + 0.04 * i, speechy=bool(i % 2)), sr)
    ex = AudioFeatureExtractor(sr=sr, frame_length=400, hop_length=160, n_mels=40, device=0)
    res = ex.batch_process(str(tmp_path))
    assert len(res) == 6
    for d in res:
        one = ex.extract_features(d["file_path"])
        assert list(one) == list(d)
        for k in one:
            if k == "file_path":
                assert one[k] == d[k]
            else:
                np.testing.assert_array_equal(np.asarray(one[k]), np.asarray(d[k]), err_msg=k)


def test_power_of_two_plan_is_unchanged_by_a_400_plan(ctx):
    """Tables and dispatch do not leak between plans: 1024 / 256 before and after a 400 / 160 plan in one process."""
    clips = [make_clip(60 + i, 22050, 0.5, speechy=bool(i % 2)) for i in range(4)]
    args = pack(clips)

    def pow2():
        pl = N.Plan(ctx, N.make_params(22050, 1024, 256, 13))
        try:
            return pl.extract_batch(*args)
        finally:
            pl.close()
    before = pow2()
    mr = N.Plan(ctx, N.make_params(16000, 400, 160, 13, 40))
    y = make_clip(70, 16000, 0.5)
    a = run_one(mr, y)
    mid = pow2()
    b = run_one(mr, y)
    mr.close()
    after = pow2()
    for o in (mid, after):
        np.testing.assert_array_equal(before["stats"], o["stats"])
        np.testing.assert_array_equal(before["trim"], o["trim"])
    np.testing.assert_array_equal(a["stats"], b["stats"])


def test_hop_too_large_for_lds_is_refused(ctx):
    with pytest.raises(NotImplementedError, match="160 KiB"):
        N.Plan(ctx, N.make_params(48000, 1920, 1920, 13))
