"""GPU tests of afx_groups_batch, the fused pass over the spectral, harmonic, timbre and rhythm groups, and of
``AudioFeatureExtractor.extract_signal_features_batch`` on top of it.

  bit equality    with the preprocess, every field the separate entry points also compute -- afx_sosfiltfilt_batch to a device
                  buffer, then afx_hpss_batch, afx_chroma_batch and afx_rhythm_batch on it -- is array-equal to theirs
  restatement     tests/groups_ref.py on inputs whose tuning and tempo are robust (tuning_is_robust, tempo_is_robust of the
                  preprocessed signal; tests/test_groups_host.py::test_chosen_inputs_are_robust pins that on the CPU): the bounds are those of the
                  per-group tests -- test_gpu_spectral.py::test_extract_spectral_features_dict, test_gpu_hpss.py::
                  test_stats_match_the_oracle, test_gpu_chroma.py's 1e-5 / 1e-4 of |mean| + std.  White noise is in none of
                  these: its tuning histogram has no robust maximum at any level tried, so it runs in the exact tests only.
  k_spec_rows     frame by frame through AFX_GROUPS_STORE_DESC, with the assertions of test_gpu_spectral.py::
                  test_spectral_descriptors_match_the_oracle
  independence    a clip alone, a batch cut into chunks (fresh process: the budget is read once) and a batch with failed clips
                  give array-equal records
  subsets         a group alone equals its slice of the all-groups record, array-equal

Shapes are the kernels' edges: T = 1 and 2, the 16-frame tile of the MFMA and tempogram kernels, the 64-frame tile of
k_hpss_mask, one clip past it."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from audio_feature_extraction_amd.synth import make_clip
from oracle import cpu_ref
from tests import chroma_ref, groups_ref as G, rhythm_ref, wavfiles

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (19, 511, 512, 513, 15 * 512, 16 * 512, 16 * 512 + 1, 63 * 512, 64 * 512 + 1, 70 * 512 + 100)
CHUNK_BUDGET = 3000000


@pytest.fixture(scope="module")
def N():
    from audio_feature_extraction_amd import _native
    if _native.device_count() < 1:
        pytest.fail("no GPU visible")
    return _native


@pytest.fixture(scope="module")
def plans(N):
    out = {}
    for sr in (8000, 16000, 22050, 44100):
        ctx = N.Context(0)
        out[sr] = (ctx, N.Plan(ctx, N.make_params(sr, 2048, 512, 13, 128, "hann")))
    return out


def _pack(sigs):
    lengths = np.array([s.size for s in sigs], np.int64)
    offsets = np.zeros(len(sigs), np.int64)
    offsets[1:] = np.cumsum(lengths)[:-1]
    return np.concatenate(sigs).astype(np.float32), offsets, lengths


@functools.lru_cache(maxsize=None)
def _batch(sr=22050):
    """the edge shapes as speech-like clips, noise and a click train, with an empty clip, an 18-sample clip and a clip that
    holds a NaN mixed in (indices 3, 7 and 10)"""
    rng = np.random.default_rng(5)
    sigs = []
    for k, n in enumerate(LENGTHS):
        if k % 3 == 0:
            y = make_clip(80 + k, sr, (n + 1) / sr, speechy=True)[:n]
        elif k % 3 == 1:
            y = (0.3 * rng.standard_normal(n)).astype(np.float32)
        else:
            y = rhythm_ref.clicks(sr, 150, seconds=(n + 1) / sr)[:n]
        assert y.size == n
        sigs.append(np.ascontiguousarray(y, np.float32))
    bad = sigs[5].copy()
    bad[4000] = np.nan
    sigs.insert(3, np.zeros(0, np.float32))
    sigs.insert(7, sigs[0][:18].copy())
    sigs.insert(10, bad)
    return tuple(sigs)


FAILED = {3: 1, 7: 1, 10: 2}          # index -> afx_clip_status with the preprocess


def _flat(out):
    return {k: np.asarray(out[k]) for k in ("stats", "tuning", "lag", "status")}


# ---- 1. bit equality with the separate entry points ---------------------------------------------------------------------
@pytest.mark.parametrize("sr", [22050, 16000])
def test_fields_equal_the_separate_entry_points(plans, N, sr):
    ctx, plan = plans[sr]
    y, off, ln = _pack(_batch(sr))
    got = plan.groups_batch(y, off, ln, preprocess=True)          # absent before this feature: AttributeError
    sos = N.butter_sos(5, 200 / (sr / 2), True)
    ooff = N.packed_offsets(ln, 4)
    dev = N.DeviceBuffer(ctx, 4 * int(ooff[-1] + ln[-1]) + 64)
    try:
        f = ctx.sosfiltfilt_batch(y, off, ln, sos, 18, mode=N.FILT_EXPERIMENT, preemph=0.98, out=dev, out_offsets=ooff)
        live = np.where(f["status"] == N.CLIP_OK, ln, 0)          # a failed clip's range of dev was never written
        h = plan.hpss_batch(dev, ooff, live, mem=N.MEM_DEVICE, want_harm=False)
        c = plan.chroma_batch(dev, ooff, live, mem=N.MEM_DEVICE, want_chroma=False)
        r = plan.rhythm_batch(dev, ooff, live, mem=N.MEM_DEVICE, want_env=False, want_acmean=True)
    finally:
        dev.free()
    np.testing.assert_array_equal(got["status"], f["status"])
    assert {i: int(s) for i, s in enumerate(got["status"]) if s} == FAILED
    ok = got["status"] == N.CLIP_OK
    s = got["stats"]
    assert np.isnan(s[~ok]).all() and np.isfinite(s[ok][:, 12:]).all()
    np.testing.assert_array_equal(s[ok, 8:10], h["stats"][ok, 0:2])
    np.testing.assert_array_equal(s[ok, 12:16], c["stats"][ok])
    np.testing.assert_array_equal(s[ok, 18], r["tempo"][ok])
    np.testing.assert_array_equal(s[ok, 19:21], r["stats"][ok])
    np.testing.assert_array_equal(got["tuning"][ok], c["tuning"][ok])
    np.testing.assert_array_equal(got["lag"][ok], r["lag"][ok])
    np.testing.assert_array_equal(s[ok, 21], r["acmean"][np.flatnonzero(ok), r["lag"][ok]])
    np.testing.assert_array_equal(s[ok, 22:24], f["peak"][ok])
    assert (got["tuning"][~ok] == 0.0).all() and (got["lag"][~ok] == 0).all()


# ---- 2. against the restatement ---------------------------------------------------------------------------------------------
def _beat(sr, n, bpm):
    return np.exp(-np.mod(np.arange(n) / float(sr), 60.0 / bpm) / 0.05)


@functools.lru_cache(maxsize=None)
def _robust_inputs(sr):
    """(name, signal, preprocess): speech-like clips, a chord gated at a tempo, a click track, taken as given or sent through
    the preprocess -- every one with a robust tuning, a robust tempo and well-conditioned contrast statistics in the signal
    the groups see (tests/test_groups_host.py::test_chosen_inputs_are_robust).  Every one carries a noise floor, as a
    recording does: the descriptors are taken from float32 power rows, here as in afx_spectral_batch, so a frame whose
    magnitudes lie below 1e-19 -- the digital silence between make_clip's syllables -- has all-zero rows and a centroid of 0.
    Behind the preprocess only the chords qualify: groups_ref.contrast_is_well_conditioned says why."""
    n = 3 * sr
    chord = lambda bpm: (chroma_ref.tones(sr, n, (220.0, 440.0, 1320.0), noise=0.002) * (0.05 + _beat(sr, n, bpm))).astype(np.float32)
    out = [(f"speech{i}", (make_clip(i, sr, 3.0, speechy=True) + 1e-3 * np.random.default_rng(i).standard_normal(n)).astype(np.float32), False)
           for i in (63, 68)]
    out.append(("clicks120", rhythm_ref.clicks(sr, 120, seconds=4.0), False))
    if sr == 22050:
        out.append(("tones120", chord(120), False))
    out += [(f"tones{bpm}_pre", chord(bpm), True) for bpm in ((120, 150) if sr == 22050 else (100, 120))]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _reference(sr):
    """the restatement's dicts of _robust_inputs(sr), computed once"""
    return tuple(G.signal_features(y, sr, preprocess_first=pre) for _, y, pre in _robust_inputs(sr))


def _extract(fx, sr):
    """extract_signal_features_batch of _robust_inputs(sr): one call for the signals taken as given, one with the preprocess"""
    inputs = _robust_inputs(sr)
    res = [None] * len(inputs)
    for pre in (False, True):
        idx = [i for i, c in enumerate(inputs) if c[2] == pre]
        for i, d in zip(idx, fx.extract_signal_features_batch([inputs[i][1] for i in idx], preprocess=pre)):
            res[i] = d
    return res


def _assert_within_bounds(d, ref, what, tempo=True):
    assert list(d) == list(ref), what
    assert all(type(v) is float for v in d.values()), what
    for k in G.SPECTRAL_KEYS:
        if k in ref:                     # test_gpu_spectral.py::test_extract_spectral_features_dict
            tol = 1e-4 * max(abs(ref[k]), 1.0) if "rolloff" not in k else 2e-3 * abs(ref[k])
            print(f"{what}: {k} {abs(d[k] - ref[k]) / tol:.3f} of the bound")
            assert abs(d[k] - ref[k]) <= tol, (what, k, d[k], ref[k])
    if "harmonic_energy" in ref:         # test_gpu_hpss.py::test_stats_match_the_oracle
        for k in ("harmonic_energy", "harmonic_ratio"):
            assert abs(d[k] - ref[k]) <= 1e-4 * abs(ref[k]) + 1e-9, (what, k, d[k], ref[k])
        fm = ref["harmonic_freq_mean"]
        print(f"{what}: harmonic_freq_mean {abs(d['harmonic_freq_mean'] - fm) / (1e-3 * fm + 1e-3):.3f} "
              f"harmonic_freq_std {abs(d['harmonic_freq_std'] - ref['harmonic_freq_std']) / (2e-3 * fm + 1e-3):.3f} of the bound")
        assert abs(d["harmonic_freq_mean"] - fm) <= 1e-3 * fm + 1e-3, (what, d, ref)
        assert abs(d["harmonic_freq_std"] - ref["harmonic_freq_std"]) <= 2e-3 * fm + 1e-3, (what, d, ref)
    if "mfcc_mean" in ref:               # test_gpu_chroma.py: 1e-5 (mel, chroma) and 1e-4 (MFCC) of |mean| + std
        for mk, sk, tol in (("mel_energy_mean", "mel_energy_std", 1e-5), ("chroma_mean", "chroma_std", 1e-5), ("mfcc_mean", "mfcc_std", 1e-4)):
            bound = tol * (abs(ref[mk]) + ref[sk])
            print(f"{what}: {mk} {abs(d[mk] - ref[mk]) / bound:.3f} {sk} {abs(d[sk] - ref[sk]) / bound:.3f} of the bound")
            assert abs(d[mk] - ref[mk]) <= bound, (what, mk, d[mk], ref[mk])
            assert abs(d[sk] - ref[sk]) <= bound, (what, sk, d[sk], ref[sk])
    if tempo and "tempo" in ref:         # pinned: the inputs' tempo is robust
        assert d["tempo"] == ref["tempo"], (what, d["tempo"], ref["tempo"])


@pytest.mark.parametrize("sr", [22050, 44100])
def test_records_match_the_restatement(sr):
    """44100 Hz: 15-value band extremes (band 6) and 12 lags per lane in the tempogram"""
    from audio_feature_extraction_amd import AudioFeatureExtractor
    res = _extract(AudioFeatureExtractor(sr=sr), sr)
    for (name, _, _), d, ref in zip(_robust_inputs(sr), res, _reference(sr)):
        _assert_within_bounds(d, ref, f"{name}@{sr}")


# ---- 3. k_spec_rows<true>, frame by frame ---------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", [22050, 44100, 16000])
def test_descriptor_rows_match_the_oracle(plans, N, sr):
    from tests.test_gpu_spectral import _clips, _truth64
    R = cpu_ref
    clips = _clips(sr)
    out = plans[sr][1].groups_batch(*_pack(clips), groups=N.GROUP_SPECTRAL, store_desc=True)
    assert (out["status"] == 0).all()
    for i, c in enumerate(clips):
        m = out["desc"][i]
        g = {"centroid": m[:, 0], "bandwidth": m[:, 1], "rolloff": m[:, 2], "valley": m[:, 3:10].T, "peak": m[:, 10:17].T}
        cen, bw, ro = R.spectral_centroid(c, sr)[0], R.spectral_bandwidth(c, sr)[0], R.spectral_rolloff(c, sr)[0]
        pk, vl = R.spectral_contrast_parts(c, sr)
        assert g["centroid"].shape == cen.shape and g["peak"].shape == pk.shape
        nyq = sr / 2
        cen64, bw64, cen_cond, bw_cond = _truth64(c, sr)
        cen_tol = np.maximum(2e-5 * nyq, cen_cond)
        bw_tol = np.maximum(5e-5 * nyq, bw_cond)
        assert (np.abs(g["centroid"] - cen64) <= cen_tol).all(), (sr, i, (np.abs(g["centroid"] - cen64) / cen_tol).max())
        assert (np.abs(g["bandwidth"] - bw64) <= bw_tol).all(), (sr, i, (np.abs(g["bandwidth"] - bw64) / bw_tol).max())
        assert (np.abs(g["bandwidth"] - bw) <= 5e-5 * nyq)[bw > 1e-2 * nyq].all(), (sr, i)
        off_by = np.abs(g["rolloff"] - ro) / (sr / 2048)
        assert off_by.max() <= 1.001 and (off_by > 0.5).mean() <= 0.02, (sr, i, off_by.max())
        sc = max(float(pk.max()), 1e-30)
        assert np.abs(g["peak"] - pk).max() <= 2e-5 * sc, (sr, i)
        v_tol = 1e-3 * np.abs(vl) + 5e-6 * sc
        assert (np.abs(g["valley"] - vl) <= v_tol).all(), (sr, i, (np.abs(g["valley"] - vl) / v_tol).max())
        well = vl > 1e-3 * sc
        if well.any():
            con_g = 10.0 * np.log10(np.maximum(1e-10, g["peak"].astype(np.float64))) - 10.0 * np.log10(np.maximum(1e-10, g["valley"].astype(np.float64)))
            con_r = 10.0 * np.log10(np.maximum(1e-10, pk)) - 10.0 * np.log10(np.maximum(1e-10, vl))
            assert np.abs(con_g - con_r)[well].max() <= 1e-2, (sr, i, np.abs(con_g - con_r)[well].max())
        # the record's eight statistics are those of the rows it kept: float64, the clamp of either matrix at its own maximum
        def db(S):
            L = 10.0 * np.log10(np.maximum(1e-10, S.astype(np.float64)))
            return np.maximum(L, L.max() - 80.0)
        con = db(g["peak"]) - db(g["valley"])
        want = [f(v.astype(np.float64)) for v in (g["centroid"], g["bandwidth"], g["rolloff"], con) for f in (np.mean, np.std)]
        np.testing.assert_allclose(out["stats"][i, :8], want, rtol=1e-12, atol=1e-9)


# ---- 4. independence ----------------------------------------------------------------------------------------------------
def test_a_clip_alone_equals_the_clip_in_the_batch(plans, N):
    plan = plans[22050][1]
    sigs = _batch()
    ref = _flat(plan.groups_batch(*_pack(sigs), preprocess=True))
    for i in (0, 1, 4, 6, 9, 12):
        one = _flat(plan.groups_batch(*_pack([sigs[i]]), preprocess=True))
        for k, v in one.items():
            np.testing.assert_array_equal(v[0], ref[k][i], err_msg=f"{k} of clip {i}")


def test_failed_clips_do_not_disturb_their_neighbours(plans, N):
    plan = plans[22050][1]
    sigs = _batch()
    ref = _flat(plan.groups_batch(*_pack(sigs), preprocess=True))
    keep = [i for i in range(len(sigs)) if i not in FAILED]
    got = _flat(plan.groups_batch(*_pack([sigs[i] for i in keep]), preprocess=True))
    assert (got["status"] == 0).all()
    for k, v in got.items():
        np.testing.assert_array_equal(v, ref[k][keep], err_msg=k)
    raw = plan.groups_batch(*_pack(sigs))                           # without the preprocess 18 samples are a clip like any other
    assert {i: int(s) for i, s in enumerate(raw["status"]) if s} == {3: 1, 10: 2}
    assert np.isnan(raw["stats"][[3, 10]]).all() and (raw["stats"][keep + [7], 22:] == 0.0).all()


_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_groups import _batch, _flat, _pack
from audio_feature_extraction_amd import _native as N
plan = N.Plan(N.Context(0), N.make_params(22050, 2048, 512, 13, 128, "hann"))
np.savez(sys.argv[2], **_flat(plan.groups_batch(*_pack(_batch()), preprocess=True)))
"""


def test_chunked_batch_equals_one_chunk(plans, N, tmp_path):
    y, off, ln = _pack(_batch())
    eff = np.where(ln <= 18, 0, ln)
    cut = N.stft_chunks(eff, N.groups_cost(N.GROUP_ALL, N.GROUPS_PREPROCESS), CHUNK_BUDGET)
    assert cut.max() + 1 >= 3 and N.stft_chunks(eff, N.groups_cost(N.GROUP_ALL, N.GROUPS_PREPROCESS), 2 << 30).max() == 0
    ref = _flat(plans[22050][1].groups_batch(y, off, ln, preprocess=True))
    env = dict(os.environ, AFX_TEST_GROUPS_BUDGET=str(CHUNK_BUDGET))
    dst = str(tmp_path / "chunked.npz")
    subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _CHILD, ROOT, dst], env=env, check=True, timeout=150)
    z = np.load(dst)
    for k, v in ref.items():
        np.testing.assert_array_equal(z[k], v, err_msg=k)


# ---- 5. group subsets -----------------------------------------------------------------------------------------------------
def test_a_group_alone_equals_its_slice(plans, N):
    plan = plans[22050][1]
    y, off, ln = _pack(_batch())
    ref = _flat(plan.groups_batch(y, off, ln, preprocess=True))
    slices = {N.GROUP_SPECTRAL: slice(0, 8), N.GROUP_HARMONIC: slice(8, 12), N.GROUP_TIMBRE: slice(12, 18), N.GROUP_RHYTHM: slice(18, 22)}
    for bit, sl in slices.items():
        got = _flat(plan.groups_batch(y, off, ln, groups=bit, preprocess=True))
        np.testing.assert_array_equal(got["status"], ref["status"])
        np.testing.assert_array_equal(got["stats"][:, sl], ref["stats"][:, sl], err_msg=str(bit))
        np.testing.assert_array_equal(got["stats"][:, 22:], ref["stats"][:, 22:], err_msg=str(bit))
        rest = np.delete(got["stats"][:, :22], np.r_[sl], axis=1)
        assert np.isnan(rest).all(), bit
        np.testing.assert_array_equal(got["tuning"], ref["tuning"] if bit == N.GROUP_TIMBRE else np.zeros(len(ln)))
        np.testing.assert_array_equal(got["lag"], ref["lag"] if bit == N.GROUP_RHYTHM else np.zeros(len(ln), np.int32))
    # a one-sample clip: no centroid (afx_hpss_batch's record), everything else as from one all-but-empty frame
    one = plan.groups_batch(np.array([0.25], np.float32), [0], [1])
    assert one["status"][0] == 0 and np.isnan(one["stats"][0, :8]).all() and np.isnan(one["stats"][0, 10:12]).all()
    assert np.isfinite(one["stats"][0, 8:10]).all() and np.isfinite(one["stats"][0, 12:]).all()


def test_low_rate_runs_without_the_spectral_group(plans, N):
    plan = plans[8000][1]
    sigs = [make_clip(90, 8000, 1.0, speechy=True), rhythm_ref.clicks(8000, 120, seconds=2.0)]
    out = plan.groups_batch(*_pack(sigs), groups=N.GROUP_HARMONIC | N.GROUP_TIMBRE | N.GROUP_RHYTHM, preprocess=True)
    assert (out["status"] == 0).all() and np.isfinite(out["stats"][:, 8:]).all() and np.isnan(out["stats"][:, :8]).all()
    p = G.preprocess(sigs[1], 8000)
    ref = G.signal_features(sigs[1], 8000, groups=("harmonic", "timbre", "rhythm"))
    from audio_feature_extraction_amd import AudioFeatureExtractor
    d = AudioFeatureExtractor(sr=8000).extract_signal_features(sigs[1], groups=("harmonic", "timbre", "rhythm"))
    _assert_within_bounds(d, ref, "clicks@8000", tempo=rhythm_ref.tempo_is_robust(p, 8000))
    with pytest.raises(NotImplementedError):                        # librosa: frequency band exceeds Nyquist
        plan.groups_batch(*_pack(sigs), groups=N.GROUP_SPECTRAL)
    with pytest.raises(NotImplementedError):
        plan.groups_batch(*_pack(sigs))
    with pytest.raises(NotImplementedError):
        plan.groups_batch(*_pack(sigs), flags=N.FLAG_TRIM)
    for groups, flags in ((0, 0), (16, 0), (15, 64), (15, N.FLAG_PREEMPH | N.GROUPS_PREPROCESS)):
        with pytest.raises(ValueError):
            plans[22050][1].groups_batch(*_pack(sigs), groups=groups, flags=flags)


def test_a_short_clip_has_mfcc_statistics(plans, N):
    """2000 samples are four frames: the per-group method refuses them (its extract pass needs nine), the fused pass does not"""
    sr = 22050
    y = make_clip(91, sr, 0.2, speechy=True)[:2000]
    out = plans[sr][1].groups_batch(*_pack([y]), groups=N.GROUP_TIMBRE)
    ref = chroma_ref.timbre_features(y, sr)
    got = out["stats"][0, 12:18]
    assert out["status"][0] == 0 and np.isfinite(got).all()
    bound = 1e-4 * (abs(ref["mfcc_mean"]) + ref["mfcc_std"])
    print(f"mfcc_mean {abs(got[4] - ref['mfcc_mean']) / bound:.3f} mfcc_std {abs(got[5] - ref['mfcc_std']) / bound:.3f} of the bound")
    assert abs(got[4] - ref["mfcc_mean"]) <= bound and abs(got[5] - ref["mfcc_std"]) <= bound
    from audio_feature_extraction_amd import AudioFeatureExtractor
    with pytest.raises(ValueError):
        AudioFeatureExtractor(sr=sr).extract_timbre_features(y)     # unchanged


# ---- 6. Python ------------------------------------------------------------------------------------------------------------
def test_python_batch_gives_none_for_clips_the_reference_drops():
    from audio_feature_extraction_amd import AudioFeatureExtractor
    sr = 22050
    fx = AudioFeatureExtractor(sr=sr)
    pre = [(c, r) for c, r in zip(_robust_inputs(sr), _reference(sr)) if c[2]]
    sigs = [c[1] for c, _ in pre]
    bad = sigs[0].copy()
    bad[100] = np.inf
    batch = [sigs[0], sigs[0][:18], bad, sigs[1]]
    res = fx.extract_signal_features_batch(batch)                   # the preprocess is the default
    assert res[1] is None and res[2] is None
    assert [G.signal_features(y, sr) is None for y in batch] == [False, True, True, False]
    for (c, ref), d in zip(pre, (res[0], res[3])):
        _assert_within_bounds(d, ref, c[0])
    assert fx.extract_signal_features(sigs[1]) == res[3]
    for y in (sigs[0][:18], bad):
        with pytest.raises(ValueError):
            fx.extract_signal_features(y)
    sub = fx.extract_signal_features_batch([sigs[1]], groups=("rhythm", "spectral"))[0]
    assert sub == {k: res[3][k] for k in G.SPECTRAL_KEYS + rhythm_ref.KEYS}
    assert fx.extract_signal_features_batch([sigs[0][:18]], preprocess=False)[0] is not None     # 18 samples are a clip as given


def test_python_files(tmp_path):
    from audio_feature_extraction_amd import AudioFeatureExtractor, wavio
    fx = AudioFeatureExtractor(sr=22050)
    paths = [str(tmp_path / "a.wav"), str(tmp_path / "b16k.wav")]
    wavfiles.write_wav(paths[0], wavfiles.quantize(make_clip(95, 22050, 0.8, speechy=True), "s16"), 22050, "s16")
    wavfiles.write_wav(paths[1], wavfiles.quantize(make_clip(96, 16000, 0.7, speechy=True), "f32"), 16000, "f32")
    res = fx.extract_signal_features_files(paths)
    loaded = wavio.load_batch(paths, sr=22050)
    assert [r for _, r in loaded] == [22050, 22050]
    want = fx.extract_signal_features_batch([y for y, _ in loaded])
    for p, d, w in zip(paths, res, want):
        assert d.pop("filename") == os.path.basename(p)
        assert d == w and list(d) == [k for g in G.GROUPS for k in G.KEYS[g]]
