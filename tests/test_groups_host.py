"""The host side of afx_groups_batch, the fused pass over the spectral, harmonic, timbre and rhythm groups: its symbols,
the cost record it cuts a batch with (afx_groups_cost, through afx_stft_chunks), its MFCC table, and the argument
refusals and key order of ``extract_signal_features_batch``.  CPU only."""
import itertools
import os
import re

import numpy as np
import pytest

from tests import groups_ref as G
from tests.test_stft_chunks_host import chunks_restated, clip_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("afx_groups_batch", "afx_groups_cost", "afx_groups_dct_table", "afx_groups_debug_rows")


def test_symbols_are_declared_and_bound():
    from audio_feature_extraction_amd import _native as N
    header = open(os.path.join(ROOT, "include", "afx.h")).read()
    for name in NAMES:
        assert name in N.SYMBOLS
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert hasattr(N.lib(), name)
    assert re.search(r"#define\s+AFX_VERSION\s+107\b", header)                  # found by their presence
    stubs = open(os.path.join(ROOT, "audio_feature_extraction_amd", "csrc", "afx_host_stubs.cpp")).read()
    assert "afx_groups_batch" in stubs and "afx_groups_debug_rows" in stubs
    assert "afx_groups_cost" not in stubs and "afx_groups_dct_table" not in stubs     # real in the host build
    for k, name in enumerate(("SPECTRAL", "HARMONIC", "TIMBRE", "RHYTHM")):
        assert getattr(N, "GROUP_" + name) == 1 << k
        assert re.search(r"AFX_GROUP_" + name + r"\s*=\s*" + str(1 << k) + r"\b", header)
    assert N.GROUPS_PREPROCESS == 16 and re.search(r"AFX_GROUPS_PREPROCESS\s*=\s*16\b", header)


def test_cost_is_monotone_in_the_groups():
    from audio_feature_extraction_amd import _native as N
    for flags in (0, N.GROUPS_PREPROCESS):
        cost = {g: N.groups_cost(g, flags) for g in range(1, 16)}
        for a, b in itertools.product(range(1, 16), repeat=2):
            if a & b == a:                                            # a's groups are among b's
                assert (cost[a][:4] <= cost[b][:4]).all(), (a, b, cost[a], cost[b])
                assert cost[a][4] == cost[b][4] == 16 and cost[a][5] >= cost[b][5]
        for g in range(1, 16):
            assert (cost[g][:4] <= N.groups_cost(g, N.GROUPS_PREPROCESS)[:4]).all()
    # the power rows of h lie where X lay: the harmonic group adds two complex rows and the centroid row, no power rows
    assert N.groups_cost(N.GROUP_HARMONIC)[0] == 2 * 1032 * 8 + 17 * 4
    assert N.groups_cost(N.GROUP_SPECTRAL)[0] == 1040 * 4 + 17 * 4
    assert N.groups_cost(N.GROUP_HARMONIC | N.GROUP_SPECTRAL)[0] == 2 * 1032 * 8 + 1040 * 4 + 2 * 17 * 4
    assert N.groups_cost(N.GROUP_HARMONIC)[5] == 65535                # k_hpss_mask's grid
    for bad in (0, 16, -1, 31):
        with pytest.raises(ValueError):
            N.groups_cost(bad)


@pytest.mark.parametrize("groups,preprocess", [(15, True), (15, False), (2, False), (13, True), (8, False)])
def test_the_cut_is_the_restatement_of_the_shared_rule(groups, preprocess):
    """afx_groups_batch cuts with cut_stft_chunk like the three entry points; with the preprocess a clip of 18 samples or
    fewer is in no chunk, like an empty one"""
    from audio_feature_extraction_amd import _native as N
    cost = N.groups_cost(groups, N.GROUPS_PREPROCESS if preprocess else 0)
    rng = np.random.default_rng(77 + groups)
    for trial in range(5):
        n = int(rng.integers(1, 50))
        lengths = rng.integers(1, 30000, n)
        lengths[rng.random(n) < 0.15] = 0
        lengths[rng.random(n) < 0.2] = rng.choice([1, 18, 19, 511, 512, 513, 8191, 8192, 8193])
        eff = np.where(lengths <= 18, 0, lengths) if preprocess else lengths
        one = clip_bytes(8192, tuple(cost))[0]
        for budget in (1, 3 * one, 2 ** 31):
            got = N.stft_chunks(eff, cost, budget).tolist()
            assert got == chunks_restated(eff, tuple(int(c) for c in cost), budget), (groups, trial, budget)
            if budget == 2 ** 31:
                assert set(got) <= {-1, 0}


def test_dct_table_is_scipys():
    import scipy.fft
    from audio_feature_extraction_amd import _native as N
    ref = scipy.fft.dct(np.eye(128), type=2, norm="ortho", axis=0)[:13].astype(np.float32)
    np.testing.assert_array_equal(N.groups_dct_table(128), ref)
    t40 = N.groups_dct_table(40)
    # fewer bands: entries that are zero in exact arithmetic come out of either route as a different 1e-16, so the bound
    # is one float32 rounding of a value below sqrt(2 / 40) < 0.25
    ref40 = scipy.fft.dct(np.eye(40), type=2, norm="ortho", axis=0)[:13]
    assert np.abs(t40[:, :40].astype(np.float64) - ref40).max() <= 2.0 ** -24 * 0.25
    assert not t40[:, 40:].any()
    for bad in (0, 129):
        with pytest.raises(ValueError):
            N.groups_dct_table(bad)


def test_python_refuses_bad_arguments_before_any_device_call():
    from audio_feature_extraction_amd import AudioFeatureExtractor
    fx = AudioFeatureExtractor(sr=22050)
    y = np.zeros(4000, np.float32)
    with pytest.raises(ValueError, match="unknown feature group"):
        fx.extract_signal_features_batch([y], groups=("spectral", "pitch"))
    with pytest.raises(ValueError, match="no feature group"):
        fx.extract_signal_features_batch([y], groups=())
    with pytest.raises(ValueError, match="1-D"):
        fx.extract_signal_features_batch([y, np.zeros((2, 100), np.float32)])
    with pytest.raises(ValueError, match="1-D"):
        fx.extract_signal_features(np.zeros((2, 100), np.float32))
    assert fx.extract_signal_features_batch([]) == []


def test_key_order_is_the_restatements():
    import audio_feature_extraction_amd as pkg
    from audio_feature_extraction_amd import AudioFeatureExtractor as A
    from audio_feature_extraction_amd import _native as N
    assert A._SIGNAL_GROUPS == G.GROUPS
    assert (A._SPECTRAL_KEYS, A._HARMONIC_KEYS, A._TIMBRE_KEYS, A._RHYTHM_KEYS) == tuple(G.KEYS[g] for g in G.GROUPS)
    rec = np.arange(24, dtype=np.float64)
    fx = A(sr=22050)
    ref = G.signal_features(0.1 * np.random.default_rng(0).standard_normal(3000).astype(np.float32), 22050, preprocess_first=False)
    assert list(fx._signal_dict(N.GROUP_ALL, rec)) == list(ref)
    for groups in (("rhythm", "spectral"), ("timbre",), ("harmonic", "timbre", "rhythm")):
        want = [k for g in G.GROUPS if g in groups for k in G.KEYS[g]]
        assert list(fx._signal_dict(A._group_bits(groups), rec)) == want
    d = fx._signal_dict(N.GROUP_ALL, rec)
    assert d["harmonic_ratio"] == 8.0 / (9.0 + 1e-8) and d["rhythm_regularity"] == 20.0 / (19.0 + 1e-8)
    assert d["tempo"] == 18.0 and d["mfcc_std"] == 17.0 and d["spectral_contrast_std"] == 7.0
    assert all(type(v) is float for v in d.values())
    assert "extract_signal_features_batch" not in pkg.__all__


@pytest.mark.parametrize("sr", [22050, 44100])
def test_chosen_inputs_are_robust(sr):
    """the CPU half of tests/test_gpu_groups.py::test_records_match_the_restatement: every input chosen there passes the
    three predicates on the signal the groups see, so its tuning and tempo may be pinned and its contrast statistics held
    to the bound of the per-group test"""
    from tests import chroma_ref, rhythm_ref
    from tests.test_gpu_groups import _robust_inputs
    assert sum(pre for _, _, pre in _robust_inputs(sr)) >= 2 and sum(not pre for _, _, pre in _robust_inputs(sr)) >= 3
    for name, y, pre in _robust_inputs(sr):
        p = G.preprocess(y, sr) if pre else y
        assert chroma_ref.tuning_is_robust(p, sr) and rhythm_ref.tempo_is_robust(p, sr), (sr, name)
        assert G.contrast_is_well_conditioned(p, sr), (sr, name)


def test_the_preprocess_leaves_the_contrast_of_most_signals_ill_conditioned():
    """why only the chords go through the preprocess in the restatement test: librosa's own dtypes miss the bound there"""
    from tests.test_gpu_groups import _robust_inputs
    name, y, _ = _robust_inputs(22050)[1]
    assert G.contrast_is_well_conditioned(y, 22050) and not G.contrast_is_well_conditioned(G.preprocess(y, 22050), 22050), name
