"""The chunk cut afx_hpss_batch, afx_chroma_batch and afx_rhythm_batch share (cut_stft_chunk), through the host-only query
afx_stft_chunks, against a restatement of the loop the three entry points each carried before.  CPU only; no sample
memory is allocated."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# cost records (bytes per frame, per tile, per sample, per clip; frames per tile; tile cap) of a default plan -- 22050 Hz,
# 128 mel bands, so 358 piptrack bins and a 344-lag tempogram window -- fed float32 samples from host memory
HALF_INT32 = (2 ** 31 - 1) // 2
COSTS = {
    "hpss": (1032 * 8 * 2 + 17 * 4, 0, 4 * 2 + 4, 128, 64, 65535),                             # harmonic only
    "hpss_perc_spec": (1032 * 8 * 3 + 17 * 4 + 3 * 1025 * 4, 0, 4 * 3 + 4, 128, 64, 65535),    # want_perc, AFX_HPSS_STORE_SPEC
    "chroma": (1040 * 4 + 358 * 5 + 48 + 128 * 4 + 32, 0, 4 + 4, 102 * 4 + 128, 16, HALF_INT32),   # tuning estimated, mel wanted
    "chroma_given": (1040 * 4 + 48 + 32, 0, 4 + 4, 102 * 4 + 128, 16, HALF_INT32),             # tuning given, no mel
    "rhythm": (1040 * 4 + 128 * 4 + 4, 344 * 8, 4 + 4, 344 * 8 + 128, 16, HALF_INT32),
    "rhythm_tempogram": (1040 * 4 + 128 * 4 + 4 + 344 * 4, 344 * 8, 4 + 4, 344 * 8 + 128, 16, HALF_INT32),
}
TEST_BUDGET = {"hpss": 2000000, "chroma": 400000, "rhythm": 400000}      # what the GPU tests set AFX_TEST_*_BUDGET to
BIG = 2 ** 62


def clip_bytes(L, cost):
    per_frame, per_tile, per_sample, per_clip, tile, _ = cost
    T = 1 + L // 512
    nt = (T + tile - 1) // tile
    return T * per_frame + nt * per_tile + L * per_sample + per_clip, nt


def chunks_restated(lengths, cost, budget):
    """the loop of the three entry points, as each of them had it"""
    n, out, c0, chunk = len(lengths), [-1] * len(lengths), 0, 0
    while c0 < n:
        held, nbytes, tiles, c1 = [], 0, 0, c0
        while c1 < n and len(held) < 32768:
            L = int(lengths[c1])
            if L != 0:
                pb, nt = clip_bytes(L, cost)
                if held and (nbytes + pb > budget or tiles + nt > cost[5]):
                    break
                held.append(c1)
                nbytes += pb
                tiles += nt
            c1 += 1
        for i in held:
            out[i] = chunk
        chunk += bool(held)
        c0 = c1
    return out


def chunks(lengths, cost, budget):
    from audio_feature_extraction_amd import _native as N
    return N.stft_chunks(lengths, cost, budget).tolist()


@pytest.mark.parametrize("name", sorted(COSTS))
def test_random_batches_cut_as_the_restatement_cuts_them(name):
    rng = np.random.default_rng(20260 + sorted(COSTS).index(name))
    cost = COSTS[name]
    for trial in range(6):
        n = int(rng.integers(1, 60))
        lengths = rng.integers(1, 30000, n)
        lengths[rng.random(n) < 0.2] = 0
        lengths[rng.random(n) < 0.15] = rng.choice([1, 511, 512, 513, 8191, 8192])
        for budget in (1, TEST_BUDGET[name.split("_")[0]], BIG):
            got = chunks(lengths, cost, budget)
            assert got == chunks_restated(lengths, cost, budget), (name, trial, budget)
            live = [c for c in got if c >= 0]
            assert [c for c, L in zip(got, lengths) if L == 0] == [-1] * int((lengths == 0).sum())
            if budget == 1:
                assert live == list(range(len(live)))              # every clip its own chunk
            if budget == BIG:
                assert set(live) <= {0}


@pytest.mark.parametrize("name", sorted(COSTS))
def test_a_clip_that_lands_on_the_budget_stays(name):
    cost = COSTS[name]
    lengths = [5000, 0, 12345, 700]
    total = sum(clip_bytes(L, cost)[0] for L in lengths if L)
    assert chunks(lengths, cost, total) == [0, -1, 0, 0]
    assert chunks(lengths, cost, total - 1) == [0, -1, 0, 1]
    assert chunks_restated(lengths, cost, total - 1) == [0, -1, 0, 1]


def test_a_chunk_ends_at_32768_clips_however_many_empty_ones_lie_between():
    lengths = np.ones(40000 + 40000 // 3, np.int64)
    lengths[3::4] = 0                                               # 40000 clips of one sample, an empty one after every third
    assert int((lengths == 1).sum()) == 40000
    got = np.array(chunks(lengths, COSTS["rhythm"], BIG))
    live = got[lengths == 1]
    assert (got[lengths == 0] == -1).all()
    assert (live[:32768] == 0).all() and (live[32768:] == 1).all()
    assert got.tolist() == chunks_restated(lengths, COSTS["rhythm"], BIG)


def test_hpss_tile_cap_cuts_after_127_clips_of_2_to_24_samples():
    """T = 1 + 2^24 / 512 = 32769 frames are 513 tiles of 64, and 127 * 513 = 65151 <= 65535 < 128 * 513"""
    lengths = [2 ** 24] * 128
    assert clip_bytes(2 ** 24, COSTS["hpss"])[1] == 513
    got = chunks(lengths, COSTS["hpss"], BIG)
    assert got == [0] * 127 + [1]
    assert got == chunks_restated(lengths, COSTS["hpss"], BIG)
    assert chunks(lengths, COSTS["chroma"], BIG) == [0] * 128       # the other groups' cap is far away


def test_all_empty_and_empty_batches():
    assert chunks([0] * 9, COSTS["chroma"], 400000) == [-1] * 9
    assert chunks([], COSTS["chroma"], 400000) == []


def test_a_clip_larger_than_the_budget_runs_alone():
    cost = COSTS["hpss"]
    assert clip_bytes(100000, cost)[0] > 2000000 > 2 * clip_bytes(700, cost)[0]
    assert chunks([100000], cost, 2000000) == [0]
    assert chunks([700, 700, 100000, 0, 700, 700], cost, 2000000) == [0, 0, 1, -1, 2, 2]


def test_arguments_out_of_range_are_refused():
    from audio_feature_extraction_amd import _native as N
    cost = list(COSTS["hpss"])
    for lengths, c, budget in (([-1], cost, 1), ([2 ** 31 + 1], cost, 1), ([1], cost, 0), ([1], cost, 2 ** 62 + 1),
                               ([1], cost[:4] + [0, 1], 1), ([1], cost[:5] + [0], 1), ([1], [-1] + cost[1:], 1),
                               ([1], [2 ** 20 + 1] + cost[1:], 1)):
        with pytest.raises(ValueError):
            N.stft_chunks(lengths, c, budget)
    with pytest.raises(ValueError):
        N.stft_chunks([1], cost[:5], 1)


def test_symbol_is_declared_and_bound():
    from audio_feature_extraction_amd import _native as N
    header = open(os.path.join(ROOT, "include", "afx.h")).read()
    assert "afx_stft_chunks" in N.SYMBOLS
    assert re.search(r"\bint\s+afx_stft_chunks\s*\(", header)
    assert hasattr(N.lib(), "afx_stft_chunks")
    assert re.search(r"#define\s+AFX_VERSION\s+107\b", header)                  # found by its presence
    stubs = open(os.path.join(ROOT, "audio_feature_extraction_amd", "csrc", "afx_host_stubs.cpp")).read()
    assert "afx_stft_chunks" not in stubs                                       # the query is real in the host build
