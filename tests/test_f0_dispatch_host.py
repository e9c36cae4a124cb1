"""Which pYIN kernels a configuration runs (afx_f0_dispatch, host-only): the routes pinned, the refusals pinned, every route
an accepted framing can take covered by a shape the GPU tests run, and the strict clips of tests/test_gpu_f0_shapes.py
checked against the oracle alone.  No GPU is used."""
import numpy as np
import pytest

from audio_feature_extraction_amd import _native as N
from oracle import cpu_ref as R
from tests import f0_shapes as S

C2, C7 = S.C2, S.C7


def mr_supported(n):
    if n < 256 or n > 2048 or n % 16:
        return False
    for p in (2, 3, 5):
        while n % p == 0:
            n //= p
    return n == 1


@pytest.mark.parametrize("row", list(S.ROUTES) + list(S.COMPILED), ids=lambda r: "%d-%d-%d-%d" % (r[0], r[1], r[2], round(r[3])))
def test_dispatch_of_pinned_shapes(row):
    """The sweep's rows take the routes they exist to cover, and the three compiled shapes stay on their instantiations."""
    want = {**S.ROUTES, **S.COMPILED}[row]
    assert S.route_of(N.f0_dispatch(*row)) == want


def test_dispatch_names_the_tight_lds_cases():
    assert N.f0_dispatch(44100, 2048, 600, C2, C7)["yin_lds"] == 157952
    # 162 752 bytes: 1088 under the limit of 160 KiB = 163 840, so accepted -- on the route of 2048 / 600
    d = N.f0_dispatch(44100, 2048, 640, C2, C7)
    assert d["yin_lds"] == 162752 and S.route_of(d) == S.ROUTES[(44100, 2048, 600, C2, C7)]
    # the reference's shape runs the compact layout (a fourth workgroup per CU)
    assert N.f0_dispatch(22050, 1024, 256, C2, C7)["yin_lds"] == 39672


@pytest.mark.parametrize("sr,n_fft,hop,bins,band", [(22050, 2048, 512, 101, 50), (16000, 1024, 256, 71, 35)])
def test_band_wider_than_backtrack_is_refused_by_name(sr, n_fft, hop, bins, band):
    with pytest.raises(NotImplementedError, match=rf"transition band of {bins} bins \(2 \* band \+ 1, band {band}\) is wider than "
                                                  r"the 64 lanes of k_f0_backtrack: hop_length / sr is too large") as e:
        N.f0_dispatch(sr, n_fft, hop, C2, C7)
    assert "LDS" not in str(e.value)


def test_lds_refusal_names_the_kernel():
    with pytest.raises(NotImplementedError, match=r"more than 160 KiB of LDS \(k_f0_yin: 175552 bytes\)"):
        N.f0_dispatch(44100, 2048, 512, 45.0, 2093.0)
    with pytest.raises(NotImplementedError, match="160 KiB of LDS"):
        N.f0_dispatch(44100, 2048, 512, 45.0, C7)


def test_invalid_arguments():
    for bad in [(0, 1024, 256), (22050, 1024, 0), (22050, 0, 256), (22050, 8192, 256)]:
        with pytest.raises(ValueError):
            N.f0_dispatch(*bad, C2, C7)
    with pytest.raises(NotImplementedError, match="f0_min"):
        N.f0_dispatch(22050, 1024, 256, 300.0, 200.0)


def test_dispatch_agrees_with_the_tables():
    for row in S.SWEEP:
        t, d = N.f0_build_tables(*row), N.f0_dispatch(*row)
        assert (t["band"], t["n_bins"]) == (d["band"], d["n_bins"])
        assert d["yin_n"] >= max(t["R"], t["slots"]) and d["vit_tpt"] == -(-t["n_bins"] // 640)
        assert d["bt_depth"] == (6 if 10 * t["band"] + 2 <= 256 else 5)


def test_every_reachable_route_is_run_by_a_gpu_test():
    """Every value of every dispatch field, and every k_f0_yin instantiation, that some accepted framing selects is
    selected by a shape the GPU suite runs: a dispatch change that opens a new route fails here until a shape covers it."""
    fields = ("energy_lpw", "epb", "yin_n", "yin_fpb", "yin_sh", "vit_nbt", "vit_bandt", "vit_tpt", "bt_depth", "band")

    def groups(d):
        g = {(k, d[k]) for k in fields}
        g.add(("yin", d["yin_n"], d["yin_fpb"], d["yin_sh"]))
        g.add(("viterbi", d["vit_nbt"], d["vit_bandt"], d["band"] if d["vit_nbt"] == 0 else 0))
        g.add(("energy", d["energy_lpw"], d["epb"]))
        return g

    covered = set()
    for row in list(S.SWEEP) + S.ALREADY_RUN:
        covered |= groups(N.f0_dispatch(*row))
    found, example, accepted = set(), {}, 0
    frames = [n for n in range(256, 2049, 16) if mr_supported(n)]
    assert len(frames) == 27
    for sr in (8000, 11025, 16000, 22050, 32000, 44100, 48000):
        for n_fft in frames:
            for hop in range(8, n_fft + 1, 8):
                for fmin, fmax in [(C2, C7)] + S.OTHER_RANGES:
                    try:
                        d = N.f0_dispatch(sr, n_fft, hop, fmin, fmax)
                    except NotImplementedError:
                        continue
                    accepted += 1
                    for g in groups(d) - found:
                        found.add(g)
                        example[g] = (sr, n_fft, hop, fmin, fmax)
    assert accepted > 10000
    missing = {g: example[g] for g in found - covered}
    assert not missing, missing
    assert ("yin", 4, 8, 0) in found and ("bt_depth", 5) in found


@pytest.mark.parametrize("row", S.SWEEP, ids=lambda r: "%d-%d-%d" % r[:3])
def test_strict_clips_do_not_hang_on_the_unvoiced_bit(row):
    """The clips the GPU test holds to '0 differing frames' decode to the same path whichever value the unvoiced
    observation of their strongly voiced frames takes (the one bit of the oracle that is BLAS's)."""
    epb = N.f0_dispatch(*row)["epb"]
    clips = S.clip_set(row, epb)
    tags = [t for t, _ in clips]
    loose = [t for t in tags if not S.is_strict(row, t)]
    assert len(loose) <= 2 and all(t in ("low-end", "high-end", "noise") for t in loose), loose
    assert {t for r, t in S.NON_ROBUST if r == row} <= set(tags)
    for tag, y in clips:
        if not S.is_strict(row, tag):
            continue
        ok, fragile, T = S.robust_to_unvoiced_bit(row, y)
        print(f"[f0 robust] {row[:3]} {tag}: {fragile} of {T} frames fragile, path {'kept' if ok else 'CHANGED'}")
        assert ok, (row, tag, fragile, T)
    zeros = dict(clips)["zeros"]
    o = S.oracle(row, "zeros", zeros)
    assert [o["f0_mean"], o["f0_std"], o["f0_missing_rate"], o["f0_quality"]] == [0, 0, 1, 0]
    assert np.isnan(o["f0"]).all()


def test_fused_and_reuse_clips_do_not_hang_on_the_unvoiced_bit():
    """The other clips tests/test_gpu_f0_shapes.py holds to the oracle's track: the preprocessed signals of the fused runs,
    and the tone the 22050 / 1024 / 300 plan decodes at 100 .. 400 Hz between two C2 .. C7 calls."""
    for row in S.FUSED_ROWS:
        for i, c in enumerate(S.fused_clips(row[0])):
            ok, fragile, T = S.robust_to_unvoiced_bit(row, R.preprocess_audio(c)[0])
            assert ok, (row, i, fragile, T)
    row = (22050, 1024, 300) + S.REUSE_RANGE
    assert N.f0_dispatch(*row)["band"] == 30 and N.f0_dispatch(*row)["bt_depth"] == 5
    ok, fragile, T = S.robust_to_unvoiced_bit(row, S.padded_tone(22050, 196.0))
    assert ok and fragile > 0, (fragile, T)
