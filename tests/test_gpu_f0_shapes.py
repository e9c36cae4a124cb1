"""extract_f0 on every kernel route a non-default framing takes (tests/f0_shapes.py names the rows and their routes): the
generic instantiations of k_f0_yin, k_f0_energy at 64 / 32 / 16 frames per block, the generic Viterbi at bands 5 .. 30 and
k_f0_backtrack<5>, each against the pYIN oracle with the criteria of tests/test_gpu_f0.py."""
import numpy as np
import pytest

from audio_feature_extraction_amd import _native as N
from audio_feature_extraction_amd.synth import make_clip
from oracle import cpu_ref as R
from oracle import pyin_ref as P
from tests import f0_shapes as S

pytestmark = pytest.mark.gpu

C2, C7 = S.C2, S.C7
NON_IDENTICAL = {}      # tag -> (frames that differ from the oracle's track, frames): printed by the last test of the module
REFUSAL = r"transition band of 101 bins \(2 \* band \+ 1, band 50\) is wider than the 64 lanes of k_f0_backtrack"


def open_plan(sr, n_fft, hop):
    ctx = N.Context(0)
    try:
        return ctx, N.Plan(ctx, N.make_params(sr, n_fft, hop, 13, 128 if n_fft >= 512 else 40))
    except Exception:
        ctx.close()
        raise


def pack(clips):
    lengths = np.array([c.size for c in clips], np.int64)
    pad = (lengths + 3) // 4 * 4
    offsets = np.concatenate([[0], np.cumsum(pad)[:-1]]).astype(np.int64)
    buf = np.zeros(int(pad.sum()), np.float32)
    for c, o in zip(clips, offsets):
        buf[o:o + c.size] = c
    return buf, offsets, lengths


def run(plan, clips, fmin, fmax, flags=0):
    buf, offsets, lengths = pack(clips)
    out = plan.f0_batch(buf, offsets, lengths, fmin, fmax, flags=flags, want_frames=True)
    hop = plan.params.hop
    return out, [out["f0_flat"][o:o + 1 + n // hop] for o, n in zip(out["f0_offsets"], lengths)]


def differing(f0_gpu, f0_ref):
    """Frames that are not the oracle's: another NaN pattern, or a voiced pitch more than 1e-9 relative away."""
    assert f0_gpu.shape == f0_ref.shape, (f0_gpu.shape, f0_ref.shape)
    same = np.isnan(f0_gpu) == np.isnan(f0_ref)
    v = ~np.isnan(f0_ref) & ~np.isnan(f0_gpu)
    same[v] &= np.abs(f0_gpu[v] - f0_ref[v]) <= 1e-9 * f0_ref[v]
    return np.flatnonzero(~same)


def check_clip(f0_gpu, stats_gpu, ref, tag, strict=True):
    """ref: pyin_ref.extract_f0(..., return_frames=True).  strict: the track is the oracle's frame for frame and the
    statistics agree to rounding; otherwise the mixture bounds of tests/test_gpu_f0.py (at most 3 frames)."""
    bad = differing(f0_gpu, ref["f0"])
    NON_IDENTICAL[tag] = (int(bad.size), int(f0_gpu.size))
    print(f"[f0 shapes] {tag}: {bad.size} of {f0_gpu.size} frames differ from the oracle's track")
    want = [ref["f0_mean"], ref["f0_std"], ref["f0_missing_rate"], ref["f0_quality"]]
    if strict:
        assert bad.size == 0, (tag, bad.size, f0_gpu.size, bad[:10])
        np.testing.assert_allclose(stats_gpu, want, rtol=1e-10, atol=1e-12, err_msg=tag)
    else:
        assert bad.size <= 3, (tag, bad.size, f0_gpu.size, bad[:10])
        assert abs(stats_gpu[0] - ref["f0_mean"]) <= 5e-3 * max(ref["f0_mean"], 1.0), tag
        assert abs(stats_gpu[2] - ref["f0_missing_rate"]) <= 0.02, tag


@pytest.mark.parametrize("row", S.SWEEP, ids=lambda r: "%d-%d-%d" % r[:3])
def test_f0_on_the_route_of(row):
    sr, n_fft, hop, fmin, fmax = row
    d = N.f0_dispatch(*row)
    assert S.route_of(d) == S.ROUTES[row]
    named = list(S.clip_set(row, d["epb"]))
    named.append(("repeat", named[0][1]))                         # the first tone again, behind the one-frame clips
    ctx, plan = open_plan(sr, n_fft, hop)
    try:
        out, f0 = run(plan, [c for _, c in named], fmin, fmax)
    finally:
        plan.close()
        ctx.close()
    assert out["status"].tolist() == [0] * len(named)
    loose = 0
    for i, (tag, y) in enumerate(named):
        strict = S.is_strict(row, tag)
        loose += not strict
        ref = S.oracle(row, named[0][0] if tag == "repeat" else tag, y)
        check_clip(f0[i], out["stats"][i], ref, "%d/%d/%d %s" % (sr, n_fft, hop, tag), strict)
    assert loose <= 2
    tags = [t for t, _ in named]
    assert out["stats"][tags.index("zeros")].tolist() == [0.0, 0.0, 1.0, 0.0]
    # position in the batch and the neighbouring clips do not matter
    np.testing.assert_array_equal(f0[-1], f0[0])
    np.testing.assert_array_equal(out["stats"][-1], out["stats"][0])
    # the tones are found where the framing can see them (a period must fit half a frame)
    for f in S.TONES:
        if f >= 1.1 * sr / (n_fft - n_fft // 2 - 1):
            k = tags.index(f"tone{int(f)}")
            assert abs(out["stats"][k][0] - f) <= 0.02 * f and out["stats"][k][2] < 0.5, (f, out["stats"][k])


@pytest.mark.parametrize("sr,n_fft,hop", [r[:3] for r in S.FUSED_ROWS])
def test_f0_fused_with_preemphasis_and_trim_on_a_generic_shape(sr, n_fft, hop):
    clips = S.fused_clips(sr)
    ctx, plan = open_plan(sr, n_fft, hop)
    try:
        out, f0 = run(plan, clips, C2, C7, flags=N.FLAG_PREEMPH | N.FLAG_TRIM)
    finally:
        plan.close()
        ctx.close()
    assert out["status"].tolist() == [0, 0]
    for i, c in enumerate(clips):
        yp, _ = R.preprocess_audio(c)
        ref = P.extract_f0(yp, sr=sr, frame_length=n_fft, hop_length=hop, return_frames=True)
        check_clip(f0[i][:1 + yp.size // hop], out["stats"][i], ref, "%d/%d/%d fused%d" % (sr, n_fft, hop, i))


def test_plan_rebuilds_tables_across_band_30_ranges():
    row = (22050, 1024, 300, C2, C7)
    clips = [c for t, c in S.clip_set(row, N.f0_dispatch(*row)["epb"]) if t in ("tone196", "tone330", "edge9")]
    lo, hi = S.REUSE_RANGE
    ctx, plan = open_plan(*row[:3])
    try:
        a, fa = run(plan, clips, C2, C7)
        b, fb = run(plan, clips, lo, hi)
        c, fc = run(plan, clips, C2, C7)
    finally:
        plan.close()
        ctx.close()
    assert N.f0_dispatch(22050, 1024, 300, lo, hi)["band"] == 30
    for o in (a, b, c):
        assert (o["status"] == 0).all()
    np.testing.assert_array_equal(a["stats"], c["stats"])
    np.testing.assert_array_equal(a["f0_flat"], c["f0_flat"])
    # the narrower range in between decoded with its own tables
    ref = P.extract_f0(clips[0], sr=22050, frame_length=1024, hop_length=300, fmin=lo, fmax=hi, return_frames=True)
    check_clip(fb[0], b["stats"][0], ref, "22050/1024/300 100..400 Hz tone196")


def test_band_refusal_on_a_live_plan_leaves_it_usable():
    clips = [make_clip(60 + i, 22050, 0.5, speechy=bool(i % 2)) for i in range(3)]
    buf, offsets, lengths = pack(clips)
    ctx, plan = open_plan(22050, 2048, 512)
    try:
        before = plan.extract_batch(buf, offsets, lengths)
        with pytest.raises(NotImplementedError, match=REFUSAL):
            plan.f0_batch(buf, offsets, lengths, C2, C7, flags=0)
        after = plan.extract_batch(buf, offsets, lengths)
    finally:
        plan.close()
        ctx.close()
    assert (before["status"] == 0).all()
    np.testing.assert_array_equal(before["stats"], after["stats"])
    np.testing.assert_array_equal(before["trim"], after["trim"])


def test_lds_refusal_keeps_the_tables_of_the_last_accepted_range():
    sr = 44100
    clips = [S.padded_tone(sr, 196.0), S.padded_tone(sr, 330.0)]
    ctx, plan = open_plan(sr, 2048, 512)
    try:
        a, _ = run(plan, clips, C2, C7)
        with pytest.raises(NotImplementedError, match=r"160 KiB of LDS \(k_f0_yin"):
            run(plan, clips, 45.0, C7)
        b, _ = run(plan, clips, C2, C7)              # f0_setup returns early: the old tables are still installed
    finally:
        plan.close()
        ctx.close()
    assert (a["status"] == 0).all() and (b["status"] == 0).all()
    np.testing.assert_array_equal(a["stats"], b["stats"])
    np.testing.assert_array_equal(a["f0_flat"], b["f0_flat"])
    assert not np.isnan(a["f0_flat"]).all()


def test_zz_report_non_identical_frames():
    """Not a check of its own: prints, per clip tested above, how many frames differed from the oracle's decoded track
    (run with -s), so that a drift from 0 is visible; the per-route totals are the table of DESIGN.md 7."""
    routes = {}
    for tag, (bad, frames) in NON_IDENTICAL.items():
        r = routes.setdefault(tag.split(" ")[0], [0, 0, 0])
        r[0] += 1; r[1] += frames; r[2] += bad
    for k, (n, frames, bad) in routes.items():
        print(f"[f0 shapes] {k}: {n} clips, {frames} frames compared, {bad} differ")
    assert sum(v[0] for v in NON_IDENTICAL.values()) == 0, {k: v for k, v in NON_IDENTICAL.items() if v[0]}
