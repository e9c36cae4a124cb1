"""GPU checks of afx_clip_fft_batch / afx_specdist_batch and the PESQ-like score of audio_feature_extraction_amd.quality
against the long-double truth and the yardsticks of tests/spectrum_ref.py, on the smallest shapes where the kernels can go
wrong: trivial N, a prime, M exactly at the tile (N = 2048) and the first four-step M (N = 2049), powers of two and their
successors, a prime with M = 2^18, and one clip of the workload's own length (220500: M = 2^19, M1 != M2), int16 and
float32 from host and device memory.

Tolerances (spectrum_ref): a clip's bins within bound(N) = 8 max(e_ref(N), 2^-52) of the truth, relative L2; spec_dist
within bound(N) kappa; Parseval to 1e-12; pesq within 0.7 x the spec_dist tolerance (d pesq / d spec_dist = 3.5 x 0.2)
plus 1e-11, the bound the STOI test puts on the compare-record terms.  Every test prints its figures before it asserts."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import spectrum_ref as S
from tests.test_spectrum_host import check_bins, check_record

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK_BUDGET = 3000000


@pytest.fixture(scope="module")
def N():
    from audio_feature_extraction_amd import _native
    if _native.device_count() < 1:
        pytest.fail("no GPU visible")
    return _native


@pytest.fixture(scope="module")
def ctx(N):
    return N.Context(0)


@functools.lru_cache(maxsize=None)
def _s16_clips():
    """the reference clips as int16, their float32 conversion (value / 32768) and its true spectrum"""
    out = []
    for p in S.pairs():
        q = S.as_s16(p["r"])
        f = q.astype(np.float32) / np.float32(32768.0)
        out.append({"n": p["n"], "q": q, "r": f, "R": S.truth_fft(f), "bound": p["bound"]})
    return tuple(out)


def _fft(N, ctx, clips, device=False, gap=0):
    """rfft of every clip (one dtype), laid out with ``gap`` poisoned elements between neighbours, from host or device memory"""
    dtype = clips[0].dtype
    offs, pos = np.zeros(len(clips), np.int64), 0
    for i, c in enumerate(clips):
        offs[i] = pos
        pos += c.size + gap
    buf = np.full(max(pos, 1), -32768 if dtype == np.int16 else np.nan, dtype)
    for o, c in zip(offs, clips):
        buf[o:o + c.size] = c
    lens = np.array([c.size for c in clips], np.int64)
    if device:
        dev = N.DeviceBuffer(ctx, buf.nbytes)
        dev.upload(buf)
        try:
            r = ctx.clip_fft_batch(dev, offs, lens, fmt=N.FMT_S16 if dtype == np.int16 else N.FMT_F32)
        finally:
            dev.free()
    else:
        r = ctx.clip_fft_batch(buf, offs, lens)
    return [r["bins"][o:o + k] for o, k in zip(r["offsets"], r["counts"])], r["status"]


def _specdist(N, ctx, pairs, device=False, fmt16=False):
    conv = S.as_s16 if fmt16 else (lambda a: np.ascontiguousarray(a, np.float32))
    refs, degs = [conv(r) for r, _ in pairs], [conv(d) for _, d in pairs]
    rl, dl = np.array([r.size for r in refs], np.int64), np.array([d.size for d in degs], np.int64)
    both = np.concatenate(refs + degs + [np.zeros(1, refs[0].dtype)])
    offs = N.packed_offsets(np.concatenate([rl, dl]))
    m = len(pairs)
    if device:
        dev = N.DeviceBuffer(ctx, both.nbytes)
        dev.upload(both)
        try:
            return ctx.specdist_batch(dev, offs[:m], rl, dev, offs[m:], dl, fmt=N.FMT_S16 if fmt16 else N.FMT_F32)
        finally:
            dev.free()
    return ctx.specdist_batch(both, offs[:m], rl, both, offs[m:], dl)


def _all_pairs():
    return [(p["r"], p["d"]) for p in S.pairs()]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_clip_fft_of_every_length_in_one_ragged_batch(N, ctx, device):
    P, Q = S.pairs(), _s16_clips()
    gap = 3 if device else 0                                                     # device clips at every alignment
    f32, st = _fft(N, ctx, [p["r"] for p in P], device, gap)
    assert (st == N.CLIP_OK).all()
    for p, b in zip(P, f32):
        check_bins(b, p, "f32 " + ("device" if device else "host"))
    s16, st = _fft(N, ctx, [q["q"] for q in Q], device, gap)
    assert (st == N.CLIP_OK).all()
    for q, b in zip(Q, s16):
        check_bins(b, q, "s16 " + ("device" if device else "host"))
    conv, _ = _fft(N, ctx, [q["r"] for q in Q], device, gap)
    for q, a, b in zip(Q, s16, conv):                                            # int16 is its float32 conversion, bit for bit
        np.testing.assert_array_equal(a, b, err_msg=str(q["n"]))
    if not device:                                                               # the device agrees with its specification
        for p, b in zip(P, f32):
            assert S.rel_l2(b, N.clip_fft_host(p["r"])["bins"]) <= p["bound"], p["n"]
        e, st = _fft(N, ctx, [P[4]["r"], np.zeros(0, np.float32), np.array([0.5, np.nan, 0.25], np.float32), P[6]["r"]])
        assert st.tolist() == [0, N.CLIP_TOO_SHORT, N.CLIP_NONFINITE, 0] and e[1].size == 0 and np.isnan(e[2]).all()
        np.testing.assert_array_equal(e[0], f32[4])
        np.testing.assert_array_equal(e[3], f32[6])


def test_specdist_records(N, ctx):
    P = S.pairs()
    ref = _specdist(N, ctx, _all_pairs())
    assert (ref["status"] == N.CLIP_OK).all()
    for p, rec in zip(P, ref["rec"]):
        check_record(rec, p, "specdist_batch")
        host = N.specdist_host(p["r"], p["d"])["rec"]
        assert abs(rec[1] - host[1]) / p["n"] <= 2 * p["tol"], p["n"]
    np.testing.assert_array_equal(_specdist(N, ctx, _all_pairs(), device=True)["rec"], ref["rec"])
    s16 = _specdist(N, ctx, _all_pairs(), fmt16=True)
    np.testing.assert_array_equal(_specdist(N, ctx, _all_pairs(), device=True, fmt16=True)["rec"], s16["rec"])
    conv = [(S.as_s16(r).astype(np.float32) / np.float32(32768.0), S.as_s16(d).astype(np.float32) / np.float32(32768.0)) for r, d in _all_pairs()]
    np.testing.assert_array_equal(_specdist(N, ctx, conv)["rec"], s16["rec"])
    # lengths that differ within a pair: the shorter one counts
    cut = _specdist(N, ctx, [(P[8]["r"], P[8]["d"][:2049]), (P[8]["r"][:2049], P[8]["d"][:2049])])["rec"]
    np.testing.assert_array_equal(cut[0], cut[1])
    assert cut[0][0] == 2049
    # equal sample for sample: exactly no distance
    same = _specdist(N, ctx, [(p["r"], p["r"].copy()) for p in P])["rec"]
    assert (same[:, 1] == 0).all() and (same[:, 2] == same[:, 3]).all()


def test_records_do_not_depend_on_the_batch(N, ctx):
    pairs = _all_pairs()
    n = len(pairs)
    ref = _specdist(N, ctx, pairs)["rec"]
    np.testing.assert_array_equal(_specdist(N, ctx, pairs)["rec"], ref)
    np.testing.assert_array_equal(_specdist(N, ctx, pairs[::-1])["rec"], ref[::-1])
    perm = np.random.default_rng(1).permutation(n)
    np.testing.assert_array_equal(_specdist(N, ctx, [pairs[i] for i in perm])["rec"], ref[perm])
    for i, p in enumerate(pairs):
        np.testing.assert_array_equal(_specdist(N, ctx, [p])["rec"][0], ref[i], err_msg=str(S.LENGTHS[i]))
    # three pairs of one N in a chunk share one filter spectrum; small and four-step lengths
    for i in (4, 5, 6, 10):
        r, d = pairs[i]
        trio = _specdist(N, ctx, [(r, d), (d, r), (r, d), pairs[2]])["rec"]
        np.testing.assert_array_equal(trio[0], ref[i])
        np.testing.assert_array_equal(trio[2], ref[i])
        np.testing.assert_array_equal(trio[3], ref[2])
        assert trio[1][2] == ref[i][3] or abs(trio[1][2] - ref[i][3]) <= 1e-12 * ref[i][3]
    # a NaN pair and an empty pair in the middle leave their neighbours' bits alone
    bad = pairs[9][1].copy()
    bad[4321] = np.nan
    inf = pairs[6][0].copy()
    inf[7] = -np.inf
    mixed = pairs[:6] + [(pairs[9][0], bad), (pairs[3][0], np.zeros(0, np.float32)), (inf, pairs[6][1])] + pairs[6:]
    r = _specdist(N, ctx, mixed)
    assert r["status"][6:9].tolist() == [N.CLIP_NONFINITE, N.CLIP_TOO_SHORT, N.CLIP_NONFINITE] and np.isnan(r["rec"][6:9]).all()
    np.testing.assert_array_equal(np.delete(r["rec"], [6, 7, 8], axis=0), ref)
    assert (np.delete(r["status"], [6, 7, 8]) == 0).all()


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_spectrum import _all_pairs, _fft, _specdist
from tests import spectrum_ref as S
from audio_feature_extraction_amd import _native as N
ctx = N.Context(0)
out = {"rec": _specdist(N, ctx, _all_pairs())["rec"], "dev": _specdist(N, ctx, _all_pairs(), device=True)["rec"]}
bins, st = _fft(N, ctx, [p["r"] for p in S.pairs()])
out["bins"], out["st"] = np.concatenate(bins), st
np.savez(sys.argv[2], **out)
"""


def test_chunked_batch_equals_one_chunk(N, ctx, tmp_path):
    assert N.stft_chunks(S.LENGTHS, N.specdist_cost(), CHUNK_BUDGET).max() + 1 >= 4
    assert N.stft_chunks(S.LENGTHS, N.specdist_cost(N.FMT_F32, N.MEM_DEVICE), CHUNK_BUDGET).max() + 1 >= 4
    assert N.stft_chunks(S.LENGTHS, N.specdist_cost(), 2 << 30).max() == 0
    dst = str(tmp_path / "chunked.npz")
    env = dict(os.environ, AFX_TEST_SPECDIST_BUDGET=str(CHUNK_BUDGET))
    subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _CHILD, ROOT, dst], env=env, check=True, timeout=150)
    z = np.load(dst)
    ref = _specdist(N, ctx, _all_pairs())["rec"]
    np.testing.assert_array_equal(z["rec"], ref)
    np.testing.assert_array_equal(z["dev"], ref)
    bins, st = _fft(N, ctx, [p["r"] for p in S.pairs()])
    np.testing.assert_array_equal(z["bins"], np.concatenate(bins))
    np.testing.assert_array_equal(z["st"], st)


def test_refusals(N, ctx):
    big = np.zeros(N.CFFT_MAX_N + 1, np.float32)
    with pytest.raises(NotImplementedError, match="2\\^21"):
        ctx.clip_fft_batch(big, [0], [big.size])
    with pytest.raises(NotImplementedError, match="2\\^21"):
        ctx.specdist_batch(big, [0], [big.size], big, [0], [big.size])
    with pytest.raises(ValueError):
        ctx.specdist_batch(big, [0], [-1], big, [0], [5])
    with pytest.raises(ValueError):
        ctx.clip_fft_batch(big, [0], [-1])
    r = ctx.specdist_batch(big, [0], [big.size], big, [0], [100])                # the shorter side decides
    assert r["status"][0] == 0 and r["rec"][0][0] == 100


def test_pesq_like_batch(N, monkeypatch):
    from audio_feature_extraction_amd import quality
    P = S.pairs()
    got = quality.pesq_like_batch(_all_pairs()[2:])                              # a correlation needs more than two samples
    dist = quality.spec_dist_batch(_all_pairs())
    for p, d in zip(P, dist):
        assert abs(d - p["spec_dist"]) <= p["tol"], (p["n"], d, p["spec_dist"])
    for p, g in zip(P[2:], got):
        assert list(g) == ["snr", "correlation", "spec_dist", "pesq"]
        want = S.pesq_exact(p["r"], p["d"], p["spec_dist"])
        allowed = 0.7 * p["tol"] + 1e-11
        print(f"pesq_like n {p['n']:7d}  {g['pesq']:.15f}  error {abs(g['pesq'] - want):.2e}  allowed {allowed:.2e}")
        assert abs(g["pesq"] - want) <= allowed, (p["n"], g["pesq"], want)
        assert abs(want - S.pesq_like(p["r"], p["d"])["pesq"]) <= 1e-5           # numpy's own float32 means
    assert quality.pesq_like(P[5]["r"], P[5]["d"]) == got[3]["pesq"] and quality.spec_dist(P[5]["r"], P[5]["d"]) == dist[5]
    const = np.full(3000, 0.25, np.float32)
    g = quality.pesq_like_batch([(const, P[8]["r"][:3000])])[0]
    assert np.isnan(g["correlation"]) and np.isnan(g["pesq"]) and np.isfinite(g["spec_dist"])
    for p in (P[4], P[6]):
        check_bins(quality.clip_rfft(p["r"]), p, "quality.clip_rfft")
    # a pair over the device's limit goes through the host executor, with no error to the caller (the limit itself:
    # test_refusals; lowered here, a host transform of 2^23 points takes seconds)
    monkeypatch.setattr(N, "CFFT_MAX_N", 5000)
    both = quality.spec_dist_batch([(P[9]["r"], P[9]["d"]), (P[8]["r"], P[8]["d"])])
    assert both[1] == dist[8] and both[0] == N.specdist_host(P[9]["r"], P[9]["d"])["rec"][1] / 8000
    assert S.rel_l2(quality.clip_rfft(P[9]["r"]), N.clip_fft_host(P[9]["r"])["bins"]) == 0


def test_evaluate_noise_reduction_with_pesq(N):
    from audio_feature_extraction_amd import effects, quality
    from tests import assess_clips as K
    sr = 22050
    rng = np.random.default_rng(11)
    n = 3 * sr
    y = (0.02 * rng.standard_normal(n)).astype(np.float32)                      # the 3 s clip of tests/test_gpu_assess.py
    y[int(0.4 * sr):] += K.tone(sr, n - int(0.4 * sr))
    two = quality.evaluate_noise_reduction(y, sr)
    got = quality.evaluate_noise_reduction(y, sr, pesq=True)
    assert list(got) == ["original", "spectral_subtraction", "wiener_filter"] and all(list(v) == ["snr", "pesq", "stoi"] for v in got.values())
    for k in got:
        assert got[k]["snr"] == two[k]["snr"] and got[k]["stoi"] == two[k]["stoi"], k            # bit for bit
        assert list(two[k]) == ["snr", "stoi"]
    assert got["original"]["pesq"] == 4.5
    outs = {"spectral_subtraction": effects.spectral_subtraction(y, sr), "wiener_filter": effects.wiener_filter(y, sr)}
    for k, d in outs.items():
        R, D = S.truth_fft(y), S.truth_fft(d)
        aR, aD = np.abs(R), np.abs(D)
        dist = float(np.mean(np.abs(aR - aD) / (aR + 1e-10)))
        tol = max(S.bound_for(y), S.bound_for(d)) * S.kappa(R, D)                # this clip's own e_ref: N = 66150 = 2 3^3 5^2 7^2
        want = S.pesq_exact(y, d, dist)
        print(f"evaluate {k:22s} pesq {got[k]['pesq']:.15f}  error {abs(got[k]['pesq'] - want):.2e}  allowed {0.7 * tol + 1e-11:.2e}")
        assert tol <= S.CONDITION_CAP, (k, tol)
        assert abs(got[k]["pesq"] - want) <= 0.7 * tol + 1e-11, (k, got[k]["pesq"], want)
        assert 1.0 <= got[k]["pesq"] < 4.5
