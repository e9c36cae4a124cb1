"""GPU test of the staging buffers the context entry points share (afx_ctx::wave_in / wave_out, afx_plan.h).

Every entry point stages a host batch through the same two device buffers, which grow to the largest batch any of them has
seen.  So one Context runs the nine entry points one after another, three times: a large batch (the buffers grow), a small
one with an empty clip and a NaN clip (each call finds a buffer larger than it needs, holding another call's data), the
large one again.  Every result must equal, element for element, the same call on a fresh Context that has run nothing else;
the outputs go into sentinel-filled arrays whose gaps and failed clips' ranges must stay untouched.  A child process repeats
the first two rounds with the smoothers' budget lowered, so that a call stages more than one chunk."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = np.float32(1234.5)
SR = 22050
OPS = ("sosfiltfilt", "medfilt", "energy_zcr", "loudness", "gate", "compare", "clip_fft", "resample", "decode")
CHUNK_BUDGET = 40000          # medfilt, host to host: 8 bytes a sample, so each clip of the large batch goes alone


def _signal(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / SR
    return (0.3 * np.sin(2 * np.pi * (180.0 + 40.0 * seed) * t) + 0.05 * rng.standard_normal(n)).astype(np.float32)


def batch(which):
    """large: eight clips of about 20 000 samples; small: 300, empty, 700 with a NaN, 513"""
    if which == "large":
        return [_signal(20000 + 37 * k - 400 * (k % 3), k) for k in range(8)]
    bad = _signal(700, 22)
    bad[350] = np.nan
    return [_signal(300, 20), np.zeros(0, np.float32), bad, _signal(513, 23)]


def _pack(clips):
    lengths = np.array([c.size for c in clips], np.int64)
    offsets = np.zeros(len(clips), np.int64)
    offsets[1:] = np.cumsum(lengths)[:-1]
    return np.concatenate(clips).astype(np.float32), offsets, lengths


def _out_for(N, counts):
    """a sentinel-filled array and 4-aligned offsets in it, eight elements in from either end"""
    counts = np.asarray(counts, np.int64)
    oo = N.packed_offsets(counts, 4) + 8
    return np.full(int((oo + counts).max()) + 11, SENTINEL, np.float32), oo


def _gaps_untouched(out, oo, counts, written):
    mask = np.ones(out.size, bool)
    for i, w in enumerate(written):
        if w:
            mask[int(oo[i]):int(oo[i]) + int(counts[i])] = False
    assert mask.sum() >= 16 and (out[mask] == SENTINEL).all()


def run_op(N, ctx, op, clips):
    """one entry point on the batch, host in and host out -> its result arrays by name"""
    y, off, ln = _pack(clips)
    if op in ("sosfiltfilt", "medfilt"):
        out, oo = _out_for(N, ln)
        if op == "sosfiltfilt":
            r = ctx.sosfiltfilt_batch(y, off, ln, N.butter_sos(5, 200 / (SR / 2), True), 18, out=out, out_offsets=oo)
        else:
            r = ctx.medfilt_batch(y, off, ln, 5, out=out, out_offsets=oo)
        _gaps_untouched(out, oo, ln, r["status"] == N.CLIP_OK)
        return {k: np.asarray(v) for k, v in r.items() if k != "offsets"}
    if op == "energy_zcr":
        r = ctx.energy_zcr_batch(y, off, ln, SR, 2048, 512, N.EZ_PREPROCESS | N.EZ_ENERGY | N.EZ_ZCR)
        return {"rec": r["rec"], "status": r["status"]}
    if op == "loudness":
        res = {}
        for mode in (N.LOUD_NORM_LOUDNESS, N.LOUD_NORM_PEAK):
            out, oo = _out_for(N, ln)
            r = ctx.loudness_batch(y, off, ln, SR, mode=mode, target=-20.0 if mode == N.LOUD_NORM_LOUDNESS else -3.0, out=out, out_offsets=oo)
            _gaps_untouched(out, oo, ln, r["status"] == N.CLIP_OK)
            res.update({f"out{mode}": out, f"rec{mode}": r["rec"], f"status{mode}": r["status"]})
        return res
    if op == "gate":
        # each clip's noise clip lies behind the clips in the same buffer
        noise = [_signal(min(4000, max(c.size, 256)), 50 + i) for i, c in enumerate(clips)]
        yn, noff, nln = _pack(list(clips) + noise)
        n = len(clips)
        out, oo = _out_for(N, ln)
        r = ctx.gate_batch(yn, noff[:n], nln[:n], N.gate_opts(SR, stationary=True), noise_offsets=noff[n:], noise_lengths=nln[n:],
                           out=out, out_offsets=oo, want_thresh=True)
        _gaps_untouched(out, oo, ln, np.isin(r["status"], (N.CLIP_OK, N.CLIP_NONFINITE)))     # a non-finite clip comes back as zeros
        return {"out": out, "status": r["status"], "thresh": r["thresh"]}
    if op == "compare":
        deg = (np.float32(0.9) * y + np.float32(0.01)).astype(np.float32)
        r = ctx.compare_batch(y, off, ln, deg, off, ln)
        return {"rec": r["rec"], "status": r["status"]}
    if op == "clip_fft":
        r = ctx.clip_fft_batch(y, off, ln)
        return {"bins": r["bins"], "status": r["status"]}
    if op == "resample":
        olen = N.resample_lengths(ln, SR, 16000)
        out, oo = _out_for(N, olen)
        r = ctx.resample_batch(y, off, ln, SR, 16000, out=out, out_offsets=oo)
        _gaps_untouched(out, oo, olen, olen > 0)
        return {"out": out, "lengths": r["lengths"]}
    assert op == "decode"
    # float32 mono and 16-bit stereo clips in turn, each from a multiple of 16 bytes
    raws, frames, kinds, chans = [], [], [], []
    for i, c in enumerate(clips):
        if i % 2 == 0:
            raws.append(c.astype("<f4").tobytes()); frames.append(c.size); kinds.append(N.SMP_F32); chans.append(1)
        else:
            q = np.round(np.nan_to_num(c[:c.size // 2 * 2]) * 32767.0).astype("<i2")
            raws.append(q.tobytes()); frames.append(c.size // 2); kinds.append(N.SMP_S16); chans.append(2)
    boff = N.packed_offsets([len(b) for b in raws], 16)
    raw = np.zeros(int(boff[-1]) + len(raws[-1]), np.uint8)
    for b, o in zip(raws, boff):
        raw[int(o):int(o) + len(b)] = np.frombuffer(b, np.uint8)
    slots = (np.asarray(frames, np.int64) + 3) // 4 * 4                 # a clip's slot is written up to a multiple of 4
    out, oo = _out_for(N, slots)
    ctx.decode_batch(raw, boff, np.asarray(frames, np.int64), kinds, chans, out=out, out_offsets=oo)
    _gaps_untouched(out, oo, slots, slots > 0)
    return {"out": out}


def fresh(N, clips):
    """every entry point on a Context of its own"""
    res = {}
    for op in OPS:
        ctx = N.Context(0)
        res[op] = run_op(N, ctx, op, clips)
        ctx.close()
    return res


def run_round(N, ctx, clips):
    return {op: run_op(N, ctx, op, clips) for op in OPS}


def assert_same(got, want, what):
    for op in OPS:
        assert got[op].keys() == want[op].keys()
        for k, w in want[op].items():
            g = got[op][k]
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w, equal_nan=True), (what, op, k)


@pytest.fixture(scope="module")
def N():
    from audio_feature_extraction_amd import _native
    if _native.device_count() < 1:
        pytest.fail("no GPU visible")
    return _native


@pytest.fixture(scope="module")
def refs(N):
    return {which: fresh(N, batch(which)) for which in ("large", "small")}


def test_a_context_that_ran_other_batches_gives_a_fresh_contexts_results(N, refs):
    ctx = N.Context(0)
    for rnd, which in enumerate(("large", "small", "large"), 1):
        assert_same(run_round(N, ctx, batch(which)), refs[which], f"round {rnd}")
    ctx.close()
    # what the small batch must show: its empty and its NaN clip, seen as such
    small = refs["small"]
    assert list(small["medfilt"]["status"]) == [N.CLIP_OK, N.CLIP_TOO_SHORT, N.CLIP_NONFINITE, N.CLIP_OK]
    assert list(small["sosfiltfilt"]["status"]) == [N.CLIP_OK, N.CLIP_TOO_SHORT, N.CLIP_NONFINITE, N.CLIP_OK]
    assert list(refs["large"]["loudness"][f"status{N.LOUD_NORM_LOUDNESS}"]) == [N.CLIP_OK] * 8


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_ctx_staging import OPS, batch, run_round
from audio_feature_extraction_amd import _native as N
ctx = N.Context(0)
flat = {}
for which in ("large", "small"):
    for op, res in run_round(N, ctx, batch(which)).items():
        flat.update({f"{which}.{op}.{k}": v for k, v in res.items()})
np.savez(sys.argv[2], **flat)
"""


def test_the_same_with_calls_that_stage_several_chunks(refs, tmp_path):
    env = dict(os.environ, AFX_TEST_SMOOTH_BUDGET=str(CHUNK_BUDGET))
    dst = str(tmp_path / "rounds.npz")
    subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _CHILD, ROOT, dst], env=env, check=True, timeout=150)
    z = np.load(dst)
    for which in ("large", "small"):
        got = {op: {k: z[f"{which}.{op}.{k}"] for k in refs[which][op]} for op in OPS}
        assert_same(got, refs[which], f"chunked {which}")
