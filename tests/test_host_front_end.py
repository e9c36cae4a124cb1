"""The host layer's shared front end, called directly (no library, no device): the packed-offset arithmetic, the clip-array
and sample-source checks every batch method of _native goes through, and the run cutter of parallel.process_files."""
import numpy as np
import pytest

from audio_feature_extraction_amd import _native as N
from audio_feature_extraction_amd import parallel


def test_packed_offsets():
    for align in (1, 4):
        e = N.packed_offsets([], align)
        assert e.dtype == np.int64 and e.shape == (0,)
        one = N.packed_offsets([7], align)
        assert one.dtype == np.int64 and one.tolist() == [0]
    assert N.packed_offsets([3, 4, 5, 0, 2]).tolist() == [0, 3, 7, 12, 12]
    assert N.packed_offsets([3, 4, 5, 0, 2], 4).tolist() == [0, 4, 8, 16, 16]
    assert N.packed_offsets(np.array([8, 1], np.int32), 4).tolist() == [0, 8]
    got = N.packed_offsets(np.array([5, 5, 5]), align=1)
    assert got.dtype == np.int64 and got.flags.c_contiguous and got.tolist() == [0, 5, 10]


def test_pack_output_is_unchanged():
    clips = [np.arange(1, 6, dtype=np.int16), np.arange(10, 14, dtype=np.int16), np.array([7], np.int16),
             np.zeros(0, np.int16), np.array([9, 9], np.int16)]
    buf, offs, lens = parallel._pack(clips, np.int16)
    assert buf.dtype == np.int16 and offs.dtype == np.int64 and lens.dtype == np.int64
    assert lens.tolist() == [5, 4, 1, 0, 2] and offs.tolist() == [0, 8, 12, 16, 16]
    assert buf.tolist() == [1, 2, 3, 4, 5, 0, 0, 0, 10, 11, 12, 13, 7, 0, 0, 0, 9, 9, 0, 0]
    buf, offs, lens = parallel._pack([], np.float32)
    assert buf.shape == (0,) and buf.dtype == np.float32 and offs.shape == (0,) and lens.shape == (0,)


def test_clip_arrays():
    offs, lens = np.array([0, 8], np.int64), np.array([5, 3], np.int64)
    o, l, n = N._clip_arrays(offs, lens)
    assert n == 2 and np.shares_memory(o, offs) and np.shares_memory(l, lens)         # qualifying arrays are not copied
    o, l, n = N._clip_arrays([0, 8, 16], np.array([5, 3, 1], np.int32))
    assert n == 3 and o.dtype == l.dtype == np.int64 and o.flags.c_contiguous and l.tolist() == [5, 3, 1]
    o, l, n = N._clip_arrays(np.arange(0, 40, 4, dtype=np.int64)[::2], np.ones(5, np.int64))
    assert n == 5 and o.flags.c_contiguous and o.tolist() == [0, 8, 16, 24, 32]
    assert N._clip_arrays([], [])[2] == 0
    for bad in (([0, 8], [5]), ([0], [5, 3]), ([], [1])):
        with pytest.raises(ValueError):
            N._clip_arrays(*bad)


def test_sample_source_of_a_host_array():
    offs, lens, _ = N._clip_arrays([0, 8], [5, 4])
    y = np.zeros(12, np.float32)
    assert N._sample_source(y, N.FMT_F32, offs, lens) == (y.ctypes.data, N.MEM_HOST)
    assert N._sample_source(y, N.FMT_F32, offs, lens, mem=N.MEM_HOST) == (y.ctypes.data, N.MEM_HOST)
    q = np.zeros(12, np.int16)
    assert N._sample_source(q, N.FMT_S16, offs, lens) == (q.ctypes.data, N.MEM_HOST)
    empty = N._clip_arrays([], [])
    assert N._sample_source(np.zeros(0, np.float32), N.FMT_F32, empty[0], empty[1])[1] == N.MEM_HOST
    for mem in (None, N.MEM_HOST):
        with pytest.raises(ValueError):                                   # wrong dtype for the format, both ways
            N._sample_source(q, N.FMT_F32, offs, lens, mem=mem)
        with pytest.raises(ValueError):
            N._sample_source(y, N.FMT_S16, offs, lens, mem=mem)
        with pytest.raises(ValueError):
            N._sample_source(y.astype(np.float64), N.FMT_F32, offs, lens, mem=mem)
        with pytest.raises(ValueError):                                   # not contiguous
            N._sample_source(np.zeros(24, np.float32)[::2], N.FMT_F32, offs, lens, mem=mem)
        with pytest.raises(ValueError):                                   # the second clip ends at 12 > 11
            N._sample_source(np.zeros(11, np.float32), N.FMT_F32, offs, lens, mem=mem)


def test_sample_source_on_the_device():
    offs, lens, _ = N._clip_arrays([0, 8], [5, 4])
    assert N._sample_source(0x7f0000001000, N.FMT_S16, offs, lens) == (0x7f0000001000, N.MEM_DEVICE)
    assert N._sample_source(0x7f0000001000, N.FMT_S16, offs, lens, mem=N.MEM_DEVICE) == (0x7f0000001000, N.MEM_DEVICE)
    buf = N.DeviceBuffer.__new__(N.DeviceBuffer)                          # no allocation: only the address is read
    buf.ptr = 0x7f0000002000
    try:
        assert N._sample_source(buf, N.FMT_F32, offs, lens) == (0x7f0000002000, N.MEM_DEVICE)
        with pytest.raises(ValueError):                                   # host only (zcr_batch, spectral_batch)
            N._sample_source(buf, N.FMT_F32, offs, lens, mem=N.MEM_HOST)
    finally:
        buf.ptr = None
    with pytest.raises(ValueError):
        N._sample_source(0x7f0000001000, N.FMT_F32, offs, lens, mem=N.MEM_HOST)


def test_sample_fmt_inference_of_resample_batch():
    assert N._sample_fmt(np.zeros(4, np.int16), None) == N.FMT_S16
    assert N._sample_fmt(np.zeros(4, np.float32), None) == N.FMT_F32
    assert N._sample_fmt(np.zeros(4, np.float64), None) == N.FMT_F32      # ... which the dtype check then rejects
    assert N._sample_fmt(np.zeros(4, np.float32), N.FMT_S16) == N.FMT_S16  # an explicit fmt is taken as given
    assert N._sample_fmt(0x1000, N.FMT_S16) == N.FMT_S16
    with pytest.raises(ValueError):
        N._sample_fmt(0x1000, None)                                       # a device address says nothing about its samples


def test_budget_runs():
    runs = lambda *a, **k: list(parallel._budget_runs(*a, **k))
    assert runs([], 10) == []
    assert runs([3, 3, 3, 3], 10) == [(0, 3), (3, 4)]
    # an item larger than the budget is a run of its own
    assert runs([4, 25, 4, 4], 10) == [(0, 1), (1, 2), (2, 4)]
    assert runs([25], 10) == [(0, 1)]
    # exact fit: tot + size == budget stays in the run, one more does not
    assert runs([4, 6, 1], 10) == [(0, 2), (2, 3)]
    assert runs([4, 6, 0, 1], 10) == [(0, 3), (3, 4)]
    # a key change ends a run although budget is left; the same key later starts a new run
    assert runs([1, 1, 1, 1, 1], 10, keys=[8000, 8000, 16000, 16000, 8000]) == [(0, 2), (2, 4), (4, 5)]
    assert runs([6, 6, 6], 10, keys=[1, 1, 1]) == [(0, 1), (1, 2), (2, 3)]
    # numpy inputs, as process_files passes them
    assert runs(np.array([5, 5, 5], np.int64), 10, keys=np.array([2, 2, 2], np.int64)) == [(0, 2), (2, 3)]
    rng = np.random.default_rng(3)
    sizes, keys = rng.integers(1, 50, 200), np.sort(rng.integers(0, 3, 200))
    got = runs(sizes, 100, keys=keys)
    assert got[0][0] == 0 and got[-1][1] == 200 and all(a[1] == b[0] for a, b in zip(got, got[1:]))
    for pos, end in got:
        assert end > pos and (end - pos == 1 or sizes[pos:end].sum() <= 100) and len(set(keys[pos:end])) == 1
        if end < 200 and keys[end] == keys[pos]:                          # greedy: the next item did not fit
            assert sizes[pos:end].sum() + sizes[end] > 100
