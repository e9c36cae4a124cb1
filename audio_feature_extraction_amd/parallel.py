"""Embarrassingly parallel file sharding for ``batch_process``.

Clips are independent (every cross-frame coupling -- trim max, top_db max, delta
stencil, mean/std -- is intra-clip), so N GPUs = N independent shards and the only
"collective" is a host-side gather of 4*n_mfcc+3 floats per file.  No RCCL, no xGMI
traffic.  Two deployment shapes share the partition/gather helpers here:

* in-process: one worker thread per visible GPU, each with its own afx context,
  plan and stream (``process_files``; what ``AudioFeatureExtractor.batch_process`` uses);
* one process per GPU under ``torch.distributed`` (``shard_range`` + ``gather_shards``;
  what ``bench.py --gpus N`` uses) -- the reference's only parallel precedent is a
  ``multiprocessing.Pool`` over files
  (04_feature_extraction_experiment/feature_extraction_for_student.py:168-174).
"""
from __future__ import annotations

import os
import queue
import sys
import threading
import time
from concurrent.futures import ThreadPoolExecutor
from typing import Any, Dict, List, Sequence, Tuple

import numpy as np

from . import _native, wavio
from .core.feature_extractor import AudioFeatureExtractor, _status_error
from .hostinfo import usable_cpus


def lpt_partition(lengths: Sequence[int], n_parts: int) -> List[List[int]]:
    """Longest-processing-time-first: sort by length (desc), give each clip to the least
    loaded part.  Equal lengths degenerate to a round-robin deal.  Every part keeps its
    indices in ascending order."""
    n_parts = max(1, int(n_parts))
    parts: List[List[int]] = [[] for _ in range(n_parts)]
    load = [0] * n_parts
    order = sorted(range(len(lengths)), key=lambda i: (-int(lengths[i]), i))
    for i in order:
        p = min(range(n_parts), key=lambda q: (load[q], q))
        parts[p].append(i)
        load[p] += int(lengths[i]) + 1
    for p in parts:
        p.sort()
    return parts


def shard_range(n_items: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous balanced shard [lo, hi) of rank ``rank`` out of ``world``."""
    base, rem = divmod(int(n_items), int(world))
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def gather_shards(local: np.ndarray, n_total: int, rank: int, world: int, group=None) -> np.ndarray:
    """All ranks contribute the rows of their ``shard_range`` shard; every rank gets the
    [n_total, ...] array in global order.  Host-side gather (gloo or nccl-backed object
    gather); the data path itself has no collective."""
    if world == 1:
        return np.asarray(local)
    import torch.distributed as dist
    parts: List[Any] = [None] * world
    dist.all_gather_object(parts, np.asarray(local), group=group)
    out = np.concatenate([np.asarray(p) for p in parts], axis=0)
    if out.shape[0] != n_total:
        raise RuntimeError(f"gathered {out.shape[0]} rows, expected {n_total}")
    return out


def _decode(path: str, sr: int, keep_rate: bool = False):
    """-> ('s16'|'f32', mono array, its rate) ; PCM16 mono files at the target rate stay int16 so that
    the upload is 2 bytes/sample and the /32768 happens on the GPU (bit-identical).  A file at another rate is
    resampled to ``sr`` on the host, or with ``keep_rate`` left at its own rate for the device resampler."""
    a, rate, kind = wavio.read_wav_raw(path)
    if kind == "s16" and a.shape[1] == 1 and rate == sr:
        return "s16", np.ascontiguousarray(a[:, 0]), rate
    y = wavio.to_mono(wavio.to_float32(a, kind))
    if rate != sr and not keep_rate:
        y, rate = wavio.resample(y, rate, sr), sr
    return "f32", y, rate


_ALIGN = 4               # clips start on 4-element boundaries (enables the kernels' 16-byte loads)
_RAW_ALIGN = 16          # raw WAVE data: clips start on 16-byte boundaries (afx_decode_batch)


def _raw_padded(nbytes):
    """A clip's byte count, or an array of them, rounded up to the raw alignment."""
    return (nbytes + (_RAW_ALIGN - 1)) // _RAW_ALIGN * _RAW_ALIGN


def _padded(n):
    """A clip length, or an array of them, rounded up to the alignment."""
    return (n + (_ALIGN - 1)) // _ALIGN * _ALIGN


def _pack(clips: List[np.ndarray], dtype) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Packs clips with 4-element alignment."""
    lengths = np.array([c.size for c in clips], np.int64)
    offsets = _native.packed_offsets(lengths, _ALIGN)
    buf = np.zeros(int(_padded(lengths).sum()), dtype)
    for c, o in zip(clips, offsets):
        buf[o:o + c.size] = c
    return buf, offsets, lengths


class _PinPool:
    """Page-locked window buffers of one (device, lane) worker, kept across windows and calls: the native reader fills
    them, the upload is one DMA.  At most two are out at a time (window k on the device, k + 1 being read)."""

    def __init__(self, plan):
        self.plan, self.free, self.lock = plan, [], threading.Lock()

    def get(self, nbytes: int):
        with self.lock:
            for i, b in enumerate(self.free):
                if b.nbytes >= nbytes:
                    return self.free.pop(i)
            for b in self.free:                      # too small: give the memory back before taking more
                b.free()
            self.free.clear()
        return self.plan.pinned_buffer(max(int(nbytes * 1.25), 1 << 20))

    def put(self, b):
        with self.lock:
            self.free.append(b)


class _DevPool:
    """The HBM window buffer of one (device, lane) worker, kept across windows and calls (a worker has one window on the
    device at a time).  hipMalloc / hipFree per window cost more than their own time: a free synchronises the whole device,
    i.e. also the passes the other workers have in flight."""

    def __init__(self, plan):
        self.plan, self.buf, self.lock = plan, None, threading.Lock()

    def get(self, nbytes: int):
        with self.lock:
            b, self.buf = self.buf, None
        if b is not None and getattr(b, "nbytes", 0) >= nbytes:
            return b
        if b is not None:
            b.free()
        return self.plan.device_buffer(max(int(nbytes * 1.25), 16))

    def put(self, b):
        with self.lock:
            old, self.buf = self.buf, b
        if old is not None:
            old.free()


_switch_lock = threading.Lock()
_switch_state = [0, 0.0]               # process_files calls in flight, the interpreter's own switch interval


def _fast_switch(on: bool):
    """The interpreter's thread switch interval at 0.2 ms while any process_files call runs (first in saves it, last out
    restores it: calls may overlap)."""
    with _switch_lock:
        if on:
            if _switch_state[0] == 0:
                _switch_state[1] = sys.getswitchinterval()
                sys.setswitchinterval(2e-4)
            _switch_state[0] += 1
        else:
            _switch_state[0] -= 1
            if _switch_state[0] == 0:
                sys.setswitchinterval(_switch_state[1])


LAST_TIMING: Dict[str, Any] = {}     # seconds per phase of the last process_files call (developer aid)
WORKERS_PER_GPU = 3     # sub-batches in flight per GPU (own context / stream / thread): copies, the bandwidth-bound
                        # kernels and the host round trip of one hide under the frame kernel of another
DECODE_THREADS_PER_GPU = 16


def _windows(sizes: Sequence[int], idxs: Sequence[int], budget: int) -> List[List[int]]:
    """Cuts a lane's files (in order) into windows whose estimated sample count stays under ``budget``;
    a single file larger than the budget is a window of its own.  The windows are of even size -- as many as the budget
    demands, each an even share of the lane's samples: a short last window costs a whole device pass (the pYIN pass of 30
    clips takes as long as that of 300: its Viterbi kernel is 862 dependent steps whatever the number of clips)."""
    total = sum(int(sizes[i]) for i in idxs)
    nwin = max(1, -(-total // max(int(budget), 1)))
    share = total / nwin
    out: List[List[int]] = []
    cur: List[int] = []
    tot = done = 0
    for i in idxs:
        sz = int(sizes[i])
        if cur and (tot + sz > budget or (done + tot >= share * (len(out) + 1) and len(out) + 1 < nwin)):
            out.append(cur)
            done += tot
            cur, tot = [], 0
        cur.append(i)
        tot += sz
    if cur:
        out.append(cur)
    return out


FEATURE_GROUPS = ("f0", "mfcc", "energy")        # README.md:141-146 (features_to_extract); dict order is this order


def normalize_features(features_to_extract) -> Tuple[str, ...]:
    """None -> all three groups (the reference's behaviour); otherwise the requested subset, validated, in dict order."""
    if features_to_extract is None:
        return FEATURE_GROUPS
    if isinstance(features_to_extract, str):
        features_to_extract = [features_to_extract]
    req = [str(f) for f in features_to_extract]
    bad = [f for f in req if f not in FEATURE_GROUPS]
    if bad:
        raise ValueError(f"features_to_extract: unknown feature group(s) {bad}; choose from {list(FEATURE_GROUPS)}")
    if not req:
        raise ValueError(f"features_to_extract is empty; choose from {list(FEATURE_GROUPS)}")
    return tuple(g for g in FEATURE_GROUPS if g in req)


def _size_estimate(path) -> int:
    """A file's sample count as its size says (a proxy for clip length that needs no decode, not even a header read: exact
    for 16-bit mono; a stereo or wider file counts for more than its mono samples, so its windows -- which bound the
    page-locked host memory, two per worker -- come out smaller than the device budget allows; the sub-batches themselves
    are cut from the frame counts the probe reports)."""
    try:
        return max(1, os.path.getsize(str(path)) // 2)
    except OSError:
        return 1


def _budget_runs(sizes: Sequence[int], budget: int, keys=None):
    """Cuts items (in order) into runs (pos, end): a run holds at least one item, never exceeds ``budget`` with more than
    one item, and with ``keys`` never mixes keys."""
    pos, n = 0, len(sizes)
    while pos < n:
        tot, end = int(sizes[pos]), pos + 1
        while end < n and (keys is None or keys[end] == keys[pos]) and tot + int(sizes[end]) <= budget:
            tot += int(sizes[end])
            end += 1
        yield pos, end
        pos = end


def _lane_pool(extractor, attr: str, key, make):
    """The pool ``key`` of the extractor's ``attr`` (_dev_pools / _pin_pools: kept with the extractor across calls)."""
    pools = extractor.__dict__.setdefault(attr, {})
    return pools.get(key) or pools.setdefault(key, make())


class _Lane:
    """What one (device, lane) worker drives: the MFCC / RMS plan and the pYIN plan (own context and stream each), its
    pooled device buffers and, where the plan offers them, page-locked window buffers, the device resampler and the device
    decoder."""

    def __init__(self, extractor, lane, want_f0: bool):
        self.plan = extractor._plan(lane[0], lane[1])
        self.plan_f0 = extractor._plan(lane[0], (lane[1], "f0")) if want_f0 else None
        self.dev = _lane_pool(extractor, "_dev_pools", lane, lambda: _DevPool(self.plan))
        self.can_rs = hasattr(self.plan, "resample_batch")
        self.can_dec = hasattr(self.plan, "decode_batch")          # raw WAVE data is converted and mixed down on the device
        self.dev_in = self.dev_raw = self.pin = None
        if self.can_rs or self.can_dec:                           # the resampler's input: a second pooled device buffer
            self.dev_in = _lane_pool(extractor, "_dev_pools", (lane, "in"), lambda: _DevPool(self.plan))
        if self.can_dec:                                          # the decoder's input: the raw bytes of a sub-batch
            self.dev_raw = _lane_pool(extractor, "_dev_pools", (lane, "raw"), lambda: _DevPool(self.plan))
        self.pin_raw = None
        if hasattr(self.plan, "pinned_buffer"):                   # page-locked window buffers, kept with the extractor:
            self.pin = _lane_pool(extractor, "_pin_pools", lane, lambda: _PinPool(self.plan))     # int16 windows
            if self.can_dec:                                      # raw byte windows, of other sizes: a pool of their own
                self.pin_raw = _lane_pool(extractor, "_pin_pools", (lane, "raw"), lambda: _PinPool(self.plan))


class _Job:
    """The state of one process_files call: what its lane workers and the calling thread share."""

    def __init__(self, extractor, files, budget, workers_per_gpu, features_to_extract):
        self.ex, self.files, self.budget, self.log = extractor, files, budget, extractor.logger
        n = len(files)
        devices = extractor._devices()
        self.t_start = time.perf_counter()
        self.errors: List[Any] = [None] * n
        K = self.K = extractor.n_mfcc
        self.stats = np.zeros((n, 4 * K + 3), np.float32)
        self.status = np.full(n, -1, np.int32)          # -1: not extracted (yet)
        self.nframes = np.zeros(n, np.int32)
        self.f0s = np.zeros((n, 4), np.float64)
        self.f0_done = np.zeros(n, bool)
        self.nsamp = np.zeros(n, np.int64)
        self.lanes = [(d, w) for d in devices for w in range(max(1, int(workers_per_gpu)))]
        if n < 4 * len(self.lanes):                             # small jobs: one worker per GPU
            self.lanes = [(d, 0) for d in devices]
        # shard by file size: longest-processing-time-first
        self.sizes = [_size_estimate(f) for f in files]
        self.parts = lpt_partition(self.sizes, len(self.lanes))
        self.flags = _native.FLAG_PREEMPH | _native.FLAG_TRIM
        self.want = normalize_features(features_to_extract)
        self.want_f0, self.want_stats = "f0" in self.want, ("mfcc" in self.want or "energy" in self.want)
        host_cpus = usable_cpus()                   # the job's share of the host, not os.cpu_count()
        self.pool = ThreadPoolExecutor(max(1, min(host_cpus, DECODE_THREADS_PER_GPU * len(devices), n)))
        self.native_threads = max(1, min(host_cpus, DECODE_THREADS_PER_GPU * len(devices)) // max(1, min(len(self.lanes), 4)))
        self.win_pool = ThreadPoolExecutor(max(1, len(self.lanes)))
        self.phase = {"decode_wait": 0.0, "device": 0.0}
        # files by the ingest path that took them: native_s16 / native_raw count files the native readers delivered to a
        # device pass, python the files handed to the Python decoder (those it rejects included)
        self.ingest = {"native_s16": 0, "native_raw": 0, "python": 0}
        self.phase_lock = threading.Lock()
        self.timeline: List[Any] = []            # (lane, clips, t_begin, t_uploaded, t_f0_done, t_collected) per sub-batch
        self.finished: Any = queue.SimpleQueue()  # index lists of sub-batches whose results are in the arrays
        self.recs: List[Any] = [None] * n
        # the result dicts are built here, in plain Python, while the extractor's own builders are the stock ones
        self.stock = (getattr(type(extractor), "_stats_to_dicts", None) is AudioFeatureExtractor._stats_to_dicts and
                      getattr(type(extractor), "_f0_to_dict", None) is AudioFeatureExtractor._f0_to_dict)

    def now(self) -> float:
        return time.perf_counter() - self.t_start

    def decode(self, i: int, keep_rate: bool):
        try:
            return _decode(str(self.files[i]), self.ex.sr, keep_rate)
        except Exception as e:          # load_audio: log + the file is dropped
            self.log.error(f"載入音頻文件失敗: {str(e)}")
            self.errors[i] = e
            return None

    def load_window(self, win, pin=None, can_rs=False, can_dec=False, pin_raw=None):
        """-> (packed 16-bit group or None, packed raw group or None, indices decoded by wavio, their decoded clips);
        pin / pin_raw: the worker's pools of page-locked int16 / byte buffers (None: ordinary memory); can_rs: the plan resamples on the device, so
        16-bit mono files of any rate are read natively (laid out rate by rate, the extractor's own rate first) and
        decoded files keep theirs; can_dec: the plan converts and mixes down raw WAVE data on the device.

        Files that need no conversion -- 16-bit PCM, mono, at the target rate: what a corpus of speech clips is -- never
        pass through Python: libafx parses their headers and reads their samples straight into the packed int16 batch
        buffer with native threads (afx_wav_probe / afx_wav_read_s16).  With can_dec, the data chunk of every other file
        afx_decode_batch takes (PCM 8 / 16 / 24 / 32 bit, float 32 / 64 bit, 1 to 7 channels, any rate) is read as it is
        into a byte window, each clip at a 16-byte boundary (afx_wav_read_raw).  Everything else, and any file the native
        readers cannot open or parse, goes through wavio (which also produces the error a bad file is logged with)."""
        sr = self.ex.sr
        rest = list(win)
        packed = rawpack = None
        held = None
        try:
            paths = [str(self.files[i]) for i in win]
            pr = _native.wav_probe(paths, self.native_threads)
            ok = (pr["status"] == 0) & (pr["tag"] == 1) & (pr["bits"] == 16) & (pr["channels"] == 1)
            ok &= (pr["rate"] > 0) if can_rs else (pr["rate"] == sr)
            sel = np.nonzero(ok)[0]
            if sel.size and (pr["rate"][sel] != sr).any():
                sel = sel[np.lexsort((sel, pr["rate"][sel], pr["rate"][sel] != sr))]
            if sel.size:
                lens = pr["frames"][sel].astype(np.int64)
                padded = _padded(lens)
                offs = _native.packed_offsets(lens, _ALIGN)
                nel = max(int(padded.sum()), 1)
                if pin is not None:
                    held = pin.get(nel * 2)
                    buf = held.array(np.int16, nel)
                else:
                    buf = np.empty(nel, np.int16)
                st = _native.wav_read_s16([paths[j] for j in sel], pr["data_off"][sel], lens, buf, offs, self.native_threads)
                for o, ln, pd in zip(offs[padded > lens], lens[padded > lens], padded[padded > lens]):
                    buf[o + ln: o + pd] = 0
                good = st == 0
                if good.any():
                    packed = ([win[j] for j in sel[good]], buf, offs[good], lens[good], held,
                              pr["rate"][sel[good]].astype(np.int64))
                    held = None
                    taken = set(packed[0])
                    rest = [i for i in win if i not in taken]
            if can_dec:
                rawpack = self.load_raw(win, paths, pr, ~ok, pin_raw)
                if rawpack is not None:
                    taken = set(rawpack[0])
                    rest = [i for i in rest if i not in taken]
        except Exception:                                         # no native reader: the Python decoder takes the window
            for pool, held_by in ((pin, packed and packed[4]), (pin_raw, rawpack and rawpack[7])):
                if held_by is not None:
                    pool.put(held_by)
            rest, packed, rawpack = list(win), None, None
        if held is not None:
            pin.put(held)
        decoded = list(self.pool.map(self.decode, rest, [can_rs] * len(rest))) if rest else []
        return packed, rawpack, rest, decoded

    def load_raw(self, win, paths, pr, free, pin):
        """The raw group of a window: of the probed files ``free`` marks (not taken as 16-bit mono), those the device
        decoder takes, their data chunks read into one byte window (page-locked with ``pin``) rate by rate, the extractor's
        own rate first -> (file indices, bytes, byte offsets, frames, kinds, channels, rates, held buffer) or None.  A file
        whose read fails is left to the Python decoder."""
        kinds = _native.wav_sample_kinds(pr)
        sel = np.nonzero(free & (kinds >= 0))[0]
        if not sel.size:
            return None
        sr = self.ex.sr
        sel = sel[np.lexsort((sel, pr["rate"][sel], pr["rate"][sel] != sr))]
        frames = pr["frames"][sel].astype(np.int64)
        chans = pr["channels"][sel].astype(np.int32)
        nbytes = frames * _native.SMP_BYTES[kinds[sel]] * chans
        boffs = _native.packed_offsets(nbytes, _RAW_ALIGN)
        total = max(int(boffs[-1] + _raw_padded(nbytes[-1])), _RAW_ALIGN)
        held = pin.get(total) if pin is not None else None
        good = None
        try:
            buf = held.array(np.uint8, total) if held is not None else np.empty(total, np.uint8)
            st = _native.wav_read_raw([paths[j] for j in sel], pr["data_off"][sel], nbytes, buf, boffs, self.native_threads)
            good = st == 0
        finally:
            if held is not None and (good is None or not good.any()):
                pin.put(held)
        if not good.any():
            return None
        return ([win[j] for j in sel[good]], buf, boffs[good], frames[good], kinds[sel[good]], chans[good],
                pr["rate"][sel[good]].astype(np.int64), held)

    def resample_on_device(self, lane: _Lane, buf, offs, lens, fmt, rate: int, din=None):
        """Clips at ``rate`` -> float32 clips at the extractor's rate in a pooled device buffer (4-aligned, as _pack):
        (buffer, offsets, lengths), or None for a rate pair the device resampler does not hold.  ``buf``: the clips in host
        memory, uploaded to a pooled input buffer that always goes back to its pool (the resampler is synchronous: it is
        done with); or ``din``: a device buffer that holds them already and stays the caller's.  The output buffer goes
        back to its pool on every exit but the first."""
        sr = int(self.ex.sr)
        olens = _native.resample_lengths(lens, rate, sr)             # known on the host: no read-back
        ooffs = _native.packed_offsets(olens, _ALIGN)
        own = din is None
        if own:
            din = lane.dev_in.get(max(buf.nbytes, 16))
        dbuf = None
        try:
            if own:
                din.upload(buf)
            dbuf = lane.dev.get(max(4 * int(ooffs[-1] + _padded(olens[-1])), 16))
            lane.plan.resample_batch(din, offs, lens, rate, sr, fmt=fmt, out=dbuf, out_offsets=ooffs)
        except BaseException as e:
            if dbuf is not None:
                lane.dev.put(dbuf)
            if isinstance(e, NotImplementedError):
                return None
            raise
        finally:
            if own:
                lane.dev_in.put(din)
        return dbuf, ooffs, olens

    def resample_on_host(self, buf, offs, lens, fmt, rate: int):
        """The fallback of resample_on_device: wavio.resample clip by clip -> packed float32 (buffer, offsets, lengths)."""
        f = np.float32(1.0 / 32768.0) if fmt == _native.FMT_S16 else None
        ys = [wavio.resample(buf[o:o + ln].astype(np.float32) * f if f is not None else buf[o:o + ln], rate, int(self.ex.sr))
              for o, ln in zip(offs, lens)]
        return _pack(ys, np.float32)

    def run_group(self, lane: _Lane, cur, buf, offs, lens, fmt, rate: int):
        """One sub-batch: upload, (resample on the device when ``rate`` is another rate than the extractor's,) both passes."""
        tl = [None, len(cur), self.now(), 0.0, 0.0, 0.0]
        dbuf = None
        if rate != int(self.ex.sr):
            res = self.resample_on_device(lane, buf, offs, lens, fmt, rate)
            if res is not None:
                dbuf, offs, lens = res
            else:
                buf, offs, lens = self.resample_on_host(buf, offs, lens, fmt, rate)
            fmt = _native.FMT_F32
        if dbuf is None:
            dbuf = lane.dev.get(max(buf.nbytes, 16))                  # one PCIe copy for both passes
            try:
                dbuf.upload(buf)
            except BaseException:
                lane.dev.put(dbuf)
                raise
        self.run_passes(lane, cur, dbuf, offs, lens, fmt, tl)

    def run_raw_group(self, lane: _Lane, cur, raw, boffs, frames, kinds, chans, rate: int):
        """One sub-batch of raw WAVE data: one upload of the bytes as they are, conversion and mix-down on the device
        (afx_decode_batch) into a pooled float32 buffer (4-aligned, as _pack) that the passes read -- or, at another rate
        than the extractor's, that the device resampler reads.  Every buffer goes back to its pool on every exit path."""
        tl = [None, len(cur), self.now(), 0.0, 0.0, 0.0]
        sr = int(self.ex.sr)
        offs = _native.packed_offsets(frames, _ALIGN)
        lens = frames
        pool = lane.dev if rate == sr else lane.dev_in
        dbuf = pool.get(max(4 * int(offs[-1] + _padded(frames[-1])), 16))
        try:
            draw = lane.dev_raw.get(max(raw.nbytes, 16))
            try:
                draw.upload(raw)
                lane.plan.decode_batch(draw, boffs, frames, kinds, chans, out=dbuf, out_offsets=offs)
            finally:
                lane.dev_raw.put(draw)                            # the decoder is synchronous: it is done with
            if rate != sr:
                res = self.resample_on_device(lane, None, offs, lens, _native.FMT_F32, rate, din=dbuf) if lane.can_rs else None
                host = None
                if res is None:                                   # no device table: the decoded samples copied back
                    host = np.empty(int(offs[-1] + _padded(frames[-1])), np.float32)
                    dbuf.download(host)
                pool.put(dbuf)
                dbuf = None
                if res is not None:
                    dbuf, offs, lens = res
                else:
                    buf, offs, lens = self.resample_on_host(host, offs, lens, _native.FMT_F32, rate)
                    dbuf = lane.dev.get(max(buf.nbytes, 16))
                    pool = lane.dev
                    dbuf.upload(buf)
        except BaseException:
            if dbuf is not None:
                pool.put(dbuf)
            raise
        self.run_passes(lane, cur, dbuf, offs, lens, _native.FMT_F32, tl)

    def run_passes(self, lane: _Lane, cur, dbuf, offs, lens, fmt, tl):
        """Both passes over the clips of a sub-batch in ``dbuf``, a buffer of lane.dev's that goes back to that pool."""
        try:
            tl[3] = self.now()
            submitted = False
            if self.want_stats:                                   # MFCC / RMS pass: queued, runs beside the pYIN pass below
                lane.plan.extract_submit(dbuf, offs, lens, flags=self.flags, fmt=fmt)
                submitted = True
            out = f0 = None
            try:
                if self.want_f0:
                    f0 = lane.plan_f0.f0_batch(dbuf, offs, lens, self.ex.f0_min, self.ex.f0_max, flags=self.flags, fmt=fmt)
                tl[4] = self.now()
            finally:
                if submitted:                                     # always: the buffer must outlive the queued pass
                    out = lane.plan.extract_collect()
            tl[5] = self.now()
            self.timeline.append(tl)
            self.nsamp[cur] = lens
            if out is not None:
                self.stats[cur] = out["stats"]
                self.nframes[cur] = out["nframes"]
            if f0 is not None:
                self.f0s[cur] = f0["stats"]
            self.f0_done[cur] = True
            # last: a file counts only with every requested pass done.  Without the MFCC / RMS pass the f0 pass's own
            # status (non-finite input) decides
            self.status[cur] = out["status"] if out is not None else f0["status"]
            self.finished.put(list(cur))
        finally:
            lane.dev.put(dbuf)                                    # both passes are through (collect above): reusable

    def count(self, path: str, n: int):
        with self.phase_lock:
            self.ingest[path] += n

    def run_window(self, lane: _Lane, packed, rawpack, rest, decoded):
        """The sub-batches of one loaded window: runs of one file rate and sample type, within the budget before and after
        resampling, counted in mono samples (a window may still exceed the budget: its sizes were estimates)."""
        sr = self.ex.sr
        self.count("python", len(rest))
        if packed is not None:                                    # the natively packed 16-bit clips
            ids, buf, offs, lens, _held, rates = packed
            olens = np.maximum(lens, _native.resample_lengths(lens, rates, sr))
            for pos, end in _budget_runs(olens, self.budget, rates):
                lo = int(offs[pos])
                hi = int(offs[end - 1] + _padded(lens[end - 1]))
                self.count("native_s16", end - pos)
                self.run_group(lane, ids[pos:end], buf[lo:hi], offs[pos:end] - lo, lens[pos:end], _native.FMT_S16,
                               int(rates[pos]))
        if rawpack is not None:                                   # the raw data chunks the device decodes
            ids, raw, boffs, frames, kinds, chans, rates, _held = rawpack
            olens = np.maximum(frames, _native.resample_lengths(frames, rates, sr))
            for pos, end in _budget_runs(olens, self.budget, rates):
                lo = int(boffs[pos])
                hi = int(boffs[end - 1] + _raw_padded(frames[end - 1] * _native.SMP_BYTES[kinds[end - 1]] * chans[end - 1]))
                self.count("native_raw", end - pos)
                self.run_raw_group(lane, ids[pos:end], raw[lo:hi], boffs[pos:end] - lo, frames[pos:end], kinds[pos:end],
                                   chans[pos:end], int(rates[pos]))
        groups = sorted({(d[2] != sr, d[2], d[0] != "s16") for d in decoded if d is not None})
        for _, rate, is_f32 in groups:
            kind, fmt, dt = (("f32", _native.FMT_F32, np.float32) if is_f32 else ("s16", _native.FMT_S16, np.int16))
            sel = [(i, d[1]) for i, d in zip(rest, decoded) if d is not None and d[0] == kind and d[2] == rate]
            osz = [max(y.size, int(_native.resample_lengths(y.size, rate, sr))) for _, y in sel]
            for pos, end in _budget_runs(osz, self.budget):
                buf, offs, lens = _pack([y for _, y in sel[pos:end]], dt)
                self.run_group(lane, [i for i, _ in sel[pos:end]], buf, offs, lens, fmt, int(rate))

    def lane_worker(self, lane_id, idxs):
        """One (device, lane): its files in windows; window k + 1 loads while window k is on the device."""
        wins = _windows(self.sizes, idxs, self.budget)
        try:
            lane = _Lane(self.ex, lane_id, self.want_f0)
        except Exception as e:                                    # no device for this lane: its files are dropped, the batch goes on
            for i in idxs:
                self.errors[i] = e
            return
        load = lambda w: self.win_pool.submit(self.load_window, w, lane.pin, lane.can_rs, lane.can_dec, lane.pin_raw)
        pending = load(wins[0]) if wins else None
        for k, win in enumerate(wins):
            t0 = time.perf_counter()
            packed, rawpack, rest, decoded = pending.result()
            # next window loads while this one is on the device
            pending = load(wins[k + 1]) if k + 1 < len(wins) else None
            t1 = time.perf_counter()
            try:
                self.run_window(lane, packed, rawpack, rest, decoded)
            except Exception as e:          # a device-level failure drops the files of the sub-batch it hit, and the
                for i in win:               # rest of this window; later windows are still attempted
                    if self.errors[i] is None and not (self.status[i] >= 0 and self.f0_done[i]):
                        self.errors[i] = e
                        self.status[i] = -1
            if packed is not None and packed[4] is not None:
                lane.pin.put(packed[4])
            if rawpack is not None and rawpack[7] is not None:
                lane.pin_raw.put(rawpack[7])
            del decoded, packed, rawpack
            with self.phase_lock:
                self.phase["decode_wait"] += t1 - t0
                self.phase["device"] += time.perf_counter() - t1

    def delivered(self, i: int) -> bool:
        # fewer than nine frames fails the MFCC group only (the width-9 delta); extract_energy has its statistics
        st = self.status[i]
        return st == _native.CLIP_OK or ("mfcc" not in self.want and st == _native.CLIP_TOO_SHORT and
                                         self.nsamp[i] >= 2 and self.nframes[i] >= 1)

    def record(self, i: int) -> Dict[str, Any]:
        """The result dict of file i.  With the stock extractor: what _stats_to_dicts / _f0_to_dict build, key for key, in
        plain Python from tolist() rows (cheap enough to run beside the workers); else through the extractor's own."""
        want, rec = self.want, {"file_path": str(self.files[i])}
        if not self.stock:
            mfcc, energy = self.ex._stats_to_dicts(self.stats[i])
            if self.want_f0:
                rec.update(self.ex._f0_to_dict(self.f0s[i]))
            if "mfcc" in want:
                rec.update(mfcc)
            if "energy" in want:
                rec.update(energy)
            return rec
        K, K4, row = self.K, 4 * self.K, self.stats[i].tolist()
        if self.want_f0:
            q = self.f0s[i].tolist()
            rec["f0_mean"], rec["f0_std"], rec["f0_missing_rate"], rec["f0_quality"] = q[0], q[1], q[2], q[3]
        if "mfcc" in want:
            rec["mfcc_mean"], rec["mfcc_std"] = row[0:K], row[K:2 * K]
            rec["mfcc_delta_mean"], rec["mfcc_delta2_mean"] = row[2 * K:3 * K], row[3 * K:K4]
        if "energy" in want:
            rec["energy_mean"], rec["energy_std"], rec["energy_range"] = row[K4], row[K4 + 1], row[K4 + 2]
        return rec

    def drain(self, block: bool) -> bool:
        """Takes one finished sub-batch off the queue and builds its files' dicts; False when there was none."""
        try:
            cur = self.finished.get(timeout=0.002) if block else self.finished.get_nowait()
        except queue.Empty:
            return False
        if self.stock:
            for i in cur:
                if self.errors[i] is None and self.delivered(i):
                    self.recs[i] = self.record(i)
        return True

    def results(self) -> List[Dict[str, Any]]:
        """The dicts of the delivered files in input order; every other file is logged with the reference's messages."""
        out: List[Dict[str, Any]] = []
        for i, f in enumerate(self.files):
            name = getattr(f, "name", str(f))
            err = self.errors[i]
            if err is None and not self.delivered(i):
                err = _status_error(int(self.status[i]), "extract_features", int(self.nframes[i]))
                self.log.error(f"特徵提取失敗: {str(err)}")
            if err is not None:
                self.log.error(f"處理文件 {name} 失敗: {str(err)}")
                continue
            out.append(self.recs[i] if self.recs[i] is not None else self.record(i))
            self.log.info(f"成功處理文件: {name}")
        return out


def process_files(extractor, files: Sequence, max_batch_samples: int = 80 * 1024 * 1024,
                  workers_per_gpu: int = WORKERS_PER_GPU, features_to_extract=None) -> List[Dict[str, Any]]:
    """Shard over GPUs (and over a few workers per GPU) -> per worker a pipeline of bounded windows:
    decode window k + 1 on the shared host pool while window k is packed, uploaded and extracted ->
    dicts in input (glob) order.  Host memory holds at most two windows per worker, not the directory.

    16-bit PCM mono files are read natively and uploaded as int16.  Every other layout the device decoder takes (PCM 8 /
    16 / 24 / 32 bit, float 32 / 64 bit, up to 7 channels) is read natively as raw bytes, uploaded once and converted and
    mixed down on the device (afx_decode_batch, bit for bit wavio.to_float32 + wavio.to_mono) into the buffer the passes --
    or the device resampler -- read; a plan without ``decode_batch`` leaves those files, like files of 8 or more channels
    and other sample widths, to the Python decoder.  LAST_TIMING["ingest"] counts the files by the path that took them.

    Files at another sample rate than the extractor's are resampled on the device (afx_resample_batch, the arithmetic of
    wavio.resample): 16-bit PCM mono ones are read natively like the rest and uploaded as int16, files Python decodes are
    uploaded as float32 at their own rate; a sub-batch holds one file rate, its resampled clips go to a second pooled device
    buffer (4-aligned, as _pack) that both passes read.  Sub-batches are cut so that neither their input nor their
    resampled samples exceed ``max_batch_samples``.  A plan without ``resample_batch``, or a rate pair the device
    resampler does not hold (NotImplementedError), leaves those files to wavio.resample on the host.

    On the device a worker owns two plans (own stream each): the MFCC / RMS pass of a sub-batch is queued with
    afx_extract_submit on the first and collected only after the pYIN pass of the same sub-batch (afx_f0_batch, second
    plan) has run beside it -- one upload serves both.  ``features_to_extract`` (README.md:141-146) leaves out the passes
    nobody asked for: without 'f0' no pYIN pass runs (it is ~30x the MFCC pass).

    Error behaviour is the reference's (feature_extractor.py:229-235): a file that cannot be loaded, a clip the
    kernels reject, or a device-level failure while its window is processed is logged and left out; the batch goes on."""
    if len(files) == 0:
        return []
    job = _Job(extractor, files, max_batch_samples, workers_per_gpu, features_to_extract)
    threads = [threading.Thread(target=job.lane_worker, args=(ln, p)) for ln, p in zip(job.lanes, job.parts) if p]
    # The calling thread builds the result dicts of finished sub-batches while the workers drive the device (55 Python floats
    # and four lists per file: 35-50 ms for 8192 files if left to the end).  The workers need the interpreter only for
    # microseconds between two native calls, but would wait a whole switch interval (5 ms) for it: shortened for the duration.
    _fast_switch(True)
    try:
        for t in threads:
            t.start()
        while any(t.is_alive() for t in threads):
            job.drain(True)
        while job.drain(False):
            pass
        for t in threads:
            t.join()
    finally:
        _fast_switch(False)
    job.win_pool.shutdown()
    job.pool.shutdown()

    t_gpu = time.perf_counter()
    results = job.results()
    LAST_TIMING.update(pipeline=t_gpu - job.t_start, decode_wait=job.phase["decode_wait"], device=job.phase["device"],
                       dicts=time.perf_counter() - t_gpu, files=len(files), workers=len(threads), ingest=dict(job.ingest),
                       timeline=sorted(job.timeline, key=lambda r: r[2]))
    return results
