"""``librosa.sequence.dtw`` on the GPU: the alignment step the reference's aligner runs on pairs of MFCC frame matrices
(05_dtw_alignment_experiment/dtw_alignment.py:930-970, :1092-1130).

Semantics are librosa 0.11's: step sizes (1,1), (0,1), (1,0) with unit weights by default, the first minimum winning a tie,
``global_constraints`` as ``fill_off_diagonal`` with radius ``round(band_rad * min(N, M))``, the path returned end to start.
The local cost is scipy ``cdist``'s metric evaluated in float32 from direct differences; the accumulation is float64.
``step_sizes_sigma``, ``weights_add``, ``weights_mul`` and ``subseq`` are librosa's too: up to five custom steps with
components 0 .. 2, one weight pair per step, and the match of X inside a longer Y.  Not taken: a precomputed ``C`` and
``return_steps``.
The DP and the back-track run in ``libafx.so`` (``afx_dtw_batch`` for a call at the defaults, ``afx_dtw_steps_batch``
otherwise); there is no CPU fallback.
"""
from __future__ import annotations

import logging
from typing import Any, List, Optional, Sequence, Tuple

import numpy as np

from . import _native

logger = logging.getLogger(__name__)

_contexts: dict = {}


def _context(device: int) -> _native.Context:
    ctx = _contexts.get(device)
    if ctx is None:
        ctx = _contexts[device] = _native.Context(device)
    return ctx


def _as_seq(a, name: str) -> np.ndarray:
    a = np.atleast_2d(np.asarray(a))
    if a.ndim != 2:
        raise ValueError(f"{name} must be 1-D or 2-D (features x frames), got shape {a.shape}")
    if a.shape[1] < 1 or a.shape[0] < 1:
        raise ValueError(f"{name} is empty: shape {a.shape}")
    return a


def _check_pair(X, Y, metric: str) -> Tuple[np.ndarray, np.ndarray]:
    X, Y = _as_seq(X, "X"), _as_seq(Y, "Y")
    if X.shape[0] != Y.shape[0]:
        raise ValueError(f"X and Y must have the same feature dimension: {X.shape[0]} != {Y.shape[0]}")
    if X.shape[0] > _native.DTW_MAX_DIM:
        raise ValueError(f"feature dimension {X.shape[0]} > {_native.DTW_MAX_DIM} is not supported")
    if X.shape[1] * Y.shape[1] > 2 ** 31:
        raise ValueError(f"{X.shape[1]} x {Y.shape[1]} cells exceed the 2^31 supported")
    if metric not in _native.DTW_METRICS:
        raise ValueError(f"unsupported metric {metric!r} ({', '.join(_native.DTW_METRICS)})")
    return X, Y


def band_radius(n: int, m: int, band_rad: float) -> int:
    """librosa's ``fill_off_diagonal`` radius: ``round(band_rad * min(n, m))`` (numpy rounds half to even)."""
    return int(np.round(band_rad * min(n, m)))


def _status_error(status: int, general=None) -> ValueError:
    if status == _native.DTW_NONFINITE:
        return ValueError("DTW cost matrix C has NaN values (non-finite features, or a zero-norm frame under cosine)")
    if status == _native.DTW_NO_PATH:
        if general is not None:
            return ValueError("No valid DTW path: the step sizes (or the global constraint band) admit none")
        return ValueError("No valid DTW path: the global constraint band admits none")
    return ValueError(f"DTW pair status {status}")


def _step_args(step_sizes_sigma, weights_add, weights_mul, subseq):
    """The four step arguments, checked before any native call.  None when all are at their defaults (the call then takes
    the default-step path); otherwise (steps [k, 2] int32 or None, weights_add, weights_mul, subseq)."""
    if step_sizes_sigma is None and weights_add is None and weights_mul is None and not subseq:
        return None
    steps = None
    k = 3
    if step_sizes_sigma is not None:
        raw = np.asarray(step_sizes_sigma)
        if raw.ndim != 2 or raw.shape[1] != 2 or raw.shape[0] < 1:
            raise ValueError(f"step_sizes_sigma must be a non-empty list of (di, dj) pairs, got shape {raw.shape}")
        if not np.issubdtype(raw.dtype, np.integer):
            if not (np.issubdtype(raw.dtype, np.floating) and np.all(np.isfinite(raw)) and np.all(raw == np.round(raw))):
                raise ValueError("step_sizes_sigma must hold integers")
        steps = raw.astype(np.int64)
        if (steps < 0).any():
            raise ValueError("step_sizes_sigma: a step component is negative")
        if (steps == 0).all(axis=1).any():
            raise ValueError("step_sizes_sigma: (0, 0) is not a step")
        if steps.shape[0] > _native.DTW_MAX_STEPS:
            raise NotImplementedError(f"more than {_native.DTW_MAX_STEPS} custom steps are not supported")
        if (steps > _native.DTW_MAX_STEP).any():
            raise NotImplementedError(f"step components above {_native.DTW_MAX_STEP} are not supported")
        steps = np.ascontiguousarray(steps, np.int32)
        k = int(steps.shape[0])
    weights = []
    for name, w in (("weights_add", weights_add), ("weights_mul", weights_mul)):
        if w is not None:
            w = np.asarray(w, np.float64).reshape(-1)
            if w.shape[0] != k:
                raise ValueError(f"{name} has {w.shape[0]} entries for {k} steps")
            if not np.all(np.isfinite(w)) or (w < 0).any():
                raise ValueError(f"{name} must be finite and non-negative")
        weights.append(w)
    return steps, weights[0], weights[1], bool(subseq)


def _orient(X: np.ndarray, Y: np.ndarray, general) -> Tuple[np.ndarray, np.ndarray, bool]:
    """librosa's orientation rules for a call with step arguments: under ``subseq`` the shorter sequence is matched inside
    the longer (C = C.T when N > M), and the step list [(1,1)] alone cannot align more rows than columns."""
    swap = general[3] and X.shape[1] > Y.shape[1]
    if swap:
        X, Y = Y, X
    st = general[0]
    if st is not None and st.shape[0] == 1 and tuple(st[0]) == (1, 1) and X.shape[1] > Y.shape[1]:
        raise ValueError("For diagonal matching: Y.shape[-1] >= X.shape[-1] is required "
                         f"(N = {X.shape[1]}, M = {Y.shape[1]})")
    return X, Y, swap


def _unswap(first, wp, swap: bool, return_cost_matrix: bool):
    if swap:
        if return_cost_matrix:
            first = np.ascontiguousarray(first.T)
        if wp is not None:
            wp = np.ascontiguousarray(wp[:, ::-1])
    return first, wp


def _run(pairs: Sequence[Tuple[np.ndarray, np.ndarray]], metric: str, global_constraints: bool, band_rad: float,
         backtrack: bool, store_d: bool, device: int, general=None) -> dict:
    dim = pairs[0][0].shape[0]
    # X and Y of every pair go into one frame-major buffer; an array object used in several pairs is uploaded once
    chunks, where, total = [], {}, 0

    def place(a: np.ndarray) -> int:
        nonlocal total
        key = id(a)
        if key not in where:
            where[key] = total
            chunks.append(np.ascontiguousarray(a.T, np.float32))
            total += a.shape[1]
        return where[key]

    xo = np.array([place(X) for X, _ in pairs], np.int64)
    yo = np.array([place(Y) for _, Y in pairs], np.int64)
    xl = np.array([X.shape[1] for X, _ in pairs], np.int64)
    yl = np.array([Y.shape[1] for _, Y in pairs], np.int64)
    feats = np.concatenate(chunks, axis=0) if len(chunks) > 1 else chunks[0]
    band = None
    if global_constraints:
        band = np.array([band_radius(int(n), int(m), band_rad) for n, m in zip(xl, yl)], np.int32)
    if general is None:
        return _context(device).dtw_batch(feats.reshape(-1, dim), xo, xl, yo, yl, band, metric, backtrack, store_d)
    steps, wa, wm, subseq = general
    return _context(device).dtw_steps_batch(feats.reshape(-1, dim), xo, xl, yo, yl, band, metric, backtrack, store_d,
                                            steps, wa, wm, subseq)


def dtw(X, Y, *, metric: str = "euclidean", step_sizes_sigma=None, weights_add=None, weights_mul=None,
        subseq: bool = False, global_constraints: bool = False, band_rad: float = 0.25,
        backtrack: bool = True, return_cost_matrix: bool = False, device: int = 0):
    """``librosa.sequence.dtw(X, Y, metric=..., step_sizes_sigma=..., weights_add=..., weights_mul=..., subseq=...,
    global_constraints=..., band_rad=..., backtrack=...)``.

    X (dim, N) and Y (dim, M) are features x frames (1-D inputs are one feature).  Returns ``(cost, wp)``: the total
    alignment cost D[N-1, M-1] and the warping path as an (L, 2) int array from (N-1, M-1) to (0, 0); with
    ``return_cost_matrix`` the accumulated cost matrix D (N, M float64, inf outside the band) takes the cost's place, and
    with ``backtrack=False`` only the first item is returned.  Raises ValueError on bad shapes (before any device work),
    on non-finite features and when the band admits no path.

    ``step_sizes_sigma`` (up to five (di, dj) steps, components 0 .. 2), ``weights_add`` / ``weights_mul`` (one value per
    step; three for the default steps) and ``subseq`` follow librosa: a custom list is searched behind the three default
    steps, whose weights are inf; a candidate is ``D[i-di, j-dj] + (weights_mul * C[i, j] + weights_add)``; under
    ``subseq`` X may start and end anywhere in Y (the roles are swapped when N > M, and the path and D are returned in
    the caller's orientation), the cost is the minimum of D's last row and the path runs from there to row 0.  A call that
    leaves the four at their defaults is the default-step path, bit for bit.  Step lists and weights outside those limits
    raise NotImplementedError (too many steps, a component above 2) or ValueError before any device work."""
    general = _step_args(step_sizes_sigma, weights_add, weights_mul, subseq)
    X, Y = _check_pair(X, Y, metric)
    swap = False
    if general is not None:
        X, Y, swap = _orient(X, Y, general)
    out = _run([(X, Y)], metric, global_constraints, band_rad, backtrack, return_cost_matrix, device, general)
    st = int(out["status"][0])
    if st != _native.DTW_OK:
        raise _status_error(st, general)
    first = out["D"][0] if return_cost_matrix else float(out["cost"][0])
    first, wp = _unswap(first, out["paths"][0] if backtrack else None, swap, return_cost_matrix)
    if not backtrack:
        return first
    return first, wp


def dtw_batch(pairs: Sequence[Tuple[Any, Any]], *, metric: str = "euclidean", step_sizes_sigma=None, weights_add=None,
              weights_mul=None, subseq: bool = False, global_constraints: bool = False,
              band_rad: float = 0.25, backtrack: bool = True, return_cost_matrix: bool = False,
              device: int = 0) -> List[Optional[Any]]:
    """:func:`dtw` of many (X, Y) pairs in one device pass.  Returns a list aligned with ``pairs``: each entry is what
    :func:`dtw` would return, or None for a pair that fails (bad shape, non-finite features, no path), which is logged
    with its reason -- as ``batch_process`` logs and skips a failing file.  The step arguments hold for every pair; a bad
    one raises before any device work, as in :func:`dtw`."""
    general = _step_args(step_sizes_sigma, weights_add, weights_mul, subseq)
    good, idx, swaps, result = [], [], [], [None] * len(pairs)
    dim = None
    for p, (X, Y) in enumerate(pairs):
        try:
            X, Y = _check_pair(X, Y, metric)
            if dim is None:
                dim = X.shape[0]
            elif X.shape[0] != dim:
                raise ValueError(f"feature dimension {X.shape[0]} differs from the batch's {dim}")
            swap = False
            if general is not None:
                X, Y, swap = _orient(X, Y, general)
        except ValueError as e:
            logger.error(f"DTW pair {p} skipped: {e}")
            continue
        good.append((X, Y))
        idx.append(p)
        swaps.append(swap)
    if not good:
        return result
    out = _run(good, metric, global_constraints, band_rad, backtrack, return_cost_matrix, device, general)
    for q, p in enumerate(idx):
        st = int(out["status"][q])
        if st != _native.DTW_OK:
            logger.error(f"DTW pair {p} skipped: {_status_error(st, general)}")
            continue
        first = out["D"][q] if return_cost_matrix else float(out["cost"][q])
        first, wp = _unswap(first, out["paths"][q] if backtrack else None, swaps[q], return_cost_matrix)
        result[p] = (first, wp) if backtrack else first
    return result
