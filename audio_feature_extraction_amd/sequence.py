"""``librosa.sequence.dtw`` on the GPU: the alignment step the reference's aligner runs on pairs of MFCC frame matrices
(05_dtw_alignment_experiment/dtw_alignment.py:930-970, :1092-1130).

Semantics are librosa 0.11's defaults: step sizes (1,1), (0,1), (1,0) with unit weights, the first minimum winning a tie,
``global_constraints`` as ``fill_off_diagonal`` with radius ``round(band_rad * min(N, M))``, the path returned end to start.
The local cost is scipy ``cdist``'s metric evaluated in float32 from direct differences; the accumulation is float64.
The DP and the back-track run in ``libafx.so`` (``afx_dtw_batch``); there is no CPU fallback.
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


def _status_error(status: int) -> ValueError:
    if status == _native.DTW_NONFINITE:
        return ValueError("DTW cost matrix C has NaN values (non-finite features, or a zero-norm frame under cosine)")
    if status == _native.DTW_NO_PATH:
        return ValueError("No valid DTW path: the global constraint band admits none")
    return ValueError(f"DTW pair status {status}")


def _run(pairs: Sequence[Tuple[np.ndarray, np.ndarray]], metric: str, global_constraints: bool, band_rad: float,
         backtrack: bool, store_d: bool, device: int) -> dict:
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
    return _context(device).dtw_batch(feats.reshape(-1, dim), xo, xl, yo, yl, band, metric, backtrack, store_d)


def dtw(X, Y, *, metric: str = "euclidean", global_constraints: bool = False, band_rad: float = 0.25,
        backtrack: bool = True, return_cost_matrix: bool = False, device: int = 0):
    """``librosa.sequence.dtw(X, Y, metric=..., global_constraints=..., band_rad=..., backtrack=...)``.

    X (dim, N) and Y (dim, M) are features x frames (1-D inputs are one feature).  Returns ``(cost, wp)``: the total
    alignment cost D[N-1, M-1] and the warping path as an (L, 2) int array from (N-1, M-1) to (0, 0); with
    ``return_cost_matrix`` the accumulated cost matrix D (N, M float64, inf outside the band) takes the cost's place, and
    with ``backtrack=False`` only the first item is returned.  Raises ValueError on bad shapes (before any device work),
    on non-finite features and when the band admits no path."""
    X, Y = _check_pair(X, Y, metric)
    out = _run([(X, Y)], metric, global_constraints, band_rad, backtrack, return_cost_matrix, device)
    st = int(out["status"][0])
    if st != _native.DTW_OK:
        raise _status_error(st)
    first = out["D"][0] if return_cost_matrix else float(out["cost"][0])
    if not backtrack:
        return first
    return first, out["paths"][0]


def dtw_batch(pairs: Sequence[Tuple[Any, Any]], *, metric: str = "euclidean", global_constraints: bool = False,
              band_rad: float = 0.25, backtrack: bool = True, return_cost_matrix: bool = False,
              device: int = 0) -> List[Optional[Any]]:
    """:func:`dtw` of many (X, Y) pairs in one device pass.  Returns a list aligned with ``pairs``: each entry is what
    :func:`dtw` would return, or None for a pair that fails (bad shape, non-finite features, no path), which is logged
    with its reason -- as ``batch_process`` logs and skips a failing file."""
    good, idx, result = [], [], [None] * len(pairs)
    dim = None
    for p, (X, Y) in enumerate(pairs):
        try:
            X, Y = _check_pair(X, Y, metric)
            if dim is None:
                dim = X.shape[0]
            elif X.shape[0] != dim:
                raise ValueError(f"feature dimension {X.shape[0]} differs from the batch's {dim}")
        except ValueError as e:
            logger.error(f"DTW pair {p} skipped: {e}")
            continue
        good.append((X, Y))
        idx.append(p)
    if not good:
        return result
    out = _run(good, metric, global_constraints, band_rad, backtrack, return_cost_matrix, device)
    for q, p in enumerate(idx):
        st = int(out["status"][q])
        if st != _native.DTW_OK:
            logger.error(f"DTW pair {p} skipped: {_status_error(st)}")
            continue
        first = out["D"][q] if return_cost_matrix else float(out["cost"][q])
        result[p] = (first, out["paths"][q]) if backtrack else first
    return result
