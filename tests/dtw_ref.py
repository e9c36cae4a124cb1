"""float64 oracle of ``librosa.sequence.dtw`` at its defaults (librosa 0.11 is not installed; the rules below restate it).

C is scipy's ``cdist`` of the frames (librosa calls it), the band is ``fill_off_diagonal``, and D accumulates the three
candidate sums in the order diagonal, (0, 1), (1, 0) with the first minimum winning.  Two forms: ``dtw_loop`` is the
literal per-cell loop, ``dtw_vec`` walks anti-diagonals with numpy for big pairs.  Both return (D, steps, cost, wp,
status) with status 0 ok, 1 non-finite, 2 no path (the afx_dtw_status codes)."""
from __future__ import annotations

import numpy as np
from scipy.spatial.distance import cdist

OK, NONFINITE, NO_PATH = 0, 1, 2


def band_radius(n: int, m: int, band_rad: float) -> int:
    return int(np.round(band_rad * min(n, m)))


def band_mask(n: int, m: int, r) -> np.ndarray:
    """True where cell (i, j) is allowed: -r - (off if n >= m) < j - i < r + (off if n < m); r None: everywhere."""
    if r is None:
        return np.ones((n, m), bool)
    off = abs(n - m)
    lo = -r - (off if n >= m else 0)
    hi = r + (off if n < m else 0)
    d = np.arange(m)[None, :] - np.arange(n)[:, None]
    return (d > lo) & (d < hi)


def local_cost(X, Y, metric: str = "euclidean", r=None) -> np.ndarray:
    X = np.atleast_2d(np.asarray(X, np.float64))
    Y = np.atleast_2d(np.asarray(Y, np.float64))
    C = cdist(X.T, Y.T, metric=metric)
    C[~band_mask(C.shape[0], C.shape[1], r)] = np.inf
    return C


def backtrack(steps: np.ndarray) -> np.ndarray:
    i, j = steps.shape[0] - 1, steps.shape[1] - 1
    wp = [(i, j)]
    while (i, j) != (0, 0):
        s = steps[i, j]
        if s == 0:
            i, j = i - 1, j - 1
        elif s == 1:
            j -= 1
        else:
            i -= 1
        wp.append((i, j))
    return np.asarray(wp, np.int64)


def _finish(C, D, steps):
    if np.isnan(C).any():
        return None, None, np.nan, None, NONFINITE
    cost = D[-1, -1]
    if np.isinf(cost):
        return D, steps, cost, None, NO_PATH
    return D, steps, cost, backtrack(steps), OK


def dtw_loop(C: np.ndarray):
    n, m = C.shape
    D = np.full((n, m), np.inf)
    steps = np.zeros((n, m), np.int8)
    for i in range(n):
        for j in range(m):
            if i == 0 and j == 0:
                D[0, 0] = C[0, 0]
                continue
            best, code = np.inf, 0
            for k, (di, dj) in enumerate(((1, 1), (0, 1), (1, 0))):
                pi, pj = i - di, j - dj
                prev = D[pi, pj] if pi >= 0 and pj >= 0 else np.inf
                s = prev + C[i, j]
                if s < best:
                    best, code = s, k
            D[i, j], steps[i, j] = best, code
    return _finish(C, D, steps)


def dtw_vec(C: np.ndarray):
    n, m = C.shape
    if np.isnan(C).any():
        return _finish(C, None, None)
    P = np.full((n + 1, m + 1), np.inf)      # P[i+1, j+1] = D[i, j]
    steps = np.zeros((n, m), np.int8)
    P[1, 1] = C[0, 0]
    for a in range(1, n + m - 1):
        i = np.arange(max(0, a - m + 1), min(n, a + 1))
        j = a - i
        c = C[i, j]
        cand = np.stack([P[i, j] + c, P[i + 1, j] + c, P[i, j + 1] + c])
        k = np.argmin(cand, axis=0)            # the first minimum wins, as the loop's strict <
        best = cand[k, np.arange(i.size)]
        allinf = np.isinf(cand).all(axis=0)
        k[allinf] = 0
        P[i + 1, j + 1] = best
        steps[i, j] = k
    return _finish(C, P[1:, 1:].copy(), steps)


def dtw(X, Y, metric="euclidean", global_constraints=False, band_rad=0.25, vectorised=True):
    X = np.atleast_2d(np.asarray(X, np.float64))
    Y = np.atleast_2d(np.asarray(Y, np.float64))
    r = band_radius(X.shape[1], Y.shape[1], band_rad) if global_constraints else None
    C = local_cost(X, Y, metric, r)
    return (dtw_vec if vectorised else dtw_loop)(C)


def path_cost(C: np.ndarray, wp: np.ndarray) -> float:
    return float(np.sum(C[wp[:, 0], wp[:, 1]]))


def check_path(wp: np.ndarray, n: int, m: int, mask=None) -> None:
    """wp is a valid DTW path end to start: the endpoints, unit steps, every cell allowed."""
    assert tuple(wp[0]) == (n - 1, m - 1) and tuple(wp[-1]) == (0, 0), (wp[0], wp[-1])
    d = wp[:-1] - wp[1:]
    ok = ((d == (1, 1)).all(1) | (d == (0, 1)).all(1) | (d == (1, 0)).all(1))
    assert ok.all(), np.nonzero(~ok)[0][:5]
    if mask is not None:
        assert mask[wp[:, 0], wp[:, 1]].all()
