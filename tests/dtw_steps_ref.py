"""float64 oracle of ``librosa.sequence.dtw`` with ``step_sizes_sigma``, ``weights_add``, ``weights_mul`` and ``subseq``
(librosa 0.11 is not installed; the rules below restate it, and this file is the spec of ``sequence.dtw``'s step arguments).

1. Step list.  DEFAULT = [(1,1), (0,1), (1,0)].  Without ``step_sizes_sigma`` the list is DEFAULT with weights zeros(3) /
   ones(3) unless given.  With it the list is DEFAULT + custom, the caller's weights behind three inf entries: the defaults
   never win (inf * 0 is NaN, and a NaN candidate never compares smaller), but the step indices keep the offset 3.
2. C = cdist(X.T, Y.T, metric), N x M.  Under ``subseq`` with N > M the roles are swapped (C = C.T); afterwards the path's
   columns are flipped back and D is transposed back.
3. A custom list that is exactly [[1,1]] raises ValueError when C has more rows than columns after rule 2.
4. A NaN in C (a non-finite feature, a zero-norm frame under cosine): status NONFINITE.
5. ``global_constraints`` puts inf outside the band of the (possibly swapped) C: ``tests/dtw_ref.band_mask``.
6. Every cell starts at its seed -- C[0,0] at (0,0), C[0,j] on row 0 under ``subseq``, inf elsewhere -- and then, for each
   step k in list order, cand = D[i-di, j-dj] + (wm[k] * C[i,j] + wa[k]) (a predecessor outside the matrix is inf)
   replaces D[i,j] and the recorded step only when cand < D[i,j]: the first minimum wins.  Row 0 goes through the same rule.
7. The end cell is (N-1, M-1), or under ``subseq`` (N-1, j*) with j* the first argmin of D[N-1, :]; status NO_PATH when
   that cell (the whole last row) is inf.  The cost is D at the end cell.
8. The path starts at the end cell, subtracts the recorded step, and stops at (0,0) -- under ``subseq`` at the first cell
   with i == 0.  It is returned end to start.

Two forms: ``dtw_loop`` is the literal per-cell loop, ``dtw_vec`` walks anti-diagonals with numpy (every step reaches a
smaller i + j, so the cells of one anti-diagonal are independent).  Both return (D, steps, cost, end, wp, status) for a
cost matrix; ``dtw`` applies rules 1-3 to (X, Y) and returns (D, wp, cost, end, status) in the caller's orientation, with
``end`` the column j* of the matrix the DP ran on."""
from __future__ import annotations

import numpy as np

from tests import dtw_ref as R

OK, NONFINITE, NO_PATH = R.OK, R.NONFINITE, R.NO_PATH
DEFAULT = ((1, 1), (0, 1), (1, 0))


def step_table(step_sizes_sigma=None, weights_add=None, weights_mul=None):
    """Rule 1: (S [k, 2] int, wa [k], wm [k])."""
    if step_sizes_sigma is None:
        S = np.array(DEFAULT, np.int64)
        wa = np.zeros(3) if weights_add is None else np.asarray(weights_add, np.float64)
        wm = np.ones(3) if weights_mul is None else np.asarray(weights_mul, np.float64)
    else:
        custom = np.asarray(step_sizes_sigma, np.int64).reshape(-1, 2)
        k = custom.shape[0]
        wa = np.zeros(k) if weights_add is None else np.asarray(weights_add, np.float64)
        wm = np.ones(k) if weights_mul is None else np.asarray(weights_mul, np.float64)
        S = np.concatenate([np.array(DEFAULT, np.int64), custom])
        wa = np.concatenate([np.full(3, np.inf), wa])
        wm = np.concatenate([np.full(3, np.inf), wm])
    assert wa.shape == wm.shape == (S.shape[0],), "one weight per step"
    return S, wa, wm


def backtrack(steps: np.ndarray, S: np.ndarray, end: int, subseq: bool) -> np.ndarray:
    i, j = steps.shape[0] - 1, int(end)
    wp = [(i, j)]
    while (i != 0) if subseq else ((i, j) != (0, 0)):
        di, dj = S[steps[i, j]]
        i, j = i - int(di), j - int(dj)
        assert i >= 0 and j >= 0
        wp.append((i, j))
    return np.asarray(wp, np.int64)


def _finish(C, D, steps, S, subseq):
    if np.isnan(C).any():
        return None, None, np.nan, -1, None, NONFINITE
    end = int(np.argmin(D[-1])) if subseq else D.shape[1] - 1
    cost = D[-1, end]
    if np.isinf(cost):
        return D, steps, cost, end, None, NO_PATH
    return D, steps, cost, end, backtrack(steps, S, end, subseq), OK


def dtw_loop(C: np.ndarray, S, wa, wm, subseq: bool = False):
    n, m = C.shape
    D = np.full((n, m), np.inf)
    steps = np.zeros((n, m), np.int8)
    D[0, 0] = C[0, 0]
    if subseq:
        D[0, :] = C[0, :]
    with np.errstate(invalid="ignore"):
        for i in range(n):
            for j in range(m):
                for k in range(S.shape[0]):
                    pi, pj = i - S[k, 0], j - S[k, 1]
                    prev = D[pi, pj] if pi >= 0 and pj >= 0 else np.inf
                    w = wm[k] * C[i, j]
                    cand = prev + (w + wa[k])
                    if cand < D[i, j]:
                        D[i, j], steps[i, j] = cand, k
    return _finish(C, D, steps, S, subseq)


def dtw_vec(C: np.ndarray, S, wa, wm, subseq: bool = False):
    n, m = C.shape
    if np.isnan(C).any():
        return _finish(C, None, None, S, subseq)
    P = np.full((n + 2, m + 2), np.inf)      # P[i+2, j+2] = D[i, j]; the two leading rows / columns are "outside"
    steps = np.zeros((n, m), np.int8)
    P[2, 2] = C[0, 0]
    if subseq:
        P[2, 2:] = C[0, :]
    with np.errstate(invalid="ignore"):
        for a in range(n + m - 1):
            i = np.arange(max(0, a - m + 1), min(n, a + 1))
            j = a - i
            c = C[i, j]
            best = P[i + 2, j + 2].copy()
            code = np.zeros(i.size, np.int8)
            for k in range(S.shape[0]):
                w = wm[k] * c
                cand = P[i + 2 - S[k, 0], j + 2 - S[k, 1]] + (w + wa[k])
                win = cand < best                # strict, in list order: the first minimum wins
                best = np.where(win, cand, best)
                code = np.where(win, k, code).astype(np.int8)
            P[i + 2, j + 2] = best
            steps[i, j] = code
    return _finish(C, P[2:, 2:].copy(), steps, S, subseq)


def dtw(X, Y, metric="euclidean", step_sizes_sigma=None, weights_add=None, weights_mul=None, subseq=False,
        global_constraints=False, band_rad=0.25, vectorised=True):
    """Rules 1-8 on (X, Y): returns (D, wp, cost, end, status); D and wp in the caller's orientation."""
    S, wa, wm = step_table(step_sizes_sigma, weights_add, weights_mul)
    X = np.atleast_2d(np.asarray(X, np.float64))
    Y = np.atleast_2d(np.asarray(Y, np.float64))
    swap = bool(subseq) and X.shape[1] > Y.shape[1]
    if swap:
        X, Y = Y, X
    n, m = X.shape[1], Y.shape[1]
    if step_sizes_sigma is not None and np.array_equal(np.asarray(step_sizes_sigma), [[1, 1]]) and n > m:
        raise ValueError("For diagonal matching: Y.shape[-1] >= X.shape[-1] is required")
    r = R.band_radius(n, m, band_rad) if global_constraints else None
    C = R.local_cost(X, Y, metric, r)
    D, steps, cost, end, wp, status = (dtw_vec if vectorised else dtw_loop)(C, S, wa, wm, bool(subseq))
    if swap:
        D = None if D is None else np.ascontiguousarray(D.T)
        wp = None if wp is None else np.ascontiguousarray(wp[:, ::-1])
    return D, wp, cost, end, status


def path_cost(C: np.ndarray, wp: np.ndarray, S, wa, wm) -> float:
    """The cost of walking wp (end to start) on C: the seed C[wp[-1]] plus wm[k] * C[cell] + wa[k] per step taken, k the
    first finite-weight entry of the list with that (di, dj).  Under ``subseq`` this equals D at the end cell only when
    the path's row-0 cell kept its seed, which holds whenever every step with di == 0 has wm >= 1: rule 6 lets such a step
    lower a row-0 cell below its seed otherwise, and rule 8 still stops the path there."""
    total = float(C[wp[-1, 0], wp[-1, 1]])
    for t in range(len(wp) - 2, -1, -1):
        d = wp[t] - wp[t + 1]
        ks = [k for k in range(S.shape[0]) if tuple(S[k]) == tuple(d) and np.isfinite(wm[k])]
        assert ks, ("step not in the list", tuple(d))
        k = ks[0]
        total += wm[k] * float(C[wp[t, 0], wp[t, 1]]) + wa[k]
    return total


def check_path(wp: np.ndarray, n: int, m: int, S, wm, subseq: bool, end=None, mask=None) -> None:
    """wp is a valid path end to start on an n x m matrix: rule 8's end points, every step one of the list's live steps,
    every cell allowed."""
    assert wp[0, 0] == n - 1 and (wp[0, 1] == (m - 1 if end is None else end)), wp[0]
    if subseq:
        assert wp[-1, 0] == 0 and (wp[:-1, 0] > 0).all(), wp[-1]
    else:
        assert tuple(wp[-1]) == (0, 0), wp[-1]
    live = {tuple(S[k]) for k in range(S.shape[0]) if np.isfinite(wm[k])}
    d = wp[:-1] - wp[1:]
    bad = [t for t in range(len(d)) if tuple(d[t]) not in live]
    assert not bad, (bad[:5], d[bad[:5]])
    assert (wp >= 0).all() and (wp[:, 0] < n).all() and (wp[:, 1] < m).all()
    if mask is not None:
        assert mask[wp[:, 0], wp[:, 1]].all()
