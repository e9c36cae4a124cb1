"""A per-cell certificate of a DTW result: float64 numpy, for the D and the path a device returns for (X, Y).

The device is given no cost matrix: it forms the local cost of every cell in float32 from X and Y (``dtw_local_cost`` and
``k_dtw_norms``), widens it to float64 and accumulates D in float64.  ``certify`` therefore checks every cell against the
device's *own* D at the cell's predecessors: the error it allows is that of one float32 local cost, local to the cell and
never accumulated along a path.  What it asserts (the letters are those of the messages):

a. reachability: ``isinf(D)`` is exactly the oracle's (``dtw_ref.dtw_vec`` / ``dtw_steps_ref.dtw_vec`` on the float64 C);
b. start cells: D[0, 0] -- under ``subseq`` all of row 0 -- lies within C +- T;
c. every other finite cell: with pred_k the cell one step k back,
   ``lo = min_k(D[pred_k] + (wm_k (C - T) + wa_k))``, ``hi`` the same with C + T, and
   ``lo (1 - 4 * 2^-53) <= D[i, j] <= hi (1 + 4 * 2^-53)``.  (Row 0 under ``subseq`` goes through the same minimum with its
   seed C +- T as one more candidate; with every D >= 0 and wm >= 1 on the steps that stay on a row that is (b).)
   Where C == 0 under the two Euclidean metrics T is 0 and the cell must equal ``min_k(D[pred_k] + wa_k)`` bit for bit;
d. the path is a back-track of that D: it starts at (N-1, M-1) -- under ``subseq`` at the first minimum of D[N-1, :] --,
   stops at (0, 0) -- at its first cell of row 0 --, takes only steps of the list, and at every cell the step taken is
   the first minimum of the device's predecessor values in list order when the steps share one weight pair (no
   tolerance: see ``_first_minimum``), and otherwise satisfies the interval of (c) for its own k;
e. the cost is D at the path's first cell bit for bit, with and without back-tracking, and lies within
   ``[ref - sum_dev, ref + sum_ref]``: ``sum_ref`` / ``sum_dev`` are the sums of wm_k T over the oracle's / the device's path.
   (The device's cost is a minimum over paths of sums of device costs, each within T of C: it is at most the oracle's path
   walked on the device's costs, and the oracle's cost is at most the device's path walked on C.)

The tolerance T of one local cost.  u = 2^-24 is the unit roundoff of float32, DIMP the compiled width that serves ``dim``
(8, 16, 24, 40, 64, 128; the padding is zeros, whose terms are exact).  All device operations are correctly rounded
(fused multiply-add, add, sqrt, divide), so each contributes a factor (1 + d), abs(d) <= u.

* ``sqeuclidean``: T = (DIMP / 2 + 4) u C.  A difference fl(x - y) carries one rounding, its square two: 2 u.  The squares go
  into two accumulators by fused multiply-add, DIMP / 2 terms each, so a term sees at most DIMP / 2 roundings on its way:
  (DIMP / 2) u.  The sum of the two accumulators rounds once more: u.  Every term is >= 0, so the relative errors do not
  amplify: (DIMP / 2 + 3) u in first order, and the fourth u holds the second-order terms ((1 + u)^67 - 1 < 67.001 u).
* ``euclidean``: T = (DIMP / 4 + 3) u C.  The square root halves the relative error of its argument, (DIMP / 4 + 1.5) u,
  and rounds once: (DIMP / 4 + 2.5) u; half a u is left for the second order.
* ``cosine``: T = (1.5 DIMP + 6) u, absolute.  The dot product, two accumulators of DIMP / 2 fused terms and their sum,
  is off by at most (DIMP / 2 + 1) u sum(abs(x y)) <= (DIMP / 2 + 1) u |x| |y|.  A norm (``k_dtw_norms``: one accumulator
  of DIMP fused terms, then sqrt) is off by (DIMP / 2 + 1) u relative, the product of two norms by (DIMP + 3) u, the
  quotient by one more: (DIMP + 4) u relative on a cosine of magnitude <= 1.  Together (1.5 DIMP + 5) u absolute; the clamp
  to [-1, 1] moves the value towards the true one.  1 - cs is exact for cs >= 1 / 2 and otherwise rounds a result in
  [1 / 2, 2] by at most u: (1.5 DIMP + 6) u.

These are worst-case bounds, derived and not measured.  ``kernel_local_cost`` restates the kernel's accumulation order in
numpy float32 so that ``tests/test_dtw_cert.py`` can say how much of T plain rounding uses (about half at most).  The
float64 accumulation of D takes at most three roundings per cell (wm c, + wa, + predecessor, all terms >= 0): the factor
4 * 2^-53 above.  C itself is scipy's float64 ``cdist`` of the float32 inputs, whose own error is some 2^-53 C and not
counted."""
from __future__ import annotations

import numpy as np

from tests import dtw_ref as R
from tests import dtw_steps_ref as S

U = 2.0 ** -24
EPS = 4.0 * 2.0 ** -53
WIDTHS = (8, 16, 24, 40, 64, 128)

# what tests/test_gpu_dtw_cells.py runs and tests/test_dtw_cert.py measures the float32 restatement on
DIMS = [1, 8, 9, 16, 17, 20, 24, 25, 40, 41, 64, 65, 128]
METRICS = ["euclidean", "sqeuclidean", "cosine"]
# strip edges at 63, 64, 65 and 129; the ring of 72 columns; the 8-step tile and the 16-step code word on both sides
SHAPES = [(1, 1), (1, 73), (2, 9), (64, 64), (65, 71), (129, 72), (130, 65), (63, 200)]


def compiled_width(dim: int) -> int:
    """DIMP: the kernel width that serves ``dim`` (``dtw_with_dimp``)."""
    for w in WIDTHS:
        if dim <= w:
            return w
    raise ValueError(f"dim {dim} > {WIDTHS[-1]}")


def tolerance(C: np.ndarray, metric: str, dim: int) -> np.ndarray:
    """T: the bound on abs(device float32 local cost - C) per cell (module docstring)."""
    w = compiled_width(dim)
    if metric == "sqeuclidean":
        return (w / 2 + 4) * U * C
    if metric == "euclidean":
        return (w / 4 + 3) * U * C
    if metric == "cosine":
        return np.full(C.shape, (1.5 * w + 6) * U)
    raise ValueError(metric)


def _fma32(a, b, c):
    """fl32(a * b + c) of float32 arrays: the product of two float32 is exact in float64, the sum is rounded to float64
    and then to float32 (a double rounding, which differs from the fused operation in rare last-bit cases)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def kernel_local_cost(X, Y, metric: str) -> np.ndarray:
    """The device's local cost restated in numpy float32, in the kernel's order: rows padded with zeros to DIMP; elements
    4q, 4q+2 go into one accumulator and 4q+1, 4q+3 into the other by fused multiply-add; the two are added; sqrt
    (euclidean); or (cosine) the dot product divided by the product of the float32 norms (one accumulator over the row,
    sqrt), clamped to [-1, 1] and subtracted from 1.  [N, M] float32."""
    X = np.atleast_2d(np.asarray(X, np.float32))
    Y = np.atleast_2d(np.asarray(Y, np.float32))
    dim, n, m = X.shape[0], X.shape[1], Y.shape[1]
    w = compiled_width(dim)
    xp, yp = np.zeros((w, n), np.float32), np.zeros((w, m), np.float32)
    xp[:dim], yp[:dim] = X, Y
    acc = [np.zeros((n, m), np.float32), np.zeros((n, m), np.float32)]
    for e in range(w):
        a, b = xp[e][:, None], yp[e][None, :]
        if metric == "cosine":
            acc[e & 1] = _fma32(a, b, acc[e & 1])
        else:
            d = (a - b).astype(np.float32)
            acc[e & 1] = _fma32(d, d, acc[e & 1])
    s = (acc[0] + acc[1]).astype(np.float32)
    if metric == "sqeuclidean":
        return s
    if metric == "euclidean":
        return np.sqrt(s, dtype=np.float32)

    def norms(p):
        t = np.zeros(p.shape[1], np.float32)
        for e in range(w):
            t = _fma32(p[e], p[e], t)
        return np.sqrt(t, dtype=np.float32)

    den = (norms(xp)[:, None] * norms(yp)[None, :]).astype(np.float32)
    cs = np.minimum(np.float32(1), np.maximum(np.float32(-1), (s / den).astype(np.float32)))
    return (np.float32(1) - cs).astype(np.float32)


def make_pair(kind: str, n: int, m: int, dim: int, seed: int):
    """One float32 test pair (X [dim, n], Y [dim, m]).  kind "normal": N(0, 1); "mfcc": coefficient 0 near -300, the others
    scaled by about 20 and falling off with their index.  Both kinds: a run of repeated frames inside X, and a block of Y
    copied from X (exact zero cost under the Euclidean metrics, real ties); no zero-norm frame."""
    rng = np.random.default_rng(seed)

    def draw(t):
        a = rng.standard_normal((dim, t))
        if kind == "mfcc":
            a *= (20.0 / (1.0 + 0.15 * np.arange(dim)))[:, None]
            a[0] = -300.0 + 30.0 * rng.standard_normal(t)
        else:
            assert kind == "normal", kind
        return a.astype(np.float32)

    X, Y = draw(n), draw(m)
    if n >= 4:                                       # frames r0 .. r0 + run - 1 of X repeat frame r0
        run = max(2, n // 8)
        r0 = int(rng.integers(0, n - run + 1))
        X[:, r0:r0 + run] = X[:, r0:r0 + 1]
    b = max(1, min(n, m) // 3) if max(n, m) > 1 else 0      # the 1 x 1 pair keeps two different frames
    if b:
        i0, j0 = int(rng.integers(0, n - b + 1)), int(rng.integers(0, m - b + 1))
        Y[:, j0:j0 + b] = X[:, i0:i0 + b]
    assert (np.abs(X).sum(axis=0) > 0).all() and (np.abs(Y).sum(axis=0) > 0).all()
    return X, Y


def grid_pairs(dim: int):
    """The eight pairs of one GPU call at ``dim``: SHAPES, alternating the two input kinds."""
    return [make_pair(("normal", "mfcc")[p % 2], n, m, dim, 100 * dim + p) for p, (n, m) in enumerate(SHAPES)]


def _bits(v) -> bytes:
    return np.asarray(v, np.float64).tobytes()


def _live(St, wm):
    return [k for k in range(St.shape[0]) if np.isfinite(wm[k])]


def _pred(P, k, St, n, m):
    """D at the predecessor of every cell under step k (inf outside the matrix); P is D padded by two."""
    di, dj = int(St[k, 0]), int(St[k, 1])
    return P[2 - di:2 - di + n, 2 - dj:2 - dj + m]


def _bounds(D, Cb, T, St, wa, wm, subseq):
    """(lo, hi, mid, wmid) of check (c) for every cell: the minimum over the seed and the live steps of
    pred + (wm (C -+ T) + wa) from the given D; mid is the same at C itself and wmid the wm of mid's winner."""
    n, m = D.shape
    P = np.full((n + 2, m + 2), np.inf)
    P[2:, 2:] = D
    seed = np.zeros((n, m), bool)
    seed[0, 0] = True
    if subseq:
        seed[0, :] = True
    out = []
    with np.errstate(invalid="ignore"):
        for c in (Cb - T, Cb + T, Cb):
            best = np.where(seed, c, np.inf)
            wbest = np.ones((n, m))
            for k in _live(St, wm):
                cand = _pred(P, k, St, n, m) + (wm[k] * c + wa[k])
                win = cand < best
                best = np.where(win, cand, best)
                wbest = np.where(win, wm[k], wbest)
            out.append(best)
    return out[0], out[1], out[2], wbest


def _first_minimum(preds, k, d):
    """Check (d) for steps that share one weight pair: the device adds the same w to every predecessor and keeps the first
    strict minimum of the sums.  Rounding is monotone, so a step listed before k with a predecessor <= k's would have won;
    a step listed after k with a smaller predecessor would have won too unless the two sums rounded to the same double,
    which needs the predecessors to lie within one ulp of the cell's value d."""
    own = preds[k]
    for q, v in preds.items():                       # in list order
        if q < k and v <= own:
            return "step %d (pred %r) is listed before the step taken (%d, pred %r) and is not larger" % (q, v, k, own)
        if q > k and v < own - np.spacing(d):
            return "step %d (pred %r) is smaller than the step taken (%d, pred %r)" % (q, v, k, own)
    return None


def oracle(X, Y, metric, St, wa, wm, radius=None, subseq=False):
    """(D_ref, cost, wp_ref, status) of the float64 oracle on C = ``dtw_ref.local_cost`` of the float32 inputs:
    ``dtw_ref.dtw_vec`` for the default call, ``dtw_steps_ref.dtw_vec`` for every other.  ``certify`` takes it as
    ``reference`` so that callers that certify several results of one input compute it once."""
    wa, wm = np.asarray(wa, np.float64), np.asarray(wm, np.float64)
    C = R.local_cost(X, Y, metric, radius)
    if St.shape[0] == 3 and not subseq and (wa == 0).all() and (wm == 1).all():
        D_ref, _, ref, wp_ref, st = R.dtw_vec(C)
    else:
        D_ref, _, ref, _, wp_ref, st = S.dtw_vec(C, St, wa, wm, subseq)
    return D_ref, ref, wp_ref, st


def certify(D, wp, cost, cost_no_backtrack, X, Y, metric, St, wa, wm, radius=None, subseq=False, label="", reference=None):
    """Assert (a) - (e) of the module docstring on what the device returned for (X, Y): D [N, M] float64, wp [L, 2] end to
    start, the cost of the call with back-tracking and of the call without (None: not checked).  (St, wa, wm) is
    ``dtw_steps_ref.step_table``'s (inf weights mark the dead default entries), ``radius`` the band radius or None, all in
    the orientation the DP ran in; ``reference`` is ``oracle``'s result for the same arguments (computed here when None).
    Returns {"ratio": the maximum over cells of abs(D - mid) / (w T), "cells": the finite cells}, with
    mid = min_k(D[pred_k] + (wm_k C + wa_k)) and w the wm of mid's winning step (the largest wm of the list where D < mid:
    the device's own winner, which bounds that side, is not known).  With unit weights that is abs(D - (min pred + C)) / T."""
    X = np.atleast_2d(np.asarray(X))
    Y = np.atleast_2d(np.asarray(Y))
    assert X.dtype == np.float32 and Y.dtype == np.float32, "the certificate is of the float32 inputs the device saw"
    n, m, dim = X.shape[1], Y.shape[1], X.shape[0]
    D = np.asarray(D, np.float64)
    wp = np.asarray(wp, np.int64)
    wa, wm = np.asarray(wa, np.float64), np.asarray(wm, np.float64)
    assert D.shape == (n, m), (label, D.shape, (n, m))
    live = _live(St, wm)
    assert not np.isnan(D).any(), (label, "NaN in D")

    C = R.local_cost(X, Y, metric)
    T = tolerance(C, metric, dim)
    mask = R.band_mask(n, m, radius)
    Cb = np.where(mask, C, np.inf)

    # ---- a. reachability
    D_ref, ref, wp_ref, st = reference if reference is not None else oracle(X, Y, metric, St, wa, wm, radius, subseq)
    assert st == R.OK, (label, "the oracle finds no path: nothing to certify", st)
    bad = np.argwhere(np.isinf(D) != np.isinf(D_ref))
    assert bad.size == 0, "%s (a) reachability differs from the oracle's at %d cells, first %s" % (label, len(bad), bad[0])

    # ---- b, c. every finite cell against the device's own predecessors
    lo, hi, mid, wmid = _bounds(D, Cb, T, St, wa, wm, subseq)
    fin = np.isfinite(D)
    start = np.zeros((n, m), bool)
    start[0, 0] = True
    if subseq:
        start[0, :] = True
    with np.errstate(invalid="ignore"):
        out = fin & ((D < lo - EPS * np.abs(lo)) | (D > hi + EPS * np.abs(hi)))
    for name, sel in (("(b) start cell", out & start), ("(c) cell", out & ~start)):
        bad = np.argwhere(sel)
        if bad.size:
            i, j = bad[0]
            raise AssertionError("%s %s (%d, %d): D = %r outside [%r, %r]; C = %r, T = %r (%d such cells)"
                                 % (label, name, i, j, D[i, j], lo[i, j], hi[i, j], C[i, j], T[i, j], len(bad)))
    exact = fin & (T == 0) & (C == 0)
    bad = np.argwhere(exact & (D != mid))
    assert bad.size == 0, "%s (c) zero-cost cell %s: D = %r, not the minimum predecessor %r" % (
        label, bad[0], D[tuple(bad[0])], mid[tuple(bad[0])])
    meas = fin & (T > 0)
    ratio = 0.0
    if meas.any():
        off = D[meas] - mid[meas]
        ratio = float((np.abs(off) / (np.where(off < 0, wm[live].max(), wmid[meas]) * T[meas])).max())

    # ---- d. the path as a back-track of D
    assert wp.ndim == 2 and wp.shape[1] == 2 and len(wp) >= 1, (label, wp.shape)
    end = int(np.argmin(D[n - 1])) if subseq else m - 1
    assert tuple(wp[0]) == (n - 1, end), "%s (d) the path starts at %s, not at (%d, %d)" % (label, tuple(wp[0]), n - 1, end)
    if subseq:
        assert wp[-1, 0] == 0 and (wp[:-1, 0] > 0).all(), "%s (d) the path does not stop at its first cell of row 0" % label
    else:
        assert tuple(wp[-1]) == (0, 0), "%s (d) the path stops at %s" % (label, tuple(wp[-1]))
    assert (wp >= 0).all() and (wp[:, 0] < n).all() and (wp[:, 1] < m).all(), (label, "(d) a path cell outside the matrix")
    assert np.isfinite(D[wp[:, 0], wp[:, 1]]).all(), "%s (d) the path crosses an unreachable cell" % label
    shared = len({(wa[k], wm[k]) for k in live}) == 1
    taken = []
    for t in range(len(wp) - 1):
        i, j = int(wp[t, 0]), int(wp[t, 1])
        step = (i - int(wp[t + 1, 0]), j - int(wp[t + 1, 1]))
        ks = [k for k in live if (int(St[k, 0]), int(St[k, 1])) == step]
        assert ks, "%s (d) path step %d, %s at (%d, %d), is not in the list" % (label, t, step, i, j)
        preds = {k: (D[i - St[k, 0], j - St[k, 1]] if i >= St[k, 0] and j >= St[k, 1] else np.inf) for k in live}
        d = D[i, j]
        why = "no step with that offset fits"
        for k in ks:
            p = preds[k]
            a, b = p + (wm[k] * (C[i, j] - T[i, j]) + wa[k]), p + (wm[k] * (C[i, j] + T[i, j]) + wa[k])
            if not (a - EPS * abs(a) <= d <= b + EPS * abs(b)):
                why = "D = %r is not pred %r + wm (C +- T) + wa = [%r, %r]" % (d, p, a, b)
                continue
            why = _first_minimum(preds, k, d) if shared else None
            if why is None:
                taken.append(k)
                break
        assert why is None, "%s (d) path step %d at (%d, %d): %s" % (label, t, i, j, why)

    # ---- e. the cost
    dend = D[wp[0, 0], wp[0, 1]]
    assert _bits(cost) == _bits(dend), "%s (e) cost %r is not D at the path's end %r" % (label, float(cost), float(dend))
    if cost_no_backtrack is not None:
        assert _bits(cost_no_backtrack) == _bits(dend), "%s (e) cost without back-tracking %r is not D at the path's end %r" % (
            label, float(cost_no_backtrack), float(dend))

    def path_tolerance(path, ks):
        return float(T[path[-1, 0], path[-1, 1]] + sum(wm[k] * T[path[t, 0], path[t, 1]] for t, k in enumerate(ks)))

    ks_ref = []
    for t in range(len(wp_ref) - 1):
        step = tuple(int(v) for v in wp_ref[t] - wp_ref[t + 1])
        ks_ref.append([k for k in live if (int(St[k, 0]), int(St[k, 1])) == step][0])
    sum_ref, sum_dev = path_tolerance(wp_ref, ks_ref), path_tolerance(wp, taken)
    slack = EPS * (len(wp) + len(wp_ref)) * max(abs(ref), abs(float(cost)))      # the float64 sums along the two paths
    assert ref - sum_dev - slack <= cost <= ref + sum_ref + slack, "%s (e) cost %r outside [%r - %r, %r + %r]" % (
        label, float(cost), ref, sum_dev, ref, sum_ref)
    return {"ratio": ratio, "cells": int(fin.sum())}
