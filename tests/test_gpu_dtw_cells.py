"""Every cell of D, the path and the cost of k_dtw and k_dtw_steps against the per-cell certificate (tests/dtw_cert.py):
real-valued inputs at every compiled width and both of its edges, all three metrics, the band, weights, custom step lists
and subseq.  One dtw_batch call with the cost matrix per (dim, metric, mode), eight pairs each; every test prints the
maximum over its cells of |D - (min pred + C)| / T before it asserts."""
import numpy as np
import pytest

from tests import dtw_cert as K
from tests import dtw_ref as R
from tests import dtw_steps_ref as S

pytestmark = pytest.mark.gpu

SLOPE = [[1, 1], [1, 2], [2, 1]]
FIVE = [[1, 1], [2, 1], [1, 2], [2, 2], [0, 1]]
_W = dict(weights_add=[0.0, 0.5, 1.0], weights_mul=[1.0, 1.5, 2.0])
MODES = {                                            # the first three run k_dtw, the others k_dtw_steps
    "dtw": dict(),
    "dtw-band25": dict(global_constraints=True, band_rad=0.25),
    "dtw-band10": dict(global_constraints=True, band_rad=0.1),
    "steps-unit": dict(weights_mul=[1.0, 1.0, 1.0]),
    "slope-w": dict(step_sizes_sigma=SLOPE, **_W),
    "slope-w-sub": dict(step_sizes_sigma=SLOPE, subseq=True, **_W),
    "five-sub": dict(step_sizes_sigma=FIVE, subseq=True),
}


@pytest.fixture(scope="module")
def seq():
    from audio_feature_extraction_amd import _native, sequence
    if _native.device_count() < 1:
        pytest.fail("no GPU visible")
    return sequence


_PAIRS, _ORACLE, _RUNS = {}, {}, {}


def _pairs(dim):
    if dim not in _PAIRS:
        _PAIRS[dim] = K.grid_pairs(dim)
        for X, Y in _PAIRS[dim]:
            X.setflags(write=False)
            Y.setflags(write=False)
    return _PAIRS[dim]


def _table(mode):
    kw = MODES[mode]
    return S.step_table(kw.get("step_sizes_sigma"), kw.get("weights_add"), kw.get("weights_mul"))


def _oriented(X, Y, mode):
    """(X, Y, swapped) as the DP runs them: under subseq the shorter sequence is matched inside the longer."""
    swap = bool(MODES[mode].get("subseq")) and X.shape[1] > Y.shape[1]
    return (Y, X, True) if swap else (X, Y, False)


def _radius(X, Y, mode):
    kw = MODES[mode]
    return R.band_radius(X.shape[1], Y.shape[1], kw["band_rad"]) if kw.get("global_constraints") else None


def _oracle(dim, metric, mode, p):
    """The float64 oracle of pair p, once per (dim, metric, what the oracle depends on): "dtw" and "steps-unit" share it."""
    key = (dim, metric, "dtw" if mode == "steps-unit" else mode, p)
    if key not in _ORACLE:
        X, Y, _ = _oriented(*_pairs(dim)[p], mode)
        St, wa, wm = _table(mode)
        out = K.oracle(X, Y, metric, St, wa, wm, _radius(X, Y, mode), bool(MODES[mode].get("subseq")))
        if out[0] is not None:
            out[0].setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


def _run(seq, dim, metric, mode):
    """The device's results for the eight pairs: (D, wp) from one call with the cost matrix, and the costs of the calls
    with and without back-tracking."""
    key = (dim, metric, mode)
    if key not in _RUNS:
        pairs = _pairs(dim)
        full = seq.dtw_batch(pairs, metric=metric, return_cost_matrix=True, **MODES[mode])
        cost = seq.dtw_batch(pairs, metric=metric, **MODES[mode])
        bare = seq.dtw_batch(pairs, metric=metric, backtrack=False, **MODES[mode])
        _RUNS[key] = (full, cost, bare)
    return _RUNS[key]


def _certify_pair(dim, metric, mode, p, D, wp, cost, bare, reference=None):
    X, Y, swap = _oriented(*_pairs(dim)[p], mode)
    if swap:
        D, wp = D.T, wp[:, ::-1]
    St, wa, wm = _table(mode)
    return K.certify(D, wp, cost, bare, X, Y, metric, St, wa, wm, _radius(X, Y, mode), bool(MODES[mode].get("subseq")),
                     label="d%d %s %s pair %d (%d x %d)" % (dim, metric, mode, p, X.shape[1], Y.shape[1]),
                     reference=reference if reference is not None else _oracle(dim, metric, mode, p))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("metric", K.METRICS)
@pytest.mark.parametrize("dim", K.DIMS)
def test_every_cell_is_certified(seq, dim, metric, mode):
    full, cost, bare = _run(seq, dim, metric, mode)
    worst, cells, done = 0.0, 0, 0
    for p in range(len(K.SHAPES)):
        st = _oracle(dim, metric, mode, p)[3]
        assert st in (R.OK, R.NO_PATH)
        if st == R.NO_PATH:                          # the band or the step list admits no path: the pair fails, alone
            assert full[p] is None and cost[p] is None and bare[p] is None, (p, K.SHAPES[p])
            continue
        assert full[p] is not None and cost[p] is not None and bare[p] is not None, (p, K.SHAPES[p])
        np.testing.assert_array_equal(cost[p][1], full[p][1])
        r = _certify_pair(dim, metric, mode, p, full[p][0], full[p][1], cost[p][0], bare[p])
        worst, cells, done = max(worst, r["ratio"]), cells + r["cells"], done + 1
    print("dtw_cells dim=%d width=%d metric=%s mode=%s pairs=%d cells=%d max_ratio=%.3f"
          % (dim, K.compiled_width(dim), metric, mode, done, cells, worst))
    # the pairs with a path: radius round(0.25 * min) = 0 for the three smallest shapes, and the slope-limited list needs
    # M in [N / 2 + 1, 2 N - 1] without subseq
    assert done == {"dtw-band25": 5, "dtw-band10": 5, "slope-w": 4}.get(mode, 8)
    assert worst < 1.0
    if mode == "steps-unit":                         # 1.0 * c + 0.0 == c: the two kernels form the same sums
        ref = _run(seq, dim, metric, "dtw")
        for p in range(len(K.SHAPES)):
            np.testing.assert_array_equal(full[p][0], ref[0][p][0])
            np.testing.assert_array_equal(full[p][1], ref[0][p][1])
            assert cost[p][0] == ref[1][p][0] and bare[p] == ref[2][p]


@pytest.mark.parametrize("metric", K.METRICS)
def test_a_pair_alone_equals_the_pair_in_the_batch(seq, metric):
    for dim in K.DIMS:
        for mode in ("dtw", "slope-w-sub"):
            full, cost, bare = _run(seq, dim, metric, mode)
            for p in (4, 5):                         # 65 x 71 and 129 x 72 (swapped under subseq)
                X, Y = _pairs(dim)[p]
                D, wp = seq.dtw(X, Y, metric=metric, return_cost_matrix=True, **MODES[mode])
                np.testing.assert_array_equal(D, full[p][0])
                np.testing.assert_array_equal(wp, full[p][1])
                c, wp2 = seq.dtw(X, Y, metric=metric, **MODES[mode])
                assert c == cost[p][0] and c == bare[p]
                np.testing.assert_array_equal(wp2, wp)


@pytest.mark.parametrize("dim", [7, 15, 23, 39, 63, 127])
def test_padding_reads_zeros_not_the_neighbour(seq, dim):
    """A dim one under the compiled width, followed in the same feature buffer by a pair whose features are 1e30: a padding
    element that read a neighbouring frame instead of zero would put 1e30 (or that frame's first coefficient) into the
    local cost of the first pair, which is certified cell by cell."""
    X, Y = K.make_pair("normal", 65, 71, dim, 5000 + dim)
    big = (np.full((dim, 9), 1e30, np.float32), np.full((dim, 10), 1e30, np.float32))
    assert K.compiled_width(dim) == dim + 1
    for metric in K.METRICS:
        for mode in ("dtw", "steps-unit"):
            St, wa, wm = _table(mode)
            reference = K.oracle(X, Y, metric, St, wa, wm)
            full = seq.dtw_batch([(X, Y), big], metric=metric, return_cost_matrix=True, **MODES[mode])
            cost = seq.dtw_batch([(X, Y), big], metric=metric, **MODES[mode])
            bare = seq.dtw_batch([(X, Y), big], metric=metric, backtrack=False, **MODES[mode])
            assert full[0] is not None and cost[0] is not None and bare[0] is not None
            np.testing.assert_array_equal(cost[0][1], full[0][1])
            r = K.certify(full[0][0], full[0][1], cost[0][0], bare[0], X, Y, metric, St, wa, wm,
                          label="d%d %s %s before 1e30" % (dim, metric, mode), reference=reference)
            print("dtw_pad dim=%d width=%d metric=%s mode=%s max_ratio=%.3f" % (dim, dim + 1, metric, mode, r["ratio"]))
            assert r["ratio"] < 1.0
