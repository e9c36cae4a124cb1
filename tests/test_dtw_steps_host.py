"""CPU checks of afx_dtw_steps_batch's declaration and of sequence.dtw's step-argument validation (no device is opened)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts), encoding="utf-8") as f:
        return f.read()


def test_symbol_is_declared_bound_and_stubbed():
    from audio_feature_extraction_amd import _native as N
    hdr = _read("include", "afx.h")
    assert re.search(r"\bint afx_dtw_steps_batch\(", hdr)
    assert re.search(r"\bAFX_DTW_SUBSEQ\s*=\s*4\b", hdr) and N.DTW_SUBSEQ == 4
    assert "afx_dtw_steps_batch" in N.SYMBOLS
    assert re.search(r"\bint afx_dtw_steps_batch\(", _read("audio_feature_extraction_amd", "csrc", "afx_host_stubs.cpp"))
    assert re.search(r'extern "C" int afx_dtw_steps_batch\(', _read("audio_feature_extraction_amd", "csrc", "afx_ctx_ops.cpp"))
    assert "afx_dtw_steps_batch" in _read("INTEGRATION.md")
    # the declaration and the stub take the same number of arguments as the binding passes (23)
    decl = re.search(r"\bint afx_dtw_steps_batch\((.*?)\);", hdr, re.S).group(1)
    assert len(decl.split(",")) == 23
    assert hasattr(N.Context, "dtw_steps_batch")


@pytest.fixture
def seq(monkeypatch):
    from audio_feature_extraction_amd import _native, sequence

    def no_device(*a, **k):
        raise AssertionError("a device was opened")
    monkeypatch.setattr(_native, "Context", no_device)
    monkeypatch.setattr(sequence, "_contexts", {})
    return sequence


X, Y = np.zeros((3, 6), np.float32), np.zeros((3, 8), np.float32)


@pytest.mark.parametrize("kwargs,exc", [
    (dict(step_sizes_sigma=[[1, 1], [3, 1]]), NotImplementedError),                       # a component of 3
    (dict(step_sizes_sigma=[[1, 1], [1, 4]]), NotImplementedError),
    (dict(step_sizes_sigma=[[1, 1], [1, 2], [2, 1], [2, 2], [0, 1], [1, 0]]), NotImplementedError),   # six steps
    (dict(step_sizes_sigma=[[1, 1], [-1, 1]]), ValueError),                               # a negative component
    (dict(step_sizes_sigma=[[1, 1], [1, -2]]), ValueError),
    (dict(step_sizes_sigma=[[1, 1], [0, 0]]), ValueError),                                # (0, 0)
    (dict(step_sizes_sigma=[]), ValueError),
    (dict(step_sizes_sigma=[1, 1]), ValueError),                                          # not a list of pairs
    (dict(step_sizes_sigma=[[1, 1.5]]), ValueError),
    (dict(weights_mul=[1.0, -1.0, 1.0]), ValueError),                                     # negative weight
    (dict(weights_add=[0.0, np.nan, 0.0]), ValueError),
    (dict(weights_mul=[1.0, np.inf, 1.0]), ValueError),
    (dict(step_sizes_sigma=[[1, 1], [1, 2]], weights_add=[0.0, -0.5]), ValueError),
    (dict(weights_add=[0.0, 0.0]), ValueError),                                           # length: three default steps
    (dict(step_sizes_sigma=[[1, 1], [1, 2]], weights_mul=[1.0, 1.0, 1.0]), ValueError),   # length: two custom steps
    (dict(step_sizes_sigma=[[1, 1], [1, 2]], weights_add=[0.0]), ValueError),
])
def test_step_arguments_are_refused_before_any_native_call(seq, kwargs, exc):
    with pytest.raises(exc):
        seq.dtw(X, Y, **kwargs)
    with pytest.raises(exc):
        seq.dtw(X, Y, subseq=True, **kwargs)
    with pytest.raises(exc):
        seq.dtw_batch([(X, Y)], **kwargs)


def test_diagonal_only_with_more_rows_than_columns_is_refused(seq):
    with pytest.raises(ValueError):
        seq.dtw(Y, X, step_sizes_sigma=[[1, 1]])                   # N = 8 > M = 6
    assert seq.dtw_batch([(Y, X)], step_sizes_sigma=[[1, 1]]) == [None]
    # the shape checks of the default path still come first
    with pytest.raises(ValueError):
        seq.dtw(np.zeros((3, 5)), np.zeros((4, 5)), subseq=True)


def test_accepted_arguments_reach_the_device_call(seq):
    # a valid call gets as far as opening the device (which this test forbids): nothing before that refuses it
    for kwargs in (dict(subseq=True), dict(step_sizes_sigma=[[1, 1], [1, 2], [2, 1]]), dict(weights_mul=[1, 2, 2]),
                   dict(step_sizes_sigma=np.array([[1, 1], [2, 2], [0, 1], [0, 2], [2, 0]]), weights_add=np.zeros(5)),
                   dict(step_sizes_sigma=[[1, 1]], subseq=True)):
        with pytest.raises(AssertionError, match="a device was opened"):
            seq.dtw(Y, X, **kwargs)


def test_code_word_accounting_of_the_general_kernel():
    # afx_dtw.h: 4-bit codes, one word per lane and tile of 8 wavefront steps (steps 0 .. m + 62 of a strip)
    hdr = _read("audio_feature_extraction_amd", "csrc", "afx_dtw.h")
    assert "inline int32_t dtw_steps_qn(int m) { return (m + 62) / 8 + 1; }" in hdr
    assert "dtw_steps_code_words" in _read("audio_feature_extraction_amd", "csrc", "afx_ctx_ops.cpp")
    for m in (1, 2, 3, 9, 10, 11, 862):
        assert ((m + 62) // 8 + 1) * 8 > m - 1 + 63          # the last step of a strip, m - 1 + 63, has a word
