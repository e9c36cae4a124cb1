"""afx_wav_read_raw: the data chunk of every WAVE layout read natively as bytes (host only: no device needed)."""
import numpy as np
import pytest

from audio_feature_extraction_amd import _native as N
from tests.wavfiles import FORMAT, KINDS, quantize, write_wav


def _files(tmp_path):
    rng = np.random.default_rng(3)
    out = []
    for kind in KINDS:
        for ch in (1, 2, 3):
            n = int(rng.integers(5, 700))
            p = tmp_path / f"{kind}_{ch}.wav"
            out.append((str(p), kind, ch, n, write_wav(p, quantize(rng.uniform(-1, 1, n), kind, ch), 16000, kind)))
    return out


def test_every_layout_is_read_byte_for_byte_at_the_given_offsets(tmp_path):
    files = _files(tmp_path)
    paths = [f[0] for f in files]
    pr = N.wav_probe(paths, 4)
    assert (pr["status"] == 0).all()
    for k, (_, kind, ch, n, data) in enumerate(files):
        assert (pr["tag"][k], pr["bits"][k]) == FORMAT[kind] and pr["channels"][k] == ch and pr["frames"][k] == n
        assert N.wav_sample_kinds(pr)[k] == N.SMP_KINDS[kind] and len(data) == n * ch * N.SMP_BYTES[N.SMP_KINDS[kind]]
    nbytes = np.array([len(f[4]) for f in files], np.int64)
    offs = N.packed_offsets(nbytes, 16) + 32                    # 16-byte boundaries, behind a margin
    buf = np.full(int(offs[-1] + nbytes[-1]), 0xA5, np.uint8)   # ends with the last clip's last byte
    for threads in (1, 5):
        buf[:] = 0xA5
        st = N.wav_read_raw(paths, pr["data_off"], nbytes, buf, offs, threads)
        assert (st == 0).all()
        seen = np.zeros(buf.size, bool)
        for o, (_, _, _, _, data) in zip(offs, files):
            assert buf[o:o + len(data)].tobytes() == data
            seen[o:o + len(data)] = True
        assert (buf[~seen] == 0xA5).all()                       # nothing written between the clips


def test_a_missing_file_fails_alone(tmp_path):
    files = _files(tmp_path)[:5]
    paths = [f[0] for f in files]
    pr = N.wav_probe(paths, 2)
    paths[2] = str(tmp_path / "gone.wav")
    nbytes = np.array([len(f[4]) for f in files], np.int64)
    offs = N.packed_offsets(nbytes, 16)
    buf = np.full(int(offs[-1] + nbytes[-1]), 0xA5, np.uint8)
    st = N.wav_read_raw(paths, pr["data_off"], nbytes, buf, offs, 3)
    assert st.tolist() == [0, 0, 2, 0, 0]
    for k, (o, f) in enumerate(zip(offs, files)):
        want = bytes([0xA5]) * len(f[4]) if k == 2 else f[4]
        assert buf[o:o + len(f[4])].tobytes() == want
    assert N.wav_probe(paths, 2)["status"].tolist() == [0, 0, 2, 0, 0]


def test_clips_that_do_not_fit_are_refused_before_anything_is_read(tmp_path):
    files = _files(tmp_path)[:4]
    paths = [f[0] for f in files]
    pr = N.wav_probe(paths, 2)
    nbytes = np.array([len(f[4]) for f in files], np.int64)
    offs = N.packed_offsets(nbytes, 16)
    size = int(offs[-1] + nbytes[-1])
    buf = np.full(size, 0xA5, np.uint8)
    big, neg = nbytes.copy(), offs.copy()
    big[1] = size + 1
    neg[0] = -16
    far = offs.copy()
    far[3] = np.iinfo(np.int64).max - 2                          # offset + size would overflow
    for kw in (dict(nbytes=big, offsets=offs, out=buf), dict(nbytes=nbytes, offsets=neg, out=buf),
               dict(nbytes=nbytes, offsets=far, out=buf), dict(nbytes=nbytes, offsets=offs, out=buf[:size - 1])):
        with pytest.raises(ValueError):
            N.wav_read_raw(paths, pr["data_off"], kw["nbytes"], kw["out"], kw["offsets"], 2)
        assert (buf == 0xA5).all()
    lib = N.lib()
    st = np.zeros(4, np.int32)
    rc = lib.afx_wav_read_raw(N._path_array(paths), 4, 2, pr["data_off"].ctypes.data, nbytes.ctypes.data, buf.ctypes.data,
                              size - 1, offs.ctypes.data, st.ctypes.data)
    assert rc == -1 and (buf == 0xA5).all()                     # AFX_ERR_INVALID
    assert (N.wav_read_raw(paths, pr["data_off"], nbytes, buf, offs, 2) == 0).all()       # and the exact size is taken
