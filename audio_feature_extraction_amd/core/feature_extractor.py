"""MI355X-native ``AudioFeatureExtractor`` -- drop-in for the reference class
(audio_feature_extraction_toolkit/core/feature_extractor.py:7-237): same
constructor arguments and attributes (:10-39), same methods, same result-dict
keys / key order / Python types (:109-114, :146-151, :175-178, :202-207) and the
same error behaviour (log + re-raise in ``load_audio`` / ``extract_features``;
``batch_process`` logs and skips a failing file, :233-235).

The MFCC / RMS arithmetic that the reference delegates to librosa runs in the
hand-written HIP kernels of ``libafx.so`` through the ctypes C-ABI in
``include/afx.h``.  There is no CPU fallback: without the library or a GPU the
calls raise.
"""
from __future__ import annotations

import logging
import threading
from pathlib import Path
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .. import _native, wavio

# librosa.note_to_hz('C2') / ('C7') -- the reference evaluates these at class-definition
# time (feature_extractor.py:15-16); written out so that importing needs no librosa.
_C2_HZ = 65.40639132514966
_C7_HZ = 2093.004522404789



def _one_clip(y: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(samples, offsets, lengths) of a batch that is the one clip ``y``, as contiguous float32."""
    y = np.ascontiguousarray(y, dtype=np.float32)
    return y, np.zeros(1, np.int64), np.array([y.size], np.int64)


def _status_error(status: int, what: str, n_frames: int = 0) -> Exception:
    if status == _native.CLIP_NONFINITE:
        return ValueError("Audio buffer is not finite everywhere")
    if status == _native.CLIP_TOO_SHORT:
        return ValueError(
            f"when mode='interp', width=9 cannot exceed data.shape[axis]={n_frames} ({what})")
    return RuntimeError(f"{what}: clip status {status}")


class AudioFeatureExtractor:
    """音頻特徵提取器類 (GPU)"""

    def __init__(self,
                 sr: int = 22050,
                 frame_length: int = 1024,
                 hop_length: int = 256,
                 n_mfcc: int = 13,
                 f0_min: float = _C2_HZ,
                 f0_max: float = _C7_HZ,
                 pre_emphasis: float = 0.97,
                 *,
                 window: str = "hamming",
                 n_mels: int = 128,
                 fmin: float = 0.0,
                 fmax: Optional[float] = None,
                 htk: bool = False,
                 lifter: float = 0.0,
                 device: Optional[Sequence[int] | int] = None):
        """Positional arguments are the reference's (feature_extractor.py:10-17).
        Keyword-only extensions default to the reference's hard-coded values:
        ``window`` ('hamming', :133; 'hann' also supported), ``n_mels`` (librosa's 128), ``fmin`` / ``fmax`` /
        ``htk`` (librosa.filters.mel's band edges and mel scale) and ``lifter`` (librosa.feature.mfcc's) -- the
        variants the reference's experiment extractors pass (04_feature_extraction_experiment/
        audio_feature_extraction 2/audio_feature_extraction/feature_extractor.py:148-181),
        ``device`` (GPU index or list of indices; None = all visible GPUs for
        ``batch_process``, GPU 0 for single-clip calls)."""
        self.sr = sr
        self.frame_length = frame_length
        self.hop_length = hop_length
        self.n_mfcc = n_mfcc
        self.f0_min = f0_min
        self.f0_max = f0_max
        self.pre_emphasis = pre_emphasis
        self.window = window
        self.n_mels = n_mels
        self.fmin, self.fmax, self.htk, self.lifter = fmin, fmax, htk, lifter
        self.device = device

        logging.basicConfig(level=logging.INFO)
        self.logger = logging.getLogger(__name__)
        self._plans: Dict[Tuple[int, int], _native.Plan] = {}
        self._plan_lock = threading.Lock()

    # ------------------------------------------------------------------ plumbing
    def _devices(self) -> List[int]:
        if self.device is None:
            n = _native.device_count()
            if n <= 0:
                raise _native.AfxError("no MI355X / HIP device visible (no CPU fallback exists)")
            return list(range(n))
        if isinstance(self.device, int):
            return [self.device]
        return [int(d) for d in self.device]

    def _cached_plan(self, device: int, key, make_params) -> _native.Plan:
        """The plan (own context + stream) cached under (device, key), created from ``make_params()`` on first use."""
        with self._plan_lock:
            pl = self._plans.get((device, key))
            if pl is None:
                pl = self._plans[(device, key)] = _native.Plan(_native.Context(device), make_params())
            return pl

    def _plan(self, device: Optional[int] = None, lane: int = 0) -> _native.Plan:
        """One plan (own context + stream) per (device, lane); lanes > 0 are the extra in-flight
        workers ``batch_process`` runs per GPU."""
        if device is None:
            device = self._devices()[0]
        return self._cached_plan(device, lane, lambda: _native.make_params(
            self.sr, self.frame_length, self.hop_length, self.n_mfcc, self.n_mels, self.window, self.pre_emphasis,
            self.fmin, self.fmax, self.htk, self.lifter))

    def _uses_reference_stages(self) -> bool:
        """True when no stage method has been replaced on the instance or in a subclass
        (README.md:135-136 shows users monkey-patching ``preprocess_audio``); only then may
        ``extract_features`` / ``batch_process`` take the fused single-pass GPU path."""
        for name in ("preprocess_audio", "extract_mfcc", "extract_energy", "extract_f0", "load_audio"):
            if name in self.__dict__ or getattr(type(self), name) is not getattr(AudioFeatureExtractor, name):
                return False
        return True

    def _stats_to_dicts(self, stats: np.ndarray) -> Tuple[Dict[str, Any], Dict[str, Any]]:
        K = self.n_mfcc
        mfcc = {
            "mfcc_mean": stats[0:K].tolist(),
            "mfcc_std": stats[K:2 * K].tolist(),
            "mfcc_delta_mean": stats[2 * K:3 * K].tolist(),
            "mfcc_delta2_mean": stats[3 * K:4 * K].tolist(),
        }
        energy = {
            "energy_mean": float(stats[4 * K]),
            "energy_std": float(stats[4 * K + 1]),
            "energy_range": float(stats[4 * K + 2]),
        }
        return mfcc, energy

    def _run_one(self, y: np.ndarray, flags: int) -> np.ndarray:
        out = self._plan().extract_batch(*_one_clip(y), flags=flags)
        if out["status"][0] != _native.CLIP_OK:
            raise _status_error(int(out["status"][0]), "extract", int(out["nframes"][0]))
        return out["stats"][0]

    # ------------------------------------------------------------------ reference API
    def load_audio(self, audio_path: str) -> Tuple[np.ndarray, int]:
        """載入音頻文件 -> (float32 mono, sr).  WAV decode + channel mean as librosa.load
        (feature_extractor.py:52); files at another rate are resampled on the host."""
        try:
            y, sr = wavio.load(audio_path, self.sr)
            return y, sr
        except Exception as e:
            self.logger.error(f"載入音頻文件失敗: {str(e)}")
            raise

    def preprocess_audio(self, y: np.ndarray) -> np.ndarray:
        """音頻預處理: pre-emphasis (coef=self.pre_emphasis) then silence trim at 30 dB
        (feature_extractor.py:58-74), on the GPU."""
        y_pre, start, end, status = self._plan().preprocess(np.asarray(y, dtype=np.float32))
        if status != _native.CLIP_OK:
            raise _status_error(status, "preprocess_audio")
        return y_pre[start:end]

    @staticmethod
    def _f0_to_dict(s: np.ndarray) -> Dict[str, Any]:
        return {
            "f0_mean": float(s[0]),
            "f0_std": float(s[1]),
            "f0_missing_rate": float(s[2]),
            "f0_quality": float(s[3]),
        }

    def _f0_on_gpu(self) -> bool:
        """The batched path may compute F0 on the device only while ``extract_f0`` is the stock method."""
        return "extract_f0" not in self.__dict__ and type(self).extract_f0 is AudioFeatureExtractor.extract_f0

    def _run_f0(self, y: np.ndarray, flags: int) -> np.ndarray:
        out = self._plan().f0_batch(*_one_clip(y), float(self.f0_min), float(self.f0_max), flags=flags)
        if out["status"][0] != _native.CLIP_OK:
            raise _status_error(int(out["status"][0]), "extract_f0")
        return out["stats"][0]

    def extract_f0(self, y: np.ndarray) -> Dict[str, Any]:
        """提取基頻特徵 (feature_extractor.py:76-114): ``librosa.pyin(y, fmin=f0_min, fmax=f0_max,
        frame_length, hop_length, sr)`` on the GPU -- difference function, probabilistic thresholds,
        Viterbi -- reduced to mean / std over the voiced frames, missing rate and quality."""
        return self._f0_to_dict(self._run_f0(y, 0))

    def extract_mfcc(self, y: np.ndarray) -> Dict[str, Any]:
        """提取MFCC特徵 of an already preprocessed signal (feature_extractor.py:116-151)."""
        return self._stats_to_dicts(self._run_one(y, 0))[0]

    def extract_energy(self, y: np.ndarray) -> Dict[str, Any]:
        """提取能量特徵 of an already preprocessed signal (feature_extractor.py:153-179).  Only ``librosa.feature.rms``
        is involved there, so a clip with fewer than 9 frames -- which fails ``extract_mfcc`` on the width-9 delta --
        still has its energy statistics."""
        return self._energy_from(y, 0)

    def _energy_from(self, y: np.ndarray, flags: int) -> Dict[str, Any]:
        y, off, ln = _one_clip(y)
        out = self._plan().extract_batch(y, off, ln, flags=flags)
        st = int(out["status"][0])
        # a TOO_SHORT clip with at least two samples has its RMS statistics on every shape (include/afx.h, out_stats)
        if st != _native.CLIP_OK and not (st == _native.CLIP_TOO_SHORT and y.size >= 2 and out["nframes"][0] >= 1):
            raise _status_error(st, "extract_energy", int(out["nframes"][0]))
        return self._stats_to_dicts(out["stats"][0])[1]

    def extract_features(self, audio_path: str, *, features_to_extract: Optional[Sequence[str]] = None) -> Dict[str, Any]:
        """提取所有特徵 (feature_extractor.py:181-213).

        ``features_to_extract`` (keyword-only; README.md:141-146 shows ``['f0', 'mfcc', 'energy']``): the feature groups
        wanted.  None = all three, the reference's behaviour; a subset leaves the other groups' keys out of the dict
        (key order unchanged) and skips their GPU passes -- without ``'f0'`` no pYIN pass runs."""
        try:
            from ..parallel import normalize_features
            want = normalize_features(features_to_extract)
            y, _ = self.load_audio(audio_path)
            f0_features: Dict[str, Any] = {}
            mfcc_features: Dict[str, Any] = {}
            energy_features: Dict[str, Any] = {}
            if self._uses_reference_stages():
                flags = _native.FLAG_PREEMPH | _native.FLAG_TRIM
                if "mfcc" in want:
                    # fused: pre-emphasis + trim + MFCC + RMS in one pass over the samples
                    mfcc_features, energy_features = self._stats_to_dicts(self._run_one(y, flags))
                elif "energy" in want:
                    energy_features = self._energy_from(y, flags)
                if "f0" in want:
                    f0_features = self._f0_to_dict(self._run_f0(y, flags))
            else:
                y_processed = self.preprocess_audio(y)
                if "f0" in want:
                    f0_features = self.extract_f0(y_processed)
                if "mfcc" in want:
                    mfcc_features = self.extract_mfcc(y_processed)
                if "energy" in want:
                    energy_features = self.extract_energy(y_processed)
            features = {"file_path": audio_path}
            if "f0" in want:
                features.update(f0_features)
            if "mfcc" in want:
                features.update(mfcc_features)
            if "energy" in want:
                features.update(energy_features)
            return features
        except Exception as e:
            self.logger.error(f"特徵提取失敗: {str(e)}")
            raise

    # ------------------------------------------------------------------ per-frame export
    def extract_frame_features(self, audio_path: str) -> Dict[str, np.ndarray]:
        """The per-frame matrices the reference computes and then reduces (feature_extractor.py:127-138,
        :164, :87), in the layout its experiment scripts save and its DTW aligner reads
        (04_feature_extraction_experiment/feature_extraction.py:191-215, 340-352): ``mfcc`` is
        ``vstack([mfcc, delta, delta2])`` of shape (3*n_mfcc, T) float32, ``f0`` the pYIN track (T,)
        float64 with NaN on unvoiced frames, ``energy`` the RMS row (T,) float32, ``zcr`` the
        zero-crossing rate (T,) float64 -- all of the preprocessed signal, all computed on the GPU."""
        y, off, ln = _one_clip(self.load_audio(audio_path)[0])
        flags = _native.FLAG_PREEMPH | _native.FLAG_TRIM
        plan = self._plan()
        out = plan.extract_batch(y, off, ln, flags=flags, want_frames=True)
        if out["status"][0] != _native.CLIP_OK:
            raise _status_error(int(out["status"][0]), "extract_frame_features", int(out["nframes"][0]))
        fr = out["frames"][0]
        T = int(out["nframes"][0])
        f0 = plan.f0_batch(y, off, ln, float(self.f0_min), float(self.f0_max), flags=flags, want_frames=True)
        zcr = plan.zcr_batch(y, off, ln, flags=flags)
        return {
            "mfcc": np.vstack([fr["mfcc"], fr["mfcc_delta"], fr["mfcc_delta2"]]),
            "f0": f0["f0_flat"][:T].copy(),
            "energy": fr["rms"][0].copy(),
            "zcr": zcr["zcr_flat"][:T].copy(),
        }

    # ------------------------------------------------------------------ sibling frame features
    def _spectral_plan(self) -> _native.Plan:
        """librosa's defaults for the spectral descriptors: n_fft 2048, hop 512, Hann -- a plan of its own."""
        return self._cached_plan(self._devices()[0], "spectral",
                                 lambda: _native.make_params(self.sr, 2048, 512, 13, 128, "hann", self.pre_emphasis))

    def extract_spectral_frames(self, y: np.ndarray) -> Dict[str, np.ndarray]:
        """Frame-level ``librosa.feature.spectral_centroid / spectral_bandwidth / spectral_rolloff / spectral_contrast`` of
        a signal at librosa's defaults, as the reference's experiment extractor calls them
        (04_feature_extraction_experiment/feature_extractor.py:497-506): STFT, moments, roll-off search and the band
        extremes of the contrast on the GPU; the contrast's dB difference with its clip-global ``top_db`` on the host."""
        out = self._spectral_plan().spectral_batch(*_one_clip(y))
        if out["status"][0] != _native.CLIP_OK:
            raise _status_error(int(out["status"][0]), "extract_spectral_features")
        d = out["clips"][0]

        def power_to_db(S):            # librosa.power_to_db(ref=1.0, amin=1e-10, top_db=80.0) of the whole matrix
            L = 10.0 * np.log10(np.maximum(1e-10, S.astype(np.float64)))
            return np.maximum(L, L.max() - 80.0)
        return {"spectral_centroid": d["centroid"], "spectral_bandwidth": d["bandwidth"], "spectral_rolloff": d["rolloff"],
                "spectral_contrast": power_to_db(d["peak"]) - power_to_db(d["valley"])}

    def extract_spectral_features(self, y: np.ndarray) -> Dict[str, Any]:
        """提取頻譜特徵: the eight statistics of 04_feature_extraction_experiment/feature_extractor.py:509-518."""
        f = self.extract_spectral_frames(y)
        out: Dict[str, Any] = {}
        for k in ("spectral_centroid", "spectral_bandwidth", "spectral_rolloff", "spectral_contrast"):
            out[k + "_mean"] = float(np.mean(f[k]))
            out[k + "_std"] = float(np.std(f[k]))
        return out

    _HARMONIC_KEYS = ("harmonic_energy", "harmonic_ratio", "harmonic_freq_mean", "harmonic_freq_std")

    def extract_harmonic_features_batch(self, signals: Sequence[np.ndarray]) -> List[Dict[str, Any]]:
        """``extract_harmonic_features`` of many signals in one device pass (a failing clip raises)."""
        ys = [np.ascontiguousarray(y, dtype=np.float32) for y in signals]
        if not ys:
            return []
        for y in ys:
            if y.ndim != 1:
                raise ValueError(f"signals must be 1-D (mono), got shape {y.shape}")
        lengths = np.array([y.size for y in ys], np.int64)
        out = self._spectral_plan().hpss_batch(np.concatenate(ys), _native.packed_offsets(lengths), lengths, want_harm=False)
        res = []
        for i, st in enumerate(out["status"]):
            if st != _native.CLIP_OK:
                raise _status_error(int(st), "extract_harmonic_features")
            eh, ey, fm, fs = (float(v) for v in out["stats"][i])
            res.append(dict(zip(self._HARMONIC_KEYS, (eh, eh / (ey + 1e-8), fm, fs))))
        return res

    def extract_harmonic_features(self, y: np.ndarray) -> Dict[str, Any]:
        """提取諧波特徵 (04_feature_extraction_experiment/feature_extractor.py:525-556): the energy of
        ``librosa.effects.harmonic(y)``, its ratio to the energy of ``y`` and the mean / std of the harmonic signal's
        spectral centroid, all on the GPU."""
        return self.extract_harmonic_features_batch([y])[0]

    _TIMBRE_KEYS = ("mel_energy_mean", "mel_energy_std", "chroma_mean", "chroma_std", "mfcc_mean", "mfcc_std")

    def extract_timbre_features_batch(self, signals: Sequence[np.ndarray]) -> List[Dict[str, Any]]:
        """``extract_timbre_features`` of many signals in two device passes (a failing clip raises)."""
        ys = [np.ascontiguousarray(y, dtype=np.float32) for y in signals]
        if not ys:
            return []
        for y in ys:
            if y.ndim != 1:
                raise ValueError(f"signals must be 1-D (mono), got shape {y.shape}")
            if y.size < 4096:
                raise ValueError(f"extract_timbre_features needs at least 4096 samples (nine frames), got {y.size}")
        lengths = np.array([y.size for y in ys], np.int64)
        packed, offsets = np.concatenate(ys), _native.packed_offsets(lengths)
        plan = self._spectral_plan()
        out = plan.chroma_batch(packed, offsets, lengths, want_chroma=False)
        mf = plan.extract_batch(packed, offsets, lengths, flags=0)
        K = 13
        res = []
        for i in range(len(ys)):
            for st in (out["status"][i], mf["status"][i]):
                if st != _native.CLIP_OK:
                    raise _status_error(int(st), "extract_timbre_features", int(mf["nframes"][i]))
            # the MFCC rows share T: the matrix mean is the mean of the row means, its variance the mean of the rows'
            # second moments less that mean squared
            m, sd = mf["stats"][i][:K].astype(np.float64), mf["stats"][i][K:2 * K].astype(np.float64)
            mean = float(np.mean(m))
            var = float(np.mean(sd * sd + m * m)) - mean * mean
            vals = [float(v) for v in out["stats"][i]] + [mean, float(np.sqrt(max(var, 0.0)))]
            res.append(dict(zip(self._TIMBRE_KEYS, vals)))
        return res

    def extract_timbre_features(self, y: np.ndarray) -> Dict[str, Any]:
        """提取音色特徵 (04_feature_extraction_experiment/feature_extractor.py:558-590): mean and std of
        ``librosa.feature.melspectrogram``, of ``librosa.feature.chroma_stft`` (tuning estimated, as librosa does) and of
        ``librosa.feature.mfcc(n_mfcc=13)``, all at librosa's defaults and on the GPU; the signal is taken as given.  The
        MFCC statistics come from the extract pass, which needs nine frames: a signal under 4096 samples raises
        ``ValueError`` (``feature.chroma_stft`` / ``feature.melspectrogram`` work from one sample up)."""
        return self.extract_timbre_features_batch([y])[0]

    _RHYTHM_KEYS = ("tempo", "rhythm_regularity", "onset_strength_mean", "onset_strength_std")

    def extract_rhythm_features_batch(self, signals: Sequence[np.ndarray]) -> List[Dict[str, Any]]:
        """``extract_rhythm_features`` of many signals in one device pass (a failing clip raises)."""
        ys = [np.ascontiguousarray(y, dtype=np.float32) for y in signals]
        if not ys:
            return []
        for y in ys:
            if y.ndim != 1:
                raise ValueError(f"signals must be 1-D (mono), got shape {y.shape}")
        lengths = np.array([y.size for y in ys], np.int64)
        out = self._spectral_plan().rhythm_batch(np.concatenate(ys), _native.packed_offsets(lengths), lengths, want_env=False)
        res = []
        for i, st in enumerate(out["status"]):
            if st != _native.CLIP_OK:
                raise _status_error(int(st), "extract_rhythm_features")
            mean, std = (float(v) for v in out["stats"][i])
            res.append(dict(zip(self._RHYTHM_KEYS, (float(out["tempo"][i]), std / (mean + 1e-8), mean, std))))
        return res

    def extract_rhythm_features(self, y: np.ndarray) -> Dict[str, Any]:
        """提取節奏特徵 (04_feature_extraction_experiment/feature_extractor.py:592-622): the tempo
        ``librosa.beat.beat_track`` reports for ``librosa.onset.onset_strength(y)`` (the beat positions, which the reference
        discards, are ``extract_beats``'), the mean and std of that envelope and their ratio, all at librosa's defaults and on
        the GPU; the signal is taken as given and may be as short as one sample (tempo 0.0 up to three frames)."""
        return self.extract_rhythm_features_batch([y])[0]

    _BEAT_KEYS = ("tempo", "beat_frames", "beat_times", "beat_count", "beat_interval_mean", "beat_interval_std")

    def extract_beats_batch(self, signals: Sequence[np.ndarray]) -> List[Dict[str, Any]]:
        """``extract_beats`` of many signals in one device pass (a failing clip raises)."""
        ys = [np.ascontiguousarray(y, dtype=np.float32) for y in signals]
        if not ys:
            return []
        for y in ys:
            if y.ndim != 1:
                raise ValueError(f"signals must be 1-D (mono), got shape {y.shape}")
        lengths = np.array([y.size for y in ys], np.int64)
        plan = self._spectral_plan()
        out = plan.beat_batch(np.concatenate(ys), _native.packed_offsets(lengths), lengths)
        spf = 512.0 / float(plan.params.sr)                # seconds per frame
        res = []
        for i, st in enumerate(out["status"]):
            if st != _native.CLIP_OK:
                raise _status_error(int(st), "extract_beats")
            frames = out["beats"][i]
            gaps = np.diff(frames).astype(np.float64) * spf
            few = frames.size < 2
            res.append(dict(zip(self._BEAT_KEYS, (float(out["tempo"][i]), [int(f) for f in frames], [float(f) * spf for f in frames],
                                                   int(frames.size), float("nan") if few else float(np.mean(gaps)),
                                                   float("nan") if few else float(np.std(gaps))))))
        return res

    def extract_beats(self, y: np.ndarray) -> Dict[str, Any]:
        """The beat positions ``librosa.beat.beat_track(onset_envelope=librosa.onset.onset_strength(y), sr=sr)`` finds -- the
        second half of the call whose tempo ``extract_rhythm_features`` reports -- on the GPU: ``tempo``, ``beat_frames``
        (hop 512), ``beat_times`` (seconds), ``beat_count`` and the mean and std (ddof 0) of the inter-beat interval in seconds
        (NaN below two beats), as Python floats, ints and lists."""
        return self.extract_beats_batch([y])[0]

    _SPECTRAL_KEYS = tuple(f"spectral_{k}_{s}" for k in ("centroid", "bandwidth", "rolloff", "contrast") for s in ("mean", "std"))
    _SIGNAL_GROUPS = ("spectral", "harmonic", "timbre", "rhythm")       # the reference's order in extract_all_features

    @classmethod
    def _group_bits(cls, groups: Sequence[str]) -> int:
        if isinstance(groups, str):
            groups = (groups,)
        bits = 0
        for g in groups:
            if g not in cls._SIGNAL_GROUPS:
                raise ValueError(f"unknown feature group {g!r}: expected some of {cls._SIGNAL_GROUPS}")
            bits |= 1 << cls._SIGNAL_GROUPS.index(g)
        if not bits:
            raise ValueError(f"no feature group asked for: expected some of {cls._SIGNAL_GROUPS}")
        return bits

    def _signal_dict(self, bits: int, s: np.ndarray) -> Dict[str, Any]:
        """One clip's record of afx_groups_batch as the merged dict, the asked groups in the reference's order."""
        out: Dict[str, Any] = {}
        if bits & _native.GROUP_SPECTRAL:
            out.update(zip(self._SPECTRAL_KEYS, (float(v) for v in s[0:8])))
        if bits & _native.GROUP_HARMONIC:
            eh, ey, fm, fs = (float(v) for v in s[8:12])
            out.update(zip(self._HARMONIC_KEYS, (eh, eh / (ey + 1e-8), fm, fs)))
        if bits & _native.GROUP_TIMBRE:
            out.update(zip(self._TIMBRE_KEYS, (float(v) for v in s[12:18])))
        if bits & _native.GROUP_RHYTHM:
            tempo, mean, std = (float(v) for v in s[18:21])
            out.update(zip(self._RHYTHM_KEYS, (tempo, std / (mean + 1e-8), mean, std)))
        return out

    def _signal_features(self, signals: Sequence[np.ndarray], preprocess: bool, groups: Sequence[str]):
        bits = self._group_bits(groups)
        ys = [np.ascontiguousarray(y, dtype=np.float32) for y in signals]
        for y in ys:
            if y.ndim != 1:
                raise ValueError(f"signals must be 1-D (mono), got shape {y.shape}")
        if not ys:
            return bits, None
        lengths = np.array([y.size for y in ys], np.int64)
        return bits, self._spectral_plan().groups_batch(np.concatenate(ys), _native.packed_offsets(lengths), lengths,
                                                        groups=bits, preprocess=bool(preprocess))

    def extract_signal_features_batch(self, signals: Sequence[np.ndarray], *, preprocess: bool = True,
                                      groups: Sequence[str] = _SIGNAL_GROUPS) -> List[Optional[Dict[str, Any]]]:
        """What the experiment extractor's ``extract_all_features`` computes per file from the signal
        (04_feature_extraction_experiment/feature_extractor.py:624-687): its ``preprocess_audio`` and the spectral,
        harmonic, timbre and rhythm groups, for many signals in one device pass -- one upload, one STFT, scalars back.
        ``groups``: which of the four to compute; the dict holds their keys in the reference's order.  ``preprocess``
        False takes the signals as given.  ``None`` for a clip the reference returns None for (its preprocess fails: 18
        samples or fewer, or a NaN / inf sample; without the preprocess, an empty or non-finite clip)."""
        bits, out = self._signal_features(signals, preprocess, groups)
        if out is None:
            return []
        return [self._signal_dict(bits, out["stats"][i]) if st == _native.CLIP_OK else None
                for i, st in enumerate(out["status"])]

    def extract_signal_features(self, y: np.ndarray, *, preprocess: bool = True,
                                groups: Sequence[str] = _SIGNAL_GROUPS) -> Dict[str, Any]:
        """``extract_signal_features_batch`` of one signal; raises ``ValueError`` where that gives ``None``."""
        bits, out = self._signal_features([y], preprocess, groups)
        if out["status"][0] != _native.CLIP_OK:
            raise _status_error(int(out["status"][0]), "extract_signal_features", int(np.size(y)))
        return self._signal_dict(bits, out["stats"][0])

    def extract_signal_features_files(self, paths: Sequence[str], *, preprocess: bool = True,
                                      groups: Sequence[str] = _SIGNAL_GROUPS) -> List[Optional[Dict[str, Any]]]:
        """``extract_signal_features_batch`` of WAV files loaded at this extractor's ``sr`` (``wavio.load_batch``), each dict
        with the file's ``filename`` added, as the reference's ``extract_all_features`` adds it."""
        import os
        paths = [str(p) for p in paths]
        res = self.extract_signal_features_batch([y for y, _ in wavio.load_batch(paths, sr=self.sr)],
                                                 preprocess=preprocess, groups=groups)
        for p, d in zip(paths, res):
            if d is not None:
                d["filename"] = os.path.basename(p)
        return res

    # ------------------------------------------------------------------ the experiment's energy and ZCR groups
    _ENERGY_KEYS = ("energy_mean", "energy_std", "energy_cv", "energy_snr", "energy_range_valid", "energy_stability",
                    "energy_snr_valid", "energy_quality_score")
    _ZCR_KEYS = ("zcr_mean", "zcr_std", "zcr_cv", "zcr_local_stability", "zcr_range_valid", "zcr_stability",
                 "zcr_local_stable", "zcr_quality_score")

    @classmethod
    def _energy_dict(cls, rec: np.ndarray) -> Dict[str, Any]:
        """The energy group's dict from a record of afx_energy_zcr_batch: thresholds and score of
        04_feature_extraction_experiment/feature_extractor.py:367-399."""
        i = _native.EZ_FIELDS.index
        mean, std, floor = float(rec[i("energy_mean")]), float(rec[i("energy_std")]), float(rec[i("energy_p10")])
        cv = std / mean if mean != 0 else float("inf")
        snr = 20 * float(np.log10(mean / floor)) if floor > 0 else 0
        range_valid = bool(5.67e-03 <= mean <= 2.62e+00)
        stability = bool(cv <= 0.3)
        snr_valid = bool(snr >= 20)
        score = 1.0
        for ok in (range_valid, stability, snr_valid):
            if not ok:
                score -= 0.3
        return dict(zip(cls._ENERGY_KEYS, (mean, std, cv, snr, range_valid, stability, snr_valid, max(0.0, score))))

    @classmethod
    def _zcr_dict(cls, rec: np.ndarray) -> Dict[str, Any]:
        """The ZCR group's dict from a record of afx_energy_zcr_batch: thresholds and score of :444-480."""
        i = _native.EZ_FIELDS.index
        mean, std, local = float(rec[i("zcr_mean")]), float(rec[i("zcr_std")]), float(rec[i("zcr_local_stability")])
        cv = std / mean if mean != 0 else float("inf")
        range_valid = bool(0.034 <= mean <= 0.491)
        stability = bool(cv <= 0.35)
        local_stable = bool(local <= 0.1)
        score = 1.0
        for ok, cost in ((range_valid, 0.4), (stability, 0.3), (local_stable, 0.3)):
            if not ok:
                score -= cost
        return dict(zip(cls._ZCR_KEYS, (mean, std, cv, local, range_valid, stability, local_stable, max(0.0, score))))

    @classmethod
    def _energy_zcr_dicts(cls, flags: int, rec: np.ndarray, status: np.ndarray) -> List[Optional[Dict[str, Any]]]:
        out: List[Optional[Dict[str, Any]]] = []
        for r, st in zip(rec, status):
            if st != _native.CLIP_OK:
                out.append(None)
                continue
            d: Dict[str, Any] = {}
            if flags & _native.EZ_ENERGY:
                d.update(cls._energy_dict(r))
            if flags & _native.EZ_ZCR:
                d.update(cls._zcr_dict(r))
            out.append(d)
        return out

    def _energy_zcr(self, signals: Sequence[np.ndarray], flags: int, frame_length: int, hop_length: int):
        ys = [np.ascontiguousarray(y, dtype=np.float32) for y in signals]
        for y in ys:
            if y.ndim != 1:
                raise ValueError(f"signals must be 1-D (mono), got shape {y.shape}")
        if frame_length < 64 or frame_length > 2048 or frame_length & (frame_length - 1):
            raise ValueError("frame_length must be a power of two in [64, 2048]")
        if hop_length < 1:
            raise ValueError("hop_length must be positive")
        if not ys:
            return None
        from .. import filters
        lengths = np.array([y.size for y in ys], np.int64)
        return filters._ctx(self._devices()[0]).energy_zcr_batch(np.concatenate(ys), _native.packed_offsets(lengths), lengths,
                                                                 self.sr, frame_length, hop_length, flags)

    def extract_energy_zcr_features_batch(self, signals: Sequence[np.ndarray], *, preprocess: bool = True,
                                          frame_length: int = 2048, hop_length: int = 512) -> List[Optional[Dict[str, Any]]]:
        """The energy group (04_feature_extraction_experiment/feature_extractor.py:341-403) and the ZCR group (:405-483) of
        the experiment extractor for many signals at this extractor's ``sr`` in one device pass: its ``preprocess_audio``,
        ``librosa.feature.rms``, and ``medfilt(3)`` -> ``savgol_filter(11, 3)`` -> peak normalisation ->
        ``zero_crossing_rate``; one upload, scalars back.  ``frame_length`` / ``hop_length`` default to that class's 2048 /
        512 and are adjusted per clip as its ``_adjust_frame_length`` does.  The dict holds the reference's sixteen keys,
        energy first.  ``None`` for a clip the reference returns None for (18 samples or fewer, or a NaN / inf sample;
        without the preprocess, an empty or non-finite clip)."""
        flags = _native.EZ_ENERGY | _native.EZ_ZCR | (_native.EZ_PREPROCESS if preprocess else 0)
        out = self._energy_zcr(signals, flags, frame_length, hop_length)
        return [] if out is None else self._energy_zcr_dicts(flags, out["rec"], out["status"])

    def _one_energy_zcr(self, y: np.ndarray, group: int, what: str) -> Dict[str, Any]:
        flags = group | _native.EZ_PREPROCESS
        out = self._energy_zcr([y], flags, 2048, 512)
        if out["status"][0] == _native.CLIP_TOO_SHORT:           # what the reference's filtfilt raises and its caller logs
            raise ValueError(f"The length of the input vector x must be greater than padlen, which is 18. ({what})")
        if out["status"][0] != _native.CLIP_OK:
            raise _status_error(int(out["status"][0]), what, int(np.size(y)))
        return self._energy_zcr_dicts(flags, out["rec"], out["status"])[0]

    def extract_energy_features(self, y: np.ndarray) -> Dict[str, Any]:
        """The experiment extractor's ``extract_energy`` (:341-403) of one signal, its preprocess included; raises
        ``ValueError`` where the reference returns None."""
        return self._one_energy_zcr(y, _native.EZ_ENERGY, "extract_energy_features")

    def extract_zcr_features(self, y: np.ndarray) -> Dict[str, Any]:
        """The experiment extractor's ``extract_zcr`` (:405-483) of one signal, its preprocess included; raises
        ``ValueError`` where the reference returns None."""
        return self._one_energy_zcr(y, _native.EZ_ZCR, "extract_zcr_features")

    def preprocess_experiment_batch(self, signals: Sequence[np.ndarray]) -> List[Optional[np.ndarray]]:
        """``preprocess_experiment`` of many signals in one device pass; ``None`` for a clip the reference's
        ``preprocess_audio`` returns None for (18 samples or fewer, or not finite)."""
        from .. import filters
        return filters.preprocess_experiment_batch(signals, self.sr, device=self._devices()[0])

    def preprocess_experiment(self, y: np.ndarray) -> np.ndarray:
        """音頻預處理：降噪和正規化 (04_feature_extraction_experiment/feature_extractor.py:133-154), the stage that experiment
        class runs ahead of every feature group: peak normalisation, pre-emphasis 0.98, a 5th-order Butterworth high-pass at
        200 Hz applied forward and backward (``scipy.signal.filtfilt``), peak normalisation, at this extractor's ``sr`` and on
        the GPU.  float32 (the reference's float64 result rounded once).  Where the reference logs and returns None -- a
        signal of 18 samples or fewer, a NaN / inf sample -- this raises ``ValueError``."""
        from .. import filters
        y = np.asarray(y)
        out = filters._preprocess_experiment([y], self.sr, self._devices()[0])
        if out["status"][0] != _native.CLIP_OK:
            raise _status_error(int(out["status"][0]), "preprocess_experiment", int(y.size))
        return out["clips"][0]

    def normalize_volume_batch(self, signals: Sequence[np.ndarray], reference_level: float = -23.0) -> List[np.ndarray]:
        """``normalize_volume`` of many signals in one device pass (``loudness.normalize_batch`` at this extractor's ``sr``)."""
        from .. import loudness
        return loudness.normalize_batch(signals, self.sr, reference_level, device=self._devices()[0])[0]

    def normalize_volume(self, y: np.ndarray, reference_level: float = -23.0) -> np.ndarray:
        """音量正規化 (04_feature_extraction_experiment/process_audio.py:134-147): the BS.1770 integrated loudness of ``y`` at
        this extractor's ``sr`` brought to ``reference_level`` LUFS (config/experiment_config.yaml:26), measured and scaled on
        the GPU; float32.  Audio shorter than a gating block (0.4 s) comes back unchanged, as the reference's does when
        pyloudnorm raises; so does audio without a level (silence)."""
        return self.normalize_volume_batch([y], reference_level)[0]

    # config/experiment_config.yaml:15-22
    _NR_WIENER = dict(stationary=True, prop_decrease=0.95)
    _NR_SPECTRAL = dict(n_fft=2048, win_length=2048, hop_length=512)

    def _nr_keywords(self, method: str, kw: dict) -> dict:
        if method not in ("wiener", "spectral"):
            raise ValueError(f"method={method!r} is not supported ('wiener' or 'spectral')")
        return {**(self._NR_WIENER if method == "wiener" else self._NR_SPECTRAL), **kw}

    def apply_noise_reduction_batch(self, signals: Sequence[np.ndarray], method: str = "wiener", **kw) -> List[np.ndarray]:
        """``apply_noise_reduction`` of many signals in one device pass."""
        from .. import effects
        return effects.reduce_noise_batch(signals, self.sr, device=lambda: self._devices()[0], **self._nr_keywords(method, kw))

    def apply_noise_reduction(self, y: np.ndarray, method: str = "wiener", **kw) -> np.ndarray:
        """應用降噪處理 (04_feature_extraction_experiment/process_audio.py:82-98): ``noisereduce.reduce_noise`` at this
        extractor's ``sr`` and on the GPU, with the configuration's values as defaults -- ``method="wiener"``: stationary
        gating with ``prop_decrease=0.95`` at noisereduce's 1024 / 256 frames; ``"spectral"``: non-stationary gating at
        2048 / 2048 / 512.  Further keywords are noisereduce's.  float32 of ``y``'s length."""
        return self.apply_noise_reduction_batch([y], method, **kw)[0]

    def stretch_to_length_batch(self, signals: Sequence[np.ndarray], n_samples, **kw) -> List[Optional[np.ndarray]]:
        """``stretch_to_length`` of many signals in one device pass; ``n_samples``: one length for all, or one per signal.
        None for a signal the transform refuses (empty, not finite)."""
        from .. import effects
        signals = [np.asarray(s) for s in signals]
        lengths = [n_samples] * len(signals) if np.isscalar(n_samples) else list(n_samples)
        if len(lengths) != len(signals) or any(int(n) < 1 for n in lengths):
            raise ValueError("n_samples must be at least 1, one per signal or one for all")
        # istft's length is round(len / rate): len / (len / n) is n to a few parts in 2^52, far from a half
        rates = [max(s.size, 1) / int(n) for s, n in zip(signals, lengths)]
        return effects.time_stretch_batch(signals, rates, device=lambda: self._devices()[0], **kw)

    def stretch_to_length(self, y: np.ndarray, n_samples: int, **kw) -> np.ndarray:
        """``y`` brought to exactly ``n_samples`` samples without a change of pitch -- what puts a student take on a
        teacher's clock before the two are compared: ``librosa.effects.time_stretch`` at ``rate = len(y) / n_samples`` on the
        GPU, with ``n_samples`` taken as istft's ``length``.  Further keywords are time_stretch's (n_fft 2048 or 1024,
        hop_length, window, pad_mode); float32."""
        out, = self.stretch_to_length_batch([y], [int(n_samples)], **kw)
        if out is None:
            raise ValueError("stretch_to_length: y is too short for this framing or not finite everywhere")
        return out

    def process_recordings_batch(self, signals: Sequence[np.ndarray], method: str = "wiener", reference_level: float = -23.0,
                                 **kw) -> Tuple[List[np.ndarray], List[Optional[float]]]:
        """The conditioning of 04_feature_extraction_experiment/process_audio.py:28-61 without its VAD: ``normalize_volume``
        then ``apply_noise_reduction``, the normalised samples staying on the device between the two.  Returns the denoised
        signals (what the reference writes to disk) and, per signal, the integrated loudness of the *normalised* signal as
        the reference reports it -- ``None`` where its meter raises ``ValueError`` (shorter than a gating block) and for a
        signal that is not finite."""
        from .. import effects, loudness
        opts = effects._gate_opts(self.sr, self._nr_keywords(method, dict(kw)))
        sig = effects._gate_signals([loudness._as_clip(s, f"signal {i}") for i, s in enumerate(signals)], opts,
                                    "process_recordings_batch")
        if not sig:
            return [], []
        ctx = effects._ctx(self._devices()[0])
        buf, offsets, lengths = loudness._pack(sig)
        dev = _native.DeviceBuffer(ctx, max(4 * buf.size, 4))
        try:
            norm = ctx.loudness_batch(buf, offsets, lengths, self.sr, 0.400, _native.LOUD_NORM_LOUDNESS, float(reference_level),
                                      out=dev, out_offsets=offsets)
            for i in np.flatnonzero(norm["status"] != _native.CLIP_OK):   # the reference keeps such audio as it is
                dev.upload(sig[i], 4 * int(offsets[i]))
            meas = ctx.loudness_batch(dev, offsets, lengths, self.sr, 0.400, _native.LOUD_MEASURE, fmt=_native.FMT_F32)
            out = ctx.gate_batch(dev, offsets, lengths, opts, fmt=_native.FMT_F32)
        finally:
            dev.free()
        ys = [out["out"][o:o + n].copy() for o, n in zip(out["offsets"], lengths)]
        ls = [float(r[0]) if st == _native.CLIP_OK else None for r, st in zip(meas["rec"], meas["status"])]
        return ys, ls

    def preprocess_alignment_batch(self, signals: Sequence[np.ndarray]) -> List[Optional[np.ndarray]]:
        """``preprocess_alignment`` of many signals in one device pass; ``None`` for a clip of fewer than 512 samples or with
        a NaN / inf sample."""
        from .. import effects
        return effects.preprocess_alignment_batch(signals, self.sr, device=self._devices()[0])

    def preprocess_alignment(self, y: np.ndarray) -> np.ndarray:
        """The conditioning 05_dtw_alignment_experiment/process_audio.py:13-51 gives a recording before the DTW aligner sees
        it -- gain to RMS 0.1, spectral subtraction of the noise profile of the first ten frames, an energy VAD that zeroes
        what lies outside its speech frames -- at this extractor's ``sr`` and on the GPU (``effects.preprocess_alignment``)."""
        from .. import effects
        return effects.preprocess_alignment(y, self.sr, device=self._devices()[0])

    @staticmethod
    def save_frame_features(features: Dict[str, np.ndarray], npz_path: str) -> None:
        """``np.savez(npz_path, **features)`` -- the reference's on-disk schema for frame-level features."""
        np.savez(npz_path, **features)

    # ------------------------------------------------------------------ alignment (05_dtw_alignment_experiment)
    def _frames_of(self, paths: Sequence[str], stack_deltas: bool) -> Dict[str, np.ndarray]:
        """(features, frames) MFCC matrices of the given files: ``.npz`` files written by ``save_frame_features`` are read
        (``npz['mfcc']``), ``.wav`` files go through one ``extract_batch(want_frames=True)`` pass on the GPU."""
        out: Dict[str, np.ndarray] = {}
        wavs = []
        K = self.n_mfcc
        for p in dict.fromkeys(str(q) for q in paths):
            if p.lower().endswith(".npz"):
                with np.load(p, allow_pickle=False) as z:
                    m = np.asarray(z["mfcc"], np.float32)
                out[p] = m if stack_deltas or m.shape[0] != 3 * K else m[:K]
            else:
                wavs.append(p)
        if wavs:
            ys = [np.ascontiguousarray(self.load_audio(p)[0], np.float32) for p in wavs]
            lengths = np.array([y.size for y in ys], np.int64)
            res = self._plan().extract_batch(np.concatenate(ys), _native.packed_offsets(lengths), lengths,
                                             flags=_native.FLAG_PREEMPH | _native.FLAG_TRIM, want_frames=True)
            for i, p in enumerate(wavs):
                st = int(res["status"][i])
                if st != _native.CLIP_OK:
                    raise _status_error(st, f"align: {p}", int(res["nframes"][i]))
                fr = res["frames"][i]
                rows = [fr["mfcc"], fr["mfcc_delta"], fr["mfcc_delta2"]] if stack_deltas else [fr["mfcc"]]
                out[p] = np.ascontiguousarray(np.vstack(rows), np.float32)
        return out

    @staticmethod
    def _alignment(teacher: str, student: str, cost: float, wp: np.ndarray) -> Dict[str, Any]:
        return {"teacher_path": teacher, "student_path": student, "dtw_distance": float(cost),
                "normalized_distance": float(cost) / len(wp), "path": wp}

    def align_files(self, teacher: str, student: str, *, stack_deltas: bool = True, **dtw_kwargs) -> Dict[str, Any]:
        """DTW alignment of a student's utterance to a teacher's, the step the reference's aligner runs
        (05_dtw_alignment_experiment/dtw_alignment.py:1206-1250 loads ``npz['mfcc']``, :930-970 aligns it).
        ``teacher`` / ``student``: ``.wav`` files (MFCC, with ``stack_deltas`` + delta + delta2, computed on the GPU) or
        ``.npz`` files written by ``save_frame_features``.  ``dtw_kwargs`` go to ``sequence.dtw`` (metric,
        global_constraints, band_rad, and librosa's step_sizes_sigma, weights_add, weights_mul, subseq).  Returns
        teacher_path, student_path, dtw_distance, normalized_distance (distance over path length) and path (L x 2, teacher
        frame, student frame, end to start).  With ``subseq=True`` the shorter of the two is matched inside the longer --
        a teacher utterance inside a student's take with lead-in and trailing noise: dtw_distance is the cost of that
        match (the minimum of D's last row), the path covers only the matched span of the longer file, and
        normalized_distance is still that cost over that path's length, so surplus frames no longer inflate either."""
        from .. import sequence
        f = self._frames_of([teacher, student], stack_deltas)
        cost, wp = sequence.dtw(f[str(teacher)], f[str(student)], **dtw_kwargs)
        return self._alignment(teacher, student, cost, wp)

    def align_batch(self, pairs: Sequence[Tuple[str, str]], *, stack_deltas: bool = True,
                    **dtw_kwargs) -> List[Optional[Dict[str, Any]]]:
        """``align_files`` of many (teacher, student) pairs: every distinct file is extracted once (one GPU pass for the
        ``.wav`` files) and all pairs are aligned in one ``sequence.dtw_batch`` call.  ``dtw_kwargs`` as in
        ``align_files`` (the step arguments hold for every pair).  The list is aligned with ``pairs``; a pair that fails
        is logged and None."""
        from .. import sequence
        f = self._frames_of([p for pr in pairs for p in pr], stack_deltas)
        res = sequence.dtw_batch([(f[str(t)], f[str(s)]) for t, s in pairs], **dtw_kwargs)
        return [None if r is None else self._alignment(t, s, r[0], r[1]) for (t, s), r in zip(pairs, res)]

    def batch_process(self, audio_dir: str, *, features_to_extract: Optional[Sequence[str]] = None) -> List[Dict[str, Any]]:
        """批量處理音頻文件 (feature_extractor.py:215-237): every ``*.wav`` directly inside
        ``audio_dir`` in glob order; a failing file is logged and left out.  Files are
        sharded over the visible GPUs (no inter-GPU traffic; see parallel.py).
        ``features_to_extract``: as for ``extract_features``."""
        from ..parallel import normalize_features, process_files
        normalize_features(features_to_extract)            # a bad request fails the call, not every file
        files = list(Path(audio_dir).glob("*.wav"))
        if not self._uses_reference_stages():
            results = []
            for audio_file in files:
                try:
                    results.append(self.extract_features(str(audio_file), features_to_extract=features_to_extract))
                    self.logger.info(f"成功處理文件: {audio_file.name}")
                except Exception as e:
                    self.logger.error(f"處理文件 {audio_file.name} 失敗: {str(e)}")
                    continue
            return results
        return process_files(self, files, features_to_extract=features_to_extract)
