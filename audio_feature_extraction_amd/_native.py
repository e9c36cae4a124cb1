"""ctypes binding of libafx.so (include/afx.h).  The product path has no CPU
fallback: if the HIP library is missing or no GPU is visible, calls fail loudly."""
from __future__ import annotations

import ctypes as C
import weakref
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# AFX_LIB: developer override used to A/B two builds of the library on the same GPU box
LIB_PATH = os.environ.get("AFX_LIB") or os.path.join(_HERE, "libafx.so")

AFX_OK = 0
CLIP_OK, CLIP_TOO_SHORT, CLIP_NONFINITE = 0, 1, 2
WINDOW_HAMMING, WINDOW_HANN = 0, 1
FMT_F32, FMT_S16 = 0, 1
MEM_HOST, MEM_DEVICE = 0, 1
FLAG_PREEMPH, FLAG_TRIM = 1, 2
DTW_OK, DTW_NONFINITE, DTW_NO_PATH = 0, 1, 2
DTW_METRICS = {"euclidean": 0, "sqeuclidean": 1, "cosine": 2}
DTW_BACKTRACK, DTW_STORE_D, DTW_SUBSEQ = 1, 2, 4
DTW_MAX_STEPS, DTW_MAX_STEP = 5, 2       # afx_dtw_steps_batch: custom steps per list, and the largest component of one
DTW_MAX_DIM = 128
HPSS_STORE_SPEC = 4
HPSS_BINS = 1025
CHROMA_STORE_HIST = 8
CHROMA_HIST = 102            # per clip: peaks, kept, counts[100]
TEMPO_MAX_WIN = 768          # lags of the tempogram window afx_rhythm_batch holds (sr <= 49215 at hop 512)
SMP_U8, SMP_S16, SMP_S24, SMP_S32, SMP_F32, SMP_F64 = range(6)
SMP_KINDS = {"u8": SMP_U8, "s16": SMP_S16, "s24": SMP_S24, "s32": SMP_S32, "f32": SMP_F32, "f64": SMP_F64}     # wavio's kind names
SMP_BYTES = np.array([1, 2, 3, 4, 4, 8], np.int64)
SMP_OF_WAV = {(1, 8): SMP_U8, (1, 16): SMP_S16, (1, 24): SMP_S24, (1, 32): SMP_S32, (3, 32): SMP_F32, (3, 64): SMP_F64}   # (tag, bits)
DECODE_MAX_CHANNELS = 7
FILT_PLAIN, FILT_EXPERIMENT = 0, 1
GROUP_SPECTRAL, GROUP_HARMONIC, GROUP_TIMBRE, GROUP_RHYTHM = 1, 2, 4, 8     # afx_groups_batch: the groups asked for
GROUP_ALL = 15
GROUPS_PREPROCESS, GROUPS_STORE_DESC = 16, 32                                # its flags, beside FLAG_PREEMPH
BEAT_INPUT_ENVELOPE = 64                                                     # afx_beat_batch: the clips are onset envelopes
DENOISE_SPECSUB, DENOISE_WIENER = 0, 1                                       # afx_denoise_batch: its modes
DENOISE_RMS_GAIN, DENOISE_VAD = 128, 256                                     # its flags, beside FLAG_PREEMPH
DENOISE_MAX_NOISE_FRAMES = 64
BEAT_MAX_FPB = 768                                                           # frames per beat it holds
ASSESS_N, COMPARE_N = 10, 10                                                 # doubles per record of afx_assess_batch / afx_compare_batch
ASSESS_FIELDS = ("n_short", "silent", "longest_run", "max_rms_short", "mean_square", "peak", "noise_mean_square",
                 "n_long", "rms_long_mean", "rms_long_std")
COMPARE_FIELDS = ("n", "sum_r", "sum_d", "sum_rr", "sum_dd", "sum_rd", "sum_ee", "m2_r", "m2_d", "m2_rd")
COST_ASSESS, COST_COMPARE = 0, 1                                             # afx_assess_cost: whose record
SPECDIST_N = 4                                                               # doubles per record of afx_specdist_batch
SPECDIST_FIELDS = ("n", "sum_dist", "sum_rr", "sum_dd")
CFFT_MAX_N = 1 << 21                                                         # samples of a clip the device transforms
EZ_PREPROCESS, EZ_ENERGY, EZ_ZCR = 1, 2, 4                                    # afx_energy_zcr_batch: its flags
EZ_N = 12                                                                    # doubles per clip of its record
EZ_FIELDS = ("T", "fl", "hop", "energy_mean", "energy_std", "energy_p10", "zcr_mean", "zcr_std", "zcr_local_stability",
             "peak_smooth", "peak_in", "peak_filt")
LOUD_MEASURE, LOUD_NORM_LOUDNESS, LOUD_NORM_PEAK = 0, 1, 2                    # afx_loudness_batch: its modes
LOUD_N = 11                                                                  # doubles per clip of its record
CLIP_TOO_LONG = 3                                                            # afx_gate_batch: more than chunk_size samples
PAD_CONSTANT, PAD_REFLECT = 0, 1                                             # afx_stft_batch: its pad modes
STFT_COMPLEX, STFT_MAG, STFT_POWER = 0, 1, 2                                 # and output kinds
PVOC_TILE = 32                                                               # afx_pvoc_batch: output steps per summation tile
LOUD_FIELDS = ("lufs", "blocks", "n1", "n2", "gamma_r", "gated_ms", "peak", "gain", "peak_out", "first_ms", "ungated_ms")
GROUPS_STATS = 24                                                            # doubles per clip of its record
K_NAMES = ("trim_blocks", "trim_decide", "frames", "dct", "stats")
K_FRAMES = 2

# every symbol include/afx.h declares
SYMBOLS = (
    "afx_version", "afx_device_count", "afx_last_error", "afx_init", "afx_destroy",
    "afx_malloc", "afx_free", "afx_host_alloc", "afx_host_free", "afx_memcpy_h2d", "afx_memcpy_d2h", "afx_synchronize",
    "afx_default_params", "afx_plan_create", "afx_plan_destroy", "afx_build_tables", "afx_build_mel_schedule",
    "afx_extract_batch", "afx_extract_submit", "afx_extract_collect", "afx_f0_batch", "afx_zcr_batch", "afx_spectral_batch", "afx_f0_build_tables", "afx_f0_dispatch", "afx_preprocess", "afx_plan_set_timing", "afx_plan_get_timings", "afx_plan_get_intervals",
    "afx_wav_probe", "afx_wav_read_s16", "afx_batch_geometry", "afx_dtw_batch", "afx_hpss_batch",
    "afx_resample_design", "afx_resample_batch", "afx_rfft_host", "afx_wav_read_raw", "afx_decode_batch",
    "afx_chroma_batch", "afx_chroma_filters", "afx_rhythm_batch", "afx_tempo_table",
    "afx_stft_chunks",
    "afx_butter_sos", "afx_filtfilt_geometry", "afx_sosfiltfilt_host", "afx_sosfiltfilt_batch",
    "afx_groups_batch", "afx_groups_cost", "afx_groups_dct_table", "afx_groups_debug_rows",
    "afx_beat_track_host", "afx_beat_batch",
    "afx_dtw_steps_batch",
    "afx_denoise_batch", "afx_denoise_cost",
    "afx_assess_batch", "afx_compare_batch", "afx_assess_host", "afx_compare_host", "afx_assess_cost",
    "afx_specdist_batch", "afx_clip_fft_batch", "afx_specdist_host", "afx_clip_fft_host", "afx_specdist_cost",
    "afx_smooth_geometry", "afx_savgol_tables", "afx_medfilt_host", "afx_savgol_host", "afx_energy_zcr_host",
    "afx_medfilt_batch", "afx_savgol_batch", "afx_energy_zcr_batch",
    "afx_kweight_sos", "afx_loudness_geometry", "afx_loudness_blocks", "afx_loudness_cost", "afx_loudness_host",
    "afx_loudness_batch",
    "afx_gate_params", "afx_gate_cost", "afx_gate_batch",
    "afx_stft_frames", "afx_istft_samples", "afx_stft_cost", "afx_stft_batch", "afx_istft_batch",
    "afx_pvoc_frames", "afx_time_stretch_samples", "afx_pvoc_cost", "afx_time_stretch_cost", "afx_pvoc_host",
    "afx_pvoc_batch", "afx_time_stretch_batch",
)


class AfxError(RuntimeError):
    pass


class GateOpts(C.Structure):
    """afx_gate_opts: noisereduce's arguments as afx_gate_batch takes them."""
    _fields_ = [
        ("sr", C.c_int32), ("n_fft", C.c_int32), ("win_length", C.c_int32), ("hop", C.c_int32),
        ("stationary", C.c_int32), ("clip_noise", C.c_int32), ("padding", C.c_int32), ("chunk_size", C.c_int32),
        ("prop_decrease", C.c_double), ("time_constant_s", C.c_double), ("freq_mask_smooth_hz", C.c_double),
        ("time_mask_smooth_ms", C.c_double), ("thresh_n_mult", C.c_double), ("sigmoid_slope", C.c_double),
        ("n_std_thresh", C.c_double),
    ]


class StftOpts(C.Structure):
    """afx_stft_opts: the framing of afx_stft_batch / afx_istft_batch."""
    _fields_ = [("n_fft", C.c_int32), ("hop", C.c_int32), ("center", C.c_int32), ("pad_mode", C.c_int32),
                ("out_kind", C.c_int32), ("reserved", C.c_int32 * 3)]


class Params(C.Structure):
    _fields_ = [
        ("sr", C.c_int32), ("n_fft", C.c_int32), ("hop", C.c_int32), ("n_mfcc", C.c_int32),
        ("n_mels", C.c_int32), ("window", C.c_int32), ("preemph", C.c_float),
        ("trim_top_db", C.c_float), ("trim_frame", C.c_int32), ("trim_hop", C.c_int32),
        ("top_db", C.c_float), ("amin", C.c_float), ("delta_width", C.c_int32),
        ("reserved", C.c_int32),
        ("fmin", C.c_float), ("fmax", C.c_float), ("htk", C.c_int32), ("lifter", C.c_float),
    ]


_lib = None
_lock = threading.Lock()


def lib() -> C.CDLL:
    """Loads libafx.so once; raises AfxError (never falls back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise AfxError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C audio_feature_extraction_amd/csrc` (no CPU fallback exists)")
        L = C.CDLL(LIB_PATH)
        vp, i32, i64p, f32p, i32p = C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_int32)
        L.afx_version.restype = i32
        L.afx_device_count.restype = i32
        L.afx_last_error.restype = C.c_char_p
        L.afx_init.argtypes = [i32, C.POINTER(vp)]
        L.afx_destroy.argtypes = [vp]; L.afx_destroy.restype = None
        L.afx_malloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
        L.afx_free.argtypes = [vp, vp]
        L.afx_host_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
        L.afx_host_free.argtypes = [vp, vp]
        L.afx_memcpy_h2d.argtypes = [vp, vp, vp, C.c_size_t]
        L.afx_memcpy_d2h.argtypes = [vp, vp, vp, C.c_size_t]
        L.afx_synchronize.argtypes = [vp]
        L.afx_default_params.argtypes = [C.POINTER(Params)]; L.afx_default_params.restype = None
        L.afx_plan_create.argtypes = [vp, C.POINTER(Params), C.POINTER(vp)]
        L.afx_plan_destroy.argtypes = [vp]; L.afx_plan_destroy.restype = None
        L.afx_build_tables.argtypes = [C.POINTER(Params), vp, vp, vp]
        L.afx_build_mel_schedule.argtypes = [C.POINTER(Params), vp, vp, vp]
        L.afx_extract_batch.argtypes = [vp, vp, i32, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp]
        L.afx_extract_submit.argtypes = [vp, vp, i32, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp]
        L.afx_extract_collect.argtypes = [vp]
        L.afx_f0_batch.argtypes = [vp, vp, i32, i32, vp, vp, i32, i32, C.c_double, C.c_double, vp, vp, vp, vp]
        L.afx_zcr_batch.argtypes = [vp, vp, i32, i32, vp, vp, i32, i32, vp, vp, vp]
        L.afx_spectral_batch.argtypes = [vp, vp, i32, i32, vp, vp, i32, i32, vp, vp, vp]
        L.afx_f0_build_tables.argtypes = [i32, i32, i32, C.c_double, C.c_double, vp, vp, vp, vp]
        L.afx_f0_dispatch.argtypes = [i32, i32, i32, C.c_double, C.c_double, vp]
        L.afx_preprocess.argtypes = [vp, vp, C.c_int64, vp, i64p, i64p, i32p]
        L.afx_plan_set_timing.argtypes = [vp, i32]
        L.afx_plan_get_timings.argtypes = [vp, vp, vp, i32]
        L.afx_plan_get_intervals.argtypes = [vp, i32, vp, vp, i32, i32p]
        L.afx_batch_geometry.argtypes = [C.POINTER(Params), vp, vp, i32, vp, vp]
        L.afx_wav_probe.argtypes = [vp, i32, i32, vp, vp, vp, vp]
        L.afx_wav_read_s16.argtypes = [vp, i32, i32, vp, vp, vp, C.c_int64, vp, vp]
        L.afx_dtw_batch.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp]
        L.afx_hpss_batch.argtypes = [vp, vp, i32, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp]
        if hasattr(L, "afx_dtw_steps_batch"):                # newer than version 107 says: found by its presence
            L.afx_dtw_steps_batch.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, i32, i32, i32, vp, i32, vp, vp,
                                              vp, vp, vp, vp, vp, vp, vp, vp]
        if hasattr(L, "afx_resample_batch"):                 # absent from a library older than version 107
            L.afx_resample_design.argtypes = [i32, i32, vp, vp]
            L.afx_resample_batch.argtypes = [vp, vp, i32, i32, vp, vp, i32, i32, i32, vp, i32, vp, i32, vp, vp]
        if hasattr(L, "afx_decode_batch"):                   # newer than version 107 says: found by their presence
            L.afx_wav_read_raw.argtypes = [vp, i32, i32, vp, vp, vp, C.c_int64, vp, vp]
            L.afx_decode_batch.argtypes = [vp, vp, i32, vp, vp, vp, vp, i32, vp, i32, vp]
        if hasattr(L, "afx_chroma_batch"):                   # newer than version 107 says: found by their presence
            L.afx_chroma_batch.argtypes = [vp, vp, i32, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
            L.afx_chroma_filters.argtypes = [i32, C.c_double, vp]
        if hasattr(L, "afx_rhythm_batch"):                   # newer than version 107 says: found by their presence
            L.afx_rhythm_batch.argtypes = [vp, vp, i32, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
            L.afx_tempo_table.argtypes = [i32, i32p, i32p, vp, vp]
        if hasattr(L, "afx_stft_chunks"):                    # newer than version 107 says: found by its presence
            L.afx_stft_chunks.argtypes = [vp, i32, vp, C.c_int64, vp]
        if hasattr(L, "afx_sosfiltfilt_batch"):              # newer than version 107 says: found by their presence
            L.afx_butter_sos.argtypes = [i32, C.c_double, i32, vp]
            L.afx_filtfilt_geometry.argtypes = [vp]
            L.afx_sosfiltfilt_host.argtypes = [vp, i32, C.c_int64, vp, i32, i32, i32, C.c_float, vp, vp, vp]
            L.afx_sosfiltfilt_batch.argtypes = [vp, vp, i32, i32, vp, vp, i32, vp, i32, i32, i32, C.c_float, vp, i32, vp, vp, vp]
        if hasattr(L, "afx_groups_batch"):                   # newer than version 107 says: found by their presence
            L.afx_groups_batch.argtypes = [vp, vp, i32, i32, vp, vp, i32, i32, i32, vp, vp, vp, vp]
            L.afx_groups_cost.argtypes = [i32, i32, vp]
            L.afx_groups_dct_table.argtypes = [i32, vp]
            L.afx_groups_debug_rows.argtypes = [vp, vp, C.c_int64, i64p]
        if hasattr(L, "afx_beat_batch"):                     # newer than version 107 says: found by their presence
            dbl = C.c_double
            L.afx_beat_track_host.argtypes = [vp, C.c_int64, dbl, dbl, dbl, i32, vp, i64p, vp, vp, vp]
            L.afx_beat_batch.argtypes = [vp, vp, i32, i32, vp, vp, i32, i32, vp, dbl, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        if hasattr(L, "afx_denoise_batch"):                  # newer than version 107 says: found by their presence
            L.afx_denoise_batch.argtypes = [vp, vp, i32, i32, vp, vp, i32, i32, i32, C.c_double, i32, vp, vp, vp]
            L.afx_denoise_cost.argtypes = [i32, i32, i32, vp]
        if hasattr(L, "afx_assess_batch"):                   # newer than version 107 says: found by their presence
            L.afx_assess_cost.argtypes = [i32, i32, i32, vp]
            L.afx_assess_host.argtypes = [vp, i32, C.c_int64, i32, i32, C.c_double, C.c_int64, vp, vp]
            L.afx_compare_host.argtypes = [vp, vp, i32, C.c_int64, C.c_int64, vp, vp]
            L.afx_assess_batch.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, i32, C.c_double, C.c_int64, vp, vp]
            L.afx_compare_batch.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, i32, vp, vp]
        if hasattr(L, "afx_specdist_batch"):                 # newer than version 107 says: found by their presence
            L.afx_specdist_cost.argtypes = [i32, i32, vp]
            L.afx_specdist_host.argtypes = [vp, vp, i32, C.c_int64, C.c_int64, vp, vp]
            L.afx_clip_fft_host.argtypes = [vp, i32, C.c_int64, vp, vp]
            L.afx_specdist_batch.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, i32, vp, vp]
            L.afx_clip_fft_batch.argtypes = [vp, vp, i32, i32, vp, vp, i32, vp, vp, vp]
        if hasattr(L, "afx_medfilt_batch"):                  # newer than version 107 says: found by their presence
            dbl = C.c_double
            L.afx_smooth_geometry.argtypes = [vp]
            L.afx_savgol_tables.argtypes = [i32, i32, i32, dbl, vp, vp, vp]
            L.afx_medfilt_host.argtypes = [vp, i32, C.c_int64, i32, vp, vp]
            L.afx_savgol_host.argtypes = [vp, i32, C.c_int64, i32, i32, i32, dbl, vp, vp]
            L.afx_energy_zcr_host.argtypes = [vp, C.c_int64, i32, i32, i32, vp, vp]
            L.afx_medfilt_batch.argtypes = [vp, vp, i32, i32, vp, vp, i32, i32, vp, i32, vp, vp]
            L.afx_savgol_batch.argtypes = [vp, vp, i32, i32, vp, vp, i32, i32, i32, i32, dbl, vp, i32, vp, vp]
            L.afx_energy_zcr_batch.argtypes = [vp, vp, i32, i32, vp, vp, i32, i32, i32, i32, i32, vp, vp]
        if hasattr(L, "afx_loudness_batch"):                 # newer than version 107 says: found by their presence
            dbl = C.c_double
            L.afx_kweight_sos.argtypes = [i32, vp]
            L.afx_loudness_geometry.argtypes = [vp]
            L.afx_loudness_blocks.argtypes = [C.c_int64, i32, dbl, i64p]
            L.afx_loudness_cost.argtypes = [i32, i32, i32, i32, vp]
            L.afx_loudness_host.argtypes = [vp, i32, C.c_int64, i32, dbl, dbl, i32, vp, vp, vp, vp]
            L.afx_loudness_batch.argtypes = [vp, vp, i32, i32, vp, vp, vp, i32, dbl, i32, dbl, vp, vp, vp, vp, i32, vp, vp]
        if hasattr(L, "afx_gate_batch"):                     # newer than version 107 says: found by their presence
            L.afx_gate_params.argtypes = [vp, C.c_int64, vp, vp, vp, vp]
            L.afx_gate_cost.argtypes = [vp, i32, i32, i32, i32, vp]
            L.afx_gate_batch.argtypes = [vp, vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp]
        if hasattr(L, "afx_stft_batch"):                     # newer than version 107 says: found by their presence
            i64 = C.c_int64
            L.afx_stft_frames.argtypes = [vp, i64, vp, vp]
            L.afx_istft_samples.argtypes = [vp, i64, i64, vp, vp]
            L.afx_stft_cost.argtypes = [vp, i32, i32, i32, i32, vp]
            L.afx_stft_batch.argtypes = [vp, vp, i32, i32, vp, vp, i32, vp, vp, vp, i32, vp, vp]
            L.afx_istft_batch.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, i32, vp, vp]
        if hasattr(L, "afx_pvoc_batch"):                     # newer than version 107 says: found by their presence
            i64, dbl = C.c_int64, C.c_double
            L.afx_pvoc_frames.argtypes = [i32, i32, i64, dbl, vp, vp]
            L.afx_time_stretch_samples.argtypes = [vp, i64, dbl, vp, vp, vp, vp]
            L.afx_pvoc_cost.argtypes = [i32, i32, i32, vp]
            L.afx_time_stretch_cost.argtypes = [vp, i32, i32, i32, vp]
            L.afx_pvoc_host.argtypes = [vp, i64, dbl, i32, i32, vp, vp]
            L.afx_pvoc_batch.argtypes = [vp, vp, i32, vp, vp, vp, i32, i32, i32, vp, i32, vp, vp]
            L.afx_time_stretch_batch.argtypes = [vp, vp, i32, i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp]
        if hasattr(L, "afx_rfft_host"):                      # absent from a library built before the mixed-radix lengths
            L.afx_rfft_host.argtypes = [i32, vp, vp]
        _lib = L
    return _lib


def _path_array(paths):
    arr = (C.c_char_p * len(paths))()
    arr[:] = [os.fsencode(p) for p in paths]
    return arr


def wav_probe(paths, threads: int = 16) -> dict:
    """Host-only: RIFF headers of many files at once (native threads).  tag 1 = PCM, 3 = float; status 0 ok,
    1 not a usable WAVE file, 2 cannot be opened."""
    n = len(paths)
    info = np.zeros((n, 4), np.int32)
    frames, off, status = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int32)
    if n:
        arr = _path_array(paths)
        _check(lib().afx_wav_probe(arr, n, int(threads), info.ctypes.data, frames.ctypes.data, off.ctypes.data,
                                   status.ctypes.data), "afx_wav_probe")
    return {"tag": info[:, 0], "channels": info[:, 1], "rate": info[:, 2], "bits": info[:, 3],
            "frames": frames, "data_off": off, "status": status}


def wav_read_s16(paths, data_off, frames, out: np.ndarray, offsets, threads: int = 16) -> np.ndarray:
    """Host-only: the 16-bit samples of the files straight into ``out`` (int16, C-contiguous) at ``offsets``."""
    n = len(paths)
    status = np.zeros(n, np.int32)
    if n:
        if out.dtype != np.int16 or not out.flags.c_contiguous:
            raise ValueError("out must be C-contiguous int16")
        data_off = np.ascontiguousarray(data_off, np.int64)
        frames = np.ascontiguousarray(frames, np.int64)
        offsets = np.ascontiguousarray(offsets, np.int64)
        arr = _path_array(paths)
        _check(lib().afx_wav_read_s16(arr, n, int(threads), data_off.ctypes.data, frames.ctypes.data, out.ctypes.data,
                                      int(out.size), offsets.ctypes.data, status.ctypes.data), "afx_wav_read_s16")
    return status


def wav_read_raw(paths, data_off, nbytes, out: np.ndarray, offsets, threads: int = 16) -> np.ndarray:
    """Host-only: ``nbytes[i]`` bytes of file i from ``data_off[i]`` straight into ``out`` (uint8, C-contiguous) at byte
    ``offsets[i]``; -> status per file (0 read, 2 cannot be opened / read).  ValueError, with ``out`` untouched, when a
    clip does not fit ``out``."""
    n = len(paths)
    status = np.zeros(n, np.int32)
    if not hasattr(lib(), "afx_wav_read_raw"):
        raise NotImplementedError("this libafx has no afx_wav_read_raw")
    if n:
        if out.dtype != np.uint8 or not out.flags.c_contiguous:
            raise ValueError("out must be C-contiguous uint8")
        data_off = np.ascontiguousarray(data_off, np.int64)
        nbytes = np.ascontiguousarray(nbytes, np.int64)
        offsets = np.ascontiguousarray(offsets, np.int64)
        if not (data_off.shape[0] == nbytes.shape[0] == offsets.shape[0] == n):
            raise ValueError("data_off, nbytes and offsets must have one entry per file")
        arr = _path_array(paths)
        _check(lib().afx_wav_read_raw(arr, n, int(threads), data_off.ctypes.data, nbytes.ctypes.data, out.ctypes.data,
                                      int(out.size), offsets.ctypes.data, status.ctypes.data), "afx_wav_read_raw")
    return status


def wav_sample_kinds(probe: dict) -> np.ndarray:
    """Per probed file the SMP_* kind afx_decode_batch takes it as, or -1: status 0, a (tag, bits) pair of SMP_OF_WAV,
    1 .. DECODE_MAX_CHANNELS channels and a positive rate."""
    kinds = np.full(probe["status"].shape[0], -1, np.int32)
    for (tag, bits), k in SMP_OF_WAV.items():
        kinds[(probe["tag"] == tag) & (probe["bits"] == bits)] = k
    kinds[(probe["status"] != 0) | (probe["channels"] < 1) | (probe["channels"] > DECODE_MAX_CHANNELS) | (probe["rate"] <= 0)] = -1
    return kinds


def batch_geometry(p: "Params", offsets, lengths) -> dict:
    """Host-only: how a ragged batch is laid out on the device (frame slots padded to 16-frame blocks)."""
    offsets = np.ascontiguousarray(offsets, np.int64)
    lengths = np.ascontiguousarray(lengths, np.int64)
    n = int(offsets.shape[0])
    rec = np.zeros((max(n, 1), 4), np.int64)
    tot = np.zeros(4, np.int64)
    _check(lib().afx_batch_geometry(C.byref(p), offsets.ctypes.data, lengths.ctypes.data, n, rec.ctypes.data, tot.ctypes.data),
           "afx_batch_geometry")
    rec = rec[:n]
    return {"frame_base": rec[:, 0], "tmax": rec[:, 1], "tpad": rec[:, 2], "blk_base": rec[:, 3],
            "frame_slots": int(tot[0]), "blocks": int(tot[1]), "trim_blocks": int(tot[2]), "max_tmax": int(tot[3])}


def f0_build_tables(sr: int, n_fft: int, hop: int, fmin: float, fmax: float) -> dict:
    """Host-only: the pYIN tables of a configuration (no GPU needed)."""
    info = np.zeros(8, np.int32)
    _check(lib().afx_f0_build_tables(sr, n_fft, hop, fmin, fmax, info.ctypes.data, None, None, None), "afx_f0_build_tables")
    band, nb = int(info[3]), int(info[2])
    w = 2 * band + 1
    beta, lt, freqs = np.zeros(100), np.zeros(2 * w * w), np.zeros(nb)
    _check(lib().afx_f0_build_tables(sr, n_fft, hop, fmin, fmax, info.ctypes.data, beta.ctypes.data, lt.ctypes.data,
                                     freqs.ctypes.data), "afx_f0_build_tables")
    keys = ("min_period", "max_period", "n_bins", "band", "cap", "n_lag", "R", "slots")
    return {**{k: int(v) for k, v in zip(keys, info)}, "beta": beta, "lt": lt.reshape(2, w, w), "freqs": freqs}


F0_DISPATCH_KEYS = ("energy_lpw", "epb", "yin_n", "yin_fpb", "yin_sh", "vit_nbt", "vit_bandt", "vit_tpt", "bt_depth",
                    "band", "n_bins", "yin_lds")


def f0_dispatch(sr: int, n_fft: int, hop: int, fmin: float, fmax: float) -> dict:
    """Host-only: the kernel instantiations afx_f0_batch launches for a configuration (what its launchers switch on):
    k_f0_energy (energy_lpw 0) or k_f0_energy2<energy_lpw> with epb frames per workgroup, k_f0_yin<yin_n, yin_n, yin_fpb,
    yin_sh>, k_f0_viterbi<0, vit_nbt, vit_bandt> (0 / 0: generic) with vit_tpt targets per thread, k_f0_backtrack<bt_depth>.
    NotImplementedError, with afx_f0_batch's reason, for a configuration extract_f0 refuses."""
    out = np.zeros(len(F0_DISPATCH_KEYS), np.int32)
    _check(lib().afx_f0_dispatch(int(sr), int(n_fft), int(hop), float(fmin), float(fmax), out.ctypes.data), "afx_f0_dispatch")
    return {k: int(v) for k, v in zip(F0_DISPATCH_KEYS, out)}


def resample_design(sr_in: int, sr_out: int) -> dict:
    """Host-only: the polyphase filter afx_resample_batch applies for a rate pair (wavio._resample_filter's design)."""
    info = np.zeros(4, np.int32)
    _check(lib().afx_resample_design(int(sr_in), int(sr_out), info.ctypes.data, None), "afx_resample_design")
    taps = np.zeros(int(info[2]), np.float64)
    _check(lib().afx_resample_design(int(sr_in), int(sr_out), info.ctypes.data, taps.ctypes.data), "afx_resample_design")
    return {"up": int(info[0]), "down": int(info[1]), "n_taps": int(info[2]), "half": int(info[3]), "taps": taps}


def rfft_host(x) -> np.ndarray:
    """Host-only: the frame kernel's mixed-radix real FFT of one frame, in float32 on the CPU (complex64, n/2 + 1 bins)."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    out = np.zeros(2 * (x.size // 2 + 1), np.float32)
    _check(lib().afx_rfft_host(int(x.size), x.ctypes.data, out.ctypes.data), "afx_rfft_host")
    return out.view(np.complex64)


def chroma_filters(sr: int, tuning: float = 0.0) -> np.ndarray:
    """Host-only: librosa.filters.chroma(sr, 2048, tuning) at its defaults, [12, 1025] float32 (what afx_chroma_batch uploads)."""
    if not hasattr(lib(), "afx_chroma_filters"):
        raise NotImplementedError("this libafx has no afx_chroma_filters")
    out = np.zeros((12, HPSS_BINS), np.float32)
    _check(lib().afx_chroma_filters(int(sr), float(tuning), out.ctypes.data), "afx_chroma_filters")
    return out


def tempo_table(sr: int) -> dict:
    """Host-only: what afx_rhythm_batch decides the tempo with at a sample rate (hop 512): ``win`` = int(8 sr) // 512 lags,
    ``kmin`` (the first lag slower than 320 bpm), ``bpm`` [win] (bpm[0] = inf) and ``logprior`` [win] (-inf below kmin), float64.
    NotImplementedError when win is not in 2 .. 768 (sr above 49215)."""
    if not hasattr(lib(), "afx_tempo_table"):
        raise NotImplementedError("this libafx has no afx_tempo_table")
    win, kmin = C.c_int32(), C.c_int32()
    _check(lib().afx_tempo_table(int(sr), C.byref(win), C.byref(kmin), None, None), "afx_tempo_table")
    bpm, logprior = np.zeros(win.value, np.float64), np.zeros(win.value, np.float64)
    _check(lib().afx_tempo_table(int(sr), C.byref(win), C.byref(kmin), bpm.ctypes.data, logprior.ctypes.data), "afx_tempo_table")
    return {"win": int(win.value), "kmin": int(kmin.value), "bpm": bpm, "logprior": logprior}


def stft_chunks(lengths, cost, budget: int) -> np.ndarray:
    """Host-only: the chunk each clip falls into when afx_hpss_batch / afx_chroma_batch / afx_rhythm_batch cut a batch at
    ``budget`` bytes (-1 for a clip of length 0).  ``cost``: bytes per frame, per tile, per sample and per clip, frames per
    tile, most tiles of a chunk."""
    if not hasattr(lib(), "afx_stft_chunks"):
        raise NotImplementedError("this libafx has no afx_stft_chunks")
    lengths = np.ascontiguousarray(lengths, np.int64)
    cost = np.ascontiguousarray(cost, np.int64)
    if lengths.ndim != 1 or cost.shape != (6,):
        raise ValueError("lengths must be one-dimensional and cost hold 6 values")
    out = np.zeros(lengths.shape[0], np.int32)
    _check(lib().afx_stft_chunks(lengths.ctypes.data, int(lengths.shape[0]), cost.ctypes.data, int(budget), out.ctypes.data),
           "afx_stft_chunks")
    return out


def _need_groups():
    if not hasattr(lib(), "afx_groups_batch"):
        raise NotImplementedError("this libafx has no afx_groups_batch")


def groups_cost(groups: int, flags: int = 0) -> np.ndarray:
    """Host-only: the cost record afx_groups_batch cuts a batch with (bytes per frame, per tile, per sample and per clip,
    frames per tile, most tiles of a chunk), for ``stft_chunks``."""
    _need_groups()
    cost = np.zeros(6, np.int64)
    _check(lib().afx_groups_cost(int(groups), int(flags), cost.ctypes.data), "afx_groups_cost")
    return cost


def _need_denoise():
    if not hasattr(lib(), "afx_denoise_batch"):
        raise NotImplementedError("this libafx has no afx_denoise_batch")


def denoise_cost(flags: int = 0, fmt: int = FMT_F32, mem: int = MEM_HOST) -> np.ndarray:
    """Host-only: the cost record afx_denoise_batch cuts a batch with (bytes per frame, per tile, per sample, per clip;
    frames per tile, most tiles of a chunk), for ``stft_chunks``."""
    _need_denoise()
    cost = np.zeros(6, np.int64)
    _check(lib().afx_denoise_cost(int(flags), int(fmt), int(mem), cost.ctypes.data), "afx_denoise_cost")
    return cost


def denoise_check(params: "Params", flags: int, mode: int, beta: float, noise_frames: int) -> None:
    """What afx_denoise_batch refuses of a plan's parameters and of its own arguments, raised as the call itself would
    raise it (NotImplementedError: a plan or flag it does not support; ValueError: an invalid argument).  No device."""
    if params.n_fft != 2048 or params.hop != 512 or params.window != WINDOW_HANN:
        raise NotImplementedError("afx_denoise_batch: the plan must have frame_length 2048, hop_length 512 and the Hann window")
    if flags & FLAG_TRIM:
        raise NotImplementedError("afx_denoise_batch: trim is not applied here; pass the preprocessed signal")
    if flags & ~(FLAG_PREEMPH | DENOISE_RMS_GAIN | DENOISE_VAD):
        raise ValueError("afx_denoise_batch: unknown flag")
    if mode not in (DENOISE_SPECSUB, DENOISE_WIENER):
        raise ValueError("afx_denoise_batch: unknown mode")
    if not (np.isfinite(beta) and beta >= 0):
        raise ValueError("afx_denoise_batch: beta must be finite and >= 0")
    if not 1 <= int(noise_frames) <= DENOISE_MAX_NOISE_FRAMES or int(noise_frames) != noise_frames:
        raise ValueError("afx_denoise_batch: noise_frames must be in [1, 64]")
    if flags & DENOISE_VAD and int(0.010 * params.sr) < 1:
        raise ValueError("afx_denoise_batch: the VAD needs a sample rate of at least 100 Hz")


def _need_assess():
    if not hasattr(lib(), "afx_assess_batch"):
        raise NotImplementedError("this libafx has no afx_assess_batch")


def assess_cost(what: int = COST_ASSESS, fmt: int = FMT_F32, mem: int = MEM_HOST) -> np.ndarray:
    """Host-only: the cost record afx_assess_batch (COST_ASSESS) or afx_compare_batch (COST_COMPARE) cuts a batch with
    (bytes per frame, per tile, per sample, per clip; frames per tile, most tiles of a chunk), for ``stft_chunks``."""
    _need_assess()
    cost = np.zeros(6, np.int64)
    _check(lib().afx_assess_cost(int(what), int(fmt), int(mem), cost.ctypes.data), "afx_assess_cost")
    return cost


def _mono_clip(x, what: str) -> np.ndarray:
    x = np.ascontiguousarray(x)
    if x.ndim != 1 or x.dtype not in (np.int16, np.float32):
        raise ValueError(f"{what} must be a one-dimensional int16 or float32 array")
    return x


def assess_host(x, frame_short: int, frame_long: int, threshold_db: float = -40.0, noise_cap: int = 2000) -> dict:
    """Host-only: afx_assess_host, one int16 / float32 clip through the definitions of afx_assess_batch on the CPU.
    Returns rec (float64 [ASSESS_N], NaN when the clip failed; ASSESS_FIELDS names the entries) and status."""
    _need_assess()
    x = _mono_clip(x, "x")
    rec = np.zeros(ASSESS_N, np.float64)
    status = np.zeros(1, np.int32)
    _check(lib().afx_assess_host(x.ctypes.data, FMT_S16 if x.dtype == np.int16 else FMT_F32, int(x.size), int(frame_short),
                                 int(frame_long), float(threshold_db), int(noise_cap), rec.ctypes.data, status.ctypes.data),
           "afx_assess_host")
    return {"rec": rec, "status": int(status[0])}


def compare_host(ref, deg) -> dict:
    """Host-only: afx_compare_host, one pair of int16 / float32 clips (both of one type) through the definitions of
    afx_compare_batch on the CPU.  Returns rec (float64 [COMPARE_N]; COMPARE_FIELDS names the entries) and status."""
    _need_assess()
    ref, deg = _mono_clip(ref, "ref"), _mono_clip(deg, "deg")
    if ref.dtype != deg.dtype:
        raise ValueError("ref and deg must have one sample type")
    rec = np.zeros(COMPARE_N, np.float64)
    status = np.zeros(1, np.int32)
    _check(lib().afx_compare_host(ref.ctypes.data, deg.ctypes.data, FMT_S16 if ref.dtype == np.int16 else FMT_F32,
                                  int(ref.size), int(deg.size), rec.ctypes.data, status.ctypes.data), "afx_compare_host")
    return {"rec": rec, "status": int(status[0])}


def _need_specdist():
    if not hasattr(lib(), "afx_specdist_batch"):
        raise NotImplementedError("this libafx has no afx_specdist_batch")


def specdist_cost(fmt: int = FMT_F32, mem: int = MEM_HOST) -> np.ndarray:
    """Host-only: the cost record afx_specdist_batch / afx_clip_fft_batch cut a batch with (bytes per frame, per tile, per
    sample, per clip; frames per tile, most tiles of a chunk), for ``stft_chunks``."""
    _need_specdist()
    cost = np.zeros(6, np.int64)
    _check(lib().afx_specdist_cost(int(fmt), int(mem), cost.ctypes.data), "afx_specdist_cost")
    return cost


def specdist_host(ref, deg) -> dict:
    """Host-only: afx_specdist_host, one pair of int16 / float32 clips (both of one type) through the definitions of
    afx_specdist_batch on the CPU.  Returns rec (float64 [SPECDIST_N]; SPECDIST_FIELDS names the entries) and status."""
    _need_specdist()
    ref, deg = _mono_clip(ref, "ref"), _mono_clip(deg, "deg")
    if ref.dtype != deg.dtype:
        raise ValueError("ref and deg must have one sample type")
    rec = np.zeros(SPECDIST_N, np.float64)
    status = np.zeros(1, np.int32)
    _check(lib().afx_specdist_host(ref.ctypes.data, deg.ctypes.data, FMT_S16 if ref.dtype == np.int16 else FMT_F32,
                                   int(ref.size), int(deg.size), rec.ctypes.data, status.ctypes.data), "afx_specdist_host")
    return {"rec": rec, "status": int(status[0])}


def clip_fft_host(x) -> dict:
    """Host-only: afx_clip_fft_host, np.fft.rfft of one int16 / float32 clip by the Bluestein transform of
    afx_clip_fft_batch on the CPU.  Returns bins (complex128 [n // 2 + 1]; empty for an empty clip, NaN for a clip that is
    not finite everywhere) and status."""
    _need_specdist()
    x = _mono_clip(x, "x")
    bins = np.zeros(x.size // 2 + 1 if x.size else 0, np.complex128)
    status = np.zeros(1, np.int32)
    _check(lib().afx_clip_fft_host(x.ctypes.data, FMT_S16 if x.dtype == np.int16 else FMT_F32, int(x.size),
                                   bins.ctypes.data, status.ctypes.data), "afx_clip_fft_host")
    return {"bins": bins, "status": int(status[0])}


def groups_dct_table(n_mels: int = 128) -> np.ndarray:
    """Host-only: rows 0 .. 12 of the orthonormal DCT-II of ``n_mels`` points as afx_groups_batch's MFCC statistics apply
    them, [13, 128] float32 (columns past ``n_mels`` zero)."""
    _need_groups()
    out = np.zeros((13, 128), np.float32)
    _check(lib().afx_groups_dct_table(int(n_mels), out.ctypes.data), "afx_groups_dct_table")
    return out


def _need_filt():
    if not hasattr(lib(), "afx_sosfiltfilt_batch"):
        raise NotImplementedError("this libafx has no afx_sosfiltfilt_batch")


def _sos_array(sos) -> np.ndarray:
    sos = np.ascontiguousarray(sos, np.float64)
    if sos.ndim != 2 or sos.shape[1] != 6 or sos.shape[0] < 1:
        raise ValueError("sos array must be shape (n_sections, 6)")
    return sos


def butter_sos(order: int, wn: float, highpass: bool) -> np.ndarray:
    """Host-only: afx_butter_sos, the (order + 1) // 2 second-order sections of a digital Butterworth filter (wn: 1 = Nyquist)."""
    _need_filt()
    if int(order) < 1:
        raise ValueError("the order must be at least 1")
    sos = np.zeros(((int(order) + 1) // 2, 6), np.float64)
    _check(lib().afx_butter_sos(int(order), float(wn), int(bool(highpass)), sos.ctypes.data), "afx_butter_sos")
    return sos


def filtfilt_geometry() -> dict:
    """Host-only: the block decomposition of afx_sosfiltfilt_batch (samples per block, blocks per tile) and its bounds."""
    _need_filt()
    info = np.zeros(4, np.int32)
    _check(lib().afx_filtfilt_geometry(info.ctypes.data), "afx_filtfilt_geometry")
    return {"block": int(info[0]), "tile_blocks": int(info[1]), "tile": int(info[0]) * int(info[1]),
            "max_sections": int(info[2]), "max_padlen": int(info[3])}


def sosfiltfilt_host(x, sos, padlen: int, mode: int = FILT_PLAIN, preemph: float = 0.98) -> dict:
    """Host-only: afx_sosfiltfilt_host, one int16 / float32 clip through the kernels' block decomposition on the CPU.
    Returns out (float32; zeros when the clip failed), peak (max|x|, max|y|) and status."""
    _need_filt()
    sos = _sos_array(sos)
    x = np.ascontiguousarray(x)
    if x.ndim != 1 or x.dtype not in (np.int16, np.float32):
        raise ValueError("x must be a one-dimensional int16 or float32 array")
    out = np.zeros(x.size, np.float32)
    peak = np.zeros(2, np.float64)
    status = np.zeros(1, np.int32)
    _check(lib().afx_sosfiltfilt_host(x.ctypes.data, FMT_S16 if x.dtype == np.int16 else FMT_F32, int(x.size), sos.ctypes.data,
                                      int(sos.shape[0]), int(padlen), int(mode), float(preemph), out.ctypes.data,
                                      peak.ctypes.data, status.ctypes.data), "afx_sosfiltfilt_host")
    return {"out": out, "peak": peak, "status": int(status[0])}


def _need_smooth():
    if not hasattr(lib(), "afx_medfilt_batch"):
        raise NotImplementedError("this libafx has no afx_medfilt_batch")


def smooth_geometry() -> dict:
    """Host-only: the tile of afx_medfilt_batch / afx_savgol_batch (samples a workgroup stages) and their bounds."""
    _need_smooth()
    info = np.zeros(4, np.int32)
    _check(lib().afx_smooth_geometry(info.ctypes.data), "afx_smooth_geometry")
    return {"tile": int(info[0]), "max_window": int(info[1]), "max_polyorder": int(info[2]), "max_deriv": int(info[3])}


def savgol_tables(window_length: int, polyorder: int, deriv: int = 0, delta: float = 1.0) -> dict:
    """Host-only: afx_savgol_tables.  coeffs [W] (scipy.signal.savgol_coeffs' order), left / right [W // 2, W]: the first /
    last W // 2 outputs as weights over the first / last W samples."""
    _need_smooth()
    W = max(int(window_length), 1)
    coeffs, left, right = np.zeros(W, np.float64), np.zeros((W // 2, W), np.float64), np.zeros((W // 2, W), np.float64)
    _check(lib().afx_savgol_tables(int(window_length), int(polyorder), int(deriv), float(delta), coeffs.ctypes.data,
                                   left.ctypes.data, right.ctypes.data), "afx_savgol_tables")
    return {"coeffs": coeffs, "left": left, "right": right}


def medfilt_host(x, kernel_size: int = 3) -> dict:
    """Host-only: afx_medfilt_host, one int16 / float32 clip through the kernels' median on the CPU.  Returns out (float32;
    zeros when the clip failed) and status."""
    _need_smooth()
    x = _mono_clip(x, "x")
    out = np.zeros(x.size, np.float32)
    status = np.zeros(1, np.int32)
    _check(lib().afx_medfilt_host(x.ctypes.data, FMT_S16 if x.dtype == np.int16 else FMT_F32, int(x.size), int(kernel_size),
                                  out.ctypes.data, status.ctypes.data), "afx_medfilt_host")
    return {"out": out, "status": int(status[0])}


def savgol_host(x, window_length: int, polyorder: int, deriv: int = 0, delta: float = 1.0) -> dict:
    """Host-only: afx_savgol_host, one int16 / float32 clip through the kernels' fused chains on the CPU.  Returns out
    (float32; zeros when the clip failed) and status."""
    _need_smooth()
    x = _mono_clip(x, "x")
    out = np.zeros(x.size, np.float32)
    status = np.zeros(1, np.int32)
    _check(lib().afx_savgol_host(x.ctypes.data, FMT_S16 if x.dtype == np.int16 else FMT_F32, int(x.size), int(window_length),
                                 int(polyorder), int(deriv), float(delta), out.ctypes.data, status.ctypes.data),
           "afx_savgol_host")
    return {"out": out, "status": int(status[0])}


def energy_zcr_host(y, frame_length: int = 2048, hop_length: int = 512, flags: int = EZ_ENERGY | EZ_ZCR) -> dict:
    """Host-only: afx_energy_zcr_host, one float32 clip (already preprocessed) through the operations of
    afx_energy_zcr_batch on the CPU.  Returns rec (float64 [EZ_N]; EZ_FIELDS names the entries) and status."""
    _need_smooth()
    y = np.ascontiguousarray(y)
    if y.ndim != 1 or y.dtype != np.float32:
        raise ValueError("y must be a one-dimensional float32 array")
    rec = np.zeros(EZ_N, np.float64)
    status = np.zeros(1, np.int32)
    _check(lib().afx_energy_zcr_host(y.ctypes.data, int(y.size), int(frame_length), int(hop_length), int(flags),
                                     rec.ctypes.data, status.ctypes.data), "afx_energy_zcr_host")
    return {"rec": rec, "status": int(status[0])}


def _need_gate():
    if not hasattr(lib(), "afx_gate_batch"):
        raise NotImplementedError("this libafx has no afx_gate_batch")


def gate_opts(sr: int, stationary: bool = False, prop_decrease: float = 1.0, time_constant_s: float = 2.0,
              freq_mask_smooth_hz: float = 500, time_mask_smooth_ms: float = 50, thresh_n_mult_nonstationary: float = 2,
              sigmoid_slope_nonstationary: float = 10, n_std_thresh_stationary: float = 1.5, chunk_size: int = 600000,
              padding: int = 30000, n_fft: int = 1024, win_length=None, hop_length=None,
              clip_noise_stationary: bool = True) -> GateOpts:
    """noisereduce.reduce_noise's keywords (its names and defaults) as the record afx_gate_batch takes."""
    win = int(n_fft) if win_length is None else int(win_length)
    hop = win // 4 if hop_length is None else int(hop_length)
    return GateOpts(int(sr), int(n_fft), win, hop, int(bool(stationary)), int(bool(clip_noise_stationary)), int(padding),
                    int(chunk_size), float(prop_decrease), float(time_constant_s), float(freq_mask_smooth_hz),
                    float(time_mask_smooth_ms), float(thresh_n_mult_nonstationary), float(sigmoid_slope_nonstationary),
                    float(n_std_thresh_stationary))


def gate_params(opts: GateOpts, length: int = 0) -> dict:
    """Host-only: afx_gate_params, what noisereduce derives from its arguments: n_f, n_t, the frames T of a clip of
    ``length`` samples, whether the mask is smoothed, beta, and the normalised taps of each axis of the smoothing filter.
    ValueError where noisereduce raises."""
    _need_gate()
    info = np.zeros(4, np.int64)
    beta = C.c_double()
    tf, tt = np.zeros(257, np.float64), np.zeros(129, np.float64)
    _check(lib().afx_gate_params(C.addressof(opts), int(length), info.ctypes.data, C.addressof(beta), tf.ctypes.data,
                                 tt.ctypes.data), "afx_gate_params")
    n_f, n_t = int(info[0]), int(info[1])
    return {"n_f": n_f, "n_t": n_t, "frames": int(info[2]), "smooth": bool(info[3]), "beta": float(beta.value),
            "taps_f": tf[:2 * n_f + 1].copy(), "taps_t": tt[:2 * n_t + 1].copy()}


def gate_cost(opts: GateOpts, fmt: int = FMT_F32, mem: int = MEM_HOST, out_mem: int = MEM_HOST, with_noise: bool = False) -> np.ndarray:
    """Host-only: the int64 [6] cost record afx_gate_batch cuts a batch with, for :func:`stft_chunks` (over
    max(length, noise length) per clip)."""
    _need_gate()
    cost = np.zeros(6, np.int64)
    _check(lib().afx_gate_cost(C.addressof(opts), int(fmt), int(mem), int(out_mem), int(bool(with_noise)), cost.ctypes.data),
           "afx_gate_cost")
    return cost


def _need_stft():
    if not hasattr(lib(), "afx_stft_batch"):
        raise NotImplementedError("this libafx has no afx_stft_batch")


def stft_opts(n_fft: int = 2048, hop_length=None, center: bool = True, pad_mode="constant", out_kind: int = STFT_COMPLEX) -> StftOpts:
    """librosa.stft's framing keywords as the record afx_stft_batch / afx_istft_batch take (hop_length None: n_fft // 4).
    ``pad_mode``: "constant", "reflect" or a PAD_* value; ValueError for any other, as for the modes librosa refuses."""
    modes = {"constant": PAD_CONSTANT, "reflect": PAD_REFLECT, PAD_CONSTANT: PAD_CONSTANT, PAD_REFLECT: PAD_REFLECT}
    if isinstance(pad_mode, bool) or pad_mode not in modes:
        raise ValueError(f"pad_mode {pad_mode!r} is not supported (constant, reflect)")
    hop = int(n_fft) // 4 if hop_length is None else int(hop_length)
    return StftOpts(int(n_fft), hop, int(bool(center)), modes[pad_mode], int(out_kind))


def stft_frames(opts: StftOpts, length: int):
    """Host-only: afx_stft_frames -> (T, status) of a clip of ``length`` samples (T = 0 unless CLIP_OK).
    NotImplementedError for an n_fft other than 1024 / 2048 or a hop outside [1, n_fft]."""
    _need_stft()
    T, st = C.c_int64(0), C.c_int32(0)
    _check(lib().afx_stft_frames(C.addressof(opts), int(length), C.addressof(T), C.addressof(st)), "afx_stft_frames")
    return int(T.value), int(st.value)


def istft_samples(opts: StftOpts, T: int, length=None):
    """Host-only: afx_istft_samples -> (frames used, samples written) by istft of ``T`` frames (``length`` None: natural)."""
    _need_stft()
    nf, no = C.c_int64(0), C.c_int64(0)
    _check(lib().afx_istft_samples(C.addressof(opts), int(T), -1 if length is None else int(length), C.addressof(nf),
                                   C.addressof(no)), "afx_istft_samples")
    return int(nf.value), int(no.value)


def stft_cost(opts: StftOpts, fmt: int = FMT_F32, mem: int = MEM_HOST, out_mem: int = MEM_HOST, inverse: bool = False) -> np.ndarray:
    """Host-only: the int64 [6] cost record afx_stft_batch (over the clips' lengths, 0 for a clip that is too short) or
    afx_istft_batch (``inverse``: over frames used + ceil(samples written / hop)) cuts a batch with, for :func:`stft_chunks`."""
    _need_stft()
    cost = np.zeros(6, np.int64)
    _check(lib().afx_stft_cost(C.addressof(opts), int(fmt), int(mem), int(out_mem), int(bool(inverse)), cost.ctypes.data),
           "afx_stft_cost")
    return cost


def _stft_window(opts: StftOpts, window) -> np.ndarray:
    window = np.ascontiguousarray(window, np.float32).reshape(-1)
    if window.shape[0] != opts.n_fft:
        raise ValueError("window must hold n_fft values (pad a shorter one centred, as librosa.util.pad_center does)")
    return window


def _need_pvoc():
    if not hasattr(lib(), "afx_pvoc_batch"):
        raise NotImplementedError("this libafx has no afx_pvoc_batch")


def pvoc_frames(n_fft: int, hop: int, T: int, rate: float):
    """Host-only: afx_pvoc_frames -> (T_out, status) of a clip of ``T`` rows stretched by ``rate``: T_out = ceil(T / rate).
    ValueError for a rate that is not finite and > 0; NotImplementedError for an odd n_fft, an n_fft outside [2, 4096], a
    hop outside [1, n_fft] or T_out x bins >= 2^31."""
    _need_pvoc()
    To, st = C.c_int64(0), C.c_int32(0)
    _check(lib().afx_pvoc_frames(int(n_fft), int(hop), int(T), float(rate), C.addressof(To), C.addressof(st)), "afx_pvoc_frames")
    return int(To.value), int(st.value)


def time_stretch_samples(opts: StftOpts, length: int, rate: float):
    """Host-only: afx_time_stretch_samples -> (T, T_out, n_out, status): the frames of a clip of ``length`` samples, the rows
    of its stretch by ``rate`` and the samples written, round(length / rate) as Python rounds."""
    _need_pvoc()
    T, To, no, st = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int32(0)
    _check(lib().afx_time_stretch_samples(C.addressof(opts), int(length), float(rate), C.addressof(T), C.addressof(To),
                                          C.addressof(no), C.addressof(st)), "afx_time_stretch_samples")
    return int(T.value), int(To.value), int(no.value), int(st.value)


def pvoc_cost(n_fft: int, mem: int = MEM_HOST, out_mem: int = MEM_HOST) -> np.ndarray:
    """Host-only: the int64 [6] cost record afx_pvoc_batch cuts a batch with (over T + T_out per clip), for :func:`stft_chunks`."""
    _need_pvoc()
    cost = np.zeros(6, np.int64)
    _check(lib().afx_pvoc_cost(int(n_fft), int(mem), int(out_mem), cost.ctypes.data), "afx_pvoc_cost")
    return cost


def time_stretch_cost(opts: StftOpts, fmt: int = FMT_F32, mem: int = MEM_HOST, out_mem: int = MEM_HOST) -> np.ndarray:
    """Host-only: the int64 [6] cost record afx_time_stretch_batch cuts a batch with (over T + T_out + ceil(length / hop) +
    ceil(n_out / hop) per clip, 0 for a clip with nothing to run), for :func:`stft_chunks`."""
    _need_pvoc()
    cost = np.zeros(6, np.int64)
    _check(lib().afx_time_stretch_cost(C.addressof(opts), int(fmt), int(mem), int(out_mem), cost.ctypes.data), "afx_time_stretch_cost")
    return cost


def pvoc_host(D, rate: float, hop_length=None, n_fft=None):
    """Host-only: afx_pvoc_host, the phase vocoder's definition in plain C++ for one [bins, T] complex64 spectrum ->
    (the [bins, T_out] complex64 result in librosa's memory order, or None for T = 0; status)."""
    _need_pvoc()
    D = np.asarray(D)
    if D.ndim != 2:
        raise NotImplementedError(f"a spectrum must be 2-D (mono), got shape {D.shape}")
    bins, T = D.shape
    n_fft = 2 * (bins - 1) if n_fft is None else int(n_fft)
    hop = n_fft // 4 if hop_length is None else int(hop_length)
    if n_fft // 2 + 1 != bins:
        raise ValueError(f"the spectrum must have 1 + n_fft / 2 = {n_fft // 2 + 1} rows")
    T_out, st = pvoc_frames(n_fft, hop, T, rate)
    rows = np.ascontiguousarray(np.asarray(D, np.complex64).T)
    out = np.zeros((T_out, bins), np.complex64)
    status = C.c_int32(0)
    _check(lib().afx_pvoc_host(rows.ctypes.data, int(T), float(rate), n_fft, hop, out.ctypes.data, C.addressof(status)), "afx_pvoc_host")
    return (out.T if T else None), int(status.value)


def _need_loudness():
    if not hasattr(lib(), "afx_loudness_batch"):
        raise NotImplementedError("this libafx has no afx_loudness_batch")


def kweight_sos(rate: int) -> np.ndarray:
    """Host-only: afx_kweight_sos, the K-weighting of BS.1770 at ``rate`` as two sections (b0 b1 b2 1 a1 a2), float64."""
    _need_loudness()
    sos = np.zeros((2, 6), np.float64)
    _check(lib().afx_kweight_sos(int(rate), sos.ctypes.data), "afx_kweight_sos")
    return sos


def loudness_geometry() -> dict:
    """Host-only: the block decomposition of afx_loudness_batch (samples per block, blocks per tile) and its bounds."""
    _need_loudness()
    info = np.zeros(5, np.int32)
    _check(lib().afx_loudness_geometry(info.ctypes.data), "afx_loudness_geometry")
    return {"block": int(info[0]), "tile_blocks": int(info[1]), "tile": int(info[0]) * int(info[1]),
            "min_rate": int(info[2]), "max_rate": int(info[3]), "max_rates": int(info[4])}


def loudness_blocks(n: int, rate: int, block_size: float = 0.400) -> int:
    """Host-only: afx_loudness_blocks, the gating blocks of a clip of ``n`` samples (0: too short to measure)."""
    _need_loudness()
    nb = C.c_int64(0)
    _check(lib().afx_loudness_blocks(int(n), int(rate), float(block_size), C.byref(nb)), "afx_loudness_blocks")
    return int(nb.value)


def loudness_cost(fmt: int = FMT_F32, mem: int = MEM_HOST, out_mem: int = MEM_HOST, mode: int = LOUD_MEASURE) -> np.ndarray:
    """Host-only: the int64 [6] cost record afx_loudness_batch cuts a batch with, for :func:`stft_chunks`."""
    _need_loudness()
    cost = np.zeros(6, np.int64)
    _check(lib().afx_loudness_cost(int(fmt), int(mem), int(out_mem), int(mode), cost.ctypes.data), "afx_loudness_cost")
    return cost


def loudness_host(x, rate: int, block_size: float = 0.400, mode: int = LOUD_MEASURE, target: float = -23.0) -> dict:
    """Host-only: afx_loudness_host, one int16 / float32 clip through the kernels' block decomposition and summation order
    on the CPU.  Returns rec (float64 [LOUD_N]; LOUD_FIELDS names the entries; NaN for a failed clip), z (every z_j),
    out (float32, the normalised clip; None in LOUD_MEASURE; the input's values when the clip failed) and status."""
    _need_loudness()
    x = _mono_clip(x, "x")
    nb = loudness_blocks(x.size, rate, block_size)
    rec, z = np.zeros(LOUD_N, np.float64), np.zeros(nb, np.float64)
    out = None if mode == LOUD_MEASURE else (x.astype(np.float32) / np.float32(32768.0) if x.dtype == np.int16 else x.copy())
    status = np.zeros(1, np.int32)
    _check(lib().afx_loudness_host(x.ctypes.data, FMT_S16 if x.dtype == np.int16 else FMT_F32, int(x.size), int(rate),
                                   float(block_size), float(target), int(mode), rec.ctypes.data, z.ctypes.data if nb else None,
                                   _ptr(out), status.ctypes.data), "afx_loudness_host")
    return {"rec": rec, "z": z, "out": out, "status": int(status[0])}


def beat_track_host(env, fps: float, bpm: float, tightness: float = 100.0, trim: bool = True) -> dict:
    """Host-only: afx_beat_track_host, one float32 onset envelope through the beat tracker's definition in float64 on the
    CPU.  Returns beats (int64 frames), mask (uint8 [T]), localscore, cumscore (float64 [T]) and backlink (int32 [T])."""
    if not hasattr(lib(), "afx_beat_track_host"):
        raise NotImplementedError("this libafx has no afx_beat_track_host")
    env = np.ascontiguousarray(env)
    if env.ndim != 1 or env.dtype != np.float32:
        raise ValueError("env must be a one-dimensional float32 array")
    T = int(env.size)
    mask = np.zeros(T, np.uint8)
    ls, cum, bl = np.zeros(T, np.float64), np.zeros(T, np.float64), np.zeros(T, np.int32)
    nb = C.c_int64(0)
    _check(lib().afx_beat_track_host(env.ctypes.data, T, float(fps), float(bpm), float(tightness), int(bool(trim)),
                                     mask.ctypes.data, C.byref(nb), ls.ctypes.data, cum.ctypes.data, bl.ctypes.data),
           "afx_beat_track_host")
    beats = np.flatnonzero(mask).astype(np.int64)
    assert beats.size == nb.value
    return {"beats": beats, "mask": mask, "localscore": ls, "cumscore": cum, "backlink": bl}


def resample_lengths(lengths, sr_in: int, sr_out: int) -> np.ndarray:
    """ceil(n * sr_out / sr_in) per clip, in integers (librosa's length rule)."""
    sr_in = np.asarray(sr_in, np.int64)              # a scalar, or one rate per clip
    g = np.gcd(sr_in, int(sr_out))
    up, down = int(sr_out) // g, sr_in // g
    return (np.asarray(lengths, np.int64) * up + down - 1) // down


def _check(rc: int, what: str):
    if rc != AFX_OK:
        msg = lib().afx_last_error().decode("utf-8", "replace")
        if rc == -5:
            raise NotImplementedError(f"{what}: {msg}")
        if rc == -1:
            raise ValueError(f"{what}: {msg}")
        raise AfxError(f"{what} failed ({rc}): {msg}")


def device_count() -> int:
    return int(lib().afx_device_count())


# The front end every batch method shares.  The C side trusts what it is handed: these checks are the only ones.
def _ptr(a):
    """Address of an optional array (None: NULL)."""
    return None if a is None else a.ctypes.data


def packed_offsets(counts, align: int = 1) -> np.ndarray:
    """Where each item starts when items of ``counts`` elements lie one after another, each rounded up to ``align``
    elements: the exclusive cumulative sum, int64 (empty for no items)."""
    counts = np.asarray(counts, np.int64).reshape(-1)
    if align > 1:
        counts = (counts + (align - 1)) // align * align
    out = np.zeros(counts.shape[0], np.int64)
    if counts.shape[0] > 1:
        np.cumsum(counts[:-1], out=out[1:])
    return out


def _clip_arrays(offsets, lengths):
    """-> (offsets, lengths, n): contiguous 1-D int64 (an array that already is one is not copied), one entry per clip."""
    offsets = np.ascontiguousarray(offsets, np.int64).reshape(-1)
    lengths = np.ascontiguousarray(lengths, np.int64).reshape(-1)
    n = int(offsets.shape[0])
    if lengths.shape[0] != n:
        raise ValueError("offsets and lengths must have one entry per clip")
    return offsets, lengths, n


def _sample_fmt(samples, fmt):
    """``fmt`` when the caller gave one; else what a numpy array's dtype says (resample_batch's convention)."""
    if fmt is not None:
        return fmt
    if isinstance(samples, np.ndarray):
        return FMT_S16 if samples.dtype == np.int16 else FMT_F32
    raise ValueError("fmt is required for device-resident samples")


def _sample_source(samples, fmt, offsets, lengths, mem=None):
    """-> (pointer, MEM_HOST | MEM_DEVICE) of a batch's samples.  ``mem`` None: a numpy array is host memory, anything
    else a DeviceBuffer or a device address; MEM_HOST / MEM_DEVICE: the caller says which, and only that is taken.
    A host array must be C-contiguous, of ``fmt``'s dtype, and hold every clip of ``_clip_arrays``' offsets / lengths."""
    if mem is None:
        mem = MEM_HOST if isinstance(samples, np.ndarray) else MEM_DEVICE
    if mem != MEM_HOST:
        return (samples.ptr if isinstance(samples, DeviceBuffer) else int(samples)), MEM_DEVICE
    want = np.int16 if fmt == FMT_S16 else np.float32
    if not isinstance(samples, np.ndarray) or samples.dtype != want or not samples.flags.c_contiguous:
        raise ValueError(f"samples must be a C-contiguous {want.__name__} array")
    if offsets.shape[0] and int((offsets + lengths).max()) > samples.size:
        raise ValueError("a clip extends past the sample buffer")
    return samples.ctypes.data, MEM_HOST


def make_params(sr=22050, n_fft=1024, hop=256, n_mfcc=13, n_mels=128, window="hamming",
                preemph=0.97, fmin=0.0, fmax=None, htk=False, lifter=0.0) -> Params:
    p = Params()
    lib().afx_default_params(C.byref(p))
    p.sr, p.n_fft, p.hop, p.n_mfcc, p.n_mels = int(sr), int(n_fft), int(hop), int(n_mfcc), int(n_mels)
    wl = {"hamming": WINDOW_HAMMING, "hann": WINDOW_HANN}
    if window not in wl:
        raise ValueError(f"unsupported window {window!r} (hamming, hann)")
    p.window = wl[window]
    p.preemph = float(preemph)
    p.fmin, p.fmax, p.htk, p.lifter = float(fmin), float(fmax or 0.0), int(bool(htk)), float(lifter)
    return p


def build_tables(p: Params):
    """Host-only: (window[n_fft], mel[n_mels, n_fft/2+1], dct[n_mfcc, n_mels]) as uploaded by a plan."""
    nb = p.n_fft // 2 + 1
    win = np.empty(p.n_fft, np.float32)
    mel = np.empty((p.n_mels, nb), np.float32)
    dct = np.empty((p.n_mfcc, p.n_mels), np.float32)
    _check(lib().afx_build_tables(C.byref(p), win.ctypes.data, mel.ctypes.data, dct.ctypes.data), "afx_build_tables")
    return win, mel, dct


def build_mel_schedule(p: Params) -> dict:
    """Host-only: the per-lane mel schedule of the wave-level frame kernel (rounds of nb batches of 4 taps)."""
    info = np.zeros(26, np.int32)
    _check(lib().afx_build_mel_schedule(C.byref(p), info.ctypes.data, None, None), "afx_build_mel_schedule")
    rounds, nw = int(info[0]), int(info[1])
    w = np.zeros(nw, np.float32)
    meta = np.zeros(64 * rounds, np.int32)
    _check(lib().afx_build_mel_schedule(C.byref(p), info.ctypes.data, w.ctypes.data, meta.ctypes.data), "afx_build_mel_schedule")
    return {"rounds": rounds, "nb": [int(info[2 + 3 * r]) for r in range(rounds)],
            "width": [int(info[3 + 3 * r]) for r in range(rounds)], "woff": [int(info[4 + 3 * r]) for r in range(rounds)],
            "weights": w, "meta": meta.reshape(rounds, 64)}


class _Owner:
    """Base of the objects that own a native resource: ``close()`` when collected (a failure there, as at interpreter
    shutdown, is ignored)."""

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceBuffer(_Owner):
    """HBM allocation owned by a Context (for device-resident batches)."""

    def __init__(self, ctx: "Context", nbytes: int):
        self.ctx, self.nbytes = ctx, int(nbytes)
        ptr = C.c_void_p()
        _check(lib().afx_malloc(ctx.handle, self.nbytes, C.byref(ptr)), "afx_malloc")
        self.ptr = ptr.value

    def upload(self, arr: np.ndarray, byte_offset: int = 0):
        arr = np.ascontiguousarray(arr)
        assert byte_offset + arr.nbytes <= self.nbytes
        _check(lib().afx_memcpy_h2d(self.ctx.handle, self.ptr + byte_offset, arr.ctypes.data, arr.nbytes), "afx_memcpy_h2d")

    def download(self, arr: np.ndarray, byte_offset: int = 0):
        """Fills the C-contiguous array ``arr`` from the buffer (synchronous)."""
        assert arr.flags.c_contiguous and byte_offset + arr.nbytes <= self.nbytes
        _check(lib().afx_memcpy_d2h(self.ctx.handle, arr.ctypes.data, self.ptr + byte_offset, arr.nbytes), "afx_memcpy_d2h")

    def free(self):
        if self.ptr:
            lib().afx_free(self.ctx.handle, self.ptr)
            self.ptr = None

    close = free


class PinnedBuffer(_Owner):
    """Page-locked host memory owned by a Context: ``array(dtype, count)`` is a numpy view of its start.  Uploads from it
    are DMA at link rate (no staging copy by the runtime)."""

    def __init__(self, ctx: "Context", nbytes: int):
        self.ctx, self.nbytes = ctx, int(nbytes)
        ptr = C.c_void_p()
        _check(lib().afx_host_alloc(ctx.handle, self.nbytes, C.byref(ptr)), "afx_host_alloc")
        self.ptr = ptr.value
        self._raw = (C.c_char * max(self.nbytes, 1)).from_address(self.ptr)

    def array(self, dtype, count: int) -> np.ndarray:
        dt = np.dtype(dtype)
        if count * dt.itemsize > self.nbytes:
            raise ValueError("view larger than the pinned block")
        return np.frombuffer(self._raw, dtype=dt, count=int(count))

    def free(self):
        if self.ptr:
            self._raw = None
            lib().afx_host_free(self.ctx.handle, self.ptr)
            self.ptr = None

    close = free


class Context(_Owner):
    """One HIP device + stream.  Not thread-safe: one per worker thread."""

    def __init__(self, device: int = 0):
        h = C.c_void_p()
        _check(lib().afx_init(int(device), C.byref(h)), f"afx_init(device={device})")
        self.handle, self.device = h, int(device)
        self._plans = weakref.WeakSet()        # closed before the context itself (their workspace lives on its stream)

    def close(self):
        if self.handle:
            for pl in list(self._plans):
                pl.close()
            lib().afx_destroy(self.handle)
            self.handle = None

    def dtw_steps_batch(self, feats, x_off, x_len, y_off, y_len, band_r=None, metric: str = "euclidean",
                        backtrack: bool = True, store_d: bool = False, steps=None, weights_add=None, weights_mul=None,
                        subseq: bool = False) -> dict:
        """afx_dtw_steps_batch: :meth:`dtw_batch` with a step list.  ``steps``: None (the default steps, with optional
        weights of three entries) or an int array [n, 2] of (di, dj); ``weights_add`` / ``weights_mul``: None or one value
        per step; ``subseq``: X is matched inside Y (as given: no swap).  Also returns ``end`` [n] int32, the column j* the
        path starts at (M - 1 without ``subseq``)."""
        st = None if steps is None else np.ascontiguousarray(steps, np.int32).reshape(-1, 2)
        k = 3 if st is None else int(st.shape[0])
        wa, wm = (None if w is None else np.ascontiguousarray(w, np.float64).reshape(-1) for w in (weights_add, weights_mul))
        for w in (wa, wm):
            if w is not None and w.shape[0] != k:
                raise ValueError(f"a weight array has {w.shape[0]} entries for {k} steps")
        return self._dtw(feats, x_off, x_len, y_off, y_len, band_r, metric, backtrack, store_d, (st, k, wa, wm, bool(subseq)))

    def dtw_batch(self, feats, x_off, x_len, y_off, y_len, band_r=None, metric: str = "euclidean",
                  backtrack: bool = True, store_d: bool = False) -> dict:
        """afx_dtw_batch: DTW of pairs of frame sequences held in one frame-major float32 buffer ``feats`` [frames, dim]
        (pair p aligns frames x_off[p] .. + x_len[p] with y_off[p] .. + y_len[p]).  ``band_r``: None, or per pair the
        band radius (< 0: unconstrained).  Returns cost [n] float64, status [n] int32 and, when asked, ``paths`` (list of
        [L, 2] int arrays, end to start; None for a failed pair) and ``D`` (list of [N, M] float64 arrays)."""
        return self._dtw(feats, x_off, x_len, y_off, y_len, band_r, metric, backtrack, store_d, None)

    def _dtw(self, feats, x_off, x_len, y_off, y_len, band_r, metric, backtrack, store_d, general) -> dict:
        feats = np.ascontiguousarray(feats, np.float32)
        if feats.ndim != 2:
            raise ValueError("feats must be [frames, dim]")
        dim = int(feats.shape[1])
        xo, xl, yo, yl = (np.ascontiguousarray(a, np.int64).reshape(-1) for a in (x_off, x_len, y_off, y_len))
        n = int(xo.shape[0])
        if not (xl.shape[0] == yo.shape[0] == yl.shape[0] == n):
            raise ValueError("x_off, x_len, y_off, y_len must have one entry per pair")
        if n and (int(np.maximum(xo + xl, yo + yl).max()) > feats.shape[0] or xo.min() < 0 or yo.min() < 0):
            raise ValueError("a pair extends past the feature buffer")
        if metric not in DTW_METRICS:
            raise ValueError(f"unsupported metric {metric!r} ({', '.join(DTW_METRICS)})")
        br = None if band_r is None else np.ascontiguousarray(band_r, np.int32).reshape(-1)
        if br is not None and br.shape[0] != n:
            raise ValueError("band_r must have one entry per pair")
        cost, status = np.zeros(n, np.float64), np.zeros(n, np.int32)
        flags = (DTW_BACKTRACK if backtrack else 0) | (DTW_STORE_D if store_d else 0)
        path = poff = plen = dmat = doff = None
        if backtrack:
            steps = xl + yl - 1
            poff = packed_offsets(steps)
            path = np.zeros((int(steps.sum()), 2), np.int32)
            plen = np.zeros(n, np.int32)
        if store_d:
            cells = xl * yl
            doff = packed_offsets(cells)
            dmat = np.empty(int(cells.sum()), np.float64)
        out = {"cost": cost, "status": status}
        if general is None:
            _check(lib().afx_dtw_batch(self.handle, feats.ctypes.data, dim, xo.ctypes.data, xl.ctypes.data, yo.ctypes.data,
                                       yl.ctypes.data, _ptr(br), n, DTW_METRICS[metric], flags, cost.ctypes.data,
                                       status.ctypes.data, _ptr(path), _ptr(poff), _ptr(plen), _ptr(dmat), _ptr(doff)),
                   "afx_dtw_batch")
        else:
            st, k, wa, wm, subseq = general
            if not hasattr(lib(), "afx_dtw_steps_batch"):
                raise AfxError("this libafx.so has no afx_dtw_steps_batch: rebuild it")
            out["end"] = end = np.zeros(n, np.int32)
            _check(lib().afx_dtw_steps_batch(self.handle, feats.ctypes.data, dim, xo.ctypes.data, xl.ctypes.data,
                                             yo.ctypes.data, yl.ctypes.data, _ptr(br), n, DTW_METRICS[metric],
                                             flags | (DTW_SUBSEQ if subseq else 0), _ptr(st), k, _ptr(wa), _ptr(wm),
                                             cost.ctypes.data, status.ctypes.data, _ptr(path), _ptr(poff), _ptr(plen),
                                             _ptr(dmat), _ptr(doff), end.ctypes.data),
                   "afx_dtw_steps_batch")
        if backtrack:
            path = path.astype(np.int64)
            out["paths"] = [path[poff[p]:poff[p] + plen[p]] if status[p] == DTW_OK else None for p in range(n)]
        if store_d:
            out["D"] = [dmat[doff[p]:doff[p] + xl[p] * yl[p]].reshape(int(xl[p]), int(yl[p])) for p in range(n)]
        return out


    def resample_batch(self, samples, offsets, lengths, sr_in: int, sr_out: int, fmt=None, taps=None, out=None,
                       out_offsets=None) -> dict:
        """afx_resample_batch: clips samples[offsets[i] .. + lengths[i]) at sr_in -> float32 at sr_out, as wavio.resample.
        ``samples``: numpy int16 / float32 array (host) or a DeviceBuffer / device pointer (then ``fmt`` says which).
        ``out``: None (a new host array), a float32 numpy array, or a DeviceBuffer the result stays in; ``out_offsets``:
        where each clip goes (default: packed with 4-element alignment, as parallel._pack).  Returns out, offsets, lengths."""
        offsets, lengths, n = _clip_arrays(offsets, lengths)
        if int(sr_in) <= 0 or int(sr_out) <= 0:
            raise ValueError("sample rates must be positive")
        fmt = _sample_fmt(samples, fmt)
        sptr, kind = _sample_source(samples, fmt, offsets, lengths)
        olen = resample_lengths(np.maximum(lengths, 0), sr_in, sr_out)
        if out_offsets is None:
            out_offsets = packed_offsets(olen, 4)
        out_offsets = np.ascontiguousarray(out_offsets, np.int64).reshape(-1)
        if out_offsets.shape[0] != n:
            raise ValueError("out_offsets must have one entry per clip")
        need = int((out_offsets + olen).max()) if n else 0
        if out is None:
            out = np.zeros(need, np.float32)
        if isinstance(out, np.ndarray):
            if out.dtype != np.float32 or not out.flags.c_contiguous or out.size < need:
                raise ValueError("out must be a C-contiguous float32 array that holds every clip")
            optr, okind = out.ctypes.data, MEM_HOST
        else:
            if isinstance(out, DeviceBuffer) and out.nbytes < 4 * need:
                raise ValueError("the output DeviceBuffer is too small")
            optr, okind = (out.ptr if isinstance(out, DeviceBuffer) else int(out)), MEM_DEVICE
        tp = None if taps is None else np.ascontiguousarray(taps, np.float64).reshape(-1)
        got = np.zeros(n, np.int64)
        if not hasattr(lib(), "afx_resample_batch"):
            raise NotImplementedError("this libafx has no afx_resample_batch")
        _check(lib().afx_resample_batch(self.handle, sptr, int(fmt), kind, offsets.ctypes.data, lengths.ctypes.data, n,
                                        int(sr_in), int(sr_out), _ptr(tp),
                                        0 if tp is None else int(tp.size), optr, okind, out_offsets.ctypes.data,
                                        got.ctypes.data), "afx_resample_batch")
        return {"out": out, "offsets": out_offsets, "lengths": got}

    def sosfiltfilt_batch(self, samples, offsets, lengths, sos, padlen: int, mode: int = FILT_PLAIN, preemph: float = 0.98,
                          fmt=None, out=None, out_offsets=None) -> dict:
        """afx_sosfiltfilt_batch: clips samples[offsets[i] .. + lengths[i]) through the zero-phase cascade ``sos`` (FILT_PLAIN)
        or through the experiment extractor's whole preprocess_audio around it (FILT_EXPERIMENT), float32 out.
        ``samples``, ``out``, ``out_offsets``: as resample_batch (outputs have their inputs' lengths).  Returns out, offsets,
        peak (max|x|, max|y| per clip) and status; the output range of a clip whose status is not CLIP_OK is not written."""
        _need_filt()
        offsets, lengths, n = _clip_arrays(offsets, lengths)
        sos = _sos_array(sos)
        fmt = _sample_fmt(samples, fmt)
        sptr, kind = _sample_source(samples, fmt, offsets, lengths)
        if out_offsets is None:
            out_offsets = packed_offsets(np.maximum(lengths, 0), 4)
        out_offsets = np.ascontiguousarray(out_offsets, np.int64).reshape(-1)
        if out_offsets.shape[0] != n:
            raise ValueError("out_offsets must have one entry per clip")
        need = int((out_offsets + np.maximum(lengths, 0)).max()) if n else 0
        if out is None:
            out = np.zeros(need, np.float32)
        if isinstance(out, np.ndarray):
            if out.dtype != np.float32 or not out.flags.c_contiguous or out.size < need:
                raise ValueError("out must be a C-contiguous float32 array that holds every clip")
            optr, okind = out.ctypes.data, MEM_HOST
        else:
            if isinstance(out, DeviceBuffer) and out.nbytes < 4 * need:
                raise ValueError("the output DeviceBuffer is too small")
            optr, okind = (out.ptr if isinstance(out, DeviceBuffer) else int(out)), MEM_DEVICE
        peak = np.zeros((n, 2), np.float64)
        status = np.zeros(n, np.int32)
        _check(lib().afx_sosfiltfilt_batch(self.handle, sptr, int(fmt), kind, offsets.ctypes.data, lengths.ctypes.data, n,
                                           sos.ctypes.data, int(sos.shape[0]), int(padlen), int(mode), float(preemph),
                                           optr, okind, out_offsets.ctypes.data, peak.ctypes.data, status.ctypes.data),
               "afx_sosfiltfilt_batch")
        return {"out": out, "offsets": out_offsets, "peak": peak, "status": status}

    def _smooth_out(self, lengths, n, out, out_offsets):
        """-> (out, out_offsets, pointer, memory kind) of a filter whose outputs have their inputs' lengths (resample_batch's
        conventions for ``out`` and ``out_offsets``)"""
        if out_offsets is None:
            out_offsets = packed_offsets(np.maximum(lengths, 0), 4)
        out_offsets = np.ascontiguousarray(out_offsets, np.int64).reshape(-1)
        if out_offsets.shape[0] != n:
            raise ValueError("out_offsets must have one entry per clip")
        need = int((out_offsets + np.maximum(lengths, 0)).max()) if n else 0
        if out is None:
            out = np.zeros(need, np.float32)
        if isinstance(out, np.ndarray):
            if out.dtype != np.float32 or not out.flags.c_contiguous or out.size < need:
                raise ValueError("out must be a C-contiguous float32 array that holds every clip")
            return out, out_offsets, out.ctypes.data, MEM_HOST
        if isinstance(out, DeviceBuffer) and out.nbytes < 4 * need:
            raise ValueError("the output DeviceBuffer is too small")
        return out, out_offsets, (out.ptr if isinstance(out, DeviceBuffer) else int(out)), MEM_DEVICE

    def medfilt_batch(self, samples, offsets, lengths, kernel_size: int = 3, fmt=None, out=None, out_offsets=None) -> dict:
        """afx_medfilt_batch: scipy.signal.medfilt(x, kernel_size) of the clips samples[offsets[i] .. + lengths[i]), float32
        out.  ``samples``, ``out``, ``out_offsets``: as sosfiltfilt_batch.  Returns out, offsets and status; the output range
        of a clip whose status is not CLIP_OK (empty, or not finite) is not written."""
        _need_smooth()
        offsets, lengths, n = _clip_arrays(offsets, lengths)
        fmt = _sample_fmt(samples, fmt)
        sptr, kind = _sample_source(samples, fmt, offsets, lengths)
        out, out_offsets, optr, okind = self._smooth_out(lengths, n, out, out_offsets)
        status = np.zeros(n, np.int32)
        _check(lib().afx_medfilt_batch(self.handle, sptr, int(fmt), kind, offsets.ctypes.data, lengths.ctypes.data, n,
                                       int(kernel_size), optr, okind, out_offsets.ctypes.data, status.ctypes.data),
               "afx_medfilt_batch")
        return {"out": out, "offsets": out_offsets, "status": status}

    def savgol_batch(self, samples, offsets, lengths, window_length: int, polyorder: int, deriv: int = 0, delta: float = 1.0,
                     fmt=None, out=None, out_offsets=None) -> dict:
        """afx_savgol_batch: scipy.signal.savgol_filter(x, window_length, polyorder, deriv, delta, mode='interp') of the
        clips, float32 out; otherwise as medfilt_batch (a clip shorter than the window is CLIP_TOO_SHORT)."""
        _need_smooth()
        offsets, lengths, n = _clip_arrays(offsets, lengths)
        fmt = _sample_fmt(samples, fmt)
        sptr, kind = _sample_source(samples, fmt, offsets, lengths)
        out, out_offsets, optr, okind = self._smooth_out(lengths, n, out, out_offsets)
        status = np.zeros(n, np.int32)
        _check(lib().afx_savgol_batch(self.handle, sptr, int(fmt), kind, offsets.ctypes.data, lengths.ctypes.data, n,
                                      int(window_length), int(polyorder), int(deriv), float(delta), optr, okind,
                                      out_offsets.ctypes.data, status.ctypes.data), "afx_savgol_batch")
        return {"out": out, "offsets": out_offsets, "status": status}

    def loudness_batch(self, samples, offsets, lengths, rates, block_size: float = 0.400, mode: int = LOUD_MEASURE,
                       target: float = -23.0, want_blocks: bool = False, fmt=None, out=None, out_offsets=None) -> dict:
        """afx_loudness_batch: BS.1770 integrated loudness of the clips samples[offsets[i] .. + lengths[i]), clip i at its own
        rate ``rates[i]`` (a scalar: one rate for all), and in LOUD_NORM_LOUDNESS / LOUD_NORM_PEAK the clips scaled to
        ``target`` LUFS / dB peak, float32 out.  ``samples``, ``out``, ``out_offsets``: as sosfiltfilt_batch (``out`` is neither
        made nor written in LOUD_MEASURE).  Returns rec (float64 [n, LOUD_N]; LOUD_FIELDS names the entries; NaN for a failed
        clip), status and, in a normalising mode, out and offsets (the output range of a clip whose status is not CLIP_OK is
        not written); with ``want_blocks`` also z (every z_j, clip after clip) and z_offsets."""
        _need_loudness()
        offsets, lengths, n = _clip_arrays(offsets, lengths)
        rates = np.ascontiguousarray(np.broadcast_to(np.asarray(rates, np.int32), (n,)))
        fmt = _sample_fmt(samples, fmt)
        sptr, kind = _sample_source(samples, fmt, offsets, lengths)
        res = {}
        optr, okind, ooff = None, MEM_HOST, None
        if mode != LOUD_MEASURE:
            out, out_offsets, optr, okind = self._smooth_out(lengths, n, out, out_offsets)
            ooff = out_offsets.ctypes.data
            res.update(out=out, offsets=out_offsets)
        rec = np.zeros((n, LOUD_N), np.float64)
        status = np.zeros(n, np.int32)
        z = z_off = None
        if want_blocks:
            counts = np.array([loudness_blocks(int(l), int(r), block_size) for l, r in zip(lengths, rates)], np.int64)
            z_off = packed_offsets(counts)
            z = np.zeros(int(counts.sum()), np.float64)
            res.update(z=z, z_offsets=z_off, z_counts=counts)
        _check(lib().afx_loudness_batch(self.handle, sptr, int(fmt), kind, offsets.ctypes.data, lengths.ctypes.data,
                                        rates.ctypes.data, n, float(block_size), int(mode), float(target), rec.ctypes.data,
                                        _ptr(z), _ptr(z_off), optr, okind, ooff, status.ctypes.data), "afx_loudness_batch")
        res.update(rec=rec, status=status)
        return res

    def gate_batch(self, samples, offsets, lengths, opts: GateOpts, noise_offsets=None, noise_lengths=None, fmt=None,
                   out=None, out_offsets=None, want_thresh: bool = False, want_mask: bool = False) -> dict:
        """afx_gate_batch: spectral-gating noise reduction (noisereduce.reduce_noise as :func:`gate_opts` records it) of the
        clips samples[offsets[i] .. + lengths[i]), float32 out.  ``noise_offsets`` / ``noise_lengths``: each clip's noise clip
        in the same buffer (stationary; None: the clip itself).  ``samples``, ``out``, ``out_offsets``: as sosfiltfilt_batch.
        Returns out, offsets and status (CLIP_TOO_SHORT, CLIP_TOO_LONG: the clip's output range is not written;
        CLIP_NONFINITE: zeros); stationary with ``want_thresh``: thresh, float64 [n, n_fft / 2 + 1] in dB; with ``want_mask``:
        mask, a list of bool [n_fft / 2 + 1, T] arrays (None for a clip that is empty or too long)."""
        _need_gate()
        offsets, lengths, n = _clip_arrays(offsets, lengths)
        fmt = _sample_fmt(samples, fmt)
        sptr, kind = _sample_source(samples, fmt, offsets, lengths)
        if (noise_offsets is None) != (noise_lengths is None):
            raise ValueError("noise_offsets and noise_lengths come together")
        n_off = n_len = None
        if noise_offsets is not None:
            n_off, n_len, nn = _clip_arrays(noise_offsets, noise_lengths)
            if nn != n:
                raise ValueError("noise_offsets must have one entry per clip")
            _sample_source(samples, fmt, n_off, n_len)
        out, out_offsets, optr, okind = self._smooth_out(lengths, n, out, out_offsets)
        status = np.zeros(n, np.int32)
        bins, words = opts.n_fft // 2 + 1, (opts.n_fft // 2 + 1 + 31) // 32
        stat = bool(opts.stationary)
        thresh = np.zeros((n, bins), np.float64) if (want_thresh and stat) else None
        frames = [0 if (l == 0 or l > opts.chunk_size or (stat and n_len is not None and n_len[i] == 0))
                  else 1 + (int(l) + 2 * opts.padding) // max(opts.hop, 1) for i, l in enumerate(lengths)]
        plane = np.zeros(sum(frames) * words, np.uint32) if (want_mask and stat) else None
        _check(lib().afx_gate_batch(self.handle, sptr, int(fmt), kind, offsets.ctypes.data, lengths.ctypes.data, n,
                                    _ptr(n_off), _ptr(n_len), C.addressof(opts), optr, okind, out_offsets.ctypes.data,
                                    _ptr(thresh), _ptr(plane), status.ctypes.data), "afx_gate_batch")
        res = {"out": out, "offsets": out_offsets, "status": status}
        if thresh is not None:
            res["thresh"] = thresh
        if plane is not None:
            masks, pos = [], 0
            for T in frames:
                if T == 0:
                    masks.append(None)
                    continue
                w = plane[pos:pos + T * words].reshape(T, words)
                b = np.unpackbits(w.view(np.uint8), axis=1, bitorder="little")[:, :bins]
                masks.append(np.ascontiguousarray(b.T.astype(bool)))
                pos += T * words
            res["mask"] = masks
        return res

    def stft_batch(self, samples, offsets, lengths, opts: StftOpts, window, fmt=None, out=None, out_offsets=None) -> dict:
        """afx_stft_batch: librosa.stft of the clips samples[offsets[i] .. + lengths[i]) with the framing of ``opts``
        (:func:`stft_opts`) and ``window`` (n_fft float32 values).  Clip i takes frames[i] rows of n_fft / 2 + 1 elements
        (complex64, or float32 for STFT_MAG / STFT_POWER) from element ``out_offsets[i]`` (default: packed) of ``out``: None
        (a new host array), a numpy array of the element type, or a DeviceBuffer / device address the result stays in.
        Returns out, offsets, frames, status (CLIP_TOO_SHORT: no rows; CLIP_NONFINITE: zeros) and, for a host result, spec:
        per clip the [n_fft / 2 + 1, frames] view in librosa's memory order (None for a failed clip)."""
        _need_stft()
        offsets, lengths, n = _clip_arrays(offsets, lengths)
        fmt = _sample_fmt(samples, fmt)
        sptr, kind = _sample_source(samples, fmt, offsets, lengths)
        window = _stft_window(opts, window)
        bins = opts.n_fft // 2 + 1
        dt = np.complex64 if opts.out_kind == STFT_COMPLEX else np.float32
        frames = np.array([stft_frames(opts, int(l))[0] for l in lengths], np.int64)
        if out_offsets is None:
            out_offsets = packed_offsets(frames * bins)
        out_offsets = np.ascontiguousarray(out_offsets, np.int64).reshape(-1)
        if out_offsets.shape[0] != n:
            raise ValueError("out_offsets must have one entry per clip")
        need = int((out_offsets + frames * bins).max()) if n else 0
        if out is None:
            out = np.zeros(need, dt)
        if isinstance(out, np.ndarray):
            if out.dtype != dt or not out.flags.c_contiguous or out.size < need:
                raise ValueError(f"out must be a C-contiguous {np.dtype(dt).name} array that holds every clip")
            optr, okind = out.ctypes.data, MEM_HOST
        else:
            if isinstance(out, DeviceBuffer) and out.nbytes < np.dtype(dt).itemsize * need:
                raise ValueError("the output DeviceBuffer is too small")
            optr, okind = (out.ptr if isinstance(out, DeviceBuffer) else int(out)), MEM_DEVICE
        status = np.zeros(n, np.int32)
        _check(lib().afx_stft_batch(self.handle, sptr, int(fmt), kind, offsets.ctypes.data, lengths.ctypes.data, n,
                                    C.addressof(opts), window.ctypes.data, optr, okind, out_offsets.ctypes.data,
                                    status.ctypes.data), "afx_stft_batch")
        res = {"out": out, "offsets": out_offsets, "frames": frames, "status": status}
        if okind == MEM_HOST:
            flat = out.reshape(-1)
            res["spec"] = [flat[o:o + T * bins].reshape(T, bins).T if st == CLIP_OK else None
                           for o, T, st in zip(out_offsets, frames, status)]
        return res

    def istft_batch(self, spec, spec_offsets, n_frames, opts: StftOpts, window, lengths=None, out=None, out_offsets=None) -> dict:
        """afx_istft_batch: librosa.istft of the spectra in ``spec``, a C-contiguous complex64 numpy array or a DeviceBuffer /
        device address: clip i is n_frames[i] rows of n_fft / 2 + 1 bins from element ``spec_offsets[i]``, frame after frame
        (the memory of librosa's Fortran-ordered array).  ``lengths``: None, or per clip the ``length`` asked for (negative:
        none).  ``out`` / ``out_offsets``: as sosfiltfilt_batch.  Returns out, offsets, samples (written per clip), status."""
        _need_stft()
        spec_offsets, n_frames, n = _clip_arrays(spec_offsets, n_frames)
        window = _stft_window(opts, window)
        bins = opts.n_fft // 2 + 1
        if isinstance(spec, np.ndarray):
            if spec.dtype != np.complex64 or not spec.flags.c_contiguous:
                raise ValueError("spec must be a C-contiguous complex64 array")
            if n and int((spec_offsets + n_frames * bins).max()) > spec.size:
                raise ValueError("a clip extends past the spectrum buffer")
            sptr, kind = spec.ctypes.data, MEM_HOST
        else:
            sptr, kind = (spec.ptr if isinstance(spec, DeviceBuffer) else int(spec)), MEM_DEVICE
        if lengths is not None:
            lengths = np.ascontiguousarray(lengths, np.int64).reshape(-1)
            if lengths.shape[0] != n:
                raise ValueError("lengths must have one entry per clip")
        samples = np.array([istft_samples(opts, int(T), None if lengths is None or lengths[i] < 0 else int(lengths[i]))[1]
                            for i, T in enumerate(n_frames)], np.int64)
        out, out_offsets, optr, okind = self._smooth_out(samples, n, out, out_offsets)
        status = np.zeros(n, np.int32)
        _check(lib().afx_istft_batch(self.handle, sptr, kind, spec_offsets.ctypes.data, n_frames.ctypes.data, n,
                                     C.addressof(opts), window.ctypes.data, _ptr(lengths), optr, okind,
                                     out_offsets.ctypes.data, status.ctypes.data), "afx_istft_batch")
        return {"out": out, "offsets": out_offsets, "samples": samples, "status": status}

    def pvoc_batch(self, spec, spec_offsets, n_frames, rates, n_fft: int, hop: int, out=None, out_offsets=None) -> dict:
        """afx_pvoc_batch: librosa.phase_vocoder of the spectra in ``spec`` (as istft_batch takes them), clip i stretched by
        ``rates[i]``.  Clip i takes frames[i] = ceil(n_frames[i] / rates[i]) rows of n_fft / 2 + 1 complex64 from element
        ``out_offsets[i]`` (default: packed) of ``out``: None (a new host array), a complex64 numpy array, or a DeviceBuffer /
        device address.  Returns out, offsets, frames, status (CLIP_TOO_SHORT: no rows; CLIP_NONFINITE: zeros) and, for a
        host result, spec: per clip the [n_fft / 2 + 1, frames] view in librosa's memory order (None for a failed clip)."""
        _need_pvoc()
        spec_offsets, n_frames, n = _clip_arrays(spec_offsets, n_frames)
        rates = np.ascontiguousarray(rates, np.float64).reshape(-1)
        if rates.shape[0] != n:
            raise ValueError("rates must have one entry per clip")
        n_fft, hop = int(n_fft), int(hop)
        bins = n_fft // 2 + 1
        if isinstance(spec, np.ndarray):
            if spec.dtype != np.complex64 or not spec.flags.c_contiguous:
                raise ValueError("spec must be a C-contiguous complex64 array")
            if n and int((spec_offsets + n_frames * bins).max()) > spec.size:
                raise ValueError("a clip extends past the spectrum buffer")
            sptr, kind = spec.ctypes.data, MEM_HOST
        else:
            sptr, kind = (spec.ptr if isinstance(spec, DeviceBuffer) else int(spec)), MEM_DEVICE
        frames = np.array([pvoc_frames(n_fft, hop, int(T), float(r))[0] for T, r in zip(n_frames, rates)], np.int64)
        if out_offsets is None:
            out_offsets = packed_offsets(frames * bins)
        out_offsets = np.ascontiguousarray(out_offsets, np.int64).reshape(-1)
        if out_offsets.shape[0] != n:
            raise ValueError("out_offsets must have one entry per clip")
        need = int((out_offsets + frames * bins).max()) if n else 0
        if out is None:
            out = np.zeros(need, np.complex64)
        if isinstance(out, np.ndarray):
            if out.dtype != np.complex64 or not out.flags.c_contiguous or out.size < need:
                raise ValueError("out must be a C-contiguous complex64 array that holds every clip")
            optr, okind = out.ctypes.data, MEM_HOST
        else:
            if isinstance(out, DeviceBuffer) and out.nbytes < 8 * need:
                raise ValueError("the output DeviceBuffer is too small")
            optr, okind = (out.ptr if isinstance(out, DeviceBuffer) else int(out)), MEM_DEVICE
        status = np.zeros(n, np.int32)
        _check(lib().afx_pvoc_batch(self.handle, sptr, kind, spec_offsets.ctypes.data, n_frames.ctypes.data, rates.ctypes.data, n,
                                    n_fft, hop, optr, okind, out_offsets.ctypes.data, status.ctypes.data), "afx_pvoc_batch")
        res = {"out": out, "offsets": out_offsets, "frames": frames, "status": status}
        if okind == MEM_HOST:
            flat = out.reshape(-1)
            res["spec"] = [flat[o:o + T * bins].reshape(T, bins).T if st == CLIP_OK else None
                           for o, T, st in zip(out_offsets, frames, status)]
        return res

    def time_stretch_batch(self, samples, offsets, lengths, rates, opts: StftOpts, window, fmt=None, out=None, out_offsets=None) -> dict:
        """afx_time_stretch_batch: librosa.effects.time_stretch of the clips samples[offsets[i] .. + lengths[i]) by ``rates[i]``
        with the framing of ``opts`` and ``window``: stft, phase vocoder and istft in one call, the spectra staying on the
        device.  ``samples``, ``out``, ``out_offsets``: as sosfiltfilt_batch.  Returns out, offsets, samples (written per clip:
        round(length / rate)) and status."""
        _need_pvoc()
        offsets, lengths, n = _clip_arrays(offsets, lengths)
        rates = np.ascontiguousarray(rates, np.float64).reshape(-1)
        if rates.shape[0] != n:
            raise ValueError("rates must have one entry per clip")
        fmt = _sample_fmt(samples, fmt)
        sptr, kind = _sample_source(samples, fmt, offsets, lengths)
        window = _stft_window(opts, window)
        n_out = np.array([time_stretch_samples(opts, int(L), float(r))[2] for L, r in zip(lengths, rates)], np.int64)
        out, out_offsets, optr, okind = self._smooth_out(n_out, n, out, out_offsets)
        status = np.zeros(n, np.int32)
        _check(lib().afx_time_stretch_batch(self.handle, sptr, int(fmt), kind, offsets.ctypes.data, lengths.ctypes.data,
                                            rates.ctypes.data, n, C.addressof(opts), window.ctypes.data, optr, okind,
                                            out_offsets.ctypes.data, status.ctypes.data), "afx_time_stretch_batch")
        return {"out": out, "offsets": out_offsets, "samples": n_out, "status": status}

    def energy_zcr_batch(self, samples, offsets, lengths, sr: int, frame_length: int = 2048, hop_length: int = 512,
                         flags: int = EZ_PREPROCESS | EZ_ENERGY | EZ_ZCR, fmt=None) -> dict:
        """afx_energy_zcr_batch: the experiment extractor's energy and ZCR groups of the clips at rate ``sr``.  Returns rec
        (float64 [n, EZ_N]; EZ_FIELDS names the entries; NaN for a group not asked for and for a failed clip) and status."""
        _need_smooth()
        offsets, lengths, n = _clip_arrays(offsets, lengths)
        fmt = _sample_fmt(samples, fmt)
        sptr, kind = _sample_source(samples, fmt, offsets, lengths)
        rec = np.zeros((n, EZ_N), np.float64)
        status = np.zeros(n, np.int32)
        _check(lib().afx_energy_zcr_batch(self.handle, sptr, int(fmt), kind, offsets.ctypes.data, lengths.ctypes.data, n,
                                          int(sr), int(frame_length), int(hop_length), int(flags), rec.ctypes.data,
                                          status.ctypes.data), "afx_energy_zcr_batch")
        return {"rec": rec, "status": status}

    def decode_batch(self, raw, byte_offsets, frames, kinds, channels, out=None, out_offsets=None) -> dict:
        """afx_decode_batch: raw WAVE data -> mono float32, bit for bit wavio.to_mono(wavio.to_float32(...)).  Clip i is
        ``frames[i]`` interleaved frames of ``channels[i]`` (1 .. 7) channels of kind ``kinds[i]`` (SMP_*) from byte
        ``byte_offsets[i]`` (a multiple of 16) of ``raw``: a uint8 numpy array (host) or a DeviceBuffer / device pointer.
        ``out``: None (a new host array), a float32 numpy array, or a DeviceBuffer the result stays in; ``out_offsets``:
        where each clip goes (multiples of 4; default: packed with 4-element alignment, as parallel._pack).  The elements
        from a clip's end to the next multiple of 4 are zeroed.  Returns out, offsets, lengths."""
        byte_offsets, frames, n = _clip_arrays(byte_offsets, frames)
        kinds = np.ascontiguousarray(kinds, np.int32).reshape(-1)
        channels = np.ascontiguousarray(channels, np.int32).reshape(-1)
        if kinds.shape[0] != n or channels.shape[0] != n:
            raise ValueError("kinds and channels must have one entry per clip")
        if not hasattr(lib(), "afx_decode_batch"):
            raise NotImplementedError("this libafx has no afx_decode_batch")
        flen = np.maximum(frames, 0)
        if isinstance(raw, np.ndarray):
            if raw.dtype != np.uint8 or not raw.flags.c_contiguous:
                raise ValueError("raw must be a C-contiguous uint8 array")
            known = (kinds >= 0) & (kinds < 6)
            nbytes = flen * SMP_BYTES[np.where(known, kinds, 0)] * np.maximum(channels, 0)
            if n and int((byte_offsets + np.where(known, nbytes, 0)).max()) > raw.size:
                raise ValueError("a clip extends past the raw buffer")
            rptr, rkind = raw.ctypes.data, MEM_HOST
        else:
            rptr, rkind = (raw.ptr if isinstance(raw, DeviceBuffer) else int(raw)), MEM_DEVICE
        if out_offsets is None:
            out_offsets = packed_offsets(flen, 4)
        out_offsets = np.ascontiguousarray(out_offsets, np.int64).reshape(-1)
        if out_offsets.shape[0] != n:
            raise ValueError("out_offsets must have one entry per clip")
        need = int((out_offsets + (flen + 3) // 4 * 4).max()) if n else 0
        if out is None:
            out = np.zeros(need, np.float32)
        if isinstance(out, np.ndarray):
            if out.dtype != np.float32 or not out.flags.c_contiguous or out.size < need:
                raise ValueError("out must be a C-contiguous float32 array that holds every clip, padded to 4 elements")
            optr, okind = out.ctypes.data, MEM_HOST
        else:
            if isinstance(out, DeviceBuffer) and out.nbytes < 4 * need:
                raise ValueError("the output DeviceBuffer is too small")
            optr, okind = (out.ptr if isinstance(out, DeviceBuffer) else int(out)), MEM_DEVICE
        _check(lib().afx_decode_batch(self.handle, rptr, rkind, byte_offsets.ctypes.data, frames.ctypes.data,
                                      kinds.ctypes.data, channels.ctypes.data, n, optr, okind, out_offsets.ctypes.data),
               "afx_decode_batch")
        return {"out": out, "offsets": out_offsets, "lengths": frames}

    def assess_batch(self, samples, offsets, lengths, frame_short, frame_long, threshold_db: float = -40.0,
                     noise_cap: int = 2000, fmt=None) -> dict:
        """afx_assess_batch: the recording screen's reductions of clips samples[offsets[i] .. + lengths[i]), each with its own
        two frame lengths (int(0.01 sr), int(0.1 sr) at the clip's rate).  ``samples``: an int16 / float32 numpy array
        (host) or a DeviceBuffer / device pointer (``fmt`` required).  Returns rec (float64 [n, ASSESS_N], NaN rows for
        failed clips; ASSESS_FIELDS names the columns) and status."""
        _need_assess()
        offsets, lengths, n = _clip_arrays(offsets, lengths)
        fs = np.ascontiguousarray(frame_short, np.int32).reshape(-1)
        fl = np.ascontiguousarray(frame_long, np.int32).reshape(-1)
        if fs.shape[0] != n or fl.shape[0] != n:
            raise ValueError("frame_short and frame_long must have one entry per clip")
        fmt = _sample_fmt(samples, fmt)
        sptr, kind = _sample_source(samples, fmt, offsets, np.maximum(lengths, 0))
        rec = np.full((n, ASSESS_N), np.nan, np.float64)
        status = np.zeros(n, np.int32)
        _check(lib().afx_assess_batch(self.handle, sptr, int(fmt), kind, offsets.ctypes.data, lengths.ctypes.data,
                                      fs.ctypes.data, fl.ctypes.data, n, float(threshold_db), int(noise_cap),
                                      rec.ctypes.data, status.ctypes.data), "afx_assess_batch")
        return {"rec": rec, "status": status}

    def compare_batch(self, ref, ref_offsets, ref_lengths, deg, deg_offsets, deg_lengths, fmt=None) -> dict:
        """afx_compare_batch: the sums behind correlation, MSE and the SNR of the difference for pairs
        ref[ref_offsets[i] .. + ref_lengths[i]) / deg[deg_offsets[i] .. + deg_lengths[i]), over the shorter length of each
        pair.  ``ref`` and ``deg``: numpy arrays of one sample type, or DeviceBuffers / device pointers (``fmt`` required;
        they may be one buffer).  Returns rec (float64 [n, COMPARE_N]; COMPARE_FIELDS names the columns) and status."""
        _need_assess()
        ref_offsets, ref_lengths, n = _clip_arrays(ref_offsets, ref_lengths)
        deg_offsets, deg_lengths, nd = _clip_arrays(deg_offsets, deg_lengths)
        if nd != n:
            raise ValueError("both sides must have one entry per pair")
        if isinstance(ref, np.ndarray) != isinstance(deg, np.ndarray):
            raise ValueError("ref and deg must both be host arrays or both be device memory")
        fmt = _sample_fmt(ref, fmt)
        rptr, kind = _sample_source(ref, fmt, ref_offsets, np.maximum(ref_lengths, 0))
        dptr, _ = _sample_source(deg, fmt, deg_offsets, np.maximum(deg_lengths, 0))
        rec = np.full((n, COMPARE_N), np.nan, np.float64)
        status = np.zeros(n, np.int32)
        _check(lib().afx_compare_batch(self.handle, rptr, dptr, int(fmt), kind, ref_offsets.ctypes.data, ref_lengths.ctypes.data,
                                       deg_offsets.ctypes.data, deg_lengths.ctypes.data, n, rec.ctypes.data, status.ctypes.data),
               "afx_compare_batch")
        return {"rec": rec, "status": status}

    def specdist_batch(self, ref, ref_offsets, ref_lengths, deg, deg_offsets, deg_lengths, fmt=None) -> dict:
        """afx_specdist_batch: for the pairs of ``compare_batch`` (same arguments), over the shorter length n of each pair,
        the sums behind the spectral distance of the two whole-clip magnitude spectra.  Returns rec (float64
        [n, SPECDIST_N]; SPECDIST_FIELDS names the columns) and status.  NotImplementedError past CFFT_MAX_N samples."""
        _need_specdist()
        ref_offsets, ref_lengths, n = _clip_arrays(ref_offsets, ref_lengths)
        deg_offsets, deg_lengths, nd = _clip_arrays(deg_offsets, deg_lengths)
        if nd != n:
            raise ValueError("both sides must have one entry per pair")
        if isinstance(ref, np.ndarray) != isinstance(deg, np.ndarray):
            raise ValueError("ref and deg must both be host arrays or both be device memory")
        fmt = _sample_fmt(ref, fmt)
        rptr, kind = _sample_source(ref, fmt, ref_offsets, np.maximum(ref_lengths, 0))
        dptr, _ = _sample_source(deg, fmt, deg_offsets, np.maximum(deg_lengths, 0))
        rec = np.full((n, SPECDIST_N), np.nan, np.float64)
        status = np.zeros(n, np.int32)
        _check(lib().afx_specdist_batch(self.handle, rptr, dptr, int(fmt), kind, ref_offsets.ctypes.data, ref_lengths.ctypes.data,
                                        deg_offsets.ctypes.data, deg_lengths.ctypes.data, n, rec.ctypes.data, status.ctypes.data),
               "afx_specdist_batch")
        return {"rec": rec, "status": status}

    def clip_fft_batch(self, samples, offsets, lengths, fmt=None) -> dict:
        """afx_clip_fft_batch: np.fft.rfft of every clip samples[offsets[i] .. + lengths[i]), whatever its length.
        ``samples``: an int16 / float32 numpy array (host) or a DeviceBuffer / device pointer (``fmt`` required).  Returns
        bins (complex128, clip after clip), offsets (where each clip's lengths[i] // 2 + 1 bins begin) and status (a clip
        with a NaN / inf sample: NaN bins; an empty clip: no bins)."""
        _need_specdist()
        offsets, lengths, n = _clip_arrays(offsets, lengths)
        fmt = _sample_fmt(samples, fmt)
        sptr, kind = _sample_source(samples, fmt, offsets, np.maximum(lengths, 0))
        nb = np.where(lengths > 0, np.maximum(lengths, 0) // 2 + 1, 0).astype(np.int64)
        out_offsets = np.zeros(n, np.int64)
        if n:
            out_offsets[1:] = np.cumsum(nb)[:-1]
        bins = np.zeros(max(int(nb.sum()), 1), np.complex128)
        status = np.zeros(n, np.int32)
        _check(lib().afx_clip_fft_batch(self.handle, sptr, int(fmt), kind, offsets.ctypes.data, lengths.ctypes.data, n,
                                        bins.ctypes.data, out_offsets.ctypes.data, status.ctypes.data), "afx_clip_fft_batch")
        return {"bins": bins[:int(nb.sum())], "offsets": out_offsets, "counts": nb, "status": status}


class Plan(_Owner):
    def __init__(self, ctx: Context, params: Params):
        self.ctx, self.params = ctx, params
        h = C.c_void_p()
        _check(lib().afx_plan_create(ctx.handle, C.byref(params), C.byref(h)), "afx_plan_create")
        self.handle = h
        ctx._plans.add(self)
        self.n_stats = 4 * params.n_mfcc + 3
        self._pending = None                   # (out, keep, want_frames) between extract_submit and extract_collect

    def close(self):
        if self.handle:
            lib().afx_plan_destroy(self.handle)
            self.handle = None

    def device_buffer(self, nbytes: int) -> "DeviceBuffer":
        """HBM allocation on this plan's device (the seam parallel.process_files uploads a window through)."""
        return DeviceBuffer(self.ctx, nbytes)

    def pinned_buffer(self, nbytes: int) -> "PinnedBuffer":
        """Page-locked host block on this plan's device context (what a window of files is packed into)."""
        return PinnedBuffer(self.ctx, nbytes)

    def resample_batch(self, samples, offsets, lengths, sr_in: int, sr_out: int, **kw) -> dict:
        """Context.resample_batch on this plan's context (synchronous on return: any plan may read the result)."""
        return self.ctx.resample_batch(samples, offsets, lengths, sr_in, sr_out, **kw)

    def decode_batch(self, raw, byte_offsets, frames, kinds, channels, **kw) -> dict:
        """Context.decode_batch on this plan's context (synchronous on return: any plan may read the result)."""
        return self.ctx.decode_batch(raw, byte_offsets, frames, kinds, channels, **kw)

    def set_timing(self, on, frames_only: bool = False):
        """HIP events around every kernel of a batch (or, frames_only, around the frame kernel alone)."""
        _check(lib().afx_plan_set_timing(self.handle, (2 if frames_only else 1) if on else 0), "afx_plan_set_timing")

    def timings(self, reset: bool = True):
        ms = np.zeros(len(K_NAMES), np.float32)
        n = np.zeros(len(K_NAMES), np.int32)
        _check(lib().afx_plan_get_timings(self.handle, ms.ctypes.data, n.ctypes.data, 1 if reset else 0), "afx_plan_get_timings")
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(K_NAMES)}

    def intervals(self, kernel: str = "frames", cap: int = 65536) -> np.ndarray:
        """[n, 2] (start, end) ms of the kernel's launches since the last timings(reset=True), on the device-wide clock."""
        st, en = np.zeros(cap), np.zeros(cap)
        cnt = C.c_int32()
        _check(lib().afx_plan_get_intervals(self.handle, K_NAMES.index(kernel), st.ctypes.data, en.ctypes.data, cap, C.byref(cnt)),
               "afx_plan_get_intervals")
        n = min(int(cnt.value), cap)
        return np.stack([st[:n], en[:n]], axis=1)

    def _extract_args(self, samples, offsets, lengths, flags, fmt, want_frames, out):
        offsets, lengths, n = _clip_arrays(offsets, lengths)
        sptr, kind = _sample_source(samples, fmt, offsets, lengths)
        K, hop = self.params.n_mfcc, self.params.hop
        if out is None:
            out = {
                "stats": np.zeros((n, self.n_stats), np.float32),
                "status": np.zeros(n, np.int32),
                "trim": np.zeros((n, 2), np.int64),
                "nframes": np.zeros(n, np.int32),
            }
        frames = foffs = None
        if want_frames:
            cnt = (3 * K + 1) * (1 + lengths // hop)
            foffs = packed_offsets(cnt)
            frames = np.zeros(int(cnt.sum()), np.float32)
        args = (self.handle, sptr, int(fmt), kind, offsets.ctypes.data, lengths.ctypes.data, n, int(flags),
                out["stats"].ctypes.data, out["status"].ctypes.data, out["trim"].ctypes.data,
                out["nframes"].ctypes.data, _ptr(frames), _ptr(foffs))
        keep = (samples, offsets, lengths, frames, foffs)       # alive until the call (or the collect) is over
        return args, out, keep

    def _frames_out(self, out, keep, want_frames):
        if want_frames:
            _, _, lengths, frames, foffs = keep
            K, hop = self.params.n_mfcc, self.params.hop
            res = []
            for i in range(int(lengths.shape[0])):
                tm, T = int(1 + lengths[i] // hop), int(out["nframes"][i])
                blk = frames[foffs[i]: foffs[i] + (3 * K + 1) * tm].reshape(3 * K + 1, tm)[:, :T]
                res.append({"mfcc": blk[:K].copy(), "mfcc_delta": blk[K:2 * K].copy(),
                            "mfcc_delta2": blk[2 * K:3 * K].copy(), "rms": blk[3 * K:].copy()})
            out["frames"] = res
        return out

    def extract_batch(self, samples, offsets, lengths, flags=FLAG_PREEMPH | FLAG_TRIM,
                      fmt=FMT_F32, want_frames: bool = False, out=None):
        """samples: numpy array (host) or DeviceBuffer/int device pointer.  Returns a dict with
        stats [n, 4K+3], status [n], trim [n, 2], nframes [n] (and frames list when asked)."""
        args, out, keep = self._extract_args(samples, offsets, lengths, flags, fmt, want_frames, out)
        _check(lib().afx_extract_batch(*args), "afx_extract_batch")
        return self._frames_out(out, keep, want_frames)

    def extract_submit(self, samples, offsets, lengths, flags=FLAG_PREEMPH | FLAG_TRIM,
                       fmt=FMT_F32, want_frames: bool = False, out=None):
        """First half of extract_batch: queues the batch on the context's stream and returns.  extract_collect() waits
        for it and returns the result dict.  Two plans of one context used alternately keep the device busy while
        the host takes one batch's results and submits the next."""
        args, out, keep = self._extract_args(samples, offsets, lengths, flags, fmt, want_frames, out)
        _check(lib().afx_extract_submit(*args), "afx_extract_submit")
        self._pending = (out, keep, want_frames)

    def extract_collect(self):
        if self._pending is None:
            raise AfxError("extract_collect: nothing submitted")
        out, keep, want_frames = self._pending
        self._pending = None
        _check(lib().afx_extract_collect(self.handle), "afx_extract_collect")
        return self._frames_out(out, keep, want_frames)

    def f0_batch(self, samples, offsets, lengths, fmin: float, fmax: float,
                 flags=FLAG_PREEMPH | FLAG_TRIM, fmt=FMT_F32, want_frames: bool = False):
        """extract_f0 (pYIN) of a ragged batch.  Returns stats [n, 4] float64 (f0_mean, f0_std,
        f0_missing_rate, f0_quality), status [n] and, when asked, f0: list of per-frame arrays (NaN = unvoiced)."""
        offsets, lengths, n = _clip_arrays(offsets, lengths)
        sptr, kind = _sample_source(samples, fmt, offsets, lengths)
        out = {"stats": np.zeros((n, 4), np.float64), "status": np.zeros(n, np.int32)}
        f0 = foffs = None
        if want_frames:
            tmax = 1 + lengths // self.params.hop
            foffs = packed_offsets(tmax)
            f0 = np.full(int(tmax.sum()), np.nan, np.float64)
        rc = lib().afx_f0_batch(
            self.handle, sptr, int(fmt), kind, offsets.ctypes.data, lengths.ctypes.data, n, int(flags),
            C.c_double(fmin), C.c_double(fmax), out["stats"].ctypes.data, out["status"].ctypes.data, _ptr(f0), _ptr(foffs))
        _check(rc, "afx_f0_batch")
        if want_frames:
            out["f0_flat"], out["f0_offsets"] = f0, foffs
        return out

    def zcr_batch(self, samples, offsets, lengths, flags=FLAG_PREEMPH | FLAG_TRIM, fmt=FMT_F32):
        """Zero-crossing rate per frame (float64) of a ragged host batch: list of arrays, plus status."""
        offsets, lengths, n = _clip_arrays(offsets, lengths)
        sptr, kind = _sample_source(samples, fmt, offsets, lengths, mem=MEM_HOST)
        tmax = 1 + lengths // self.params.hop
        zoffs = packed_offsets(tmax)
        z = np.zeros(int(tmax.sum()), np.float64)
        status = np.zeros(n, np.int32)
        _check(lib().afx_zcr_batch(self.handle, sptr, int(fmt), kind, offsets.ctypes.data,
                                   lengths.ctypes.data, n, int(flags), z.ctypes.data, zoffs.ctypes.data,
                                   status.ctypes.data), "afx_zcr_batch")
        return {"zcr_flat": z, "zcr_offsets": zoffs, "status": status}

    def spectral_batch(self, samples, offsets, lengths, flags=0, fmt=FMT_F32):
        """Frame-level spectral descriptors of a ragged host batch (plan: frame_length 2048, hop_length 512).  Returns per
        clip a dict: centroid / bandwidth / rolloff (T,) float32, valley / peak (7, T) float32 (spectral_contrast's band
        extremes before the dB difference)."""
        offsets, lengths, n = _clip_arrays(offsets, lengths)
        sptr, kind = _sample_source(samples, fmt, offsets, lengths, mem=MEM_HOST)
        T = 1 + lengths // self.params.hop
        doffs = packed_offsets(17 * T)
        d = np.zeros(int(17 * T.sum()), np.float32)
        status = np.zeros(n, np.int32)
        _check(lib().afx_spectral_batch(self.handle, sptr, int(fmt), kind, offsets.ctypes.data,
                                        lengths.ctypes.data, n, int(flags), d.ctypes.data, doffs.ctypes.data,
                                        status.ctypes.data), "afx_spectral_batch")
        out = []
        for i in range(n):
            m = d[doffs[i]: doffs[i] + 17 * T[i]].reshape(int(T[i]), 17)
            out.append({"centroid": m[:, 0].copy(), "bandwidth": m[:, 1].copy(), "rolloff": m[:, 2].copy(),
                        "valley": m[:, 3:10].T.copy(), "peak": m[:, 10:17].T.copy()})
        return {"clips": out, "status": status}

    def hpss_batch(self, samples, offsets, lengths, flags=0, fmt=FMT_F32, mem=MEM_HOST, want_harm: bool = True,
                   want_perc: bool = False, want_stats: bool = True, store_spec: bool = False) -> dict:
        """afx_hpss_batch: librosa.effects.hpss of a ragged batch (plan: frame_length 2048, hop_length 512, Hann).
        ``samples``: a C-contiguous host array, or with ``mem=MEM_DEVICE`` a device address (int) of ``fmt`` samples.
        Returns status [n] int32 and, as asked, ``harm`` / ``perc`` (lists of float32 arrays), ``stats`` [n, 4] float64
        (sum h^2, sum y^2, mean and std of h's spectral centroid) and ``spec`` (per clip S, Hm, Pm as [3, 1025, T])."""
        offsets, lengths, n = _clip_arrays(offsets, lengths)
        sptr, kind = _sample_source(samples, fmt, offsets, lengths, mem=mem)
        total = int((offsets + lengths).max()) if n else 0
        harm = np.zeros(total, np.float32) if want_harm else None
        perc = np.zeros(total, np.float32) if want_perc else None
        stats = np.zeros((n, 4), np.float64) if want_stats else None
        status = np.zeros(n, np.int32)
        spec = soff = None
        T = 1 + lengths // self.params.hop
        if store_spec:
            flags |= HPSS_STORE_SPEC
            cnt = 3 * HPSS_BINS * T
            soff = packed_offsets(cnt)
            spec = np.zeros(int(cnt.sum()), np.float32)
        _check(lib().afx_hpss_batch(self.handle, sptr, int(fmt), kind, offsets.ctypes.data, lengths.ctypes.data, n,
                                    int(flags), _ptr(harm), _ptr(perc), _ptr(stats), _ptr(spec), _ptr(soff),
                                    status.ctypes.data), "afx_hpss_batch")
        out = {"status": status}
        if want_harm:
            out["harm"] = [harm[o:o + l] for o, l in zip(offsets, lengths)]
        if want_perc:
            out["perc"] = [perc[o:o + l] for o, l in zip(offsets, lengths)]
        if want_stats:
            out["stats"] = stats
        if store_spec:
            out["spec"] = [spec[soff[i]:soff[i] + 3 * HPSS_BINS * T[i]].reshape(3, HPSS_BINS, int(T[i])) for i in range(n)]
        return out

    def denoise_batch(self, samples, offsets, lengths, *, mode: int = DENOISE_SPECSUB, beta: float = 0.01, noise_frames: int = 10,
                      rms_gain: bool = False, vad: bool = False, fmt=FMT_F32, mem=MEM_HOST, flags: int = 0) -> dict:
        """afx_denoise_batch: spectral subtraction (``DENOISE_SPECSUB``) or the Wiener filter (``DENOISE_WIENER``) of a ragged
        batch on the 2048 / 512 Hann STFT; ``rms_gain`` and ``vad`` add the aligner's gain to RMS 0.1 in front and its
        energy VAD behind.  ``samples`` as for ``hpss_batch``.  Returns ``out`` (a list of float32 arrays of the clips'
        lengths, zero from 512 (len // 512) on), ``info`` [n, 4] float64 (gain, VAD threshold, speech frames, VAD frames)
        and ``status`` [n] int32."""
        _need_denoise()
        flags = int(flags) | (DENOISE_RMS_GAIN if rms_gain else 0) | (DENOISE_VAD if vad else 0)
        denoise_check(self.params, flags, mode, beta, noise_frames)
        offsets, lengths, n = _clip_arrays(offsets, lengths)
        sptr, kind = _sample_source(samples, fmt, offsets, lengths, mem=mem)
        total = int((offsets + lengths).max()) if n else 0
        out = np.zeros(total, np.float32)
        info = np.zeros((n, 4), np.float64)
        status = np.zeros(n, np.int32)
        _check(lib().afx_denoise_batch(self.handle, sptr, int(fmt), kind, offsets.ctypes.data, lengths.ctypes.data, n, flags,
                                       int(mode), float(beta), int(noise_frames), out.ctypes.data, info.ctypes.data,
                                       status.ctypes.data), "afx_denoise_batch")
        return {"out": [out[o:o + l] for o, l in zip(offsets, lengths)], "info": info, "status": status}

    def chroma_batch(self, samples, offsets, lengths, flags=0, fmt=FMT_F32, mem=MEM_HOST, tuning=None,
                     want_chroma: bool = True, want_mel: bool = False, want_stats: bool = True, store_hist: bool = False) -> dict:
        """afx_chroma_batch: librosa.feature.chroma_stft / melspectrogram of a ragged batch (plan: frame_length 2048,
        hop_length 512, Hann).  ``tuning``: None (estimated per clip on the device), a scalar, or one value per clip.
        Returns status [n] int32, ``tuning`` [n] float64 (the tuning used) and, as asked, ``chroma`` (list of [12, T]
        float32), ``mel`` (list of [n_mels, T] float32 power), ``stats`` [n, 4] float64 (mel mean, std, chroma mean, std)
        and ``hist`` [n, 102] int32 (peaks, kept, the 100 residual counts)."""
        if not hasattr(lib(), "afx_chroma_batch"):
            raise NotImplementedError("this libafx has no afx_chroma_batch")
        offsets, lengths, n = _clip_arrays(offsets, lengths)
        sptr, kind = _sample_source(samples, fmt, offsets, lengths, mem=mem)
        T = 1 + lengths // self.params.hop
        M = int(self.params.n_mels)
        tin = None
        if tuning is not None:
            tin = np.ascontiguousarray(np.broadcast_to(np.asarray(tuning, np.float64), (n,)))
        coff, moff = packed_offsets(12 * T), packed_offsets(M * T)
        chroma = np.zeros(int(12 * T.sum()), np.float32) if want_chroma else None
        mel = np.zeros(int(M * T.sum()), np.float32) if want_mel else None
        stats = np.zeros((n, 4), np.float64) if want_stats else None
        hist = np.zeros((n, CHROMA_HIST), np.int32) if store_hist else None
        tout, status = np.zeros(n, np.float64), np.zeros(n, np.int32)
        if store_hist:
            flags |= CHROMA_STORE_HIST
        _check(lib().afx_chroma_batch(self.handle, sptr, int(fmt), kind, offsets.ctypes.data, lengths.ctypes.data, n,
                                      int(flags), _ptr(tin), _ptr(chroma), coff.ctypes.data, _ptr(mel), moff.ctypes.data,
                                      tout.ctypes.data, _ptr(stats), _ptr(hist), status.ctypes.data), "afx_chroma_batch")
        out = {"status": status, "tuning": tout}
        if want_chroma:
            out["chroma"] = [chroma[coff[i]:coff[i] + 12 * T[i]].reshape(12, int(T[i])) for i in range(n)]
        if want_mel:
            out["mel"] = [mel[moff[i]:moff[i] + M * T[i]].reshape(M, int(T[i])) for i in range(n)]
        if want_stats:
            out["stats"] = stats
        if store_hist:
            out["hist"] = hist
        return out

    def rhythm_batch(self, samples, offsets, lengths, flags=0, fmt=FMT_F32, mem=MEM_HOST, want_env: bool = True,
                     want_tempogram: bool = False, want_acmean: bool = False, want_stats: bool = True) -> dict:
        """afx_rhythm_batch: librosa.onset.onset_strength, the tempogram and tempo of librosa.beat.beat_track of a ragged
        batch (plan: frame_length 2048, hop_length 512, Hann; sr <= 49215).  Returns status [n] int32, ``tempo`` [n] float64
        (0.0 for an all-zero envelope, NaN for a failed clip), ``lag`` [n] int32 and, as asked, ``env`` (list of (T,) float32),
        ``tempogram`` (list of [win, T] float32), ``acmean`` [n, win] float64 and ``stats`` [n, 2] float64 (mean, std of env)."""
        if not hasattr(lib(), "afx_rhythm_batch"):
            raise NotImplementedError("this libafx has no afx_rhythm_batch")
        offsets, lengths, n = _clip_arrays(offsets, lengths)
        sptr, kind = _sample_source(samples, fmt, offsets, lengths, mem=mem)
        T = 1 + lengths // self.params.hop
        win = (8 * int(self.params.sr)) // 512
        eoff, toff = packed_offsets(T), packed_offsets(win * T)
        env = np.zeros(int(T.sum()), np.float32) if want_env else None
        tg = np.zeros(int(win * T.sum()), np.float32) if want_tempogram else None
        acmean = np.zeros((n, win), np.float64) if want_acmean else None
        stats = np.zeros((n, 2), np.float64) if want_stats else None
        tempo, lag, status = np.zeros(n, np.float64), np.zeros(n, np.int32), np.zeros(n, np.int32)
        _check(lib().afx_rhythm_batch(self.handle, sptr, int(fmt), kind, offsets.ctypes.data, lengths.ctypes.data, n,
                                      int(flags), _ptr(env), eoff.ctypes.data, _ptr(tg), toff.ctypes.data, _ptr(acmean),
                                      tempo.ctypes.data, lag.ctypes.data, _ptr(stats), status.ctypes.data), "afx_rhythm_batch")
        out = {"status": status, "tempo": tempo, "lag": lag}
        if want_env:
            out["env"] = [env[eoff[i]:eoff[i] + T[i]] for i in range(n)]
        if want_tempogram:
            out["tempogram"] = [tg[toff[i]:toff[i] + win * T[i]].reshape(win, int(T[i])) for i in range(n)]
        if want_acmean:
            out["acmean"] = acmean
        if want_stats:
            out["stats"] = stats
        return out

    def beat_batch(self, samples, offsets, lengths, flags=0, fmt=FMT_F32, mem=MEM_HOST, envelopes: bool = False, bpm=None,
                   tightness: float = 100.0, trim: bool = True, want_env: bool = False, want_scores: bool = False) -> dict:
        """afx_beat_batch: the beat positions of librosa.beat.beat_track of a ragged batch (plan: frame_length 2048,
        hop_length 512, Hann; sr <= 49215).  ``envelopes``: the clips are float32 onset envelopes (lengths in frames), not
        samples.  ``bpm``: None, or one tempo per clip (0: the tempo afx_rhythm_batch decides).  Returns status [n] int32,
        ``tempo`` [n] float64 (NaN for a failed clip), ``fpb`` and ``n_beats`` [n] int32, ``beats`` (list of int64 frame
        indices), ``mask`` (list of (T,) uint8) and, as asked, ``env`` (list of (T,) float32) and ``localscore``,
        ``cumscore`` (float64), ``backlink`` (int32) as lists of (T,) arrays."""
        if not hasattr(lib(), "afx_beat_batch"):
            raise NotImplementedError("this libafx has no afx_beat_batch")
        offsets, lengths, n = _clip_arrays(offsets, lengths)
        sptr, kind = _sample_source(samples, fmt, offsets, lengths, mem=mem)
        T = lengths.copy() if envelopes else 1 + lengths // self.params.hop
        foff = packed_offsets(T)
        total = int(T.sum())
        if bpm is not None:
            bpm = np.ascontiguousarray(bpm, np.float64).reshape(-1)
            if bpm.shape[0] != n:
                raise ValueError("bpm must have one entry per clip")
        mask = np.zeros(total, np.uint8)
        env = np.zeros(total, np.float32) if want_env else None
        ls = np.zeros(total, np.float64) if want_scores else None
        cum = np.zeros(total, np.float64) if want_scores else None
        bl = np.zeros(total, np.int32) if want_scores else None
        tempo, fpb, nb, status = np.zeros(n, np.float64), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        _check(lib().afx_beat_batch(self.handle, sptr, int(fmt), kind, offsets.ctypes.data, lengths.ctypes.data, n,
                                    int(flags) | (BEAT_INPUT_ENVELOPE if envelopes else 0), _ptr(bpm), float(tightness),
                                    int(bool(trim)), mask.ctypes.data, foff.ctypes.data, nb.ctypes.data, tempo.ctypes.data,
                                    fpb.ctypes.data, _ptr(env), _ptr(ls), _ptr(cum), _ptr(bl), status.ctypes.data), "afx_beat_batch")
        cut = lambda a: [a[foff[i]:foff[i] + T[i]] for i in range(n)]
        out = {"status": status, "tempo": tempo, "fpb": fpb, "n_beats": nb, "mask": cut(mask)}
        out["beats"] = [np.flatnonzero(m).astype(np.int64) for m in out["mask"]]
        if want_env:
            out["env"] = cut(env)
        if want_scores:
            out["localscore"], out["cumscore"], out["backlink"] = cut(ls), cut(cum), cut(bl)
        return out

    def groups_batch(self, samples, offsets, lengths, groups: int = GROUP_ALL, flags: int = 0, fmt=FMT_F32, mem=MEM_HOST,
                     preprocess: bool = False, store_desc: bool = False) -> dict:
        """afx_groups_batch: the spectral, harmonic, timbre and rhythm groups of a ragged batch on one STFT (plan:
        frame_length 2048, hop_length 512, Hann).  ``groups``: GROUP_* bits; ``preprocess``: the experiment extractor's
        preprocess_audio on the device first.  Returns ``stats`` [n, 24] float64 (include/afx.h lists the fields; NaN for a
        group not asked for and for a failed clip), ``tuning`` [n] float64, ``lag`` [n] int32, ``status`` [n] int32 and,
        with ``store_desc`` (and GROUP_SPECTRAL), ``desc``: per clip the [T, 17] float32 rows of afx_spectral_batch's
        layout (None for a clip of status CLIP_TOO_SHORT)."""
        _need_groups()
        offsets, lengths, n = _clip_arrays(offsets, lengths)
        sptr, kind = _sample_source(samples, fmt, offsets, lengths, mem=mem)
        if preprocess:
            flags |= GROUPS_PREPROCESS
        if store_desc:
            flags |= GROUPS_STORE_DESC
        stats = np.zeros((n, GROUPS_STATS), np.float64)
        tuning, lag, status = np.zeros(n, np.float64), np.zeros(n, np.int32), np.zeros(n, np.int32)
        _check(lib().afx_groups_batch(self.handle, sptr, int(fmt), kind, offsets.ctypes.data, lengths.ctypes.data, n,
                                      int(flags), int(groups), stats.ctypes.data, tuning.ctypes.data, lag.ctypes.data,
                                      status.ctypes.data), "afx_groups_batch")
        out = {"stats": stats, "tuning": tuning, "lag": lag, "status": status}
        if store_desc and groups & GROUP_SPECTRAL:
            T = np.where(status == CLIP_TOO_SHORT, 0, 1 + lengths // self.params.hop)
            rows = np.zeros(int(17 * T.sum()), np.float32)
            count = C.c_int64()
            _check(lib().afx_groups_debug_rows(self.handle, _ptr(rows) if rows.size else None, int(rows.size), C.byref(count)),
                   "afx_groups_debug_rows")
            if int(count.value) != rows.size:
                raise AfxError(f"afx_groups_debug_rows: {count.value} floats kept, {rows.size} expected")
            roff = packed_offsets(17 * T)
            out["desc"] = [rows[roff[i]:roff[i] + 17 * T[i]].reshape(int(T[i]), 17) if T[i] else None for i in range(n)]
        return out

    def preprocess(self, y: np.ndarray):
        y = np.ascontiguousarray(y, np.float32)
        out = np.empty_like(y)
        s, e, st = C.c_int64(), C.c_int64(), C.c_int32()
        _check(lib().afx_preprocess(self.handle, y.ctypes.data, y.size, out.ctypes.data,
                                    C.byref(s), C.byref(e), C.byref(st)), "afx_preprocess")
        return out, int(s.value), int(e.value), int(st.value)
