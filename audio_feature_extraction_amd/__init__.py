"""audio_feature_extraction_amd -- MI355X-native drop-in for
``audio_feature_extraction_toolkit`` (reference __init__.py:1-6): same two exports."""
from .core.feature_extractor import AudioFeatureExtractor
from .evaluation.evaluator import FeatureEvaluator
from . import quality  # noqa: F401  (the recording screen and the denoising scores; a module, not one of the two exports)
from . import loudness  # noqa: F401  (BS.1770 loudness and normalisation; a module, likewise)
# librosa's transform and its helpers under librosa's names (core/spectrum.py); beside the two exports, not among them
from .core.spectrum import stft, istft, magphase, amplitude_to_db, power_to_db, phase_vocoder  # noqa: F401

__version__ = '0.1.0'

__all__ = ['AudioFeatureExtractor', 'FeatureEvaluator']
