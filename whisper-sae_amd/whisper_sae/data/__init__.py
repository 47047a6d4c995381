"""Activation feed: on-device ring buffer + the reference's on-disk cache format + the extraction driver + the audio front end
(resampling, log-mel)."""

from .audio import (LogMel, dft_basis, frame_of_sample, log_mel_spectrogram, mel_filter_bank,
                    sample_span_of_frames)
from .feature_cache import ActivationRing, CacheMetadata, FeatureCache, RingLoader, extract_and_cache_features
from .resample import AudioFrontEnd, Resampler, compact_taps, resample, resampled_length, sinc_resample_kernel

__all__ = ["ActivationRing", "AudioFrontEnd", "CacheMetadata", "FeatureCache", "LogMel", "Resampler", "RingLoader", "compact_taps",
           "dft_basis", "extract_and_cache_features", "frame_of_sample", "log_mel_spectrogram", "mel_filter_bank", "resample",
           "resampled_length", "sample_span_of_frames", "sinc_resample_kernel"]
