"""Activation feed: on-device ring buffer + the reference's on-disk cache format + the extraction driver + the log-mel front end."""

from .audio import (LogMel, dft_basis, frame_of_sample, log_mel_spectrogram, mel_filter_bank,
                    sample_span_of_frames)
from .feature_cache import ActivationRing, CacheMetadata, FeatureCache, RingLoader, extract_and_cache_features

__all__ = ["ActivationRing", "CacheMetadata", "FeatureCache", "LogMel", "RingLoader", "dft_basis", "extract_and_cache_features",
           "frame_of_sample", "log_mel_spectrogram", "mel_filter_bank", "sample_span_of_frames"]
