"""Feature analysis right after the SAE path: per-feature top activations kept on the
device, and the comparison of two dictionaries by their decoder (or encoder) directions.  Mirrors the names of the
reference's ``whisper_sae.analysis.feature_viz`` that sit on that path."""

from .dictionary import NearestFeatures, compare_dictionaries, duplicate_features, nearest_features
from .feature_viz import FeatureActivation, TopKTracker, collect_top_activations

__all__ = ["FeatureActivation", "TopKTracker", "collect_top_activations", "NearestFeatures", "nearest_features",
           "compare_dictionaries", "duplicate_features"]
