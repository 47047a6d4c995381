"""Feature analysis right after the SAE path: per-feature top activations kept on the
device, the comparison of two dictionaries by their decoder (or encoder) directions, and co-activation statistics of
their codes.  Mirrors the names of the reference's ``whisper_sae.analysis.feature_viz`` that sit on that path."""

from .coactivation import (CoactivationNeighbors, CoactivationTracker, collect_coactivation,
                           compare_activations)
from .dictionary import NearestFeatures, compare_dictionaries, duplicate_features, nearest_features
from .feature_viz import FeatureActivation, TopKTracker, collect_top_activations

__all__ = ["FeatureActivation", "TopKTracker", "collect_top_activations", "NearestFeatures", "nearest_features",
           "compare_dictionaries", "duplicate_features", "CoactivationNeighbors", "CoactivationTracker",
           "collect_coactivation", "compare_activations"]
