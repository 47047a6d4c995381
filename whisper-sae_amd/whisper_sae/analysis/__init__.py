"""Feature analysis right after the SAE path: per-feature top activations kept on the
device, the comparison of two dictionaries by their decoder (or encoder) directions, co-activation statistics of
their codes, effect sizes of the features between two groups of utterances, the temporal run statistics of the
features (run lengths, gaps, event lists), feature-triggered averages of a per-frame signal, activation profiles
(per-feature value histograms and uniform samples per value stratum), and label association (feature-by-class counts per
value stratum and lag against a per-frame label: precision, recall, F1, phi, mutual information and AUROC at the best
threshold and lag), and sparse linear probes (softmax regression of a label on the compact code over all or a subset of
the features, and the k-sparse probing curve), and sparse ridge regression (the Gram matrix of the code and the target
moments in one streaming pass, then ridge fits of any feature subset as host-side solves), and code dynamics (the
similarity of a frame's whole code to the code a few frames later, its statistics within and across labels, and the score
of the curve's peaks against reference boundaries at every threshold), and code clustering (k-means of the frames by
their whole code, the units' purity, PNMI and adjusted Rand index against a label, and the unit strings), and ABX phone discrimination (DTW distances between segments of the code and the count of the
triples in which a token lies closer to a token of its own phone than to one of another), and token association (exact
counts of every (feature, token) pair that occurs, for vocabularies of 10^4 to 10^7 tokens, in a device hash table, with the
top tokens of a feature and the top features of a token ranked on the device), and token alignment (a token label for
every encoder frame from Whisper's cross-attention: the fused z-score / median / head-mean cost and dynamic time warping), and
audio clip export (the clips a feature fires on, cut, peak-normalised, faded and converted to 16-bit PCM for all features in
one launch over a device-resident waveform bank, written as WAV files with a manifest, and per-feature reports).  Mirrors the names of the reference's ``whisper_sae.analysis.feature_viz``
that sit on that path."""

from .alignment import (CrossAttentionTap, FrameAlignment, RawAlignment, align_tokens, align_weights, aligned_batches,
                        alignment_heads)
from .audio_extraction import (AudioClipConfig, AudioClipExtractor, ClipBatch, WaveformBank, clip_table_for_activations,
                               clip_table_for_events, create_indexed_audio_loader, cut_clips, read_wav, write_wav)
from .clustering import (ClusterScores, CodeKMeans, IterationStats, cluster_scores, collect_code_clusters,
                         unit_sequences)
from .coactivation import (CoactivationNeighbors, CoactivationTracker, collect_coactivation,
                           compare_activations)
from .dictionary import NearestFeatures, compare_dictionaries, duplicate_features, nearest_features
from .discrimination import AbxItems, AbxScores, collect_abx, items_from_labels, segment_distances
from .dynamics import (BoundaryCurve, BoundaryScorer, CodeDynamics, DynamicsSummary, LagStats, boundaries_from_labels,
                       boundary_curve, collect_code_dynamics, detect_boundaries, frame_similarity, novelty)
from .feature_viz import FeatureActivation, FeatureInterpretation, FeatureReport, TopKTracker, collect_top_activations
from .group_stats import (GroupEffects, SegmentPooler, bootstrap_weights, collect_pooled, group_effect_sizes,
                          top_group_features)
from .labels import (BestLabels, LabelAssociation, LabelScores, automated_labels, best_labels, collect_label_association,
                     top_label_features)
from .probe import (ProbeCurve, ProbeData, ProbeFit, ProbeReport, SparseProbe, collect_probe_data, sparse_probe_curve,
                    utterance_split)
from .profile import (ActivationProfile, ActivationSampler, DensityHistogram, ProfileSummary, SampledActivations,
                      collect_activation_profile, collect_activation_samples, top_profile_features)
from .regression import (RegressionCurve, RegressionFit, RegressionReport, SparseRegression, collect_regression,
                         regression_curve, ridge_from_statistics, top_correlated_features)
from .temporal import FeatureEvents, RunSummary, RunTracker, collect_runs, summarize_runs, top_temporal_features
from .tokens import PairExport, TokenAssociation, TopPairs, collect_token_association
from .triggered import (TriggeredAverageTracker, as_spectrogram, collect_triggered_averages, mel_frames,
                        top_template_features)

__all__ = ["FeatureActivation", "TopKTracker", "collect_top_activations", "NearestFeatures", "nearest_features",
           "compare_dictionaries", "duplicate_features", "CoactivationNeighbors", "CoactivationTracker",
           "collect_coactivation", "compare_activations", "GroupEffects", "SegmentPooler", "bootstrap_weights",
           "collect_pooled", "group_effect_sizes", "top_group_features", "FeatureEvents", "RunSummary", "RunTracker",
           "collect_runs", "summarize_runs", "top_temporal_features", "TriggeredAverageTracker", "collect_triggered_averages",
           "mel_frames", "as_spectrogram", "top_template_features", "ActivationProfile", "ActivationSampler", "DensityHistogram",
           "ProfileSummary", "SampledActivations", "collect_activation_profile", "collect_activation_samples",
           "top_profile_features", "BestLabels", "LabelAssociation", "LabelScores", "automated_labels", "best_labels",
           "collect_label_association", "top_label_features", "ProbeCurve", "ProbeData", "ProbeFit", "ProbeReport", "SparseProbe",
           "collect_probe_data", "sparse_probe_curve", "utterance_split", "RegressionCurve", "RegressionFit", "RegressionReport",
           "SparseRegression", "collect_regression", "regression_curve", "ridge_from_statistics", "top_correlated_features",
           "BoundaryCurve", "BoundaryScorer", "CodeDynamics", "DynamicsSummary", "LagStats", "boundaries_from_labels",
           "boundary_curve", "collect_code_dynamics", "detect_boundaries", "frame_similarity", "novelty", "ClusterScores", "CodeKMeans",
           "IterationStats", "cluster_scores", "collect_code_clusters", "unit_sequences", "AbxItems", "AbxScores", "collect_abx",
           "items_from_labels", "segment_distances", "PairExport", "TokenAssociation", "TopPairs", "collect_token_association",
           "CrossAttentionTap", "FrameAlignment", "RawAlignment", "align_tokens", "align_weights", "aligned_batches",
           "alignment_heads", "AudioClipConfig", "AudioClipExtractor", "ClipBatch", "WaveformBank", "clip_table_for_activations",
           "clip_table_for_events", "create_indexed_audio_loader", "cut_clips", "read_wav", "write_wav", "FeatureInterpretation",
           "FeatureReport"]
