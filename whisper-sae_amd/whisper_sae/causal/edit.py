"""``FeatureEdit``: what an intervention does to the activations of individual SAE features.

An edit is a per-feature factor (``scale``; ``ablate`` is the factor 0) plus at most ``MAX_FORCED`` *forced* features
whose activation is set to a constant on every selected row, whether or not the row's code holds them (``clamp``).
Edits combine with ``|``.  A feature may carry one factor and one clamp value; where both are present the clamp
wins, as in the kernel (``wsae_intervene``: a forced feature that is in the code takes its constant instead of
``scale * act``).  The device tables the kernel reads are built once per ``(hidden_dim, device)``.
"""

from __future__ import annotations

from typing import Iterable, Union

import torch

from .. import _native as N

MAX_FORCED = N.IV_MAX_FORCE


def _feature_list(features: Union[int, Iterable[int]]) -> list:
    items = [features] if isinstance(features, int) else list(features)
    out = []
    for f in items:
        if isinstance(f, bool) or int(f) != f:
            raise ValueError(f"feature ids are integers, got {f!r}")
        f = int(f)
        if f < 0:
            raise ValueError(f"feature id {f} is negative")
        if f in out:
            raise ValueError(f"feature {f} is listed twice")
        out.append(f)
    return out


class FeatureEdit:
    """``FeatureEdit.ablate([3, 7]) | FeatureEdit.clamp(12, 4.0)``; ``FeatureEdit()`` is the identity."""

    def __init__(self, scales: dict | None = None, forced: dict | None = None):
        self.scales: dict = dict(scales or {})  # feature -> factor
        self.forced: dict = dict(forced or {})  # feature -> constant activation (insertion order = the kernel's sum order)
        if len(self.forced) > MAX_FORCED:
            raise ValueError(f"{len(self.forced)} forced features: the kernel takes at most {MAX_FORCED}")
        self._tables: dict = {}

    @classmethod
    def identity(cls) -> "FeatureEdit":
        return cls()

    @classmethod
    def scale(cls, features, factor: float) -> "FeatureEdit":
        return cls(scales={f: float(factor) for f in _feature_list(features)})

    @classmethod
    def ablate(cls, features) -> "FeatureEdit":
        return cls.scale(features, 0.0)

    @classmethod
    def clamp(cls, features, value: float) -> "FeatureEdit":
        return cls(forced={f: float(value) for f in _feature_list(features)})

    def __or__(self, other: "FeatureEdit") -> "FeatureEdit":
        if not isinstance(other, FeatureEdit):
            return NotImplemented
        for mine, theirs, what in ((self.scales, other.scales, "scaled"), (self.forced, other.forced, "clamped")):
            both = sorted(set(mine) & set(theirs))
            if both:
                raise ValueError(f"features {both} are {what} by both operands")
        return FeatureEdit({**self.scales, **other.scales}, {**self.forced, **other.forced})

    @property
    def is_identity(self) -> bool:
        return not self.forced and all(v == 1.0 for v in self.scales.values())

    def features(self) -> list:
        return sorted(set(self.scales) | set(self.forced))

    def tables(self, hidden_dim: int, device) -> tuple:
        """``(scale f32[H], force_idx i32[n], force_val f32[n], n)`` on ``device``, cached."""
        device = torch.device(device)
        key = (int(hidden_dim), str(device))
        have = self._tables.get(key)
        if have is not None:
            return have
        bad = [f for f in self.features() if f >= hidden_dim]
        if bad:
            raise ValueError(f"features {bad} are outside the dictionary of {hidden_dim} features")
        scale = torch.ones(hidden_dim, dtype=torch.float32)
        for f, factor in self.scales.items():
            scale[f] = factor
        n = len(self.forced)
        # (one spare slot keeps the tables non-empty, so their pointers are always valid)
        force_idx = torch.zeros(max(n, 1), dtype=torch.int32)
        force_val = torch.zeros(max(n, 1), dtype=torch.float32)
        for slot, (f, value) in enumerate(self.forced.items()):
            force_idx[slot] = f
            force_val[slot] = value
        have = (scale.to(device), force_idx.to(device), force_val.to(device), n)
        self._tables[key] = have
        return have

    def __repr__(self) -> str:
        return f"FeatureEdit(scales={self.scales!r}, forced={self.forced!r})"
