#!/usr/bin/env python
"""Generate tests/golden/g20_audio_clips.npz and g20_manifest.json by running the REAL reference's audio clip extractor
and reports on the CPU.  Run where the reference is installed (it does not travel with the tests):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference>/src python tests/golden/make_golden_clips.py

Inputs are the seeded waveforms of ``tests/clip_oracle.golden_waveform`` (the counter generator of ``oracle/synth.py``);
only the reference's OUTPUTS are stored - data (npz / json), no reference source text.

  g20_audio_clips.npz   ``AudioClipExtractor.extract_clip`` (clip_duration_ms = 50, context_before_ms = 25: 800-sample
                        clips, 400 before the position) for every case below, with ``normalize_audio`` on and off:
                        ``n{0|1}_{case}`` = the returned float32 clip.  ``cases`` lists (name, utterance, position).
                        With ``normalize_audio`` on, the reference raises on an EMPTY clip (``max()`` of no elements):
                        those keys are absent and named in ``raises``.
  g20_manifest.json     a reference ``TopKTracker`` (6 features, k = 3) over the three utterances, its saved state, the
                        manifest that ``extract_all_clips`` + ``save_manifest`` write, and ``FeatureReport``'s per-feature
                        and summary dicts with one interpretation added.  The reference's ``_save_audio`` needs
                        ``soundfile``: it is replaced by a stub that writes nothing.  Paths are made relative to the
                        output directory.
"""

from __future__ import annotations

import json
import sys
import tempfile
from pathlib import Path

sys.dont_write_bytecode = True  # the reference tree is read-only input: importing it must not leave __pycache__ there

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[1]))
sys.path.insert(0, str(HERE.parent))

import clip_oracle as CO  # noqa: E402
from oracle import synth  # noqa: E402

from whisper_sae.analysis.audio_extraction import AudioClipConfig, AudioClipExtractor  # noqa: E402  (reference)
from whisper_sae.analysis.feature_viz import FeatureActivation, FeatureReport, TopKTracker  # noqa: E402  (reference)

# (name, utterance, position): 160 samples per position, the clip starts 400 samples before it
CASES = (("frame0", 0, 0),        # start -400 -> 0, keeps its 800 samples
         ("middle", 0, 10),       # 1200 .. 2000
         ("cut_by_end", 0, 23),   # 3280 .. 4000 of 4000
         ("beyond_end", 0, 40),   # 6000 >= 4000: empty
         ("all_zero", 1, 10),     # 1200 .. 2000 inside the silence of utterance 1: no gain
         ("row_audio", 2, 5))     # utterance 2 is handed over as [1, n]


def loader(sample_idx: int) -> torch.Tensor:
    wave = torch.from_numpy(CO.golden_waveform(sample_idx))
    return wave.unsqueeze(0) if sample_idx == 2 else wave


def clips():
    out = {"cases": np.array([[name, str(u), str(p)] for name, u, p in CASES])}
    raises = []
    for norm in (0, 1):
        cfg = AudioClipConfig(clip_duration_ms=50.0, context_before_ms=25.0, normalize_audio=bool(norm))
        with tempfile.TemporaryDirectory() as tmp:
            ex = AudioClipExtractor(TopKTracker(num_features=1, k=1), loader, tmp, cfg)
            for name, u, p in CASES:
                act = FeatureActivation(feature_idx=0, activation_value=1.0, sample_idx=u, position_idx=p)
                try:
                    clip = ex.extract_clip(act) if u != 1 else ex.extract_clip(act, loader(u))
                except RuntimeError:
                    raises.append(f"n{norm}_{name}")
                    continue
                assert clip.dtype == torch.float32 and clip.ndim == 1
                out[f"n{norm}_{name}"] = clip.numpy().copy()
    out["raises"] = np.array(raises)
    np.savez_compressed(HERE / "g20_audio_clips.npz", **out)
    print({k: v.shape for k, v in out.items()})


def manifest():
    H, KEEP, T = 6, 3, 15  # positions 0 .. 14: every clip has samples (the reference cannot normalise an empty one)
    tracker = TopKTracker(num_features=H, k=KEEP)
    n = 3 * T * H
    raw = synth.counter_u64(n, 20, 100)
    val = ((raw >> np.uint64(40)).astype(np.float64) + 1.0) / float(1 << 24) + np.arange(n) * 2.0 ** -30
    act = np.where((raw % np.uint64(4)) == 0, val, 0.0).astype(np.float32).reshape(3, T, H)
    act[:, :, 5] = 0  # a feature without examples
    assert len(np.unique(act[act > 0])) == int((act > 0).sum())
    tracker.update(torch.from_numpy(act), [0, 1, 2], transcriptions=["utt0", "utt1", "utt2"])
    cfg = AudioClipConfig(clip_duration_ms=50.0, context_before_ms=25.0)
    with tempfile.TemporaryDirectory() as tmp:
        state_path = Path(tmp) / "state.json"
        tracker.save(state_path)
        state = json.loads(state_path.read_text())
        ex = AudioClipExtractor(tracker, loader, Path(tmp) / "clips", cfg)
        ex._save_audio = lambda audio, path: None  # (soundfile is not installed; nothing about the files is stored)
        written = ex.extract_all_clips()
        doc = json.loads(ex.save_manifest().read_text())
        report = FeatureReport(tracker, Path(tmp) / "reports")
        report.add_interpretation(2, "phoneme", "fires on a synthetic burst", confidence=0.75, evidence=["rank 0", "rank 1"])
        reports = {str(f): report.generate_feature_report(f) for f in range(H)}
        summary = report.generate_summary_report(top_n=4)
        text = json.dumps({"tracker_state": state, "manifest": doc, "written": {str(f): [str(p) for p in ps] for f, ps in written.items()},
                           "feature_reports": reports, "summary": summary}, indent=1)
        text = text.replace(str(Path(tmp) / "clips") + "/", "")
    assert tmp not in text
    (HERE / "g20_manifest.json").write_text(text + "\n")
    print(f"g20_manifest.json: {len(text)} bytes, features {sorted(doc['features'])}")


if __name__ == "__main__":
    clips()
    manifest()
