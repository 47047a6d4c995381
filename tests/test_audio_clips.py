"""Audio clip export without a GPU: the oracle of tests/clip_oracle.py against the reference's own
clips (G20), every argument error of ``wsae_clip_extract`` (found on the host before any HIP call), the workspace query,
header / ``SIGNATURES`` / constants / exports, the WAV round trip, the two clip-table builders against hand-computed bounds,
the manifest and the reports against the reference's JSON, and the errors of the Python layer."""

from __future__ import annotations

import json
import math
import re
import wave
from pathlib import Path

import numpy as np
import pytest
import torch

import clip_oracle as CO
from whisper_sae import _native as N
from whisper_sae.analysis import (AudioClipConfig, AudioClipExtractor, FeatureActivation, FeatureEvents, FeatureInterpretation,
                                  FeatureReport, TopKTracker, WaveformBank, clip_table_for_activations, clip_table_for_events,
                                  create_indexed_audio_loader, cut_clips, read_wav, write_wav)
from whisper_sae.analysis import audio_extraction as AE

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "wsae.h"
GOLDEN = ROOT / "tests" / "golden"
NAMES = ("wsae_clip_workspace_bytes", "wsae_clip_extract")
CFG = dict(clip_duration_ms=50.0, context_before_ms=25.0)  # the goldens' clips: 800 samples, 400 before the position


# ---- 1: the oracle is the reference's arithmetic -----------------------------------------------------------------------------
def test_oracle_equals_the_reference_clips_bit_for_bit():
    g = np.load(GOLDEN / "g20_audio_clips.npz")
    assert list(g["raises"]) == ["n1_beyond_end"]  # (the reference cannot normalise an empty clip; here it is empty)
    seen = set()
    for name, u, p in g["cases"]:
        u, p = int(u), int(p)
        x = CO.golden_waveform(u)
        s0, n = CO.bounds(p * 160 - 400, 800, len(x), len(x), 800)
        for norm in (0, 1):
            got, peak = CO.clip_values(x[s0:s0 + n], norm, 0.95, 0, False)
            key = f"n{norm}_{name}"
            if key in g.files:
                want = g[key]
                assert want.dtype == np.float32 and got.shape == want.shape, key
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), key
                if norm and n and peak > 0:
                    assert np.abs(got).max() == np.float32(0.95)
            else:
                assert n == 0 and got.size == 0
            seen.add((name, n))
    assert seen == {("frame0", 800), ("middle", 800), ("cut_by_end", 720), ("beyond_end", 0), ("all_zero", 800), ("row_audio", 800)}
    assert not g["n1_all_zero"].any() and not g["n0_all_zero"].any()


def test_oracle_rules_on_small_cases():
    assert CO.bounds(-5, 10, 100, 100, 10) == (0, 10) and CO.bounds(95, 10, 100, 100, 10) == (95, 5)
    assert CO.bounds(100, 10, 100, 100, 10) == (100, 0) and CO.bounds(3, 10, 100, 50, 4) == (3, 4)
    assert CO.bounds(3, -2, 100, 100, 10) == (3, 0) and CO.bounds(0, 10, -7, 100, 10) == (0, 0)
    assert np.array_equal(CO.fade_ramp(7, 3), np.array([1, 2, 3, 3, 3, 2, 1], np.float32) / np.float32(3))
    assert np.array_equal(CO.fade_ramp(4, 7), np.array([1, 2, 2, 1], np.float32) / np.float32(7))
    pcm = np.array([-32768, -1, 0, 1, 32767], np.int16)
    same, m = CO.clip_values(pcm, CO.GAIN_NONE, 0.5, 0, True)
    assert np.array_equal(same, pcm) and m == np.float32(1.0)
    full, _ = CO.clip_values(pcm, CO.GAIN_PEAK, 1.0, 0, True)  # target 1: the peak becomes -32767, nothing clips
    assert full[0] == -32767 and full[-1] == np.rint(np.float32(32767 / 32768) * np.float32(32767))
    half, _ = CO.clip_values(np.array([0.5 / 32767, 1.5 / 32767, 2.5 / 32767], np.float64).astype(np.float32), 0, 1.0, 0, True)
    assert half.dtype == np.int16


# ---- 2: the C ABI's argument checks -------------------------------------------------------------------------------------------
def test_argument_errors_do_not_need_a_gpu():
    lib = N.lib()
    A = 0x1000  # any non-null aligned address: an argument error returns before anything is read
    need = lib.wsae_clip_workspace_bytes(3, 5000)
    # 0 x, 1 x_dtype, 2 n_utt, 3 ld_x, 4 length, 5 max_length, 6 n_clips, 7 clip_utt, 8 clip_start, 9 clip_count, 10 max_count,
    # 11 clip_off, 12 gain_mode, 13 target, 14 fade, 15 out, 16 out_dtype, 17 out_elems, 18 out_len, 19 out_peak, 20 workspace,
    # 21 workspace_bytes, 22 stream
    good = [A, N.DT_F32, 2, 1000, A, 1000, 3, A, A, A, 5000, A, N.CLIP_GAIN_PEAK, 0.95, 0, A, N.DT_I16, 15000, A, None, A, need, None]
    cases = [(pos, None, "null") for pos in (0, 4, 7, 8, 9, 11, 15, 18)]
    cases += [(1, N.DT_BF16, "x_dtype"), (1, 7, "x_dtype"), (16, N.DT_F16, "out_dtype"), (16, -1, "out_dtype"), (3, 999, "ld_x"),
              (2, -1, "n_utt"), (6, -1, "n_clips"), (10, -1, "max_count"), (10, (1 << 30) + 1, "max_count"), (5, -1, "max_length"),
              (5, 1 << 31, "max_length"), (17, -1, "out_elems"), (12, 2, "gain_mode"), (13, math.inf, "target"),
              (13, math.nan, "target"), (14, -1, "fade"), (21, need - 1, "workspace"), (20, None, "workspace"), (0, A + 2, "aligned"),
              (15, A + 1, "aligned"), (8, A + 4, "aligned"), (19, A + 2, "aligned"), (20, A + 2, "aligned")]
    for pos, bad, word in cases:
        args = list(good)
        args[pos] = bad
        assert lib.wsae_clip_extract(*args) == -1, (pos, bad)
        assert "wsae_clip_extract" in N.last_error() and word in N.last_error(), (pos, bad, N.last_error())
    assert lib.wsae_clip_extract(*good[:6], 0, *good[7:]) == 0  # no clips: nothing is touched
    assert lib.wsae_clip_extract(*good[:6], 0, *good[7:20], None, 0, None) == 0  # ... and no workspace is needed


def test_workspace_size():
    lib = N.lib()
    q = lib.wsae_clip_workspace_bytes
    for bad in ((-1, 100), (1, -1), (1, (1 << 30) + 1)):
        assert q(*bad) == -1, bad
    T = N.CLIP_TILE
    assert T == 4096 and q(0, 16000) == 0
    assert q(64, 0) == q(64, 1) == q(64, T) == 256  # one float per clip at least
    assert q(64, T + 1) == 512 and q(61440, 16000) == 61440 * 4 * 4
    by_clips = [q(n, 16000) for n in (0, 1, 2, 63, 64, 65, 4096, 61440)]
    by_count = [q(1000, c) for c in (0, 1, T - 1, T, T + 1, 2 * T + 5, 16000, 1 << 20, 1 << 30)]
    for sizes in (by_clips, by_count):
        assert sizes == sorted(sizes) and all(s % 256 == 0 for s in sizes)


def test_header_signatures_constants_and_exports_agree():
    import whisper_sae.analysis as A
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    lib = N.lib()
    for name in NAMES:
        proto = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert proto, name
        assert len(proto.group(1).split(",")) == len(N.SIGNATURES[name][1]), name
        assert getattr(lib, name) is not None
    assert {n for n in N.SIGNATURES if n.startswith("wsae_clip_")} == set(NAMES)
    defines = {k: int(v) for k, v in re.findall(r"#define (WSAE_CLIP_[A-Z0-9_]+) (\d+)", text)}
    assert defines == {"WSAE_CLIP_TILE": N.CLIP_TILE, "WSAE_CLIP_GAIN_NONE": N.CLIP_GAIN_NONE, "WSAE_CLIP_GAIN_PEAK": N.CLIP_GAIN_PEAK}
    assert (CO.GAIN_NONE, CO.GAIN_PEAK) == (N.CLIP_GAIN_NONE, N.CLIP_GAIN_PEAK)
    for name in ("AudioClipConfig", "AudioClipExtractor", "ClipBatch", "WaveformBank", "cut_clips", "clip_table_for_activations",
                 "clip_table_for_events", "write_wav", "read_wav", "create_indexed_audio_loader", "FeatureInterpretation",
                 "FeatureReport"):
        assert name in A.__all__ and hasattr(A, name)


# ---- 3: files -------------------------------------------------------------------------------------------------------------------
def test_wav_round_trip_of_every_int16_value(tmp_path):
    every = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    write_wav(tmp_path / "all.wav", torch.from_numpy(every), 16000)
    with wave.open(str(tmp_path / "all.wav"), "rb") as fh:
        assert (fh.getnchannels(), fh.getsampwidth(), fh.getframerate(), fh.getnframes()) == (1, 2, 16000, 65536)
        assert np.array_equal(np.frombuffer(fh.readframes(65536), "<i2"), every)
    back, rate = read_wav(tmp_path / "all.wav", return_rate=True)
    assert back.dtype == torch.float32 and rate == 16000
    assert np.array_equal(back.numpy(), every.astype(np.float32) * np.float32(2.0 ** -15))
    assert np.array_equal((back.numpy() * 32768).astype(np.int16), every)
    # floats go through the cutter's rule: rint(x * 32767), half to even, clamped
    x = np.array([0.0, 0.5 / 32767, 1.5 / 32767, 2.5 / 32767, -1.0, 1.0, 1.5, -1.5, 0.95, 1e-9], np.float32)
    write_wav(tmp_path / "f.wav", x, 8000)
    want = np.clip(np.rint(x * np.float32(32767)), -32768, 32767).astype(np.int16)
    with wave.open(str(tmp_path / "f.wav"), "rb") as fh:
        assert fh.getframerate() == 8000 and np.array_equal(np.frombuffer(fh.readframes(len(x)), "<i2"), want)
    assert want[-4] == 32767 and want[-3] == -32768 and want[4] == -32767
    write_wav(tmp_path / "empty.wav", np.zeros(0, np.int16))
    assert read_wav(tmp_path / "empty.wav").numel() == 0
    write_wav(tmp_path / "row.wav", torch.zeros(1, 5))  # [1, n] is mono
    assert read_wav(tmp_path / "row.wav").shape == (5,)


def test_indexed_loader(tmp_path):
    paths = []
    for i in range(2):
        write_wav(tmp_path / f"{i}.wav", np.full(10 + i, 1000 * (i + 1), np.int16))
        paths.append(tmp_path / f"{i}.wav")
    load = create_indexed_audio_loader(paths)
    for i in range(2):
        got = load(i)
        assert got.dtype == torch.float32 and got.shape == (10 + i,) and bool((got == 1000 * (i + 1) / 32768).all())
    with pytest.raises(IndexError, match="Sample index 2 out of range"):
        load(2)


# ---- 4: clip tables against hand-computed bounds ------------------------------------------------------------------------------
def test_config_is_the_references_plus_two_fields():
    cfg = AudioClipConfig()
    assert list(cfg.__dataclass_fields__) == ["sample_rate", "samples_per_frame", "clip_duration_ms", "context_before_ms",
                                              "output_format", "normalize_audio", "fade_ms", "target_peak"]
    assert (cfg.sample_rate, cfg.samples_per_frame, cfg.clip_duration_ms, cfg.context_before_ms, cfg.output_format,
            cfg.normalize_audio, cfg.fade_ms, cfg.target_peak) == (16000, 160, 1000.0, 500.0, "wav", True, 0.0, 0.95)
    assert cfg.ms_to_samples(1000.0) == 16000 and cfg.ms_to_samples(2.5) == 40 and cfg.ms_to_samples(0.03) == 0


def test_clip_table_for_activations():
    ex = [FeatureActivation(0, 1.0, sample_idx=7, position_idx=0), FeatureActivation(0, 0.5, sample_idx=3, position_idx=10),
          FeatureActivation(1, 0.25, sample_idx=7, position_idx=1499)]
    sample, start, count = clip_table_for_activations(ex, AudioClipConfig(**CFG))
    assert sample.tolist() == [7, 3, 7] and start.tolist() == [-400, 1200, 239440] and count.tolist() == [800, 800, 800]
    assert (sample.dtype, start.dtype, count.dtype) == (torch.int64, torch.int64, torch.int32)
    _, start, count = clip_table_for_activations(ex)  # the defaults: 1 s, half of it before; 160 samples per frame
    assert start.tolist() == [-8000, -6400, 231840] and count.tolist() == [16000] * 3
    _, start, _ = clip_table_for_activations(ex, AudioClipConfig(samples_per_frame=320, **CFG))  # encoder frames
    assert start.tolist() == [-400, 2800, 479280]
    assert [t.numel() for t in clip_table_for_activations([])] == [0, 0, 0]


def test_clip_table_for_events():
    # an utterance of 10 encoder frames (3200 samples): a run at frame 0, one in the middle, one ending at the last frame
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    ev = FeatureEvents(feature=i32(4, 4, 9), utterance=i32(0, 0, 2), start=i32(0, 3, 7), length=i32(3, 1, 3),
                       total=torch.ones(3), peak=torch.ones(3))
    utt, start, count = clip_table_for_events(ev)
    assert utt.tolist() == [0, 0, 2] and start.tolist() == [0, 960, 2240] and count.tolist() == [960, 320, 960]
    assert (utt.dtype, start.dtype, count.dtype) == (torch.int32, torch.int64, torch.int32)
    assert (start + count).tolist() == [960, 1280, 3200]  # the last run ends with the utterance
    lo, hi = ev.sample_bounds(320, 2)
    utt, start, count = clip_table_for_events(ev, context_frames=2)
    assert start.tolist() == lo.tolist() == [0, 320, 1600] and (start + count).tolist() == hi.tolist() == [1600, 1920, 3840]
    _, start, count = clip_table_for_events(ev, stride=1, context_frames=1, max_samples=500)
    assert start.tolist() == [0, 320, 960] and count.tolist() == [500, 480, 500]  # 640, 480 and 800 before the cut


# ---- 5: manifest and reports against the reference's JSON --------------------------------------------------------------------
@pytest.fixture()
def golden_run(tmp_path):
    doc = json.loads((GOLDEN / "g20_manifest.json").read_text())
    (tmp_path / "state.json").write_text(json.dumps(doc["tracker_state"]))
    tracker = TopKTracker.load(tmp_path / "state.json")
    return doc, tracker


def relative(obj, root: Path):
    return json.loads(json.dumps(obj).replace(str(root) + "/", ""))


def test_manifest_and_reports_equal_the_references(golden_run, tmp_path):
    doc, tracker = golden_run
    out = tmp_path / "clips"
    ex = AudioClipExtractor(tracker, lambda i: None, out, AudioClipConfig(**CFG))
    assert ex.examples(0) is ex.examples(0)  # the same objects on every call: audio_path stays
    for f in range(tracker.num_features):
        for rank, e in enumerate(ex.examples(f)):  # the layout extract_all_clips writes (checked on the GPU)
            e.audio_path = str(out / f"feature_{f:05d}" / f"rank{rank:02d}_act{e.activation_value:.3f}.wav")
    path = ex.save_manifest()
    assert path == out / "manifest.json"
    assert relative(json.loads(path.read_text()), out) == doc["manifest"]
    assert {f: [m["audio_path"] for m in lst] for f, lst in doc["manifest"]["features"].items()} == doc["written"]

    report = FeatureReport(tracker, tmp_path / "reports", clips=ex)
    report.add_interpretation(2, "phoneme", "fires on a synthetic burst", confidence=0.75, evidence=["rank 0", "rank 1"])
    for f in range(tracker.num_features):
        assert relative(report.generate_feature_report(f), out) == doc["feature_reports"][str(f)], f
    assert "audio_path" not in json.dumps(report.generate_feature_report(0, include_audio_paths=False))
    assert report.generate_summary_report(top_n=4) == doc["summary"]
    report.save_reports(top_n=4)
    assert json.loads((tmp_path / "reports" / "summary.json").read_text()) == doc["summary"]
    for entry in doc["summary"]["top_features"]:
        f = entry["feature_idx"]
        saved = json.loads((tmp_path / "reports" / "features" / f"feature_{f:05d}.json").read_text())
        assert relative(saved, out) == doc["feature_reports"][str(f)]
    assert json.loads((tmp_path / "reports" / "tracker_state.json").read_text())["num_features"] == tracker.num_features
    # without an extractor the tracker's own (fresh) examples are reported: the same but for the paths
    plain = FeatureReport(tracker, tmp_path / "plain").generate_feature_report(1)
    want = doc["feature_reports"]["1"]
    assert [{k: v for k, v in e.items() if k != "audio_path"} for e in want["top_examples"]] == plain["top_examples"]


def test_interpretation_takes_automated_labels():
    labels = {"label": "AH", "metric": "f1", "score": 0.5, "threshold": 0.25, "lag": 0, "precision": 0.5, "recall": 0.5}
    it = FeatureInterpretation(3, "phoneme", "the vowel AH", 0.9, automated_labels=labels)
    assert it.to_dict() == {"feature_idx": 3, "category": "phoneme", "description": "the vowel AH", "confidence": 0.9,
                            "evidence": [], "automated_labels": labels}
    assert list(it.to_dict()) == ["feature_idx", "category", "description", "confidence", "evidence", "automated_labels"]


# ---- 6: the Python layer's errors ----------------------------------------------------------------------------------------------
def test_python_layer_errors_without_a_gpu(tmp_path):
    one = [0]
    for kw, word in ((dict(layout="columns"), "layout must be"), (dict(fade=-1), "fade and gap"), (dict(gap=-1), "fade and gap"),
                     (dict(target=math.nan), "target must be finite"), (dict(max_count=-1), "max_count must not be negative")):
        with pytest.raises(ValueError, match=word):
            cut_clips(None, one, one, one, **kw)
    with pytest.raises(ValueError, match="utt must be 1-D"):
        cut_clips(None, [[0]], one, one)
    with pytest.raises(ValueError, match="start must hold integers"):
        cut_clips(None, one, [0.5], one)
    with pytest.raises(ValueError, match="one entry per clip, got 1, 2, 1"):
        cut_clips(None, one, [0, 1], one)
    with pytest.raises(ValueError, match="bank must be a WaveformBank, got NoneType"):
        cut_clips(None, one, one, one)

    with pytest.raises(ValueError, match=r"waveforms must be \[n_utt, samples\]"):
        WaveformBank(torch.zeros(5))
    with pytest.raises(ValueError, match="float32 or int16, got torch.float64"):
        WaveformBank(torch.zeros(2, 5, dtype=torch.float64))
    with pytest.raises(ValueError, match="float32 or int16, got torch.int32"):
        WaveformBank([torch.zeros(5, dtype=torch.int32)])
    with pytest.raises(ValueError, match="the list of waveforms is empty"):
        WaveformBank([])
    with pytest.raises(ValueError, match="lengths come from the waveforms"):
        WaveformBank([torch.zeros(5)], lengths=[5])
    with pytest.raises(ValueError, match="waveform 1 must be a 1-D tensor"):
        WaveformBank([torch.zeros(5), torch.zeros(1, 5)])
    with pytest.raises(ValueError, match="waveform 1 is torch.int16, waveform 0 is torch.float32"):
        WaveformBank([torch.zeros(5), torch.zeros(5, dtype=torch.int16)])
    with pytest.raises(ValueError, match="lengths has 3 entries for 2 utterances"):
        WaveformBank(torch.zeros(2, 5), lengths=[1, 2, 3])
    with pytest.raises(N.WsaeError, match="cannot run on 'cpu'"):
        WaveformBank(torch.zeros(2, 5), device="cpu")

    ev = FeatureEvents(*(torch.zeros(1, dtype=torch.int32) for _ in range(4)), torch.zeros(1), torch.zeros(1))
    with pytest.raises(ValueError, match="stride must be positive"):
        clip_table_for_events(ev, stride=0)
    with pytest.raises(ValueError, match="max_samples must not be negative"):
        clip_table_for_events(ev, max_samples=-1)
    with pytest.raises(ValueError, match="context_frames not negative"):
        clip_table_for_events(ev, context_frames=-1)
    with pytest.raises(ValueError, match="samples_per_frame >= 1"):
        clip_table_for_activations([], AudioClipConfig(samples_per_frame=0))

    with pytest.raises(ValueError, match="samples must be 1-D"):
        write_wav(tmp_path / "x.wav", np.zeros((2, 5), np.float32))
    with pytest.raises(ValueError, match="int16 or floating point, got int32"):
        write_wav(tmp_path / "x.wav", np.zeros(5, np.int32))
    with pytest.raises(ValueError, match="sample_rate must be positive"):
        write_wav(tmp_path / "x.wav", np.zeros(5, np.int16), 0)
    with wave.open(str(tmp_path / "stereo.wav"), "wb") as fh:
        fh.setnchannels(2)
        fh.setsampwidth(2)
        fh.setframerate(16000)
        fh.writeframes(b"\0" * 8)
    with pytest.raises(ValueError, match="need mono 16-bit PCM, got 2 channel"):
        read_wav(tmp_path / "stereo.wav")

    tracker = TopKTracker(num_features=2, k=1)
    with pytest.raises(ValueError, match="bank_bytes must be positive"):
        AudioClipExtractor(tracker, lambda i: None, tmp_path / "c", bank_bytes=0)
    if AE._soundfile() is None:
        with pytest.raises(ValueError, match="output_format 'flac' needs soundfile"):
            AudioClipExtractor(tracker, lambda i: None, tmp_path / "c", AudioClipConfig(output_format="flac"))
    ex = AudioClipExtractor(tracker, lambda i: None, tmp_path / "c")
    assert (tmp_path / "c").is_dir() and ex.config == AudioClipConfig() and ex.extract_all_clips() == {}
    with pytest.raises(ValueError, match="gap_ms must not be negative"):
        ex.extract_all_clips(gap_ms=-1.0)
