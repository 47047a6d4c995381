"""Audio clip export: from a top list or a list of run events to something a human can play.

A feature is interpreted by listening to what it fires on.  ``WaveformBank`` keeps the waveforms of a set of utterances on
the device, ``cut_clips`` cuts any number of ragged sample ranges out of it in one call of ``wsae_clip_extract`` - bounds,
peak, gain, linear fades and the conversion to float32 or 16-bit PCM (include/wsae.h carries the arithmetic,
tests/clip_oracle.py restates it) - and ``AudioClipExtractor`` offers the reference's interface on top: the clips of the
features of a ``TopKTracker`` as ``feature_{idx:05d}/rank{rank:02d}_act{value:.3f}.wav`` plus a manifest, with one bank,
one launch and one copy to the host per chunk of features, and every utterance loaded once per chunk.  WAV files are
written and read with the standard library's ``wave`` (mono, 16-bit PCM); ``soundfile`` is used for other formats and for
reading when it is installed.

Frames and samples: ``AudioClipConfig.samples_per_frame`` defaults to 160, as in the reference, which is one MEL frame.
Whisper's encoder halves the frame rate, so positions of encoder activations (what an SAE on the encoder sees) need
``samples_per_frame=320``; ``clip_table_for_events`` takes that stride directly (``stride=2``).

Out of scope: decoding other audio formats without ``soundfile``, resampling, stereo, the LibriSpeech loader (it needs
``datasets`` and a download).  There is no CPU path for the cutting itself.
"""

from __future__ import annotations

import json
import wave
from dataclasses import dataclass
from pathlib import Path
from typing import Callable, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from .. import _native as N
from .._device import workspace
from ..data.audio import HOP
from ..data.waveforms import _DTYPES, pack_waveforms
from .feature_viz import FeatureActivation, TopKTracker
from .temporal import FeatureEvents


@dataclass
class AudioClipConfig:
    """The reference's six fields with its defaults, then ``fade_ms`` (a linear fade in and out of that length; 0 = none,
    the reference's behaviour) and ``target_peak`` (what the largest sample of a normalised clip becomes).

    ``samples_per_frame = 160`` is the reference's value: 10 ms, one mel frame.  Whisper's ENCODER frames are 20 ms - the
    second convolution has stride 2 - so clips for encoder positions need ``samples_per_frame=320``."""

    sample_rate: int = 16000
    samples_per_frame: int = 160
    clip_duration_ms: float = 1000.0
    context_before_ms: float = 500.0
    output_format: str = "wav"
    normalize_audio: bool = True
    fade_ms: float = 0.0
    target_peak: float = 0.95

    def ms_to_samples(self, ms: float) -> int:
        return int(ms * self.sample_rate / 1000)


class ClipBatch(NamedTuple):
    """``samples``: ``[n_clips, max_count]`` (layout ``"rows"``) or 1-D (``"montage"``), float32 or int16, zero wherever no
    clip wrote; ``offsets`` int64: the first cell of each clip in ``samples.reshape(-1)``; ``lengths`` int32: its samples
    (-1: the utterance index was out of range); ``peaks`` float32: ``max |x|`` of the clip before the gain."""

    samples: Tensor
    offsets: Tensor
    lengths: Tensor
    peaks: Tensor


class WaveformBank:
    """The waveforms of ``n_utt`` utterances on the device: ``[n_utt, S]`` float32 or int16 (16-bit PCM, scaled by 2^-15
    when read), or a list of 1-D tensors of different lengths, packed once.  CPU tensors are moved.  ``lengths [n_utt]``:
    the valid samples of each row (default ``S``; from the list itself when a list is given)."""

    def __init__(self, waveforms: Union[Tensor, Sequence[Tensor]], lengths=None, device="cuda"):
        self.samples, self.lengths, self.n_utt, self.max_length, _ = pack_waveforms("WaveformBank", waveforms, lengths, device,
                                                                                   host=True, contiguous=True)
        self.device = self.samples.device
        self._ws: Optional[Tensor] = None

    @property
    def _workspace(self) -> Optional[Tensor]:  # (the name the buffer had before it became the shared ``_ws``)
        return self._ws

    @property
    def dtype(self) -> torch.dtype:
        return self.samples.dtype


def _table(name: str, t) -> Tensor:
    t = torch.as_tensor(t)
    if t.dim() != 1:
        raise ValueError(f"{name} must be 1-D, got {tuple(t.shape)}")
    if t.numel() and (t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool):
        raise ValueError(f"{name} must hold integers, got {t.dtype}")
    return t


def cut_clips(bank: WaveformBank, utt, start, count, *, normalize: bool = True, target: float = 0.95, fade: int = 0,
              pcm16: bool = False, layout: str = "rows", gap: int = 0, max_count: Optional[int] = None) -> ClipBatch:
    """Clip ``c`` is ``count[c]`` samples of utterance ``utt[c]`` of the bank from sample ``start[c]`` on: a negative start
    moves to 0 and keeps its count, the end is cut at the utterance's length.  ``normalize``: every clip with a non-zero
    peak is scaled so that its peak becomes ``target``; ``fade``: samples of linear fade at both ends; ``pcm16``: int16
    output (``rint(y * 32767)``, clamped) instead of float32.  ``layout="rows"`` gives ``[n_clips, max_count]``,
    ``"montage"`` one 1-D buffer with the clips in order and ``gap`` zeros between them.  The tables may be device tensors
    (nothing of them is read on the host when ``max_count``, the bound on ``count``, is given and the layout is rows)."""
    if layout not in ("rows", "montage"):
        raise ValueError(f"layout must be 'rows' or 'montage', got {layout!r}")
    fade, gap = int(fade), int(gap)
    if fade < 0 or gap < 0:
        raise ValueError(f"fade and gap must not be negative, got {fade}, {gap}")
    target = float(target)
    if not np.isfinite(target):
        raise ValueError(f"target must be finite, got {target}")
    utt, start, count = _table("utt", utt), _table("start", start), _table("count", count)
    n_clips = utt.numel()
    if start.numel() != n_clips or count.numel() != n_clips:
        raise ValueError(f"utt, start and count must have one entry per clip, got {n_clips}, {start.numel()}, {count.numel()}")
    if max_count is not None and int(max_count) < 0:
        raise ValueError(f"max_count must not be negative, got {max_count}")
    if not isinstance(bank, WaveformBank):
        raise ValueError(f"bank must be a WaveformBank, got {type(bank).__name__}")
    dev = bank.device
    utt = utt.to(device=dev, dtype=torch.int32).contiguous()
    start = start.to(device=dev, dtype=torch.int64).contiguous()
    count = count.to(device=dev, dtype=torch.int32).contiguous()
    max_count = int(max_count) if max_count is not None else (max(int(count.max().item()), 0) if n_clips else 0)
    out_dtype = torch.int16 if pcm16 else torch.float32
    if layout == "rows":
        samples = torch.zeros(n_clips, max_count, dtype=out_dtype, device=dev)
        offsets = torch.arange(n_clips, dtype=torch.int64, device=dev) * max_count
    else:  # the clips' lengths decide the offsets: the kernel's bounds, restated on the device
        n = torch.zeros(n_clips, dtype=torch.int64, device=dev)
        if bank.n_utt and n_clips:
            known = (utt >= 0) & (utt < bank.n_utt)
            length = bank.lengths.clamp(0, bank.max_length).to(torch.int64)[utt.clamp(0, bank.n_utt - 1).long()]
            first = start.clamp(min=0)
            n = torch.minimum(count.clamp(0, max_count).to(torch.int64), (length - first).clamp(min=0))
            n = torch.where(known, n, torch.zeros_like(n))
        ends = torch.cumsum(n + gap, 0)
        offsets = ends - (n + gap)
        samples = torch.zeros(max(int(ends[-1].item()) - gap, 0) if n_clips else 0, dtype=out_dtype, device=dev)
    lengths = torch.zeros(n_clips, dtype=torch.int32, device=dev)
    peaks = torch.zeros(n_clips, dtype=torch.float32, device=dev)
    if n_clips == 0:
        return ClipBatch(samples, offsets, lengths, peaks)
    lib = N.lib()
    need = lib.wsae_clip_workspace_bytes(n_clips, max_count)
    if need < 0:
        raise N.WsaeError(f"wsae_clip_workspace_bytes rejects n_clips={n_clips} max_count={max_count}")
    ws = workspace(bank, need, dev)
    x = bank.samples
    out = samples if samples.numel() else torch.zeros(1, dtype=out_dtype, device=dev)  # (a non-null address)
    with torch.cuda.device(dev):
        N.check(lib.wsae_clip_extract(x.data_ptr(), _DTYPES[x.dtype], bank.n_utt, max(x.stride(0), bank.max_length),
                                      bank.lengths.data_ptr(), bank.max_length, n_clips, utt.data_ptr(), start.data_ptr(),
                                      count.data_ptr(), max_count, offsets.data_ptr(),
                                      N.CLIP_GAIN_PEAK if normalize else N.CLIP_GAIN_NONE, target, fade, out.data_ptr(),
                                      _DTYPES[out_dtype], samples.numel(), lengths.data_ptr(), peaks.data_ptr(),
                                      ws.data_ptr(), ws.numel(),
                                      torch.cuda.current_stream(dev).cuda_stream), "wsae_clip_extract")
    return ClipBatch(samples, offsets, lengths, peaks)


def clip_table_for_activations(examples: Sequence[FeatureActivation], config: Optional[AudioClipConfig] = None
                               ) -> Tuple[Tensor, Tensor, Tensor]:
    """``(sample_idx, start, count)`` on the host, one entry per example, with the reference's arithmetic: the clip starts
    ``context_before_ms`` before sample ``position_idx * samples_per_frame`` (a negative start is left to the cutter, which
    moves it to 0 and keeps the count) and has ``clip_duration_ms`` worth of samples."""
    cfg = config or AudioClipConfig()
    context, duration = cfg.ms_to_samples(cfg.context_before_ms), cfg.ms_to_samples(cfg.clip_duration_ms)
    if duration < 0 or cfg.samples_per_frame < 1:
        raise ValueError(f"need clip_duration_ms >= 0 and samples_per_frame >= 1, got {cfg.clip_duration_ms}, "
                         f"{cfg.samples_per_frame}")
    sample = torch.tensor([int(e.sample_idx) for e in examples], dtype=torch.int64)
    start = torch.tensor([int(e.position_idx) * cfg.samples_per_frame - context for e in examples], dtype=torch.int64)
    return sample, start, torch.full((len(examples),), duration, dtype=torch.int32)


def clip_table_for_events(events: FeatureEvents, stride: int = 2, context_frames: int = 0,
                          max_samples: Optional[int] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """``(utt, start, count)`` on the events' device: each run of ``RunTracker.events()`` widened by ``context_frames`` on
    either side (``FeatureEvents.sample_bounds`` with ``160 * stride`` samples per frame; ``stride = 2`` for encoder
    frames), optionally cut to ``max_samples`` from its start.  The cutter clips the end to the utterance's length."""
    stride = int(stride)
    if stride < 1:
        raise ValueError(f"stride must be positive, got {stride}")
    if max_samples is not None and int(max_samples) < 0:
        raise ValueError(f"max_samples must not be negative, got {max_samples}")
    lo, hi = events.sample_bounds(HOP * stride, context_frames)
    count = hi - lo
    if max_samples is not None:
        count = count.clamp(max=int(max_samples))
    if count.numel() and int(count.max().item()) > 2 ** 30:
        raise ValueError("a run is longer than 2^30 samples")
    return events.utterance.to(torch.int32), lo, count.to(torch.int32)


# ---- files -----------------------------------------------------------------------------------------------------------
def pcm16(samples) -> np.ndarray:
    """int16 passes through; floats become ``clamp(rint(x * 32767), -32768, 32767)`` in float32: the cutter's rule."""
    a = samples.detach().cpu().numpy() if isinstance(samples, Tensor) else np.asarray(samples)
    if a.ndim == 2 and a.shape[0] == 1:
        a = a[0]
    if a.ndim != 1:
        raise ValueError(f"samples must be 1-D (mono), got shape {tuple(a.shape)}")
    if a.dtype == np.int16:
        return np.ascontiguousarray(a)
    if not np.issubdtype(a.dtype, np.floating):
        raise ValueError(f"samples must be int16 or floating point, got {a.dtype}")
    scaled = np.rint(a.astype(np.float32) * np.float32(32767))
    return np.clip(scaled, -32768, 32767).astype(np.int16)


def write_wav(path, samples, sample_rate: int = 16000, channels: int = 1) -> None:
    """A 16-bit PCM WAV file through the standard library's ``wave``: mono, or with ``channels > 1`` the interleaved frames
    ``samples [n, channels]``."""
    sample_rate, channels = int(sample_rate), int(channels)
    if sample_rate < 1:
        raise ValueError(f"sample_rate must be positive, got {sample_rate}")
    if channels > 1:
        a = samples.detach().cpu().numpy() if isinstance(samples, Tensor) else np.asarray(samples)
        if a.ndim != 2 or a.shape[1] != channels:
            raise ValueError(f"samples must be [n, {channels}], got shape {tuple(a.shape)}")
        data = pcm16(a.reshape(-1))
    else:
        data = pcm16(samples)
    with wave.open(str(path), "wb") as fh:
        fh.setnchannels(channels)
        fh.setsampwidth(2)
        fh.setframerate(sample_rate)
        fh.writeframes(data.astype("<i2", copy=False).tobytes())


def read_wav(path, return_rate: bool = False, mono: bool = True):
    """A mono 16-bit PCM WAV file as a float32 tensor, samples scaled by 2^-15 (exact); with ``return_rate`` the pair
    ``(samples, sample_rate)``.  With ``mono=False`` a file of several channels is read too, as interleaved frames
    ``[n, channels]`` (what ``Resampler`` takes)."""
    with wave.open(str(path), "rb") as fh:
        channels = fh.getnchannels()
        if (mono and channels != 1) or fh.getsampwidth() != 2:
            raise ValueError(f"{path}: need {'mono ' if mono else ''}16-bit PCM, got {channels} channel(s) of {8 * fh.getsampwidth()} bits")
        rate = fh.getframerate()
        raw = fh.readframes(fh.getnframes())
    samples = torch.from_numpy(np.frombuffer(raw, dtype="<i2").astype(np.float32) * np.float32(2.0 ** -15))
    if channels > 1:
        samples = samples.reshape(-1, channels)
    return (samples, rate) if return_rate else samples


def _soundfile():
    try:
        import soundfile
        return soundfile
    except ImportError:
        return None


def create_indexed_audio_loader(audio_paths: Sequence[Union[Path, str]]) -> Callable[[int], Tensor]:
    """``load(sample_idx) -> float32 tensor`` over a list of audio files indexed by ``sample_idx``: through ``soundfile``
    when it is installed, else ``read_wav``.  ``IndexError`` past the end of the list."""
    paths = list(audio_paths)
    sf = _soundfile()

    def load_audio(sample_idx: int) -> Tensor:
        if sample_idx >= len(paths):
            raise IndexError(f"Sample index {sample_idx} out of range")
        if sf is not None:
            data, _ = sf.read(paths[sample_idx])
            return torch.from_numpy(data).float()
        return read_wav(paths[sample_idx])

    return load_audio


def _mono(audio) -> Tensor:
    """What a loader returned as a 1-D float32 or int16 CPU tensor (``[1, n]`` is squeezed, as in the reference)."""
    a = torch.as_tensor(audio).detach().cpu()
    if a.dim() == 2:
        a = a.squeeze(0)
    if a.dim() != 1:
        raise ValueError(f"audio must be [samples] or [1, samples], got {tuple(a.shape)}")
    return a if a.dtype == torch.int16 else a.to(torch.float32)


class AudioClipExtractor:
    """The reference's extractor on the device: ``extract_clip``, ``extract_feature_clips``, ``extract_all_clips`` and
    ``save_manifest`` with its file layout.  ``audio_loader(sample_idx)`` returns ``[samples]`` or ``[1, samples]``;
    ``bank_bytes`` bounds the waveforms (and the clips) that one chunk of features puts on the device.

    The tracker builds its examples anew on every read, so the extractor keeps the lists it has handed out
    (``examples(feature_idx)``): ``audio_path`` is written into those, and the manifest and ``FeatureReport(clips=...)``
    read them."""

    def __init__(self, tracker: TopKTracker, audio_loader: Callable[[int], Tensor], output_dir, config: Optional[AudioClipConfig] = None,
                 *, device=None, bank_bytes: int = 1 << 30):
        self.tracker, self.audio_loader = tracker, audio_loader
        self.output_dir = Path(output_dir)
        self.config = config or AudioClipConfig()
        if self.config.output_format != "wav" and _soundfile() is None:
            raise ValueError(f"output_format {self.config.output_format!r} needs soundfile, which is not installed; "
                             f"'wav' is written with the standard library")
        if int(bank_bytes) < 1:
            raise ValueError(f"bank_bytes must be positive, got {bank_bytes}")
        self.device = device if device is not None else getattr(tracker, "device", None) or "cuda"
        self.bank_bytes = int(bank_bytes)
        self.loads = 0  # calls of audio_loader so far
        self._examples: dict = {}
        self.output_dir.mkdir(parents=True, exist_ok=True)

    def examples(self, feature_idx: int) -> list:
        """The feature's examples, strongest first - the same objects on every call, ``audio_path`` filled in once cut."""
        if feature_idx not in self._examples:
            self._examples[feature_idx] = self.tracker.get_top_examples(feature_idx)
        return self._examples[feature_idx]

    def _load(self, sample_idx: int) -> Optional[Tensor]:
        self.loads += 1
        try:
            return _mono(self.audio_loader(sample_idx))
        except Exception as exc:  # a loader that raises costs that utterance's clips, never the run
            print(f"Failed to load audio for sample {sample_idx}: {exc}")
            return None

    def _cut(self, waves: list, utt, start, count, pcm: bool) -> ClipBatch:
        if any(w.dtype != waves[0].dtype for w in waves):  # 16-bit and float utterances in one chunk: all float
            waves = [w.to(torch.float32) * 2.0 ** -15 if w.dtype == torch.int16 else w for w in waves]
        cfg = self.config
        bank = WaveformBank(waves, device=self.device)
        return cut_clips(bank, utt, start, count, normalize=cfg.normalize_audio, target=cfg.target_peak,
                         fade=cfg.ms_to_samples(cfg.fade_ms), pcm16=pcm, layout="rows")

    # ---- one clip ------------------------------------------------------------------------------------------------------
    def extract_clip(self, activation: FeatureActivation, audio: Optional[Tensor] = None) -> Optional[Tensor]:
        """The clip of one activation as a float32 CPU tensor (cut on the device), or None when the loader raised."""
        if audio is None:
            self.loads += 1
            try:
                audio = self.audio_loader(activation.sample_idx)
            except Exception:
                return None
        _, start, count = clip_table_for_activations([activation], self.config)
        batch = self._cut([_mono(audio)], [0], start, count, pcm=False)
        return batch.samples[0, :int(batch.lengths[0].item())].cpu()

    # ---- many clips ----------------------------------------------------------------------------------------------------
    def _save(self, pcm: np.ndarray, path: Path) -> None:
        if self.config.output_format == "wav":
            write_wav(path, pcm, self.config.sample_rate)
        else:
            _soundfile().write(str(path), pcm, self.config.sample_rate)

    def _flush(self, features: list, waves: dict, montage: bool, gap: int, result: dict) -> None:
        """One chunk: ``features`` = [(feature_idx, examples)], ``waves`` = {sample_idx: tensor or None}."""
        rows = {s: i for i, s in enumerate(s for s, w in waves.items() if w is not None)}
        jobs = []  # (feature, rank, example)
        for f, examples in features:
            jobs += [(f, rank, ex) for rank, ex in enumerate(examples) if ex.sample_idx in rows]
        if jobs:
            _, start, count = clip_table_for_activations([ex for _, _, ex in jobs], self.config)
            batch = self._cut([w for w in waves.values() if w is not None], [rows[ex.sample_idx] for _, _, ex in jobs],
                              start, count, pcm=True)
            pcm, lengths = batch.samples.cpu().numpy(), batch.lengths.cpu().numpy()  # the one copy of the chunk
        silence = np.zeros(gap, np.int16)
        at = 0
        for f, examples in features:
            feature_dir = self.output_dir / f"feature_{f:05d}"
            feature_dir.mkdir(exist_ok=True)
            paths, pieces = [], []
            while at < len(jobs) and jobs[at][0] == f:
                _, rank, ex = jobs[at]
                clip = pcm[at, :max(int(lengths[at]), 0)]
                path = feature_dir / f"rank{rank:02d}_act{ex.activation_value:.3f}.{self.config.output_format}"
                self._save(clip, path)
                ex.audio_path = str(path)
                paths.append(path)
                pieces += [silence, clip] if pieces else [clip]
                at += 1
            if montage and pieces:
                self._save(np.concatenate(pieces), feature_dir / f"montage.{self.config.output_format}")
            if paths:
                result[f] = paths

    def extract_all_clips(self, feature_indices: Optional[Sequence[int]] = None, max_clips_per_feature: Optional[int] = None,
                          progress_callback: Optional[Callable[[int, int], None]] = None, *, montage: bool = False,
                          gap_ms: float = 250.0) -> dict:
        """``{feature_idx: [paths]}`` for every feature with examples (or the given ones).  Features are taken in chunks
        whose utterances - and whose clips - fit ``bank_bytes``; per chunk every utterance is loaded once, one bank is
        packed, one launch cuts all clips as 16-bit PCM, one copy brings them to the host and the files are written.
        ``montage``: also ``feature_{idx:05d}/montage.wav``, the feature's clips in rank order, ``gap_ms`` of silence apart."""
        if feature_indices is None:
            feature_indices = [i for i in range(self.tracker.num_features) if self.examples(i)]
        gap = self.config.ms_to_samples(gap_ms)
        if gap < 0:
            raise ValueError(f"gap_ms must not be negative, got {gap_ms}")
        clip_bytes = 2 * max(self.config.ms_to_samples(self.config.clip_duration_ms), 0)
        result: dict = {}
        total = len(feature_indices)
        chunk, waves, used = [], {}, 0
        for done, f in enumerate(feature_indices):
            if progress_callback:
                progress_callback(done, total)
            examples = self.examples(f)
            if max_clips_per_feature:
                examples = examples[:max_clips_per_feature]
            fresh = {}
            for ex in examples:
                if ex.sample_idx not in waves and ex.sample_idx not in fresh:
                    fresh[ex.sample_idx] = self._load(ex.sample_idx)
            cost = sum(w.numel() * w.element_size() for w in fresh.values() if w is not None) + clip_bytes * len(examples)
            if chunk and used + cost > self.bank_bytes:  # this feature opens the next chunk and takes its utterances along
                carried = {ex.sample_idx: waves[ex.sample_idx] for ex in examples if ex.sample_idx in waves}
                self._flush(chunk, waves, montage, gap, result)
                chunk, waves = [], carried
                used = sum(w.numel() * w.element_size() for w in carried.values() if w is not None)
            waves.update(fresh)
            chunk.append((f, examples))
            used += cost
        if chunk:
            self._flush(chunk, waves, montage, gap, result)
        return result

    def extract_feature_clips(self, feature_idx: int, max_clips: Optional[int] = None) -> list:
        """The clips of one feature (a chunk of one): the paths written."""
        return self.extract_all_clips([feature_idx], max_clips_per_feature=max_clips).get(feature_idx, [])

    def save_manifest(self) -> Path:
        """``manifest.json`` in the reference's form: the config and, per feature, the examples that have a clip."""
        manifest = {"config": {"sample_rate": self.config.sample_rate, "clip_duration_ms": self.config.clip_duration_ms,
                               "output_format": self.config.output_format},
                    "features": {}}
        for f in range(self.tracker.num_features):
            examples = self.examples(f)
            if examples:
                manifest["features"][str(f)] = [
                    {"rank": i, "activation_value": ex.activation_value, "sample_idx": ex.sample_idx,
                     "position_idx": ex.position_idx, "timestamp_ms": ex.timestamp_ms, "audio_path": ex.audio_path,
                     "transcription": ex.transcription}
                    for i, ex in enumerate(examples) if ex.audio_path]
        path = self.output_dir / "manifest.json"
        with open(path, "w") as fh:
            json.dump(manifest, fh, indent=2)
        return path


__all__ = ["AudioClipConfig", "AudioClipExtractor", "ClipBatch", "WaveformBank", "clip_table_for_activations",
           "clip_table_for_events", "create_indexed_audio_loader", "cut_clips", "pcm16", "read_wav", "write_wav"]
