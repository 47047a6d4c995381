"""Log-mel front end: waveforms in, Whisper's ``input_features`` out, on the device.

``LogMel`` holds the two tables of ``wsae_logmel`` - the windowed DFT basis and the mel filter bank - and a workspace, and
turns a batch of waveforms (float32, or 16-bit PCM) into ``[n_utt, n_mels, frames]`` float32, the layout the encoder takes.
The arithmetic is fixed operation by operation in ``include/wsae.h``; ``tests/logmel_oracle.py`` restates it in numpy.
Framing follows the installed ``WhisperFeatureExtractor`` after its padding to ``n_samples``: a reflect pad of 200 samples
around the padded signal, frames of 400 samples every 160, and no frame beyond ``n_samples / 160``.

Other rates and channel counts go through ``Resampler`` / ``AudioFrontEnd`` (``resample.py``) first.  Out of scope: decoding
audio files other than 16-bit PCM WAV, dithering, other ``n_fft`` / hop values, chunking of recordings longer than
``n_samples``.  There is no CPU path.
"""

from __future__ import annotations

from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from .. import _native as N
from .._device import gpu_device, workspace
from .waveforms import _DTYPES, head_device, pack_waveforms

N_FFT, HOP, N_BINS, SAMPLE_RATE = N.LOGMEL_NFFT, N.LOGMEL_HOP, N.LOGMEL_BINS, 16000
N_SAMPLES = 30 * SAMPLE_RATE  # Whisper's 30 s window
MEL_PER_ENCODER_FRAME = 2     # the encoder's second convolution has stride 2


def _slaney_mel(hz):
    hz = np.asarray(hz, dtype=np.float64)
    mels = 3.0 * hz / 200.0
    log_region = hz >= 1000.0
    mels[log_region] = 15.0 + np.log(hz[log_region] / 1000.0) * (27.0 / np.log(6.4))
    return mels


def _slaney_hz(mels):
    mels = np.asarray(mels, dtype=np.float64)
    hz = 200.0 * mels / 3.0
    log_region = mels >= 15.0
    hz[log_region] = 1000.0 * np.exp((np.log(6.4) / 27.0) * (mels[log_region] - 15.0))
    return hz


def mel_filter_bank(n_mels: int) -> np.ndarray:
    """Whisper's filter bank, float64 ``[201, n_mels]``: triangles on the Slaney mel scale between 0 and 8000 Hz over the
    201 bins of a 400-point DFT at 16 kHz, each scaled by ``2 / (its width in Hz)`` (Slaney's area normalisation).  The
    operations and their order are those of ``transformers.audio_utils.mel_filter_bank(201, n_mels, 0, 8000, 16000,
    "slaney", "slaney")``, so the two agree bit for bit (tests/test_logmel.py); nothing of ``transformers`` is imported."""
    n_mels = int(n_mels)
    if n_mels < 1:
        raise ValueError(f"n_mels must be positive, got {n_mels}")
    lo, hi = _slaney_mel(np.array([0.0, 8000.0]))
    edges = _slaney_hz(np.linspace(lo, hi, n_mels + 2))
    bins = np.linspace(0, SAMPLE_RATE // 2, N_BINS)
    width = np.diff(edges)
    slopes = np.expand_dims(edges, 0) - np.expand_dims(bins, 1)
    down = -slopes[:, :-2] / width[:-1]
    up = slopes[:, 2:] / width[1:]
    bank = np.maximum(np.zeros(1), np.minimum(down, up))
    bank *= np.expand_dims(2.0 / (edges[2:n_mels + 2] - edges[:n_mels]), 0)
    return bank


def hann_window() -> np.ndarray:
    """The periodic Hann window of 400 points, float64 (``np.hanning(401)[:-1]``: what the extractor multiplies by)."""
    return np.hanning(N_FFT + 1)[:-1]


def dft_basis() -> np.ndarray:
    """The DFT table of ``wsae_logmel``, float32 ``[400, 416]``: column ``k`` (0..200) is ``w[n] cos(2 pi ((k n) mod 400) /
    400)``, column ``208 + k`` the same with ``sin``; the other columns are zero.  Computed in float64 - the argument is
    reduced in integers first - and rounded once."""
    n = np.arange(N_FFT, dtype=np.int64)[:, None]
    k = np.arange(N_BINS, dtype=np.int64)[None, :]
    angle = 2.0 * np.pi * ((k * n) % N_FFT).astype(np.float64) / N_FFT
    w = hann_window()[:, None]
    table = np.zeros((N_FFT, N.LOGMEL_COLS), dtype=np.float64)
    table[:, :N_BINS] = w * np.cos(angle)
    table[:, N.LOGMEL_SIN_COL:N.LOGMEL_SIN_COL + N_BINS] = w * np.sin(angle)
    return table.astype(np.float32)


def frame_of_sample(sample: int, stride: int = MEL_PER_ENCODER_FRAME) -> int:
    """The encoder frame (``stride = 2``; mel frame with ``stride = 1``) whose hop interval holds ``sample``."""
    if sample < 0 or stride < 1:
        raise ValueError(f"need sample >= 0 and stride >= 1, got {sample}, {stride}")
    return int(sample) // (HOP * int(stride))


def sample_span_of_frames(first: int, last: int, stride: int = MEL_PER_ENCODER_FRAME) -> Tuple[int, int]:
    """``(start, stop)``: the samples ``[start, stop)`` that frames ``first .. last`` (inclusive, as ``RunTracker``'s events
    give them) advance over - 160 samples per mel frame, ``stride`` mel frames per frame: 320 per encoder frame, the
    arithmetic of the reference's ``AudioClipConfig``.  (A mel frame also *sees* 120 samples on either side of its hop.)"""
    if first < 0 or last < first or stride < 1:
        raise ValueError(f"need 0 <= first <= last and stride >= 1, got {first}, {last}, {stride}")
    step = HOP * int(stride)
    return int(first) * step, (int(last) + 1) * step


class LogMel:
    """``LogMel(n_mels)(waveforms, lengths) -> [n_utt, n_mels, n_samples / 160]`` float32 on ``device``.

    ``filters``: a ``[201, n_mels]`` array or tensor in place of ``mel_filter_bank(n_mels)``; ``basis``: a ``[400, 416]``
    float32 table in place of ``dft_basis()`` (the tests pass integer tables).  The tables go to the device once; the
    workspace grows on demand and is reused."""

    def __init__(self, n_mels: int = 80, device="cuda", n_samples: int = N_SAMPLES, filters=None, basis=None):
        n_mels, n_samples = int(n_mels), int(n_samples)
        if n_mels not in (80, 128):
            raise ValueError(f"n_mels must be 80 or 128, got {n_mels}")
        if n_samples % HOP or n_samples < 3 * HOP:
            raise ValueError(f"n_samples must be a multiple of {HOP} and at least {3 * HOP}, got {n_samples}")
        filt = torch.as_tensor(mel_filter_bank(n_mels) if filters is None else filters)
        if tuple(filt.shape) != (N_BINS, n_mels):
            raise ValueError(f"filters must be [{N_BINS}, {n_mels}], got {tuple(filt.shape)}")
        table = torch.as_tensor(dft_basis() if basis is None else basis)
        if tuple(table.shape) != (N_FFT, N.LOGMEL_COLS):
            raise ValueError(f"basis must be [{N_FFT}, {N.LOGMEL_COLS}], got {tuple(table.shape)}")
        self.device = gpu_device("LogMel", device)
        self.n_mels, self.n_samples, self.frames = n_mels, n_samples, n_samples // HOP
        self.filters = filt.to(device=self.device, dtype=torch.float32).contiguous()
        self.basis = table.to(device=self.device, dtype=torch.float32).contiguous()
        self._ws: Optional[Tensor] = None

    @staticmethod
    def is_waveform(t) -> bool:
        """Whether ``t`` is a batch of waveforms ``[n_utt, S]`` (and not of mel features, which are 3-D)."""
        return isinstance(t, Tensor) and t.dim() == 2

    def __call__(self, waveforms: Union[Tensor, Sequence[Tensor]], lengths=None, *, out: Optional[Tensor] = None,
                 return_power: bool = False):
        """``waveforms``: ``[n_utt, S]`` on the device, float32 or int16 (scaled by 2^-15), ``S <= n_samples`` - the missing
        columns count as zeros - or a list of 1-D tensors of different lengths.  ``lengths [n_utt]``: the valid samples
        (default ``S``; values above ``S`` are clamped to it).  ``out``: a float32 ``[n_utt, n_mels, frames]`` tensor (or
        view with unit stride along the frames) to write into.  With ``return_power`` the result is ``(features,
        mel_power)``, the second the mel energies before floor and log."""
        x, lengths, n_utt, s, _ = pack_waveforms("LogMel", waveforms, lengths, self.device, max_samples=self.n_samples)
        shape = (n_utt, self.n_mels, self.frames)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        else:
            if not isinstance(out, Tensor) or tuple(out.shape) != shape or out.dtype != torch.float32:
                raise ValueError(f"out must be float32 {list(shape)}, got "
                                 f"{out.dtype} {list(out.shape)}" if isinstance(out, Tensor) else "out must be a tensor")
            if out.device != self.device:
                raise ValueError(f"out is on {out.device}, this LogMel on {self.device}")
            if out.stride(2) != 1 or out.stride(1) < self.frames or (n_utt > 1 and out.stride(0) < self.n_mels * out.stride(1)):
                raise ValueError(f"out needs unit stride along the frames and rows that do not overlap, got strides {out.stride()}")
        ld_m = out.stride(1)
        ld_u = out.stride(0) if n_utt > 1 else max(out.stride(0), self.n_mels * ld_m)
        power = None
        if return_power:
            power = torch.empty(n_utt * ld_u, dtype=torch.float32, device=self.device)
        if n_utt == 0:
            return (out, out.new_empty(shape)) if return_power else out
        lib = N.lib()
        need = lib.wsae_logmel_workspace_bytes(n_utt, self.n_samples, self.n_mels)
        if need < 0:
            raise N.WsaeError(f"wsae_logmel_workspace_bytes rejects n_utt={n_utt} n_samples={self.n_samples} n_mels={self.n_mels}")
        ws = workspace(self, need, self.device)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            N.check(lib.wsae_logmel(x.data_ptr(), _DTYPES[x.dtype], n_utt, x.stride(0) if n_utt > 1 else max(x.stride(0), s, 1),
                                    lengths.data_ptr(), s, self.n_samples, self.basis.data_ptr(), self.filters.data_ptr(),
                                    self.n_mels, out.data_ptr(), ld_m, ld_u, N.ptr(power), ws.data_ptr(), ws.numel(),
                                    stream), "wsae_logmel")
        if return_power:
            return out, power.as_strided(shape, (ld_u, ld_m, 1))
        return out


def log_mel_spectrogram(waveforms, lengths=None, *, n_mels: int = 80, device=None, n_samples: int = N_SAMPLES, filters=None,
                        **kw):
    """One-shot ``LogMel(n_mels, device, n_samples, filters)(waveforms, lengths, **kw)``; ``device`` defaults to that of
    the waveforms.  Build a ``LogMel`` once where more than one batch is converted: it keeps the tables on the device."""
    return LogMel(n_mels, head_device(waveforms) if device is None else device, n_samples, filters)(waveforms, lengths, **kw)


def features_from_batch(frontend: Optional[LogMel], batch):
    """What ``extract_and_cache_features(frontend=...)`` and ``aligned_batches(frontend=...)`` do to the first item of a
    batch: a 2-D tensor is a batch of waveforms and is converted, with the second item of a tuple / list as its lengths;
    a 3-D tensor is mel features already and passes through, as does everything when there is no front end.  An
    ``AudioFrontEnd`` also converts the 3-D tensors that are interleaved waveforms ``[n_utt, S, C]`` (its ``is_waveform``)."""
    if frontend is None:
        return batch[0] if isinstance(batch, (list, tuple)) else batch
    first = batch[0] if isinstance(batch, (list, tuple)) else batch
    if not frontend.is_waveform(first):
        return first
    return frontend(first, batch[1] if isinstance(batch, (list, tuple)) and len(batch) > 1 else None)


__all__ = ["LogMel", "dft_basis", "frame_of_sample", "hann_window", "log_mel_spectrogram", "mel_filter_bank",
           "sample_span_of_frames"]
