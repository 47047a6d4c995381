"""The reader the audio kernels share (``pcm_load`` and ``pcm_for_span``, csrc/wsae_pcm.h) on the MI355X, through the public
calls: every length of the scalar head in front of the first 16-byte boundary, spans shorter than the head, spans of exactly
one vector and one more or less, a full tile and the first element of the next, mono, stereo and the element-wise route,
float32 and int16.  The expected values are plain numpy and exact: no oracle, no tolerance."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from whisper_sae.analysis import WaveformBank, cut_clips
from whisper_sae.data import Resampler

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = (np.int16, np.float32)


def as_float(x: np.ndarray) -> np.ndarray:
    return x.astype(np.float32) * np.float32(2.0 ** -15) if x.dtype == np.int16 else x


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("dtype", DTYPES)
def test_clips_at_every_head_length_and_count(dtype):
    j = np.arange(4096 + 64 + 8, dtype=np.int64)
    if dtype == np.int16:
        x = ((j * 37) % 65536 - 32768).astype(np.int16)
    else:  # distinct multiples of 2^-10 below 4 in magnitude: every value is exact
        x = (((j * 37) % 8192 - 4096) * 2.0 ** -10).astype(np.float32)
    counts = (0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 4095, 4096, 4097)
    table = [(s, c) for s in range(9) for c in counts]
    start, count = [s for s, _ in table], [c for _, c in table]
    bank = WaveformBank(torch.from_numpy(x)[None, :], device=DEV)
    assert bank.samples.data_ptr() % 16 == 0  # (so that start is the offset from a 16-byte boundary, in elements)
    batch = cut_clips(bank, [0] * len(table), start, count, normalize=False, fade=0, pcm16=False, layout="rows")
    got, got_len = batch.samples.cpu().numpy(), batch.lengths.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (len(table), 4097)
    assert np.array_equal(got_len, np.asarray(count, np.int32))
    want = as_float(x)
    for row, (s, c) in zip(got, table):
        assert np.array_equal(bits(row[:c]), bits(want[s:s + c])), (s, c)
        assert not row[c:].any(), (s, c)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("channels", (1, 2, 3))
def test_identity_resampling_from_every_offset(channels, dtype):
    lengths = (0, 1, 3, 4, 5, 8, 9, 1023, 1024, 1025)
    rng = np.random.default_rng(channels)
    shape = (len(lengths), max(lengths) + 8, channels)
    if dtype == np.int16:
        x = rng.integers(-32768, 32768, size=shape).astype(np.int16)
    else:
        x = (rng.integers(-4095, 4096, size=shape) * 2.0 ** -10).astype(np.float32)
    f = as_float(x)
    mono = f[:, :, 0]
    for c in range(1, channels):  # the channels summed in their order, then one division
        mono = mono + f[:, :, c]
    if channels > 1:
        mono = mono / np.float32(channels)
    assert mono.dtype == np.float32
    rs = Resampler(16000, 16000, device=DEV)  # equal rates: the identity table, which still runs the kernel
    dx = torch.from_numpy(x).to(DEV)
    if channels == 1:
        dx = dx[:, :, 0]
    for o in range(9):
        y, out_len = rs(dx[:, o:], list(lengths))
        y, out_len = y.cpu().numpy(), out_len.cpu().numpy()
        assert y.dtype == np.float32 and y.shape == (len(lengths), shape[1] - o)
        assert np.array_equal(out_len, np.asarray(lengths, np.int32))
        for u, n in enumerate(lengths):
            assert np.array_equal(bits(y[u, :n]), bits(mono[u, o:o + n])), (o, u)
            assert not y[u, n:].any(), (o, u)
