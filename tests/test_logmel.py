"""The log-mel front end without a GPU: the oracles of tests/logmel_oracle.py against the installed ``transformers``
extractor, the two tables against their definitions, the reflect indices against ``np.pad``, every argument error of
``wsae_logmel`` (found on the host before any HIP call), the workspace size, and the errors of the Python layer."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import logmel_oracle as LO
from whisper_sae import _native as N
from whisper_sae.data import (LogMel, dft_basis, frame_of_sample, log_mel_spectrogram, mel_filter_bank,
                              sample_span_of_frames)

SIGNALS = ("noise", "tone_silence", "am_tone")


@pytest.fixture(scope="module")
def extractor():
    from transformers import WhisperFeatureExtractor
    return WhisperFeatureExtractor()


@pytest.fixture(scope="module")
def short():
    """P = 48000: the signals and ``ideal`` of each - computed once."""
    P = 48000
    sig = LO.signals(P)
    return P, sig, {name: LO.ideal(sig[name], P, 80) for name in SIGNALS}


@pytest.mark.parametrize("name", SIGNALS)
def test_ideal_matches_the_extractors_numpy_path_to_one_ulp(extractor, short, name):
    """Both are float64 up to the log and float32 after it; ``|.|^2`` against ``re^2 + im^2`` and ``filters.T @ power`` against
    ``power @ filters`` differ in the last float64 bits, which can move a value across a float32 rounding boundary: one
    float32 ulp at these magnitudes (values in [-1, 2): 2^-23 = 1.1920929e-07).  All 24000 cells, none excluded."""
    P, sig, ideal = short
    want = extractor._np_extract_fbank_features(sig[name][None, :], "cpu")[0]
    assert want.shape == ideal[name].shape == (80, 300) and ideal[name].dtype == np.float32
    delta = np.abs(ideal[name].astype(np.float64) - want.astype(np.float64)).max()
    print(f"{name}: max |ideal - extractor| = {delta:.8e}")
    assert delta <= 2.0 ** -23


def test_ideal_against_the_extractors_default_call(extractor):
    """The default call pads to 30 s and runs ``torch.stft`` in float32.  Measured in this setup (P = 480000, the three
    signals of ``logmel_oracle.signals``): 1.79e-06, 2.65e-05, 5.31e-05 (profiles/logmel_note.md); the bound is three times
    the largest."""
    P = 480000
    bound = 3 * 5.31e-05  # (measured, profiles/logmel_note.md)
    for name, wave in LO.signals(P).items():
        want = extractor(wave.astype(np.float32), sampling_rate=16000, return_tensors="np").input_features[0]
        got = LO.ideal(wave.astype(np.float32).astype(np.float64), P, 80)
        delta = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
        print(f"{name}: max |ideal - default extractor| = {delta:.3e} (bound {bound:.3e})")
        assert want.shape == got.shape == (80, 3000) and delta <= bound


@pytest.mark.parametrize("n_mels", (80, 128))
def test_mel_filter_bank_equals_the_library_bit_for_bit(n_mels):
    """The same numpy operations in the same order, so: bit for bit."""
    from transformers.audio_utils import mel_filter_bank as theirs
    want = theirs(201, n_mels, 0.0, 8000.0, 16000, "slaney", "slaney")
    got = mel_filter_bank(n_mels)
    assert got.dtype == np.float64 and got.shape == (201, n_mels) and np.array_equal(got, want)
    assert (got >= 0).all() and (got.max(axis=0) > 0).all()


def test_dft_basis_is_the_windowed_cosine_and_sine_to_half_an_ulp():
    b = dft_basis()
    assert b.dtype == np.float32 and b.shape == (400, N.LOGMEL_COLS)
    n = np.arange(400)[:, None]
    k = np.arange(201)[None, :]
    w = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(400) / 400))[:, None]  # the periodic Hann window, written out
    angle = 2 * np.pi * ((n * k) % 400) / 400
    for lo, exact in ((0, w * np.cos(angle)), (N.LOGMEL_SIN_COL, w * np.sin(angle))):
        got = b[:, lo:lo + 201].astype(np.float64)
        # half a float32 ulp of the exact value, plus the float64 evaluation's own error (a few 2^-53) on either side
        half_ulp = 0.5 * np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
        assert (np.abs(got - exact) <= half_ulp + 1e-15).all()
    assert (b[:, 201:N.LOGMEL_SIN_COL] == 0).all() and (b[:, N.LOGMEL_SIN_COL + 201:] == 0).all()
    assert (b[:, N.LOGMEL_SIN_COL] == 0).all()  # the sine of bin 0


@pytest.mark.parametrize("P", (480, 640, 48000))
def test_reflect_indices_match_np_pad(P):
    ramp = np.arange(P, dtype=np.float64)
    padded = np.pad(ramp, 200, mode="reflect")
    assert np.array_equal(ramp[LO.reflect_index(np.arange(-200, P + 200), P)], padded)
    frames = LO.frames_of(ramp, P)
    assert frames.shape == (P // 160, 400)
    for t in (0, 1, P // 160 - 1):
        assert np.array_equal(frames[t], padded[160 * t:160 * t + 400])


def test_mirror_agrees_with_ideal_within_its_own_bound():
    """On the package's tables the mirror (float32 tables) and ``ideal`` (float64 tables) differ by the rounding of the
    tables only - far inside what a float32 evaluation is allowed."""
    P = 160 * 65
    basis, filt = dft_basis(), mel_filter_bank(80).astype(np.float32)
    for name, wave in LO.signals(P).items():
        x = wave.astype(np.float32)
        out, e_out, mel, e_mel = LO.mirror(x, basis, filt, P)
        assert out.shape == e_out.shape == mel.shape == e_mel.shape == (80, 65)
        assert (e_out > 0).all() and (e_mel >= 0).all()
        assert (np.abs(LO.ideal(x.astype(np.float64), P, 80) - out) <= e_out + 2.0 ** -23).all(), name


def test_integer_tables_are_exact_and_asymmetric():
    basis, filt = LO.integer_tables(80)
    assert set(np.unique(basis)) == {-1.0, 0.0, 1.0} and (filt.sum(axis=0) > 0).all()
    assert not np.array_equal(basis[:, :201], basis[:, N.LOGMEL_SIN_COL:N.LOGMEL_SIN_COL + 201])
    x = np.random.default_rng(0).integers(-2, 2, size=480) / 2.0
    mel = LO.integer_mel_power(x, basis, filt, 480)
    assert mel.shape == (80, 3) and mel.max() > 0


def test_argument_errors_do_not_need_a_gpu():
    lib = N.lib()
    A = 0x1000  # any non-null aligned address: an argument error returns before anything is read
    P = 48000
    need = lib.wsae_logmel_workspace_bytes(2, P, 80)
    # x, x_dtype, n_utt, ld_x, length, max_length, n_samples, basis, filt, n_mels, out, ld_m, ld_u, mel_power, ws, ws_bytes, stream
    good = [A, N.DT_F32, 2, P, A, P, P, A, A, 80, A, 300, 80 * 300, None, A, need, None]
    cases = ((0, None, "null"), (4, None, "null"), (7, None, "null"), (8, None, "null"), (10, None, "null"),
             (1, 1, "x_dtype"), (1, 7, "x_dtype"), (2, -1, "n_utt"), (6, P + 1, "multiple of 160"), (6, 320, "n_samples"),
             (9, 64, "n_mels"), (3, P - 1, "ld_x"), (5, P + 160, "max_length"), (11, 299, "ld_m"), (12, 80 * 300 - 1, "ld_u"),
             (15, need - 1, "workspace"), (14, None, "workspace"), (7, A + 4, "aligned"))
    for pos, bad, word in cases:
        args = list(good)
        args[pos] = bad
        assert lib.wsae_logmel(*args) == -1, (pos, bad)
        assert "wsae_logmel" in N.last_error() and word in N.last_error(), (pos, bad, N.last_error())
    assert lib.wsae_logmel(*good[:2], 0, *good[3:]) == 0  # no utterances: nothing is touched


def test_workspace_size():
    lib = N.lib()
    for bad in ((-1, 480000, 80), (1, 480001, 80), (1, 320, 80), (1, 480000, 64), (1 << 17, 480000, 80)):
        assert lib.wsae_logmel_workspace_bytes(*bad) == -1, bad
    big = lib.wsae_logmel_workspace_bytes(64, 480000, 128)
    assert big == 64 * 47 * 4 and big % 256 == 0  # one float per 64 frames: 3000 frames are 47 tiles
    sizes = [lib.wsae_logmel_workspace_bytes(n, 480000, 80) for n in (0, 1, 2, 16, 64, 65)]
    assert sizes[0] == 0 and sizes == sorted(sizes) and all(s % 256 == 0 for s in sizes)
    by_p = [lib.wsae_logmel_workspace_bytes(64, p, 80) for p in (480, 160 * 64, 160 * 65, 480000, 960000)]
    assert by_p == sorted(by_p) and by_p[0] > 0


def test_python_layer_errors_without_a_gpu():
    with pytest.raises(ValueError, match="n_mels must be 80 or 128, got 64"):
        LogMel(64)
    with pytest.raises(ValueError, match="n_samples must be a multiple of 160"):
        LogMel(80, n_samples=1000)
    with pytest.raises(ValueError, match="at least 480"):
        LogMel(80, n_samples=320)
    with pytest.raises(ValueError, match=r"filters must be \[201, 80\], got \(201, 128\)"):
        LogMel(80, filters=np.zeros((201, 128)))
    with pytest.raises(ValueError, match=r"basis must be \[400, 416\]"):
        LogMel(80, basis=np.zeros((400, 402), np.float32))
    with pytest.raises(N.WsaeError, match="cannot run on 'cpu'"):
        LogMel(80, device="cpu")
    with pytest.raises(N.WsaeError, match="cannot run on 'cpu'"):
        log_mel_spectrogram(torch.zeros(2, 480))
    with pytest.raises(ValueError, match="n_mels must be positive"):
        mel_filter_bank(0)


def test_frame_and_sample_arithmetic():
    assert frame_of_sample(0) == 0 and frame_of_sample(319) == 0 and frame_of_sample(320) == 1
    assert frame_of_sample(160, stride=1) == 1 and frame_of_sample(479999) == 1499
    assert sample_span_of_frames(0, 0) == (0, 320) and sample_span_of_frames(3, 7) == (960, 2560)
    assert sample_span_of_frames(0, 1499) == (0, 480000) and sample_span_of_frames(2, 2, stride=1) == (320, 480)
    first, last = 10, 24  # an event of RunTracker: frames first .. last
    start, stop = sample_span_of_frames(first, last)
    assert frame_of_sample(start) == first and frame_of_sample(stop - 1) == last and frame_of_sample(stop) == last + 1
    for bad in ((-1, 0), (3, 2)):
        with pytest.raises(ValueError):
            sample_span_of_frames(*bad)
    with pytest.raises(ValueError):
        frame_of_sample(-1)
