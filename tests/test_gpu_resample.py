"""The resampler on the MI355X: ``wsae_resample`` through the C ABI - junk tails behind every array, junk in ``x`` beyond
every length and between the rows, a sentinel in every output cell the kernel must not write - bit for bit against
``resample_exact`` (tests/resample_oracle.py) on the real tables, and the Python layer up to ``scripts/train.py``.  The
oracle itself is checked on the CPU in tests/test_resample.py."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import resample_oracle as RO
from test_token_alignment import tiny_whisper
from whisper_sae import _native as N
from whisper_sae.analysis.audio_extraction import read_wav, write_wav
from whisper_sae.data import AudioFrontEnd, LogMel, Resampler, compact_taps, resample, sinc_resample_kernel
from whisper_sae.data.audio import features_from_batch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TAIL = 5  # junk elements behind every array
TILE = N.RESAMPLE_TILE
GAP = {np.dtype(np.float32): np.float32(7.5), np.dtype(np.int16): np.int16(12345)}   # what an unwritten output cell holds
JUNK = {np.dtype(np.float32): np.float32(3.0e4), np.dtype(np.int16): np.int16(-12345)}
TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.int16): torch.int16}
ROOT = __import__("pathlib").Path(__file__).resolve().parents[1]
RATIOS = {"3/1": 48000, "441/160": 44100, "1/2": 8000, "441/640": 11025, "6/1": 96000, "1/1": 16000}


@functools.lru_cache(maxsize=None)
def tables(orig_freq: int, lowpass_filter_width: int = 6):
    """``(orig, new, taps, first, halo)`` of ``orig_freq -> 16000``; equal rates give the identity table."""
    if orig_freq == 16000:
        return 1, 1, np.ones((1, 1), np.float32), np.zeros(1, np.int32), 0
    kernel, width = sinc_resample_kernel(orig_freq, 16000, lowpass_filter_width)
    g = np.gcd(orig_freq, 16000)
    return (orig_freq // g, 16000 // g) + compact_taps(kernel, width)


def padded(a: np.ndarray, junk) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(a)).reshape(-1)
    return torch.cat((t, torch.full((TAIL,), junk, dtype=t.dtype))).to(DEV)


def cols_of(frames: int, orig: int, new: int) -> int:
    return (new * frames + orig - 1) // orig


def run_resample(x: np.ndarray, lengths, channels: int, table, out_dtype, *, ld_x=None, pad_y=9, extra_cols=3):
    """``wsae_resample`` on ``x [n_utt, S * channels]`` (float32 or int16, interleaved) -> ``(out [n_utt, out_cols], out_len)``
    as numpy.  Rows of ``x`` have stride ``ld_x`` with junk between, behind and beyond every length; ``out`` has row stride
    ``out_cols + pad_y`` and starts 4 bytes (int16: 2) behind a 64-byte boundary; every cell outside ``[:, :out_cols]``
    must keep its sentinel."""
    orig, new, taps, first, halo = table
    out_dtype = np.dtype(out_dtype)
    n_utt, width = x.shape
    S = width // channels
    ld_x = width if ld_x is None else ld_x
    rows = np.full((n_utt, ld_x), JUNK[x.dtype], dtype=x.dtype)
    rows[:, :width] = x
    for u, n in enumerate(lengths):
        rows[u, max(min(int(n), S), 0) * channels:] = JUNK[x.dtype]
    dx = padded(rows, JUNK[x.dtype])
    dl = padded(np.asarray(lengths, np.int32), 0x5a5a5a5)
    dt, df = padded(taps, 9.0e9), padded(first, 0x5a5a5a5)
    out_cols = cols_of(S, orig, new) + extra_cols
    ld_y = out_cols + pad_y
    store = torch.full((1 + n_utt * ld_y + TAIL,), GAP[out_dtype].item(), dtype=TORCH[out_dtype], device=DEV)
    assert store.data_ptr() % 64 == 0
    out = store[1:]  # (one element behind the boundary)
    olen = torch.full((n_utt + TAIL,), -77, dtype=torch.int32, device=DEV)
    code = {np.dtype(np.float32): N.DT_F32, np.dtype(np.int16): N.DT_I16}
    N.check(N.lib().wsae_resample(dx.data_ptr(), code[x.dtype], n_utt, ld_x, channels, dl.data_ptr(), S, orig, new, dt.data_ptr(),
                                  df.data_ptr(), taps.shape[1], halo, out.data_ptr(), code[out_dtype], ld_y, out_cols,
                                  olen.data_ptr(), torch.cuda.current_stream().cuda_stream), "wsae_resample")
    torch.cuda.synchronize()
    gap = GAP[out_dtype].item()
    assert store[0].item() == gap and bool((out[n_utt * ld_y:] == gap).all()) and bool((olen[n_utt:] == -77).all())
    full = out[:n_utt * ld_y].reshape(n_utt, ld_y).cpu().numpy()
    assert (full[:, out_cols:] == gap).all(), "cells at or beyond out_cols were written"
    return np.ascontiguousarray(full[:, :out_cols]), olen[:n_utt].cpu().numpy()


def waves(n_utt: int, S: int, channels: int, dtype, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.int16:
        return rng.integers(-32768, 32768, size=(n_utt, S * channels)).astype(np.int16)
    return (rng.standard_normal((n_utt, S * channels)) * 0.3).astype(np.float32)


def expect(x, lengths, channels, table, out_dtype, out_cols):
    """The oracle's rows, zero from ``out_len`` to ``out_cols``, and the lengths."""
    orig, new, taps, first, _ = table
    S = x.shape[1] // channels
    want = np.zeros((x.shape[0], out_cols), out_dtype)
    lens = []
    for u, n in enumerate(lengths):
        L = max(min(int(n), S), 0)
        y = RO.resample_exact(x[u], channels, L, orig, new, taps, first, out_dtype)
        want[u, :y.size] = y
        lens.append(y.size)
    return want, np.asarray(lens, np.int32)


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    view = np.uint32 if a.dtype == np.float32 else np.uint16
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(view), b.view(view))


def case_lengths(orig: int, new: int):
    return [0, 1, orig - 1, 4 * orig, 2 * TILE * orig // new + 7]


@pytest.mark.parametrize("channels", (1, 2, 3))
@pytest.mark.parametrize("out_dtype", (np.float32, np.int16))
@pytest.mark.parametrize("x_dtype", (np.float32, np.int16))
@pytest.mark.parametrize("ratio", tuple(RATIOS))
def test_every_cell_equals_the_oracle(ratio, x_dtype, out_dtype, channels):
    """Five utterances - empty, one frame, ``orig - 1``, a multiple of ``orig``, more than two tiles and a remainder - with
    ``ld_x`` beyond the frames and an output that starts off a 64-byte boundary.  Routes: one-phase table (3/1, 6/1, 1/1)
    and table in LDS (the others); 16-byte loads (1 and 2 channels: ``ld_x`` keeps the frames on the boundaries) and loads
    by element (3 channels)."""
    table = tables(RATIOS[ratio])
    orig, new = table[:2]
    lengths = case_lengths(orig, new)
    S = max(lengths)
    x = waves(5, S, channels, x_dtype, seed=len(ratio) + channels)
    got, got_len = run_resample(x, lengths, channels, table, out_dtype, ld_x=S * channels + 4 * channels)
    want, want_len = expect(x, lengths, channels, table, out_dtype, got.shape[1])
    assert np.array_equal(got_len, want_len) and want_len.tolist() == [cols_of(n, orig, new) for n in lengths]
    assert same_bits(got, want)
    assert (got[0] == 0).all() and (got[1, want_len[1]:] == 0).all()


def test_independence_of_row_batch_and_alignment():
    """Utterance 4 of a stereo int16 batch whose odd ``ld_x`` puts the rows off the frame boundaries (loads by element),
    alone as row 0 of another batch (16-byte loads), and at a third ``ld_x``: the same bits."""
    table = tables(44100)
    orig, new = table[:2]
    lengths = case_lengths(orig, new)
    S = max(lengths)
    x = waves(5, S, 2, np.int16, seed=5)
    batch, _ = run_resample(x, lengths, 2, table, np.float32, ld_x=2 * S + 3)
    alone, n1 = run_resample(x[4:], lengths[4:], 2, table, np.float32)
    other, _ = run_resample(np.concatenate((x[4:], x[:1])), [lengths[4], 17], 2, table, np.float32, ld_x=2 * S + 10, pad_y=16)
    want, _ = expect(x[4:], lengths[4:], 2, table, np.float32, alone.shape[1])
    assert same_bits(alone, want) and same_bits(batch[4:], alone) and same_bits(other[:1], alone)
    assert n1.tolist() == [cols_of(S, orig, new)]


def test_int16_output_saturates_on_both_sides():
    table = tables(48000)
    S = 3 * 700
    square = np.where((np.arange(S) // 150) % 2 == 0, 32767, -32768).astype(np.int16)[None, :]
    want, _ = expect(square, [S], 1, table, np.int16, cols_of(S, 3, 1) + 3)
    assert want.min() == -32768 and want.max() == 32767  # the overshoot of the filter hits the clamp
    wide, _ = expect(square, [S], 1, table, np.float32, cols_of(S, 3, 1) + 3)
    assert wide.max() > 1.0 and wide.min() < -1.0
    got, _ = run_resample(square, [S], 1, table, np.int16)
    assert same_bits(got, want)


def test_a_table_too_large_for_lds_and_a_shrunk_tile():
    """The two routes the real tables above do not take.  ``lowpass_filter_width = 16`` at 441/640: a table of about 85 KB,
    which is read through the cache.  ``orig = 1021``, ``new = 2`` with a made-up table of 40 taps: the span of a whole tile
    would be half a million samples, so a workgroup owns 16 outputs."""
    big = tables(11025, 16)
    assert 4 * big[2].shape[1] * (big[1] | 1) > N.RESAMPLE_LDS_BYTES
    lengths = [0, 1, 440, 441 * 3, 2 * TILE * 441 // 640 + 7]
    x = waves(5, max(lengths), 2, np.float32, seed=16)
    got, got_len = run_resample(x, lengths, 2, big, np.float32, ld_x=2 * max(lengths) + 8)
    want, want_len = expect(x, lengths, 2, big, np.float32, got.shape[1])
    assert np.array_equal(got_len, want_len) and same_bits(got, want)

    rng = np.random.default_rng(1021)
    orig, new, n_taps, halo = 1021, 2, 40, 30
    made_up = (orig, new, rng.standard_normal((new, n_taps)).astype(np.float32) / 8,
               np.array([-halo, orig + halo - n_taps], np.int32), halo)
    lengths = [0, 1, orig - 1, 2 * orig, 40 * orig + 7]  # 81 outputs: five tiles of 16 and one more
    x = waves(5, max(lengths), 1, np.int16, seed=2)
    got, got_len = run_resample(x, lengths, 1, made_up, np.int16)
    want, want_len = expect(x, lengths, 1, made_up, np.int16, got.shape[1])
    assert np.array_equal(got_len, want_len) and same_bits(got, want)


def test_a_broken_halo_promise_is_clamped():
    """``first[0] = -halo - 5``: the call completes, every phase but 0 equals the oracle and the sentinels are intact (the
    harness checks them).  Phase 0's values are unspecified and not compared."""
    orig, new, taps, first, halo = tables(44100)
    broken = first.copy()
    broken[0] = -halo - 5
    lengths = [3 * orig, TILE * orig // new + 50]
    x = waves(2, max(lengths), 1, np.float32, seed=8)
    got, got_len = run_resample(x, lengths, 1, (orig, new, taps, broken, halo), np.float32)
    want, want_len = expect(x, lengths, 1, (orig, new, taps, first, halo), np.float32, got.shape[1])
    keep = np.arange(got.shape[1]) % new != 0
    assert np.array_equal(got_len, want_len) and same_bits(np.ascontiguousarray(got[:, keep]), np.ascontiguousarray(want[:, keep]))
    assert np.isfinite(got).all()


# ---- the Python layer -------------------------------------------------------------------------------------------------------
def test_resampler_on_ragged_stereo_lists_views_and_errors():
    table = tables(44100)
    rng = np.random.default_rng(7)
    sizes = (5000, 441, 1)
    clips = [rng.integers(-32768, 32768, size=(n, 2)).astype(np.int16) for n in sizes]
    rs = Resampler(44100, device=DEV)
    y, n = rs([torch.from_numpy(c).to(DEV) for c in clips])
    cols = cols_of(max(sizes), 441, 160)
    assert y.shape == (3, cols) and y.dtype == torch.float32 and n.dtype == torch.int32 and n.device == y.device
    x = np.zeros((3, max(sizes) * 2), np.int16)
    for u, c in enumerate(clips):
        x[u, :c.size] = c.reshape(-1)
    want, want_len = expect(x, sizes, 2, table, np.float32, cols)
    assert np.array_equal(n.cpu().numpy(), want_len) and same_bits(y.cpu().numpy(), want)
    batch = torch.from_numpy(x).to(DEV).reshape(3, -1, 2)
    assert torch.equal(rs(batch, list(sizes))[0], y) and torch.equal(resample(batch, 44100, lengths=list(sizes))[0], y)
    # out= with gaps between the rows, int16 on the way out
    store = torch.full((3, cols + 11), 77, dtype=torch.int16, device=DEV)
    got, _ = rs(batch, list(sizes), out=store[:, 3:3 + cols])
    want16, _ = expect(x, sizes, 2, table, np.int16, cols)
    assert got.data_ptr() == store[:, 3:].data_ptr() and same_bits(got.cpu().numpy(), want16)
    assert bool((store[:, :3] == 77).all()) and bool((store[:, 3 + cols:] == 77).all())
    assert torch.equal(rs(batch, list(sizes), out_dtype=torch.int16)[0], got)
    # equal rates: the downmix and the conversion alone
    mixed, m = Resampler(16000, device=DEV)(batch[:, :100], out_dtype=torch.int16)
    plain = RO.downmix(x[0, :200], 2)
    assert m.tolist() == [100] * 3 and mixed[0].tolist() == np.clip(np.rint(plain * np.float32(32768)), -32768, 32767).tolist()
    empty, zero = rs(batch[:, :0])
    assert empty.shape == (3, 0) and zero.tolist() == [0, 0, 0]
    with pytest.raises(N.WsaeError, match="cannot run on 'cpu'"):
        rs(torch.zeros(2, 480))
    with pytest.raises(ValueError, match=r"waveforms must be \[n_utt, samples\]"):
        rs(torch.zeros(2, 3, 480, 2, device=DEV))
    with pytest.raises(ValueError, match="float32 or int16, got torch.float64"):
        rs(torch.zeros(2, 480, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError, match="9 channels"):
        rs(torch.zeros(2, 480, 9, device=DEV))
    with pytest.raises(ValueError, match="lengths has 3 entries for 2 utterances"):
        rs(torch.zeros(2, 480, device=DEV), [1, 2, 3])
    with pytest.raises(ValueError, match="waveform 1 must be a 1-D or"):
        rs([torch.zeros(4, device=DEV), torch.zeros(2, 2, 2, device=DEV)])
    with pytest.raises(ValueError, match="the channels differ"):
        rs([torch.zeros(4, 2, device=DEV), torch.zeros(4, device=DEV)])
    with pytest.raises(ValueError, match=r"out must be float32 or int16 \[2, 160\]"):
        rs(torch.zeros(2, 441, device=DEV), out=torch.zeros(2, 161, device=DEV))
    with pytest.raises(ValueError, match="unit stride along the samples"):
        rs(torch.zeros(2, 441, device=DEV), out=torch.zeros(2, 320, device=DEV)[:, ::2])


@pytest.fixture(scope="module")
def stereo_48k():
    """Two stereo clips at 48 kHz, float32, and the oracle's 16 kHz signal of each."""
    table = tables(48000)
    S = 3 * 4000
    rng = np.random.default_rng(48)
    x = (rng.standard_normal((2, S * 2)) * 0.2).astype(np.float32)
    lengths = [S, 7001]
    y, n = expect(x, lengths, 2, table, np.float32, cols_of(S, 3, 1))
    return x, lengths, y, n


def test_audio_front_end_is_logmel_of_the_resampled_signal(stereo_48k):
    x, lengths, y, n = stereo_48k
    P = 16000  # 100 mel frames: the tiny model's 50 positions
    fe = AudioFrontEnd(48000, 80, DEV, n_samples=P)
    mel = LogMel(80, DEV, n_samples=P)
    want = mel(torch.from_numpy(y).to(DEV), torch.from_numpy(n))
    batch = torch.from_numpy(x).to(DEV).reshape(2, -1, 2)
    assert torch.equal(fe(batch, lengths), want)
    assert torch.equal(features_from_batch(fe, (batch, torch.tensor(lengths))), want)
    assert torch.equal(features_from_batch(fe, want), want)  # mel features pass through an AudioFrontEnd too
    # 16 kHz mono: the LogMel alone
    mono = torch.from_numpy(y).to(DEV)
    assert torch.equal(AudioFrontEnd(16000, 80, DEV, n_samples=P)(mono, torch.from_numpy(n)), want)
    # a plain LogMel still passes every 3-D tensor through
    assert features_from_batch(mel, batch) is batch and features_from_batch(mel, (batch, lengths)) is batch


def test_cli_from_wav_files_equals_audio_from_the_resampled_tensor(tmp_path):
    """scripts/train.py --wav on two 8 kHz stereo files against --audio on the oracle's 16 kHz signal: the same cache."""
    import importlib.util
    import yaml
    spec = importlib.util.spec_from_file_location("wsae_train_cli_wav", ROOT / "scripts" / "train.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    rng = np.random.default_rng(80)
    sizes = (7000, 5001)
    paths = []
    for i, s in enumerate(sizes):
        write_wav(tmp_path / f"{i}.wav", rng.integers(-20000, 20000, size=(s, 2)).astype(np.int16), 8000, channels=2)
        paths.append(str(tmp_path / f"{i}.wav"))
    clips = [read_wav(p, return_rate=True, mono=False) for p in paths]
    assert all(rate == 8000 and tuple(w.shape) == (s, 2) for (w, rate), s in zip(clips, sizes))
    x = np.zeros((2, max(sizes) * 2), np.float32)
    for u, (w, _) in enumerate(clips):
        x[u, :w.numel()] = w.reshape(-1).numpy()
    y, n = expect(x, sizes, 2, tables(8000), np.float32, 2 * max(sizes))
    torch.save({"waveforms": torch.from_numpy(y), "lengths": torch.from_numpy(n)}, tmp_path / "audio.pt")
    torch.save({"waveforms": torch.from_numpy(x).reshape(2, -1, 2), "lengths": torch.tensor(sizes), "sample_rate": 8000},
               tmp_path / "audio8k.pt")
    caches = []
    for name, flags in (("wav", ["--wav"] + paths), ("audio", ["--audio", str(tmp_path / "audio.pt")]),
                        ("audio8k", ["--audio", str(tmp_path / "audio8k.pt")])):
        cfg = {"whisper": {"model_name": "local/tiny-random", "hidden_dim": 64, "num_encoder_layers": 2, "num_decoder_layers": 2},
               "sae": {"expansion_factor": 4, "k": 8, "dead_feature_resample": False},
               "training": {"batch_size": 50, "epochs": 1, "use_amp": False, "num_workers": 0, "warmup_steps": 0, "checkpoint_every": 1},
               "data": {"cache_dir": str(tmp_path / name), "max_samples": 2}, "wandb": {"enabled": False},
               "encoder_layers": [1], "decoder_layers": [], "output_dir": str(tmp_path / "out"), "experiment_name": name}
        (tmp_path / f"{name}.yaml").write_text(yaml.safe_dump(cfg))
        cli.main(["--config", str(tmp_path / f"{name}.yaml"), "--no-wandb", "--device", DEV, "--mel-frames", "100", "--extract-only"]
                 + flags, whisper_model=tiny_whisper(0))
        caches.append(torch.load(tmp_path / name / "features" / "tiny-random_encoder_layer1.pt", weights_only=True))
    assert tuple(caches[0].shape) == (100, 64) and torch.equal(caches[0], caches[1]) and torch.equal(caches[2], caches[1])
    with pytest.raises(SystemExit, match="exceed --mel-frames 50 x 160"):
        cli.wav_batches(paths, 80, torch.device(DEV), 50 * 160, 50)
