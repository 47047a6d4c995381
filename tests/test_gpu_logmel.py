"""The log-mel front end on the MI355X: ``wsae_logmel`` through the C ABI - junk tails behind every array, junk in the
gaps of the output, a poisoned workspace - exactly on integer data, within the derived per-cell bound of the float64 mirror
(tests/logmel_oracle.py) on real tables, and the Python layer up to ``scripts/train.py``.  The oracles themselves are
checked against the installed extractor on the CPU in tests/test_logmel.py."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import logmel_oracle as LO
from test_token_alignment import tiny_whisper
from whisper_sae import _native as N
from whisper_sae.data import ActivationRing, LogMel, dft_basis, extract_and_cache_features, log_mel_spectrogram, mel_filter_bank

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TAIL = 5       # junk elements behind every array
GAP = 7.5      # what the output holds wherever the kernel must not write
ROOT = __import__("pathlib").Path(__file__).resolve().parents[1]


def padded(a: np.ndarray, junk) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(a)).reshape(-1)
    return torch.cat((t, torch.full((TAIL,), junk, dtype=t.dtype))).to(DEV)


def run_logmel(x: np.ndarray, lengths, P: int, basis: np.ndarray, filt: np.ndarray, *, ld_x=None, ld_m=None, power=True,
               junk_x=None):
    """``wsae_logmel`` on ``x [n_utt, S]`` (float32 or int16) -> ``(out, mel_power)`` as numpy ``[n_utt, n_mels, T]``.
    Rows of ``x`` are laid out with stride ``ld_x`` and junk between and behind them; ``out`` / ``mel_power`` have row stride
    ``ld_m`` and must keep ``GAP`` in every cell outside ``[:, :, :T]``."""
    n_utt, s = x.shape
    n_mels, T = filt.shape[1], P // 160
    ld_x = s if ld_x is None else ld_x
    ld_m = T if ld_m is None else ld_m
    ld_u = n_mels * ld_m + 16
    junk = (np.float32(3.0e4) if x.dtype == np.float32 else np.int16(-12345)) if junk_x is None else junk_x
    rows = np.full((n_utt, ld_x), junk, dtype=x.dtype)
    rows[:, :s] = x
    for u, n in enumerate(lengths):  # nothing beyond the length is read: junk there too
        rows[u, max(min(int(n), s), 0):] = junk
    dx = padded(rows, junk)
    code = N.DT_F32 if x.dtype == np.float32 else N.DT_I16
    dl = padded(np.asarray(lengths, np.int32), 0x5a5a5a5)
    db, df = padded(basis.astype(np.float32), 9.0e9), padded(filt.astype(np.float32), 9.0e9)
    out = torch.full((n_utt * ld_u + TAIL,), GAP, dtype=torch.float32, device=DEV)
    pw = torch.full((n_utt * ld_u + TAIL,), GAP, dtype=torch.float32, device=DEV) if power else None
    lib = N.lib()
    need = lib.wsae_logmel_workspace_bytes(n_utt, P, n_mels)
    assert need > 0
    ws = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device=DEV)  # (NaNs on entry)
    N.check(lib.wsae_logmel(dx.data_ptr(), code, n_utt, ld_x, dl.data_ptr(), s, P, db.data_ptr(), df.data_ptr(), n_mels,
                            out.data_ptr(), ld_m, ld_u, N.ptr(pw), ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream),
            "wsae_logmel")
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xFF).all())
    got = []
    for t in (out, pw):
        if t is None:
            got.append(None)
            continue
        assert bool((t[n_utt * ld_u:] == GAP).all())
        full = t[:n_utt * ld_u].reshape(n_utt, ld_u).cpu().numpy()
        assert (full[:, n_mels * ld_m:] == GAP).all()
        cells = full[:, :n_mels * ld_m].reshape(n_utt, n_mels, ld_m)
        assert (cells[:, :, T:] == GAP).all(), "the gaps behind the frames were written"
        got.append(np.ascontiguousarray(cells[:, :, :T]))
    return got


# ---- exact, nothing excluded ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def int_tables():
    return {n: LO.integer_tables(n) for n in (80, 128)}


def integer_wave(n_utt, P, halves, seed):
    rng = np.random.default_rng(seed)
    if halves:  # multiples of 1/2 in -1 .. 1/2: exactly int16 * 2^-15
        return rng.integers(-2, 2, size=(n_utt, P)).astype(np.float32) / 2
    return rng.integers(-1, 2, size=(n_utt, P)).astype(np.float32)


@pytest.mark.parametrize("as_int16", (False, True))
@pytest.mark.parametrize("T", (3, 64, 65))
def test_mel_power_is_exact_on_integer_data(int_tables, T, as_int16):
    """One utterance: both reflections in one tile (T = 3), a full tile, a ragged second tile.  An integer basis that
    differs in every column and between the cosine and sine halves: a swapped operand map or row cannot pass."""
    P = 160 * T
    basis, filt = int_tables[80]
    x = integer_wave(1, P, as_int16, seed=T)
    want = LO.integer_mel_power(x[0], basis, filt, P).astype(np.float32)
    xin = (x * 32768).astype(np.int16) if as_int16 else x
    _, power = run_logmel(xin, [P], P, basis, filt)
    assert np.array_equal(power[0].view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("n_mels", (80, 128))
@pytest.mark.parametrize("as_int16", (False, True))
def test_mel_power_is_exact_on_a_ragged_batch(int_tables, n_mels, as_int16):
    """(3, 130): lengths P, 1000 and 0, ld_x > P, three tiles with a ragged last one, ld_m > T."""
    T, n_utt = 130, 3
    P = 160 * T
    basis, filt = int_tables[n_mels]
    x = integer_wave(n_utt, P, as_int16, seed=n_mels)
    lengths = [P, 1000, 0]
    xin = (x * 32768).astype(np.int16) if as_int16 else x
    out, power = run_logmel(xin, lengths, P, basis, filt, ld_x=P + 37, ld_m=T + 14)
    for u, n in enumerate(lengths):
        want = LO.integer_mel_power(x[u, :n], basis, filt, P).astype(np.float32)
        assert np.array_equal(power[u].view(np.uint32), want.view(np.uint32)), u
    assert (power[2] == 0).all() and (out[2] == -1.5).all()


# ---- against the mirror, real tables ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def real_tables():
    return dft_basis(), {n: mel_filter_bank(n).astype(np.float32) for n in (80, 128)}


@pytest.mark.parametrize("T,n_mels", ((65, 80), (300, 128)))
def test_every_cell_is_within_the_mirrors_bound(real_tables, T, n_mels):
    """The three signals as float32 and full-scale noise as int16, one batch; every cell of ``out`` and of ``mel_power``
    within the bound ``mirror`` derives for it - none left out."""
    P = 160 * T
    basis, filts = real_tables
    sig = LO.signals(P, seed=T)
    x = np.stack([sig[name].astype(np.float32) for name in ("noise", "tone_silence", "am_tone")])
    out, power = run_logmel(x, [P] * 3, P, basis, filts[n_mels], ld_m=T + 3)
    pcm = np.random.default_rng(T).integers(-32768, 32768, size=(1, P)).astype(np.int16)
    out16, power16 = run_logmel(pcm, [P], P, basis, filts[n_mels])
    rows = [(x[u], out[u], power[u]) for u in range(3)] + [(pcm[0].astype(np.float32) / np.float32(32768), out16[0], power16[0])]
    for u, (wave, got, got_p) in enumerate(rows):
        want, e_out, mel, e_mel = LO.mirror(wave, basis, filts[n_mels], P)
        ratio = np.abs(got - want) / e_out
        ratio_p = np.abs(got_p - mel) / np.maximum(e_mel, 1e-300)
        print(f"signal {u}: max |out - mirror| = {np.abs(got - want).max():.3e}, max over cells of |delta| / E = {ratio.max():.3f}; "
              f"mel_power: {np.nanmax(np.where(e_mel > 0, ratio_p, 0)):.3f}")
        assert (np.abs(got - want) <= e_out).all(), u
        assert (np.abs(got_p - mel) <= e_mel).all(), u


def test_an_all_zero_utterance_is_exactly_the_floor(real_tables):
    basis, filts = real_tables
    P = 160 * 70
    out, power = run_logmel(np.zeros((2, P), np.float32), [P, 0], P, basis, filts[80])
    assert (power == 0).all() and (out == np.float32(-1.5)).all()  # (-10 + 4) / 4
    out16, _ = run_logmel(np.zeros((1, P), np.int16), [P], P, basis, filts[128], power=False)
    assert (out16 == np.float32(-1.5)).all()


def test_independence_of_batch_position_and_repetition(real_tables):
    """An utterance alone and as row 2 of a batch of three; two calls; ``mel_power`` requested or not; 16-byte
    write-through stores (ld_m a multiple of 16) and 4-byte stores (ld_m = 130)."""
    basis, filts = real_tables
    T = 130
    P = 160 * T
    sig = LO.signals(P, seed=9)
    x = np.stack([sig[name].astype(np.float32) for name in ("noise", "tone_silence", "am_tone")])
    lengths = [P, P - 777, 12345]
    out3, power3 = run_logmel(x, lengths, P, basis, filts[80], ld_x=P + 3, ld_m=T + 14)  # (ld_m = 144: the wide stores)
    again, power_again = run_logmel(x, lengths, P, basis, filts[80], ld_x=P + 3, ld_m=T + 14)
    assert np.array_equal(out3.view(np.uint32), again.view(np.uint32))
    assert np.array_equal(power3.view(np.uint32), power_again.view(np.uint32))
    alone, power1 = run_logmel(x[2:, :12345], lengths[2:], P, basis, filts[80])  # (ld_m = 130: the narrow stores)
    assert np.array_equal(alone[0].view(np.uint32), out3[2].view(np.uint32))
    assert np.array_equal(power1[0].view(np.uint32), power3[2].view(np.uint32))
    quiet, _ = run_logmel(x, lengths, P, basis, filts[80], power=False)
    assert np.array_equal(quiet.view(np.uint32), out3.view(np.uint32))


# ---- the Python layer -------------------------------------------------------------------------------------------------------
def test_logmel_on_ragged_lists_views_and_errors():
    P = 16000
    fe = LogMel(80, DEV, n_samples=P)
    g = torch.Generator().manual_seed(1)
    waves = [torch.randn(n, generator=g).mul(0.1).to(DEV) for n in (16000, 9000, 1)]
    batch = torch.zeros(3, P, device=DEV)
    for i, w in enumerate(waves):
        batch[i, :w.numel()] = w
    want = fe(batch, [16000, 9000, 1])
    assert want.shape == (3, 80, 100) and want.dtype == torch.float32 and want.device == batch.device
    assert torch.equal(fe(waves), want)
    assert torch.equal(fe(batch), want)  # (the zeros behind a length are what the length stands for)
    assert torch.equal(log_mel_spectrogram(waves, n_samples=P), want)
    assert torch.equal(fe(batch[:, :9000], [9000, 9000, 1])[1:], want[1:])  # missing columns count as zeros
    pcm = (batch * 32768).round().clamp(-32768, 32767).to(torch.int16)
    assert torch.equal(fe(pcm), fe(pcm.float() / 32768))
    # out= with gaps between the rows, and the linear mel next to it
    store = torch.full((3, 80, 128), GAP, device=DEV)
    got, power = fe(batch, [16000, 9000, 1], out=store[:, :, :100], return_power=True)
    assert got.data_ptr() == store.data_ptr() and torch.equal(store[:, :, :100], want) and bool((store[:, :, 100:] == GAP).all())
    assert power.shape == want.shape and bool((power >= 0).all())
    mel = torch.log10(power.clamp(min=1e-10))
    ref = (torch.maximum(mel, mel.amax(dim=(1, 2), keepdim=True) - 8.0) + 4.0) / 4.0
    assert float((ref - want).abs().max()) < 1e-5  # (torch's log10 against the kernel's: a sanity check, not the contract)
    with pytest.raises(N.WsaeError, match="cannot run on 'cpu'"):
        fe(torch.zeros(2, 480))
    with pytest.raises(N.WsaeError, match="cannot run on 'cpu'"):
        fe([torch.zeros(480)])
    with pytest.raises(ValueError, match=r"waveforms must be \[n_utt, samples\]"):
        fe(torch.zeros(2, 3, 480, device=DEV))
    with pytest.raises(ValueError, match="float32 or int16, got torch.float64"):
        fe(torch.zeros(2, 480, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError, match="16001 samples"):
        fe(torch.zeros(1, 16001, device=DEV))
    with pytest.raises(ValueError, match="lengths has 3 entries for 2 utterances"):
        fe(torch.zeros(2, 480, device=DEV), [1, 2, 3])
    with pytest.raises(ValueError, match="waveform 1 must be a 1-D tensor"):
        fe([torch.zeros(4, device=DEV), torch.zeros(2, 2, device=DEV)])
    with pytest.raises(ValueError, match=r"out must be float32 \[2, 80, 100\]"):
        fe(torch.zeros(2, 480, device=DEV), out=torch.zeros(2, 80, 99, device=DEV))
    # the C entry point refuses a float32 x that is not aligned to its element, before anything is launched
    x, n, out = torch.zeros(P + 1, device=DEV), torch.full((1,), P, dtype=torch.int32, device=DEV), torch.empty(1, 80, 100, device=DEV)
    need = N.lib().wsae_logmel_workspace_bytes(1, P, 80)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    with pytest.raises(N.WsaeError, match="aligned to"):
        N.check(N.lib().wsae_logmel(x.data_ptr() + 2, N.DT_F32, 1, P, n.data_ptr(), P, P, fe.basis.data_ptr(), fe.filters.data_ptr(), 80,
                                    out.data_ptr(), 100, 8000, None, ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream),
                "wsae_logmel")


def test_extraction_from_waveforms_equals_extraction_from_their_mel():
    model = tiny_whisper(0).to(DEV)
    P = 16000  # 100 mel frames: the tiny model's 50 positions
    fe = LogMel(80, DEV, n_samples=P)
    g = torch.Generator().manual_seed(2)
    wave = torch.randn(4, P, generator=g).mul(0.2).to(DEV)
    lengths = torch.tensor([P, 12000, 8000, 100], dtype=torch.int32)
    rings = [ActivationRing(4 * 50, 64, device=DEV, dtype=torch.float32) for _ in range(3)]
    info = extract_and_cache_features(model, None, [(wave[:2], lengths[:2]), (wave[2:], lengths[2:])], None, [1], [], device=DEV,
                                      rings={("encoder", 1): rings[0]}, show_progress=False, frontend=fe)
    mel = fe(wave, lengths)
    extract_and_cache_features(model, None, [mel[:2], mel[2:]], None, [1], [], device=DEV, rings={("encoder", 1): rings[1]},
                               show_progress=False)
    extract_and_cache_features(model, None, [mel[:2], mel[2:]], None, [1], [], device=DEV, rings={("encoder", 1): rings[2]},
                               show_progress=False, frontend=fe)  # 3-D batches pass through
    assert info["num_samples"] == 4 and len(rings[0]) == 200
    assert torch.equal(rings[0].data, rings[1].data) and torch.equal(rings[2].data, rings[1].data)
    assert bool(torch.isfinite(rings[0].data).all())


def test_aligned_batches_from_waveforms_equal_those_from_their_mel():
    from whisper_sae.analysis import aligned_batches
    model = tiny_whisper(0).to(DEV)
    fe = LogMel(80, DEV, n_samples=16000)
    wave = torch.randn(2, 16000, generator=torch.Generator().manual_seed(4)).mul(0.2).to(DEV)
    lengths = torch.tensor([16000, 11000], dtype=torch.int32)
    ids = torch.tensor([[1, 3, 17, 33, 150, 2], [1, 3, 8, 9, 2, 0]])
    rest = (ids, [6, 5], [100, 68])
    want = list(aligned_batches(model, [(fe(wave, lengths),) + rest], encoder_layer=1, n_prefix=2, device=DEV))
    silenced = wave * (torch.arange(16000, device=DEV) < lengths.to(DEV)[:, None])  # a 2-D item has no lengths: zeros stand for them
    for first in (silenced, (wave, lengths)):
        got = list(aligned_batches(model, [(first,) + rest], encoder_layer=1, n_prefix=2, device=DEV, frontend=fe))
        for a, b in zip(got[0], want[0]):
            assert torch.equal(a, b)
    assert want[0][0].shape == (2, 50, 64) and bool(want[0][2].any())


def test_cli_flows_from_synthetic_audio(tmp_path):
    """scripts/train.py --synthetic-audio 2: extract-only, training from the cache it wrote, and --stream-to-ring."""
    import importlib.util
    import yaml
    spec = importlib.util.spec_from_file_location("wsae_train_cli_audio", ROOT / "scripts" / "train.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    cfg = {"whisper": {"model_name": "local/tiny-random", "hidden_dim": 64, "num_encoder_layers": 2, "num_decoder_layers": 2},
           "sae": {"expansion_factor": 4, "k": 8, "dead_feature_resample": False},
           "training": {"batch_size": 50, "epochs": 1, "use_amp": False, "num_workers": 0, "warmup_steps": 0, "checkpoint_every": 1},
           "data": {"cache_dir": str(tmp_path / "cache"), "max_samples": 2}, "wandb": {"enabled": False},
           "encoder_layers": [1], "decoder_layers": [], "output_dir": str(tmp_path / "out"), "experiment_name": "audio"}
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
    base = ["--config", str(tmp_path / "cfg.yaml"), "--no-wandb", "--device", DEV, "--mel-frames", "100"]
    cli.main(base + ["--synthetic-audio", "2", "--extract-only"], whisper_model=tiny_whisper(0))
    feats = tmp_path / "cache" / "features" / "tiny-random_encoder_layer1.pt"
    assert tuple(torch.load(feats, weights_only=True).shape) == (100, 64)
    cli.main(base)  # trains from the cache
    assert (tmp_path / "out" / "audio_encoder_layer1" / "sae_final.pt").exists()
    cfg["data"]["cache_dir"], cfg["experiment_name"] = str(tmp_path / "cache2"), "audioring"
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
    wave, lengths = cli.synthetic_audio(2, 16000, 7)
    torch.save({"waveforms": (wave * 32767).to(torch.int16), "lengths": lengths}, tmp_path / "audio.pt")
    cli.main(base + ["--audio", str(tmp_path / "audio.pt"), "--stream-to-ring"], whisper_model=tiny_whisper(0))
    assert (tmp_path / "out" / "audioring_encoder_layer1" / "sae_final.pt").exists()
    assert not list((tmp_path / "cache2" / "features").glob("*.pt"))


def test_a_train_step_does_not_notice_a_logmel_call(tmp_path):
    from whisper_sae.config import TrainingConfig
    from whisper_sae.sae.model import TopKSAE
    from whisper_sae.sae.training import SAETrainer

    def step(intrude: bool):
        torch.manual_seed(11)
        sae = TopKSAE(64, 512, k=8)
        tr = SAETrainer(sae, TrainingConfig(batch_size=128, learning_rate=3e-3, warmup_steps=0, use_amp=False, num_workers=0),
                        device=torch.device(DEV), run_dir=tmp_path / ("a" if intrude else "b"))
        x = torch.randn(128, 64, generator=torch.Generator().manual_seed(12))
        tr.train_step(x)
        if intrude:
            LogMel(80, DEV, n_samples=16000)(torch.randn(2, 16000, device=DEV))
        met = tr.train_step(x)
        return met.loss, {k: v.detach().cpu().clone() for k, v in sae.state_dict().items()}

    loss_a, state_a = step(True)
    loss_b, state_b = step(False)
    assert loss_a == loss_b
    for name in state_b:
        assert torch.equal(state_a[name], state_b[name]), name
