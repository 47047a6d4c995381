"""Token alignment without a GPU: the oracle of tests/align_oracle.py against the formulation of the installed
``transformers`` (the cost evaluated in float64 within a derived bound, the DTW index for index on the same float32
matrix, with and without ties), the per-frame and per-token tables against a direct reading of the path, the argument
errors of the two entry points, and ``CrossAttentionTap`` on a tiny Whisper."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import align_oracle as AO
from whisper_sae import _native as N
from whisper_sae.analysis import CrossAttentionTap, align_tokens, alignment_heads
from whisper_sae.sae.hooks import run_whisper_transcript

SHAPES = ((3, 9, 50), (2, 5, 23), (4, 17, 70))  # (heads, tokens, frames)


def tiny_whisper(seed: int = 0):
    from transformers import WhisperConfig, WhisperForConditionalGeneration
    cfg = WhisperConfig(vocab_size=200, num_mel_bins=80, encoder_layers=2, decoder_layers=2, encoder_attention_heads=2,
                        decoder_attention_heads=2, encoder_ffn_dim=128, decoder_ffn_dim=128, d_model=64,
                        max_source_positions=50, max_target_positions=16, decoder_start_token_id=1, pad_token_id=0,
                        bos_token_id=1, eos_token_id=2)
    torch.manual_seed(seed)
    return WhisperForConditionalGeneration(cfg).eval()


def library(name):
    import transformers.models.whisper.generation_whisper as G
    fn = getattr(G, name, None)
    if fn is None:
        pytest.skip(f"this transformers has no {name}")
    return fn


@pytest.fixture(scope="module")
def cases():
    """Per shape: the weights, and the oracle's cost at width 7 - computed once."""
    out = []
    for seed, (h, n, k) in enumerate(SHAPES):
        w = AO.attention(h, n, k, seed=seed)
        c, bad = AO.cost_one(w, n, k, 7)
        assert bad == 0
        out.append((w, c))
    return out


# ---- the cost -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_oracle_cost_matches_the_library_formulation_in_float64(cases, case):
    """|delta| <= 2^-22 sqrt(n_tok): a z-score is at most sqrt(n_tok) in magnitude (one value against n_tok - 1 equal
    ones), the oracle rounds it to float32 once and the head mean once more, 2^-24 relative each; margin 2."""
    median_filter = library("_median_filter")
    w, got = cases[case]
    h, n, k = SHAPES[case]
    x = torch.from_numpy(w).double()
    std, mean = torch.std_mean(x, dim=-2, keepdim=True, unbiased=False)
    want = -median_filter((x - mean) / std, 7).mean(dim=0)
    delta = np.abs(got[:n, :k].astype(np.float64) - want.numpy()).max()
    bound = 2.0 ** -22 * np.sqrt(n)
    print(f"shape {SHAPES[case]}: max |delta| = {delta:.3e}, bound {bound:.3e}")
    assert delta <= bound


def test_oracle_cost_fills_and_counts():
    w = AO.attention(2, 6, 20, seed=5)
    padded = np.full((3, 2, 8, 24), 7.0, np.float32)
    padded[:, :, :6, :20] = w
    padded[1, 1, 2, 3] = np.nan
    padded[1, 0, 5, 19] = np.inf
    cost, n_bad, status = AO.cost(padded, [6, 6, 0], [20, 20, 20], 3)
    assert n_bad.tolist() == [0, 2, -1] and status.tolist() == [2, 2]
    assert np.isfinite(cost[0, :6, :20]).all() and np.isinf(cost[0, 6:]).all() and np.isinf(cost[0, :, 20:]).all()
    assert np.isinf(cost[1:]).all()
    assert np.array_equal(cost[0, :6, :20], AO.cost_one(w, 6, 20, 3)[0])  # the junk behind the sizes is never read
    assert AO.cost_one(w, 6, 3, 7)[1] == -1 and AO.cost_one(w, 6, 4, 7)[1] == 0  # n_frames <= width // 2 is invalid


def test_constant_column_scores_zero():
    w = AO.attention(1, 5, 12, seed=2)
    w[0, :, 4] = 0.25
    c, bad = AO.cost_one(w, 5, 12, 1)
    assert bad == 0 and (c[:5, 4] == 0).all() and not np.signbit(c[:5, 4]).any()  # sd == 0: z = 0, and never -0


# ---- the DTW --------------------------------------------------------------------------------------------------------------------
def library_path(m):
    text, time = library("_dynamic_time_warping")(m)
    return np.asarray(text, np.int64), np.asarray(time, np.int64)


@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_oracle_dtw_matches_the_library(cases, case):
    _, c = cases[case]
    _, n, k = SHAPES[case]
    m = np.ascontiguousarray(c[:n, :k])
    D, trace = AO.dtw_cells(m)
    rows, frames = AO.walk(trace)
    text, time = library_path(m)
    assert np.array_equal(rows, text) and np.array_equal(frames, time)
    D2, trace2 = AO.dtw_cells_wavefront(m)
    assert np.array_equal(D, D2) and np.array_equal(trace, trace2)


@pytest.mark.parametrize("shape", ((9, 50), (17, 23), (30, 30)))
def test_oracle_dtw_matches_the_library_on_ties(shape):
    m = AO.quantised(*shape, seed=shape[0])
    tied = AO.tied_fraction(m)
    assert tied >= 0.10, tied  # the tie rule is exercised
    D, trace = AO.dtw_cells(m)
    rows, frames = AO.walk(trace)
    text, time = library_path(m)
    assert np.array_equal(rows, text) and np.array_equal(frames, time)
    D2, trace2 = AO.dtw_cells_wavefront(m)
    assert np.array_equal(D, D2) and np.array_equal(trace, trace2)


def read_path(rows, frames, n, k):
    """frame_pos / tok_start / tok_end by their definitions, cell by cell."""
    cells = set(zip(rows.tolist(), frames.tolist()))
    frame_pos = [max(r for r in range(n) if (r, f) in cells) for f in range(k)]
    tok_start = [min(f for f in range(k) if (r, f) in cells) for r in range(n)]
    tok_end = tok_start[1:] + [k]
    return frame_pos, tok_start, tok_end


@pytest.mark.parametrize("shape", ((9, 50), (17, 23), (30, 7), (1, 6), (6, 1)))
def test_tables_match_a_direct_reading_of_the_path(shape):
    n, k = shape
    m = AO.quantised(n, k, seed=n + k)
    out = AO.dtw(m[None], [0], [n], [k])
    rows, frames = AO.walk(AO.dtw_cells(m)[1])
    fp, ts, te = read_path(rows, frames, n, k)
    assert out["frame_pos"][0].tolist() == fp and out["tok_start"][0].tolist() == ts and out["tok_end"][0].tolist() == te
    assert out["path_len"][0] == len(rows) and rows[0] == 0 and frames[0] == 0 and rows[-1] == n - 1 and frames[-1] == k - 1
    assert (np.diff(rows) >= 0).all() and (np.diff(frames) >= 0).all() and ((np.diff(rows) + np.diff(frames)) >= 1).all()
    if n > k:  # more rows than frames: vertical runs, several rows on one frame, zero-length tokens
        assert (np.diff(frames) == 0).any() and (np.asarray(ts) == np.asarray(te)).any()


def test_row_window_and_invalid_utterances():
    m = AO.quantised(12, 20, seed=1)
    cost = np.stack((m, m, m))
    cost[2, 5, 5] = np.nan
    out = AO.dtw(cost, [3, 0, 3], [7, 0, 7], [20, 20, 20])
    alone = AO.dtw(m[None, 3:10], [0], [7], [20])
    assert np.array_equal(out["frame_pos"][0], alone["frame_pos"][0] + 3)
    assert np.array_equal(out["tok_start"][0, 3:10], alone["tok_start"][0]) and (out["tok_start"][0, :3] == -1).all()
    assert (out["tok_end"][0, 10:] == -1).all() and out["path_cost"][0] == alone["path_cost"][0]
    for u in (1, 2):
        assert (out["frame_pos"][u] == -1).all() and out["path_len"][u] == 0 and np.isinf(out["path_cost"][u])
    assert out["status"].tolist() == [2, 1]


# ---- the entry points -----------------------------------------------------------------------------------------------------------
def test_argument_errors_do_not_need_a_gpu():
    lib = N.lib()
    P = 0x1000  # any non-null address: an argument error returns before anything is read
    good_cost = [P, N.DT_F32, 1, 2, 8, 16, P, P, 7, P, P, P, None]
    assert lib.wsae_align_cost(*good_cost[:0], None, *good_cost[1:]) == -1 and "null" in N.last_error()
    for pos, bad, word in ((1, 5, "w_dtype"), (2, -1, "n_utt"), (3, 0, "n_heads"), (3, N.ALIGN_MAX_HEADS + 1, "n_heads"),
                           (4, 0, "ld_t"), (5, 0, "ld_f"), (8, 4, "width"), (8, 17, "width"), (8, -1, "width")):
        args = list(good_cost)
        args[pos] = bad
        assert lib.wsae_align_cost(*args) == -1, (pos, bad)
        assert "wsae_align_cost" in N.last_error() and word in N.last_error()
    assert lib.wsae_align_workspace_bytes(-1, 8, 16) == -1 and lib.wsae_align_workspace_bytes(1, 0, 16) == -1
    assert lib.wsae_align_workspace_bytes(1, 8, 0) == -1
    need = lib.wsae_align_workspace_bytes(16, 448, 1500)
    assert need >= 16 * 448 * 1500 // 4 and need % 256 == 0  # two bits a cell
    good_dtw = [P, 1, 8, 16, P, P, P, None, P, P, P, P, P, P, P, lib.wsae_align_workspace_bytes(1, 8, 16), None]
    for pos, bad, word in ((0, None, "null"), (4, None, "null"), (13, None, "null"), (1, -1, "n_utt"), (2, 0, "ld_t"),
                           (3, 0, "ld_f"), (15, 8, "workspace"), (14, None, "workspace"), (14, P + 4, "aligned")):
        args = list(good_dtw)
        args[pos] = bad
        assert lib.wsae_align_dtw(*args) == -1, (pos, bad)
        assert "wsae_align_dtw" in N.last_error() and word in N.last_error()
    with pytest.raises(N.WsaeError):
        N.check(-1, "wsae_align_dtw")


def test_no_cpu_path():
    model = tiny_whisper(0)
    ids = torch.tensor([[1, 5, 6, 7, 2]])
    with pytest.raises(N.WsaeError, match="GPU"):
        align_tokens(model, torch.randn(1, 80, 100), ids, n_prefix=1, device="cpu")


# ---- the tap --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def whisper():
    return tiny_whisper(0)


def test_alignment_heads_default_and_configured(whisper):
    assert alignment_heads(whisper) == [(1, 0), (1, 1)]  # the upper half of two layers
    whisper.generation_config.alignment_heads = [[0, 1], [1, 0]]
    try:
        assert alignment_heads(whisper) == [(0, 1), (1, 0)]
    finally:
        whisper.generation_config.alignment_heads = None


def test_tap_keeps_the_selected_heads_and_restores_the_implementation(whisper):
    mel = torch.randn(2, 80, 100, generator=torch.Generator().manual_seed(3))
    ids = torch.tensor([[1, 17, 33, 150, 199, 2], [1, 8, 9, 2, 0, 0]])
    before = whisper.config._attn_implementation
    assert before != "eager"
    heads = [(1, 1), (0, 1)]
    with torch.no_grad(), CrossAttentionTap(whisper, heads) as tap:
        assert whisper.config._attn_implementation == "eager"
        run_whisper_transcript(whisper, None, mel, ids, "cpu")
        got = tap.weights()
    assert whisper.config._attn_implementation == before
    assert not tap._hooks and not whisper.model.decoder.layers[1].encoder_attn._forward_hooks  # the hooks are gone
    assert tap.heads ==[(0, 1), (1, 1)] and sorted(tap._kept) == [0, 1]
    assert all(t.shape == (2, 1, 6, 50) for t in tap._kept.values())  # one head of each layer: the others are not kept
    assert got.shape == (2, 2, 6, 50)
    assert torch.allclose(got.sum(-1), torch.ones(2, 2, 6), atol=1e-5)  # attention probabilities
    # the same weights as the model reports them itself under the eager implementation
    whisper.set_attn_implementation("eager")
    try:
        with torch.no_grad():
            enc = whisper.model.encoder(mel).last_hidden_state
            out = whisper.model.decoder(input_ids=ids, encoder_hidden_states=enc, output_attentions=True)
        want = torch.stack((out.cross_attentions[0][:, 1], out.cross_attentions[1][:, 1]), dim=1)
    finally:
        whisper.set_attn_implementation(before)
    assert torch.equal(got, want)


def test_tap_names_eager_when_the_weights_are_missing(whisper):
    mel, ids = torch.randn(1, 80, 100), torch.tensor([[1, 5, 2]])
    with torch.no_grad(), CrossAttentionTap(whisper, [(1, 0)], switch_to_eager=False) as tap:
        with pytest.raises(N.WsaeError, match="eager"):
            run_whisper_transcript(whisper, None, mel, ids, "cpu")
        with pytest.raises(N.WsaeError, match="no forward"):
            tap.weights()
    with pytest.raises(ValueError):
        CrossAttentionTap(whisper, [(2, 0)])


def test_transcript_driver_runs_the_whole_sequence(whisper):
    from whisper_sae.sae.hooks import WhisperActivationExtractor
    mel, ids = torch.randn(2, 80, 100), torch.tensor([[1, 5, 6, 2], [1, 7, 2, 0]])
    ex = WhisperActivationExtractor(whisper, encoder_layers=[1], decoder_layers=[])
    with torch.no_grad(), ex:
        enc, dec = run_whisper_transcript(whisper, ex, mel, ids, "cpu")
    assert enc.shape == (2, 50, 64) and dec.shape == (2, 4, 64)
    assert ex.cache.get_encoder_activations(1).shape == (2, 50, 64)
    with pytest.raises(ValueError):
        run_whisper_transcript(whisper, None, mel, ids[:1], "cpu")
