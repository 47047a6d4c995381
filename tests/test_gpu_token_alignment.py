"""Token alignment on the MI355X: ``wsae_align_cost`` and ``wsae_align_dtw`` bit for bit against the sequential oracle of
tests/align_oracle.py through the C ABI - junk tails behind every array, junk (NaN) in every cell the kernels must not
read, a poisoned workspace - and the Python layer on a tiny Whisper.  The oracle itself is checked against the installed
library's formulation on the CPU in tests/test_token_alignment.py."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import align_oracle as AO
from test_token_alignment import tiny_whisper
from whisper_sae import _native as N
from whisper_sae.analysis import CrossAttentionTap, align_tokens, align_weights, aligned_batches, collect_token_association
from whisper_sae.sae.hooks import run_whisper_transcript
from whisper_sae.sae.model import TopKSAE

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
JUNK = 0x5a5a5a5
TAIL = 3  # junk elements behind every array


def padded(a: np.ndarray, junk, dtype=None) -> torch.Tensor:
    """``a`` flattened on the device with TAIL junk elements behind it."""
    t = torch.from_numpy(np.ascontiguousarray(a)).reshape(-1)
    if dtype is not None:
        t = t.to(dtype)
    return torch.cat((t, torch.full((TAIL,), junk, dtype=t.dtype))).to(DEV)


def output(n: int, junk, dtype) -> torch.Tensor:
    return torch.full((n + TAIL,), junk, dtype=dtype, device=DEV)


def intact(t: torch.Tensor, n: int, junk) -> bool:
    return bool((t[n:] == junk).all())


def stream():
    return torch.cuda.current_stream().cuda_stream


def run_cost(w: np.ndarray, n_tok, n_frames, width: int, dtype=None):
    """``wsae_align_cost`` on ``w [n_utt, n_heads, ld_t, ld_f]`` -> (cost, n_bad, status) as numpy."""
    n_utt, n_heads, ld_t, ld_f = w.shape
    dw = padded(w, 0.5, dtype)
    code = {torch.float32: N.DT_F32, torch.bfloat16: N.DT_BF16, torch.float16: N.DT_F16}[dw.dtype]
    nt, nf = padded(np.asarray(n_tok, np.int32), JUNK), padded(np.asarray(n_frames, np.int32), JUNK)
    cost = output(n_utt * ld_t * ld_f, 7.5, torch.float32)
    n_bad = output(n_utt, JUNK, torch.int32)
    status = torch.zeros(2 + TAIL, dtype=torch.int64, device=DEV)
    status[2:] = JUNK
    N.check(N.lib().wsae_align_cost(dw.data_ptr(), code, n_utt, n_heads, ld_t, ld_f, nt.data_ptr(), nf.data_ptr(), width,
                                    cost.data_ptr(), n_bad.data_ptr(), status.data_ptr(), stream()), "wsae_align_cost")
    torch.cuda.synchronize()
    assert intact(cost, n_utt * ld_t * ld_f, 7.5) and intact(n_bad, n_utt, JUNK) and intact(status, 2, JUNK)
    return (cost[:-TAIL].reshape(n_utt, ld_t, ld_f).cpu().numpy(), n_bad[:n_utt].cpu().numpy(), status[:2].cpu().numpy())


def run_dtw(cost: np.ndarray, row_first, row_count, n_frames, n_bad=None) -> dict:
    """``wsae_align_dtw`` on ``cost [n_utt, ld_t, ld_f]`` -> its outputs as numpy."""
    n_utt, ld_t, ld_f = cost.shape
    lib = N.lib()
    need = lib.wsae_align_workspace_bytes(n_utt, ld_t, ld_f)
    assert need >= 0
    ws = torch.full((need + 64,), 0xAB, dtype=torch.uint8, device=DEV)  # (arbitrary contents on entry)
    dc = padded(cost.astype(np.float32), 0.5)
    first, count, frames = (padded(np.asarray(v, np.int32), JUNK) for v in (row_first, row_count, n_frames))
    bad = None if n_bad is None else padded(np.asarray(n_bad, np.int32), JUNK)
    out = {"frame_pos": output(n_utt * ld_f, JUNK, torch.int32), "tok_start": output(n_utt * ld_t, JUNK, torch.int32),
           "tok_end": output(n_utt * ld_t, JUNK, torch.int32), "path_cost": output(n_utt, 7.5, torch.float32),
           "path_len": output(n_utt, JUNK, torch.int32)}
    status = torch.zeros(2 + TAIL, dtype=torch.int64, device=DEV)
    status[2:] = JUNK
    N.check(lib.wsae_align_dtw(dc.data_ptr(), n_utt, ld_t, ld_f, first.data_ptr(), count.data_ptr(), frames.data_ptr(), N.ptr(bad),
                               out["frame_pos"].data_ptr(), out["tok_start"].data_ptr(), out["tok_end"].data_ptr(),
                               out["path_cost"].data_ptr(), out["path_len"].data_ptr(), status.data_ptr(), ws.data_ptr(), need,
                               stream()), "wsae_align_dtw")
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xAB).all()) and intact(status, 2, JUNK)
    shapes = {"frame_pos": (n_utt, ld_f), "tok_start": (n_utt, ld_t), "tok_end": (n_utt, ld_t), "path_cost": (n_utt,),
              "path_len": (n_utt,)}
    got = {}
    for name, t in out.items():
        n = int(np.prod(shapes[name]))
        assert intact(t, n, 7.5 if name == "path_cost" else JUNK), name
        got[name] = t[:n].reshape(shapes[name]).cpu().numpy()
    got["status"] = status[:2].cpu().numpy()
    return got


def same_bits(got: np.ndarray, want: np.ndarray, what: str = ""):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    assert np.array_equal(got.view(np.uint32) if got.dtype == np.float32 else got,
                          want.view(np.uint32) if want.dtype == np.float32 else want), what


def same_dtw(got: dict, want: dict):
    for name in ("frame_pos", "tok_start", "tok_end", "path_cost", "path_len", "status"):
        same_bits(got[name], want[name], name)


# ---- the cost -------------------------------------------------------------------------------------------------------------------
LD_T, LD_F = 72, 140


def ragged_weights(n_heads: int, width: int, dtype=np.float32):
    """Five utterances of different sizes in one array; every cell outside an utterance's rows and frames holds NaN, which
    the kernel would count if it read it.  The sizes: one token (every column constant: sd = 0), the smallest number of
    frames the width admits, one tile, one tile and a frame, three tiles; a constant column in the last."""
    p = width // 2
    sizes = [(1, 23), (2, p + 1), (9, 64), (70, 65), (9, 131)]
    w = np.full((len(sizes), n_heads, LD_T, LD_F), np.nan, dtype)
    for u, (n, k) in enumerate(sizes):
        w[u, :, :n, :k] = AO.attention(n_heads, n, k, seed=10 * width + u, dtype=dtype)
    w[4, 0, :9, 77] = 0.125
    return w, [s[0] for s in sizes], [s[1] for s in sizes]


@pytest.mark.parametrize("n_heads,width", [(1, 1), (3, 3), (3, 7), (1, 15), (3, 15)])
def test_cost_equals_the_oracle(n_heads, width):
    w, n_tok, n_frames = ragged_weights(n_heads, width)
    cost, n_bad, status = run_cost(w, n_tok, n_frames, width)
    want, want_bad, want_status = AO.cost(w, n_tok, n_frames, width)
    assert n_bad.tolist() == want_bad.tolist() == [0] * 5 and status.tolist() == want_status.tolist() == [0, 0]
    same_bits(cost, want)
    assert (cost[0, 0, :23] == 0).all() and not np.signbit(cost[0, 0, :23]).any()  # sd == 0: +0


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_cost_of_half_precision_weights(dtype):
    w, n_tok, n_frames = ragged_weights(3, 7)
    half = torch.from_numpy(np.nan_to_num(w, nan=0.0)).to(dtype)
    exact = half.float().numpy()  # (what the kernel reads, exactly)
    exact[np.isnan(w)] = np.nan
    cost, n_bad, status = run_cost(exact, n_tok, n_frames, 7, dtype=dtype)
    want, _, _ = AO.cost(exact, n_tok, n_frames, 7)
    assert n_bad.tolist() == [0] * 5 and status.tolist() == [0, 0]
    same_bits(cost, want)


def test_cost_of_invalid_utterances():
    """One NaN and one +inf in the middle utterance, invalid sizes in two others: their cost is the fill, status counts,
    and the neighbours are what they are alone."""
    w = np.stack([AO.attention(2, 9, 70, seed=s) for s in range(5)])
    w[1, 1, 3, 69] = np.nan
    w[1, 0, 8, 0] = np.inf
    n_tok, n_frames = [9, 9, 9, 0, 9], [70, 70, 70, 70, 3]
    cost, n_bad, status = run_cost(w, n_tok, n_frames, 7)
    want, want_bad, want_status = AO.cost(w, n_tok, n_frames, 7)
    assert n_bad.tolist() == want_bad.tolist() == [0, 2, 0, -1, -1] and status.tolist() == want_status.tolist() == [3, 2]
    same_bits(cost, want)
    assert np.isinf(cost[[1, 3, 4]]).all()
    alone, _, _ = run_cost(w[2:3], [9], [70], 7)
    same_bits(alone[0], cost[2])


def test_cost_alone_and_in_a_batch():
    w, n_tok, n_frames = ragged_weights(3, 7)
    cost, _, _ = run_cost(w, n_tok, n_frames, 7)
    for u in (0, 3):
        alone, _, _ = run_cost(w[u:u + 1], n_tok[u:u + 1], n_frames[u:u + 1], 7)
        same_bits(alone[0], cost[u])


# ---- the DTW --------------------------------------------------------------------------------------------------------------------
def ridge_cost(n: int, k: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((n, k)).astype(np.float32)
    centre = (np.arange(n)[:, None] + 0.5) * k / n
    return (m - 3.0 * np.exp(-0.5 * ((np.arange(k)[None, :] - centre) / max(k / n, 1.0)) ** 2)).astype(np.float32)


def dtw_batch():
    """(cost [n_utt, 133, 135], row_first, row_count, n_frames): 1 x M, N x 1, N > M, the strip and block edges both ways,
    an all-zero matrix, the quantised tie matrix and a non-zero first row.  NaN wherever the kernel must not read."""
    items = [(ridge_cost(1, 37, 1), 0), (ridge_cost(9, 1, 2), 0), (ridge_cost(30, 7, 3), 0), (ridge_cost(65, 130, 4), 0),
             (ridge_cost(130, 65, 5), 0), (np.zeros((20, 33), np.float32), 0), (AO.quantised(40, 90, 6), 0),
             (ridge_cost(64, 64, 7), 3), (ridge_cost(70, 16, 8), 63)]
    cost = np.full((len(items), 133, 135), np.nan, np.float32)
    for u, (m, first) in enumerate(items):
        cost[u, first:first + m.shape[0], :m.shape[1]] = m
    return cost, [f for _, f in items], [m.shape[0] for m, _ in items], [m.shape[1] for m, _ in items]


def test_dtw_equals_the_oracle():
    cost, first, count, frames = dtw_batch()
    assert AO.tied_fraction(cost[6, :40, :90]) >= 0.10
    got = run_dtw(cost, first, count, frames)
    want = AO.dtw(cost, first, count, frames, wavefront=True)
    assert want["status"].tolist() == [0, 0] and (want["path_len"] > 0).all()
    same_dtw(got, want)
    # alone and in the batch
    for u in (4, 8):
        alone = run_dtw(cost[u:u + 1], first[u:u + 1], count[u:u + 1], frames[u:u + 1])
        for name in ("frame_pos", "tok_start", "tok_end", "path_cost", "path_len"):
            same_bits(alone[name][0], got[name][u], name)


def test_dtw_of_invalid_utterances():
    m = ridge_cost(12, 40, 9)
    cost = np.stack([m] * 6)
    cost[2, 5, 17] = np.nan      # a non-finite cost inside the window
    cost[3, 11, 39] = np.inf     # ... and one outside it: never read
    first, count, frames = [0, 0, 2, 0, 5, 0], [12, 0, 9, 11, 8, 12], [40, 40, 40, 39, 40, 0]
    n_bad = [0, 0, 0, 0, 0, 0]
    got = run_dtw(cost, first, count, frames, n_bad)
    want = AO.dtw(cost, first, count, frames, n_bad)
    assert want["status"].tolist() == [4, 1] and (want["path_len"] > 0).tolist() == [True, False, False, True, False, False]
    same_dtw(got, want)
    flagged = run_dtw(cost[:1], [0], [12], [40], [2])  # rejected by the cost kernel
    same_dtw(flagged, AO.dtw(cost[:1], [0], [12], [40], [2]))
    assert flagged["path_len"].tolist() == [0] and flagged["status"].tolist() == [1, 0]


def test_dtw_at_the_size_of_a_full_utterance():
    m = ridge_cost(448, 1500, 11)
    got = run_dtw(m[None], [0], [448], [1500])
    want = AO.dtw(m[None], [0], [448], [1500], wavefront=True)
    same_dtw(got, want)
    assert want["path_len"][0] >= 1500


# ---- the Python layer -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def whisper():
    return tiny_whisper(0).to(DEV)


MEL = torch.randn(3, 80, 100, generator=torch.Generator().manual_seed(7))
IDS = torch.tensor([[1, 3, 17, 33, 150, 199, 64, 2], [1, 3, 8, 9, 120, 2, 0, 0], [1, 3, 44, 2, 0, 0, 0, 0]])
LENGTHS, MEL_FRAMES, PREFIX = [8, 6, 4], [100, 80, 100], 2


def oracle_alignment(whisper):
    """The oracle on the weights the tap captures: (frame_pos, tokens per frame) as numpy."""
    with torch.no_grad(), CrossAttentionTap(whisper) as tap:
        run_whisper_transcript(whisper, None, MEL, IDS, DEV)
        w = tap.weights()
    w = w.float().cpu().numpy()
    n_frames = [f // 2 for f in MEL_FRAMES]
    cost, n_bad, _ = AO.cost(w, LENGTHS, n_frames, 7)
    want = AO.dtw(cost, [PREFIX - 1] * 3, [n - PREFIX for n in LENGTHS], n_frames, n_bad)
    pos = want["frame_pos"].astype(np.int64)
    tokens = np.where(pos >= 0, np.take_along_axis(IDS.numpy(), np.maximum(pos + 1, 0), axis=1), -1)
    return w, want, tokens


def test_align_tokens_equals_the_oracle_on_the_captured_weights(whisper):
    w, want, tokens = oracle_alignment(whisper)
    found = align_tokens(whisper, MEL, IDS, n_prefix=PREFIX, token_lengths=LENGTHS, num_frames=MEL_FRAMES, device=DEV)
    assert found.valid.tolist() == [True] * 3 and whisper.config._attn_implementation != "eager"
    assert np.array_equal(found.frame_pos.cpu().numpy(), want["frame_pos"])
    assert np.array_equal(found.frame_tokens.cpu().numpy(), tokens)
    assert np.array_equal(found.frame_mask.cpu().numpy(), want["frame_pos"] >= 0)
    assert (found.frame_tokens[1, 40:] == -1).all() and (found.frame_tokens[1, :40] >= 0).all()
    assert np.array_equal(found.token_start[:, 1:].cpu().numpy(), want["tok_start"][:, :-1])
    assert np.array_equal(found.token_end[:, 1:].cpu().numpy(), want["tok_end"][:, :-1])
    same_bits(found.path_cost.cpu().numpy(), want["path_cost"])
    assert found.path_len.tolist() == want["path_len"].tolist()
    start, end = found.token_times()
    assert float(start[0, PREFIX]) == 0.0 and float(end[0, LENGTHS[0] - 1]) == 50 * 0.02 and bool(torch.isnan(start[0, 0]))
    words = found.word_labels(torch.arange(8).expand(3, 8) // 2)
    assert np.array_equal(words.cpu().numpy(), np.where(want["frame_pos"] >= 0, (want["frame_pos"] + 1) // 2, -1))
    raw = align_weights(torch.from_numpy(w).to(DEV), LENGTHS, [50, 40, 50], row_first=[PREFIX - 1] * 3,
                        row_count=[n - PREFIX for n in LENGTHS])
    assert np.array_equal(raw.frame_pos.cpu().numpy(), want["frame_pos"]) and raw.status.tolist() == [0, 0]


def test_token_association_fed_by_aligned_batches(whisper):
    _, want, tokens = oracle_alignment(whisper)
    torch.manual_seed(3)
    sae = TopKSAE(64, 256, k=8).to(DEV)
    items = list(aligned_batches(whisper, [(MEL, IDS, LENGTHS, MEL_FRAMES)], encoder_layer=1, n_prefix=PREFIX, device=DEV))
    (x, frame_tokens, frame_mask), = items
    assert x.shape == (3, 50, 64) and x.device.type == "cuda"
    assert np.array_equal(frame_tokens.cpu().numpy(), tokens) and np.array_equal(frame_mask.cpu().numpy(), tokens >= 0)
    got = collect_token_association(sae, items, 200, capacity=1 << 12, device=DEV).pairs()
    fed = collect_token_association(sae, [(x, torch.from_numpy(tokens).to(DEV), torch.from_numpy(tokens >= 0).to(DEV))], 200,
                                    capacity=1 << 12, device=DEV).pairs()
    assert got.count.numel() > 0 and int(got.count.sum()) > 0
    for a, b in zip(got, fed):
        assert torch.equal(a, b)
