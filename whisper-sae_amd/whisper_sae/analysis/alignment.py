"""Token alignment: a token label for every encoder frame, from Whisper's own cross-attention.

Every label-driven analysis of this package (``TokenAssociation``, ``LabelAssociation``, ``SparseProbe``, ...) takes one
integer per frame.  This module produces it from ``(mel, transcript)`` pairs with the recipe behind Whisper's word
timestamps: the cross-attention weights of a few *alignment heads* are z-scored over the token axis, median-filtered along
time, averaged and negated (``wsae_align_cost``), and dynamic time warping over that tokens x frames matrix
(``wsae_align_dtw``) gives every frame the token whose span it falls in.  ``CrossAttentionTap`` captures the weights of the
selected heads during a teacher-forced forward (``run_whisper_transcript``); ``aligned_batches`` runs the activation
extractor and the tap in ONE forward and yields ``(x, frame_tokens, frame_mask)`` items, the format every ``collect_*``
function accepts.

Row ``q`` of the attention (the decoder at input position ``q``) predicts the token at position ``q + 1``; as in Whisper the
rows are normalised over the whole sequence, and the alignment then runs over rows ``n_prefix - 1 .. length - 2``: the
start-of-transcript prefix and the row of the final end-of-text input are dropped.  The tokens aligned are therefore the
positions ``n_prefix .. length - 1`` - the transcript and its end-of-text token, which takes the trailing frames.

Out of scope: Whisper's word merging and punctuation heuristics, its long-pause corrections, beam-search index gathering,
Sakoe-Chiba bands, and the softmax recomputed from hooked queries and keys inside the kernel (``exp`` on the device would
cost the bit-exact oracle).  There is no CPU path.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Iterable, List, NamedTuple, Optional, Sequence, Tuple

import torch
from torch import Tensor

from .. import _native as N
from ..sae.hooks import WhisperActivationExtractor, run_whisper_transcript
from . import _stream

_DTYPES = {torch.float32: N.DT_F32, torch.bfloat16: N.DT_BF16, torch.float16: N.DT_F16}


def alignment_heads(model) -> List[Tuple[int, int]]:
    """``[(decoder layer, head), ...]``: ``generation_config.alignment_heads`` where the checkpoint ships them, else every
    head of the upper half of the decoder layers (OpenAI's default)."""
    heads = getattr(getattr(model, "generation_config", None), "alignment_heads", None)
    if heads:
        return [(int(layer), int(head)) for layer, head in heads]
    layers, per_layer = model.config.decoder_layers, model.config.decoder_attention_heads
    return [(layer, head) for layer in range(layers // 2, layers) for head in range(per_layer)]


class CrossAttentionTap:
    """Context manager that keeps the cross-attention weights of the selected ``heads`` during the forward passes inside it.

    Forward hooks sit on ``decoder.layers[l].encoder_attn`` of only the layers that hold a selected head, and keep
    ``weights[:, heads of l]`` where they were produced; the other heads are never kept.  The fused attention
    implementations return no weights, so the tap switches the model to the eager implementation for its lifetime and
    restores the previous one.  ``weights()`` is ``[n_utt, len(heads), n_tok, frames]`` of the last forward, heads in the
    order of ``self.heads`` (sorted by layer, then head)."""

    def __init__(self, model, heads: Optional[Sequence[Tuple[int, int]]] = None, switch_to_eager: bool = True):
        self.model = model
        chosen = alignment_heads(model) if heads is None else [(int(layer), int(head)) for layer, head in heads]
        self.heads = sorted(set(chosen))
        if not self.heads:
            raise ValueError("CrossAttentionTap needs at least one (layer, head)")
        layers, per_layer = model.config.decoder_layers, model.config.decoder_attention_heads
        for layer, head in self.heads:
            if not (0 <= layer < layers and 0 <= head < per_layer):
                raise ValueError(f"head ({layer}, {head}) is outside {layers} decoder layers x {per_layer} heads")
        self.switch_to_eager = switch_to_eager
        self._by_layer = {}
        for layer, head in self.heads:
            self._by_layer.setdefault(layer, []).append(head)
        self._kept: dict = {}
        self._hooks: list = []
        self._previous: Optional[str] = None

    def _hook(self, layer: int):
        def take(module, inputs, output):
            weights = output[1] if isinstance(output, (tuple, list)) and len(output) > 1 else None
            if weights is None:
                raise N.WsaeError(
                    f"decoder layer {layer}: the cross-attention returned no weights under the "
                    f"'{self.model.config._attn_implementation}' attention implementation; they exist only under the eager "
                    f"implementation (model.set_attn_implementation(\"eager\"))")
            self._kept[layer] = weights.detach()[:, self._by_layer[layer]]
        return take

    def __enter__(self) -> "CrossAttentionTap":
        self._previous = self.model.config._attn_implementation
        if self.switch_to_eager and self._previous != "eager":
            self.model.set_attn_implementation("eager")
        for layer in self._by_layer:
            block = self.model.model.decoder.layers[layer].encoder_attn
            self._hooks.append(block.register_forward_hook(self._hook(layer)))
        return self

    def __exit__(self, *exc) -> None:
        while self._hooks:
            self._hooks.pop().remove()
        if self.model.config._attn_implementation != self._previous:
            self.model.set_attn_implementation(self._previous)

    def weights(self) -> Tensor:
        missing = [layer for layer in self._by_layer if layer not in self._kept]
        if missing:
            raise N.WsaeError(f"CrossAttentionTap: no forward has passed decoder layers {missing} yet")
        return torch.cat([self._kept[layer] for layer in sorted(self._by_layer)], dim=1)


class RawAlignment(NamedTuple):
    """The outputs of the two kernels, rows numbered as in the weights: ``cost`` float32 ``[n_utt, n_tok, frames]``;
    ``frame_pos`` ``[n_utt, frames]``, ``tok_start`` / ``tok_end`` ``[n_utt, n_tok]``, ``path_len`` ``[n_utt]`` int32;
    ``path_cost`` float32 ``[n_utt]``; ``n_bad`` int32 ``[n_utt]``; ``status`` int64 ``[2]``: the invalid utterances and
    the non-finite values met, of both kernels together."""

    cost: Tensor
    frame_pos: Tensor
    tok_start: Tensor
    tok_end: Tensor
    path_cost: Tensor
    path_len: Tensor
    n_bad: Tensor
    status: Tensor


def _int32(values, n_utt: int, default: int, dev, name: str) -> Tensor:
    if values is None:
        return torch.full((n_utt,), default, dtype=torch.int32, device=dev)
    t = torch.as_tensor(values).reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
    if t.numel() != n_utt:
        raise ValueError(f"{name} has {t.numel()} entries for {n_utt} utterances")
    return t


def align_weights(weights: Tensor, n_tok=None, n_frames=None, *, row_first=None, row_count=None, width: int = 7) -> RawAlignment:
    """The two kernels on weights the caller already has: ``weights [n_utt, n_heads, n_tok, frames]`` on the GPU, float32,
    float16 or bfloat16.  ``n_tok`` / ``n_frames`` (per utterance; default: all) are the rows and frames that are read;
    the alignment runs over rows ``row_first .. row_first + row_count - 1`` (default: all ``n_tok`` rows)."""
    if weights.dim() != 4:
        raise ValueError(f"weights must be [n_utt, n_heads, n_tok, frames], got {tuple(weights.shape)}")
    dev = _stream.need_gpu("align_weights", weights.device)
    if weights.dtype not in _DTYPES:
        raise ValueError(f"weights must be float32, float16 or bfloat16, got {weights.dtype}")
    if not (1 <= int(width) <= N.ALIGN_MAX_WIDTH and int(width) % 2 == 1):
        raise ValueError(f"width must be odd in 1..{N.ALIGN_MAX_WIDTH}, got {width}")
    w = weights.detach().contiguous()
    n_utt, n_heads, ld_t, ld_f = w.shape
    if not 1 <= n_heads <= N.ALIGN_MAX_HEADS:
        raise ValueError(f"1..{N.ALIGN_MAX_HEADS} heads can be averaged, got {n_heads}")
    nt = _int32(n_tok, n_utt, ld_t, dev, "n_tok")
    nf = _int32(n_frames, n_utt, ld_f, dev, "n_frames")
    first = _int32(row_first, n_utt, 0, dev, "row_first")
    count = nt - first if row_count is None else _int32(row_count, n_utt, 0, dev, "row_count")
    cost = torch.empty(n_utt, ld_t, ld_f, dtype=torch.float32, device=dev)
    n_bad = torch.empty(n_utt, dtype=torch.int32, device=dev)
    status = torch.zeros(2, 2, dtype=torch.int64, device=dev)
    frame_pos = torch.empty(n_utt, ld_f, dtype=torch.int32, device=dev)
    tok_start = torch.empty(n_utt, ld_t, dtype=torch.int32, device=dev)
    tok_end = torch.empty(n_utt, ld_t, dtype=torch.int32, device=dev)
    path_cost = torch.empty(n_utt, dtype=torch.float32, device=dev)
    path_len = torch.empty(n_utt, dtype=torch.int32, device=dev)
    if n_utt == 0 or ld_t == 0 or ld_f == 0:
        return RawAlignment(cost, frame_pos, tok_start, tok_end, path_cost, path_len, n_bad, status[0])
    lib = N.lib()
    need = lib.wsae_align_workspace_bytes(n_utt, ld_t, ld_f)
    if need < 0:
        raise N.WsaeError(f"wsae_align_workspace_bytes rejects n_utt={n_utt} n_tok={ld_t} frames={ld_f}")
    ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)  # (8-byte aligned)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        N.check(lib.wsae_align_cost(w.data_ptr(), _DTYPES[w.dtype], n_utt, n_heads, ld_t, ld_f, nt.data_ptr(), nf.data_ptr(),
                                    int(width), cost.data_ptr(), n_bad.data_ptr(), status[0].data_ptr(), stream),
                "wsae_align_cost")
        N.check(lib.wsae_align_dtw(cost.data_ptr(), n_utt, ld_t, ld_f, first.data_ptr(), count.data_ptr(), nf.data_ptr(),
                                   n_bad.data_ptr(), frame_pos.data_ptr(), tok_start.data_ptr(), tok_end.data_ptr(),
                                   path_cost.data_ptr(), path_len.data_ptr(), status[1].data_ptr(), ws.data_ptr(), need, stream),
                "wsae_align_dtw")
    # an utterance the cost kernel rejects is rejected again by the DTW: count it once
    both = torch.stack((status[1, 0], status[0, 1] + status[1, 1]))
    return RawAlignment(cost, frame_pos, tok_start, tok_end, path_cost, path_len, n_bad, both)


@dataclass
class FrameAlignment:
    """The alignment of a batch.  ``frame_pos [n_utt, T]`` int64: the attention row that owns the frame (-1 where
    unaligned: beyond the utterance's frames, or an invalid utterance); the token it predicts sits at position
    ``frame_pos + 1``.  ``frame_tokens [n_utt, T]`` int64: that token's id, -1 where unaligned; ``frame_mask`` bool.
    ``token_start`` / ``token_end [n_utt, n_tok]`` int64 by token POSITION: the frames ``[start, end)`` of the token, -1
    for the positions that were not aligned (the prefix, padding); a token the path passes in no time has ``start == end``.
    ``path_cost`` float32, ``path_len`` int64 ``[n_utt]``; ``valid`` bool ``[n_utt]``: the utterance was aligned."""

    frame_pos: Tensor
    frame_tokens: Tensor
    frame_mask: Tensor
    token_start: Tensor
    token_end: Tensor
    path_cost: Tensor
    path_len: Tensor
    valid: Tensor

    def token_times(self, time_precision: float = 0.02) -> Tuple[Tensor, Tensor]:
        """``(start, end)`` in seconds, float64 ``[n_utt, n_tok]``; NaN for the positions that were not aligned."""
        nan = torch.full(self.token_start.shape, float("nan"), dtype=torch.float64, device=self.token_start.device)
        on = self.token_start >= 0
        return (torch.where(on, self.token_start.double() * time_precision, nan),
                torch.where(on, self.token_end.double() * time_precision, nan))

    def word_labels(self, word_of_position: Tensor) -> Tensor:
        """For callers who group tokens into words: ``word_of_position [n_utt, n_tok]`` (an integer per token position)
        gathered through the alignment, ``[n_utt, T]`` int64, -1 where unaligned."""
        words = torch.as_tensor(word_of_position).to(device=self.frame_pos.device, dtype=torch.int64)
        if words.shape != self.token_start.shape:
            raise ValueError(f"word_of_position must be {tuple(self.token_start.shape)}, got {tuple(words.shape)}")
        return _gather_positions(words, self.frame_pos)


def _gather_positions(per_position: Tensor, frame_pos: Tensor) -> Tensor:
    """``per_position[u, frame_pos[u, t] + 1]``, -1 where ``frame_pos < 0``."""
    on = frame_pos >= 0
    at = torch.where(on, frame_pos + 1, torch.zeros_like(frame_pos))
    return torch.where(on, per_position.gather(1, at), torch.full_like(at, -1))


def _frame_alignment(weights: Tensor, ids: Tensor, n_prefix: int, token_lengths, num_frames, width: int) -> FrameAlignment:
    n_utt, _, n_tok, frames = weights.shape
    n_prefix = int(n_prefix)
    if not 1 <= n_prefix < n_tok:
        raise ValueError(f"n_prefix must be in 1..{n_tok - 1} (the start-of-transcript tokens of {n_tok} positions), got {n_prefix}")
    dev = weights.device
    lengths = _int32(token_lengths, n_utt, n_tok, dev, "token_lengths")
    n_frames = None if num_frames is None else _int32(num_frames, n_utt, 0, dev, "num_frames") // 2  # (mel frames: two per position)
    raw = align_weights(weights, lengths, n_frames, row_first=torch.full_like(lengths, n_prefix - 1),
                        row_count=lengths - n_prefix, width=width)
    frame_pos = raw.frame_pos.to(torch.int64)
    minus = torch.full((n_utt, 1), -1, dtype=torch.int64, device=dev)
    return FrameAlignment(frame_pos=frame_pos, frame_tokens=_gather_positions(ids.to(device=dev, dtype=torch.int64), frame_pos),
                          frame_mask=frame_pos >= 0,
                          token_start=torch.cat((minus, raw.tok_start[:, :-1].to(torch.int64)), dim=1),
                          token_end=torch.cat((minus, raw.tok_end[:, :-1].to(torch.int64)), dim=1),
                          path_cost=raw.path_cost, path_len=raw.path_len.to(torch.int64), valid=raw.path_len > 0)


def align_tokens(model, input_features: Tensor, decoder_input_ids: Tensor, *, n_prefix: int, token_lengths=None,
                 num_frames=None, heads: Optional[Sequence[Tuple[int, int]]] = None, width: int = 7,
                 device="cuda") -> FrameAlignment:
    """Align the transcripts ``decoder_input_ids [n_utt, n_tok]`` (``n_prefix`` start-of-transcript tokens, the
    transcript, the end-of-text token, then padding) to the encoder frames of ``input_features`` in one teacher-forced
    forward of ``model`` (on ``device`` already).  ``token_lengths [n_utt]``: the tokens of every utterance up to and
    including its end-of-text token (default: all); ``num_frames [n_utt]``: its mel frames (default: all; two per
    encoder position).  ``heads``: see ``alignment_heads``; ``width``: the median filter's (Whisper: 7)."""
    _stream.need_gpu("align_tokens", torch.device(device))
    with torch.no_grad(), CrossAttentionTap(model, heads) as tap:
        run_whisper_transcript(model, None, input_features, decoder_input_ids, device)
        weights = tap.weights()
    return _frame_alignment(weights, decoder_input_ids, n_prefix, token_lengths, num_frames, width)


def aligned_batches(model, batches: Iterable, *, encoder_layer: int, n_prefix: int,
                    heads: Optional[Sequence[Tuple[int, int]]] = None, width: int = 7, apply_layer_norm: bool = True,
                    device="cuda", frontend=None):
    """``(x [n_utt, T, D], frame_tokens [n_utt, T], frame_mask [n_utt, T])`` of every item ``(input_features,
    decoder_input_ids[, token_lengths[, num_frames]])``: the (layer-normed) output of encoder layer ``encoder_layer`` and the
    token label of every frame, from ONE forward - the activation extractor and the cross-attention tap together.  The
    items are what ``collect_token_association`` and the other ``collect_*`` functions accept.  With a ``frontend`` (a
    ``whisper_sae.data.LogMel``) the first entry of an item may be a 2-D tensor of waveforms, or ``(waveforms, lengths)``:
    it is converted to mel features on the device first."""
    _stream.need_gpu("aligned_batches", torch.device(device))
    for item in batches:
        if not isinstance(item, (tuple, list)) or not 2 <= len(item) <= 4:
            raise ValueError("an item must be (input_features, decoder_input_ids[, token_lengths[, num_frames]])")
        features, ids = item[0], item[1]
        if frontend is not None:
            from ..data.audio import features_from_batch
            features = features_from_batch(frontend, features)
        lengths = item[2] if len(item) > 2 else None
        mel_frames = item[3] if len(item) > 3 else None
        extractor = WhisperActivationExtractor(model, encoder_layers=[encoder_layer], decoder_layers=[],
                                               apply_layer_norm=apply_layer_norm, keep_on_device=True)
        with torch.no_grad(), extractor, CrossAttentionTap(model, heads) as tap:
            run_whisper_transcript(model, extractor, features, ids, device)
            weights = tap.weights()
        x = extractor.cache.get_encoder_activations(encoder_layer)
        found = _frame_alignment(weights, ids, n_prefix, lengths, mel_frames, width)
        yield x, found.frame_tokens, found.frame_mask
