"""Dictionary comparison: which feature of dictionary B is feature f of dictionary A, how much of
A reappears in B (mean max cosine similarity), which features of one dictionary are near-duplicates.

All of it is one computation, ``wsae_match_rows``: for every row of one ``[H_a, D]`` matrix the ``n`` most similar rows
of another ``[H_b, D]`` matrix, from a GEMM whose epilogue is the selection, so the ``[H_a, H_b]`` similarity matrix is
never materialised.  The rows of a bound module are read in place from its parameter pack (``W_dT`` rows for the
decoder, ``W_e`` rows for the encoder, one layer's column slice for a crosscoder), with the pack's row stride as the
leading dimension.  The reductions over the resulting ``[H]`` vectors are plain torch.

Out of scope: optimal one-to-one assignment (Hungarian), a feature -> token
"logit lens" on the dot metric (the kernel takes any ``rows_b``; the Whisper-side glue is not here), fp8 operands.
"""

from __future__ import annotations

from typing import List, NamedTuple, Optional, Tuple, Union

import torch
from torch import Tensor, nn

from .. import _native as N
from ..sae.engine import require_device_tensor
from ..sae.packed import PackedModule

_METRICS = {"cosine": N.MATCH_COSINE, "dot": N.MATCH_DOT}
_PRECISIONS = {"fp32": N.PREC_FP32, "bf16": N.PREC_BF16}


class NearestFeatures(NamedTuple):
    """``values [H_a, n]`` float32 and ``indices [H_a, n]`` int32, per row sorted by value descending, then index
    ascending; where fewer than ``n`` candidates exist the tail is ``(-inf, -1)``."""

    values: Tensor
    indices: Tensor


def _rows(src: Union[nn.Module, Tensor], which: str, layer: Optional[int]) -> Tensor:
    """``[H, D]`` float32 device view with unit column stride of the rows to compare (no copy for a bound module)."""
    if which not in ("decoder", "encoder"):
        raise ValueError(f"which must be 'decoder' or 'encoder', got {which!r}")
    if isinstance(src, Tensor):
        if src.dim() != 2:
            raise ValueError(f"expected a [H, D] tensor, got shape {tuple(src.shape)}")
        require_device_tensor(src, "dictionary tensor")
        t = src.detach()
        if t.dtype != torch.float32:
            t = t.float()
        if t.shape[1] % 32:  # zero columns change neither a dot product nor a norm
            t = torch.nn.functional.pad(t, (0, 32 - t.shape[1] % 32))
        if t.stride(1) != 1 or t.stride(0) % 4 or t.stride(0) < t.shape[1] or t.data_ptr() % 16:
            t = t.contiguous()
        return t
    if not isinstance(src, PackedModule):
        raise TypeError(f"expected an SAE-family module or a [H, D] tensor, got {type(src).__name__}")
    eng = src.bind()
    # the pack's rows at the engine width: columns beyond a narrower module's real width are zero and stay zero
    full = eng.view("decoder.weight").t() if which == "decoder" else eng.view("encoder.weight")
    n_layers = getattr(src, "n_layers", None)
    if n_layers is None:  # (layer= speaks to the crosscoder arguments only)
        return full
    if layer is None:
        raise ValueError("a crosscoder needs layer= (an entry of its layer_indices)")
    if layer not in src.layer_indices:
        raise ValueError(f"layer {layer} is not one of {src.layer_indices}")
    i, d = src.layer_indices.index(layer), src.d_model
    if d % 32:
        raise ValueError(f"d_model = {d}: a crosscoder layer slice is compared in place and must be a multiple of 32 wide")
    return full[:, i * d:(i + 1) * d]


def nearest_features(a, b=None, *, n: int = 4, which: str = "decoder", metric: str = "cosine", precision: str = "fp32",
                     exclude_self: Optional[bool] = None, layer: Optional[int] = None) -> NearestFeatures:
    """For every feature of ``a`` its ``n`` most similar features of ``b``.

    ``a``, ``b``: SAE-family modules (``TopKSAE``, ``BatchTopKSAE``, ``ReLUSAE``, transcoders, crosscoders with
    ``layer=``) or ``[H, D]`` device tensors.  ``b=None``: ``a`` against itself with ``exclude_self=True``.
    ``which``: decoder directions (default) or encoder rows.  ``metric``: ``"cosine"`` or ``"dot"``; ``precision``:
    ``"fp32"`` or ``"bf16"`` operands of the contraction (fp32 accumulation in both)."""
    if metric not in _METRICS:
        raise ValueError(f"metric must be one of {sorted(_METRICS)}, got {metric!r}")
    if precision not in _PRECISIONS:
        raise ValueError(f"precision must be one of {sorted(_PRECISIONS)}, got {precision!r}")
    if not 1 <= int(n) <= N.MATCH_MAX_N:
        raise ValueError(f"n must be in 1..{N.MATCH_MAX_N}, got {n}")
    ra = _rows(a, which, layer)
    if b is None:
        rb = ra
        if exclude_self is None:
            exclude_self = True
    else:
        rb = _rows(b, which, layer)
    if ra.shape[1] != rb.shape[1]:
        raise ValueError(f"the dictionaries have different widths: {ra.shape[1]} and {rb.shape[1]}")
    if ra.device != rb.device:
        raise N.WsaeError(f"the dictionaries are on different devices: {ra.device} and {rb.device}")
    lib = N.lib()
    ha, hb, dim, n = ra.shape[0], rb.shape[0], ra.shape[1], int(n)
    prec = _PRECISIONS[precision]
    need = int(lib.wsae_match_workspace_bytes(ha, hb, dim, n, prec))
    if need < 0:
        raise N.WsaeError(f"wsae_match_rows does not take [{ha}, {dim}] x [{hb}, {dim}] (width a multiple of 32, <= 2048)")
    with torch.cuda.device(ra.device):
        ws = torch.empty(need, dtype=torch.uint8, device=ra.device)
        values = torch.empty(ha, n, dtype=torch.float32, device=ra.device)
        indices = torch.empty(ha, n, dtype=torch.int32, device=ra.device)
        N.check(lib.wsae_match_rows(ra.data_ptr(), ha, ra.stride(0), rb.data_ptr(), hb, rb.stride(0), dim, _METRICS[metric],
                                    prec, n, 1 if exclude_self else 0, values.data_ptr(), indices.data_ptr(),
                                    ws.data_ptr(), need, torch.cuda.current_stream(ra.device).cuda_stream),
                "wsae_match_rows")
    return NearestFeatures(values, indices)


def _side(best: Tensor, thresholds) -> dict:
    return {"mmcs": float(best.mean()),
            "fraction_at_least": {str(float(t)): float((best >= float(t)).float().mean()) for t in thresholds},
            "histogram": {"lo": -1.0, "hi": 1.0,
                          "counts": [int(c) for c in torch.histc(best.clamp(-1.0, 1.0), bins=20, min=-1.0, max=1.0).cpu()]}}


def compare_dictionaries(a, b, *, which: str = "decoder", precision: str = "fp32", thresholds=(0.5, 0.7, 0.9),
                         layer: Optional[int] = None) -> dict:
    """Summary of how two dictionaries overlap, as plain JSON: the mean max cosine similarity in both directions, per
    threshold the fraction of each side's features whose best match reaches it, the mutual nearest neighbours (``[i, j]``
    with ``j`` the best match of ``a``'s feature ``i`` and ``i`` the best match of ``b``'s feature ``j``) and a 20-bin
    histogram over ``[-1, 1]`` of the best-match cosine of each side."""
    ab = nearest_features(a, b, n=1, which=which, precision=precision, exclude_self=False, layer=layer)
    ba = nearest_features(b, a, n=1, which=which, precision=precision, exclude_self=False, layer=layer)
    va, ia = ab.values[:, 0], ab.indices[:, 0].long()
    vb, ib = ba.values[:, 0], ba.indices[:, 0].long()
    mutual = ib[ia] == torch.arange(ia.shape[0], device=ia.device)
    mi = torch.nonzero(mutual).flatten()
    sa, sb = _side(va, thresholds), _side(vb, thresholds)
    return {"which": which, "precision": precision, "features_a": int(va.shape[0]), "features_b": int(vb.shape[0]),
            "mmcs_a_to_b": sa["mmcs"], "mmcs_b_to_a": sb["mmcs"],
            "fraction_at_least": {"a": sa["fraction_at_least"], "b": sb["fraction_at_least"]},
            "mutual_nearest": int(mi.numel()),
            "mutual_pairs": [[int(i), int(j)] for i, j in zip(mi.cpu().tolist(), ia[mi].cpu().tolist())],
            "histogram": {"a": sa["histogram"], "b": sb["histogram"]}}


def duplicate_features(sae, threshold: float = 0.9, which: str = "decoder", n: int = 4, *, precision: str = "fp32",
                       layer: Optional[int] = None) -> List[Tuple[int, int, float]]:
    """Pairs ``(i, j, cos)`` with ``i < j`` of features of one dictionary whose cosine reaches ``threshold``, among each
    feature's ``n`` nearest neighbours; sorted by ``cos`` descending, then ``i``, then ``j``."""
    nf = nearest_features(sae, None, n=n, which=which, precision=precision, layer=layer)
    vals, idx = nf.values.cpu(), nf.indices.cpu()
    rows, cols = torch.nonzero((vals >= float(threshold)) & (idx >= 0), as_tuple=True)
    pairs = {}
    for i, v, j in zip(rows.tolist(), vals[rows, cols].tolist(), idx[rows, cols].tolist()):
        key = (min(i, j), max(i, j))
        pairs[key] = max(v, pairs.get(key, v))  # (the pair may be seen from both sides)
    return sorted(((i, j, v) for (i, j), v in pairs.items()), key=lambda t: (-t[2], t[0], t[1]))
