"""The device plumbing that ``data/`` and ``analysis/`` share: the GPU-only check and the workspace an object keeps."""

from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from . import _native as N


def need_gpu(what: str, dev: Optional[torch.device]) -> torch.device:
    if dev is None:
        if not torch.cuda.is_available():
            raise N.WsaeError(f"{what} needs a GPU: its kernels run on the device and there is no CPU implementation")
        dev = torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise N.WsaeError(f"{what} cannot run on '{dev}': its kernels run on the GPU only")
    N.lib()  # fail loudly when the HIP library is not built
    return dev


def gpu_device(what: str, device) -> torch.device:
    """``need_gpu(what, torch.device(device))`` with a missing index filled in by the current device."""
    dev = need_gpu(what, torch.device(device))
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


def grow(tracker, elems: int, dtype, dev) -> Tensor:
    """``tracker._ws`` with at least ``elems`` elements of ``dtype``."""
    if tracker._ws is None or tracker._ws.numel() < elems:
        tracker._ws = None  # (release before the larger one is taken)
        tracker._ws = torch.empty(elems, dtype=dtype, device=dev)
    return tracker._ws


def workspace(tracker, nbytes: int, dev) -> Tensor:
    """``tracker._ws`` as at least ``nbytes`` bytes (one at least, so that it has an address)."""
    return grow(tracker, max(int(nbytes), 1), torch.uint8, dev)
