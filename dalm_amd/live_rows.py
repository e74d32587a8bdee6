"""Row liveness of a PADDED tower call: which rows of the [B T, H] activations the loss and the gradients depend on.

The padded layout pushes every padding position through both towers, and padding contributes exactly zero to the loss and to
every gradient (dalm_amd/packed.py states why and which rows matter: generator row (b, t) iff mask[b, t] or mask[b, t + 1],
retriever row iff mask[b, t] - or t = T - 1 for a causal-LM retriever, which pools that column).  The packed path removes those rows; the padded path keeps the layout - GEMM shapes, graph sets -
and lets the hand-written row-wise kernels skip them instead: every `dalm_*_live` entry point takes the uint8 vector built
here (include/dalm_hip.h: a dead row is not read, freshly written outputs hold zeros there, live rows get the same bits).

The vector is built ON THE DEVICE from the attention mask (no host sync, no change of shape; inside a tower graph it is
recomputed from the graph's static mask input on every replay) and held for the duration of ONE tower call by `tower_call`;
the op wrappers (tower_ops, lora_ops, bert_ops) read it in their forward with `current(rows)` and keep it for their backward.
Nothing outside a training step enters the context: a module called directly gets None and the plain kernels.

The frozen-projection GEMMs of the padded step (dalm_amd/linear_live.py) want the same information as a stable PARTITION of the
rows - live rows first - plus the live count, both on the device: `current_partition(rows, device)` builds it from the vector with
one launch of `dalm_row_partition`, on the first request inside a tower call (a tower whose projections never route never pays
for it), and holds it beside the vector; inside a tower graph that launch is part of the graph, so the partition too is
recomputed from the static mask on every replay.  The nodes keep it for their backward as they keep the vector.
"""
from __future__ import annotations

import contextlib
import threading
from typing import Optional

import torch

_state = threading.local()


def live_rows(attention_mask: torch.Tensor, shifted: bool, last_column: bool = False) -> torch.Tensor:
    """attention_mask [B, T] -> uint8 [B T], non-zero = the row matters.  shifted=True (generator): a row also matters when the
    NEXT column is live (it carries that token's label) - the `keep` of `packed.pack_plan`; shifted=False (retriever): live.
    last_column=True (causal-LM retriever): column T - 1 matters whatever the mask says - it is the pooled one (`eos_mask`), on a
    right-padded row too."""
    keep = attention_mask != 0
    if shifted:
        keep = keep.clone()
        keep[:, :-1] |= attention_mask[:, 1:] != 0
    if last_column:
        keep = keep.clone()
        keep[:, -1] = True
    return keep.contiguous().view(torch.uint8).reshape(-1)


@contextlib.contextmanager
def tower_call(attention_mask: Optional[torch.Tensor], shifted: bool, enabled: bool = True, last_column: bool = False):
    """Hold the liveness vector of `attention_mask` while one padded tower call runs (forward only: the wrappers save it)."""
    vec = None
    if enabled and attention_mask is not None and attention_mask.dim() == 2 and attention_mask.is_cuda:
        vec = live_rows(attention_mask, shifted, last_column)
    prev, prev_part = getattr(_state, "vec", None), getattr(_state, "part", None)
    _state.vec, _state.part = vec, None
    try:
        yield vec
    finally:
        _state.vec, _state.part = prev, prev_part


def current(rows: int, device=None) -> Optional[torch.Tensor]:
    """The vector of the tower call in progress when it describes `rows` rows (on `device`), else None (= every row matters)."""
    vec = getattr(_state, "vec", None)
    if vec is None or vec.numel() != rows or (device is not None and vec.device != device):
        return None
    return vec


def current_partition(rows: int, device=None):
    """(perm int32 [rows], n_live int32 [1]) of the tower call in progress - `current(rows, device)` as a stable partition, live
    rows first (dalm_amd/linear_live.py) - or None where `current` gives None."""
    vec = current(rows, device)
    if vec is None:
        return None
    part = getattr(_state, "part", None)
    if part is None:
        from . import linear_live

        part = _state.part = linear_live.row_partition(vec)
    return part
