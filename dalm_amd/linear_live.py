"""Frozen projections of a PADDED tower call over the live rows only: the wrappers of `dalm_row_partition` / `dalm_linear_live` and
of the two MLP-node forwards `dalm_linear_live_swiglu` / `dalm_linear_live_relu2` (include/dalm_hip.h), the routing predicate the frozen-linear nodes ask, and the tile accounting behind the routing table.

The padded layout keeps every padding row in the GEMM shapes (dalm_amd/live_rows.py); the row-wise kernels skip the rows nothing
depends on, the library GEMMs cannot.  `dalm_linear_live` is the lm_head MFMA main loop with a row gather on its A operand: it
reads a stable partition of the liveness vector on the device (live rows first), walks only the row tiles that hold live rows and
writes zeros (fresh output) or nothing (accumulating) for the others.  Launch shapes, tensor shapes and graph keys do not change.

Routing is by a static table of (rows, N, K) measured with tools/linear_live_bench.py (profiles/linear_live_bench.txt): a shape
goes to the kernel only where it beat the tuned library GEMM at the benchmark's masks.  Everything else - fp32, biased projections,
calls outside a padded tower call, the packed path, unlisted shapes - stays with the library.
"""
from __future__ import annotations

from typing import Iterable, Optional, Tuple

import torch

from . import hip

# (rows, N, K) of C[rows, N] = A[rows, K] . W[N, K]^T that go to the kernel - forward and dgrad shapes alike.  From
# profiles/linear_live_bench.txt (cfg3 padded step, 4608 generator rows); DESIGN.md "Live-row GEMM" lists what stayed out and why.
ROUTED_SHAPES = frozenset({
    (4608, 22016, 4096),     # gate | up forward
    (4608, 4096, 11008),     # down forward; gate and up dgrad (accumulated)
    (4608, 11008, 4096),     # down dgrad
    (4608, 32000, 4096),     # lm_head forward (materialised logits)
    (4608, 4096, 32000),     # lm_head dgrad
})
# Not listed: (4608, 4096, 4096) (o_proj both ways, the members of the q | k | v dgrad) and (4608, 12288, 4096) (q | k | v forward) -
# the kernel is faster there too, but not by three spreads of the library arm at every mask in every run of the bench.
# Not listed either: AFM-4.5B's MLP shapes (tools/linear_live_bench.py --candidates, profiles/arcee_bench.txt).  (4608, 2560, 18432) -
# 180 tiles on 256 CUs - loses to the library at every mask; (4608, 18432, 2560) wins, but over a library arm that was never tuned at
# that shape.  The ReLU^2 MLP node needs both, so it routes under `set_table` only.

_enabled = True
_mlp_fused = True
_table = ROUTED_SHAPES
_calls = 0


def set_enabled(on: bool) -> None:
    """Turn the route on or off (A/B tools, tests); off = every frozen projection runs in the library, as before."""
    global _enabled
    _enabled = bool(on)


def enabled() -> bool:
    return _enabled


def set_mlp_fused(on: bool) -> None:
    """Turn the fused frozen-MLP nodes (SwiGLU, ReLU^2) on or off (A/B tools, tests); off = the projections and the activation
    kernels run as separate nodes, as before.  A function, not an environment variable: same bits either way, nothing a deployment selects."""
    global _mlp_fused
    _mlp_fused = bool(on)


def mlp_fused() -> bool:
    return _mlp_fused


def set_table(shapes: Optional[Iterable[Tuple[int, int, int]]]) -> None:
    """Replace the routing table ((rows, N, K) triples); None restores the measured one.  For tests at small shapes."""
    global _table
    _table = ROUTED_SHAPES if shapes is None else frozenset(tuple(int(v) for v in s) for s in shapes)


def calls() -> int:
    """How many times `linear_live` has launched the kernel in this process."""
    return _calls


def shape_ok(rows: int, n: int, k: int) -> bool:
    """What the kernel accepts at all (include/dalm_hip.h)."""
    return rows > 0 and n > 0 and k > 0 and k % 64 == 0 and n % 8 == 0


def routed(rows: int, n: int, k: int, dtype: torch.dtype, has_bias: bool, have_partition: bool) -> bool:
    """The routing predicate: bf16 compute, no bias, a partition that describes the rows, and a shape in the table."""
    return (_enabled and have_partition and not has_bias and dtype == torch.bfloat16 and shape_ok(rows, n, k)
            and (rows, n, k) in _table)


_mlp_prepared: set = set()


def mlp_prepare(device) -> bool:
    """Fill the forward epilogue's silu table on `device` (once; synchronises the current stream).  False while a stream capture is
    in progress and the table is not there yet: the caller keeps the unfused kernels for this call."""
    device = torch.device(device)
    if device in _mlp_prepared:
        return True
    if torch.cuda.is_current_stream_capturing():
        return False
    with torch.cuda.device(device):
        hip.call("dalm_linear_live_swiglu_prepare", hip.stream())
    _mlp_prepared.add(device)
    return True


def mlp_routed(rows: int, c: int, h: int, dtype: torch.dtype, has_bias: bool, have_partition: bool) -> bool:
    """The frozen SwiGLU MLP (hidden h, intermediate c) as ONE node around `linear_live_swiglu`: the switch, 128-column mixed
    tiles, and ALL four GEMM shapes of the node in the table - gate | up forward, down forward, down dgrad, gate and up dgrad (the
    last two share one shape)."""
    if not (_mlp_fused and c > 0 and c % 128 == 0):
        return False
    return all(routed(rows, n, k, dtype, has_bias, have_partition) for n, k in ((2 * c, h), (h, c), (c, h)))


def relu2_mlp_routed(rows: int, c: int, h: int, dtype: torch.dtype, has_bias: bool, have_partition: bool) -> bool:
    """The frozen ReLU^2 MLP (Arcee: hidden h, intermediate c, no gate) as ONE node around `linear_live_relu2`: `mlp_routed`'s
    switches and BOTH GEMM shapes of the node in the table - (rows, c, h): up forward and down dgrad, (rows, h, c): down forward and
    up dgrad."""
    if not (_mlp_fused and c > 0):
        return False
    return all(routed(rows, n, k, dtype, has_bias, have_partition) for n, k in ((c, h), (h, c)))


def _operand_ok(t: torch.Tensor) -> bool:
    return (t.dim() == 2 and t.dtype == torch.bfloat16 and t.is_cuda and t.stride(1) == 1 and t.stride(0) % 8 == 0
            and t.stride(0) >= t.shape[1] and t.data_ptr() % 16 == 0)


def accepts(x2: torch.Tensor, w: torch.Tensor, has_bias: bool) -> bool:
    """`x2 [rows, K] . w [N, K]^T` goes to the kernel once a partition of its rows is at hand: the predicate on these tensors."""
    if w.dim() != 2 or x2.dim() != 2 or w.dtype != x2.dtype:
        return False
    rows, (n, k) = x2.shape[0], w.shape
    if not routed(rows, n, k, x2.dtype, has_bias, True):
        return False
    return _operand_ok(x2) and w.is_contiguous() and w.data_ptr() % 16 == 0 and w.device == x2.device


def route(x2: torch.Tensor, w: torch.Tensor, has_bias: bool):
    """Forward: the partition of the tower call in progress to run `x2 . w^T` with, or None when the call stays with the library.
    (A backward runs after the tower call's context: it asks `accepts` and uses the partition its forward kept.)"""
    if not accepts(x2, w, has_bias):
        return None
    from . import live_rows

    return live_rows.current_partition(x2.shape[0], x2.device)


def row_partition(live: torch.Tensor):
    """uint8 [R] -> (perm int32 [R], n_live int32 [1]) on the device: live rows first, ascending, then the dead ones."""
    hip.require_gpu(live)
    if live.dtype != torch.uint8 or live.dim() != 1 or not live.is_contiguous():
        raise TypeError("row_partition: a contiguous uint8 vector expected")
    perm = torch.empty(live.numel(), dtype=torch.int32, device=live.device)
    n_live = torch.empty(1, dtype=torch.int32, device=live.device)
    with torch.cuda.device(live.device):
        hip.call("dalm_row_partition", hip.ptr(live), live.numel(), hip.ptr(perm), hip.ptr(n_live), hip.stream())
    return perm, n_live


def partition_reference(live) -> Tuple[list, int]:
    """Host reference of `row_partition` for any sequence of truth values."""
    flags = [bool(v) for v in live]
    alive = [i for i, f in enumerate(flags) if f]
    return alive + [i for i, f in enumerate(flags) if not f], len(alive)


def linear_live(a: torch.Tensor, w: torch.Tensor, part, out: Optional[torch.Tensor] = None,
                accumulate: bool = False) -> torch.Tensor:
    """out[perm[i]] (+)= a[perm[i]] . w^T for the live rows of `part` = (perm, n_live); a [R, K] and out [R, N] may be column
    views (row strides multiples of 8), w [N, K] contiguous, all bf16.  Fresh output: dead rows are zeros."""
    global _calls
    perm, n_live = part
    hip.require_gpu(a, w, perm, n_live)
    rows, k = a.shape
    n = w.shape[0]
    if out is None:
        if accumulate:
            raise ValueError("linear_live: accumulate needs the output to add to")
        out = torch.empty((rows, n), dtype=torch.bfloat16, device=a.device)
    if not (_operand_ok(a) and _operand_ok(out) and w.dtype == torch.bfloat16 and w.is_contiguous()):
        raise TypeError("linear_live: bf16 operands with unit column stride expected (w contiguous)")
    if w.shape[1] != k or out.shape != (rows, n) or perm.numel() != rows or perm.dtype != torch.int32 or n_live.dtype != torch.int32:
        raise ValueError("linear_live: inconsistent shapes")
    with torch.cuda.device(a.device):
        hip.call("dalm_linear_live", hip.ptr(a), a.stride(0), hip.ptr(w), hip.ptr(out), out.stride(0), rows, n, k, hip.ptr(perm),
                 hip.ptr(n_live), int(bool(accumulate)), hip.stream())
    _calls += 1
    return out


def _check_part(part, rows: int):
    perm, n_live = part
    if perm.numel() != rows or perm.dtype != torch.int32 or n_live.dtype != torch.int32:
        raise ValueError("linear_live: the partition does not describe these rows")
    return perm, n_live


def linear_live_swiglu(a: torch.Tensor, wcat: torch.Tensor, part):
    """(y, act) for the live rows of `part`: y[r] = a[r] . wcat^T with wcat = [Wgate; Wup] [2C, K], act[r] = silu(y[r, :C]) * y[r, C:]
    - the bits of `linear_live` followed by `dalm_swiglu_fwd_2d_live`.  Dead rows of BOTH outputs are NOT written (torch.empty):
    the buffers are meant to stay inside one autograd node."""
    global _calls
    rows, k = a.shape
    c = wcat.shape[0] // 2
    perm, n_live = _check_part(part, rows)
    hip.require_gpu(a, wcat, perm, n_live)
    if not mlp_prepare(a.device):
        raise RuntimeError("linear_live_swiglu: first use on this device inside a stream capture (call linear_live.mlp_prepare before)")
    if not (_operand_ok(a) and wcat.dtype == torch.bfloat16 and wcat.is_contiguous()) or wcat.shape != (2 * c, k):
        raise TypeError("linear_live_swiglu: bf16 a [R, K] with unit column stride and contiguous wcat [2C, K] expected")
    y = torch.empty((rows, 2 * c), dtype=torch.bfloat16, device=a.device)
    act = torch.empty((rows, c), dtype=torch.bfloat16, device=a.device)
    with torch.cuda.device(a.device):
        hip.call("dalm_linear_live_swiglu", hip.ptr(a), a.stride(0), hip.ptr(wcat), hip.ptr(y), 2 * c, hip.ptr(act), c, rows, c, k,
                 hip.ptr(perm), hip.ptr(n_live), hip.stream())
    _calls += 1
    return y, act


def linear_live_relu2(a: torch.Tensor, w_up: torch.Tensor, part):
    """(y, act) for the live rows of `part`: y[r] = a[r] . w_up^T (w_up [C, K] contiguous), act[r] = relu(y[r])^2 - the bits of
    `linear_live` followed by `dalm_relu2_fwd`.  Dead rows of BOTH outputs are NOT written (torch.empty): the buffers are meant to
    stay inside one autograd node."""
    global _calls
    rows, k = a.shape
    perm, n_live = _check_part(part, rows)
    hip.require_gpu(a, w_up, perm, n_live)
    if not (_operand_ok(a) and w_up.dim() == 2 and w_up.dtype == torch.bfloat16 and w_up.is_contiguous()) or w_up.shape[1] != k:
        raise TypeError("linear_live_relu2: bf16 a [R, K] with unit column stride and contiguous w_up [C, K] expected")
    c = w_up.shape[0]
    y = torch.empty((rows, c), dtype=torch.bfloat16, device=a.device)
    act = torch.empty((rows, c), dtype=torch.bfloat16, device=a.device)
    with torch.cuda.device(a.device):
        hip.call("dalm_linear_live_relu2", hip.ptr(a), a.stride(0), hip.ptr(w_up), hip.ptr(y), c, hip.ptr(act), c, rows, c, k,
                 hip.ptr(perm), hip.ptr(n_live), hip.stream())
    _calls += 1
    return y, act


# ---- tile accounting (pure Python: the estimate table of DESIGN.md, and the bench's FLOP column) -------------------------------
CUS = 256


def tiles(rows_live: int, n: int, tile_rows: int = 256, tile_cols: int = 256) -> int:
    """Workgroup tiles that multiply: row tiles holding a live row x column tiles."""
    return -(-rows_live // tile_rows) * -(-n // tile_cols)


def rounds(rows_live: int, n: int, tile_rows: int = 256, cus: int = CUS) -> int:
    """Rounds of one tile per CU the live tiles take."""
    return -(-tiles(rows_live, n, tile_rows) // cus)


def flops(rows_live: int, n: int, k: int) -> int:
    return 2 * rows_live * n * k
