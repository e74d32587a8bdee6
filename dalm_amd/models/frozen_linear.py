"""Frozen projections with a transposed copy of the weight for the backward GEMM.

Under LoRA (the reference's configuration for 7B generators: dalm/models/rag_e2e_base_model.py:61-80) every base projection is
frozen: its backward is one GEMM, dx = g W with W [N, K] as stored - the library's "NN" layout.  hipBLASLt runs that layout
slower than the forward's ("TN"): measured at the cfg3 shapes with the tuned solution table (profiles/r05_gemm_layout_probe.txt)
    q/k/v/o   162.5 us (NN)  ->  148.6 us through a transposed copy (TN), 135.6 us when it accumulates into an existing dx
    down_proj 376.1 us       ->  327.3 us        gate/up_proj 349.6 us -> 334.7 us
A frozen weight never changes, so the copy W^T [K, N] is made once (lazily, on the weight's device; +1x the frozen weights'
bytes - 13.5 GB for Llama-2-7b in bf16, on a 288 GB GPU) and the backward becomes F.linear(g, W^T).  Same values as autograd's
own backward up to the summation order inside the library's kernel.

Nothing in transformers is patched: frozen `nn.Linear` modules get the subclass below by class swap (same parameters, same
state_dict keys); trainable weights, CPU tensors and inference keep `nn.Linear.forward`.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F


def enabled() -> bool:
    return True


import weakref

# the copies live in a side table keyed by the parameter OBJECT's id, not on the parameter: `torch.save(model)` / pickling a
# module does not serialise them, and a parameter that goes away takes its copy with it (a finalizer removes the entry; a
# WeakKeyDictionary cannot hold tensors - its key comparison calls Tensor.__eq__)
_WT_CACHE: dict = {}


def dgrad_weight(w: torch.Tensor, dtype: Optional[torch.dtype] = None) -> Optional[torch.Tensor]:
    """W^T [K, N], contiguous, in `dtype` (default: w's own); None when w is trainable or not on a GPU, when the
    copy would not fit comfortably (free HBM < 4 x its size: the backward then runs on W as stored), or when the first request
    for it comes from inside a hipGraph capture (an allocation that must outlive the graph's pool).  The cache is keyed by the
    weight's storage, version, device and dtype: a reloaded or moved weight gets a fresh copy."""
    if w.requires_grad or not w.is_cuda or w.dim() != 2:
        return None
    dtype = dtype or w.dtype
    key = (w.data_ptr(), w._version, w.device, dtype, tuple(w.shape))
    cached = _WT_CACHE.get(id(w))
    if cached is not None and cached[0] == key and cached[2]() is w:
        return cached[1]
    if torch.cuda.is_current_stream_capturing():
        return None
    need = w.numel() * torch.empty((), dtype=dtype).element_size()
    try:
        free, _total = torch.cuda.mem_get_info(w.device)
        if free < 4 * need:
            return None
    except Exception:
        pass
    with torch.no_grad():
        wt = w.detach().to(dtype).t().contiguous()
    # the copy is made by kernels on THIS stream and then shared through the cache: a backward of the same module running on
    # another stream (the retriever-only step runs its two towers on two streams) would pick it up before it is written - one
    # host sync per weight, once (seen as a wrong first-step gradient at cfg2: 0.62 instead of 0.34)
    torch.cuda.current_stream(w.device).synchronize()
    try:
        fresh = id(w) not in _WT_CACHE
        _WT_CACHE[id(w)] = (key, wt, weakref.ref(w))
        if fresh:
            weakref.finalize(w, _WT_CACHE.pop, id(w), None)
    except TypeError:       # an object that cannot be weakly referenced: recompute next time
        _WT_CACHE.pop(id(w), None)
    return wt


def drop_dgrad_copy(w: torch.Tensor) -> None:
    _WT_CACHE.pop(id(w), None)


def _compute_dtype(x: torch.Tensor) -> torch.dtype:
    return torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled() else x.dtype


# ---------------------------------------------------------------------------------------------------------------------
# padded tower call: the GEMM over the live rows only (dalm_amd/linear_live.py).  `_live_fwd` / `_live_dgrad` return None
# when the call stays with the library - then nothing below differs from what it was.
# ---------------------------------------------------------------------------------------------------------------------
def _live_fwd(x: torch.Tensor, w: torch.Tensor, b):
    """(y, partition) through dalm_linear_live, or None.  bf16 in and out without autocast's casts: x and w already are bf16."""
    from .. import linear_live

    if not linear_live.enabled() or b is not None or x.dtype != torch.bfloat16 or w.dtype != torch.bfloat16:
        return None
    x2 = x.reshape(-1, w.shape[1])
    part = linear_live.route(x2, w, False)
    if part is None:
        return None
    y = linear_live.linear_live(x2, w, part)
    return y.view(*x.shape[:-1], w.shape[0]), part


def _live_dgrad(g2: torch.Tensor, wt, part, dx=None):
    """dx (+)= g2 . wt^T over the live rows (wt = the transposed copy [K, N]), or None when this shape stays with the library."""
    from .. import linear_live

    if part is None or wt is None or part[0].numel() != g2.shape[0] or not linear_live.accepts(g2, wt, False):
        return None
    return linear_live.linear_live(g2, wt, part, out=dx, accumulate=dx is not None)


class _FrozenLinearFn(torch.autograd.Function):
    """y = x W^T + b with W, b frozen: the backward is dx = F.linear(g, W^T copy)."""

    @staticmethod
    def forward(ctx, x, w, b):
        lv = _live_fwd(x, w, b)
        y, ctx.part = lv if lv is not None else (F.linear(x, w, b), None)   # under autocast this casts exactly as nn.Linear.forward does
        ctx.w = w
        ctx.cdt = y.dtype
        ctx.xshape, ctx.xdtype = x.shape, x.dtype
        return y

    @staticmethod
    def backward(ctx, g):
        w = ctx.w
        wt = dgrad_weight(w, ctx.cdt)
        g2 = g.reshape(-1, w.shape[0])
        if g2.dtype != ctx.cdt:
            g2 = g2.to(ctx.cdt)
        dx = _live_dgrad(g2, wt, ctx.part)
        if dx is None:
            dx = F.linear(g2, wt) if wt is not None else torch.mm(g2, w.to(ctx.cdt))
        dx = dx.view(ctx.xshape)
        return (dx if dx.dtype == ctx.xdtype else dx.to(ctx.xdtype)), None, None


class _FrozenPairFn(torch.autograd.Function):
    """(x W0^T, x W1^T) for two frozen bias-free projections of ONE input (gate_proj / up_proj): the two backward GEMMs
    accumulate into one dx - no separate add of two [rows, K] tensors."""

    @staticmethod
    def forward(ctx, x, w0, w1):
        lv0 = _live_fwd(x, w0, None)
        lv1 = _live_fwd(x, w1, None) if lv0 is not None else None
        if lv1 is not None:
            (y0, ctx.part), y1 = lv0, lv1[0]
        else:
            y0, y1, ctx.part = F.linear(x, w0), F.linear(x, w1), None
        ctx.w = (w0, w1)
        ctx.cdt = y0.dtype
        ctx.xshape, ctx.xdtype = x.shape, x.dtype
        ctx.set_materialize_grads(False)
        return y0, y1

    @staticmethod
    def backward(ctx, g0, g1):
        dx = None
        for g, w in zip((g0, g1), ctx.w):
            if g is None:
                continue
            g2 = g.reshape(-1, w.shape[0])              # a view for the column halves of one [rows, 2 N] buffer (row stride 2 N)
            if g2.dtype != ctx.cdt:
                g2 = g2.to(ctx.cdt)
            wt = dgrad_weight(w, ctx.cdt)
            lv = _live_dgrad(g2, wt, ctx.part, dx)           # accumulating: adds into dx in f32, one rounding, as addmm_ does
            if lv is not None:
                dx = lv
            elif dx is None:
                dx = F.linear(g2, wt) if wt is not None else torch.mm(g2, w.to(ctx.cdt))
            elif wt is not None:
                dx.addmm_(g2, wt.t())
            else:
                dx.addmm_(g2, w.to(ctx.cdt))
        if dx is None:
            return None, None, None
        dx = dx.view(ctx.xshape)
        return (dx if dx.dtype == ctx.xdtype else dx.to(ctx.xdtype)), None, None


# ---------------------------------------------------------------------------------------------------------------------
# two frozen projections of one input as ONE forward GEMM: x [W0 | W1]^T
# ---------------------------------------------------------------------------------------------------------------------
_CAT = True            # tests clear it to build their two-GEMM reference


def _cat_weights(*mods: torch.nn.Linear) -> Optional[torch.Tensor]:
    """[W0; W1; ...] as ONE contiguous [N0 + N1 + ..., K] tensor that the modules' weights are VIEWS of (no second copy of the
    weights: the parameters are re-pointed at the row blocks, state_dict keys and values unchanged).  Two members for gate | up,
    three for q | k | v; the N may differ (grouped-query k / v).  Made on first use; re-made when a parameter was replaced or moved
    (its storage is then no longer the cat's).  None when the members cannot share (devices, dtypes, K, trainable, not on a GPU).

    Why: hipBLASLt runs the [rows, K] x [K, N] projections on 256 x 256 tiles; one GEMM over the summed columns fills the last
    wave of tiles better than one GEMM per member (measured, tools/gemm_concat_probe.py: gate | up forward 672 -> 621 us at 4608
    rows, 493 -> 425 us at 2944 packed rows; q | k | v 408 -> 355 us at 4608 rows)."""
    ws = [m.weight for m in mods]
    w0 = ws[0]
    if not _CAT or len(ws) < 2 or not w0.is_cuda or w0.dim() != 2:
        return None
    for w in ws:
        if w.requires_grad or w.device != w0.device or w.dtype != w0.dtype or w.dim() != 2 or w.shape[1] != w0.shape[1]:
            return None
    cat = getattr(mods[0], "_dalm_cat", None)
    el, K = w0.element_size(), w0.shape[1]
    if cat is not None and cat.dtype == w0.dtype and cat.shape == (sum(w.shape[0] for w in ws), K):
        off, ok = cat.data_ptr(), True
        for w in ws:
            ok = ok and w.data_ptr() == off and w.is_contiguous()
            off += w.shape[0] * K * el
        if ok:
            return cat
    if torch.cuda.is_current_stream_capturing():
        return None                            # never re-point parameters inside a hipGraph capture
    with torch.no_grad():
        cat = torch.cat([w.detach() for w in ws], dim=0)
        torch.cuda.current_stream(w0.device).synchronize()      # other streams may run these modules next (see dgrad_weight)
        n0 = 0
        for w in ws:
            w.data = cat[n0:n0 + w.shape[0]]
            n0 += w.shape[0]
    for w in ws:                               # transposed dgrad copies made from the old storage are still VALUES-correct, but
        drop_dgrad_copy(w)                     # keyed by pointer: drop them, they are rebuilt on the next backward
    try:
        mods[0]._dalm_cat = cat
    except Exception:
        return None
    return cat


def _cat_biases(*mods: torch.nn.Linear) -> Optional[torch.Tensor]:
    """[b0; b1; ...] as ONE [N0 + N1 + ...] vector the modules' (frozen) biases are views of: the bias of the one GEMM over
    `_cat_weights(*mods)`.  Same rules as there; None when a member has no bias or the biases cannot share."""
    bs = [m.bias for m in mods]
    if not _CAT or any(b is None for b in bs):
        return None
    b0 = bs[0]
    for b in bs:
        if b.requires_grad or not b.is_cuda or b.device != b0.device or b.dtype != b0.dtype or b.dim() != 1:
            return None
    cat = getattr(mods[0], "_dalm_cat_bias", None)
    if cat is not None and cat.dtype == b0.dtype and cat.numel() == sum(b.numel() for b in bs):
        off, ok = cat.data_ptr(), True
        for b in bs:
            ok = ok and b.data_ptr() == off and b.is_contiguous()
            off += b.numel() * b.element_size()
        if ok:
            return cat
    if torch.cuda.is_current_stream_capturing():
        return None
    with torch.no_grad():
        cat = torch.cat([b.detach() for b in bs], dim=0)
        torch.cuda.current_stream(b0.device).synchronize()
        n0 = 0
        for b in bs:
            b.data = cat[n0:n0 + b.numel()]
            n0 += b.numel()
    try:
        mods[0]._dalm_cat_bias = cat
    except Exception:
        return None
    return cat


def uncat_weights(model: torch.nn.Module) -> int:
    """Give every projection group that shares ONE concatenated weight tensor (`_cat_weights`, and `_cat_biases` with it) its own
    storage again - for callers that serialise whole modules tensor by tensor (`save_pretrained` of a frozen full model:
    safetensors refuses tensors that share memory).  The next eligible forward concatenates again.  Returns how many groups were
    separated."""
    n = 0
    for m in model.modules():
        if getattr(m, "_dalm_cat", None) is None:
            continue
        cats = [(m._dalm_cat, "weight", 2)]
        if getattr(m, "_dalm_cat_bias", None) is not None:
            cats.append((m._dalm_cat_bias, "bias", 1))
        for cat, attr, dim in cats:
            for other in model.modules():
                w = getattr(other, attr, None)
                if isinstance(w, torch.Tensor) and w.dim() == dim and w.untyped_storage().data_ptr() == cat.untyped_storage().data_ptr():
                    with torch.no_grad():
                        w.data = w.detach().clone()
                    if dim == 2:
                        drop_dgrad_copy(w)
        drop_dgrad_copy(m._dalm_cat)
        for a in ("_dalm_cat", "_dalm_cat_bias"):
            if hasattr(m, a):
                try:
                    delattr(m, a)
                except Exception:
                    setattr(m, a, None)
        n += 1
    return n


class _FrozenCatPairFn(torch.autograd.Function):
    """(x W0^T, x W1^T) as the two column halves of ONE GEMM output x [W0; W1]^T; backward: the two accumulating dgrad GEMMs of
    `_FrozenPairFn` (one GEMM over the 2 N-deep contraction measured slower at 4608 rows, tools/gemm_concat_probe.py), reading the
    gradient halves in place when they arrive as the halves of one buffer (tower_ops._SwiGLU does that)."""

    @staticmethod
    def forward(ctx, x, cat, w0, w1):
        lv = _live_fwd(x, cat, None)
        y, ctx.part = lv if lv is not None else (F.linear(x, cat), None)
        n0 = w0.shape[0]
        ctx.w = (w0, w1)
        ctx.cdt = y.dtype
        ctx.xshape, ctx.xdtype = x.shape, x.dtype
        ctx.set_materialize_grads(False)
        return y[..., :n0], y[..., n0:]

    @staticmethod
    def backward(ctx, g0, g1):
        return _FrozenPairFn.backward(ctx, g0, g1) + (None,)


class _FrozenSwigluMlpFn(torch.autograd.Function):
    """down(silu(gate(x)) * up(x)) with all three projections frozen, inside a padded tower call, as ONE node: the SwiGLU forward
    runs in the epilogue of the gate | up GEMM (dalm_amd/linear_live.py); the backward runs the down dgrad GEMM and the row-wise
    SwiGLU backward kernel as two launches (an epilogue form of the pair measured slower: DESIGN.md 5.7.1).
    y = [gate | up], act, d_gate and d_up never leave the node, so their dead rows are never written - nobody reads them: every
    consumer is a live-row GEMM whose A gather skips them.  The output and dx leave the node and keep zeros in their dead rows.
    Same bits as the separate nodes: same contraction order, same element arithmetic (csrc/swiglu_math.hpp)."""

    @staticmethod
    def forward(ctx, x, cat, w0, w1, wd, part):
        from .. import linear_live, live_rows

        x2 = x.reshape(-1, cat.shape[1])
        y, act = linear_live.linear_live_swiglu(x2, cat, part)
        out = linear_live.linear_live(act, wd, part)            # leaves the node: zeros for the dead rows
        ctx.save_for_backward(y)                                # act is not needed again: every weight is frozen
        ctx.part, ctx.w, ctx.wd = part, (w0, w1), wd
        ctx.live = live_rows.current(x2.shape[0], x2.device)    # the vector behind `part`, for the row-wise backward kernel
        ctx.xshape = x.shape
        return out.view(*x.shape[:-1], wd.shape[0])

    @staticmethod
    def backward(ctx, g):
        from .. import hip, linear_live

        (y,) = ctx.saved_tensors
        w0, w1 = ctx.w
        part = ctx.part
        g2 = g.reshape(-1, ctx.wd.shape[0])
        if g2.dtype != torch.bfloat16:
            g2 = g2.to(torch.bfloat16)
        if g2.stride(-1) != 1 or g2.stride(0) % 8 or g2.data_ptr() % 16:
            g2 = g2.contiguous()
        wdt, wt0, wt1 = (dgrad_weight(w, torch.bfloat16) for w in (ctx.wd, w0, w1))
        if wdt is not None and wt0 is not None and wt1 is not None:
            # two launches: a SwiGLU backward inside the down dgrad's epilogue measured slower than this pair
            c = w0.shape[0]
            d_act = linear_live.linear_live(g2, wdt, part)
            dg, du = torch.empty_like(d_act), torch.empty_like(d_act)
            hip.call("dalm_swiglu_bwd_2d_live", hip.ptr(d_act), hip.ptr(y), hip.ptr(y[:, c:]), hip.ptr(dg), hip.ptr(du),
                     hip.dtype_code(y), y.shape[0], c, c, 2 * c, 2 * c, c, c, hip.ptr(ctx.live), hip.stream())
            dx = linear_live.linear_live(dg, wt0, part)                     # as _FrozenPairFn.backward: fresh, zeros for dead rows,
            dx = linear_live.linear_live(du, wt1, part, out=dx, accumulate=True)    # then accumulated in f32 with one rounding
            return dx.view(ctx.xshape), None, None, None, None, None
        raise RuntimeError("frozen SwiGLU MLP node: the transposed dgrad copies of its weights are missing (make them outside a "
                           "graph capture: frozen_linear.dgrad_weight)")


def swiglu_mlp_candidate(x: torch.Tensor, gate_proj, up_proj, down_proj):
    """The part of the routing predicate that needs no device (meta tensors will do): (rows, C, H) when the switches are on, the
    three projections are plain, bias-free, frozen and bf16 like x, the shapes are those of one gated MLP, C % 128 == 0 and all
    four GEMM shapes of the node are in linear_live's table; else None."""
    from .. import linear_live

    if not (linear_live.enabled() and linear_live.mlp_fused()):
        return None
    plain = (torch.nn.Linear, FrozenLinearT)
    mods = (gate_proj, up_proj, down_proj)
    if any(type(m) not in plain or m.bias is not None or m.weight.requires_grad for m in mods):
        return None
    if x.dtype != torch.bfloat16 or any(m.weight.dtype != torch.bfloat16 or m.weight.dim() != 2 for m in mods):
        return None
    c, h = gate_proj.weight.shape
    if up_proj.weight.shape != (c, h) or down_proj.weight.shape != (h, c) or x.dim() < 2 or x.shape[-1] != h:
        return None
    rows = x.numel() // h
    if not linear_live.mlp_routed(rows, c, h, x.dtype, False, True):
        return None
    return rows, c, h


def swiglu_mlp_route(x: torch.Tensor, gate_proj, up_proj, down_proj):
    """The routing predicate of `swiglu_mlp_forward`: (cat, partition) when the call goes to the fused node, else None."""
    from .. import linear_live

    cand = swiglu_mlp_candidate(x, gate_proj, up_proj, down_proj)
    if cand is None or not _eligible(x, gate_proj, up_proj, down_proj):
        return None
    cat = _cat_weights(gate_proj, up_proj)
    if cat is None:
        return None
    x2 = x.reshape(-1, cand[2])
    wd = down_proj.weight
    if not (linear_live.accepts(x2, cat, False) and wd.is_contiguous() and wd.data_ptr() % 16 == 0 and wd.device == x.device):
        return None
    part = linear_live.route(x2, cat, False)             # None outside a padded tower call
    if part is None:
        return None
    if not linear_live.mlp_prepare(x.device):            # the forward epilogue's silu table: not inside a capture the first time
        return None
    # the backward needs the three transposed copies; a first request from inside a graph capture cannot make them
    if any(dgrad_weight(m.weight, torch.bfloat16) is None for m in (gate_proj, up_proj, down_proj)):
        return None
    return cat, part


def swiglu_mlp_forward(x: torch.Tensor, gate_proj, up_proj, down_proj):
    """down_proj(silu(gate_proj(x)) * up_proj(x)) through `_FrozenSwigluMlpFn`, or None when the call does not route (the caller then
    runs the separate nodes): linear_live on with a padded tower call in progress and a partition of these rows, bf16, no biases,
    three frozen plain projections whose gate | up weights share one tensor, C % 128 == 0, all four GEMM shapes in linear_live's
    table, and `linear_live.set_mlp_fused` on."""
    r = swiglu_mlp_route(x, gate_proj, up_proj, down_proj)
    if r is None:
        return None
    cat, part = r
    return _FrozenSwigluMlpFn.apply(x, cat, gate_proj.weight, up_proj.weight, down_proj.weight, part)


class _FrozenRelu2MlpFn(torch.autograd.Function):
    """down(relu(up(x))^2) (ArceeMLP) with both projections frozen, inside a padded tower call, as ONE node: relu(y)^2 runs in the
    epilogue of the up GEMM (dalm_amd/linear_live.py); the backward is the down dgrad GEMM, the row-wise ReLU^2 backward kernel and
    the up dgrad GEMM.  y, act and d_y never leave the node, so their dead rows are never written - every consumer is a live-row GEMM
    whose A gather skips them, or the row-wise kernel under the node's liveness vector.  The output and dx leave the node and keep
    zeros in their dead rows.  Same bits as the separate nodes: same contraction order, same element arithmetic
    (csrc/relu2_math.hpp)."""

    @staticmethod
    def forward(ctx, x, wu, wd, part):
        from .. import linear_live, live_rows

        x2 = x.reshape(-1, wu.shape[1])
        y, act = linear_live.linear_live_relu2(x2, wu, part)
        out = linear_live.linear_live(act, wd, part)            # leaves the node: zeros for the dead rows
        ctx.save_for_backward(y)                                # act is not needed again: every weight is frozen
        ctx.part, ctx.wu, ctx.wd = part, wu, wd
        ctx.live = live_rows.current(x2.shape[0], x2.device)    # the vector behind `part`, for the row-wise backward kernel
        ctx.xshape = x.shape
        return out.view(*x.shape[:-1], wd.shape[0])

    @staticmethod
    def backward(ctx, g):
        from .. import hip, linear_live

        (y,) = ctx.saved_tensors
        part = ctx.part
        g2 = g.reshape(-1, ctx.wd.shape[0])
        if g2.dtype != torch.bfloat16:
            g2 = g2.to(torch.bfloat16)
        if g2.stride(-1) != 1 or g2.stride(0) % 8 or g2.data_ptr() % 16:
            g2 = g2.contiguous()
        wdt, wut = (dgrad_weight(w, torch.bfloat16) for w in (ctx.wd, ctx.wu))
        if wdt is None or wut is None:
            raise RuntimeError("frozen ReLU^2 MLP node: the transposed dgrad copies of its weights are missing (make them outside a "
                               "graph capture: frozen_linear.dgrad_weight)")
        rows, c = y.shape
        d_act = linear_live.linear_live(g2, wdt, part)
        dy = torch.empty_like(d_act)
        hip.call("dalm_relu2_bwd", hip.ptr(d_act), hip.ptr(y), hip.ptr(dy), hip.dtype_code(y), rows, c, c, c, c, hip.ptr(ctx.live),
                 hip.stream())
        dx = linear_live.linear_live(dy, wut, part)             # fresh: zeros for the dead rows
        return dx.view(ctx.xshape), None, None, None


def relu2_mlp_candidate(x: torch.Tensor, up_proj, down_proj):
    """The part of the routing predicate that needs no device (meta tensors will do): (rows, C, H) when the switches are on, the two
    projections are plain, bias-free, frozen and bf16 like x, the shapes are those of one ungated MLP and both GEMM shapes of the
    node are in linear_live's table; else None."""
    from .. import linear_live

    if not (linear_live.enabled() and linear_live.mlp_fused()):
        return None
    plain = (torch.nn.Linear, FrozenLinearT)
    mods = (up_proj, down_proj)
    if any(type(m) not in plain or m.bias is not None or m.weight.requires_grad for m in mods):
        return None
    if x.dtype != torch.bfloat16 or any(m.weight.dtype != torch.bfloat16 or m.weight.dim() != 2 for m in mods):
        return None
    c, h = up_proj.weight.shape
    if down_proj.weight.shape != (h, c) or x.dim() < 2 or x.shape[-1] != h:
        return None
    rows = x.numel() // h
    if not linear_live.relu2_mlp_routed(rows, c, h, x.dtype, False, True):
        return None
    return rows, c, h


def relu2_mlp_route(x: torch.Tensor, up_proj, down_proj):
    """The routing predicate of `relu2_mlp_forward`: the partition when the call goes to the fused node, else None."""
    from .. import linear_live

    cand = relu2_mlp_candidate(x, up_proj, down_proj)
    if cand is None or not _eligible(x, up_proj, down_proj):
        return None
    x2 = x.reshape(-1, cand[2])
    wu, wd = up_proj.weight, down_proj.weight
    if not (linear_live.accepts(x2, wu, False) and wd.is_contiguous() and wd.data_ptr() % 16 == 0 and wd.device == x.device):
        return None
    part = linear_live.route(x2, wu, False)              # None outside a padded tower call
    if part is None:
        return None
    # the backward needs the two transposed copies; a first request from inside a graph capture cannot make them
    if any(dgrad_weight(m.weight, torch.bfloat16) is None for m in (up_proj, down_proj)):
        return None
    return part


def relu2_mlp_forward(x: torch.Tensor, up_proj, down_proj):
    """down_proj(relu(up_proj(x))^2) through `_FrozenRelu2MlpFn`, or None when the call does not route (the caller then runs the
    separate nodes): linear_live on with a padded tower call in progress and a partition of these rows, bf16, no biases, two frozen
    plain projections, both GEMM shapes in linear_live's table, and `linear_live.set_mlp_fused` on."""
    part = relu2_mlp_route(x, up_proj, down_proj)
    if part is None:
        return None
    return _FrozenRelu2MlpFn.apply(x, up_proj.weight, down_proj.weight, part)


def _eligible(x: torch.Tensor, *mods) -> bool:
    if not (x.is_cuda and torch.is_grad_enabled() and x.requires_grad):
        return False
    cdt = _compute_dtype(x)
    if cdt not in (torch.bfloat16, torch.float16, torch.float32):
        return False
    for m in mods:
        if m.weight.requires_grad or (m.bias is not None and m.bias.requires_grad) or not m.weight.is_cuda:
            return False
    return True


class FrozenLinearT(torch.nn.Linear):
    """nn.Linear whose backward uses the transposed copy while the layer is frozen."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if _eligible(x, self):
            from .bert_ops import twin

            return _FrozenLinearFn.apply(twin(x), self.weight, self.bias)       # an f32 LayerNorm output carrying its bf16 copy
        return super().forward(x)


def pair_forward(x: torch.Tensor, m0: torch.nn.Linear, m1: torch.nn.Linear):
    """(m0(x), m1(x)); one autograd node with an accumulating backward when both are frozen and bias-free."""
    plain = (torch.nn.Linear, FrozenLinearT)
    if m0.bias is None and m1.bias is None and type(m0) in plain and type(m1) in plain and _eligible(x, m0, m1):
        cat = _cat_weights(m0, m1)
        if cat is not None:
            return _FrozenCatPairFn.apply(x, cat, m0.weight, m1.weight)
        return _FrozenPairFn.apply(x, m0.weight, m1.weight)
    return m0(x), m1(x)


def _is_plain_linear(m: torch.nn.Module) -> bool:
    # nn.Linear itself, or Falcon's FalconLinear (y = x W^T + b spelled as a matmul: the same function)
    return type(m) is torch.nn.Linear or (isinstance(m, torch.nn.Linear) and type(m).__name__ == "FalconLinear")


def use_transposed_dgrad(model: torch.nn.Module) -> int:
    """Class-swap the FROZEN plain `nn.Linear` modules of `model` to FrozenLinearT (a model that is fine-tuned in full is left
    alone; the forward still checks per call that the layer is frozen); returns how many were swapped.  LoRA-wrapped projections
    and their siblings keep their own modules: the LoRA group node (models/lora_ops.py) asks `dgrad_weight` itself."""
    n = 0
    for name, m in model.named_modules():
        if not _is_plain_linear(m) or name.endswith("base_layer"):              # LoRALinear.base_layer: the group node's business
            continue
        if m.weight.requires_grad or (m.bias is not None and m.bias.requires_grad):
            continue
        m.__class__ = FrozenLinearT
        n += 1
    return n
