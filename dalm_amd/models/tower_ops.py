"""Autograd wrappers of `dalm_rope_qk` / `dalm_swiglu_{fwd,bwd}` (dalm_amd/csrc/tower.hip): the rotary embedding of q and k
and the SwiGLU activation of a Llama-family decoder layer as ONE HIP launch per direction each.

transformers evaluates both as chains of eager elementwise ops (modeling_llama.py `apply_rotary_pos_emb`,
`LlamaMLP.forward`; the reference reaches them through `self.generator_model(...)`,
dalm/models/rag_e2e_base_model.py:104-106).  The kernels round where those chains round, so forward values and gradients
are the eager chain's (tests/test_tower_ops_gpu.py asserts equality, not closeness).

Also here: RMSNorm with the residual add, Qwen3's head norm + rotary, Gemma's GeGLU and (1 + w) RMSNorm (`dalm_geglu_*`,
`dalm_gemma_norm_*`: modeling_gemma.py `GemmaMLP.forward`, `GemmaRMSNorm.forward`), Arcee's ReLU^2 (`dalm_relu2_*`: modeling_arcee.py
`ArceeMLP.forward`), OLMo-2's norm-then-add and row-wide q / k norm + rotary (`dalm_norm_add_*`, `dalm_row_norm_*`: modeling_olmo2.py),
Granite's scaled residual add with and without the norm behind it (`dalm_rms_norm_scaled_*`, `dalm_scale_add`: modeling_granite.py
`GraniteDecoderLayer.forward`), Cohere's interleaved f32 rotary embedding, f32 LayerNorm and three-way add (`dalm_rope_il_qk`,
`dalm_cohere_norm_*`, `dalm_add3_live`: modeling_cohere.py), Phi-3's partial rotary embedding (`dalm_rope_partial_qk`:
modeling_phi3.py `apply_rotary_pos_emb`), and Falcon's layer ops.

GPU tensors only: the callers in `fastpath.py` keep transformers' own code for CPU tensors.
"""
from __future__ import annotations

import ctypes as C

import torch

from .. import hip, live_rows


def _strides3(t: torch.Tensor):
    return (C.c_int64 * 3)(t.stride(0), t.stride(1), t.stride(2))


def _rope_launch(q, k, cos, sin, backward: bool, live=None):
    """q, k: [B, H, T, hd] (any b/h/t strides, contiguous last dim); cos, sin: [B or 1, T, hd]; live: uint8 [B T] or None
    (dalm_amd/live_rows.py: a dead (b, t) is not read and leaves as zeros for every head)."""
    hip.require_gpu(q, k, cos, sin)
    if q.stride(-1) != 1:
        q = q.contiguous()
    if k.stride(-1) != 1:
        k = k.contiguous()
    qo, ko = torch.empty_like(q), torch.empty_like(k)       # preserve_format: same strides as the (dense) views
    if qo.stride(-1) != 1 or ko.stride(-1) != 1:            # overlapping / exotic input layout: plain contiguous outputs
        qo = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        ko = torch.empty(k.shape, dtype=k.dtype, device=k.device)
    B, Hq, T, hd = q.shape
    Hk = k.shape[1]
    cs = (C.c_int64 * 2)(cos.stride(0) if cos.shape[0] > 1 else 0, cos.stride(1))   # [1, T, hd]: one table for the batch
    hip.call("dalm_rope_qk_live", hip.ptr(q), hip.ptr(k), hip.ptr(qo), hip.ptr(ko), hip.ptr(cos), hip.ptr(sin), hip.dtype_code(q),
             B, T, Hq, Hk, hd, _strides3(q), _strides3(k), _strides3(qo), _strides3(ko), cs, int(backward), hip.ptr(live),
             hip.stream())
    return qo, ko


class _RopeQK(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, cos, sin, live=None):
        if live is None and q.dim() == 4:
            live = live_rows.current(q.shape[0] * q.shape[2], q.device)
        ctx.save_for_backward(cos, sin, *([live] if live is not None else []))   # the backward runs after the tower call's context
        return _rope_launch(q, k, cos, sin, False, live)

    @staticmethod
    def backward(ctx, gq, gk):
        cos, sin, *live = ctx.saved_tensors
        dq, dk = _rope_launch(gq, gk, cos, sin, True, live[0] if live else None)
        return dq, dk, None, None, None


def rope_supported(q, k, cos, sin) -> bool:
    return (q.is_cuda and q.dim() == 4 and k.dim() == 4 and cos.dim() == 3 and sin.shape == cos.shape
            and q.dtype in (torch.float32, torch.bfloat16) and k.dtype == q.dtype and cos.dtype == q.dtype
            and sin.dtype == q.dtype and q.shape[-1] % 2 == 0 and k.shape[-1] == q.shape[-1]
            and q.shape[0] == k.shape[0] and q.shape[2] == k.shape[2]
            and cos.shape[0] in (1, q.shape[0]) and cos.shape[1:] == (q.shape[2], q.shape[3]) and cos.stride(-1) == 1
            and sin.stride() == cos.stride()
            and not cos.requires_grad and not sin.requires_grad)


def rope_qk(q, k, cos, sin, live=None):
    """(q*cos + rotate_half(q)*sin, k*cos + rotate_half(k)*sin) with cos / sin broadcast over the head dimension.
    live: uint8 [B T] row liveness; None: that of the tower call in progress (dalm_amd/live_rows.py), if any."""
    return _RopeQK.apply(q, k, cos, sin, live)


def _halves_of_one(gate: torch.Tensor, up: torch.Tensor) -> bool:
    """gate and up are the two column halves of ONE contiguous [R, 2 C] buffer (the output of the concatenated gate | up GEMM,
    frozen_linear.pair_forward)."""
    if gate.dim() < 2 or gate.shape != up.shape or gate.stride() != up.stride() or gate.stride(-1) != 1:
        return False
    C = gate.shape[-1]
    el = gate.element_size()
    lead = 1
    for d in range(gate.dim() - 2, -1, -1):            # rows must be laid out as one [R, 2 C] matrix
        if gate.shape[d] != 1 and gate.stride(d) != 2 * C * lead:
            return False
        lead *= gate.shape[d]
    return up.data_ptr() == gate.data_ptr() + C * el and C % (16 // el) == 0 and gate.data_ptr() % 16 == 0


class _SwiGLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gate, up, live=None):
        hip.require_gpu(gate, up)
        ctx.halves = _halves_of_one(gate, up)
        C = gate.shape[-1] if gate.dim() else 0
        R = gate.numel() // C if C else 0
        if live is None and gate.dim() >= 2:
            live = live_rows.current(R, gate.device)
        if live is not None and (live.numel() != R or C % (16 // gate.element_size())):
            live = None                    # the row-aware kernels walk 16-byte vectors that never cross a row
        keep = [live] if live is not None else []          # the backward runs after the tower call's context
        if ctx.halves:                     # strided views of one [R, 2 C] GEMM output: read in place, no .contiguous() copies
            act = torch.empty(gate.shape, dtype=gate.dtype, device=gate.device)
            hip.call("dalm_swiglu_fwd_2d_live", hip.ptr(gate), hip.ptr(up), hip.ptr(act), hip.dtype_code(gate), R, C, 2 * C, 2 * C, C,
                     hip.ptr(live), hip.stream())
            ctx.save_for_backward(gate, up, *keep)
            return act
        gate, up = gate.contiguous(), up.contiguous()
        act = torch.empty_like(gate)
        if live is not None:
            hip.call("dalm_swiglu_fwd_live", hip.ptr(gate), hip.ptr(up), hip.ptr(act), hip.dtype_code(gate), R, C, hip.ptr(live),
                     hip.stream())
        else:
            hip.call("dalm_swiglu_fwd", hip.ptr(gate), hip.ptr(up), hip.ptr(act), hip.dtype_code(gate), gate.numel(), hip.stream())
        ctx.save_for_backward(gate, up, *keep)
        return act

    @staticmethod
    def backward(ctx, d_act):
        gate, up, *keep = ctx.saved_tensors
        live = keep[0] if keep else None
        d_act = d_act.contiguous()
        if ctx.halves:
            # gate / up read in place; d_gate and d_up leave as two CONTIGUOUS tensors: the two dgrad GEMMs then are the shapes
            # (and leading dimensions) the tuned solution table holds - gradient halves of one [R, 2 C] buffer (lda = 2 C) cost
            # the padded cfg3 step 20 ms (148 vs 128 ms/step, library-default solutions for the strided operand)
            C = gate.shape[-1]
            R = gate.numel() // C
            dg = torch.empty(gate.shape, dtype=gate.dtype, device=gate.device)
            du = torch.empty(gate.shape, dtype=gate.dtype, device=gate.device)
            hip.call("dalm_swiglu_bwd_2d_live", hip.ptr(d_act), hip.ptr(gate), hip.ptr(up), hip.ptr(dg), hip.ptr(du),
                     hip.dtype_code(gate), R, C, C, 2 * C, 2 * C, C, C, hip.ptr(live), hip.stream())
            return dg, du, None
        dg, du = torch.empty_like(gate), torch.empty_like(up)
        if live is not None:
            C = gate.shape[-1]
            hip.call("dalm_swiglu_bwd_live", hip.ptr(d_act), hip.ptr(gate), hip.ptr(up), hip.ptr(dg), hip.ptr(du),
                     hip.dtype_code(gate), gate.numel() // C, C, hip.ptr(live), hip.stream())
        else:
            hip.call("dalm_swiglu_bwd", hip.ptr(d_act), hip.ptr(gate), hip.ptr(up), hip.ptr(dg), hip.ptr(du),
                     hip.dtype_code(gate), gate.numel(), hip.stream())
        return dg, du, None


def swiglu_supported(gate, up) -> bool:
    return (gate.is_cuda and gate.dtype in (torch.float32, torch.bfloat16) and up.dtype == gate.dtype
            and up.shape == gate.shape)


def swiglu(gate, up, live=None):
    """silu(gate) * up.  live: uint8 row liveness over the leading dimensions; None: that of the tower call in progress
    (dalm_amd/live_rows.py), if any."""
    return _SwiGLU.apply(gate, up, live)


# ---------------------------------------------------------------------------
# RMSNorm, optionally fused with the residual add in front of it (dalm_rms_norm_{fwd,bwd})
# ---------------------------------------------------------------------------
def rms_norm_supported(x: torch.Tensor, w: torch.Tensor) -> bool:
    D = x.shape[-1]
    vec = 4 if x.dtype == torch.float32 else 8
    # w.dtype == x.dtype: eager LlamaRMSNorm with an f32 weight and bf16 activations promotes the product to f32 - another
    # output dtype and rounding than the kernel's: those modules keep transformers' code
    return (x.is_cuda and x.dtype in (torch.float32, torch.bfloat16) and w.dim() == 1 and w.shape[0] == D
            and w.dtype == x.dtype and D % vec == 0 and D <= 64 * vec * 16)


def _norm_fwd(x2, delta2, w, eps, live=None):
    R, D = x2.shape
    y = torch.empty_like(x2)
    h = torch.empty_like(x2) if delta2 is not None else None
    rstd = torch.empty(R, device=x2.device, dtype=torch.float32)
    hip.call("dalm_rms_norm_fwd_live", hip.ptr(x2), hip.ptr(delta2), hip.ptr(w), hip.dtype_code(x2), R, D, float(eps), hip.ptr(h),
             hip.ptr(y), hip.ptr(rstd), hip.ptr(live), hip.stream())
    return h, y, rstd


def _norm_bwd(dy2, h2, w, rstd, dres2, live=None):
    R, D = h2.shape
    dx = torch.empty_like(h2)
    hip.call("dalm_rms_norm_bwd_live", hip.ptr(dy2), hip.ptr(h2), hip.ptr(w), hip.ptr(rstd), hip.ptr(dres2), hip.dtype_code(h2), R, D,
             hip.ptr(dx), hip.ptr(live), hip.stream())
    return dx


def _weight_grad(dy2, h2, rstd):
    # the normalised value rounded to the activation dtype first, as the eager chain does before its weight multiply
    xh = (h2.float() * rstd.unsqueeze(1)).to(h2.dtype)
    return (dy2.float() * xh.float()).sum(0)


def _as_rows(t, D, dtype):
    t = t.reshape(-1, D)
    if t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


class _AddRmsNorm(torch.autograd.Function):
    """(h, y) = (x + delta, rmsnorm(x + delta) * w);  with delta None: h IS x (returned as is) and only the backward is fused:
    the gradient that reaches h through the residual path is added inside the norm's backward kernel."""

    @staticmethod
    def forward(ctx, x, delta, w, eps, live=None):
        D = x.shape[-1]
        w_c = w if w.dtype == x.dtype else w.to(x.dtype)
        x2 = _as_rows(x, D, x.dtype)
        d2 = _as_rows(delta, D, x.dtype) if delta is not None else None
        if live is None:
            live = live_rows.current(x2.shape[0], x2.device)
        h2, y2, rstd = _norm_fwd(x2, d2, w_c, eps, live)
        # (the liveness vector is kept: the backward runs after the tower call's context, on autograd's thread)
        ctx.save_for_backward(h2 if h2 is not None else x2, w_c, rstd, *([live] if live is not None else []))
        ctx.shape, ctx.has_delta, ctx.w_dtype = x.shape, delta is not None, w.dtype
        h = h2.view(x.shape) if h2 is not None else x
        return h, y2.view(x.shape)

    @staticmethod
    def backward(ctx, dh, dy):
        h2, w_c, rstd, *live = ctx.saved_tensors
        D = h2.shape[1]
        dy2 = _as_rows(dy, D, h2.dtype)
        dres2 = _as_rows(dh, D, h2.dtype) if dh is not None else None
        d = _norm_bwd(dy2, h2, w_c, rstd, dres2, live[0] if live else None).view(ctx.shape)
        dw = _weight_grad(dy2, h2, rstd).to(ctx.w_dtype) if ctx.needs_input_grad[2] else None
        return d, (d if ctx.has_delta else None), dw, None, None


def add_rms_norm(x, delta, w, eps, live=None):
    """x + delta and its RMSNorm in one launch (one more in the backward, which also folds in the residual-path gradient).
    delta = None: (x itself, rmsnorm(x) * w).  live: uint8 row liveness; None: that of the tower call in progress
    (dalm_amd/live_rows.py), if any."""
    return _AddRmsNorm.apply(x, delta, w, eps, live)


# ---------------------------------------------------------------------------
# Granite: the sub-block's output enters the residual stream scaled by a Python float (modeling_granite.py
# `GraniteDecoderLayer.forward`: residual + hidden_states * self.residual_multiplier) - with the RMSNorm behind it
# (dalm_rms_norm_scaled_{fwd,bwd}) and alone (dalm_scale_add).  The product is rounded to the tensor dtype before the add, as torch's
# `tensor * float` is.
# ---------------------------------------------------------------------------
scaled_add_rms_norm_supported = rms_norm_supported       # the same rows, widths and weight dtype as `add_rms_norm`


class _ScaledAddRmsNorm(torch.autograd.Function):
    """(h, y) = (x + delta * mult, rmsnorm(h) * w), one launch; backward, one launch: dx (with the gradient that reaches h through
    the residual path added inside) and ddelta = dx * mult, formed from the rounded dx as autograd's backward of the multiply would."""

    @staticmethod
    def forward(ctx, x, delta, mult, w, eps, live=None):
        D = x.shape[-1]
        w_c = w if w.dtype == x.dtype else w.to(x.dtype)
        x2, d2 = _as_rows(x, D, x.dtype), _as_rows(delta, D, x.dtype)
        R = x2.shape[0]
        if live is None:
            live = live_rows.current(R, x2.device)
        h2, y2 = torch.empty_like(x2), torch.empty_like(x2)
        rstd = torch.empty(R, device=x2.device, dtype=torch.float32)
        hip.call("dalm_rms_norm_scaled_fwd", hip.ptr(x2), hip.ptr(d2), float(mult), hip.ptr(w_c), hip.dtype_code(x2), R, D, float(eps),
                 hip.ptr(h2), hip.ptr(y2), hip.ptr(rstd), hip.ptr(live), hip.stream())
        # (the liveness vector is kept: the backward runs after the tower call's context, on autograd's thread)
        ctx.save_for_backward(h2, w_c, rstd, *([live] if live is not None else []))
        ctx.shape, ctx.mult, ctx.w_dtype = x.shape, float(mult), w.dtype
        return h2.view(x.shape), y2.view(x.shape)

    @staticmethod
    def backward(ctx, dh, dy):
        h2, w_c, rstd, *live = ctx.saved_tensors
        R, D = h2.shape
        dy2 = _as_rows(dy, D, h2.dtype)
        dres2 = _as_rows(dh, D, h2.dtype) if dh is not None else None
        dx, dd = torch.empty_like(h2), torch.empty_like(h2)
        hip.call("dalm_rms_norm_scaled_bwd", hip.ptr(dy2), hip.ptr(h2), hip.ptr(w_c), hip.ptr(rstd), hip.ptr(dres2), ctx.mult,
                 hip.dtype_code(h2), R, D, hip.ptr(dx), hip.ptr(dd), hip.ptr(live[0] if live else None), hip.stream())
        dw = _weight_grad(dy2, h2, rstd).to(ctx.w_dtype) if ctx.needs_input_grad[3] else None
        return dx.view(ctx.shape), dd.view(ctx.shape), None, dw, None, None


def scaled_add_rms_norm(x, delta, mult, w, eps, live=None):
    """(x + delta * mult, its RMSNorm) in one launch, one more in the backward.  live: uint8 row liveness; None: that of the tower
    call in progress (dalm_amd/live_rows.py), if any."""
    return _ScaledAddRmsNorm.apply(x, delta, mult, w, eps, live)


def scale_add_supported(x: torch.Tensor, res=None) -> bool:
    """What `dalm_scale_add` takes: f32 or bf16 on the GPU, rows a multiple of 16 bytes wide (no upper limit), res of x's shape and
    dtype."""
    vec = 4 if x.dtype == torch.float32 else 8
    return (x.is_cuda and x.dtype in (torch.float32, torch.bfloat16) and x.dim() >= 1 and x.shape[-1] % vec == 0
            and x.numel() // vec < 2 ** 31
            and (res is None or (res.is_cuda and res.dtype == x.dtype and res.shape == x.shape)))


def _scale_add_launch(r2, x2, mult, live):
    out = torch.empty_like(x2)
    hip.call("dalm_scale_add", hip.ptr(r2), hip.ptr(x2), float(mult), hip.ptr(out), hip.dtype_code(x2), x2.shape[0], x2.shape[1],
             hip.ptr(live), hip.stream())
    return out


class _ScaleAdd(torch.autograd.Function):
    """res + x * mult (res None: x * mult), one launch; backward: the same kernel without res on the incoming gradient, and the
    incoming gradient itself for res."""

    @staticmethod
    def forward(ctx, res, x, mult, live=None):
        D = x.shape[-1]
        x2 = _as_rows(x, D, x.dtype)
        r2 = _as_rows(res, D, x.dtype) if res is not None else None
        if live is None:
            live = live_rows.current(x2.shape[0], x2.device)
        ctx.save_for_backward(*([live] if live is not None else []))
        ctx.mult = float(mult)
        return _scale_add_launch(r2, x2, ctx.mult, live).view(x.shape)

    @staticmethod
    def backward(ctx, dout):
        live = ctx.saved_tensors[0] if ctx.saved_tensors else None
        dx = None
        if ctx.needs_input_grad[1]:
            dx = _scale_add_launch(None, _as_rows(dout, dout.shape[-1], dout.dtype), ctx.mult, live).view(dout.shape)
        return (dout if ctx.needs_input_grad[0] else None), dx, None, None


def scale_add(res, x, mult, live=None):
    """res + x * mult in one launch - the product rounded to the dtype first, as the eager pair rounds - or x * mult with res None.
    live: uint8 row liveness; None: that of the tower call in progress (dalm_amd/live_rows.py), if any."""
    return _ScaleAdd.apply(res, x, mult, live)


# ---------------------------------------------------------------------------
# Cohere (modeling_cohere.py): the interleaved rotary embedding computed in f32 (dalm_rope_il_qk), CohereLayerNorm - bias-free, f32,
# one rounding - with the residual-path gradient folded into its backward (dalm_cohere_norm_{fwd,bwd}), and the parallel block's
# `residual + attn + mlp` (dalm_add3_live)
# ---------------------------------------------------------------------------
_ROPE_IL_DIMS = (32, 64, 128)


def _il_strides(t: torch.Tensor, n: int) -> list:
    """The first n strides, a dimension of size 1 counted as stride 0 (whatever torch kept there is never multiplied with anything)."""
    return [t.stride(i) if t.shape[i] > 1 else 0 for i in range(n)]


def rope_il_supported(q, k, cos, sin) -> bool:
    """What `dalm_rope_il_qk` takes: q / k [B, H, T, hd] f32 or bf16 GPU views with a contiguous last dimension, 16-byte aligned rows,
    head width 32, 64 or 128; cos / sin [B or 1, T, hd] of the activations' dtype or f32, laid out alike, no gradient."""
    if not (q.is_cuda and q.dim() == 4 and k.dim() == 4 and cos.dim() == 3 and sin.shape == cos.shape
            and q.dtype in (torch.float32, torch.bfloat16) and k.dtype == q.dtype and cos.dtype in (q.dtype, torch.float32)
            and sin.dtype == cos.dtype and q.shape[-1] in _ROPE_IL_DIMS and k.shape[-1] == q.shape[-1]
            and q.shape[0] == k.shape[0] and q.shape[2] == k.shape[2] and q.numel() > 0 and k.numel() > 0
            and cos.shape[0] in (1, q.shape[0]) and cos.shape[1:] == (q.shape[2], q.shape[3])
            and sin.stride() == cos.stride() and not cos.requires_grad and not sin.requires_grad):
        return False
    vec = 16 // q.element_size()
    return (all(t.stride(-1) == 1 and t.data_ptr() % 16 == 0 for t in (q, k, cos, sin))
            and all(s % vec == 0 for t, n in ((q, 3), (k, 3), (cos, 2)) for s in _il_strides(t, n)))


def _rope_il_launch(q, k, cos, sin, backward: bool, live=None, in_place: bool = False):
    """One `dalm_rope_il_qk` launch over what `rope_il_supported` took.  in_place: the results overwrite q and k (a lane reads the
    16 bytes it writes and no others) - the un-rotation of gradients nobody else holds."""
    hip.require_gpu(q, k, cos, sin)
    if in_place:
        qo, ko = q, k
    else:
        qo, ko = torch.empty_like(q), torch.empty_like(k)       # preserve_format: same strides as the (dense) views
        if qo.stride(-1) != 1 or ko.stride(-1) != 1:            # overlapping / exotic input layout: plain contiguous outputs
            qo = torch.empty(q.shape, dtype=q.dtype, device=q.device)
            ko = torch.empty(k.shape, dtype=k.dtype, device=k.device)
    B, Hq, T, hd = q.shape
    s3 = lambda t: (C.c_int64 * 3)(*_il_strides(t, 3))  # noqa: E731
    hip.call("dalm_rope_il_qk", hip.ptr(q), hip.ptr(k), hip.ptr(qo), hip.ptr(ko), hip.ptr(cos), hip.ptr(sin), hip.dtype_code(q),
             hip.dtype_code(cos), B, T, Hq, k.shape[1], hd, s3(q), s3(k), s3(qo), s3(ko), (C.c_int64 * 2)(*_il_strides(cos, 2)),
             int(backward), hip.ptr(live), hip.stream())
    return qo, ko


def _il_gradient(g: torch.Tensor) -> torch.Tensor:
    vec = 16 // g.element_size()
    ok = g.stride(-1) == 1 and g.data_ptr() % 16 == 0 and all(s % vec == 0 for s in _il_strides(g, 3))
    return g if ok else g.contiguous()


class _RopeIlQK(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, cos, sin, live=None):
        if live is None:
            live = live_rows.current(q.shape[0] * q.shape[2], q.device)
        ctx.save_for_backward(cos, sin, *([live] if live is not None else []))   # the backward runs after the tower call's context
        return _rope_il_launch(q, k, cos, sin, False, live)

    @staticmethod
    def backward(ctx, gq, gk):
        cos, sin, *live = ctx.saved_tensors
        dq, dk = _rope_il_launch(_il_gradient(gq), _il_gradient(gk), cos, sin, True, live[0] if live else None)
        return dq, dk, None, None, None


def rope_il_qk(q, k, cos, sin, live=None):
    """modeling_cohere.py's apply_rotary_pos_emb - (x.float() * cos + rotate_half(x.float()) * sin).to(dtype) with the interleaved
    rotate_half - for q and k in one launch, one more backward; values and gradients are the eager chain's, bit for bit.
    live: uint8 [B T] row liveness; None: that of the tower call in progress (dalm_amd/live_rows.py), if any."""
    return _RopeIlQK.apply(q, k, cos, sin, live)


# ---------------------------------------------------------------------------
# Phi-3 / Phi-4 (modeling_phi3.py): the partial rotary embedding (dalm_rope_partial_qk) - the first rot = cos.shape[-1] elements of
# a head rotate, half-split within those rot; the rest pass through
# ---------------------------------------------------------------------------
def rope_partial_supported(q, k, cos, sin) -> bool:
    """What `dalm_rope_partial_qk` takes: q / k [B, H, T, hd] f32 or bf16 GPU views with a contiguous last dimension, 16-byte
    aligned rows, head width 32, 64 or 128; cos / sin [B or 1, T, rot] of the activations' dtype, laid out alike, no gradient;
    0 < rot <= hd with rot / 2 a multiple of 16 bytes (rot a multiple of 16 for bf16, of 8 for f32)."""
    if not (q.is_cuda and q.dim() == 4 and k.dim() == 4 and cos.dim() == 3 and sin.shape == cos.shape
            and q.dtype in (torch.float32, torch.bfloat16) and k.dtype == q.dtype and cos.dtype == q.dtype
            and sin.dtype == q.dtype and q.shape[-1] in _ROPE_IL_DIMS and k.shape[-1] == q.shape[-1]
            and q.shape[0] == k.shape[0] and q.shape[2] == k.shape[2] and q.numel() > 0 and k.numel() > 0
            and cos.shape[0] in (1, q.shape[0]) and cos.shape[1] == q.shape[2]
            and sin.stride() == cos.stride() and not cos.requires_grad and not sin.requires_grad):
        return False
    vec = 16 // q.element_size()
    rot = cos.shape[-1]
    return (0 < rot <= q.shape[-1] and rot % (2 * vec) == 0
            and all(t.stride(-1) == 1 and t.data_ptr() % 16 == 0 for t in (q, k, cos, sin))
            and all(s % vec == 0 for t, n in ((q, 3), (k, 3), (cos, 2)) for s in _il_strides(t, n)))


def _rope_partial_launch(q, k, cos, sin, backward: bool, live=None, in_place: bool = False):
    """One `dalm_rope_partial_qk` launch over what `rope_partial_supported` took.  in_place: the rotated part of live rows is
    overwritten in q and k, the pass part and dead rows stay as they are - the un-rotation of gradients nobody else holds."""
    hip.require_gpu(q, k, cos, sin)
    if in_place:
        qo, ko = q, k
    else:
        qo, ko = torch.empty_like(q), torch.empty_like(k)       # preserve_format: same strides as the (dense) views
        if qo.stride(-1) != 1 or ko.stride(-1) != 1:            # overlapping / exotic input layout: plain contiguous outputs
            qo = torch.empty(q.shape, dtype=q.dtype, device=q.device)
            ko = torch.empty(k.shape, dtype=k.dtype, device=k.device)
    B, Hq, T, hd = q.shape
    s3 = lambda t: (C.c_int64 * 3)(*_il_strides(t, 3))  # noqa: E731
    hip.call("dalm_rope_partial_qk", hip.ptr(q), hip.ptr(k), hip.ptr(qo), hip.ptr(ko), hip.ptr(cos), hip.ptr(sin),
             hip.dtype_code(q), B, T, Hq, k.shape[1], hd, cos.shape[-1], s3(q), s3(k), s3(qo), s3(ko),
             (C.c_int64 * 2)(*_il_strides(cos, 2)), int(backward), hip.ptr(live), hip.stream())
    return qo, ko


class _RopePartialQK(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, cos, sin, live=None):
        if live is None:
            live = live_rows.current(q.shape[0] * q.shape[2], q.device)
        ctx.save_for_backward(cos, sin, *([live] if live is not None else []))   # the backward runs after the tower call's context
        return _rope_partial_launch(q, k, cos, sin, False, live)

    @staticmethod
    def backward(ctx, gq, gk):
        cos, sin, *live = ctx.saved_tensors
        dq, dk = _rope_partial_launch(_il_gradient(gq), _il_gradient(gk), cos, sin, True, live[0] if live else None)
        return dq, dk, None, None, None


def rope_partial_qk(q, k, cos, sin, live=None):
    """modeling_phi3.py's apply_rotary_pos_emb - cat([x_rot * cos + rotate_half(x_rot) * sin, x_pass]) with x_rot the first
    cos.shape[-1] elements of each head - for q and k in one launch, one more backward; values and gradients are the eager
    chain's, bit for bit.  live: uint8 [B T] row liveness; None: that of the tower call in progress (dalm_amd/live_rows.py), if any."""
    return _RopePartialQK.apply(q, k, cos, sin, live)


def cohere_norm_supported(x: torch.Tensor, w: torch.Tensor) -> bool:
    """What `dalm_cohere_norm_*` take: `rms_norm_supported`'s widths, at least one row; the weight [D], f32 or bf16 under either
    activation dtype (CohereLayerNorm computes in f32 and casts once, whatever the weight's dtype is)."""
    D = x.shape[-1] if x.dim() else 0
    vec = 4 if x.dtype == torch.float32 else 8
    return (x.is_cuda and x.dtype in (torch.float32, torch.bfloat16) and x.numel() > 0 and w.is_cuda and w.dim() == 1
            and w.shape[0] == D and w.dtype in (torch.float32, torch.bfloat16) and w.is_contiguous() and w.data_ptr() % 16 == 0
            and D % vec == 0 and D <= 64 * vec * 16)


class _CohereNormRes(torch.autograd.Function):
    """(x, y) = (x, CohereLayerNorm(x)); x is handed back so that the gradient reaching it through the residual path is added INSIDE
    the norm's backward kernel (as `_AddRmsNorm` with delta None)."""

    @staticmethod
    def forward(ctx, x, w, eps, live=None):
        D = x.shape[-1]
        x2 = _as_rows(x, D, x.dtype)
        R = x2.shape[0]
        if live is None:
            live = live_rows.current(R, x2.device)
        w = w.detach()
        y2 = torch.empty_like(x2)
        mean = torch.empty(R, device=x2.device, dtype=torch.float32)
        rstd = torch.empty(R, device=x2.device, dtype=torch.float32)
        hip.call("dalm_cohere_norm_fwd", hip.ptr(x2), hip.ptr(w), hip.dtype_code(x2), hip.dtype_code(w), R, D, float(eps), hip.ptr(y2),
                 hip.ptr(mean), hip.ptr(rstd), hip.ptr(live), hip.stream())
        # (the liveness vector is kept: the backward runs after the tower call's context, on autograd's thread)
        ctx.save_for_backward(x2, w, mean, rstd, *([live] if live is not None else []))
        ctx.shape, ctx.eps = x.shape, float(eps)
        ctx.set_materialize_grads(False)           # no residual-path gradient: the backward kernel reads none, not a tensor of zeros
        return x, y2.view(x.shape)

    @staticmethod
    def backward(ctx, dres, dy):
        if dy is None:
            return dres, None, None, None
        x2, w, mean, rstd, *keep = ctx.saved_tensors
        live = keep[0] if keep else None
        R, D = x2.shape
        dy2 = _as_rows(dy, D, x2.dtype)
        dres2 = _as_rows(dres, D, x2.dtype) if dres is not None else None
        dx = torch.empty_like(x2)
        hip.call("dalm_cohere_norm_bwd", hip.ptr(dy2), hip.ptr(x2), hip.ptr(w), hip.ptr(mean), hip.ptr(rstd), hip.ptr(dres2),
                 hip.dtype_code(x2), hip.dtype_code(w), R, D, hip.ptr(dx), hip.ptr(live), hip.stream())
        dw = None
        if ctx.needs_input_grad[1]:
            # sum over the rows of dy * xh, formed by torch.  A rare path (LoRA freezes the norm weights), so it is taken in
            # float64 from x itself: rounded once, whatever the number of rows
            xd = x2.double()
            xd = xd - xd.mean(1, keepdim=True)
            prod = dy2.double() * (xd * torch.rsqrt(xd.pow(2).mean(1, keepdim=True) + ctx.eps))
            if live is not None:                   # dead rows: dy and x are whatever their producers left
                prod = prod.masked_fill((live == 0).unsqueeze(1), 0.0)
            dw = prod.sum(0).to(w.dtype)
        return dx.view(ctx.shape), dw, None, None


def cohere_norm_res(x, w, eps, live=None):
    """(x itself, CohereLayerNorm(x)): one launch forward, one backward (which also folds in the residual-path gradient).
    live: uint8 row liveness; None: that of the tower call in progress (dalm_amd/live_rows.py), if any."""
    return _CohereNormRes.apply(x, w, eps, live)


def add3_live_supported(res, a, b) -> bool:
    """What `dalm_add3_live` takes: three f32 or bf16 GPU tensors of one shape and dtype, rows a multiple of 16 bytes wide (no upper
    limit)."""
    vec = 4 if res.dtype == torch.float32 else 8
    return (res.is_cuda and res.dtype in (torch.float32, torch.bfloat16) and res.dim() >= 1 and res.shape[-1] % vec == 0
            and 0 < res.numel() // vec < 2 ** 31
            and all(t.is_cuda and t.dtype == res.dtype and t.shape == res.shape for t in (a, b)))


class _Add3Live(torch.autograd.Function):
    """(res + a) + b, one launch; the backward hands the incoming gradient to all three without a launch."""

    @staticmethod
    def forward(ctx, res, a, b, live=None):
        D = res.shape[-1]
        r2, a2, b2 = (_as_rows(t, D, res.dtype) for t in (res, a, b))
        if live is None:
            live = live_rows.current(r2.shape[0], r2.device)
        out = torch.empty_like(r2)
        hip.call("dalm_add3_live", hip.ptr(r2), hip.ptr(a2), hip.ptr(b2), hip.ptr(out), hip.dtype_code(r2), r2.shape[0], D,
                 hip.ptr(live), hip.stream())
        return out.view(res.shape)

    @staticmethod
    def backward(ctx, g):
        return g, g, g, None


def add3_live(res, a, b, live=None):
    """res + a + b as eager evaluates it - the first sum rounded to the dtype, then the second - in one launch.
    live: uint8 row liveness; None: that of the tower call in progress (dalm_amd/live_rows.py), if any."""
    return _Add3Live.apply(res, a, b, live)


# ---------------------------------------------------------------------------
# Gemma: GeGLU (dalm_geglu_{fwd,bwd}) and the (1 + w) RMSNorm with the residual add in front of it (dalm_gemma_norm_{fwd,bwd})
# ---------------------------------------------------------------------------
class _GeGLU(torch.autograd.Function):
    """gelu_tanh(gate) * up, `_SwiGLU`'s shape: gate / up as the halves of one [R, 2 C] buffer are read in place, nothing but gate and
    up is saved, d_gate and d_up leave as two contiguous tensors (the reason `_SwiGLU.backward` gives)."""

    @staticmethod
    def forward(ctx, gate, up, live=None):
        hip.require_gpu(gate, up)
        halves = _halves_of_one(gate, up)
        if not halves:
            gate, up = gate.contiguous(), up.contiguous()
        C = gate.shape[-1]
        R = gate.numel() // C if C else 0
        if live is None and gate.dim() >= 2:
            live = live_rows.current(R, gate.device)
        if live is not None and live.numel() != R:
            live = None
        ctx.ld = 2 * C if halves else C
        act = torch.empty(gate.shape, dtype=gate.dtype, device=gate.device)
        hip.call("dalm_geglu_fwd", hip.ptr(gate), hip.ptr(up), hip.ptr(act), hip.dtype_code(gate), R, C, ctx.ld, ctx.ld, C, hip.ptr(live),
                 hip.stream())
        ctx.save_for_backward(gate, up, *([live] if live is not None else []))    # the backward runs after the tower call's context
        return act

    @staticmethod
    def backward(ctx, d_act):
        gate, up, *keep = ctx.saved_tensors
        d_act = d_act.contiguous()
        C = gate.shape[-1]
        R = gate.numel() // C if C else 0
        dg = torch.empty(gate.shape, dtype=gate.dtype, device=gate.device)
        du = torch.empty(gate.shape, dtype=gate.dtype, device=gate.device)
        hip.call("dalm_geglu_bwd", hip.ptr(d_act), hip.ptr(gate), hip.ptr(up), hip.ptr(dg), hip.ptr(du), hip.dtype_code(gate), R, C, C,
                 ctx.ld, ctx.ld, C, C, hip.ptr(keep[0] if keep else None), hip.stream())
        return dg, du, None


def geglu_supported(gate, up) -> bool:
    return (gate.is_cuda and gate.dtype in (torch.float32, torch.bfloat16) and up.dtype == gate.dtype and up.shape == gate.shape
            and gate.dim() >= 1 and gate.shape[-1] % (16 // gate.element_size()) == 0 and gate.numel() < 2 ** 32
            and gate.data_ptr() % 16 == 0 and up.data_ptr() % 16 == 0)     # a view at an odd storage offset: the eager chain


def geglu(gate, up, live=None):
    """gelu_tanh(gate) * up (GemmaMLP's activation).  live: uint8 row liveness over the leading dimensions; None: that of the tower
    call in progress (dalm_amd/live_rows.py), if any."""
    return _GeGLU.apply(gate, up, live)


# ---------------------------------------------------------------------------
# Arcee: ReLU^2 (dalm_relu2_{fwd,bwd}; modeling_arcee.py `ArceeMLP.forward`: down(act_fn(up(x))), act_fn = square(relu(x)))
# ---------------------------------------------------------------------------
class _ReLU2(torch.autograd.Function):
    """relu(y)^2, `_GeGLU`'s shape with one input: y (a row-strided 2-D view is read in place) is all that is saved, the backward
    recomputes relu(y) and leaves d_y contiguous."""

    @staticmethod
    def forward(ctx, y, live=None):
        hip.require_gpu(y)
        C = y.shape[-1]
        rows_in_place = y.dim() == 2 and y.stride(1) == 1 and y.stride(0) >= C and y.stride(0) % (16 // y.element_size()) == 0
        if not rows_in_place:
            y = y.contiguous()
        R = y.numel() // C if C else 0
        if live is None and y.dim() >= 2:
            live = live_rows.current(R, y.device)
        if live is not None and live.numel() != R:
            live = None
        ctx.ld = y.stride(0) if rows_in_place else C
        act = torch.empty(y.shape, dtype=y.dtype, device=y.device)
        hip.call("dalm_relu2_fwd", hip.ptr(y), hip.ptr(act), hip.dtype_code(y), R, C, ctx.ld, C, hip.ptr(live), hip.stream())
        ctx.save_for_backward(y, *([live] if live is not None else []))    # the backward runs after the tower call's context
        return act

    @staticmethod
    def backward(ctx, d_act):
        y, *keep = ctx.saved_tensors
        d_act = d_act.contiguous()
        C = y.shape[-1]
        R = y.numel() // C if C else 0
        dy = torch.empty(y.shape, dtype=y.dtype, device=y.device)
        hip.call("dalm_relu2_bwd", hip.ptr(d_act), hip.ptr(y), hip.ptr(dy), hip.dtype_code(y), R, C, C, ctx.ld, C,
                 hip.ptr(keep[0] if keep else None), hip.stream())
        return dy, None


def relu2_supported(y) -> bool:
    return (y.is_cuda and y.dtype in (torch.float32, torch.bfloat16) and y.dim() >= 1
            and y.shape[-1] % (16 // y.element_size()) == 0 and y.numel() < 2 ** 32
            and y.data_ptr() % 16 == 0)                                    # a view at an odd storage offset: the eager chain


def relu2(y, live=None):
    """relu(y)^2 (ArceeMLP's activation).  live: uint8 row liveness over the leading dimensions; None: that of the tower call in
    progress (dalm_amd/live_rows.py), if any."""
    return _ReLU2.apply(y, live)


def gemma_rms_norm_supported(x: torch.Tensor, w: torch.Tensor) -> bool:
    """What `dalm_gemma_norm_*` take: `rms_norm_supported`'s widths; the weight f32 or bf16 under either activation dtype (GemmaRMSNorm
    computes in f32 and casts once, to the activation's dtype, whatever the weight's is)."""
    D = x.shape[-1]
    vec = 4 if x.dtype == torch.float32 else 8
    return (x.is_cuda and x.dtype in (torch.float32, torch.bfloat16) and w.is_cuda and w.dim() == 1 and w.shape[0] == D
            and w.dtype in (torch.float32, torch.bfloat16) and w.is_contiguous() and w.data_ptr() % 16 == 0
            and D % vec == 0 and D <= 64 * vec * 16)


def _gemma_weight_grad(dy2, h2, rstd, live=None):
    # sum over the rows of f32(dy) * xh; xh stays f32 (the eager chain multiplies with the weight before its one rounding)
    prod = dy2.float() * (h2.float() * rstd.unsqueeze(1))
    if live is not None:                           # dead rows: dy and h are whatever their producers left
        prod = prod.masked_fill((live == 0).unsqueeze(1), 0.0)
    return prod.sum(0)


class _GemmaAddRmsNorm(torch.autograd.Function):
    """`_AddRmsNorm` with GemmaRMSNorm's formula: (h, y) = (x + delta, (f32(h) * rstd * (1 + f32(w))).to(x.dtype)); with delta None h
    IS x and only the backward is fused (the residual-path gradient is added inside the norm's backward kernel)."""

    @staticmethod
    def forward(ctx, x, delta, w, eps, live=None):
        D = x.shape[-1]
        x2 = _as_rows(x, D, x.dtype)
        d2 = _as_rows(delta, D, x.dtype) if delta is not None else None
        R = x2.shape[0]
        if live is None:
            live = live_rows.current(R, x2.device)
        w = w.detach()
        y2 = torch.empty_like(x2)
        h2 = torch.empty_like(x2) if d2 is not None else None
        rstd = torch.empty(R, device=x2.device, dtype=torch.float32)
        hip.call("dalm_gemma_norm_fwd", hip.ptr(x2), hip.ptr(d2), hip.ptr(w), hip.dtype_code(x2), hip.dtype_code(w), R, D, float(eps),
                 hip.ptr(h2), hip.ptr(y2), hip.ptr(rstd), hip.ptr(live), hip.stream())
        # (the liveness vector is kept: the backward runs after the tower call's context, on autograd's thread)
        ctx.save_for_backward(h2 if h2 is not None else x2, w, rstd, *([live] if live is not None else []))
        ctx.shape, ctx.has_delta = x.shape, delta is not None
        ctx.set_materialize_grads(False)           # no residual-path gradient: the backward kernel reads none, not a tensor of zeros
        return (h2.view(x.shape) if h2 is not None else x), y2.view(x.shape)

    @staticmethod
    def backward(ctx, dh, dy):
        if dy is None:
            return dh, (dh if ctx.has_delta else None), None, None, None
        h2, w, rstd, *keep = ctx.saved_tensors
        live = keep[0] if keep else None
        R, D = h2.shape
        dy2 = _as_rows(dy, D, h2.dtype)
        dres2 = _as_rows(dh, D, h2.dtype) if dh is not None else None
        dx = torch.empty_like(h2)
        hip.call("dalm_gemma_norm_bwd", hip.ptr(dy2), hip.ptr(h2), hip.ptr(w), hip.ptr(rstd), hip.ptr(dres2), hip.dtype_code(h2),
                 hip.dtype_code(w), R, D, hip.ptr(dx), hip.ptr(live), hip.stream())
        d = dx.view(ctx.shape)
        dw = _gemma_weight_grad(dy2, h2, rstd, live).to(w.dtype) if ctx.needs_input_grad[2] else None
        return d, (d if ctx.has_delta else None), dw, None, None


def gemma_add_rms_norm(x, delta, w, eps, live=None):
    """x + delta and its GemmaRMSNorm in one launch (one more in the backward, which also folds in the residual-path gradient).
    delta = None: (x itself, the norm of x).  live: uint8 row liveness; None: that of the tower call in progress
    (dalm_amd/live_rows.py), if any."""
    return _GemmaAddRmsNorm.apply(x, delta, w, eps, live)


# ---------------------------------------------------------------------------
# Qwen3: RMSNorm over the head dimension of q and k + rotary embedding (dalm_head_norm_rope_fwd / dalm_head_norm_bwd), bf16
# ---------------------------------------------------------------------------
_HEAD_NORM_DIMS = (64, 128)            # the widths the fused rotary attention takes


def head_norm_rope_supported(q, k, wq, wk, cos, sin) -> bool:
    """What `dalm_head_norm_rope_fwd` takes: q / k [B, H, T, hd] bf16 GPU views (contiguous last dimension, 16-byte rows), head
    width 64 or 128, norm weights [hd] in the activation dtype (an f32 weight promotes the eager product to f32: another
    output dtype and rounding, those modules keep transformers' code), and the cos / sin tables of `rope_supported`."""
    if not (q.is_cuda and q.dtype == torch.bfloat16 and q.dim() == 4 and k.dim() == 4 and q.shape[-1] in _HEAD_NORM_DIMS):
        return False
    if not rope_supported(q, k, cos, sin):
        return False
    hd = q.shape[-1]
    for w in (wq, wk):
        if not (w.is_cuda and w.dtype == q.dtype and w.dim() == 1 and w.shape[0] == hd and w.is_contiguous()
                and w.data_ptr() % 16 == 0):
            return False
    views = all(t.stride(-1) == 1 and all(s % 8 == 0 for s in t.stride()[:3]) and t.data_ptr() % 16 == 0 for t in (q, k))
    tables = all(t.data_ptr() % 16 == 0 and t.stride(1) % 8 == 0 and (t.shape[0] == 1 or t.stride(0) % 8 == 0) for t in (cos, sin))
    return views and tables and q.shape[0] * q.shape[2] * (q.shape[1] + k.shape[1]) * (hd // 8) < 2 ** 31


def _token_major(B, H, T, hd, like):
    """[B, H, T, hd] view of fresh [B, T, H, hd] memory: the layout of the projections' views, dense as [B T, H hd]."""
    return torch.empty(B, T, H, hd, dtype=like.dtype, device=like.device).transpose(1, 2)


def head_norm_rope(q, k, wq, wk, eps_q, eps_k, cos, sin, live=None):
    """(rope(rmsnorm_hd(q) * wq), rope(rmsnorm_hd(k) * wk), rstd_q [B, T, Hq], rstd_k [B, T, Hk]) in one launch; q / k are read
    in place (column slices of a q|k|v GEMM output included).  live: uint8 [B T] row liveness; None: that of the tower call in
    progress (dalm_amd/live_rows.py), if any.  Returns the vector it used as the fifth value: the backward needs the same one."""
    hip.require_gpu(q, k, wq, wk, cos, sin)
    B, Hq, T, hd = q.shape
    Hk = k.shape[1]
    if live is None:
        live = live_rows.current(B * T, q.device)
    qo, ko = _token_major(B, Hq, T, hd, q), _token_major(B, Hk, T, hd, k)
    rq = torch.empty(B, T, Hq, dtype=torch.float32, device=q.device)
    rk = torch.empty(B, T, Hk, dtype=torch.float32, device=q.device)
    cs = (C.c_int64 * 2)(cos.stride(0) if cos.shape[0] > 1 else 0, cos.stride(1))
    hip.call("dalm_head_norm_rope_fwd", hip.ptr(q), hip.ptr(k), hip.ptr(wq), hip.ptr(wk), float(eps_q), float(eps_k), hip.ptr(cos),
             hip.ptr(sin), B, T, Hq, Hk, hd, _strides3(q), _strides3(k), _strides3(qo), _strides3(ko), cs, hip.ptr(qo), hip.ptr(ko),
             hip.ptr(rq), hip.ptr(rk), hip.ptr(live), hip.stream())
    return qo, ko, rq, rk, live


def head_norm_bwd(gq, gk, q, k, wq, wk, rstd_q, rstd_k, live=None):
    """Gradients of the pre-norm q / k from those of the normed, un-rotated ones (what `dalm_attn_bwd` leaves when it is given
    cos / sin).  dq / dk come in [B, T, H, hd] memory order: their reshape to [B T, H hd] is dense and the dgrad GEMMs keep the
    leading dimensions the tuned table holds.  live: the vector the forward used."""
    B, Hq, T, hd = q.shape
    Hk = k.shape[1]
    if gq.stride(-1) != 1 or any(s % 8 for s in gq.stride()[:3]):
        gq = gq.contiguous()
    if gk.stride(-1) != 1 or any(s % 8 for s in gk.stride()[:3]):
        gk = gk.contiguous()
    dq, dk = _token_major(B, Hq, T, hd, q), _token_major(B, Hk, T, hd, k)
    hip.call("dalm_head_norm_bwd", hip.ptr(gq), hip.ptr(gk), hip.ptr(q), hip.ptr(k), hip.ptr(wq), hip.ptr(wk), hip.ptr(rstd_q),
             hip.ptr(rstd_k), B, T, Hq, Hk, hd, _strides3(gq), _strides3(gk), _strides3(q), _strides3(k), _strides3(dq), _strides3(dk),
             hip.ptr(dq), hip.ptr(dk), hip.ptr(live), hip.stream())
    return dq, dk


def head_norm_weight_grad(g, x, rstd, live=None):
    """Gradient of a head-norm weight [hd] (training without adapters; the kernels produce none): sum over (b, head, t) of
    g * xh with xh rounded to the activation dtype first, as `_weight_grad`.  g, x: [B, H, T, hd]; rstd: [B, T, H]."""
    xh = (x.float() * rstd.transpose(1, 2).unsqueeze(-1)).to(x.dtype)
    prod = g.float() * xh.float()
    if live is not None:                           # dead rows: g is whatever the attention backward left, x is not read
        B, _, T, _ = x.shape
        prod = prod.masked_fill((live == 0).view(B, 1, T, 1), 0.0)
    return prod.sum((0, 1, 2))


# ---------------------------------------------------------------------------
# OLMo-2: the norm AFTER the sub-block, inside the residual (dalm_norm_add_{fwd,bwd}), and q_norm / k_norm over the whole projection
# width + rotary embedding (dalm_row_norm_rope_fwd / dalm_row_norm_bwd, bf16).  modeling_olmo2.py `Olmo2DecoderLayer.forward`,
# `Olmo2Attention.forward`, `Olmo2RMSNorm.forward`: (w * (x.float() * rstd)).to(x.dtype) - the weight enters in f32, one rounding
# ---------------------------------------------------------------------------
def _f32_weight_ok(w: torch.Tensor, D: int) -> bool:
    return (w.is_cuda and w.dim() == 1 and w.shape[0] == D and w.dtype in (torch.float32, torch.bfloat16) and w.is_contiguous()
            and w.data_ptr() % 16 == 0)


def norm_add_supported(x: torch.Tensor, res: torch.Tensor, w: torch.Tensor) -> bool:
    """What `dalm_norm_add_*` take: x (the sub-block's output) and res (the residual) of one shape and dtype (f32 or bf16) on the
    GPU, `rms_norm_supported`'s widths; the weight f32 or bf16 under either activation dtype (Olmo2RMSNorm multiplies in f32)."""
    D = x.shape[-1]
    vec = 4 if x.dtype == torch.float32 else 8
    return (x.is_cuda and res.is_cuda and x.dtype in (torch.float32, torch.bfloat16) and res.dtype == x.dtype and res.shape == x.shape
            and _f32_weight_ok(w, D) and D % vec == 0 and D <= 64 * vec * 16)


class _NormAdd(torch.autograd.Function):
    """res + rmsnorm(x) * w with Olmo2RMSNorm's rounding, one launch; backward: one launch for x (`dalm_norm_add_bwd`), the
    residual's gradient is the incoming one itself, the weight's is computed in torch when it is wanted."""

    @staticmethod
    def forward(ctx, x, res, w, eps, live=None):
        D = x.shape[-1]
        x2, r2 = _as_rows(x, D, x.dtype), _as_rows(res, D, x.dtype)
        R = x2.shape[0]
        if live is None:
            live = live_rows.current(R, x2.device)
        w = w.detach()
        out = torch.empty_like(x2)
        rstd = torch.empty(R, device=x2.device, dtype=torch.float32)
        hip.call("dalm_norm_add_fwd", hip.ptr(x2), hip.ptr(r2), hip.ptr(w), hip.dtype_code(x2), hip.dtype_code(w), R, D, float(eps),
                 hip.ptr(out), hip.ptr(rstd), hip.ptr(live), hip.stream())
        # (the liveness vector is kept: the backward runs after the tower call's context, on autograd's thread)
        ctx.save_for_backward(x2, w, rstd, *([live] if live is not None else []))
        ctx.shape = x.shape
        return out.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x2, w, rstd, *keep = ctx.saved_tensors
        live = keep[0] if keep else None
        R, D = x2.shape
        dy2 = _as_rows(dy, D, x2.dtype)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x2)
            hip.call("dalm_norm_add_bwd", hip.ptr(dy2), hip.ptr(x2), hip.ptr(w), hip.ptr(rstd), hip.dtype_code(x2), hip.dtype_code(w), R,
                     D, hip.ptr(dx), hip.ptr(live), hip.stream())
            dx = dx.view(ctx.shape)
        dead = None if live is None else (live == 0).unsqueeze(1)
        dw = _olmo2_weight_grad(dy2, x2, rstd.unsqueeze(1), dead, 0).to(w.dtype) if ctx.needs_input_grad[2] else None
        return dx, dy, dw, None, None


def _olmo2_weight_grad(g, x, rstd, dead, dims):
    """Sum over `dims` of g * (x * rstd), rstd and dead (a bool mask of the dead rows, or None) broadcastable against g: the gradient of an
    Olmo2RMSNorm weight.  xh is not rounded (the eager chain multiplies with the weight in f32 before its one rounding), and the
    products and the sum are taken in f64: the result is rounded once, so an f32 weight's gradient is at least as close to the
    truth as the eager chain's.  Only a trainable norm weight pays for it (not the LoRA step)."""
    prod = g.double() * (x.double() * rstd.double())
    if dead is not None:                           # dead rows: g and x are whatever their producers left
        prod = prod.masked_fill(dead, 0.0)
    return prod.sum(dims).float()


def norm_add(x, res, w, eps, live=None):
    """res + Olmo2RMSNorm(x) in one launch (one more in the backward).  live: uint8 row liveness; None: that of the tower call in
    progress (dalm_amd/live_rows.py), if any."""
    return _NormAdd.apply(x, res, w, eps, live)


def row_norm_rope_supported(q, k, wq, wk, cos, sin) -> bool:
    """What `dalm_row_norm_rope_fwd` takes: `head_norm_rope_supported`'s q / k / cos / sin, rows of at most 8192 elements, and norm
    weights [Hq hd] / [Hk hd] in f32 or bf16 (one dtype for both)."""
    if not (q.is_cuda and q.dtype == torch.bfloat16 and q.dim() == 4 and k.dim() == 4 and q.shape[-1] in _HEAD_NORM_DIMS):
        return False
    if not rope_supported(q, k, cos, sin):
        return False
    hd = q.shape[-1]
    if not (_f32_weight_ok(wq, q.shape[1] * hd) and _f32_weight_ok(wk, k.shape[1] * hd) and wq.dtype == wk.dtype
            and q.shape[1] * hd <= 8192 and k.shape[1] * hd <= 8192):
        return False
    views = all(t.stride(-1) == 1 and all(s % 8 == 0 for s in t.stride()[:3]) and t.data_ptr() % 16 == 0 for t in (q, k))
    tables = all(t.data_ptr() % 16 == 0 and t.stride(1) % 8 == 0 and (t.shape[0] == 1 or t.stride(0) % 8 == 0) for t in (cos, sin))
    return views and tables and q.shape[0] * q.shape[2] * (q.shape[1] + k.shape[1]) * (hd // 8) < 2 ** 31


def row_norm_rope(q, k, wq, wk, eps_q, eps_k, cos, sin, live=None):
    """(rope(rmsnorm_row(q) * wq), rope(rmsnorm_row(k) * wk), rstd_q [B, T], rstd_k [B, T]) in one launch, the norms over all heads of
    a token; q / k are read in place (column slices of a q|k|v GEMM output included).  live: uint8 [B T] row liveness; None: that
    of the tower call in progress (dalm_amd/live_rows.py), if any.  Returns the vector it used as the fifth value: the backward
    needs the same one."""
    hip.require_gpu(q, k, wq, wk, cos, sin)
    B, Hq, T, hd = q.shape
    Hk = k.shape[1]
    if live is None:
        live = live_rows.current(B * T, q.device)
    qo, ko = _token_major(B, Hq, T, hd, q), _token_major(B, Hk, T, hd, k)
    rq = torch.empty(B, T, dtype=torch.float32, device=q.device)
    rk = torch.empty(B, T, dtype=torch.float32, device=q.device)
    cs = (C.c_int64 * 2)(cos.stride(0) if cos.shape[0] > 1 else 0, cos.stride(1))
    hip.call("dalm_row_norm_rope_fwd", hip.ptr(q), hip.ptr(k), hip.ptr(wq), hip.ptr(wk), hip.dtype_code(wq), float(eps_q), float(eps_k),
             hip.ptr(cos), hip.ptr(sin), B, T, Hq, Hk, hd, _strides3(q), _strides3(k), _strides3(qo), _strides3(ko), cs, hip.ptr(qo),
             hip.ptr(ko), hip.ptr(rq), hip.ptr(rk), hip.ptr(live), hip.stream())
    return qo, ko, rq, rk, live


def row_norm_bwd(gq, gk, q, k, wq, wk, rstd_q, rstd_k, live=None):
    """`head_norm_bwd` for the row-wide norms: gradients of the pre-norm q / k from those of the normed, un-rotated ones, in
    [B, T, H, hd] memory order.  live: the vector the forward used."""
    B, Hq, T, hd = q.shape
    Hk = k.shape[1]
    if gq.stride(-1) != 1 or any(s % 8 for s in gq.stride()[:3]):
        gq = gq.contiguous()
    if gk.stride(-1) != 1 or any(s % 8 for s in gk.stride()[:3]):
        gk = gk.contiguous()
    dq, dk = _token_major(B, Hq, T, hd, q), _token_major(B, Hk, T, hd, k)
    hip.call("dalm_row_norm_bwd", hip.ptr(gq), hip.ptr(gk), hip.ptr(q), hip.ptr(k), hip.ptr(wq), hip.ptr(wk), hip.dtype_code(wq),
             hip.ptr(rstd_q), hip.ptr(rstd_k), B, T, Hq, Hk, hd, _strides3(gq), _strides3(gk), _strides3(q), _strides3(k), _strides3(dq),
             _strides3(dk), hip.ptr(dq), hip.ptr(dk), hip.ptr(live), hip.stream())
    return dq, dk


def row_norm_weight_grad(g, x, rstd, live=None):
    """Gradient of a row-norm weight [H hd] (the kernels produce none): sum over (b, t) of g * xh, `_olmo2_weight_grad`'s arithmetic.
    g, x: [B, H, T, hd]; rstd: [B, T]."""
    B, H, T, hd = x.shape
    dead = None if live is None else (live == 0).view(B, 1, T, 1)      # dead rows: g is whatever the attention backward left
    return _olmo2_weight_grad(g, x, rstd.view(B, 1, T, 1), dead, (0, 2)).reshape(H * hd)


# ---------------------------------------------------------------------------
# Falcon decoder layer: LayerNorm, erf-GELU and the three-way residual add (dalm_amd/csrc/falcon.hip), bf16 activations
# ---------------------------------------------------------------------------
def layer_norm_supported(x: torch.Tensor, w: torch.Tensor, b) -> bool:
    D = x.shape[-1]
    return (x.is_cuda and x.dtype == torch.bfloat16 and w.dim() == 1 and w.shape[0] == D and w.dtype == torch.bfloat16
            and (b is None or (b.dtype == torch.bfloat16 and b.shape == w.shape)) and D % 8 == 0 and D <= 8192)


class _LayerNormRes(torch.autograd.Function):
    """(x, y) = (x, LayerNorm(x) in the activation dtype); x is handed back so that the gradient reaching it through the
    residual path is added INSIDE the norm's backward kernel (as `_AddRmsNorm` with delta None)."""

    @staticmethod
    def forward(ctx, x, w, b, eps):
        D = x.shape[-1]
        x2 = _as_rows(x, D, x.dtype)
        R = x2.shape[0]
        y = torch.empty_like(x2)
        mean = torch.empty(R, device=x.device, dtype=torch.float32)
        rstd = torch.empty(R, device=x.device, dtype=torch.float32)
        hip.call("dalm_layer_norm_fwd", hip.ptr(x2), hip.ptr(w), hip.ptr(b), R, D, float(eps), hip.ptr(y), hip.ptr(mean),
                 hip.ptr(rstd), hip.stream())
        ctx.save_for_backward(x2, w, mean, rstd)
        ctx.shape, ctx.has_bias = x.shape, b is not None
        return x, y.view(x.shape)

    @staticmethod
    def backward(ctx, dres, dy):
        x2, w, mean, rstd = ctx.saved_tensors
        R, D = x2.shape
        if dy is None:
            return dres, None, None, None
        dy2 = _as_rows(dy, D, x2.dtype)
        dres2 = _as_rows(dres, D, x2.dtype) if dres is not None else None
        dx = torch.empty_like(x2)
        hip.call("dalm_layer_norm_bwd", hip.ptr(dy2), hip.ptr(x2), hip.ptr(w), hip.ptr(mean), hip.ptr(rstd), hip.ptr(dres2), R, D,
                 hip.ptr(dx), hip.stream())
        dw = db = None
        if ctx.needs_input_grad[1]:
            xh = (x2.float() - mean.unsqueeze(1)) * rstd.unsqueeze(1)
            dw = (dy2.float() * xh).sum(0).to(w.dtype)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = dy2.float().sum(0).to(w.dtype)
        return dx.view(ctx.shape), dw, db, None


def layer_norm_res(x, w, b, eps):
    """(x, LayerNorm(x)): one launch forward, one backward (which also folds in the residual-path gradient)."""
    return _LayerNormRes.apply(x, w, b, eps)


def flat_bf16_supported(*ts) -> bool:
    t0 = ts[0]
    return all(t.is_cuda and t.dtype == torch.bfloat16 and t.shape == t0.shape for t in ts) and t0.numel() % 8 == 0


class _Gelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        hip.require_gpu(x)
        x = x.contiguous()
        y = torch.empty_like(x)
        hip.call("dalm_gelu_fwd", hip.ptr(x), hip.ptr(y), x.numel(), hip.stream())
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        hip.call("dalm_gelu_bwd", hip.ptr(dy), hip.ptr(x), hip.ptr(dx), x.numel(), hip.stream())
        return dx


def gelu(x):
    """0.5 x (1 + erf(x / sqrt 2)), bf16 in and out, f32 arithmetic."""
    return _Gelu.apply(x)


class _Add3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, c):
        hip.require_gpu(a, b, c)
        a, b, c = a.contiguous(), b.contiguous(), c.contiguous()
        out = torch.empty_like(a)
        hip.call("dalm_add3", hip.ptr(a), hip.ptr(b), hip.ptr(c), hip.ptr(out), a.numel(), hip.stream())
        return out

    @staticmethod
    def backward(ctx, g):
        return g, g, g


def add3(a, b, c):
    """c + (a + b), the inner sum rounded to bf16 first (what `a += b; c + a` leaves)."""
    return _Add3.apply(a, b, c)
