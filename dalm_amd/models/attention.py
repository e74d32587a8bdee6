"""Scaled-dot-product attention of the generator tower with a hand-written HIP BACKWARD (`dalm_attn_bwd`,
dalm_amd/csrc/attn.hip), registered with transformers as the attention implementation "dalm_sdpa".

transformers evaluates a decoder layer's attention through `sdpa_attention_forward`
(transformers/integrations/sdpa_attention.py) -> torch.nn.functional.scaled_dot_product_attention; the reference reaches it through
`self.generator_model(...)` (dalm/models/rag_e2e_base_model.py:104-106) and differentiates it in `loss.backward()`
(dalm/training/rag_e2e/train_rage2e.py:466).  Head widths 128 (Llama-2-7b), 64 (bge-large / BERT; Falcon-7b through fastpath's
FalconAttention patch) and 32 (bge-small, e5-small, gte-small, all-MiniLM: hidden 384, 12 heads - equal heads, no fused rotary
epilogue, no grouped heads: `rope_fusable` and `grouped_supported` decline that width).  With HF's boolean mask (causal + left padding) torch runs its memory-efficient
kernels: 60 us forward, 440 us backward per layer at cfg3 (2.7 % of the MFMA peak).  Here

  forward   `dalm_attn_fwd` (one launch, online softmax, writes the rows' log-sum-exp);  DALM_ATTN_FWD_KERNEL=0: torch's own
            memory-efficient kernel called as the aten op so that its log-sum-exp comes back
            (`aten::_scaled_dot_product_efficient_attention`, the values of F.scaled_dot_product_attention bit for bit);
  backward  `dalm_attn_bwd`: two launches.
Both read the mask as packed bits (packed once per mask tensor - every layer passes the same one) and skip dead 32 x 32 tiles.

Attention dropout (BERT's attention_probs_dropout_prob in training mode) is applied inside the kernels, its keep mask regenerated
from (a device seed word, a per-call salt, the element index) and never stored - this library's own generator
(oracle/attn_dropout.py), not torch's philox stream.  Not supported under activation recompute (torch.utils.checkpoint): the
salt is a host call counter, a re-run forward would draw another mask.
Grouped-query heads (Llama-3 / Mistral / TinyLlama: k, v with Hkv < H heads) run un-expanded on `dalm_attn_gqa_fwd` /
`dalm_attn_gqa_bwd` where `grouped_supported` holds: query head h reads KV head h // (H // Hkv), dk / dv come back with Hkv heads,
summed over each group in f32 inside the kernel.  Elsewhere k / v are expanded by `repeat_kv` first.
Qwen3 (q_norm / k_norm over the head dimension in front of the rotary embedding) and OLMo-2 (q_norm / k_norm over the whole
projection width, in front of the head split) run norm + rotation + attention as one node, `norm_rope_sdpa`; a call that carries a `sliding_window` shorter than the sequence goes to transformers' own function.
MPNet (a per-head relative-position bias by column difference on top of BERT's attention) runs on `dalm_attn_rel_*` with the bias
as one [H, 2 Tc - 1] vector per forward: `rel_sdpa`, reached from fastpath's MPNetSelfAttention patch, not through "dalm_sdpa".
Everything the kernels do not take (CPU tensors, other head widths, odd T with dropout, float masks, a KV cache, no gradient wanted) goes
to transformers' own `sdpa_attention_forward`, unchanged.  DALM_ATTN_KERNEL=0 keeps the model on "sdpa".
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from .. import hip
from ..packed import packed_of
from .fastpath import _off
from .lora import dropout_salt

NAME = "dalm_sdpa"
_HEAD_DIMS = (32, 64, 128)             # what dalm_attn_fwd / _bwd and their packed forms take
_WIDE_HEAD_DIMS = (64, 128)            # what the rotary epilogues of dalm_attn_bwd and the grouped entry points (dalm_attn_gqa_*) take


class _MaskPack:
    """What the kernels read of one mask tensor: bias (for torch's forward), row / column bit words, live tiles."""

    __slots__ = ("mask", "key", "bias", "rows", "cols", "live", "packed")


_last: list = [None]          # the pack of the mask seen last: one forward pass hands the same tensor object to every layer


def _pack(mask: Optional[torch.Tensor], B: int, H: int, T: int, causal: bool, dtype, device) -> _MaskPack:
    seqs = packed_of(mask)
    if seqs is not None:                       # packed (un-padded) call: the words come from the sequence list (dalm_amd/packed.py)
        pk = _MaskPack()
        pk.mask, pk.key, pk.bias, pk.packed = mask, None, None, seqs
        pk.rows, pk.cols, pk.live = seqs.bits()
        return pk
    key = (None if mask is None else (mask.data_ptr(), mask._version, tuple(mask.shape), tuple(mask.stride())), B, T, causal,
           dtype, device, torch.cuda.current_stream(device).cuda_stream)
    cur = _last[0]
    if cur is not None and cur.mask is mask and cur.key == key:
        return cur
    pk = _MaskPack()
    pk.mask, pk.key = mask, key
    W = (T + 31) // 32
    pk.rows = torch.empty(B * 32 * W * W, dtype=torch.int32, device=device)
    pk.cols = torch.empty_like(pk.rows)
    pk.live = torch.empty(B * W * W, dtype=torch.uint8, device=device)
    pk.bias = None
    pk.packed = None
    if mask is None:
        hip.call("dalm_attn_mask_bits", None, B, T, 0, 0, int(causal), hip.ptr(pk.rows), hip.ptr(pk.cols), hip.ptr(pk.live), hip.stream())
    else:
        m = mask if mask.stride(-1) == 1 else mask.contiguous()
        hip.call("dalm_attn_mask_bits", hip.ptr(m), B, T, m.stride(0), m.stride(2), int(causal), hip.ptr(pk.rows), hip.ptr(pk.cols),
                 hip.ptr(pk.live), hip.stream())
    _last[0] = pk
    return pk


def _torch_bias(pk: _MaskPack, B: int, H: int, T: int, dtype, device):
    """torch's own conversion of a boolean mask (aten convert_boolean_attn_mask): 0 where attended, -inf elsewhere; the last
    dimension's allocation padded to a multiple of 8 elements as its memory-efficient kernel wants the bias aligned."""
    if pk.mask is None:
        return None
    if pk.bias is None:
        m = pk.mask
        Ta = (T + 7) // 8 * 8
        bias = torch.zeros(B, 1, T, Ta, dtype=dtype, device=device)[..., :T]
        bias.masked_fill_(m.logical_not(), float("-inf"))
        pk.bias = bias.expand(B, H, T, T)
    return pk.bias


def _strides3(t: torch.Tensor):
    return [t.stride(0), t.stride(1), t.stride(2)]


def _dense_like(t: torch.Tensor) -> torch.Tensor:
    out = torch.empty_like(t)                       # preserve_format: the [B, T, H, hd] memory of the projections' views
    if out.stride(-1) != 1:
        out = torch.empty(t.shape, dtype=t.dtype, device=t.device)
    return out


def _grouped(q, k) -> bool:
    """k (and v) carry Hkv heads, 1 < Hkv < H: the grouped entry points.  (One KV head arrives as stride-0 views with H heads.)"""
    return k.shape[1] != q.shape[1] and k.shape[1] > 1


def _attn_forward_grouped(q, k, v, pk, scale):
    B, H, T, hd = q.shape
    sq = pk.packed
    nseq, Tm = (B, T) if sq is None else (sq.nseq, sq.T)
    out = torch.empty(B, T, H, hd, dtype=q.dtype, device=q.device).transpose(1, 2)
    lse = torch.empty(nseq, H, Tm, dtype=torch.float32, device=q.device)
    flat = []
    for t in (q, k, v, out):
        flat += _strides3(t)
    hip.call("dalm_attn_gqa_fwd", hip.ptr(q), hip.ptr(k), hip.ptr(v), hip.ptr(pk.rows), hip.ptr(pk.live),
             None if sq is None else hip.ptr(sq.cu), nseq, H, k.shape[1], Tm, hd, float(scale), (C.c_int64 * 12)(*flat), hip.ptr(out),
             hip.ptr(lse), hip.stream())
    return out, lse


_gqa_splits = [0]           # 0: the library's choice by grid size (dalm_attn_gqa_bwd_splits); tests set 1 or a divisor of H // Hkv


def _attn_backward_grouped(q, k, v, out, lse, d_out, pk, scale, cos, sin):
    B, H, T, hd = q.shape
    sq = pk.packed
    nseq, Tm = (B, T) if sq is None else (sq.nseq, sq.T)
    dq, dk, dv = _dense_like(q), _dense_like(k), _dense_like(v)          # dk, dv: Hkv heads
    delta = torch.empty(nseq, H, Tm, dtype=torch.float32, device=q.device)
    flat = []
    for t in (q, k, v, out, d_out, dq, dk, dv):
        flat += _strides3(t)
    cs_b = 0 if (cos is None or sq is not None or cos.shape[0] == 1) else cos.stride(0)
    lib = hip.load()
    splits = _gqa_splits[0] or int(lib.dalm_attn_gqa_bwd_splits(nseq, H, k.shape[1], Tm))
    ws_bytes = int(lib.dalm_attn_gqa_bwd_workspace_bytes(B * T, k.shape[1], hd, splits))       # B T: the token rows of k / v
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=q.device) if ws_bytes else None
    hip.call("dalm_attn_gqa_bwd", hip.ptr(q), hip.ptr(k), hip.ptr(v), hip.ptr(out), hip.ptr(d_out), hip.ptr(lse), hip.ptr(pk.rows),
             hip.ptr(pk.cols), hip.ptr(pk.live), None if sq is None else hip.ptr(sq.cu), nseq, H, k.shape[1], Tm, hd, float(scale),
             (C.c_int64 * 24)(*flat), hip.ptr(cos), hip.ptr(sin), cs_b, 0 if cos is None else cos.stride(1), splits,
             hip.ptr(ws), ws_bytes, hip.ptr(dq), hip.ptr(dk), hip.ptr(dv), hip.ptr(delta), hip.stream())
    return dq, dk, dv


def _attn_forward(q, k, v, pk, scale, causal, drop=(0.0, None, 0)):
    B, H, T, hd = q.shape
    if _grouped(q, k):
        if drop[0] != 0.0:
            raise ValueError("dalm_amd: grouped-query attention kernels take no dropout (expand k / v with repeat_kv)")
        return _attn_forward_grouped(q, k, v, pk, scale)
    if pk.packed is not None:                   # q, k, v: [1, H, n, hd] views of [n, H hd] projections; sequences from cu_seqlens
        sq = pk.packed
        out = torch.empty(1, T, H, hd, dtype=q.dtype, device=q.device).transpose(1, 2)
        lse = torch.empty(sq.nseq, H, sq.T, dtype=torch.float32, device=q.device)
        flat = []
        for t in (q, k, v, out):
            flat += _strides3(t)
        hip.call("dalm_attn_fwd_packed", hip.ptr(q), hip.ptr(k), hip.ptr(v), hip.ptr(pk.rows), hip.ptr(pk.live), hip.ptr(sq.cu),
                 sq.nseq, H, sq.T, hd, float(scale), (C.c_int64 * 12)(*flat), float(drop[0]), hip.ptr(drop[1]),
                 int(drop[2]) & 0xFFFFFFFF, hip.ptr(out), hip.ptr(lse), hip.stream())
        return out, lse
    if _off("DALM_ATTN_FWD_KERNEL") and drop[0] == 0.0:    # torch's memory-efficient forward + its log-sum-exp
        out, lse, _, _ = torch.ops.aten._scaled_dot_product_efficient_attention(
            q, k, v, _torch_bias(pk, B, H, T, q.dtype, q.device), True, 0.0, causal, scale=scale)
        return out, lse
    out = torch.empty(B, T, H, hd, dtype=q.dtype, device=q.device).transpose(1, 2)   # torch's layout: the caller's
    lse = torch.empty(B, H, T, dtype=torch.float32, device=q.device)                  # transpose(1, 2).contiguous() is free
    flat = []
    for t in (q, k, v, out):
        flat += _strides3(t)
    hip.call("dalm_attn_fwd", hip.ptr(q), hip.ptr(k), hip.ptr(v), hip.ptr(pk.rows), hip.ptr(pk.live), B, H, T, hd, float(scale),
             (C.c_int64 * 12)(*flat), float(drop[0]), hip.ptr(drop[1]), int(drop[2]) & 0xFFFFFFFF, hip.ptr(out), hip.ptr(lse),
             hip.stream())
    return out, lse


def _attn_backward(q, k, v, out, lse, d_out, pk, scale, cos=None, sin=None, drop=(0.0, None, 0)):
    B, H, T, hd = q.shape
    if d_out.stride(-1) != 1 or any(s % 8 for s in d_out.stride()[:3]):
        d_out = d_out.contiguous()
    if _grouped(q, k):
        return _attn_backward_grouped(q, k, v, out, lse, d_out, pk, scale, cos, sin)
    if pk.packed is not None:
        sq = pk.packed
        dq, dk, dv = _dense_like(q), _dense_like(k), _dense_like(v)
        delta = torch.empty(sq.nseq, H, sq.T, dtype=torch.float32, device=q.device)
        flat = []
        for t in (q, k, v, out, d_out, dq, dk, dv):
            flat += _strides3(t)
        hip.call("dalm_attn_bwd_packed", hip.ptr(q), hip.ptr(k), hip.ptr(v), hip.ptr(out), hip.ptr(d_out), hip.ptr(lse),
                 hip.ptr(pk.rows), hip.ptr(pk.cols), hip.ptr(pk.live), hip.ptr(sq.cu), sq.nseq, H, sq.T, hd, float(scale),
                 (C.c_int64 * 24)(*flat), hip.ptr(cos), hip.ptr(sin), 0 if cos is None else cos.stride(1), float(drop[0]),
                 hip.ptr(drop[1]), int(drop[2]) & 0xFFFFFFFF, hip.ptr(dq), hip.ptr(dk), hip.ptr(dv), hip.ptr(delta), hip.stream())
        return dq, dk, dv
    lse = lse if (lse.is_contiguous() and lse.shape[-1] == T) else lse[..., :T].contiguous()
    dq, dk, dv = _dense_like(q), _dense_like(k), _dense_like(v)
    delta = torch.empty(B, H, T, dtype=torch.float32, device=q.device)
    flat = []
    for t in (q, k, v, out, d_out, dq, dk, dv):
        flat += _strides3(t)
    cs_b = 0 if (cos is None or cos.shape[0] == 1) else cos.stride(0)
    hip.call("dalm_attn_bwd", hip.ptr(q), hip.ptr(k), hip.ptr(v), hip.ptr(out), hip.ptr(d_out), hip.ptr(lse), hip.ptr(pk.rows),
             hip.ptr(pk.cols), hip.ptr(pk.live), B, H, T, hd, float(scale), (C.c_int64 * 24)(*flat), hip.ptr(cos), hip.ptr(sin),
             cs_b, 0 if cos is None else cos.stride(1), float(drop[0]), hip.ptr(drop[1]), int(drop[2]) & 0xFFFFFFFF, hip.ptr(dq),
             hip.ptr(dk), hip.ptr(dv), hip.ptr(delta), hip.stream())
    return dq, dk, dv


class _SdpaHipBackward(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, mask, scale, causal, dropout_p=0.0, salt=0):
        B, H, T, hd = q.shape
        pk = _pack(mask, B, H, T, causal, q.dtype, q.device)
        drop = (0.0, None, 0)
        if dropout_p > 0.0:
            # this STEP's copy of the device seed word (8 bytes, capturable): the step advances the word itself, a backward that
            # runs after the next advance must still see the forward's value.  Taken per advance, not per mask pack: a pack that
            # is re-used across steps (attention_mask=None: same key every step) must not freeze the seed
            from . import lora_ops

            drop = (float(dropout_p), lora_ops.dropout_seed_snapshot(q.device), int(salt))
        out, lse = _attn_forward(q, k, v, pk, scale, causal, drop)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.pack, ctx.scale, ctx.drop = pk, scale, drop
        return out

    @staticmethod
    def backward(ctx, d_out):
        q, k, v, out, lse = ctx.saved_tensors
        dq, dk, dv = _attn_backward(q, k, v, out, lse, d_out, ctx.pack, ctx.scale, drop=ctx.drop)
        return dq, dk, dv, None, None, None, None, None


class _RopeSdpaHip(torch.autograd.Function):
    """rotary embedding of q and k (`dalm_rope_qk`, one launch) + the attention; the backward of the rotation happens in the
    epilogues of `dalm_attn_bwd` (no launch of its own, the rotated gradients never reach memory)."""

    @staticmethod
    def forward(ctx, q, k, v, cos, sin, mask, scale, causal):
        from . import tower_ops

        B, H, T, hd = q.shape
        from .. import live_rows

        # dead (b, t) of a padded tower call leave the rotation as zeros (the attention kernels read finite values; the
        # rotation's backward is inside dalm_attn_bwd, which is not row-aware)
        q2, k2 = tower_ops._rope_launch(q, k, cos, sin, False, live_rows.current(B * T, q.device))
        pk = _pack(mask, B, H, T, causal, q.dtype, q.device)
        # multi-query (ONE key / value head, Falcon-7B): the kernels read it through stride-0 head views - nothing is broadcast
        # in memory; the backward kernels write per-head dk / dv, summed over the heads below.  Grouped heads (1 < Hkv < H) go
        # straight through: `_attn_forward` / `_attn_backward` take them to the grouped entry points, dk / dv return with Hkv heads
        ctx.mqa = k.shape[1] == 1 and H > 1
        kx = k2.expand(B, H, T, hd) if ctx.mqa else k2
        vx = v.expand(B, H, T, hd) if ctx.mqa else v
        out, lse = _attn_forward(q2, kx, vx, pk, scale, causal)
        ctx.save_for_backward(q2, k2, v, out, lse, cos, sin)
        ctx.pack, ctx.scale = pk, scale
        return out

    @staticmethod
    def backward(ctx, d_out):
        q2, k2, v, out, lse, cos, sin = ctx.saved_tensors
        if ctx.mqa:
            B, H, T, hd = q2.shape
            dq, dk, dv = _attn_backward(q2, k2.expand(B, H, T, hd), v.expand(B, H, T, hd), out, lse, d_out, ctx.pack, ctx.scale, cos, sin)
            return dq, dk.sum(dim=1, keepdim=True), dv.sum(dim=1, keepdim=True), None, None, None, None, None
        dq, dk, dv = _attn_backward(q2, k2, v, out, lse, d_out, ctx.pack, ctx.scale, cos, sin)
        return dq, dk, dv, None, None, None, None, None


class _NormRopeSdpaHip(torch.autograd.Function):
    """q_norm / k_norm + rotary embedding (one launch) + the attention.  The norms are RMSNorms over the head dimension (Qwen3:
    `dalm_head_norm_rope_fwd`) or - `row_wide` - over the whole projection width of a token, all heads (OLMo-2:
    `dalm_row_norm_rope_fwd`).  Backward: `dalm_attn_bwd` / `dalm_attn_gqa_bwd` un-rotate dq / dk in their epilogues (as for
    `_RopeSdpaHip`), then `dalm_head_norm_bwd` / `dalm_row_norm_bwd` (one launch) takes them through the two norms.  Equal and
    grouped heads, padded and packed; one key / value head is not routed here (`supported` / `grouped_supported` decline it).  No
    host synchronisation."""

    @staticmethod
    def forward(ctx, q, k, v, wq, wk, eps_q, eps_k, cos, sin, mask, scale, causal, row_wide=False):
        from . import tower_ops

        B, H, T, hd = q.shape
        # dead (b, t) of a padded tower call leave norm + rotation as zeros (finite values for the attention kernels) and get
        # zero gradients from the norm's backward
        norm_rope = tower_ops.row_norm_rope if row_wide else tower_ops.head_norm_rope
        q2, k2, rq, rk, live = norm_rope(q, k, wq, wk, eps_q, eps_k, cos, sin)
        pk = _pack(mask, B, H, T, causal, q.dtype, q.device)
        out, lse = _attn_forward(q2, k2, v, pk, scale, causal)
        ctx.save_for_backward(q, k, q2, k2, v, out, lse, cos, sin, wq, wk, rq, rk, *([live] if live is not None else []))
        ctx.pack, ctx.scale, ctx.row_wide = pk, scale, row_wide
        return out

    @staticmethod
    def backward(ctx, d_out):
        from . import tower_ops

        q, k, q2, k2, v, out, lse, cos, sin, wq, wk, rq, rk, *live = ctx.saved_tensors
        live = live[0] if live else None
        norm_bwd, weight_grad = ((tower_ops.row_norm_bwd, tower_ops.row_norm_weight_grad) if ctx.row_wide
                                 else (tower_ops.head_norm_bwd, tower_ops.head_norm_weight_grad))
        gq, gk, dv = _attn_backward(q2, k2, v, out, lse, d_out, ctx.pack, ctx.scale, cos, sin)    # of the normed, un-rotated q / k
        dq, dk = norm_bwd(gq, gk, q, k, wq, wk, rq, rk, live)
        dwq = weight_grad(gq, q, rq, live).to(wq.dtype) if ctx.needs_input_grad[3] else None
        dwk = weight_grad(gk, k, rk, live).to(wk.dtype) if ctx.needs_input_grad[4] else None
        return dq, dk, dv, dwq, dwk, None, None, None, None, None, None, None, None


def norm_rope_sdpa(query, key, value, wq, wk, eps_q: float, eps_k: float, cos, sin, mask, scale: float, causal: bool,
                   row_wide: bool = False):
    """sdpa(apply_rotary_pos_emb(rmsnorm(query) * wq, rmsnorm(key) * wk, cos, sin), value, ...) with the norms over the head
    dimension (Qwen3's q_norm / k_norm) or, `row_wide`, over all heads of a token (OLMo-2's), for what
    `tower_ops.head_norm_rope_supported` / `tower_ops.row_norm_rope_supported`, `rope_fusable` and `node_supported` accept.  The
    norm weights may require grad."""
    return _NormRopeSdpaHip.apply(query, key, value, wq, wk, eps_q, eps_k, cos, sin, mask, scale, causal, row_wide)


def rope_fusable(q, k, cos, sin) -> bool:
    """cos / sin tables `dalm_attn_bwd` reads in its epilogues: what `tower_ops.rope_supported` takes, bf16, 16-byte rows."""
    from . import tower_ops

    return (q.shape[-1] in _WIDE_HEAD_DIMS                      # width 32: separate rotary kernels (tower_ops.rope_qk)
            and tower_ops.rope_supported(q, k, cos, sin) and cos.dtype == torch.bfloat16 and cos.shape[-1] == q.shape[-1]
            and cos.stride(1) % 8 == 0 and (cos.shape[0] == 1 or cos.stride(0) % 8 == 0)
            and cos.data_ptr() % 16 == 0 and sin.data_ptr() % 16 == 0
            and k.shape[0] == q.shape[0] and k.shape[2:] == q.shape[2:] and k.shape[1] >= 1 and q.shape[1] % k.shape[1] == 0)


def rope_sdpa(query, key, value, cos, sin, mask, scale: float, causal: bool):
    """sdpa(apply_rotary_pos_emb(query, key, cos, sin), value, ...) for what `node_supported` and `rope_fusable` accept."""
    return _RopeSdpaHip.apply(query, key, value, cos, sin, mask, scale, causal)


class _RopeIlSdpaHip(torch.autograd.Function):
    """Cohere's interleaved rotary embedding of q and k (`dalm_rope_il_qk`, one launch) + the attention.  The rotary epilogues of
    `dalm_attn_bwd` are Llama's half-split rotation, so the backward calls it WITHOUT tables - dq / dk then are the gradients of
    the rotated q / k - and un-rotates them with one more `dalm_rope_il_qk` launch (backward = 1, in place).  Equal and grouped
    heads, padded and packed; one key / value head is not routed here (`supported` / `grouped_supported` decline it)."""

    @staticmethod
    def forward(ctx, q, k, v, cos, sin, mask, scale, causal):
        from . import tower_ops
        from .. import live_rows

        B, H, T, hd = q.shape
        # dead (b, t) of a padded tower call leave the rotation as zeros (the attention kernels read finite values) and get zero
        # gradients from the un-rotation
        live = live_rows.current(B * T, q.device)
        q2, k2 = tower_ops._rope_il_launch(q, k, cos, sin, False, live)
        pk = _pack(mask, B, H, T, causal, q.dtype, q.device)
        out, lse = _attn_forward(q2, k2, v, pk, scale, causal)
        ctx.save_for_backward(q2, k2, v, out, lse, cos, sin, *([live] if live is not None else []))
        ctx.pack, ctx.scale = pk, scale
        return out

    @staticmethod
    def backward(ctx, d_out):
        from . import tower_ops

        q2, k2, v, out, lse, cos, sin, *live = ctx.saved_tensors
        dq, dk, dv = _attn_backward(q2, k2, v, out, lse, d_out, ctx.pack, ctx.scale)       # of the ROTATED q / k: no tables
        dq, dk = tower_ops._rope_il_launch(dq, dk, cos, sin, True, live[0] if live else None, in_place=True)
        return dq, dk, dv, None, None, None, None, None


def rope_il_sdpa(query, key, value, cos, sin, mask, scale: float, causal: bool):
    """sdpa(modeling_cohere.apply_rotary_pos_emb(query, key, cos, sin), value, ...) for what `node_supported` and
    `tower_ops.rope_il_supported` accept."""
    return _RopeIlSdpaHip.apply(query, key, value, cos, sin, mask, scale, causal)


class _RopePartialSdpaHip(torch.autograd.Function):
    """Phi-3's partial rotary embedding of q and k (`dalm_rope_partial_qk`, one launch) + the attention.  The rotary epilogues of
    `dalm_attn_bwd` pair i with i + hd/2 over tables of width hd, so - as in `_RopeIlSdpaHip` - the backward calls it WITHOUT
    tables and un-rotates dq / dk with one more `dalm_rope_partial_qk` launch (backward = 1, in place: the pass part of the
    gradients is already what it has to be).  Equal and grouped heads, padded and packed; one key / value head is not routed
    here (`supported` / `grouped_supported` decline it)."""

    @staticmethod
    def forward(ctx, q, k, v, cos, sin, mask, scale, causal):
        from . import tower_ops
        from .. import live_rows

        B, H, T, hd = q.shape
        # dead (b, t) of a padded tower call leave the rotation as zeros over the whole head (the attention kernels read finite
        # values); their dq / dk rows are left as the attention backward wrote them
        live = live_rows.current(B * T, q.device)
        q2, k2 = tower_ops._rope_partial_launch(q, k, cos, sin, False, live)
        pk = _pack(mask, B, H, T, causal, q.dtype, q.device)
        out, lse = _attn_forward(q2, k2, v, pk, scale, causal)
        ctx.save_for_backward(q2, k2, v, out, lse, cos, sin, *([live] if live is not None else []))
        ctx.pack, ctx.scale = pk, scale
        return out

    @staticmethod
    def backward(ctx, d_out):
        from . import tower_ops

        q2, k2, v, out, lse, cos, sin, *live = ctx.saved_tensors
        dq, dk, dv = _attn_backward(q2, k2, v, out, lse, d_out, ctx.pack, ctx.scale)       # of the ROTATED q / k: no tables
        dq, dk = tower_ops._rope_partial_launch(dq, dk, cos, sin, True, live[0] if live else None, in_place=True)
        return dq, dk, dv, None, None, None, None, None


def rope_partial_sdpa(query, key, value, cos, sin, mask, scale: float, causal: bool):
    """sdpa(modeling_phi3.apply_rotary_pos_emb(query, key, cos, sin), value, ...) with cos.shape[-1] < head_dim, for what
    `node_supported` and `tower_ops.rope_partial_supported` accept."""
    return _RopePartialSdpaHip.apply(query, key, value, cos, sin, mask, scale, causal)


def _views_ok(*ts) -> bool:
    return all(t.stride(-1) == 1 and all(s % 8 == 0 for s in t.stride()[:3]) and t.data_ptr() % 16 == 0 for t in ts)


def supported(query, key, value, mask, dropout, causal, kwargs) -> bool:
    if not (query.is_cuda and query.dtype == torch.bfloat16 and key.dtype == query.dtype and value.dtype == query.dtype):
        return False
    if query.dim() != 4 or query.shape[-1] not in _HEAD_DIMS or key.shape != query.shape or value.shape != query.shape:
        return False                                 # a KV cache (kv length != q length) or grouped heads left unexpanded
    if query.shape[2] < 2 or query.shape[2] > 2048 or kwargs.get("position_bias") is not None:
        return False
    if dropout != 0.0 and not (0.0 < dropout < 1.0 and query.shape[2] % 2 == 0):
        return False                                 # the in-kernel mask pairs elements (i, j), (i, j + 1): even T
    if not (torch.is_grad_enabled() and (query.requires_grad or key.requires_grad or value.requires_grad)):
        return False                                 # nothing to differentiate: torch's fused forward alone is the best path
    B, _, T, _ = query.shape
    if mask is None:
        pass                                         # causal, or fully bidirectional (an encoder batch without padding)
    elif not (mask.dtype == torch.bool and mask.dim() == 4 and tuple(mask.shape) == (B, 1, T, T) and mask.is_cuda and not causal):
        return False
    return _views_ok(query, key, value)


def packed_supported(query, key, value, dropout: float = 0.0) -> bool:
    """What `dalm_attn_*_packed` take: [1, H, n, hd] bf16 views with 16-byte aligned rows, head width 32 / 64 / 128."""
    if not (query.is_cuda and query.dtype == torch.bfloat16 and key.dtype == query.dtype and value.dtype == query.dtype):
        return False
    if query.dim() != 4 or query.shape[0] != 1 or query.shape[-1] not in _HEAD_DIMS or key.shape != query.shape \
            or value.shape != query.shape:
        return False
    if dropout != 0.0 and not 0.0 < dropout < 1.0:
        return False
    return _views_ok(query, key, value) and not _off("DALM_ATTN_KERNEL")


_MAX_GROUP = 16


def group_ok(H: int, Hkv: int) -> bool:
    """Head counts the grouped kernels are routed for: 1 < Hkv < H, whole groups of at most 16 query heads."""
    return 1 < Hkv < H and H % Hkv == 0 and H // Hkv <= _MAX_GROUP


def grouped_supported(query, key, value, mask=None, dropout: float = 0.0, causal: bool = False, kwargs=None, packed: bool = False) -> bool:
    """What `dalm_attn_gqa_*` take un-expanded: key / value with Hkv heads, 1 < Hkv < H, H % Hkv == 0, H / Hkv <= 16, no dropout,
    head width 64 / 128, and everything `supported` (`packed_supported` for a packed call) asks of equal heads."""
    if query.dim() != 4 or key.dim() != 4 or key.shape != value.shape or dropout != 0.0:
        return False
    if query.shape[-1] not in _WIDE_HEAD_DIMS:       # width 32: k / v are expanded by repeat_kv and run on the equal-heads kernels
        return False
    if not group_ok(query.shape[1], key.shape[1]):
        return False
    if key.shape[0] != query.shape[0] or key.shape[2:] != query.shape[2:] or not _views_ok(key, value):
        return False
    if _off("DALM_ATTN_FWD_KERNEL"):                 # torch's forward knows equal heads only
        return False
    # the remaining conditions are those of equal heads: asked of head views with the query's shape
    kx, vx = key[:, :1].expand(query.shape), value[:, :1].expand(query.shape)
    if packed:
        return packed_supported(query, kx, vx, dropout)
    return supported(query, kx, vx, mask, dropout, causal, kwargs or {})


def node_supported(query, key, value, mask, causal: bool) -> bool:
    """Whether the attention of a rotary + attention node (`rope_sdpa`, `norm_rope_sdpa`; no dropout) can run on these tensors:
    equal heads or grouped heads left un-expanded, padded or - `mask` a packed descriptor - packed.  The callers ask
    `rope_fusable` as well."""
    if packed_of(mask) is not None:
        return packed_supported(query, key, value) or grouped_supported(query, key, value, packed=True)
    return supported(query, key, value, mask, 0.0, causal, {}) or grouped_supported(query, key, value, mask, 0.0, causal, {})


def _packed_sdpa_torch(query, key, value, seqs, scale: float, dropout: float):
    """The packed attention without the kernels (CPU tensors, fp32, head widths they do not take): re-pad q / k / v to
    [nseq, H, T, hd] by index, torch's SDPA under the mask the sequence list describes, rows gathered back.  A row without a
    live key attends itself and its output is zeroed afterwards - every intermediate stays finite, and the result is what the
    kernels (and torch's memory-efficient kernels on the padded layout) return for such rows: 0."""
    _, H, n, hd = query.shape
    slot, gather = seqs.padded_index()
    nseq, T = seqs.nseq, seqs.T

    def pad(t):                                                   # [1, H, n, hd] -> [nseq, H, T, hd]
        rows = torch.cat((t[0].transpose(0, 1), t.new_zeros((1, H, hd))), dim=0)           # [n + 1, H, hd]
        return rows.index_select(0, gather).view(nseq, T, H, hd).transpose(1, 2)

    kl = torch.cat((seqs.key_live != 0, seqs.key_live.new_zeros((1,), dtype=torch.bool))).index_select(0, gather).view(nseq, 1, 1, T)
    mask = kl.expand(nseq, 1, T, T)
    if seqs.causal:
        mask = mask & torch.ones((T, T), dtype=torch.bool, device=query.device).tril()
    has_key = mask.any(dim=-1, keepdim=True)                                                  # [nseq, 1, T, 1]
    mask = mask | (~has_key & torch.eye(T, dtype=torch.bool, device=query.device))
    out = torch.nn.functional.scaled_dot_product_attention(pad(query), pad(key), pad(value), attn_mask=mask, dropout_p=dropout,
                                                           scale=scale)
    out = torch.where(has_key, out, torch.zeros_like(out))
    return out.transpose(1, 2).reshape(nseq * T, H, hd).index_select(0, slot).unsqueeze(0)  # [1, n, H, hd]


def _packed_attention(module, query, key, value, attention_mask, seqs, dropout, scaling):
    from transformers.integrations.sdpa_attention import repeat_kv

    groups = getattr(module, "num_key_value_groups", 1)
    native = groups > 1 and key.shape[1] != query.shape[1] and grouped_supported(query, key, value, dropout=dropout, packed=True)
    if groups > 1 and key.shape[1] != query.shape[1] and not native:
        key, value = repeat_kv(key, groups), repeat_kv(value, groups)
    scale = float(scaling) if scaling is not None else float(query.shape[-1]) ** -0.5
    if native or packed_supported(query, key, value, dropout):
        salt = dropout_salt(module, "_dalm_attn_calls") if dropout > 0.0 else 0
        out = _SdpaHipBackward.apply(query, key, value, attention_mask, scale, False, float(dropout), salt)
        return out.transpose(1, 2).contiguous(), None
    return _packed_sdpa_torch(query, key, value, seqs, scale, float(dropout)), None


def dalm_sdpa_attention_forward(module, query, key, value, attention_mask, dropout: float = 0.0, scaling: Optional[float] = None,
                                is_causal: Optional[bool] = None, **kwargs):
    """Same contract as transformers' `sdpa_attention_forward`: ([B, T, H, hd] output, None)."""
    from transformers.integrations.sdpa_attention import repeat_kv, sdpa_attention_forward

    seqs = packed_of(attention_mask)
    if seqs is not None:                     # packed (un-padded) tower call: `attention_mask` is a descriptor, not a mask
        return _packed_attention(module, query, key, value, attention_mask, seqs, dropout, scaling)
    window = kwargs.get("sliding_window")        # Qwen3 passes the keyword: None unless the layer is a `sliding_attention` one
    if window is not None and window < key.shape[2]:     # the kernels know no window shorter than the sequence
        return sdpa_attention_forward(module, query, key, value, attention_mask, dropout=dropout, scaling=scaling,
                                      is_causal=is_causal, **kwargs)
    groups = getattr(module, "num_key_value_groups", 1)
    causal = bool(query.shape[2] > 1 and attention_mask is None
                  and (is_causal if is_causal is not None else getattr(module, "is_causal", True)))
    grouped = groups > 1 and key.shape[1] != query.shape[1]
    native = (grouped and not _off("DALM_ATTN_KERNEL")                 # grouped heads the kernels read un-expanded
              and grouped_supported(query, key, value, attention_mask, dropout, causal, kwargs))
    k2, v2 = (repeat_kv(key, groups), repeat_kv(value, groups)) if (grouped and not native) else (key, value)
    if _off("DALM_ATTN_KERNEL") or not (native or supported(query, k2, v2, attention_mask, dropout, causal, kwargs)):
        return sdpa_attention_forward(module, query, key, value, attention_mask, dropout=dropout, scaling=scaling,
                                      is_causal=is_causal, **kwargs)
    scale = float(scaling) if scaling is not None else float(query.shape[-1]) ** -0.5
    salt = dropout_salt(module, "_dalm_attn_calls") if dropout > 0.0 else 0
    out = _SdpaHipBackward.apply(query, k2, v2, attention_mask, scale, causal, float(dropout), salt)
    return out.transpose(1, 2).contiguous(), None


# ---------------------------------------------------------------------------------------------------------------------------
# Relative-position bias (MPNet): score = scale q.k + rel[h][col(j) - col(i) + Tc - 1] on `dalm_attn_rel_*`
# ---------------------------------------------------------------------------------------------------------------------------
# MPNetEncoder.compute_position_bias builds relative_attention_bias(bucket(j - i))[h] from positions arange(T): it ignores
# position_ids and padding, so the bias is a function of the head and the column difference only - a Toeplitz matrix per head.
# One f32 vector [H, 2 Tc - 1] per forward (Tc = the padded column count) replaces the [B, H, T, T] tensor; the kernels index it.
_bucket_index: dict = {}      # (encoder class, Tc, bucket count, device) -> int64 [2 Tc - 1]: bucket of every column difference


def rel_bias_vector(encoder, Tc: int, device=None) -> torch.Tensor:
    """[H, 2 Tc - 1] f32: entry [h, d + Tc - 1] = the bias of head h at column difference d = key column - query column, from the
    encoder's OWN `relative_position_bucket` (the formula is not restated here) and its table as it is NOW (gathered on every
    call; only the bucket index is cached per Tc)."""
    import inspect

    table = encoder.relative_attention_bias.weight
    device = table.device if device is None else torch.device(device)
    # the bucket count is compute_position_bias's default argument (the encoder calls it without one), not the table's row count
    buckets = int(inspect.signature(type(encoder).compute_position_bias).parameters["num_buckets"].default)
    key = (type(encoder), int(Tc), buckets, device)
    idx = _bucket_index.get(key)
    if idx is None:
        d = torch.arange(-(Tc - 1), Tc, dtype=torch.long)
        idx = type(encoder).relative_position_bucket(d, num_buckets=buckets).to(device)
        _bucket_index[key] = idx
    return table.detach().to(device=device, dtype=torch.float32).index_select(0, idx).t().contiguous()


class RelBiasSource:
    """What the routed `compute_position_bias` hands the layers in place of the [B, H, T, T] tensor: the encoder whose table holds
    the bias, and the vectors built from it during THIS forward (every layer asks for the same Tc)."""

    __slots__ = ("encoder", "_vec")

    def __init__(self, encoder):
        self.encoder, self._vec = encoder, {}

    def vector(self, Tc: int, device) -> torch.Tensor:
        key = (int(Tc), torch.device(device))
        if key not in self._vec:
            self._vec[key] = rel_bias_vector(self.encoder, Tc, device)
        return self._vec[key]


def tag_rel_bias(encoder) -> torch.Tensor:
    """The tagged stand-in for MPNet's position bias: the [H, buckets] table view (small), carrying its `RelBiasSource`."""
    t = encoder.relative_attention_bias.weight.detach().t()
    t._dalm_rel = RelBiasSource(encoder)
    return t


def rel_source_of(position_bias) -> Optional[RelBiasSource]:
    return getattr(position_bias, "_dalm_rel", None) if position_bias is not None else None


def expand_rel_bias(rel: torch.Tensor, cols_q: torch.Tensor, cols_k: Optional[torch.Tensor] = None) -> torch.Tensor:
    """rel [H, 2 Tc - 1] -> [..., H, Tq, Tk] with element rel[h, cols_k[j] - cols_q[i] + Tc - 1]; cols: int64 [..., T]."""
    cols_k = cols_q if cols_k is None else cols_k
    Tc = (rel.shape[1] + 1) // 2
    idx = cols_k.unsqueeze(-2) - cols_q.unsqueeze(-1) + (Tc - 1)                       # [..., Tq, Tk]
    return rel[:, idx].movedim(0, -3)


def _bool_key_mask(mask: torch.Tensor) -> torch.Tensor:
    """The boolean [B, 1, T, T] mask of an additive float mask (0 = attend), made ONCE per mask tensor: every layer of a forward
    passes the same tensor object, and the mask-bits cache (`_pack`) is keyed by the object it is handed."""
    if mask.dtype == torch.bool:
        return mask
    got = getattr(mask, "_dalm_bool", None)
    if got is None or got[0] != mask._version:
        got = (mask._version, mask == 0)
        mask._dalm_bool = got
    return got[1]


def _rel_launch_forward(q, k, v, pk, scale, rel, cols, drop):
    B, H, T, hd = q.shape
    sq = pk.packed
    nseq, Tm = (B, T) if sq is None else (sq.nseq, sq.T)
    out = torch.empty(B, T, H, hd, dtype=q.dtype, device=q.device).transpose(1, 2)
    lse = torch.empty(nseq, H, Tm, dtype=torch.float32, device=q.device)
    flat = []
    for t in (q, k, v, out):
        flat += _strides3(t)
    tail = (float(drop[0]), hip.ptr(drop[1]), int(drop[2]) & 0xFFFFFFFF, hip.ptr(out), hip.ptr(lse), hip.stream())
    relargs = (hip.ptr(rel), rel.stride(0), (rel.shape[1] + 1) // 2)
    if sq is None:
        hip.call("dalm_attn_rel_fwd", hip.ptr(q), hip.ptr(k), hip.ptr(v), hip.ptr(pk.rows), hip.ptr(pk.live), B, H, T, hd, float(scale),
                 (C.c_int64 * 12)(*flat), *relargs, *tail)
    else:
        hip.call("dalm_attn_rel_fwd_packed", hip.ptr(q), hip.ptr(k), hip.ptr(v), hip.ptr(pk.rows), hip.ptr(pk.live), hip.ptr(sq.cu),
                 nseq, H, Tm, hd, float(scale), (C.c_int64 * 12)(*flat), *relargs, hip.ptr(cols), *tail)
    return out, lse


def _rel_launch_backward(q, k, v, out, lse, d_out, pk, scale, rel, cols, drop):
    B, H, T, hd = q.shape
    if d_out.stride(-1) != 1 or any(s % 8 for s in d_out.stride()[:3]):
        d_out = d_out.contiguous()
    sq = pk.packed
    nseq, Tm = (B, T) if sq is None else (sq.nseq, sq.T)
    dq, dk, dv = _dense_like(q), _dense_like(k), _dense_like(v)
    delta = torch.empty(nseq, H, Tm, dtype=torch.float32, device=q.device)
    flat = []
    for t in (q, k, v, out, d_out, dq, dk, dv):
        flat += _strides3(t)
    head = (hip.ptr(q), hip.ptr(k), hip.ptr(v), hip.ptr(out), hip.ptr(d_out), hip.ptr(lse), hip.ptr(pk.rows), hip.ptr(pk.cols),
            hip.ptr(pk.live))
    tail = (float(drop[0]), hip.ptr(drop[1]), int(drop[2]) & 0xFFFFFFFF, hip.ptr(dq), hip.ptr(dk), hip.ptr(dv), hip.ptr(delta),
            hip.stream())
    relargs = (hip.ptr(rel), rel.stride(0), (rel.shape[1] + 1) // 2)
    if sq is None:
        hip.call("dalm_attn_rel_bwd", *head, B, H, T, hd, float(scale), (C.c_int64 * 24)(*flat), *relargs, *tail)
    else:
        hip.call("dalm_attn_rel_bwd_packed", *head, hip.ptr(sq.cu), nseq, H, Tm, hd, float(scale), (C.c_int64 * 24)(*flat), *relargs,
                 hip.ptr(cols), *tail)
    return dq, dk, dv


class _RelSdpaHip(torch.autograd.Function):
    """The attention with a relative-position bias vector on `dalm_attn_rel_*` (padded, or - `mask` a packed descriptor - packed).
    Shares the mask-bits cache (`_pack`) and the dropout salt counter with `_SdpaHipBackward`.  The bias is a constant of the step
    (a frozen table): the backward reads it to recompute P and returns no gradient for it."""

    @staticmethod
    def forward(ctx, q, k, v, rel, mask, scale, dropout_p=0.0, salt=0, cols=None):
        B, H, T, hd = q.shape
        pk = _pack(mask, B, H, T, False, q.dtype, q.device)
        drop = (0.0, None, 0)
        if dropout_p > 0.0:
            from . import lora_ops

            drop = (float(dropout_p), lora_ops.dropout_seed_snapshot(q.device), int(salt))
        out, lse = _rel_launch_forward(q, k, v, pk, scale, rel, cols, drop)
        ctx.save_for_backward(q, k, v, out, lse, rel, *([cols] if cols is not None else []))
        ctx.pack, ctx.scale, ctx.drop = pk, scale, drop
        return out

    @staticmethod
    def backward(ctx, d_out):
        q, k, v, out, lse, rel, *cols = ctx.saved_tensors
        dq, dk, dv = _rel_launch_backward(q, k, v, out, lse, d_out, ctx.pack, ctx.scale, rel, cols[0] if cols else None, ctx.drop)
        return dq, dk, dv, None, None, None, None, None, None


def rel_supported(query, key, value, rel, mask, dropout: float) -> bool:
    """What `dalm_attn_rel_*` take: bf16 GPU [B, H, T, 64] views with 16-byte rows, equal heads, 1 <= T <= 2048, an f32 vector
    with Tc >= T, no mask / a boolean [B, 1, T, T] mask / a packed descriptor, dropout only with an even T."""
    if _off("DALM_ATTN_KERNEL"):
        return False
    if not (query.is_cuda and query.dtype == torch.bfloat16 and key.dtype == query.dtype and value.dtype == query.dtype):
        return False
    if query.dim() != 4 or query.shape[-1] != 64 or key.shape != query.shape or value.shape != query.shape:
        return False
    seqs = packed_of(mask)
    B, _, T, _ = query.shape
    Tm = T if seqs is None else seqs.T
    if not (rel.is_cuda and rel.dtype == torch.float32 and rel.dim() == 2 and rel.shape[0] == query.shape[1] and rel.stride(1) == 1
            and Tm <= (rel.shape[1] + 1) // 2 <= 2048 and Tm >= 1):
        return False
    if dropout != 0.0 and not (0.0 < dropout < 1.0 and Tm % 2 == 0):
        return False
    if seqs is None and mask is not None and not (mask.dtype == torch.bool and tuple(mask.shape) == (B, 1, T, T) and mask.is_cuda):
        return False
    if seqs is not None and query.shape[0] != 1:
        return False
    return _views_ok(query, key, value)


def _rel_sdpa_torch(query, key, value, rel, mask, seqs, scale: float, dropout: float):
    """The same attention without the kernels (CPU tensors, fp32, what `rel_supported` declines): torch's SDPA with the bias
    expanded into a float mask - per sequence for a packed call, at the tokens' original column differences."""
    H = query.shape[1]
    neg = torch.finfo(torch.float32).min
    if seqs is None:
        B, _, T, _ = query.shape
        bias = expand_rel_bias(rel, torch.arange(T, device=query.device))[None]                    # [1, H, T, T]
        if mask is not None:
            bias = bias + (torch.zeros_like(mask, dtype=torch.float32).masked_fill(~mask, neg) if mask.dtype == torch.bool else mask)
        return torch.nn.functional.scaled_dot_product_attention(query, key, value, attn_mask=bias.to(query.dtype), dropout_p=dropout,
                                                                scale=scale)
    _, _, n, hd = query.shape
    slot, gather = seqs.padded_index()
    nseq, T = seqs.nseq, seqs.T

    def pad(t):                                                   # [1, H, n, hd] -> [nseq, H, T, hd]
        rows = torch.cat((t[0].transpose(0, 1), t.new_zeros((1, H, hd))), dim=0)
        return rows.index_select(0, gather).view(nseq, T, H, hd).transpose(1, 2)

    cols = seqs.cols.to(torch.int64) if seqs.cols is not None else (torch.arange(n, device=query.device) - seqs.cu.to(torch.int64)[
        torch.bucketize(torch.arange(n, device=query.device), seqs.cu[1:].to(torch.int64), right=True).clamp_max(nseq - 1)])
    cpad = torch.cat((cols, cols.new_zeros((1,)))).index_select(0, gather).view(nseq, T)
    kl = torch.cat((seqs.key_live != 0, seqs.key_live.new_zeros((1,), dtype=torch.bool))).index_select(0, gather).view(nseq, 1, 1, T)
    live = kl.expand(nseq, 1, T, T)
    has_key = live.any(dim=-1, keepdim=True)
    live = live | (~has_key & torch.eye(T, dtype=torch.bool, device=query.device))
    bias = expand_rel_bias(rel, cpad).masked_fill(~live, neg)                                      # [nseq, H, T, T]
    out = torch.nn.functional.scaled_dot_product_attention(pad(query), pad(key), pad(value), attn_mask=bias.to(query.dtype),
                                                           dropout_p=dropout, scale=scale)
    out = torch.where(has_key, out, torch.zeros_like(out))
    return out.transpose(1, 2).reshape(nseq * T, H, hd).index_select(0, slot).unsqueeze(0).transpose(1, 2)   # [1, H, n, hd]


def rel_sdpa(module, query, key, value, source: RelBiasSource, mask, dropout: float = 0.0):
    """softmax(q k^T / sqrt(hd) + bias + mask) v for [B, H, T, hd] q / k / v with MPNet's relative-position bias: on the kernels
    where `rel_supported` holds, through torch's SDPA with a float mask elsewhere.  `mask`: None, transformers' additive float
    mask or a boolean mask [B, 1, T, T], or a packed descriptor.  Returns [B, H, T, hd]."""
    seqs = packed_of(mask)
    Tc = query.shape[2] if seqs is None else seqs.T
    rel = source.vector(Tc, query.device)
    scale = float(query.shape[-1]) ** -0.5
    if seqs is None and mask is not None:
        mask = _bool_key_mask(mask)
    if rel_supported(query, key, value, rel, mask, dropout):
        salt = dropout_salt(module, "_dalm_attn_calls") if dropout > 0.0 else 0
        cols = None if seqs is None else seqs.cols
        return _RelSdpaHip.apply(query, key, value, rel, mask, scale, float(dropout), salt, cols)
    return _rel_sdpa_torch(query, key, value, rel, mask, seqs, scale, float(dropout))


_registered = [False]


def register() -> bool:
    """Register "dalm_sdpa" with transformers (attention function + the SDPA mask builder).  False when this transformers has
    no such registry or its `sdpa_attention_forward` is not the code the replacement restates."""
    if _registered[0]:
        return True
    try:
        import inspect

        from transformers import AttentionInterface
        from transformers.integrations import sdpa_attention
        from transformers.masking_utils import AttentionMaskInterface, sdpa_mask

        src = inspect.getsource(sdpa_attention.sdpa_attention_forward)
        if not ("torch.nn.functional.scaled_dot_product_attention(" in src and "attn_output.transpose(1, 2).contiguous()" in src
                and "is_causal = q_length > 1 and attention_mask is None and is_causal" in src
                and "return attn_output, None" in src):
            return False
        AttentionInterface.register(NAME, dalm_sdpa_attention_forward)
        AttentionMaskInterface.register(NAME, sdpa_mask)
    except Exception:
        return False
    _registered[0] = True
    return True


def sdpa(query, key, value, mask, scale: float, causal: bool, dropout_p: float = 0.0, salt: int = 0):
    """F.scaled_dot_product_attention(query, key, value, attn_mask=mask, is_causal=causal, scale=scale, dropout_p=dropout_p) for
    what `supported` accepts (the dropout mask comes from this library's own generator, oracle/attn_dropout.py)."""
    return _SdpaHipBackward.apply(query, key, value, mask, scale, causal, dropout_p, salt)


def use_hip_attention_backward(model: torch.nn.Module) -> bool:
    """Switch a Llama-family, Gemma, Arcee, OLMo-2, Granite, Cohere, Phi-3, BERT or RoBERTa-family (roberta, xlm-roberta, camembert: BERT's
    layer code) model of head width 32, 64 or 128 from "sdpa" to "dalm_sdpa".  xlm-roberta-xl (pre-LayerNorm layers) is not taken, and
    neither is a Gemma of head width 256 (every released checkpoint) or an Arcee of head width 80 (`ArceeConfig()`'s defaults;
    AFM-4.5B has 128): it keeps transformers' SDPA and does not pack.  Granite's softmax scale (`attention_multiplier`, not
    hd ** -0.5) reaches the kernels as the `scaling` argument of the attention call, like any other.  Phi-3 / Phi-4 (`model_type`
    phi3) under the same head-width rule: Phi-3-mini and Phi-3.5-mini (width 96) keep "sdpa" and do not pack, Phi-3-medium, Phi-4
    and Phi-4-mini (128) are switched; a phi3 config whose `sliding_window` is shorter than its positions is not switched (the
    packed attention knows no window).  DALM_ATTN_KERNEL=0 disables."""
    if _off("DALM_ATTN_KERNEL"):
        return False
    cfg = getattr(model, "config", None)
    if cfg is None or getattr(cfg, "_attn_implementation", None) != "sdpa":
        return False
    if getattr(cfg, "model_type", "") not in ("llama", "mistral", "qwen2", "qwen3", "gemma", "arcee", "olmo2", "granite", "cohere",
                                              "phi3", "bert", "roberta", "xlm-roberta", "camembert"):
        return False
    if cfg.model_type == "phi3":
        window = getattr(cfg, "sliding_window", None)
        if window is not None and window < getattr(cfg, "max_position_embeddings", 1 << 30):
            return False
    hd = getattr(cfg, "head_dim", None) or (cfg.hidden_size // cfg.num_attention_heads)
    if hd not in _HEAD_DIMS or not register():
        return False
    cfg._attn_implementation = NAME
    return True
