"""`dropout + residual add + LayerNorm` of a BERT encoder layer as one HIP launch per direction (`dalm_bert_add_norm_{fwd,bwd}`,
dalm_amd/csrc/bert.hip), for the configuration the trainers and bench.py run the retriever in: bf16 autocast over a frozen
(LoRA) base.

transformers' BertSelfOutput / BertOutput compute `LayerNorm(dropout(dense(h)) + input_tensor)`; the reference reaches them
through `self.retriever_model(...)` (dalm/models/rag_e2e_base_model.py:84-93).  Under autocast the dense output is bf16, the
residual stream and the LayerNorm are f32 (autocast runs layer_norm in f32), and every consumer GEMM casts the f32 result back to
bf16.  The kernel rounds at those points and hands back BOTH forms: `y32` (the module's output, exactly the eager dtype) and
`y16 = bf16(y32)`, attached to `y32` as `_dalm_bf16` - the consumers in this package (`frozen_linear.FrozenLinearT`, the LoRA
group node) take the twin instead of casting again (`twin`), which keeps autograd exact: the twin is a second output of the same
node, its gradient is added to y32's in the backward kernel.

Dropout (BERT's hidden_dropout_prob, training mode) comes from this library's generator (seed word + salt + element index, mask
kept as bits; oracle/lora_mask.py::keep_mask_v2) - torch's philox stream has no reference to match.  Needs its own RNG state to be
re-run: not supported under activation recompute.

The RoBERTa family (roberta, xlm-roberta, camembert) runs the same layer code, so the node above serves it unchanged; its
embeddings front end - positions counted from the ids, three table gathers, two adds, an f32 LayerNorm, a dropout: ~20 eager
launches per tower call - is `dalm_embed_norm_fwd` (`embed_norm`, forward only: used while the tables and the LayerNorm are
frozen f32 tensors under bf16 autocast, so nothing needs a backward).  BertEmbeddings keeps transformers' code.
"""
from __future__ import annotations

import torch

from .. import hip, live_rows


def twin(x: torch.Tensor) -> torch.Tensor:
    """The bf16 copy a `_BertAddNorm` output carries, when the caller is about to cast x to bf16 anyway (bf16 autocast)."""
    t = getattr(x, "_dalm_bf16", None)
    if t is not None and x.is_cuda and torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == t.dtype \
            and t.shape == x.shape and x._version == getattr(x, "_dalm_bf16_version", -1) and t._version == getattr(x, "_dalm_bf16_tversion", -1):
        return t                  # (an in-place write to either tensor since they were made: the twin is stale, cast instead)
    return x


class _BertAddNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, res, w, b, eps, p, salt, live=None):
        D = a.shape[-1]
        a2, r2 = a.reshape(-1, D), res.reshape(-1, D)
        a2 = a2 if a2.is_contiguous() else a2.contiguous()
        r2 = r2 if r2.is_contiguous() else r2.contiguous()
        R = a2.shape[0]
        dev = a.device
        if live is None:
            live = live_rows.current(R, dev)      # the padded tower call in progress: dead rows are not read, they leave as zeros
        y32 = torch.empty((R, D), dtype=torch.float32, device=dev)
        y16 = torch.empty((R, D), dtype=torch.bfloat16, device=dev)
        mean = torch.empty(R, dtype=torch.float32, device=dev)
        rstd = torch.empty(R, dtype=torch.float32, device=dev)
        bits, seed = None, None
        if p > 0.0:
            from . import lora_ops

            bits = torch.empty((R, D // 8), dtype=torch.uint8, device=dev)
            seed = lora_ops.dropout_seed(dev)         # read in this launch only: the backward reads the stored bits
        hip.call("dalm_bert_add_norm_fwd_live", hip.ptr(a2), hip.ptr(r2), hip.ptr(w), hip.ptr(b), int(w.dtype == torch.bfloat16), R, D,
                 float(eps), float(p), hip.ptr(seed), int(salt) & 0xFFFFFFFF, hip.ptr(y32), hip.ptr(y16), hip.ptr(bits), hip.ptr(mean),
                 hip.ptr(rstd), hip.ptr(live), hip.stream())
        # (the liveness vector is kept: the backward runs after the tower call's context)
        ctx.save_for_backward(a2, r2, w, mean, rstd, *([bits] if bits is not None else []), *([live] if live is not None else []))
        ctx.p, ctx.shape, ctx.has_bits = float(p), a.shape, bits is not None
        ctx.set_materialize_grads(False)
        return y32.view(a.shape), y16.view(a.shape)

    @staticmethod
    def backward(ctx, g32, g16):
        sv = ctx.saved_tensors
        a2, r2, w, mean, rstd = sv[:5]
        rest = list(sv[5:])
        bits = rest.pop(0) if ctx.has_bits else None
        live = rest.pop(0) if rest else None
        R, D = a2.shape
        if g32 is None and g16 is None:
            return None, None, None, None, None, None, None, None
        if g32 is not None:
            g32 = g32.reshape(R, D)
            g32 = g32 if (g32.dtype == torch.float32 and g32.is_contiguous()) else g32.float().contiguous()
        if g16 is not None:
            g16 = g16.reshape(R, D)
            g16 = g16 if (g16.dtype == torch.bfloat16 and g16.is_contiguous()) else g16.to(torch.bfloat16).contiguous()
        d_res = torch.empty((R, D), dtype=torch.float32, device=a2.device)
        d_a = torch.empty((R, D), dtype=torch.bfloat16, device=a2.device)
        hip.call("dalm_bert_add_norm_bwd_live", hip.ptr(g32), hip.ptr(g16), hip.ptr(a2), hip.ptr(r2), hip.ptr(w),
                 int(w.dtype == torch.bfloat16), hip.ptr(bits), hip.ptr(mean), hip.ptr(rstd), R, D, ctx.p, hip.ptr(d_res), hip.ptr(d_a),
                 hip.ptr(live), hip.stream())
        return d_a.view(ctx.shape), d_res.view(ctx.shape), None, None, None, None, None, None


def supported(a: torch.Tensor, res: torch.Tensor, ln: torch.nn.Module) -> bool:
    """bf16 dense output + f32 residual (what bf16 autocast produces), a frozen affine LayerNorm over the last dimension."""
    w, b = getattr(ln, "weight", None), getattr(ln, "bias", None)
    if not isinstance(ln, torch.nn.LayerNorm) or w is None or b is None or w.requires_grad or b.requires_grad:
        return False
    D = a.shape[-1]
    return (a.is_cuda and a.dtype == torch.bfloat16 and res.dtype == torch.float32 and res.shape == a.shape and res.device == a.device
            and tuple(ln.normalized_shape) == (D,) and D % 8 == 0 and D <= 2048 and w.dtype == b.dtype
            and w.dtype in (torch.float32, torch.bfloat16) and w.is_contiguous() and b.is_contiguous()
            and torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16)


def add_norm(a, res, ln: torch.nn.LayerNorm, p: float, salt: int, live=None) -> torch.Tensor:
    """LayerNorm(dropout_p(a) + res) -> the f32 result carrying its bf16 twin.  live: uint8 row liveness; None: that of the tower
    call in progress (dalm_amd/live_rows.py), if any."""
    y32, y16 = _BertAddNorm.apply(a, res, ln.weight, ln.bias, float(ln.eps), float(p), int(salt), live)
    y32._dalm_bf16 = y16
    y32._dalm_bf16_version, y32._dalm_bf16_tversion = y32._version, y16._version
    return y32


# ---- RoBERTa-family embeddings front end: `dalm_embed_norm_fwd` (forward only) -------------------------------------------------
def embed_supported(emb: torch.nn.Module, input_ids, token_type_ids, position_ids, inputs_embeds, past_key_values_length) -> bool:
    """A {Roberta,XLMRoberta,Camembert}Embeddings call the kernel stands for: ids [B, T] on a GPU under bf16 autocast, three frozen
    f32 tables and a frozen affine LayerNorm (the LoRA configuration: the output carries no gradient, nothing is saved), no
    `inputs_embeds`, no cache offset, and - where the positions are derived from the ids - room for them in the position table
    (T + padding_idx + 1 <= max_position_embeddings: a longer row makes eager raise, and eager is what then runs)."""
    if inputs_embeds is not None or input_ids is None or not isinstance(past_key_values_length, int) or past_key_values_length != 0:
        return False
    if not (input_ids.is_cuda and input_ids.dim() == 2 and input_ids.dtype == torch.int64):
        return False
    ln, pad = emb.LayerNorm, emb.padding_idx
    tables = (emb.word_embeddings, emb.token_type_embeddings, emb.position_embeddings)
    w, b = getattr(ln, "weight", None), getattr(ln, "bias", None)
    if w is None or b is None or w.requires_grad or b.requires_grad or not isinstance(pad, int) or pad < 0:
        return False
    D = tables[0].weight.shape[1]
    for t in tables:
        tw = t.weight
        if (tw.requires_grad or tw.dtype != torch.float32 or not tw.is_contiguous() or tw.device != input_ids.device
                or tw.shape[1] != D or t.max_norm is not None):
            return False
    for ids in (token_type_ids, position_ids):
        if ids is not None and not (ids.dtype == torch.int64 and ids.device == input_ids.device and ids.dim() == 2
                                    and ids.shape[1] == input_ids.shape[1] and ids.shape[0] in (1, input_ids.shape[0])):
            return False
    if position_ids is None and input_ids.shape[1] + pad + 1 > tables[2].weight.shape[0]:
        return False
    return (tuple(ln.normalized_shape) == (D,) and D % 8 == 0 and D <= 2048 and w.dtype == b.dtype
            and w.dtype in (torch.float32, torch.bfloat16) and w.is_contiguous() and b.is_contiguous() and w.device == input_ids.device
            and torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16)


def _ids(t, like):
    if t is None:
        return None
    t = t.expand_as(like) if t.shape != like.shape else t
    return t if t.is_contiguous() else t.contiguous()


def embed_norm(emb: torch.nn.Module, input_ids, token_type_ids, position_ids, p: float, salt: int, live=None) -> torch.Tensor:
    """dropout_p(LayerNorm((word[ids] + type[token_type_ids]) + pos[positions])) of a RoBERTa-family embeddings module for what
    `embed_supported` accepts -> the f32 result [B, T, D] carrying its bf16 twin (as `add_norm`'s), no autograd node.
    position_ids None: derived from the ids in the kernel.  live: uint8 row liveness; None: that of the tower call in progress."""
    B, T = input_ids.shape
    dev = input_ids.device
    word, typ, pos = emb.word_embeddings.weight, emb.token_type_embeddings.weight, emb.position_embeddings.weight
    ln = emb.LayerNorm
    D = word.shape[1]
    ids = input_ids if input_ids.is_contiguous() else input_ids.contiguous()
    tt, ps = _ids(token_type_ids, ids), _ids(position_ids, ids)
    if live is None:
        live = live_rows.current(B * T, dev)
    y32 = torch.empty((B, T, D), dtype=torch.float32, device=dev)
    y16 = torch.empty((B, T, D), dtype=torch.bfloat16, device=dev)
    seed = None
    if p > 0.0:
        from . import lora_ops

        seed = lora_ops.dropout_seed(dev)
    hip.call("dalm_embed_norm_fwd", hip.ptr(ids), hip.ptr(tt), hip.ptr(ps), hip.ptr(word), hip.ptr(typ), hip.ptr(pos), word.shape[0],
             typ.shape[0], pos.shape[0], int(emb.padding_idx), hip.ptr(ln.weight), hip.ptr(ln.bias), int(ln.weight.dtype == torch.bfloat16),
             B, T, D, float(ln.eps), float(p), hip.ptr(seed), int(salt) & 0xFFFFFFFF, hip.ptr(y32), hip.ptr(y16), hip.ptr(live),
             hip.stream())
    y32._dalm_bf16 = y16
    y32._dalm_bf16_version, y32._dalm_bf16_tversion = y32._version, y16._version
    return y32
