"""The attention kernels at head width 32 (dalm_amd/csrc/attn.hip: attn_fwd_kernel<32>, attn_bwd_dq_kernel<32>,
attn_bwd_dkdv32_kernel - the bge-small / e5-small / gte-small / all-MiniLM class of retrievers, hidden 384 = 12 heads of 32) with
the constructions and bounds the other widths are tested with (tests/test_attention_gpu.py, tests/test_packed_gpu.py):

* padded: out, dq, dk, dv against a float64 evaluation, no further from it than torch's bf16 SDPA on the same inputs is
  (x 1.5 + 1e-3), exact zeros in padding rows, [B, T, H, hd] output memory - at the smallest shapes that reach each edge of the
  kernels (T below one tile, a partial tile, exactly one 128-row block with a single live key, two blocks with a partial last one,
  three 128-row blocks under the causal mask), an arbitrary boolean mask;
* dropout: every keep bit of the forward against oracle/attn_dropout.py, gradients against float64 with the oracle's mask;
* packed: against float64 and `_packed_sdpa_torch`, slack and key-dead rows exactly zero, an empty sequence, dropout;
* a BERT and a Llama of that width on "dalm_sdpa" against the same weights on "sdpa";
* a RetrieverStep of bge-small width: padded on torch's attention, padded on the kernels and packed, each against fp32 on the host.
"""
import copy
import os
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu
HD = 32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _hf_mask(B, T, starts, dev):
    col = torch.arange(T, device=dev)
    st = torch.tensor(starts, device=dev)
    return ((col[None, None, :] <= col[None, :, None]) & (col[None, None, :] >= st[:, None, None]))[:, None]


def _ref64(q, k, v, mask, causal, scale, go):
    q, k, v = [t.detach().double().requires_grad_(True) for t in (q, k, v)]
    s = (q @ k.transpose(-1, -2)) * scale
    T = s.shape[-1]
    live = torch.ones(T, T, dtype=torch.bool, device=s.device).tril() if causal else torch.ones(T, T, dtype=torch.bool, device=s.device)
    live = live[None, None] if mask is None else (mask & live)
    s = s.masked_fill(~live, float("-inf"))
    p = torch.nan_to_num(torch.softmax(s, -1), nan=0.0)     # rows without a live key: zero output, zero gradient
    o = p @ v
    o.backward(go.double())
    return o, q.grad, k.grad, v.grad


def _run(fn, q, k, v, go):
    q, k, v = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
    o = fn(q, k, v)
    o.backward(go)
    return o.detach(), q.grad, k.grad, v.grad


CASES = [
    # B, H, T, starts (left padding per batch row; None = no mask, is_causal), layout        reaches
    (2, 3, 50, [3, 0], "bthd"),                # a partial tile, T not a multiple of 32 (the query shape)
    (3, 2, 128, [0, 127, 64], "bhtd"),         # exactly one 128-row block (the passage shape); a row with ONE live key
    (2, 2, 200, [5, 150], "bthd"),             # two 128-row blocks, the last one partial
    (2, 3, 320, None, "bhtd"),                 # causal, no mask: three 128-row blocks = five 64-row blocks streamed
    (1, 2, 8, None, "bthd"),                   # T below one tile
]


@pytest.mark.parametrize("B,H,T,starts,layout", CASES)
def test_backward_vs_fp64_and_torch(dev, B, H, T, starts, layout):
    from dalm_amd.models import attention

    g = torch.Generator().manual_seed(B * 1000 + T)

    def mk():
        if layout == "bthd":
            return (torch.randn(B, T, H, HD, generator=g) * 1.2).bfloat16().to(dev).transpose(1, 2)
        return (torch.randn(B, H, T, HD, generator=g) * 1.2).bfloat16().to(dev)

    q, k, v, go = mk(), mk(), mk(), mk()
    mask = None if starts is None else _hf_mask(B, T, starts, dev)
    causal = starts is None
    scale = HD ** -0.5
    assert attention.supported(q.requires_grad_(True), k, v, mask, 0.0, causal, {})

    ours = _run(lambda a, b, c: attention._SdpaHipBackward.apply(a, b, c, mask, scale, causal), q, k, v, go)
    theirs = _run(lambda a, b, c: torch.nn.functional.scaled_dot_product_attention(a, b, c, attn_mask=mask, is_causal=causal,
                                                                                    scale=scale), q, k, v, go)
    ref = _ref64(q, k, v, mask, causal, scale, go)
    assert ours[0].transpose(1, 2).is_contiguous()           # [B, T, H, hd] memory: the caller's transpose(1, 2).contiguous() is free
    for name, a, b, r in zip(("out", "dq", "dk", "dv"), ours, theirs, ref):
        assert torch.isfinite(a).all(), name
        e_a, e_b = _rel(a, r), _rel(b, r)
        print(f"hd32 padded B{B} H{H} T{T} {name}: ours {e_a:.3e} torch {e_b:.3e}")
        assert e_a <= 1.5 * e_b + 1e-3, (name, e_a, e_b)
    if starts is not None:                                   # rows in the padding have no live key and are nobody's key: exactly zero
        for b_, st in enumerate(starts):
            if st > 0:
                for t in ours:
                    assert float(t[b_, :, :st].abs().max()) == 0.0


def test_arbitrary_boolean_mask(dev):
    from dalm_amd.models import attention

    B, H, T = 2, 2, 96
    g = torch.Generator().manual_seed(7)
    q, k, v, go = [(torch.randn(B, T, H, HD, generator=g)).bfloat16().to(dev).transpose(1, 2) for _ in range(4)]
    mask = (torch.rand(B, 1, T, T, generator=g) < 0.3).to(dev)
    mask[:, :, :, 0] = True                                  # every row keeps a key
    mask[0, 0, 64:96, :] = False
    mask[0, 0, 64:96, 5] = True                              # a block of rows with one live key, 32 x 32 tiles entirely dead
    scale = 0.11
    ours = _run(lambda a, b, c: attention._SdpaHipBackward.apply(a, b, c, mask, scale, False), q, k, v, go)
    theirs = _run(lambda a, b, c: torch.nn.functional.scaled_dot_product_attention(a, b, c, attn_mask=mask, scale=scale), q, k, v, go)
    ref = _ref64(q, k, v, mask, False, scale, go)
    for a, b, r in zip(ours, theirs, ref):
        assert _rel(a, r) <= 1.5 * _rel(b, r) + 1e-3


def _oracle():
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "oracle"))
    import attn_dropout as AD

    return AD


def test_every_keep_bit_of_the_forward_equals_the_oracle(dev):
    """V = one-hot columns: out[b, h, i, d] = sum_j P_drop[i, j] [j == d] exposes every element of P o M / (1 - p) for T <= hd."""
    from dalm_amd.models import attention, lora_ops

    AD = _oracle()
    B, H, T, p, salt = 2, 3, 32, 0.25, 99
    q = torch.zeros(B, H, T, HD, dtype=torch.bfloat16, device=dev).requires_grad_(True)       # uniform probabilities 1 / T
    k = torch.zeros_like(q)
    v = torch.eye(T, HD, dtype=torch.bfloat16, device=dev).expand(B, H, T, HD).contiguous()
    out = attention.sdpa(q, k, v, None, 1.0, False, p, salt)
    got = out.detach().float() > 0
    want = torch.from_numpy(AD.keep_mask(int(lora_ops.dropout_seed(dev).item()), salt, B, H, T, p)).to(dev)
    assert torch.equal(got, want)
    assert torch.allclose(out.detach().float()[got], torch.tensor(1.0 / T / (1 - p), device=dev), rtol=1e-2)


@pytest.mark.parametrize("B,H,T,pad", [(3, 4, 128, [128, 90, 17]), (2, 3, 50, [50, 31])])
def test_attention_dropout_mask_and_gradients(dev, B, H, T, pad):
    """BERT's attention dropout inside the kernels (bidirectional padding mask, p = 0.1): out, dq, dk, dv against a float64
    evaluation of softmax -> (P o M) / (1 - p) -> P V with the ORACLE's mask; forward and backward therefore use those bits."""
    from dalm_amd.models import attention, lora_ops

    AD = _oracle()
    p, salt = 0.1, 0x5A17
    g = torch.Generator().manual_seed(T + HD)
    q, k, v, go = [(torch.randn(B, T, H, HD, generator=g)).bfloat16().to(dev).transpose(1, 2) for _ in range(4)]
    col = torch.arange(T, device=dev)
    lens = torch.tensor(pad, device=dev)
    mask = (col[None, None, None, :] < lens[:, None, None, None]).expand(B, 1, T, T)          # HF's bidirectional padding mask
    scale = HD ** -0.5
    assert attention.supported(q.requires_grad_(True), k, v, mask, p, False, {})
    seed = int(lora_ops.dropout_seed(dev).item())
    keep = torch.from_numpy(AD.keep_mask(seed, salt, B, H, T, p)).to(dev)
    assert abs(float((~keep).float().mean()) - p) < 0.01

    ours = _run(lambda a, b, c: attention.sdpa(a, b, c, mask, scale, False, p, salt), q, k, v, go)
    q64, k64, v64 = [t.detach().double().requires_grad_(True) for t in (q, k, v)]
    s = (q64 @ k64.transpose(-1, -2)) * scale
    s = s.masked_fill(~mask, float("-inf"))
    pr = torch.softmax(s, -1) * keep.double() / (1.0 - p)
    o64 = pr @ v64
    o64.backward(go.double())
    for name, a, r in zip(("out", "dq", "dk", "dv"), ours, (o64, q64.grad, k64.grad, v64.grad)):
        assert torch.isfinite(a).all(), name
        print(f"hd32 dropout T{T} {name}: {_rel(a, r):.3e}")
        assert _rel(a, r) < 1.2e-2, (name, _rel(a, r))
    # a different salt draws a different mask; p = 0 is the plain attention
    other = _run(lambda a, b, c: attention.sdpa(a, b, c, mask, scale, False, p, salt + 1), q, k, v, go)
    assert not torch.equal(other[0], ours[0])
    plain = _run(lambda a, b, c: attention.sdpa(a, b, c, mask, scale, False, 0.0, 0), q, k, v, go)
    plain2 = _run(lambda a, b, c: attention._SdpaHipBackward.apply(a, b, c, mask, scale, False), q, k, v, go)
    for a, b in zip(plain, plain2):
        assert torch.equal(a, b)
    theirs = _run(lambda a, b, c: torch.nn.functional.scaled_dot_product_attention(a, b, c, attn_mask=mask, scale=scale), q, k, v, go)
    for a, b in zip(plain, theirs):
        assert _rel(a, b) < 1.2e-2


# ---- packed ----------------------------------------------------------------------------------------------------------------
def _seq_ref64(q, k, v, key_live, causal, scale, go):
    """float64 attention of ONE sequence [H, n, hd] with key-live flags [n]; rows without a live key: 0."""
    q, k, v = [t.detach().double().requires_grad_(True) for t in (q, k, v)]
    s = (q @ k.transpose(-1, -2)) * scale
    n = s.shape[-1]
    live = key_live.bool()[None, :].expand(n, n)
    if causal:
        live = live & torch.ones(n, n, dtype=torch.bool, device=s.device).tril()
    s = s.masked_fill(~live[None], float("-inf"))
    p = torch.nan_to_num(torch.softmax(s, -1), nan=0.0)
    o = p @ v
    o.backward(go.double())
    return o, q.grad, k.grad, v.grad


def _mask_2d(B, T, lens, left):
    ar = torch.arange(T).unsqueeze(0)
    L = torch.tensor(lens).unsqueeze(1)
    return ((ar >= T - L) if left else (ar < L)).long()


PACKED_CASES = [
    # B, H, T, lens, left padding, causal
    (4, 4, 128, [128, 30, 77, 5], False, False),        # BERT passages
    (5, 2, 50, [5, 15, 9, 50, 1], False, False),        # BERT queries
    (3, 2, 256, [200, 0, 129], False, True),            # causal; an all-padding row: an empty sequence
]


@pytest.mark.parametrize("B,H,T,lens,left,causal", PACKED_CASES)
def test_packed_attention_kernels_vs_float64_and_padded(dev, B, H, T, lens, left, causal):
    from dalm_amd import packed
    from dalm_amd.models import attention

    g = torch.Generator().manual_seed(B * 1000 + T + HD)
    m2 = _mask_2d(B, T, lens, left)
    rows, cu = packed.pack_plan(m2, shifted=causal, multiple=64)
    rows_d, cu_d = rows.to(dev), cu.to(dev)
    n = rows.numel()
    ids = torch.zeros(B, T, dtype=torch.long, device=dev)
    _ids_p, _pos, desc, _valid = packed.packed_inputs(ids, m2.to(dev), rows_d, cu_d, causal)
    seqs = packed.packed_of(desc)
    q, k, v, go = [(0.7 * torch.randn(1, n, H, HD, generator=g)).to(dev, torch.bfloat16).transpose(1, 2) for _ in range(4)]
    scale = HD ** -0.5

    def run(fn):
        qq, kk, vv = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
        o = fn(qq, kk, vv)
        o.backward(go if o.shape == go.shape else go.transpose(1, 2))
        return o.detach(), qq.grad, kk.grad, vv.grad

    assert attention.packed_supported(q, k, v)
    got = run(lambda a, b, c: attention.sdpa(a, b, c, desc, scale, False))
    alt = run(lambda a, b, c: attention._packed_sdpa_torch(a, b, c, seqs, scale, 0.0).transpose(1, 2))   # torch's bf16 kernels, re-padded

    want_o = torch.zeros(1, H, n, HD, dtype=torch.float64, device=dev)
    want = [torch.zeros_like(want_o) for _ in range(3)]
    for b in range(cu.numel() - 1):
        a, e = int(cu[b]), int(cu[b + 1])
        if e == a:
            continue
        o, dq_, dk_, dv_ = _seq_ref64(q[0, :, a:e], k[0, :, a:e], v[0, :, a:e], seqs.key_live[a:e], causal, scale, go[0, :, a:e])
        want_o[0, :, a:e] = o
        for t, gsrc in zip(want, (dq_, dk_, dv_)):
            t[0, :, a:e] = gsrc
    for name, gt, al, wt in zip(("out", "dq", "dk", "dv"), got, alt, [want_o] + want):
        e_k, e_t = _rel(gt, wt), _rel(al, wt)
        print(f"hd32 packed T{T} {name}: ours {e_k:.3e} torch {e_t:.3e}")
        assert e_k <= 1.5 * e_t + 2e-3, (name, e_k, e_t)
        assert torch.isfinite(gt).all(), name
    # slack rows and key-dead rows: exactly zero output / gradients
    dead_q = torch.zeros(n, dtype=torch.bool, device=dev)
    for b in range(cu.numel() - 1):
        a, e = int(cu[b]), int(cu[b + 1])
        kl = seqs.key_live[a:e].bool()
        for i in range(e - a):
            has = bool(kl[:i + 1].any()) if causal else bool(kl.any())
            dead_q[a + i] = not has
    assert (got[0][0, :, dead_q] == 0).all() and (got[1][0, :, dead_q] == 0).all()
    dead_k = seqs.key_live == 0
    assert (got[2][0, :, dead_k] == 0).all() and (got[3][0, :, dead_k] == 0).all()


def test_packed_attention_dropout_statistics_and_backward(dev):
    """BERT's attention dropout inside the packed kernels: deterministic for one seed word, different after an advance, E[out]
    close to the no-dropout output, finite gradients."""
    from dalm_amd import packed
    from dalm_amd.models import attention, lora_ops

    B, H, T, p = 6, 4, 128, 0.1
    m2 = _mask_2d(B, T, [128, 64, 100, 33, 128, 90], False)
    rows, cu = packed.pack_plan(m2, shifted=False, multiple=64)
    _i, _p, desc, _v = packed.packed_inputs(torch.zeros(B, T, dtype=torch.long, device=dev), m2.to(dev), rows.to(dev), cu.to(dev), False)
    n = rows.numel()
    g = torch.Generator().manual_seed(5)
    q, k, v = [(0.5 * torch.randn(1, n, H, HD, generator=g)).to(dev, torch.bfloat16).transpose(1, 2).requires_grad_(True) for _ in range(3)]
    base = attention.sdpa(q, k, v, desc, HD ** -0.5, False).float()
    lora_ops.advance_dropout_seed(dev)
    a = attention.sdpa(q, k, v, desc, HD ** -0.5, False, p, 7).float()
    b = attention.sdpa(q, k, v, desc, HD ** -0.5, False, p, 7).float()
    assert torch.equal(a, b)
    lora_ops.advance_dropout_seed(dev)
    c = attention.sdpa(q, k, v, desc, HD ** -0.5, False, p, 7).float()
    assert not torch.equal(a, c)
    acc = torch.zeros_like(base)
    reps = 24
    for i in range(reps):
        lora_ops.advance_dropout_seed(dev)
        acc += attention.sdpa(q, k, v, desc, HD ** -0.5, False, p, 7).float()
    assert _rel(acc / reps, base) < 0.12                       # ~ sqrt(p / (1 - p) / reps / keys) scale, loose
    out = attention.sdpa(q, k, v, desc, HD ** -0.5, False, p, 7)
    out.float().square().sum().backward()
    assert all(torch.isfinite(t.grad).all() for t in (q, k, v))


# ---- model level -----------------------------------------------------------------------------------------------------------
def test_bert_of_width_32_on_dalm_sdpa_trains_with_dropout(dev):
    """A BERT encoder of hidden 128 = 4 heads of 32 on "dalm_sdpa" in training mode against the same weights on "sdpa" with dropout
    off; with attention dropout 0.1: finite, deterministic for a fixed seed word and call count, different from the plain output."""
    from transformers import BertConfig, BertModel

    from dalm_amd.models import attention

    torch.manual_seed(0)
    cfg = BertConfig(hidden_size=128, num_hidden_layers=2, num_attention_heads=4, intermediate_size=256, vocab_size=300,
                     hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    ref = BertModel(cfg).to(dev).train()                            # f32 parameters under bf16 autocast, as the trainers run it
    new = copy.deepcopy(ref)
    assert attention.use_hip_attention_backward(new) and new.config._attn_implementation == "dalm_sdpa"
    assert ref.config._attn_implementation == "sdpa"
    seen = []
    orig = attention._attn_forward

    def spy(q, *a, **kw):
        seen.append(tuple(q.shape))
        return orig(q, *a, **kw)

    B, T = 4, 64
    ids = torch.randint(0, 300, (B, T), device=dev)
    am = torch.ones(B, T, dtype=torch.long, device=dev)
    am[1, 40:] = 0
    outs = []
    attention._attn_forward = spy
    try:
        for m in (ref, new):
            with torch.autocast("cuda", dtype=torch.bfloat16):
                h = m(input_ids=ids, attention_mask=am)[0]
            (h.float() * am[..., None] * torch.linspace(-1, 1, h.shape[-1], device=dev)).sum().backward()
            # (the key bias has a zero gradient in exact arithmetic: what it holds is rounding noise, left out)
            outs.append((h.detach(), {n: p_.grad.detach().clone() for n, p_ in m.named_parameters()
                                      if p_.grad is not None and not n.endswith("key.bias")}))
    finally:
        attention._attn_forward = orig
    assert seen == [(B, 4, T, HD)] * 2                              # both layers of the new model ran the kernels, at width 32
    live = am.bool()
    assert _rel(outs[1][0][live], outs[0][0][live]) < 1e-2
    for n in outs[0][1]:
        assert _rel(outs[1][1][n], outs[0][1][n]) < 3e-2, (n, _rel(outs[1][1][n], outs[0][1][n]))
    new.config.attention_probs_dropout_prob = 0.1
    for layer in new.encoder.layer:
        layer.attention.self.dropout.p = 0.1
        layer.attention.self._dalm_attn_calls = 0
    with torch.autocast("cuda", dtype=torch.bfloat16):
        h1 = new(input_ids=ids, attention_mask=am)[0]
        for layer in new.encoder.layer:
            layer.attention.self._dalm_attn_calls = 0
        h2 = new(input_ids=ids, attention_mask=am)[0]
    assert torch.isfinite(h1).all() and torch.equal(h1, h2) and not torch.equal(h1[live], outs[1][0][live])
    h1.float().sum().backward()
    assert all(torch.isfinite(p_.grad).all() for p_ in new.parameters() if p_.grad is not None)


def test_llama_of_width_32_on_dalm_sdpa_matches_sdpa_with_the_rotary_left_unfused(dev):
    """hidden 64 = 2 heads of 32: the model is switched to "dalm_sdpa", `use_llama_attention_node` may patch the layers but
    `rope_fusable` is False at this width, so the rotary embedding keeps its own kernels; logits and the q_proj gradients against
    the same weights on "sdpa" (bounds of test_llama_layer_on_dalm_sdpa_matches_sdpa)."""
    from transformers import LlamaConfig, LlamaForCausalLM

    from dalm_amd.models import attention, fastpath

    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2,
                      vocab_size=300)
    ref = LlamaForCausalLM(cfg).to(dev).to(torch.bfloat16).train()
    new = copy.deepcopy(ref)
    assert attention.use_hip_attention_backward(new) and new.config._attn_implementation == "dalm_sdpa"
    fastpath.use_llama_attention_node(new)
    fused, plain = [], []
    orig_rope, orig_fwd = attention.rope_sdpa, attention._attn_forward

    def spy_rope(*a, **kw):
        fused.append(1)
        return orig_rope(*a, **kw)

    def spy_fwd(q, *a, **kw):
        plain.append(tuple(q.shape))
        return orig_fwd(q, *a, **kw)

    B, T = 3, 64
    ids = torch.randint(0, 300, (B, T), device=dev)
    am = torch.ones(B, T, dtype=torch.long, device=dev)
    am[0, :20] = 0
    am[2, :63] = 0
    q = torch.zeros(B, 2, T, HD, dtype=torch.bfloat16, device=dev)
    cos = torch.zeros(1, T, HD, dtype=torch.bfloat16, device=dev)
    assert not attention.rope_fusable(q, q, cos, cos)
    assert attention.rope_fusable(q.repeat(1, 1, 1, 2), q.repeat(1, 1, 1, 2), cos.repeat(1, 1, 2), cos.repeat(1, 1, 2))
    outs = []
    attention.rope_sdpa, attention._attn_forward = spy_rope, spy_fwd
    try:
        for m in (ref, new):
            logits = m(input_ids=ids, attention_mask=am).logits
            (logits.float() * am[..., None]).square().sum().backward()
            outs.append((logits.detach(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}))
    finally:
        attention.rope_sdpa, attention._attn_forward = orig_rope, orig_fwd
    assert not fused and plain == [(B, 2, T, HD)] * 2               # the kernels ran, the fused rotary node did not
    live = am.bool()
    assert _rel(outs[1][0][live], outs[0][0][live]) < 1e-2
    for layer in (0, 1):
        qn = f"model.layers.{layer}.self_attn.q_proj.weight"
        assert _rel(outs[1][1][qn], outs[0][1][qn]) < 2e-2, (qn, _rel(outs[1][1][qn], outs[0][1][qn]))


# ---- step level ------------------------------------------------------------------------------------------------------------
def test_retriever_step_of_bge_small_width_padded_kernels_and_packed_vs_fp32_host(dev, monkeypatch):
    """RetrieverStep, bf16 autocast, train() with dropout 0, a 2-layer BERT of bge-small width (384 = 12 heads of 32), B 19, queries
    T 50 (5 - 15 live tokens, one single-token query), passages T 128: (a) padded on torch's attention (DALM_ATTN_KERNEL=0: what
    the model ran before the kernels took this width), (b) padded on the kernels, (c) packed.  Loss and gradient norm of each
    against the same model in fp32 on the host: (b) and (c) within max(1.5 x (a)'s distance, the bf16 bounds of the packed
    retriever-only test: 2.5e-4 loss, 7e-3 gradient norm)."""
    import dalm_oracle as O
    import realwidth as RW
    from transformers import BertConfig, BertModel

    from dalm_amd import packed
    from dalm_amd.models import AutoModelForSentenceEmbedding, attention
    from dalm_amd.training.step import RetrieverStep

    torch.manual_seed(0)
    bert = BertModel(BertConfig(hidden_size=384, num_hidden_layers=2, num_attention_heads=12, intermediate_size=1536, vocab_size=2000,
                                max_position_embeddings=512, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0))
    B, Tq, Tp = 19, 50, 128
    g = torch.Generator().manual_seed(3)
    ql = torch.randint(5, 16, (B, 1), generator=g)
    ql[3] = 1                                                        # a single-token query
    pl = torch.randint(30, Tp + 1, (B, 1), generator=g)
    batch = {"query_input_ids": torch.randint(5, 2000, (B, Tq), generator=g),
             "query_attention_mask": (torch.arange(Tq).unsqueeze(0) < ql).long(),
             "passage_input_ids": torch.randint(5, 2000, (B, Tp), generator=g),
             "passage_attention_mask": (torch.arange(Tp).unsqueeze(0) < pl).long()}

    calls = {"kernel": [], "fallback": 0}
    orig_fwd, orig_fb = attention._attn_forward, attention._packed_sdpa_torch

    def spy_fwd(q, k, v, pk, *a, **kw):
        calls["kernel"].append((tuple(q.shape), pk.packed is not None))
        return orig_fwd(q, k, v, pk, *a, **kw)

    def spy_fb(*a, **kw):
        calls["fallback"] += 1
        return orig_fb(*a, **kw)

    monkeypatch.setattr(attention, "_attn_forward", spy_fwd)
    monkeypatch.setattr(attention, "_packed_sdpa_torch", spy_fb)
    res = {}
    for mode in ("torch", "kernels", "packed"):
        calls["kernel"].clear()
        calls["fallback"] = 0
        if mode == "torch":
            monkeypatch.setenv("DALM_ATTN_KERNEL", "0")
        else:
            monkeypatch.delenv("DALM_ATTN_KERNEL", raising=False)
        model = AutoModelForSentenceEmbedding.from_modules(copy.deepcopy(bert), None, normalize=True, get_peft=False).to(dev)
        model.train()
        assert model.model.config._attn_implementation == ("sdpa" if mode == "torch" else "dalm_sdpa")
        params = [p for p in model.parameters() if p.requires_grad]
        opt = torch.optim.SGD(params, lr=0.0)
        step = RetrieverStep(model, opt, None, 100, autocast_dtype=torch.bfloat16, overlap_towers=True, track_grad_norm=True)
        host = packed.add_pack_plans(batch, packed.RETRIEVER_GROUPS) if mode == "packed" else batch
        loss = float(step({k: v.to(dev) for k, v in host.items()}))
        res[mode] = {"loss": loss, "grad_norm": float(step.grad_norm)}
        if mode == "torch":
            assert not calls["kernel"] and calls["fallback"] == 0
        elif mode == "kernels":      # two layers x (queries, passages), padded
            assert sorted(calls["kernel"]) == sorted([((B, 12, Tq, HD), False), ((B, 12, Tp, HD), False)] * 2), calls
        else:                        # really packed: one encoder call on the live tokens, a descriptor at the attention, no re-padding
            assert calls["fallback"] == 0 and len(calls["kernel"]) == 2, calls
            n_rows = host["query_pack_rows"].numel() + host["passage_pack_rows"].numel()
            assert all(shape == (1, 12, n_rows, HD) and saw_desc for shape, saw_desc in calls["kernel"]), calls
            assert n_rows < B * (Tq + Tp)
        del model, step, opt
        torch.cuda.empty_cache()

    old = torch.get_num_threads()
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    try:
        bert.train()
        q = O.ref_retrieval_embed(bert(batch["query_input_ids"], batch["query_attention_mask"])[0], batch["query_attention_mask"])
        p = O.ref_retrieval_embed(bert(batch["passage_input_ids"], batch["passage_attention_mask"])[0], batch["passage_attention_mask"])
        out = O.ref_step_loss(q, p, None, None, None, None, 100)
        out["loss"].backward()
    finally:
        torch.set_num_threads(old)
    host_s = {"loss": float(out["loss"].detach()), "grad_norm": RW.grad_norm([p_ for p_ in bert.parameters() if p_.requires_grad])}
    dist = {m: {k: abs(r[k] - host_s[k]) / max(abs(host_s[k]), 1e-30) for k in ("loss", "grad_norm")} for m, r in res.items()}
    print("hd32 retriever step:", {"host_fp32": host_s, **res}, "distance to host:", dist)
    floor = {"loss": 2.5e-4, "grad_norm": 7e-3}
    for mode in ("kernels", "packed"):
        for k in ("loss", "grad_norm"):
            assert dist[mode][k] <= max(1.5 * dist["torch"][k], floor[k]), (mode, k, dist)
