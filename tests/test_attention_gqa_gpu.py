"""Grouped-query attention on `dalm_attn_gqa_fwd` / `dalm_attn_gqa_bwd` (dalm_amd/csrc/attn.hip): k / v keep their Hkv heads,
query head h reads KV head h // (H // Hkv), dk / dv are summed over a group in f32 inside one workgroup.

The comparison path everywhere is the behaviour before these kernels: the equal-heads kernels on `repeat_kv`-materialised K / V
under autograd (per-head bf16 dk / dv summed by the expansion's backward).  O, the log-sum-exp and dq must carry the SAME BITS
(same arithmetic on the same values); dk / dv are held against a float64 evaluation, no further from it than the expanded path is
(x 1.5 + 1e-3, the rule tests/test_attention_gpu.py applies against torch)."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


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


def _expand(t, G):
    """transformers' repeat_kv, materialised: KV head j -> query heads j G .. j G + G - 1."""
    return t.repeat_interleave(G, dim=1)


def _ref64(q, k, v, mask, causal, scale, go, G):
    """tests/test_attention_gpu.py's float64 evaluation with the expansion INSIDE the graph: k.grad / v.grad have Hkv heads."""
    q, k, v = [t.detach().double().requires_grad_(True) for t in (q, k, v)]
    s = (q @ _expand(k, G).transpose(-1, -2)) * scale
    T = s.shape[-1]
    live = torch.ones(T, T, dtype=torch.bool, device=s.device).tril() if causal else torch.ones(T, T, dtype=torch.bool, device=s.device)
    live = live[None, None] if mask is None else (mask & live)
    s = s.masked_fill(~live, float("-inf"))
    p = torch.nan_to_num(torch.softmax(s, -1), nan=0.0)       # rows without a live key: zero output, zero gradient
    o = p @ _expand(v, G)
    o.backward(go.double())
    return o, q.grad, k.grad, v.grad


def _run(fn, q, k, v, go):
    q, k, v = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
    o = fn(q, k, v)
    o.backward(go)
    return o.detach(), q.grad, k.grad, v.grad


def _lse_of(fn, q, k, v, mask, causal):
    """The log-sum-exp the forward kernel wrote (what the backward kernels read)."""
    from dalm_amd.models import attention

    pk = attention._pack(mask, q.shape[0], q.shape[1], q.shape[2], causal, q.dtype, q.device)
    return fn(q, k, v, pk)[1]


def _check(native, expanded, ref, Hkv, dead_rows):
    """native / expanded / ref: (o, dq, dk, dv); dead_rows: boolean [B, T] (or [1, n]) - rows that attend nothing and are no key."""
    assert torch.equal(native[0], expanded[0]), float((native[0].float() - expanded[0].float()).abs().max())
    assert torch.equal(native[1], expanded[1]), float((native[1].float() - expanded[1].float()).abs().max())
    for name, a, b, r in zip(("dk", "dv"), native[2:], expanded[2:], ref[2:]):
        assert a.shape[1] == Hkv and a.shape == r.shape, name
        assert torch.isfinite(a).all(), name
        e_a, e_b = _rel(a, r), _rel(b, r)
        print(f"{name}: native {e_a:.3e} expanded-and-summed {e_b:.3e}")
        assert e_a <= 1.5 * e_b + 1e-3, (name, e_a, e_b)
    if dead_rows.any():
        for name, a in zip(("o", "dq", "dk", "dv"), native):
            x = a.transpose(1, 2)[dead_rows]                   # [rows, heads, hd]
            assert x.numel() and float(x.abs().max()) == 0.0, name


@pytest.fixture(params=[0, 1], ids=["split-by-grid", "unsplit"])
def splits(request, monkeypatch):
    """The dk / dv form: 0 = the library's choice (these grids are small: one query head per workgroup + the combine kernel),
    1 = one workgroup per KV head running through its whole group (what large grids get)."""
    from dalm_amd.models import attention

    monkeypatch.setattr(attention, "_gqa_splits", [request.param])
    return request.param


HEADS = [(128, 4, 2), (128, 8, 2), (64, 6, 2), (64, 8, 4)]       # (64, 7, 1): one KV head is the stride-0 multi-query route
LENGTHS = [40, 200, 256, 320]
STARTS = [[3, 0], [5, 150], [0, 255, 128], None]                   # left padding per batch row (a start past T: a row of padding only)
GRID = [(hd, H, Hkv, T, starts, layout) for (hd, H, Hkv) in HEADS for T in LENGTHS for starts in STARTS for layout in ("bthd", "bhtd")]


@pytest.mark.parametrize("hd,H,Hkv,T,starts,layout", GRID)
def test_grouped_kernels_against_the_expanded_path(dev, splits, hd, H, Hkv, T, starts, layout):
    """One partial key block (T 40), a ragged last block (200), a sequence that is almost all padding (start 255 of 256), key
    blocks dead for some rows, several query blocks per head (the dk / dv pipeline crosses head boundaries mid-stream)."""
    from dalm_amd.models import attention

    B, G = (2 if starts is None else len(starts)), H // Hkv
    g = torch.Generator().manual_seed(1000 * H + T + hd)

    def mk(heads):
        if layout == "bthd":
            return (torch.randn(B, T, heads, hd, generator=g) * 1.2).bfloat16().to(dev).transpose(1, 2)
        return (torch.randn(B, heads, T, hd, generator=g) * 1.2).bfloat16().to(dev)

    q, k, v, go = mk(H), mk(Hkv), mk(Hkv), mk(H)
    mask = None if starts is None else _hf_mask(B, T, starts, dev)
    causal = starts is None
    scale = hd ** -0.5
    assert attention.grouped_supported(q.requires_grad_(True), k, v, mask, 0.0, causal, {})
    assert not attention.grouped_supported(q, k, v, mask, 0.1, causal, {})                          # dropout: expand as before
    assert not attention.grouped_supported(q.float().requires_grad_(True), k.float(), v.float(), mask, 0.0, causal, {})

    native = _run(lambda a, b, c: attention._SdpaHipBackward.apply(a, b, c, mask, scale, causal), q, k, v, go)
    expanded = _run(lambda a, b, c: attention._SdpaHipBackward.apply(a, _expand(b, G), _expand(c, G), mask, scale, causal), q, k, v, go)
    ref = _ref64(q, k, v, mask, causal, scale, go, G)
    lse_n = _lse_of(lambda a, b, c, pk: attention._attn_forward(a, b, c, pk, scale, causal), q, k, v, mask, causal)
    lse_e = _lse_of(lambda a, b, c, pk: attention._attn_forward(a, _expand(b, G), _expand(c, G), pk, scale, causal), q, k, v, mask, causal)
    assert lse_n.shape == (B, H, T) and torch.equal(lse_n, lse_e)
    assert native[0].transpose(1, 2).is_contiguous()
    dead = torch.zeros(B, T, dtype=torch.bool, device=dev)
    for b_, st in enumerate(starts or []):
        dead[b_, :st] = True
    _check(native, expanded, ref, Hkv, dead)


def _packed_setup(dev, hd):
    """lens [128, 50, 90] left-padded to T 128, packed with multiple 64 (tests/test_attention_gpu.py's multi-query case)."""
    from dalm_amd import packed

    B, T, lens = 3, 128, [128, 50, 90]
    m2 = (torch.arange(T).unsqueeze(0) >= (T - torch.tensor(lens)).unsqueeze(1)).long()
    rows, cu = packed.pack_plan(m2, shifted=True, multiple=64)
    _i, pos, mask, _v = packed.packed_inputs(torch.zeros(B, T, dtype=torch.long, device=dev), m2.to(dev), rows.to(dev), cu.to(dev), True)
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, device=dev).float() / hd))
    ang = pos[0].float()[:, None] * inv[None, :]
    cos = torch.cat((ang.cos(), ang.cos()), -1).to(torch.bfloat16)[None]
    sin = torch.cat((ang.sin(), ang.sin()), -1).to(torch.bfloat16)[None]
    sq = packed.packed_of(mask)
    n = rows.numel()
    # the dense [1, 1, n, n] mask the descriptor stands for: same sequence, live key, causal
    r = torch.arange(n, device=dev)
    seq = torch.bucketize(r, sq.cu[1:].to(torch.int64), right=True)
    dense = (seq[:, None] == seq[None, :]) & (sq.key_live != 0)[None, :] & (r[None, :] <= r[:, None])
    # the [nseq, T] slots of the log-sum-exp layout that belong to a row (the rest is never written)
    slots = torch.arange(sq.T, device=dev)[None, :] < (sq.cu[1:] - sq.cu[:-1])[:, None]
    return n, mask, dense[None, None], cos, sin, (sq.key_live == 0)[None], slots


@pytest.mark.parametrize("hd,H,Hkv", [(64, 6, 2), (128, 4, 2)])
def test_grouped_kernels_packed_layout(dev, splits, hd, H, Hkv):
    from dalm_amd.models import attention

    n, mask, dense, _cos, _sin, dead, slots = _packed_setup(dev, hd)
    G = H // Hkv
    g = torch.Generator().manual_seed(hd + H)
    q, k, v, go = [(torch.randn(1, n, h_, hd, generator=g) * 1.2).bfloat16().to(dev).transpose(1, 2) for h_ in (H, Hkv, Hkv, H)]
    scale = hd ** -0.5
    assert attention.grouped_supported(q.requires_grad_(True), k, v, packed=True)
    native = _run(lambda a, b, c: attention._SdpaHipBackward.apply(a, b, c, mask, scale, False), q, k, v, go)
    expanded = _run(lambda a, b, c: attention._SdpaHipBackward.apply(a, _expand(b, G), _expand(c, G), mask, scale, False), q, k, v, go)
    ref = _ref64(q, k, v, dense, False, scale, go, G)
    lse_n = _lse_of(lambda a, b, c, pk: attention._attn_forward(a, b, c, pk, scale, False), q, k, v, mask, False)
    lse_e = _lse_of(lambda a, b, c, pk: attention._attn_forward(a, _expand(b, G), _expand(c, G), pk, scale, False), q, k, v, mask, False)
    assert lse_n.shape == (slots.shape[0], H, slots.shape[1])
    assert torch.equal(lse_n.transpose(1, 2)[slots], lse_e.transpose(1, 2)[slots])
    _check(native, expanded, ref, Hkv, dead)


@pytest.mark.parametrize("packed_mode", [False, True])
@pytest.mark.parametrize("hd,H,Hkv", [(64, 8, 2), (128, 4, 2)])
def test_rotation_in_the_epilogue_with_grouped_heads(dev, splits, hd, H, Hkv, packed_mode):
    """`rope_sdpa` with grouped k / v (the rotation's backward on the SUMMED f32 dk, once per KV head, one rounding) against
    `rope_sdpa` on expanded k / v (the rotation's backward per query head at the eager chain's rounding points, the bf16 results
    summed by the expansion's backward)."""
    from dalm_amd.models import attention

    G = H // Hkv
    g = torch.Generator().manual_seed(3 * hd + H)
    if packed_mode:
        n, mask, _dense, cos, sin, _dead, _slots = _packed_setup(dev, hd)
        Bq = 1
    else:
        Bq, n = 3, 128
        mask = _hf_mask(Bq, n, [0, 78, 38], dev)
        inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, device=dev).float() / hd))
        ang = torch.arange(n, device=dev).float()[:, None] * inv[None, :]
        cos = torch.cat((ang.cos(), ang.cos()), -1).to(torch.bfloat16)[None]
        sin = torch.cat((ang.sin(), ang.sin()), -1).to(torch.bfloat16)[None]
    q, k, v, go = [(0.7 * torch.randn(Bq, n, h_, hd, generator=g)).bfloat16().to(dev).transpose(1, 2) for h_ in (H, Hkv, Hkv, H)]
    scale = hd ** -0.5
    assert attention.rope_fusable(q, k, cos, sin)
    native = _run(lambda a, b, c: attention.rope_sdpa(a, b, c, cos, sin, mask, scale, False), q, k, v, go)
    expanded = _run(lambda a, b, c: attention.rope_sdpa(a, _expand(b, G), _expand(c, G), cos, sin, mask, scale, False), q, k, v, go)
    assert torch.equal(native[0], expanded[0])
    assert _rel(native[1], expanded[1]) < 1e-6
    assert native[2].shape[1] == Hkv and native[3].shape[1] == Hkv
    for name, a, b in zip(("dk", "dv"), native[2:], expanded[2:]):
        print(name, _rel(a, b))
        assert _rel(a, b) < 4e-3, (name, _rel(a, b))


@pytest.mark.parametrize("T,starts", [(320, [5, 150]), (256, None)])
def test_two_workgroups_per_group(dev, monkeypatch, T, starts):
    """G = 4 split over TWO workgroups (two heads each): neither the unsplit form nor one head per workgroup."""
    from dalm_amd.models import attention

    monkeypatch.setattr(attention, "_gqa_splits", [2])
    hd, H, Hkv, G, B = 64, 8, 2, 4, 2
    g = torch.Generator().manual_seed(T)
    q, k, v, go = [(torch.randn(B, T, h_, hd, generator=g) * 1.2).bfloat16().to(dev).transpose(1, 2) for h_ in (H, Hkv, Hkv, H)]
    mask = None if starts is None else _hf_mask(B, T, starts, dev)
    causal, scale = starts is None, hd ** -0.5
    native = _run(lambda a, b, c: attention._SdpaHipBackward.apply(a, b, c, mask, scale, causal), q, k, v, go)
    expanded = _run(lambda a, b, c: attention._SdpaHipBackward.apply(a, _expand(b, G), _expand(c, G), mask, scale, causal), q, k, v, go)
    dead = torch.zeros(B, T, dtype=torch.bool, device=dev)
    for b_, st in enumerate(starts or []):
        dead[b_, :st] = True
    _check(native, expanded, _ref64(q, k, v, mask, causal, scale, go, G), Hkv, dead)


def _model(hidden, dev):
    from transformers import LlamaConfig, LlamaForCausalLM

    from dalm_amd.models import attention, fastpath

    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=hidden, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                      vocab_size=300)
    cpu = LlamaForCausalLM(cfg).train()
    m = copy.deepcopy(cpu).to(dev).to(torch.bfloat16).train()
    cpu.load_state_dict({n: t.float().cpu() for n, t in m.state_dict().items()})       # fp32 copies of the SAME (bf16) weights
    assert attention.use_hip_attention_backward(m) and fastpath.use_roll_rope(m)
    assert fastpath.use_llama_attention_node(m) == 2
    return cpu, m


def _qkv_grads(m):
    return {n: p.grad.detach().clone() for n, p in m.named_parameters() if any(x in n for x in ("q_proj", "k_proj", "v_proj"))}


@pytest.mark.parametrize("hidden", [512, 256])
def test_llama_with_grouped_heads_runs_the_fused_node_without_repeat_kv(dev, monkeypatch, hidden):
    import transformers.integrations.sdpa_attention as hf_sdpa

    from dalm_amd import hip, packed
    from dalm_amd.models import attention

    cpu, m = _model(hidden, dev)
    B, T = 3, 64
    ids = torch.randint(0, 300, (B, T), device=dev)
    am = torch.ones(B, T, dtype=torch.long, device=dev)
    am[0, :20] = 0
    am[2, :41] = 0
    live = am.bool()

    def step(model, ids_, am_):
        model.zero_grad(set_to_none=True)
        logits = model(input_ids=ids_, attention_mask=am_, use_cache=False).logits
        (logits.float() * am_[..., None]).square().sum().backward()
        return logits.detach(), _qkv_grads(model)

    # the expanded path first: the same model with the grouped route switched off
    with monkeypatch.context() as mp:
        mp.setattr(attention, "grouped_supported", lambda *a, **kw: False)
        logits_e, grads_e = step(m, ids, am)
        rows, cu = packed.pack_plan(am, shifted=True, multiple=64)
        ids_p, pos, desc, valid = packed.packed_inputs(ids, am, rows.to(dev), cu.to(dev), causal=True)
        packed_e = m(input_ids=ids_p, attention_mask=desc, position_ids=pos, use_cache=False).logits.detach()

    calls = []
    real_call = hip.call

    def spy(name, *args):
        calls.append(name)
        return real_call(name, *args)

    def no_repeat(*a, **kw):
        raise AssertionError("repeat_kv called: k / v were expanded in memory")

    monkeypatch.setattr(hip, "call", spy)
    monkeypatch.setattr(hf_sdpa, "repeat_kv", no_repeat)
    logits_n, grads_n = step(m, ids, am)
    assert calls.count("dalm_attn_gqa_fwd") == 2 and calls.count("dalm_attn_gqa_bwd") == 2      # one fused node per layer
    assert not any(c in ("dalm_attn_fwd", "dalm_attn_bwd") for c in calls)
    assert calls.count("dalm_rope_qk_live") == 2                    # forward only: the rotation's backward rides in the epilogues
    assert torch.equal(logits_n[live], logits_e[live])

    # packed tower call
    calls.clear()
    packed_n = m(input_ids=ids_p, attention_mask=desc, position_ids=pos, use_cache=False).logits.detach()
    assert calls.count("dalm_attn_gqa_fwd") == 2 and "dalm_attn_fwd_packed" not in calls
    assert torch.equal(packed_n[0][valid], packed_e[0][valid])
    monkeypatch.undo()

    # projection weight gradients against an fp32 CPU run of the same weights on "eager" attention
    cpu.config._attn_implementation = "eager"
    cpu.zero_grad(set_to_none=True)
    lc = cpu(input_ids=ids.cpu(), attention_mask=am.cpu(), use_cache=False).logits
    (lc.float() * am.cpu()[..., None]).square().sum().backward()
    grads_c = _qkv_grads(cpu)
    for n in grads_c:
        e_n, e_e = _rel(grads_n[n], grads_c[n]), _rel(grads_e[n], grads_c[n])
        print(f"{n}: native {e_n:.3e} expanded {e_e:.3e}")
        assert e_n <= 1.5 * e_e + 1e-3, (n, e_n, e_e)
