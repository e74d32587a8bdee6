"""Qwen3 on the GPU: `dalm_head_norm_rope_fwd` / `dalm_head_norm_bwd` (dalm_amd/csrc/tower.hip) against a float64 restatement
and against transformers' own bf16 chain (Qwen3RMSNorm, then apply_rotary_pos_emb) on the same tensors; the fused node
`attention.norm_rope_sdpa`; a tiny Qwen3 with LoRA, patched against unpatched, padded and packed.

Tolerance rule for every comparison with a bf16 side: E_ref is the largest absolute error of transformers' own bf16 sequence
against the truth on the same inputs (float64 for kernels and node, the unpatched model in float32 for models); the new path's
error must be at most 2 E_ref, per tensor (the margin is for single-ulp flips from the summation order of mean(x^2)).  Zeros in
dead rows and "live rows get the same bits with and without row_live" are exact."""
import copy
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-6


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _rot(x):
    h = x.shape[-1] // 2
    return torch.cat((-x[..., h:], x[..., :h]), -1)


def _norm64(x, w, eps=EPS):
    x = x.double()
    rstd = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    return w.double() * (x * rstd), rstd.squeeze(-1)


def _truth_fwd(x, w, cos, sin):
    """[B, H, T, hd] -> (rotated normed value, rstd [B, H, T]) in float64."""
    y, rstd = _norm64(x, w)
    return y * cos.double().unsqueeze(1) + _rot(y) * sin.double().unsqueeze(1), rstd


def _hf_norm(w):
    """transformers' Qwen3RMSNorm.forward on the weight tensor `w` itself (a leaf's .grad is then the chain's weight gradient)."""
    import types

    from transformers.models.qwen3 import modeling_qwen3 as mq

    me = types.SimpleNamespace(weight=w, variance_epsilon=EPS)
    return lambda x: mq.Qwen3RMSNorm.forward(me, x)


def _tables(B, T, hd, cos_b, dev, pos=None):
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, device=dev).float() / hd))
    if pos is None:
        pos = torch.arange(T, device=dev).float()[None, :] + 7.0 * torch.arange(cos_b, device=dev).float()[:, None]
    ang = pos[..., None] * inv
    return (torch.cat((ang.cos(), ang.cos()), -1).to(torch.bfloat16), torch.cat((ang.sin(), ang.sin()), -1).to(torch.bfloat16))


def _qk(dev, hd, Hq, Hk, B, T, sliced, seed):
    """Pre-norm q / k as [B, H, T, hd] views: of dense [B, T, H, hd] tensors, or column slices of one [R, (Hq + 2 Hk) hd] buffer."""
    g = torch.Generator().manual_seed(seed)
    if sliced:
        buf = (3.0 * torch.randn(B * T, (Hq + 2 * Hk) * hd, generator=g)).bfloat16().to(dev)
        q = buf[:, :Hq * hd].view(B, T, Hq, hd).transpose(1, 2)
        k = buf[:, Hq * hd:(Hq + Hk) * hd].view(B, T, Hk, hd).transpose(1, 2)
        assert q.stride(2) == (Hq + 2 * Hk) * hd
    else:
        q = (3.0 * torch.randn(B, T, Hq, hd, generator=g)).bfloat16().to(dev).transpose(1, 2)
        k = (3.0 * torch.randn(B, T, Hk, hd, generator=g)).bfloat16().to(dev).transpose(1, 2)
    wq = (1.0 + 0.3 * (2.0 * torch.rand(hd, generator=g) - 1.0)).bfloat16().to(dev)
    wk = (1.0 + 0.3 * (2.0 * torch.rand(hd, generator=g) - 1.0)).bfloat16().to(dev)
    return q, k, wq, wk


def _s3(t):
    return (C.c_int64 * 3)(t.stride(0), t.stride(1), t.stride(2))


SENTINEL = 7.0


def _fresh(B, H, T, hd, dev):
    return torch.full((B, T, H, hd), SENTINEL, dtype=torch.bfloat16, device=dev).transpose(1, 2)


def _fwd_raw(q, k, wq, wk, cos, sin, live=None, hd=None, qs=None):
    """The C entry point with output buffers the test owns (pre-filled: an untouched buffer shows)."""
    from dalm_amd import hip

    B, Hq, T, hd_ = q.shape
    Hk = k.shape[1]
    qo, ko = _fresh(B, Hq, T, hd_, q.device), _fresh(B, Hk, T, hd_, q.device)
    rq = torch.full((B, T, Hq), SENTINEL, dtype=torch.float32, device=q.device)
    rk = torch.full((B, T, Hk), SENTINEL, dtype=torch.float32, device=q.device)
    cs = (C.c_int64 * 2)(cos.stride(0) if cos.shape[0] > 1 else 0, cos.stride(1))
    out = (qo, ko, rq, rk)
    try:
        hip.call("dalm_head_norm_rope_fwd", hip.ptr(q), hip.ptr(k), hip.ptr(wq), hip.ptr(wk), EPS, EPS, hip.ptr(cos), hip.ptr(sin), B, T,
                 Hq, Hk, hd or hd_, qs or _s3(q), _s3(k), _s3(qo), _s3(ko), cs, hip.ptr(qo), hip.ptr(ko), hip.ptr(rq), hip.ptr(rk),
                 hip.ptr(live), hip.stream())
    except ValueError as e:
        return out, str(e)
    return out, None


def _bwd_raw(gq, gk, q, k, wq, wk, rq, rk, live=None, hd=None, gqs=None):
    from dalm_amd import hip

    B, Hq, T, hd_ = q.shape
    Hk = k.shape[1]
    dq, dk = _fresh(B, Hq, T, hd_, q.device), _fresh(B, Hk, T, hd_, q.device)
    try:
        hip.call("dalm_head_norm_bwd", hip.ptr(gq), hip.ptr(gk), hip.ptr(q), hip.ptr(k), hip.ptr(wq), hip.ptr(wk), hip.ptr(rq), hip.ptr(rk),
                 B, T, Hq, Hk, hd or hd_, gqs or _s3(gq), _s3(gk), _s3(q), _s3(k), _s3(dq), _s3(dk), hip.ptr(dq), hip.ptr(dk),
                 hip.ptr(live), hip.stream())
    except ValueError as e:
        return (dq, dk), str(e)
    return (dq, dk), None


def _err(a, truth):
    return float((a.detach().double() - truth.double()).abs().max())


def _held(name, got, ref, truth, ratios=None):
    """The tolerance rule: the new path's largest absolute error against the truth is at most twice the bf16 reference's."""
    e_new, e_ref = _err(got, truth), _err(ref, truth)
    print(f"{name}: new {e_new:.4e} reference {e_ref:.4e} ratio {e_new / max(e_ref, 1e-300):.3f}")
    if ratios is not None:
        ratios.append(e_new / max(e_ref, 1e-300))
    assert torch.isfinite(got).all(), name
    assert e_new <= 2.0 * e_ref, (name, e_new, e_ref)


HEADS = [(4, 2), (2, 2), (3, 1)]
SIZES = [(2, 5), (1, 33), (3, 64)]         # odd row counts, head rows not a multiple of 4 / 8 per wave, more than one workgroup


@pytest.mark.parametrize("B,T", SIZES)
@pytest.mark.parametrize("Hq,Hk", HEADS)
@pytest.mark.parametrize("hd", [64, 128])
def test_kernels_against_float64_and_the_eager_chain(dev, hd, Hq, Hk, B, T):
    from transformers.models.qwen3 import modeling_qwen3 as mq

    from dalm_amd.models import tower_ops

    for sliced in (False, True):
        for cos_b in (1, B):
            q, k, wq, wk = _qk(dev, hd, Hq, Hk, B, T, sliced, 1000 * hd + 100 * Hq + 10 * B + T + sliced)
            cos, sin = _tables(B, T, hd, cos_b, dev)
            assert tower_ops.head_norm_rope_supported(q, k, wq, wk, cos, sin)
            (qo, ko, rq, rk), err = _fwd_raw(q, k, wq, wk, cos, sin)
            assert err is None, err
            nq, nk = _hf_norm(wq), _hf_norm(wk)
            with torch.no_grad():
                eq, ek = mq.apply_rotary_pos_emb(nq(q), nk(k), cos, sin)
            tag = f"hd{hd} H{Hq}/{Hk} B{B} T{T} {'sliced' if sliced else 'dense'} cos{cos_b}"
            for name, x, w, o, r, e in (("q", q, wq, qo, rq, eq), ("k", k, wk, ko, rk, ek)):
                truth, rstd = _truth_fwd(x, w, cos, sin)
                _held(f"fwd {name} {tag}", o, e, truth)
                # rstd is f32 throughout: 8 fma + log2(hd / 8) adds on positive terms, the division, the add and the hardware
                # rsqrt (1 ulp) - the reciprocal square root halves what the sum carries: well inside 16 x 2^-24 relative
                assert float(((r.transpose(1, 2).double() - rstd) / rstd).abs().max()) <= 16 * 2.0 ** -24, name
            # the launcher the node uses gives the same bits
            lo = tower_ops.head_norm_rope(q, k, wq, wk, EPS, EPS, cos, sin)
            assert torch.equal(lo[0], qo) and torch.equal(lo[1], ko) and torch.equal(lo[2], rq) and torch.equal(lo[3], rk)
            assert lo[0].transpose(1, 2).is_contiguous() and lo[4] is None

            # backward of the norm alone: gradients of the normed, un-rotated values in
            g = torch.Generator().manual_seed(T + hd)
            gq = torch.randn(B, T, Hq, hd, generator=g).bfloat16().to(dev).transpose(1, 2)
            gk = torch.randn(B, T, Hk, hd, generator=g).bfloat16().to(dev).transpose(1, 2)
            (dq, dk), err = _bwd_raw(gq, gk, q, k, wq, wk, rq, rk)
            assert err is None, err
            for name, x, w, go, d, norm in (("q", q, wq, gq, dq, nq), ("k", k, wk, gk, dk, nk)):
                x64 = x.detach().double().requires_grad_(True)
                _norm64(x64, w)[0].backward(go.double())
                xe = x.detach().clone().requires_grad_(True)
                norm(xe).backward(go)
                _held(f"bwd {name} {tag}", d, xe.grad, x64.grad)
            lo = tower_ops.head_norm_bwd(gq, gk, q, k, wq, wk, rq, rk)
            assert torch.equal(lo[0], dq) and torch.equal(lo[1], dk) and lo[0].transpose(1, 2).is_contiguous()


@pytest.mark.parametrize("B,T", SIZES)
@pytest.mark.parametrize("Hq,Hk", HEADS)
@pytest.mark.parametrize("hd", [64, 128])
def test_row_liveness_is_exact(dev, hd, Hq, Hk, B, T):
    """About 40 % dead rows, the first and the last among them; their inputs are NaN: nothing of a dead row may be loaded."""
    q, k, wq, wk = _qk(dev, hd, Hq, Hk, B, T, True, 7 * hd + Hq + B * T)
    cos, sin = _tables(B, T, hd, B, dev)
    g = torch.Generator().manual_seed(B * T)
    gq = torch.randn(B, T, Hq, hd, generator=g).bfloat16().to(dev).transpose(1, 2)
    gk = torch.randn(B, T, Hk, hd, generator=g).bfloat16().to(dev).transpose(1, 2)
    live = (torch.rand(B * T, generator=g) >= 0.4)
    live[0] = live[-1] = False
    assert 0 < int(live.sum()) < B * T
    live = live.to(dev)
    lv = live.view(torch.uint8)
    (qo, ko, rq, rk), err = _fwd_raw(q, k, wq, wk, cos, sin)
    assert err is None, err
    (dq, dk), err = _bwd_raw(gq, gk, q, k, wq, wk, rq, rk)
    assert err is None, err
    dead = ~live.view(B, T)
    nan = float("nan")
    for t in (q, k, gq, gk, cos.unsqueeze(1), sin.unsqueeze(1)):
        t.transpose(1, 2)[dead] = nan
    rq_in, rk_in = rq.clone(), rk.clone()
    (qo2, ko2, rq2, rk2), err = _fwd_raw(q, k, wq, wk, cos, sin, lv)
    assert err is None, err
    rq_in[dead], rk_in[dead] = nan, nan
    (dq2, dk2), err = _bwd_raw(gq, gk, q, k, wq, wk, rq_in, rk_in, lv)
    assert err is None, err
    for name, a, b in (("q_out", qo, qo2), ("k_out", ko, ko2), ("dq", dq, dq2), ("dk", dk, dk2)):
        a, b = a.transpose(1, 2), b.transpose(1, 2)                  # [B, T, H, hd]
        assert torch.equal(a[~dead].view(torch.int16), b[~dead].view(torch.int16)), name
        assert b[dead].numel() and float(b[dead].abs().max()) == 0.0 and not torch.isnan(b[dead]).any(), name
    for name, a, b in (("rstd_q", rq, rq2), ("rstd_k", rk, rk2)):
        assert torch.equal(a[~dead], b[~dead]) and float(b[dead].abs().max()) == 0.0, name


def test_unsupported_calls_return_the_error_code_and_write_nothing(dev):
    from dalm_amd.models import tower_ops

    def untouched(bufs):
        torch.cuda.synchronize()
        return all(float((b.float() - SENTINEL).abs().max()) == 0.0 for b in bufs)

    B, T, Hq, Hk = 2, 5, 4, 2
    for hd in (32, 96):
        q, k, wq, wk = _qk(dev, hd, Hq, Hk, B, T, False, hd)
        cos, sin = _tables(B, T, hd, 1, dev)
        assert not tower_ops.head_norm_rope_supported(q, k, wq, wk, cos, sin)
        out, err = _fwd_raw(q, k, wq, wk, cos, sin)
        assert err is not None and "code -2" in err and "head width" in err and untouched(out)
        out, err = _bwd_raw(q, k, q, k, wq, wk, out[2], out[3])
        assert err is not None and "code -2" in err and untouched(out)
    hd = 64
    q, k, wq, wk = _qk(dev, hd, Hq, Hk, B, T, False, 5)
    cos, sin = _tables(B, T, hd, 1, dev)
    rq = torch.ones(B, T, Hq, device=dev)
    rk = torch.ones(B, T, Hk, device=dev)
    # a pointer 2 bytes off a 16-byte boundary
    flat = torch.zeros(q.numel() + 8, dtype=torch.bfloat16, device=dev)
    q_off = flat[1:1 + q.numel()].view(B, T, Hq, hd).transpose(1, 2)
    assert q_off.data_ptr() % 16 == 2 and not tower_ops.head_norm_rope_supported(q_off, k, wq, wk, cos, sin)
    out, err = _fwd_raw(q_off, k, wq, wk, cos, sin)
    assert err is not None and "code -4" in err and untouched(out)
    out, err = _bwd_raw(q_off, k, q, k, wq, wk, rq, rk)
    assert err is not None and "code -4" in err and untouched(out)
    # an odd row stride (the kernel is never launched: the strides only need to be what is passed)
    odd = (C.c_int64 * 3)(q.stride(0), q.stride(1), q.stride(2) + 1)
    out, err = _fwd_raw(q, k, wq, wk, cos, sin, qs=odd)
    assert err is not None and "code -4" in err and untouched(out)
    out, err = _bwd_raw(q, k, q, k, wq, wk, rq, rk, gqs=odd)
    assert err is not None and "code -4" in err and untouched(out)
    wide = torch.zeros(B, T, Hq, hd + 1, dtype=torch.bfloat16, device=dev)[..., :hd].transpose(1, 2)
    assert not tower_ops.head_norm_rope_supported(wide, k, wq, wk, cos, sin)
    assert not tower_ops.head_norm_rope_supported(q, k, wq.float(), wk, cos, sin)            # an f32 weight promotes the eager product
    assert not tower_ops.head_norm_rope_supported(q.float(), k.float(), wq.float(), wk.float(), cos.float(), sin.float())
    assert not tower_ops.head_norm_rope_supported(q.cpu(), k.cpu(), wq.cpu(), wk.cpu(), cos.cpu(), sin.cpu())


# ---- the node -----------------------------------------------------------------------------------------------------------
def _attention64(q, k, v, dense, causal, scale, G):
    s = (q @ k.repeat_interleave(G, dim=1).transpose(-1, -2)) * scale
    T = s.shape[-1]
    keep = torch.ones(T, T, dtype=torch.bool, device=s.device)
    keep = keep.tril() if causal else keep
    keep = keep[None, None] if dense is None else (dense & keep)
    p = torch.nan_to_num(torch.softmax(s.masked_fill(~keep, float("-inf")), -1), nan=0.0)   # rows without a live key: zeros
    return p @ v.repeat_interleave(G, dim=1)


NODE_CASES = [("left", 4, 4, 64), ("left", 4, 2, 128), ("bidirectional", 4, 4, 128), ("bidirectional", 6, 2, 64),
              ("causal", 4, 2, 64), ("packed", 4, 4, 128), ("packed", 4, 2, 64)]


@pytest.mark.parametrize("mode,Hq,Hk,hd", NODE_CASES)
def test_node_against_float64_and_the_eager_chain(dev, mode, Hq, Hk, hd):
    from test_attention_gqa_gpu import _hf_mask, _packed_setup
    from transformers.models.qwen3 import modeling_qwen3 as mq

    from dalm_amd.models import attention

    G = Hq // Hk
    if mode == "packed":
        T, mask, dense, cos, sin, _dead, _slots = _packed_setup(dev, hd)
        B, causal = 1, False
    else:
        B, T = 3, 96
        starts = [0, 50, 17]
        cos, sin = _tables(B, T, hd, 1, dev)
        col = torch.arange(T, device=dev)
        if mode == "left":
            mask, causal = _hf_mask(B, T, starts, dev), False
        elif mode == "bidirectional":
            mask, causal = (col[None, :] >= torch.tensor(starts, device=dev)[:, None])[:, None, None, :].expand(B, 1, T, T).contiguous(), False
        else:
            mask, causal = None, True
        dense = mask
    g = torch.Generator().manual_seed(hd + 10 * Hq + len(mode))
    W = (Hq + 2 * Hk) * hd
    buf = (1.5 * torch.randn(B * T, W, generator=g)).bfloat16().to(dev)
    go = torch.randn(B, T, Hq, hd, generator=g).bfloat16().to(dev).transpose(1, 2)
    wq0 = (1.0 + 0.3 * (2.0 * torch.rand(hd, generator=g) - 1.0)).bfloat16().to(dev)
    wk0 = (1.0 + 0.3 * (2.0 * torch.rand(hd, generator=g) - 1.0)).bfloat16().to(dev)
    scale = hd ** -0.5

    def split(x):
        q = x[:, :Hq * hd].view(B, T, Hq, hd).transpose(1, 2)
        k = x[:, Hq * hd:(Hq + Hk) * hd].view(B, T, Hk, hd).transpose(1, 2)
        v = x[:, (Hq + Hk) * hd:].view(B, T, Hk, hd).transpose(1, 2)
        return q, k, v

    def run(fn, dtype):
        x = buf.detach().to(dtype).requires_grad_(True)
        wq, wk = wq0.detach().to(dtype).requires_grad_(True), wk0.detach().to(dtype).requires_grad_(True)
        out = fn(*split(x), wq, wk)
        out.backward(go.to(dtype))
        dq, dk, dv = split(x.grad)
        return {"out": out.detach(), "dq": dq, "dk": dk, "dv": dv, "dwq": wq.grad, "dwk": wk.grad}

    def new(q, k, v, wq, wk):
        assert attention.rope_fusable(q, k, cos, sin)
        return attention.norm_rope_sdpa(q, k, v, wq, wk, EPS, EPS, cos, sin, mask, scale, causal)

    def eager(q, k, v, wq, wk):
        qr, kr = mq.apply_rotary_pos_emb(_hf_norm(wq)(q), _hf_norm(wk)(k), cos, sin)
        return attention.sdpa(qr, kr, v, mask, scale, causal)

    def truth(q, k, v, wq, wk):
        yq, yk = _norm64(q, wq)[0], _norm64(k, wk)[0]
        c, s = cos.double().unsqueeze(1), sin.double().unsqueeze(1)
        return _attention64(yq * c + _rot(yq) * s, yk * c + _rot(yk) * s, v, dense, causal, scale, G)

    got, ref, tru = run(new, torch.bfloat16), run(eager, torch.bfloat16), run(truth, torch.float64)
    for name in ("out", "dq", "dk", "dv", "dwq", "dwk"):
        _held(f"node {mode} H{Hq}/{Hk} hd{hd} {name}", got[name], ref[name], tru[name])


# ---- the model -----------------------------------------------------------------------------------------------------------
def _tiny(dev):
    from transformers import Qwen3Config, Qwen3ForCausalLM

    torch.manual_seed(0)
    cfg = Qwen3Config(vocab_size=128, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, head_dim=64)
    m = Qwen3ForCausalLM(cfg)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith(("q_norm.weight", "k_norm.weight")):
                p.add_(0.3 * (2.0 * torch.rand(p.shape) - 1.0))
            p.copy_(p.to(torch.bfloat16).float())              # every copy below holds the SAME (bf16-exact) weights
    return m.train()


def _with_lora(model, train_norms):
    from dalm_amd.models import lora

    lora.inject_lora(model, ["q_proj", "v_proj"], lora_dropout=0.0)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if "lora_B" in name:                # at its zero initialisation dA is identically zero and proves nothing
                p.copy_((0.05 * torch.randn(p.shape, generator=g)).to(torch.bfloat16).float())
            if "lora_A" in name:
                p.copy_(p.to(torch.bfloat16).float())
    if train_norms:
        for name, p in model.named_parameters():
            if name.endswith(("q_norm.weight", "k_norm.weight")):
                p.requires_grad_(True)
    return model


def _cast(model, dev, dtype):
    model = model.to(dev)
    if dtype == torch.bfloat16:
        for p in model.parameters():
            if not p.requires_grad or p.dim() == 1:           # frozen base and the norm weights; the adapters stay f32
                p.data = p.data.to(torch.bfloat16)
    return model.train()


@pytest.mark.parametrize("train_norms", [False, True])
def test_tiny_model_with_lora_patched_against_unpatched(dev, monkeypatch, train_norms):
    from dalm_amd import hip, packed
    from dalm_amd.models import attention, fastpath, lora
    from dalm_amd.models.frozen_linear import use_transposed_dgrad

    base = _tiny(dev)
    B, T = 3, 48
    ids = torch.randint(0, 128, (B, T), generator=torch.Generator().manual_seed(1)).to(dev)
    am = torch.ones(B, T, dtype=torch.long, device=dev)
    am[0, :20] = 0
    am[2, :33] = 0
    w = torch.randn(B, T, 128, generator=torch.Generator().manual_seed(2)).to(dev) * am[..., None]
    rows, cu = packed.pack_plan(am.cpu(), shifted=True, multiple=64)
    rows, cu = rows.to(dev), cu.to(dev)
    valid = rows >= 0
    sel = rows[valid]
    seen = am.reshape(-1).index_select(0, sel) != 0         # the rows a loss reads (a padding row in front of a sequence is packed too)
    wh = torch.randn(B * T, 256, generator=torch.Generator().manual_seed(4)).to(dev).index_select(0, sel) * seen[:, None]

    def trainable(model):
        return {n: p for n, p in model.named_parameters() if p.requires_grad}

    def grads(model):
        return {n: p.grad.detach().float().clone() for n, p in trainable(model).items()}

    def padded(model, dtype):
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
            logits = model(input_ids=ids, attention_mask=am, use_cache=False).logits
        (logits.float() * w).sum().backward()
        return logits.detach().float() * am[..., None], grads(model)

    def hidden_padded(model, dtype):
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
            h = model.base_model(input_ids=ids, attention_mask=am, use_cache=False)[0].reshape(B * T, -1).index_select(0, sel)
        (h.float() * wh).sum().backward()
        return h.detach().float()[seen], grads(model)

    with monkeypatch.context() as mp:                                 # the references: transformers' own code, one eager LoRA
        mp.setattr(lora, "_GROUPS", False)                            # branch per projection
        mp.setattr(lora, "_FUSED", False)
        truth = _cast(_with_lora(copy.deepcopy(base), train_norms), dev, torch.float32)
        plain = _cast(_with_lora(copy.deepcopy(base), train_norms), dev, torch.bfloat16)
        t_logits, t_grads = padded(truth, torch.float32)
        r_logits, r_grads = padded(plain, torch.bfloat16)
        t_h, t_g = hidden_padded(truth, torch.float32)
        r_h, r_g = hidden_padded(plain, torch.bfloat16)

    fast = copy.deepcopy(base)
    fastpath.use_native_rms_norm(fast)
    assert fastpath.use_swiglu_kernel(fast) == 2 and fastpath.use_fused_residual_norm(fast) == 2
    assert attention.use_hip_attention_backward(fast) and fastpath.use_qwen3_attention_node(fast) == 2
    fast = _cast(_with_lora(fast, train_norms), dev, torch.bfloat16)
    use_transposed_dgrad(fast)
    for layer in fast.model.layers:                                    # q | k | v of a Qwen3 layer form one group
        a = layer.self_attn
        assert a.q_proj._group is not None and a.q_proj._group is a.k_proj._group is a.v_proj._group
        assert len(a.q_proj._group.members) == 3

    calls = []
    real_call = hip.call

    def spy(name, *args):
        calls.append(name)
        return real_call(name, *args)

    monkeypatch.setattr(hip, "call", spy)
    f_logits, f_grads = padded(fast, torch.bfloat16)
    assert calls.count("dalm_head_norm_rope_fwd") == 2 and calls.count("dalm_head_norm_bwd") == 2, calls   # the node ran, once per layer
    assert calls.count("dalm_attn_gqa_fwd") == 2 and calls.count("dalm_attn_gqa_bwd") == 2
    assert any(c.startswith("dalm_lora2_") for c in calls), calls                                 # and the q|k|v group's kernels
    assert all(l.self_attn.q_proj._group.enabled for l in fast.model.layers)
    names = set(t_grads)
    assert names == set(r_grads) == set(f_grads) and any("lora_A" in n for n in names)
    assert train_norms == any(n.endswith("q_norm.weight") for n in names)
    _held("model padded logits", f_logits, r_logits, t_logits)
    for n in sorted(names):
        _held(f"model padded {n}", f_grads[n], r_grads[n], t_grads[n])

    # packed: the generator's decoder stack on the un-padded rows, against the same rows of the padded truth
    calls.clear()
    fast.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        h = packed.generator_hidden(fast, ids, am, rows, cu)[valid]
    (h.float() * wh).sum().backward()
    assert calls.count("dalm_head_norm_rope_fwd") == 2 and calls.count("dalm_head_norm_bwd") == 2, calls
    _held("model packed hidden", h.detach().float()[seen], r_h, t_h)
    f_g = grads(fast)
    for n in sorted(names):
        _held(f"model packed {n}", f_g[n], r_g[n], t_g[n])


# ---- steps ---------------------------------------------------------------------------------------------------------------
_BUILT = {}


def _qwen3_lm(bare=False):
    """The tiny Qwen3 with LoRA on q / v (no dropout, lora_B randomised), weights on the bf16 grid; built once on the CPU."""
    if "lm" not in _BUILT:
        from dalm_amd.models.lora import LoRALinear

        lm = _with_lora(_tiny(None), False)
        for m in lm.modules():
            if isinstance(m, LoRALinear):
                assert m.lora_dropout_p == 0.0 if hasattr(m, "lora_dropout_p") else True
        _BUILT["lm"] = lm
    lm = copy.deepcopy(_BUILT["lm"])
    return lm.model if bare else lm


def _tiny_bert():
    if "bert" not in _BUILT:
        from transformers import BertConfig, BertModel

        from dalm_amd.models import lora

        torch.manual_seed(5)
        bert = BertModel(BertConfig(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512, vocab_size=128,
                                    max_position_embeddings=64, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0))
        with torch.no_grad():
            for p in bert.parameters():
                p.copy_(p.to(torch.bfloat16).float())
        lora.inject_lora(bert, ["key", "query", "value"], lora_dropout=0.0)
        g = torch.Generator().manual_seed(6)
        with torch.no_grad():
            for n, p in bert.named_parameters():
                if "lora_B" in n:
                    p.copy_(0.05 * torch.randn(p.shape, generator=g))
        _BUILT["bert"] = bert
    return copy.deepcopy(_BUILT["bert"])


def _rag_model(dev, precision, causal_retriever=False):
    from dalm_amd.models import AutoModelForRagE2E

    retriever = _qwen3_lm(bare=True) if causal_retriever else _tiny_bert()
    model = AutoModelForRagE2E.from_modules(retriever, _qwen3_lm(), None, None, normalize=True, get_peft=None,
                                            retriever_is_autoregressive=causal_retriever).to(dev)
    if precision == "bf16":
        for p in model.parameters():
            if not p.requires_grad:
                p.data = p.data.to(torch.bfloat16)
    return model.train()


def _one_step(kind, batch, mode, precision, dev, spy_on=None):
    """test_causal_retriever_gpu.py's `_run_step` with a Qwen3 in it: kind "rag" = tiny BERT retriever + tiny Qwen3 generator,
    kind "retriever" = a tiny Qwen3 as a causal-LM retriever."""
    from test_causal_retriever_gpu import _GradSnapshot

    from dalm_amd import hip, packed
    from dalm_amd.models import AutoModelForSentenceEmbedding
    from dalm_amd.training.step import RagE2EStep, RetrieverStep

    if kind == "retriever":
        model = AutoModelForSentenceEmbedding.from_modules(_qwen3_lm(), None, normalize=True, get_peft=False, is_autoregressive=True).to(dev)
        if precision == "bf16":
            for p in model.parameters():
                if not p.requires_grad:
                    p.data = p.data.to(torch.bfloat16)
        model.train()
        groups = packed.RETRIEVER_GROUPS_CAUSAL
    else:
        model = _rag_model(dev, precision)
        groups = packed.RAG_GROUPS
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    opt = torch.optim.SGD([p for _, p in named], lr=0.0)
    snap = _GradSnapshot(named)
    opt.register_step_pre_hook(snap)
    cls = RetrieverStep if kind == "retriever" else RagE2EStep
    step = cls(model, opt, None, 100, autocast_dtype=torch.bfloat16 if precision == "bf16" else None, overlap_towers=True,
               track_grad_norm=True)
    host = packed.add_pack_plans(batch, groups) if mode == "packed" else batch
    calls, real_call = [], hip.call
    hip.call = lambda name, *a: (calls.append(name), real_call(name, *a))[1]
    try:
        dbatch = {k: v.to(dev) for k, v in host.items()}
        loss = float(step(dbatch))
    finally:
        hip.call = real_call
    if kind == "rag" and mode == "packed":
        assert step._packed_generator(dbatch), "the packed generator path did not run"
    return {"loss": loss, "grad_norm": float(step.grad_norm)}, snap.grads, calls


def _rel_norm(a, b):
    return float((a.double() - b.double()).norm()) / max(float(b.double().norm()), 1e-30)


def test_rag_step_with_a_qwen3_generator_packed_against_padded(dev):
    """One RAG-e2e step, tiny BERT retriever + tiny Qwen3 generator, at the bounds tests/test_packed_gpu.py holds the Llama step
    to: fp32 - loss, gradient norm and every gradient within 1e-4; bf16 autocast - loss within 2.5e-4 and gradient norm within
    2.2e-3 of the padded bf16 step, every parameter's gradient within twice the padded bf16 step's own distance from the fp32
    step + 5e-3, and within 4e-2 outright."""
    from test_causal_retriever_gpu import _rag_batch

    batch = _rag_batch(False)
    res = {(m, p): _one_step("rag", batch, m, p, dev) for p in ("fp32", "bf16") for m in ("padded", "packed")}
    for m in ("padded", "packed"):                    # the fused node ran in both bf16 layouts, one launch per layer each way
        calls = res[m, "bf16"][2]
        assert calls.count("dalm_head_norm_rope_fwd") == 2 and calls.count("dalm_head_norm_bwd") == 2, (m, calls)
        assert "dalm_head_norm_rope_fwd" not in res[m, "fp32"][2]
    g32, p32 = res["padded", "fp32"][1], res["packed", "fp32"][1]
    assert set(g32) == set(p32) and any("generator_model" in n for n in g32)
    for k in ("loss", "grad_norm"):
        d = abs(res["packed", "fp32"][0][k] - res["padded", "fp32"][0][k]) / abs(res["padded", "fp32"][0][k])
        print(f"fp32 packed vs padded {k}: {d:.3e}")
        assert d <= 1e-4, (k, d)
    worst = max(_rel_norm(p32[n], g32[n]) for n in g32 if float(g32[n].double().norm()) >= 1e-7)
    print(f"fp32 worst gradient: {worst:.3e}")
    assert worst <= 1e-4
    for k, tol in (("loss", 2.5e-4), ("grad_norm", 2.2e-3)):
        d = abs(res["packed", "bf16"][0][k] - res["padded", "bf16"][0][k]) / abs(res["padded", "bf16"][0][k])
        print(f"bf16 packed vs padded {k}: {d:.3e}")
        assert d <= tol, (k, d)
    g16, p16 = res["padded", "bf16"][1], res["packed", "bf16"][1]
    for n in sorted(g32):
        den = max(float(g32[n].double().norm()), 1e-30)
        d_pad, d_pack = float((g16[n].double() - g32[n].double()).norm()) / den, float((p16[n].double() - g32[n].double()).norm()) / den
        print(f"{n}: padded {d_pad:.3e} packed {d_pack:.3e}")
        if float(g32[n].double().norm()) >= 1e-7:
            assert d_pack <= 2.0 * d_pad + 5e-3 and d_pack <= 4e-2, (n, d_pack, d_pad)


@pytest.mark.parametrize("left", [True, False], ids=["left", "right"])
def test_qwen3_retriever_step_packed_against_padded(dev, left):
    """A tiny Qwen3 as a causal-LM retriever at the bounds tests/test_causal_retriever_gpu.py holds llama to.  The padded run is
    the existing padded call; packed, its q_norm / k_norm / rotary stay transformers' code (no fused node on retrievers)."""
    from test_causal_retriever_gpu import _dist, _retriever_batch

    batch = _retriever_batch(left)
    res = {(m, p): _one_step("retriever", batch, m, p, dev) for p in ("fp32", "bf16") for m in ("padded", "packed")}
    for key, (_, _, calls) in res.items():
        assert "dalm_head_norm_rope_fwd" not in calls, key
    assert any(c.startswith("dalm_attn_gqa") for c in res["packed", "bf16"][2])            # "dalm_sdpa" did serve the packed rows
    assert any(c.startswith("dalm_swiglu") for c in res["padded", "bf16"][2]) and any(c.startswith("dalm_rms_norm") for c in res["padded", "bf16"][2])
    d32 = _dist(res["packed", "fp32"][0], res["padded", "fp32"][0])
    gp, gq = res["packed", "fp32"][1], res["padded", "fp32"][1]
    assert set(gp) == set(gq)
    worst = max(_rel_norm(gp[n], gq[n]) for n in gq if float(gq[n].double().norm()) >= 1e-7)
    d16 = _dist(res["packed", "bf16"][0], res["padded", "bf16"][0])
    pad16 = _dist(res["padded", "bf16"][0], res["padded", "fp32"][0])
    pack16 = _dist(res["packed", "bf16"][0], res["padded", "fp32"][0])
    print(f"fp32 packed vs padded {d32}, worst gradient {worst:.3e}; bf16 packed vs padded {d16}; padded vs fp32 {pad16}; packed vs fp32 {pack16}")
    assert d32["loss"] <= 1e-4 and d32["grad_norm"] <= 1e-4 and worst <= 1e-4
    for k, tol in (("loss", 2.5e-4), ("grad_norm", 7e-3)):
        assert d16[k] <= tol, (k, d16)
        assert pack16[k] <= (tol if pad16[k] <= tol else 2.0 * pad16[k] + tol), (k, pack16, pad16)


def test_three_graphed_steps_against_eager(dev):
    """bf16 autocast (the node takes bf16 only), tiny BERT retriever + tiny Qwen3 generator: three optimizer steps through
    `GraphedStep` against the eager step, at the bounds of tests/test_step_parity_gpu.py's graphed-against-eager comparison
    (losses within 2e-5, the final parameter sum within 1e-5, no eager fall-back)."""
    from test_causal_retriever_gpu import _rag_batch

    from dalm_amd import hip
    from dalm_amd.training.graphed import GraphedStep, make_capturable_adam
    from dalm_amd.training.step import RagE2EStep

    batches = []
    for i in range(3):
        b = _rag_batch(False)
        g = torch.Generator().manual_seed(40 + i)
        b["generator_input_input_ids"] = torch.randint(3, 128, b["generator_input_input_ids"].shape, generator=g)
        batches.append({k: v.to(dev) for k, v in b.items()})

    def run(graph):
        model = _rag_model(dev, "bf16")
        params = [p for p in model.parameters() if p.requires_grad]
        opt = make_capturable_adam(params, 1e-3, dev) if graph else torch.optim.Adam(params, lr=1e-3)
        step = RagE2EStep(model, opt, None, 100, autocast_dtype=torch.bfloat16, inplace_grad=True, overlap_towers=graph)
        if graph:
            step = GraphedStep(step, warmup=0)
        calls, real_call = [], hip.call
        hip.call = lambda name, *a: (calls.append(name), real_call(name, *a))[1]
        try:
            losses = [float(step(b)) for b in batches]
        finally:
            hip.call = real_call
        final = float(sum(p.detach().double().abs().sum() for p in params))
        return losses, final, step, calls

    eager, e_final, _, e_calls = run(False)
    graphed, g_final, gstep, g_calls = run(True)
    assert e_calls.count("dalm_head_norm_rope_fwd") == 6 and e_calls.count("dalm_head_norm_bwd") == 6
    assert g_calls.count("dalm_head_norm_rope_fwd") >= 2 and g_calls.count("dalm_head_norm_bwd") >= 2      # recorded at capture
    assert gstep.failed is None and gstep.eager_calls == 0, (gstep.failed, gstep.eager_calls)
    print("eager", eager, e_final, "graphed", graphed, g_final)
    for a, b in zip(eager, graphed):
        assert abs(a - b) <= 2e-5 * abs(a), (eager, graphed)
    assert abs(e_final - g_final) <= 1e-5 * e_final
