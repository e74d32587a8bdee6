"""`dalm_rope_qk` / `dalm_swiglu_*` (dalm_amd/csrc/tower.hip) against the eager chains they replace: transformers' own
`apply_rotary_pos_emb` and `LlamaMLP` (what the reference's generator runs, dalm/models/rag_e2e_base_model.py:104-106).
The kernels round where the eager ops round, so the rotary results must be EQUAL (forward and backward, bf16 and f32);
SwiGLU goes through exp(), where one f32 ulp of difference between two exp implementations may move a bf16 rounding: equal
up to one bf16 ulp on a vanishing fraction of elements, 1e-6 relative in f32."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _hf_rope():
    from transformers.models.llama import modeling_llama as m

    return getattr(m, "_dalm_orig_apply_rotary_pos_emb", m.apply_rotary_pos_emb)


def _cos_sin(B, T, hd, dtype, dev, g):
    inv = 1.0 / (10000 ** (torch.arange(0, hd, 2).float() / hd))
    if B % 2 == 0:       # transformers' default position_ids are [1, T]: one table broadcast over the batch
        B = 1
    pos = torch.arange(T).float()[None, :].expand(B, T) + torch.randint(0, 50, (B, 1), generator=g).float()
    fr = pos[..., None] * inv[None, None, :]
    emb = torch.cat((fr, fr), dim=-1)
    return emb.cos().to(dtype).to(dev), emb.sin().to(dtype).to(dev)


ROPE = [(18, 32, 32, 256, 128), (2, 4, 2, 7, 64), (3, 2, 2, 5, 8), (1, 3, 1, 9, 6), (2, 8, 8, 33, 96),
        (2, 71, 1, 19, 64)]       # Falcon-7B: 71 query heads, one shared key head


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("B,Hq,Hk,T,hd", ROPE)
@pytest.mark.parametrize("layout", ["projection-view", "contiguous"])
def test_rope_kernel_equals_transformers_chain(dev, B, Hq, Hk, T, hd, dtype, layout):
    from dalm_amd.models import tower_ops

    g = torch.Generator().manual_seed(B * 100 + T + hd)
    cos, sin = _cos_sin(B, T, hd, dtype, dev, g)

    def make(H):
        x = torch.randn(B, T, H * hd, generator=g).to(dtype).to(dev)
        if layout == "projection-view":            # what LlamaAttention hands over: a transposed view of [B, T, H*hd]
            return x.requires_grad_(True), lambda t: t.view(B, T, H, hd).transpose(1, 2)
        x = x.view(B, T, H, hd).transpose(1, 2).contiguous()
        return x.requires_grad_(True), lambda t: t

    (q0, vq), (k0, vk) = make(Hq), make(Hk)
    q1, k1 = q0.detach().clone().requires_grad_(True), k0.detach().clone().requires_grad_(True)
    up_q = torch.randn(B, Hq, T, hd, generator=g).to(dtype).to(dev)
    up_k = torch.randn(B, T, Hk, hd, generator=g).to(dtype).to(dev).transpose(1, 2)      # a strided upstream gradient
    qe, ke = _hf_rope()(vq(q0), vk(k0), cos, sin)
    torch.autograd.backward([qe, ke], [up_q, up_k])
    assert tower_ops.rope_supported(vq(q1), vk(k1), cos, sin)
    qh, kh = tower_ops.rope_qk(vq(q1), vk(k1), cos, sin)
    torch.autograd.backward([qh, kh], [up_q, up_k])
    assert torch.equal(qh, qe) and torch.equal(kh, ke)
    assert torch.equal(q1.grad, q0.grad) and torch.equal(k1.grad, k0.grad)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shape", [(4608, 11008), (3, 7, 33), (1, 5), (2, 8192 + 3)])
def test_swiglu_kernel_vs_eager_chain(dev, shape, dtype):
    from dalm_amd.models import tower_ops

    g = torch.Generator().manual_seed(sum(shape))
    gate = (torch.randn(shape, generator=g) * 3).to(dtype).to(dev)
    up = torch.randn(shape, generator=g).to(dtype).to(dev)
    d_act = torch.randn(shape, generator=g).to(dtype).to(dev)
    g0, u0 = gate.clone().requires_grad_(True), up.clone().requires_grad_(True)
    g1, u1 = gate.clone().requires_grad_(True), up.clone().requires_grad_(True)
    ref = torch.nn.functional.silu(g0) * u0
    ref.backward(d_act)
    out = tower_ops.swiglu(g1, u1)
    out.backward(d_act)
    for name, a, b in (("act", out, ref), ("d_gate", g1.grad, g0.grad), ("d_up", u1.grad, u0.grad)):
        a, b = a.detach().float(), b.detach().float()
        if dtype == torch.float32:
            torch.testing.assert_close(a, b, rtol=2e-6, atol=1e-7, msg=lambda m: f"{name}: {m}")
            continue
        diff = (a - b).abs()
        ulp = b.abs().clamp_min(1e-30) * 2.0 ** -7                 # one bf16 ulp is at most 2^-7 of the value
        assert bool((diff <= ulp).all()), f"{name}: more than one bf16 ulp apart (max {float(diff.max())})"
        frac = float((diff > 0).float().mean())
        assert frac < 1e-3, f"{name}: {frac:.2e} of the elements differ from the eager chain"


NORM_CASES = [(R, D, dt) for dt in (torch.bfloat16, torch.float32)
              for R, D in [(4608, 4096), (7, 4096), (33, 1024), (5, 8192), (9, 40), (3, 4544)]
              if not (dt == torch.float32 and D > 4096)]          # f32 rows are supported up to 4096 elements
# the launcher's chunk ladder (1, 2, 4, 8, 16 chunks of 64 lanes x 16 bytes per row; bf16 rows of up to 8 chunks take the second
# backward form): the arms the list above leaves out, and both sides of every edge.  Chunks: bf16 3 (the last one partly filled),
# 4, 5; f32 2, 3, 5, 8 (the last one partly filled), 9
NORM_CASES += [(5, 1536, torch.bfloat16), (5, 2048, torch.bfloat16), (5, 2056, torch.bfloat16),
               (5, 384, torch.float32), (5, 520, torch.float32), (5, 1028, torch.float32), (5, 1800, torch.float32),
               (5, 2052, torch.float32)]


@pytest.mark.parametrize("R,D,dtype", NORM_CASES)
@pytest.mark.parametrize("with_add", [False, True])
def test_rms_norm_kernels_vs_llama_rms_norm(dev, R, D, dtype, with_add):
    """forward against transformers' LlamaRMSNorm (and the eager residual add in front of it): the same two roundings, so equal
    up to the f32 summation order of mean(x^2) - at most one bf16 ulp on a vanishing fraction of elements; backward (dx, with
    the residual-path gradient folded in) against autograd through a float64 copy of the same chain."""
    from transformers.models.llama.modeling_llama import LlamaRMSNorm

    from dalm_amd.models import tower_ops

    g = torch.Generator().manual_seed(R + D)
    x = torch.randn(R, D, generator=g).to(dtype).to(dev)
    delta = torch.randn(R, D, generator=g).to(dtype).to(dev) if with_add else None
    norm = LlamaRMSNorm(D, eps=1e-5).to(dev)
    with torch.no_grad():
        norm.weight.copy_(1 + 0.1 * torch.randn(D, generator=g))
    norm = norm.to(dtype)
    up_h = torch.randn(R, D, generator=g).to(dtype).to(dev)
    up_y = torch.randn(R, D, generator=g).to(dtype).to(dev)
    assert tower_ops.rms_norm_supported(x, norm.weight)
    x1 = x.clone().requires_grad_(True)
    d1 = delta.clone().requires_grad_(True) if with_add else None
    h1, y1 = tower_ops.add_rms_norm(x1, d1, norm.weight, 1e-5)
    torch.autograd.backward([h1, y1], [up_h, up_y])
    # eager chain in the tensor dtype: forward values
    with torch.no_grad():
        h0 = x + delta if with_add else x
        y0 = norm(h0)
    assert torch.equal(h1.detach(), h0)
    diff = (y1.detach().float() - y0.float()).abs()
    if dtype == torch.float32:
        torch.testing.assert_close(y1.detach(), y0, rtol=2e-6, atol=1e-6)
    else:
        # a last-bit difference of rstd can move the inner rounding by one ulp; the weight (|w| ~ 1.1) and the outer rounding can
        # turn that into two
        worst = float((diff / (y0.float().abs() + 1e-30)).max())
        assert worst <= 2.0 ** -6, f"more than two bf16 ulps apart ({worst:.3e} relative)"
        assert float((diff > 0).float().mean()) < 2e-3
    # float64 chain: gradients
    x64 = x.double().requires_grad_(True)
    d64 = delta.double().requires_grad_(True) if with_add else None
    h64 = x64 + d64 if with_add else x64
    y64 = norm.weight.double() * (h64 * torch.rsqrt(h64.pow(2).mean(-1, keepdim=True) + 1e-5))
    torch.autograd.backward([h64, y64], [up_h.double(), up_y.double()])
    tol = 2e-6 if dtype == torch.float32 else 4e-3
    rel = lambda a, b: float((a.double() - b).norm() / b.norm())
    assert rel(x1.grad, x64.grad) < tol
    if with_add:
        assert rel(d1.grad, d64.grad) < tol


def _record_measured(key, values):
    import json
    from pathlib import Path

    try:
        path = Path(__file__).resolve().parent.parent / "gpurun_out" / "measured_tolerances.json"
        path.parent.mkdir(exist_ok=True)
        cur = json.loads(path.read_text()) if path.exists() else {}
        cur[key] = values
        path.write_text(json.dumps(cur, indent=1))
    except OSError:
        pass


def test_patched_llama_layer_matches_transformers(dev):
    """A 2-layer Llama (head_dim 128) with the rotary and SwiGLU kernels patched in against the unpatched module: logits and
    every parameter gradient, bf16 autocast and fp32."""
    from transformers import LlamaConfig, LlamaForCausalLM

    from dalm_amd.models import fastpath

    cfg = LlamaConfig(hidden_size=256, intermediate_size=704, num_hidden_layers=2, num_attention_heads=2,
                      num_key_value_heads=2, vocab_size=300, attention_dropout=0.0, pad_token_id=0)
    torch.manual_seed(0)
    ref = LlamaForCausalLM(cfg).to(dev)
    new = LlamaForCausalLM(cfg).to(dev)
    new.load_state_dict(ref.state_dict())
    assert fastpath.use_swiglu_kernel(new) == 2
    assert fastpath.use_fused_residual_norm(new) == 2
    ids = torch.randint(1, 300, (3, 17), device=dev)
    mask = torch.ones_like(ids)
    mask[1, :5] = 0
    import transformers.models.llama.modeling_llama as m

    for autocast in (False, True):
        outs = []
        for model, patched in ((ref, False), (new, True)):
            if patched:
                assert fastpath.use_roll_rope(model)
            else:
                m.apply_rotary_pos_emb = getattr(m, "_dalm_orig_apply_rotary_pos_emb", m.apply_rotary_pos_emb)
            model.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                logits = model(input_ids=ids, attention_mask=mask).logits
            logits.float().square().mean().backward()
            outs.append((logits.detach().float(), {n: p.grad.detach().float() for n, p in model.named_parameters()}))
        (l0, g0), (l1, g1) = outs
        worst = max(float((g1[n] - g0[n]).norm()) / (float(g0[n].norm()) + 1e-12) for n in g0)
        _record_measured("llama_layer:" + ("bf16-autocast" if autocast else "fp32"),
                         {"logits_rel": float((l1 - l0).norm() / l0.norm()), "logits_max_abs": float((l1 - l0).abs().max()),
                          "logits_max": float(l0.abs().max()), "worst_grad_rel": worst})
        # measured on the MI355X (profiles/r05_measured_tolerances.json): bf16 autocast - logits IDENTICAL, worst gradient 7.6e-8
        # (the kernels round where the eager chains round); fp32 - logits 8.3e-7 absolute, worst gradient 9.4e-7 (summation
        # order of mean(x^2)).  Bounds = 5 x measured (one bf16 ulp of the largest logit where 0 was measured).
        if autocast:
            assert float((l1 - l0).abs().max()) <= 2.0 ** -8 * float(l0.abs().max())
        else:
            torch.testing.assert_close(l1, l0, rtol=0, atol=4.2e-6)
        for n in g0:
            num = float((g1[n] - g0[n]).norm())
            den = float(g0[n].norm()) + 1e-12
            assert num / den < (4e-7 if autocast else 4.7e-6), f"{n}: relative gradient error {num / den:.2e}"
