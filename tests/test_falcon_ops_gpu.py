"""`dalm_layer_norm_{fwd,bwd}`, `dalm_gelu_{fwd,bwd}`, `dalm_add3` (dalm_amd/csrc/falcon.hip) against the eager chains of
transformers' FalconDecoderLayer / FalconMLP they stand in for (the reference reaches them through self.generator_model(...),
dalm/models/rag_e2e_base_model.py:104-106; BASELINE.json config 5):

* add3 and GELU forward/backward: EQUAL to torch's bf16 kernels (same f32 arithmetic, one rounding) - a handful of GELU
  elements may differ by one bf16 ulp where erff and torch's erf disagree in the last f32 bit; bounded and counted;
* LayerNorm: against a float64 evaluation, no further from it than torch's autocast chain (f32 LayerNorm + casts) is;
* a patched depth-1 Falcon-7B-shaped layer (width 256 and the real 4544) against transformers' own forward under bf16
  autocast: output and every gradient."""
import copy
import os

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


@pytest.mark.parametrize("n", [8, 4096, 4608 * 4544, 1000 * 8 + 8])
def test_add3_equals_the_eager_pair_of_adds(dev, n):
    from dalm_amd.models import tower_ops

    g = torch.Generator().manual_seed(n)
    a, b, c = [torch.randn(n, generator=g).bfloat16().to(dev).requires_grad_(True) for _ in range(3)]
    out = tower_ops.add3(a, b, c)
    want = a.detach().clone()
    want += b.detach()
    want = c.detach() + want
    assert torch.equal(out, want)
    go = torch.randn(n, generator=g).bfloat16().to(dev)
    out.backward(go)
    assert torch.equal(a.grad, go) and torch.equal(b.grad, go) and torch.equal(c.grad, go)


@pytest.mark.parametrize("shape", [(3, 8), (4608, 18176), (17, 1000)])
def test_gelu_matches_torch_bf16(dev, shape):
    from dalm_amd.models import tower_ops

    g = torch.Generator().manual_seed(shape[0])
    x = (2.5 * torch.randn(*shape, generator=g)).bfloat16().to(dev)
    x.view(-1)[:8] = torch.tensor([0.0, -0.0, 10.0, -10.0, 40.0, -40.0, 1e-3, -1e-3], dtype=torch.bfloat16)
    go = torch.randn(*shape, generator=g).bfloat16().to(dev)
    xk, xe = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    yk = tower_ops.gelu(xk)
    ye = torch.nn.functional.gelu(xe)
    yk.backward(go)
    ye.backward(go)
    x64 = x.double().requires_grad_(True)
    y64 = torch.nn.functional.gelu(x64)
    y64.backward(go.double())
    for got, eager, ref in ((yk, ye, y64), (xk.grad, xe.grad, x64.grad)):
        diff = (got.float() - eager.float()).abs()
        n_diff = int((diff > 0).sum())
        assert n_diff <= max(2, got.numel() // 2000), n_diff                      # measured: 0 .. a few per million
        # where they differ, by one bf16 ulp of the value, and the kernel is as close to float64 as torch is
        assert float((diff / eager.float().abs().clamp_min(1e-30))[diff > 0].max() if n_diff else 0.0) <= 2 ** -7
        assert _rel(got, ref) <= 1.02 * _rel(eager, ref) + 1e-7
    assert torch.isfinite(yk).all() and torch.isfinite(xk.grad).all()


@pytest.mark.parametrize("R,D,bias", [(5, 8, True), (130, 256, True), (4608, 4544, True), (333, 1024, False), (64, 8192, True),
                                      (77, 4544 - 8, True),
                                      # the launcher's ladder of 1, 2, 4, 6, 8, 9, 12, 16 chunks of 512 elements: every arm the
                                      # shapes above leave out, on both sides of every edge (3, 4, 5, 6, 7, 8, 10, 12, 13 chunks)
                                      (5, 1032, True), (5, 2048, False), (5, 2056, True), (5, 3072, True), (5, 3080, False),
                                      (5, 4096, True), (5, 4616, True), (5, 6144, False), (5, 6152, True)])
def test_layer_norm_vs_fp64_and_the_autocast_chain(dev, R, D, bias):
    from dalm_amd.models import tower_ops

    g = torch.Generator().manual_seed(R + D)
    x = (torch.randn(R, D, generator=g) * 1.5 + 0.3).bfloat16().to(dev)
    w = (1.0 + 0.2 * torch.randn(D, generator=g)).bfloat16().to(dev)
    b = (0.1 * torch.randn(D, generator=g)).bfloat16().to(dev) if bias else None
    gy = torch.randn(R, D, generator=g).bfloat16().to(dev)
    gres = torch.randn(R, D, generator=g).bfloat16().to(dev)
    eps = 1e-5

    xk = x.clone().requires_grad_(True)
    res, yk = tower_ops.layer_norm_res(xk, w, b, eps)
    assert yk.dtype == torch.bfloat16 and res.data_ptr() == xk.data_ptr()
    torch.autograd.backward([res, yk], [gres, gy])

    xe = x.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        ye32 = torch.nn.functional.layer_norm(xe, (D,), w, b, eps)
        assert ye32.dtype == torch.float32
    ye = ye32.to(torch.bfloat16)                                    # what the two Linear consumers read
    torch.autograd.backward([xe, ye], [gres, gy])

    x64 = x.double().requires_grad_(True)
    y64 = torch.nn.functional.layer_norm(x64, (D,), w.double(), b.double() if bias else None, eps)
    torch.autograd.backward([x64, y64], [gres.double(), gy.double()])

    e_k, e_e = _rel(yk, y64), _rel(ye, y64)
    assert e_k <= 1.02 * e_e + 1e-6, (e_k, e_e)
    assert float((yk.float() - ye.float()).abs().max()) <= 2 ** -7 * float(ye.float().abs().max())
    g_k, g_e = _rel(xk.grad, x64.grad), _rel(xe.grad, x64.grad)
    assert g_k <= 1.02 * g_e + 1e-6, (g_k, g_e)
    # the kernel without the residual gradient
    xk2 = x.clone().requires_grad_(True)
    _, y2 = tower_ops.layer_norm_res(xk2, w, b, eps)
    y2.backward(gy)
    x64b = x.double().requires_grad_(True)
    torch.nn.functional.layer_norm(x64b, (D,), w.double(), b.double() if bias else None, eps).backward(gy.double())
    assert _rel(xk2.grad, x64b.grad) < 4e-3
    assert torch.equal(y2, yk)


def test_layer_norm_weight_and_bias_gradients(dev):
    from dalm_amd.models import tower_ops

    g = torch.Generator().manual_seed(4)
    R, D = 96, 512
    x = torch.randn(R, D, generator=g).bfloat16().to(dev)
    w = (1.0 + 0.2 * torch.randn(D, generator=g)).bfloat16().to(dev).requires_grad_(True)
    b = (0.1 * torch.randn(D, generator=g)).bfloat16().to(dev).requires_grad_(True)
    gy = torch.randn(R, D, generator=g).bfloat16().to(dev)
    _, y = tower_ops.layer_norm_res(x.clone().requires_grad_(True), w, b, 1e-5)
    y.backward(gy)
    w64, b64 = w.detach().double().requires_grad_(True), b.detach().double().requires_grad_(True)
    torch.nn.functional.layer_norm(x.double(), (D,), w64, b64, 1e-5).backward(gy.double())
    assert _rel(w.grad, w64.grad) < 5e-3 and _rel(b.grad, b64.grad) < 5e-3


def _falcon_layer(width, heads, dev, seed):
    from transformers import FalconConfig
    from transformers.models.falcon.modeling_falcon import FalconModel

    cfg = FalconConfig(vocab_size=512, hidden_size=width, num_hidden_layers=1, num_attention_heads=heads, multi_query=True,
                       parallel_attn=True, new_decoder_architecture=False, bias=False, alibi=False, hidden_dropout=0.0,
                       attention_dropout=0.0)
    cfg._attn_implementation = "sdpa"
    torch.manual_seed(seed)
    m = FalconModel(cfg)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.LayerNorm):
                mod.weight.add_(0.1 * torch.randn_like(mod.weight))
                mod.bias.add_(0.1 * torch.randn_like(mod.bias))
    return m.to(dev).to(torch.bfloat16)


@pytest.mark.parametrize("width,heads,T", [(256, 4, 40), (4544, 71, 64)])
def test_patched_falcon_layer_against_transformers(dev, width, heads, T):
    from dalm_amd.models import fastpath

    ref = _falcon_layer(width, heads, dev, 3)
    fast = copy.deepcopy(ref)
    assert fastpath.use_falcon_layer_kernels(fast) == 1
    layer = fast.h[0]
    assert layer.forward.__func__ is fastpath._falcon_layer_forward
    assert layer.mlp.forward.__func__ is fastpath._falcon_mlp_forward
    g = torch.Generator().manual_seed(width)
    B = 3
    ids = torch.randint(0, 512, (B, T), generator=g).to(dev)
    mask = torch.ones(B, T, dtype=torch.long)
    mask[1, : T // 3] = 0
    mask = mask.to(dev)
    emb_r = ref.word_embeddings.weight
    outs = []
    for m in (ref, fast):
        m.train()
        for p in m.parameters():
            p.requires_grad_(False)
        e = m.word_embeddings(ids).detach().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            h = m(inputs_embeds=e, attention_mask=mask).last_hidden_state
        (h.float() * torch.linspace(-1, 1, h.shape[-1], device=dev)).sum().backward()
        outs.append((h.detach(), e.grad.detach()))
    (h_r, g_r), (h_f, g_f) = outs
    live = mask.bool()
    assert _rel(h_f[live], h_r[live]) < 6e-3, _rel(h_f[live], h_r[live])
    assert _rel(g_f[live], g_r[live]) < 1.2e-2, _rel(g_f[live], g_r[live])
    # DALM_FALCON_KERNELS=0 leaves transformers' code in place
    os.environ["DALM_FALCON_KERNELS"] = "0"
    try:
        assert fastpath.use_falcon_layer_kernels(copy.deepcopy(ref)) == 0
    finally:
        os.environ.pop("DALM_FALCON_KERNELS", None)
