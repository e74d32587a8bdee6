"""Arcee (AFM) on the GPU.

Row-wise kernels: `dalm_relu2_fwd` / `dalm_relu2_bwd` (dalm_amd/csrc/tower.hip) against torch's own eager chain
`torch.square(F.relu(y))` and its autograd backward on the same tensors: EQUAL values (torch.equal on the non-NaN elements) and NaN in
the same places - one rounding each way, nothing to tolerate.  Dead input rows hold NaN and must not be read; outputs there are zeros.

Up GEMM: `dalm_linear_live_relu2` (dalm_amd/csrc/linear_live.hip) against `dalm_linear_live` followed by `dalm_relu2_fwd`, run in the
same process (those are checked on their own above and in test_linear_live_gpu.py): same contraction order, same element arithmetic
(csrc/relu2_math.hpp) - live rows EQUAL bit for bit, dead rows, guard rows and pad columns keep their sentinel.

Node: `_FrozenRelu2MlpFn` against the separate nodes (`linear_live.set_mlp_fused(False)`): output and dx bit-identical, at H 128 and
300 rows.  The width first asked for, C = 264, cannot be run: C is also the contraction depth of the down GEMM, and `dalm_linear_live`
takes K % 64 == 0 only, so such an MLP never routes (asserted below) - the node runs at C = 320 instead: % 64 == 0, one full
256-column tile and a partial one, as 264 would have had.

Step: the tiny model of tests/test_arcee_cpu.py with LoRA on q / v in bf16, routed (`use_generator_fast_paths`) against unrouted
(transformers' own code; the `DALM_*=0` switches leave a model in that state, asserted first), padded and packed.  The bound is the
one tests/test_qwen3_gpu.py and tests/test_gemma_gpu.py hold this comparison to: E_ref is the largest absolute error of the unrouted
bf16 model against the unrouted float32 model on the same weights; the routed path's error against that truth is at most 2 E_ref,
per tensor (the logits / hidden states a loss reads, and every LoRA gradient).  One case runs YaRN rotary scaling.
A RAG step packed against padded is held to tests/test_packed_gpu.py's bounds (stated in that test's docstring)."""
import copy
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SENT = 7.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from dalm_amd import hip

    hip.load()
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ---- the row-wise kernels -----------------------------------------------------------------------------------------------------
Y_SPECIAL = [0.0, -0.0, -1.5, 1e-40, -1e-40, 3e38, 1e20, float("inf"), float("-inf"), float("nan"), 2.5]
D_SPECIAL = [0.0, float("inf"), float("-inf"), float("nan"), 3e38, 1e-40, -2.0]      # 11 and 7 are coprime: every pair meets

_ROWWISE = {}


def _rowwise_case(R, C, dtype, dev):
    """(y, d_act, eager act, autograd d_y) on the device, computed ONCE per case and left unchanged: +-0, negatives, subnormals, values
    whose square overflows, +-inf and NaN at every second element, each y special against each d_act special."""
    key = (R, C, dtype)
    if key not in _ROWWISE:
        g = torch.Generator().manual_seed(1000 * R + C)
        n = R * C
        y = (2.0 * torch.randn(n, generator=g)).float()
        d = torch.randn(n, generator=g).float()
        j = torch.arange((n + 1) // 2)
        y[0::2] = torch.tensor(Y_SPECIAL)[j % len(Y_SPECIAL)]
        d[0::2] = torch.tensor(D_SPECIAL)[j % len(D_SPECIAL)]
        y, d = y.view(R, C).to(dev, dtype), d.view(R, C).to(dev, dtype)
        leaf = y.clone().requires_grad_(True)
        act = torch.square(F.relu(leaf))
        act.backward(d)
        torch.cuda.synchronize()
        _ROWWISE[key] = (y, d, act.detach(), leaf.grad.detach())
    return _ROWWISE[key]


def _vectors(R, dev):
    g = torch.Generator().manual_seed(31 + R)
    mixed = (torch.rand(R, generator=g) < 0.6).to(torch.uint8)
    one = torch.zeros(R, dtype=torch.uint8)
    one[R // 2] = 1
    return (("none", None), ("all dead", torch.zeros(R, dtype=torch.uint8, device=dev)), ("mixed", mixed.to(dev)), ("one live", one.to(dev)))


def _laid_out(t, ld, fill, vec=None):
    """`t` [R, C] inside a fresh [R, ld] buffer filled with `fill`; dead rows of the copy poisoned with NaN."""
    R, C = t.shape
    buf = torch.full((R, ld), fill, dtype=t.dtype, device=t.device)
    view = buf[:, :C]
    view.copy_(t)
    if vec is not None:
        view[vec == 0] = float("nan")
    return buf, view


def _same(tag, got, want):
    nan_g, nan_w = torch.isnan(got), torch.isnan(want)
    assert torch.equal(nan_g, nan_w), f"{tag}: NaN in other places ({int(nan_g.sum())} against {int(nan_w.sum())})"
    ok = ~nan_w
    assert torch.equal(got[ok], want[ok]), f"{tag}: {int((got[ok] != want[ok]).sum())} of {int(ok.sum())} values differ"


@pytest.mark.parametrize("C", [8, 136, 2056])            # one vector / rows that are no multiple of a tile / tiles that straddle rows
@pytest.mark.parametrize("R", [1, 37, 300])              # 300 x 2056: more than one workgroup and more than one trip per thread
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_row_wise_kernels_equal_eager_and_autograd(dev, dtype, R, C):
    from dalm_amd import hip

    y0, d0, act_ref, dy_ref = _rowwise_case(R, C, dtype, dev)
    code = hip.dtype_code(y0)
    for ld in (C, C + 8):
        for name, vec in _vectors(R, dev):
            tag = f"{dtype} R={R} C={C} ld={ld} {name}"
            live = torch.ones(R, dtype=torch.bool, device=dev) if vec is None else vec != 0
            ybuf, y = _laid_out(y0, ld, float("nan"), vec)
            dbuf, d = _laid_out(d0, ld, float("nan"), vec)
            abuf, act = _laid_out(torch.full_like(y0, SENT), ld, SENT)
            gbuf, dy = _laid_out(torch.full_like(y0, SENT), ld, SENT)
            hip.call("dalm_relu2_fwd", hip.ptr(y), hip.ptr(act), code, R, C, ld, ld, hip.ptr(vec), hip.stream())
            hip.call("dalm_relu2_bwd", hip.ptr(d), hip.ptr(y), hip.ptr(dy), code, R, C, ld, ld, ld, hip.ptr(vec), hip.stream())
            torch.cuda.synchronize()
            _same(tag + " forward", act[live], act_ref[live])
            _same(tag + " backward", dy[live], dy_ref[live])
            for out in (act, dy):                        # a dead row: nothing read (the inputs there are NaN), zeros written
                assert bool((_bits(out[~live]) == 0).all()), f"{tag}: dead rows are not zeros"
            for buf in (abuf, gbuf):                     # pad columns of a strided output are not touched
                assert bool((buf[:, C:] == SENT).all()), f"{tag}: pad columns written"


def test_autograd_wrapper_equals_the_eager_chain(dev):
    """`tower_ops.relu2`: a [B, T, C] tensor and a row-strided 2-D view (read in place), with and without a tower call's vector."""
    from dalm_amd import live_rows
    from dalm_amd.models import tower_ops

    B, T, C = 3, 20, 136
    y0, d0, _, _ = _rowwise_case(300, 136, torch.bfloat16, dev)
    y0, d0 = y0[:B * T].reshape(B, T, C), d0[:B * T].reshape(B, T, C)
    leaf = y0.clone().requires_grad_(True)
    torch.square(F.relu(leaf)).backward(d0)
    for shape in ("3d", "strided"):
        x = y0.clone().requires_grad_(True)
        if shape == "strided":
            wide = torch.full((B * T, C + 8), float("nan"), dtype=y0.dtype, device=dev)
            wide[:, :C] = y0.reshape(B * T, C)
            x = wide.requires_grad_(True)
            y_in = x[:, :C]
        else:
            y_in = x
        assert tower_ops.relu2_supported(y_in)
        act = tower_ops.relu2(y_in)
        act.backward(d0.reshape(act.shape))
        _same(shape + " forward", act.detach().reshape(B, T, C), torch.square(F.relu(y0)))
        got = x.grad[:, :C].reshape(B, T, C) if shape == "strided" else x.grad
        _same(shape + " backward", got, leaf.grad)
    mask = torch.ones(B, T, dtype=torch.long, device=dev)
    mask[0, :7] = 0
    mask[2, :19] = 0
    x = y0.clone().requires_grad_(True)
    with live_rows.tower_call(mask, shifted=True) as vec:
        act = tower_ops.relu2(x)
    act.backward(d0)                                     # after the context: the node kept the vector
    live = (vec != 0).view(B, T)
    assert 0 < int(live.sum()) < B * T
    _same("live forward", act.detach()[live], torch.square(F.relu(y0))[live])
    _same("live backward", x.grad[live], leaf.grad[live])
    assert bool((act.detach()[~live] == 0).all()) and bool((x.grad[~live] == 0).all())
    assert not tower_ops.relu2_supported(y0.cpu()) and not tower_ops.relu2_supported(y0[..., :5])


# ---- ReLU^2 inside the epilogue of the live-row up GEMM --------------------------------------------------------------------------
R = 300                                                  # one full 256-row tile and a partial one
GUARD = 3
_GEMM_IN = {}


def _gemm_inputs(C, K, dev):
    if (C, K) not in _GEMM_IN:
        g = torch.Generator().manual_seed(100 * C + K)
        a = torch.randn(R, K, generator=g).bfloat16()
        w = (2.0 * torch.randn(C, K, generator=g) / math.sqrt(K)).bfloat16()
        _GEMM_IN[(C, K)] = (a.to(dev), w.to(dev))
    return _GEMM_IN[(C, K)]


def _gemm_masks(dev):
    g = torch.Generator().manual_seed(977)
    mixed = (torch.rand(R, generator=g) < 0.5).to(torch.uint8)
    one = torch.zeros(R, dtype=torch.uint8)
    one[271] = 1                                         # in the second row tile
    return (("none live", torch.zeros(R, dtype=torch.uint8)), ("all live", torch.ones(R, dtype=torch.uint8)), ("one live", one),
            ("mixed", mixed))


def _guarded(C, dev):
    """[GUARD + R + GUARD, C + 8] of the sentinel; the [R, C] view the kernel writes (row stride C + 8)."""
    buf = torch.full((R + 2 * GUARD, C + 8), SENT, dtype=torch.bfloat16, device=dev)
    return buf, buf[GUARD:GUARD + R, :C]


def _assert_untouched(buf, view, keep, C, tag):
    assert bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + R:] == SENT).all()), f"{tag}: guard rows written"
    assert bool((buf[:, C:] == SENT).all()), f"{tag}: pad columns written"
    assert bool((view[~keep] == SENT).all()), f"{tag}: dead rows written"


def _fused(a, w, C, K, part, dev):
    from dalm_amd import hip

    ybuf, y = _guarded(C, dev)
    abuf, act = _guarded(C, dev)
    hip.call("dalm_linear_live_relu2", hip.ptr(a), a.stride(0), hip.ptr(w), hip.ptr(y), y.stride(0), hip.ptr(act), act.stride(0), R, C, K,
             hip.ptr(part[0]), hip.ptr(part[1]), hip.stream())
    return ybuf, y, abuf, act


def _relu2_ref(y, vec):
    from dalm_amd import hip

    C = y.shape[1]
    act = torch.full((R, C), SENT, dtype=torch.bfloat16, device=y.device)
    hip.call("dalm_relu2_fwd", hip.ptr(y), hip.ptr(act), hip.dtype_code(y), R, C, y.stride(0), C, hip.ptr(vec), hip.stream())
    return act


@pytest.mark.parametrize("K", [64, 192])                 # the single-K-tile path / an odd number of K tiles
@pytest.mark.parametrize("C", [8, 256, 264, 520])        # a partial tile / one tile / one column vector past a tile edge / two tiles + 8
def test_up_gemm_with_relu2_equals_the_unfused_pair(dev, C, K):
    from dalm_amd import linear_live

    a0, w = _gemm_inputs(C, K, dev)
    for name, vec in _gemm_masks(dev):
        vec = vec.to(dev)
        tag = f"C={C} K={K} {name}"
        keep = vec != 0
        a = a0.clone()
        a[~keep] = float("nan")                          # nothing of a dead row is read
        part = linear_live.row_partition(vec)
        y_ref = linear_live.linear_live(a, w, part)
        act_ref = _relu2_ref(y_ref, vec)
        ybuf, y, abuf, act = _fused(a, w, C, K, part, dev)
        torch.cuda.synchronize()
        assert torch.equal(_bits(y[keep]), _bits(y_ref[keep])), f"{tag}: y differs from dalm_linear_live"
        assert torch.equal(_bits(act[keep]), _bits(act_ref[keep])), f"{tag}: act differs from dalm_relu2_fwd"
        assert torch.isfinite(y[keep].float()).all() and torch.isfinite(act[keep].float()).all(), f"{tag}: NaN leaked in"
        if int(keep.sum()) > 1:
            assert bool((act[keep] > 0).any()) and bool((act[keep] == 0).any()), f"{tag}: the case shows neither side of the relu"
        _assert_untouched(ybuf, y, keep, C, tag + " (y)")
        _assert_untouched(abuf, act, keep, C, tag + " (act)")


def test_wrapper_returns_the_same_bits(dev):
    from dalm_amd import linear_live

    C, K = 520, 192
    a0, w = _gemm_inputs(C, K, dev)
    vec = _gemm_masks(dev)[3][1].to(dev)
    keep = vec != 0
    part = linear_live.row_partition(vec)
    before = linear_live.calls()
    y, act = linear_live.linear_live_relu2(a0, w, part)
    assert linear_live.calls() == before + 1
    y_ref = linear_live.linear_live(a0, w, part)
    assert torch.equal(_bits(y[keep]), _bits(y_ref[keep]))
    assert torch.equal(_bits(act[keep]), _bits(_relu2_ref(y_ref, vec)[keep]))


def test_a_corrupt_partition_stores_nothing_out_of_bounds(dev):
    """perm entries outside [0, R) select nothing: only the rows a valid entry names may change; guard rows keep their sentinel."""
    C, K = 520, 192
    a, w = _gemm_inputs(C, K, dev)
    g = torch.Generator().manual_seed(11)
    perm = torch.randperm(R, generator=g).to(torch.int32)
    bad = torch.tensor([-1, R, R + 1, R + GUARD, 2 ** 31 - 1, -2 ** 31, -R, 1 << 20], dtype=torch.int32)
    where = torch.randperm(R, generator=g)[:64]
    perm[where] = bad.repeat(8)
    named = torch.zeros(R, dtype=torch.bool)
    ok = (perm >= 0) & (perm < R)
    named[perm[ok].long()] = True
    named = named.to(dev)
    part = (perm.to(dev), torch.tensor([R], dtype=torch.int32, device=dev))
    ybuf, y, abuf, act = _fused(a, w, C, K, part, dev)
    torch.cuda.synchronize()
    _assert_untouched(ybuf, y, named, C, "y")
    _assert_untouched(abuf, act, named, C, "act")
    assert torch.isfinite(y[named].float()).all() and not bool((act[named] == SENT).all())


# ---- the frozen MLP node ---------------------------------------------------------------------------------------------------------
def test_node_equals_the_separate_nodes(dev, monkeypatch):
    from transformers import ArceeConfig
    from transformers.models.arcee.modeling_arcee import ArceeMLP

    from dalm_amd import hip, linear_live, live_rows
    from dalm_amd.models import fastpath, frozen_linear

    H, C, B, T = 128, 320, 3, 100                       # 300 rows
    torch.manual_seed(3)
    mlp = ArceeMLP(ArceeConfig(hidden_size=H, intermediate_size=C, bos_token_id=1, eos_token_id=2)).to(dev).to(torch.bfloat16)
    for p in mlp.parameters():
        p.requires_grad_(False)
    assert frozen_linear.use_transposed_dgrad(mlp) == 2
    mask = torch.ones(B, T, dtype=torch.long, device=dev)
    mask[0, :31] = 0
    mask[2, :77] = 0
    g = torch.Generator().manual_seed(4)
    x0 = torch.randn(B, T, H, generator=g).bfloat16().to(dev)
    g0 = torch.randn(B, T, H, generator=g).bfloat16().to(dev)
    calls, real_call = [], hip.call
    monkeypatch.setattr(hip, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])

    def run(fused):
        linear_live.set_table([(B * T, C, H), (B * T, H, C)])
        linear_live.set_enabled(True)
        linear_live.set_mlp_fused(fused)
        calls.clear()
        try:
            with live_rows.tower_call(mask, shifted=True) as vec:
                x = x0.clone()
                x.view(B * T, H)[vec == 0] = float("nan")            # nothing of a dead row is read, by either arm
                x.requires_grad_(True)
                out = fastpath._relu2_mlp_forward(mlp, x)
            gg = g0.clone()
            gg.view(B * T, H)[vec == 0] = float("nan")
            (dx,) = torch.autograd.grad(out, x, gg)
            torch.cuda.synchronize()
        finally:
            linear_live.set_table(None)
            linear_live.set_mlp_fused(True)
        return out.detach(), dx, (vec != 0).view(B, T), list(calls)

    out_f, dx_f, live, calls_f = run(True)
    out_s, dx_s, _, calls_s = run(False)
    assert 0 < int(live.sum()) < B * T
    # the node: one fused up launch, the down forward, down dgrad and up dgrad as live-row GEMMs, one row-wise backward launch
    assert calls_f.count("dalm_linear_live_relu2") == 1 and calls_f.count("dalm_linear_live") == 3, calls_f
    assert calls_f.count("dalm_relu2_bwd") == 1 and "dalm_relu2_fwd" not in calls_f, calls_f
    # `set_mlp_fused(False)` restores the separate nodes: the same GEMMs one by one, the row-wise kernel both ways
    assert "dalm_linear_live_relu2" not in calls_s and calls_s.count("dalm_linear_live") == 4, calls_s
    assert calls_s.count("dalm_relu2_fwd") == 1 and calls_s.count("dalm_relu2_bwd") == 1, calls_s
    assert torch.equal(_bits(out_f), _bits(out_s)) and torch.equal(_bits(dx_f), _bits(dx_s))
    assert torch.isfinite(out_f.float()).all() and torch.isfinite(dx_f.float()).all()
    assert bool((out_f[~live] == 0).all()) and bool((dx_f[~live] == 0).all())
    assert float(out_f[live].float().abs().max()) > 0 and float(dx_f[live].float().abs().max()) > 0
    # and against the module's own formula on the live rows: the same function, another GEMM kernel's summation order
    x = x0.clone().requires_grad_(True)
    want = mlp.down_proj(torch.square(F.relu(mlp.up_proj(x))))
    (dx_w,) = torch.autograd.grad(want, x, g0)
    for got, ref in ((out_f, want.detach()), (dx_f, dx_w)):
        err = float((got[live].float() - ref[live].float()).abs().max())
        assert err <= 2.0 ** -6 * float(ref[live].float().abs().max()), err      # a few bf16 ulps of the largest entry
    # C = 264: the down GEMM would contract over 264, no multiple of 64 - such an MLP never routes
    linear_live.set_table([(B * T, 264, H), (B * T, H, 264)])
    try:
        narrow = [torch.nn.Linear(H, 264, bias=False, device="meta", dtype=torch.bfloat16).requires_grad_(False),
                  torch.nn.Linear(264, H, bias=False, device="meta", dtype=torch.bfloat16).requires_grad_(False)]
        assert frozen_linear.relu2_mlp_candidate(torch.empty(B, T, H, device="meta", dtype=torch.bfloat16), *narrow) is None
    finally:
        linear_live.set_table(None)


# ---- the model -------------------------------------------------------------------------------------------------------------------
def _err(a, truth):
    return float((a.detach().double() - truth.double()).abs().max())


def _held(name, got, ref, truth):
    """The tolerance rule of tests/test_qwen3_gpu.py: the new path's largest absolute error against the truth is at most twice the
    bf16 reference's."""
    e_new, e_ref = _err(got, truth), _err(ref, truth)
    print(f"{name}: new {e_new:.4e} reference {e_ref:.4e} ratio {e_new / max(e_ref, 1e-300):.3f}")
    assert torch.isfinite(got).all(), name
    assert e_new <= 2.0 * e_ref, (name, e_new, e_ref)


_YARN = {"rope_type": "yarn", "factor": 4.0, "original_max_position_embeddings": 16, "rope_theta": 10000.0}


def _tiny(rope=None):
    from transformers import ArceeConfig, ArceeForCausalLM

    torch.manual_seed(0)
    kw = dict(vocab_size=128, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
              num_key_value_heads=2, head_dim=64, max_position_embeddings=64, bos_token_id=1, eos_token_id=2)
    if rope is not None:
        kw["rope_parameters"] = dict(rope)
    m = ArceeForCausalLM(ArceeConfig(**kw))
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p.to(torch.bfloat16).float())              # every copy below holds the SAME (bf16-exact) weights
    return m.train()


def _with_lora(model):
    from dalm_amd.models import lora

    lora.inject_lora(model, ["q_proj", "v_proj"], lora_dropout=0.0)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if "lora_B" in name:                # at its zero initialisation dA is identically zero and proves nothing
                p.copy_((0.05 * torch.randn(p.shape, generator=g)).to(torch.bfloat16).float())
            if "lora_A" in name:
                p.copy_(p.to(torch.bfloat16).float())
    return model


def _cast(model, dev, dtype):
    model = model.to(dev)
    if dtype == torch.bfloat16:
        for p in model.parameters():
            if not p.requires_grad or p.dim() == 1:           # frozen base and the norm weights; the adapters stay f32
                p.data = p.data.to(torch.bfloat16)
    return model.train()


@pytest.mark.parametrize("rope", [None, _YARN], ids=["default-rope", "yarn"])
def test_tiny_model_with_lora_routed_against_unrouted(dev, monkeypatch, rope):
    from dalm_amd import hip, live_rows, packed
    from dalm_amd.models import lora
    from dalm_amd.models.frozen_linear import use_transposed_dgrad
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    base = _tiny(rope)
    if rope is not None:
        assert base.config.rope_parameters["rope_type"] == "yarn" and base.model.rotary_emb.rope_type == "yarn"
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

    def grads(model):
        return {n: p.grad.detach().float().clone() for n, p in model.named_parameters() if p.requires_grad}

    def padded(model, dtype, tower=False):
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16), live_rows.tower_call(am, True, enabled=tower):
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
        from transformers.models.arcee import modeling_arcee          # the rotary swap is process-wide: undone for the references
        mp.setattr(modeling_arcee, "apply_rotary_pos_emb",
                   getattr(modeling_arcee, "_dalm_orig_apply_rotary_pos_emb", modeling_arcee.apply_rotary_pos_emb))
        assert modeling_arcee.apply_rotary_pos_emb.__name__ != "_rope_hip"
        for name in ("DALM_SWIGLU_KERNEL", "DALM_NORM_KERNEL", "DALM_ATTN_KERNEL", "DALM_FAST_ROPE"):
            mp.setenv(name, "0")
        off = use_generator_fast_paths(copy.deepcopy(base))           # what the switches leave of the routing: nothing of Arcee's
        assert not any(off[k] for k in ("use_relu2_kernel", "use_fused_residual_norm", "use_hip_attention_backward",
                                        "use_llama_attention_node", "use_roll_rope")), off
        truth = _cast(_with_lora(copy.deepcopy(base)), dev, torch.float32)
        plain = _cast(_with_lora(copy.deepcopy(base)), dev, torch.bfloat16)
        t_logits, t_grads = padded(truth, torch.float32)
        r_logits, r_grads = padded(plain, torch.bfloat16)
        t_h, t_g = hidden_padded(truth, torch.float32)
        r_h, r_g = hidden_padded(plain, torch.bfloat16)

    fast = copy.deepcopy(base)
    went_in = use_generator_fast_paths(fast)
    assert went_in["use_relu2_kernel"] == 2 and went_in["use_fused_residual_norm"] == 2 and went_in["use_llama_attention_node"] == 2
    assert went_in["use_hip_attention_backward"] and went_in["use_roll_rope"] and packed.attention_is_packable(fast)
    fast = _cast(_with_lora(fast), dev, torch.bfloat16)
    assert use_transposed_dgrad(fast) == 7                              # o_proj, up_proj, down_proj per layer, and the lm_head
    for layer in fast.model.layers:                                    # q | k | v of an Arcee layer form one group, as Llama's
        a = layer.self_attn
        assert a.q_proj._group is not None and a.q_proj._group is a.k_proj._group is a.v_proj._group
        assert len(a.q_proj._group.members) == 3

    calls = []
    real_call = hip.call

    def spy(name, *args):
        calls.append(name)
        return real_call(name, *args)

    monkeypatch.setattr(hip, "call", spy)
    f_logits, f_grads = padded(fast, torch.bfloat16, tower=True)
    assert calls.count("dalm_relu2_fwd") == 2 and calls.count("dalm_relu2_bwd") == 2, calls           # once per layer each way
    assert calls.count("dalm_attn_gqa_fwd") == 2 and calls.count("dalm_attn_gqa_bwd") == 2, calls     # grouped heads, un-expanded
    # Llama's layer forward: two norms per layer; the first one's input is the frozen embedding, autograd skips its backward
    assert calls.count("dalm_rms_norm_fwd_live") == 4 and calls.count("dalm_rms_norm_bwd_live") == 3, calls
    assert calls.count("dalm_rope_qk_live") == 2, calls                      # the node: the rotation forward only, its backward rides in dalm_attn_*_bwd
    assert any(c.startswith("dalm_lora2_") for c in calls), calls                                     # the q | k | v group's kernels
    assert all(l.self_attn.q_proj._group.enabled for l in fast.model.layers)
    assert all(getattr(l.self_attn.q_proj.base_layer, "_dalm_cat", None) is not None for l in fast.model.layers), \
        "q | k | v did not run as one GEMM over one concatenated weight"
    names = set(t_grads)
    assert names == set(r_grads) == set(f_grads) and any("lora_A" in n for n in names) and all("lora_" in n for n in names)
    _held("model padded logits", f_logits, r_logits, t_logits)
    for n in sorted(names):
        _held(f"model padded {n}", f_grads[n], r_grads[n], t_grads[n])

    # packed: the generator's decoder stack on the un-padded rows, against the same rows of the padded truth
    calls.clear()
    fast.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        h = packed.generator_hidden(fast, ids, am, rows, cu)[valid]
    (h.float() * wh).sum().backward()
    assert calls.count("dalm_relu2_fwd") == 2 and calls.count("dalm_relu2_bwd") == 2, calls
    assert calls.count("dalm_attn_gqa_fwd") == 2 and calls.count("dalm_attn_gqa_bwd") == 2, calls
    _held("model packed hidden", h.detach().float()[seen], r_h, t_h)
    f_g = grads(fast)
    for n in sorted(names):
        _held(f"model packed {n}", f_g[n], r_g[n], t_g[n])


# ---- a RAG step -------------------------------------------------------------------------------------------------------------------
_BUILT = {}


def _arcee_lm():
    if "lm" not in _BUILT:
        _BUILT["lm"] = _with_lora(_tiny())
    return copy.deepcopy(_BUILT["lm"])


def _one_step(batch, mode, precision, dev):
    from test_causal_retriever_gpu import _GradSnapshot
    from test_qwen3_gpu import _tiny_bert

    from dalm_amd import hip, packed
    from dalm_amd.models import AutoModelForRagE2E
    from dalm_amd.training.step import RagE2EStep

    model = AutoModelForRagE2E.from_modules(_tiny_bert(), _arcee_lm(), None, None, normalize=True, get_peft=None).to(dev)
    if precision == "bf16":
        for p in model.parameters():
            if not p.requires_grad:
                p.data = p.data.to(torch.bfloat16)
    model.train()
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    opt = torch.optim.SGD([p for _, p in named], lr=0.0)
    snap = _GradSnapshot(named)
    opt.register_step_pre_hook(snap)
    step = RagE2EStep(model, opt, None, 100, autocast_dtype=torch.bfloat16 if precision == "bf16" else None, overlap_towers=True,
                      track_grad_norm=True)
    host = packed.add_pack_plans(batch, packed.RAG_GROUPS) if mode == "packed" else batch
    calls, real_call = [], hip.call
    hip.call = lambda name, *a: (calls.append(name), real_call(name, *a))[1]
    try:
        dbatch = {k: v.to(dev) for k, v in host.items()}
        loss = float(step(dbatch))
    finally:
        hip.call = real_call
    if mode == "packed":
        assert step._packed_generator(dbatch), "the packed generator path did not run"
    return {"loss": loss, "grad_norm": float(step.grad_norm)}, snap.grads, calls


def _rel_norm(a, b):
    return float((a.double() - b.double()).norm()) / max(float(b.double().norm()), 1e-30)


def test_rag_step_with_an_arcee_generator_packed_against_padded(dev):
    """One RAG-e2e step, tiny BERT retriever + tiny Arcee generator, at the bounds tests/test_packed_gpu.py holds the Llama step
    to: fp32 - loss, gradient norm and every gradient within 1e-4; bf16 autocast - loss within 2.5e-4 and gradient norm within
    2.2e-3 of the padded bf16 step, every parameter's gradient within twice the padded bf16 step's own distance from the fp32
    step + 5e-3, and within 4e-2 outright."""
    from test_causal_retriever_gpu import _rag_batch

    batch = _rag_batch(False)
    res = {(m, p): _one_step(batch, m, p, dev) for p in ("fp32", "bf16") for m in ("padded", "packed")}
    for m in ("padded", "packed"):                    # the ReLU^2 kernels ran in both layouts, one launch per layer each way
        for p in ("fp32", "bf16"):
            calls = res[m, p][2]
            assert calls.count("dalm_relu2_fwd") == 2 and calls.count("dalm_relu2_bwd") == 2, (m, p, calls)
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
