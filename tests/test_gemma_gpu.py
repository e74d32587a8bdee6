"""Gemma on the GPU: `dalm_geglu_{fwd,bwd}` and `dalm_gemma_norm_{fwd,bwd}` (dalm_amd/csrc/tower.hip) against the eager chains of
transformers' GemmaMLP / GemmaRMSNorm on the device and against float64; row liveness; a tiny Gemma (head width 64, so the attention
kernels run too) with LoRA, routed by `use_generator_fast_paths` against the unrouted copy, padded and packed; one RAG step with a
Gemma generator, packed against padded.

Standards.  GeGLU (from test_falcon_ops_gpu.py::test_gelu_matches_torch_bf16): rel(kernel, f64) <= 1.02 rel(eager, f64) + 1e-7 for
the output and both gradients, everything finite, and in bf16 every element within 2 ulp of the eager value (one ulp from a flipped
rounding of a = gelu_tanh(gate), one more from the rounding of the product).  Norm (from
test_falcon_ops_gpu.py::test_layer_norm_vs_fp64_and_the_autocast_chain): rel(kernel, f64) <= 1.02 rel(eager module, f64) + 1e-6 for y,
dx and dw; h_out EQUAL to the eager add.  Liveness is exact: zeros in dead rows, the same bits in live ones.  Model and step: the
bounds tests/test_qwen3_gpu.py holds Qwen3 to."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-6
SENTINEL = 7.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _max_ulps_bf16(got, eager):
    """The largest distance of `got` from `eager` in units of the last place of the eager bf16 value."""
    e = eager.detach().float()
    ulp = torch.exp2(torch.floor(torch.log2(e.abs().clamp_min(2.0 ** -126))) - 7.0)
    return float(((got.detach().float() - e).abs() / ulp).max())


# ---- GeGLU ---------------------------------------------------------------------------------------------------------------
EDGES = [0.0, -0.0, 10.0, -10.0, 40.0, -40.0, 1e-3, -1e-3]          # tanh saturation and the linear region

# (R, C, dtype, halves of one [R, 2 C] buffer)
GEGLU_CASES = [(3, 8, torch.bfloat16, False), (3, 4, torch.float32, False), (17, 1000, torch.bfloat16, False),
               (17, 1000, torch.float32, False), (64, 24576, torch.bfloat16, False), (5, 24, torch.bfloat16, True),
               (130, 256, torch.bfloat16, True)]
# The capped grid: at most 2048 workgroups of 256 threads, so above 2048 * 256 vectors a thread walks further tiles by the launcher's
# (stride / C, stride % C) steps, two in flight per trip.  Both cases hold more than two grid strides (a second trip of the loop, its
# last tile partly outside) and C does not divide the stride (the column carry): the Gemma-7B rows at the hidden width as halves of
# one buffer, and an f32 tensor at an odd-ish width.
GEGLU_STRIDED = [(4608, 3072, torch.bfloat16, True), (4300, 1000, torch.float32, False)]
for _R, _C, _dt, _ in GEGLU_STRIDED:
    _stride = 2048 * 256 * (16 // _dt.itemsize)
    assert _R * _C > 2 * _stride and _stride % _C != 0
GEGLU_CASES += GEGLU_STRIDED


def _gate_up(R, C, dtype, halves, dev):
    """(leaf, gate view, up view): dense [R, C] tensors stacked in one leaf, or the column halves of one [R, 2 C] leaf."""
    g = torch.Generator().manual_seed(R * 1000 + C)
    gate = 2.5 * torch.randn(R, C, generator=g)
    gate.view(-1)[:8] = torch.tensor(EDGES)
    up = torch.randn(R, C, generator=g)
    go = torch.randn(R, C, generator=g).to(dtype).to(dev)
    if halves:
        leaf = torch.cat((gate, up), dim=1).to(dtype).to(dev)
        split = lambda t: (t[:, :C], t[:, C:])
    else:
        leaf = torch.stack((gate, up)).to(dtype).to(dev)
        split = lambda t: (t[0], t[1])
    return leaf, split, go


@pytest.mark.parametrize("R,C,dtype,halves", GEGLU_CASES)
def test_geglu_against_the_eager_chain_and_float64(dev, monkeypatch, R, C, dtype, halves):
    from dalm_amd import hip
    from dalm_amd.models import tower_ops

    leaf, split, go = _gate_up(R, C, dtype, halves, dev)
    calls, real_call = [], hip.call
    monkeypatch.setattr(hip, "call", lambda name, *a: (calls.append((name, a)), real_call(name, *a))[1])

    def run(fn, x):
        x = x.detach().clone().requires_grad_(True)
        out = fn(*split(x))
        out.backward(go.to(x.dtype))
        dg, du = split(x.grad)
        return out.detach(), dg, du

    def kernel(gate, up):
        assert tower_ops.geglu_supported(gate, up) and tower_ops._halves_of_one(gate, up) == halves
        return tower_ops.geglu(gate, up)

    def eager(gate, up):
        return torch.nn.functional.gelu(gate, approximate="tanh") * up

    got, ref, truth = run(kernel, leaf), run(eager, leaf), run(eager, leaf.double())
    assert [c[0] for c in calls] == ["dalm_geglu_fwd", "dalm_geglu_bwd"]
    ld = 2 * C if halves else C
    assert calls[0][1][4:9] == (R, C, ld, ld, C) and calls[1][1][6:13] == (R, C, C, ld, ld, C, C)      # read in place
    for name, a, e, t in zip(("act", "d_gate", "d_up"), got, ref, truth):
        assert a.dtype == dtype and a.shape == (R, C) and torch.isfinite(a).all(), name
        r_k, r_e = _rel(a, t), _rel(e, t)
        print(f"geglu {R}x{C} {dtype} halves={halves} {name}: kernel {r_k:.4e} eager {r_e:.4e}", end="")
        if dtype == torch.bfloat16:
            ulps = _max_ulps_bf16(a, e)
            print(f" max ulp {ulps:.2f} differing {int((a != e).sum())} of {a.numel()}", end="")
        print()
        assert r_k <= 1.02 * r_e + 1e-7, (name, r_k, r_e)
        if dtype == torch.bfloat16:
            assert ulps <= 2.0, (name, ulps)


def _geglu_raw(gate, up, d_act, live, ld):
    """The C entry points with output buffers the test owns (pre-filled: an untouched element shows)."""
    from dalm_amd import hip

    R, C = gate.shape
    fresh = lambda: torch.full((R, C), SENTINEL, dtype=gate.dtype, device=gate.device)
    act, dg, du = fresh(), fresh(), fresh()
    code = hip.dtype_code(gate)
    hip.call("dalm_geglu_fwd", hip.ptr(gate), hip.ptr(up), hip.ptr(act), code, R, C, ld, ld, C, hip.ptr(live), hip.stream())
    hip.call("dalm_geglu_bwd", hip.ptr(d_act), hip.ptr(gate), hip.ptr(up), hip.ptr(dg), hip.ptr(du), code, R, C, C, ld, ld, C, C,
             hip.ptr(live), hip.stream())
    return act, dg, du


def _dead_rows(R):
    """The first row, the last row and a run in the middle; with many rows also every 97th, so that every tile of a grid-stride
    walk meets dead and live rows."""
    dead = torch.zeros(R, dtype=torch.bool)
    dead[0] = dead[-1] = True
    dead[R // 2 - 1:R // 2 + 2] = True
    if R > 1000:
        dead[::97] = True
    assert 0 < int(dead.sum()) < R
    return dead


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("R,C,dtype,halves", [(17, 1000, torch.bfloat16, False), (130, 256, torch.bfloat16, True),
                                               (9, 4, torch.float32, False), (64, 24576, torch.bfloat16, True)] + GEGLU_STRIDED)
def test_geglu_row_liveness_is_exact(dev, R, C, dtype, halves):
    """Dead rows' inputs are NaN in the call with the vector: nothing of a dead row may be loaded."""
    leaf, split, go = _gate_up(R, C, dtype, halves, dev)
    gate, up = split(leaf)
    ld = 2 * C if halves else C
    want = _geglu_raw(gate, up, go, None, ld)
    dead = _dead_rows(R).to(dev)
    live = (~dead).to(torch.uint8)
    gate[dead], up[dead], go[dead] = float("nan"), float("nan"), float("nan")
    got = _geglu_raw(gate, up, go, live, ld)
    for name, a, b in zip(("act", "d_gate", "d_up"), want, got):
        assert _same_bits(a[~dead], b[~dead]), name
        assert float(b[dead].abs().max()) == 0.0 and not torch.isnan(b).any(), name


def test_geglu_declines_a_view_at_an_odd_storage_offset(dev):
    """A contiguous view 8 bytes into its storage: `geglu_supported` says no, so `_geglu_mlp_forward` keeps the eager chain for it
    instead of meeting DALM_E_ALIGN in the launcher."""
    from dalm_amd.models import tower_ops

    up = torch.randn(3, 8, device=dev).to(torch.bfloat16)
    gate = torch.randn(3 * 8 + 4, device=dev).to(torch.bfloat16)[4:].view(3, 8)
    assert gate.is_contiguous() and gate.data_ptr() % 16 == 8
    assert not tower_ops.geglu_supported(gate, up) and not tower_ops.geglu_supported(up, gate)
    assert tower_ops.geglu_supported(up, up.clone())


# ---- the norm ------------------------------------------------------------------------------------------------------------
def test_the_norm_guard_probes_f32_weights_under_bf16_activations_too(dev, monkeypatch):
    """With f32 norm weights the kernel runs with f32 activations, or - under autocast - with bf16 ones: the guard asks both, and
    as a predicate it leaves the module as it found it."""
    from transformers.models.gemma.modeling_gemma import GemmaRMSNorm

    from dalm_amd import hip
    from dalm_amd.models import fastpath

    mod = GemmaRMSNorm(64).to(dev)
    before = set(vars(mod))
    monkeypatch.delitem(fastpath._checked, ("gemma-norm", GemmaRMSNorm, torch.float32, "cuda"), raising=False)
    calls, real_call = [], hip.call
    monkeypatch.setattr(hip, "call", lambda name, *a: (calls.append((name, a[3], a[4])), real_call(name, *a))[1])
    assert fastpath._gemma_norm_matches(mod)
    assert sorted(calls) == sorted([("dalm_gemma_norm_fwd", hip.F32, hip.F32), ("dalm_gemma_norm_fwd", hip.BF16, hip.F32)]), calls
    assert set(vars(mod)) == before and float(mod.weight.abs().max()) == 0.0


def _hf_norm(w, eps=EPS):
    """transformers' GemmaRMSNorm.forward on the weight tensor `w` itself (a leaf's .grad is then the chain's weight gradient)."""
    import types

    from transformers.models.gemma import modeling_gemma as mg

    me = types.SimpleNamespace(weight=w, eps=eps)
    me._norm = lambda x: mg.GemmaRMSNorm._norm(me, x)
    return lambda x: mg.GemmaRMSNorm.forward(me, x)


NORM_CASES = ([(D, torch.bfloat16, wd) for D in (8, 256, 2048, 3072, 3080, 8192) for wd in (torch.float32, torch.bfloat16)]
              + [(D, torch.float32, torch.float32) for D in (4, 3072, 4096)] + [(3072, torch.float32, torch.bfloat16)]
              # the 2-chunk arm of the ladder (bf16 513 ... 1024, f32 257 ... 512) and the first width past it
              + [(1024, torch.bfloat16, torch.float32), (1032, torch.bfloat16, torch.bfloat16), (512, torch.float32, torch.float32),
                 (516, torch.float32, torch.float32)])


def _norm_inputs(D, dtype, w_dtype, dev):
    R = 37                                                          # odd, no multiple of the 4 rows of a workgroup, 10 workgroups
    g = torch.Generator().manual_seed(D)
    x = (torch.randn(R, D, generator=g) * 1.5 + 0.3).to(dtype).to(dev)
    delta = torch.randn(R, D, generator=g).to(dtype).to(dev)
    w = (0.3 * torch.randn(D, generator=g)).to(w_dtype).to(dev)
    gy = torch.randn(R, D, generator=g).to(dtype).to(dev)
    gres = torch.randn(R, D, generator=g).to(dtype).to(dev)
    return x, delta, w, gy, gres


def _norm_run(norm_of, x, delta, w, gy, gres):
    """(h, y, dx, dw) of `norm_of(x, delta, w) -> (h, y)` with the gradients gres (to h, or None) and gy (to y)."""
    x = x.detach().clone().requires_grad_(True)
    w = w.detach().clone().requires_grad_(True)
    h, y = norm_of(x, delta, w)
    if gres is None:
        y.backward(gy.to(y.dtype))
    else:
        torch.autograd.backward([h, y], [gres.to(h.dtype), gy.to(y.dtype)])
    return h.detach(), y.detach(), x.grad, w.grad


@pytest.mark.parametrize("with_dres", [True, False], ids=["dres", "nodres"])
@pytest.mark.parametrize("with_delta", [True, False], ids=["delta", "nodelta"])
@pytest.mark.parametrize("D,dtype,w_dtype", NORM_CASES)
def test_gemma_norm_against_the_eager_module_and_float64(dev, D, dtype, w_dtype, with_delta, with_dres):
    from dalm_amd.models import tower_ops

    x, delta, w, gy, gres = _norm_inputs(D, dtype, w_dtype, dev)
    delta = delta if with_delta else None
    gres = gres if with_dres else None
    assert tower_ops.gemma_rms_norm_supported(x, w)

    def kernel(x, delta, w):
        return tower_ops.gemma_add_rms_norm(x, delta, w, EPS)

    def eager(x, delta, w):
        h = x + delta if delta is not None else x
        return h, _hf_norm(w)(h)

    def truth(x, delta, w):
        h = x + delta if delta is not None else x
        hf = h.double()
        return h, hf * torch.rsqrt(hf.pow(2).mean(-1, keepdim=True) + EPS) * (1.0 + w.double())

    got, ref = _norm_run(kernel, x, delta, w, gy, gres), _norm_run(eager, x, delta, w, gy, gres)
    tru = _norm_run(truth, x.double(), None if delta is None else delta.double(), w.double(), gy.double(),
                    None if gres is None else gres.double())
    assert got[0].dtype == dtype and got[1].dtype == dtype and got[3].dtype == w_dtype
    assert torch.equal(got[0], ref[0])                              # h_out IS the eager add
    if not with_delta:
        assert torch.equal(got[0], x)                               # h IS x
    for name, i in (("y", 1), ("dx", 2), ("dw", 3)):
        r_k, r_e = _rel(got[i], tru[i]), _rel(ref[i], tru[i])
        print(f"gemma norm D={D} {dtype} w {w_dtype} delta={with_delta} dres={with_dres} {name}: kernel {r_k:.4e} eager {r_e:.4e}")
        assert torch.isfinite(got[i]).all(), name
        assert r_k <= 1.02 * r_e + 1e-6, (name, r_k, r_e)


def _norm_raw(x, delta, w, gy, h, rstd_in, gres, live):
    from dalm_amd import hip

    R, D = x.shape
    fresh = lambda: torch.full((R, D), SENTINEL, dtype=x.dtype, device=x.device)
    h_out, y, dx = (fresh() if delta is not None else None), fresh(), fresh()
    rstd = torch.full((R,), SENTINEL, dtype=torch.float32, device=x.device)
    hip.call("dalm_gemma_norm_fwd", hip.ptr(x), hip.ptr(delta), hip.ptr(w), hip.dtype_code(x), hip.dtype_code(w), R, D, EPS, hip.ptr(h_out),
             hip.ptr(y), hip.ptr(rstd), hip.ptr(live), hip.stream())
    hip.call("dalm_gemma_norm_bwd", hip.ptr(gy), hip.ptr(h if h is not None else h_out), hip.ptr(w),
             hip.ptr(rstd_in if rstd_in is not None else rstd), hip.ptr(gres), hip.dtype_code(x), hip.dtype_code(w), R, D, hip.ptr(dx),
             hip.ptr(live), hip.stream())
    return h_out, y, rstd, dx


@pytest.mark.parametrize("with_delta", [True, False], ids=["delta", "nodelta"])
@pytest.mark.parametrize("D,dtype,w_dtype", [(8, torch.bfloat16, torch.bfloat16), (3080, torch.bfloat16, torch.float32),
                                             (8192, torch.bfloat16, torch.bfloat16), (3072, torch.float32, torch.float32),
                                             (1024, torch.bfloat16, torch.float32)])
def test_gemma_norm_row_liveness_is_exact(dev, D, dtype, w_dtype, with_delta):
    x, delta, w, gy, gres = _norm_inputs(D, dtype, w_dtype, dev)
    delta = delta if with_delta else None
    h_in = None if with_delta else x                                # the backward reads the forward's h_out, or x itself
    want = _norm_raw(x, delta, w, gy, h_in, None, gres, None)
    dead = _dead_rows(x.shape[0]).to(dev)
    live = (~dead).to(torch.uint8)
    nan = float("nan")
    for t in (x, delta, gy, gres):
        if t is not None:
            t[dead] = nan
    # the backward of the second call gets NaN in the dead rows of h and rstd too
    h_nan, rstd_nan = (want[0] if with_delta else x).clone(), want[2].clone()
    h_nan[dead], rstd_nan[dead] = nan, nan
    got = _norm_raw(x, delta, w, gy, h_nan, rstd_nan, gres, live)
    for name, a, b in zip(("h_out", "y", "rstd", "dx"), want, got):
        if a is None:
            assert b is None
            continue
        assert _same_bits(a[~dead], b[~dead]), name
        assert float(b[dead].abs().max()) == 0.0 and not torch.isnan(b).any(), name


# ---- the model -----------------------------------------------------------------------------------------------------------
def _tiny(dev=None):
    from transformers import GemmaConfig, GemmaForCausalLM

    torch.manual_seed(0)
    cfg = GemmaConfig(vocab_size=128, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, head_dim=64)
    m = GemmaForCausalLM(cfg)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("norm.weight"):                   # away from the zero initialisation: a dropped "1 +" shows
                p.add_(0.3 * (2.0 * torch.rand(p.shape) - 1.0))
            p.copy_(p.to(torch.bfloat16).float())              # every copy below holds the SAME (bf16-exact) weights
    return m.train()


def _with_lora(model):
    from test_qwen3_gpu import _with_lora as with_lora

    return with_lora(model, False)


def _held(name, got, ref, truth):
    from test_qwen3_gpu import _held as held

    held(name, got, ref, truth)


def test_tiny_gemma_with_lora_routed_against_unrouted(dev, monkeypatch):
    """bf16 autocast, LoRA on q / v, left-padded rows of lengths 7 / 4 / 1: the logits and every LoRA gradient of the routed model are
    no further from the unrouted fp32 model than twice what the unrouted bf16 model is (tests/test_qwen3_gpu.py's rule, which it
    applies to the logits: the backward's loss is a signed sum of them, one scalar whose error is chance); the causal-LM loss of the
    routed logits within what that rule leaves it (the step test below also holds the step's loss to that file's bound for it);
    then the packed decoder run on the same rows against the same truth."""
    from test_qwen3_gpu import _cast

    from dalm_amd import hip, packed
    from dalm_amd.models import attention, lora
    from dalm_amd.models.frozen_linear import use_transposed_dgrad
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    base = _tiny()
    B, T = 3, 7
    ids = torch.randint(0, 128, (B, T), generator=torch.Generator().manual_seed(1)).to(dev)
    am = torch.ones(B, T, dtype=torch.long, device=dev)
    am[1, :3] = 0                                                    # lengths 7 / 4 / 1, left-padded
    am[2, :6] = 0
    w = torch.randn(B, T, 128, generator=torch.Generator().manual_seed(2)).to(dev) * am[..., None]
    rows, cu = packed.pack_plan(am.cpu(), shifted=True, multiple=64)
    rows, cu = rows.to(dev), cu.to(dev)
    valid = rows >= 0
    sel = rows[valid]
    seen = am.reshape(-1).index_select(0, sel) != 0
    wh = torch.randn(B * T, 256, generator=torch.Generator().manual_seed(4)).to(dev).index_select(0, sel) * seen[:, None]

    def grads(model):
        return {n: p.grad.detach().float().clone() for n, p in model.named_parameters() if p.requires_grad}

    def padded(model, dtype):
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
            logits = model(input_ids=ids, attention_mask=am, use_cache=False).logits
        (logits.float() * w).sum().backward()
        return logits.detach().float() * am[..., None], grads(model)

    def lm_loss(logits):
        """The causal-LM loss of these logits: mean next-token cross entropy over the pairs of live tokens (6 + 3 + 0)."""
        pair = (am[:, :-1] * am[:, 1:]).bool()
        return float(torch.nn.functional.cross_entropy(logits[:, :-1][pair].double(), ids[:, 1:][pair]))

    def hidden_padded(model, dtype):
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
            h = model.base_model(input_ids=ids, attention_mask=am, use_cache=False)[0].reshape(B * T, -1).index_select(0, sel)
        (h.float() * wh).sum().backward()
        return h.detach().float()[seen], grads(model)

    with monkeypatch.context() as mp:                                 # the references: transformers' own code, one eager LoRA
        mp.setattr(lora, "_GROUPS", False)                            # branch per projection
        mp.setattr(lora, "_FUSED", False)
        truth = _cast(_with_lora(copy.deepcopy(base)), dev, torch.float32)
        plain = _cast(_with_lora(copy.deepcopy(base)), dev, torch.bfloat16)
        t_logits, t_grads = padded(truth, torch.float32)
        r_logits, r_grads = padded(plain, torch.bfloat16)
        t_h, t_g = hidden_padded(truth, torch.float32)
        r_h, r_g = hidden_padded(plain, torch.bfloat16)
        assert not any(hasattr(l, "_dalm_orig_forward") for l in plain.model.layers)

    fast = copy.deepcopy(base)
    routed = use_generator_fast_paths(fast)
    assert routed["use_geglu_kernel"] == 2 and routed["use_gemma_rms_norm"] == 5 and routed["use_fused_residual_norm"] == 2
    assert routed["use_hip_attention_backward"] is True and fast.config._attn_implementation == attention.NAME
    assert routed["use_swiglu_kernel"] == 0 and routed["use_llama_attention_node"] == 0
    fast = _cast(_with_lora(fast), dev, torch.bfloat16)
    use_transposed_dgrad(fast)

    calls = []
    real_call = hip.call
    monkeypatch.setattr(hip, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    f_logits, f_grads = padded(fast, torch.bfloat16)
    # two MLPs; two norms a layer and the final one (the first layer's input norm has no backward: nothing in front of it
    # trains); the attention kernels at width 64
    assert calls.count("dalm_geglu_fwd") == 2 and calls.count("dalm_geglu_bwd") == 2, calls
    assert calls.count("dalm_gemma_norm_fwd") == 5 and calls.count("dalm_gemma_norm_bwd") == 4, calls
    assert calls.count("dalm_attn_gqa_fwd") == 2 and calls.count("dalm_attn_gqa_bwd") == 2, calls
    assert not any(c.startswith(("dalm_swiglu", "dalm_rms_norm")) for c in calls)
    names = set(t_grads)
    assert names == set(r_grads) == set(f_grads) and any("lora_A" in n for n in names)
    _held("gemma padded logits", f_logits, r_logits, t_logits)
    # the loss: one token's cross entropy moves by at most 2 max|d logits| (the log-sum-exp and the picked logit by at most one
    # each), so does their mean; with the rule above for the logits that is 4 x the unrouted bf16 model's largest logit error
    e_ref = float((r_logits - t_logits).abs().max())
    l_t, l_r, l_f = lm_loss(t_logits), lm_loss(r_logits), lm_loss(f_logits)
    print(f"gemma padded loss: fp32 {l_t:.6f} unrouted bf16 {l_r:.6f} routed {l_f:.6f}; largest unrouted logit error {e_ref:.3e}")
    assert abs(l_f - l_t) <= 4.0 * e_ref, (l_f, l_t, e_ref)
    for n in sorted(names):
        _held(f"gemma padded {n}", f_grads[n], r_grads[n], t_grads[n])

    # packed: the decoder stack on the un-padded rows, against the same rows of the padded truth
    assert packed.attention_is_packable(fast)
    calls.clear()
    fast.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        h = packed.generator_hidden(fast, ids, am, rows, cu)[valid]
    (h.float() * wh).sum().backward()
    assert calls.count("dalm_geglu_fwd") == 2 and calls.count("dalm_gemma_norm_bwd") == 4, calls
    _held("gemma packed hidden", h.detach().float()[seen], r_h, t_h)
    f_g = grads(fast)
    for n in sorted(names):
        _held(f"gemma packed {n}", f_g[n], r_g[n], t_g[n])


# ---- the step ------------------------------------------------------------------------------------------------------------
_BUILT = {}


def _gemma_lm():
    if "lm" not in _BUILT:
        _BUILT["lm"] = _with_lora(_tiny())
    return copy.deepcopy(_BUILT["lm"])


def _one_step(batch, mode, precision, dev):
    """test_qwen3_gpu.py's `_one_step` for kind "rag" with a tiny Gemma as the generator (tiny BERT retriever)."""
    from test_causal_retriever_gpu import _GradSnapshot
    from test_qwen3_gpu import _tiny_bert

    from dalm_amd import hip, packed
    from dalm_amd.models import AutoModelForRagE2E
    from dalm_amd.training.step import RagE2EStep

    model = AutoModelForRagE2E.from_modules(_tiny_bert(), _gemma_lm(), None, None, normalize=True, get_peft=None,
                                            retriever_is_autoregressive=False).to(dev)
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


def test_rag_step_with_a_gemma_generator_packed_against_padded(dev):
    """One RAG-e2e step, tiny BERT retriever + tiny Gemma generator (width 64: "dalm_sdpa", so it packs), at the bounds
    tests/test_qwen3_gpu.py holds the Qwen3 step to: fp32 - loss, gradient norm and every gradient within 1e-4; bf16 autocast - loss
    within 2.5e-4 and gradient norm within 2.2e-3 of the padded bf16 step, every parameter's gradient within twice the padded bf16
    step's own distance from the fp32 step + 5e-3, and within 4e-2 outright."""
    from test_causal_retriever_gpu import _rag_batch
    from test_qwen3_gpu import _rel_norm

    batch = _rag_batch(False)
    res = {(m, p): _one_step(batch, m, p, dev) for p in ("fp32", "bf16") for m in ("padded", "packed")}
    for key, (_, _, calls) in res.items():             # the Gemma kernels ran in every layout and precision, once per module
        assert calls.count("dalm_geglu_fwd") == 2 and calls.count("dalm_geglu_bwd") == 2, (key, calls)
        assert calls.count("dalm_gemma_norm_fwd") == 5 and calls.count("dalm_gemma_norm_bwd") == 4, (key, calls)
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
