"""Granite on the GPU: `dalm_rms_norm_scaled_{fwd,bwd}` and `dalm_scale_add` (dalm_amd/csrc/tower.hip) against transformers' own chain
(`residual + hidden_states * residual_multiplier`, GraniteRMSNorm) and its float64 restatement on the same tensors, against
`dalm_rms_norm_{fwd,bwd}_live` at a unit multiplier, with row liveness and with arguments they decline; a tiny Granite with LoRA, routed
against unrouted, padded and packed; one RAG step with a Granite generator, padded against packed and with the logits-free head.

Exact where the eager chain is exact: h = x + delta * m, ddelta = dx * m (from the kernel's own rounded dx) and both forms of
`dalm_scale_add` are compared by BITS with what torch computes on the same tensors; so are the kernels with m == 1 and
`dalm_rms_norm_{fwd,bwd}_live`.  Elsewhere the tolerance rule of tests/test_qwen3_gpu.py (`_held`): E_ref is the largest absolute error
of transformers' own sequence in the activation dtype against the truth on the same inputs (float64 for the kernels, the unrouted
model in float32 for models); the new path's error must be at most 2 E_ref, per tensor."""
import copy
import types

import pytest
import torch

from test_qwen3_gpu import _held, _rel_norm

pytestmark = pytest.mark.gpu

EPS = 1e-6
SENTINEL = 7.0
ROWS = (1, 17, 130)                          # one wave of a workgroup, an odd count, 33 workgroups with a partial last one
MULTS = (0.22, 1.0)
# widths: one 16-byte chunk of one lane; one chunk per lane over half a wave (bf16) / the whole wave (f32); 4 chunks (bf16) / 8 (f32);
# 3080 = 6 chunks and 8 elements, the 8-chunk kernel with a partial last chunk; 8 chunks (bf16) / 16 (f32); the bf16 cap, 16 chunks
NORM_WIDTHS = {torch.bfloat16: (8, 256, 2048, 3080, 4096, 8192), torch.float32: (8, 256, 2048, 4096)}
NORM_CASES = [(D, dt, m) for dt, Ds in NORM_WIDTHS.items() for D in Ds for m in MULTS]
ADD_CASES = [(D, dt, m) for dt, Ds in NORM_WIDTHS.items() for D in (*Ds, 12800, 24) for m in MULTS]       # no cap, and 24
BITS = {torch.bfloat16: torch.int16, torch.float32: torch.int32}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(BITS[a.dtype]), b.contiguous().view(BITS[b.dtype]))


def _hf_norm(w, eps=EPS):
    """transformers' GraniteRMSNorm.forward on the weight tensor `w` itself (a leaf's .grad is then the chain's weight gradient)."""
    from transformers.models.granite import modeling_granite as mg

    me = types.SimpleNamespace(weight=w, variance_epsilon=eps)
    return lambda x: mg.GraniteRMSNorm.forward(me, x)


def _norm64(h, w, eps=EPS):
    return w * (h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + eps))


def _dead_rows(R, seed):
    """About 40 % dead rows, the first and the last among them (one row: it is dead)."""
    dead = torch.rand(R, generator=torch.Generator().manual_seed(seed)) < 0.4
    dead[0] = dead[-1] = True
    return dead


def _inputs(R, D, dtype, dev):
    g = torch.Generator().manual_seed(1000 * R + D)
    x = (torch.randn(R, D, generator=g) * 1.5 + 0.3).to(dtype).to(dev)
    delta = (torch.randn(R, D, generator=g) * 2.0).to(dtype).to(dev)
    w = (1.0 + 0.3 * torch.randn(D, generator=g)).to(dtype).to(dev)
    gy = torch.randn(R, D, generator=g).to(dtype).to(dev)
    gh = torch.randn(R, D, generator=g).to(dtype).to(dev)
    return x, delta, w, gy, gh


def test_cases_are_the_issues():
    assert {D for D, dt, _ in NORM_CASES if dt == torch.bfloat16} == {8, 256, 2048, 3080, 4096, 8192}
    assert {D for D, dt, _ in NORM_CASES if dt == torch.float32} == {8, 256, 2048, 4096}
    assert {m for _, _, m in NORM_CASES} == {0.22, 1.0} and ROWS == (1, 17, 130)
    assert {12800, 24} <= {D for D, dt, _ in ADD_CASES if dt == torch.bfloat16} & {D for D, dt, _ in ADD_CASES if dt == torch.float32}


# ---- the scaled add with the norm behind it --------------------------------------------------------------------------------
def _pair_run(fn, x, delta, w, gy, gh):
    """(h, y) = fn(x, delta, w); the loss reads both: gh reaches h through the residual path, gy reaches y."""
    x, delta, w = [t.detach().clone().requires_grad_(True) for t in (x, delta, w)]
    h, y = fn(x, delta, w)
    torch.autograd.backward([h, y], [gh.to(h.dtype), gy.to(y.dtype)])
    return {"h": h.detach(), "y": y.detach(), "dx": x.grad, "ddelta": delta.grad, "dw": w.grad}


@pytest.mark.parametrize("D,dtype,mult", NORM_CASES)
def test_scaled_add_norm_against_float64_and_the_eager_pair(dev, D, dtype, mult):
    from dalm_amd.models import tower_ops

    def eager(x, delta, w):
        h = x + delta * mult
        return h, _hf_norm(w)(h)

    def truth(x, delta, w):
        h = x + delta * mult
        return h, _norm64(h, w)

    for R in ROWS:
        x, delta, w, gy, gh = _inputs(R, D, dtype, dev)
        assert tower_ops.scaled_add_rms_norm_supported(x, w)
        got = _pair_run(lambda x, delta, w: tower_ops.scaled_add_rms_norm(x, delta, mult, w, EPS), x, delta, w, gy, gh)
        ref = _pair_run(eager, x, delta, w, gy, gh)
        tru = _pair_run(truth, *[t.double() for t in (x, delta, w, gy, gh)])
        tag = f"R{R} D{D} {dtype} m{mult}"
        assert all(got[k].dtype == dtype for k in got), tag
        assert _same_bits(got["h"], ref["h"]), tag                         # h IS eager's x + delta * m
        assert _same_bits(got["ddelta"], got["dx"] * mult), tag            # what autograd makes of the rounded dx
        for name in ("y", "dx", "dw"):
            _held(f"scaled norm {tag} {name}", got[name], ref[name], tru[name])
        # without a gradient through the residual path (autograd hands the kernel zeros): the same equality, and dx alone is held
        x2, d2 = x.detach().clone().requires_grad_(True), delta.detach().clone().requires_grad_(True)
        _, y = tower_ops.scaled_add_rms_norm(x2, d2, mult, w, EPS)
        y.backward(gy)
        assert _same_bits(d2.grad, x2.grad * mult), tag
        xe, de = x.detach().clone().requires_grad_(True), delta.detach().clone().requires_grad_(True)
        eager(xe, de, w)[1].backward(gy)
        x64, d64 = x.double().requires_grad_(True), delta.double().requires_grad_(True)
        truth(x64, d64, w.double())[1].backward(gy.double())
        _held(f"scaled norm {tag} dx, no dres", x2.grad, xe.grad, x64.grad)


def _raw_fwd(x, delta, mult, w, live=None, pad=0):
    """The C entry point with output buffers the test owns: pre-filled, `pad` rows more on either side of what the call may write."""
    from dalm_amd import hip

    R, D = x.shape
    h = torch.full((R + 2 * pad, D), SENTINEL, dtype=x.dtype, device=x.device)
    y = torch.full_like(h, SENTINEL)
    rstd = torch.full((R + 2 * pad,), SENTINEL, dtype=torch.float32, device=x.device)
    hip.call("dalm_rms_norm_scaled_fwd", hip.ptr(x), hip.ptr(delta), mult, hip.ptr(w), hip.dtype_code(x), R, D, EPS, hip.ptr(h[pad:]),
             hip.ptr(y[pad:]), hip.ptr(rstd[pad:]), hip.ptr(live), hip.stream())
    return h, y, rstd


def _raw_bwd(gy, h, w, rstd, dres, mult, live=None, pad=0):
    from dalm_amd import hip

    R, D = h.shape
    dx = torch.full((R + 2 * pad, D), SENTINEL, dtype=h.dtype, device=h.device)
    dd = torch.full_like(dx, SENTINEL)
    hip.call("dalm_rms_norm_scaled_bwd", hip.ptr(gy), hip.ptr(h), hip.ptr(w), hip.ptr(rstd), hip.ptr(dres), mult, hip.dtype_code(h), R, D,
             hip.ptr(dx[pad:]), hip.ptr(dd[pad:]), hip.ptr(live), hip.stream())
    return dx, dd


@pytest.mark.parametrize("D,dtype", [(D, dt) for dt, Ds in NORM_WIDTHS.items() for D in Ds])
def test_unit_multiplier_gives_the_bits_of_the_unscaled_kernels(dev, D, dtype):
    """mult == 1: h, y, rstd and dx are `dalm_rms_norm_fwd_live` / `dalm_rms_norm_bwd_live`'s on the same inputs, bit for bit, with and
    without the residual-path gradient; ddelta is dx."""
    from dalm_amd.models import tower_ops

    for R in ROWS:
        x, delta, w, gy, gh = _inputs(R, D, dtype, dev)
        h0, y0, r0 = tower_ops._norm_fwd(x, delta, w, EPS)
        h1, y1, r1 = _raw_fwd(x, delta, 1.0, w)
        assert _same_bits(h0, h1) and _same_bits(y0, y1) and torch.equal(r0, r1), (R, D)
        for dres in (gh, None):
            dx0 = tower_ops._norm_bwd(gy, h0, w, r0, dres)
            dx1, dd1 = _raw_bwd(gy, h0, w, r0, dres, 1.0)
            assert _same_bits(dx0, dx1) and _same_bits(dd1, dx1), (R, D, dres is None)


# ---- the scaled add alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dtype,mult", ADD_CASES)
def test_scale_add_is_torchs_pair_bit_for_bit(dev, D, dtype, mult):
    from dalm_amd.models import tower_ops

    for R in ROWS:
        g = torch.Generator().manual_seed(7 * R + D)
        res = (torch.randn(R, D, generator=g) * 1.5 + 0.3).to(dtype).to(dev)
        x = (torch.randn(R, D, generator=g) * 2.0).to(dtype).to(dev)
        go = torch.randn(R, D, generator=g).to(dtype).to(dev)
        assert tower_ops.scale_add_supported(x, res) and tower_ops.scale_add_supported(x)
        r1, x1 = res.clone().requires_grad_(True), x.clone().requires_grad_(True)
        out = tower_ops.scale_add(r1, x1, mult)
        out.backward(go)
        r2, x2 = res.clone().requires_grad_(True), x.clone().requires_grad_(True)
        want = r2 + x2 * mult
        want.backward(go)
        tag = (R, D, dtype, mult)
        assert _same_bits(out.detach(), want.detach()), tag
        assert _same_bits(x1.grad, x2.grad) and _same_bits(r1.grad, r2.grad) and _same_bits(r1.grad, go), tag
        x3 = x.clone().requires_grad_(True)
        alone = tower_ops.scale_add(None, x3, mult)
        alone.backward(go)
        assert _same_bits(alone.detach(), x * mult) and _same_bits(x3.grad, go * mult), tag
        y = tower_ops.scale_add(res.view(1, R, D), x.view(1, R, D), mult)                     # leading dimensions are rows
        assert y.shape == (1, R, D) and _same_bits(y.view(R, D), want.detach()), tag


# ---- row liveness -----------------------------------------------------------------------------------------------------------
def _dead_zero_live_same(name, want, got, dead, pad, tag):
    """Rows of `got` (the call with the vector): zeros where dead, the bits of `want` (the call without) where live, and the `pad`
    rows on either side of both still hold what the test put there."""
    R = dead.numel()
    for t in (want, got):
        edge = torch.cat((t[:pad], t[pad + R:])).float()
        assert edge.numel() and float((edge - SENTINEL).abs().max()) == 0.0, (name, tag)
    a, b = want[pad:pad + R], got[pad:pad + R]
    assert float(b[dead].float().abs().max()) == 0.0 and not torch.isnan(b[dead].float()).any(), (name, tag)
    if (~dead).any():
        va, vb = (a, b) if a.dtype == torch.float32 and a.dim() == 1 else (a.view(BITS[a.dtype]), b.view(BITS[b.dtype]))
        assert torch.equal(va[~dead], vb[~dead]), (name, tag)


@pytest.mark.parametrize("D,dtype,mult", [(8, torch.bfloat16, 0.22), (3080, torch.bfloat16, 0.22), (4096, torch.bfloat16, 1.0),
                                          (8192, torch.bfloat16, 0.22), (256, torch.float32, 0.22), (4096, torch.float32, 0.22)])
def test_row_liveness_is_exact(dev, D, dtype, mult):
    """Dead rows' inputs are NaN in the calls with the vector: nothing of a dead row may be loaded; their outputs are zeros; live
    rows carry the bits of the call without the vector; two rows in front of and behind every output keep their fill."""
    from dalm_amd import hip
    from dalm_amd.models import tower_ops

    PAD = 2
    for R in ROWS:
        x, delta, w, gy, gh = _inputs(R, D, dtype, dev)
        tag = (R, D, dtype, mult)
        dead = _dead_rows(R, R + D).to(dev)
        live = (~dead).to(torch.uint8)
        want_f = _raw_fwd(x, delta, mult, w, None, PAD)
        h, rstd = want_f[0][PAD:PAD + R].clone(), want_f[2][PAD:PAD + R].clone()
        want_b = [_raw_bwd(gy, h, w, rstd, dres, mult, None, PAD) for dres in (gh, None)]

        def add_raw(res, xx, lv):
            out = torch.full((R + 2 * PAD, D), SENTINEL, dtype=dtype, device=dev)
            hip.call("dalm_scale_add", hip.ptr(res), hip.ptr(xx), mult, hip.ptr(out[PAD:]), hip.dtype_code(xx), R, D, hip.ptr(lv),
                     hip.stream())
            return out

        want_a = [add_raw(res, delta, None) for res in (x, None)]
        xn, dn, gyn, ghn, hn, rn = [t.clone() for t in (x, delta, gy, gh, h, rstd)]
        for t in (xn, dn, gyn, ghn, hn, rn):
            t[dead] = float("nan")
        got_f = _raw_fwd(xn, dn, mult, w, live, PAD)
        for name, a, b in zip(("h", "y", "rstd"), want_f, got_f):
            _dead_zero_live_same(name, a, b, dead, PAD, tag)
        for (wdx, wdd), dres in zip(want_b, (ghn, None)):
            gdx, gdd = _raw_bwd(gyn, hn, w, rn, dres, mult, live, PAD)
            _dead_zero_live_same("dx", wdx, gdx, dead, PAD, tag)
            _dead_zero_live_same("ddelta", wdd, gdd, dead, PAD, tag)
        for want, res in zip(want_a, (xn, None)):
            _dead_zero_live_same("scale_add", want, add_raw(res, dn, live), dead, PAD, tag)
        # the autograd functions take the vector as an argument and give the same bits, forward and backward
        xa, da = xn.clone().requires_grad_(True), dn.clone().requires_grad_(True)
        hh, yy = tower_ops.scaled_add_rms_norm(xa, da, mult, w, EPS, live)
        assert _same_bits(hh.detach(), got_f[0][PAD:PAD + R]) and _same_bits(yy.detach(), got_f[1][PAD:PAD + R]), tag
        torch.autograd.backward([hh, yy], [ghn, gyn])
        assert float(xa.grad[dead].float().abs().max()) == 0.0 and float(da.grad[dead].float().abs().max()) == 0.0, tag
        assert _same_bits(xa.grad[~dead], want_b[0][0][PAD:PAD + R][~dead]), tag
        xs = dn.clone().requires_grad_(True)
        out = tower_ops.scale_add(xn, xs, mult, live)
        out.backward(gyn)
        assert float(out.detach()[dead].float().abs().max()) == 0.0 and float(xs.grad[dead].float().abs().max()) == 0.0, tag
        assert _same_bits(xs.grad[~dead], (gy * mult)[~dead]), tag


def test_the_tower_calls_vector_is_picked_up(dev):
    from dalm_amd import live_rows
    from dalm_amd.models import tower_ops

    B, T, D = 3, 7, 256
    x, delta, w, gy, _ = _inputs(B * T, D, torch.bfloat16, dev)
    mask = (torch.arange(T).unsqueeze(0) >= (T - torch.tensor([7, 4, 1])).unsqueeze(1)).long().to(dev)
    with live_rows.tower_call(mask, True) as vec:
        assert vec is not None and int(vec.sum()) == 7 + 5 + 2             # a row also matters when the next column is live
        h, y = tower_ops.scaled_add_rms_norm(x.view(B, T, D), delta.view(B, T, D), 0.22, w, EPS)
        out = tower_ops.scale_add(x.view(B, T, D), delta.view(B, T, D), 0.22)
    dead = vec == 0
    for t in (h, y, out):
        assert float(t.reshape(B * T, D)[dead].float().abs().max()) == 0.0
    assert _same_bits(out.reshape(B * T, D)[~dead], (x + delta * 0.22)[~dead])
    outside = tower_ops.scale_add(x.view(B, T, D), delta.view(B, T, D), 0.22)                 # no tower call: every row
    assert _same_bits(outside.reshape(B * T, D), x + delta * 0.22)


# ---- what the entry points decline ------------------------------------------------------------------------------------------
def test_unsupported_calls_return_the_error_code_and_write_nothing(dev):
    from dalm_amd import hip
    from dalm_amd.models import tower_ops

    R, D = 5, 64
    x, delta, w, gy, gh = _inputs(R, D, torch.bfloat16, dev)
    rstd = torch.ones(R, device=dev)
    outs = [torch.full((R, 8200), SENTINEL, dtype=torch.bfloat16, device=dev) for _ in range(2)]
    stat = torch.full((R,), SENTINEL, dtype=torch.float32, device=dev)
    wide = torch.zeros(R, 8200, dtype=torch.bfloat16, device=dev)
    w_wide = torch.ones(8200, dtype=torch.bfloat16, device=dev)
    flat = torch.zeros(R * D + 8, dtype=torch.bfloat16, device=dev)
    off = flat[1:1 + R * D].view(R, D)                                      # a pointer 2 bytes off a 16-byte boundary
    assert off.data_ptr() % 16 == 2

    def fwd(x=x, delta=delta, w=w, dtype=hip.BF16, D=D, h=outs[0], y=outs[1]):
        hip.call("dalm_rms_norm_scaled_fwd", hip.ptr(x), hip.ptr(delta), 0.22, hip.ptr(w), dtype, R, D, EPS, hip.ptr(h), hip.ptr(y),
                 hip.ptr(stat), None, hip.stream())

    def bwd(gy=gy, h=x, w=w, dtype=hip.BF16, D=D, dx=outs[0], dd=outs[1]):
        hip.call("dalm_rms_norm_scaled_bwd", hip.ptr(gy), hip.ptr(h), hip.ptr(w), hip.ptr(rstd), hip.ptr(gh), 0.22, dtype, R, D,
                 hip.ptr(dx), hip.ptr(dd), None, hip.stream())

    def add(res=x, xx=delta, dtype=hip.BF16, D=D, out=outs[0]):
        hip.call("dalm_scale_add", hip.ptr(res), hip.ptr(xx), 0.22, hip.ptr(out), dtype, R, D, None, hip.stream())

    cases = [(-1, lambda: fwd(delta=None)),                                 # dalm_rms_norm_fwd_live takes a NULL delta; this one does not
             (-1, lambda: fwd(h=None)), (-1, lambda: bwd(dd=None)), (-1, lambda: add(xx=None)), (-1, lambda: add(out=None)),
             (-2, lambda: fwd(x=wide, delta=wide, w=w_wide, D=8200)),       # over the cap of 8192
             (-2, lambda: bwd(gy=wide, h=wide, w=w_wide, D=8200)),
             (-2, lambda: fwd(dtype=hip.F32, D=4100)),                      # over the f32 cap of 4096
             (-2, lambda: fwd(D=60)), (-2, lambda: bwd(D=60)), (-2, lambda: add(D=60)),       # 120 bytes: no multiple of 16
             (-4, lambda: fwd(x=off)), (-4, lambda: fwd(delta=off)), (-4, lambda: fwd(y=off)), (-4, lambda: bwd(gy=off)),
             (-4, lambda: bwd(dd=off)), (-4, lambda: add(res=off)), (-4, lambda: add(xx=off)), (-4, lambda: add(out=off)),
             (-3, lambda: fwd(dtype=2)), (-3, lambda: bwd(dtype=5)), (-3, lambda: add(dtype=-1))]
    for code, call in cases:
        with pytest.raises(ValueError, match=f"code {code}"):
            call()
    torch.cuda.synchronize()
    for t in (*outs, stat):
        assert float((t.float() - SENTINEL).abs().max()) == 0.0
    assert float(flat.float().abs().max()) == 0.0
    # and what the host-side predicates say of the same tensors
    assert not tower_ops.scaled_add_rms_norm_supported(wide, w_wide) and not tower_ops.scaled_add_rms_norm_supported(x[:, :60], w[:60])
    assert not tower_ops.scaled_add_rms_norm_supported(x.cpu(), w.cpu()) and not tower_ops.scaled_add_rms_norm_supported(x.half(), w.half())
    assert not tower_ops.scaled_add_rms_norm_supported(x, w.float())        # an f32 weight promotes the eager product: not this kernel
    assert tower_ops.scale_add_supported(wide)                              # no cap without a reduction
    assert not tower_ops.scale_add_supported(x[:, :60]) and not tower_ops.scale_add_supported(x.cpu())
    assert not tower_ops.scale_add_supported(x, x.float()) and not tower_ops.scale_add_supported(x.half())


# ---- the model -----------------------------------------------------------------------------------------------------------
_NORMS = ("norm.weight", "layernorm.weight")
VOCAB = 259


def _tiny():
    from transformers import GraniteConfig, GraniteForCausalLM

    torch.manual_seed(0)
    cfg = GraniteConfig(vocab_size=VOCAB, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                        num_key_value_heads=2, max_position_embeddings=64, tie_word_embeddings=True, pad_token_id=1, bos_token_id=None,
                        eos_token_id=2, embedding_multiplier=12.0, residual_multiplier=0.22, attention_multiplier=0.015625,
                        logits_scaling=8.0)
    m = GraniteForCausalLM(cfg)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith(_NORMS):
                p.add_(0.3 * (2.0 * torch.rand(p.shape) - 1.0))
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


def test_tiny_model_with_lora_routed_against_unrouted(dev, monkeypatch):
    """Left-padded rows of lengths 7 / 4 / 1, bf16 autocast: logits and every LoRA gradient of the routed model are no further from
    the unrouted fp32 model than twice what the unrouted bf16 model is; then the packed decoder run on the same rows."""
    from dalm_amd import hip, packed
    from dalm_amd.models import lora
    from dalm_amd.models.frozen_linear import FrozenLinearT, use_transposed_dgrad
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    base = _tiny()
    B, T = 3, 7
    ids = torch.randint(3, VOCAB, (B, T), generator=torch.Generator().manual_seed(1)).to(dev)
    am = (torch.arange(T).unsqueeze(0) >= (T - torch.tensor([7, 4, 1])).unsqueeze(1)).long().to(dev)
    w = torch.randn(B, T, VOCAB, generator=torch.Generator().manual_seed(2)).to(dev) * am[..., None]
    rows, cu = packed.pack_plan(am.cpu(), shifted=True, multiple=64)
    rows, cu = rows.to(dev), cu.to(dev)
    valid = rows >= 0
    sel = rows[valid]
    seen = am.reshape(-1).index_select(0, sel) != 0         # the rows a loss reads (a padding row in front of a sequence is packed too)
    wh = torch.randn(B * T, 256, generator=torch.Generator().manual_seed(4)).to(dev).index_select(0, sel) * seen[:, None]

    def grads(model):
        return {n: p.grad.detach().float().clone() for n, p in model.named_parameters() if p.requires_grad}

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
        truth = _cast(_with_lora(copy.deepcopy(base)), dev, torch.float32)
        plain = _cast(_with_lora(copy.deepcopy(base)), dev, torch.bfloat16)
        assert not any(hasattr(l, "_dalm_orig_forward") for l in plain.model.layers)
        t_logits, t_grads = padded(truth, torch.float32)
        r_logits, r_grads = padded(plain, torch.bfloat16)
        t_h, t_g = hidden_padded(truth, torch.float32)
        r_h, r_g = hidden_padded(plain, torch.bfloat16)

    fast = copy.deepcopy(base)
    routed = use_generator_fast_paths(fast)
    assert routed["use_fused_residual_norm"] == 2 and routed["use_llama_attention_node"] == 2 and routed["use_swiglu_kernel"] == 2
    assert routed["use_hip_attention_backward"] is True
    fast = _cast(_with_lora(fast), dev, torch.bfloat16)
    assert use_transposed_dgrad(fast) == 2 * 4 + 1                     # o, gate, up, down per layer and the lm_head
    for layer in fast.model.layers:                                    # q | k | v of a Granite layer form one group
        a = layer.self_attn
        assert a.q_proj._group is not None and a.q_proj._group is a.k_proj._group is a.v_proj._group
        assert len(a.q_proj._group.members) == 3
        assert type(a.o_proj) is FrozenLinearT and type(layer.mlp.gate_proj) is FrozenLinearT

    calls, scales = [], []
    real_call = hip.call

    def spy(name, *args):
        calls.append(name)
        if name == "dalm_attn_gqa_fwd":
            scales.append(args[11])
        return real_call(name, *args)

    def ran_routed(extra_scale_adds=0):
        assert calls.count("dalm_rms_norm_scaled_fwd") == 2 and calls.count("dalm_rms_norm_scaled_bwd") == 2, calls   # once per layer
        assert calls.count("dalm_scale_add") == 4 + extra_scale_adds, calls                  # the trailing add of a layer, each way
        # input_layernorm; its backward in the second layer only (the first one's input is the frozen embedding: nothing asks for dx)
        assert calls.count("dalm_rms_norm_fwd_live") == 2 and calls.count("dalm_rms_norm_bwd_live") == 1, calls
        assert calls.count("dalm_attn_gqa_fwd") == 2 and calls.count("dalm_attn_gqa_bwd") == 2, calls
        assert scales[-2:] == [0.015625] * 2, scales                                         # the softmax scale is attention_multiplier
        assert any(c.startswith("dalm_swiglu") or c.startswith("dalm_linear_live_swiglu") for c in calls), calls
        assert any(c.startswith("dalm_lora2_") for c in calls), calls                        # the q|k|v group's kernels

    monkeypatch.setattr(hip, "call", spy)
    f_logits, f_grads = padded(fast, torch.bfloat16)
    ran_routed()
    assert all(l.self_attn.q_proj._group.enabled for l in fast.model.layers)
    names = set(t_grads)
    assert names == set(r_grads) == set(f_grads) and any("lora_A" in n for n in names)
    _held("model padded logits", f_logits, r_logits, t_logits)
    for n in sorted(names):
        _held(f"model padded {n}", f_grads[n], r_grads[n], t_grads[n])

    # packed: the generator's decoder stack on the un-padded rows, against the same rows of the padded truth
    calls.clear()
    fast.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        h = packed.generator_hidden(fast, ids, am, rows, cu)[valid]
    (h.float() * wh).sum().backward()
    ran_routed()
    _held("model packed hidden", h.detach().float()[seen], r_h, t_h)
    f_g = grads(fast)
    for n in sorted(names):
        _held(f"model packed {n}", f_g[n], r_g[n], t_g[n])


# ---- one step ------------------------------------------------------------------------------------------------------------
_BUILT = {}


def _granite_lm():
    """The tiny Granite with LoRA on q / v (no dropout, lora_B randomised), weights on the bf16 grid; built once on the CPU."""
    if "lm" not in _BUILT:
        _BUILT["lm"] = _with_lora(_tiny())
    return copy.deepcopy(_BUILT["lm"])


def _one_rag_step(batch, mode, precision, dev):
    """tests/test_olmo2_gpu.py's `_one_rag_step`: tiny BERT retriever + tiny Granite generator; mode "padded", "packed" or "fused"
    (padded, fuse_lm_head)."""
    from test_causal_retriever_gpu import _GradSnapshot
    from test_qwen3_gpu import _tiny_bert

    from dalm_amd import hip, packed
    from dalm_amd.models import AutoModelForRagE2E
    from dalm_amd.training.step import RagE2EStep

    model = AutoModelForRagE2E.from_modules(_tiny_bert(), _granite_lm(), None, None, normalize=True, get_peft=None,
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
                      track_grad_norm=True, fuse_lm_head=mode == "fused")
    host = packed.add_pack_plans(batch, packed.RAG_GROUPS) if mode == "packed" else batch
    calls, real_call = [], hip.call
    hip.call = lambda name, *a: (calls.append(name), real_call(name, *a))[1]
    try:
        dbatch = {k: v.to(dev) for k, v in host.items()}
        loss = float(step(dbatch))
    finally:
        hip.call = real_call
    assert step._packed_generator(dbatch) == (mode == "packed")
    return {"loss": loss, "grad_norm": float(step.grad_norm)}, snap.grads, calls


def test_rag_step_with_a_granite_generator_packed_and_fused_against_padded(dev):
    """One RAG-e2e step, tiny BERT retriever + tiny Granite generator (logits_scaling 8): the packed step and the padded step with
    fuse_lm_head, each against the padded step that materialises the model's own logits, at the bounds
    `test_rag_step_with_an_olmo2_generator_packed_against_padded` (tests/test_olmo2_gpu.py) holds packed against padded to: fp32 -
    loss, gradient norm and every gradient within 1e-4; bf16 autocast - loss within 2.5e-4 and gradient norm within 2.2e-3 of the
    padded bf16 step, every parameter's gradient within twice the padded bf16 step's own distance from the fp32 step + 5e-3, and
    within 4e-2 outright.  Both other routes multiply the hidden states with lm_head.weight themselves: without the scaling their
    logits are 8 x too large and none of the bounds holds."""
    from test_causal_retriever_gpu import _rag_batch

    batch = _rag_batch(False)
    res = {(m, p): _one_rag_step(batch, m, p, dev) for p in ("fp32", "bf16") for m in ("padded", "packed", "fused")}
    for (m, p), (_, _, calls) in res.items():             # both scaled adds of both layers ran as kernels, in f32 and in bf16
        assert calls.count("dalm_rms_norm_scaled_fwd") == 2 and calls.count("dalm_rms_norm_scaled_bwd") == 2, (m, p, calls)
        assert calls.count("dalm_scale_add") == (4 if m == "padded" else 6), (m, p, calls)     # + the logits scaling, each way
    g32 = res["padded", "fp32"][1]
    assert any("generator_model" in n for n in g32)
    for other in ("packed", "fused"):
        o32 = res[other, "fp32"][1]
        assert set(g32) == set(o32)
        for k in ("loss", "grad_norm"):
            d = abs(res[other, "fp32"][0][k] - res["padded", "fp32"][0][k]) / abs(res["padded", "fp32"][0][k])
            print(f"fp32 {other} vs padded {k}: {d:.3e}")
            assert d <= 1e-4, (other, k, d)
        worst = max(_rel_norm(o32[n], g32[n]) for n in g32 if float(g32[n].double().norm()) >= 1e-7)
        print(f"fp32 {other} worst gradient: {worst:.3e}")
        assert worst <= 1e-4, other
        for k, tol in (("loss", 2.5e-4), ("grad_norm", 2.2e-3)):
            d = abs(res[other, "bf16"][0][k] - res["padded", "bf16"][0][k]) / abs(res["padded", "bf16"][0][k])
            print(f"bf16 {other} vs padded {k}: {d:.3e}")
            assert d <= tol, (other, k, d)
        g16, o16 = res["padded", "bf16"][1], res[other, "bf16"][1]
        for n in sorted(g32):
            den = max(float(g32[n].double().norm()), 1e-30)
            d_pad, d_oth = float((g16[n].double() - g32[n].double()).norm()) / den, float((o16[n].double() - g32[n].double()).norm()) / den
            print(f"{n}: padded {d_pad:.3e} {other} {d_oth:.3e}")
            if float(g32[n].double().norm()) >= 1e-7:
                assert d_oth <= 2.0 * d_pad + 5e-3 and d_oth <= 4e-2, (other, n, d_oth, d_pad)
