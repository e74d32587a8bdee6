"""Cohere on the GPU: `dalm_rope_il_qk`, `dalm_cohere_norm_{fwd,bwd}` and `dalm_add3_live` (dalm_amd/csrc/tower.hip) against
transformers' own chains (modeling_cohere.py `apply_rotary_pos_emb`, `CohereLayerNorm`, `residual + attn + mlp`) on the same tensors,
with row liveness; a tiny Cohere with LoRA, routed against unrouted, padded and packed, in fp32 and bf16; one RAG step with a Cohere
generator, padded against packed and with the logits-free head.

Exact where the eager chain is exact: the rotation (forward and autograd's backward) and the three-way add are compared by BITS with
what torch computes on the same tensors.  The norm follows the tolerance rule of tests/test_qwen3_gpu.py (`_held`): E_ref is the largest
absolute error of the eager CohereLayerNorm under autograd, in the activation dtype, against a float64 evaluation of its formula on the
same inputs; the kernel's error must be at most 2 E_ref, per tensor.  Models: the same rule with the unrouted fp32 model as the truth."""
import copy
import types

import pytest
import torch

from test_qwen3_gpu import _held, _rel_norm

pytestmark = pytest.mark.gpu

EPS = 1e-5
SENTINEL = 7.0
ROWS = (1, 17, 130)                          # one wave of a workgroup, an odd count, 33 workgroups with a partial last one
# widths: one 16-byte chunk of one lane; one chunk per lane over half a wave (bf16) / the whole wave (f32); 4 chunks (bf16) / 8 (f32);
# 3080 = 6 chunks and 8 elements, the 8-chunk kernel with a partial last chunk; 8 chunks (bf16) / 16 (f32); the bf16 cap, 16 chunks
NORM_WIDTHS = {torch.bfloat16: (8, 256, 2048, 3080, 4096, 8192), torch.float32: (8, 256, 2048, 4096)}
NORM_CASES = [(D, dt, wdt) for dt, Ds in NORM_WIDTHS.items() for D in Ds for wdt in (torch.bfloat16, torch.float32)]
ADD_CASES = [(D, dt) for dt, Ds in NORM_WIDTHS.items() for D in (*Ds, 12800, 24)]               # no cap, and 24
BITS = {torch.bfloat16: torch.int16, torch.float32: torch.int32}
HEADS = [(4, 2), (2, 2), (3, 1)]
SIZES = [(2, 5), (1, 33), (3, 64)]           # odd row counts, head rows not a multiple of the rows of a workgroup, more than one workgroup
PAIRS = [(torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32), (torch.float32, torch.float32)]   # activations, tables


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(BITS[a.dtype]), b.contiguous().view(BITS[b.dtype]))


def _dead_rows(R, seed):
    """About 40 % dead rows, the first and the last among them (one row: it is dead)."""
    dead = torch.rand(R, generator=torch.Generator().manual_seed(seed)) < 0.4
    dead[0] = dead[-1] = True
    return dead


def test_cases_are_the_issues():
    assert {D for D, dt, _ in NORM_CASES if dt == torch.bfloat16} == {8, 256, 2048, 3080, 4096, 8192}
    assert {D for D, dt, _ in NORM_CASES if dt == torch.float32} == {8, 256, 2048, 4096}
    assert {w for _, _, w in NORM_CASES} == {torch.bfloat16, torch.float32} and ROWS == (1, 17, 130)
    assert {12800, 24} <= {D for D, dt in ADD_CASES if dt == torch.bfloat16} & {D for D, dt in ADD_CASES if dt == torch.float32}
    assert HEADS == [(4, 2), (2, 2), (3, 1)] and SIZES == [(2, 5), (1, 33), (3, 64)] and len(PAIRS) == 3


# ---- the interleaved rotary embedding ------------------------------------------------------------------------------------
def _tables(B, T, hd, kind, dtype, dev, g):
    """cos / sin [1, T, hd] or [B, T, hd].  "one" / "batch": CohereRotaryEmbedding's (repeat_interleave: equal within a pair);
    "distinct": independent values at 2i and 2i + 1, so a kernel that reads one of a pair for both fails."""
    nb = 1 if kind == "one" else B
    if kind == "distinct":
        ang = torch.rand(nb, T, hd, generator=g) * 6.28
        cos, sin = ang.cos(), (ang + torch.rand(nb, T, hd, generator=g)).sin()
    else:
        inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2).float() / hd))
        pos = torch.randint(0, 512, (nb, T), generator=g).float()
        emb = torch.repeat_interleave(pos[..., None] * inv, 2, dim=-1)
        cos, sin = emb.cos(), emb.sin()
    return cos.to(dtype).to(dev), sin.to(dtype).to(dev)


def _qkv(B, T, Hq, Hk, hd, dtype, dev, g):
    """One [B, T, (Hq + 2 Hk) hd] buffer - the q | k | v GEMM's output - as a leaf, and q, k as column slices of it."""
    buf = torch.randn(B, T, (Hq + 2 * Hk) * hd, generator=g).to(dtype).to(dev).requires_grad_(True)
    q = buf[..., :Hq * hd].view(B, T, Hq, hd).transpose(1, 2)
    k = buf[..., Hq * hd:(Hq + Hk) * hd].view(B, T, Hk, hd).transpose(1, 2)
    return buf, q, k


@pytest.mark.parametrize("B,T", SIZES)
@pytest.mark.parametrize("Hq,Hk", HEADS)
@pytest.mark.parametrize("hd", [32, 64, 128])
def test_rotary_is_the_eager_chain_bit_for_bit(dev, hd, Hq, Hk, B, T):
    from transformers.models.cohere import modeling_cohere as mc

    from dalm_amd.models import tower_ops

    for dtype, tab in PAIRS:
        for kind in ("one", "batch", "distinct"):
            g = torch.Generator().manual_seed(hd + 7 * B + T + Hq)
            cos, sin = _tables(B, T, hd, kind, tab, dev, g)
            buf1, q1, k1 = _qkv(B, T, Hq, Hk, hd, dtype, dev, g)
            buf2 = buf1.detach().clone().requires_grad_(True)
            q2 = buf2[..., :Hq * hd].view(B, T, Hq, hd).transpose(1, 2)
            k2 = buf2[..., Hq * hd:(Hq + Hk) * hd].view(B, T, Hk, hd).transpose(1, 2)
            gq = torch.randn(B, Hq, T, hd, generator=g).to(dtype).to(dev)
            gk = torch.randn(B, Hk, T, hd, generator=g).to(dtype).to(dev)
            tag = (hd, Hq, Hk, B, T, dtype, tab, kind)
            assert tower_ops.rope_il_supported(q1, k1, cos, sin), tag
            qe, ke = tower_ops.rope_il_qk(q1, k1, cos, sin)
            qw, kw = mc.apply_rotary_pos_emb(q2, k2, cos, sin)
            assert _same_bits(qe.detach(), qw.detach()) and _same_bits(ke.detach(), kw.detach()), tag
            torch.autograd.backward([qe, ke], [gq, gk])
            torch.autograd.backward([qw, kw], [gq, gk])
            assert _same_bits(buf1.grad, buf2.grad), tag                   # dq | dk in the buffer's columns, zeros under v
            assert float(buf1.grad[..., :(Hq + Hk) * hd].float().abs().max()) > 0.0
            # in place: the un-rotation of the attention node
            a, b = gq.clone(), gk.clone()
            a2, b2 = tower_ops._rope_il_launch(a, b, cos, sin, True, None, in_place=True)
            assert a2 is a and b2 is b
            want = tower_ops._rope_il_launch(gq, gk, cos, sin, True)
            assert _same_bits(a, want[0]) and _same_bits(b, want[1]), tag


@pytest.mark.parametrize("dtype,tab", PAIRS)
@pytest.mark.parametrize("hd", [32, 64, 128])
def test_rotary_row_liveness_is_exact(dev, hd, dtype, tab):
    """Dead (b, t) hold NaN in q, k and the tables of the call with the vector: nothing of them may be loaded; their outputs are zeros
    for every head; live rows carry the bits of the call without the vector, forward and backward."""
    from dalm_amd.models import tower_ops

    for (B, T), (Hq, Hk) in zip(SIZES, HEADS):
        g = torch.Generator().manual_seed(hd + B + T)
        cos, sin = _tables(B, T, hd, "distinct", tab, dev, g)
        _, q, k = _qkv(B, T, Hq, Hk, hd, dtype, dev, g)
        q, k = q.detach(), k.detach()
        dead = _dead_rows(B * T, hd + B).to(dev)
        live = (~dead).to(torch.uint8)
        dead_bt = dead.view(B, T)
        for backward in (False, True):
            want_q, want_k = tower_ops._rope_il_launch(q, k, cos, sin, backward)
            qn, kn, cn, sn = q.clone(), k.clone(), cos.clone(), sin.clone()
            qn.transpose(1, 2)[dead_bt] = float("nan")
            kn.transpose(1, 2)[dead_bt] = float("nan")
            cn[dead_bt] = float("nan")
            sn[dead_bt] = float("nan")
            got_q, got_k = tower_ops._rope_il_launch(qn, kn, cn, sn, backward, live)
            for want, got in ((want_q, got_q), (want_k, got_k)):
                w2, g2 = want.transpose(1, 2).reshape(B * T, -1), got.transpose(1, 2).reshape(B * T, -1)
                assert float(g2[dead].float().abs().max()) == 0.0 and not torch.isnan(g2.float()).any(), (hd, dtype, backward)
                assert _same_bits(w2[~dead], g2[~dead]), (hd, dtype, backward)


# ---- the norm ------------------------------------------------------------------------------------------------------------
def _inputs(R, D, dtype, w_dtype, dev):
    g = torch.Generator().manual_seed(1000 * R + D)
    x = (torch.randn(R, D, generator=g) * 1.5 + 0.3).to(dtype).to(dev)         # a mean: the subtraction is exercised
    w = (1.0 + 0.3 * torch.randn(D, generator=g)).to(w_dtype).to(dev)
    gy = torch.randn(R, D, generator=g).to(dtype).to(dev)
    gh = torch.randn(R, D, generator=g).to(dtype).to(dev)
    return x, w, gy, gh


def _hf_norm(x, w):
    """transformers' CohereLayerNorm.forward on the weight tensor `w` itself (a leaf's .grad is then the chain's weight gradient)."""
    from transformers.models.cohere import modeling_cohere as mc

    return mc.CohereLayerNorm.forward(types.SimpleNamespace(weight=w, variance_epsilon=EPS), x)


def _norm64(x, w):
    """CohereLayerNorm's formula in float64."""
    mean = x.mean(-1, keepdim=True)
    var = (x - mean).pow(2).mean(-1, keepdim=True)
    return w * ((x - mean) * torch.rsqrt(var + EPS))


def _norm_run(fn, x, w, gy, gh):
    """(res, y) = (x, fn(x, w)); gh reaches x through the residual path (None: not at all), gy reaches y."""
    x, w = x.detach().clone().requires_grad_(True), w.detach().clone().requires_grad_(True)
    res, y = fn(x, w)
    if gh is None:
        y.backward(gy.to(y.dtype))
    else:
        torch.autograd.backward([res, y], [gh.to(res.dtype), gy.to(y.dtype)])
    return {"y": y.detach(), "dx": x.grad, "dw": w.grad}


@pytest.mark.parametrize("D,dtype,w_dtype", NORM_CASES)
def test_norm_against_float64_and_the_eager_module(dev, D, dtype, w_dtype):
    from dalm_amd.models import tower_ops

    for R in ROWS:
        x, w, gy, gh = _inputs(R, D, dtype, w_dtype, dev)
        assert tower_ops.cohere_norm_supported(x, w)
        for dres in (gh, None):
            got = _norm_run(lambda x, w: tower_ops.cohere_norm_res(x, w, EPS), x, w, gy, dres)
            ref = _norm_run(lambda x, w: (x.view_as(x), _hf_norm(x, w)), x, w, gy, dres)
            tru = _norm_run(lambda x, w: (x.view_as(x), _norm64(x, w)), x.double(), w.double(), gy.double(),
                            None if dres is None else dres.double())
            tag = f"R{R} D{D} {dtype} w {w_dtype} dres {dres is not None}"
            assert got["y"].dtype == dtype and got["dx"].dtype == dtype and got["dw"].dtype == w_dtype, tag
            for name in ("y", "dx", "dw"):
                _held(f"cohere norm {tag} {name}", got[name], ref[name], tru[name])


def _raw_norm_fwd(x, w, live=None, pad=0):
    """The C entry point with output buffers the test owns: pre-filled, `pad` rows more on either side of what the call may write."""
    from dalm_amd import hip

    R, D = x.shape
    y = torch.full((R + 2 * pad, D), SENTINEL, dtype=x.dtype, device=x.device)
    mean = torch.full((R + 2 * pad,), SENTINEL, dtype=torch.float32, device=x.device)
    rstd = torch.full_like(mean, SENTINEL)
    hip.call("dalm_cohere_norm_fwd", hip.ptr(x), hip.ptr(w), hip.dtype_code(x), hip.dtype_code(w), R, D, EPS, hip.ptr(y[pad:]),
             hip.ptr(mean[pad:]), hip.ptr(rstd[pad:]), hip.ptr(live), hip.stream())
    return y, mean, rstd


def _raw_norm_bwd(gy, x, w, mean, rstd, dres, live=None, pad=0):
    from dalm_amd import hip

    R, D = x.shape
    dx = torch.full((R + 2 * pad, D), SENTINEL, dtype=x.dtype, device=x.device)
    hip.call("dalm_cohere_norm_bwd", hip.ptr(gy), hip.ptr(x), hip.ptr(w), hip.ptr(mean), hip.ptr(rstd), hip.ptr(dres), hip.dtype_code(x),
             hip.dtype_code(w), R, D, hip.ptr(dx[pad:]), hip.ptr(live), hip.stream())
    return dx


def _raw_add3(res, a, b, live=None, pad=0):
    from dalm_amd import hip

    R, D = res.shape
    out = torch.full((R + 2 * pad, D), SENTINEL, dtype=res.dtype, device=res.device)
    hip.call("dalm_add3_live", hip.ptr(res), hip.ptr(a), hip.ptr(b), hip.ptr(out[pad:]), hip.dtype_code(res), R, D, hip.ptr(live),
             hip.stream())
    return out


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


@pytest.mark.parametrize("D,dtype,w_dtype", [(8, torch.bfloat16, torch.bfloat16), (3080, torch.bfloat16, torch.float32),
                                             (4096, torch.bfloat16, torch.bfloat16), (8192, torch.bfloat16, torch.bfloat16),
                                             (256, torch.float32, torch.bfloat16), (4096, torch.float32, torch.float32)])
def test_norm_and_add3_row_liveness_is_exact(dev, D, dtype, w_dtype):
    """Dead rows' inputs are NaN in the calls with the vector: nothing of a dead row may be loaded; their outputs are zeros; live
    rows carry the bits of the call without the vector; two rows in front of and behind every output keep their fill."""
    from dalm_amd.models import tower_ops

    PAD = 2
    for R in ROWS:
        x, w, gy, gh = _inputs(R, D, dtype, w_dtype, dev)
        tag = (R, D, dtype, w_dtype)
        dead = _dead_rows(R, R + D).to(dev)
        live = (~dead).to(torch.uint8)
        want_f = _raw_norm_fwd(x, w, None, PAD)
        mean, rstd = want_f[1][PAD:PAD + R].clone(), want_f[2][PAD:PAD + R].clone()
        want_b = [_raw_norm_bwd(gy, x, w, mean, rstd, dres, None, PAD) for dres in (gh, None)]
        want_a = _raw_add3(x, gy, gh, None, PAD)
        xn, gyn, ghn, mn, rn = [t.clone() for t in (x, gy, gh, mean, rstd)]
        for t in (xn, gyn, ghn, mn, rn):
            t[dead] = float("nan")
        got_f = _raw_norm_fwd(xn, w, live, PAD)
        for name, a, b in zip(("y", "mean", "rstd"), want_f, got_f):
            _dead_zero_live_same(name, a, b, dead, PAD, tag)
        for wdx, dres in zip(want_b, (ghn, None)):
            _dead_zero_live_same("dx", wdx, _raw_norm_bwd(gyn, xn, w, mn, rn, dres, live, PAD), dead, PAD, tag)
        _dead_zero_live_same("add3", want_a, _raw_add3(xn, gyn, ghn, live, PAD), dead, PAD, tag)
        # the autograd functions take the vector as an argument and give the same bits, forward and backward
        xa = xn.clone().requires_grad_(True)
        wa = w.clone().requires_grad_(True)
        res, yy = tower_ops.cohere_norm_res(xa, wa, EPS, live)
        assert _same_bits(yy.detach(), got_f[0][PAD:PAD + R]), tag
        torch.autograd.backward([res, yy], [ghn, gyn])
        assert float(xa.grad[dead].float().abs().max()) == 0.0 and torch.isfinite(wa.grad.float()).all(), tag
        assert _same_bits(xa.grad[~dead], want_b[0][PAD:PAD + R][~dead]), tag
        out = tower_ops.add3_live(xn, gyn, ghn, live)
        assert float(out[dead].float().abs().max()) == 0.0 and _same_bits(out[~dead], (x + gy + gh)[~dead]), tag


# ---- the three-way add ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dtype", ADD_CASES)
def test_add3_live_is_torchs_pair_of_adds_bit_for_bit(dev, D, dtype):
    from dalm_amd.models import tower_ops

    for R in ROWS:
        g = torch.Generator().manual_seed(7 * R + D)
        res = (torch.randn(R, D, generator=g) * 1.5 + 0.3).to(dtype).to(dev)
        a = (torch.randn(R, D, generator=g) * 2.0).to(dtype).to(dev)
        b = torch.randn(R, D, generator=g).to(dtype).to(dev)
        go = torch.randn(R, D, generator=g).to(dtype).to(dev)
        assert tower_ops.add3_live_supported(res, a, b)
        t1 = [t.clone().requires_grad_(True) for t in (res, a, b)]
        out = tower_ops.add3_live(*t1)
        out.backward(go)
        t2 = [t.clone().requires_grad_(True) for t in (res, a, b)]
        want = t2[0] + t2[1] + t2[2]
        want.backward(go)
        tag = (R, D, dtype)
        assert _same_bits(out.detach(), want.detach()), tag
        for p, q in zip(t1, t2):
            assert _same_bits(p.grad, q.grad) and _same_bits(p.grad, go), tag
        y = tower_ops.add3_live(res.view(1, R, D), a.view(1, R, D), b.view(1, R, D))             # leading dimensions are rows
        assert y.shape == (1, R, D) and _same_bits(y.view(R, D), want.detach()), tag


def test_the_tower_calls_vector_is_picked_up(dev):
    from dalm_amd import live_rows
    from dalm_amd.models import tower_ops

    B, T, D = 3, 7, 256
    x, w, gy, gh = _inputs(B * T, D, torch.bfloat16, torch.bfloat16, dev)
    mask = (torch.arange(T).unsqueeze(0) >= (T - torch.tensor([7, 4, 1])).unsqueeze(1)).long().to(dev)
    with live_rows.tower_call(mask, True) as vec:
        assert vec is not None and int(vec.sum()) == 7 + 5 + 2             # a row also matters when the next column is live
        _, y = tower_ops.cohere_norm_res(x.view(B, T, D), w, EPS)
        out = tower_ops.add3_live(x.view(B, T, D), gy.view(B, T, D), gh.view(B, T, D))
    dead = vec == 0
    for t in (y, out):
        assert float(t.reshape(B * T, D)[dead].float().abs().max()) == 0.0
    assert _same_bits(out.reshape(B * T, D)[~dead], (x + gy + gh)[~dead])
    outside = tower_ops.add3_live(x.view(B, T, D), gy.view(B, T, D), gh.view(B, T, D))           # no tower call: every row
    assert _same_bits(outside.reshape(B * T, D), x + gy + gh)


def test_what_the_predicates_decline(dev):
    from dalm_amd.models import tower_ops

    x, w, _, _ = _inputs(5, 64, torch.bfloat16, torch.bfloat16, dev)
    wide = torch.zeros(5, 12288, dtype=torch.bfloat16, device=dev)            # Command-R+'s width: over the norm's cap
    assert not tower_ops.cohere_norm_supported(wide, torch.ones(12288, dtype=torch.bfloat16, device=dev))
    assert tower_ops.add3_live_supported(wide, wide, wide)                    # no cap without a reduction
    assert not tower_ops.cohere_norm_supported(x[:, :60], w[:60]) and not tower_ops.cohere_norm_supported(x.half(), w.half())
    assert not tower_ops.cohere_norm_supported(x, torch.ones(2, 32, dtype=torch.bfloat16, device=dev))     # a [H, hd] q / k norm weight
    assert not tower_ops.add3_live_supported(x, x, x.float()) and not tower_ops.add3_live_supported(x[:, :60], x[:, :60], x[:, :60])
    q, k = torch.zeros(1, 2, 4, 48, dtype=torch.bfloat16, device=dev), torch.zeros(1, 1, 4, 48, dtype=torch.bfloat16, device=dev)
    cos = torch.zeros(1, 4, 48, dtype=torch.bfloat16, device=dev)
    assert not tower_ops.rope_il_supported(q, k, cos, cos)                    # head width 48
    q, k, cos = (torch.zeros(1, 2, 4, 64, device=dev), torch.zeros(1, 1, 4, 64, device=dev),
                 torch.zeros(1, 4, 64, dtype=torch.bfloat16, device=dev))
    assert not tower_ops.rope_il_supported(q, k, cos, cos)                    # bf16 tables beside f32 activations


# ---- the model -----------------------------------------------------------------------------------------------------------
_NORMS = ("norm.weight", "layernorm.weight")
VOCAB = 259
LAYERS = 2


def _tiny():
    from transformers import CohereConfig, CohereForCausalLM

    torch.manual_seed(0)
    cfg = CohereConfig(vocab_size=VOCAB, hidden_size=256, intermediate_size=512, num_hidden_layers=LAYERS, num_attention_heads=4,
                       num_key_value_heads=2, max_position_embeddings=64, tie_word_embeddings=True, pad_token_id=1, bos_token_id=None,
                       eos_token_id=2, logit_scale=0.0625)
    m = CohereForCausalLM(cfg)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith(_NORMS):
                p.add_(0.3 * (2.0 * torch.rand(p.shape) - 1.0))
            p.copy_(p.to(torch.bfloat16).float())              # every copy below holds the SAME (bf16-exact) weights
    return m.train()


def _with_lora(model):
    from dalm_amd.models import lora

    torch.manual_seed(3)                        # lora_A is drawn from the global generator: the same adapters in every copy
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


_SWITCHES = {"dalm_rope_il_qk": "DALM_FAST_ROPE", "dalm_cohere_norm_fwd": "DALM_NORM_KERNEL", "dalm_add3_live": "DALM_NORM_KERNEL"}


def test_tiny_model_with_lora_routed_against_unrouted(dev, monkeypatch):
    """Left-padded rows of lengths 7 / 4 / 1, padded and packed.  fp32: loss and every LoRA gradient of the routed model within 1e-4
    of the unrouted model's.  bf16 autocast: logits / hidden states and every LoRA gradient of the routed model are no further from
    the unrouted fp32 model than twice what the unrouted bf16 model is.  The kernels are counted, and none runs with its switch off."""
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
        loss = (logits.float() * w).sum()
        loss.backward()
        return logits.detach().float() * am[..., None], grads(model), float(loss.detach())

    def hidden_padded(model, dtype):
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
            h = model.base_model(input_ids=ids, attention_mask=am, use_cache=False)[0].reshape(B * T, -1).index_select(0, sel)
        loss = (h.float() * wh).sum()
        loss.backward()
        return h.detach().float()[seen], grads(model), float(loss.detach())

    def hidden_packed(model, dtype):
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
            h = packed.generator_hidden(model, ids, am, rows, cu)[valid]
        loss = (h.float() * wh).sum()
        loss.backward()
        return h.detach().float()[seen], grads(model), float(loss.detach())

    with monkeypatch.context() as mp:                                 # the references: transformers' own code, one eager LoRA
        mp.setattr(lora, "_GROUPS", False)                            # branch per projection
        mp.setattr(lora, "_FUSED", False)
        truth = _cast(_with_lora(copy.deepcopy(base)), dev, torch.float32)
        plain = _cast(_with_lora(copy.deepcopy(base)), dev, torch.bfloat16)
        assert not any(hasattr(l, "_dalm_orig_forward") for l in plain.model.layers)
        t_logits, t_grads, t_loss = padded(truth, torch.float32)
        r_logits, r_grads, _ = padded(plain, torch.bfloat16)
        t_h, t_g, t_hloss = hidden_padded(truth, torch.float32)
        r_h, r_g, _ = hidden_padded(plain, torch.bfloat16)
    names = set(t_grads)
    assert any("lora_A" in n for n in names)

    def routed_model(dtype, swiglu=False):
        from dalm_amd.models import fastpath

        fast = copy.deepcopy(base)
        got = use_generator_fast_paths(fast)
        assert got["use_cohere_layer"] == LAYERS and got["use_cohere_layer_norm"] == 1 and got["use_cohere_attention_node"] == LAYERS
        assert got["use_swiglu_kernel"] == 0 and got["use_hip_attention_backward"] is True
        if swiglu:
            assert fastpath.use_swiglu_kernel(fast, cohere=True) == LAYERS
        return _cast(_with_lora(fast), dev, dtype)

    calls = []
    real_call = hip.call
    monkeypatch.setattr(hip, "call", lambda name, *args: (calls.append(name), real_call(name, *args))[1])

    def ran_routed(tag):
        assert calls.count("dalm_rope_il_qk") == 2 * LAYERS, (tag, calls)           # forward, and the un-rotation of dq / dk
        assert calls.count("dalm_cohere_norm_fwd") == LAYERS + 1, (tag, calls)      # every layer's norm and the final one
        # the final norm and the second layer's; the first layer's input is the frozen embedding: nothing asks for its dx
        assert calls.count("dalm_cohere_norm_bwd") == LAYERS, (tag, calls)
        assert calls.count("dalm_add3_live") == LAYERS, (tag, calls)
        # CohereMLP's SwiGLU route is not in the installer lists (`use_swiglu_kernel(model, cohere=True)` asks for it)
        assert not any(c.startswith("dalm_swiglu") or c.startswith("dalm_linear_live_swiglu") for c in calls), (tag, calls)
        calls.clear()

    # fp32: the norm, the rotation (a node of its own: the attention kernels are bf16) and the add run as kernels
    fast32 = routed_model(torch.float32)
    for name, run, (t_out, t_gr, t_l) in (("padded", padded, (t_logits, t_grads, t_loss)),
                                         ("packed", hidden_packed, (t_h, t_g, t_hloss))):
        out, gr, loss = run(fast32, torch.float32)
        ran_routed(("fp32", name))
        print(f"fp32 {name}: loss {loss:.6f} against {t_l:.6f}; outputs {_rel_norm(out, t_out):.3e}")
        assert abs(loss - t_l) <= 1e-4 * abs(t_l), (name, loss, t_l)
        assert _rel_norm(out, t_out) <= 1e-4, name
        assert set(gr) == names
        for n in sorted(names):
            err = _rel_norm(gr[n], t_gr[n])
            print(f"fp32 {name} {n}: {err:.3e}")
            assert err <= 1e-4, (name, n, err)
    del fast32

    # bf16 autocast
    fast = routed_model(torch.bfloat16)
    assert use_transposed_dgrad(fast) == 2 * 4 + 1                     # o, gate, up, down per layer and the lm_head
    for layer in fast.model.layers:                                    # q | k | v of a Cohere layer form one group
        a = layer.self_attn
        assert a.q_proj._group is not None and a.q_proj._group is a.k_proj._group is a.v_proj._group
        assert len(a.q_proj._group.members) == 3
        assert type(a.o_proj) is FrozenLinearT and type(layer.mlp.gate_proj) is FrozenLinearT
    calls.clear()
    f_logits, f_grads, _ = padded(fast, torch.bfloat16)
    assert calls.count("dalm_attn_gqa_fwd") == LAYERS and calls.count("dalm_attn_gqa_bwd") == LAYERS, calls
    assert any(c.startswith("dalm_lora2_") for c in calls), calls                            # the q|k|v group's kernels
    ran_routed(("bf16", "padded"))
    assert set(f_grads) == names == set(r_grads)
    _held("model padded logits", f_logits, r_logits, t_logits)
    for n in sorted(names):
        _held(f"model padded {n}", f_grads[n], r_grads[n], t_grads[n])
    h, f_g, _ = hidden_packed(fast, torch.bfloat16)
    assert calls.count("dalm_attn_gqa_fwd") == LAYERS and calls.count("dalm_attn_gqa_bwd") == LAYERS, calls
    ran_routed(("bf16", "packed"))
    _held("model packed hidden", h, r_h, t_h)
    for n in sorted(names):
        _held(f"model packed {n}", f_g[n], r_g[n], t_g[n])

    # the MLP route, asked for: the SwiGLU kernels run and the bound holds
    asked = routed_model(torch.bfloat16, swiglu=True)
    calls.clear()
    a_logits, a_grads, _ = padded(asked, torch.bfloat16)
    assert any(c.startswith("dalm_swiglu") or c.startswith("dalm_linear_live_swiglu") for c in calls), calls
    _held("model padded logits, SwiGLU kernels", a_logits, r_logits, t_logits)
    for n in sorted(names):
        _held(f"model padded, SwiGLU kernels {n}", a_grads[n], r_grads[n], t_grads[n])
    del asked

    # each switch off: its kernels do not run (DALM_FAST_ROPE is read at call time, DALM_NORM_KERNEL by the installers)
    for kernel, switch in sorted(_SWITCHES.items()):
        with monkeypatch.context() as mp:
            mp.setenv(switch, "0")
            off = copy.deepcopy(base)
            use_generator_fast_paths(off)
            off = _cast(_with_lora(off), dev, torch.bfloat16)
            calls.clear()
            o_logits, o_grads, _ = padded(off, torch.bfloat16)
            assert kernel not in calls, (kernel, switch, calls)
            assert ("dalm_rope_il_qk" in calls) == (switch != "DALM_FAST_ROPE"), (switch, calls)
            _held(f"model {switch}=0 logits", o_logits, r_logits, t_logits)
    calls.clear()


# ---- one step ------------------------------------------------------------------------------------------------------------
_BUILT = {}


def _cohere_lm():
    """The tiny Cohere with LoRA on q / v (no dropout, lora_B randomised), weights on the bf16 grid; built once on the CPU."""
    if "lm" not in _BUILT:
        _BUILT["lm"] = _with_lora(_tiny())
    return copy.deepcopy(_BUILT["lm"])


def _one_rag_step(batch, mode, precision, dev):
    """tests/test_granite_gpu.py's `_one_rag_step`: tiny BERT retriever + tiny Cohere generator; mode "padded", "packed" or "fused"
    (padded, fuse_lm_head)."""
    from test_causal_retriever_gpu import _GradSnapshot
    from test_qwen3_gpu import _tiny_bert

    from dalm_amd import hip, packed
    from dalm_amd.models import AutoModelForRagE2E
    from dalm_amd.training.step import RagE2EStep

    model = AutoModelForRagE2E.from_modules(_tiny_bert(), _cohere_lm(), None, None, normalize=True, get_peft=None,
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


def test_rag_step_with_a_cohere_generator_packed_and_fused_against_padded(dev):
    """One RAG-e2e step, tiny BERT retriever + tiny Cohere generator (logit_scale 0.0625): the packed step and the padded step with
    fuse_lm_head, each against the padded step that materialises the model's own logits, at the bounds
    `test_rag_step_with_a_granite_generator_packed_and_fused_against_padded` (tests/test_granite_gpu.py) uses: fp32 - loss, gradient
    norm and every gradient within 1e-4; bf16 autocast - loss within 2.5e-4 and gradient norm within 2.2e-3 of the padded bf16 step,
    every parameter's gradient within twice the padded bf16 step's own distance from the fp32 step + 5e-3, and within 4e-2 outright.
    Both other routes multiply the hidden states with lm_head.weight themselves: without the scaling their logits are 16 x too large
    and none of the bounds holds."""
    from test_causal_retriever_gpu import _rag_batch

    batch = _rag_batch(False)
    res = {(m, p): _one_rag_step(batch, m, p, dev) for p in ("fp32", "bf16") for m in ("padded", "packed", "fused")}
    for (m, p), (_, _, calls) in res.items():             # the layer's kernels ran, in f32 and in bf16; the logits scaling each way
        assert calls.count("dalm_cohere_norm_fwd") == LAYERS + 1 and calls.count("dalm_add3_live") == LAYERS, (m, p, calls)
        assert calls.count("dalm_rope_il_qk") == 2 * LAYERS, (m, p, calls)
        assert calls.count("dalm_scale_add") == (0 if m == "padded" else 2), (m, p, calls)
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
