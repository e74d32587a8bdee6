"""OLMo-2 on the GPU: `dalm_norm_add_{fwd,bwd}` and `dalm_row_norm_rope_fwd` / `dalm_row_norm_bwd` (dalm_amd/csrc/tower.hip) against
float64 restatements and against transformers' own chains (Olmo2RMSNorm, the residual add, apply_rotary_pos_emb) on the same
tensors; the fused node `attention.norm_rope_sdpa(..., row_wide=True)`; a tiny OLMo-2 with LoRA, routed against unrouted, padded and
packed; one RAG step with an OLMo-2 generator.

Tolerance rule (tests/test_qwen3_gpu.py's) for every comparison with a rounded side: E_ref is the largest absolute error of
transformers' own sequence in the activation dtype against the truth on the same inputs (float64 for kernels and node, the unrouted
model in float32 for models); the new path's error must be at most 2 E_ref, per tensor.  Zeros in dead rows and "live rows get the
same bits with and without row_live" are exact."""
import copy
import ctypes as C
import types

import pytest
import torch

from test_qwen3_gpu import _attention64, _held, _rel_norm, _rot, _s3, _tables

pytestmark = pytest.mark.gpu

EPS = 1e-6
SENTINEL = 7.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _hf_norm(w, eps=EPS):
    """transformers' Olmo2RMSNorm.forward on the weight tensor `w` itself (a leaf's .grad is then the chain's weight gradient)."""
    from transformers.models.olmo2 import modeling_olmo2 as mo

    me = types.SimpleNamespace(weight=w, variance_epsilon=eps)
    return lambda x: mo.Olmo2RMSNorm.forward(me, x)


def _norm64(x, w, eps=EPS):
    x = x.double()
    rstd = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    return w.double() * (x * rstd), rstd.squeeze(-1)


def _dead_rows(R, seed):
    """About 40 % dead rows, the first and the last among them (one row: it is dead)."""
    dead = torch.rand(R, generator=torch.Generator().manual_seed(seed)) < 0.4
    dead[0] = dead[-1] = True
    return dead


# ---- norm, then add ------------------------------------------------------------------------------------------------------
NORM_ADD_CASES = ([(D, torch.bfloat16, wd) for D in (8, 256, 2048, 3072, 3080, 8192) for wd in (torch.float32, torch.bfloat16)]
                  + [(D, torch.float32, wd) for D in (8, 256, 2048, 3072, 3080) for wd in (torch.float32, torch.bfloat16)])
ROWS = (1, 17, 130)                          # one wave of a workgroup, an odd count, 33 workgroups with a partial last one


def test_norm_add_cases_cover_the_issue_and_the_f32_cap():
    assert {D for D, dt, _ in NORM_ADD_CASES if dt == torch.bfloat16} == {8, 256, 2048, 3072, 3080, 8192}
    assert 8192 > 64 * 4 * 16 >= max(D for D, dt, _ in NORM_ADD_CASES if dt == torch.float32)      # f32 rows hold at most 4096


def _norm_add_inputs(R, D, dtype, w_dtype, dev):
    g = torch.Generator().manual_seed(1000 * R + D)
    x = (torch.randn(R, D, generator=g) * 1.5 + 0.3).to(dtype).to(dev)
    res = torch.randn(R, D, generator=g).to(dtype).to(dev)
    w = (1.0 + 0.3 * torch.randn(D, generator=g)).to(w_dtype).to(dev)
    gy = torch.randn(R, D, generator=g).to(dtype).to(dev)
    return x, res, w, gy


def _norm_add_run(fn, x, res, w, gy):
    x, res, w = [t.detach().clone().requires_grad_(True) for t in (x, res, w)]
    out = fn(x, res, w)
    out.backward(gy.to(out.dtype))
    return {"out": out.detach(), "dx": x.grad, "dres": res.grad, "dw": w.grad}


@pytest.mark.parametrize("D,dtype,w_dtype", NORM_ADD_CASES)
def test_norm_add_against_float64_and_the_eager_pair(dev, D, dtype, w_dtype):
    from dalm_amd.models import tower_ops

    for R in ROWS:
        x, res, w, gy = _norm_add_inputs(R, D, dtype, w_dtype, dev)
        assert tower_ops.norm_add_supported(x, res, w)
        got = _norm_add_run(lambda x, res, w: tower_ops.norm_add(x, res, w, EPS), x, res, w, gy)
        ref = _norm_add_run(lambda x, res, w: res + _hf_norm(w)(x), x, res, w, gy)
        tru = _norm_add_run(lambda x, res, w: res + _norm64(x, w)[0], x.double(), res.double(), w.double(), gy.double())
        assert got["out"].dtype == dtype and got["dx"].dtype == dtype and got["dw"].dtype == w_dtype
        assert torch.equal(got["dres"], gy)                               # the residual's gradient IS the incoming one
        for name in ("out", "dx", "dw"):
            _held(f"norm_add R{R} D{D} {dtype} w {w_dtype} {name}", got[name], ref[name], tru[name])


def _norm_add_raw(x, res, w, gy, live, rstd_in=None):
    """The C entry points with output buffers the test owns (pre-filled: an untouched element shows)."""
    from dalm_amd import hip

    R, D = x.shape
    out, dx = torch.full_like(x, SENTINEL), torch.full_like(x, SENTINEL)
    rstd = torch.full((R,), SENTINEL, dtype=torch.float32, device=x.device)
    hip.call("dalm_norm_add_fwd", hip.ptr(x), hip.ptr(res), hip.ptr(w), hip.dtype_code(x), hip.dtype_code(w), R, D, EPS, hip.ptr(out),
             hip.ptr(rstd), hip.ptr(live), hip.stream())
    hip.call("dalm_norm_add_bwd", hip.ptr(gy), hip.ptr(x), hip.ptr(w), hip.ptr(rstd_in if rstd_in is not None else rstd),
             hip.dtype_code(x), hip.dtype_code(w), R, D, hip.ptr(dx), hip.ptr(live), hip.stream())
    return out, rstd, dx


@pytest.mark.parametrize("D,dtype,w_dtype", [(8, torch.bfloat16, torch.bfloat16), (3080, torch.bfloat16, torch.float32),
                                             (8192, torch.bfloat16, torch.bfloat16), (3072, torch.float32, torch.float32),
                                             (2048, torch.float32, torch.bfloat16), (256, torch.bfloat16, torch.float32)])
def test_norm_add_row_liveness_is_exact(dev, D, dtype, w_dtype):
    """Dead rows' inputs are NaN in the call with the vector: nothing of a dead row may be loaded."""
    for R in ROWS:
        x, res, w, gy = _norm_add_inputs(R, D, dtype, w_dtype, dev)
        want = _norm_add_raw(x, res, w, gy, None)
        dead = _dead_rows(R, R + D).to(dev)
        live = (~dead).to(torch.uint8)
        rstd_in = want[1].clone()
        for t in (x, res, gy, rstd_in):
            t[dead] = float("nan")
        got = _norm_add_raw(x, res, w, gy, live, rstd_in)
        bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
        for name, a, b in zip(("out", "rstd", "dx"), want, got):
            assert float(b[dead].float().abs().max()) == 0.0 and not torch.isnan(b[dead]).any(), (R, name)
            if R > 1:
                va, vb = (a, b) if name == "rstd" else (a.view(bits), b.view(bits))
                assert torch.equal(va[~dead], vb[~dead]), (R, name)
        # the autograd function: the vector of the tower call in progress is picked up, and passing one gives the same
        from dalm_amd.models import tower_ops

        y = tower_ops.norm_add(x, res, w, EPS, live)
        assert torch.equal(y.view(bits), got[0].view(bits))


def test_norm_add_unsupported_tensors(dev):
    from dalm_amd import hip
    from dalm_amd.models import tower_ops

    x, res, w, gy = _norm_add_inputs(5, 64, torch.bfloat16, torch.bfloat16, dev)
    assert not tower_ops.norm_add_supported(x[:, :60], res[:, :60], w[:60])                 # 60 bf16: no multiple of 16 bytes
    assert not tower_ops.norm_add_supported(x, res.float(), w)                               # the sub-block answered in another dtype
    assert not tower_ops.norm_add_supported(x.cpu(), res.cpu(), w.cpu())
    assert not tower_ops.norm_add_supported(x.half(), res.half(), w)
    wide = torch.zeros(2, 8200, dtype=torch.bfloat16, device=dev)
    assert not tower_ops.norm_add_supported(wide, wide, torch.ones(8200, dtype=torch.bfloat16, device=dev))
    out = torch.full_like(wide, SENTINEL)
    with pytest.raises(ValueError, match="code -2"):
        hip.call("dalm_norm_add_fwd", hip.ptr(wide), hip.ptr(wide), hip.ptr(w), hip.BF16, hip.BF16, 2, 8200, EPS, hip.ptr(out),
                 hip.ptr(torch.empty(2, device=dev)), None, hip.stream())
    torch.cuda.synchronize()
    assert float((out.float() - SENTINEL).abs().max()) == 0.0


# ---- q_norm / k_norm over the whole row + rotary --------------------------------------------------------------------------
# (hd, Hq, Hk): rows of 192, 512, 576, 640 and 8192 elements - under, at and over one wave's 16-byte pass of 512, a partial last
# chunk (192, 576, 640), k narrower than q's chunk count (9 / 1, 5 / 1, 64 / 8)
ROW_CASES = [(64, 3, 3), (64, 8, 2), (64, 9, 1), (128, 4, 4), (128, 5, 1), (128, 64, 8)]
ROW_SIZES = [(2, 5), (2, 37)]


def test_row_cases_are_the_widths_the_issue_names():
    assert sorted({Hq * hd for hd, Hq, _ in ROW_CASES}) == [192, 512, 576, 640, 8192]


def _qk(dev, hd, Hq, Hk, B, T, sliced, w_dtype, seed):
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
    wq = (1.0 + 0.3 * (2.0 * torch.rand(Hq * hd, generator=g) - 1.0)).to(w_dtype).to(dev)
    wk = (1.0 + 0.3 * (2.0 * torch.rand(Hk * hd, generator=g) - 1.0)).to(w_dtype).to(dev)
    return q, k, wq, wk


def _flat(x):
    """[B, H, T, hd] view -> [B, T, H hd]: what the projection returned, and what q_norm / k_norm see."""
    B, H, T, hd = x.shape
    return x.transpose(1, 2).reshape(B, T, H * hd)


def _heads(x, H):
    B, T, W = x.shape
    return x.view(B, T, H, W // H).transpose(1, 2)


def _fresh(B, H, T, hd, dev):
    return torch.full((B, T, H, hd), SENTINEL, dtype=torch.bfloat16, device=dev).transpose(1, 2)


def _fwd_raw(q, k, wq, wk, cos, sin, live=None, hd=None, qs=None):
    from dalm_amd import hip

    B, Hq, T, hd_ = q.shape
    Hk = k.shape[1]
    qo, ko = _fresh(B, Hq, T, hd_, q.device), _fresh(B, Hk, T, hd_, q.device)
    rq = torch.full((B, T), SENTINEL, dtype=torch.float32, device=q.device)
    rk = torch.full((B, T), SENTINEL, dtype=torch.float32, device=q.device)
    cs = (C.c_int64 * 2)(cos.stride(0) if cos.shape[0] > 1 else 0, cos.stride(1))
    out = (qo, ko, rq, rk)
    try:
        hip.call("dalm_row_norm_rope_fwd", hip.ptr(q), hip.ptr(k), hip.ptr(wq), hip.ptr(wk), hip.dtype_code(wq), EPS, EPS, hip.ptr(cos),
                 hip.ptr(sin), B, T, Hq, Hk, hd or hd_, qs or _s3(q), _s3(k), _s3(qo), _s3(ko), cs, hip.ptr(qo), hip.ptr(ko), hip.ptr(rq),
                 hip.ptr(rk), hip.ptr(live), hip.stream())
    except ValueError as e:
        return out, str(e)
    return out, None


def _bwd_raw(gq, gk, q, k, wq, wk, rq, rk, live=None, hd=None, gqs=None):
    from dalm_amd import hip

    B, Hq, T, hd_ = q.shape
    Hk = k.shape[1]
    dq, dk = _fresh(B, Hq, T, hd_, q.device), _fresh(B, Hk, T, hd_, q.device)
    try:
        hip.call("dalm_row_norm_bwd", hip.ptr(gq), hip.ptr(gk), hip.ptr(q), hip.ptr(k), hip.ptr(wq), hip.ptr(wk), hip.dtype_code(wq),
                 hip.ptr(rq), hip.ptr(rk), B, T, Hq, Hk, hd or hd_, gqs or _s3(gq), _s3(gk), _s3(q), _s3(k), _s3(dq), _s3(dk), hip.ptr(dq),
                 hip.ptr(dk), hip.ptr(live), hip.stream())
    except ValueError as e:
        return (dq, dk), str(e)
    return (dq, dk), None


@pytest.mark.parametrize("B,T", ROW_SIZES)
@pytest.mark.parametrize("hd,Hq,Hk", ROW_CASES)
def test_row_norm_kernels_against_float64_and_the_eager_chain(dev, hd, Hq, Hk, B, T):
    from transformers.models.olmo2 import modeling_olmo2 as mo

    from dalm_amd.models import tower_ops

    for sliced, cos_b, w_dtype in ((False, 1, torch.bfloat16), (True, B, torch.bfloat16), (True, 1, torch.float32),
                                   (False, B, torch.float32)):
        q, k, wq, wk = _qk(dev, hd, Hq, Hk, B, T, sliced, w_dtype, 1000 * hd + 100 * Hq + 10 * B + T + sliced)
        cos, sin = _tables(B, T, hd, cos_b, dev)
        assert tower_ops.row_norm_rope_supported(q, k, wq, wk, cos, sin)
        (qo, ko, rq, rk), err = _fwd_raw(q, k, wq, wk, cos, sin)
        assert err is None, err
        nq, nk = _hf_norm(wq), _hf_norm(wk)
        with torch.no_grad():                                             # Olmo2Attention's own sequence, eagerly in bf16
            eq, ek = mo.apply_rotary_pos_emb(_heads(nq(_flat(q)), Hq), _heads(nk(_flat(k)), Hk), cos, sin)
        tag = f"hd{hd} H{Hq}/{Hk} B{B} T{T} {'sliced' if sliced else 'dense'} cos{cos_b} w {w_dtype}"
        for name, x, w, H, o, r, e in (("q", q, wq, Hq, qo, rq, eq), ("k", k, wk, Hk, ko, rk, ek)):
            y, rstd = _norm64(_flat(x), w)
            y = _heads(y, H)
            truth = y * cos.double().unsqueeze(1) + _rot(y) * sin.double().unsqueeze(1)
            assert e.dtype == torch.bfloat16
            _held(f"fwd {name} {tag}", o, e, truth)
            # rstd is f32 throughout: fma chains of at most 128 positive terms per lane, a 64-lane tree, the division, the add and
            # the hardware rsqrt (1 ulp); the reciprocal square root halves what the sum carries: well inside 32 x 2^-24 relative
            assert float(((r.double() - rstd) / rstd).abs().max()) <= 32 * 2.0 ** -24, name
        # the launcher the node uses gives the same bits
        lo = tower_ops.row_norm_rope(q, k, wq, wk, EPS, EPS, cos, sin)
        assert torch.equal(lo[0], qo) and torch.equal(lo[1], ko) and torch.equal(lo[2], rq) and torch.equal(lo[3], rk)
        assert lo[0].transpose(1, 2).is_contiguous() and lo[4] is None

        # backward of the norm alone: gradients of the normed, un-rotated values in
        g = torch.Generator().manual_seed(T + hd)
        gq = torch.randn(B, T, Hq, hd, generator=g).bfloat16().to(dev).transpose(1, 2)
        gk = torch.randn(B, T, Hk, hd, generator=g).bfloat16().to(dev).transpose(1, 2)
        (dq, dk), err = _bwd_raw(gq, gk, q, k, wq, wk, rq, rk)
        assert err is None, err
        for name, x, w, go, d, norm in (("q", q, wq, gq, dq, nq), ("k", k, wk, gk, dk, nk)):
            x64 = _flat(x).detach().double().requires_grad_(True)
            w64 = w.detach().double().requires_grad_(True)
            _norm64(x64, w64)[0].backward(_flat(go).double())
            xe = _flat(x).detach().clone().requires_grad_(True)
            we = w.detach().clone().requires_grad_(True)
            norm_e = _hf_norm(we)
            norm_e(xe).backward(_flat(go))
            _held(f"bwd {name} {tag}", _flat(d), xe.grad, x64.grad)
            # the weight gradient the node computes in torch
            dw = tower_ops.row_norm_weight_grad(go, x, rq if name == "q" else rk).to(w.dtype)
            _held(f"dw {name} {tag}", dw, we.grad, w64.grad)
        lo = tower_ops.row_norm_bwd(gq, gk, q, k, wq, wk, rq, rk)
        assert torch.equal(lo[0], dq) and torch.equal(lo[1], dk) and lo[0].transpose(1, 2).is_contiguous()


@pytest.mark.parametrize("B,T", ROW_SIZES)
@pytest.mark.parametrize("hd,Hq,Hk", ROW_CASES)
def test_row_norm_liveness_is_exact(dev, hd, Hq, Hk, B, T):
    """About 40 % dead rows, the first and the last among them; their inputs are NaN: nothing of a dead row may be loaded."""
    q, k, wq, wk = _qk(dev, hd, Hq, Hk, B, T, True, torch.bfloat16, 7 * hd + Hq + B * T)
    cos, sin = _tables(B, T, hd, B, dev)
    g = torch.Generator().manual_seed(B * T)
    gq = torch.randn(B, T, Hq, hd, generator=g).bfloat16().to(dev).transpose(1, 2)
    gk = torch.randn(B, T, Hk, hd, generator=g).bfloat16().to(dev).transpose(1, 2)
    dead = _dead_rows(B * T, B * T + hd).to(dev)
    lv = (~dead).to(torch.uint8)
    dead = dead.view(B, T)
    (qo, ko, rq, rk), err = _fwd_raw(q, k, wq, wk, cos, sin)
    assert err is None, err
    (dq, dk), err = _bwd_raw(gq, gk, q, k, wq, wk, rq, rk)
    assert err is None, err
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


def test_unsupported_row_norm_calls_return_the_error_code_and_write_nothing(dev):
    from dalm_amd.models import tower_ops

    def untouched(bufs):
        torch.cuda.synchronize()
        return all(float((b.float() - SENTINEL).abs().max()) == 0.0 for b in bufs)

    B, T, Hq, Hk = 2, 5, 4, 2
    for hd in (32, 96):
        q, k, wq, wk = _qk(dev, hd, Hq, Hk, B, T, False, torch.bfloat16, hd)
        cos, sin = _tables(B, T, hd, 1, dev)
        assert not tower_ops.row_norm_rope_supported(q, k, wq, wk, cos, sin)
        out, err = _fwd_raw(q, k, wq, wk, cos, sin)
        assert err is not None and "code -2" in err and "head width" in err and untouched(out)
        out, err = _bwd_raw(q, k, q, k, wq, wk, out[2], out[3])
        assert err is not None and "code -2" in err and untouched(out)
    # a row of 65 x 128 = 8320 elements
    q, k, wq, wk = _qk(dev, 128, 65, 1, 1, 2, False, torch.bfloat16, 3)
    cos, sin = _tables(1, 2, 128, 1, dev)
    assert not tower_ops.row_norm_rope_supported(q, k, wq, wk, cos, sin)
    out, err = _fwd_raw(q, k, wq, wk, cos, sin)
    assert err is not None and "code -2" in err and "8192" in err and untouched(out)
    hd = 64
    q, k, wq, wk = _qk(dev, hd, Hq, Hk, B, T, False, torch.bfloat16, 5)
    cos, sin = _tables(B, T, hd, 1, dev)
    rq = torch.ones(B, T, device=dev)
    rk = torch.ones(B, T, device=dev)
    flat = torch.zeros(q.numel() + 8, dtype=torch.bfloat16, device=dev)      # a pointer 2 bytes off a 16-byte boundary
    q_off = flat[1:1 + q.numel()].view(B, T, Hq, hd).transpose(1, 2)
    assert q_off.data_ptr() % 16 == 2 and not tower_ops.row_norm_rope_supported(q_off, k, wq, wk, cos, sin)
    out, err = _fwd_raw(q_off, k, wq, wk, cos, sin)
    assert err is not None and "code -4" in err and untouched(out)
    out, err = _bwd_raw(q_off, k, q, k, wq, wk, rq, rk)
    assert err is not None and "code -4" in err and untouched(out)
    odd = (C.c_int64 * 3)(q.stride(0), q.stride(1), q.stride(2) + 1)         # an odd row stride (never launched)
    out, err = _fwd_raw(q, k, wq, wk, cos, sin, qs=odd)
    assert err is not None and "code -4" in err and untouched(out)
    out, err = _bwd_raw(q, k, q, k, wq, wk, rq, rk, gqs=odd)
    assert err is not None and "code -4" in err and untouched(out)
    assert not tower_ops.row_norm_rope_supported(q, k, wq.float(), wk, cos, sin)             # one dtype for both weights
    assert not tower_ops.row_norm_rope_supported(q, k, wq[:hd], wk[:hd], cos, sin)           # head-wide weights are Qwen3's
    assert not tower_ops.row_norm_rope_supported(q.float(), k.float(), wq, wk, cos.float(), sin.float())
    assert not tower_ops.row_norm_rope_supported(q.cpu(), k.cpu(), wq.cpu(), wk.cpu(), cos.cpu(), sin.cpu())


# ---- the node -----------------------------------------------------------------------------------------------------------
def _packed_setup(dev, hd, T, lens):
    """Sequences of `lens` left-padded to T and packed with multiple 64: (n, descriptor, the dense mask it stands for, cos, sin)."""
    from dalm_amd import packed

    B = len(lens)
    m2 = (torch.arange(T).unsqueeze(0) >= (T - torch.tensor(lens)).unsqueeze(1)).long()
    rows, cu = packed.pack_plan(m2, shifted=True, multiple=64)
    _i, pos, mask, _v = packed.packed_inputs(torch.zeros(B, T, dtype=torch.long, device=dev), m2.to(dev), rows.to(dev), cu.to(dev), True)
    cos, sin = _tables(1, rows.numel(), hd, 1, dev, pos=pos[:1].float())
    sq = packed.packed_of(mask)
    n = rows.numel()
    r = torch.arange(n, device=dev)
    seq = torch.bucketize(r, sq.cu[1:].to(torch.int64), right=True)
    dense = (seq[:, None] == seq[None, :]) & (sq.key_live != 0)[None, :] & (r[None, :] <= r[:, None])
    return n, mask, dense[None, None], cos, sin


NODE_CASES = [("left", 4, 4, 64, 40), ("left", 4, 2, 128, 200), ("causal", 4, 2, 64, 200), ("causal", 4, 4, 128, 40),
              ("packed", 4, 4, 128, 200), ("packed", 4, 2, 64, 40), ("packed", 6, 2, 64, 200)]


@pytest.mark.parametrize("mode,Hq,Hk,hd,T", NODE_CASES)
def test_node_against_float64_and_the_eager_chain(dev, mode, Hq, Hk, hd, T):
    from test_attention_gqa_gpu import _hf_mask
    from transformers.models.olmo2 import modeling_olmo2 as mo

    from dalm_amd.models import attention, tower_ops

    G = Hq // Hk
    if mode == "packed":
        T, mask, dense, cos, sin = _packed_setup(dev, hd, T, [T, T // 4, (2 * T) // 3])
        B, causal = 1, False
    else:
        B = 3
        cos, sin = _tables(B, T, hd, 1, dev)
        mask, causal = (_hf_mask(B, T, [0, T // 2, T // 6], dev), False) if mode == "left" else (None, True)
        dense = mask
    g = torch.Generator().manual_seed(hd + 10 * Hq + len(mode) + T)
    W = (Hq + 2 * Hk) * hd
    buf = (1.5 * torch.randn(B * T, W, generator=g)).bfloat16().to(dev)
    go = torch.randn(B, T, Hq, hd, generator=g).bfloat16().to(dev).transpose(1, 2)
    wq0 = (1.0 + 0.3 * (2.0 * torch.rand(Hq * hd, generator=g) - 1.0)).bfloat16().to(dev)
    wk0 = (1.0 + 0.3 * (2.0 * torch.rand(Hk * hd, generator=g) - 1.0)).bfloat16().to(dev)
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
        assert attention.rope_fusable(q, k, cos, sin) and attention.node_supported(q, k, v, mask, causal)
        assert tower_ops.row_norm_rope_supported(q, k, wq, wk, cos, sin)
        return attention.norm_rope_sdpa(q, k, v, wq, wk, EPS, EPS, cos, sin, mask, scale, causal, row_wide=True)

    def eager(q, k, v, wq, wk):
        qr, kr = mo.apply_rotary_pos_emb(_heads(_hf_norm(wq)(_flat(q)), Hq), _heads(_hf_norm(wk)(_flat(k)), Hk), cos, sin)
        return attention.sdpa(qr, kr, v, mask, scale, causal)

    def truth(q, k, v, wq, wk):
        yq, yk = _heads(_norm64(_flat(q), wq)[0], Hq), _heads(_norm64(_flat(k), wk)[0], Hk)
        c, s = cos.double().unsqueeze(1), sin.double().unsqueeze(1)
        return _attention64(yq * c + _rot(yq) * s, yk * c + _rot(yk) * s, v, dense, causal, scale, G)

    got, ref, tru = run(new, torch.bfloat16), run(eager, torch.bfloat16), run(truth, torch.float64)
    for name in ("out", "dq", "dk", "dv", "dwq", "dwk"):
        _held(f"node {mode} H{Hq}/{Hk} hd{hd} T{T} {name}", got[name], ref[name], tru[name])


# ---- the model -----------------------------------------------------------------------------------------------------------
_NORMS = ("norm.weight", "layernorm.weight")


def _tiny(dev=None):
    from transformers import Olmo2Config, Olmo2ForCausalLM

    torch.manual_seed(0)
    cfg = Olmo2Config(vocab_size=128, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, pad_token_id=1, bos_token_id=None, eos_token_id=2)
    m = Olmo2ForCausalLM(cfg)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith(_NORMS):
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
    if train_norms:                             # the layers' two post-norms and q_norm / k_norm: the torch weight-gradient paths
        for name, p in model.named_parameters():
            if name.endswith(_NORMS) and ".layers." in name:
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
def test_tiny_model_with_lora_routed_against_unrouted(dev, monkeypatch, train_norms):
    from dalm_amd import hip, packed
    from dalm_amd.models import lora
    from dalm_amd.models.frozen_linear import FrozenLinearT, use_transposed_dgrad
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    base = _tiny()
    B, T = 3, 48
    Hq, Hk, hd = 4, 2, 64
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
        assert not any(hasattr(l, "_dalm_orig_forward") for l in plain.model.layers)
        t_logits, t_grads = padded(truth, torch.float32)
        r_logits, r_grads = padded(plain, torch.bfloat16)
        t_h, t_g = hidden_padded(truth, torch.float32)
        r_h, r_g = hidden_padded(plain, torch.bfloat16)

    fast = copy.deepcopy(base)
    routed = use_generator_fast_paths(fast)
    assert routed["use_olmo2_layer"] == 2 and routed["use_olmo2_attention_node"] == 2 and routed["use_swiglu_kernel"] == 2
    assert routed["use_hip_attention_backward"] is True
    fast = _cast(_with_lora(fast, train_norms), dev, torch.bfloat16)
    assert use_transposed_dgrad(fast) == 2 * 4 + 1                     # o, gate, up, down per layer and the lm_head
    for layer in fast.model.layers:                                    # q | k | v of an OLMo-2 layer form one group
        a = layer.self_attn
        assert a.q_proj._group is not None and a.q_proj._group is a.k_proj._group is a.v_proj._group
        assert len(a.q_proj._group.members) == 3
        assert type(a.o_proj) is FrozenLinearT and type(layer.mlp.gate_proj) is FrozenLinearT

    calls, seen_args = [], []
    real_call = hip.call

    def spy(name, *args):
        calls.append(name)
        if name == "dalm_row_norm_rope_fwd":
            seen_args.append((args[0], args[1], list(args[14]), list(args[15])))
        return real_call(name, *args)

    monkeypatch.setattr(hip, "call", spy)
    f_logits, f_grads = padded(fast, torch.bfloat16)
    assert calls.count("dalm_row_norm_rope_fwd") == 2 and calls.count("dalm_row_norm_bwd") == 2, calls   # the node ran, once per layer
    assert calls.count("dalm_norm_add_fwd") == 4 and calls.count("dalm_norm_add_bwd") == 4, calls        # two pairs per layer
    assert calls.count("dalm_attn_gqa_fwd") == 2 and calls.count("dalm_attn_gqa_bwd") == 2
    assert any(c.startswith("dalm_swiglu") or c.startswith("dalm_linear_live_swiglu") for c in calls), calls
    assert any(c.startswith("dalm_lora2_") for c in calls), calls                                 # and the q|k|v group's kernels
    assert all(l.self_attn.q_proj._group.enabled for l in fast.model.layers)
    # q and k reached the row-norm kernel as column slices of the ONE q|k|v GEMM output: k starts Hq hd elements behind q in the
    # same rows, and both walk tokens with the concatenated width as their stride
    for q_ptr, k_ptr, qs, ks in seen_args:
        assert k_ptr - q_ptr == Hq * hd * 2, (q_ptr, k_ptr)
        assert qs[2] == ks[2] == (Hq + 2 * Hk) * hd and qs[1] == ks[1] == hd, (qs, ks)
    names = set(t_grads)
    assert names == set(r_grads) == set(f_grads) and any("lora_A" in n for n in names)
    assert train_norms == any(n.endswith("q_norm.weight") for n in names) == any(n.endswith("post_feedforward_layernorm.weight") for n in names)
    _held("model padded logits", f_logits, r_logits, t_logits)
    for n in sorted(names):
        _held(f"model padded {n}", f_grads[n], r_grads[n], t_grads[n])

    # packed: the generator's decoder stack on the un-padded rows, against the same rows of the padded truth
    calls.clear()
    fast.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        h = packed.generator_hidden(fast, ids, am, rows, cu)[valid]
    (h.float() * wh).sum().backward()
    assert calls.count("dalm_row_norm_rope_fwd") == 2 and calls.count("dalm_row_norm_bwd") == 2, calls
    assert calls.count("dalm_norm_add_fwd") == 4 and calls.count("dalm_norm_add_bwd") == 4, calls
    _held("model packed hidden", h.detach().float()[seen], r_h, t_h)
    f_g = grads(fast)
    for n in sorted(names):
        _held(f"model packed {n}", f_g[n], r_g[n], t_g[n])


# ---- one step ------------------------------------------------------------------------------------------------------------
_BUILT = {}


def _olmo2_lm():
    """The tiny OLMo-2 with LoRA on q / v (no dropout, lora_B randomised), weights on the bf16 grid; built once on the CPU."""
    if "lm" not in _BUILT:
        _BUILT["lm"] = _with_lora(_tiny(), False)
    return copy.deepcopy(_BUILT["lm"])


def _one_rag_step(batch, mode, precision, dev):
    """tests/test_qwen3_gpu.py's `_one_step` for kind "rag": tiny BERT retriever + tiny OLMo-2 generator."""
    from test_causal_retriever_gpu import _GradSnapshot
    from test_qwen3_gpu import _tiny_bert

    from dalm_amd import hip, packed
    from dalm_amd.models import AutoModelForRagE2E
    from dalm_amd.training.step import RagE2EStep

    model = AutoModelForRagE2E.from_modules(_tiny_bert(), _olmo2_lm(), None, None, normalize=True, get_peft=None,
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


def test_rag_step_with_an_olmo2_generator_packed_against_padded(dev):
    """One RAG-e2e step, tiny BERT retriever + tiny OLMo-2 generator, at the bounds tests/test_qwen3_gpu.py's test of the same name
    holds the Qwen3 step to: fp32 - loss, gradient norm and every gradient within 1e-4; bf16 autocast - loss within 2.5e-4 and
    gradient norm within 2.2e-3 of the padded bf16 step, every parameter's gradient within twice the padded bf16 step's own distance
    from the fp32 step + 5e-3, and within 4e-2 outright."""
    from test_causal_retriever_gpu import _rag_batch

    batch = _rag_batch(False)
    res = {(m, p): _one_rag_step(batch, m, p, dev) for p in ("fp32", "bf16") for m in ("padded", "packed")}
    for m in ("padded", "packed"):                    # the fused node and the post-norm pairs ran in both bf16 layouts
        calls = res[m, "bf16"][2]
        assert calls.count("dalm_row_norm_rope_fwd") == 2 and calls.count("dalm_row_norm_bwd") == 2, (m, calls)
        assert calls.count("dalm_norm_add_fwd") == 4 and calls.count("dalm_norm_add_bwd") == 4, (m, calls)
        assert "dalm_row_norm_rope_fwd" not in res[m, "fp32"][2]
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
