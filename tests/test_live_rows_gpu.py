"""Row liveness of the padded step (dalm_amd/live_rows.py, the `dalm_*_live` entry points of include/dalm_hip.h).

Every row-wise kernel is called twice through the same entry point, with the liveness vector and with NULL, and must
  (a) give the same BITS on the rows that matter,
  (b) leave exact zeros in the dead rows of everything it freshly writes (in-place kernels: leave dead rows untouched),
  (c) do both with the dead rows of every input filled with NaN - the proof that dead rows are not read,
  (d) colacc (a reduction over rows): equal the NULL call on inputs whose dead rows were zeroed,
  (e) equal the NULL call when every row is live.
Rows: B = 3 sequences of T = 40 (R = 120: the last 8- / 16-row tile is partial) - one fully live, one left-padded by 23 rows
(the dead run ends inside a 16-row tile), one with only its last token live - plus a hole, a fully dead sequence and the
all-live case, each in the generator (`shifted`) and the retriever form of the helper, which is checked against
`packed.pack_plan`'s keep set.  The step-level test compares skip_dead_rows=True with False over three optimizer steps.
"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

B, T = 3, 40
R = B * T
VARIANTS = ["base", "hole", "seq2_dead", "all_live"]


def _mask(variant, T=T):
    pad = {40: 23, 20: 11, 12: 7}[T]
    m = torch.ones(B, T, dtype=torch.int64)
    m[1, :pad] = 0
    m[2, :-1] = 0
    if variant == "hole":
        m[1, pad + 7:pad + 10] = 0
    elif variant == "seq2_dead":
        m[2] = 0
    elif variant == "all_live":
        m[:] = 1
    return m


@pytest.fixture(scope="module")
def dev():
    from dalm_amd import hip

    hip.load()
    return torch.device("cuda:0")


@pytest.fixture(params=[(v, s) for v in VARIANTS for s in (True, False)], ids=lambda p: f"{p[0]}-{'gen' if p[1] else 'ret'}")
def live(request, dev):
    from dalm_amd import live_rows

    variant, shifted = request.param
    vec = live_rows.live_rows(_mask(variant).to(dev), shifted)
    assert vec.dtype == torch.uint8 and vec.shape == (R,) and vec.is_contiguous()
    return vec


@pytest.mark.parametrize("shifted", [True, False])
@pytest.mark.parametrize("variant", VARIANTS)
def test_helper_is_pack_plans_keep_set(dev, variant, shifted):
    from dalm_amd import live_rows, packed

    m = _mask(variant)
    vec = live_rows.live_rows(m.to(dev), shifted).cpu()
    rows, _ = packed.pack_plan(m, shifted, multiple=1)
    keep = torch.zeros(R, dtype=torch.uint8)
    keep[rows[rows >= 0]] = 1
    assert torch.equal(vec != 0, keep != 0)
    if variant == "base":
        assert int(keep.sum()) == (40 + 17 + 1) + (2 if shifted else 0)       # generator form: rows 22 and 38 carry a label
    with live_rows.tower_call(m.to(dev), shifted) as held:
        assert torch.equal(live_rows.current(R), held) and live_rows.current(R + 1) is None
        with live_rows.tower_call(m.to(dev), shifted, enabled=False):
            assert live_rows.current(R) is None
        assert live_rows.current(R) is held
    assert live_rows.current(R) is None


# ---------------------------------------------------------------------------------------------------------------------
def _nan_dead(t, dead):
    """A copy of a row-wise input ([R, ...]) with its dead rows filled with NaN (0xFF bytes for integer tensors)."""
    t = t.clone()
    if t.is_floating_point():
        t[dead] = float("nan")
    else:
        t[dead] = 255
    return t


def _check(run, rowwise, other, live, fresh, inplace=(), bits=()):
    """run(**inputs, live=vec or None) -> dict of [R, ...] outputs.  `rowwise`: inputs with one row per liveness byte; `other`:
    weights and the like.  `fresh`: outputs that must be zero in dead rows; `inplace`: outputs that keep their input's dead rows
    (name -> input name); `bits`: keep-bit outputs, which need not be written for dead rows.  The row count is the vector's
    (tests/test_lora2_forms_gpu.py brings its own shapes)."""
    R = live.shape[0]
    keep = live != 0
    dead = ~keep
    ref = run(**{k: v.clone() for k, v in rowwise.items()}, **other, live=None)
    out = run(**{k: v.clone() for k, v in rowwise.items()}, **other, live=live)
    nan_in = {k: _nan_dead(v, dead) for k, v in rowwise.items()}
    out_nan = run(**{k: v.clone() for k, v in nan_in.items()}, **other, live=live)
    assert set(fresh) | set(inplace) | set(bits) == set(ref)
    for name in ref:
        assert out[name].shape[0] == R, name
        assert torch.equal(out[name][keep], ref[name][keep]), f"(a) {name}: kept rows differ from the NULL call"
        assert torch.equal(out_nan[name][keep], ref[name][keep]), f"(c) {name}: kept rows differ with NaN in the dead rows"
        if name in fresh:
            assert not out[name][dead].any(), f"(b) {name}: dead rows are not zero"
            assert not out_nan[name][dead].any(), f"(c) {name}: dead rows are not zero with NaN inputs"
            assert torch.isfinite(out_nan[name].float()).all(), f"(c) {name}: not finite"
        elif name in inplace:
            src = rowwise[inplace[name]]
            assert torch.equal(out[name][dead], src[dead]), f"(b) {name}: dead rows of an in-place output were touched"
            assert torch.isfinite(out_nan[name][keep].float()).all(), f"(c) {name}: not finite"
        if bool(keep.all()):
            assert torch.equal(out[name], ref[name]), f"(e) {name}"


# ---------------------------------------------------------------------------------------------------------------------
# SwiGLU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["halves", "contiguous"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_swiglu_skips_dead_rows(dev, live, layout, dtype):
    """C = 136: one 2048-element tile covers ~15 rows, so tiles straddle live and dead rows."""
    from dalm_amd import hip

    C = 136
    g = torch.Generator(device=dev).manual_seed(1)
    gu = torch.randn(R, 2 * C, device=dev, generator=g).to(dtype)
    da = torch.randn(R, C, device=dev, generator=g).to(dtype)

    def run(gu, da, live):
        act, dg, du = (torch.full((R, C), 7.0, dtype=dtype, device=dev) for _ in range(3))
        code = hip.dtype_code(gu)
        if layout == "halves":
            gate, up = gu[:, :C], gu[:, C:]
            hip.call("dalm_swiglu_fwd_2d_live", hip.ptr(gate), hip.ptr(up), hip.ptr(act), code, R, C, 2 * C, 2 * C, C, hip.ptr(live),
                     hip.stream())
            hip.call("dalm_swiglu_bwd_2d_live", hip.ptr(da), hip.ptr(gate), hip.ptr(up), hip.ptr(dg), hip.ptr(du), code, R, C, C, 2 * C,
                     2 * C, C, C, hip.ptr(live), hip.stream())
        else:
            gate, up = gu[:, :C].contiguous(), gu[:, C:].contiguous()
            hip.call("dalm_swiglu_fwd_live", hip.ptr(gate), hip.ptr(up), hip.ptr(act), code, R, C, hip.ptr(live), hip.stream())
            hip.call("dalm_swiglu_bwd_live", hip.ptr(da), hip.ptr(gate), hip.ptr(up), hip.ptr(dg), hip.ptr(du), code, R, C,
                     hip.ptr(live), hip.stream())
        return {"act": act, "dg": dg, "du": du}

    _check(run, {"gu": gu, "da": da}, {}, live, fresh=("act", "dg", "du"))


def test_swiglu_autograd_wrapper_takes_the_vector(dev, live):
    from dalm_amd.models import tower_ops

    C = 136
    g = torch.Generator(device=dev).manual_seed(2)
    gu = torch.randn(B, T, 2 * C, device=dev, generator=g).bfloat16().requires_grad_(True)
    da = torch.randn(B, T, C, device=dev, generator=g).bfloat16()
    outs = []
    for vec in (None, live):
        gu.grad = None
        act = tower_ops.swiglu(gu[..., :C], gu[..., C:], vec)
        act.backward(da)
        outs.append((act.detach().reshape(R, C), gu.grad.reshape(R, 2 * C).clone()))
    keep = live != 0
    for a, b in zip(*outs):
        assert torch.equal(a[keep], b[keep]) and not b[~keep].any()


# ---------------------------------------------------------------------------------------------------------------------
# RMSNorm
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("add", [True, False])
@pytest.mark.parametrize("D,dtype", [(72, torch.bfloat16), (4096, torch.bfloat16), (72, torch.float32), (4096, torch.float32)])
def test_rms_norm_skips_dead_rows(dev, live, D, dtype, add):
    from dalm_amd.models import tower_ops

    g = torch.Generator(device=dev).manual_seed(3)
    x, delta, dy, dres = (torch.randn(R, D, device=dev, generator=g).to(dtype) for _ in range(4))
    w = (1.0 + 0.1 * torch.randn(D, device=dev, generator=g)).to(dtype)

    def run(x, delta, dy, dres, w, live):
        h, y, rstd = tower_ops._norm_fwd(x, delta if add else None, w, 1e-5, live)
        out = {"y": y, "rstd": rstd.unsqueeze(1).clone()}
        saved = h if add else x
        if live is not None:                       # what the forward kept for its backward: dead rows poisoned, they are not read
            saved, rstd = saved.clone(), rstd.clone()
            saved[live == 0] = float("nan")
            rstd[live == 0] = float("nan")
        out["dx"] = tower_ops._norm_bwd(dy, saved, w, rstd, dres if add else None, live)
        if add:
            out["h"] = h
        return out

    _check(run, {"x": x, "delta": delta, "dy": dy, "dres": dres}, {"w": w}, live,
           fresh=("y", "rstd", "dx") + (("h",) if add else ()))


# ---------------------------------------------------------------------------------------------------------------------
# rotary embedding
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("hd,dtype", [(128, torch.bfloat16), (64, torch.bfloat16), (64, torch.float32)])
def test_rope_skips_dead_rows(dev, live, hd, dtype, backward):
    from dalm_amd.models import tower_ops

    H = 2
    g = torch.Generator(device=dev).manual_seed(4)
    q, k = (torch.randn(R, H * hd, device=dev, generator=g).to(dtype) for _ in range(2))
    cs = torch.randn(R, 2 * hd, device=dev, generator=g).to(dtype)         # per-(b, t) tables: a dead row's are not read either

    def run(q, k, cs, live):
        q4, k4 = (t.view(B, T, H, hd).transpose(1, 2) for t in (q, k))       # the [B, H, T, hd] views transformers hands over
        cos, sin = cs[:, :hd].contiguous().view(B, T, hd), cs[:, hd:].contiguous().view(B, T, hd)
        qo, ko = tower_ops._rope_launch(q4, k4, cos, sin, backward, live)
        return {"q": qo.transpose(1, 2).reshape(R, H * hd), "k": ko.transpose(1, 2).reshape(R, H * hd)}

    _check(run, {"q": q, "k": k, "cs": cs}, {}, live, fresh=("q", "k"))


# ---------------------------------------------------------------------------------------------------------------------
# LoRA
# ---------------------------------------------------------------------------------------------------------------------
LORA_CASES = [(1, 8), (1, 16), (2, 8), (3, 8), (3, 16)]


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("mode,rank", LORA_CASES)
def test_lora_rowdot_skips_dead_rows(dev, live, mode, rank, p):
    """K = 64: two 32-column MFMA steps.  Dead rows: z zero, x not read; their keep bits need not be written."""
    from dalm_amd.models import lora_ops

    K = 64
    g = torch.Generator(device=dev).manual_seed(5)
    x0, x1 = (torch.randn(R, K, device=dev, generator=g).bfloat16() for _ in range(2))
    W = [torch.randn(rank, K, device=dev, generator=g) for _ in range(2)]
    n = 1 if mode == 1 else 2

    def run(x0, x1, live):
        xs = [x0, x1] if mode == 3 else [x0]
        zs, bits = lora_ops.rowdot2(xs, W[:n], rank, 1.0 / (1.0 - p), p, [11, 12][:n], mode, live)
        out = {f"z{i}": z for i, z in enumerate(zs)}
        if p > 0:
            out.update({f"bits{i}": b for i, b in enumerate(bits)})
        return out

    names = [f"z{i}" for i in range(n)]
    _check(run, {"x0": x0, "x1": x1}, {}, live, fresh=names, bits=[f"bits{i}" for i in range(n)] if p > 0 else ())


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("C", [544, 256])
@pytest.mark.parametrize("mode,rank", LORA_CASES)
def test_lora_rankupd_skips_dead_rows(dev, live, mode, rank, C, masked):
    """C = 544: one full 512-column slab and a partial one (mask bytes read per lane); C = 256: the mask bytes staged in LDS.
    In place: dead rows of y stay as they were, their z rows and mask bytes are not read."""
    from dalm_amd.models import lora_ops

    g = torch.Generator(device=dev).manual_seed(6)
    y0, y1 = (torch.randn(R, C, device=dev, generator=g).bfloat16() for _ in range(2))
    z0, z1 = (torch.randn(R, rank, device=dev, generator=g) for _ in range(2))
    b0, b1 = (torch.randint(0, 256, (R, C // 8), device=dev, generator=g, dtype=torch.uint8) for _ in range(2))
    W = [torch.randn(rank, C, device=dev, generator=g) for _ in range(2)]
    n = 1 if mode == 1 else 2

    def run(y0, y1, z0, z1, b0, b1, live):
        ys = [y0, y1] if mode == 3 else [y0]
        lora_ops.rankupd2_(ys, [z0, z1][:n], W[:n], [b0, b1][:n] if masked else None, rank, 0.5, mode, live)
        return {f"y{i}": y for i, y in enumerate(ys)}

    ins = {"y0": y0, "y1": y1, "z0": z0, "z1": z1, "b0": b0, "b1": b1}
    _check(run, ins, {}, live, fresh=(), inplace={f"y{i}": f"y{i}" for i in range(2 if mode == 3 else 1)})


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("C", [544, 256])
@pytest.mark.parametrize("mode,rank", LORA_CASES)
def test_lora_colacc_adds_dead_rows_as_zeros(dev, live, mode, rank, C, masked):
    """(d): the sum over rows with the vector == the NULL call on inputs whose dead rows were zeroed - same row partition (two
    splits at R = 120), same order - also with NaN in the dead rows of x, z and the mask bytes."""
    from dalm_amd.models import lora_ops

    g = torch.Generator(device=dev).manual_seed(7)
    x0, x1 = (torch.randn(R, C, device=dev, generator=g).bfloat16() for _ in range(2))
    z0, z1 = (torch.randn(R, rank, device=dev, generator=g) for _ in range(2))
    b0, b1 = (torch.randint(0, 256, (R, C // 8), device=dev, generator=g, dtype=torch.uint8) for _ in range(2))
    n = 1 if mode == 1 else 2
    keep = live != 0

    def run(x0, x1, z0, z1, b0, b1, live):
        xs = [x0, x1] if mode == 3 else [x0]
        return lora_ops.colacc2(xs, [z0, z1][:n], [b0, b1][:n] if masked else None, rank, 0.5, mode, live)

    ins = {"x0": x0, "x1": x1, "z0": z0, "z1": z1, "b0": b0, "b1": b1}
    zeroed = {k: v.clone() for k, v in ins.items()}
    for v in zeroed.values():
        v[~keep] = 0
    ref = run(**zeroed, live=None)
    out = run(**ins, live=live)
    out_nan = run(**{k: _nan_dead(v, ~keep) for k, v in ins.items()}, live=live)
    for r, o, on in zip(ref, out, out_nan):
        assert torch.isfinite(on).all()
        assert torch.equal(o, r), "(d) differs from the NULL call on zeroed inputs"
        assert torch.equal(on, r), "(c) differs with NaN in the dead rows"
    if bool(keep.all()):
        for r, o in zip(run(**ins, live=None), out):
            assert torch.equal(o, r), "(e)"


# ---------------------------------------------------------------------------------------------------------------------
# BERT dropout + residual add + LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.0])
def test_bert_add_norm_skips_dead_rows(dev, live, p):
    from dalm_amd import hip
    from dalm_amd.models import lora_ops

    D = 1024
    g = torch.Generator(device=dev).manual_seed(8)
    a = torch.randn(R, D, device=dev, generator=g).bfloat16()
    res, g32 = (torch.randn(R, D, device=dev, generator=g) for _ in range(2))
    g16 = torch.randn(R, D, device=dev, generator=g).bfloat16()
    w, b = 1.0 + 0.1 * torch.randn(D, device=dev, generator=g), 0.1 * torch.randn(D, device=dev, generator=g)
    seed = lora_ops.dropout_seed(dev)

    def run(a, res, g32, g16, live):
        y32, d_res = torch.full((R, D), 7.0, device=dev), torch.full((R, D), 7.0, device=dev)
        y16, d_a = torch.full((R, D), 7.0, device=dev, dtype=torch.bfloat16), torch.full((R, D), 7.0, device=dev, dtype=torch.bfloat16)
        mean, rstd = torch.full((R,), 7.0, device=dev), torch.full((R,), 7.0, device=dev)
        bits = torch.zeros(R, D // 8, dtype=torch.uint8, device=dev) if p > 0 else None
        hip.call("dalm_bert_add_norm_fwd_live", hip.ptr(a), hip.ptr(res), hip.ptr(w), hip.ptr(b), 0, R, D, 1e-12, p,
                 hip.ptr(seed) if p > 0 else None, 77, hip.ptr(y32), hip.ptr(y16), hip.ptr(bits), hip.ptr(mean), hip.ptr(rstd),
                 hip.ptr(live), hip.stream())
        out = {"y32": y32, "y16": y16, "mean": mean.unsqueeze(1).clone(), "rstd": rstd.unsqueeze(1).clone()}
        if live is not None:                       # the backward must not read the dead rows' statistics and keep bits either
            if p > 0:
                bits[live == 0] = 255
            mean[live == 0] = float("nan")
            rstd[live == 0] = float("nan")
        hip.call("dalm_bert_add_norm_bwd_live", hip.ptr(g32), hip.ptr(g16), hip.ptr(a), hip.ptr(res), hip.ptr(w), 0, hip.ptr(bits),
                 hip.ptr(mean), hip.ptr(rstd), R, D, p, hip.ptr(d_res), hip.ptr(d_a), hip.ptr(live), hip.stream())
        out.update({"d_res": d_res, "d_a": d_a})
        if p > 0:
            out["bits"] = bits
        return out

    _check(run, {"a": a, "res": res, "g32": g32, "g16": g16}, {}, live, fresh=("y32", "y16", "mean", "rstd", "d_res", "d_a"),
           bits=("bits",) if p > 0 else ())


# ---------------------------------------------------------------------------------------------------------------------
# the step: skip_dead_rows=True against False
# ---------------------------------------------------------------------------------------------------------------------
_TOWERS = {}


def _towers():
    """Two-layer towers of real head widths, built once on the CPU: Llama 256 = 2 heads of 128, BERT 128 = 2 heads of 64."""
    if not _TOWERS:
        from transformers import BertConfig, BertModel, LlamaConfig, LlamaForCausalLM

        from dalm_amd.models import lora
        from dalm_amd.models.lora import LoRALinear

        torch.manual_seed(1234)
        retriever = BertModel(BertConfig(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                                         vocab_size=512, max_position_embeddings=64, hidden_dropout_prob=0.1,
                                         attention_probs_dropout_prob=0.1))
        generator = LlamaForCausalLM(LlamaConfig(hidden_size=256, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2,
                                                 intermediate_size=688, vocab_size=512, max_position_embeddings=64,
                                                 attention_dropout=0.0, pad_token_id=0))
        lora.inject_lora(retriever, ["key", "query", "value"])
        lora.inject_lora(generator, ["q_proj", "v_proj"])
        g = torch.Generator().manual_seed(99)
        for mod in (retriever, generator):
            for m in mod.modules():
                if isinstance(m, LoRALinear):      # lora_B starts at zero, which zeroes every lora_A gradient
                    with torch.no_grad():
                        m.lora_B["default"].weight.copy_(0.05 * torch.randn(m.lora_B["default"].weight.shape, generator=g))
        _TOWERS["r"], _TOWERS["g"] = retriever, generator
    return copy.deepcopy(_TOWERS["r"]), copy.deepcopy(_TOWERS["g"])


def _batch(dev):
    g = torch.Generator().manual_seed(5)
    gm = _mask("base", 40)
    return {k: v.to(dev) for k, v in {
        "retriever_query_input_ids": torch.randint(5, 512, (B, 12), generator=g),
        "retriever_query_attention_mask": _mask("base", 12),
        "retriever_passage_input_ids": torch.randint(5, 512, (B, 20), generator=g),
        "retriever_passage_attention_mask": _mask("base", 20),
        "generator_input_input_ids": torch.randint(5, 512, (B, 40), generator=g),
        "generator_input_attention_mask": gm,
        "query_passage_input_len": torch.tensor([30, 10, 1]),
    }.items()}


def _run_steps(dev, skip, graph_towers):
    from dalm_amd.models import AutoModelForRagE2E, lora_ops
    from dalm_amd.training.step import RagE2EStep

    from dalm_amd.models.lora import LoRALinear

    r, g = _towers()
    # the attention / add-norm dropout sites number themselves from this counter on their first masked call (lora.dropout_uid):
    # both runs must hand out the same numbers, or they would draw different masks
    LoRALinear._count = 100000
    model = AutoModelForRagE2E.from_modules(r, g, None, None, normalize=True, get_peft=None).to(dev)
    for p in model.parameters():
        if not p.requires_grad:
            p.data = p.data.to(torch.bfloat16)
    model.train()
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    opt = torch.optim.Adam([p for _, p in named], lr=1e-3)
    lora_ops.dropout_seed(dev).fill_(0x1234567)            # the same dropout seed word for both runs ...
    torch.manual_seed(4321)                                # ... and the same torch stream (BERT's embedding dropout is torch's)
    step = RagE2EStep(model, opt, None, 100, autocast_dtype=torch.bfloat16, inplace_grad=True, overlap_towers=True,
                      graph_towers=graph_towers, graph_after=0, skip_dead_rows=skip)
    batch = _batch(dev)
    losses = [step(batch).clone() for _ in range(3)]
    torch.cuda.synchronize()
    if graph_towers:
        assert step.towers is not None and not step.towers_failed, "the tower graphs did not run"
    params = {n: p.detach().clone() for n, p in named}
    return torch.stack(losses), params


@pytest.mark.parametrize("graph_towers", [False, True], ids=["eager", "tower_graphs"])
def test_step_is_bit_identical_with_and_without_dead_rows(dev, graph_towers):
    """bf16 autocast, train(), LoRA / hidden / attention dropout on, Adam: three steps from identical weights and the same
    dropout seed word - every loss and every trainable parameter after step 3 is the same with the dead rows skipped."""
    loss_skip, p_skip = _run_steps(dev, True, graph_towers)
    loss_full, p_full = _run_steps(dev, False, graph_towers)
    assert torch.isfinite(loss_skip).all()
    assert torch.equal(loss_skip, loss_full), (loss_skip.tolist(), loss_full.tolist())
    assert set(p_skip) == set(p_full) and len(p_skip) > 0
    moved = 0
    r0, g0 = _towers()
    init = {("retriever_model." + n): p for n, p in r0.named_parameters()}
    init.update({("generator_model." + n): p for n, p in g0.named_parameters()})
    for n in p_skip:
        assert torch.equal(p_skip[n], p_full[n]), n
        if n in init:
            moved += int(not torch.equal(p_skip[n].cpu(), init[n].detach()))
    assert moved > 0 or not any(n in init for n in p_skip)      # the optimizer did move the adapters
