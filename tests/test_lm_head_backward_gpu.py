"""SURVEY 8 f1, the training direction: lm_head + marginalised cross-entropy + d(hidden) through the hand-written bf16 MFMA
kernels (`dalm_lm_head_lse_fwd`, `dalm_lm_head_dlogits`, `dalm_transpose_bf16`, `dalm_lm_head_dhidden`) - nothing of size
[rows, V] is ever allocated.  Stands in for `logits = lm_head(hidden)` + `compute_marginalized_loss_from_logits(...).backward()`
(dalm/models/rag_e2e_base_model.py:104-106, dalm/training/utils/train_utils.py:113-138) when the head is frozen (LoRA).

* the backward kernels against a float64 evaluation of  dh = sum_c coef (softmax - onehot) W  (ragged rows / vocabulary,
  several chunks, labels in every tile, rows without loss);
* `rag_e2e_loss_from_hidden` through the kernels against the fp64 oracle and against the chunked library path
  (`closed_chunked` of the repo: torch.mm + the CE kernel), all rows and live rows;
* the same at the full cfg3 (Llama-2-7b head, 32000 x 4096) and cfg5 (Falcon-7B head, 65024 x 4544) sizes."""
import os
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "oracle"))
sys.path.insert(0, str(Path(__file__).resolve().parent))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def test_transpose_bf16_is_exact(dev):
    from dalm_amd import hip

    for rows, cols, ld_dst in ((100, 64, 128), (4099, 512, 4160), (256, 4544, 256), (1, 64, 64)):
        src = torch.randn(rows, cols, generator=torch.Generator().manual_seed(rows)).bfloat16().to(dev)
        dst = torch.full((cols, ld_dst), 7.0, device=dev, dtype=torch.bfloat16)
        hip.call("dalm_transpose_bf16", hip.ptr(src), rows, cols, cols, hip.ptr(dst), ld_dst, hip.stream())
        assert torch.equal(dst[:, :rows], src.t())
        assert float(dst[:, rows:].abs().sum()) == 0.0


@pytest.mark.parametrize("R,V,K,chunk", [(128, 256, 64, None), (200, 1000, 128, 512), (1, 130, 64, None), (333, 4099, 512, 1024),
                                         (640, 32000, 1024, 8192), (300, 5000, 4544, 2048)])
def test_backward_kernels_vs_fp64(dev, R, V, K, chunk):
    from dalm_amd.ops import default_ops

    g = torch.Generator().manual_seed(R * 7 + V)
    h = (0.5 * torch.randn(R, K, generator=g)).to(torch.bfloat16)
    W = (0.5 * torch.randn(V, K, generator=g) / (K / 64) ** 0.5).to(torch.bfloat16)
    labels = torch.randint(0, V, (R,), generator=g)
    coef = torch.rand(R, generator=g) / R
    labels[::5] = -1
    coef[::5] = 0.0
    if R > 3:
        labels[1], labels[2], labels[3] = 0, V - 1, min(V - 1, 257)
    ops = default_ops()
    lse, _ = ops.lm_head_lse(h.to(dev), W.to(dev), labels.to(dev))
    dh = ops.lm_head_backward(h.to(dev), W.to(dev), labels.to(dev), lse, coef.to(dev), chunk_cols=chunk)
    x = h.double() @ W.double().t()
    sm = torch.softmax(x, dim=1)
    onehot = torch.zeros_like(sm)
    live = labels >= 0
    onehot[live, labels[live]] = 1.0
    dl = coef.double().unsqueeze(1) * (sm - onehot)
    ref = dl @ W.double()
    # the staged gradient is rounded to bf16 once (as the logits' gradient is on the reference's bf16 path); the same rounding
    # applied to the fp64 gradient bounds what that costs
    ref_b = dl.to(torch.bfloat16).double() @ W.double()
    cost = _rel(ref_b, ref)
    got = _rel(dh, ref)
    assert got < 6e-3 and got < 2.0 * cost + 2e-3, (got, cost)
    assert float(dh.cpu()[~live].abs().max() if (~live).any() else 0.0) == 0.0          # rows without loss: exactly zero
    again = ops.lm_head_backward(h.to(dev), W.to(dev), labels.to(dev), lse, coef.to(dev), chunk_cols=chunk)
    assert torch.equal(again, dh)                                                       # fixed summation order


def _batch(B, Tg, H, V, D, seed, dev, pad_left=True):
    g = torch.Generator().manual_seed(seed)
    glen = torch.randint(Tg // 4, Tg + 1, (B, 1), generator=g)
    glen[0] = Tg
    ar = torch.arange(Tg).unsqueeze(0)
    mask = ((ar >= (Tg - glen)) if pad_left else (ar < glen)).long()
    ids = torch.randint(0, V, (B, Tg), generator=g)
    qlen = (glen.squeeze(1).float() * 0.7).long().clamp(min=1)
    q = torch.nn.functional.normalize(torch.randn(B, D, generator=g), dim=1)
    p = torch.nn.functional.normalize(torch.randn(B, D, generator=g), dim=1)
    h = torch.randn(B, Tg, H, generator=g).bfloat16()
    W = (torch.randn(V, H, generator=g) / H ** 0.5 * 2.0).bfloat16()
    return [t.to(dev) for t in (q, p, h, W, ids, mask, qlen)]


def _run(q, p, h, W, ids, mask, qlen, live, kernel: bool):
    from dalm_amd.fused import rag_e2e_loss_from_hidden

    os.environ["DALM_LM_HEAD_TRAIN_KERNEL"] = kernel if isinstance(kernel, str) else ("1" if kernel else "0")
    try:
        qq, pp, hh = [t.clone().requires_grad_(True) for t in (q, p, h)]
        aux = {}
        loss = rag_e2e_loss_from_hidden(qq, pp, hh, W, ids, mask, qlen, 100.0, live_rows=live, aux=aux)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach(), qq.grad, pp.grad, hh.grad, aux
    finally:
        os.environ.pop("DALM_LM_HEAD_TRAIN_KERNEL", None)


@pytest.mark.parametrize("use_live", [False, True])
def test_training_through_the_kernels_vs_fp64_oracle_and_library_path(dev, use_live):
    import dalm_oracle as O

    from dalm_amd.fused import live_row_index

    B, Tg, H, V, D = 8, 96, 128, 3000, 64
    q, p, h, W, ids, mask, qlen = _batch(B, Tg, H, V, D, 11, dev)
    live = live_row_index(mask, multiple=64).to(dev) if use_live else None
    loss_k, dq_k, dp_k, dh_k, _ = _run(q, p, h, W, ids, mask, qlen, live, True)
    loss_l, dq_l, dp_l, dh_l, _ = _run(q, p, h, W, ids, mask, qlen, live, False)
    h64 = h.double().cpu().requires_grad_(True)
    q64, p64 = q.double().cpu().requires_grad_(True), p.double().cpu().requires_grad_(True)
    ref = O.ref_step_loss(q64, p64, h64 @ W.double().cpu().t(), ids.cpu(), mask.cpu(), qlen.cpu(), 100)
    ref["loss"].backward()
    # the kernels keep the logits in f32 (the library path rounds them to bf16 first): closer to fp64 than the library path
    assert abs(float(loss_k) - float(ref["loss"])) <= 2e-5 * abs(float(ref["loss"]))
    assert abs(float(loss_l) - float(ref["loss"])) <= 2e-3 * abs(float(ref["loss"]))
    for name, got, lib, want in (("dq", dq_k, dq_l, q64.grad), ("dp", dp_k, dp_l, p64.grad), ("dh", dh_k, dh_l, h64.grad)):
        e_k, e_l = _rel(got, want), _rel(lib, want)
        assert e_k < 6e-3 and e_k < 1.5 * e_l + 1e-3, (name, e_k, e_l)
    dead = (torch.cat((mask[:, 1:], torch.zeros_like(mask[:, :1])), 1) == 0)
    assert float(dh_k[dead].abs().max()) == 0.0


@pytest.mark.parametrize("cfg,V,H", [("cfg3", 32000, 4096), ("cfg5", 65024, 4544)])
def test_full_size_heads_match_the_chunked_library_path(dev, cfg, V, H):
    """B = 18, Tg = 256 (BASELINE configs 3 and 5): loss and d(hidden) of the kernel path against the repo's chunked library
    path (torch.mm + the fused CE kernel, what `--fuse-lm-head` ran through round 4), over the live rows as bench.py uses them;
    every element of d(hidden) is compared.  Written to profiles/ by tools/lm_head_train_bench.py with its times."""
    from dalm_amd.fused import gemm_wave_rows, live_row_index

    B, Tg, D = 18, 256, 1024
    q, p, h, W, ids, mask, qlen = _batch(B, Tg, H, V, D, 3 if cfg == "cfg3" else 5, dev)
    live = live_row_index(mask, multiple=gemm_wave_rows(V)).to(dev)
    loss_k, _, _, dh_k, _ = _run(q, p, h, W, ids, mask, qlen, live, True)
    loss_l, _, _, dh_l, _ = _run(q, p, h, W, ids, mask, qlen, live, False)
    assert abs(float(loss_k) - float(loss_l)) <= 1e-3 * abs(float(loss_l))
    # the two paths round different things to bf16 (the library: logits and their gradient; the kernels: the gradient only)
    assert _rel(dh_k, dh_l) < 8e-3
    assert float((dh_k.float() - dh_l.float()).abs().max()) <= 0.05 * float(dh_l.float().abs().max())
    dead = (torch.cat((mask[:, 1:], torch.zeros_like(mask[:, :1])), 1) == 0)
    assert float(dh_k[dead].abs().max()) == 0.0


@pytest.mark.parametrize("cfg,V,H", [("cfg3", 32000, 4096), ("cfg5", 65024, 4544), ("small", 3008, 128)])
def test_two_contraction_kernels_match_the_library_path(dev, cfg, V, H):
    """Round 6: the hand-written head WITHOUT the third contraction (DALM_LM_HEAD_TRAIN_KERNEL=2: `dalm_lm_head_logits` stores the
    bf16 logits of a row chunk, the fused CE kernel turns them into d(logits) in place, `dalm_lm_head_dhidden` contracts them) -
    the same algorithm as the library path (torch.mm x 2 around the same CE kernel), so the two agree to the summation order of
    the two GEMMs: loss and every element of d(hidden)."""
    from dalm_amd.fused import gemm_wave_rows, live_row_index

    B, Tg, D = (18, 256, 1024) if cfg != "small" else (6, 64, 64)
    q, p, h, W, ids, mask, qlen = _batch(B, Tg, H, V, D, 7, dev)
    live = live_row_index(mask, multiple=gemm_wave_rows(V) if cfg != "small" else 64).to(dev)
    loss_k, dq_k, dp_k, dh_k, _ = _run(q, p, h, W, ids, mask, qlen, live, "2")
    loss_l, dq_l, dp_l, dh_l, _ = _run(q, p, h, W, ids, mask, qlen, live, "0")
    assert abs(float(loss_k) - float(loss_l)) <= 2e-5 * abs(float(loss_l))
    assert _rel(dh_k, dh_l) < 4e-3                     # bf16 logits rounded from differently ordered f32 sums; dh rounded once
    assert _rel(dq_k, dq_l) < 1e-4 and _rel(dp_k, dp_l) < 1e-4
    dead = (torch.cat((mask[:, 1:], torch.zeros_like(mask[:, :1])), 1) == 0)
    assert float(dh_k[dead].abs().max()) == 0.0


# ---------------------------------------------------------------------------
# every (selection, engine) pair `fused._lm_head_engine` can name for a frozen bf16 head: forced through the two variables, run,
# and compared with `rag_e2e_loss` on the materialised logits of the same bf16 values
# ---------------------------------------------------------------------------
_PAIRS = {   # (selection, engine, gradient wanted) -> (DALM_LM_HEAD_KERNEL, DALM_LM_HEAD_TRAIN_KERNEL)
    ("all", "recompute", True): (None, "1"), ("all", "sample_chunks", True): (None, "0"),
    ("live", "recompute", True): (None, None), ("live", "logits_rows", True): (None, "2"), ("live", "mm_rows", True): (None, "0"),
    ("packed", "recompute", True): (None, "1"), ("packed", "logits_rows", True): (None, "2"), ("packed", "mm_rows", True): (None, None),
    ("all", "lse", False): ("1", None), ("all", "sample_chunks", False): ("0", None),
    ("live", "lse", False): ("1", None), ("live", "mm_rows", False): ("0", None), ("packed", "mm_rows", False): ("1", None),
}
_PAIR_SHAPES = dict(B=4, Tg=64, H=64, V=512, D=32)
_PAIR_CACHE = {}


def _pair_batch(dev):
    """Left padding; sample 0 is full, sample 1 has a single live token.  Built once, never written to."""
    if "batch" not in _PAIR_CACHE:
        from dalm_amd.fused import live_row_index, rag_e2e_loss
        from dalm_amd.packed import packed_labels

        B, Tg, H, V, D = (_PAIR_SHAPES[k] for k in ("B", "Tg", "H", "V", "D"))
        g = torch.Generator().manual_seed(23)
        glen = torch.tensor([Tg, 1, 23, 39]).unsqueeze(1)
        mask = (torch.arange(Tg).unsqueeze(0) >= (Tg - glen)).long()
        ids = torch.randint(0, V, (B, Tg), generator=g)
        qlen = (glen.squeeze(1).float() * 0.7).long().clamp(min=1)
        q = torch.nn.functional.normalize(torch.randn(B, D, generator=g), dim=1)
        p = torch.nn.functional.normalize(torch.randn(B, D, generator=g), dim=1)
        h = torch.randn(B, Tg, H, generator=g).bfloat16()
        W = (torch.randn(V, H, generator=g) / H ** 0.5 * 2.0).bfloat16()
        live = live_row_index(mask, 64)
        assert live.numel() == 128 and int((live < 0).sum()) == 2
        nxt = torch.cat((mask[:, 1:], torch.zeros_like(mask[:, :1])), 1)
        tok = ((mask != 0) | (nxt != 0)).reshape(-1).nonzero().squeeze(1)   # the packed rows (dalm_amd/packed.py) + slack entries
        pack = torch.cat((tok, torch.full((192 - tok.numel(),), -1)))
        assert tok.numel() == 130
        q, p, h, W, ids, mask, qlen, live, pack = [t.to(dev) for t in (q, p, h, W, ids, mask, qlen, live, pack)]
        labels, weights = packed_labels(ids, mask, pack)
        # reference: the logits of the same bf16 values, materialised in f64 and handed to the logits node in f32
        logits = (h.double().reshape(B * Tg, H) @ W.double().t()).float().view(B, Tg, V).requires_grad_(True)
        qq, pp = q.clone().requires_grad_(True), p.clone().requires_grad_(True)
        loss = rag_e2e_loss(qq, pp, logits, ids, mask, qlen, 100.0)
        loss.backward()
        dh = (logits.grad.double().reshape(B * Tg, V) @ W.double()).view(B, Tg, H)
        _PAIR_CACHE["batch"] = dict(q=q, p=p, h=h, W=W, ids=ids, mask=mask, qlen=qlen, live=live, pack=pack, labels=labels,
                                    weights=weights, ref=(loss.detach(), qq.grad, pp.grad, dh),
                                    x_max=float(logits.detach().abs().max()))
    return _PAIR_CACHE["batch"]


def _pair_run(dev, selection, engine, grad):
    """(loss, dq, dp, dh [B, Tg, H]) of one pair, run once per module; the gradients are None for a forward-only pair."""
    key = (selection, engine, grad)
    if key in _PAIR_CACHE:
        return _PAIR_CACHE[key]
    from dalm_amd.fused import _pick_lm_head_engine, rag_e2e_loss_from_hidden, rag_e2e_loss_packed
    from dalm_amd.ops import default_ops

    b = _pair_batch(dev)
    saved = {k: os.environ.pop(k, None) for k in ("DALM_LM_HEAD_KERNEL", "DALM_LM_HEAD_TRAIN_KERNEL")}
    try:
        for k, v in zip(saved, _PAIRS[key]):
            if v is not None:
                os.environ[k] = v
        assert _pick_lm_head_engine(default_ops(), b["h"], b["W"], grad, False, selection) == engine
        qq, pp, hh = [b[k].clone().requires_grad_(grad) for k in ("q", "p", "h")]
        with torch.enable_grad() if grad else torch.no_grad():
            if selection == "packed":
                hr = hh.reshape(-1, hh.shape[-1]).index_select(0, b["pack"].clamp_min(0))
                loss = rag_e2e_loss_packed(qq, pp, hr, b["W"], b["labels"], b["weights"], b["mask"], b["qlen"], 100.0)
            else:
                loss = rag_e2e_loss_from_hidden(qq, pp, hh, b["W"], b["ids"], b["mask"], b["qlen"], 100.0,
                                                live_rows=b["live"] if selection == "live" else None)
            if grad:
                loss.backward()
        torch.cuda.synchronize()
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    _PAIR_CACHE[key] = (loss.detach(), qq.grad, pp.grad, hh.grad)
    return _PAIR_CACHE[key]


def test_the_pairs_are_all_the_table_names_at_these_shapes():
    import itertools

    from dalm_amd.fused import _lm_head_engine

    V, H = _PAIR_SHAPES["V"], _PAIR_SHAPES["H"]
    got = set()
    for sel, grad, k, t in itertools.product(("all", "live", "packed"), (False, True), (None, "0", "1", "2"), (None, "0", "1", "2")):
        got.add((sel, _lm_head_engine(selection=sel, need_grad=grad, need_dw=False, cuda=True, h_dtype=torch.bfloat16,
                                      w_dtype=torch.bfloat16, H=H, V=V, weight_bytes=2 * V * H, tunable=False,
                                      has=frozenset(("lm_head_lse", "lm_head_backward", "lm_head_logits")), env_kernel=k,
                                      env_train_kernel=t), grad))
    assert got == set(_PAIRS)


@pytest.mark.parametrize("selection,engine,grad", sorted(_PAIRS), ids=lambda v: str(v))
def test_every_selection_and_engine_vs_materialised_logits(dev, selection, engine, grad):
    """Loss bounds as in test_training_through_the_kernels_vs_fp64_oracle_and_library_path: 2e-5 for the engines that keep the
    logits in f32 (lse, recompute), 2e-3 for the ones that round them to bf16 (mm_rows, logits_rows, sample_chunks).  Gradients
    of recompute: the same test's 6e-3 and 1.5 x the library engine's error + 1e-3.  d(hidden) of the bf16-logits engines, with
    u = 2^-9 the unit roundoff of bf16: a logit x rounded to bf16 is off by at most u |x|, which moves a softmax probability by
    at most a factor exp(2 u x_max) ~ 1 + 2 u x_max; d(logits) and d(hidden) are rounded to bf16 once each, u apiece - in all
    (2 x_max + 2) u relative to the exact d(hidden), x_max the largest |logit| of the batch.  dq and dp do not depend on the head."""
    b = _pair_batch(dev)
    loss_ref, dq_ref, dp_ref, dh_ref = b["ref"]
    loss, dq, dp, dh = _pair_run(dev, selection, engine, grad)
    f32_logits = engine in ("lse", "recompute")
    err = abs(float(loss) - float(loss_ref)) / abs(float(loss_ref))
    print(f"{selection}/{engine}/grad={grad}: loss rel err {err:.3e}")
    assert err <= (2e-5 if f32_logits else 2e-3)
    if not grad:
        return
    e = {n: _rel(got, want) for n, got, want in (("dq", dq, dq_ref), ("dp", dp, dp_ref), ("dh", dh, dh_ref))}
    print(f"{selection}/{engine}: {e}, x_max {b['x_max']:.2f}")
    if f32_logits:
        lib = _pair_run(dev, selection, "sample_chunks" if selection == "all" else "mm_rows", True)
        for n, got_l, want in (("dq", lib[1], dq_ref), ("dp", lib[2], dp_ref), ("dh", lib[3], dh_ref)):
            assert e[n] < 6e-3 and e[n] < 1.5 * _rel(got_l, want) + 1e-3, (n, e[n], _rel(got_l, want))
    else:
        assert e["dq"] < 6e-3 and e["dp"] < 6e-3, e
        assert e["dh"] < (2.0 * b["x_max"] + 2.0) * 2.0 ** -9, (e, b["x_max"])
    dead = (torch.cat((b["mask"][:, 1:], torch.zeros_like(b["mask"][:, :1])), 1) == 0)
    assert float(dh[dead].abs().max()) == 0.0
