"""Causal-LM retrievers on the GPU: the last-token pool kernels (`dalm_pool_last_packed_fwd` / `_bwd`) against fp64, the training
steps padded vs packed (pack plans that keep the pooled column, decoder stack on the packed rows, pooling straight from [n, D]),
the padded step on right-padded batches against the reference's formula (row liveness keeps column T - 1), the retriever-only
trainer with and without --pack_tokens, and the packed evaluation sweep.
Reference: dalm/models/retriever_only_base_model.py:43-63, dalm/models/rag_e2e_base_model.py:84-93."""
import copy
import csv
import json
from pathlib import Path

import pytest
import torch

from test_eval_gpu import POOL_NORM_RTOL, POOL_PROFILES

pytestmark = pytest.mark.gpu
G = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def dev():
    from dalm_amd import hip

    hip.load()  # fail loudly if libdalm_hip.so is absent: no fallback
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------------
# kernels vs fp64
# ---------------------------------------------------------------------------------------------------------------------
def _pool_case(profile, D, dtype):
    lens = POOL_PROFILES[profile]                              # the LAST entry is a slack tail beyond nseq_out
    g = torch.Generator().manual_seed(D + len(lens))
    n = sum(lens)
    h = (torch.randn(n, D, generator=g) * 0.7 + 0.1).to(dtype)
    cu = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32)
    d_emb = torch.randn(len(lens) - 1, D, generator=g)
    return lens, h, cu, d_emb


def _rel(a, b):
    return float((a - b).norm()) / max(float(b.norm()), 1e-300)


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("D", [32, 384, 4096, 8192])
@pytest.mark.parametrize("profile", sorted(POOL_PROFILES))
def test_last_token_pool_kernels_vs_fp64(dev, profile, D, dtype, normalize):
    from dalm_amd import hip
    from dalm_amd.ops import default_ops

    lens, h, cu, d_emb = _pool_case(profile, D, dtype)
    nseq, nseq_out, n = len(lens), len(lens) - 1, h.shape[0]
    ld = D + 8
    out = torch.full((nseq_out + 2, ld), 7.0, device=dev)
    hd, cud = h.to(dev), cu.to(dev)
    got, norm = default_ops().pool_last_packed_fwd(hd, cud, nseq_out, bool(normalize), out=out[:nseq_out, :D])
    assert got.data_ptr() == out.data_ptr() and got.dtype == torch.float32 and norm.shape == (nseq_out,)
    last = [int(cu[s + 1]) - 1 for s in range(nseq_out)]
    u = torch.stack([h[r].double() if ln else torch.zeros(D, dtype=torch.float64) for r, ln in zip(last, lens)])
    nrm = u.norm(dim=1, keepdim=True)
    ref = u / nrm.clamp_min(1e-12) if normalize else u
    e = got.cpu()
    if normalize:
        err = _rel(e.double(), ref)
        print(f"fwd {profile} D={D} {dtype}: norm-relative error {err:.3e}")
        assert err <= POOL_NORM_RTOL
    else:
        assert torch.equal(e, u.float())                                  # the upcast row, bit for bit
    assert _rel(norm.cpu().double(), nrm.squeeze(1)) <= 2e-6                # f32: 32 serial terms per thread + an 8-level tree
    for s, ln in enumerate(lens[:nseq_out]):
        if ln == 0:
            assert float(e[s].abs().max()) == 0.0 and float(norm[s]) == 0.0     # an empty sequence: a zero row, norm 0
    assert bool((out[nseq_out:] == 7.0).all()) and bool((out[:, D:] == 7.0).all())      # untouched

    # backward into a NaN-filled dh, the saved rows read at their leading dimension
    de = torch.full((nseq_out, ld), float("nan"), device=dev)
    de[:, :D] = d_emb.to(dev)
    dh = torch.full((n, D), float("nan"), device=dev, dtype=dtype)
    hip.call("dalm_pool_last_packed_bwd", hip.ptr(de), ld, hip.ptr(out), ld, hip.ptr(norm), hip.ptr(cud), n, nseq, nseq_out, D,
             int(normalize), hip.ptr(dh), hip.dtype_code(dh), hip.stream())
    dh = dh.cpu()
    assert not bool(torch.isnan(dh).any())
    closing = {r: s for s, (r, ln) in enumerate(zip(last, lens)) if ln}
    others = torch.tensor([r for r in range(n) if r not in closing], dtype=torch.int64)
    assert bool((dh[others] == 0).all())                                  # exactly 0.0, the slack tail's rows included
    d64 = d_emb.double()
    for r, s in closing.items():
        if normalize:
            es = ref[s]
            want = (d64[s] - es * (es @ d64[s])) / nrm[s].clamp_min(1e-12)
        else:
            want = d64[s]
        if dtype == torch.float32:
            assert _rel(dh[r].double(), want) <= 1e-4, (r, s)
        else:
            assert _rel(dh[r].double(), want.float().to(torch.bfloat16).double()) <= 2.0 ** -8, (r, s)


def test_autograd_function_and_the_degenerate_row_as_the_mean_pool_treats_it(dev):
    """`fused.pool_last_packed` end to end, against `fused.pool_l2norm` on the padded layout with the one-token mask of
    `eos_mask`: same embeddings and the same dh at the pooled rows - a zero row (|u| < 1e-12) included, which both kernels
    answer with d_e / 1e-12."""
    from dalm_amd import fused, packed
    from dalm_amd.utils import eos_mask

    B, T, D = 5, 8, 128
    g = torch.Generator().manual_seed(3)
    h = torch.randn(B, T, D, generator=g)
    h[2, T - 1] = 0                                                        # the degenerate row
    mask = torch.ones(B, T, dtype=torch.long)
    mask[1, :3] = 0
    mask[3, 5:] = 0                                                        # right-padded: column T - 1 is kept all the same
    rows, cu = packed.pack_plan(mask, False, 16, last_column=True)
    w = torch.randn(B, D, generator=g).to(dev)
    hp = h.reshape(B * T, D).index_select(0, rows.clamp_min(0)).to(dev).requires_grad_(True)
    e1 = fused.pool_last_packed(hp, cu.to(dev), B, True)
    (e1 * w).sum().backward()
    h2 = h.to(dev).requires_grad_(True)
    e2 = fused.pool_l2norm(h2, eos_mask(mask).to(dev), True)
    (e2 * w).sum().backward()
    assert e1.shape == (B, D) and float((e1 - e2).abs().max()) <= 1e-6
    pooled = (cu[1:B + 1].long() - 1).to(dev)
    got, want = hp.grad.index_select(0, pooled), h2.grad[:, T - 1]
    assert torch.equal(got[2], want[2]) and float(got[2].abs().max()) > 1e6          # d_e / 1e-12
    keep = torch.tensor([0, 1, 3, 4], device=dev)
    assert _rel(got[keep].double(), want[keep].double()) <= 1e-5
    rest = torch.ones(hp.shape[0], dtype=torch.bool, device=dev)
    rest[pooled] = False
    assert bool((hp.grad[rest] == 0).all())


def test_nothing_pooled_and_an_int64_cu(dev):
    """nseq_out == 0: the forward writes nothing, the backward still writes all of dh (zeros) - the pooled side is empty tensors.
    A cu of another integer type is converted by both ops, not misread."""
    from dalm_amd.ops import default_ops

    ops = default_ops()
    n, D = 40, 64
    h = torch.randn(n, D, device=dev)
    cu = torch.tensor([0, 7, 7, 40], device=dev)                           # int64
    emb, norm = ops.pool_last_packed_fwd(h, cu, 0, True)
    assert emb.shape == (0, D) and norm.shape == (0,)
    dh = ops.pool_last_packed_bwd(torch.empty(0, D, device=dev), emb, norm, cu, n, True, torch.float32)
    assert dh.shape == (n, D) and bool((dh == 0).all())
    emb, norm = ops.pool_last_packed_fwd(h, cu, None, False)
    assert torch.equal(emb[0], h[6]) and bool((emb[1] == 0).all()) and torch.equal(emb[2], h[39])
    dh = ops.pool_last_packed_bwd(torch.ones(3, D, device=dev), emb, norm, cu, n, False, torch.float32)
    want = torch.zeros(n, D, device=dev)
    want[6] = 1
    want[39] = 1
    assert torch.equal(dh, want)


# ---------------------------------------------------------------------------------------------------------------------
# steps: padded vs packed
# ---------------------------------------------------------------------------------------------------------------------
_LMS = {}


def _llama(kv, bare=False):
    """Llama 256 = 4 heads x 64, `kv` KV heads, 2 layers, LoRA on q / v without dropout; built once on the CPU, weights on the
    bf16 grid so that the fp32 and the bf16 runs hold the same numbers."""
    if kv not in _LMS:
        from transformers import LlamaConfig, LlamaForCausalLM

        from dalm_amd.models import lora
        from dalm_amd.models.lora import LoRALinear

        torch.manual_seed(77 + kv)
        lm = LlamaForCausalLM(LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                                          num_key_value_heads=kv, vocab_size=128, max_position_embeddings=64, attention_dropout=0.0,
                                          pad_token_id=0))
        with torch.no_grad():
            for p in lm.parameters():
                p.copy_(p.to(torch.bfloat16).float())
        lora.inject_lora(lm, ["q_proj", "v_proj"], lora_dropout=0.0)
        g = torch.Generator().manual_seed(99)
        for m in lm.modules():
            if isinstance(m, LoRALinear):          # lora_B starts at zero, which zeroes every lora_A gradient
                with torch.no_grad():
                    m.lora_B["default"].weight.copy_(0.05 * torch.randn(m.lora_B["default"].weight.shape, generator=g))
        _LMS[kv] = lm
    lm = copy.deepcopy(_LMS[kv])
    return lm.model if bare else lm


def _mask(lens, T, left):
    ar = torch.arange(T).unsqueeze(0)
    lens = torch.tensor(lens).unsqueeze(1)
    return ((ar >= T - lens) if left else (ar < lens)).long()


def _retriever_batch(left, prefix=""):
    g = torch.Generator().manual_seed(21)
    return {f"{prefix}query_input_ids": torch.randint(3, 128, (6, 16), generator=g),
            f"{prefix}query_attention_mask": _mask([16, 1, 7, 12, 3, 9], 16, left),
            f"{prefix}passage_input_ids": torch.randint(3, 128, (6, 32), generator=g),
            f"{prefix}passage_attention_mask": _mask([32, 20, 1, 31, 11, 25], 32, left)}


def _rag_batch(left):
    b = _retriever_batch(left, "retriever_")
    g = torch.Generator().manual_seed(22)
    b.update({"generator_input_input_ids": torch.randint(3, 80, (6, 24), generator=g),
              "generator_input_attention_mask": _mask([24, 10, 17, 5, 21, 13], 24, True),
              "query_passage_input_len": torch.tensor([14, 6, 9, 2, 11, 7])})
    return b


class _GradSnapshot:
    """optimizer pre-step hook: copies of every trainable gradient while they still exist."""

    def __init__(self, named):
        self.named, self.grads = named, {}

    def __call__(self, *_):
        self.grads = {n: p.grad.detach().float().cpu().clone() for n, p in self.named if p.grad is not None}


def _run_step(kind, kv, batch, mode, precision, dev):
    from transformers import AutoModelForCausalLM

    from dalm_amd import packed
    from dalm_amd.models import AutoModelForRagE2E, AutoModelForSentenceEmbedding
    from dalm_amd.training.step import RagE2EStep, RetrieverStep

    if kind == "retriever":
        model = AutoModelForSentenceEmbedding.from_modules(_llama(kv), None, normalize=True, get_peft=False, is_autoregressive=True)
        groups = packed.RETRIEVER_GROUPS_CAUSAL
    else:
        gen = AutoModelForCausalLM.from_pretrained(str(G / "tiny_generator"))
        model = AutoModelForRagE2E.from_modules(_llama(kv, bare=True), gen, None, None, normalize=True, get_peft=None,
                                                retriever_is_autoregressive=True)
        groups = packed.RAG_GROUPS_CAUSAL
    model = model.to(dev)
    if precision == "bf16":
        for p in model.parameters():
            if not p.requires_grad:
                p.data = p.data.to(torch.bfloat16)
    model.train()
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    assert named
    opt = torch.optim.SGD([p for _, p in named], lr=0.0)
    snap = _GradSnapshot(named)
    opt.register_step_pre_hook(snap)
    cls = RetrieverStep if kind == "retriever" else RagE2EStep
    step = cls(model, opt, None, 100, autocast_dtype=torch.bfloat16 if precision == "bf16" else None, overlap_towers=True,
               track_grad_norm=True)
    host = packed.add_pack_plans(batch, groups) if mode == "packed" else batch
    called = []
    real = packed.causal_retrieval_embed_pair
    packed.causal_retrieval_embed_pair = lambda *a, **k: (called.append(1), real(*a, **k))[1]
    try:
        loss = float(step({k: v.to(dev) for k, v in host.items()}))
    finally:
        packed.causal_retrieval_embed_pair = real
    assert bool(called) == (mode == "packed")                 # the packed batch took the packed causal route, the padded one did not
    return {"loss": loss, "grad_norm": float(step.grad_norm)}, snap.grads


def _dist(a, b):
    return {k: abs(a[k] - b[k]) / max(abs(b[k]), 1e-30) for k in ("loss", "grad_norm")}


@pytest.mark.parametrize("left", [True, False], ids=["left", "right"])
@pytest.mark.parametrize("kv", [4, 2])
@pytest.mark.parametrize("kind", ["retriever", "rag"])
def test_packed_step_equals_padded(dev, kind, kv, left):
    """fp32: loss, gradient norm and every gradient within 1e-4.  bf16 autocast: loss within 2.5e-4 and gradient norm within
    7e-3 of the padded bf16 step (the bounds of test_packed_gpu.py's retriever-only step), in every case.  Against the fp32 step
    the same bounds - or, where the PADDED bf16 step itself is further than that from fp32 (the loss, at this narrow width),
    packed within twice the padded step's own distance plus the bound."""
    batch = _retriever_batch(left) if kind == "retriever" else _rag_batch(left)
    res = {(mode, prec): _run_step(kind, kv, batch, mode, prec, dev) for prec in ("fp32", "bf16") for mode in ("padded", "packed")}
    d32 = _dist(res["packed", "fp32"][0], res["padded", "fp32"][0])
    gp, gq = res["packed", "fp32"][1], res["padded", "fp32"][1]
    assert set(gp) == set(gq)
    worst = max(float((gp[n].double() - gq[n].double()).norm()) / max(float(gq[n].double().norm()), 1e-30)
                for n in gq if float(gq[n].double().norm()) >= 1e-7)
    d16 = _dist(res["packed", "bf16"][0], res["padded", "bf16"][0])
    pad16 = _dist(res["padded", "bf16"][0], res["padded", "fp32"][0])
    pack16 = _dist(res["packed", "bf16"][0], res["padded", "fp32"][0])
    print(f"{kind} kv={kv} {'left' if left else 'right'}: fp32 packed vs padded {d32}, worst gradient {worst:.3e}; "
          f"bf16 packed vs padded {d16}; bf16 padded vs fp32 {pad16}; bf16 packed vs fp32 {pack16}")
    assert d32["loss"] <= 1e-4 and d32["grad_norm"] <= 1e-4 and worst <= 1e-4
    for k, tol in (("loss", 2.5e-4), ("grad_norm", 7e-3)):
        assert d16[k] <= tol, (k, d16)                            # packed vs padded: always
        # against the fp32 step: the bound, or - where the padded bf16 step itself is further away - twice its distance + the bound
        assert pack16[k] <= (tol if pad16[k] <= tol else 2.0 * pad16[k] + tol), (k, pack16, pad16)


def test_single_input_packed_call_equals_the_pair_call(dev):
    """`causal_retrieval_embed` (what a rank of a multi-GPU step calls, one input at a time) against the one-call pair form."""
    from dalm_amd import packed
    from dalm_amd.models import AutoModelForSentenceEmbedding

    model = AutoModelForSentenceEmbedding.from_modules(_llama(2), None, normalize=True, get_peft=False, is_autoregressive=True)
    model = model.to(dev).to(torch.bfloat16).eval()
    b = {k: v.to(dev) for k, v in packed.add_pack_plans(_retriever_batch(False), packed.RETRIEVER_GROUPS_CAUSAL).items()}
    q = tuple(b[f"query_{k}"] for k in ("input_ids", "attention_mask", "pack_rows", "pack_cu"))
    p = tuple(b[f"passage_{k}"] for k in ("input_ids", "attention_mask", "pack_rows", "pack_cu"))
    with torch.no_grad():
        ep, eq = packed.causal_retrieval_embed_pair(model.model, p, q, True)
        ep1, eq1 = packed.causal_retrieval_embed(model.model, *p, True), packed.causal_retrieval_embed(model.model, *q, True)
    assert ep.shape == ep1.shape == (6, 256) and eq.shape == eq1.shape == (6, 256)
    assert float((ep - ep1).norm(dim=1).max()) <= 2.0 ** -7 and float((eq - eq1).norm(dim=1).max()) <= 2.0 ** -7   # bf16 rows, unit norm


# ---------------------------------------------------------------------------------------------------------------------
# the padded step on a right-padded batch: column T - 1 is live
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kv", [4, 2])
def test_right_padded_padded_step_matches_the_reference_formula(dev, kv):
    """The reference pools column T - 1 whatever the mask says (eos_mask's default): on a right-padded batch that column is
    padding, and the padded step's row liveness must keep it.  fp32 step against the formula in plain torch on the host:
    loss, gradient norm and every gradient within 1e-4.  Under bf16 autocast the embedding inside the step's liveness context
    is bit for bit the one computed without any liveness vector."""
    import dalm_oracle as O

    from dalm_amd import live_rows
    from dalm_amd.models import AutoModelForSentenceEmbedding

    batch = _retriever_batch(False)
    got, grads = _run_step("retriever", kv, batch, "padded", "fp32", dev)
    lm = _llama(kv)
    lm.config._attn_implementation = "sdpa"
    embs = []
    for side in ("query", "passage"):
        ids, mask = batch[f"{side}_input_ids"], batch[f"{side}_attention_mask"]
        h = lm(ids, attention_mask=mask, output_hidden_states=True, return_dict=True).hidden_states[-1]
        m = O.ref_eos_mask(mask).unsqueeze(-1).expand(h.size()).float()
        embs.append(torch.nn.functional.normalize(torch.sum(h * m, 1) / torch.clamp(m.sum(1), min=1e-9), p=2, dim=1))
    out = O.ref_step_loss(embs[0], embs[1], None, None, None, None, 100)
    out["loss"].backward()
    ref_g = {"model." + n: p.grad for n, p in lm.named_parameters() if p.requires_grad and p.grad is not None}
    ref_norm = float(torch.linalg.vector_norm(torch.stack([g.double().norm() for g in ref_g.values()])))
    d_loss = abs(got["loss"] - float(out["loss"])) / abs(float(out["loss"]))
    d_norm = abs(got["grad_norm"] - ref_norm) / ref_norm
    assert set(ref_g) == set(grads)
    worst = max(float((grads[n].double() - g.double()).norm()) / float(g.double().norm()) for n, g in ref_g.items()
                if float(g.double().norm()) >= 1e-7)
    print(f"right-padded padded step vs the reference formula, kv={kv}: loss {d_loss:.3e}, gradient norm {d_norm:.3e}, "
          f"worst gradient {worst:.3e}")
    assert d_loss <= 1e-4 and d_norm <= 1e-4 and worst <= 1e-4

    model = AutoModelForSentenceEmbedding.from_modules(_llama(kv), None, normalize=True, get_peft=False, is_autoregressive=True)
    model = model.to(dev).to(torch.bfloat16).eval()
    ids, mask = batch["passage_input_ids"].to(dev), batch["passage_attention_mask"].to(dev)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        plain = model(ids, mask)
        with live_rows.tower_call(mask, False, True, last_column=True) as vec:
            live = model(ids, mask)
    assert vec is not None and int(vec.sum()) == int(mask.sum()) + 5          # five right-padded rows gain their last column
    assert torch.equal(plain, live)


# ---------------------------------------------------------------------------------------------------------------------
# trainer and evaluation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["tiny_generator", "head_width_64"])
def test_train_retriever_autoregressive_with_and_without_pack_tokens(dev, tmp_path, monkeypatch, which):
    """Four steps of the retriever-only trainer with a causal-LM retriever, fp32: --pack_tokens keeps the per-step losses (1e-4
    relative).  tiny_generator has head width 16, which the "dalm_sdpa" attention does not take: the trainer builds the row lists
    and the step falls back to the padded call.  The same trainer on a Llama of head width 64 (same tokenizer) takes the packed
    route - one rank: the whole step is captured as a graph from the third step on, so it runs under capture and replay too."""
    from dalm_amd.training.retriever_only.train_retriever_only import train_retriever

    name = str(G / "tiny_generator")
    if which == "head_width_64":
        from transformers import AutoTokenizer, LlamaConfig, LlamaForCausalLM

        torch.manual_seed(5)
        name = str(tmp_path / "llama_hd64")
        LlamaForCausalLM(LlamaConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                                     num_key_value_heads=2, vocab_size=80, max_position_embeddings=64, pad_token_id=0, bos_token_id=1,
                                     eos_token_id=2)).save_pretrained(name)
        AutoTokenizer.from_pretrained(str(G / "tiny_generator")).save_pretrained(name)

    rows = json.loads((G / "host_golden.json").read_text())["rows"]
    path = tmp_path / "rows.csv"
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["Question", "Abstract", "Answer"])
        for i in range(16):
            k = i % 5
            w.writerow([rows["Question"][k] + " " + str(i), rows["Abstract"][(k + i // 5) % 5], rows["Answer"][k]])
    from dalm_amd import packed

    runs, routed = {}, {}
    real = packed.causal_retrieval_embed_pair
    for pack in (False, True):
        losses, calls = [], []
        monkeypatch.setattr(packed, "causal_retrieval_embed_pair", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
        train_retriever(name, str(path), query_max_len=12, passage_max_len=24, per_device_train_batch_size=4,
                        learning_rate=1e-3, num_train_epochs=1, num_warmup_steps=0, output_dir=str(tmp_path / f"out{int(pack)}"),
                        with_tracking=False, seed=7, use_peft=False, use_bnb=False, is_autoregressive=True, mixed_precision="no",
                        pack_tokens=pack, on_step=lambda s, l: losses.append(float(l)))
        runs[pack], routed[pack] = losses, len(calls)
    print("train_retriever(is_autoregressive=True) losses, padded / packed:", runs, "python-level calls of the packed route:", routed)
    assert len(runs[True]) == len(runs[False]) == 4
    # python-level calls: the two eager steps and the capture went the packed way where the model allows it
    assert routed[False] == 0 and (routed[True] >= 2 if which == "head_width_64" else routed[True] == 0)
    for a, b in zip(runs[False], runs[True]):
        assert abs(a - b) <= 1e-4 * abs(a), runs


def test_packed_sweep_with_an_autoregressive_owner(dev, monkeypatch):
    """`embed_dataset(packed_sweep=True)` with a causal-LM retriever against the padded bf16 forward, both measured against an
    fp32 run of the same rows (torch SDPA, the reference's pooling expression): the packed sweep may be off by twice the padded
    forward's own error.  The sweep pools with `pool_last_packed_fwd`; rows are left- and right-padded."""
    import datasets

    from dalm_amd.eval import utils as EU
    from dalm_amd.models import AutoModelForSentenceEmbedding
    from dalm_amd.ops import HipOps
    from dalm_amd.utils import eos_mask

    N, T = 40, 32
    g = torch.Generator().manual_seed(8)
    ids = torch.randint(3, 128, (N, T), generator=g)
    lens = torch.randint(1, T + 1, (N,), generator=g).tolist()
    lens[0], lens[1] = T, 1
    mask = torch.cat([_mask(lens[:N // 2], T, True), _mask(lens[N // 2:], T, False)])
    ds = datasets.Dataset.from_dict({"retriever_passage_input_ids": ids.tolist(), "retriever_passage_attention_mask": mask.tolist()})
    ref_lm = _llama(2).to(dev)
    ref_lm.config._attn_implementation = "sdpa"
    with torch.no_grad():
        h = ref_lm(ids.to(dev), attention_mask=mask.to(dev), output_hidden_states=True, return_dict=True).hidden_states[-1].double()
        m = eos_mask(mask).to(dev).unsqueeze(-1).double()
        ref = torch.nn.functional.normalize((h * m).sum(1) / m.sum(1).clamp_min(1e-9), p=2, dim=1).cpu()
    model = AutoModelForSentenceEmbedding.from_modules(_llama(2), None, normalize=True, get_peft=False, is_autoregressive=True)
    model = model.to(dev).to(torch.bfloat16).eval()
    calls = []
    real = HipOps.pool_last_packed_fwd
    monkeypatch.setattr(HipOps, "pool_last_packed_fwd", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    packed_e = EU.embed_dataset(ds, "retriever_passage", model.forward, "cuda:0", torch.bfloat16, 8, packed_sweep=True)
    assert len(calls) >= 2                                                # the new kernel pooled, in several batches
    n0 = len(calls)
    padded_e = EU.embed_dataset(ds, "retriever_passage", model.forward, "cuda:0", torch.bfloat16, 8, packed_sweep=False)
    assert len(calls) == n0
    assert packed_e.is_cuda and packed_e.dtype == torch.float32 and packed_e.shape == padded_e.shape == (N, 256)
    err_packed = float((packed_e.double().cpu() - ref).norm(dim=1).max())
    err_padded = float((padded_e.double().cpu() - ref).norm(dim=1).max())
    print(f"causal-LM retriever sweep, max row L2 error vs fp32: padded bf16 {err_padded:.3e}, packed sweep {err_packed:.3e}")
    assert err_padded > 0 and err_packed <= 2 * err_padded
