"""MPNet retrievers on the GPU: the routed model (attention with the relative-position bias on `dalm_attn_rel_*`, dropout + add +
LayerNorm on BERT's kernel) against transformers' own code, the packed retriever-only step against the padded one, and the
packed evaluation sweep."""
import copy
import json

import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu
PAD = 1                                                            # MPNetEmbeddings' hard-coded padding_idx


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


def _autocast():
    return torch.autocast("cuda", dtype=torch.bfloat16)


def _mpnet(hidden=128, heads=2, layers=3, vocab=200, max_pos=66, seed=0):
    from transformers import MPNetConfig, MPNetModel

    torch.manual_seed(seed)
    m = MPNetModel(MPNetConfig(hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=heads, intermediate_size=2 * hidden,
                               vocab_size=vocab, max_position_embeddings=max_pos, hidden_dropout_prob=0.0,
                               attention_probs_dropout_prob=0.0))
    with torch.no_grad():                                          # a bias that matters: the default init is N(0, 0.02)
        m.encoder.relative_attention_bias.weight.normal_(0.0, 1.0)
    return m


def _right_padded(B, T, lens, lo, hi, seed):
    ids = torch.randint(lo, hi, (B, T), generator=torch.Generator().manual_seed(seed))
    mask = (torch.arange(T).unsqueeze(0) < torch.tensor(lens).unsqueeze(1)).long()
    return torch.where(mask.bool(), ids, torch.full_like(ids, PAD)), mask


def _rel(a, b):
    return float((a.double() - b.double()).norm()) / max(float(b.double().norm()), 1e-30)


def test_routed_model_against_fp32(dev):
    """Tiny MPNetModel, everything frozen but the word table, dropout 0: routed bf16-autocast and unrouted bf16-autocast, each
    against the unrouted model in fp32.  The routed error on live hidden states and on the word-table gradient is at most 1.5 x
    the unrouted bf16 error + 1e-3 (`helpers.ROW_FACTOR` / `ROW_OFFSET`): the eager bf16 chain rounds the scores to bf16, it is a
    yardstick for the error, not for the values.  The routed forward builds no [B, H, T, T] bias."""
    from dalm_amd import packed
    from dalm_amd.models import attention, fastpath, frozen_linear

    B, T, lens = 3, 40, (40, 25, 7)
    ref = _mpnet().to(dev).requires_grad_(False).train()
    new = copy.deepcopy(ref)
    assert fastpath.use_mpnet_attention_kernels(new) == 4          # 3 self-attention modules + the encoder
    assert packed.attention_is_packable(new) and not packed.attention_is_packable(ref)
    frozen_linear.use_transposed_dgrad(new)
    assert fastpath.use_bert_layer_kernels(new) == 6               # 3 MPNetOutput + 3 MPNetAttention
    ids, mask = _right_padded(B, T, lens, 2, 200, 4)
    ids, mask = ids.to(dev), mask.to(dev)
    up = torch.randn(B, T, 128, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    biases, launches = [], []
    real_bias = new.encoder.compute_position_bias
    new.encoder.compute_position_bias = lambda *a, **k: (biases.append(real_bias(*a, **k)), biases[-1])[1]
    real_launch = attention._rel_launch_forward
    attention._rel_launch_forward = lambda *a, **k: (launches.append(1), real_launch(*a, **k))[1]
    outs = {}
    try:
        for name, m, ctx in (("fp32", ref, None), ("bf16", ref, _autocast), ("routed", new, _autocast)):
            emb = m.embeddings.word_embeddings.weight
            emb.requires_grad_(True)
            emb.grad = None
            if ctx is None:
                h = m(ids, mask)[0]
            else:
                with ctx():
                    h = m(ids, mask)[0]
            (h.float() * mask.unsqueeze(-1) * up).sum().backward()
            outs[name] = (h.detach().float(), emb.grad.detach().float().clone())
            emb.requires_grad_(False)
    finally:
        attention._rel_launch_forward = real_launch
    assert len(launches) == 3, "the routed model did not reach dalm_attn_rel_fwd once per layer"
    assert len(biases) == 1 and attention.rel_source_of(biases[0]) is not None
    assert biases[0].numel() < B * 2 * T * T, "the routed forward allocated a [B, H, T, T] bias"
    live = mask.bool()
    for what, idx in (("hidden", 0), ("word-table gradient", 1)):
        pick = (lambda t: t[live]) if idx == 0 else (lambda t: t)
        e_routed = _rel(pick(outs["routed"][idx]), pick(outs["fp32"][idx]))
        e_bf16 = _rel(pick(outs["bf16"][idx]), pick(outs["fp32"][idx]))
        print(f"mpnet routed vs fp32, {what}: routed {e_routed:.3e}, unrouted bf16 {e_bf16:.3e}")
        assert e_routed <= helpers.ROW_FACTOR * e_bf16 + helpers.ROW_OFFSET, (what, e_routed, e_bf16)


class _GradSnapshot:
    def __init__(self, named):
        self.named, self.grads = named, {}

    def __call__(self, *_):
        self.grads = {n: p.grad.detach().float().cpu().clone() for n, p in self.named if p.grad is not None}


def _prepare_lora(module, seed):
    """No LoRA dropout (the two layouts index its mask differently) and a lora_B that is not zero (else lora_A's gradient is)."""
    from dalm_amd.models.lora import LoRALinear

    g = torch.Generator().manual_seed(seed)
    for m in module.modules():
        if isinstance(m, LoRALinear):
            drop = m.lora_dropout["default"]
            if hasattr(drop, "p"):
                drop.p = 0.0
            w = m.lora_B["default"].weight
            with torch.no_grad():
                w.copy_(0.02 * torch.randn(w.shape, generator=g).to(w.device))


def _batch():
    B = 6
    qi, qm = _right_padded(B, 12, (12, 5, 3, 9, 1, 7), 3, 80, 21)
    pi, pm = _right_padded(B, 24, (24, 11, 17, 6, 20, 13), 3, 80, 22)
    # one left-padded row: its tokens keep columns 15 .. 23 in the packed call (the bias goes by column difference, which the
    # shift leaves alone; the position ids count non-pad ids)
    pm[3] = (torch.arange(24) >= 15).long()
    pi[3] = torch.where(pm[3].bool(), torch.randint(3, 80, (24,), generator=torch.Generator().manual_seed(5)), torch.full((24,), PAD))
    return {"query_input_ids": qi, "query_attention_mask": qm, "passage_input_ids": pi, "passage_attention_mask": pm}


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_packed_retriever_only_step_equals_padded_step(dev, precision):
    """The structure and tolerances of tests/test_roberta_retriever_gpu.py::test_packed_retriever_only_step_equals_padded_step with
    an MPNet retriever (LoRA on q / k / v, the bias table frozen with the base): padded step vs packed step (queries and passages
    in ONE packed call).  fp32 runs the torch fallback of the routed attention in both layouts, bf16 the kernels."""
    from dalm_amd import packed
    from dalm_amd.models import AutoModelForSentenceEmbedding, attention
    from dalm_amd.training.step import RetrieverStep

    base = _mpnet(layers=2, vocab=80, seed=3)
    batch = _batch()
    res = {}
    launches = []
    real_launch = attention._rel_launch_forward
    attention._rel_launch_forward = lambda *a, **k: (launches.append(a[3].packed is not None), real_launch(*a, **k))[1]
    try:
        for mode in ("padded", "packed"):
            torch.manual_seed(17)
            model = AutoModelForSentenceEmbedding.from_modules(copy.deepcopy(base), None, normalize=True, get_peft=True)
            _prepare_lora(model.model, 11)
            model = model.to(dev).train()
            assert packed.attention_is_packable(model.model) and packed.position_padding_idx(model.model) == PAD
            named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
            assert named and all("lora_" in n for n, _ in named)
            opt = torch.optim.SGD([p for _, p in named], lr=0.0)
            snap = _GradSnapshot(named)
            opt.register_step_pre_hook(snap)
            step = RetrieverStep(model, opt, None, 100, autocast_dtype=torch.bfloat16 if precision == "bf16" else None,
                                 overlap_towers=True, track_grad_norm=True)
            host = packed.add_pack_plans(batch, packed.RETRIEVER_GROUPS) if mode == "packed" else batch
            n0 = len(launches)
            loss = float(step({k: v.to(dev) for k, v in host.items()}))
            if precision == "bf16":                                # the kernels ran, in this mode's layout
                assert len(launches) > n0 and all(x == (mode == "packed") for x in launches[n0:]), (mode, launches[n0:])
            res[mode] = ({"loss": loss, "grad_norm": float(step.grad_norm)}, snap.grads)
            del model, step, opt
    finally:
        attention._rel_launch_forward = real_launch
    rel = {k: abs(res["packed"][0][k] - res["padded"][0][k]) / max(abs(res["padded"][0][k]), 1e-30) for k in ("loss", "grad_norm")}
    print(f"mpnet retriever-only step {precision}: packed vs padded {json.dumps(rel)} {json.dumps(res['padded'][0])}")
    tol = {"loss": 1e-4, "grad_norm": 1e-4} if precision == "fp32" else {"loss": 2.5e-4, "grad_norm": 7e-3}
    for k, v in rel.items():
        assert v <= tol[k], (k, rel)
    if precision == "fp32":
        gp, gq = res["packed"][1], res["padded"][1]
        assert set(gp) == set(gq) and gq
        for n in gq:
            den = max(float(gq[n].double().norm()), 1e-30)
            assert float((gp[n].double() - gq[n].double()).norm()) / den <= 1e-4 or float(gq[n].double().norm()) < 1e-7, n


def test_packed_sweep_with_an_mpnet_retriever(dev, monkeypatch):
    """`embed_dataset(packed_sweep=True)` with a frozen MPNet retriever on 64 rows of random lengths against the padded bf16
    forward, both measured against an fp32 eager run of the same weights: the packed sweep may be off by twice the padded forward's
    own error (the bound of test_packed_sweep_with_an_xlmr_retriever)."""
    import datasets

    from dalm_amd.eval import utils as EU
    from dalm_amd.models import AutoModelForSentenceEmbedding
    from dalm_amd.ops import HipOps

    N, T = 64, 32
    lens = torch.randint(1, T + 1, (N,), generator=torch.Generator().manual_seed(8)).tolist()
    lens[0], lens[1] = T, 1
    ids, mask = _right_padded(N, T, lens, 2, 200, 9)
    ds = datasets.Dataset.from_dict({"retriever_passage_input_ids": ids.tolist(), "retriever_passage_attention_mask": mask.tolist()})
    enc = _mpnet(hidden=256, heads=4, layers=2).to(torch.bfloat16).requires_grad_(False)
    ref_enc = copy.deepcopy(enc).float().to(dev).eval()
    with torch.no_grad():
        h = ref_enc(input_ids=ids.to(dev), attention_mask=mask.to(dev))[0].double()
        mm = mask.to(dev).unsqueeze(-1).double()
        ref = torch.nn.functional.normalize((h * mm).sum(1) / mm.sum(1).clamp_min(1e-9), p=2, dim=1).cpu()
    model = AutoModelForSentenceEmbedding.from_modules(enc.to(dev), None, normalize=True, get_peft=False).eval()
    calls = []
    real = HipOps.pool_packed_fwd
    monkeypatch.setattr(HipOps, "pool_packed_fwd", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    packed_e = EU.embed_dataset(ds, "retriever_passage", model.forward, "cuda:0", torch.bfloat16, 8, packed_sweep=True)
    assert len(calls) >= 2
    n0 = len(calls)
    padded_e = EU.embed_dataset(ds, "retriever_passage", model.forward, "cuda:0", torch.bfloat16, 8, packed_sweep=False)
    assert len(calls) == n0 and packed_e.shape == padded_e.shape == (N, 256) and packed_e.dtype == torch.float32
    err_packed = float((packed_e.double().cpu() - ref).norm(dim=1).max())
    err_padded = float((padded_e.double().cpu() - ref).norm(dim=1).max())
    print(f"mpnet retriever sweep, max row L2 error vs fp32: padded bf16 {err_padded:.3e}, packed sweep {err_packed:.3e}")
    assert err_padded > 0 and err_packed <= 2 * err_padded
