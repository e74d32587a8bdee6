"""RoBERTa-family retrievers (roberta, xlm-roberta, camembert) on the GPU.  The oracle for everything family-specific is
transformers' own eager model:
* `dalm_embed_norm_fwd` (dalm_amd/csrc/bert.hip) against an fp64 restatement of {Roberta,XLMRoberta,Camembert}Embeddings.forward,
  its dropout mask against oracle/lora_mask.py::keep_mask_v2 (the mask is indexed by the flat chunk index of the [B T, D] output,
  which that restatement covers);
* a routed model ("dalm_sdpa", the BERT layer kernels, the embeddings kernel) against an un-routed deep copy;
* the padded step against the packed step (RAG end-to-end and retriever-only), the retriever-only trainer with and without
  --pack_tokens, and the packed evaluation sweep."""
import copy
import csv
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
G = ROOT / "tests" / "golden"
sys.path.insert(0, str(ROOT / "oracle"))
PAD = 1


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _family(name):
    import transformers

    return getattr(transformers, name + "Config"), getattr(transformers, name + "Model")


def _autocast():
    return torch.autocast("cuda", dtype=torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------------
VOCAB = 50


def _embeddings(D, T, type_vocab, wdt, dev, seed=0):
    from transformers import XLMRobertaConfig
    from transformers.models.xlm_roberta.modeling_xlm_roberta import XLMRobertaEmbeddings

    torch.manual_seed(seed)
    cfg = XLMRobertaConfig(hidden_size=D, vocab_size=VOCAB, pad_token_id=PAD, max_position_embeddings=T + PAD + 2,
                           type_vocab_size=type_vocab, hidden_dropout_prob=0.1, layer_norm_eps=1e-5)
    emb = XLMRobertaEmbeddings(cfg)
    with torch.no_grad():
        for t in (emb.word_embeddings, emb.token_type_embeddings, emb.position_embeddings):
            t.weight.copy_(torch.randn(t.weight.shape))                 # (the padding rows too: they are read like any other)
        emb.LayerNorm.weight.copy_(1.0 + 0.2 * torch.randn(D))
        emb.LayerNorm.bias.copy_(0.1 * torch.randn(D))
    emb = emb.to(dev).requires_grad_(False)
    emb.LayerNorm.to(wdt)
    return emb.eval()


def _ids(T, seed):
    """Six rows: full, right-padded, left-padded, a pad id mid-row, all pad, a single live token at the end."""
    ids = torch.randint(2, VOCAB, (6, T), generator=torch.Generator().manual_seed(seed))
    a, b = max(T // 3, 1), max(2 * T // 3, 1)
    ids[1, a:] = PAD
    ids[2, :T - a] = PAD
    ids[3, b - 1] = PAD
    ids[3, 0] = PAD if T > 2 else ids[3, 0]
    ids[4] = PAD
    ids[5, :T - 1] = PAD
    return ids


def _ref64(emb, ids, tt=None, pos=None):
    """The eager statements in fp64: positions (create_position_ids_from_input_ids), the three gathers, two adds, LayerNorm."""
    if pos is None:
        tok = ids.ne(PAD).int()
        pos = (torch.cumsum(tok, dim=1).type_as(tok) * tok).long() + PAD
        assert torch.equal(pos, type(emb).create_position_ids_from_input_ids(ids, PAD))
    if tt is None:
        tt = torch.zeros_like(ids)
    s = (emb.word_embeddings.weight.double()[ids] + emb.token_type_embeddings.weight.double()[tt]) + emb.position_embeddings.weight.double()[pos]
    return torch.nn.functional.layer_norm(s, (s.shape[-1],), emb.LayerNorm.weight.double(), emb.LayerNorm.bias.double(), emb.LayerNorm.eps)


@pytest.mark.parametrize("wdt", [torch.float32, torch.bfloat16], ids=["w32", "w16"])
@pytest.mark.parametrize("T", [1, 63, 65, 130])
@pytest.mark.parametrize("D", [256, 384, 1024, 2048])
def test_embed_norm_vs_fp64_restatement(dev, D, T, wdt):
    from dalm_amd.models import bert_ops

    ids = _ids(T, D + T).to(dev)
    B = ids.shape[0]

    def run(emb, ids, tt=None, pos=None, live=None):
        with _autocast():
            assert bert_ops.embed_supported(emb, ids, tt, pos, None, 0)
            y = bert_ops.embed_norm(emb, ids, tt, pos, 0.0, 0, live)
        assert y.dtype == torch.float32 and y.shape == (B, T, D) and not y.requires_grad
        assert torch.equal(y._dalm_bf16, y.to(torch.bfloat16))                        # y16 == bf16(y32) exactly
        return y

    # type_vocab_size 1, token_type_ids None, positions derived in the kernel
    emb1 = _embeddings(D, T, 1, wdt, dev)
    y = run(emb1, ids)
    torch.testing.assert_close(y, _ref64(emb1, ids).float(), rtol=3e-6, atol=3e-6)
    with _autocast():
        assert bert_ops.twin(y) is y._dalm_bf16
    # type_vocab_size 2, mixed types; explicit position ids (any values inside the table: the packed route's)
    emb2 = _embeddings(D, T, 2, wdt, dev, seed=1)
    g = torch.Generator().manual_seed(T)
    tt = torch.randint(0, 2, (B, T), generator=g).to(dev)
    y2 = run(emb2, ids, tt)
    torch.testing.assert_close(y2, _ref64(emb2, ids, tt).float(), rtol=3e-6, atol=3e-6)
    pos = torch.randint(0, T + PAD + 2, (B, T), generator=g).to(dev)
    torch.testing.assert_close(run(emb2, ids, tt, pos), _ref64(emb2, ids, tt, pos).float(), rtol=3e-6, atol=3e-6)
    torch.testing.assert_close(run(emb2, ids, None, pos[:1]), _ref64(emb2, ids, None, pos[:1].expand(B, T)).float(), rtol=3e-6, atol=3e-6)
    # liveness: dead rows exactly zero, the others bit-identical
    live = (torch.rand(B * T, generator=g) < 0.6).to(torch.uint8).to(dev)
    yl3 = run(emb2, ids, tt, None, live)
    yl, yl16, alive = yl3.reshape(B * T, D), yl3._dalm_bf16.reshape(B * T, D), live.bool()
    assert bool((yl[~alive] == 0).all()) and bool((yl16[~alive] == 0).all())
    assert torch.equal(yl[alive], y2.reshape(B * T, D)[alive])
    # an id outside the vocabulary (not a pad id before, so no other row's position moves): the call returns, other rows unchanged
    bad = ids.clone()
    bad[0, 0] = VOCAB + 7
    bad[3, T - 1] = -5 if T > 1 else bad[3, T - 1]
    yb = run(emb2, bad, tt)
    torch.cuda.synchronize()
    keep = torch.ones(B, T, dtype=torch.bool, device=dev)
    keep[0, 0] = False
    keep[3, T - 1] = False
    assert torch.equal(yb[keep], y2[keep]) and bool(torch.isfinite(yb).all())


def test_embed_norm_needs_room_in_the_position_table(dev):
    """T + padding_idx + 1 > max_position_embeddings: eager runs (and raises as it does today); explicit positions are taken."""
    from dalm_amd.models import bert_ops

    emb = _embeddings(64, 8, 1, torch.float32, dev)                     # 8 + 1 + 2 rows
    ids = torch.randint(2, VOCAB, (2, 10), device=dev)
    with _autocast():
        assert not bert_ops.embed_supported(emb, ids, None, None, None, 0)
        assert bert_ops.embed_supported(emb, ids, None, torch.zeros_like(ids), None, 0)
        assert bert_ops.embed_supported(emb, ids[:, :8], None, None, None, 0)
    assert not bert_ops.embed_supported(emb, ids[:, :8], None, None, None, 0)      # no autocast
    emb.word_embeddings.weight.requires_grad_(True)
    with _autocast():
        assert not bert_ops.embed_supported(emb, ids[:, :8], None, None, None, 0)  # a table that trains


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_embed_norm_dropout(dev, p):
    import lora_mask as LM

    from dalm_amd.models import bert_ops, lora_ops

    B, T, D = 64, 32, 256
    emb = _embeddings(D, T, 2, torch.float32, dev)
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(0, VOCAB, (B, T), generator=g).to(dev)
    tt = torch.randint(0, 2, (B, T), generator=g).to(dev)
    lora_ops.advance_dropout_seed(dev)
    seed = int(lora_ops.dropout_seed(dev).item())
    salt = 0x1D5
    with _autocast():
        base = bert_ops.embed_norm(emb, ids, tt, None, 0.0, 0)
        y = bert_ops.embed_norm(emb, ids, tt, None, p, salt)
        again = bert_ops.embed_norm(emb, ids, tt, None, p, salt)
        other = bert_ops.embed_norm(emb, ids, tt, None, p, salt + 1)
    assert torch.equal(y._dalm_bf16, y.to(torch.bfloat16))
    n = B * T * D
    kept = y != 0
    frac = float(kept.float().mean())
    assert abs(frac - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / n), frac             # (a LayerNorm output that is exactly 0: none here)
    assert int((base == 0).sum()) == 0
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    want = base * scale                                                          # f32 x f32, rounded once - as the kernel does
    ulp = torch.abs(torch.nextafter(want, torch.full_like(want, float("inf"))) - want)
    assert bool(((y - want).abs()[kept] <= ulp[kept]).all())
    assert bool((y[~kept] == 0).all())
    assert torch.equal(again, y) and not torch.equal(other != 0, kept)
    mask = torch.from_numpy(LM.keep_mask_v2(seed, salt, B * T, D, p)).to(dev).view(B, T, D)
    assert torch.equal(kept, mask)
    lora_ops.advance_dropout_seed(dev)                                           # another step: another mask
    with _autocast():
        nxt = bert_ops.embed_norm(emb, ids, tt, None, p, salt)
    assert not torch.equal(nxt != 0, kept)


# ---------------------------------------------------------------------------------------------------------------------
# routed vs un-routed model
# ---------------------------------------------------------------------------------------------------------------------
def _encoder(name, hidden, heads, layers=3, vocab=200, seed=0, max_pos=64, pad=PAD):
    cfg_cls, model_cls = _family(name)
    torch.manual_seed(seed)
    return model_cls(cfg_cls(hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=heads, intermediate_size=2 * hidden,
                             vocab_size=vocab, pad_token_id=pad, max_position_embeddings=max_pos, type_vocab_size=1,
                             hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0))


def _right_padded(B, T, lens, lo, hi, seed, pad=PAD):
    ids = torch.randint(lo, hi, (B, T), generator=torch.Generator().manual_seed(seed))
    mask = (torch.arange(T).unsqueeze(0) < torch.tensor(lens).unsqueeze(1)).long()
    return torch.where(mask.bool(), ids, torch.full_like(ids, pad)), mask


@pytest.mark.parametrize("name,hidden,heads", [("XLMRoberta", 256, 4), ("Roberta", 128, 4), ("Camembert", 128, 4)])
def test_routed_model_matches_transformers(dev, name, hidden, heads):
    """A frozen encoder (LoRA-style: nothing trainable but an input perturbation) on "dalm_sdpa" with the patched output modules
    against the same encoder on transformers' code, bf16 autocast, dropout off: hidden states on live rows and input gradients at
    the bounds tests/test_bert_ops_gpu.py holds the BERT layers to.  With the word table frozen too the embeddings kernel is in
    the route: same hidden states."""
    from dalm_amd import packed
    from dalm_amd.models import attention, fastpath, frozen_linear

    ref = _encoder(name, hidden, heads).to(dev).requires_grad_(False).train()
    new = copy.deepcopy(ref)
    assert attention.use_hip_attention_backward(new) and new.config._attn_implementation == attention.NAME == "dalm_sdpa"
    assert packed.attention_is_packable(new) and not packed.attention_is_packable(ref)
    frozen_linear.use_transposed_dgrad(new)
    assert fastpath.use_bert_layer_kernels(new) == 6
    assert fastpath.use_roberta_embeddings(new) == 1
    ids, mask = _right_padded(3, 40, (40, 25, 7), 2, 200, 4)
    ids, mask = ids.to(dev), mask.to(dev)
    up = torch.randn(3, 40, hidden, device=dev)
    outs = []
    for m in (ref, new):
        emb = m.embeddings.word_embeddings.weight
        emb.requires_grad_(True)
        emb.grad = None
        with _autocast():
            h = m(ids, mask)[0]
        assert h.dtype == torch.float32
        (h.float() * mask.unsqueeze(-1) * up).sum().backward()
        outs.append((h.detach(), emb.grad.clone()))
        emb.requires_grad_(False)
    live = mask.bool()
    assert _rel(outs[1][0][live], outs[0][0][live]) < 2e-3
    assert _rel(outs[1][1], outs[0][1]) < 2e-2
    # everything frozen: the embeddings kernel runs (its output has no autograd node and carries the bf16 twin)
    seen = []
    hook = new.embeddings.register_forward_hook(lambda mod, a, out: seen.append(out))
    with torch.no_grad(), _autocast():
        h_new, h_ref = new(ids, mask)[0], ref(ids, mask)[0]
    hook.remove()
    assert getattr(seen[0], "_dalm_bf16", None) is not None
    assert _rel(h_new[live], h_ref[live]) < 2e-3
    with torch.no_grad(), _autocast():
        torch.testing.assert_close(seen[0], ref.embeddings(input_ids=ids), rtol=3e-6, atol=3e-6)


# ---------------------------------------------------------------------------------------------------------------------
# padded step vs packed step
# ---------------------------------------------------------------------------------------------------------------------
class _GradSnapshot:
    def __init__(self, named):
        self.named, self.grads = named, {}

    def __call__(self, *_):
        self.grads = {n: p.grad.detach().float().cpu().clone() for n, p in self.named if p.grad is not None}


def _tiny_llama():
    from transformers import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(5)
    return LlamaForCausalLM(LlamaConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                                        num_key_value_heads=2, vocab_size=80, max_position_embeddings=64, pad_token_id=0, bos_token_id=1,
                                        eos_token_id=2, attention_dropout=0.0))


def _rag_batch():
    B = 6
    qi, qm = _right_padded(B, 12, (12, 5, 3, 9, 1, 7), 3, 80, 21)           # right-padded, row 0 truncated to full length
    pi, pm = _right_padded(B, 24, (24, 11, 17, 6, 20, 13), 3, 80, 22)
    g = torch.Generator().manual_seed(23)
    Tg = 32
    glen = torch.tensor([32, 20, 9, 27, 15, 30]).unsqueeze(1)
    return {"retriever_query_input_ids": qi, "retriever_query_attention_mask": qm, "retriever_passage_input_ids": pi,
            "retriever_passage_attention_mask": pm, "generator_input_input_ids": torch.randint(3, 80, (B, Tg), generator=g),
            "generator_input_attention_mask": (torch.arange(Tg).unsqueeze(0) >= (Tg - glen)).long(),
            "query_passage_input_len": (glen.squeeze(1).float() * 0.8).long().clamp(min=1)}


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


def _per_param(ga, gb):
    """Relative deviation of every parameter's gradient (tests/test_packed_gpu.py: a LoRA factor whose gradient is a rounding-level
    residue of a much larger one is scaled by 5 % of the largest norm of its kind)."""
    big = {}
    for n, t in gb.items():
        kind = n.split(".")[-3] + "." + n.split(".")[0]
        big[kind] = max(big.get(kind, 0.0), float(t.double().norm()))
    return {n: float((ga[n].double() - t.double()).norm()) / max(float(t.double().norm()), 0.05 * big[n.split(".")[-3] + "." + n.split(".")[0]], 1e-30)
            for n, t in gb.items()}


def _host_grad_norm(grads):
    return float(torch.stack([g.double().norm() for g in grads.values()]).norm())


def _count_packed_positions(monkeypatch):
    """Record the padding_idx of every `packed.packed_positions` call: the packed route ran, and with the family's rule."""
    from dalm_amd import packed

    seen, real = [], packed.packed_positions
    monkeypatch.setattr(packed, "packed_positions", lambda ids, rows, padding_idx=None: (seen.append(padding_idx), real(ids, rows, padding_idx))[1])
    return seen


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_packed_rag_step_equals_padded_step(dev, precision, monkeypatch):
    """AutoModelForRagE2E.from_modules(xlmr, tiny_llama, get_peft="both"): loss terms, gradient norm and every LoRA gradient of the
    packed step against the padded step and against the reference's op sequence in fp32 on the host, at the bounds
    tests/test_packed_gpu.py holds the BERT retriever to."""
    import dalm_oracle as O

    from dalm_amd import packed
    from dalm_amd.models import AutoModelForRagE2E, lora
    from dalm_amd.training.step import RagE2EStep

    xlmr, llama = _encoder("XLMRoberta", 128, 2, layers=2, vocab=80, seed=3), _tiny_llama()
    if precision == "bf16":
        with torch.no_grad():
            for mod in (xlmr, llama):
                for p in mod.parameters():
                    p.copy_(p.to(torch.bfloat16).float())
    batch = _rag_batch()
    res, positions = {}, _count_packed_positions(monkeypatch)
    for mode in ("padded", "packed"):
        torch.manual_seed(17)                                               # lora_A's initialisation
        model = AutoModelForRagE2E.from_modules(copy.deepcopy(xlmr), copy.deepcopy(llama), None, None, normalize=True, get_peft="both")
        _prepare_lora(model.retriever_model, 11)
        _prepare_lora(model.generator_model, 12)
        model = model.to(dev)
        assert packed.attention_is_packable(model.retriever_model) and packed.attention_is_packable(model.generator_model)
        if precision == "bf16":
            for p in model.parameters():
                if not p.requires_grad:
                    p.data = p.data.to(torch.bfloat16)
        model.train()
        named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        assert named and all("lora_" in n for n, _ in named)
        opt = torch.optim.SGD([p for _, p in named], lr=0.0)
        snap = _GradSnapshot(named)
        opt.register_step_pre_hook(snap)
        step = RagE2EStep(model, opt, None, 100, autocast_dtype=torch.bfloat16 if precision == "bf16" else None, inplace_grad=True,
                          overlap_towers=True, track_grad_norm=True)
        host = packed.add_pack_plans(dict(batch)) if mode == "packed" else dict(batch)
        dbatch = {k: v.to(dev) for k, v in host.items()}
        loss = float(step(dbatch))
        # the retriever's inputs went through the family's position rule, the generator's through the column rule
        assert sorted(set(map(str, positions))) == (["1", "None"] if mode == "packed" else []), positions
        if mode == "packed":
            assert step._packed_generator(dbatch) and step._retriever_packable(model.retriever_model, dbatch, "retriever_query")
        res[mode] = ({"loss": loss, "contrastive": float(step.aux["contrastive"]), "generator": float(step.aux["generator"]),
                      "grad_norm": float(step.grad_norm)}, snap.grads)
        del model, step, opt
    # the reference's op sequence on the host, fp32, transformers' own modules
    torch.manual_seed(17)
    lora.inject_lora(xlmr, ["key", "query", "value"])
    lora.inject_lora(llama, ["q_proj", "v_proj"])
    _prepare_lora(xlmr, 11)
    _prepare_lora(llama, 12)
    xlmr.train(), llama.train()
    q = O.ref_retrieval_embed(xlmr(batch["retriever_query_input_ids"], batch["retriever_query_attention_mask"])[0],
                              batch["retriever_query_attention_mask"])
    p = O.ref_retrieval_embed(xlmr(batch["retriever_passage_input_ids"], batch["retriever_passage_attention_mask"])[0],
                              batch["retriever_passage_attention_mask"])
    logits = llama(input_ids=batch["generator_input_input_ids"], attention_mask=batch["generator_input_attention_mask"]).logits
    out = O.ref_step_loss(q, p, logits, batch["generator_input_input_ids"], batch["generator_input_attention_mask"],
                          batch["query_passage_input_len"], 100)
    out["loss"].backward()
    g_host = {("retriever_model." + n): p.grad.detach().float() for n, p in xlmr.named_parameters() if p.requires_grad}
    g_host.update({("generator_model." + n): p.grad.detach().float() for n, p in llama.named_parameters() if p.requires_grad})
    host_s = {"loss": float(out["loss"].detach()), "contrastive": float(out["contrastive"].detach()),
              "generator": float(out["generator"].detach()), "grad_norm": _host_grad_norm(g_host)}
    (padded, g_pad), (packd, g_pack) = res["padded"], res["packed"]
    assert set(g_host) == set(g_pad) == set(g_pack)
    keys = ("loss", "contrastive", "generator", "grad_norm")
    rel = {"packed_vs_padded": {k: abs(packd[k] - padded[k]) / max(abs(padded[k]), 1e-30) for k in keys},
           "packed_vs_host": {k: abs(packd[k] - host_s[k]) / max(abs(host_s[k]), 1e-30) for k in keys},
           "padded_vs_host": {k: abs(padded[k] - host_s[k]) / max(abs(host_s[k]), 1e-30) for k in keys}}
    d = {"packed_vs_padded": _per_param(g_pack, g_pad), "packed_vs_host": _per_param(g_pack, g_host), "padded_vs_host": _per_param(g_pad, g_host)}
    print(f"xlm-r RAG step {precision}: {json.dumps(rel)}; worst gradient " + json.dumps({k: max(v.values()) for k, v in d.items()}))
    if precision == "fp32":
        for pair in rel:
            for k in keys:
                assert rel[pair][k] <= 1e-4, (pair, k, rel)
            assert max(d[pair].values()) <= 1e-4, (pair, max(d[pair], key=d[pair].get))
    else:
        for k in keys:
            assert rel["packed_vs_padded"][k] <= (2.2e-3 if k == "grad_norm" else 2.5e-4), (k, rel)
            assert rel["packed_vs_host"][k] <= (7e-3 if k == "grad_norm" else 4e-4), (k, rel)
        for n in d["packed_vs_host"]:
            assert d["packed_vs_host"][n] <= 2.0 * d["padded_vs_host"][n] + 5e-3 and d["packed_vs_host"][n] <= 4e-2, \
                (n, d["packed_vs_host"][n], d["padded_vs_host"][n])


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_packed_retriever_only_step_equals_padded_step(dev, precision, monkeypatch):
    """The retriever-only model (fp32 weights; bf16 = autocast over them, as the retriever-only trainer runs it - the embeddings
    kernel is in both routes there): padded step vs packed step (queries and passages in ONE packed call) vs the host's fp32."""
    import dalm_oracle as O

    from dalm_amd import packed
    from dalm_amd.models import AutoModelForSentenceEmbedding, lora
    from dalm_amd.training.step import RetrieverStep

    xlmr = _encoder("XLMRoberta", 128, 2, layers=2, vocab=80, seed=3)
    b = _rag_batch()
    batch = {"query_input_ids": b["retriever_query_input_ids"], "query_attention_mask": b["retriever_query_attention_mask"],
             "passage_input_ids": b["retriever_passage_input_ids"], "passage_attention_mask": b["retriever_passage_attention_mask"]}
    res, positions = {}, _count_packed_positions(monkeypatch)
    for mode in ("padded", "packed"):
        torch.manual_seed(17)
        model = AutoModelForSentenceEmbedding.from_modules(copy.deepcopy(xlmr), None, normalize=True, get_peft=True)
        _prepare_lora(model.model, 11)
        model = model.to(dev).train()
        assert packed.attention_is_packable(model.model)
        assert model.model.embeddings.forward.__func__.__name__ == "_roberta_embeddings_forward"
        seen = []
        hook = model.model.embeddings.register_forward_hook(lambda mod, a, out: seen.append(getattr(out, "_dalm_bf16", None) is not None))
        named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        opt = torch.optim.SGD([p for _, p in named], lr=0.0)
        snap = _GradSnapshot(named)
        opt.register_step_pre_hook(snap)
        step = RetrieverStep(model, opt, None, 100, autocast_dtype=torch.bfloat16 if precision == "bf16" else None,
                             overlap_towers=True, track_grad_norm=True)
        host = packed.add_pack_plans(batch, packed.RETRIEVER_GROUPS) if mode == "packed" else batch
        loss = float(step({k: v.to(dev) for k, v in host.items()}))
        hook.remove()
        assert positions == ([PAD, PAD] if mode == "packed" else []), positions       # queries + passages, the family's rule
        assert seen and all(seen) == (precision == "bf16"), (mode, seen)      # the kernel's output carries the twin
        res[mode] = ({"loss": loss, "grad_norm": float(step.grad_norm)}, snap.grads)
        del model, step, opt
    torch.manual_seed(17)
    lora.inject_lora(xlmr, ["key", "query", "value"])
    _prepare_lora(xlmr, 11)
    xlmr.train()
    q = O.ref_retrieval_embed(xlmr(batch["query_input_ids"], batch["query_attention_mask"])[0], batch["query_attention_mask"])
    p = O.ref_retrieval_embed(xlmr(batch["passage_input_ids"], batch["passage_attention_mask"])[0], batch["passage_attention_mask"])
    out = O.ref_step_loss(q, p, None, None, None, None, 100)
    out["loss"].backward()
    g_host = {("model." + n): p.grad.detach().float() for n, p in xlmr.named_parameters() if p.requires_grad}
    host_s = {"loss": float(out["loss"].detach()), "grad_norm": _host_grad_norm(g_host)}
    rel = {f"{a}_vs_{c}": {k: abs(x[k] - y[k]) / max(abs(y[k]), 1e-30) for k in ("loss", "grad_norm")}
           for a, x, c, y in (("packed", res["packed"][0], "padded", res["padded"][0]), ("packed", res["packed"][0], "host", host_s),
                              ("padded", res["padded"][0], "host", host_s))}
    print(f"xlm-r retriever-only step {precision}: {json.dumps(rel)}")
    tol = {"loss": 1e-4, "grad_norm": 1e-4} if precision == "fp32" else {"loss": 2.5e-4, "grad_norm": 7e-3}
    for pair, dd in rel.items():
        for k, v in dd.items():
            assert v <= tol[k], (pair, k, rel)
    if precision == "fp32":
        gp, gq = res["packed"][1], res["padded"][1]
        assert set(gp) == set(gq) == set(g_host)
        for n in gq:
            den = max(float(gq[n].double().norm()), 1e-30)
            assert float((gp[n].double() - gq[n].double()).norm()) / den <= 1e-4 or float(gq[n].double().norm()) < 1e-7, n


# ---------------------------------------------------------------------------------------------------------------------
# trainer and evaluation
# ---------------------------------------------------------------------------------------------------------------------
def test_train_retriever_with_and_without_pack_tokens(dev, tmp_path, monkeypatch):
    """Three steps of the retriever-only trainer on a tiny XLM-R around the word-level tokenizer fixture (the config's pad id is the
    tokenizer's), fp32: --pack_tokens keeps the per-step losses (1e-4 relative, the bound of the existing trainer tests) and
    goes the packed way."""
    from transformers import PreTrainedTokenizerFast

    from dalm_amd import packed
    from dalm_amd.models import AutoModelForSentenceEmbedding
    from dalm_amd.training.retriever_only.train_retriever_only import train_retriever

    tok = PreTrainedTokenizerFast.from_pretrained(str(G / "wordlevel_tokenizer"))
    base = _encoder("XLMRoberta", 128, 2, layers=2, vocab=len(tok), seed=6, pad=tok.pad_token_id)
    rows = json.loads((G / "host_golden.json").read_text())["rows"]
    path = tmp_path / "rows.csv"
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["Question", "Abstract", "Answer"])
        for i in range(12):
            k = i % 5
            w.writerow([rows["Question"][k] + " " + str(i), rows["Abstract"][(k + i // 5) % 5], rows["Answer"][k]])
    runs, routed = {}, {}
    real = packed.retrieval_hidden_pair
    for pack in (False, True):
        losses, calls = [], []
        monkeypatch.setattr(packed, "retrieval_hidden_pair", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
        model = AutoModelForSentenceEmbedding.from_modules(copy.deepcopy(base), tok, normalize=True, get_peft=False)
        assert packed.attention_is_packable(model.model) and packed.position_padding_idx(model.model) == tok.pad_token_id
        train_retriever("", str(path), query_max_len=12, passage_max_len=24, per_device_train_batch_size=4, learning_rate=1e-3,
                        num_train_epochs=1, num_warmup_steps=0, output_dir=str(tmp_path / f"out{int(pack)}"), with_tracking=False,
                        seed=7, use_peft=False, use_bnb=False, mixed_precision="no", pack_tokens=pack, model=model,
                        on_step=lambda s, l: losses.append(float(l)))
        runs[pack], routed[pack] = losses, len(calls)
    print("train_retriever(xlm-r) losses, padded / packed:", runs, "python-level calls of the packed route:", routed)
    assert len(runs[True]) == len(runs[False]) == 3
    assert routed[False] == 0 and routed[True] >= 2
    for a, b in zip(runs[False], runs[True]):
        assert abs(a - b) <= 1e-4 * abs(a), runs


def test_packed_sweep_with_an_xlmr_retriever(dev, monkeypatch):
    """`embed_dataset(packed_sweep=True)` with an XLM-R retriever against the padded bf16 forward, both measured against an fp32
    eager run of the same weights (transformers on torch SDPA, mean pooling + normalize restated): the packed sweep may be off by
    twice the padded forward's own error (tests/test_eval_gpu.py::test_packed_sweep_vs_fp32_eager)."""
    import datasets

    from dalm_amd.eval import utils as EU
    from dalm_amd.models import AutoModelForSentenceEmbedding
    from dalm_amd.ops import HipOps

    N, T = 48, 32
    lens = torch.randint(1, T + 1, (N,), generator=torch.Generator().manual_seed(8)).tolist()
    lens[0], lens[1] = T, 1
    ids, mask = _right_padded(N, T, lens, 2, 200, 9)
    ds = datasets.Dataset.from_dict({"retriever_passage_input_ids": ids.tolist(), "retriever_passage_attention_mask": mask.tolist()})
    enc = _encoder("XLMRoberta", 256, 4, layers=2).to(torch.bfloat16)
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
    print(f"xlm-r retriever sweep, max row L2 error vs fp32: padded bf16 {err_padded:.3e}, packed sweep {err_packed:.3e}")
    assert err_padded > 0 and err_packed <= 2 * err_padded
