#!/usr/bin/env python
"""bench.py - training pairs/sec of the RAG-end2end step on N MI355X (one process per GPU).

Workload (BASELINE.json configs[2], the config the headline metric is quoted on; fits one GPU):
    retriever  bge-large-en architecture (BERT 24L/1024/16H/4096, vocab 30522), LoRA r=8 on q/k/v
    generator  Llama-2-7b-hf architecture (32L/4096/32H/11008, vocab 32000), LoRA r=8 on q_proj/v_proj
    per-GPU batch 18, Tq=50, Tp=128, Tg=256, logit_scale 100, Adam lr 1e-4, bf16 autocast
    random-init weights of those architectures + synthetic (Passage, Query, Answer) token rows
    (no network for checkpoints/datasets).
A "step" = passage tower + query tower + generator forward, the fused HIP loss path
(pool/normalise, f32-MFMA similarity + contrastive, marginalised CE with the logits gradient written
in the same pass), backward, gradient all-reduce (N>1), Adam, scheduler, zero_grad - nothing skipped.
With N>1 every rank keeps batch 18 (weak scaling) and the in-batch negatives span the global batch
(RCCL all-gather of the embeddings over xGMI, overlapped with the query tower on a side stream).
Launch structure (`config.launch`): one single-stream hipGraph per tower and direction (generator on the main stream, the retriever
pair on a side stream), loss / optimizer / collectives launched eagerly between them - at every N.  (`--whole-step-graph`: the
whole step as ONE hipGraph, the default of rounds 2-5; a graph captured across two streams replays with a dependency bubble per
node and measures 5-6 ms per step slower on the same box, tools/queue_ab.sh.)

Prints ONE JSON line (rank 0).  `roofline` is for the dominant hand-written kernel
(marg_ce_row_kernel: 2*R*V*el algorithmic bytes per launch, R = B*(Tg-1) dense rows), timed live with
HIP events on the launch stream.  `cpu_baseline` times the reference-equivalent CPU path (oracle
restatement + the same HF architectures) on the host cores, bounded by depth-scaling (see
cpu_reference_baseline).

A plain run sets up, warms up, times the steps, writes --dump-outputs and prints the line: `roofline` then holds only what the
timed steps measured themselves.  `--full` adds everything that needs work of its own after the timed steps: eager steps to time
the dominant kernel behind a whole-step hipGraph, its HBM traffic (rocprofv3 --pmc passes), the loss path alone, the kernel back
to back, the lm_head paths (`f1_lm_head_paths`), `cpu_baseline` (+ `loss_path`) and the `parity` step.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

import dalm_amd  # noqa: E402,F401
import torch  # noqa: E402

HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md)
A100_README_PAIRS_PER_S = 200000.0 / (7 * 3600.0)  # reference README.md:34-40 (1x A100 80GB), BASELINE.md section 1

CFG = dict(B=18, Tq=50, Tp=128, Tg=256, D=1024, V=32000, logit_scale=100)
FULL_ONLY = "bench.py --full measures it"  # what a plain run says where a figure needs work beyond the timed steps


GENERATORS = {
    # name -> (config factory, vocabulary).  Defaults of the HF configs == the published 7B architectures.
    "llama-2-7b": (lambda layers: __import__("transformers").LlamaConfig(num_hidden_layers=layers), 32000),
    "falcon-7b": (lambda layers: __import__("transformers").FalconConfig(num_hidden_layers=layers, hidden_dropout=0.0,
                                                                          attention_dropout=0.0), 65024),
}


def build_models(device, dtype, bert_layers=24, llama_layers=32, lora=True, generator="llama-2-7b", use_bnb=None):
    from transformers import AutoModelForCausalLM, BertConfig, BertModel

    from dalm_amd.models import AutoModelForRagE2E, Mode

    bc = BertConfig(hidden_size=1024, num_hidden_layers=bert_layers, num_attention_heads=16, intermediate_size=4096,
                    vocab_size=30522, max_position_embeddings=512)
    gc = GENERATORS[generator][0](llama_layers)
    torch.manual_seed(0)  # identical weights on every rank
    with torch.device(device):
        old = torch.get_default_dtype()
        torch.set_default_dtype(dtype)
        try:
            retriever = BertModel(bc)
            gen = AutoModelForCausalLM.from_config(gc)
        finally:
            torch.set_default_dtype(old)
    return AutoModelForRagE2E.from_modules(retriever, gen, None, None, normalize=True,
                                           get_peft=Mode.BOTH if lora else None,
                                           use_bnb=Mode(use_bnb) if use_bnb else None)


def _tower_kernels(model) -> dict:
    """Which of this library's tower-side kernels the generator actually runs on (models/fastpath.py, models/lora.py): read
    off the patched modules, not off the environment."""
    from dalm_amd.models import lora as lora_mod

    gen = model.generator_model
    names = {type(m).__name__ for m in gen.modules()}
    fwd = lambda cls: [getattr(m.forward, "__func__", m.forward).__name__ for m in gen.modules() if type(m).__name__ == cls]
    import importlib

    rope = getattr(getattr(importlib.import_module(type(getattr(gen, "base_model", gen)).__module__), "apply_rotary_pos_emb", None),
                   "__name__", None)
    from dalm_amd.models import frozen_linear

    grouped = any(getattr(m, "_group", None) is not None and m._group.enabled for m in gen.modules() if isinstance(m, lora_mod.LoRALinear))
    return {"lora_branch": ("dalm_lora2_* (q / k / v of a block as ONE autograd node, mask bits)" if grouped and lora_mod._GROUPS
                            else "dalm_lora2_* / dalm_lora_* (one node per projection)") if lora_mod._FUSED and "LoRALinear" in names else "eager",
            "frozen_dgrad": "transposed weight copies (F.linear(g, W^T))" if frozen_linear.enabled() and "FrozenLinearT" in names
                            else "autograd (torch.mm(g, W))",
            "rotary": {"_rope_hip": "dalm_rope_qk", "_rope_roll": "roll + addcmul (torch)"}.get(rope, "transformers"),
            "swiglu": "dalm_swiglu_*" if "_swiglu_mlp_forward" in fwd("LlamaMLP") else "transformers",
            "residual_norm": "dalm_rms_norm_*" if "_llama_layer_forward" in fwd("LlamaDecoderLayer") else "transformers / torch",
            "attention": ("dalm_attn_fwd / dalm_attn_bwd (bit-packed mask)"
                          if (getattr(gen.config, "_attn_implementation", None) == "dalm_sdpa"
                              or "_falcon_attention_forward" in fwd("FalconAttention")) else "torch SDPA"),
            "falcon_layer": ("dalm_layer_norm_* / dalm_gelu_* / dalm_add3" if "_falcon_layer_forward" in fwd("FalconDecoderLayer")
                             else None),
            "use_cache": False}


def _matmul_params(module) -> int:
    """Parameters that multiply every token (all 2-D weights except the embedding tables; the lm_head counts even when it is
    tied to the input embedding)."""
    skip = {id(m.weight) for m in module.modules() if isinstance(m, torch.nn.Embedding)}
    n = sum(p.numel() for p in module.parameters() if p.dim() == 2 and id(p) not in skip)
    head = module.get_output_embeddings() if hasattr(module, "get_output_embeddings") else None
    if head is not None and id(head.weight) in skip:
        n += head.weight.numel()
    return n


def step_model_tflops(model, gen_tokens: float, retr_tokens: float) -> float:
    """Informational step-level model FLOPs from THIS model and the token rows that go through its GEMMs:
    2 x matmul-parameters x tokens forward, the same again backward (frozen base + LoRA: activation gradients only; attention
    score products not counted).  cfg3 padded: generator 6.74e9 x 4608 -> 62 + 62 TFLOP, retriever 0.30e9 x 3204 -> 1.9 + 1.9."""
    gen = 4.0 * _matmul_params(model.generator_model) * gen_tokens if getattr(model, "generator_model", None) is not None else 0.0
    retr_mod = getattr(model, "retriever_model", None) or getattr(model, "model", None)
    retr = 4.0 * _matmul_params(retr_mod) * retr_tokens if retr_mod is not None else 0.0
    return (gen + retr) / 1e12


def _resident_weight_bytes(model):
    from dalm_amd.models import nf4

    return {"retriever": nf4.weight_bytes(model.retriever_model), "generator": nf4.weight_bytes(model.generator_model)}


def synthetic_batch(device, seed, B=CFG["B"], Tq=CFG["Tq"], Tp=CFG["Tp"], Tg=CFG["Tg"], V=CFG["V"]):
    """Token-id level synthetic (Passage, Query, Answer) rows, SURVEY.md section 8(d)."""
    g = torch.Generator().manual_seed(seed)

    def ids(n, T, V):
        return torch.randint(1000, V, (n, T), generator=g)

    def right_mask(T, lo, hi):
        lens = torch.randint(lo, hi + 1, (B, 1), generator=g)
        return (torch.arange(T).unsqueeze(0) < lens).long()

    glen = torch.randint(60, Tg + 1, (B, 1), generator=g)
    gmask = (torch.arange(Tg).unsqueeze(0) >= (Tg - glen)).long()  # Llama tokenizers pad left
    batch = {
        "retriever_query_input_ids": ids(B, Tq, 30522), "retriever_query_attention_mask": right_mask(Tq, 5, 15),
        "retriever_passage_input_ids": ids(B, Tp, 30522), "retriever_passage_attention_mask": right_mask(Tp, 30, Tp),
        "generator_input_input_ids": ids(B, Tg, V), "generator_input_attention_mask": gmask,
        "query_passage_input_len": (glen.squeeze(1).float() * 0.8).long().clamp(min=1),
    }
    return {k: v.to(device) for k, v in batch.items()}


def bucketed_batches(device, seed, V, n_batches=12):
    """The trainer's opt-in host data path on synthetic rows: a pool of n_batches * B rows is ordered by generator length
    (`shards.bucketed_order`), cut into batches of B and every batch loses its all-padding columns (`shards.trim_batch`)."""
    from dalm_amd.training.shards import bucketed_order, trim_batch

    B = CFG["B"]
    pool = [synthetic_batch(torch.device("cpu"), seed + i, V=V) for i in range(n_batches)]
    rows = {k: torch.cat([b[k] for b in pool]) for k in pool[0]}
    lengths = (rows["generator_input_attention_mask"] != 0).sum(dim=1)
    order = bucketed_order(lengths, B, torch.Generator().manual_seed(seed))
    groups = [("retriever_query_input_ids", "retriever_query_attention_mask"),
              ("retriever_passage_input_ids", "retriever_passage_attention_mask"),
              ("generator_input_input_ids", "generator_input_attention_mask")]
    out = []
    for i in range(n_batches):
        idx = order[i * B:(i + 1) * B]
        host = trim_batch({k: v.index_select(0, idx) for k, v in rows.items()}, groups,
                          qlen_key="query_passage_input_len", qlen_follows="generator_input_attention_mask")
        out.append({k: v.to(device) for k, v in host.items()})
    return out


class TimedOps:
    """HipOps with HIP events around the dominant kernel launch (marginalised CE, fused fwd+grad)."""

    def __init__(self):
        from dalm_amd.ops import HipOps

        self._ops = HipOps()
        self.events = []
        self.enabled = False

    def __getattr__(self, name):
        return getattr(self._ops, name)

    def ce_fwd(self, logits, ids, mask, stats, want_grad, inplace=False):
        if not self.enabled:
            return self._ops.ce_fwd(logits, ids, mask, stats, want_grad, inplace)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        # recorded inside HipOps.ce_fwd on torch's current stream (== the stream the kernel is launched on), right
        # around the launch: output allocation and argument marshalling are not inside the interval
        out = self._ops.ce_fwd(logits, ids, mask, stats, want_grad, inplace, events=(a, b))
        # bytes this launch really has to move: live rows are read once; with want_grad every row of the
        # [B,Tg,V] gradient is written (zeros for masked rows and the last position)
        B, Tg, V = logits.shape
        live = (mask[:, 1:] != 0).sum()  # stays on the device: no host sync inside the timed region
        self.events.append((a, b, live, (B * Tg if want_grad else 0), V * logits.element_size()))
        return out


def ce_back_to_back_probe(dev, batch, dtype, V, launches=20):
    """The dominant kernel (fused CE forward + gradient, in place) at the step's shapes and masks, `launches` times back to
    back between ONE pair of HIP events on the launch stream: the per-launch event pair of the in-step number brackets a
    few microseconds of launch gap with every kernel (89 vs 84 us by rocprofv3 in round 4); this is the same kernel with
    that gap amortised, for comparison with the rocprofv3 average under profiles/."""
    from dalm_amd.ops import HipOps

    ops = HipOps()
    ids, mask = batch["generator_input_input_ids"], batch["generator_input_attention_mask"]
    g = torch.Generator(device="cpu").manual_seed(0)
    logits = torch.randn(ids.shape[0], ids.shape[1], V, generator=g).to(dev, dtype)
    stats, _, _ = ops.ce_prep(mask, batch["query_passage_input_len"])
    for _ in range(3):
        ops.ce_fwd(logits, ids, mask, stats, True, True)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        ops.ce_fwd(logits, ids, mask, stats, True, True)
    b.record()
    torch.cuda.synchronize()
    us = a.elapsed_time(b) * 1e3 / launches
    live = int((mask[:, 1:] != 0).sum())
    nbytes = (live + ids.shape[0] * ids.shape[1]) * V * logits.element_size()
    del logits
    torch.cuda.empty_cache()
    return us, nbytes / (us * 1e-6) / 1e9


class _ReferenceLossCode:
    """The REFERENCE'S OWN loss functions ("run the reference code itself") behind the two entry points the CPU
    baselines call: dalm/training/utils/train_utils.py:76-138 and AutoModelForRagE2E.mean_pooling
    (dalm/models/rag_e2e_base_model.py:108-111), composed as train_rage2e.py:431-467 composes them.  Importable only where
    /root/reference exists (the build container; the GPU box has no copy of the reference): there `kind` = "reference"."""

    kind = "reference"

    def __init__(self, root):
        import types

        import transformers  # noqa: F401  (resolve it before the stub goes in, as oracle/make_golden.py does)

        stub = types.ModuleType("peft")        # the image has no peft; the reference only needs the four names to import
        for name in ("LoraConfig", "PeftModel", "TaskType", "get_peft_model"):
            setattr(stub, name, type(name, (), {}))
        sys.modules["peft"] = stub
        sys.path.insert(0, str(root))
        try:
            import dalm.models.rag_e2e_base_model as m_rag
            import dalm.training.utils.train_utils as tu
        finally:
            sys.modules.pop("peft", None)
            sys.path.remove(str(root))
        self.tu, self.m_rag = tu, m_rag

    def ref_retrieval_embed(self, token_states, mask):
        e = self.m_rag.AutoModelForRagE2E.mean_pooling(None, token_states, mask)
        return torch.nn.functional.normalize(e, p=2, dim=1)

    def ref_step_loss(self, q, p, logits, ids, mask, qlen, scale):
        tu = self.tu
        S = tu.get_cosine_sim(q, p, scale)
        con = (tu.get_nt_xent_loss(S) + tu.get_nt_xent_loss(S.t())) / 2.0
        gen = tu.compute_marginalized_loss_from_logits(logits, ids, mask, S, qlen)
        return {"loss": con + gen, "contrastive": con, "generator": gen}


def _cpu_loss_code():
    """(implementation, kind): the reference's own functions when /root/reference is present, else the oracle restatement
    ("port": oracle/dalm_oracle.py ref_*, pinned to the reference by tests/test_oracle_golden.py)."""
    root = Path(os.environ.get("DALM_REFERENCE_ROOT", "/root/reference"))
    if (root / "dalm" / "training" / "utils" / "train_utils.py").exists():
        try:
            return _ReferenceLossCode(root), "reference"
        except Exception:
            pass
    sys.path.insert(0, str(ROOT / "oracle"))
    import dalm_oracle as O

    return O, "port"


def cpu_loss_path_baseline(batch_cpu, V):
    """SURVEY 8d level (i), the like-for-like number for what this repo replaces: the reference's LOSS PATH op sequence
    (oracle ref_*: mean-pool + normalise x2, get_cosine_sim, get_nt_xent_loss x2, compute_marginalized_loss_from_logits),
    forward + backward in fp32 at the step's full shapes on the host cores - beside `roofline.loss_path_us`."""
    O, kind = _cpu_loss_code()
    threads = min(os.cpu_count() or 1, 16)
    torch.set_num_threads(threads)
    B, Tq, Tp, Tg, D = CFG["B"], CFG["Tq"], CFG["Tp"], CFG["Tg"], CFG["D"]
    g = torch.Generator().manual_seed(0)
    hq = torch.randn(B, Tq, D, generator=g, requires_grad=True)
    hp = torch.randn(B, Tp, D, generator=g, requires_grad=True)
    logits = torch.randn(B, Tg, V, generator=g, requires_grad=True)
    best = None
    for it in range(3):
        for t in (hq, hp, logits):
            t.grad = None
        t0 = time.time()
        q = O.ref_retrieval_embed(hq, batch_cpu["retriever_query_attention_mask"])
        p = O.ref_retrieval_embed(hp, batch_cpu["retriever_passage_attention_mask"])
        out = O.ref_step_loss(q, p, logits, batch_cpu["generator_input_input_ids"], batch_cpu["generator_input_attention_mask"],
                              batch_cpu["query_passage_input_len"], CFG["logit_scale"])
        out["loss"].backward()
        dt = time.time() - t0
        if it > 0:                       # first pass warms the thread pool / allocator
            best = dt if best is None else min(best, dt)
    return {"ms": 1e3 * best, "cores": threads, "kind": kind,
            "what": f"reference loss-path op sequence ({'the reference package itself' if kind == 'reference' else 'oracle ref_*'}), fwd+bwd, fp32, [B={B},Tg={Tg},V={V}] logits + pooling of "
                    f"[{B},{Tq}|{Tp},{D}] token states; min of 2 after a warm-up"}


def f1_head_paths(dev, batch, model, iters=6):
    """lm_head + marginalised CE + d(hidden) of THIS batch's generator rows through (a) the library's own bf16
    MFMA kernels end to end (`fused._lm_head_train_kernel`: forward lse, logits recomputed per vocabulary chunk for the
    backward - nothing [rows, V]-sized is allocated) and (b) the chunked library path (torch.mm + the fused CE kernel), both
    over the live rows; run alone after the timed region, HIP events around `iters` eager calls each.  The timed step itself
    uses whichever path its flags select (default: materialised logits + the fused CE kernel)."""
    from dalm_amd.fused import gemm_wave_rows, live_row_index, rag_e2e_loss_from_hidden

    head = model.generator_model.get_output_embeddings()
    W = head.weight.detach()
    if W.dtype != torch.bfloat16 or W.requires_grad or getattr(head, "bias", None) is not None:
        return None
    V, H = W.shape
    ids, mask, qlen = batch["generator_input_input_ids"], batch["generator_input_attention_mask"], batch["query_passage_input_len"]
    B, Tg = ids.shape
    g = torch.Generator(device=dev).manual_seed(0)
    h = torch.randn(B, Tg, H, device=dev, dtype=torch.bfloat16, generator=g)
    q = torch.nn.functional.normalize(torch.randn(B, 1024, device=dev, generator=g), dim=1)
    p = torch.nn.functional.normalize(torch.randn(B, 1024, device=dev, generator=g), dim=1)
    live = live_row_index(mask, multiple=gemm_wave_rows(V))
    live = live.to(dev) if live is not None else None
    res = {}
    saved = os.environ.get("DALM_LM_HEAD_TRAIN_KERNEL")
    try:
        for name, env in (("kernels", "1"), ("kernels2", "2"), ("library", "0")):
            os.environ["DALM_LM_HEAD_TRAIN_KERNEL"] = env

            def call():
                hh = h.clone().requires_grad_(True)
                loss = rag_e2e_loss_from_hidden(q, p, hh, W, ids, mask, qlen, CFG["logit_scale"], live_rows=live)
                loss.backward()
                return loss.detach(), hh.grad

            for _ in range(2):
                loss, dh = call()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                loss, dh = call()
            e1.record()
            torch.cuda.synchronize()
            res[name] = (e0.elapsed_time(e1) / iters, float(loss), dh.float())
    finally:
        if saved is None:
            os.environ.pop("DALM_LM_HEAD_TRAIN_KERNEL", None)
        else:
            os.environ["DALM_LM_HEAD_TRAIN_KERNEL"] = saved
    k, l, k2 = res["kernels"], res["library"], res["kernels2"]
    return {"rows": int(live.numel()) if live is not None else B * Tg, "V": V, "H": H,
            "kernels_ms": k[0], "library_ms": l[0], "kernels_over_library": k[0] / l[0],
            "kernels_two_contractions_ms": k2[0], "kernels_two_contractions_over_library": k2[0] / l[0],
            "kernels_two_contractions_dhidden_rel_diff": float((k2[2] - l[2]).norm() / l[2].norm()),
            "loss_rel_diff": abs(k[1] - l[1]) / max(abs(l[1]), 1e-30),
            "dhidden_rel_diff": float((k[2] - l[2]).norm() / l[2].norm()),
            "note": "lm_head + marginalised CE + d(hidden) over the live rows, eager launches (HIP events over "
                    f"{iters} calls): `kernels` = dalm_lm_head_lse_fwd + dalm_lm_head_dlogits / dalm_transpose_bf16 / "
                    "dalm_lm_head_dhidden (three contractions, the logits recomputed; workspace <= 160 MB), `kernels_two_contractions` "
                    "= dalm_lm_head_logits + the fused CE kernel in place + dalm_lm_head_dhidden per row chunk (hand-written, no "
                    "recomputation: the chunk's logits stay in the Infinity Cache; DALM_LM_HEAD_TRAIN_KERNEL=2), `library` = torch.mm "
                    "x2 + the fused CE kernel in row chunks.  RagE2EStep(fuse_lm_head='auto') takes the fused path when a batch's "
                    "logits would exceed DALM_LOGITS_BUDGET_MB (1024)"}


def gpu_loss_path_probe(dev, batch, dtype, V, iters=20):
    """GPU time of the HIP loss path alone at the step's shapes (pool + normalise x2, similarity / contrastive, marginalised CE
    with the gradient written in the same pass, finalize, and the backward of all of them down to the token states): tower
    outputs are random tensors of the right shapes, `iters` forward+backward passes are captured in ONE hipGraph so the host
    is out of the number.  Returns microseconds per pass."""
    from dalm_amd.fused import pool_l2norm, rag_e2e_loss

    B, Tq, Tp, Tg, D = CFG["B"], CFG["Tq"], CFG["Tp"], CFG["Tg"], CFG["D"]
    g = torch.Generator().manual_seed(0)
    hq = torch.randn(B, Tq, D, generator=g).to(dev, dtype).requires_grad_(True)
    hp = torch.randn(B, Tp, D, generator=g).to(dev, dtype).requires_grad_(True)
    logits = torch.randn(B, Tg, V, generator=g).to(dev, dtype).requires_grad_(True)

    def one():
        q = pool_l2norm(hq, batch["retriever_query_attention_mask"], True)
        p = pool_l2norm(hp, batch["retriever_passage_attention_mask"], True)
        loss = rag_e2e_loss(q, p, logits, batch["generator_input_input_ids"], batch["generator_input_attention_mask"],
                            batch["query_passage_input_len"], CFG["logit_scale"], inplace_grad=True)
        loss.backward()
        hq.grad = hp.grad = logits.grad = None

    how = "hipGraph of %d passes" % iters
    try:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                one()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(iters):
                one()
        gr.replay()
        torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); gr.replay(); b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) * 1e3 / iters)
        us = sorted(ts)[len(ts) // 2]
    except Exception as e:   # same kernels launched eagerly: the host launch path is then inside the number
        torch.cuda.synchronize()
        how = f"eager launches (graph capture failed: {e!r}): includes host launch gaps"
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            one()
        b.record()
        torch.cuda.synchronize()
        us = a.elapsed_time(b) * 1e3 / iters
    return us, how


def collect_ce_traffic(workload, dtype, V, timeout_s=150):
    """HBM bytes per launch of the dominant kernel from rocprofv3 PMC passes run NOW, around tools/ce_traffic_probe.py (the
    same kernel at the bench's shapes and masks): FETCH_SIZE and WRITE_SIZE in separate passes, FETCH doubled as the gfx950
    guide prescribes.  Returns (bytes or None, source string)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile

    exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if exe is None:
        return None, "not collected this run: rocprofv3 not on PATH"
    B, Tg = CFG["B"], CFG["Tg"]
    vals = {}
    tmp = tempfile.mkdtemp(prefix="dalm_pmc_", dir="/tmp")
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(tmp, counter)
            cmd = [exe, "--pmc", counter, "--output-format", "csv", "-d", d, "--", sys.executable,
                   str(ROOT / "tools" / "ce_traffic_probe.py"), "--workload", workload, "--dtype", dtype]
            try:
                subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), timeout=timeout_s,
                               stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            except subprocess.TimeoutExpired:
                return None, f"not collected this run: rocprofv3 --pmc {counter} pass exceeded {timeout_s} s"
            got = []
            for f in glob.glob(d + "/**/*counter_collection.csv", recursive=True):
                for r in csv.DictReader(open(f)):
                    if (r.get("Counter_Name") == counter and "marg_ce" in r["Kernel_Name"]
                            and int(r["Grid_Size"]) // max(int(r["Workgroup_Size"]), 1) == B * Tg):
                        got.append(float(r["Counter_Value"]))
            if not got:
                return None, f"not collected this run: no {counter} rows for the CE kernel in the rocprofv3 output"
            vals[counter] = sum(got) / len(got)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    total = 2.0 * vals["FETCH_SIZE"] * 1024.0 + vals["WRITE_SIZE"] * 1024.0
    return total, (f"rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE (separate passes) run by this bench.py invocation around "
                   f"tools/ce_traffic_probe.py (the same kernel, shapes and masks as the timed step): mean over its launches, "
                   f"FETCH_SIZE x 2 x 1024 (gfx950 correction) + WRITE_SIZE x 1024 = {2.0 * vals['FETCH_SIZE'] * 1024.0:.4g} + "
                   f"{vals['WRITE_SIZE'] * 1024.0:.4g} bytes")


def step_parity_block(dev, model_cpu, batch_cpu):
    """One fp32 step of the depth-1 full-width model on the HOST through the reference's op sequence (oracle ref_*) and on
    the GPU through RagE2EStep, same weights (deep copy), dropout off: loss and global gradient norm, relative."""
    import copy

    sys.path.insert(0, str(ROOT / "oracle"))
    import dalm_oracle as O
    from dalm_amd.training.step import RagE2EStep

    model_cpu.eval()
    model_cpu.zero_grad()
    m = model_cpu
    qh = m.retriever_model(batch_cpu["retriever_query_input_ids"], batch_cpu["retriever_query_attention_mask"])[0]
    ph = m.retriever_model(batch_cpu["retriever_passage_input_ids"], batch_cpu["retriever_passage_attention_mask"])[0]
    q = O.ref_retrieval_embed(qh, batch_cpu["retriever_query_attention_mask"])
    p = O.ref_retrieval_embed(ph, batch_cpu["retriever_passage_attention_mask"])
    logits = m.generator_model(input_ids=batch_cpu["generator_input_input_ids"],
                               attention_mask=batch_cpu["generator_input_attention_mask"]).logits
    out = O.ref_step_loss(q, p, logits, batch_cpu["generator_input_input_ids"], batch_cpu["generator_input_attention_mask"],
                          batch_cpu["query_passage_input_len"], CFG["logit_scale"])
    out["loss"].backward()
    params = [x for x in m.parameters() if x.requires_grad]
    cpu = {"loss": float(out["loss"].detach()),
           "grad_norm": float(torch.sqrt(sum((x.grad.double() ** 2).sum() for x in params if x.grad is not None)))}
    m.zero_grad()
    g = copy.deepcopy(m).to(dev)
    g.eval()
    gp = [x for x in g.parameters() if x.requires_grad]
    step = RagE2EStep(g, torch.optim.SGD(gp, lr=0.0), None, CFG["logit_scale"], autocast_dtype=None, inplace_grad=True,
                      overlap_towers=False, track_grad_norm=True)
    loss = step({k: v.to(dev) for k, v in batch_cpu.items()})
    gpu = {"loss": float(loss), "grad_norm": float(step.grad_norm)}
    del g, step
    torch.cuda.empty_cache()
    rel = {k: abs(gpu[k] - cpu[k]) / max(abs(cpu[k]), 1e-30) for k in cpu}
    return {"what": "one fp32 step, depth-1 towers at full cfg3 width (bge-large 1024, Llama-2-7b 4096 / V 32000, LoRA), batch 18, "
                    "dropout off: HIP loss path + PyTorch-ROCm towers vs the reference op sequence (oracle ref_*) on the host",
            "host": cpu, "gpu": gpu, "rel": rel, "tolerance": 1e-3, "ok": max(rel.values()) <= 1e-3}


def cpu_reference_baseline(max_seconds=90.0, parity_dev=None):
    """Reference CPU path on the host cores, bounded (~50 s): the oracle restatement of the reference's
    loss code at the full cfg3 shapes around the same HF architectures (LoRA, fp32) at depth 1 and
    depth 2 instead of 24 / 32 layers, median of 3 steps each; the per-layer increment is extrapolated to full
    depth.  Threads: min(host cores, 16) - measured on the 256-core GPU-box host, 16 threads is the
    fastest setting for this eager-torch workload (16: 4.9 s, 32: 5.5 s, 64: 6.8 s, 256: 80 s per
    depth-1 step), so this is the CPU path at its best, and `cores` reports the threads used.
    Loss code: the reference package itself where /root/reference exists (`kind` "reference"), the oracle restatement
    otherwise (`kind` "port": the GPU box has no copy of the reference)."""
    O, kind = _cpu_loss_code()
    threads = min(os.cpu_count() or 1, 16)
    torch.set_num_threads(threads)
    dev = torch.device("cpu")
    times, spread = {}, {}
    parity = None
    t_start = time.time()
    for depth in (1, 2):
        model = build_models(dev, torch.float32, bert_layers=depth, llama_layers=depth)
        model.train()
        params = [p for p in model.parameters() if p.requires_grad]
        opt = torch.optim.Adam(params, lr=1e-4)
        batch = synthetic_batch(dev, 0)

        def step():
            qh = model.retriever_model(batch["retriever_query_input_ids"], batch["retriever_query_attention_mask"])[0]
            ph = model.retriever_model(batch["retriever_passage_input_ids"], batch["retriever_passage_attention_mask"])[0]
            q = O.ref_retrieval_embed(qh, batch["retriever_query_attention_mask"])
            p = O.ref_retrieval_embed(ph, batch["retriever_passage_attention_mask"])
            logits = model.generator_model(input_ids=batch["generator_input_input_ids"],
                                           attention_mask=batch["generator_input_attention_mask"]).logits
            out = O.ref_step_loss(q, p, logits, batch["generator_input_input_ids"],
                                  batch["generator_input_attention_mask"], batch["query_passage_input_len"],
                                  CFG["logit_scale"])
            out["loss"].backward()
            opt.step()
            model.zero_grad()

        if depth == 1:
            step()  # warm-up (thread pools, allocator)
        samples = []
        for _ in range(3):          # median of 3 (one un-repeated step swung 26 % between rounds)
            t0 = time.time()
            step()
            samples.append(time.time() - t0)
        times[depth] = sorted(samples)[1]
        spread[depth] = (min(samples), max(samples))
        if depth == 1 and parity_dev is not None:
            try:        # the weights have taken two Adam steps by now: lora_B is no longer zero, both LoRA factors carry gradient
                parity = step_parity_block(parity_dev, model, batch)
            except Exception as e:
                parity = {"ok": None, "error": repr(e)}
        del model, opt
        if time.time() - t_start > max_seconds:
            break
    if len(times) == 2:
        delta = max(times[2] - times[1], 0.0)   # one more BERT layer (both towers) + one more Llama layer
        fixed = max(times[1] - delta, 0.0)      # embeddings, lm_head, loss path, Adam
        # split the increment by layer FLOPs (Llama layer 202 M params x 4608 tokens vs BERT layer
        # 12.6 M x 3204 tokens -> 95.8 % / 4.2 %) and scale each share to its true depth (32 / 24)
        full = fixed + delta * (0.958 * 32 + 0.042 * 24)
        code = "the reference's own loss functions" if kind == "reference" else "oracle loss code"
        note = (f"reference-equivalent CPU step ({code} at full cfg3 shapes + HF towers, LoRA, fp32, "
                f"{threads} threads): median of 3 steps per depth after a warm-up step - depth 1 = {times[1]:.2f} s "
                f"(min {spread[1][0]:.2f}, max {spread[1][1]:.2f}), depth 2 = {times[2]:.2f} s (min {spread[2][0]:.2f}, max "
                f"{spread[2][1]:.2f}); per-layer increment extrapolated to 24 BERT / 32 Llama layers -> {full:.1f} s per "
                f"18-pair step (the extrapolation multiplies the depth-2 minus depth-1 difference by ~32: quote it as +-30 %)")
    else:
        full = times[1] * 30.0
        note = (f"depth-1 towers only (median of 3: {times[1]:.2f} s/step, min {spread[1][0]:.2f}, max {spread[1][1]:.2f}, "
                f"{threads} threads) x30 (time bound hit before depth 2)")
    return {"value": CFG["B"] / full, "unit": "training pairs/s", "cores": threads, "kind": kind, "sample": note}, parity


DUMP_BUDGET_BYTES = 64 << 20


def dump_outputs(out_dir, loss, model) -> None:
    """--dump-outputs DIR: what the timed step handed back in its last step - the loss it returned (float64) and the trainable
    parameters the optimizer wrote (float32) - as DIR/<name>.npy, so that two builds can be compared output for output.
    Above DUMP_BUDGET_BYTES every parameter keeps the same seeded sample of its elements (flattened, ascending index)."""
    import numpy as np

    out = Path(out_dir)
    out.mkdir(parents=True, exist_ok=True)
    np.save(out / "loss.npy", np.asarray([float(loss)], dtype=np.float64))
    params = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    total = sum(p.numel() for _, p in params) * 4
    for name, p in params:
        a = p.detach().float().cpu()
        if total > DUMP_BUDGET_BYTES:
            keep = max(1, p.numel() * DUMP_BUDGET_BYTES // total)
            a = a.flatten()[torch.randperm(p.numel(), generator=torch.Generator().manual_seed(0))[:keep].sort().values]
        np.save(out / f"param.{name}.npy", a.numpy())


def _flush_c_stdio() -> None:
    """RCCL prints its version banner through C stdio; on a pipe that buffer is flushed at process exit - AFTER Python's own
    output, i.e. after the JSON line.  Flush it now so that the JSON line stays the LAST line on stdout."""
    try:
        import ctypes

        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure what the headline does not need (see the module docstring): "
                         "probe kernels, PMC traffic, f1 lm_head paths, CPU baselines, parity step")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip cpu_baseline, loss_path and parity")
    ap.add_argument("--no-pmc", action="store_true",
                    help="with --full: skip the two rocprofv3 --pmc passes (FETCH_SIZE / WRITE_SIZE of the dominant kernel, ~30 s) "
                         "that fill roofline.traffic")
    ap.add_argument("--no-graph", action="store_true", help="launch the step eagerly instead of replaying a hipGraph")
    ap.add_argument("--no-overlap", action="store_true", help="run the retriever towers on the main stream")
    ap.add_argument("--graph-collectives", action="store_true",
                    help="W > 1: capture the WHOLE step including the RCCL collectives in one hipGraph.  Needs the library's own "
                         "communicator (dalm_comm_*_on enqueue on the capturing stream; implies DALM_NATIVE_COMM=1 - a capture "
                         "around torch.distributed's nccl ops aborts).  Measured with one rank: 192.7 ms/step against 188.1 ms "
                         "for graphed towers + eager collectives, so the latter stays the default")
    ap.add_argument("--graph-towers", action="store_true",
                    help="graph the tower fwd/bwd (one single-stream hipGraph per tower and direction) and launch loss / optimizer / "
                         "collectives eagerly between them: the default at every rank count since round 6 (bucketed data path "
                         "excepted: more batch shapes than tower-graph sets)")
    ap.add_argument("--whole-step-graph", action="store_true",
                    help="one rank: capture the WHOLE step (both streams, loss, optimizer) as ONE hipGraph - the default of rounds "
                         "2-5.  A graph captured across two streams replays with a dependency bubble at every node (1400 idle gaps "
                         "per step in the kernel trace against 180): measured 5-6 ms per step slower than the tower graphs on the "
                         "same box (tools/queue_ab.sh)")
    ap.add_argument("--fuse-lm-head", action="store_true",
                    help="SURVEY 8(f) rank 1: chunked lm_head + CE, the [B,Tg,V] logits are never materialised")
    ap.add_argument("--data-path", default="fixed", choices=["fixed", "bucketed", "loader", "packed"],
                    help="fixed (default, the named configuration): every batch padded to Tq50/Tp128/Tg256 and resident in HBM "
                         "before the timed region; loader: the same rows fed through the trainer's host data path inside the "
                         "timed loop (ShardedBatches: int32 pinned columns, one index_select per column into pinned staging, "
                         "H2D of batch i+1 on a copy stream) - shows what the loader costs the step; bucketed: the trainer's "
                         "opt-in --length_bucketing + --trim_padding applied to a pool of synthetic rows "
                         "(extra lines next to the headline, never the headline); packed: the SAME rows of the SAME named "
                         "configuration as `fixed`, resident in HBM, with the host-side list of live tokens next to every mask "
                         "(dalm_amd/packed.py): both towers run on the un-padded [n_live, H] rows (per-sequence attention through "
                         "dalm_attn_*_packed, original positions kept) - padding contributes exactly zero to the reference's loss "
                         "and gradients, so the step computes the same update; a line BESIDE the padded headline")
    ap.add_argument("--all-rows", action="store_true",
                    help="with --fuse-lm-head: run the padding rows through the lm_head GEMMs too (sample chunks)")
    ap.add_argument("--workload", default="cfg3", choices=["cfg3", "cfg5", "cfg2", "cfg1"],
                    help="cfg3 = RAG-e2e bge-large + Llama-2-7b batch 18 (headline, default); "
                         "cfg5 = RAG-e2e bge-large + Falcon-7B architecture (V = 65024: the 1024-thread CE rows); "
                         "cfg2 = retriever-only bge-large batch 150 (BASELINE.json configs[1]); "
                         "cfg1 = retriever-only bge-small batch 19 (the toy-CSV shape of configs[0])")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"],
                    help="bf16 = bf16 weights + autocast (default); fp32 = fp32 weights, no autocast "
                         "(the reference's default precision; quoted beside the bf16 line in DESIGN.md)")
    ap.add_argument("--use-bnb", default=None, choices=["generator", "retriever", "both"],
                    help="extra line, not the headline: the reference's use_bnb - frozen base Linears of the named tower(s) "
                         "held as nf4 (dalm_nf4_* kernels), dequantised to bf16 in front of every GEMM")
    ap.add_argument("--through-trainer", action="store_true",
                    help="extra line, not the headline: run the TRAINER ENTRY POINT itself (train_e2e; train_retriever for cfg2) at "
                         "this workload's full size on a synthetic csv - tokenise -> token cache -> ShardedBatches -> GraphedStep "
                         "(incl. the partial last batch) -> step_N checkpoint -> kill -> --resume_from_checkpoint - and report "
                         "the trainer's own pairs/s (tools/trainer_bench.py)")
    ap.add_argument("--trainer-rows", type=int, default=10000, help="rows of the synthetic csv for --through-trainer")
    ap.add_argument("--bench-line", default=None, help="--through-trainer: file with this workload's bench.py line (ratio)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps write what the last one computed (loss, updated trainable parameters) as DIR/<name>.npy")
    ap.add_argument("--retriever-layers", type=int, default=24, help=argparse.SUPPRESS)
    ap.add_argument("--generator-layers", type=int, default=32, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit("--steps must be at least 1")

    from dalm_amd.launch import in_distributed_env, spawn_ranks

    if args.through_trainer:
        if args.dump_outputs:
            raise SystemExit("--dump-outputs is not available with --through-trainer")
        if args.gpus != 1 or args.workload == "cfg1":
            raise SystemExit("--through-trainer runs on one GPU at cfg3 / cfg5 / cfg2")
        sys.path.insert(0, str(ROOT / "tools"))
        import trainer_bench

        argv = ["--workload", args.workload, "--rows", str(args.trainer_rows), "--retriever-layers", str(args.retriever_layers),
                "--generator-layers", str(args.generator_layers)] + (["--bench-line", args.bench_line] if args.bench_line else []) \
            + (["--pack-tokens"] if args.data_path == "packed" else [])
        return trainer_bench.main(argv)
    if args.gpus > 1 and not in_distributed_env():
        # `python bench.py --gpus N`: no torchrun needed - spawn one rank per GPU ourselves (RANK / LOCAL_RANK /
        # WORLD_SIZE / MASTER_ADDR=127.0.0.1), rank 0 prints the JSON line; fewer than N visible GPUs -> exit 2
        raise SystemExit(spawn_ranks([sys.executable, str(Path(__file__).resolve())] + sys.argv[1:], args.gpus))
    if args.graph_collectives:
        os.environ["DALM_NATIVE_COMM"] = "1"       # a capture needs the collectives on the capturing stream: insist
    args.hw_queues = dalm_amd.configure_hw_queues(args.gpus)   # before the HIP runtime starts

    from dalm_amd import hip
    from dalm_amd.sharded import barrier, init_distributed
    from dalm_amd.training.step import RagE2EStep

    hip.load()  # no HIP extension -> fail here, loudly
    from dalm_amd.tuning import enable_tuned_gemms

    args.tuned_gemms = enable_tuned_gemms()  # replay-only hipBLASLt/rocBLAS solution table for the tower GEMMs
    if args.workload in ("cfg2", "cfg1"):
        return main_retriever_only(args)
    comm, dev = init_distributed()
    if dev.type != "cuda":
        raise SystemExit("bench.py needs an MI355X (no CPU fallback for the product path)")
    if comm.world_size != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but the launcher set WORLD_SIZE={comm.world_size}")
    rank = comm.rank
    gen_name = "falcon-7b" if args.workload == "cfg5" else "llama-2-7b"
    V = GENERATORS[gen_name][1]
    wdtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    autocast = torch.bfloat16 if args.dtype == "bf16" else None

    model = build_models(dev, wdtype, args.retriever_layers, args.generator_layers, generator=gen_name, use_bnb=args.use_bnb)
    model.train()
    params = [p for p in model.parameters() if p.requires_grad]
    from transformers import get_scheduler

    from dalm_amd.fused import LocalComm
    from dalm_amd.training.graphed import GraphedStep, TensorLRScheduler, make_capturable_adam

    towers_default = (isinstance(comm, LocalComm) and not args.whole_step_graph and not args.graph_collectives
                      and args.data_path != "bucketed")
    args.graph_towers = args.graph_towers or towers_default
    use_graph = (isinstance(comm, LocalComm) or args.graph_collectives) and not args.no_graph and not args.graph_towers
    opt = make_capturable_adam(params, 1e-4, dev) if use_graph else torch.optim.Adam(params, lr=1e-4, fused=True)

    def mk_sched(o):
        return get_scheduler("linear", optimizer=o, num_warmup_steps=100, num_training_steps=100000)

    sched = TensorLRScheduler(opt, 1e-4, mk_sched) if use_graph else mk_sched(opt)
    ops = TimedOps()
    step = RagE2EStep(model, opt, sched, CFG["logit_scale"], comm=comm, autocast_dtype=autocast, ops=ops,
                      inplace_grad=True, overlap_towers=not args.no_overlap, fuse_lm_head=args.fuse_lm_head,
                      graph_towers=(args.graph_towers or not isinstance(comm, LocalComm)) and not args.no_graph
                      and not args.graph_collectives,
                      graph_after=0, grad_overlap=not args.graph_collectives)
    if use_graph:
        step = GraphedStep(step, max_graphs=8 if args.data_path == "fixed" else 32)
    # a few distinct pre-staged batches (inputs resident in HBM before the timed region)
    loader = None
    if args.data_path == "fixed":
        batches = [synthetic_batch(dev, 100 + 17 * rank + i, V=V) for i in range(4)]
    elif args.data_path == "packed":
        from dalm_amd.packed import add_pack_plans

        host = [add_pack_plans(synthetic_batch(torch.device("cpu"), 100 + 17 * rank + i, V=V)) for i in range(4)]
        batches = [{k: v.to(dev) for k, v in b.items()} for b in host]
        args.warmup = max(args.warmup, len(batches))   # one hipGraph per packed row count, captured before the timed region
    elif args.data_path == "loader":
        from dalm_amd.training.common import ShardedBatches

        nb = args.steps + max(args.warmup, 1) + 2
        pool = [synthetic_batch(torch.device("cpu"), 100 + 17 * rank + i, V=V) for i in range(nb)]
        rows = {k: torch.cat([b[k] for b in pool]) for k in pool[0]}          # a tokenised dataset of nb * 18 rows
        loader = ShardedBatches(rows, CFG["B"], 0, 1, 1234, list(rows.keys()))
        stream = loader.epoch(0, dev, 0)
        batches = None
    else:
        batches = bucketed_batches(dev, 100 + 17 * rank, V)
        args.warmup = max(args.warmup, len(batches))   # one hipGraph per trimmed shape, all captured before the timed region
    if args.fuse_lm_head and not args.all_rows:
        # the data loader's job (ShardedBatches(live_rows=...)): list the rows that carry loss while the mask is host memory
        from dalm_amd.fused import gemm_wave_rows, live_row_index

        for b in batches:
            idx = live_row_index(b["generator_input_attention_mask"], gemm_wave_rows(V))
            if idx is not None:
                b["generator_live_rows"] = idx.to(dev)

    # graphs are captured during the first untimed step; with --warmup 0 one untimed step still runs so that
    # the capture never lands inside the timed region
    def next_batch(i):
        return next(stream) if loader is not None else batches[i % len(batches)]

    for i in range(max(args.warmup, 1)):
        step(next_batch(i))
    torch.cuda.synchronize()
    barrier(comm)
    graphed = use_graph and getattr(step, "graph", None) is not None
    ops.enabled = not graphed  # HIP events cannot bracket a kernel inside a replayed graph
    t0 = time.perf_counter()
    for i in range(args.steps):
        loss = step(next_batch(i))
    torch.cuda.synchronize()
    barrier(comm)
    elapsed = time.perf_counter() - t0
    ops.enabled = False
    loss_val = float(loss)
    if args.dump_outputs and rank == 0:        # before the eager probe steps below move the parameters on
        dump_outputs(args.dump_outputs, loss, model)
    probe_note = "HIP events around the launch in every timed step"
    if batches is None:                                   # loader mode: probes below use plain resident batches
        batches = [synthetic_batch(dev, 100 + 17 * rank + i, V=V) for i in range(4)]
    if graphed and not args.full:
        probe_note = f"not timed: the timed region replays a hipGraph ({FULL_ONLY})"
    elif graphed:
        # the timed region replays a hipGraph; time the dominant kernel live with HIP events in a few
        # eager launches of the very same step right after it (not part of `value`)
        ops.enabled = True
        for i in range(min(args.steps, 5)):
            step.step(batches[i % len(batches)])
        torch.cuda.synchronize()
        ops.enabled = False
        probe_note = "HIP events around the launch in 5 eager steps run right after the timed hipGraph-replay region"
    from dalm_amd.sharded import max_over_ranks

    elapsed = max_over_ranks(comm, elapsed)        # the slowest rank's clock

    ranks_seen, backend = 1, "none (one process)"
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        ranks_seen, backend = torch.distributed.get_world_size(), torch.distributed.get_backend()
    elif type(comm).__name__ == "NativeRcclComm":
        ranks_seen, backend = comm.world_size, "RCCL through libdalm_hip.so (dalm_comm_*_on, caller's stream)"
    if rank == 0:
        B, Tg = CFG["B"], CFG["Tg"]
        el = 2 if args.dtype == "bf16" else 4   # logits element size (bf16 lm_head output / fp32)
        ce_ms = [e[0].elapsed_time(e[1]) for e in ops.events]
        ce_avg_s = (sum(ce_ms) / max(len(ce_ms), 1)) * 1e-3
        lives = [int(e[2]) for e in ops.events]
        alg_bytes = sum((lv + e[3]) * e[4] for lv, e in zip(lives, ops.events)) / max(len(ops.events), 1)  # per launch
        live_rows = sum(lives) / max(len(lives), 1)
        dense_bytes = 2 * B * (Tg - 1) * V * el                               # SURVEY 8(d) dense definition
        achieved = alg_bytes / ce_avg_s / 1e9 if ce_avg_s > 0 else 0.0
        # HBM traffic of that kernel comes from rocprofv3 PMC passes of THIS command (FETCH_SIZE and WRITE_SIZE
        # cannot share a pass, and counters perturb timing, so they are never collected inside the timed run):
        # tools/pmc_bench.sh writes profiles/roofline_traffic.json; the value is per launch, FETCH doubled as the
        # gfx950 guide prescribes.  Only quoted for the workload/dtype it was collected on.
        traffic, traffic_source = None, "not collected this run" + ("" if args.full else f" ({FULL_ONLY})")
        if args.full and args.gpus == 1 and not args.no_pmc and not args.fuse_lm_head and args.data_path in ("fixed", "loader"):
            try:
                traffic, traffic_source = collect_ce_traffic(args.workload, args.dtype, V)
            except Exception as e:
                traffic, traffic_source = None, f"not collected this run: {e!r}"
        loss_path_us, loss_path_how = None, (None if args.full else f"not measured ({FULL_ONLY})")
        if args.full and args.gpus == 1 and not args.fuse_lm_head:
            try:
                loss_path_us, loss_path_how = gpu_loss_path_probe(dev, batches[0], torch.bfloat16 if args.dtype == "bf16" else torch.float32, V)
            except Exception as e:
                loss_path_how = f"failed: {e!r}"
        b2b_us, b2b_gbps = None, None
        if args.full and args.gpus == 1 and not args.fuse_lm_head and args.data_path == "fixed":
            try:
                b2b_us, b2b_gbps = ce_back_to_back_probe(dev, batches[0], torch.bfloat16 if args.dtype == "bf16" else torch.float32, V)
            except Exception:
                pass
        value = args.gpus * B * args.steps / elapsed
        # token rows that go through the towers' GEMMs per step (mean over the staged batches): every padded position on the
        # fixed / loader paths, the trimmed width on the bucketed path, the packed row lists on the packed path
        def _rows(b, prefix, ids_key):
            return float(b[f"{prefix}_pack_rows"].numel()) if f"{prefix}_pack_rows" in b else float(b[ids_key].numel())
        gen_tokens = sum(_rows(b, "generator", "generator_input_input_ids") for b in batches) / len(batches)
        retr_tokens = sum(_rows(b, "retriever_query", "retriever_query_input_ids")
                          + _rows(b, "retriever_passage", "retriever_passage_input_ids") for b in batches) / len(batches)
        live_tokens = {"generator": sum(float((b["generator_input_attention_mask"] != 0).sum()) for b in batches) / len(batches),
                       "retriever": sum(float((b["retriever_query_attention_mask"] != 0).sum()
                                              + (b["retriever_passage_attention_mask"] != 0).sum()) for b in batches) / len(batches)}
        model_tf = step_model_tflops(model, gen_tokens, retr_tokens)
        out = {
            "metric": "training pairs/sec (global batch) RAG-e2e bge-large+" + ("Llama-2-7b" if gen_name == "llama-2-7b" else "Falcon-7B"),
            "value": value, "unit": "pairs/s", "n_gpus": args.gpus, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": (value / A100_README_PAIRS_PER_S) if (args.gpus == 1 and args.workload == "cfg3"
                                                                   and args.data_path == "fixed" and not args.use_bnb) else None,
            "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": f"{args.workload} RAG-e2e: bge-large-en + {gen_name} architectures (random init, V={V}), "
                                   "LoRA r=8 both towers, per-GPU batch 18, Tq50/Tp128/Tg256, logit_scale 100, Adam, "
                                   + ("bf16 weights + autocast" if args.dtype == "bf16" else "fp32 weights, no autocast")
                                   + ("" if args.data_path == "fixed" else
                                      ("; DATA PATH: batches come through the trainer's host loader inside the timed loop (ShardedBatches: "
                                       "pinned int32 columns, staged index_select, H2D on a copy stream)" if args.data_path == "loader" else
                                       "; DATA PATH: packed - the same rows, both towers run on the un-padded live tokens "
                                       "(dalm_amd/packed.py; same loss and gradients as the padded step, tests/test_packed_gpu.py)"
                                       if args.data_path == "packed" else
                                       "; DATA PATH: length-bucketed batches with all-padding columns trimmed (the trainer's opt-in "
                                       "--length_bucketing --trim_padding), fewer tokens per pair than the named configuration")),
                       "global_batch": args.gpus * B, "parallelism": f"dp{args.gpus} + sharded in-batch negatives",
                       "ranks_seen_by_process_group": ranks_seen, "collective_backend": backend + (" (= RCCL)" if backend == "nccl" else ""),
                       "spawned_by": os.environ.get("TORCHELASTIC_RUN_ID") and "torch.distributed.run" or
                                     ("dalm_amd.launch (python bench.py --gpus N)" if ranks_seen > 1 else "single process"),
                       "gpu_max_hw_queues": args.hw_queues,
                       "retriever_layers": args.retriever_layers, "generator_layers": args.generator_layers,
                       "use_bnb": (None if not args.use_bnb else
                                   {"towers": args.use_bnb, "format": "nf4, blocks of 64, f32 absmax, bf16 compute (dalm_nf4_* kernels)",
                                    "weight_bytes_resident": _resident_weight_bytes(model)}),
                       "tower_rows_per_step": {"generator": gen_tokens, "retriever": retr_tokens, "live_tokens": live_tokens,
                                               "padded": {"generator": B * Tg, "retriever": B * (CFG["Tq"] + CFG["Tp"])}},
                       "lm_head": ("chunked over the packed rows with the CE kernel (no [B,Tg,V] logits tensor)" if args.data_path == "packed" else
                                   ("fused with the CE in row chunks over the rows that carry loss (no logits tensor)" if not args.all_rows
                                    else "fused with the CE in sample chunks (no logits tensor)") if args.fuse_lm_head
                                   else f"logits materialised ({args.dtype})"),
                       "tower_gemms": "pre-tuned solution table (dalm_amd/tuning)" if args.tuned_gemms else "library defaults",
                       "tower_kernels": _tower_kernels(model),
                       "launch": ("hipGraph replay of the whole step" if (use_graph and getattr(step, "graph", None) is not None)
                                  else ("hipGraph replay of tower fwd/bwd, eager collectives+loss+optimizer"
                                        if getattr(step, "towers", None) is not None else
                                        "eager" + (f" (capture failed: {getattr(step, 'failed', None) or getattr(step, 'towers_failed', None)})"
                                                   if (getattr(step, "failed", None) or getattr(step, "towers_failed", None)) else ""))),
                       "baseline_ref": "reference README.md:34-40: 200k rows in 7 h on 1x A100-80GB = 7.94 pairs/s",
                       # informational step-level roofline, from this model's parameters and the rows its GEMMs see
                       "peak_hbm_gb": torch.cuda.max_memory_allocated() / 1e9,
                       "step_model_tflops": model_tf,
                       "step_frac_of_bf16_mfma_peak": model_tf / (elapsed / args.steps) / 2500.0,
                       "final_loss": loss_val},
            "roofline": {"bound": "hbm", "kernel": f"marg_ce_row kernel (fused fwd+grad, {args.dtype} logits, V={V})",
                         "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBPS,
                         "traffic": traffic, "traffic_source": traffic_source,
                         "loss_path_us": loss_path_us,
                         "loss_path_note": (f"whole HIP loss path of one step (pool+normalise x2, similarity/contrastive, fused CE fwd+grad, "
                                            f"finalize, and their backward) run alone at the step's shapes, {args.dtype} tower outputs: "
                                            f"{loss_path_how}; beside cpu_baseline.loss_path"),
                         "avg_launch_us": ce_avg_s * 1e6, "algorithmic_bytes": alg_bytes,
                         "back_to_back_us": b2b_us, "back_to_back_frac": (b2b_gbps / HBM_PEAK_GBPS) if b2b_gbps else None,
                         "back_to_back_note": "the same kernel at the first batch's mask, 20 launches between one HIP event pair "
                                              "(launch gaps amortised): the figure to hold against the rocprofv3 average in "
                                              "profiles/*_bench_dalm_kernels_per_shape.txt; `frac` / `avg_launch_us` stay the in-step numbers",
                         "live_rows_per_launch": live_rows, "dense_rows_per_launch": B * (Tg - 1),
                         "dense_definition_GBps": dense_bytes / ce_avg_s / 1e9 if ce_avg_s > 0 else 0.0,
                         "note": "achieved counts only bytes the launch must move (padded rows are skipped on the read "
                                 "side); the all-ones-mask roofline point is in profiles/ (tools/kernel_bench.py)",
                         "timing": probe_note},
        }
        if args.full and args.gpus == 1 and args.dtype == "bf16" and batches and (not args.no_pmc or args.fuse_lm_head):
            try:
                out["f1_lm_head_paths"] = f1_head_paths(dev, batches[0], model)
            except Exception as e:
                out["f1_lm_head_paths"] = {"error": repr(e)}
        f1 = out.get("f1_lm_head_paths") or {}
        if args.fuse_lm_head and os.environ.get("DALM_LM_HEAD_TRAIN_KERNEL", "1") != "0" and f1.get("kernels_ms"):
            # the fused CE kernel does not run on this path: the loss path's dominant kernels are the three bf16 MFMA contractions
            # of the logits-free lm_head + CE (forward lse, logits recomputed for d(logits), d(hidden)), timed live above
            flop = 3 * 2.0 * f1["rows"] * f1["V"] * f1["H"]
            tf = flop / (f1["kernels_ms"] * 1e-3) / 1e12
            out["roofline"] = {"bound": "mfma", "kernel": "dalm_lm_head_lse_fwd + dalm_lm_head_dlogits + dalm_lm_head_dhidden (bf16 MFMA, "
                                                          "logits never materialised; incl. the transposes and the merge launches)",
                               "achieved": tf, "peak": 2500.0, "unit": "TFLOP/s", "frac": tf / 2500.0, "traffic": None,
                               "algorithmic_flop": flop, "avg_launch_us": f1["kernels_ms"] * 1e3,
                               "note": "3 contractions of [rows, H] x [V, H] over the live rows (HIP events around eager calls, "
                                       "f1_lm_head_paths.kernels_ms); the library path of the same rows takes f1_lm_head_paths.library_ms"}
        if args.full and args.gpus == 1 and not args.no_cpu_baseline and args.workload == "cfg3":
            try:
                out["cpu_baseline"], parity = cpu_reference_baseline(parity_dev=dev)
                if parity is not None:
                    out["parity"] = parity
            except Exception as e:  # the baseline must never take the GPU number down with it
                out["cpu_baseline"] = {"value": None, "unit": "training pairs/s", "cores": os.cpu_count(),
                                       "kind": "port", "sample": f"failed: {e!r}"}
            try:
                out["cpu_baseline"]["loss_path"] = cpu_loss_path_baseline(synthetic_batch(torch.device("cpu"), 100, V=V), V)
            except Exception as e:
                out["cpu_baseline"]["loss_path"] = {"ms": None, "what": f"failed: {e!r}"}
            # the like-for-like pair for what this repository replaces - the reference's loss-path op sequence on the host against
            # the HIP loss path on the GPU, both MEASURED at the step's full shapes (no extrapolation) - at the top level, next to
            # `value`; `cpu_baseline.value` above stays the whole-step figure the contract asks for
            lp = out["cpu_baseline"]["loss_path"]
            if lp.get("ms") and loss_path_us:
                out["loss_path"] = {"gpu_us": loss_path_us, "cpu_ms": lp["ms"], "cpu_cores": lp.get("cores"), "cpu_kind": lp.get("kind"),
                                    "gpu_over_cpu": lp["ms"] * 1e3 / loss_path_us,
                                    "what": "pool + normalise x2, similarity / contrastive, marginalised CE, forward + backward at "
                                            f"[B=18, Tg=256, V={V}]: HIP kernels (hipGraph replay) vs the reference's op sequence "
                                            "on the host cores; a baseline, not a target - kernel quality is roofline.frac"}
        _flush_c_stdio()
        print(json.dumps(out), flush=True)
    barrier(comm)
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()
    _quiet_exit()


def _quiet_exit() -> None:
    """Anything a library still holds in C stdio buffers (RCCL's banner) goes to stderr's side of the world: point fd 1 at
    /dev/null for what is flushed during interpreter shutdown, after our own output has been written."""
    try:
        sys.stdout.flush()
        _flush_c_stdio()
        devnull = os.open(os.devnull, os.O_WRONLY)
        os.dup2(devnull, 1)
    except Exception:
        pass


def main_retriever_only(args):
    """BASELINE.json configs[1]: retriever-only contrastive step, bge-large-en architecture, batch 150 per GPU,
    Tq=50 / Tp=128, LoRA on q/k/v.  Secondary workload (not the headline line)."""
    from transformers import BertConfig, BertModel, get_scheduler

    from dalm_amd.fused import LocalComm
    from dalm_amd.models import AutoModelForSentenceEmbedding
    from dalm_amd.sharded import barrier, init_distributed
    from dalm_amd.training.graphed import GraphedStep, TensorLRScheduler, make_capturable_adam
    from dalm_amd.training.step import RetrieverStep

    comm, dev = init_distributed()
    small = args.workload == "cfg1"   # bge-small-en: 384 wide, 12 layers, 12 heads; the toy csv has 19 rows (< batch 32)
    B, Tq, Tp = (19 if small else 150), 50, 128
    wdtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    autocast = torch.bfloat16 if args.dtype == "bf16" else None
    layers = min(args.retriever_layers, 12) if small else args.retriever_layers
    torch.manual_seed(0)
    with torch.device(dev):
        old = torch.get_default_dtype()
        torch.set_default_dtype(wdtype)
        try:
            bert = BertModel(BertConfig(hidden_size=384 if small else 1024, num_hidden_layers=layers,
                                        num_attention_heads=12 if small else 16, intermediate_size=1536 if small else 4096,
                                        vocab_size=30522, max_position_embeddings=512))
        finally:
            torch.set_default_dtype(old)
    model = AutoModelForSentenceEmbedding.from_modules(bert, None, normalize=True, get_peft=True)
    model.train()
    params = [p for p in model.parameters() if p.requires_grad]
    # --graph-towers: the two encoder calls as single-stream graphs, loss / optimizer eager (the RAG-e2e step's default structure).
    # NOT the default here: measured slower than the whole-step graph on this short step (cfg2 2723 against 2857 pairs/s, cfg1
    # 3479 against 4584, same box, tools/cfg2_overlap_ab.sh) - the eager loss sits on the critical path between the forward and
    # backward graphs and there is no long generator graph to hide it behind.  Packed batches go through the encoder in ONE call.
    # One rank only: with the W > 1 gradient bucket (parameter gradients as views of one flat buffer) the second replay of a set of
    # encoder graphs produced an infinite gradient norm (one-rank RCCL run, end of round 6, not understood) - W > 1 launches eagerly.
    towers = (isinstance(comm, LocalComm) and not args.no_graph and args.graph_towers and args.data_path != "packed"
              and not args.no_overlap)
    use_graph = isinstance(comm, LocalComm) and not args.no_graph and not towers
    opt = make_capturable_adam(params, 1e-4, dev) if use_graph else torch.optim.Adam(params, lr=1e-4, fused=True)
    def mk_sched(o):
        return get_scheduler("linear", optimizer=o, num_warmup_steps=0, num_training_steps=100000)

    sched = TensorLRScheduler(opt, 1e-4, mk_sched) if use_graph else mk_sched(opt)
    step = RetrieverStep(model, opt, sched, CFG["logit_scale"], comm=comm, autocast_dtype=autocast,
                         overlap_towers=not args.no_overlap, graph_towers=towers, graph_after=0)
    if use_graph:
        step = GraphedStep(step)

    def batch(seed):
        g = torch.Generator().manual_seed(seed)
        ql = torch.randint(5, 16, (B, 1), generator=g)
        pl = torch.randint(30, Tp + 1, (B, 1), generator=g)
        return {k: v.to(dev) for k, v in {
            "query_input_ids": torch.randint(1000, 30522, (B, Tq), generator=g),
            "query_attention_mask": (torch.arange(Tq).unsqueeze(0) < ql).long(),
            "passage_input_ids": torch.randint(1000, 30522, (B, Tp), generator=g),
            "passage_attention_mask": (torch.arange(Tp).unsqueeze(0) < pl).long()}.items()}

    batches = [batch(200 + 17 * comm.rank + i) for i in range(4)]
    if args.data_path == "packed":       # the same rows, the encoder run on the live tokens only (dalm_amd/packed.py)
        from dalm_amd.packed import RETRIEVER_GROUPS, add_pack_plans

        batches = [add_pack_plans(b, RETRIEVER_GROUPS) for b in batches]
        args.warmup = max(args.warmup, 4)
    rows_per_step = sum(float(b["query_pack_rows"].numel() + b["passage_pack_rows"].numel()) if "query_pack_rows" in b
                        else float(b["query_input_ids"].numel() + b["passage_input_ids"].numel()) for b in batches) / 4
    for i in range(max(args.warmup, 1)):
        step(batches[i % 4])
    torch.cuda.synchronize()
    barrier(comm)
    t0 = time.perf_counter()
    for i in range(args.steps):
        loss = step(batches[i % 4])
    torch.cuda.synchronize()
    barrier(comm)
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and comm.rank == 0:
        dump_outputs(args.dump_outputs, loss, model)
    from dalm_amd.sharded import max_over_ranks

    elapsed = max_over_ranks(comm, elapsed)
    if comm.rank == 0:
        value = args.gpus * B * args.steps / elapsed
        _flush_c_stdio()
        print(json.dumps({
            "metric": "training pairs/sec (global batch) retriever-only " + ("bge-small" if small else "bge-large"), "value": value, "unit": "pairs/s",
            "n_gpus": args.gpus, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": f"{args.workload} retriever-only: {'bge-small-en' if small else 'bge-large-en'} architecture (random init), "
                                   f"LoRA r=8 q/k/v, per-GPU batch {B}, Tq50/Tp128, logit_scale 100, Adam, {args.dtype}"
                                   + ("; DATA PATH: packed - the same rows, the encoder runs on the un-padded live tokens "
                                      "(dalm_amd/packed.py; same loss and gradients)" if args.data_path == "packed" else ""),
                       "tower_rows_per_step": {"encoder": rows_per_step, "padded": B * (Tq + Tp)},
                       "step_model_tflops": step_model_tflops(model, 0.0, rows_per_step),
                       "step_frac_of_bf16_mfma_peak": step_model_tflops(model, 0.0, rows_per_step) / (elapsed / args.steps) / 2500.0,
                       "global_batch": args.gpus * B,
                       "parallelism": f"dp{args.gpus} + sharded in-batch negatives", "final_loss": float(loss),
                       "launch": ("hipGraph replay of the whole step" if (use_graph and getattr(step, "graph", None) is not None)
                                  else ("hipGraph replay of the encoder calls fwd/bwd, eager loss+optimizer"
                                        if getattr(step, "towers", None) is not None else
                                        "eager" + (f" (capture failed: {getattr(step, 'towers_failed', None)})"
                                                   if getattr(step, "towers_failed", None) else "")))}}),
              flush=True)
    barrier(comm)
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()
    _quiet_exit()


if __name__ == "__main__":
    # the process ends through the interpreter's normal shutdown, so that exit handlers run (a profiler writes its output from
    # them, TunableOp its results file)
    main()
