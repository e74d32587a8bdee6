"""An XLM-R-large-shaped encoder, forward + backward, with and without the RoBERTa-family routing of this package.

    python tools/xlmr_layer_bench.py [--layers 4] [--rounds 5] [--iters 10] [--out FILE.json]

`--layers` XLM-RoBERTa layers at the large shape (hidden 1024, 16 heads of 64, intermediate 4096, vocabulary 250002, 514
positions), fp32 base weights under bf16 autocast (how the retriever-only trainer runs a LoRA retriever), LoRA r 8 on key / query /
value, the published dropouts (0.1), the retriever-only passage batch 150 x 128 right-padded with the pad id (uniform 30 .. 128
live tokens).  Four variants, visited in turn in every round (same process, same tensors):

  routed, padded                    "dalm_sdpa", the dropout + add + LayerNorm kernels, the embeddings kernel, row liveness
  routed, packed                    the same model on the un-padded rows (dalm_amd/packed.py, positions from the ids)
  routed, padded, eager embeddings  the first variant without `use_roberta_embeddings`: what the embeddings kernel is worth
  before, padded                    what the family got before the routing existed: the LoRA group kernels and the transposed
                                    dgrad (keyed by names it shares with BERT) on torch SDPA and the eager output modules; it
                                    cannot run packed

Time per call: device events around `iters` forward + backward calls, after a warm-up of every variant; the median of the
rounds, with the lowest and highest.  This is an ENCODER time at `--layers` layers, not a step time."""
from __future__ import annotations

import argparse
import copy
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def build(dev, layers):
    from transformers import XLMRobertaConfig, XLMRobertaModel

    from dalm_amd.models import attention, fastpath, lora
    from dalm_amd.models.frozen_linear import use_transposed_dgrad

    torch.manual_seed(0)
    cfg = XLMRobertaConfig(vocab_size=250002, hidden_size=1024, intermediate_size=4096, num_hidden_layers=layers,
                           num_attention_heads=16, max_position_embeddings=514, type_vocab_size=1, pad_token_id=1, layer_norm_eps=1e-5)
    base = XLMRobertaModel(cfg, add_pooling_layer=False)

    def finish(model, route, embeddings):
        if route:
            assert attention.use_hip_attention_backward(model)
        lora.inject_lora(model, ["key", "query", "value"], r=8)
        with torch.no_grad():
            for n, p in model.named_parameters():
                if "lora_B" in n:
                    p.normal_(0.0, 0.02)
        model = model.to(dev)
        use_transposed_dgrad(model)
        if route:
            assert fastpath.use_bert_layer_kernels(model) == 2 * layers
        if embeddings:
            assert fastpath.use_roberta_embeddings(model) == 1
        return model.train()

    return {"routed": finish(copy.deepcopy(base), True, True), "routed, eager embeddings": finish(copy.deepcopy(base), True, False),
            "before": finish(base, False, False)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="", help="also write the figures to this JSON file")
    args = ap.parse_args()
    from dalm_amd import live_rows, packed

    dev = torch.device("cuda:0")
    models = build(dev, args.layers)
    B, T, D = 150, 128, 1024
    g = torch.Generator().manual_seed(0)
    lens = torch.randint(30, T + 1, (B, 1), generator=g)
    am = (torch.arange(T).unsqueeze(0) < lens).long()
    ids = torch.where(am.bool(), torch.randint(3, 250002, (B, T), generator=g), torch.ones(B, T, dtype=torch.long))
    rows, cu = packed.pack_plan(am, shifted=False, multiple=packed.ROW_MULTIPLES["passage"])
    ids, am, rows, cu = ids.to(dev), am.to(dev), rows.to(dev), cu.to(dev)
    w = torch.randn(B, T, D, device=dev) * am.unsqueeze(-1)

    def padded(model):
        def run():
            with torch.autocast("cuda", dtype=torch.bfloat16), live_rows.tower_call(am, shifted=False):
                h = model(ids, am)[0]
            (h * w).sum().backward()
        return run

    def packed_run():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            h = packed.retrieval_hidden(models["routed"], ids, am, rows, cu)
        (h * w).sum().backward()

    variants = {"routed, padded": padded(models["routed"]), "routed, packed": packed_run,
                "routed, padded, eager embeddings": padded(models["routed, eager embeddings"]), "before, padded": padded(models["before"])}
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    seen = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            seen[name].append(a.elapsed_time(b) / args.iters)
    res = {"shape": {"layers": args.layers, "B": B, "T": T, "live_tokens": int(am.sum()), "packed_rows": int(rows.numel())}}
    for name, ts in seen.items():
        ts.sort()
        res[name] = {"ms": ts[len(ts) // 2], "lo": ts[0], "hi": ts[-1]}
        print(f"{name:34s} {res[name]['ms']:8.3f} ms per forward + backward   (rounds: {ts[0]:.3f} .. {ts[-1]:.3f})")
    print(f"layers {args.layers}, padded rows {B * T}, live tokens {res['shape']['live_tokens']}, packed rows {res['shape']['packed_rows']}")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
