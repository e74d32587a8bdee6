"""An all-mpnet-base-v2-shaped encoder, forward + backward, with and without the MPNet routing of this package.

    python tools/mpnet_layer_bench.py [--layers 4] [--rounds 20] [--iters 5] [--B 150] [--T 128] [--out FILE.json]

`--layers` MPNet layers at the base shape (hidden 768, 12 heads of 64, intermediate 3072, vocabulary 30527, 514 positions, 32
relative-position buckets), fp32 base weights under bf16 autocast (how the retriever-only trainer runs a LoRA retriever), LoRA r 8
on q / k / v, the published dropouts (0.1), a right-padded batch B x T with the pad id (uniform T/4 .. T live tokens).  Three
variants, visited in turn in every round (same process, same tensors):

  routed, padded     `use_mpnet_attention_kernels` (dalm_attn_rel_*: the bias as one [H, 2 T - 1] vector) + the dropout + add +
                     LayerNorm kernels on MPNetAttention / MPNetOutput, row liveness
  routed, packed     the same model on the un-padded rows (dalm_amd/packed.py; positions from the ids, columns in the descriptor)
  unrouted, padded   transformers' eager attention ([B, H, T, T] scores and bias) and output modules; the LoRA kernels and the
                     transposed dgrad stay (they do not depend on the family); it cannot run packed

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
    from transformers import MPNetConfig, MPNetModel

    from dalm_amd.models import fastpath, lora
    from dalm_amd.models.frozen_linear import use_transposed_dgrad

    torch.manual_seed(0)
    cfg = MPNetConfig(vocab_size=30527, hidden_size=768, intermediate_size=3072, num_hidden_layers=layers, num_attention_heads=12,
                      max_position_embeddings=514, relative_attention_num_buckets=32, layer_norm_eps=1e-5)
    base = MPNetModel(cfg, add_pooling_layer=False)

    def finish(model, route):
        lora.inject_lora(model, ["key", "query", "value"], r=8)          # resolves to q / k / v for MPNet
        with torch.no_grad():
            for n, p in model.named_parameters():
                if "lora_B" in n:
                    p.normal_(0.0, 0.02)
        model = model.to(dev)
        use_transposed_dgrad(model)
        if route:
            assert fastpath.use_bert_layer_kernels(model) == 2 * layers
            assert fastpath.use_mpnet_attention_kernels(model) == layers + 1
        return model.train()

    return {"routed": finish(copy.deepcopy(base), True), "unrouted": finish(base, False)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--B", type=int, default=150)
    ap.add_argument("--T", type=int, default=128)
    ap.add_argument("--out", default="", help="also write the figures to this JSON file")
    args = ap.parse_args()
    from dalm_amd import live_rows, packed

    dev = torch.device("cuda:0")
    models = build(dev, args.layers)
    B, T, D = args.B, args.T, 768
    g = torch.Generator().manual_seed(0)
    lens = torch.randint(max(1, T // 4), T + 1, (B, 1), generator=g)
    am = (torch.arange(T).unsqueeze(0) < lens).long()
    ids = torch.where(am.bool(), torch.randint(3, 30527, (B, T), generator=g), torch.ones(B, T, dtype=torch.long))
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

    variants = {"routed, padded": padded(models["routed"]), "routed, packed": packed_run, "unrouted, padded": padded(models["unrouted"])}
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
        print(f"{name:20s} {res[name]['ms']:8.3f} ms per forward + backward   (median of {args.rounds} rounds x {args.iters} calls: "
              f"{ts[0]:.3f} .. {ts[-1]:.3f})")
    print(f"layers {args.layers}, B {B}, T {T}, padded rows {B * T}, live tokens {res['shape']['live_tokens']}, packed rows "
          f"{res['shape']['packed_rows']};  unrouted / routed padded {res['unrouted, padded']['ms'] / res['routed, padded']['ms']:.2f}x, "
          f"unrouted / routed packed {res['unrouted, padded']['ms'] / res['routed, packed']['ms']:.2f}x")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
