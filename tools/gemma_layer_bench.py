"""One Gemma-7B decoder layer, forward + backward, with and without the Gemma routing of this package.

    python tools/gemma_layer_bench.py [--rounds 5] [--iters 10] [--out FILE.json]

A one-layer Gemma model at the 7B layer shape (hidden 3072, 16 heads of 256, intermediate 24576; a 1024-token vocabulary so that
the embedding is negligible), bf16 base weights, LoRA r 8 on q_proj / v_proj, batch 18 x 256 with the benchmark's generator
lengths (uniform 60 .. 256, left-padded).  Four variants, visited in turn in every round (same process, same tensors):

  routed           GeGLU kernel, (1 + w) RMSNorm kernel, fused residual + norm layer (`use_generator_fast_paths`)
  geglu only       `use_geglu_kernel` alone
  norms only       `use_gemma_rms_norm` + the fused residual + norm layer alone
  unrouted         what a Gemma generator got before the routing existed: the LoRA group kernels and the transposed dgrad (keyed
                   by names Gemma shares) on transformers' own layer code

Attention is transformers' "sdpa" in every variant: head width 256 is not a width the attention kernels take, so the model does
not pack either and only the padded call is timed.

Time per call: device events around `iters` forward + backward calls, after a warm-up of every variant; the median of the
rounds, with the lowest and highest.  This is a LAYER time, not a step time: no Gemma training step has been measured."""
from __future__ import annotations

import argparse
import copy
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def build(dev):
    from transformers import GemmaConfig, GemmaForCausalLM

    from dalm_amd import packed
    from dalm_amd.models import fastpath, lora
    from dalm_amd.models.frozen_linear import use_transposed_dgrad
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    torch.manual_seed(0)
    cfg = GemmaConfig(vocab_size=1024, hidden_size=3072, intermediate_size=24576, num_hidden_layers=1, num_attention_heads=16,
                      num_key_value_heads=16, head_dim=256, max_position_embeddings=4096)
    base = GemmaForCausalLM(cfg)
    with torch.no_grad():
        for n, p in base.named_parameters():
            if n.endswith("norm.weight"):
                p.normal_(0.0, 0.1)

    def finish(model):
        lora.inject_lora(model, ["q_proj", "v_proj"], r=8, lora_dropout=0.0)
        with torch.no_grad():
            for n, p in model.named_parameters():
                if "lora_B" in n:
                    p.normal_(0.0, 0.02)
        model = model.to(dev)
        for p in model.parameters():
            if not p.requires_grad:
                p.data = p.data.to(torch.bfloat16)
        use_transposed_dgrad(model)
        return model.train()

    models = {}
    routed = copy.deepcopy(base)
    went_in = use_generator_fast_paths(routed)
    assert went_in["use_geglu_kernel"] == 1 and went_in["use_gemma_rms_norm"] == 3 and went_in["use_fused_residual_norm"] == 1
    assert not went_in["use_hip_attention_backward"] and not packed.attention_is_packable(routed)       # width 256: "sdpa", padded
    models["routed"] = finish(routed)
    geglu = copy.deepcopy(base)
    assert fastpath.use_geglu_kernel(geglu) == 1
    models["geglu only"] = finish(geglu)
    norms = copy.deepcopy(base)
    assert fastpath.use_gemma_rms_norm(norms) == 3 and fastpath.use_fused_residual_norm(norms) == 1
    models["norms only"] = finish(norms)
    models["unrouted"] = finish(base)
    return models


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="", help="also write the figures to this JSON file")
    args = ap.parse_args()
    from dalm_amd import live_rows

    dev = torch.device("cuda:0")
    models = build(dev)
    B, T = 18, 256
    g = torch.Generator().manual_seed(0)
    glen = torch.randint(60, T + 1, (B, 1), generator=g)
    am = (torch.arange(T).unsqueeze(0) >= (T - glen)).long().to(dev)
    ids = torch.randint(0, 1024, (B, T), generator=g).to(dev)
    w_pad = torch.randn(B, T, 3072, device=dev, dtype=torch.bfloat16)

    def padded(model):
        def run():
            with torch.autocast("cuda", dtype=torch.bfloat16), live_rows.tower_call(am, shifted=True):
                h = model.base_model(input_ids=ids, attention_mask=am, use_cache=False)[0]
            (h * w_pad).sum().backward()
        return run

    variants = {name: padded(model) for name, model in models.items()}
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
    res = {"shape": {"B": B, "T": T, "live_tokens": int(am.sum())}}
    for name, ts in seen.items():
        ts.sort()
        res[name] = {"ms": ts[len(ts) // 2], "lo": ts[0], "hi": ts[-1]}
        print(f"{name:12s} {res[name]['ms']:8.3f} ms per forward + backward   (rounds: {ts[0]:.3f} .. {ts[-1]:.3f})")
    for name in ("routed", "geglu only", "norms only"):
        res[name]["unrouted_over_this"] = res["unrouted"]["ms"] / res[name]["ms"]
        print(f"unrouted / {name}: {res[name]['unrouted_over_this']:.3f}")
    print(f"padded rows {B * T}, live tokens {res['shape']['live_tokens']}")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
