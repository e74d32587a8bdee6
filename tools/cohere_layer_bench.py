"""One Cohere decoder layer at an 8B-class shape, forward + backward, with and without the Cohere routing of this package.

    python tools/cohere_layer_bench.py [--rounds 5] [--iters 10] [--out FILE.json]

A one-layer Cohere model at a layer shape stated explicitly (hidden 4096, 32 x 128 heads over 8 key / value heads, intermediate 14336,
no q / k norm; a 1024-token vocabulary so that the embedding is negligible) - a benchmark shape, not a claim about a checkpoint -, bf16
base weights, LoRA r 8 on q_proj / v_proj, batch 18 x 256 with the benchmark's generator lengths (uniform 60 .. 256, left-padded): 4608
rows.  Variants, visited in turn in every round (same process, same tensors):

  routed, padded          what the installers give: "dalm_sdpa", the interleaved rotary + attention node (`dalm_rope_il_qk` forward and
                          one more launch that un-rotates dq / dk), the layer on `dalm_cohere_norm_*` / `dalm_add3_live`, the final norm
  routed, packed          the same model on the un-padded rows (dalm_amd/packed.py)
  no layer, padded        routed, but the decoder layer keeps transformers' forward (CohereLayerNorm's f32 chain, two eager adds)
  no final norm, padded   routed, but the final CohereLayerNorm keeps transformers' forward
  no attn node, padded    routed, but the attention module keeps transformers' forward on "dalm_sdpa" (eager f32 rotary)
  with swiglu, padded     routed, and the MLP on the SwiGLU kernels (`use_swiglu_kernel(model, cohere=True)`: not in the installer lists)
  unrouted, padded        what a Cohere generator got before the routing existed: the LoRA group kernels and the transposed dgrad (both
                          keyed by names Cohere shares with Llama) on transformers' "sdpa"; it cannot run packed

Time per call: device events around `iters` forward + backward calls, after a warm-up of every variant; the median of the rounds,
with the lowest and highest - the run-to-run spread a difference between two variants has to exceed to count.  This is a LAYER time,
not a step time: no Cohere training step has been measured."""
from __future__ import annotations

import argparse
import copy
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

HIDDEN, HEADS, KV_HEADS, INTER = 4096, 32, 8, 14336


def build(dev):
    from transformers import CohereConfig, CohereForCausalLM

    from dalm_amd.models import fastpath, lora
    from dalm_amd.models.frozen_linear import use_transposed_dgrad
    from dalm_amd.models.rag_e2e_base_model import _GENERATOR_PATHS

    torch.manual_seed(0)
    cfg = CohereConfig(vocab_size=1024, hidden_size=HIDDEN, intermediate_size=INTER, num_hidden_layers=1, num_attention_heads=HEADS,
                       num_key_value_heads=KV_HEADS, max_position_embeddings=4096, pad_token_id=1, bos_token_id=None, eos_token_id=2,
                       logit_scale=0.0625, use_qk_norm=False)
    base = CohereForCausalLM(cfg)

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

    def routed_without(*skipped, swiglu=False):
        model = copy.deepcopy(base)
        went_in = {use.__name__: use(model) for use in _GENERATOR_PATHS if use.__name__ not in skipped}
        assert went_in["use_hip_attention_backward"] and went_in["use_swiglu_kernel"] == 0
        for name in ("use_cohere_layer", "use_cohere_attention_node"):
            assert went_in.get(name, 1) == 1, (name, went_in)
        if swiglu:
            assert fastpath.use_swiglu_kernel(model, cohere=True) == 1
        return finish(model)

    # ("no layer": without the layer route the norm installer would take the layer's norm as well, so it is left out with it)
    return {"routed": routed_without(), "no layer": routed_without("use_cohere_layer", "use_cohere_layer_norm"),
            "no final norm": routed_without("use_cohere_layer_norm"), "no attn node": routed_without("use_cohere_attention_node"),
            "with swiglu": routed_without(swiglu=True), "unrouted": finish(copy.deepcopy(base))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="", help="also write the figures to this JSON file")
    args = ap.parse_args()
    from dalm_amd import live_rows, packed

    dev = torch.device("cuda:0")
    models = build(dev)
    B, T = 18, 256
    g = torch.Generator().manual_seed(0)
    glen = torch.randint(60, T + 1, (B, 1), generator=g)
    am = (torch.arange(T).unsqueeze(0) >= (T - glen)).long().to(dev)
    ids = torch.randint(0, 1024, (B, T), generator=g).to(dev)
    rows, cu = packed.pack_plan(am.cpu(), shifted=True, multiple=packed.ROW_MULTIPLES["generator"])
    rows, cu = rows.to(dev), cu.to(dev)
    w_pad = torch.randn(B, T, HIDDEN, device=dev, dtype=torch.bfloat16)
    w_pack = torch.randn(rows.numel(), HIDDEN, device=dev, dtype=torch.bfloat16)

    def padded(model):
        def run():
            with torch.autocast("cuda", dtype=torch.bfloat16), live_rows.tower_call(am, shifted=True):
                h = model.base_model(input_ids=ids, attention_mask=am, use_cache=False)[0]
            (h * w_pad).sum().backward()
        return run

    def packed_run():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            h = packed.generator_hidden(models["routed"], ids, am, rows, cu)
        (h * w_pack).sum().backward()

    variants = {"routed, padded": padded(models["routed"]), "routed, packed": packed_run,
                "no layer, padded": padded(models["no layer"]), "no final norm, padded": padded(models["no final norm"]),
                "no attn node, padded": padded(models["no attn node"]), "with swiglu, padded": padded(models["with swiglu"]),
                "unrouted, padded": padded(models["unrouted"])}
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
    res = {"shape": {"B": B, "T": T, "live_tokens": int(am.sum()), "packed_rows": int(rows.numel())}}
    for name, ts in seen.items():
        ts.sort()
        res[name] = {"ms": ts[len(ts) // 2], "lo": ts[0], "hi": ts[-1]}
        print(f"{name:22s} {res[name]['ms']:8.3f} ms per forward + backward   (rounds: {ts[0]:.3f} .. {ts[-1]:.3f})")
    print(f"padded rows {B * T}, live tokens {res['shape']['live_tokens']}, packed rows {res['shape']['packed_rows']}")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
