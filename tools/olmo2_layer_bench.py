"""One OLMo-2-7B decoder layer, forward + backward, with and without the OLMo-2 routing of this package.

    python tools/olmo2_layer_bench.py [--rounds 5] [--iters 10] [--out FILE.json]

A one-layer OLMo-2 model at the 7B layer shape (hidden 4096, 32 x 128 heads, MHA, intermediate 11008; a 1024-token vocabulary so
that the embedding is negligible), bf16 base weights, LoRA r 8 on q_proj / v_proj, batch 18 x 256 with the benchmark's generator
lengths (uniform 60 .. 256, left-padded).  Variants, visited in turn in every round (same process, same tensors):

  routed, padded          native RMSNorm, SwiGLU, the norm + add pairs, "dalm_sdpa", the row-norm + rotary + attention node
  routed, packed          the same model on the un-padded rows (dalm_amd/packed.py)
  no norm_add, padded     routed, but the decoder layer keeps transformers' forward (F.rms_norm, then the add)
  no attn node, padded    routed, but the attention module keeps transformers' forward on "dalm_sdpa" (F.rms_norm x 2, eager rotary)
  before, padded          what an OLMo-2 generator got before the routing existed: native RMSNorm, the LoRA group kernels and the
                          transposed dgrad (all keyed by names OLMo-2 shares with Llama) on transformers' "sdpa"; it cannot run packed

Time per call: device events around `iters` forward + backward calls, after a warm-up of every variant; the median of the
rounds, with the lowest and highest.  This is a LAYER time, not a step time: no OLMo-2 training step has been measured."""
from __future__ import annotations

import argparse
import copy
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def build(dev):
    from transformers import Olmo2Config, Olmo2ForCausalLM

    from dalm_amd.models import fastpath, lora
    from dalm_amd.models.frozen_linear import use_transposed_dgrad
    from dalm_amd.models.rag_e2e_base_model import _GENERATOR_PATHS

    torch.manual_seed(0)
    cfg = Olmo2Config(vocab_size=1024, hidden_size=4096, intermediate_size=11008, num_hidden_layers=1, num_attention_heads=32,
                      num_key_value_heads=32, max_position_embeddings=4096, pad_token_id=1, bos_token_id=None, eos_token_id=2)
    base = Olmo2ForCausalLM(cfg)

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

    def routed_without(*skipped):
        model = copy.deepcopy(base)
        went_in = {use.__name__: use(model) for use in _GENERATOR_PATHS if use.__name__ not in skipped}
        assert went_in["use_swiglu_kernel"] == 1 and went_in["use_hip_attention_backward"]
        assert went_in.get("use_olmo2_layer", 1) == 1 and went_in.get("use_olmo2_attention_node", 1) == 1
        return finish(model)

    before = copy.deepcopy(base)
    fastpath.use_native_rms_norm(before)
    return {"routed": routed_without(), "no norm_add": routed_without("use_olmo2_layer"),
            "no attn node": routed_without("use_olmo2_attention_node"), "before": finish(before)}


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
    w_pad = torch.randn(B, T, 4096, device=dev, dtype=torch.bfloat16)
    w_pack = torch.randn(rows.numel(), 4096, device=dev, dtype=torch.bfloat16)

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
                "no norm_add, padded": padded(models["no norm_add"]), "no attn node, padded": padded(models["no attn node"]),
                "before, padded": padded(models["before"])}
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
