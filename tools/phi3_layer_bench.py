"""One Phi-3 decoder layer at Phi-4-mini's and Phi-4's layer shapes, forward + backward, with and without the Phi-3 routing of this
package.

    python tools/phi3_layer_bench.py [--shape phi4-mini|phi4|both] [--rounds 5] [--iters 10] [--out FILE.json]

A one-layer Phi-3 model at a layer shape stated explicitly - a benchmark shape, not a claim about a checkpoint's weights -:

  phi4-mini   hidden 3072, 24 x 128 heads over 8 key / value heads, intermediate 8192, partial_rotary_factor 0.75 (rot 96)
  phi4        hidden 5120, 40 x 128 heads over 10 key / value heads, intermediate 17920, full rotary (rot 128)

with a 1024-token vocabulary so that the embedding is negligible, `rope_type` default, bf16 base weights, LoRA r 8 on qkv_proj, batch
18 x 256 with the benchmark's generator lengths (uniform 60 .. 256, left-padded): 4608 rows.  Variants, visited in turn in every round
(same process, same tensors):

  routed, padded          what the installers give: "dalm_sdpa", the rotary + attention node (rot 96: `dalm_rope_partial_qk` forward
                          and one more launch that un-rotates dq / dk; rot 128: the rotation's backward in the attention backward's
                          epilogues), the layer on `dalm_rms_norm_*`, the MLP on the SwiGLU kernels reading gate | up in place
  routed, packed          the same model on the un-padded rows (dalm_amd/packed.py)
  no attn node, padded    routed, but the attention module keeps transformers' forward on "dalm_sdpa" (eager rotary chain)
  no mlp, padded          routed, but Phi3MLP keeps transformers' forward (chunk, silu, mul)
  no layer, padded        routed, but the decoder layer keeps transformers' forward (two eager adds, the norms as separate nodes)
  unrouted, padded        what a Phi-3 generator got before the routing existed: the native RMSNorm on transformers' "sdpa"; it cannot
                          run packed

Time per call: device events around `iters` forward + backward calls, after a warm-up of every variant; the median of the rounds,
with the lowest and highest - the run-to-run spread a difference between two variants has to exceed to count.  This is a LAYER time,
not a step time: no Phi-3 training step has been measured."""
from __future__ import annotations

import argparse
import copy
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

SHAPES = {"phi4-mini": dict(hidden=3072, heads=24, kv=8, inter=8192, factor=0.75),
          "phi4": dict(hidden=5120, heads=40, kv=10, inter=17920, factor=1.0)}
NEW = ("use_phi3_layer", "use_phi3_mlp", "use_phi3_attention_node")


def build(dev, shape):
    from transformers import Phi3Config, Phi3ForCausalLM

    from dalm_amd.models import fastpath, lora
    from dalm_amd.models.frozen_linear import use_transposed_dgrad
    from dalm_amd.models.rag_e2e_base_model import _GENERATOR_PATHS

    s = SHAPES[shape]
    torch.manual_seed(0)
    cfg = Phi3Config(vocab_size=1024, hidden_size=s["hidden"], intermediate_size=s["inter"], num_hidden_layers=1,
                     num_attention_heads=s["heads"], num_key_value_heads=s["kv"], max_position_embeddings=4096, pad_token_id=1,
                     bos_token_id=None, eos_token_id=2,
                     rope_parameters={"rope_type": "default", "rope_theta": 10000.0, "partial_rotary_factor": s["factor"]})
    base = Phi3ForCausalLM(cfg)

    def finish(model):
        lora.inject_lora(model, ["q_proj", "v_proj"], r=8, lora_dropout=0.0)              # resolves to qkv_proj
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
        assert went_in["use_hip_attention_backward"]
        for name in NEW:
            assert went_in.get(name, 1) == 1, (name, went_in)
        return finish(model)

    def unrouted():
        model = copy.deepcopy(base)
        fastpath.use_native_rms_norm(model)
        return finish(model)

    return {"routed": routed_without(), "no attn node": routed_without("use_phi3_attention_node"),
            "no mlp": routed_without("use_phi3_mlp"), "no layer": routed_without("use_phi3_layer"), "unrouted": unrouted()}


def bench(dev, shape, rounds, iters):
    from dalm_amd import live_rows, packed

    models = build(dev, shape)
    hidden = SHAPES[shape]["hidden"]
    B, T = 18, 256
    g = torch.Generator().manual_seed(0)
    glen = torch.randint(60, T + 1, (B, 1), generator=g)
    am = (torch.arange(T).unsqueeze(0) >= (T - glen)).long().to(dev)
    ids = torch.randint(0, 1024, (B, T), generator=g).to(dev)
    rows, cu = packed.pack_plan(am.cpu(), shifted=True, multiple=packed.ROW_MULTIPLES["generator"])
    rows, cu = rows.to(dev), cu.to(dev)
    w_pad = torch.randn(B, T, hidden, device=dev, dtype=torch.bfloat16)
    w_pack = torch.randn(rows.numel(), hidden, device=dev, dtype=torch.bfloat16)

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
                "no attn node, padded": padded(models["no attn node"]), "no mlp, padded": padded(models["no mlp"]),
                "no layer, padded": padded(models["no layer"]), "unrouted, padded": padded(models["unrouted"])}
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    seen = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            seen[name].append(a.elapsed_time(b) / iters)
    res = {"shape": {"name": shape, **SHAPES[shape], "B": B, "T": T, "live_tokens": int(am.sum()), "packed_rows": int(rows.numel())}}
    print(f"{shape}: {SHAPES[shape]}")
    for name, ts in seen.items():
        ts.sort()
        res[name] = {"ms": ts[len(ts) // 2], "lo": ts[0], "hi": ts[-1]}
        print(f"  {name:22s} {res[name]['ms']:8.3f} ms per forward + backward   (rounds: {ts[0]:.3f} .. {ts[-1]:.3f})")
    print(f"  padded rows {B * T}, live tokens {res['shape']['live_tokens']}, packed rows {res['shape']['packed_rows']}")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=("both", *SHAPES))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="", help="also write the figures to this JSON file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {}
    for shape in (SHAPES if args.shape == "both" else (args.shape,)):
        res[shape] = bench(dev, shape, args.rounds, args.iters)
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
