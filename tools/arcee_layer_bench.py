"""One AFM-4.5B decoder layer, forward + backward, with and without the Arcee routing of this package.

    python tools/arcee_layer_bench.py [--rounds 5] [--iters 10] [--out FILE.json]

A one-layer Arcee model at the AFM-4.5B layer shape, stated explicitly (hidden 2560, 20 heads of 128 over 4 key / value heads,
intermediate 18432, ReLU^2, no gate; a 1024-token vocabulary so that the embedding is negligible; `ArceeConfig()`'s own defaults give
head width 80, which is not the published model's), bf16 base weights, LoRA r 8 on q_proj / v_proj, batch 18 x 256 = 4608 rows with
the benchmark's generator lengths (uniform 60 .. 256, left-padded).  Four arms, visited in turn in every round (same process, same
tensors):

  routed, padded          native RMSNorm, ReLU^2 kernels, fused residual + norm, "dalm_sdpa", the rotary + attention node
  routed + node, padded   the same model with the two AFM GEMM shapes put into linear_live's table (`set_table`): the frozen MLP runs
                          as `_FrozenRelu2MlpFn` over the live rows (tools/linear_live_bench.py --candidates says whether the shapes
                          earn their place in the shipped table)
  routed, packed          the routed model on the un-padded rows (dalm_amd/packed.py)
  unrouted, padded        what an Arcee generator got before the routing existed: native RMSNorm, the LoRA group kernels and the
                          transposed dgrad (all keyed by names Arcee shares with Llama) on transformers' "sdpa"; it cannot run packed

Time per call: device events around `iters` forward + backward calls, after a warm-up of every arm; the median of the rounds, with
the lowest and highest.  This is a LAYER time, not a step time: no Arcee training step has been measured."""
from __future__ import annotations

import argparse
import copy
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

HIDDEN, INTER, HEADS, KV_HEADS, HEAD_DIM = 2560, 18432, 20, 4, 128
B, T = 18, 256


def build(dev):
    from transformers import ArceeConfig, ArceeForCausalLM

    from dalm_amd import packed
    from dalm_amd.models import fastpath, lora
    from dalm_amd.models.frozen_linear import use_transposed_dgrad
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    torch.manual_seed(0)
    cfg = ArceeConfig(vocab_size=1024, hidden_size=HIDDEN, intermediate_size=INTER, num_hidden_layers=1, num_attention_heads=HEADS,
                      num_key_value_heads=KV_HEADS, head_dim=HEAD_DIM, max_position_embeddings=4096, bos_token_id=1, eos_token_id=2)
    base = ArceeForCausalLM(cfg)

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

    before = copy.deepcopy(base)
    fastpath.use_native_rms_norm(before)
    before = finish(before)
    assert before.config._attn_implementation == "sdpa" and not packed.attention_is_packable(before)
    routed = base
    went_in = use_generator_fast_paths(routed)
    assert went_in["use_relu2_kernel"] == 1 and went_in["use_fused_residual_norm"] == 1
    assert went_in["use_hip_attention_backward"] and went_in["use_llama_attention_node"] == 1
    routed = finish(routed)
    assert packed.attention_is_packable(routed)
    return routed, before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="", help="also write the figures to this JSON file")
    args = ap.parse_args()
    from dalm_amd import hip, linear_live, live_rows, packed

    dev = torch.device("cuda:0")
    routed, before = build(dev)
    g = torch.Generator().manual_seed(0)
    glen = torch.randint(60, T + 1, (B, 1), generator=g)
    am = (torch.arange(T).unsqueeze(0) >= (T - glen)).long().to(dev)
    ids = torch.randint(0, 1024, (B, T), generator=g).to(dev)
    rows, cu = packed.pack_plan(am.cpu(), shifted=True, multiple=packed.ROW_MULTIPLES["generator"])
    rows, cu = rows.to(dev), cu.to(dev)
    w_pad = torch.randn(B, T, HIDDEN, device=dev, dtype=torch.bfloat16)
    w_pack = torch.randn(rows.numel(), HIDDEN, device=dev, dtype=torch.bfloat16)
    node_table = set(linear_live.ROUTED_SHAPES) | {(B * T, INTER, HIDDEN), (B * T, HIDDEN, INTER)}

    def padded(model, table=None):
        def run():
            linear_live.set_table(table)
            try:
                with torch.autocast("cuda", dtype=torch.bfloat16), live_rows.tower_call(am, shifted=True):
                    h = model.base_model(input_ids=ids, attention_mask=am, use_cache=False)[0]
                (h * w_pad).sum().backward()
            finally:
                linear_live.set_table(None)
        return run

    def packed_run():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            h = packed.generator_hidden(routed, ids, am, rows, cu)
        (h * w_pack).sum().backward()

    variants = {"routed, padded": padded(routed), "routed + node, padded": padded(routed, node_table), "routed, packed": packed_run,
                "unrouted, padded": padded(before)}
    # the node arm must reach the node, the others must not
    seen_calls, real_call = [], hip.call
    hip.call = lambda name, *a: (seen_calls.append(name), real_call(name, *a))[1]
    try:
        for name, fn in variants.items():
            seen_calls.clear()
            fn()
            assert ("dalm_linear_live_relu2" in seen_calls) == (name == "routed + node, padded"), (name, sorted(set(seen_calls)))
            assert ("dalm_relu2_bwd" in seen_calls) == (name != "unrouted, padded"), (name, sorted(set(seen_calls)))
    finally:
        hip.call = real_call
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
    res = {"shape": {"B": B, "T": T, "hidden": HIDDEN, "intermediate": INTER, "heads": HEADS, "kv_heads": KV_HEADS, "head_dim": HEAD_DIM,
                     "live_tokens": int(am.sum()), "packed_rows": int(rows.numel())}}
    for name, ts in seen.items():
        ts.sort()
        res[name] = {"ms": ts[len(ts) // 2], "lo": ts[0], "hi": ts[-1]}
        print(f"{name:22s} {res[name]['ms']:8.3f} ms per forward + backward   (rounds: {ts[0]:.3f} .. {ts[-1]:.3f}, "
              f"spread {ts[-1] - ts[0]:.3f})")
    ref = res["unrouted, padded"]["ms"]
    for name in variants:
        if name != "unrouted, padded":
            print(f"{name:22s} {ref / res[name]['ms']:6.3f} x the unrouted layer in the same run")
    print(f"padded rows {B * T}, live tokens {res['shape']['live_tokens']}, packed rows {res['shape']['packed_rows']}")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
