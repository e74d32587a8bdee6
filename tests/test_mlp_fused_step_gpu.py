"""The fused frozen-MLP node inside a training step: a depth-1 Llama-shaped generator (width 256 = 2 heads of 128, intermediate 384 =
three mixed tiles, LoRA on q / v) over 2 x 96 left-padded rows through `RagE2EStep`, bf16 autocast with frozen bf16 weights, with
`linear_live.set_mlp_fused` on and off.  Both arms run the same GEMM contraction order and the same elementwise function
(csrc/swiglu_math.hpp): the loss and every trainable gradient must be EQUAL, not close.  The routing table is set to this model's
shapes for the test (the measured table holds the 4608-row shapes only), as tests/test_linear_live_step_gpu.py does.

Second test: the MLP forward and backward captured in a hipGraph inside a padded tower call and replayed with a second mask - the
`perm` / `n_live` that `dalm_row_partition` writes INSIDE the graph are what the node's kernels must read on every replay.
"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

B, T, H, INTER, V = 2, 96, 256, 384, 512
R = B * T
# every frozen projection of the layer, forward and dgrad, and the lm_head: (rows, N, K)
SHAPES = [(R, 3 * H, H), (R, H, H), (R, 2 * INTER, H), (R, H, INTER), (R, INTER, H), (R, V, H), (R, H, V)]
_TOWERS = {}


def _towers():
    if not _TOWERS:
        from transformers import BertConfig, BertModel, LlamaConfig, LlamaForCausalLM

        from dalm_amd.models import lora
        from dalm_amd.models.lora import LoRALinear

        torch.manual_seed(91)
        retriever = BertModel(BertConfig(hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256,
                                         vocab_size=V, max_position_embeddings=64, hidden_dropout_prob=0.0,
                                         attention_probs_dropout_prob=0.0))
        generator = LlamaForCausalLM(LlamaConfig(hidden_size=H, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=2,
                                                 intermediate_size=INTER, vocab_size=V, max_position_embeddings=128,
                                                 attention_dropout=0.0, pad_token_id=0))
        lora.inject_lora(retriever, ["key", "query", "value"], lora_dropout=0.0)
        lora.inject_lora(generator, ["q_proj", "v_proj"], lora_dropout=0.0)
        g = torch.Generator().manual_seed(92)
        for mod in (retriever, generator):
            for m in mod.modules():
                if isinstance(m, LoRALinear):      # lora_B starts at zero, which zeroes every lora_A gradient
                    with torch.no_grad():
                        m.lora_B["default"].weight.copy_(0.05 * torch.randn(m.lora_B["default"].weight.shape, generator=g))
        _TOWERS["r"], _TOWERS["g"] = retriever, generator
    return copy.deepcopy(_TOWERS["r"]), copy.deepcopy(_TOWERS["g"])


def _batch(dev):
    g = torch.Generator().manual_seed(8)
    gm = torch.ones(B, T, dtype=torch.int64)
    gm[0, :11] = 0                                        # left-padded, as Llama tokenizers pad
    gm[1, :70] = 0

    def right(Tn, lens):
        return (torch.arange(Tn).unsqueeze(0) < torch.tensor(lens).unsqueeze(1)).long()

    return {k: v.to(dev) for k, v in {
        "retriever_query_input_ids": torch.randint(5, V, (B, 12), generator=g),
        "retriever_query_attention_mask": right(12, [12, 7]),
        "retriever_passage_input_ids": torch.randint(5, V, (B, 20), generator=g),
        "retriever_passage_attention_mask": right(20, [20, 11]),
        "generator_input_input_ids": torch.randint(5, V, (B, T), generator=g),
        "generator_input_attention_mask": gm,
        "query_passage_input_len": torch.tensor([60, 15]),
    }.items()}


class _Recording(torch.optim.SGD):
    """lr = 0: the step keeps what the backward produced instead of applying it."""

    def step(self, closure=None):
        self.seen = [p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)
                     for grp in self.param_groups for p in grp["params"]]


class _Counted:
    """Count the launches of the fused entry point through its wrapper."""

    def __init__(self, monkeypatch):
        from dalm_amd import linear_live

        self.n = {"fwd": 0}
        fwd = linear_live.linear_live_swiglu

        def cf(*a, **k):
            self.n["fwd"] += 1
            return fwd(*a, **k)

        monkeypatch.setattr(linear_live, "linear_live_swiglu", cf)


def _run(dev, fused):
    from dalm_amd import linear_live
    from dalm_amd.models import AutoModelForRagE2E
    from dalm_amd.models.lora import LoRALinear
    from dalm_amd.training.step import RagE2EStep

    r, g = _towers()
    LoRALinear._count = 300000
    model = AutoModelForRagE2E.from_modules(r, g, None, None, normalize=True, get_peft=None).to(dev)
    for p in model.parameters():
        if not p.requires_grad:
            p.data = p.data.to(torch.bfloat16)
    model.train()
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    opt = _Recording([p for _, p in named], lr=0.0)
    step = RagE2EStep(model, opt, None, 100, autocast_dtype=torch.bfloat16, inplace_grad=True, overlap_towers=False)
    linear_live.set_table(SHAPES)
    linear_live.set_enabled(True)
    linear_live.set_mlp_fused(fused)
    try:
        loss = step(_batch(dev)).detach().clone()
        torch.cuda.synchronize()
    finally:
        linear_live.set_table(None)
        linear_live.set_mlp_fused(True)
    return loss, {n: gr for (n, _), gr in zip(named, opt.seen)}


def test_step_with_the_fused_node_equals_the_step_without(monkeypatch):
    from dalm_amd import hip

    hip.load()
    dev = torch.device("cuda:0")
    counted = _Counted(monkeypatch)
    loss_off, g_off = _run(dev, fused=False)
    assert counted.n == {"fwd": 0}, counted.n
    gen = [n for n in g_off if "generator" in n]
    assert gen and all(float(g_off[n].float().norm()) > 0 for n in gen), "a generator LoRA gradient is zero: nothing compared"
    # the node: forward epilogue fused, backward as two launches
    loss_on, g_on = _run(dev, fused=True)
    print(f"fused launches: {counted.n}; loss off {float(loss_off):.8f} on {float(loss_on):.8f}")
    assert counted.n["fwd"] >= 1, f"the fused node did not run: {counted.n}"
    assert torch.equal(loss_on, loss_off), (float(loss_on), float(loss_off))
    differing = [n for n in sorted(g_off) if not torch.equal(g_on[n], g_off[n])]
    assert not differing, differing


def _mlp(dev):
    from dalm_amd.models import fastpath, frozen_linear

    _, gen = _towers()
    mlp = gen.model.layers[0].mlp.to(dev).to(torch.bfloat16)
    for p in mlp.parameters():
        p.requires_grad_(False)
    frozen_linear.use_transposed_dgrad(mlp)
    return mlp, lambda x: fastpath._swiglu_mlp_forward(mlp, x)


def _masks(dev):
    first = torch.ones(B, T, dtype=torch.int64)
    first[0, :11] = 0
    first[1, :70] = 0
    second = torch.ones(B, T, dtype=torch.int64)
    second[0, :50] = 0
    second[1, :3] = 0
    return first.to(dev), second.to(dev)


def _captured(dev, fused, x0, g0, masks):
    """MLP forward + backward inside a padded tower call, captured once with the first mask, replayed with both -> [(out, dx)]."""
    from dalm_amd import linear_live, live_rows

    mlp, fwd = _mlp(dev)
    x = x0.clone().requires_grad_(True)
    mask = masks[0].clone()

    def body():
        with live_rows.tower_call(mask, shifted=True):
            out = fwd(x)
        (dx,) = torch.autograd.grad(out, x, g0)
        return out, dx

    linear_live.set_table(SHAPES)
    linear_live.set_mlp_fused(fused)
    try:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            body()                                                   # warm-up: weight concatenation and transposed copies
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                out, dx = body()
        torch.cuda.current_stream().wait_stream(s)
        results = []
        for m in masks:
            mask.copy_(m)
            out.detach().fill_(7.0)
            dx.detach().fill_(7.0)
            graph.replay()
            torch.cuda.synchronize()
            results.append((out.detach().clone(), dx.detach().clone()))
    finally:
        linear_live.set_table(None)
        linear_live.set_mlp_fused(True)
    return results


def test_graph_replay_follows_a_changed_mask(monkeypatch):
    from dalm_amd import hip, live_rows

    hip.load()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(B, T, H, generator=g).bfloat16().to(dev)
    g0 = torch.randn(B, T, H, generator=g).bfloat16().to(dev)
    masks = _masks(dev)
    counted = _Counted(monkeypatch)
    off = _captured(dev, False, x0, g0, masks)
    assert counted.n == {"fwd": 0}
    on = _captured(dev, True, x0, g0, masks)
    assert counted.n["fwd"] >= 1, f"the fused node did not run: {counted.n}"
    for m, (o_on, d_on), (o_off, d_off) in zip(masks, on, off):
        keep = live_rows.live_rows(m, True).view(B, T) != 0
        assert torch.equal(o_on, o_off) and torch.equal(d_on, d_off)
        assert not o_on[~keep].view(torch.int16).any() and not d_on[~keep].view(torch.int16).any()     # what leaves the node: zeros
        assert bool(o_on[keep].float().abs().sum() > 0) and bool(d_on[keep].float().abs().sum() > 0)
    assert not torch.equal(on[0][0], on[1][0]), "the replay with the second mask reproduced the first mask's result"
