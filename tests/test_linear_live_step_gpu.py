"""The live-row GEMM route inside a training step: a depth-1 Llama-shaped generator (width 256 = 2 heads of 128, intermediate 512,
LoRA on q / v) over 3 x 96 left-padded rows through `RagE2EStep`, bf16 autocast with frozen bf16 weights, route on and off,
each compared to an fp32 run of the same model on the same batch (all dropout off: the three runs compute the same function).

Deviation of a run = |loss - loss_fp32| for the loss and ||g - g_fp32|| / ||g_fp32|| (Frobenius) for every LoRA gradient; the norm,
not the largest element, because one element's rounding luck is not what the route changes.  The route-on deviation may not exceed
twice the route-off deviation, quantity by quantity, and the route-on run must have launched `dalm_linear_live` (call counter).
The routing table is set to this model's shapes for the test (the measured table holds the 4608-row shapes only).
"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

B, T, H, INTER, V = 3, 96, 256, 512, 512
R = B * T
# every frozen projection of the layer, forward and dgrad, and the lm_head: (rows, N, K)
SHAPES = [(R, 3 * H, H), (R, H, H), (R, 2 * INTER, H), (R, H, INTER), (R, INTER, H), (R, V, H), (R, H, V)]
_TOWERS = {}


def _towers():
    if not _TOWERS:
        from transformers import BertConfig, BertModel, LlamaConfig, LlamaForCausalLM

        from dalm_amd.models import lora
        from dalm_amd.models.lora import LoRALinear

        torch.manual_seed(77)
        retriever = BertModel(BertConfig(hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256,
                                         vocab_size=V, max_position_embeddings=64, hidden_dropout_prob=0.0,
                                         attention_probs_dropout_prob=0.0))
        generator = LlamaForCausalLM(LlamaConfig(hidden_size=H, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=2,
                                                 intermediate_size=INTER, vocab_size=V, max_position_embeddings=128,
                                                 attention_dropout=0.0, pad_token_id=0))
        lora.inject_lora(retriever, ["key", "query", "value"], lora_dropout=0.0)
        lora.inject_lora(generator, ["q_proj", "v_proj"], lora_dropout=0.0)
        g = torch.Generator().manual_seed(78)
        for mod in (retriever, generator):
            for m in mod.modules():
                if isinstance(m, LoRALinear):      # lora_B starts at zero, which zeroes every lora_A gradient
                    with torch.no_grad():
                        m.lora_B["default"].weight.copy_(0.05 * torch.randn(m.lora_B["default"].weight.shape, generator=g))
        # frozen weights that ARE bf16 values: the fp32 run and the bf16 runs then hold the same model
        for mod in (retriever, generator):
            for p in mod.parameters():
                if not p.requires_grad:
                    p.data = p.data.bfloat16().float()
        _TOWERS["r"], _TOWERS["g"] = retriever, generator
    return copy.deepcopy(_TOWERS["r"]), copy.deepcopy(_TOWERS["g"])


def _batch(dev):
    g = torch.Generator().manual_seed(6)
    gm = torch.ones(B, T, dtype=torch.int64)
    gm[1, :37] = 0                                        # left-padded, as Llama tokenizers pad
    gm[2, :70] = 0

    def right(Tn, lens):
        return (torch.arange(Tn).unsqueeze(0) < torch.tensor(lens).unsqueeze(1)).long()

    return {k: v.to(dev) for k, v in {
        "retriever_query_input_ids": torch.randint(5, V, (B, 12), generator=g),
        "retriever_query_attention_mask": right(12, [12, 7, 3]),
        "retriever_passage_input_ids": torch.randint(5, V, (B, 20), generator=g),
        "retriever_passage_attention_mask": right(20, [20, 11, 5]),
        "generator_input_input_ids": torch.randint(5, V, (B, T), generator=g),
        "generator_input_attention_mask": gm,
        "query_passage_input_len": torch.tensor([60, 30, 10]),
    }.items()}


class _Recording(torch.optim.SGD):
    """lr = 0: the step keeps what the backward produced instead of applying it."""

    def step(self, closure=None):
        self.seen = [p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)
                     for grp in self.param_groups for p in grp["params"]]


def _run(dev, bf16, route):
    from dalm_amd import linear_live
    from dalm_amd.models import AutoModelForRagE2E
    from dalm_amd.models.lora import LoRALinear
    from dalm_amd.training.step import RagE2EStep

    r, g = _towers()
    LoRALinear._count = 200000
    model = AutoModelForRagE2E.from_modules(r, g, None, None, normalize=True, get_peft=None).to(dev)
    if bf16:
        for p in model.parameters():
            if not p.requires_grad:
                p.data = p.data.to(torch.bfloat16)
    model.train()
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    opt = _Recording([p for _, p in named], lr=0.0)
    step = RagE2EStep(model, opt, None, 100, autocast_dtype=torch.bfloat16 if bf16 else None, inplace_grad=True,
                      overlap_towers=False)
    linear_live.set_table(SHAPES)
    linear_live.set_enabled(route)
    before = linear_live.calls()
    try:
        loss = step(_batch(dev)).double().item()
        torch.cuda.synchronize()
    finally:
        linear_live.set_table(None)
        linear_live.set_enabled(True)
    grads = {n: gr.double() for (n, _), gr in zip(named, opt.seen)}
    return loss, grads, linear_live.calls() - before


def test_route_on_is_no_further_from_fp32_than_twice_route_off():
    from dalm_amd import hip

    hip.load()
    dev = torch.device("cuda:0")
    loss32, g32, n32 = _run(dev, bf16=False, route=True)          # fp32: the predicate keeps every call in the library
    loss_off, g_off, n_off = _run(dev, bf16=True, route=False)
    loss_on, g_on, n_on = _run(dev, bf16=True, route=True)
    assert n32 == 0 and n_off == 0, (n32, n_off)
    assert n_on > 0, "the route-on run never launched dalm_linear_live"
    print(f"dalm_linear_live launches with the route on: {n_on}")
    gen = [n for n in g32 if "generator" in n]
    assert gen and all(float(g32[n].norm()) > 0 for n in gen), "a generator LoRA gradient is zero: the test would compare nothing"

    def dev_of(g, n):
        return float((g[n] - g32[n]).norm() / g32[n].norm().clamp_min(1e-300))

    d_off, d_on = abs(loss_off - loss32), abs(loss_on - loss32)
    print(f"loss fp32 {loss32:.8f}  off {loss_off:.8f} (dev {d_off:.3e})  on {loss_on:.8f} (dev {d_on:.3e})")
    worst = []
    for n in sorted(g32):
        a, b = dev_of(g_off, n), dev_of(g_on, n)
        print(f"{n:90s} off {a:.3e}  on {b:.3e}")
        if b > 2 * a:
            worst.append((n, a, b))
    assert d_on <= 2 * d_off, f"loss: route on {d_on:.3e} from fp32, route off {d_off:.3e}"
    assert not worst, worst
