"""Qwen3 routing without a GPU: the source guards, the installers that must now take a Qwen3 model, the patched model falling
through to transformers' own statements on the CPU (bit for bit), `decoder_only`, and the packed decoder run of a tiny Qwen3
against the padded run."""
import copy

import pytest
import torch

from dalm_amd import packed

from test_packed_cpu import _masks


def _config(**over):
    from transformers import Qwen3Config

    kw = dict(vocab_size=128, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
              num_key_value_heads=2, head_dim=64)
    kw.update(over)
    return Qwen3Config(**kw)


def _tiny_qwen3(**over):
    from transformers import Qwen3ForCausalLM

    torch.manual_seed(0)
    model = Qwen3ForCausalLM(_config(**over))
    with torch.no_grad():                    # norm weights away from their initial ones: a dropped or doubled norm shows
        for name, p in model.named_parameters():
            if name.endswith(("q_norm.weight", "k_norm.weight")):
                p.add_(0.3 * torch.randn(p.shape, generator=torch.Generator().manual_seed(len(name))))
    return model


def test_source_guards_hold_for_the_installed_classes_and_fail_for_a_changed_forward():
    from transformers.models.qwen3 import modeling_qwen3 as mq

    from dalm_amd.models import attention, fastpath

    assert fastpath._qwen3_attention_matches(mq.Qwen3Attention)
    assert fastpath._qwen3_layer_matches(mq.Qwen3DecoderLayer)

    class Qwen3Attention(mq.Qwen3Attention):                   # same name, another forward: no q_norm / k_norm lines
        def forward(self, hidden_states, position_embeddings=None, attention_mask=None, past_key_values=None, **kwargs):
            return mq.Qwen3Attention.forward(self, hidden_states, position_embeddings, attention_mask, past_key_values, **kwargs)

    class Qwen3DecoderLayer(mq.Qwen3DecoderLayer):
        def forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_values=None, use_cache=False,
                    position_embeddings=None, **kwargs):
            return mq.Qwen3DecoderLayer.forward(self, hidden_states, attention_mask, position_ids, past_key_values, use_cache,
                                                position_embeddings, **kwargs)

    with pytest.warns(UserWarning, match="not the code this patch restates"):
        assert not fastpath._qwen3_attention_matches(Qwen3Attention)
    fastpath._warned.discard("qwen3-layer")
    with pytest.warns(UserWarning, match="not the code this patch restates"):
        assert not fastpath._qwen3_layer_matches(Qwen3DecoderLayer)

    model = _tiny_qwen3()
    assert attention.use_hip_attention_backward(model)
    model.model.layers[0].self_attn.__class__ = Qwen3Attention
    model.model.layers[0].__class__ = Qwen3DecoderLayer
    assert fastpath.use_qwen3_attention_node(model) == 1 and fastpath.use_fused_residual_norm(model) == 1
    names = [getattr(getattr(l.self_attn.forward, "__func__", None), "__name__", "") for l in model.model.layers]
    assert names == ["forward", "_qwen3_attention_forward"]                       # the subclass is left unpatched
    assert [hasattr(l, "_dalm_orig_forward") for l in model.model.layers] == [False, True]


def test_installers_take_a_qwen3_model():
    from dalm_amd.models import attention, fastpath

    model = _tiny_qwen3()
    assert model.config._attn_implementation == "sdpa"
    assert attention.use_hip_attention_backward(model) and model.config._attn_implementation == attention.NAME
    assert fastpath.use_swiglu_kernel(model) == 2
    assert fastpath.use_fused_residual_norm(model) == 2
    assert fastpath.use_qwen3_attention_node(model) == 2
    # a model that stays on "sdpa" gets no attention node
    assert fastpath.use_qwen3_attention_node(_tiny_qwen3()) == 0


def test_patched_model_is_transformers_own_on_the_cpu():
    """fp32 on the CPU: every patch falls through to the statements it restates, logits and gradients are equal bit for bit."""
    from dalm_amd.models import attention, fastpath

    ref = _tiny_qwen3()
    model = copy.deepcopy(ref)
    attention.use_hip_attention_backward(model)
    assert fastpath.use_qwen3_attention_node(model) == 2 and fastpath.use_swiglu_kernel(model) == 2
    assert fastpath.use_fused_residual_norm(model) == 2
    B, T = 3, 12
    mask = _masks(B, T, True, 4)
    ids = torch.randint(3, 128, (B, T), generator=torch.Generator().manual_seed(5))
    w = torch.randn(B, T, 128, generator=torch.Generator().manual_seed(6))
    outs = []
    for m in (model, ref):
        logits = m(input_ids=ids, attention_mask=mask, use_cache=False).logits
        (logits * w).sum().backward()
        outs.append(logits.detach())
    assert torch.equal(outs[0], outs[1])
    for (n, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        assert p.grad is not None and torch.equal(p.grad, q.grad), n


def test_decoder_only_admits_qwen3_and_declines_a_short_window():
    from transformers import Qwen3ForCausalLM

    from dalm_amd.models.rag_e2e_base_model import DECODER_ONLY_TYPES, decoder_only

    assert "qwen3" in DECODER_ONLY_TYPES
    model = _tiny_qwen3()
    assert decoder_only(model) and decoder_only(model, 32)
    windowed = Qwen3ForCausalLM(_config(layer_types=["sliding_attention", "full_attention"], sliding_window=8, use_sliding_window=True))
    assert [l.self_attn.sliding_window for l in windowed.model.layers] == [8, None]
    assert not decoder_only(windowed, 32) and not decoder_only(windowed) and decoder_only(windowed, 8)


def test_sliding_window_calls_go_to_transformers_own_function(monkeypatch):
    """`dalm_sdpa_attention_forward` hands a call whose window is shorter than the sequence to `sdpa_attention_forward`."""
    from transformers.integrations import sdpa_attention

    from dalm_amd.models import attention

    seen = []
    real = sdpa_attention.sdpa_attention_forward

    def spy(module, *args, **kwargs):
        seen.append(kwargs.get("sliding_window"))
        return real(module, *args, **kwargs)

    monkeypatch.setattr(sdpa_attention, "sdpa_attention_forward", spy)
    mod = torch.nn.Module()
    mod.num_key_value_groups, mod.is_causal = 1, True
    q = torch.randn(1, 2, 16, 64)
    out, _ = attention.dalm_sdpa_attention_forward(mod, q, q, q, None, sliding_window=8)
    assert seen == [8] and out.shape == (1, 16, 2, 64)


@pytest.mark.parametrize("left", [True, False])
def test_packed_decoder_run_equals_the_padded_run(left):
    from dalm_amd.models import attention

    model = _tiny_qwen3(max_position_embeddings=64).eval()
    B, T = 4, 16
    mask = _masks(B, T, left, 1)
    ids = torch.randint(3, 128, (B, T), generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        want = model.base_model(input_ids=ids, attention_mask=mask, use_cache=False)[0][:, T - 1]
        assert attention.use_hip_attention_backward(model) and packed.attention_is_packable(model)
        rows, cu = packed.pack_plan(mask, shifted=False, multiple=8, last_column=True)
        h = packed.causal_retrieval_hidden(model, ids, mask, rows, cu)
    last = h.index_select(0, cu[1:B + 1].long() - 1)
    assert torch.allclose(last, want, atol=2e-5, rtol=1e-4), float((last - want).abs().max())
