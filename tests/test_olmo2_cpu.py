"""OLMo-2 routing without a GPU: the installers take a tiny Olmo2ForCausalLM - "dalm_sdpa", packable, the layer, attention and MLP
forwards bound by name, the counts - the reference switches turn them off, biased projections and edited code are declined, olmo and
olmo3 models come out as they went in, the patched model is transformers' own on CPU tensors (bit for bit, LoRA gradients included),
what follows from the Llama-named projections (the q | k | v LoRA group, the transposed dgrad swap) is there, and the packed decoder
run equals the padded one."""
import copy
import warnings

import pytest
import torch

from dalm_amd import packed

from test_packed_cpu import _masks


def _config(**over):
    from transformers import Olmo2Config

    kw = dict(vocab_size=128, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
              num_key_value_heads=2, pad_token_id=1, bos_token_id=None, eos_token_id=2)
    kw.update(over)
    return Olmo2Config(**kw)


def _tiny_olmo2(**over):
    from transformers import Olmo2ForCausalLM

    torch.manual_seed(0)
    model = Olmo2ForCausalLM(_config(**over))
    with torch.no_grad():                    # norm weights away from their initial ones: a dropped, doubled or misplaced norm shows
        for name, p in model.named_parameters():
            if name.endswith(("norm.weight", "layernorm.weight")):
                p.add_(0.3 * torch.randn(p.shape, generator=torch.Generator().manual_seed(len(name))))
    return model


def _forward_names(mods):
    return [getattr(getattr(m.forward, "__func__", None), "__name__", "") for m in mods]


def test_olmo2_is_what_the_routing_rests_on():
    """Read from the installed transformers: no input_layernorm, the q / k norms span all heads of a token, rotary and MLP are
    Llama's source text."""
    import inspect

    from transformers.models.llama import modeling_llama as ml
    from transformers.models.olmo2 import modeling_olmo2 as mo

    assert inspect.getsource(mo.Olmo2MLP.forward) == inspect.getsource(ml.LlamaMLP.forward)
    layer = _tiny_olmo2().model.layers[0]
    assert not hasattr(layer, "input_layernorm")
    assert layer.self_attn.q_norm.weight.shape == (4 * 64,) and layer.self_attn.k_norm.weight.shape == (2 * 64,)
    x = torch.randn(3, 256)
    n = layer.post_attention_layernorm
    assert torch.equal(n(x), (n.weight * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + n.variance_epsilon))))


def test_installers_take_an_olmo2_model_and_bind_the_forwards():
    from dalm_amd.models import attention, fastpath
    from dalm_amd.models.rag_e2e_base_model import _GENERATOR_PATHS, _RETRIEVER_PATHS, DECODER_ONLY_TYPES, use_generator_fast_paths

    model = _tiny_olmo2()
    assert model.config._attn_implementation == "sdpa" and not packed.attention_is_packable(model)
    got = use_generator_fast_paths(model)
    assert model.config._attn_implementation == attention.NAME and packed.attention_is_packable(model)
    assert got["use_hip_attention_backward"] is True
    assert got["use_olmo2_layer"] == 2 and got["use_olmo2_attention_node"] == 2 and got["use_swiglu_kernel"] == 2
    assert got["use_native_rms_norm"] == 9                                # four per layer and the final one
    assert got["use_fused_residual_norm"] == 0 and got["use_llama_attention_node"] == 0 and got["use_qwen3_attention_node"] == 0
    assert got["use_geglu_kernel"] == 0 and got["use_relu2_kernel"] == 0 and got["use_roll_rope"] is False
    layers = model.model.layers
    assert _forward_names(layers) == ["_olmo2_layer_forward"] * 2 and all(hasattr(l, "_dalm_orig_forward") for l in layers)
    assert _forward_names(l.self_attn for l in layers) == ["_olmo2_attention_forward"] * 2
    assert all(hasattr(l.self_attn, "_dalm_orig_attn_forward") for l in layers)
    assert _forward_names(l.mlp for l in layers) == ["_swiglu_mlp_forward"] * 2
    # the attention node goes in after the switch to "dalm_sdpa"; OLMo-2 is a generator only
    order = list(_GENERATOR_PATHS)
    assert order.index(fastpath.use_olmo2_attention_node) > order.index(attention.use_hip_attention_backward)
    assert fastpath.use_olmo2_layer in order
    assert fastpath.use_olmo2_layer not in _RETRIEVER_PATHS and fastpath.use_olmo2_attention_node not in _RETRIEVER_PATHS
    assert "olmo2" not in DECODER_ONLY_TYPES
    # a model that stays on "sdpa" gets no attention node
    assert fastpath.use_olmo2_attention_node(_tiny_olmo2()) == 0


def test_head_width_32_gets_dalm_sdpa_but_no_fused_node_on_the_gpu_path():
    """The head-width rule is the attention kernels': width 32 switches to "dalm_sdpa"; the node's own support predicate declines
    that width at call time (`tower_ops.row_norm_rope_supported`), as for Qwen3.  Width 16 stays on "sdpa"."""
    from dalm_amd.models import attention, tower_ops

    narrow = _tiny_olmo2(hidden_size=128, num_attention_heads=4, num_key_value_heads=2)
    assert attention.use_hip_attention_backward(narrow) and narrow.config._attn_implementation == attention.NAME
    assert 32 not in tower_ops._HEAD_NORM_DIMS
    tiny = _tiny_olmo2(hidden_size=64, num_attention_heads=4, num_key_value_heads=2)
    assert not attention.use_hip_attention_backward(tiny) and tiny.config._attn_implementation == "sdpa"


@pytest.mark.parametrize("switch", ["DALM_NORM_KERNEL", "DALM_SWIGLU_KERNEL", "DALM_ATTN_KERNEL"])
def test_the_reference_switches_turn_the_installers_off(monkeypatch, switch):
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    monkeypatch.setenv(switch, "0")
    model = _tiny_olmo2()
    got = use_generator_fast_paths(model)
    layers = model.model.layers
    norm_on, mlp_on, attn_on = (switch != s for s in ("DALM_NORM_KERNEL", "DALM_SWIGLU_KERNEL", "DALM_ATTN_KERNEL"))
    assert got["use_olmo2_layer"] == (2 if norm_on else 0)
    assert got["use_swiglu_kernel"] == (2 if mlp_on else 0)
    assert got["use_hip_attention_backward"] is attn_on and got["use_olmo2_attention_node"] == (2 if attn_on else 0)
    assert _forward_names(layers) == ["_olmo2_layer_forward" if norm_on else "forward"] * 2
    assert _forward_names(l.mlp for l in layers) == ["_swiglu_mlp_forward" if mlp_on else "forward"] * 2
    assert _forward_names(l.self_attn for l in layers) == ["_olmo2_attention_forward" if attn_on else "forward"] * 2
    assert model.config._attn_implementation == ("dalm_sdpa" if attn_on else "sdpa")
    assert packed.attention_is_packable(model) is attn_on


def test_attention_switches_are_read_at_call_time(monkeypatch):
    """DALM_ATTN_KERNEL / DALM_FAST_ROPE set after the installers ran: the patched attention calls the module's own forward."""
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    model = _tiny_olmo2()
    use_generator_fast_paths(model)
    attn = model.model.layers[0].self_attn
    seen = []
    own = attn._dalm_orig_attn_forward
    attn._dalm_orig_attn_forward = lambda *a, **k: (seen.append(1), own(*a, **k))[1]
    ids = torch.randint(3, 128, (2, 8), generator=torch.Generator().manual_seed(1))
    model(input_ids=ids, use_cache=False)
    assert seen == []
    for switch in ("DALM_ATTN_KERNEL", "DALM_FAST_ROPE"):
        monkeypatch.setenv(switch, "0")
        model(input_ids=ids, use_cache=False)
        monkeypatch.delenv(switch)
    assert seen == [1, 1]
    model(input_ids=ids, use_cache=True)                                  # a KV cache: the module's own forward as well
    assert seen == [1, 1, 1]


def test_biased_projections_and_other_mlps_are_declined():
    from dalm_amd.models import attention, fastpath

    biased = _tiny_olmo2(attention_bias=True)
    assert attention.use_hip_attention_backward(biased)
    assert fastpath.use_olmo2_attention_node(biased) == 0
    assert _forward_names(l.self_attn for l in biased.model.layers) == ["forward"] * 2
    assert fastpath.use_olmo2_layer(biased) == 2                          # the layer's norms do not care
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gelu = _tiny_olmo2(hidden_act="gelu")
        assert fastpath.use_swiglu_kernel(gelu) == 0 and _forward_names(l.mlp for l in gelu.model.layers) == ["forward"] * 2


def test_changed_code_is_declined_and_left_in_place():
    from transformers.models.olmo2 import modeling_olmo2 as mo

    from dalm_amd.models import attention, fastpath

    class Olmo2DecoderLayer(mo.Olmo2DecoderLayer):               # the whole body with ONE statement changed (the last add)
        def forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_values=None, use_cache=False,
                    position_embeddings=None, **kwargs):
            residual = hidden_states
            hidden_states, _ = self.self_attn(
                hidden_states=hidden_states,
                attention_mask=attention_mask,
                position_ids=position_ids,
                past_key_values=past_key_values,
                use_cache=use_cache,
                position_embeddings=position_embeddings,
                **kwargs,
            )
            hidden_states = self.post_attention_layernorm(hidden_states)
            hidden_states = residual + hidden_states
            residual = hidden_states
            hidden_states = self.mlp(hidden_states)
            hidden_states = self.post_feedforward_layernorm(hidden_states)
            hidden_states = hidden_states + residual
            return hidden_states

    class Olmo2Attention(mo.Olmo2Attention):                     # same name, another forward text
        def forward(self, hidden_states, position_embeddings=None, attention_mask=None, past_key_values=None, **kwargs):
            return mo.Olmo2Attention.forward(self, hidden_states, position_embeddings, attention_mask, past_key_values, **kwargs)

    class Olmo2MLP(mo.Olmo2MLP):                                 # same name, an edited forward: the value probe says no
        def forward(self, x):
            return self.down_proj(self.act_fn(self.gate_proj(x)) * self.up_proj(x)) * 0.5

    assert fastpath._matches("olmo2-layer", mo.Olmo2DecoderLayer) and fastpath._matches("olmo2-attn", mo.Olmo2Attention)
    with pytest.warns(UserWarning, match="not the code this patch restates"):
        assert not fastpath._matches("olmo2-layer", Olmo2DecoderLayer)
    with pytest.warns(UserWarning, match="not the code this patch restates"):
        assert not fastpath._matches("olmo2-attn", Olmo2Attention)
    model = _tiny_olmo2()
    layers = model.model.layers
    layers[0].mlp.__class__ = Olmo2MLP
    layers[1].__class__ = Olmo2DecoderLayer
    layers[0].self_attn.__class__ = Olmo2Attention
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert attention.use_hip_attention_backward(model)
        assert fastpath.use_swiglu_kernel(model) == 1
        assert fastpath.use_olmo2_layer(model) == 1
        assert fastpath.use_olmo2_attention_node(model) == 1
    assert _forward_names(l.mlp for l in layers) == ["forward", "_swiglu_mlp_forward"]
    assert _forward_names(layers) == ["_olmo2_layer_forward", "forward"]
    assert [hasattr(l, "_dalm_orig_forward") for l in layers] == [True, False]
    assert _forward_names(l.self_attn for l in layers) == ["forward", "_olmo2_attention_forward"]
    # a layer whose norm is another class keeps its forward too
    model = _tiny_olmo2()
    model.model.layers[0].post_feedforward_layernorm = torch.nn.LayerNorm(256)
    assert fastpath.use_olmo2_layer(model) == 1 and _forward_names(model.model.layers) == ["forward", "_olmo2_layer_forward"]


def _olmo_relatives():
    from transformers import Olmo3Config, Olmo3ForCausalLM, OlmoConfig, OlmoForCausalLM

    kw = dict(vocab_size=128, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
              num_key_value_heads=2, pad_token_id=1, bos_token_id=None, eos_token_id=2)
    torch.manual_seed(0)
    return [("olmo", OlmoForCausalLM(OlmoConfig(**kw))), ("olmo3", Olmo3ForCausalLM(Olmo3Config(**kw)))]


def test_olmo_and_olmo3_are_left_as_they_are():
    """Neither installer of this family, nor `use_swiglu_kernel` / "dalm_sdpa", touches `olmo` or `olmo3`: what
    `use_generator_fast_paths` returns for them is what the installers known before OLMo-2 return, and every forward is the class's."""
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    for kind, model in _olmo_relatives():
        assert model.config.model_type == kind
        got = use_generator_fast_paths(model)
        assert got["use_olmo2_layer"] == 0 and got["use_olmo2_attention_node"] == 0, kind
        assert got["use_swiglu_kernel"] == 0 and got["use_hip_attention_backward"] is False and got["use_fused_residual_norm"] == 0, kind
        assert got["use_llama_attention_node"] == 0 and got["use_qwen3_attention_node"] == 0, kind
        assert model.config._attn_implementation == "sdpa" and not packed.attention_is_packable(model), kind
        layers = model.model.layers
        assert _forward_names(layers) == ["forward"] * 2, kind
        assert _forward_names(l.self_attn for l in layers) == ["forward"] * 2 and _forward_names(l.mlp for l in layers) == ["forward"] * 2
        assert not any(hasattr(m, "_dalm_orig_forward") or hasattr(m, "_dalm_orig_attn_forward") for m in model.modules()), kind


def test_patched_model_is_transformers_own_on_the_cpu():
    """fp32 on the CPU: every patch falls through to the statements it restates; logits and LoRA gradients are equal bit for bit."""
    from dalm_amd.models import lora
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    ref = _tiny_olmo2()
    model = copy.deepcopy(ref)
    got = use_generator_fast_paths(model)
    assert got["use_olmo2_layer"] == 2 and got["use_olmo2_attention_node"] == 2 and got["use_swiglu_kernel"] == 2
    for m in (model, ref):
        torch.manual_seed(3)                                              # the same adapter initialisation in both
        lora.inject_lora(m, ["q_proj", "v_proj"], lora_dropout=0.0)
        with torch.no_grad():                                             # B away from zero: the A gradients say something
            for name, p in m.named_parameters():
                if "lora_B" in name:
                    p.copy_(0.05 * torch.randn(p.shape, generator=torch.Generator().manual_seed(len(name))))
    B, T = 3, 12
    mask = _masks(B, T, True, 4)
    ids = torch.randint(3, 128, (B, T), generator=torch.Generator().manual_seed(5))
    w = torch.randn(B, T, 128, generator=torch.Generator().manual_seed(6))
    outs = []
    for m in (model, ref):
        logits = m(input_ids=ids, attention_mask=mask, use_cache=False).logits
        (logits * w).sum().backward()
        outs.append(logits.detach())
    assert torch.equal(outs[0], outs[1]), float((outs[0] - outs[1]).abs().max())
    seen = 0
    for (n, p), (n2, q) in zip(model.named_parameters(), ref.named_parameters()):
        assert n == n2 and p.requires_grad == q.requires_grad
        if p.requires_grad:
            assert "lora_" in n and p.grad is not None and torch.equal(p.grad, q.grad), n
            assert float(p.grad.abs().max()) > 0.0, n
            seen += 1
    assert seen == 2 * 2 * 2                                              # A and B of q_proj and v_proj, two layers


def test_trainable_norm_weights_get_transformers_own_gradients_on_the_cpu():
    """Without adapters everything trains: the norm weights' gradients through the patched layer and attention are the class's own."""
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    ref = _tiny_olmo2()
    model = copy.deepcopy(ref)
    use_generator_fast_paths(model)
    ids = torch.randint(3, 128, (2, 10), generator=torch.Generator().manual_seed(7))
    for m in (model, ref):
        m(input_ids=ids, use_cache=False).logits.square().sum().backward()
    for (n, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        if n.endswith(("norm.weight", "layernorm.weight")):
            assert torch.equal(p.grad, q.grad), n


def test_what_follows_from_the_llama_named_projections():
    """Confirmed, not assumed: the reference's LoRA targets apply as they stand and q | k | v form ONE group of three (the one-GEMM
    q | k | v and its LoRA kernels key on it), every other frozen projection takes the transposed-dgrad class, no projection has a
    bias, and the group sees grouped heads (k / v narrower than q)."""
    from dalm_amd.models import lora
    from dalm_amd.models.frozen_linear import FrozenLinearT, use_transposed_dgrad
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    model = _tiny_olmo2()
    use_generator_fast_paths(model)
    lora.inject_lora(model, ["q_proj", "v_proj"], lora_dropout=0.0)
    swapped = use_transposed_dgrad(model)
    assert swapped == 2 * 4 + 1                                           # o_proj, gate_proj, up_proj, down_proj per layer, the lm_head
    for layer in model.model.layers:
        a = layer.self_attn
        assert isinstance(a.q_proj, lora.LoRALinear) and isinstance(a.v_proj, lora.LoRALinear)
        assert a.q_proj._group is not None and a.q_proj._group is a.k_proj._group is a.v_proj._group
        assert len(a.q_proj._group.members) == 3
        assert all(getattr(getattr(m, "base_layer", m), "bias", None) is None for m in (a.q_proj, a.k_proj, a.v_proj, a.o_proj))
        assert type(a.o_proj) is FrozenLinearT and type(layer.mlp.down_proj) is FrozenLinearT
        assert type(layer.mlp.gate_proj) is FrozenLinearT and type(layer.mlp.up_proj) is FrozenLinearT
        q_w = getattr(a.q_proj, "base_layer", a.q_proj).weight
        k_w = getattr(a.k_proj, "base_layer", a.k_proj).weight
        assert q_w.shape == (256, 256) and k_w.shape == (128, 256)        # 4 query heads over 2 key / value heads
    trainable = [n for n, p in model.named_parameters() if p.requires_grad]
    assert trainable and all("lora_" in n for n in trainable)


@pytest.mark.parametrize("left", [True, False])
def test_packed_decoder_run_equals_the_padded_run(left):
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    model = _tiny_olmo2(max_position_embeddings=64).eval()
    B, T = 4, 16
    mask = _masks(B, T, left, 1)
    ids = torch.randint(3, 128, (B, T), generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        want = model.base_model(input_ids=ids, attention_mask=mask, use_cache=False)[0]
        use_generator_fast_paths(model)
        assert packed.attention_is_packable(model)
        rows, cu = packed.pack_plan(mask, shifted=True, multiple=8)
        h = packed.generator_hidden(model, ids, mask, rows, cu)
    valid = rows >= 0
    sel = rows[valid]
    seen = mask.reshape(-1).index_select(0, sel) != 0
    got, ref = h[valid][seen], want.reshape(B * T, -1).index_select(0, sel)[seen]
    assert torch.allclose(got, ref, atol=2e-5, rtol=1e-4), float((got - ref).abs().max())
