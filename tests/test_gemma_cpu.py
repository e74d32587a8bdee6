"""Gemma routing without a GPU: the installers take a tiny GemmaForCausalLM and bind the new forwards, the patched model is
transformers' own on CPU tensors (logits and gradients), changed code is declined, a Llama model is left as it was, and
"dalm_sdpa" follows the head width."""
import copy
import warnings

import torch

from dalm_amd import packed

from test_packed_cpu import _masks


def _config(**over):
    from transformers import GemmaConfig

    kw = dict(vocab_size=128, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
              num_key_value_heads=1, head_dim=16)
    kw.update(over)
    return GemmaConfig(**kw)


def _tiny_gemma(**over):
    from transformers import GemmaForCausalLM

    torch.manual_seed(0)
    model = GemmaForCausalLM(_config(**over))
    with torch.no_grad():                    # norm weights away from their zero initialisation: a dropped "1 +" shows
        for name, p in model.named_parameters():
            if name.endswith("norm.weight"):
                p.add_(0.3 * torch.randn(p.shape, generator=torch.Generator().manual_seed(len(name))))
    return model


def _forward_names(mods):
    return [getattr(getattr(m.forward, "__func__", None), "__name__", "") for m in mods]


def test_installers_take_a_gemma_model_and_bind_the_new_forwards():
    from dalm_amd.models import fastpath
    from dalm_amd.models.rag_e2e_base_model import _ROW_WISE_PATHS, use_generator_fast_paths

    model = _tiny_gemma()
    assert type(model.model.layers[0].mlp.act_fn).__name__ == "GELUTanh"
    assert fastpath.use_geglu_kernel(model) == 2
    assert fastpath.use_gemma_rms_norm(model) == 5                       # two per layer and the final one
    assert fastpath.use_fused_residual_norm(model) == 2
    assert fastpath.use_swiglu_kernel(model) == 0 and fastpath.use_native_rms_norm(model) == 0
    layers = model.model.layers
    assert _forward_names(l.mlp for l in layers) == ["_geglu_mlp_forward"] * 2
    assert _forward_names(layers) == ["_gemma_layer_forward"] * 2 and all(hasattr(l, "_dalm_orig_forward") for l in layers)
    assert _forward_names([model.model.norm, layers[0].input_layernorm, layers[1].post_attention_layernorm]) == ["_gemma_norm_forward"] * 3
    assert {fastpath.use_geglu_kernel, fastpath.use_gemma_rms_norm, fastpath.use_fused_residual_norm} <= set(_ROW_WISE_PATHS)
    got = use_generator_fast_paths(_tiny_gemma())
    assert got["use_geglu_kernel"] == 2 and got["use_gemma_rms_norm"] == 5 and got["use_fused_residual_norm"] == 2
    assert got["use_llama_attention_node"] == 0 and got["use_qwen3_attention_node"] == 0


def test_the_reference_switches_turn_the_installers_off(monkeypatch):
    from dalm_amd.models import fastpath

    monkeypatch.setenv("DALM_SWIGLU_KERNEL", "0")
    monkeypatch.setenv("DALM_NORM_KERNEL", "0")
    model = _tiny_gemma()
    assert fastpath.use_geglu_kernel(model) == 0 and fastpath.use_gemma_rms_norm(model) == 0
    assert fastpath.use_fused_residual_norm(model) == 0
    assert _forward_names(model.model.layers) == ["forward"] * 2


def test_patched_model_is_transformers_own_on_the_cpu():
    """fp32 on the CPU: every patch falls through to the statements it restates, logits and gradients are equal."""
    from dalm_amd.models import fastpath

    ref = _tiny_gemma()
    model = copy.deepcopy(ref)
    assert fastpath.use_geglu_kernel(model) == 2 and fastpath.use_gemma_rms_norm(model) == 5
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
    # the norm weights did not move (the value probe runs on a twin of the module)
    for (n, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        assert torch.equal(p, q), n


def test_changed_code_is_declined_and_left_in_place():
    from transformers.models.gemma import modeling_gemma as mg

    from dalm_amd.models import fastpath

    class GemmaMLP(mg.GemmaMLP):                               # same name, an edited forward
        def forward(self, x):
            return self.down_proj(self.act_fn(self.gate_proj(x)) * self.up_proj(x)) * 0.5

    class GemmaRMSNorm(mg.GemmaRMSNorm):                       # same name, Llama's formula: w, not 1 + w
        def forward(self, x):
            output = self._norm(x.float())
            return (output * self.weight.float()).type_as(x)

    class GemmaDecoderLayer(mg.GemmaDecoderLayer):             # the whole body with ONE statement changed (the last add)
        def forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_values=None, use_cache=False,
                    position_embeddings=None, **kwargs):
            residual = hidden_states
            hidden_states = self.input_layernorm(hidden_states)
            hidden_states, _ = self.self_attn(
                hidden_states=hidden_states,
                attention_mask=attention_mask,
                position_ids=position_ids,
                past_key_values=past_key_values,
                use_cache=use_cache,
                position_embeddings=position_embeddings,
                **kwargs,
            )
            hidden_states = residual + hidden_states
            residual = hidden_states
            hidden_states = self.post_attention_layernorm(hidden_states)
            hidden_states = self.mlp(hidden_states)
            hidden_states = hidden_states + residual
            return hidden_states

    model = _tiny_gemma()
    layers = model.model.layers
    layers[0].mlp.__class__ = GemmaMLP
    model.model.norm.__class__ = GemmaRMSNorm
    layers[1].__class__ = GemmaDecoderLayer
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert fastpath.use_geglu_kernel(model) == 1
        assert fastpath.use_gemma_rms_norm(model) == 4
        assert fastpath.use_fused_residual_norm(model) == 1
    assert _forward_names(l.mlp for l in layers) == ["forward", "_geglu_mlp_forward"]
    assert _forward_names([model.model.norm, layers[0].input_layernorm]) == ["forward", "_gemma_norm_forward"]
    assert _forward_names(layers) == ["_gemma_layer_forward", "forward"]
    assert [hasattr(l, "_dalm_orig_forward") for l in layers] == [True, False]

    # a layer one of whose norms has the other formula keeps transformers' forward too
    model = _tiny_gemma()
    model.model.layers[0].post_attention_layernorm.__class__ = GemmaRMSNorm
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert fastpath.use_fused_residual_norm(model) == 1
    assert _forward_names(model.model.layers) == ["forward", "_gemma_layer_forward"]

    # another activation under the same class: not tanh-GELU, not taken
    assert fastpath.use_geglu_kernel(_tiny_gemma(hidden_act="gelu")) == 0
    assert fastpath.use_geglu_kernel(_tiny_gemma(hidden_act="silu")) == 0


def test_a_llama_model_is_left_as_it_was():
    from transformers import LlamaConfig, LlamaForCausalLM

    from dalm_amd.models import fastpath

    torch.manual_seed(0)
    model = LlamaForCausalLM(LlamaConfig(vocab_size=128, hidden_size=64, intermediate_size=128, num_hidden_layers=2,
                                         num_attention_heads=4, num_key_value_heads=2))
    assert fastpath.use_geglu_kernel(model) == 0 and fastpath.use_gemma_rms_norm(model) == 0
    assert fastpath.use_native_rms_norm(model) == 5 and fastpath.use_swiglu_kernel(model) == 2
    assert fastpath.use_fused_residual_norm(model) == 2
    assert _forward_names(model.model.layers) == ["_llama_layer_forward"] * 2
    assert _forward_names(l.mlp for l in model.model.layers) == ["_swiglu_mlp_forward"] * 2


def test_dalm_sdpa_follows_the_head_width():
    from transformers import GemmaForCausalLM

    from dalm_amd.models import attention
    from dalm_amd.models.rag_e2e_base_model import DECODER_ONLY_TYPES

    narrow = GemmaForCausalLM(_config(hidden_size=128, num_attention_heads=2, head_dim=64))
    assert narrow.config._attn_implementation == "sdpa" and not packed.attention_is_packable(narrow)
    assert attention.use_hip_attention_backward(narrow)
    assert narrow.config._attn_implementation == attention.NAME and packed.attention_is_packable(narrow)
    wide = GemmaForCausalLM(_config(hidden_size=128, num_attention_heads=2, head_dim=256))      # every released checkpoint's width
    assert not attention.use_hip_attention_backward(wide)
    assert wide.config._attn_implementation == "sdpa" and not packed.attention_is_packable(wide)
    assert "gemma" not in DECODER_ONLY_TYPES
