"""Cohere routing without a GPU: what the routing rests on is read from the installed modeling_cohere.py; the two source guards take
the installed CohereDecoderLayer / CohereAttention and decline copies with one statement edited or one added; the installers take a
tiny CohereForCausalLM - "dalm_sdpa", packable, the layer, norm, attention and MLP forwards bound by name, the counts - and leave head
width 96 alone; a module with `use_qk_norm` is patched and runs transformers' own forward; the patched model is transformers' own on CPU
tensors (bit for bit, LoRA gradients included) and every kernel predicate says no there; the packed decoder run equals the padded one;
and the loss of a step whose hidden states meet `lm_head.weight` without the model's forward (fuse_lm_head, the packed route) carries
`logit_scale`."""
import copy
import warnings

import pytest
import torch

from dalm_amd import packed

from helpers import norm_rel_err
from test_packed_cpu import _masks

V = 128


def _config(**over):
    from transformers import CohereConfig

    kw = dict(vocab_size=V, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
              num_key_value_heads=1, max_position_embeddings=64, logit_scale=0.0625, pad_token_id=0, bos_token_id=None, eos_token_id=2)
    kw.update(over)
    return CohereConfig(**kw)


def _tiny_cohere(**over):
    from transformers import CohereForCausalLM

    torch.manual_seed(0)
    model = CohereForCausalLM(_config(**over))
    with torch.no_grad():                    # norm weights away from their initial ones: a dropped or misplaced norm shows
        for name, p in model.named_parameters():
            if name.endswith(("norm.weight", "layernorm.weight")):
                p.add_(0.3 * torch.randn(p.shape, generator=torch.Generator().manual_seed(len(name))))
    return model


def _forward_names(mods):
    return [getattr(getattr(m.forward, "__func__", None), "__name__", "") for m in mods]


def test_cohere_is_what_the_routing_rests_on():
    """Read from the installed transformers: the MLP is Llama's, the norm is a bias-free f32 LayerNorm with one rounding, the rotation
    is interleaved and computed in f32, the logits are multiplied with `logit_scale`."""
    import inspect

    from transformers.models.cohere import modeling_cohere as mc
    from transformers.models.llama import modeling_llama as ml

    assert inspect.getsource(mc.CohereMLP.forward).split() == inspect.getsource(ml.LlamaMLP.forward).split()
    assert "logits * self.logit_scale" in inspect.getsource(mc.CohereForCausalLM.forward)
    assert "repeat_interleave(freqs, 2, dim=-1)" in inspect.getsource(mc.CohereRotaryEmbedding.forward)
    model = _tiny_cohere()
    assert model.logit_scale == 0.0625 and model.lm_head.bias is None
    layer = model.model.layers[0]
    assert layer.self_attn.head_dim == 64 and layer.self_attn.scaling == 64 ** -0.5 and not layer.self_attn.use_qk_norm
    assert not hasattr(layer, "post_attention_layernorm")
    g = torch.Generator().manual_seed(0)
    # the norm: F.layer_norm in f32, one rounding (bf16 rows, D = 128)
    ln = mc.CohereLayerNorm(128, eps=1e-5)
    with torch.no_grad():
        ln.weight.copy_(1.0 + 0.5 * torch.randn(128, generator=g))
    x = (0.3 + 1.5 * torch.randn(7, 128, generator=g)).bfloat16()
    want = torch.nn.functional.layer_norm(x.float(), (128,), ln.weight.detach().float(), None, 1e-5).bfloat16()
    assert float((ln(x).detach().float() - want.float()).abs().max()) <= 2.0 ** -7 * float(want.float().abs().max())
    # the rotation: pairs (2i, 2i + 1), f32 products and sum, one rounding - and its autograd backward, bit for bit
    for dtype, tab in ((torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32), (torch.float32, torch.float32)):
        q = torch.randn(2, 3, 5, 32, generator=g).to(dtype).requires_grad_(True)
        k = torch.randn(2, 1, 5, 32, generator=g).to(dtype).requires_grad_(True)
        cos, sin = torch.rand(2, 5, 32, generator=g).to(tab), torch.rand(2, 5, 32, generator=g).to(tab) - 0.5
        qe, ke = mc.apply_rotary_pos_emb(q, k, cos, sin)
        gq, gk = torch.randn(qe.shape, generator=g).to(dtype), torch.randn(ke.shape, generator=g).to(dtype)
        torch.autograd.backward([qe, ke], [gq, gk])
        for x, out, gr in ((q, qe, gq), (k, ke, gk)):
            xf, c, s, gf = x.detach().float(), cos.float().unsqueeze(1), sin.float().unsqueeze(1), gr.float()
            fwd, bwd = torch.empty_like(xf), torch.empty_like(xf)
            fwd[..., 0::2] = xf[..., 0::2] * c[..., 0::2] - xf[..., 1::2] * s[..., 0::2]
            fwd[..., 1::2] = xf[..., 1::2] * c[..., 1::2] + xf[..., 0::2] * s[..., 1::2]
            bwd[..., 0::2] = gf[..., 0::2] * c[..., 0::2] + gf[..., 1::2] * s[..., 1::2]
            bwd[..., 1::2] = gf[..., 1::2] * c[..., 1::2] - gf[..., 0::2] * s[..., 0::2]
            assert torch.equal(out.detach(), fwd.to(dtype)) and torch.equal(x.grad, bwd.to(dtype)), (dtype, tab)
    # eager's residual + attn + mlp is (a + b) + c, two roundings
    a, b, c = (torch.randn(64, 128, generator=g).bfloat16() for _ in range(3))
    assert torch.equal(a + b + c, (a + b) + c)
    assert not torch.equal(a + b + c, (a.float() + b.float() + c.float()).bfloat16())


def test_source_guards_take_the_installed_classes_and_decline_edited_copies():
    from transformers.models.cohere import modeling_cohere as mc
    from transformers.models.cohere.modeling_cohere import ALL_ATTENTION_FUNCTIONS, apply_rotary_pos_emb, eager_attention_forward

    from dalm_amd.models import attention, fastpath

    assert fastpath._matches("cohere-layer", mc.CohereDecoderLayer)
    assert fastpath._matches("cohere-attn", mc.CohereAttention)

    class Same(mc.CohereDecoderLayer):                       # the class's own statements, laid out differently, no docstring: taken
        def forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_values=None, use_cache=False,
                    position_embeddings=None, **kwargs):
            residual = hidden_states
            hidden_states = self.input_layernorm(hidden_states)
            hidden_states_attention, _ = self.self_attn(hidden_states=hidden_states, attention_mask=attention_mask,
                                                        position_ids=position_ids, past_key_values=past_key_values,
                                                        use_cache=use_cache, position_embeddings=position_embeddings, **kwargs)
            hidden_states_mlp = self.mlp(hidden_states)
            hidden_states = residual + hidden_states_attention + hidden_states_mlp
            return hidden_states

    class Edited(mc.CohereDecoderLayer):                     # ONE statement changed: the MLP reads the residual stream
        def forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_values=None, use_cache=False,
                    position_embeddings=None, **kwargs):
            """A docstring, as the class's own forward has one."""
            residual = hidden_states
            hidden_states = self.input_layernorm(hidden_states)
            hidden_states_attention, _ = self.self_attn(hidden_states=hidden_states, attention_mask=attention_mask,
                                                        position_ids=position_ids, past_key_values=past_key_values,
                                                        use_cache=use_cache, position_embeddings=position_embeddings, **kwargs)
            hidden_states_mlp = self.mlp(residual)
            hidden_states = residual + hidden_states_attention + hidden_states_mlp
            return hidden_states

    class Added(mc.CohereDecoderLayer):                      # the right statements and one more
        def forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_values=None, use_cache=False,
                    position_embeddings=None, **kwargs):
            """A docstring."""
            residual = hidden_states
            hidden_states = self.input_layernorm(hidden_states)
            hidden_states_attention, _ = self.self_attn(hidden_states=hidden_states, attention_mask=attention_mask,
                                                        position_ids=position_ids, past_key_values=past_key_values,
                                                        use_cache=use_cache, position_embeddings=position_embeddings, **kwargs)
            hidden_states_mlp = self.mlp(hidden_states)
            hidden_states_mlp = hidden_states_mlp * 0.5
            hidden_states = residual + hidden_states_attention + hidden_states_mlp
            return hidden_states

    class SameAttn(mc.CohereAttention):
        def forward(self, hidden_states, position_embeddings, attention_mask, past_key_values=None, **kwargs):
            input_shape = hidden_states.shape[:-1]
            hidden_shape = (*input_shape, -1, self.head_dim)
            query_states = self.q_proj(hidden_states).view(hidden_shape)
            key_states = self.k_proj(hidden_states).view(hidden_shape)
            value_states = self.v_proj(hidden_states).view(hidden_shape)
            if self.use_qk_norm:
                query_states = self.q_norm(query_states)
                key_states = self.k_norm(key_states)
            query_states = query_states.transpose(1, 2)
            key_states = key_states.transpose(1, 2)
            value_states = value_states.transpose(1, 2)
            cos, sin = position_embeddings
            query_states, key_states = apply_rotary_pos_emb(query_states, key_states, cos, sin)
            if past_key_values is not None:
                key_states, value_states = past_key_values.update(key_states, value_states, self.layer_idx)
            attention_interface: Callable = ALL_ATTENTION_FUNCTIONS.get_interface(  # noqa: F821
                self.config._attn_implementation, eager_attention_forward)
            attn_output, attn_weights = attention_interface(
                self, query_states, key_states, value_states, attention_mask,
                dropout=0.0 if not self.training else self.attention_dropout, scaling=self.scaling, **kwargs)
            attn_output = attn_output.reshape(*input_shape, -1).contiguous()
            attn_output = self.o_proj(attn_output)
            return attn_output, attn_weights

    class EditedAttn(mc.CohereAttention):                    # ONE statement changed: the rotation takes sin and cos the other way round
        def forward(self, hidden_states, position_embeddings, attention_mask, past_key_values=None, **kwargs):
            input_shape = hidden_states.shape[:-1]
            hidden_shape = (*input_shape, -1, self.head_dim)
            query_states = self.q_proj(hidden_states).view(hidden_shape)
            key_states = self.k_proj(hidden_states).view(hidden_shape)
            value_states = self.v_proj(hidden_states).view(hidden_shape)
            if self.use_qk_norm:
                query_states = self.q_norm(query_states)
                key_states = self.k_norm(key_states)
            query_states = query_states.transpose(1, 2)
            key_states = key_states.transpose(1, 2)
            value_states = value_states.transpose(1, 2)
            cos, sin = position_embeddings
            query_states, key_states = apply_rotary_pos_emb(query_states, key_states, sin, cos)
            if past_key_values is not None:
                key_states, value_states = past_key_values.update(key_states, value_states, self.layer_idx)
            attention_interface: Callable = ALL_ATTENTION_FUNCTIONS.get_interface(  # noqa: F821
                self.config._attn_implementation, eager_attention_forward)
            attn_output, attn_weights = attention_interface(
                self, query_states, key_states, value_states, attention_mask,
                dropout=0.0 if not self.training else self.attention_dropout, scaling=self.scaling, **kwargs)
            attn_output = attn_output.reshape(*input_shape, -1).contiguous()
            attn_output = self.o_proj(attn_output)
            return attn_output, attn_weights

    class AddedAttn(mc.CohereAttention):                     # the right statements and one more: the keys scaled
        def forward(self, hidden_states, position_embeddings, attention_mask, past_key_values=None, **kwargs):
            input_shape = hidden_states.shape[:-1]
            hidden_shape = (*input_shape, -1, self.head_dim)
            query_states = self.q_proj(hidden_states).view(hidden_shape)
            key_states = self.k_proj(hidden_states).view(hidden_shape)
            value_states = self.v_proj(hidden_states).view(hidden_shape)
            if self.use_qk_norm:
                query_states = self.q_norm(query_states)
                key_states = self.k_norm(key_states)
            query_states = query_states.transpose(1, 2)
            key_states = key_states.transpose(1, 2)
            value_states = value_states.transpose(1, 2)
            cos, sin = position_embeddings
            query_states, key_states = apply_rotary_pos_emb(query_states, key_states, cos, sin)
            key_states = key_states * 2.0
            if past_key_values is not None:
                key_states, value_states = past_key_values.update(key_states, value_states, self.layer_idx)
            attention_interface: Callable = ALL_ATTENTION_FUNCTIONS.get_interface(  # noqa: F821
                self.config._attn_implementation, eager_attention_forward)
            attn_output, attn_weights = attention_interface(
                self, query_states, key_states, value_states, attention_mask,
                dropout=0.0 if not self.training else self.attention_dropout, scaling=self.scaling, **kwargs)
            attn_output = attn_output.reshape(*input_shape, -1).contiguous()
            attn_output = self.o_proj(attn_output)
            return attn_output, attn_weights

    assert fastpath._matches("cohere-layer", Same)
    assert fastpath._matches("cohere-attn", SameAttn)
    for key, cls in (("cohere-layer", Edited), ("cohere-layer", Added), ("cohere-attn", EditedAttn), ("cohere-attn", AddedAttn)):
        with pytest.warns(UserWarning, match="not the code this patch restates"):
            assert not fastpath._matches(key, cls), cls.__name__
    # Llama's classes are not Cohere's, and Cohere's are not Llama's
    from transformers.models.llama import modeling_llama as ml

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert not fastpath._matches("cohere-layer", ml.LlamaDecoderLayer)
        assert not fastpath._matches("cohere-attn", ml.LlamaAttention)
        assert not fastpath._matches("llama-attn", mc.CohereAttention)
        assert not fastpath._matches("qwen3-layer", mc.CohereDecoderLayer)

    # installed on a model: the edited modules keep their forwards
    class CohereLayerNorm(mc.CohereLayerNorm):               # same name, another formula (no mean): the value probe says no
        def forward(self, hidden_states):
            x = hidden_states.float()
            x = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + self.variance_epsilon)
            return (self.weight.float() * x).to(hidden_states.dtype)

    Edited.__name__ = "CohereDecoderLayer"
    EditedAttn.__name__ = "CohereAttention"
    model = _tiny_cohere()
    layers = model.model.layers
    layers[1].__class__ = Edited
    layers[0].self_attn.__class__ = EditedAttn
    model.model.norm.__class__ = CohereLayerNorm
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert attention.use_hip_attention_backward(model)
        assert fastpath.use_cohere_layer(model) == 1
        assert fastpath.use_cohere_layer_norm(model) == 1      # the edited layer's input_layernorm; not the edited final norm
        assert fastpath.use_cohere_attention_node(model) == 1
    assert _forward_names(layers) == ["_cohere_layer_forward", "forward"]
    assert [hasattr(l, "_dalm_orig_forward") for l in layers] == [True, False]
    assert _forward_names(l.self_attn for l in layers) == ["forward", "_cohere_attention_forward"]
    assert _forward_names([model.model.norm, layers[0].input_layernorm, layers[1].input_layernorm]) == \
        ["forward", "forward", "_cohere_norm_forward"]


def test_installers_take_a_cohere_model_and_bind_the_forwards():
    """Fails on a tree without the Cohere routing: there no installer takes anything of this model and it stays on "sdpa"."""
    from dalm_amd.models import attention, fastpath
    from dalm_amd.models.rag_e2e_base_model import _GENERATOR_PATHS, _RETRIEVER_PATHS, DECODER_ONLY_TYPES, use_generator_fast_paths

    model = _tiny_cohere()
    assert model.config._attn_implementation == "sdpa" and not packed.attention_is_packable(model)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                    # no guard refuses anything of the installed classes
        got = use_generator_fast_paths(model)
    assert model.config._attn_implementation == attention.NAME == "dalm_sdpa" and packed.attention_is_packable(model)
    assert got["use_hip_attention_backward"] is True
    assert got["use_cohere_layer"] == 2 and got["use_cohere_layer_norm"] == 1 and got["use_cohere_attention_node"] == 2
    assert got["use_swiglu_kernel"] == 0                                  # CohereMLP: only where the caller asks (`cohere=True`)
    assert got["use_native_rms_norm"] == 0 and got["use_fused_residual_norm"] == 0 and got["use_roll_rope"] is False
    assert got["use_llama_attention_node"] == 0 and got["use_qwen3_attention_node"] == 0 and got["use_olmo2_attention_node"] == 0
    layers = model.model.layers
    assert _forward_names(layers) == ["_cohere_layer_forward"] * 2 and all(hasattr(l, "_dalm_orig_forward") for l in layers)
    assert _forward_names(l.self_attn for l in layers) == ["_cohere_attention_forward"] * 2
    assert all(hasattr(l.self_attn, "_dalm_orig_attn_forward") for l in layers)
    assert _forward_names(l.mlp for l in layers) == ["forward"] * 2
    assert fastpath.use_swiglu_kernel(model, cohere=True) == 2 and _forward_names(l.mlp for l in layers) == ["_swiglu_mlp_forward"] * 2
    assert _forward_names([model.model.norm] + [l.input_layernorm for l in layers]) == ["_cohere_norm_forward", "forward", "forward"]
    order = list(_GENERATOR_PATHS)
    assert order.index(fastpath.use_cohere_attention_node) > order.index(attention.use_hip_attention_backward)
    assert order.index(fastpath.use_cohere_layer_norm) > order.index(fastpath.use_cohere_layer)
    for use in (fastpath.use_cohere_layer, fastpath.use_cohere_layer_norm, fastpath.use_cohere_attention_node):
        assert use not in _RETRIEVER_PATHS
    assert "cohere" not in DECODER_ONLY_TYPES                             # a generator only
    assert _forward_names([model, model.model]) == ["forward", "forward"]  # `logit_scale` stays CohereForCausalLM.forward's statement
    # a model that stays on "sdpa" gets no attention node
    assert fastpath.use_cohere_attention_node(_tiny_cohere()) == 0


def test_other_head_widths_keep_sdpa_and_do_not_pack():
    from dalm_amd.models import attention
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    wide = _tiny_cohere(hidden_size=192)                                  # 2 heads of width 96
    assert wide.model.layers[0].self_attn.head_dim == 96
    got = use_generator_fast_paths(wide)
    assert got["use_hip_attention_backward"] is False and got["use_cohere_attention_node"] == 0
    assert wide.config._attn_implementation == "sdpa" and not packed.attention_is_packable(wide)
    assert got["use_cohere_layer"] == 2 and got["use_cohere_layer_norm"] == 1                  # the row-wise routes do not care
    for hidden, ok in ((64, True), (256, True), (32, False)):             # widths 32 and 128 are taken, 16 is not
        m = _tiny_cohere(hidden_size=hidden)
        assert attention.use_hip_attention_backward(m) is ok and packed.attention_is_packable(m) is ok


@pytest.mark.parametrize("switch", ["DALM_NORM_KERNEL", "DALM_SWIGLU_KERNEL", "DALM_ATTN_KERNEL"])
def test_the_reference_switches_turn_the_installers_off(monkeypatch, switch):
    from dalm_amd.models import fastpath
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    monkeypatch.setenv(switch, "0")
    model = _tiny_cohere()
    got = use_generator_fast_paths(model)
    got["use_swiglu_kernel"] = fastpath.use_swiglu_kernel(model, cohere=True)     # the MLP route is asked for: its reference switch wins
    layers = model.model.layers
    norm_on, mlp_on, attn_on = (switch != s for s in ("DALM_NORM_KERNEL", "DALM_SWIGLU_KERNEL", "DALM_ATTN_KERNEL"))
    assert got["use_cohere_layer"] == (2 if norm_on else 0) and got["use_cohere_layer_norm"] == (1 if norm_on else 0)
    assert got["use_swiglu_kernel"] == (2 if mlp_on else 0)
    assert got["use_hip_attention_backward"] is attn_on and got["use_cohere_attention_node"] == (2 if attn_on else 0)
    assert _forward_names(layers) == ["_cohere_layer_forward" if norm_on else "forward"] * 2
    assert _forward_names([model.model.norm]) == ["_cohere_norm_forward" if norm_on else "forward"]
    assert _forward_names(l.mlp for l in layers) == ["_swiglu_mlp_forward" if mlp_on else "forward"] * 2
    assert _forward_names(l.self_attn for l in layers) == ["_cohere_attention_forward" if attn_on else "forward"] * 2
    assert packed.attention_is_packable(model) is attn_on


def _spy_on_own_forward(attn):
    seen, own = [], attn._dalm_orig_attn_forward
    attn._dalm_orig_attn_forward = lambda *a, **k: (seen.append(1), own(*a, **k))[1]
    return seen


def test_what_the_attention_node_declines_runs_transformers_own_forward():
    from dalm_amd.models import fastpath
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    ids = torch.randint(3, V, (2, 8), generator=torch.Generator().manual_seed(1))
    # use_qk_norm (Command-R+): the patch is installed, its forward reaches the class's own; the [H, hd] norms are left alone
    qk = _tiny_cohere(use_qk_norm=True)
    ref = copy.deepcopy(qk)
    got = use_generator_fast_paths(qk)
    assert got["use_cohere_attention_node"] == 2 and got["use_cohere_layer"] == 2 and got["use_cohere_layer_norm"] == 1
    assert qk.config._attn_implementation == "dalm_sdpa"
    attn = qk.model.layers[0].self_attn
    assert _forward_names([attn, attn.q_norm, attn.k_norm]) == ["_cohere_attention_forward", "forward", "forward"]
    assert tuple(attn.q_norm.weight.shape) == (2, 64)
    seen = _spy_on_own_forward(attn)
    with torch.no_grad():
        assert torch.equal(qk(input_ids=ids, use_cache=False).logits, ref(input_ids=ids, use_cache=False).logits)
    assert seen == [1]
    # biased projections: installed as well, declined at call time
    biased = _tiny_cohere(attention_bias=True)
    assert use_generator_fast_paths(biased)["use_cohere_attention_node"] == 2
    seen = _spy_on_own_forward(biased.model.layers[0].self_attn)
    biased(input_ids=ids, use_cache=False)
    assert seen == [1]
    # attention dropout in a training call, a KV cache
    drop = _tiny_cohere(attention_dropout=0.1)
    assert use_generator_fast_paths(drop)["use_cohere_attention_node"] == 2
    seen = _spy_on_own_forward(drop.model.layers[0].self_attn)
    drop.train()(input_ids=ids, use_cache=False)
    assert seen == [1]
    drop.eval()(input_ids=ids, use_cache=True)
    assert seen == [1, 1]
    # another activation: the MLP keeps its forward
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gelu = _tiny_cohere(hidden_act="gelu")
        assert fastpath.use_swiglu_kernel(gelu) == 0 and _forward_names(l.mlp for l in gelu.model.layers) == ["forward"] * 2


def test_every_kernel_predicate_says_no_on_the_cpu():
    from dalm_amd.models import tower_ops

    x = torch.randn(4, 128)
    w = torch.ones(128)
    q, k = torch.randn(1, 2, 4, 64), torch.randn(1, 1, 4, 64)
    cos = torch.randn(1, 4, 64)
    assert not tower_ops.cohere_norm_supported(x, w)
    assert not tower_ops.add3_live_supported(x, x, x)
    assert not tower_ops.rope_il_supported(q, k, cos, cos)
    assert not tower_ops.scale_add_supported(x)


def _with_lora(m):
    from dalm_amd.models import lora

    torch.manual_seed(3)                                                  # the same adapter initialisation in every copy
    lora.inject_lora(m, ["q_proj", "v_proj"], lora_dropout=0.0)
    with torch.no_grad():                                                 # B away from zero: the A gradients say something
        for name, p in m.named_parameters():
            if "lora_B" in name:
                p.copy_(0.05 * torch.randn(p.shape, generator=torch.Generator().manual_seed(len(name))))
    return m


def test_patched_model_is_transformers_own_on_the_cpu():
    """fp32 on the CPU: every patch falls through to the statements it restates; logits and LoRA gradients are equal bit for bit."""
    from dalm_amd.models import fastpath
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    ref = _tiny_cohere()
    model = copy.deepcopy(ref)
    got = use_generator_fast_paths(model)
    assert got["use_cohere_layer"] == 2 and got["use_cohere_attention_node"] == 2
    assert fastpath.use_swiglu_kernel(model, cohere=True) == 2            # the MLP route, asked for: it falls through as well
    assert _forward_names(l.mlp for l in model.model.layers) == ["_swiglu_mlp_forward"] * 2
    _with_lora(model), _with_lora(ref)
    B, T = 3, 12
    mask = _masks(B, T, True, 4)
    ids = torch.randint(3, V, (B, T), generator=torch.Generator().manual_seed(5))
    w = torch.randn(B, T, V, generator=torch.Generator().manual_seed(6))
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


def test_what_follows_from_the_llama_named_projections():
    """Confirmed, not assumed: the one-GEMM q | k | v group, its LoRA kernels and the transposed dgrad key on the projections' names,
    which are Llama's."""
    from dalm_amd.models import lora
    from dalm_amd.models.frozen_linear import FrozenLinearT, use_transposed_dgrad
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    model = _tiny_cohere()
    use_generator_fast_paths(model)
    lora.inject_lora(model, ["q_proj", "v_proj"], lora_dropout=0.0)
    assert use_transposed_dgrad(model) >= 2 * 4                           # o_proj, gate_proj, up_proj, down_proj per layer
    for layer in model.model.layers:
        a = layer.self_attn
        assert isinstance(a.q_proj, lora.LoRALinear) and isinstance(a.v_proj, lora.LoRALinear)
        assert a.q_proj._group is not None and a.q_proj._group is a.k_proj._group is a.v_proj._group
        assert len(a.q_proj._group.members) == 3
        assert type(a.o_proj) is FrozenLinearT and type(layer.mlp.down_proj) is FrozenLinearT
        assert type(layer.mlp.gate_proj) is FrozenLinearT and type(layer.mlp.up_proj) is FrozenLinearT
    trainable = [n for n, p in model.named_parameters() if p.requires_grad]
    assert trainable and all("lora_" in n for n in trainable)


@pytest.mark.parametrize("left", [True, False])
def test_packed_decoder_run_equals_the_padded_run(left):
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    model = _tiny_cohere().eval()
    B, T = 4, 16
    mask = _masks(B, T, left, 1)
    ids = torch.randint(3, V, (B, T), generator=torch.Generator().manual_seed(2))
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


# ---- logit_scale ---------------------------------------------------------------------------------------------------------
def _left_mask(lens, T):
    return (torch.arange(T).unsqueeze(0) >= (T - torch.tensor(lens)).unsqueeze(1)).long()


def _loss_and_grads(route: str, scale: float = 0.0625):
    """`RagE2EStep._generator` + `RagE2EStep._loss` on the CPU (fp32, the oracle's ops in place of the HIP loss kernels), with given
    retriever embeddings: the generator half of one step.  route: "logits" (the model's own forward), "hidden" (fuse_lm_head) or
    "packed".  Returns the loss and the gradients of the LoRA parameters and of the two embedding matrices."""
    from oracle.dalm_oracle import OracleOps

    from dalm_amd.models import AutoModelForRagE2E
    from dalm_amd.training.step import RagE2EStep
    from transformers import BertConfig, BertModel

    torch.manual_seed(5)
    bert = BertModel(BertConfig(hidden_size=32, num_hidden_layers=1, num_attention_heads=2, intermediate_size=64, vocab_size=128,
                                max_position_embeddings=32))
    gen = _with_lora(_tiny_cohere(logit_scale=scale))
    model = AutoModelForRagE2E.from_modules(bert, gen, None, None, normalize=True, get_peft=None, retriever_is_autoregressive=False)
    model.train()
    named = [(n, p) for n, p in model.generator_model.named_parameters() if p.requires_grad]
    assert named and all("lora_" in n for n, _ in named)
    opt = torch.optim.SGD([p for _, p in named], lr=0.0)
    step = RagE2EStep(model, opt, None, 100, ops=OracleOps(), fuse_lm_head=route == "hidden", overlap_towers=False)
    B, T, D = 6, 24, 32
    g = torch.Generator().manual_seed(22)
    batch = {"generator_input_input_ids": torch.randint(3, V, (B, T), generator=g),
             "generator_input_attention_mask": _left_mask([24, 10, 17, 5, 21, 13], T),
             "query_passage_input_len": torch.tensor([14, 6, 9, 2, 11, 7])}
    if route == "packed":
        batch = packed.add_pack_plans(batch, packed.RAG_GROUPS[:1], multiple=8)
        assert "generator_pack_rows" in batch
    q = torch.nn.functional.normalize(torch.randn(B, D, generator=g), dim=1).requires_grad_(True)
    p = torch.nn.functional.normalize(torch.randn(B, D, generator=g), dim=1).requires_grad_(True)
    is_packed = step._packed_generator(batch)
    assert is_packed == (route == "packed")
    out = step._generator(batch, None, is_packed)
    assert out.shape[-1] == 128                                           # logits and hidden states are both 128 wide here
    loss = step._loss(batch, is_packed, out, p, q, None, None)
    loss.backward()
    grads = {n: t.grad.detach().clone() for n, t in named}
    grads["q_emb"], grads["p_emb"] = q.grad.detach().clone(), p.grad.detach().clone()
    return float(loss.detach()), grads


@pytest.mark.parametrize("route", ["hidden", "packed"])
def test_logit_scale_reaches_the_loss_without_the_models_forward(route):
    """The loss from the hidden states against the loss from the model's own logits (which CohereForCausalLM.forward multiplies with
    logit_scale = 0.0625), within the fp32 bound tests/test_packed_gpu.py holds the step to: 1e-4 relative, for the loss and, by
    norm, for every gradient.  0.0625 is a power of two: the scaling adds no error of its own.  Fails on a tree that does not scale:
    there the logits of these routes are 16 x too large."""
    want, g_want = _loss_and_grads("logits")
    got, g_got = _loss_and_grads(route)
    print(f"{route}: loss {got:.8f} against {want:.8f}")
    assert abs(got - want) <= 1e-4 * abs(want), (got, want)
    assert set(g_got) == set(g_want)
    for n in sorted(g_want):
        assert float(g_want[n].abs().max()) > 0.0, n
        err = norm_rel_err(g_got[n], g_want[n])
        print(f"{route}: {n} {err:.3e}")
        assert err <= 1e-4, (n, err)


def test_a_unit_logit_scale_changes_nothing_and_both_factors_compose():
    from dalm_amd.training.step import _logits_scaled

    h = torch.randn(3, 5, 16)
    assert _logits_scaled(h, _tiny_cohere(logit_scale=1.0)) is h
    assert torch.equal(_logits_scaled(h, _tiny_cohere(logit_scale=0.0625)), h * 0.0625)
    assert torch.equal(_logits_scaled(h, _tiny_cohere(logit_scale=0.25)), h * 0.25)
