"""Phi-3 / Phi-4 routing without a GPU: what the routing rests on is read from the installed modeling_phi3.py; the three source
guards take the installed Phi3DecoderLayer / Phi3Attention / Phi3MLP and decline copies with one statement edited; the installers take
tiny Phi3ForCausalLM models of head width 64 and 128 - "dalm_sdpa", packable, the three forwards bound by name, the counts - and leave
width 96 on "sdpa" with the row-wise routes only; LoRA's q_proj / v_proj targets resolve to qkv_proj and the adapter survives save,
load and merge; the patched model is transformers' own on CPU tensors (bit for bit, LoRA gradients included) with partial, full and
longrope tables; residual dropout in a training call runs transformers' own layer forward."""
import copy
import json
import warnings

import pytest
import torch

from dalm_amd import packed

from test_packed_cpu import _masks

V = 128


def _config(hidden=256, heads=4, kv=2, factor=0.75, rope=None, **over):
    from transformers import Phi3Config

    rope_parameters = {"rope_type": "default", "rope_theta": 10000.0, "partial_rotary_factor": factor}
    rope_parameters.update(rope or {})
    kw = dict(vocab_size=V, hidden_size=hidden, intermediate_size=2 * hidden, num_hidden_layers=2, num_attention_heads=heads,
              num_key_value_heads=kv, max_position_embeddings=64, pad_token_id=0, bos_token_id=1, eos_token_id=2,
              rope_parameters=rope_parameters)
    kw.update(over)
    return Phi3Config(**kw)


def _tiny_phi3(**over):
    from transformers import Phi3ForCausalLM

    torch.manual_seed(0)
    model = Phi3ForCausalLM(_config(**over))
    with torch.no_grad():                    # norm weights away from their initial ones: a dropped or misplaced norm shows
        for name, p in model.named_parameters():
            if name.endswith(("norm.weight", "layernorm.weight")):
                p.add_(0.3 * torch.randn(p.shape, generator=torch.Generator().manual_seed(len(name))))
    return model


# (keyword arguments, head width, rotary width)
WIDTH_64_PARTIAL = (dict(hidden=256, heads=4, kv=2, factor=0.75), 64, 48)
WIDTH_64_FULL = (dict(hidden=256, heads=4, kv=2, factor=1.0), 64, 64)
WIDTH_128 = (dict(hidden=512, heads=4, kv=2, factor=0.75), 128, 96)
WIDTH_96 = (dict(hidden=384, heads=4, kv=4, factor=1.0), 96, 96)


def _longrope(rot=48):
    half = rot // 2
    return dict(rope={"rope_type": "longrope", "short_factor": [1.0 + 0.01 * i for i in range(half)],
                      "long_factor": [1.5 + 0.05 * i for i in range(half)], "original_max_position_embeddings": 64},
                max_position_embeddings=256)


def _forward_names(mods):
    return [getattr(getattr(m.forward, "__func__", None), "__name__", "") for m in mods]


def test_phi3_is_what_the_routing_rests_on():
    """Read from the installed transformers: the tables are as wide as the rotated part and arrive in the activations' dtype, the
    rotation pairs i with i + rot/2 inside that part and copies the rest, the norm is Llama's, every default dropout is 0."""
    import inspect

    from transformers.models.llama import modeling_llama as ml
    from transformers.models.phi3 import modeling_phi3 as mp

    assert inspect.getsource(mp.Phi3RMSNorm.forward).split() == inspect.getsource(ml.LlamaRMSNorm.forward).split()
    assert "cos.to(dtype=x.dtype), sin.to(dtype=x.dtype)" in inspect.getsource(mp.Phi3RotaryEmbedding.forward)
    for (kw, hd, rot) in (WIDTH_64_PARTIAL, WIDTH_64_FULL, WIDTH_128, WIDTH_96):
        model = _tiny_phi3(**kw)
        attn = model.model.layers[0].self_attn
        assert attn.head_dim == hd and attn.scaling == hd ** -0.5 and attn.qkv_proj.bias is None
        cos, sin = model.model.rotary_emb(torch.zeros(1, 5, 8), torch.arange(5).unsqueeze(0))
        assert tuple(cos.shape) == (1, 5, rot) and cos.dtype == torch.float32
    assert model.config.resid_pdrop == 0.0 and model.config.attention_dropout == 0.0 and model.config.sliding_window is None
    g = torch.Generator().manual_seed(0)
    for dtype in (torch.bfloat16, torch.float32):
        q = torch.randn(2, 3, 5, 32, generator=g).to(dtype).requires_grad_(True)
        k = torch.randn(2, 1, 5, 32, generator=g).to(dtype).requires_grad_(True)
        cos, sin = torch.rand(2, 5, 16, generator=g).to(dtype), (torch.rand(2, 5, 16, generator=g) - 0.5).to(dtype)   # distinct halves
        qe, ke = mp.apply_rotary_pos_emb(q, k, cos, sin)
        gq, gk = torch.randn(qe.shape, generator=g).to(dtype), torch.randn(ke.shape, generator=g).to(dtype)
        torch.autograd.backward([qe, ke], [gq, gk])
        rb = lambda t: t.to(dtype).float()  # noqa: E731
        for x, out, gr in ((q, qe, gq), (k, ke, gk)):
            xf, c, s, gf = x.detach().float(), cos.float().unsqueeze(1), sin.float().unsqueeze(1), gr.float()
            x1, x2, c1, c2, s1, s2, g1, g2 = xf[..., :8], xf[..., 8:16], c[..., :8], c[..., 8:], s[..., :8], s[..., 8:], gf[..., :8], \
                gf[..., 8:16]
            fwd = torch.cat((rb(rb(x1 * c1) - rb(x2 * s1)), rb(rb(x2 * c2) + rb(x1 * s2)), xf[..., 16:]), -1)
            bwd = torch.cat((rb(rb(g1 * c1) + rb(g2 * s2)), rb(rb(g2 * c2) - rb(g1 * s1)), gf[..., 16:]), -1)
            assert torch.equal(out.detach(), fwd.to(dtype)) and torch.equal(x.grad, bwd.to(dtype)), dtype
    # up * silu(gate) and silu(gate) * up round identically
    a, b = torch.randn(64, 128, generator=g).bfloat16(), torch.randn(64, 128, generator=g).bfloat16()
    assert torch.equal(a * torch.nn.functional.silu(b), torch.nn.functional.silu(b) * a)


def test_source_guards_take_the_installed_classes_and_decline_edited_copies():
    from transformers.models.phi3 import modeling_phi3 as mp
    from transformers.models.phi3.modeling_phi3 import ALL_ATTENTION_FUNCTIONS, apply_rotary_pos_emb, eager_attention_forward

    from dalm_amd.models import fastpath

    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert fastpath._matches("phi3-layer", mp.Phi3DecoderLayer)
        assert fastpath._matches("phi3-attn", mp.Phi3Attention)
        assert fastpath._matches("phi3-mlp", mp.Phi3MLP)

    class EditedLayer(mp.Phi3DecoderLayer):                  # ONE statement changed: the MLP's dropout on the attention output
        def forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_values=None, use_cache=False,
                    position_embeddings=None, **kwargs):
            residual = hidden_states
            hidden_states = self.input_layernorm(hidden_states)
            hidden_states, self_attn_weights = self.self_attn(
                hidden_states=hidden_states, attention_mask=attention_mask, position_ids=position_ids,
                past_key_values=past_key_values, use_cache=use_cache, position_embeddings=position_embeddings, **kwargs)
            hidden_states = residual + self.resid_mlp_dropout(hidden_states)
            residual = hidden_states
            hidden_states = self.post_attention_layernorm(hidden_states)
            hidden_states = self.mlp(hidden_states)
            hidden_states = residual + self.resid_mlp_dropout(hidden_states)
            return hidden_states

    class SameLayer(mp.Phi3DecoderLayer):                    # the class's own statements, laid out differently: taken
        def forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_values=None, use_cache=False,
                    position_embeddings=None, **kwargs):
            residual = hidden_states
            hidden_states = self.input_layernorm(hidden_states)
            hidden_states, self_attn_weights = self.self_attn(
                hidden_states=hidden_states, attention_mask=attention_mask, position_ids=position_ids,
                past_key_values=past_key_values, use_cache=use_cache, position_embeddings=position_embeddings, **kwargs)
            hidden_states = residual + self.resid_attn_dropout(hidden_states)
            residual = hidden_states
            hidden_states = self.post_attention_layernorm(hidden_states)
            hidden_states = self.mlp(hidden_states)
            hidden_states = residual + self.resid_mlp_dropout(hidden_states)
            return hidden_states

    class EditedAttn(mp.Phi3Attention):                      # ONE statement changed: the keys start one column late
        def forward(self, hidden_states, position_embeddings, attention_mask, past_key_values=None, **kwargs):
            input_shape = hidden_states.shape[:-1]
            hidden_shape = (*input_shape, -1, self.head_dim)
            qkv = self.qkv_proj(hidden_states)
            query_pos = self.config.num_attention_heads * self.head_dim
            query_states = qkv[..., :query_pos]
            key_states = qkv[..., query_pos + 1 : query_pos + self.num_key_value_heads * self.head_dim]
            value_states = qkv[..., query_pos + self.num_key_value_heads * self.head_dim :]
            query_states = query_states.view(hidden_shape).transpose(1, 2)
            key_states = key_states.view(hidden_shape).transpose(1, 2)
            value_states = value_states.view(hidden_shape).transpose(1, 2)
            cos, sin = position_embeddings
            query_states, key_states = apply_rotary_pos_emb(query_states, key_states, cos, sin)
            if past_key_values is not None:
                key_states, value_states = past_key_values.update(key_states, value_states, self.layer_idx)
            attention_interface: Callable = ALL_ATTENTION_FUNCTIONS.get_interface(  # noqa: F821
                self.config._attn_implementation, eager_attention_forward)
            attn_output, attn_weights = attention_interface(
                self, query_states, key_states, value_states, attention_mask,
                dropout=0.0 if not self.training else self.attention_dropout, scaling=self.scaling,
                sliding_window=getattr(self.config, "sliding_window", None), **kwargs)
            attn_output = attn_output.reshape(*input_shape, -1).contiguous()
            attn_output = self.o_proj(attn_output)
            return attn_output, attn_weights

    class EditedMLP(mp.Phi3MLP):                             # ONE statement changed: the activation on the other half
        def forward(self, hidden_states):
            up_states = self.gate_up_proj(hidden_states)
            gate, up_states = up_states.chunk(2, dim=-1)
            up_states = gate * self.activation_fn(up_states)
            return self.down_proj(up_states)

    assert fastpath._matches("phi3-layer", SameLayer)
    for key, cls in (("phi3-layer", EditedLayer), ("phi3-attn", EditedAttn), ("phi3-mlp", EditedMLP)):
        with pytest.warns(UserWarning, match="not the code this patch restates"):
            assert not fastpath._matches(key, cls), cls.__name__
    # Llama's classes are not Phi-3's, and Phi-3's are not Llama's
    from transformers.models.llama import modeling_llama as ml

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert not fastpath._matches("phi3-layer", ml.LlamaDecoderLayer)
        assert not fastpath._matches("phi3-attn", ml.LlamaAttention)
        assert not fastpath._matches("llama-attn", mp.Phi3Attention)
        assert not fastpath._matches("qwen3-layer", mp.Phi3DecoderLayer)
    # installed on a model: the edited modules keep their forwards
    EditedLayer.__name__, EditedAttn.__name__, EditedMLP.__name__ = "Phi3DecoderLayer", "Phi3Attention", "Phi3MLP"
    model = _tiny_phi3()
    layers = model.model.layers
    layers[1].__class__ = EditedLayer
    layers[0].self_attn.__class__ = EditedAttn
    layers[0].mlp.__class__ = EditedMLP
    from dalm_amd.models import attention

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert attention.use_hip_attention_backward(model)
        assert fastpath.use_phi3_layer(model) == 1 and fastpath.use_phi3_mlp(model) == 1
        assert fastpath.use_phi3_attention_node(model) == 1
    assert _forward_names(layers) == ["_phi3_layer_forward", "forward"]
    assert _forward_names(l.self_attn for l in layers) == ["forward", "_phi3_attention_forward"]
    assert _forward_names(l.mlp for l in layers) == ["forward", "_phi3_mlp_forward"]


@pytest.mark.parametrize("case", [WIDTH_64_PARTIAL, WIDTH_64_FULL, WIDTH_128], ids=["64-48", "64-64", "128-96"])
def test_installers_take_a_phi3_model_and_bind_the_forwards(case):
    """Fails on a tree without the Phi-3 routing: there only the native RMSNorm is installed and the model stays on "sdpa"."""
    from dalm_amd.models import attention
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    model = _tiny_phi3(**case[0])
    assert model.config._attn_implementation == "sdpa" and not packed.attention_is_packable(model)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                    # no guard refuses anything of the installed classes
        got = use_generator_fast_paths(model)
    assert model.config._attn_implementation == attention.NAME == "dalm_sdpa" and packed.attention_is_packable(model)
    assert got["use_hip_attention_backward"] is True
    assert got["use_phi3_layer"] == 2 and got["use_phi3_mlp"] == 2 and got["use_phi3_attention_node"] == 2
    assert got["use_native_rms_norm"] == 5
    assert got["use_swiglu_kernel"] == 0 and got["use_fused_residual_norm"] == 0 and got["use_roll_rope"] is False
    assert got["use_llama_attention_node"] == 0 and got["use_qwen3_attention_node"] == 0 and got["use_cohere_attention_node"] == 0
    layers = model.model.layers
    assert _forward_names(layers) == ["_phi3_layer_forward"] * 2 and all(hasattr(l, "_dalm_orig_forward") for l in layers)
    assert _forward_names(l.self_attn for l in layers) == ["_phi3_attention_forward"] * 2
    assert all(hasattr(l.self_attn, "_dalm_orig_attn_forward") for l in layers)
    assert _forward_names(l.mlp for l in layers) == ["_phi3_mlp_forward"] * 2


def test_installer_order_and_who_is_left_alone():
    from transformers import LlamaConfig, LlamaForCausalLM, PhiConfig, PhiForCausalLM

    from dalm_amd.models import attention, fastpath
    from dalm_amd.models.rag_e2e_base_model import _GENERATOR_PATHS, _RETRIEVER_PATHS, DECODER_ONLY_TYPES

    order = list(_GENERATOR_PATHS)
    assert order.index(fastpath.use_phi3_attention_node) > order.index(attention.use_hip_attention_backward)
    new = (fastpath.use_phi3_layer, fastpath.use_phi3_mlp, fastpath.use_phi3_attention_node)
    for use in new:
        assert use in _GENERATOR_PATHS and use not in _RETRIEVER_PATHS
    assert "phi3" not in DECODER_ONLY_TYPES                               # a generator only
    llama = LlamaForCausalLM(LlamaConfig(hidden_size=128, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=2,
                                         intermediate_size=256, vocab_size=V))
    phi = PhiForCausalLM(PhiConfig(hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256, vocab_size=V,
                                   pad_token_id=0, bos_token_id=1, eos_token_id=2))
    assert phi.config.model_type == "phi"
    for other in (llama, phi):
        attention.use_hip_attention_backward(other)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            assert [use(other) for use in new] == [0, 0, 0]
    assert phi.config._attn_implementation == "sdpa"                      # the old `phi` is not switched either
    # a model that stays on "sdpa" gets no attention node
    assert fastpath.use_phi3_attention_node(_tiny_phi3()) == 0


def test_head_width_96_keeps_sdpa_and_the_row_wise_routes():
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    wide = _tiny_phi3(**WIDTH_96[0])                                      # Phi-3-mini's and Phi-3.5-mini's head width
    assert wide.model.layers[0].self_attn.head_dim == 96
    got = use_generator_fast_paths(wide)
    assert got["use_hip_attention_backward"] is False and got["use_phi3_attention_node"] == 0
    assert wide.config._attn_implementation == "sdpa" and not packed.attention_is_packable(wide)
    assert got["use_phi3_layer"] == 2 and got["use_phi3_mlp"] == 2        # the row-wise routes do not care
    assert _forward_names(l.self_attn for l in wide.model.layers) == ["forward"] * 2
    assert _forward_names(l.mlp for l in wide.model.layers) == ["_phi3_mlp_forward"] * 2


def test_a_window_shorter_than_the_positions_is_not_switched():
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    short = _tiny_phi3(sliding_window=16)
    got = use_generator_fast_paths(short)
    assert got["use_hip_attention_backward"] is False and got["use_phi3_attention_node"] == 0
    assert short.config._attn_implementation == "sdpa" and not packed.attention_is_packable(short)
    whole = _tiny_phi3(sliding_window=64)                                 # as long as the positions: full causal attention
    got = use_generator_fast_paths(whole)
    assert got["use_hip_attention_backward"] is True and got["use_phi3_attention_node"] == 2
    # per call: a window shorter than the keys goes to the class's own forward
    whole.config.sliding_window = 4
    attn = whole.model.layers[0].self_attn
    seen, own = [], attn._dalm_orig_attn_forward
    attn._dalm_orig_attn_forward = lambda *a, **k: (seen.append(1), own(*a, **k))[1]
    ids = torch.randint(3, V, (2, 8), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        whole(input_ids=ids, use_cache=False)
    assert seen == [1]


@pytest.mark.parametrize("switch", ["DALM_NORM_KERNEL", "DALM_SWIGLU_KERNEL", "DALM_ATTN_KERNEL"])
def test_the_reference_switches_turn_the_installers_off(monkeypatch, switch):
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    monkeypatch.setenv(switch, "0")
    model = _tiny_phi3()
    got = use_generator_fast_paths(model)
    layers = model.model.layers
    norm_on, mlp_on, attn_on = (switch != s for s in ("DALM_NORM_KERNEL", "DALM_SWIGLU_KERNEL", "DALM_ATTN_KERNEL"))
    assert got["use_phi3_layer"] == (2 if norm_on else 0) and got["use_phi3_mlp"] == (2 if mlp_on else 0)
    assert got["use_hip_attention_backward"] is attn_on and got["use_phi3_attention_node"] == (2 if attn_on else 0)
    assert _forward_names(layers) == ["_phi3_layer_forward" if norm_on else "forward"] * 2
    assert _forward_names(l.mlp for l in layers) == ["_phi3_mlp_forward" if mlp_on else "forward"] * 2
    assert _forward_names(l.self_attn for l in layers) == ["_phi3_attention_forward" if attn_on else "forward"] * 2
    assert packed.attention_is_packable(model) is attn_on


def _spy(mod, attr):
    seen, own = [], getattr(mod, attr)
    setattr(mod, attr, lambda *a, **k: (seen.append(1), own(*a, **k))[1])
    return seen


def test_what_the_routes_decline_runs_transformers_own_forward(monkeypatch):
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    ids = torch.randint(3, V, (2, 8), generator=torch.Generator().manual_seed(1))
    # attention dropout in a training call, a KV cache, output_attentions off the node's path, the two reference switches at call time
    drop = _tiny_phi3(attention_dropout=0.1)
    assert use_generator_fast_paths(drop)["use_phi3_attention_node"] == 2
    seen = _spy(drop.model.layers[0].self_attn, "_dalm_orig_attn_forward")
    drop.train()(input_ids=ids, use_cache=False)
    assert seen == [1]
    drop.eval()(input_ids=ids, use_cache=True)
    assert seen == [1, 1]
    drop(input_ids=ids, use_cache=False)
    assert seen == [1, 1]                                                 # eval, no cache: the routed statements
    for switch in ("DALM_FAST_ROPE", "DALM_ATTN_KERNEL"):
        monkeypatch.setenv(switch, "0")
        n = len(seen)
        drop(input_ids=ids, use_cache=False)
        assert len(seen) == n + 1, switch
        monkeypatch.delenv(switch)
    # residual dropout: a training call of EVERY layer goes to the class's own forward, an eval call takes the routed one
    res = _tiny_phi3(resid_pdrop=0.1)
    assert use_generator_fast_paths(res)["use_phi3_layer"] == 2
    # (on CPU tensors the routed forward itself ends in the class's own: what tells them apart is whether it was entered)
    from dalm_amd.models import fastpath

    counts = [_spy(layer, "_dalm_orig_forward") for layer in res.model.layers]
    routed, inner = [], fastpath._llama_layer_forward
    monkeypatch.setattr(fastpath, "_llama_layer_forward", lambda *a, **k: (routed.append(1), inner(*a, **k))[1])
    res.train()(input_ids=ids, use_cache=False)
    assert counts == [[1], [1]] and routed == []
    res.eval()(input_ids=ids, use_cache=False)
    assert routed == [1, 1]
    # another activation, a biased MLP: the MLP keeps its forward

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gelu = _tiny_phi3(hidden_act="gelu")
        assert fastpath.use_phi3_mlp(gelu) == 0 and _forward_names(l.mlp for l in gelu.model.layers) == ["forward"] * 2
        biased = _tiny_phi3()
        mlp = biased.model.layers[0].mlp
        mlp.down_proj.bias = torch.nn.Parameter(torch.zeros(mlp.down_proj.out_features))
        assert fastpath.use_phi3_mlp(biased) == 1
        assert _forward_names(l.mlp for l in biased.model.layers) == ["forward", "_phi3_mlp_forward"]


def test_the_kernel_predicate_says_no_on_the_cpu_and_to_what_the_kernel_does_not_take():
    from dalm_amd.models import tower_ops

    q, k = torch.randn(1, 2, 4, 64), torch.randn(1, 1, 4, 64)
    cos = torch.randn(1, 4, 48)
    assert not tower_ops.rope_partial_supported(q, k, cos, cos)           # CPU tensors


def _with_lora(m):
    from dalm_amd.models import lora

    torch.manual_seed(3)                                                  # the same adapter initialisation in every copy
    lora.inject_lora(m, ["q_proj", "v_proj"], lora_dropout=0.0)
    with torch.no_grad():                                                 # B away from zero: the A gradients say something
        for name, p in m.named_parameters():
            if "lora_B" in name:
                p.copy_(0.05 * torch.randn(p.shape, generator=torch.Generator().manual_seed(len(name))))
    return m


def test_lora_targets_resolve_to_the_fused_projection_and_round_trip(tmp_path):
    """`inject_lora(model, ["q_proj", "v_proj"])` raises on a tree without the phi3 fallback: Phi-3 has one qkv_proj."""
    from dalm_amd.models import lora
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    assert lora.FUSED_QKV_FALLBACK["phi3"] == ["qkv_proj"]
    base = _tiny_phi3().eval()
    model = copy.deepcopy(base)
    use_generator_fast_paths(model)
    assert lora.resolve_targets(model, ["q_proj", "v_proj"]) == ["qkv_proj"]
    _with_lora(model)
    assert lora.build_groups(model) == 0                                  # no q / k / v siblings to group: nothing built, no failure
    for layer in model.model.layers:
        assert isinstance(layer.self_attn.qkv_proj, lora.LoRALinear) and getattr(layer.self_attn.qkv_proj, "_group", None) is None
    trainable = [n for n, p in model.named_parameters() if p.requires_grad]
    assert len(trainable) == 2 * 2 and all("qkv_proj.lora_" in n for n in trainable)
    ids = torch.randint(3, V, (2, 9), generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        want = model(input_ids=ids, use_cache=False).logits
        assert not torch.allclose(want, base(input_ids=ids, use_cache=False).logits)
    lora.save_adapter(model, str(tmp_path), task_type="CAUSAL_LM")
    cfg = json.loads((tmp_path / "adapter_config.json").read_text())
    assert cfg["target_modules"] == ["qkv_proj"]
    fresh = lora.load_adapter(copy.deepcopy(base), str(tmp_path)).eval()
    with torch.no_grad():
        assert torch.equal(fresh(input_ids=ids, use_cache=False).logits, want)
        merged = lora.merge_and_unload(fresh)
        assert not lora.has_lora(merged) and type(merged.model.layers[0].self_attn.qkv_proj) is torch.nn.Linear
        got = merged(input_ids=ids, use_cache=False).logits
    assert torch.allclose(got, want, rtol=1e-4, atol=1e-5), float((got - want).abs().max())


@pytest.mark.parametrize("case", ["partial", "full", "width-128", "longrope"])
def test_patched_model_is_transformers_own_on_the_cpu(case):
    """fp32 on the CPU, eager mode: every patch falls through to the statements it restates; logits and LoRA gradients are equal bit
    for bit.  The longrope tables (short factors here: 12 positions of 64) pass through the node as they are."""
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    kw = {"partial": WIDTH_64_PARTIAL[0], "full": WIDTH_64_FULL[0], "width-128": WIDTH_128[0],
          "longrope": dict(WIDTH_64_PARTIAL[0], **_longrope(48))}[case]
    ref = _tiny_phi3(**kw)
    if case == "longrope":
        assert ref.model.rotary_emb.rope_type == "longrope"
    model = copy.deepcopy(ref)
    got = use_generator_fast_paths(model)
    assert got["use_phi3_layer"] == 2 and got["use_phi3_attention_node"] == 2 and got["use_phi3_mlp"] == 2
    _with_lora(model), _with_lora(ref)
    B, T = 3, 16 if case == "longrope" else 12
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
    assert seen == 2 * 2                                                  # A and B of qkv_proj, two layers


@pytest.mark.parametrize("left", [True, False])
def test_packed_decoder_run_equals_the_padded_run(left):
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    model = _tiny_phi3().eval()
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
