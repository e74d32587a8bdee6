"""Granite routing without a GPU: the source guards take the installed GraniteDecoderLayer / GraniteAttention / GraniteMLP and decline
edited copies; the installers take a tiny GraniteForCausalLM - "dalm_sdpa", packable, the layer, attention and MLP forwards bound by
name, the counts - and leave head width 80, biased projections and another activation alone; the patched model is transformers' own on
CPU tensors (bit for bit, LoRA gradients included); what follows from the Llama-named projections is there; the packed decoder run
equals the padded one; and the loss of a step whose hidden states meet `lm_head.weight` without the model's forward (fuse_lm_head, the
packed route) carries `logits_scaling`."""
import copy
import warnings

import pytest
import torch

from dalm_amd import packed

from helpers import norm_rel_err
from test_packed_cpu import _masks

MULTIPLIERS = dict(embedding_multiplier=12.0, residual_multiplier=0.22, attention_multiplier=0.015625, logits_scaling=8.0)


def _config(**over):
    from transformers import GraniteConfig

    kw = dict(vocab_size=259, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
              num_key_value_heads=2, max_position_embeddings=64, tie_word_embeddings=True, pad_token_id=1, bos_token_id=None,
              eos_token_id=2, **MULTIPLIERS)
    kw.update(over)
    return GraniteConfig(**kw)


def _tiny_granite(**over):
    from transformers import GraniteForCausalLM

    torch.manual_seed(0)
    model = GraniteForCausalLM(_config(**over))
    with torch.no_grad():                    # norm weights away from their initial ones: a dropped or misplaced norm shows
        for name, p in model.named_parameters():
            if name.endswith(("norm.weight", "layernorm.weight")):
                p.add_(0.3 * torch.randn(p.shape, generator=torch.Generator().manual_seed(len(name))))
    return model


def _forward_names(mods):
    return [getattr(getattr(m.forward, "__func__", None), "__name__", "") for m in mods]


def test_granite_is_what_the_routing_rests_on():
    """Read from the installed transformers: the four scalars sit where the routing expects them, norm and MLP are Llama's."""
    import inspect

    from transformers.models.granite import modeling_granite as mg
    from transformers.models.llama import modeling_llama as ml

    assert inspect.getsource(mg.GraniteMLP.forward) == inspect.getsource(ml.LlamaMLP.forward)
    assert inspect.getsource(mg.GraniteRMSNorm.forward) == inspect.getsource(ml.LlamaRMSNorm.forward)
    model = _tiny_granite()
    layer = model.model.layers[0]
    assert layer.residual_multiplier == 0.22 and layer.self_attn.scaling == 0.015625 and layer.self_attn.head_dim == 64
    assert model.model.embedding_multiplier == 12.0 and model.config.logits_scaling == 8.0
    assert model.lm_head.weight is model.model.embed_tokens.weight and model.lm_head.bias is None
    assert "inputs_embeds * self.embedding_multiplier" in inspect.getsource(mg.GraniteModel.forward)
    assert "logits / self.config.logits_scaling" in inspect.getsource(mg.GraniteForCausalLM.forward)


def test_source_guards_take_the_installed_classes_and_decline_edited_copies():
    from transformers.models.granite import modeling_granite as mg

    from dalm_amd.models import fastpath

    assert fastpath._matches("granite-layer", mg.GraniteDecoderLayer)
    assert fastpath._matches("llama-attn", mg.GraniteAttention)

    class NoMultiplier(mg.GraniteDecoderLayer):              # Llama's body: the multiplier on neither add
        def forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_values=None, use_cache=False,
                    position_embeddings=None, **kwargs):
            residual = hidden_states
            hidden_states = self.input_layernorm(hidden_states)
            hidden_states, _ = self.self_attn(hidden_states=hidden_states, attention_mask=attention_mask, position_ids=position_ids,
                                              past_key_values=past_key_values, use_cache=use_cache,
                                              position_embeddings=position_embeddings, **kwargs)
            hidden_states = residual + hidden_states
            residual = hidden_states
            hidden_states = self.post_attention_layernorm(hidden_states)
            hidden_states = self.mlp(hidden_states)
            hidden_states = residual + hidden_states
            return hidden_states

    class OneMultiplier(mg.GraniteDecoderLayer):             # ONE statement changed: the trailing add without it
        def forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_values=None, use_cache=False,
                    position_embeddings=None, **kwargs):
            """A docstring, as the class's own forward has one."""
            residual = hidden_states
            hidden_states = self.input_layernorm(hidden_states)
            hidden_states, _ = self.self_attn(hidden_states=hidden_states, attention_mask=attention_mask, position_ids=position_ids,
                                              past_key_values=past_key_values, use_cache=use_cache,
                                              position_embeddings=position_embeddings, **kwargs)
            hidden_states = residual + hidden_states * self.residual_multiplier
            residual = hidden_states
            hidden_states = self.post_attention_layernorm(hidden_states)
            hidden_states = self.mlp(hidden_states)
            hidden_states = residual + hidden_states
            return hidden_states

    class Prefixed(mg.GraniteDecoderLayer):                  # the right statements behind one more
        def forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_values=None, use_cache=False,
                    position_embeddings=None, **kwargs):
            """A docstring."""
            hidden_states = hidden_states * 2.0
            residual = hidden_states
            hidden_states = self.input_layernorm(hidden_states)
            hidden_states, _ = self.self_attn(hidden_states=hidden_states, attention_mask=attention_mask, position_ids=position_ids,
                                              past_key_values=past_key_values, use_cache=use_cache,
                                              position_embeddings=position_embeddings, **kwargs)
            hidden_states = residual + hidden_states * self.residual_multiplier
            residual = hidden_states
            hidden_states = self.post_attention_layernorm(hidden_states)
            hidden_states = self.mlp(hidden_states)
            hidden_states = residual + hidden_states * self.residual_multiplier
            return hidden_states

    class Same(mg.GraniteDecoderLayer):                      # the class's own statements, laid out differently: taken
        def forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_values=None, use_cache=False,
                    position_embeddings=None, **kwargs):
            residual = hidden_states
            hidden_states = self.input_layernorm(hidden_states)
            hidden_states, _ = self.self_attn(hidden_states=hidden_states, attention_mask=attention_mask, position_ids=position_ids,
                                              past_key_values=past_key_values, use_cache=use_cache,
                                              position_embeddings=position_embeddings, **kwargs)
            hidden_states = residual + hidden_states * self.residual_multiplier
            residual = hidden_states
            hidden_states = self.post_attention_layernorm(hidden_states)
            hidden_states = self.mlp(hidden_states)
            hidden_states = residual + hidden_states * self.residual_multiplier
            return hidden_states

    class GraniteAttention(mg.GraniteAttention):             # same name, another forward text
        def forward(self, hidden_states, position_embeddings=None, attention_mask=None, past_key_values=None, **kwargs):
            return mg.GraniteAttention.forward(self, hidden_states, position_embeddings, attention_mask, past_key_values, **kwargs)

    assert fastpath._matches("granite-layer", Same)
    for cls in (NoMultiplier, OneMultiplier, Prefixed):
        with pytest.warns(UserWarning, match="not the code this patch restates"):
            assert not fastpath._matches("granite-layer", cls), cls.__name__
    with pytest.warns(UserWarning, match="not the code this patch restates"):
        assert not fastpath._matches("llama-attn", GraniteAttention)
    # Llama's and Qwen3's layers are not Granite's, and Granite's is not theirs
    from transformers.models.llama import modeling_llama as ml

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert not fastpath._matches("granite-layer", ml.LlamaDecoderLayer)
        assert not fastpath._matches("qwen3-layer", mg.GraniteDecoderLayer)

    # installed on a model: the edited modules keep their forwards
    class GraniteMLP(mg.GraniteMLP):                         # same name, an edited forward: the value probe says no
        def forward(self, x):
            return self.down_proj(self.act_fn(self.gate_proj(x)) * self.up_proj(x)) * 0.5

    from dalm_amd.models import attention

    OneMultiplier.__name__ = "GraniteDecoderLayer"
    model = _tiny_granite()
    layers = model.model.layers
    layers[0].mlp.__class__ = GraniteMLP
    layers[1].__class__ = OneMultiplier
    layers[0].self_attn.__class__ = GraniteAttention
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert attention.use_hip_attention_backward(model)
        assert fastpath.use_swiglu_kernel(model) == 1
        assert fastpath.use_fused_residual_norm(model) == 1
        assert fastpath.use_llama_attention_node(model) == 1
    assert _forward_names(l.mlp for l in layers) == ["forward", "_swiglu_mlp_forward"]
    assert _forward_names(layers) == ["_granite_layer_forward", "forward"]
    assert [hasattr(l, "_dalm_orig_forward") for l in layers] == [True, False]
    assert _forward_names(l.self_attn for l in layers) == ["forward", "_llama_attention_forward"]


def test_installers_take_a_granite_model_and_bind_the_forwards():
    """Fails on a tree without the Granite routing: there only `use_native_rms_norm` takes anything of this model."""
    from dalm_amd.models import attention, fastpath
    from dalm_amd.models.rag_e2e_base_model import _GENERATOR_PATHS, DECODER_ONLY_TYPES, use_generator_fast_paths

    model = _tiny_granite()
    assert model.config._attn_implementation == "sdpa" and not packed.attention_is_packable(model)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                    # no guard refuses anything of the installed classes
        got = use_generator_fast_paths(model)
    assert model.config._attn_implementation == attention.NAME == "dalm_sdpa" and packed.attention_is_packable(model)
    assert got["use_hip_attention_backward"] is True
    assert got["use_fused_residual_norm"] == 2 and got["use_llama_attention_node"] == 2 and got["use_swiglu_kernel"] == 2
    assert got["use_native_rms_norm"] == 5                                # two per layer and the final one
    assert got["use_olmo2_layer"] == 0 and got["use_qwen3_attention_node"] == 0 and got["use_olmo2_attention_node"] == 0
    assert got["use_geglu_kernel"] == 0 and got["use_relu2_kernel"] == 0 and got["use_roll_rope"] is False
    layers = model.model.layers
    assert _forward_names(layers) == ["_granite_layer_forward"] * 2 and all(hasattr(l, "_dalm_orig_forward") for l in layers)
    assert _forward_names(l.self_attn for l in layers) == ["_llama_attention_forward"] * 2
    assert all(hasattr(l.self_attn, "_dalm_orig_attn_forward") for l in layers)
    assert _forward_names(l.mlp for l in layers) == ["_swiglu_mlp_forward"] * 2
    order = list(_GENERATOR_PATHS)
    assert order.index(fastpath.use_llama_attention_node) > order.index(attention.use_hip_attention_backward)
    assert "granite" not in DECODER_ONLY_TYPES                            # a generator only
    # GraniteModel.forward and GraniteForCausalLM.forward are transformers' own: the embedding multiplier stays their statement
    assert _forward_names([model, model.model]) == ["forward", "forward"]
    # a model that stays on "sdpa" gets no attention node
    assert fastpath.use_llama_attention_node(_tiny_granite()) == 0


def test_other_head_widths_keep_sdpa_and_do_not_pack():
    from dalm_amd.models import attention
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    wide = _tiny_granite(hidden_size=320)                                 # 4 heads of width 80
    assert wide.model.layers[0].self_attn.head_dim == 80
    got = use_generator_fast_paths(wide)
    assert got["use_hip_attention_backward"] is False and got["use_llama_attention_node"] == 0
    assert wide.config._attn_implementation == "sdpa" and not packed.attention_is_packable(wide)
    assert got["use_fused_residual_norm"] == 2 and got["use_swiglu_kernel"] == 2     # the row-wise routes do not care
    for hidden, ok in ((128, True), (512, True), (64, False)):            # widths 32 and 128 are taken, 16 is not
        m = _tiny_granite(hidden_size=hidden)
        assert attention.use_hip_attention_backward(m) is ok and packed.attention_is_packable(m) is ok


@pytest.mark.parametrize("switch", ["DALM_NORM_KERNEL", "DALM_SWIGLU_KERNEL", "DALM_ATTN_KERNEL"])
def test_the_reference_switches_turn_the_installers_off(monkeypatch, switch):
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    monkeypatch.setenv(switch, "0")
    model = _tiny_granite()
    got = use_generator_fast_paths(model)
    layers = model.model.layers
    norm_on, mlp_on, attn_on = (switch != s for s in ("DALM_NORM_KERNEL", "DALM_SWIGLU_KERNEL", "DALM_ATTN_KERNEL"))
    assert got["use_fused_residual_norm"] == (2 if norm_on else 0)
    assert got["use_swiglu_kernel"] == (2 if mlp_on else 0)
    assert got["use_hip_attention_backward"] is attn_on and got["use_llama_attention_node"] == (2 if attn_on else 0)
    assert _forward_names(layers) == ["_granite_layer_forward" if norm_on else "forward"] * 2
    assert _forward_names(l.mlp for l in layers) == ["_swiglu_mlp_forward" if mlp_on else "forward"] * 2
    assert _forward_names(l.self_attn for l in layers) == ["_llama_attention_forward" if attn_on else "forward"] * 2
    assert packed.attention_is_packable(model) is attn_on


def test_biased_projections_and_other_mlps_are_declined():
    from dalm_amd.models import attention, fastpath

    biased = _tiny_granite(attention_bias=True)
    assert attention.use_hip_attention_backward(biased)
    assert fastpath.use_llama_attention_node(biased) == 0
    assert _forward_names(l.self_attn for l in biased.model.layers) == ["forward"] * 2
    assert fastpath.use_fused_residual_norm(biased) == 2                  # the layer's adds and norms do not care
    mlp_bias = _tiny_granite(mlp_bias=True)
    assert fastpath.use_swiglu_kernel(mlp_bias) == 0 and _forward_names(l.mlp for l in mlp_bias.model.layers) == ["forward"] * 2
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gelu = _tiny_granite(hidden_act="gelu")
        assert fastpath.use_swiglu_kernel(gelu) == 0 and _forward_names(l.mlp for l in gelu.model.layers) == ["forward"] * 2
    # attention dropout: the node is installed, a training call with dropout goes to transformers' forward
    drop = _tiny_granite(attention_dropout=0.1)
    attention.use_hip_attention_backward(drop)
    assert fastpath.use_llama_attention_node(drop) == 2
    attn = drop.model.layers[0].self_attn
    seen, own = [], attn._dalm_orig_attn_forward
    attn._dalm_orig_attn_forward = lambda *a, **k: (seen.append(1), own(*a, **k))[1]
    ids = torch.randint(3, 259, (2, 8), generator=torch.Generator().manual_seed(1))
    drop.eval()(input_ids=ids, use_cache=False)
    assert seen == []
    drop.train()(input_ids=ids, use_cache=False)
    assert seen == [1]


def test_unit_residual_multiplier_takes_the_same_route():
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    got = use_generator_fast_paths(_tiny_granite(residual_multiplier=1.0))
    assert got["use_fused_residual_norm"] == 2


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
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    ref = _tiny_granite()
    model = copy.deepcopy(ref)
    got = use_generator_fast_paths(model)
    assert got["use_fused_residual_norm"] == 2 and got["use_llama_attention_node"] == 2 and got["use_swiglu_kernel"] == 2
    _with_lora(model), _with_lora(ref)
    B, T = 3, 12
    mask = _masks(B, T, True, 4)
    ids = torch.randint(3, 259, (B, T), generator=torch.Generator().manual_seed(5))
    w = torch.randn(B, T, 259, generator=torch.Generator().manual_seed(6))
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


def test_everything_trainable_gets_transformers_own_gradients_on_the_cpu():
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    ref = _tiny_granite()
    model = copy.deepcopy(ref)
    use_generator_fast_paths(model)
    ids = torch.randint(3, 259, (2, 10), generator=torch.Generator().manual_seed(7))
    for m in (model, ref):
        m(input_ids=ids, use_cache=False).logits.square().sum().backward()
    for (n, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        assert torch.equal(p.grad, q.grad), n


def test_what_follows_from_the_llama_named_projections():
    """Confirmed, not assumed: the one-GEMM q | k | v group, its LoRA kernels and the transposed dgrad key on the projections' names,
    which are Llama's; the tied lm_head takes the transposed-dgrad class too."""
    from dalm_amd.models import lora
    from dalm_amd.models.frozen_linear import FrozenLinearT, use_transposed_dgrad
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    model = _tiny_granite()
    use_generator_fast_paths(model)
    lora.inject_lora(model, ["q_proj", "v_proj"], lora_dropout=0.0)
    assert use_transposed_dgrad(model) == 2 * 4 + 1                       # o_proj, gate_proj, up_proj, down_proj per layer, the lm_head
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

    model = _tiny_granite().eval()
    B, T = 4, 16
    mask = _masks(B, T, left, 1)
    ids = torch.randint(3, 259, (B, T), generator=torch.Generator().manual_seed(2))
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


# ---- logits_scaling ------------------------------------------------------------------------------------------------------
def _left_mask(lens, T):
    return (torch.arange(T).unsqueeze(0) >= (T - torch.tensor(lens)).unsqueeze(1)).long()


def _loss_and_grads(route: str, scaling: float = 8.0):
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
    gen = _with_lora(_tiny_granite(logits_scaling=scaling))
    model = AutoModelForRagE2E.from_modules(bert, gen, None, None, normalize=True, get_peft=None, retriever_is_autoregressive=False)
    model.train()
    named = [(n, p) for n, p in model.generator_model.named_parameters() if p.requires_grad]
    assert named and all("lora_" in n for n, _ in named)
    opt = torch.optim.SGD([p for _, p in named], lr=0.0)
    step = RagE2EStep(model, opt, None, 100, ops=OracleOps(), fuse_lm_head=route == "hidden", overlap_towers=False)
    B, T, D = 6, 24, 32
    g = torch.Generator().manual_seed(22)
    batch = {"generator_input_input_ids": torch.randint(3, 259, (B, T), generator=g),
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
    assert out.shape[-1] == (259 if route == "logits" else 256)
    loss = step._loss(batch, is_packed, out, p, q, None, None)
    loss.backward()
    grads = {n: t.grad.detach().clone() for n, t in named}
    grads["q_emb"], grads["p_emb"] = q.grad.detach().clone(), p.grad.detach().clone()
    return float(loss.detach()), grads


@pytest.mark.parametrize("route", ["hidden", "packed"])
def test_logits_scaling_reaches_the_loss_without_the_models_forward(route):
    """The loss from the hidden states against the loss from the model's own logits (which GraniteForCausalLM.forward divides by
    logits_scaling = 8), at the bounds tests/test_hip_parity.py's `test_lm_head_fused_loss_equals_materialised_logits` holds
    `rag_e2e_loss_from_hidden` to against `rag_e2e_loss` in fp32: the loss within 1e-5 relative + 1e-6, every gradient within 2e-5 of
    its norm.  8 is a power of two: the scaling adds no error of its own.  Fails on a tree that does not scale: there the logits of
    these routes are 8 x too large."""
    want, g_want = _loss_and_grads("logits")
    got, g_got = _loss_and_grads(route)
    print(f"{route}: loss {got:.8f} against {want:.8f}")
    assert abs(got - want) <= 1e-5 * abs(want) + 1e-6, (got, want)
    assert set(g_got) == set(g_want)
    for n in sorted(g_want):
        assert float(g_want[n].abs().max()) > 0.0, n
        err = norm_rel_err(g_got[n], g_want[n])
        print(f"{route}: {n} {err:.3e}")
        assert err <= 2e-5, (n, err)


def test_a_unit_logits_scaling_changes_nothing():
    from dalm_amd.training.step import _logits_scaled

    h = torch.randn(3, 5, 16)
    assert _logits_scaled(h, _tiny_granite(logits_scaling=1.0)) is h
    assert _logits_scaled(h, torch.nn.Linear(2, 2)) is h                  # a model without a config, or a config without the field
    assert torch.equal(_logits_scaled(h, _tiny_granite(logits_scaling=16.0)), h / 16.0)
