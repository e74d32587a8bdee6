"""Arcee (AFM) routing without a GPU: the installers take a tiny ArceeForCausalLM and bind Llama's layer and attention forwards and
the ReLU^2 MLP forward, "dalm_sdpa" follows the head width, changed code and other MLP flavours are declined, the patched model is
transformers' own on CPU tensors, what follows from the Llama-named projections (the q | k | v LoRA group, the one concatenated
weight, the transposed dgrad swap) is there, the packed decoder run equals the padded one, and every condition of the fused
frozen-MLP node's routing predicate, when false, falls back."""
import copy
import warnings

import pytest
import torch

from dalm_amd import linear_live, packed
from dalm_amd.models import frozen_linear

from test_packed_cpu import _masks


def _config(**over):
    from transformers import ArceeConfig

    kw = dict(vocab_size=128, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
              num_key_value_heads=2, head_dim=64, bos_token_id=1, eos_token_id=2)
    kw.update(over)
    return ArceeConfig(**kw)


def _tiny_arcee(**over):
    from transformers import ArceeForCausalLM

    torch.manual_seed(0)
    return ArceeForCausalLM(_config(**over))


def _forward_names(mods):
    return [getattr(getattr(m.forward, "__func__", None), "__name__", "") for m in mods]


def test_arcee_is_llama_but_for_the_mlp():
    """What the routing rests on, read from the installed transformers: these compare equal to Llama's, source text for source text."""
    import inspect

    from transformers.models.arcee import modeling_arcee as ma
    from transformers.models.llama import modeling_llama as ml

    for a, b in ((ma.ArceeAttention.forward, ml.LlamaAttention.forward), (ma.ArceeDecoderLayer.forward, ml.LlamaDecoderLayer.forward),
                 (ma.ArceeRMSNorm.forward, ml.LlamaRMSNorm.forward), (ma.apply_rotary_pos_emb, ml.apply_rotary_pos_emb)):
        assert inspect.getsource(a) == inspect.getsource(b), a.__qualname__
    mlp = _tiny_arcee().model.layers[0].mlp
    assert type(mlp.act_fn).__name__ == "ReLUSquaredActivation" and not hasattr(mlp, "gate_proj")
    x = torch.randn(3, 256)
    assert torch.equal(mlp(x), mlp.down_proj(torch.square(torch.relu(mlp.up_proj(x)))))


def test_installers_take_an_arcee_model_and_bind_the_forwards():
    from dalm_amd.models import attention, fastpath
    from dalm_amd.models.rag_e2e_base_model import _ROW_WISE_PATHS, DECODER_ONLY_TYPES, use_generator_fast_paths

    model = _tiny_arcee()
    assert model.config._attn_implementation == "sdpa" and not packed.attention_is_packable(model)
    got = use_generator_fast_paths(model)
    assert model.config._attn_implementation == attention.NAME and packed.attention_is_packable(model)
    assert got["use_hip_attention_backward"] is True and got["use_roll_rope"] is True
    assert got["use_relu2_kernel"] == 2 and got["use_fused_residual_norm"] == 2 and got["use_llama_attention_node"] == 2
    assert got["use_native_rms_norm"] == 5                                # two per layer and the final one
    assert got["use_swiglu_kernel"] == 0 and got["use_geglu_kernel"] == 0 and got["use_qwen3_attention_node"] == 0
    layers = model.model.layers
    assert _forward_names(layers) == ["_llama_layer_forward"] * 2 and all(hasattr(l, "_dalm_orig_forward") for l in layers)
    assert _forward_names(l.mlp for l in layers) == ["_relu2_mlp_forward"] * 2
    assert _forward_names(l.self_attn for l in layers) == ["_llama_attention_forward"] * 2
    assert fastpath.use_relu2_kernel in _ROW_WISE_PATHS
    assert "arcee" not in DECODER_ONLY_TYPES                              # generator only: an Arcee causal-LM retriever stays as it is
    # a model that stays on "sdpa" gets no attention node
    assert fastpath.use_llama_attention_node(_tiny_arcee()) == 0


def test_config_defaults_keep_sdpa_and_do_not_pack():
    """`ArceeConfig()`'s own head width is 2560 / 32 = 80, which the attention kernels do not take: as a Gemma of width 256."""
    from transformers import ArceeConfig, ArceeForCausalLM

    from dalm_amd.models import attention, fastpath

    cfg = ArceeConfig()
    assert (cfg.head_dim or cfg.hidden_size // cfg.num_attention_heads) == 80
    # the default proportions (head width 80, no grouping beyond the default), shrunk: two layers, a small vocabulary
    wide = ArceeForCausalLM(ArceeConfig(vocab_size=128, hidden_size=320, intermediate_size=512, num_hidden_layers=2,
                                        num_attention_heads=4, num_key_value_heads=2, bos_token_id=1, eos_token_id=2))
    assert wide.config.head_dim == 80
    assert not attention.use_hip_attention_backward(wide)
    assert wide.config._attn_implementation == "sdpa" and not packed.attention_is_packable(wide)
    assert fastpath.use_llama_attention_node(wide) == 0
    assert fastpath.use_relu2_kernel(wide) == 2 and fastpath.use_fused_residual_norm(wide) == 2     # the row-wise routes do not care
    # AFM-4.5B's own geometry: 20 heads of 128 over 4 KV heads = groups of 5, which the grouped kernels admit
    assert attention.group_ok(20, 4)


def test_the_reference_switches_turn_the_installers_off(monkeypatch):
    from dalm_amd.models import attention, fastpath

    for name in ("DALM_SWIGLU_KERNEL", "DALM_NORM_KERNEL", "DALM_ATTN_KERNEL", "DALM_FAST_ROPE"):
        monkeypatch.setenv(name, "0")
    model = _tiny_arcee()
    assert fastpath.use_relu2_kernel(model) == 0 and fastpath.use_fused_residual_norm(model) == 0
    assert not attention.use_hip_attention_backward(model) and fastpath.use_llama_attention_node(model) == 0
    assert not fastpath.use_roll_rope(model)
    assert _forward_names(model.model.layers) == ["forward"] * 2 and _forward_names(l.mlp for l in model.model.layers) == ["forward"] * 2
    assert model.config._attn_implementation == "sdpa"


def test_other_mlp_flavours_are_declined():
    from dalm_amd.models import fastpath

    biased = _tiny_arcee(mlp_bias=True)
    assert fastpath.use_relu2_kernel(biased) == 0 and _forward_names(l.mlp for l in biased.model.layers) == ["forward"] * 2
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        silu = _tiny_arcee(hidden_act="silu")
        assert fastpath.use_relu2_kernel(silu) == 0 and _forward_names(l.mlp for l in silu.model.layers) == ["forward"] * 2
        assert fastpath.use_relu2_kernel(_tiny_arcee(hidden_act="relu")) == 0
    from transformers import LlamaConfig, LlamaForCausalLM

    llama = LlamaForCausalLM(LlamaConfig(vocab_size=128, hidden_size=64, intermediate_size=128, num_hidden_layers=1,
                                         num_attention_heads=4, num_key_value_heads=2))
    assert fastpath.use_relu2_kernel(llama) == 0 and fastpath.use_swiglu_kernel(llama) == 1


def test_changed_code_is_declined_and_left_in_place():
    from transformers.models.arcee import modeling_arcee as ma

    from dalm_amd.models import attention, fastpath

    class ArceeMLP(ma.ArceeMLP):                                 # same name, an edited forward: the value probe says no
        def forward(self, x):
            return self.down_proj(self.act_fn(self.up_proj(x))) * 0.5

    class GatedArceeMLP(ma.ArceeMLP):                            # a gate beside the two projections: not the ungated formula
        pass

    class ArceeDecoderLayer(ma.ArceeDecoderLayer):               # the whole body with ONE statement changed (the last add)
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

    class ArceeAttention(ma.ArceeAttention):                     # same name, another forward text
        def forward(self, hidden_states, position_embeddings=None, attention_mask=None, past_key_values=None, **kwargs):
            return ma.ArceeAttention.forward(self, hidden_states, position_embeddings, attention_mask, past_key_values, **kwargs)

    assert fastpath._matches("arcee-layer", ma.ArceeDecoderLayer)
    with pytest.warns(UserWarning, match="not the code this patch restates"):
        assert not fastpath._matches("arcee-layer", ArceeDecoderLayer)
    model = _tiny_arcee()
    layers = model.model.layers
    layers[0].mlp.__class__ = ArceeMLP
    layers[1].__class__ = ArceeDecoderLayer
    layers[0].self_attn.__class__ = ArceeAttention
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert attention.use_hip_attention_backward(model)
        assert fastpath.use_relu2_kernel(model) == 1
        assert fastpath.use_fused_residual_norm(model) == 1
        assert fastpath.use_llama_attention_node(model) == 1
    assert _forward_names(l.mlp for l in layers) == ["forward", "_relu2_mlp_forward"]
    assert _forward_names(layers) == ["_llama_layer_forward", "forward"]
    assert [hasattr(l, "_dalm_orig_forward") for l in layers] == [True, False]
    assert _forward_names(l.self_attn for l in layers) == ["forward", "_llama_attention_forward"]

    model = _tiny_arcee()
    mlp = model.model.layers[0].mlp
    mlp.__class__ = GatedArceeMLP
    GatedArceeMLP.__name__ = "ArceeMLP"
    mlp.gate_proj = torch.nn.Linear(256, 512, bias=False)
    assert fastpath.use_relu2_kernel(model) == 1
    assert _forward_names(l.mlp for l in model.model.layers) == ["forward", "_relu2_mlp_forward"]


def test_patched_model_is_transformers_own_on_the_cpu():
    """fp32 on the CPU: every patch falls through to the statements it restates, logits and gradients are equal bit for bit."""
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    ref = _tiny_arcee()
    model = copy.deepcopy(ref)
    got = use_generator_fast_paths(model)
    assert got["use_relu2_kernel"] == 2 and got["use_llama_attention_node"] == 2 and got["use_fused_residual_norm"] == 2
    B, T = 3, 12
    mask = _masks(B, T, True, 4)
    ids = torch.randint(3, 128, (B, T), generator=torch.Generator().manual_seed(5))
    w = torch.randn(B, T, 128, generator=torch.Generator().manual_seed(6))
    outs = []
    for m in (model, ref):
        logits = m(input_ids=ids, attention_mask=mask, use_cache=False).logits
        (logits * w).sum().backward()
        outs.append(logits.detach())
    # `use_native_rms_norm` is in the list: F.rms_norm is the same formula, one rounding order apart (fastpath.py's header)
    assert torch.allclose(outs[0], outs[1], atol=2e-5, rtol=1e-4), float((outs[0] - outs[1]).abs().max())
    for (n, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        assert p.grad is not None and torch.allclose(p.grad, q.grad, atol=2e-4, rtol=1e-3), n


def test_what_follows_from_the_llama_named_projections():
    """Confirmed, not assumed: the reference's LoRA targets apply as they stand and q | k | v form ONE group of three (the one-GEMM
    q | k | v and its LoRA kernels key on it), every other frozen projection takes the transposed-dgrad class, no projection has a
    bias, and the group sees grouped heads (k / v narrower than q)."""
    from dalm_amd.models import lora
    from dalm_amd.models.frozen_linear import FrozenLinearT, use_transposed_dgrad
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    model = _tiny_arcee()
    use_generator_fast_paths(model)
    lora.inject_lora(model, ["q_proj", "v_proj"], lora_dropout=0.0)
    swapped = use_transposed_dgrad(model)
    assert swapped == 2 * 3 + 1                                           # o_proj, up_proj, down_proj per layer, and the lm_head
    for layer in model.model.layers:
        a = layer.self_attn
        assert isinstance(a.q_proj, lora.LoRALinear) and isinstance(a.v_proj, lora.LoRALinear)
        assert a.q_proj._group is not None and a.q_proj._group is a.k_proj._group is a.v_proj._group
        assert len(a.q_proj._group.members) == 3
        assert all(getattr(getattr(m, "base_layer", m), "bias", None) is None for m in (a.q_proj, a.k_proj, a.v_proj, a.o_proj))
        assert type(a.o_proj) is FrozenLinearT and type(layer.mlp.up_proj) is FrozenLinearT and type(layer.mlp.down_proj) is FrozenLinearT
        q_w = getattr(a.q_proj, "base_layer", a.q_proj).weight
        k_w = getattr(a.k_proj, "base_layer", a.k_proj).weight
        assert q_w.shape == (256, 256) and k_w.shape == (128, 256)        # 4 query heads over 2 key / value heads
    trainable = [n for n, p in model.named_parameters() if p.requires_grad]
    assert trainable and all("lora_" in n for n in trainable)


@pytest.mark.parametrize("left", [True, False])
def test_packed_decoder_run_equals_the_padded_run(left):
    from dalm_amd.models import attention

    model = _tiny_arcee(max_position_embeddings=64).eval()
    B, T = 4, 16
    mask = _masks(B, T, left, 1)
    ids = torch.randint(3, 128, (B, T), generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        want = model.base_model(input_ids=ids, attention_mask=mask, use_cache=False)[0]
        assert attention.use_hip_attention_backward(model) and packed.attention_is_packable(model)
        rows, cu = packed.pack_plan(mask, shifted=True, multiple=8)
        h = packed.generator_hidden(model, ids, mask, rows, cu)
    valid = rows >= 0
    sel = rows[valid]
    seen = mask.reshape(-1).index_select(0, sel) != 0
    got, ref = h[valid][seen], want.reshape(B * T, -1).index_select(0, sel)[seen]
    assert torch.allclose(got, ref, atol=2e-5, rtol=1e-4), float((got - ref).abs().max())


# ---- the fused frozen-MLP node's routing predicate ------------------------------------------------------------------------------
ROWS, H, C = 192, 256, 448                                         # C % 64 == 0 (it is the down GEMM's K); no `% 128` rule: full 256-column tiles
SHAPES = [(ROWS, C, H), (ROWS, H, C)]                              # up forward = down dgrad; down forward = up dgrad


@pytest.fixture
def table():
    linear_live.set_table(SHAPES)
    linear_live.set_enabled(True)
    linear_live.set_mlp_fused(True)
    yield
    linear_live.set_table(None)
    linear_live.set_enabled(True)
    linear_live.set_mlp_fused(True)


def _mlp(c=C, h=H, dtype=torch.bfloat16, bias=False, cls=torch.nn.Linear):
    mods = [cls(h, c, bias=bias, device="meta", dtype=dtype), cls(c, h, bias=bias, device="meta", dtype=dtype)]
    for m in mods:
        m.requires_grad_(False)
    return mods


def _x(rows=ROWS, h=H, dtype=torch.bfloat16):
    return torch.empty(2, rows // 2, h, device="meta", dtype=dtype, requires_grad=True)


def test_shape_predicate(table):
    ok = dict(rows=ROWS, c=C, h=H, dtype=torch.bfloat16, has_bias=False, have_partition=True)
    assert linear_live.relu2_mlp_routed(**ok)
    assert not linear_live.relu2_mlp_routed(**{**ok, "dtype": torch.float32})
    assert not linear_live.relu2_mlp_routed(**{**ok, "has_bias": True})
    assert not linear_live.relu2_mlp_routed(**{**ok, "have_partition": False})
    assert not linear_live.relu2_mlp_routed(**{**ok, "rows": ROWS + 1})
    for drop in range(2):                                          # each of the node's GEMM shapes must be in the table
        linear_live.set_table(SHAPES[:drop] + SHAPES[drop + 1:])
        assert not linear_live.relu2_mlp_routed(**ok), SHAPES[drop]
    linear_live.set_table(SHAPES)
    linear_live.set_mlp_fused(False)
    assert not linear_live.relu2_mlp_routed(**ok)
    linear_live.set_mlp_fused(True)
    linear_live.set_enabled(False)
    assert not linear_live.relu2_mlp_routed(**ok)
    linear_live.set_enabled(True)
    assert linear_live.relu2_mlp_routed(**ok)
    linear_live.set_table(None)                                    # the measured table: DESIGN.md says whether AFM's shapes went in
    afm = linear_live.relu2_mlp_routed(4608, 18432, 2560, torch.bfloat16, False, True)
    assert afm == ({(4608, 18432, 2560), (4608, 2560, 18432)} <= linear_live.ROUTED_SHAPES)


def test_candidate_conditions(table):
    assert frozen_linear.relu2_mlp_candidate(_x(), *_mlp()) == (ROWS, C, H)
    assert frozen_linear.relu2_mlp_candidate(_x(), *_mlp(cls=frozen_linear.FrozenLinearT)) == (ROWS, C, H)
    assert frozen_linear.relu2_mlp_candidate(_x(dtype=torch.float32), *_mlp()) is None                 # fp32 activations
    assert frozen_linear.relu2_mlp_candidate(_x(dtype=torch.float32), *_mlp(dtype=torch.float32)) is None    # fp32 projections
    assert frozen_linear.relu2_mlp_candidate(_x(), *_mlp(bias=True)) is None                           # biased projections
    assert frozen_linear.relu2_mlp_candidate(_x(rows=ROWS - 2), *_mlp()) is None                       # off-table shapes
    assert frozen_linear.relu2_mlp_candidate(_x(), *_mlp(c=C + 8)) is None
    for i in range(2):
        mods = _mlp()
        mods[i].weight.requires_grad_(True)                                                            # one projection trainable
        assert frozen_linear.relu2_mlp_candidate(_x(), *mods) is None, i
        mods = _mlp()

        class Wrapped(torch.nn.Linear):                                                                # not a plain projection
            pass

        mods[i].__class__ = Wrapped
        assert frozen_linear.relu2_mlp_candidate(_x(), *mods) is None, i
        mods = _mlp()
        mods[i].weight.data = mods[i].weight.data.to(torch.float32)                                    # one weight not bf16
        assert frozen_linear.relu2_mlp_candidate(_x(), *mods) is None, i
    mods = _mlp()
    mods[1] = torch.nn.Linear(C, H + 8, bias=False, device="meta", dtype=torch.bfloat16).requires_grad_(False)   # not one MLP's shapes
    assert frozen_linear.relu2_mlp_candidate(_x(), *mods) is None
    linear_live.set_mlp_fused(False)
    assert frozen_linear.relu2_mlp_candidate(_x(), *_mlp()) is None
    linear_live.set_mlp_fused(True)
    linear_live.set_enabled(False)
    assert frozen_linear.relu2_mlp_candidate(_x(), *_mlp()) is None


def test_cpu_tensors_never_route(table):
    mods = [torch.nn.Linear(H, C, bias=False, dtype=torch.bfloat16), torch.nn.Linear(C, H, bias=False, dtype=torch.bfloat16)]
    for m in mods:
        m.requires_grad_(False)
    x = torch.zeros(2, ROWS // 2, H, dtype=torch.bfloat16, requires_grad=True)
    assert frozen_linear.relu2_mlp_candidate(x, *mods) == (ROWS, C, H)
    assert frozen_linear.relu2_mlp_forward(x, *mods) is None


def test_device_side_conditions_fall_back(table, monkeypatch):
    """Past the candidate test, the route needs: an eligible call, operands the kernel accepts, a partition (a padded tower call in
    progress) and the transposed dgrad copies.  Each alone, when missing, falls back.  No table to prepare."""
    x, mods = _x(), _mlp()
    part = (object(), object())
    good = {
        (frozen_linear, "_eligible"): lambda x, *m: True,
        (linear_live, "accepts"): lambda x2, w, b: True,
        (linear_live, "route"): lambda x2, w, b: part,
        (frozen_linear, "dgrad_weight"): lambda w, dt=None: w,
    }
    bad = {
        (frozen_linear, "_eligible"): lambda x, *m: False,
        (linear_live, "accepts"): lambda x2, w, b: False,
        (linear_live, "route"): lambda x2, w, b: None,               # no partition: not inside a padded tower call
        (frozen_linear, "dgrad_weight"): lambda w, dt=None: None,
    }
    monkeypatch.setattr(linear_live, "mlp_prepare", lambda d: pytest.fail("the ReLU^2 node has no table to prepare"))
    for (mod, name), fn in good.items():
        monkeypatch.setattr(mod, name, fn)
    assert frozen_linear.relu2_mlp_route(x, *mods) is part
    for key, fn in bad.items():
        monkeypatch.setattr(key[0], key[1], fn)
        assert frozen_linear.relu2_mlp_route(x, *mods) is None, key[1]
        monkeypatch.setattr(key[0], key[1], good[key])
    assert frozen_linear.relu2_mlp_route(x, *mods) is part
    linear_live.set_mlp_fused(False)
    assert frozen_linear.relu2_mlp_route(x, *mods) is None
