"""Speed-ups of the HF towers that keep the math: PyTorch-ROCm natives, and (round 4) two HIP kernels for the elementwise
chains of a Llama-family layer the step spent the most launches on (rotary embedding, SwiGLU: `tower_ops.py`).

`use_native_rms_norm(model)`: transformers' *RMSNorm modules (Llama, Mistral, ...) spell the norm as
~7 eager elementwise kernels forward and ~10 backward (upcast, pow, mean, rsqrt, mul, downcast, mul).
`torch.nn.functional.rms_norm` computes the same `w * x * rsqrt(mean(x^2) + eps)` (fp32 internally) in
one fused kernel each way: 458 -> 124 us per norm (fwd+bwd, [4608, 4096] bf16 on MI355X), about 22 ms of
a 230 ms cfg3 step.  Differences are bf16 rounding-order only (max 1 bf16 ulp).

Every patch is a guard (`_guard`: a numeric probe, or for a forward that restates transformers' statements an entry of
`_SOURCE_GUARDS` read by `_source_guard`), a forward, and a `use_*` function that is one call of `_install`.
"""
from __future__ import annotations

import copy
import os
import types

import torch
import torch.nn.functional as F


def _off(name: str) -> bool:
    """True when the environment sets the reference switch `name` to "0".  Read at call time: the tests that build a
    "kernels off" model flip these around installer calls and between two forward calls of one process."""
    return os.environ.get(name, "1") == "0"


_warned = set()


def _warn_once(key: str, msg: str) -> None:
    if key not in _warned:
        _warned.add(key)
        import warnings

        warnings.warn("dalm_amd.fastpath: " + msg)


def _close(a: torch.Tensor, b: torch.Tensor, ulps: float = 1.0) -> bool:
    """Equal up to `ulps` units in the last place of the tensors' dtype, relative to the largest magnitude (the patches round
    where transformers' chains round; what is left is the summation order of a mean or one fused multiply-add)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    eps = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}.get(a.dtype, 2.0 ** -20)
    scale = max(float(b.float().abs().max()), 1e-6)
    return float((a.float() - b.float()).abs().max()) <= ulps * eps * scale


_checked: dict = {}


def _guard(key: tuple, who: str, what: str, probe) -> bool:
    """Run-time guard of one patch: `probe()` says whether transformers' `who` IS the code the replacement
    stands for.  Asked once per `key` (a probe that raises counts as no); every refusal warns once per patch kind and `who`."""
    if key not in _checked:
        try:
            _checked[key] = bool(probe())
        except Exception:
            _checked[key] = False
    if not _checked[key]:
        _warn_once(f"{key[0]}:{who}", f"{who} is not {what}: transformers' own code stays in place")
    return _checked[key]


def _source_guard(key: str, cls, check, what: str) -> bool:
    """The guard of a patch that restates `cls.forward`: `check(params, src)` over the parameter names and the source text."""
    import inspect

    return _guard((key, cls), cls.__name__ + ".forward", what,
                  lambda: check(list(inspect.signature(cls.forward).parameters), inspect.getsource(cls.forward)))


_RESTATED = "the code this patch restates"
_SOURCE_GUARDS: dict = {}      # patch kind -> (check(params, src), what the forward must be): filled in next to each restating forward


def _matches(key: str, cls) -> bool:
    return _source_guard(key, cls, *_SOURCE_GUARDS[key])


def _qwen3_attention_matches(cls) -> bool:            # the names tests/test_qwen3_cpu.py asks the two Qwen3 guards by
    return _matches("qwen3-attn", cls)


def _qwen3_layer_matches(cls) -> bool:
    return _matches("qwen3-layer", cls)


def _body(src: str) -> list:
    """The lines of a function's source, stripped, without blank and comment lines."""
    return [ln.strip() for ln in src.splitlines() if ln.strip() and not ln.strip().startswith("#")]


def _restates(params: list, *statements: str):
    """A source check: exactly these parameters, and every one of these statements somewhere in the text."""
    return lambda p, src: p == params and all(s in src for s in statements)


def _install(model: torch.nn.Module, names: tuple, eligible, guard, forward, keep: str = "") -> int:
    """Bind `forward` on every module whose class name matches one of `names` (fnmatch patterns), that `eligible(mod)` takes and
    whose code passes its guard: a key of `_SOURCE_GUARDS`, or a function of the module.  `keep` names the attribute under
    which the module's own forward stays reachable.  Returns how many modules were patched."""
    from fnmatch import fnmatchcase

    n = 0
    for mod in model.modules():
        if not any(fnmatchcase(type(mod).__name__, pat) for pat in names) or not eligible(mod):
            continue
        if not (_matches(guard, type(mod)) if isinstance(guard, str) else guard(mod)):
            continue
        if keep:
            setattr(mod, keep, mod.forward)
        mod.forward = types.MethodType(forward, mod)
        n += 1
    return n


def _native_forward(self, hidden_states: torch.Tensor) -> torch.Tensor:
    return F.rms_norm(hidden_states, (hidden_states.shape[-1],), self.weight, self._dalm_eps)


def _plain_rms_norm(mod) -> bool:
    w = getattr(mod, "weight", None)
    return (w is not None and w.dim() == 1 and getattr(mod, "variance_epsilon", getattr(mod, "eps", None)) is not None
            and "Gemma" not in type(mod).__name__)             # Gemma: (1 + w) parameterisation, not the same formula


def use_native_rms_norm(model: torch.nn.Module) -> int:
    """Patch every `*RMSNorm` module with a plain weight vector; returns how many were patched."""
    return _install(model, ("*RMSNorm",), _plain_rms_norm, _norm_matches, _native_forward)


def _norm_matches(mod: torch.nn.Module) -> bool:
    """The module's OWN forward against the fused formula on a small random tensor, once per class, dtype and device type."""
    w = mod.weight
    mod._dalm_eps = float(getattr(mod, "variance_epsilon", getattr(mod, "eps", None)))       # what `_native_forward` reads

    def probe():
        x = torch.randn(4, 3, w.shape[0], generator=torch.Generator().manual_seed(0)).to(device=w.device, dtype=w.dtype)
        with torch.no_grad():
            return _close(_native_forward(mod, x), type(mod).forward(mod, x), 2.0)

    return _guard(("norm", type(mod), w.dtype, w.device.type), type(mod).__name__ + ".forward",
                  "w * x * rsqrt(mean(x^2) + eps) here", probe)


# ---------------------------------------------------------------------------
# rotary embedding with fewer launches (Llama-style "rotate_half" layout)
# ---------------------------------------------------------------------------
def _rope_roll(q, k, cos, sin, position_ids=None, unsqueeze_dim=1):
    """Same result as transformers' apply_rotary_pos_emb: x*cos + rotate_half(x)*sin with
    rotate_half(x) = cat(-x2, x1).  Folding the sign into sin (a tiny [B,1,T,hd] tensor) turns
    rotate_half into a plain roll by hd/2, and addcmul fuses the second multiply with the add:
    3 launches forward / 4 backward per tensor instead of ~5 / ~8 (neg, cat and their slice backwards go)."""
    cos = cos.unsqueeze(unsqueeze_dim)
    sin = sin.unsqueeze(unsqueeze_dim)
    h = q.shape[-1] // 2
    sin_signed = torch.cat((-sin[..., :h], sin[..., h:]), dim=-1)
    q_embed = torch.addcmul(q * cos, torch.roll(q, h, dims=-1), sin_signed)
    k_embed = torch.addcmul(k * cos, torch.roll(k, h, dims=-1), sin_signed)
    return q_embed, k_embed


def _rope_hip(q, k, cos, sin, position_ids=None, unsqueeze_dim=1):
    """transformers' apply_rotary_pos_emb as one HIP launch for q and k together (`dalm_rope_qk`, one more in the backward),
    rounding where the eager chain rounds: same values and gradients as transformers' own code (round 4; the roll + addcmul
    form above was 6 launches forward / 8 backward per layer and rounded once less than transformers does).
    CPU tensors and layouts the kernel does not take use the roll form."""
    from . import tower_ops

    if unsqueeze_dim == 1 and tower_ops.rope_supported(q, k, cos, sin):
        return tower_ops.rope_qk(q, k, cos, sin)
    return _rope_roll(q, k, cos, sin, position_ids, unsqueeze_dim)


def use_roll_rope(model: torch.nn.Module) -> bool:
    """Swap the module-level apply_rotary_pos_emb of the model's own modeling file (Llama, Falcon and Arcee)."""
    if _off("DALM_FAST_ROPE"):
        return False
    import importlib

    mod_name = type(getattr(model, "base_model", model)).__module__
    # modeling files whose apply_rotary_pos_emb is the formula above, word for word (Falcon calls it only without alibi; Arcee's
    # is Llama's text)
    if not mod_name.endswith(("modeling_llama", "modeling_falcon", "modeling_arcee")):
        return False
    mod = importlib.import_module(mod_name)
    if not hasattr(mod, "apply_rotary_pos_emb"):
        return False
    if getattr(mod.apply_rotary_pos_emb, "__name__", "") != "_rope_hip":
        mod._dalm_orig_apply_rotary_pos_emb = mod.apply_rotary_pos_emb
    # The function being replaced must BE the formula the kernel implements.  The swap is PROCESS-WIDE (transformers resolves
    # apply_rotary_pos_emb through the modeling file's globals; there is no per-model hook), so every model of this modeling
    # file in the process takes the replacement.
    dev = next((p.device for p in model.parameters()), torch.device("cpu"))
    ok = _rope_matches(mod._dalm_orig_apply_rotary_pos_emb, dev, mod_name)
    mod.apply_rotary_pos_emb = _rope_hip if ok else mod._dalm_orig_apply_rotary_pos_emb
    return ok


def _rope_matches(orig, dev: torch.device, mod_name: str) -> bool:
    """orig(q, k, cos, sin) against `_rope_hip` on small random tensors: on the CPU against the roll form in float32 (the
    same formula, one fused multiply-add apart), on a GPU additionally against the HIP kernel in bfloat16 - there the values
    must be EQUAL (tests/test_tower_ops_gpu.py asserts the same)."""
    def probe():
        g = torch.Generator().manual_seed(0)
        q, k = torch.randn(2, 4, 5, 16, generator=g), torch.randn(2, 2, 5, 16, generator=g)
        ang = torch.rand(2, 5, 8, generator=g) * 6.28
        cos, sin = torch.cat((ang.cos(), ang.cos()), -1), torch.cat((ang.sin(), ang.sin()), -1)
        with torch.no_grad():
            want = orig(q, k, cos, sin)
            got = _rope_roll(q, k, cos, sin)
            ok = all(_close(a, b, 8.0) for a, b in zip(got, want))
            if ok and dev.type == "cuda":
                args = [t.to(dev, torch.bfloat16) for t in (q, k, cos, sin)]
                ok = all(torch.equal(a, b) for a, b in zip(_rope_hip(*args), orig(*args)))
        return ok

    return _guard(("rope", orig, dev.type), mod_name + ".apply_rotary_pos_emb", "x * cos + rotate_half(x) * sin here", probe)


# ---------------------------------------------------------------------------
# SwiGLU MLP: silu(gate) * up as one launch per direction, no saved activation
# ---------------------------------------------------------------------------
def _swiglu_mlp_forward(self, x):
    from . import tower_ops

    from . import frozen_linear

    out = frozen_linear.swiglu_mlp_forward(x, self.gate_proj, self.up_proj, self.down_proj)   # padded step, all frozen: one node
    if out is not None:
        return out
    gate, up = frozen_linear.pair_forward(x, self.gate_proj, self.up_proj)   # frozen: one node, the two dx GEMMs accumulate
    if tower_ops.swiglu_supported(gate, up):
        return self.down_proj(tower_ops.swiglu(gate, up))
    return self.down_proj(self.act_fn(gate) * up)


def use_swiglu_kernel(model: torch.nn.Module, cohere: bool = False) -> int:
    """Patch the `*MLP` modules that are exactly transformers' LlamaMLP formula - down(act(gate(x)) * up(x)) with
    act = SiLU - to evaluate silu(gate) * up through `dalm_swiglu_{fwd,bwd}`: 2 eager launches forward and 4 backward
    become 1 + 1, and the [tokens, intermediate] activation is recomputed instead of saved (101 MB per layer at cfg3).
    Same rounding points as the eager chain.  DALM_SWIGLU_KERNEL=0 disables; returns how many modules were patched.
    `cohere`: also name CohereMLP (Llama's formula, behind the same value probe).  Off unless asked for: in the Cohere layer
    measurements leaving the SwiGLU kernels out cost less than the run-to-run spread in two runs of three (profiles/cohere_bench.txt),
    so the installer lists do not ask."""
    if _off("DALM_SWIGLU_KERNEL"):
        return 0

    def gated_silu(mod) -> bool:
        act = getattr(mod, "act_fn", None)
        return (all(hasattr(mod, a) for a in ("gate_proj", "up_proj", "down_proj"))
                and (isinstance(act, torch.nn.SiLU) or type(act).__name__ in ("SiLUActivation", "SiLU"))
                # a GraniteMLP with `mlp_bias` keeps transformers' code
                and (type(mod).__name__ != "GraniteMLP" or _bias_free(mod, ("gate_proj", "up_proj", "down_proj"))))

    names = ("LlamaMLP", "MistralMLP", "Qwen2MLP", "Qwen3MLP", "Olmo2MLP", "GraniteMLP", *(("CohereMLP",) if cohere else ()))
    return _install(model, names, gated_silu, _mlp_matches, _swiglu_mlp_forward)


def _bias_free(mod, names: tuple) -> bool:
    return all(getattr(getattr(mod, a, None), "bias", 0) is None for a in names)


def _mlp_matches(mod: torch.nn.Module, forward=_swiglu_mlp_forward, what: str = "down(silu(gate(x)) * up(x)) here",
                 first: str = "gate_proj") -> bool:
    """The class's own forward against the patched one on a small random input, once per class, dtype and device type (on a
    GPU the patched forward runs the HIP kernel: <= 1 ulp of the output dtype).  `first`: a projection that takes x."""
    first = getattr(mod, first)
    w = getattr(first, "weight", None)
    where = (None, None) if w is None else (w.dtype, w.device.type)        # no resident weight: the probe fails, the guard says no

    def probe():
        x = torch.randn(2, 3, first.in_features, generator=torch.Generator().manual_seed(0)).to(device=w.device, dtype=w.dtype)
        with torch.no_grad():
            return _close(forward(mod, x), type(mod).forward(mod, x), 2.0)

    return _guard(("mlp", type(mod), *where), type(mod).__name__ + ".forward", what, probe)


# ---------------------------------------------------------------------------
# Gemma: GeGLU MLP and the (1 + w) RMSNorm (the decoder layer itself is Llama's: `_llama_layer_forward` below)
# ---------------------------------------------------------------------------
def _geglu_mlp_forward(self, x):
    from . import frozen_linear, tower_ops

    gate, up = frozen_linear.pair_forward(x, self.gate_proj, self.up_proj)   # frozen: one node, the two dx GEMMs accumulate
    if tower_ops.geglu_supported(gate, up):
        return self.down_proj(tower_ops.geglu(gate, up))
    return self.down_proj(self.act_fn(gate) * up)


def _is_tanh_gelu(act) -> bool:
    """torch's tanh-approximated GELU: nn.GELU(approximate="tanh"), or transformers' GELUTanh around
    nn.functional.gelu(approximate="tanh") (ACT2FN["gelu_pytorch_tanh"]) - not its python spelling, which rounds elsewhere."""
    if isinstance(act, torch.nn.GELU):
        return getattr(act, "approximate", "none") == "tanh"
    fn = getattr(act, "act", None)
    return (type(act).__name__ in ("GELUTanh", "PytorchGELUTanh") and getattr(fn, "func", None) is torch.nn.functional.gelu
            and getattr(fn, "keywords", None) == {"approximate": "tanh"})


def use_geglu_kernel(model: torch.nn.Module) -> int:
    """Patch the Gemma-family `*MLP` modules (GemmaMLP, Gemma2MLP, Gemma3MLP: the same forward text) that are
    down(act(gate(x)) * up(x)) with act = tanh-GELU to evaluate gelu_tanh(gate) * up through `dalm_geglu_{fwd,bwd}`: 2 eager
    launches forward and ~5 backward become 1 + 1 and the [tokens, intermediate] activation is recomputed instead of saved.
    Same rounding points as the eager chain.  DALM_SWIGLU_KERNEL=0 disables; returns how many modules were patched."""
    if _off("DALM_SWIGLU_KERNEL"):
        return 0

    def gated_tanh_gelu(mod) -> bool:
        return all(hasattr(mod, a) for a in ("gate_proj", "up_proj", "down_proj")) and _is_tanh_gelu(getattr(mod, "act_fn", None))

    return _install(model, ("GemmaMLP", "Gemma2MLP", "Gemma3MLP"), gated_tanh_gelu,
                    lambda mod: _mlp_matches(mod, _geglu_mlp_forward, "down(gelu_tanh(gate(x)) * up(x)) here"), _geglu_mlp_forward)


# ---------------------------------------------------------------------------
# Arcee (AFM): the ungated ReLU^2 MLP; attention, norm and decoder layer are Llama's (`_llama_attention_forward`, `_llama_layer_forward`)
# ---------------------------------------------------------------------------
def _relu2_mlp_forward(self, x):
    from . import frozen_linear, tower_ops

    out = frozen_linear.relu2_mlp_forward(x, self.up_proj, self.down_proj)   # padded step, both frozen: one node
    if out is not None:
        return out
    y = self.up_proj(x)
    if tower_ops.relu2_supported(y):
        return self.down_proj(tower_ops.relu2(y))
    return self.down_proj(self.act_fn(y))


def use_relu2_kernel(model: torch.nn.Module) -> int:
    """Patch the bias-free `ArceeMLP` modules that are down(act(up(x))) with act = transformers' ReLUSquaredActivation
    (square(relu(x))) and no gate to evaluate relu(up)^2 through `dalm_relu2_{fwd,bwd}`: 2 eager launches forward and ~4 backward become 1 + 1, and nothing
    but the up projection's output is saved.  Same rounding points as the eager chain.  DALM_SWIGLU_KERNEL=0 disables; returns how
    many modules were patched."""
    if _off("DALM_SWIGLU_KERNEL"):
        return 0

    def ungated_relu2(mod) -> bool:
        return (all(hasattr(mod, a) for a in ("up_proj", "down_proj")) and not hasattr(mod, "gate_proj")
                and mod.up_proj.bias is None and mod.down_proj.bias is None          # AFM is bias-free: `mlp_bias` stays transformers'
                and type(getattr(mod, "act_fn", None)).__name__ == "ReLUSquaredActivation")

    return _install(model, ("ArceeMLP",), ungated_relu2,
                    lambda mod: _mlp_matches(mod, _relu2_mlp_forward, "down(relu(up(x))^2) here", first="up_proj"), _relu2_mlp_forward)


def _gemma_norm_formula(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    xf = x.float()
    return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * (1.0 + w.float())).type_as(x)


def _gemma_eps(mod) -> float:
    return float(getattr(mod, "eps", getattr(mod, "variance_epsilon", None)))


def _gemma_norm_forward(self, x: torch.Tensor) -> torch.Tensor:
    from . import tower_ops

    if tower_ops.gemma_rms_norm_supported(x, self.weight):
        return tower_ops.gemma_add_rms_norm(x, None, self.weight, _gemma_eps(self))[1]
    return _gemma_norm_formula(x, self.weight, _gemma_eps(self))


def _gemma_norm_matches(mod: torch.nn.Module) -> bool:
    """The module's OWN forward against the patched one (the formula above; on a GPU the HIP kernel) on a small random tensor, once
    per class, dtype and device type: what tells GemmaRMSNorm from a `*RMSNorm` of the same name with another formula.  On a GPU
    an f32 weight is probed under f32 AND bf16 activations: under autocast the kernel sees the latter.  Leaves `mod` as it is."""
    w = mod.weight

    def probe():
        g = torch.Generator().manual_seed(0)
        x = torch.randn(4, 3, w.shape[0], generator=g)
        # at the zero initialisation (1 + w) is 1 and tells nothing: the probe runs on a twin of the module with a weight of its own
        twin = copy.copy(mod)
        twin._parameters = dict(mod._parameters)
        twin.weight = torch.nn.Parameter((0.5 * torch.randn(w.shape, generator=g)).to(device=w.device, dtype=w.dtype), requires_grad=False)
        x_dtypes = {w.dtype, torch.bfloat16} if w.is_cuda else {w.dtype}
        with torch.no_grad():
            return all(_close(_gemma_norm_forward(twin, xd), type(mod).forward(twin, xd), 2.0)
                       for xd in (x.to(device=w.device, dtype=dt) for dt in sorted(x_dtypes, key=str)))

    return _guard(("gemma-norm", type(mod), w.dtype, w.device.type), type(mod).__name__ + ".forward",
                  "(x.float() * rsqrt(mean(x.float()^2) + eps) * (1 + w.float())).type_as(x) here", probe)


def _gemma_rms_norm(mod) -> bool:
    w = getattr(mod, "weight", None)
    return w is not None and w.dim() == 1 and getattr(mod, "eps", getattr(mod, "variance_epsilon", None)) is not None


def use_gemma_rms_norm(model: torch.nn.Module) -> int:
    """Patch GemmaRMSNorm modules - and Gemma2RMSNorm / Gemma3RMSNorm where their own forward passes the same value probe - to run
    on `dalm_gemma_norm_{fwd,bwd}`: one launch each way instead of transformers' f32 chain of ~8.  DALM_NORM_KERNEL=0 disables;
    returns how many modules were patched."""
    if _off("DALM_NORM_KERNEL"):
        return 0
    return _install(model, ("GemmaRMSNorm", "Gemma2RMSNorm", "Gemma3RMSNorm"), _gemma_rms_norm, _gemma_norm_matches, _gemma_norm_forward)


# ---------------------------------------------------------------------------
# Falcon multi-query attention: make the head split capturable
# ---------------------------------------------------------------------------
def _split_heads_sliced(self, fused_qkv: torch.Tensor):
    """Falcon-7B layout [.., num_heads + 2, head_dim]: queries, then ONE shared key head and ONE shared value head.
    transformers picks the two shared heads with python-list indices (`x[..., [-2], :]`), which builds an index
    tensor on the host and copies it to the device on every call - an operation a hipGraph capture refuses.  Plain
    slices select the same elements (as views) with no host work."""
    b, t, _ = fused_qkv.shape
    x = fused_qkv.view(b, t, self.num_heads + 2, self.head_dim)
    n = self.num_heads
    return x[..., :n, :], x[..., n:n + 1, :], x[..., n + 1:, :]


def use_capturable_falcon_heads(model: torch.nn.Module) -> int:
    """Patch FalconAttention modules of the 7B flavour (multi_query, old decoder architecture); returns the count.

    The module's `num_kv_heads` is NOT touched (round 5 set it to `num_heads` so that SDPA saw equal head counts,
    which also made every reader outside the training call - the KV cache of eval / generate, export, sharding - see 71 key /
    value heads).  The broadcast of the shared key / value head happens inside the patched TRAINING call only
    (`_falcon_attention_forward`, `layer_past is None`); `_dalm_expand_kv` merely says that call may do it."""
    n = 0
    for mod in model.modules():
        if type(mod).__name__ != "FalconAttention":
            continue
        if getattr(mod, "new_decoder_architecture", False) or not getattr(mod, "multi_query", False):
            continue
        mod._split_heads = types.MethodType(_split_heads_sliced, mod)
        # multi-query + SDPA with [B, 1, T, hd] keys falls back to torch's unfused "math" path - f32 scores, softmax, masks:
        # ~1.5 ms per layer at cfg5, 48 ms of a 230 ms step (profiles/r05cfg5_step_by_stream_before.txt).
        mod._dalm_expand_kv = (getattr(mod, "num_kv_heads", None) == 1
                               and getattr(getattr(mod, "config", None), "_attn_implementation", None) == "sdpa")
        n += 1
    return n


# ---------------------------------------------------------------------------
# Falcon decoder layer (7B flavour: parallel attention, one LayerNorm, no dropout): LayerNorm, GELU and the residual adds
# ---------------------------------------------------------------------------
_FALCON_LAYER_PARAMS = ["self", "hidden_states", "alibi", "attention_mask", "position_ids", "layer_past", "use_cache",
                        "output_attentions", "position_embeddings", "kwargs"]


def _falcon_mlp_forward(self, x):
    from . import tower_ops

    h = self.dense_h_to_4h(x)
    if tower_ops.flat_bf16_supported(h):
        return self.dense_4h_to_h(tower_ops.gelu(h))
    return self.dense_4h_to_h(self.act(h))


def _falcon_layer_forward(self, hidden_states, alibi, attention_mask, position_ids=None, layer_past=None, use_cache=False,
                          output_attentions=False, position_embeddings=None, **kwargs):
    """transformers' FalconDecoderLayer.forward for `parallel_attn` without the new decoder architecture and without dropout:
        ln = input_layernorm(x);  out = x + (mlp(ln) + attention(ln))
    with the LayerNorm on `dalm_layer_norm_{fwd,bwd}` (under bf16 autocast the eager form is two up-casts, an f32 LayerNorm and
    two down-casts forward, and the same again backward) and the two adds on `dalm_add3`.  The backward kernel of the norm also
    adds the gradient that reaches x through the residual path."""
    from . import tower_ops

    ln = self.input_layernorm
    if not tower_ops.layer_norm_supported(hidden_states, ln.weight, ln.bias):
        return self._dalm_orig_forward(hidden_states, alibi, attention_mask, position_ids=position_ids, layer_past=layer_past,
                                       use_cache=use_cache, output_attentions=output_attentions,
                                       position_embeddings=position_embeddings, **kwargs)
    residual, normed = tower_ops.layer_norm_res(hidden_states, ln.weight, ln.bias, ln.eps)
    attn_out, attn_weights = self.self_attention(normed, layer_past=layer_past, attention_mask=attention_mask,
                                                 position_ids=position_ids, alibi=alibi, use_cache=use_cache,
                                                 output_attentions=output_attentions, position_embeddings=position_embeddings)
    mlp_out = self.mlp(normed)
    if tower_ops.flat_bf16_supported(mlp_out, attn_out, residual):
        return tower_ops.add3(mlp_out, attn_out, residual), attn_weights
    mlp_out = mlp_out + attn_out
    return residual + mlp_out, attn_weights


def use_falcon_layer_kernels(model: torch.nn.Module) -> int:
    """Patch FalconDecoderLayer / FalconMLP modules of the 7B flavour whose code is the one this file was written against
    (signature and source checked once per class).  DALM_FALCON_KERNELS=0 disables.  Returns how many layers were patched."""
    if _off("DALM_FALCON_KERNELS"):
        return 0

    def plain_7b_layer(mod) -> bool:
        cfg, ln = getattr(mod, "config", None), getattr(mod, "input_layernorm", None)
        return (cfg is not None and not getattr(cfg, "new_decoder_architecture", True) and getattr(cfg, "parallel_attn", False)
                # dropout_add with p > 0 draws from torch's generator: transformers' code stays
                and float(getattr(cfg, "hidden_dropout", 1.0)) == 0.0 and float(getattr(cfg, "attention_dropout", 1.0)) == 0.0
                and isinstance(ln, torch.nn.LayerNorm) and ln.weight is not None and hasattr(mod, "self_attention")
                and hasattr(mod, "mlp"))

    n = _install(model, ("FalconDecoderLayer",), plain_7b_layer, "falcon-layer", _falcon_layer_forward, keep="_dalm_orig_forward")
    for layer in model.modules():                  # the MLP of a patched layer
        if getattr(layer.forward, "__func__", None) is _falcon_layer_forward:
            _install(layer.mlp, ("FalconMLP",), lambda mlp: _is_erf_gelu(getattr(mlp, "act", None)), "falcon-mlp", _falcon_mlp_forward)
    return n


def _is_erf_gelu(act) -> bool:
    """torch's exact GELU: nn.GELU() or transformers' GELUActivation around nn.functional.gelu (config.activation = "gelu")."""
    if isinstance(act, torch.nn.GELU):
        return getattr(act, "approximate", "none") == "none"
    return type(act).__name__ == "GELUActivation" and getattr(act, "act", None) is torch.nn.functional.gelu


_SOURCE_GUARDS["falcon-layer"] = (_restates(
    _FALCON_LAYER_PARAMS,
    "attention_layernorm_out = self.input_layernorm(hidden_states)",
    "mlp_layernorm_out = attention_layernorm_out",
    "mlp_output = self.mlp(mlp_layernorm_out)",
    "mlp_output += attention_output",
    "output = dropout_add(mlp_output, residual, self.config.hidden_dropout, training=self.training)",
    "return output, attn_weights"), _RESTATED)
_SOURCE_GUARDS["falcon-mlp"] = (
    lambda params, src: ("x = self.act(self.dense_h_to_4h(x))" in src and "x = self.dense_4h_to_h(x)" in src
                         and src.count("self.") == 3), "dense_4h_to_h(act(dense_h_to_4h(x))) here")


# ---------------------------------------------------------------------------
# BERT encoder layer: dropout + residual add + LayerNorm of BertSelfOutput / BertOutput in one launch each way
# ---------------------------------------------------------------------------
def _bert_output_forward(self, hidden_states: torch.Tensor, input_tensor: torch.Tensor) -> torch.Tensor:
    """transformers' BertSelfOutput.forward / BertOutput.forward (the same three statements):
        hidden_states = self.dense(hidden_states); hidden_states = self.dropout(hidden_states)
        hidden_states = self.LayerNorm(hidden_states + input_tensor)
    with the last two on `dalm_bert_add_norm_{fwd,bwd}` where the tensors are what bf16 autocast over a frozen base produces
    (bf16 dense output, f32 residual); everything else runs the statements as they are."""
    from . import bert_ops
    from .lora import dropout_salt

    hidden_states = self.dense(hidden_states)
    if bert_ops.supported(hidden_states, input_tensor, self.LayerNorm):
        p = float(self.dropout.p) if self.training else 0.0
        return bert_ops.add_norm(hidden_states, input_tensor, self.LayerNorm, p, dropout_salt(self, "_dalm_calls"))
    hidden_states = self.dropout(hidden_states)
    return self.LayerNorm(hidden_states + input_tensor)


# BertSelfOutput / BertOutput and the classes of the RoBERTa family whose forward is the same three statements (xlm-roberta-xl's
# `XLMRobertaXL*` classes are other code - no LayerNorm in the self-output - and are not named)
_BERT_OUTPUT_CLASSES = tuple(f"{family}{kind}" for family in ("Bert", "Roberta", "XLMRoberta", "Camembert")
                             for kind in ("SelfOutput", "Output")) + ("MPNetOutput",)      # MPNetOutput: "Copied from" BertOutput


def use_bert_layer_kernels(model: torch.nn.Module) -> int:
    """Patch {Bert,Roberta,XLMRoberta,Camembert}{SelfOutput,Output} and MPNetOutput modules whose forward is the three statements
    above (source checked once per class), and MPNetAttention modules (`_mpnet_attention_forward`: the same dropout + add +
    LayerNorm behind the self-attention).  The kernel runs where the LayerNorm is frozen.  Returns how many modules were patched."""
    def dense_dropout_norm(mod) -> bool:
        return (isinstance(getattr(mod, "LayerNorm", None), torch.nn.LayerNorm)
                and isinstance(getattr(mod, "dropout", None), torch.nn.Dropout) and hasattr(mod, "dense"))

    def dropout_norm(mod) -> bool:                # MPNetAttention: the same statement without a dense of its own
        return (isinstance(getattr(mod, "LayerNorm", None), torch.nn.LayerNorm)
                and isinstance(getattr(mod, "dropout", None), torch.nn.Dropout) and hasattr(mod, "attn"))

    return (_install(model, _BERT_OUTPUT_CLASSES, dense_dropout_norm, "bert-output", _bert_output_forward)
            + _install(model, ("MPNetAttention",), dropout_norm, "mpnet-attn", _mpnet_attention_forward))


_SOURCE_GUARDS["bert-output"] = (
    lambda params, src: (params == ["self", "hidden_states", "input_tensor"]
                         and _body(src)[1:] == ["hidden_states = self.dense(hidden_states)", "hidden_states = self.dropout(hidden_states)",
                                                "hidden_states = self.LayerNorm(hidden_states + input_tensor)", "return hidden_states"]),
    "dense -> dropout -> LayerNorm(h + input) here")


# ---------------------------------------------------------------------------
# RoBERTa-family embeddings: positions from the ids + three table rows + LayerNorm + dropout in one launch (forward only)
# ---------------------------------------------------------------------------
_ROBERTA_EMBEDDINGS_PARAMS = ["self", "input_ids", "token_type_ids", "position_ids", "inputs_embeds", "past_key_values_length"]


def _roberta_embeddings_forward(self, input_ids=None, token_type_ids=None, position_ids=None, inputs_embeds=None,
                                past_key_values_length=0):
    """transformers' {Roberta,XLMRoberta,Camembert}Embeddings.forward:
        position_ids = create_position_ids_from_input_ids(input_ids, self.padding_idx)     (when none are given)
        token_type_ids = the all-zero buffer                                               (when none are given)
        embeddings = (word_embeddings(input_ids) + token_type_embeddings(token_type_ids)) + position_embeddings(position_ids)
        embeddings = self.dropout(self.LayerNorm(embeddings))
    as `dalm_embed_norm_fwd` where the three tables and the LayerNorm are frozen f32 / bf16-autocast GPU tensors
    (`bert_ops.embed_supported`); every other call runs the module's own statements.  BertEmbeddings is NOT patched: its dropout
    would draw another mask than today's."""
    from . import bert_ops
    from .lora import dropout_salt

    if bert_ops.embed_supported(self, input_ids, token_type_ids, position_ids, inputs_embeds, past_key_values_length):
        p = float(self.dropout.p) if self.training else 0.0
        return bert_ops.embed_norm(self, input_ids, token_type_ids, position_ids, p, dropout_salt(self, "_dalm_calls"))
    return self._dalm_orig_forward(input_ids=input_ids, token_type_ids=token_type_ids, position_ids=position_ids,
                                   inputs_embeds=inputs_embeds, past_key_values_length=past_key_values_length)


def use_roberta_embeddings(model: torch.nn.Module) -> int:
    """Patch {Roberta,XLMRoberta,Camembert}Embeddings modules whose forward is the code `_roberta_embeddings_forward` restates
    (signature and statements checked once per class).  Returns the count."""
    def three_tables(mod) -> bool:
        return (all(isinstance(getattr(mod, a, None), torch.nn.Embedding)
                    for a in ("word_embeddings", "token_type_embeddings", "position_embeddings"))
                and isinstance(getattr(mod, "LayerNorm", None), torch.nn.LayerNorm)
                and isinstance(getattr(mod, "dropout", None), torch.nn.Dropout) and isinstance(getattr(mod, "padding_idx", None), int))

    def guard(mod) -> bool:
        cls = type(mod)
        return _matches("roberta-embeddings", cls) and _guard(
            ("roberta-positions", cls), cls.__name__ + ".create_position_ids_from_input_ids",
            "padding_idx + cumsum(ids != padding_idx) * (ids != padding_idx) here", lambda: _roberta_positions_match(cls))

    return _install(model, ("RobertaEmbeddings", "XLMRobertaEmbeddings", "CamembertEmbeddings"), three_tables, guard,
                    _roberta_embeddings_forward, keep="_dalm_orig_forward")


def _roberta_positions_match(cls) -> bool:
    """The class's create_position_ids_from_input_ids IS the rule the kernel and `packed.packed_positions` restate."""
    import inspect

    src = inspect.getsource(cls.create_position_ids_from_input_ids)
    return all(s in src for s in ("mask = input_ids.ne(padding_idx).int()",
                                  "incremental_indices = (torch.cumsum(mask, dim=1).type_as(mask) + past_key_values_length) * mask",
                                  "return incremental_indices.long() + padding_idx"))


_ROBERTA_EMBEDDINGS_BODY = [
    "if token_type_ids is None:", 'if hasattr(self, "token_type_ids"):',
    "buffered_token_type_ids = self.token_type_ids.to(position_ids.device).expand(position_ids.shape[0], -1)",
    "buffered_token_type_ids = torch.gather(buffered_token_type_ids, dim=1, index=position_ids)",
    "token_type_ids = buffered_token_type_ids.expand(batch_size, seq_length)", "else:",
    "token_type_ids = torch.zeros(input_shape, dtype=torch.long, device=self.position_ids.device)",
    "if inputs_embeds is None:", "inputs_embeds = self.word_embeddings(input_ids)",
    "token_type_embeddings = self.token_type_embeddings(token_type_ids)", "embeddings = inputs_embeds + token_type_embeddings",
    "position_embeddings = self.position_embeddings(position_ids)", "embeddings = embeddings + position_embeddings",
    "embeddings = self.LayerNorm(embeddings)", "embeddings = self.dropout(embeddings)", "return embeddings"]
_SOURCE_GUARDS["roberta-embeddings"] = (
    lambda params, src: (params == _ROBERTA_EMBEDDINGS_PARAMS
                         and _body(src)[-len(_ROBERTA_EMBEDDINGS_BODY):] == _ROBERTA_EMBEDDINGS_BODY
                         and "position_ids = self.create_position_ids_from_input_ids(" in src
                         and "input_ids, self.padding_idx, past_key_values_length" in src), _RESTATED)


# ---------------------------------------------------------------------------
# Falcon attention (7B flavour, rotary, sdpa): the attention itself on dalm_attn_fwd / dalm_attn_bwd
# ---------------------------------------------------------------------------
_FALCON_ATTN_PARAMS = ["self", "hidden_states", "alibi", "attention_mask", "position_ids", "layer_past", "use_cache",
                       "output_attentions", "position_embeddings", "kwargs"]


def _falcon_attention_forward(self, hidden_states, alibi, attention_mask, position_ids=None, layer_past=None, use_cache=False,
                              output_attentions=False, position_embeddings=None, **kwargs):
    """transformers' FalconAttention.forward for the training call (rotary positions, no KV cache, "sdpa"): the same statements
    with F.scaled_dot_product_attention replaced by `attention.sdpa` (dalm_amd/csrc/attn.hip).  Every other call goes to
    transformers' own forward."""
    import importlib

    from . import attention

    orig = self._dalm_orig_attn_forward
    if (alibi is not None or layer_past is not None or output_attentions or position_embeddings is None
            or getattr(self.config, "_attn_implementation", None) != "sdpa" or _off("DALM_ATTN_KERNEL")):
        return orig(hidden_states, alibi, attention_mask, position_ids=position_ids, layer_past=layer_past, use_cache=use_cache,
                    output_attentions=output_attentions, position_embeddings=position_embeddings, **kwargs)
    fused_qkv = self.query_key_value(hidden_states)
    num_kv_heads = self.num_heads if self.new_decoder_architecture else self.num_kv_heads
    query_layer, key_layer, value_layer = self._split_heads(fused_qkv)
    batch_size, query_length, _, _ = query_layer.shape
    cos, sin = position_embeddings
    is_causal = bool(self.is_causal and attention_mask is None and query_length > 1)
    rope_on = not _off("DALM_FAST_ROPE")
    mqa = bool(getattr(self, "_dalm_expand_kv", False) and num_kv_heads == 1 and key_layer.shape[2] == 1)
    if mqa and rope_on:
        # multi-query, THIS call only (training, no KV cache): the ONE shared key / value head stays one head in memory.  The
        # rotation runs on the single key head, the attention kernels read key / value through stride-0 head views (every head
        # the same rows, served by the caches) - the 71 copies of K and V that the broadcast-then-reshape form materialises per
        # layer (2 x 93 us at cfg5, profiles/r06cfg5packed_step_by_stream.txt) never exist; dk / dv are summed over the heads
        # after the backward kernels, as autograd's expand backward would
        H, hd = self.num_heads, self.head_dim
        q4 = query_layer.transpose(1, 2).reshape(batch_size, H, query_length, hd)
        k1, v1 = key_layer.transpose(1, 2), value_layer.transpose(1, 2)                      # [b, 1, t, hd] views of fused_qkv
        kx, vx = k1.expand(batch_size, H, query_length, hd), v1.expand(batch_size, H, query_length, hd)
        seqs = attention.packed_of(attention_mask)
        # `node_supported` also asks for grouped heads; k / v reach it with H heads here (with H or one below), and a group needs
        # 1 < Hkv < H: for Falcon it is `packed_supported` / `supported` alone
        if attention.node_supported(q4, kx, vx, attention_mask, is_causal) and attention.rope_fusable(q4, k1, cos, sin):
            attn_output = attention.rope_sdpa(q4, k1, v1, cos, sin, attention_mask, float(hd) ** -0.5,
                                              False if seqs is not None else is_causal)
            attn_output = attn_output.permute(0, 2, 1, 3).reshape(batch_size, query_length, H * hd)
            return self.dense(attn_output), None
    if mqa:
        # the one shared key / value head broadcast to the query heads (views; the reshape below materialises them) - equal head
        # counts for the kernels and for torch's fused SDPA
        key_layer = key_layer.expand(batch_size, query_length, self.num_heads, self.head_dim)
        value_layer = value_layer.expand(batch_size, query_length, self.num_heads, self.head_dim)
        num_kv_heads = self.num_heads
    query_layer = query_layer.transpose(1, 2).reshape(batch_size, self.num_heads, query_length, self.head_dim)
    key_layer = key_layer.transpose(1, 2).reshape(batch_size, num_kv_heads, query_length, self.head_dim)
    value_layer = value_layer.transpose(1, 2).reshape(batch_size, num_kv_heads, query_length, self.head_dim)
    seqs = attention.packed_of(attention_mask)
    fused = (rope_on and attention.node_supported(query_layer, key_layer, value_layer, attention_mask, is_causal)
             and attention.rope_fusable(query_layer, key_layer, cos, sin))
    if seqs is not None:
        # packed (un-padded) call (dalm_amd/packed.py): [1, H, n, hd], sequences from the descriptor
        if fused:
            attn_output = attention.rope_sdpa(query_layer, key_layer, value_layer, cos, sin, attention_mask,
                                              float(self.head_dim) ** -0.5, False)
            attn_output = attn_output.permute(0, 2, 1, 3)
        else:
            rope = importlib.import_module(type(self).__module__).apply_rotary_pos_emb
            query_layer, key_layer = rope(query_layer, key_layer, cos, sin)
            attn_output, _ = attention._packed_attention(self, query_layer, key_layer, value_layer, attention_mask, seqs, 0.0,
                                                         float(self.head_dim) ** -0.5)            # [1, n, H, hd]
        attn_output = attn_output.reshape(batch_size, query_length, self.num_heads * self.head_dim)
        return self.dense(attn_output), None
    if fused:
        attn_output = attention.rope_sdpa(query_layer, key_layer, value_layer, cos, sin, attention_mask,
                                          float(self.head_dim) ** -0.5, is_causal)     # the rotation's backward: in dalm_attn_bwd
        attn_output = attn_output.view(batch_size, self.num_heads, query_length, self.head_dim)
        attn_output = attn_output.permute(0, 2, 1, 3)
        attn_output = attn_output.reshape(batch_size, query_length, self.num_heads * self.head_dim)
        return self.dense(attn_output), None
    rope = importlib.import_module(type(self).__module__).apply_rotary_pos_emb        # the modeling file's own (maybe swapped) one
    query_layer, key_layer = rope(query_layer, key_layer, cos, sin)
    if not attention.supported(query_layer, key_layer, value_layer, attention_mask, 0.0, is_causal, {}):
        attn_output = torch.nn.functional.scaled_dot_product_attention(query_layer, key_layer, value_layer, attn_mask=attention_mask,
                                                                       dropout_p=0.0, is_causal=is_causal)
    else:
        attn_output = attention.sdpa(query_layer, key_layer, value_layer, attention_mask, float(self.head_dim) ** -0.5, is_causal)
    attn_output = attn_output.view(batch_size, self.num_heads, query_length, self.head_dim)
    attn_output = attn_output.permute(0, 2, 1, 3)
    attn_output = attn_output.reshape(batch_size, query_length, self.num_heads * self.head_dim)
    return self.dense(attn_output), None


def use_falcon_attention_kernels(model: torch.nn.Module) -> int:
    """Patch FalconAttention modules (head width 64 or 128, no alibi) whose forward is the code `_falcon_attention_forward`
    restates (signature and statements checked once per class).  DALM_ATTN_KERNEL=0 disables.  Returns the count."""
    if _off("DALM_ATTN_KERNEL"):
        return 0

    def rotary_no_dropout(mod) -> bool:
        cfg = getattr(mod, "config", None)
        return (getattr(mod, "head_dim", None) in (64, 128) and not getattr(cfg, "alibi", True)
                and float(getattr(cfg, "attention_dropout", 1.0)) == 0.0)

    return _install(model, ("FalconAttention",), rotary_no_dropout, "falcon-attn", _falcon_attention_forward,
                    keep="_dalm_orig_attn_forward")


_SOURCE_GUARDS["falcon-attn"] = (_restates(
    _FALCON_ATTN_PARAMS,
    "fused_qkv = self.query_key_value(hidden_states)",
    "(query_layer, key_layer, value_layer) = self._split_heads(fused_qkv)",
    "query_layer, key_layer = apply_rotary_pos_emb(query_layer, key_layer, cos, sin)",
    "is_causal = self.is_causal and attention_mask is None and query_length > 1",
    "attn_output = attn_output.view(batch_size, self.num_heads, query_length, self.head_dim)",
    "attn_output = attn_output.permute(0, 2, 1, 3)",
    "attn_output = self.dense(attn_output)",
    "return attn_output, attention_scores"), _RESTATED)


# ---------------------------------------------------------------------------
# MPNet (all-mpnet-base-v2, multi-qa-mpnet-*, paraphrase-mpnet-*): the self-attention on dalm_attn_rel_* with the relative-position
# bias as ONE small vector per forward, and MPNetAttention's dropout + add + LayerNorm on BERT's kernel
# ---------------------------------------------------------------------------
_MPNET_ATTN_PARAMS = ["self", "hidden_states", "attention_mask", "position_bias", "output_attentions", "kwargs"]


def _mpnet_self_attention_forward(self, hidden_states, attention_mask=None, position_bias=None, output_attentions=False, **kwargs):
    """transformers' MPNetSelfAttention.forward: the q / k / v projections, softmax(q k^T / sqrt(hd) + position_bias +
    attention_mask), dropout, the product with v, `o` - with everything between the projections and `o` as `attention.rel_sdpa`
    when `position_bias` is the routed encoder's tagged stand-in.  A real bias tensor (an unrouted encoder, explicit position ids)
    or `output_attentions` runs transformers' own forward."""
    from . import attention

    source = attention.rel_source_of(position_bias)
    if source is None or output_attentions:
        if source is not None:
            if attention.packed_of(attention_mask) is not None:
                raise ValueError("dalm_amd: a packed MPNet call returns no attention probabilities (output_attentions)")
            _warn_once("mpnet-output-attentions", "MPNet with output_attentions runs transformers' eager attention")
            position_bias = source.encoder._dalm_orig_compute_position_bias(hidden_states)
        return self._dalm_orig_attn_forward(hidden_states, attention_mask, position_bias, output_attentions=output_attentions, **kwargs)
    input_shape = hidden_states.shape[:-1]
    hidden_shape = (*input_shape, -1, self.attention_head_size)
    q = self.q(hidden_states).view(hidden_shape).transpose(1, 2)
    k = self.k(hidden_states).view(hidden_shape).transpose(1, 2)
    v = self.v(hidden_states).view(hidden_shape).transpose(1, 2)
    p = float(self.dropout.p) if self.training else 0.0
    c = attention.rel_sdpa(self, q, k, v, source, attention_mask, p)                       # [B, H, T, hd]
    c = c.permute(0, 2, 1, 3).contiguous()
    new_c_shape = c.size()[:-2] + (self.all_head_size,)
    c = c.view(*new_c_shape)
    o = self.o(c)
    return (o,)


_SOURCE_GUARDS["mpnet-self-attn"] = (_restates(
    _MPNET_ATTN_PARAMS,
    "hidden_shape = (*input_shape, -1, self.attention_head_size)",
    "q = self.q(hidden_states).view(hidden_shape).transpose(1, 2)",
    "k = self.k(hidden_states).view(hidden_shape).transpose(1, 2)",
    "v = self.v(hidden_states).view(hidden_shape).transpose(1, 2)",
    "attention_scores = torch.matmul(q, k.transpose(-1, -2))",
    "attention_scores = attention_scores / math.sqrt(self.attention_head_size)",
    "attention_scores += position_bias",
    "attention_scores = attention_scores + attention_mask",
    "attention_probs = nn.functional.softmax(attention_scores, dim=-1)",
    "attention_probs = self.dropout(attention_probs)",
    "c = torch.matmul(attention_probs, v)",
    "c = c.permute(0, 2, 1, 3).contiguous()",
    "o = self.o(c)",
    "outputs = (o, attention_probs) if output_attentions else (o,)"), _RESTATED)


def _mpnet_compute_position_bias(self, x, position_ids=None, num_buckets=32):
    """transformers' MPNetEncoder.compute_position_bias for the call the encoder makes (`compute_position_bias(hidden_states)`:
    positions arange(T), so the bias depends on the head and the column difference only): returns the tagged stand-in
    (`attention.tag_rel_bias`) from which the routed self-attention modules build ONE [H, 2 Tc - 1] vector per forward - no
    [B, H, T, T] tensor.  Explicit `position_ids`, another bucket count or a table that has become trainable: the class's code."""
    from . import attention

    if position_ids is not None or num_buckets != 32 or self.relative_attention_bias.weight.requires_grad:
        _warn_once("mpnet-bias-declined", "MPNet position bias from position_ids / a trainable table: transformers' own code")
        return self._dalm_orig_compute_position_bias(x, position_ids, num_buckets)
    return attention.tag_rel_bias(self)


def _mpnet_bias_matches(cls) -> bool:
    """The class's compute_position_bias / relative_position_bucket ARE what `_mpnet_compute_position_bias` and
    `attention.rel_bias_vector` stand for: positions arange(T) unless ids are given, key column - query column, the class's bucket
    function with `num_buckets`, one table row per bucket, [B, H, T, T]."""
    import inspect

    src = inspect.getsource(cls.compute_position_bias)
    params = list(inspect.signature(cls.compute_position_bias).parameters)
    dflt = inspect.signature(cls.compute_position_bias).parameters["num_buckets"].default
    return (params == ["self", "x", "position_ids", "num_buckets"] and dflt == 32
            and isinstance(inspect.getattr_static(cls, "relative_position_bucket"), staticmethod)
            and list(inspect.signature(cls.relative_position_bucket).parameters) == ["relative_position", "num_buckets", "max_distance"]
            and all(s in src for s in (
                "context_position = torch.arange(qlen, dtype=torch.long)[:, None]",
                "memory_position = torch.arange(klen, dtype=torch.long)[None, :]",
                "relative_position = memory_position - context_position",
                "rp_bucket = self.relative_position_bucket(relative_position, num_buckets=num_buckets)",
                "values = self.relative_attention_bias(rp_bucket)",
                "values = values.permute([2, 0, 1]).unsqueeze(0)",
                "values = values.expand((bsz, -1, qlen, klen)).contiguous()")))


def use_mpnet_attention_kernels(model: torch.nn.Module) -> int:
    """Route MPNet encoders: every MPNetSelfAttention module (head width 64, forward = the code `_mpnet_self_attention_forward`
    restates) and the encoder's compute_position_bias (source checked, table frozen) - all of an encoder or nothing, because the
    routed modules exchange a stand-in for the bias that transformers' own forward cannot read.  The model stays on "eager";
    `packed.attention_is_packable` recognises the routed modules.  DALM_ATTN_KERNEL=0 disables.  Returns the number of modules
    patched (self-attention modules + encoders)."""
    if _off("DALM_ATTN_KERNEL"):
        return 0
    n = 0
    for enc in [m for m in model.modules() if type(m).__name__ == "MPNetEncoder"]:
        cls = type(enc)
        table = getattr(enc, "relative_attention_bias", None)
        att = [m for m in enc.modules() if "MPNetSelfAttention" in [c.__name__ for c in type(m).__mro__]]
        if not isinstance(table, torch.nn.Embedding) or not att:
            continue
        if table.weight.requires_grad:
            _warn_once("mpnet-trainable-table", "MPNet's relative_attention_bias table is trainable: transformers' own attention stays")
            continue
        if any(getattr(m, "attention_head_size", None) != 64 for m in att):
            _warn_once("mpnet-head-width", "MPNet head width is not 64: transformers' own attention stays")
            continue
        if not _guard(("mpnet-bias", cls), cls.__name__ + ".compute_position_bias", _RESTATED, lambda: _mpnet_bias_matches(cls)):
            continue
        if not all(_matches("mpnet-self-attn", type(m)) for m in att):
            continue
        for m in att:
            m._dalm_orig_attn_forward = m.forward
            m.forward = types.MethodType(_mpnet_self_attention_forward, m)
        enc._dalm_orig_compute_position_bias = enc.compute_position_bias
        enc.compute_position_bias = types.MethodType(_mpnet_compute_position_bias, enc)
        n += len(att) + 1
    return n


def _mpnet_attention_forward(self, hidden_states, attention_mask=None, position_bias=None, output_attentions=False, **kwargs):
    """transformers' MPNetAttention.forward:
        self_outputs = self.attn(hidden_states, attention_mask, position_bias, output_attentions=output_attentions)
        attention_output = self.LayerNorm(self.dropout(self_outputs[0]) + hidden_states)
    with the second statement on `dalm_bert_add_norm_{fwd,bwd}` where `bert_ops.supported` holds (as `_bert_output_forward`)."""
    from . import bert_ops
    from .lora import dropout_salt

    self_outputs = self.attn(hidden_states, attention_mask, position_bias, output_attentions=output_attentions)
    if bert_ops.supported(self_outputs[0], hidden_states, self.LayerNorm):
        p = float(self.dropout.p) if self.training else 0.0
        attention_output = bert_ops.add_norm(self_outputs[0], hidden_states, self.LayerNorm, p, dropout_salt(self, "_dalm_calls"))
    else:
        attention_output = self.LayerNorm(self.dropout(self_outputs[0]) + hidden_states)
    outputs = (attention_output,) + self_outputs[1:]
    return outputs


_SOURCE_GUARDS["mpnet-attn"] = (
    lambda params, src: (params == _MPNET_ATTN_PARAMS and _body(src)[-9:] == [
        "self_outputs = self.attn(", "hidden_states,", "attention_mask,", "position_bias,", "output_attentions=output_attentions,", ")",
        "attention_output = self.LayerNorm(self.dropout(self_outputs[0]) + hidden_states)",
        "outputs = (attention_output,) + self_outputs[1:]  # add attentions if we output them", "return outputs"]
                         and src.count("self.") == 3), _RESTATED)


# ---------------------------------------------------------------------------
# Llama / Qwen3 attention: (q_norm / k_norm over the head dimension +) rotary embedding + attention as ONE autograd node (the
# rotation's backward rides in dalm_attn_bwd's epilogues)
# ---------------------------------------------------------------------------
_LLAMA_ATTN_PARAMS = ["self", "hidden_states", "position_embeddings", "attention_mask", "past_key_values", "kwargs"]
_LLAMA_ATTN_STATEMENTS = ("value_states = self.v_proj(hidden_states).view(hidden_shape).transpose(1, 2)",
                          "query_states, key_states = apply_rotary_pos_emb(query_states, key_states, cos, sin)",
                          "dropout=0.0 if not self.training else self.attention_dropout",
                          "scaling=self.scaling",
                          "attn_output = attn_output.reshape(*input_shape, -1).contiguous()",
                          "attn_output = self.o_proj(attn_output)")
_SOURCE_GUARDS["llama-attn"] = (_restates(
    _LLAMA_ATTN_PARAMS,
    "query_states = self.q_proj(hidden_states).view(hidden_shape).transpose(1, 2)",
    "key_states = self.k_proj(hidden_states).view(hidden_shape).transpose(1, 2)",
    *_LLAMA_ATTN_STATEMENTS), _RESTATED)
_SOURCE_GUARDS["qwen3-attn"] = (_restates(
    _LLAMA_ATTN_PARAMS,
    "query_states = self.q_norm(self.q_proj(hidden_states).view(hidden_shape)).transpose(1, 2)",
    "key_states = self.k_norm(self.k_proj(hidden_states).view(hidden_shape)).transpose(1, 2)",
    "sliding_window=self.sliding_window",
    *_LLAMA_ATTN_STATEMENTS), _RESTATED)


def _norm_eps(norm) -> float:
    return float(getattr(norm, "_dalm_eps", getattr(norm, "variance_epsilon", getattr(norm, "eps", 1e-6))))


def _qk_norm_ok(norm, row_wide: bool, width: int) -> bool:
    """The q_norm / k_norm the fused node stands for, by class name, with a plain weight [width] - its own forward, or
    `_native_forward` (`use_native_rms_norm`, the same formula behind its own run-time guard):
      Qwen3RMSNorm over the head dimension            w * (x * rsqrt(mean(x^2) + eps)).to(dtype)
      Olmo2RMSNorm over all heads of a token (row_wide)   (w * (x * rsqrt(mean(x^2) + eps))).to(dtype)"""
    w = getattr(norm, "weight", None)
    return (type(norm).__name__ == ("Olmo2RMSNorm" if row_wide else "Qwen3RMSNorm") and w is not None and w.dim() == 1
            and w.shape[0] == width and (hasattr(norm, "variance_epsilon") or hasattr(norm, "_dalm_eps")))


def _decoder_attention_forward(self, hidden_states, position_embeddings, attention_mask, past_key_values, kwargs, norms, window,
                               row_wide=False, project=None):
    """transformers' LlamaAttention.forward / Qwen3Attention.forward / Olmo2Attention.forward for the training call ("dalm_sdpa", no
    KV cache, no dropout, no sliding window): the same statements with (the q / k norms +) apply_rotary_pos_emb + the attention call
    as one node.  Every other call goes to transformers' own forward.  The classes differ in
      norms     None, or (q_norm, k_norm) between the projections and the rotation;
      row_wide  where the norms act: on the head view, over the head dimension (Qwen3), or - True - on the projection's output in
                front of the head view, over all heads of a token (OLMo-2);
      window    the keyword Qwen3 adds to the attention call, `{"sliding_window": ...}`; `{}` for the others;
      project   None: q_proj / k_proj / v_proj; Phi-3: `project(self, hidden_states, hidden_shape)` -> (query_raw, key_raw,
                value_states) as column slices of the one qkv_proj output.  Only with it may the tables be narrower than the head
                (modeling_phi3.py's apply_rotary_pos_emb rotates the first cos.shape[-1] elements): `attention.rope_partial_sdpa`."""
    from . import attention, tower_ops

    cfg = self.config
    if (past_key_values is not None or position_embeddings is None or getattr(cfg, "_attn_implementation", None) != attention.NAME
            or (self.training and float(getattr(self, "attention_dropout", 0.0)) != 0.0)
            # Qwen3: any window; Phi-3 (`project`): one shorter than the keys - a longer one changes nothing
            or (window.get("sliding_window") is not None and (project is None or window["sliding_window"] < hidden_states.shape[-2]))
            or _off("DALM_FAST_ROPE") or _off("DALM_ATTN_KERNEL") or kwargs.get("output_attentions")):
        return self._dalm_orig_attn_forward(hidden_states, position_embeddings=position_embeddings, attention_mask=attention_mask,
                                            past_key_values=past_key_values, **kwargs)
    input_shape = hidden_states.shape[:-1]
    hidden_shape = (*input_shape, -1, self.head_dim)
    if project is None:
        query_raw = self.q_proj(hidden_states).view(hidden_shape)
        key_raw = self.k_proj(hidden_states).view(hidden_shape)
        value_states = self.v_proj(hidden_states).view(hidden_shape).transpose(1, 2)
    else:
        query_raw, key_raw, value_states = project(self, hidden_states, hidden_shape)
    cos, sin = position_embeddings
    q_t, k_t = query_raw.transpose(1, 2), key_raw.transpose(1, 2)          # [B, H, T, hd] views, in front of the norms
    causal = bool(q_t.shape[2] > 1 and attention_mask is None and getattr(self, "is_causal", True))
    # padded or packed (dalm_amd/packed.py: [1, H, n, hd] views, sequences from the descriptor), equal heads or grouped-query
    # heads left un-expanded: the same node
    if row_wide and q_t.is_cuda and q_t.dtype == torch.bfloat16:
        cos, sin = _tables_in_bf16(cos, sin)     # the node's tables; the fall-through below goes back to the module's own
    narrow = project is not None and cos.shape[-1] < self.head_dim         # a partial rotation: never the fused epilogue
    fused = (not narrow and attention.node_supported(q_t, k_t, value_states, attention_mask, causal)
             and attention.rope_fusable(q_t, k_t, cos, sin))
    partial = (narrow and norms is None and attention.node_supported(q_t, k_t, value_states, attention_mask, causal)
               and tower_ops.rope_partial_supported(q_t, k_t, cos, sin))
    qn, kn = norms or (None, None)
    if fused and norms is not None:
        wide = (q_t.shape[1] * self.head_dim, k_t.shape[1] * self.head_dim) if row_wide else (self.head_dim, self.head_dim)
        norm_rope_supported = tower_ops.row_norm_rope_supported if row_wide else tower_ops.head_norm_rope_supported
        fused = (_qk_norm_ok(qn, row_wide, wide[0]) and _qk_norm_ok(kn, row_wide, wide[1])
                 and norm_rope_supported(q_t, k_t, qn.weight, kn.weight, cos, sin))
    if fused and norms is None:
        attn_output = attention.rope_sdpa(q_t, k_t, value_states, cos, sin, attention_mask, float(self.scaling), causal)
    elif fused:
        attn_output = attention.norm_rope_sdpa(q_t, k_t, value_states, qn.weight, kn.weight, _norm_eps(qn), _norm_eps(kn), cos, sin,
                                               attention_mask, float(self.scaling), causal, row_wide)
    elif partial:
        attn_output = attention.rope_partial_sdpa(q_t, k_t, value_states, cos, sin, attention_mask, float(self.scaling), causal)
    else:                      # CPU tensors, fp32, one KV head, other head widths, ...: transformers' own sequence from here on
        import importlib

        from transformers.modeling_utils import ALL_ATTENTION_FUNCTIONS

        if norms is not None and row_wide:       # the norm of the projection's output ([.., H hd]: the view undone), then the head view
            q_t = qn(query_raw.flatten(-2)).view(hidden_shape).transpose(1, 2)
            k_t = kn(key_raw.flatten(-2)).view(hidden_shape).transpose(1, 2)
        elif norms is not None:
            q_t, k_t = qn(query_raw).transpose(1, 2), kn(key_raw).transpose(1, 2)
        rope = importlib.import_module(type(self).__module__).apply_rotary_pos_emb
        query_states, key_states = rope(q_t, k_t, *position_embeddings)
        attn_output, _ = ALL_ATTENTION_FUNCTIONS[cfg._attn_implementation](
            self, query_states, key_states, value_states, attention_mask, dropout=0.0, scaling=self.scaling, **window, **kwargs)
    if fused or partial:
        attn_output = attn_output.transpose(1, 2)
    attn_output = attn_output.reshape(*input_shape, -1).contiguous()
    return self.o_proj(attn_output), None


def _llama_attention_forward(self, hidden_states, position_embeddings=None, attention_mask=None, past_key_values=None, **kwargs):
    """LlamaAttention.forward: rotary + attention as `attention.rope_sdpa`."""
    return _decoder_attention_forward(self, hidden_states, position_embeddings, attention_mask, past_key_values, kwargs, None, {})


def _qwen3_attention_forward(self, hidden_states, position_embeddings=None, attention_mask=None, past_key_values=None, **kwargs):
    """Qwen3Attention.forward: q_norm + k_norm + rotary + attention as `attention.norm_rope_sdpa`."""
    return _decoder_attention_forward(self, hidden_states, position_embeddings, attention_mask, past_key_values, kwargs,
                                      (self.q_norm, self.k_norm), {"sliding_window": getattr(self, "sliding_window", None)})


def _tables_in_bf16(cos, sin):
    """Olmo2RotaryEmbedding hands every layer its tables in f32 (Llama's casts them to the activations' dtype itself) and
    apply_rotary_pos_emb then multiplies in f32.  The fused node - like the rotation's backward inside `dalm_attn_bwd` - reads bf16
    tables and rounds as Llama's chain does, so the routed OLMo-2 rotates with Llama's convention: tables rounded to bf16, ONCE per
    forward (every layer is handed the same two tensors; the copies ride on the cos tensor)."""
    if cos.dtype != torch.float32 or sin.dtype != torch.float32:
        return cos, sin
    got = getattr(cos, "_dalm_bf16", None)
    if got is None or got[0] is not sin or got[1] != (cos._version, sin._version):
        got = (sin, (cos._version, sin._version), cos.to(torch.bfloat16), sin.to(torch.bfloat16))
        cos._dalm_bf16 = got
    return got[2], got[3]


def _olmo2_attention_forward(self, hidden_states, position_embeddings=None, attention_mask=None, past_key_values=None, **kwargs):
    """Olmo2Attention.forward: q_norm + k_norm over the whole projection width + rotary + attention as `attention.norm_rope_sdpa`."""
    return _decoder_attention_forward(self, hidden_states, position_embeddings, attention_mask, past_key_values, kwargs,
                                      (self.q_norm, self.k_norm), {}, row_wide=True)


def _use_attention_node(model: torch.nn.Module, name: str, attrs: tuple, guard: str, forward, also=lambda mod: True) -> int:
    from . import attention

    if getattr(getattr(model, "config", None), "_attn_implementation", None) != attention.NAME:
        return 0
    return _install(model, (name,), lambda mod: all(hasattr(mod, a) for a in attrs) and also(mod), guard, forward,
                    keep="_dalm_orig_attn_forward")


_QKVO = ("q_proj", "k_proj", "v_proj", "o_proj")


def use_llama_attention_node(model: torch.nn.Module) -> int:
    """Patch LlamaAttention modules - and ArceeAttention and GraniteAttention ones, Llama's forward under the same source guard - of a
    model that runs on "dalm_sdpa" (models/attention.py) and whose forward is the code `_llama_attention_forward` restates.  Granite's
    softmax scale is `attention_multiplier`: the forward reads `self.scaling`, whatever the module put there.  A GraniteAttention
    with biased projections (`attention_bias`) keeps transformers' code.  Returns the count."""
    return sum(_use_attention_node(model, name, (*_QKVO, "scaling"), "llama-attn", _llama_attention_forward, also)
               for name, also in (("LlamaAttention", lambda mod: True), ("ArceeAttention", lambda mod: True),
                                  ("GraniteAttention", lambda mod: _bias_free(mod, _QKVO))))


def use_qwen3_attention_node(model: torch.nn.Module) -> int:
    """Patch Qwen3Attention modules of a model that runs on "dalm_sdpa" (models/attention.py) and whose forward is the code
    `_qwen3_attention_forward` restates.  Returns the count."""
    return _use_attention_node(model, "Qwen3Attention", ("q_proj", "k_proj", "v_proj", "o_proj", "q_norm", "k_norm", "scaling",
                                                         "sliding_window"), "qwen3-attn", _qwen3_attention_forward)


def use_olmo2_attention_node(model: torch.nn.Module) -> int:
    """Patch Olmo2Attention modules of a model that runs on "dalm_sdpa" (models/attention.py) and whose forward is the code
    `_olmo2_attention_forward` restates; a biased projection (`attention_bias`) keeps transformers' code.  Returns the count."""
    def plain(mod) -> bool:
        return all(getattr(getattr(mod, a, None), "bias", 0) is None for a in ("q_proj", "k_proj", "v_proj", "o_proj"))

    from . import attention

    if getattr(getattr(model, "config", None), "_attn_implementation", None) != attention.NAME:
        return 0
    return _install(model, ("Olmo2Attention",),
                    lambda mod: all(hasattr(mod, a) for a in ("q_norm", "k_norm", "scaling", "head_dim")) and plain(mod),
                    "olmo2-attn", _olmo2_attention_forward, keep="_dalm_orig_attn_forward")


# Olmo2Attention.forward: the norms sit on the projections' outputs, the head views come after them (other classes named Olmo*Attention
# - olmo, olmo3, olmoe - are other code: no norm, a clamp, sliding windows; they are not named and would not pass)
_SOURCE_GUARDS["olmo2-attn"] = (_restates(
    _LLAMA_ATTN_PARAMS,
    "query_states = self.q_norm(self.q_proj(hidden_states))",
    "key_states = self.k_norm(self.k_proj(hidden_states))",
    "value_states = self.v_proj(hidden_states)",
    "query_states = query_states.view(hidden_shape).transpose(1, 2)",
    "key_states = key_states.view(hidden_shape).transpose(1, 2)",
    "value_states = value_states.view(hidden_shape).transpose(1, 2)",
    *_LLAMA_ATTN_STATEMENTS[1:]), _RESTATED)


# ---------------------------------------------------------------------------
# decoder layer: residual add + RMSNorm in one launch each way
# ---------------------------------------------------------------------------
_LLAMA_LAYER_PARAMS = ["self", "hidden_states", "attention_mask", "position_ids", "past_key_values", "use_cache",
                       "position_embeddings", "kwargs"]


def _llama_layer_forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_values=None, use_cache=False,
                         position_embeddings=None, **kwargs):
    """transformers' LlamaDecoderLayer.forward with its two (residual add, RMSNorm) pairs on `dalm_rms_norm_{fwd,bwd}`:
      input_layernorm         : the norm alone forward; its backward kernel also adds the residual-path gradient
      post_attention_layernorm: residual + attention output and the norm in one launch; one launch backward
    instead of add 18 us + norm 21 us forward and norm backward 60 us + gradient add 17 us per pair (cfg3).  Same values as
    LlamaRMSNorm up to the f32 summation order of mean(x^2)."""
    from . import tower_ops

    return _two_norm_layer_forward(self, tower_ops.rms_norm_supported, tower_ops.add_rms_norm, hidden_states, attention_mask,
                                   position_ids, past_key_values, use_cache, position_embeddings, kwargs)


def _gemma_layer_forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_values=None, use_cache=False,
                         position_embeddings=None, **kwargs):
    """transformers' GemmaDecoderLayer.forward - LlamaDecoderLayer.forward, statement for statement (the "gemma-layer" guard) - with
    its two (residual add, GemmaRMSNorm) pairs on `dalm_gemma_norm_{fwd,bwd}`, placed as `_llama_layer_forward` places Llama's."""
    from . import tower_ops

    return _two_norm_layer_forward(self, tower_ops.gemma_rms_norm_supported, tower_ops.gemma_add_rms_norm, hidden_states,
                                   attention_mask, position_ids, past_key_values, use_cache, position_embeddings, kwargs)


def _two_norm_layer_forward(self, supported, add_norm, hidden_states, attention_mask, position_ids, past_key_values, use_cache,
                            position_embeddings, kwargs):
    """The body the two forwards above share; `supported(x, w)` / `add_norm(x, delta, w, eps)` are the family's norm."""
    n1, n2 = self.input_layernorm, self.post_attention_layernorm
    if not (supported(hidden_states, n1.weight) and supported(hidden_states, n2.weight)):
        return self._dalm_orig_forward(hidden_states, attention_mask=attention_mask, position_ids=position_ids,
                                       past_key_values=past_key_values, use_cache=use_cache,
                                       position_embeddings=position_embeddings, **kwargs)
    residual, normed = add_norm(hidden_states, None, n1.weight, _norm_eps(n1))
    attn_out, _ = self.self_attn(hidden_states=normed, attention_mask=attention_mask, position_ids=position_ids,
                                 past_key_values=past_key_values, use_cache=use_cache,
                                 position_embeddings=position_embeddings, **kwargs)
    residual, normed = add_norm(residual, attn_out, n2.weight, _norm_eps(n2))
    return residual + self.mlp(normed)


def _granite_layer_forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_values=None, use_cache=False,
                           position_embeddings=None, **kwargs):
    """transformers' GraniteDecoderLayer.forward - LlamaDecoderLayer.forward with `* self.residual_multiplier` on both sub-block
    outputs - on `_two_norm_layer_forward`'s structure:
      input_layernorm         : the norm alone forward; its backward kernel also adds the residual-path gradient (`add_rms_norm`)
      post_attention_layernorm: residual + attention output * m and the norm in one launch; the backward's launch also makes the
                                attention output's gradient, dx * m (`scaled_add_rms_norm`)
      the trailing add        : residual + mlp output * m in one launch each way (`scale_add`)
    The products round where the eager ones do.  A sub-block that answers in another dtype than the residual stream (autocast
    over f32 weights) has its product formed by torch, in that dtype, as the eager statement forms it."""
    from . import tower_ops

    n1, n2 = self.input_layernorm, self.post_attention_layernorm
    if not (tower_ops.scaled_add_rms_norm_supported(hidden_states, n1.weight)
            and tower_ops.scaled_add_rms_norm_supported(hidden_states, n2.weight)):
        return self._dalm_orig_forward(hidden_states, attention_mask=attention_mask, position_ids=position_ids,
                                       past_key_values=past_key_values, use_cache=use_cache,
                                       position_embeddings=position_embeddings, **kwargs)
    m = float(self.residual_multiplier)
    residual, normed = tower_ops.add_rms_norm(hidden_states, None, n1.weight, _norm_eps(n1))
    attn_out, _ = self.self_attn(hidden_states=normed, attention_mask=attention_mask, position_ids=position_ids,
                                 past_key_values=past_key_values, use_cache=use_cache,
                                 position_embeddings=position_embeddings, **kwargs)
    if attn_out.dtype == residual.dtype:
        residual, normed = tower_ops.scaled_add_rms_norm(residual, attn_out, m, n2.weight, _norm_eps(n2))
    else:
        residual, normed = tower_ops.add_rms_norm(residual, attn_out * m, n2.weight, _norm_eps(n2))
    mlp_out = self.mlp(normed)
    if mlp_out.dtype == residual.dtype and tower_ops.scale_add_supported(mlp_out, residual):
        return tower_ops.scale_add(residual, mlp_out, m)
    return residual + mlp_out * m



def _olmo2_layer_forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_values=None, use_cache=False,
                         position_embeddings=None, **kwargs):
    """transformers' Olmo2DecoderLayer.forward - the norm comes AFTER each sub-block, inside the residual, and there is no
    input_layernorm - with its two (RMSNorm, residual add) pairs on `dalm_norm_add_{fwd,bwd}`: one launch each way per pair instead
    of Olmo2RMSNorm's f32 chain and the add.  Same values as the eager pair up to the f32 summation order of mean(x^2)."""
    from . import tower_ops

    n1, n2 = self.post_attention_layernorm, self.post_feedforward_layernorm
    if not (tower_ops.norm_add_supported(hidden_states, hidden_states, n1.weight)
            and tower_ops.norm_add_supported(hidden_states, hidden_states, n2.weight)):
        return self._dalm_orig_forward(hidden_states, attention_mask=attention_mask, position_ids=position_ids,
                                       past_key_values=past_key_values, use_cache=use_cache,
                                       position_embeddings=position_embeddings, **kwargs)

    def norm_add(norm, x, residual):             # a sub-block that answers in another dtype (autocast): the two statements as they are
        if tower_ops.norm_add_supported(x, residual, norm.weight):
            return tower_ops.norm_add(x, residual, norm.weight, _norm_eps(norm))
        return residual + norm(x)

    attn_out, _ = self.self_attn(hidden_states=hidden_states, attention_mask=attention_mask, position_ids=position_ids,
                                 past_key_values=past_key_values, use_cache=use_cache,
                                 position_embeddings=position_embeddings, **kwargs)
    hidden_states = norm_add(n1, attn_out, hidden_states)
    return norm_add(n2, self.mlp(hidden_states), hidden_states)


def use_olmo2_layer(model: torch.nn.Module) -> int:
    """Patch Olmo2DecoderLayer modules whose forward is, statement for statement, the code `_olmo2_layer_forward` restates and whose
    two norms are Olmo2RMSNorm.  DALM_NORM_KERNEL=0 disables.  Returns how many layers were patched."""
    if _off("DALM_NORM_KERNEL"):
        return 0

    def two_post_norms(mod) -> bool:
        return (all(_qk_norm_ok(getattr(mod, a, None), True, getattr(mod, "hidden_size", -1))
                    for a in ("post_attention_layernorm", "post_feedforward_layernorm"))
                and not hasattr(mod, "input_layernorm") and all(hasattr(mod, a) for a in ("self_attn", "mlp")))

    return _install(model, ("Olmo2DecoderLayer",), two_post_norms, "olmo2-layer", _olmo2_layer_forward, keep="_dalm_orig_forward")


def use_fused_residual_norm(model: torch.nn.Module) -> int:
    """Patch LlamaDecoderLayer / Qwen3DecoderLayer / ArceeDecoderLayer / GemmaDecoderLayer / GraniteDecoderLayer modules whose forward
    has the signature this file was written against (transformers 5.x; Qwen3's, Arcee's, Gemma's and Granite's are also compared
    statement for statement); DALM_NORM_KERNEL=0 disables.  A Gemma layer's two norms must be GemmaRMSNorm by name and by value
    (`_gemma_norm_matches`); Gemma2 / Gemma3 layers (four norms) are other code and are not taken.  A Granite layer runs
    `_granite_layer_forward` (the two scaled residual adds).  Returns how many layers were patched."""
    if _off("DALM_NORM_KERNEL"):
        return 0

    def plain_rms_norm(nm) -> bool:
        return (nm is not None and type(nm).__name__.endswith("RMSNorm") and getattr(nm, "weight", None) is not None
                and nm.weight.dim() == 1 and "Gemma" not in type(nm).__name__)

    def gemma_rms_norm(nm) -> bool:
        return nm is not None and type(nm).__name__ == "GemmaRMSNorm" and _gemma_rms_norm(nm) and _gemma_norm_matches(nm)

    def two_norms(is_norm, *more):
        return lambda mod: (is_norm(getattr(mod, "input_layernorm", None)) and is_norm(getattr(mod, "post_attention_layernorm", None))
                            and all(hasattr(mod, a) for a in ("self_attn", "mlp", *more)))

    return sum(_install(model, (name,), eligible, guard, forward, keep="_dalm_orig_forward")
               for name, guard, eligible, forward in (
                   ("LlamaDecoderLayer", "llama-layer", two_norms(plain_rms_norm), _llama_layer_forward),
                   ("Qwen3DecoderLayer", "qwen3-layer", two_norms(plain_rms_norm), _llama_layer_forward),
                   ("ArceeDecoderLayer", "arcee-layer", two_norms(plain_rms_norm), _llama_layer_forward),
                   ("GemmaDecoderLayer", "gemma-layer", two_norms(gemma_rms_norm), _gemma_layer_forward),
                   ("GraniteDecoderLayer", "granite-layer", two_norms(plain_rms_norm, "residual_multiplier"), _granite_layer_forward)))


_SOURCE_GUARDS["llama-layer"] = (_restates(_LLAMA_LAYER_PARAMS), _RESTATED)
# Qwen3DecoderLayer.forward must be, statement for statement, the LlamaDecoderLayer.forward `_llama_layer_forward` restates: the
# whole body, behind the signature
_QWEN3_LAYER_BODY = ["residual = hidden_states", "hidden_states = self.input_layernorm(hidden_states)",
                     "hidden_states, _ = self.self_attn(", "hidden_states=hidden_states,", "attention_mask=attention_mask,",
                     "position_ids=position_ids,", "past_key_values=past_key_values,", "use_cache=use_cache,",
                     "position_embeddings=position_embeddings,", "**kwargs,", ")", "hidden_states = residual + hidden_states",
                     "residual = hidden_states", "hidden_states = self.post_attention_layernorm(hidden_states)",
                     "hidden_states = self.mlp(hidden_states)", "hidden_states = residual + hidden_states", "return hidden_states"]
_SOURCE_GUARDS["qwen3-layer"] = (
    lambda params, src: (params == _LLAMA_LAYER_PARAMS and _body(src)[-len(_QWEN3_LAYER_BODY):] == _QWEN3_LAYER_BODY
                         and _body(src)[-len(_QWEN3_LAYER_BODY) - 1].startswith(")")), _RESTATED)
_SOURCE_GUARDS["gemma-layer"] = _SOURCE_GUARDS["qwen3-layer"]       # GemmaDecoderLayer.forward: the same whole body, the same check
_SOURCE_GUARDS["arcee-layer"] = _SOURCE_GUARDS["qwen3-layer"]       # ArceeDecoderLayer.forward likewise
# GraniteDecoderLayer.forward: Qwen3's body with the two sub-block outputs scaled.  A docstring stands between the signature and the
# body there, so the statements are compared as syntax trees, the docstring left out: nothing else may stand in the function
_GRANITE_LAYER_BODY = [{"hidden_states = residual + hidden_states": "hidden_states = residual + hidden_states * self.residual_multiplier"}
                       .get(s, s) for s in _QWEN3_LAYER_BODY]


def _same_statements(src: str, body: list) -> bool:
    """The function's statements, without its docstring, against the lines of `body` joined: equal as syntax trees."""
    import ast
    import textwrap

    fn = ast.parse(textwrap.dedent(src)).body[0]
    got = fn.body[1:] if ast.get_docstring(fn) is not None else fn.body
    want = ast.parse("def f():\n" + textwrap.indent("\n".join(body), "    ")).body[0].body
    return [ast.dump(s) for s in got] == [ast.dump(s) for s in want]


_SOURCE_GUARDS["granite-layer"] = (
    lambda params, src: params == _LLAMA_LAYER_PARAMS and _same_statements(src, _GRANITE_LAYER_BODY), _RESTATED)
# Olmo2DecoderLayer.forward: the whole body, behind the signature
_OLMO2_LAYER_BODY = ["residual = hidden_states", "hidden_states, _ = self.self_attn(", "hidden_states=hidden_states,",
                     "attention_mask=attention_mask,", "position_ids=position_ids,", "past_key_values=past_key_values,",
                     "use_cache=use_cache,", "position_embeddings=position_embeddings,", "**kwargs,", ")",
                     "hidden_states = self.post_attention_layernorm(hidden_states)", "hidden_states = residual + hidden_states",
                     "residual = hidden_states", "hidden_states = self.mlp(hidden_states)",
                     "hidden_states = self.post_feedforward_layernorm(hidden_states)", "hidden_states = residual + hidden_states",
                     "return hidden_states"]
_SOURCE_GUARDS["olmo2-layer"] = (
    lambda params, src: (params == _LLAMA_LAYER_PARAMS and _body(src)[-len(_OLMO2_LAYER_BODY):] == _OLMO2_LAYER_BODY
                         and _body(src)[-len(_OLMO2_LAYER_BODY) - 1].startswith(")")), _RESTATED)


# ---------------------------------------------------------------------------
# Cohere (Command-R, Aya): a parallel block behind one bias-free f32 LayerNorm, an interleaved f32 rotary embedding
# ---------------------------------------------------------------------------
def _cohere_norm_forward(self, hidden_states: torch.Tensor) -> torch.Tensor:
    """CohereLayerNorm.forward with a weight [D] on `dalm_cohere_norm_{fwd,bwd}`; CPU tensors and unsupported widths run the class's
    own statements."""
    from . import tower_ops

    if tower_ops.cohere_norm_supported(hidden_states, self.weight):
        return tower_ops.cohere_norm_res(hidden_states, self.weight, float(self.variance_epsilon))[1]
    return type(self).forward(self, hidden_states)


def _cohere_norm_matches(mod: torch.nn.Module) -> bool:
    """The module's OWN forward against F.layer_norm in f32 with one rounding (the formula the kernel implements; on a GPU the
    patched forward, i.e. the HIP kernel) on a small random tensor with a mean, once per class, dtype and device type.  On a GPU an
    f32 weight is probed under f32 AND bf16 activations: under autocast the kernel sees the latter.  Leaves `mod` as it is."""
    w = mod.weight

    def formula(m, x):
        return F.layer_norm(x.float(), (x.shape[-1],), m.weight.float(), None, float(m.variance_epsilon)).to(x.dtype)

    def probe():
        g = torch.Generator().manual_seed(0)
        x = 0.3 + 1.5 * torch.randn(4, 3, w.shape[0], generator=g)
        # at the initialisation (ones) the weight tells nothing: the probe runs on a twin of the module with a weight of its own
        twin = copy.copy(mod)
        twin._parameters = dict(mod._parameters)
        twin.weight = torch.nn.Parameter((1.0 + 0.5 * torch.randn(w.shape, generator=g)).to(device=w.device, dtype=w.dtype),
                                         requires_grad=False)
        x_dtypes = {w.dtype, torch.bfloat16} if w.is_cuda else {w.dtype}
        with torch.no_grad():
            return all(_close(formula(twin, xd), type(mod).forward(twin, xd), 2.0)
                       and _close(_cohere_norm_forward(twin, xd), type(mod).forward(twin, xd), 2.0)
                       for xd in (x.to(device=w.device, dtype=dt) for dt in sorted(x_dtypes, key=str)))

    return _guard(("cohere-norm", type(mod), w.dtype, w.device.type), type(mod).__name__ + ".forward",
                  "(w.float() * layer_norm(x.float())).to(x.dtype), without a bias, here", probe)


def _cohere_layer_norm(mod) -> bool:
    w = getattr(mod, "weight", None)
    return w is not None and w.dim() == 1 and getattr(mod, "bias", None) is None and hasattr(mod, "variance_epsilon")


def use_cohere_layer_norm(model: torch.nn.Module) -> int:
    """Patch every CohereLayerNorm with a weight [D] that is still on its own forward (the final `model.norm`; a layer's
    input_layernorm is read by `_cohere_layer_forward` directly) onto `dalm_cohere_norm_{fwd,bwd}`: one launch each way instead of
    the f32 chain of ~9.  The [H, hd] q / k norms of `use_qk_norm` are left alone.  DALM_NORM_KERNEL=0 disables; returns the count."""
    if _off("DALM_NORM_KERNEL"):
        return 0
    routed = {id(m.input_layernorm) for m in model.modules()
              if getattr(getattr(m.forward, "__func__", None), "__name__", "") == "_cohere_layer_forward"}
    return _install(model, ("CohereLayerNorm",), lambda mod: _cohere_layer_norm(mod) and id(mod) not in routed, _cohere_norm_matches,
                    _cohere_norm_forward)


def _cohere_layer_forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_values=None, use_cache=False,
                          position_embeddings=None, **kwargs):
    """transformers' CohereDecoderLayer.forward - n = input_layernorm(x); x + self_attn(n) + mlp(n) - with
      input_layernorm: `dalm_cohere_norm_fwd`; its backward kernel also adds the gradient that reaches x through the residual path
      the two adds   : `dalm_add3_live`, (residual + attention output) + mlp output, rounded as the eager pair rounds
    A sub-block that answers in another dtype than the residual stream (autocast over f32 weights), or tensors the kernels do not
    take, run the eager statement."""
    from . import tower_ops

    ln = self.input_layernorm
    if not tower_ops.cohere_norm_supported(hidden_states, ln.weight):
        return self._dalm_orig_forward(hidden_states, attention_mask=attention_mask, position_ids=position_ids,
                                       past_key_values=past_key_values, use_cache=use_cache,
                                       position_embeddings=position_embeddings, **kwargs)
    residual, normed = tower_ops.cohere_norm_res(hidden_states, ln.weight, float(ln.variance_epsilon))
    attn_out, _ = self.self_attn(hidden_states=normed, attention_mask=attention_mask, position_ids=position_ids,
                                 past_key_values=past_key_values, use_cache=use_cache,
                                 position_embeddings=position_embeddings, **kwargs)
    mlp_out = self.mlp(normed)
    if attn_out.dtype == residual.dtype == mlp_out.dtype and tower_ops.add3_live_supported(residual, attn_out, mlp_out):
        return tower_ops.add3_live(residual, attn_out, mlp_out)
    return residual + attn_out + mlp_out


def use_cohere_layer(model: torch.nn.Module) -> int:
    """Patch CohereDecoderLayer modules whose forward is, statement for statement, the code `_cohere_layer_forward` restates and
    whose one norm is a CohereLayerNorm with a weight [D] that passes the value probe.  DALM_NORM_KERNEL=0 disables.  Returns how
    many layers were patched."""
    if _off("DALM_NORM_KERNEL"):
        return 0

    def one_norm(mod) -> bool:
        ln = getattr(mod, "input_layernorm", None)
        return (type(ln).__name__ == "CohereLayerNorm" and _cohere_layer_norm(ln) and not hasattr(mod, "post_attention_layernorm")
                and all(hasattr(mod, a) for a in ("self_attn", "mlp")) and _cohere_norm_matches(ln))

    return _install(model, ("CohereDecoderLayer",), one_norm, "cohere-layer", _cohere_layer_forward, keep="_dalm_orig_forward")


# CohereDecoderLayer.forward: the whole body (a docstring stands in front of it: `_same_statements`)
_COHERE_LAYER_BODY = ["residual = hidden_states", "hidden_states = self.input_layernorm(hidden_states)",
                      "hidden_states_attention, _ = self.self_attn(", "hidden_states=hidden_states,", "attention_mask=attention_mask,",
                      "position_ids=position_ids,", "past_key_values=past_key_values,", "use_cache=use_cache,",
                      "position_embeddings=position_embeddings,", "**kwargs,", ")", "hidden_states_mlp = self.mlp(hidden_states)",
                      "hidden_states = residual + hidden_states_attention + hidden_states_mlp", "return hidden_states"]
_SOURCE_GUARDS["cohere-layer"] = (
    lambda params, src: params == _LLAMA_LAYER_PARAMS and _same_statements(src, _COHERE_LAYER_BODY), _RESTATED)


def _cohere_attention_forward(self, hidden_states, position_embeddings=None, attention_mask=None, past_key_values=None, **kwargs):
    """transformers' CohereAttention.forward for the training call ("dalm_sdpa", no q / k norm, no biases, no KV cache, no dropout):
    the same statements with apply_rotary_pos_emb + the attention call as one node (`attention.rope_il_sdpa`: `dalm_rope_il_qk`
    forward, the attention, and one more `dalm_rope_il_qk` launch that un-rotates dq / dk).  Tensors the attention kernels do not
    take but the rotary kernel does (f32; grouped heads of width 32) get the rotary kernel as a node of its own in front of the
    attention call.  Every other call goes to transformers' own forward."""
    from . import attention, tower_ops

    cfg = self.config
    if (getattr(self, "use_qk_norm", False) or not _bias_free(self, _QKVO)
            or past_key_values is not None or position_embeddings is None or getattr(cfg, "_attn_implementation", None) != attention.NAME
            or (self.training and float(getattr(self, "attention_dropout", 0.0)) != 0.0)
            or _off("DALM_FAST_ROPE") or _off("DALM_ATTN_KERNEL") or kwargs.get("output_attentions")):
        return self._dalm_orig_attn_forward(hidden_states, position_embeddings=position_embeddings, attention_mask=attention_mask,
                                            past_key_values=past_key_values, **kwargs)
    input_shape = hidden_states.shape[:-1]
    hidden_shape = (*input_shape, -1, self.head_dim)
    query_states = self.q_proj(hidden_states).view(hidden_shape).transpose(1, 2)
    key_states = self.k_proj(hidden_states).view(hidden_shape).transpose(1, 2)
    value_states = self.v_proj(hidden_states).view(hidden_shape).transpose(1, 2)
    cos, sin = position_embeddings
    if not tower_ops.rope_il_supported(query_states, key_states, cos, sin):     # CPU tensors, ...: the class's own statements
        return self._dalm_orig_attn_forward(hidden_states, position_embeddings=position_embeddings, attention_mask=attention_mask,
                                            past_key_values=past_key_values, **kwargs)
    causal = bool(query_states.shape[2] > 1 and attention_mask is None and getattr(self, "is_causal", True))
    if attention.node_supported(query_states, key_states, value_states, attention_mask, causal):
        attn_output = attention.rope_il_sdpa(query_states, key_states, value_states, cos, sin, attention_mask, float(self.scaling),
                                             causal).transpose(1, 2)
    else:
        from transformers.modeling_utils import ALL_ATTENTION_FUNCTIONS

        query_states, key_states = tower_ops.rope_il_qk(query_states, key_states, cos, sin)
        attn_output, _ = ALL_ATTENTION_FUNCTIONS[cfg._attn_implementation](
            self, query_states, key_states, value_states, attention_mask, dropout=0.0, scaling=self.scaling, **kwargs)
    attn_output = attn_output.reshape(*input_shape, -1).contiguous()
    return self.o_proj(attn_output), None


def use_cohere_attention_node(model: torch.nn.Module) -> int:
    """Patch CohereAttention modules of a model that runs on "dalm_sdpa" (models/attention.py) and whose forward is, statement for
    statement, the code `_cohere_attention_forward` restates.  A module with `use_qk_norm` or biased projections is patched too and
    runs transformers' own forward at call time.  Returns the count."""
    return _use_attention_node(model, "CohereAttention", (*_QKVO, "scaling", "head_dim", "use_qk_norm"), "cohere-attn",
                               _cohere_attention_forward)


# CohereAttention.forward: the whole body
_COHERE_ATTN_BODY = [
    "input_shape = hidden_states.shape[:-1]", "hidden_shape = (*input_shape, -1, self.head_dim)",
    "query_states = self.q_proj(hidden_states).view(hidden_shape)", "key_states = self.k_proj(hidden_states).view(hidden_shape)",
    "value_states = self.v_proj(hidden_states).view(hidden_shape)",
    "if self.use_qk_norm:", "    query_states = self.q_norm(query_states)", "    key_states = self.k_norm(key_states)",
    "query_states = query_states.transpose(1, 2)", "key_states = key_states.transpose(1, 2)",
    "value_states = value_states.transpose(1, 2)", "cos, sin = position_embeddings",
    "query_states, key_states = apply_rotary_pos_emb(query_states, key_states, cos, sin)",
    "if past_key_values is not None:",
    "    key_states, value_states = past_key_values.update(key_states, value_states, self.layer_idx)",
    "attention_interface: Callable = ALL_ATTENTION_FUNCTIONS.get_interface(",
    "    self.config._attn_implementation, eager_attention_forward", ")",
    "attn_output, attn_weights = attention_interface(", "    self,", "    query_states,", "    key_states,", "    value_states,",
    "    attention_mask,", "    dropout=0.0 if not self.training else self.attention_dropout,", "    scaling=self.scaling,",
    "    **kwargs,", ")", "attn_output = attn_output.reshape(*input_shape, -1).contiguous()",
    "attn_output = self.o_proj(attn_output)", "return attn_output, attn_weights"]
_SOURCE_GUARDS["cohere-attn"] = (
    lambda params, src: params == _LLAMA_ATTN_PARAMS and _same_statements(src, _COHERE_ATTN_BODY), _RESTATED)


# ---------------------------------------------------------------------------
# Phi-3 / Phi-4 (`model_type` phi3): Llama's layer with fused projections (one qkv_proj, one gate_up_proj), a rotary embedding over
# the first cos.shape[-1] elements of a head only, and dropout on the two sub-block outputs (resid_pdrop, 0.0 in every released config)
# ---------------------------------------------------------------------------
def _phi3_projections(self, hidden_states, hidden_shape):
    """Phi3Attention.forward's first statements: ONE qkv_proj call, q | k | v as column slices of its output, as head views."""
    qkv = self.qkv_proj(hidden_states)
    query_pos = self.config.num_attention_heads * self.head_dim
    key_end = query_pos + self.num_key_value_heads * self.head_dim
    return (qkv[..., :query_pos].view(hidden_shape), qkv[..., query_pos:key_end].view(hidden_shape),
            qkv[..., key_end:].view(hidden_shape).transpose(1, 2))


def _phi3_attention_forward(self, hidden_states, position_embeddings=None, attention_mask=None, past_key_values=None, **kwargs):
    """Phi3Attention.forward on `_decoder_attention_forward`: full-width tables take `attention.rope_sdpa` (the rotation's backward in
    the attention backward's epilogues: Phi-3-medium, Phi-4), narrower ones `attention.rope_partial_sdpa` (Phi-4-mini), anything
    else the module's own apply_rotary_pos_emb and the registered attention function.  A `sliding_window` shorter than the keys
    goes to transformers' own forward."""
    return _decoder_attention_forward(self, hidden_states, position_embeddings, attention_mask, past_key_values, kwargs, None,
                                      {"sliding_window": getattr(self.config, "sliding_window", None)}, project=_phi3_projections)


def use_phi3_attention_node(model: torch.nn.Module) -> int:
    """Patch Phi3Attention modules of a model that runs on "dalm_sdpa" (models/attention.py) and whose forward is, statement for
    statement, the code `_phi3_attention_forward` restates.  Returns the count."""
    return _use_attention_node(model, "Phi3Attention", ("qkv_proj", "o_proj", "scaling", "head_dim", "num_key_value_heads"),
                               "phi3-attn", _phi3_attention_forward, lambda mod: _bias_free(mod, ("qkv_proj", "o_proj")))


# Phi3Attention.forward: the whole body
_PHI3_ATTN_BODY = [
    "input_shape = hidden_states.shape[:-1]", "hidden_shape = (*input_shape, -1, self.head_dim)",
    "qkv = self.qkv_proj(hidden_states)", "query_pos = self.config.num_attention_heads * self.head_dim",
    "query_states = qkv[..., :query_pos]",
    "key_states = qkv[..., query_pos : query_pos + self.num_key_value_heads * self.head_dim]",
    "value_states = qkv[..., query_pos + self.num_key_value_heads * self.head_dim :]",
    "query_states = query_states.view(hidden_shape).transpose(1, 2)", "key_states = key_states.view(hidden_shape).transpose(1, 2)",
    "value_states = value_states.view(hidden_shape).transpose(1, 2)", "cos, sin = position_embeddings",
    "query_states, key_states = apply_rotary_pos_emb(query_states, key_states, cos, sin)",
    "if past_key_values is not None:",
    "    key_states, value_states = past_key_values.update(key_states, value_states, self.layer_idx)",
    "attention_interface: Callable = ALL_ATTENTION_FUNCTIONS.get_interface(",
    "    self.config._attn_implementation, eager_attention_forward", ")",
    "attn_output, attn_weights = attention_interface(", "    self,", "    query_states,", "    key_states,", "    value_states,",
    "    attention_mask,", "    dropout=0.0 if not self.training else self.attention_dropout,", "    scaling=self.scaling,",
    "    sliding_window=getattr(self.config, \"sliding_window\", None),", "    **kwargs,", ")",
    "attn_output = attn_output.reshape(*input_shape, -1).contiguous()",
    "attn_output = self.o_proj(attn_output)", "return attn_output, attn_weights"]
_SOURCE_GUARDS["phi3-attn"] = (
    lambda params, src: params == _LLAMA_ATTN_PARAMS and _same_statements(src, _PHI3_ATTN_BODY), _RESTATED)


def _phi3_mlp_forward(self, x):
    """Phi3MLP.forward with `up * silu(gate)` on the SwiGLU kernels: gate and up are the two halves of the one gate_up_proj output,
    read in place (`dalm_swiglu_{fwd,bwd}_2d_live`).  The product commutes: the kernels' silu(gate) * up rounds identically."""
    from . import tower_ops

    gate, up = self.gate_up_proj(x).chunk(2, dim=-1)
    if tower_ops.swiglu_supported(gate, up):
        return self.down_proj(tower_ops.swiglu(gate, up))
    return self.down_proj(up * self.activation_fn(gate))


_PHI3_MLP_BODY = ["up_states = self.gate_up_proj(hidden_states)", "gate, up_states = up_states.chunk(2, dim=-1)",
                  "up_states = up_states * self.activation_fn(gate)", "return self.down_proj(up_states)"]
_SOURCE_GUARDS["phi3-mlp"] = (
    lambda params, src: params == ["self", "hidden_states"] and _same_statements(src, _PHI3_MLP_BODY), _RESTATED)


def use_phi3_mlp(model: torch.nn.Module) -> int:
    """Patch the bias-free Phi3MLP modules with a SiLU activation whose forward is, statement for statement, the code
    `_phi3_mlp_forward` restates and passes `_mlp_matches`' value probe.  DALM_SWIGLU_KERNEL=0 disables.  Returns the count."""
    if _off("DALM_SWIGLU_KERNEL"):
        return 0

    def fused_silu(mod) -> bool:
        act = getattr(mod, "activation_fn", None)
        return (_bias_free(mod, ("gate_up_proj", "down_proj"))
                and (isinstance(act, torch.nn.SiLU) or type(act).__name__ in ("SiLUActivation", "SiLU")))

    def guard(mod) -> bool:
        return _matches("phi3-mlp", type(mod)) and _mlp_matches(mod, _phi3_mlp_forward, "down(up * silu(gate)) of one gate_up GEMM here",
                                                                "gate_up_proj")

    return _install(model, ("Phi3MLP",), fused_silu, guard, _phi3_mlp_forward)


def _phi3_layer_forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_values=None, use_cache=False,
                        position_embeddings=None, **kwargs):
    """Phi3DecoderLayer.forward - LlamaDecoderLayer.forward with a dropout on each sub-block's output - on `_llama_layer_forward`
    while the two dropouts are the identity (eval, or resid_pdrop == 0: every released config); a training call with p != 0 goes
    to transformers' own forward."""
    if self.training and (float(self.resid_attn_dropout.p) != 0.0 or float(self.resid_mlp_dropout.p) != 0.0):
        return self._dalm_orig_forward(hidden_states, attention_mask=attention_mask, position_ids=position_ids,
                                       past_key_values=past_key_values, use_cache=use_cache,
                                       position_embeddings=position_embeddings, **kwargs)
    return _llama_layer_forward(self, hidden_states, attention_mask=attention_mask, position_ids=position_ids,
                                past_key_values=past_key_values, use_cache=use_cache, position_embeddings=position_embeddings, **kwargs)


def use_phi3_layer(model: torch.nn.Module) -> int:
    """Patch Phi3DecoderLayer modules whose forward is, statement for statement, the code `_phi3_layer_forward` restates, with two
    plain RMSNorms and two `nn.Dropout`s.  DALM_NORM_KERNEL=0 disables.  Returns how many layers were patched."""
    if _off("DALM_NORM_KERNEL"):
        return 0

    def plain_rms_norm(nm) -> bool:
        return (nm is not None and type(nm).__name__ == "Phi3RMSNorm" and getattr(nm, "weight", None) is not None
                and nm.weight.dim() == 1)

    def eligible(mod) -> bool:
        return (plain_rms_norm(getattr(mod, "input_layernorm", None)) and plain_rms_norm(getattr(mod, "post_attention_layernorm", None))
                and all(hasattr(mod, a) for a in ("self_attn", "mlp"))
                and all(type(getattr(mod, a, None)) is torch.nn.Dropout for a in ("resid_attn_dropout", "resid_mlp_dropout")))

    return _install(model, ("Phi3DecoderLayer",), eligible, "phi3-layer", _phi3_layer_forward, keep="_dalm_orig_forward")


# Phi3DecoderLayer.forward: Qwen3's whole body with the attention weights named and the two sub-block outputs behind a dropout;
# compared as syntax trees (`_same_statements`), as Granite's is
_PHI3_LAYER_BODY = [{"hidden_states, _ = self.self_attn(": "hidden_states, self_attn_weights = self.self_attn("}.get(s, s)
                    for s in _QWEN3_LAYER_BODY]
_PHI3_LAYER_BODY[_PHI3_LAYER_BODY.index("hidden_states = residual + hidden_states")] = \
    "hidden_states = residual + self.resid_attn_dropout(hidden_states)"
_PHI3_LAYER_BODY[_PHI3_LAYER_BODY.index("hidden_states = residual + hidden_states")] = \
    "hidden_states = residual + self.resid_mlp_dropout(hidden_states)"
_SOURCE_GUARDS["phi3-layer"] = (
    lambda params, src: params == _LLAMA_LAYER_PARAMS and _same_statements(src, _PHI3_LAYER_BODY), _RESTATED)
