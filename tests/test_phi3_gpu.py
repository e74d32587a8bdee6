"""Phi-3 / Phi-4 on the GPU: `dalm_rope_partial_qk` (dalm_amd/csrc/tower.hip) against transformers' own chain (modeling_phi3.py
`apply_rotary_pos_emb`) on the same tensors, by bits, forward and autograd's backward, out of place and in place, with row liveness;
the node `attention.rope_partial_sdpa` against that chain in front of `attention.sdpa`, by bits; a tiny Phi-3 with LoRA on qkv_proj,
routed against unrouted, padded and packed, in fp32 and bf16; one RAG step with a Phi-3 generator, padded against packed and with the
logits-free head, eager and with the towers graphed.

Exact where the eager chain is exact: the rotation is compared by BITS with what torch computes on the same tensors, and the node with
the chain that feeds the same attention kernels.  Models follow the tolerance rule of tests/test_qwen3_gpu.py (`_held`): the routed
model's largest absolute error against a more precise unrouted model is at most twice the unrouted model's at the same precision."""
import copy

import pytest
import torch

from test_cohere_gpu import _dead_rows, _same_bits
from test_qwen3_gpu import _held, _rel_norm

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
WIDTHS = [(128, 96), (128, 64), (64, 48), (64, 32), (32, 16), (128, 128), (64, 64), (32, 32)]       # (head width, rotary width)
F32_ONLY = [(32, 24)]                        # half of 24 f32 elements is 48 bytes: three chunks; 12 bf16 elements are no whole chunk
HEADS = [(4, 2), (2, 2), (3, 1)]
SIZES = [(2, 5), (1, 33), (3, 64)]           # odd row counts, a partial last workgroup, more than one workgroup
KINDS = ("one", "batch", "distinct")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def test_cases_are_the_issues():
    assert set(WIDTHS) == {(128, 96), (128, 64), (64, 48), (64, 32), (32, 16), (128, 128), (64, 64), (32, 32)}
    assert F32_ONLY == [(32, 24)] and HEADS == [(4, 2), (2, 2), (3, 1)] and SIZES == [(2, 5), (1, 33), (3, 64)]
    assert KINDS == ("one", "batch", "distinct")


def _dtypes(hd, rot):
    return (torch.float32,) if (hd, rot) in F32_ONLY else (torch.bfloat16, torch.float32)


# ---- the partial rotary embedding ----------------------------------------------------------------------------------------
def _tables(B, T, rot, kind, dtype, dev, g):
    """cos / sin [1, T, rot] or [B, T, rot].  "one" / "batch": Phi3RotaryEmbedding's (cat(freqs, freqs): the two halves equal);
    "distinct": independent values in the two halves, so a kernel that reads one half for both fails."""
    nb = 1 if kind == "one" else B
    if kind == "distinct":
        ang = torch.rand(nb, T, rot, generator=g) * 6.28
        cos, sin = ang.cos(), (ang + torch.rand(nb, T, rot, generator=g)).sin()
    else:
        inv = 1.0 / (10000.0 ** (torch.arange(0, rot, 2).float() / rot))
        pos = torch.randint(0, 512, (nb, T), generator=g).float()
        emb = torch.cat((pos[..., None] * inv, pos[..., None] * inv), dim=-1)
        cos, sin = emb.cos(), emb.sin()
    return cos.to(dtype).to(dev), sin.to(dtype).to(dev)


def _split(buf, B, T, Hq, Hk, hd):
    q = buf[..., :Hq * hd].view(B, T, Hq, hd).transpose(1, 2)
    k = buf[..., Hq * hd:(Hq + Hk) * hd].view(B, T, Hk, hd).transpose(1, 2)
    v = buf[..., (Hq + Hk) * hd:].view(B, T, Hk, hd).transpose(1, 2)
    return q, k, v


def _qkv(B, T, Hq, Hk, hd, dtype, dev, g):
    """One [B, T, (Hq + 2 Hk) hd] buffer - qkv_proj's output - as a leaf, and q, k as column slices of it."""
    buf = torch.randn(B, T, (Hq + 2 * Hk) * hd, generator=g).to(dtype).to(dev).requires_grad_(True)
    q, k, _ = _split(buf, B, T, Hq, Hk, hd)
    return buf, q, k


@pytest.mark.parametrize("B,T", SIZES)
@pytest.mark.parametrize("Hq,Hk", HEADS)
@pytest.mark.parametrize("hd,rot", WIDTHS + F32_ONLY)
def test_rotary_is_the_eager_chain_bit_for_bit(dev, hd, rot, Hq, Hk, B, T):
    from transformers.models.phi3 import modeling_phi3 as mp

    from dalm_amd.models import tower_ops

    for dtype in _dtypes(hd, rot):
        for kind in KINDS:
            g = torch.Generator().manual_seed(hd + rot + 7 * B + T + Hq)
            cos, sin = _tables(B, T, rot, kind, dtype, dev, g)
            buf1, q1, k1 = _qkv(B, T, Hq, Hk, hd, dtype, dev, g)
            buf2 = buf1.detach().clone().requires_grad_(True)
            q2, k2, _ = _split(buf2, B, T, Hq, Hk, hd)
            gq = torch.randn(B, Hq, T, hd, generator=g).to(dtype).to(dev)
            gk = torch.randn(B, Hk, T, hd, generator=g).to(dtype).to(dev)
            tag = (hd, rot, Hq, Hk, B, T, dtype, kind)
            assert tower_ops.rope_partial_supported(q1, k1, cos, sin), tag
            qe, ke = tower_ops.rope_partial_qk(q1, k1, cos, sin)
            qw, kw = mp.apply_rotary_pos_emb(q2, k2, cos, sin)
            assert _same_bits(qe.detach(), qw.detach()) and _same_bits(ke.detach(), kw.detach()), tag
            torch.autograd.backward([qe, ke], [gq, gk])
            torch.autograd.backward([qw, kw], [gq, gk])
            assert _same_bits(buf1.grad, buf2.grad), tag                   # dq | dk in the buffer's columns, zeros under v
            assert float(buf1.grad[..., (Hq + Hk) * hd:].float().abs().max()) == 0.0, tag
            assert float(buf1.grad[..., :(Hq + Hk) * hd].float().abs().max()) > 0.0
            if rot == hd:                                                  # the identity: Llama's kernel, bit for bit
                assert tower_ops.rope_supported(q1, k1, cos, sin), tag
                ql, kl = tower_ops.rope_qk(q1.detach(), k1.detach(), cos, sin)
                assert _same_bits(qe.detach(), ql) and _same_bits(ke.detach(), kl), tag
                dl = tower_ops._rope_launch(gq, gk, cos, sin, True)
                dp = tower_ops._rope_partial_launch(gq, gk, cos, sin, True)
                assert _same_bits(dp[0], dl[0]) and _same_bits(dp[1], dl[1]), tag
            # in place: the un-rotation of the attention node
            a, b = gq.clone(), gk.clone()
            a2, b2 = tower_ops._rope_partial_launch(a, b, cos, sin, True, None, in_place=True)
            assert a2 is a and b2 is b
            want = tower_ops._rope_partial_launch(gq, gk, cos, sin, True)
            assert _same_bits(a, want[0]) and _same_bits(b, want[1]), tag


@pytest.mark.parametrize("hd,rot", WIDTHS + F32_ONLY)
def test_rotary_row_liveness_is_exact(dev, hd, rot):
    """Dead (b, t) hold NaN in q, k and the tables of the call with the vector: nothing of them may be loaded.  Fresh outputs: zeros
    over the whole head there, pass part included; live rows carry the bits of the call without the vector, forward and backward.
    In place: dead rows and the pass part of every row keep what the buffer held."""
    from dalm_amd.models import tower_ops

    for dtype in _dtypes(hd, rot):
        for (B, T), (Hq, Hk) in zip(SIZES, HEADS):
            g = torch.Generator().manual_seed(hd + rot + B + T)
            cos, sin = _tables(B, T, rot, "distinct", dtype, dev, g)
            _, q, k = _qkv(B, T, Hq, Hk, hd, dtype, dev, g)
            q, k = q.detach(), k.detach()
            dead = _dead_rows(B * T, hd + B).to(dev)
            live = (~dead).to(torch.uint8)
            dead_bt = dead.view(B, T)
            for backward in (False, True):
                tag = (hd, rot, dtype, B, T, backward)
                want_q, want_k = tower_ops._rope_partial_launch(q, k, cos, sin, backward)
                qn, kn, cn, sn = q.clone(), k.clone(), cos.clone(), sin.clone()
                qn.transpose(1, 2)[dead_bt] = float("nan")
                kn.transpose(1, 2)[dead_bt] = float("nan")
                if cn.shape[0] == B:
                    cn[dead_bt] = float("nan")
                    sn[dead_bt] = float("nan")
                got_q, got_k = tower_ops._rope_partial_launch(qn, kn, cn, sn, backward, live)
                for want, got in ((want_q, got_q), (want_k, got_k)):
                    w2, g2 = want.transpose(1, 2).reshape(B * T, -1), got.transpose(1, 2).reshape(B * T, -1)
                    assert float(g2[dead].float().abs().max()) == 0.0 and not torch.isnan(g2.float()).any(), tag
                    assert _same_bits(w2[~dead], g2[~dead]), tag
                # in place, on buffers that hold a sentinel in the dead rows and in the pass part of every row
                qs, ks = q.clone(), k.clone()
                for t in (qs, ks):
                    t.transpose(1, 2)[dead_bt] = SENTINEL
                    t[..., rot:] = SENTINEL
                r_q, r_k = tower_ops._rope_partial_launch(qs, ks, cn, sn, backward, live, in_place=True)
                assert r_q is qs and r_k is ks
                for want, got in ((want_q, qs), (want_k, ks)):
                    w2, g2 = want.transpose(1, 2).reshape(B * T, -1, hd), got.transpose(1, 2).reshape(B * T, -1, hd)
                    assert float((g2[dead].float() - SENTINEL).abs().max()) == 0.0, tag
                    if rot < hd:
                        assert float((g2[..., rot:].float() - SENTINEL).abs().max()) == 0.0, tag
                    assert _same_bits(w2[~dead][..., :rot], g2[~dead][..., :rot]), tag


def test_the_tower_calls_vector_is_picked_up_and_what_the_predicate_declines(dev):
    from dalm_amd import live_rows
    from dalm_amd.models import tower_ops

    B, T, Hq, Hk, hd, rot = 3, 7, 4, 2, 64, 48
    g = torch.Generator().manual_seed(5)
    cos, sin = _tables(B, T, rot, "batch", torch.bfloat16, dev, g)
    _, q, k = _qkv(B, T, Hq, Hk, hd, torch.bfloat16, dev, g)
    q, k = q.detach(), k.detach()
    mask = (torch.arange(T).unsqueeze(0) >= (T - torch.tensor([7, 4, 1])).unsqueeze(1)).long().to(dev)
    full = tower_ops.rope_partial_qk(q, k, cos, sin)
    with live_rows.tower_call(mask, True) as vec:
        assert vec is not None and int(vec.sum()) == 7 + 5 + 2
        got = tower_ops.rope_partial_qk(q, k, cos, sin)
    dead = vec == 0
    for a, b in zip(full, got):
        a2, b2 = a.transpose(1, 2).reshape(B * T, -1), b.transpose(1, 2).reshape(B * T, -1)
        assert float(b2[dead].float().abs().max()) == 0.0 and _same_bits(a2[~dead], b2[~dead])
    # declined: rot 24 and rot 40 in bf16 (half of either is no whole number of 16-byte chunks), a head width of 96, f32 tables beside
    # bf16 activations, tables wider than the head, tables that ask for a gradient
    z = lambda *s, dt=torch.bfloat16: torch.zeros(*s, dtype=dt, device=dev)  # noqa: E731
    assert tower_ops.rope_partial_supported(z(1, 2, 4, 32), z(1, 1, 4, 32), z(1, 4, 16), z(1, 4, 16))
    assert not tower_ops.rope_partial_supported(z(1, 2, 4, 32), z(1, 1, 4, 32), z(1, 4, 24), z(1, 4, 24))
    assert tower_ops.rope_partial_supported(z(1, 2, 4, 32, dt=torch.float32), z(1, 1, 4, 32, dt=torch.float32),
                                            z(1, 4, 24, dt=torch.float32), z(1, 4, 24, dt=torch.float32))
    assert not tower_ops.rope_partial_supported(z(1, 2, 4, 64), z(1, 1, 4, 64), z(1, 4, 40), z(1, 4, 40))
    assert not tower_ops.rope_partial_supported(z(1, 2, 4, 96), z(1, 1, 4, 96), z(1, 4, 48), z(1, 4, 48))
    assert not tower_ops.rope_partial_supported(z(1, 2, 4, 64), z(1, 1, 4, 64), z(1, 4, 48, dt=torch.float32),
                                                z(1, 4, 48, dt=torch.float32))
    assert not tower_ops.rope_partial_supported(z(1, 2, 4, 32), z(1, 1, 4, 32), z(1, 4, 64), z(1, 4, 64))
    assert not tower_ops.rope_partial_supported(z(1, 2, 4, 64), z(1, 1, 4, 64), z(1, 4, 48).requires_grad_(True), z(1, 4, 48))
    # rows that start 8 bytes into a chunk
    assert not tower_ops.rope_partial_supported(z(1, 2, 4, 64)[..., 4:36], z(1, 1, 4, 64)[..., 4:36], z(1, 4, 16), z(1, 4, 16))


# ---- the attention node ----------------------------------------------------------------------------------------------------
def _packed_descriptor(dev):
    """Three sequences of lengths 5, 33 and 64 (left-padded to 64 columns) and one slack row: 103 packed rows."""
    from dalm_amd import packed

    B, T, lens = 3, 64, [5, 33, 64]
    m2 = (torch.arange(T).unsqueeze(0) >= (T - torch.tensor(lens)).unsqueeze(1)).long()
    rows, cu = packed.pack_plan(m2, shifted=False, multiple=sum(lens) + 1)
    assert rows.numel() == sum(lens) + 1 and int((rows < 0).sum()) == 1
    _i, pos, desc, _v = packed.packed_inputs(torch.zeros(B, T, dtype=torch.long, device=dev), m2.to(dev), rows.to(dev), cu.to(dev), True)
    return rows.numel(), desc, pos


NODE_CASES = [("causal", 4, 4, 64, 48), ("causal", 4, 2, 128, 96), ("key-mask", 4, 4, 128, 96), ("key-mask", 6, 2, 64, 48),
              ("packed", 4, 4, 128, 96), ("packed", 4, 2, 64, 48), ("packed", 4, 2, 128, 64)]


@pytest.mark.parametrize("mode,Hq,Hk,hd,rot", NODE_CASES)
def test_node_is_the_eager_rotation_in_front_of_the_same_attention_by_bits(dev, mode, Hq, Hk, hd, rot):
    from test_attention_gqa_gpu import _hf_mask
    from transformers.models.phi3 import modeling_phi3 as mp

    from dalm_amd.models import attention, tower_ops

    g = torch.Generator().manual_seed(hd + rot + 10 * Hq + len(mode))
    if mode == "packed":
        T, mask, pos = _packed_descriptor(dev)
        B, causal = 1, False
        inv = 1.0 / (10000.0 ** (torch.arange(0, rot, 2, device=dev).float() / rot))
        ang = pos[0].float()[:, None] * inv[None, :]
        cos, sin = torch.cat((ang.cos(), ang.cos()), -1).bfloat16()[None], torch.cat((ang.sin(), ang.sin()), -1).bfloat16()[None]
    else:
        B, T = 3, 40
        cos, sin = _tables(B, T, rot, "one", torch.bfloat16, dev, g)
        mask, causal = (None, True) if mode == "causal" else (_hf_mask(B, T, [0, 23, 9], dev), False)   # left-padded rows: a key mask
    buf = (1.5 * torch.randn(B, T, (Hq + 2 * Hk) * hd, generator=g)).bfloat16().to(dev)
    go = torch.randn(B, T, Hq, hd, generator=g).bfloat16().to(dev).transpose(1, 2)
    scale = hd ** -0.5

    def run(fn):
        x = buf.detach().clone().requires_grad_(True)
        out = fn(*_split(x, B, T, Hq, Hk, hd))
        out.backward(go)
        dq, dk, dv = _split(x.grad, B, T, Hq, Hk, hd)
        return {"out": out.detach(), "dq": dq, "dk": dk, "dv": dv}

    def new(q, k, v):
        assert attention.node_supported(q, k, v, mask, causal) and tower_ops.rope_partial_supported(q, k, cos, sin)
        return attention.rope_partial_sdpa(q, k, v, cos, sin, mask, scale, causal)

    def eager(q, k, v):
        qr, kr = mp.apply_rotary_pos_emb(q, k, cos, sin)
        return attention.sdpa(qr, kr, v, mask, scale, causal)

    got, ref = run(new), run(eager)
    for name in ("out", "dq", "dk", "dv"):
        assert torch.isfinite(got[name].float()).all(), (mode, name)
        assert float(got[name].float().abs().max()) > 0.0, (mode, name)
        assert _same_bits(got[name], ref[name]), (mode, Hq, Hk, hd, rot, name)


# ---- the model -----------------------------------------------------------------------------------------------------------
_NORMS = ("norm.weight", "layernorm.weight")
VOCAB = 259
LAYERS = 2
MODELS = {"64-48": dict(hidden_size=256, num_attention_heads=4, num_key_value_heads=2),
          "128-96": dict(hidden_size=512, num_attention_heads=4, num_key_value_heads=2)}


def _tiny(which="64-48"):
    from transformers import Phi3Config, Phi3ForCausalLM

    torch.manual_seed(0)
    kw = MODELS[which]
    cfg = Phi3Config(vocab_size=VOCAB, intermediate_size=2 * kw["hidden_size"], num_hidden_layers=LAYERS, max_position_embeddings=64,
                     pad_token_id=1, bos_token_id=None, eos_token_id=2,
                     rope_parameters={"rope_type": "default", "rope_theta": 10000.0, "partial_rotary_factor": 0.75}, **kw)
    m = Phi3ForCausalLM(cfg)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith(_NORMS):
                p.add_(0.3 * (2.0 * torch.rand(p.shape) - 1.0))
            p.copy_(p.to(torch.bfloat16).float())              # every copy below holds the SAME (bf16-exact) weights
    return m.train()


def _with_lora(model):
    from dalm_amd.models import lora

    torch.manual_seed(3)                        # lora_A is drawn from the global generator: the same adapters in every copy
    lora.inject_lora(model, ["q_proj", "v_proj"], lora_dropout=0.0)          # resolves to qkv_proj
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if "lora_B" in name:                # at its zero initialisation dA is identically zero and proves nothing
                p.copy_((0.05 * torch.randn(p.shape, generator=g)).to(torch.bfloat16).float())
            if "lora_A" in name:
                p.copy_(p.to(torch.bfloat16).float())
    return model


def _cast(model, dev, dtype):
    model = model.to(dev)
    if dtype == torch.bfloat16:
        for p in model.parameters():
            if not p.requires_grad or p.dim() == 1:           # frozen base and the norm weights; the adapters stay f32
                p.data = p.data.to(torch.bfloat16)
    elif dtype == torch.float64:
        model = model.double()
    return model.train()


_SWITCHES = ("DALM_FAST_ROPE", "DALM_ATTN_KERNEL", "DALM_SWIGLU_KERNEL", "DALM_NORM_KERNEL")


@pytest.mark.parametrize("which", sorted(MODELS))
def test_tiny_model_with_lora_routed_against_unrouted(dev, monkeypatch, which):
    """Left-padded rows of lengths 7 / 4 / 1, padded and packed.  bf16 autocast: logits / hidden states and every LoRA gradient of the
    routed model are no further from the unrouted fp32 model than twice what the unrouted bf16 model is.  fp32: the same rule one
    precision up - the routed fp32 model against the unrouted fp32 model, the truth the unrouted model in float64.  The kernels are
    counted, and none runs with its switch off."""
    from dalm_amd import hip, packed
    from dalm_amd.models import lora
    from dalm_amd.models.rag_e2e_base_model import use_generator_fast_paths

    base = _tiny(which)
    D = base.config.hidden_size
    B, T = 3, 7
    ids = torch.randint(3, VOCAB, (B, T), generator=torch.Generator().manual_seed(1)).to(dev)
    am = (torch.arange(T).unsqueeze(0) >= (T - torch.tensor([7, 4, 1])).unsqueeze(1)).long().to(dev)
    w = torch.randn(B, T, VOCAB, generator=torch.Generator().manual_seed(2)).to(dev) * am[..., None]
    rows, cu = packed.pack_plan(am.cpu(), shifted=True, multiple=64)
    rows, cu = rows.to(dev), cu.to(dev)
    valid = rows >= 0
    sel = rows[valid]
    seen = am.reshape(-1).index_select(0, sel) != 0         # the rows a loss reads (a padding row in front of a sequence is packed too)
    wh = torch.randn(B * T, D, generator=torch.Generator().manual_seed(4)).to(dev).index_select(0, sel) * seen[:, None]

    def grads(model):
        return {n: p.grad.detach().double().clone() for n, p in model.named_parameters() if p.requires_grad}

    def padded(model, dtype):
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
            logits = model(input_ids=ids, attention_mask=am, use_cache=False).logits
        loss = (logits.double() * w).sum()
        loss.backward()
        return logits.detach().double() * am[..., None], grads(model), float(loss.detach())

    def hidden_padded(model, dtype):
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
            h = model.base_model(input_ids=ids, attention_mask=am, use_cache=False)[0].reshape(B * T, -1).index_select(0, sel)
        loss = (h.double() * wh).sum()
        loss.backward()
        return h.detach().double()[seen], grads(model), float(loss.detach())

    def hidden_packed(model, dtype):
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
            h = packed.generator_hidden(model, ids, am, rows, cu)[valid]
        loss = (h.double() * wh).sum()
        loss.backward()
        return h.detach().double()[seen], grads(model), float(loss.detach())

    with monkeypatch.context() as mp:                                 # the references: transformers' own code, one eager LoRA branch
        mp.setattr(lora, "_GROUPS", False)
        mp.setattr(lora, "_FUSED", False)
        exact = _cast(_with_lora(copy.deepcopy(base)), dev, torch.float64)
        truth = _cast(_with_lora(copy.deepcopy(base)), dev, torch.float32)
        plain = _cast(_with_lora(copy.deepcopy(base)), dev, torch.bfloat16)
        assert not any(hasattr(l, "_dalm_orig_forward") for l in plain.model.layers)
        e_logits, e_grads, _ = padded(exact, torch.float64)
        e_h, e_g, _ = hidden_padded(exact, torch.float64)
        t_logits, t_grads, _ = padded(truth, torch.float32)
        r_logits, r_grads, _ = padded(plain, torch.bfloat16)
        t_h, t_g, _ = hidden_padded(truth, torch.float32)
        r_h, r_g, _ = hidden_padded(plain, torch.bfloat16)
        del exact
    names = set(t_grads)
    assert len(names) == 2 * LAYERS and all("qkv_proj.lora_" in n for n in names)

    def routed_model(dtype):
        fast = copy.deepcopy(base)
        got = use_generator_fast_paths(fast)
        assert got["use_phi3_layer"] == LAYERS and got["use_phi3_mlp"] == LAYERS and got["use_phi3_attention_node"] == LAYERS
        assert got["use_hip_attention_backward"] is True and packed.attention_is_packable(fast)
        return _cast(_with_lora(fast), dev, dtype)

    calls = []
    real_call = hip.call
    monkeypatch.setattr(hip, "call", lambda name, *args: (calls.append(name), real_call(name, *args))[1])

    def ran_routed(tag, bf16):
        # the node: forward, and the in-place un-rotation of dq / dk; fp32 tensors are not the attention kernels': the class's own chain
        assert calls.count("dalm_rope_partial_qk") == (2 * LAYERS if bf16 else 0), (tag, calls)
        assert sum(c.startswith("dalm_rms_norm_fwd") for c in calls) >= 2 * LAYERS, (tag, calls)
        assert sum(c.startswith("dalm_swiglu_fwd_2d") for c in calls) == LAYERS, (tag, calls)      # the halves of ONE buffer, in place
        assert sum(c.startswith("dalm_swiglu_bwd_2d") for c in calls) == LAYERS, (tag, calls)
        calls.clear()

    # fp32: add + norm and SwiGLU run as kernels, the rotation is the class's own
    fast32 = routed_model(torch.float32)
    for name, run, (x_out, x_gr), (t_out, t_gr) in (("padded", padded, (e_logits, e_grads), (t_logits, t_grads)),
                                                   ("packed", hidden_packed, (e_h, e_g), (t_h, t_g))):
        out, gr, _ = run(fast32, torch.float32)
        ran_routed(("fp32", name), False)
        _held(f"fp32 model {name} outputs", out, t_out, x_out)
        assert set(gr) == names
        for n in sorted(names):
            _held(f"fp32 model {name} {n}", gr[n], t_gr[n], x_gr[n])
    del fast32

    # bf16 autocast: the truth is the unrouted fp32 model
    fast = routed_model(torch.bfloat16)
    calls.clear()
    f_logits, f_grads, _ = padded(fast, torch.bfloat16)
    assert calls.count("dalm_attn_gqa_fwd") == LAYERS and calls.count("dalm_attn_gqa_bwd") == LAYERS, calls
    ran_routed(("bf16", "padded"), True)
    assert set(f_grads) == names == set(r_grads)
    _held("model padded logits", f_logits, r_logits, t_logits)
    for n in sorted(names):
        _held(f"model padded {n}", f_grads[n], r_grads[n], t_grads[n])
    h, f_g, _ = hidden_packed(fast, torch.bfloat16)
    assert calls.count("dalm_attn_gqa_fwd") == LAYERS and calls.count("dalm_attn_gqa_bwd") == LAYERS, calls
    ran_routed(("bf16", "packed"), True)
    _held("model packed hidden", h, r_h, t_h)
    for n in sorted(names):
        _held(f"model packed {n}", f_g[n], r_g[n], t_g[n])
    # padded against packed, the routed model with itself: each under the rule above against the same references
    hp, p_g, _ = hidden_padded(fast, torch.bfloat16)
    calls.clear()
    _held("model padded hidden", hp, r_h, t_h)
    for n in sorted(names):
        _held(f"model padded hidden {n}", p_g[n], r_g[n], t_g[n])

    # each switch off: its route is absent and the model still matches
    gone = {"DALM_FAST_ROPE": ("dalm_rope_partial_qk",), "DALM_ATTN_KERNEL": ("dalm_rope_partial_qk", "dalm_attn_gqa_fwd"),
            "DALM_SWIGLU_KERNEL": ("dalm_swiglu_fwd_2d_live", "dalm_swiglu_bwd_2d_live"),
            "DALM_NORM_KERNEL": ("dalm_rms_norm_fwd_live", "dalm_rms_norm_bwd_live", "dalm_rms_norm_fwd", "dalm_rms_norm_bwd")}
    for switch in _SWITCHES:
        with monkeypatch.context() as mp:
            mp.setenv(switch, "0")
            off = copy.deepcopy(base)
            use_generator_fast_paths(off)
            off = _cast(_with_lora(off), dev, torch.bfloat16)
            calls.clear()
            o_logits, o_grads, _ = padded(off, torch.bfloat16)
            for kernel in gone[switch]:
                assert kernel not in calls, (kernel, switch, calls)
            assert ("dalm_rope_partial_qk" in calls) == (switch not in ("DALM_FAST_ROPE", "DALM_ATTN_KERNEL")), (switch, calls)
            _held(f"model {switch}=0 logits", o_logits, r_logits, t_logits)
            for n in sorted(names):
                _held(f"model {switch}=0 {n}", o_grads[n], r_grads[n], t_grads[n])
    calls.clear()


# ---- one step ------------------------------------------------------------------------------------------------------------
_BUILT = {}


def _phi3_lm():
    """The tiny Phi-3 (width 64, rot 48) with LoRA on qkv_proj (no dropout, lora_B randomised), weights on the bf16 grid; built once."""
    if "lm" not in _BUILT:
        _BUILT["lm"] = _with_lora(_tiny())
    return copy.deepcopy(_BUILT["lm"])


def _one_rag_step(batch, mode, precision, dev, graphed=False):
    """tests/test_cohere_gpu.py's `_one_rag_step`: tiny BERT retriever + tiny Phi-3 generator; mode "padded", "packed" or "fused"
    (padded, fuse_lm_head).  graphed: the towers as hipGraphs from the first step on, the step run twice (the second replays)."""
    from test_causal_retriever_gpu import _GradSnapshot
    from test_qwen3_gpu import _tiny_bert

    from dalm_amd import hip, packed
    from dalm_amd.models import AutoModelForRagE2E
    from dalm_amd.training.step import RagE2EStep

    model = AutoModelForRagE2E.from_modules(_tiny_bert(), _phi3_lm(), None, None, normalize=True, get_peft=None,
                                            retriever_is_autoregressive=False).to(dev)
    if precision == "bf16":
        for p in model.parameters():
            if not p.requires_grad:
                p.data = p.data.to(torch.bfloat16)
    model.train()
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    opt = torch.optim.SGD([p for _, p in named], lr=0.0)
    snap = _GradSnapshot(named)
    opt.register_step_pre_hook(snap)
    step = RagE2EStep(model, opt, None, 100, autocast_dtype=torch.bfloat16 if precision == "bf16" else None, overlap_towers=True,
                      track_grad_norm=True, fuse_lm_head=mode == "fused", graph_towers=graphed, graph_after=0)
    host = packed.add_pack_plans(batch, packed.RAG_GROUPS) if mode == "packed" else batch
    calls, real_call = [], hip.call
    hip.call = lambda name, *a: (calls.append(name), real_call(name, *a))[1]
    try:
        dbatch = {k: v.to(dev) for k, v in host.items()}
        loss = float(step(dbatch))
        if graphed:
            first = (loss, float(step.grad_norm))
            loss = float(step(dbatch))
            torch.cuda.synchronize()
            assert step.towers is not None and not step.towers_failed, "the tower graphs did not run"
            assert (loss, float(step.grad_norm)) == first, "the replay is the captured step"
    finally:
        hip.call = real_call
    assert step._packed_generator(dbatch) == (mode == "packed")
    return {"loss": loss, "grad_norm": float(step.grad_norm)}, snap.grads, calls


def test_rag_step_with_a_phi3_generator_packed_and_fused_against_padded(dev):
    """One RAG-e2e step, tiny BERT retriever + tiny Phi-3 generator: the packed step and the padded step with fuse_lm_head, each
    against the padded step that materialises the model's own logits, at the bounds
    `test_rag_step_with_a_cohere_generator_packed_and_fused_against_padded` (tests/test_cohere_gpu.py) uses: fp32 - loss, gradient
    norm and every gradient within 1e-4; bf16 autocast - loss within 2.5e-4 and gradient norm within 2.2e-3 of the padded bf16 step,
    every parameter's gradient within twice the padded bf16 step's own distance from the fp32 step + 5e-3, and within 4e-2 outright."""
    from test_causal_retriever_gpu import _rag_batch

    batch = _rag_batch(False)
    res = {(m, p): _one_rag_step(batch, m, p, dev) for p in ("fp32", "bf16") for m in ("padded", "packed", "fused")}
    for (m, p), (_, _, calls) in res.items():             # the node in bf16, the row-wise kernels in both precisions
        assert calls.count("dalm_rope_partial_qk") == (2 * LAYERS if p == "bf16" else 0), (m, p, calls)
        assert any(c.startswith("dalm_swiglu_fwd_2d") for c in calls) and any(c.startswith("dalm_rms_norm_fwd") for c in calls), (m, p)
    g32 = res["padded", "fp32"][1]
    assert any("generator_model" in n and "qkv_proj" in n for n in g32)
    for other in ("packed", "fused"):
        o32 = res[other, "fp32"][1]
        assert set(g32) == set(o32)
        for k in ("loss", "grad_norm"):
            d = abs(res[other, "fp32"][0][k] - res["padded", "fp32"][0][k]) / abs(res["padded", "fp32"][0][k])
            print(f"fp32 {other} vs padded {k}: {d:.3e}")
            assert d <= 1e-4, (other, k, d)
        worst = max(_rel_norm(o32[n], g32[n]) for n in g32 if float(g32[n].double().norm()) >= 1e-7)
        print(f"fp32 {other} worst gradient: {worst:.3e}")
        assert worst <= 1e-4, other
        for k, tol in (("loss", 2.5e-4), ("grad_norm", 2.2e-3)):
            d = abs(res[other, "bf16"][0][k] - res["padded", "bf16"][0][k]) / abs(res["padded", "bf16"][0][k])
            print(f"bf16 {other} vs padded {k}: {d:.3e}")
            assert d <= tol, (other, k, d)
        g16, o16 = res["padded", "bf16"][1], res[other, "bf16"][1]
        for n in sorted(g32):
            den = max(float(g32[n].double().norm()), 1e-30)
            d_pad, d_oth = float((g16[n].double() - g32[n].double()).norm()) / den, float((o16[n].double() - g32[n].double()).norm()) / den
            print(f"{n}: padded {d_pad:.3e} {other} {d_oth:.3e}")
            if float(g32[n].double().norm()) >= 1e-7:
                assert d_oth <= 2.0 * d_pad + 5e-3 and d_oth <= 4e-2, (other, n, d_oth, d_pad)


@pytest.mark.parametrize("mode", ["padded", "packed", "fused"])
def test_rag_step_with_a_phi3_generator_runs_graphed(dev, mode):
    """The same step with the towers captured as hipGraphs (rope_type default: nothing in the rotary module reads a device value on
    the host): the graphs are built and replayed, and loss and gradient norm are the eager step's within the bf16 bounds above."""
    from test_causal_retriever_gpu import _rag_batch

    batch = _rag_batch(False)
    eager, _, _ = _one_rag_step(batch, mode, "bf16", dev)
    graphed, _, _ = _one_rag_step(batch, mode, "bf16", dev, graphed=True)
    for k, tol in (("loss", 2.5e-4), ("grad_norm", 2.2e-3)):
        d = abs(graphed[k] - eager[k]) / abs(eager[k])
        print(f"{mode} graphed vs eager {k}: {d:.3e}")
        assert d <= tol, (mode, k, d)
