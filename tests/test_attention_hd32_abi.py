"""Head width 32 (bge-small / e5-small / gte-small / all-MiniLM: hidden 384, 12 heads) in the attention entry points and their
routing, without a GPU: `dalm_attn_fwd` / `dalm_attn_bwd` and their packed forms take the width (their argument checks go on
past "head width" to the alignment check, before anything is enqueued), the rotary epilogues and the grouped entry points do not,
and a BERT of that width is switched to "dalm_sdpa" and packs."""
import ctypes as C

import pytest
import torch

E_NULL, E_SHAPE, E_ALIGN = -1, -2, -4


@pytest.fixture(scope="module")
def lib():
    from dalm_amd import _build, hip

    _build.build(verbose=False)
    return hip.load()


def _buffers():
    """Host memory, 16-byte aligned: the checks under test run before any pointer is read or any kernel is enqueued."""
    raw = (C.c_char * 8192)()
    base = (C.addressof(raw) + 15) & ~15
    return raw, [base + 256 * i for i in range(20)]


def _strides(n, H, T, hd):
    return (C.c_int64 * (3 * n))(*([hd * H * T, hd * T, hd] * n))


def _fwd(lib, p, hd, packed=False, B=1, H=2, T=64):
    q, k, v, rows, live, o, lse, cu = p[:8]
    args = [q, k, v, rows, live] + ([cu] if packed else []) + [B, H, T, hd, C.c_float(0.1), _strides(4, H, T, hd), C.c_float(0.0), None, 0,
                                                                 o, lse, None]
    return (lib.dalm_attn_fwd_packed if packed else lib.dalm_attn_fwd)(*args)


def _bwd(lib, p, hd, packed=False, cos=None, sin=None, B=1, H=2, T=64):
    q, k, v, o, d_o, lse, rows, cols, live, dq, dk, dv, delta, cu = p[:14]
    args = [q, k, v, o, d_o, lse, rows, cols, live] + ([cu] if packed else []) + [B, H, T, hd, C.c_float(0.1), _strides(8, H, T, hd),
                                                                                   cos, sin] + ([] if packed else [0]) + [
        hd, C.c_float(0.0), None, 0, dq, dk, dv, delta, None]
    return (lib.dalm_attn_bwd_packed if packed else lib.dalm_attn_bwd)(*args)


def _gqa_fwd(lib, p, hd, H=4, Hkv=2, T=64):
    q, k, v, rows, live, o, lse = p[:7]
    return lib.dalm_attn_gqa_fwd(q, k, v, rows, live, None, 1, H, Hkv, T, hd, C.c_float(0.1), _strides(4, H, T, hd), o, lse, None)


def _gqa_bwd(lib, p, hd, H=4, Hkv=2, T=64):
    q, k, v, o, d_o, lse, rows, cols, live, dq, dk, dv, delta = p[:13]
    return lib.dalm_attn_gqa_bwd(q, k, v, o, d_o, lse, rows, cols, live, None, 1, H, Hkv, T, hd, C.c_float(0.1), _strides(8, H, T, hd),
                                 None, None, 0, 0, 1, None, 0, dq, dk, dv, delta, None)


@pytest.mark.parametrize("packed", [False, True])
def test_width_32_passes_the_width_check_and_reaches_the_alignment_check(lib, packed):
    """One tensor pointer moved by 8 bytes: DALM_E_ALIGN, the check AFTER "head width" and before any launch."""
    raw, p = _buffers()
    for hd in (32, 64):
        for slot in (0, 2, 5):                         # q, v, o
            moved = list(p)
            moved[slot] += 8
            assert _fwd(lib, moved, hd, packed) == E_ALIGN, (hd, slot, lib.dalm_last_error_string())
            assert b"16-byte aligned" in lib.dalm_last_error_string()
        for slot in (0, 1, 4, 9, 11):                  # q, k, dO, dq, dv
            moved = list(p)
            moved[slot] += 8
            assert _bwd(lib, moved, hd, packed) == E_ALIGN, (hd, slot, lib.dalm_last_error_string())
            assert b"16-byte aligned" in lib.dalm_last_error_string()
    del raw


@pytest.mark.parametrize("packed", [False, True])
def test_width_32_has_no_rotary_epilogue(lib, packed):
    raw, p = _buffers()
    assert _bwd(lib, p, 32, packed, cos=p[14], sin=p[15]) == E_SHAPE
    msg = lib.dalm_last_error_string().decode()
    assert "rotary epilogue" in msg and "32" in msg, msg
    moved = list(p)                                    # the other widths keep theirs: the call goes on to the alignment check
    moved[0] += 8
    assert _bwd(lib, moved, 64, packed, cos=p[14], sin=p[15]) == E_ALIGN
    del raw


def test_grouped_entry_points_keep_rejecting_width_32(lib):
    raw, p = _buffers()
    for call in (_gqa_fwd, _gqa_bwd):
        assert call(lib, p, 32) == E_SHAPE
        assert b"head width" in lib.dalm_last_error_string()
        assert call(lib, p, 32, H=4, Hkv=4) == E_SHAPE     # equal heads through the grouped entry: still 64 / 128 only
        assert b"head width" in lib.dalm_last_error_string()
    del raw


def test_other_widths_are_still_shape_errors(lib):
    raw, p = _buffers()
    for hd in (48, 16, 96, 256):
        for packed in (False, True):
            assert _fwd(lib, p, hd, packed) == E_SHAPE and b"head width" in lib.dalm_last_error_string()
            assert _bwd(lib, p, hd, packed) == E_SHAPE and b"head width" in lib.dalm_last_error_string()
        assert _gqa_fwd(lib, p, hd) == E_SHAPE and b"head width" in lib.dalm_last_error_string()
        assert _gqa_bwd(lib, p, hd) == E_SHAPE and b"head width" in lib.dalm_last_error_string()
    del raw


def _bert_hd32():
    from transformers import BertConfig, BertModel

    torch.manual_seed(0)
    cfg = BertConfig(hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128, vocab_size=101,
                     max_position_embeddings=64)
    return BertModel(cfg).eval()


def test_a_bert_of_width_32_is_switched_and_packable():
    from dalm_amd import packed
    from dalm_amd.models import attention

    model = _bert_hd32()
    assert model.config._attn_implementation == "sdpa" and not packed.attention_is_packable(model)
    assert attention.use_hip_attention_backward(model) is True
    assert model.config._attn_implementation == attention.NAME and packed.attention_is_packable(model)
    assert attention._HEAD_DIMS == (32, 64, 128)


def test_routing_predicates_by_width_on_the_cpu():
    """`rope_fusable` and `grouped_supported` decline width 32 by SHAPE (before they ask for a GPU tensor); `supported` and
    `packed_supported` decline CPU tensors of any width."""
    from dalm_amd.models import attention

    q = torch.zeros(2, 4, 64, 32, dtype=torch.bfloat16).requires_grad_(True)
    kv = torch.zeros(2, 2, 64, 32, dtype=torch.bfloat16)
    cos = torch.zeros(1, 64, 32, dtype=torch.bfloat16)
    assert attention.rope_fusable(q, q, cos, cos) is False
    assert attention.grouped_supported(q, kv, kv, None, 0.0, True, {}) is False
    assert attention.supported(q, q, q, None, 0.0, True, {}) is False
    assert attention.packed_supported(q[:1], q[:1], q[:1]) is False
    assert 32 not in attention._WIDE_HEAD_DIMS and 32 in attention._HEAD_DIMS


def _masks(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(1, T + 1, (B,), generator=g)
    lens[0] = T                      # a row without padding
    lens[2] = 1                      # a single live token
    return (torch.arange(T).unsqueeze(0) < lens.unsqueeze(1)).long()


def test_packed_bert_of_width_32_equals_padded_on_live_tokens():
    """The construction and bounds of tests/test_packed_cpu.py::test_packed_bert_equals_padded_on_live_tokens, the model switched by
    `use_hip_attention_backward` instead of by hand."""
    from dalm_amd import packed
    from dalm_amd.models import attention

    model = _bert_hd32()
    B, T = 4, 14
    mask = _masks(B, T, 5)
    ids = torch.randint(3, 101, (B, T), generator=torch.Generator().manual_seed(6))
    want = model(ids, mask)[0]
    assert attention.use_hip_attention_backward(model)
    rows, cu = packed.pack_plan(mask, shifted=False, multiple=8)
    got = packed.retrieval_hidden(model, ids, mask, rows, cu)
    live = mask.bool()
    assert torch.allclose(got[live], want[live], atol=2e-5, rtol=1e-4)
    assert (got[~live] == 0).all()


def test_a_falcon_of_width_32_is_still_not_patched():
    from transformers import FalconConfig, FalconForCausalLM

    from dalm_amd.models import fastpath

    fastpath._checked.clear()
    fastpath._warned.clear()
    m = FalconForCausalLM(FalconConfig(num_hidden_layers=1, hidden_size=128, num_attention_heads=4, vocab_size=100))
    assert m.transformer.h[0].self_attention.head_dim == 32
    assert fastpath.use_falcon_attention_kernels(m) == 0
    assert m.transformer.h[0].self_attention.forward.__func__ is not fastpath._falcon_attention_forward
