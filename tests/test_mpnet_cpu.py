"""MPNet retrievers without a GPU: the relative-position bias as one vector per head, the route's guards and counts, the packing
rules, and the torch fallback of the routed attention (fp32 / CPU) against the unrouted model."""
import warnings

import pytest
import torch

transformers = pytest.importorskip("transformers")
from transformers import MPNetConfig, MPNetModel  # noqa: E402
from transformers.models.mpnet import modeling_mpnet  # noqa: E402

from dalm_amd import packed  # noqa: E402
from dalm_amd.models import attention, fastpath  # noqa: E402


def _config(**kw):
    base = dict(vocab_size=60, hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=256,
                max_position_embeddings=66, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    base.update(kw)
    return MPNetConfig(**base)


def _model(seed=0, frozen_table=True, **kw):
    torch.manual_seed(seed)
    m = MPNetModel(_config(**kw)).eval()
    with torch.no_grad():
        m.encoder.relative_attention_bias.weight.normal_(0.0, 1.0)
    m.encoder.relative_attention_bias.weight.requires_grad_(not frozen_table)
    return m


@pytest.mark.parametrize("T", [1, 2, 9, 17, 129, 200, 512])
def test_rel_bias_vector_expands_to_position_bias(T):
    """bucket edges at |d| = 8, the saturation at 128: the vector, expanded at differences j - i, IS compute_position_bias."""
    torch.manual_seed(T)
    enc = modeling_mpnet.MPNetEncoder(_config(hidden_size=192, num_attention_heads=3, num_hidden_layers=1))
    with torch.no_grad():
        enc.relative_attention_bias.weight.normal_()
    want = enc.compute_position_bias(torch.zeros(1, T, 4))[0]                       # [H, T, T]
    vec = attention.rel_bias_vector(enc, T, "cpu")
    assert vec.shape == (3, 2 * T - 1) and vec.dtype == torch.float32
    got = attention.expand_rel_bias(vec, torch.arange(T))
    assert torch.equal(got, want)
    # a longer vector serves a shorter sequence: the centre moves, the values do not
    vec2 = attention.rel_bias_vector(enc, T + 5, "cpu")
    assert torch.equal(vec2[:, 5:5 + 2 * T - 1], vec)


def test_rel_bias_vector_follows_the_table():
    enc = modeling_mpnet.MPNetEncoder(_config(num_hidden_layers=1))
    a = attention.rel_bias_vector(enc, 20, "cpu")
    with torch.no_grad():
        enc.relative_attention_bias.weight.add_(1.0)
    assert torch.equal(attention.rel_bias_vector(enc, 20, "cpu"), a + 1.0)


def test_installer_counts_and_packability():
    m = _model()
    assert not packed.attention_is_packable(m)
    assert fastpath.use_mpnet_attention_kernels(m) == 3                           # 2 self-attention modules + the encoder
    assert packed.attention_is_packable(m)
    assert fastpath.use_bert_layer_kernels(m) == 4                                 # 2 MPNetOutput + 2 MPNetAttention
    bias = m.encoder.compute_position_bias(torch.zeros(3, 40, 128))
    assert attention.rel_source_of(bias) is not None and bias.numel() < 3 * 2 * 40 * 40


def test_trainable_table_declines():
    m = _model(frozen_table=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert fastpath.use_mpnet_attention_kernels(m) == 0
    assert not packed.attention_is_packable(m)
    assert m.encoder.compute_position_bias(torch.zeros(1, 5, 128)).shape == (1, 2, 5, 5)


def test_width_32_declines():
    m = _model(hidden_size=64)                                                     # 2 heads x 32
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert fastpath.use_mpnet_attention_kernels(m) == 0
    assert not packed.attention_is_packable(m)


def test_edited_forward_declines():
    class MPNetSelfAttention(modeling_mpnet.MPNetSelfAttention):                   # same name, other code
        def forward(self, hidden_states, attention_mask=None, position_bias=None, output_attentions=False, **kwargs):
            return super().forward(hidden_states, attention_mask, position_bias, output_attentions=output_attentions, **kwargs)

    m = _model()
    old = m.encoder.layer[1].attention.attn
    new = MPNetSelfAttention(m.config)
    new.load_state_dict(old.state_dict())
    m.encoder.layer[1].attention.attn = new
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert fastpath.use_mpnet_attention_kernels(m) == 0                        # all of an encoder or nothing
    assert not packed.attention_is_packable(m)
    assert m.encoder.compute_position_bias(torch.zeros(1, 5, 128)).shape == (1, 2, 5, 5)


def test_position_padding_idx_is_one():
    m = _model(pad_token_id=7)
    assert m.config.pad_token_id == 7
    assert packed.position_padding_idx(m) == 1 == m.embeddings.padding_idx


def _ids_and_mask(B, T, lens, seed=1):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, 60, (B, T), generator=g)
    mask = (torch.arange(T)[None] < torch.tensor(lens)[:, None]).long()
    ids = torch.where(mask.bool(), ids, torch.ones_like(ids))                      # MPNet's pad id (its positions count ids != 1)
    return ids, mask


def test_fp32_fallback_padded_equals_unrouted():
    ref, m = _model(3), _model(3)
    assert fastpath.use_mpnet_attention_kernels(m) == 3
    ids, mask = _ids_and_mask(3, 40, (40, 25, 7))
    with torch.no_grad():
        want, got = ref(ids, mask)[0], m(ids, mask)[0]
        want_full, got_full = ref(ids[:1], None)[0], m(ids[:1], None)[0]
    live = mask.bool()
    torch.testing.assert_close(got[live], want[live], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(got_full, want_full, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("hole", [False, True])
def test_fp32_fallback_packed_equals_unrouted(hole):
    ref, m = _model(4), _model(4)
    assert fastpath.use_mpnet_attention_kernels(m) == 3
    ids, mask = _ids_and_mask(3, 40, (40, 25, 7), seed=2)
    if hole:
        mask[0, 10:19] = 0                                                         # a hole: later tokens keep their columns
        mask[1, 3] = 0
    rows, cu = packed.pack_plan(mask, shifted=False, multiple=16)
    with torch.no_grad():
        want = ref(ids, mask)[0]
        got = packed.retrieval_hidden(m, ids, mask, rows, cu)
    live = mask.bool()
    torch.testing.assert_close(got[live], want[live], rtol=1e-5, atol=1e-5)
    desc = packed.packed_inputs(ids, mask, rows, cu, causal=False, model=m)[2]
    cols = packed.packed_of(desc).cols
    assert cols.dtype == torch.int32
    assert torch.equal(cols[:int(live.sum())].long(), live.reshape(-1).nonzero().squeeze(1) % 40)
