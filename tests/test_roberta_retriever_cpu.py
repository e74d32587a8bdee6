"""RoBERTa-family retrievers (roberta, xlm-roberta, camembert) without a GPU: the packed route's position ids restate
transformers' `create_position_ids_from_input_ids` (the oracle is transformers' own eager model), the packed forward equals the
padded one on the live rows, and the installers admit the three families while declining xlm-roberta-xl and edited code."""
import warnings

import pytest
import torch

from dalm_amd import packed

PAD = 1
FAMILIES = ("Roberta", "XLMRoberta", "Camembert")


def _family(name):
    import transformers

    return getattr(transformers, name + "Config"), getattr(transformers, name + "Model")


def _hf_positions(ids, pad=PAD):
    from transformers.models.xlm_roberta.modeling_xlm_roberta import XLMRobertaEmbeddings

    return XLMRobertaEmbeddings.create_position_ids_from_input_ids(ids, pad)


def _right(B, T, lens, seed):
    ids = torch.randint(3, 90, (B, T), generator=torch.Generator().manual_seed(seed))
    for b, n in enumerate(lens):
        ids[b, n:] = PAD
    return ids


def _cases():
    right = _right(4, 9, (9, 4, 1, 6), 0)
    left = torch.flip(_right(4, 9, (9, 4, 1, 6), 1), dims=(1,))
    hole = _right(3, 10, (10, 7, 5), 2)
    hole_mask = hole != PAD
    hole[0, 3] = PAD                                   # a pad id INSIDE a live span: the mask keeps the row, the count skips it
    hole[1, 0] = PAD
    allpad = _right(3, 6, (6, 0, 3), 3)
    one = torch.tensor([[5], [PAD], [7]])
    return {"right": (right, right != PAD), "left": (left, left != PAD), "pad-inside-span": (hole, hole_mask),
            "all-pad-row": (allpad, allpad != PAD), "T=1": (one, one != PAD)}


@pytest.mark.parametrize("case", list(_cases()))
def test_packed_positions_restate_transformers(case):
    ids, mask = _cases()[case]
    mask = mask.long()
    B, T = ids.shape
    rows, cu = packed.pack_plan(mask, shifted=False, multiple=8)
    valid = rows >= 0
    assert int((~valid).sum()) > 0                                       # every case has slack rows
    want = _hf_positions(ids).reshape(-1).index_select(0, rows.clamp_min(0))
    got = packed.packed_positions(ids, rows, PAD)
    assert got.dtype == torch.int64
    assert torch.equal(got[valid], want[valid])
    assert (got[~valid] == PAD).all()                                    # slack rows: padding_idx
    # the same through `packed_inputs`, selected by the model's family
    cfg_cls, _ = _family("XLMRoberta")

    class Tower:
        config = cfg_cls(pad_token_id=PAD)

    _ids_p, pos, _desc, _valid = packed.packed_inputs(ids, mask, rows, cu, causal=False, model=Tower())
    assert torch.equal(pos[0], got)


def test_positions_count_ids_not_the_mask():
    """A live (mask = 1) pad id: transformers gives it padding_idx and does not count it; a masked-out real id IS counted."""
    ids = torch.tensor([[5, PAD, 6, 7, PAD, PAD]])
    mask = torch.tensor([[1, 1, 1, 0, 0, 0]])
    rows, _cu = packed.pack_plan(mask, shifted=False, multiple=4)
    got = packed.packed_positions(ids, rows, PAD)
    assert got.tolist() == [PAD + 1, PAD, PAD + 2, PAD]
    assert _hf_positions(ids)[0].tolist() == [PAD + 1, PAD, PAD + 2, PAD + 3, PAD, PAD]


def test_family_selection_and_bert_keeps_columns():
    from transformers import BertConfig, LlamaConfig, XLMRobertaXLConfig

    for name in FAMILIES:
        cfg_cls, _ = _family(name)

        class Tower:
            config = cfg_cls(pad_token_id=7)

        assert packed.position_padding_idx(Tower()) == 7
    for cfg in (BertConfig(), LlamaConfig(), XLMRobertaXLConfig()):
        class Other:
            config = cfg

        assert packed.position_padding_idx(Other()) is None
    assert packed.position_padding_idx(object()) is None and packed.position_padding_idx(None) is None

    class Bert:
        config = BertConfig()

    ids, mask = _cases()["left"]
    B, T = ids.shape
    rows, cu = packed.pack_plan(mask.long(), shifted=False, multiple=8)
    valid = rows >= 0
    for model in (Bert(), None):
        _i, pos, _d, _v = packed.packed_inputs(ids, mask.long(), rows, cu, causal=False, model=model)
        assert torch.equal(pos[0][valid], rows[valid] % T) and (pos[0][~valid] == 0).all()


def _tiny_xlmr():
    cfg_cls, model_cls = _family("XLMRoberta")
    torch.manual_seed(0)
    cfg = cfg_cls(hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128, vocab_size=101, pad_token_id=PAD,
                  max_position_embeddings=40, type_vocab_size=1)
    return model_cls(cfg).eval()


def test_packed_xlmr_equals_padded_on_live_tokens_and_column_positions_do_not():
    from dalm_amd.models import attention

    model = _tiny_xlmr()
    assert attention.register()
    B, T = 4, 14
    ids = _right(B, T, (14, 9, 3, 11), 6)                                # right-padded, one row of full length
    mask = (ids != PAD).long()
    with torch.no_grad():
        want = model(ids, mask)[0]
        model.config._attn_implementation = attention.NAME
        rows, cu = packed.pack_plan(mask, shifted=False, multiple=8)
        got = packed.retrieval_hidden(model, ids, mask, rows, cu)
        live = mask.bool()
        assert torch.allclose(got[live], want[live], atol=2e-5, rtol=1e-4)      # the bound test_packed_cpu.py holds BERT to
        assert (got[~live] == 0).all()
        # the pair call goes through the same place
        hq, hp = packed.retrieval_hidden_pair(model, (ids, mask, rows, cu), (ids[:2, :9], mask[:2, :9], *packed.pack_plan(mask[:2, :9], False, 8)))
        assert torch.allclose(hq[live], want[live], atol=2e-5, rtol=1e-4)
        # column positions (what BERT and the decoders get) are another model: the comparison above can see the bug
        ids_p, pos, desc, valid = packed.packed_inputs(ids, mask, rows, cu, causal=False)
        h = model(input_ids=ids_p, attention_mask=desc, position_ids=pos)[0][0]
        wrong = want.new_zeros((B * T + 1, h.shape[-1])).index_copy(0, torch.where(valid, rows, torch.full_like(rows, B * T)), h)
        wrong = wrong[:B * T].view(B, T, -1)
        assert not torch.allclose(wrong[live], want[live], atol=2e-5, rtol=1e-4)
        assert float((wrong[live] - want[live]).abs().max()) > 1e-2


def _tiny(name, heads=2, layers=2):
    cfg_cls, model_cls = _family(name)
    return model_cls(cfg_cls(hidden_size=64, num_hidden_layers=layers, num_attention_heads=heads, intermediate_size=128, vocab_size=101,
                             pad_token_id=PAD, max_position_embeddings=40, type_vocab_size=1))


@pytest.mark.parametrize("name", FAMILIES)
def test_installers_admit_the_family(name):
    from dalm_amd.models import attention, fastpath

    model = _tiny(name, layers=3)                                        # head width 32
    assert not packed.attention_is_packable(model)
    assert attention.use_hip_attention_backward(model) is True
    assert model.config._attn_implementation == attention.NAME and packed.attention_is_packable(model)
    assert fastpath.use_bert_layer_kernels(model) == 2 * 3
    layer = model.encoder.layer[0]
    assert layer.attention.output.forward.__func__ is fastpath._bert_output_forward
    assert layer.output.forward.__func__ is fastpath._bert_output_forward
    assert fastpath.use_roberta_embeddings(model) == 1
    assert model.embeddings.forward.__func__ is fastpath._roberta_embeddings_forward
    # on CPU tensors every patched module runs transformers' statements: same values as an untouched copy
    torch.manual_seed(1)
    ref = _tiny(name, layers=3).eval()
    model.load_state_dict(ref.state_dict())
    model.eval()
    ids = _right(2, 7, (7, 4), 3)
    with torch.no_grad():
        torch.testing.assert_close(model(ids, (ids != PAD).long())[0], ref(ids, (ids != PAD).long())[0], rtol=1e-5, atol=1e-5)
    # a head width the kernels do not take: declined
    assert attention.use_hip_attention_backward(_tiny(name, heads=4)) is False


def test_installers_decline_xlm_roberta_xl():
    from transformers import XLMRobertaXLConfig, XLMRobertaXLModel

    from dalm_amd.models import attention, fastpath

    model = XLMRobertaXLModel(XLMRobertaXLConfig(hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128,
                                                 vocab_size=101, max_position_embeddings=40))
    assert attention.use_hip_attention_backward(model) is False
    assert model.config._attn_implementation != attention.NAME and not packed.attention_is_packable(model)
    assert fastpath.use_bert_layer_kernels(model) == 0
    assert fastpath.use_roberta_embeddings(model) == 0
    assert all("forward" not in m.__dict__ for m in model.modules())


def test_altered_layer_and_embeddings_code_is_refused():
    from transformers.models.xlm_roberta import modeling_xlm_roberta as mx

    from dalm_amd.models import fastpath

    fastpath._checked.clear()
    assert fastpath._matches("roberta-embeddings", mx.XLMRobertaEmbeddings)          # the installed source passes
    assert fastpath._matches("bert-output", mx.XLMRobertaSelfOutput) and fastpath._matches("bert-output", mx.XLMRobertaOutput)
    saved = (mx.XLMRobertaSelfOutput.forward, mx.XLMRobertaEmbeddings.forward)
    fastpath._checked.clear()
    fastpath._warned.clear()
    try:
        def forward(self, hidden_states, input_tensor):
            hidden_states = self.dense(hidden_states)
            hidden_states = self.dropout(hidden_states)
            hidden_states = self.LayerNorm(hidden_states) + input_tensor
            return hidden_states

        def emb_forward(self, input_ids=None, token_type_ids=None, position_ids=None, inputs_embeds=None, past_key_values_length=0):
            embeddings = self.word_embeddings(input_ids)
            embeddings = self.LayerNorm(embeddings)
            embeddings = self.dropout(embeddings)
            return embeddings

        mx.XLMRobertaSelfOutput.forward = forward
        mx.XLMRobertaEmbeddings.forward = emb_forward
        model = _tiny("XLMRoberta")
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            assert fastpath.use_bert_layer_kernels(model) == 2               # the two untouched XLMRobertaOutput modules only
            assert fastpath.use_roberta_embeddings(model) == 0
            assert not fastpath._matches("roberta-embeddings", mx.XLMRobertaEmbeddings)
        assert any("XLMRobertaSelfOutput.forward is not" in str(m.message) for m in w)
        assert any("XLMRobertaEmbeddings.forward is not" in str(m.message) for m in w)
        assert "forward" not in model.embeddings.__dict__ and "forward" not in model.encoder.layer[0].attention.output.__dict__
    finally:
        mx.XLMRobertaSelfOutput.forward, mx.XLMRobertaEmbeddings.forward = saved
        fastpath._checked.clear()
        fastpath._warned.clear()


def test_embed_supported_declines_what_the_kernel_does_not_stand_for():
    """CPU tensors, trainable tables, inputs_embeds, a cache offset: the module's own statements run."""
    from dalm_amd.models import bert_ops

    model = _tiny("XLMRoberta").requires_grad_(False)
    ids = _right(2, 7, (7, 4), 3)
    assert not bert_ops.embed_supported(model.embeddings, ids, None, None, None, 0)          # CPU tensors
    assert not bert_ops.embed_supported(model.embeddings, None, None, None, torch.zeros(2, 7, 64), 0)
    assert not bert_ops.embed_supported(model.embeddings, ids, None, None, None, 3)
