"""Causal-LM retrievers on packed rows, host logic (no GPU): the `last_column` pack plan, the two facts the packed route rests
on (the decoder stack returns the `*ForCausalLM` call's last hidden state; column T - 1 of a padded run is what a run over the
live tokens plus that column computes), and a tiny Llama pooled from the packed rows against the padded reference call
(dalm/models/retriever_only_base_model.py:43-63).  Pooling is done in torch here: the HIP ops refuse CPU tensors."""
from pathlib import Path

import pytest
import torch

from dalm_amd import live_rows, packed
from dalm_amd.utils import eos_mask

from test_packed_cpu import _masks, _tiny_llama

G = Path(__file__).resolve().parent / "golden"


def _plan_masks():
    T = 12
    left, right = _masks(5, T, True, 0), _masks(5, T, False, 1)      # each: a full row, a single live token
    hole = _masks(5, T, True, 2, holes=True)
    hole[3, T - 1] = 0                                               # a hole in the pooled column itself
    empty = _masks(5, T, False, 3)
    empty[3] = 0                                                     # an all-padding row
    return {"left": left, "right": right, "hole": hole, "empty": empty}


@pytest.mark.parametrize("kind", ["left", "right", "hole", "empty"])
def test_last_column_plan_lists_the_live_tokens_and_the_pooled_column(kind):
    m = _plan_masks()[kind]
    B, T = m.shape
    rows, cu = packed.pack_plan(m, shifted=False, multiple=8, last_column=True)
    n = int(cu[B])
    want = [(b, t) for b in range(B) for t in range(T) if m[b, t] or t == T - 1]
    assert [(int(r) // T, int(r) % T) for r in rows[:n]] == want
    assert rows.numel() % 8 == 0 and int(cu[-1]) == rows.numel() and (rows[n:] == -1).all()
    for b in range(B):
        assert int(cu[b + 1]) > int(cu[b]) and int(rows[int(cu[b + 1]) - 1]) % T == T - 1
    # the liveness vector of the padded call has the same notion
    assert live_rows.live_rows(m, False, last_column=True).view(B, T).bool().tolist() == ((m != 0) | (torch.arange(T) == T - 1)).tolist()
    # key liveness still comes from the mask: the pooled column of a right-padded row is query-only
    _ids, pos, desc, valid = packed.packed_inputs(torch.zeros_like(m), m, rows, cu, causal=True)
    kl = packed.packed_of(desc).key_live
    assert [int(k) for k in kl[:n]] == [int(m[b, t] != 0) for b, t in want] and not kl[n:].any()
    assert [int(p) for p in pos[0, :n]] == [t for _, t in want]


@pytest.mark.parametrize("kind", ["left", "right", "hole", "empty"])
@pytest.mark.parametrize("shifted", [False, True])
def test_default_plan_is_unchanged(kind, shifted):
    m = _plan_masks()[kind]
    B, T = m.shape
    rows, cu = packed.pack_plan(m, shifted, 8)
    keep = m != 0
    if shifted:
        keep[:, :-1] |= m[:, 1:] != 0
    idx = keep.reshape(-1).nonzero().squeeze(1)
    assert torch.equal(rows[:idx.numel()], idx) and (rows[idx.numel():] == -1).all()
    assert torch.equal(cu[1:B + 1], keep.sum(1).cumsum(0).to(torch.int32))
    r2, c2 = packed.pack_plan(m, shifted, 8, last_column=False)
    assert torch.equal(rows, r2) and torch.equal(cu, c2)
    assert torch.equal(live_rows.live_rows(m, shifted), keep.view(torch.uint8).reshape(-1))


def test_causal_group_tables_and_plan_markers():
    from dalm_amd.training.common import ShardedBatches

    assert [g[:4] for g in packed.RETRIEVER_GROUPS_CAUSAL] == list(packed.RETRIEVER_GROUPS)
    assert [g[:4] for g in packed.RAG_GROUPS_CAUSAL] == list(packed.RAG_GROUPS)
    assert [len(g) > 4 and g[4] for g in packed.RAG_GROUPS_CAUSAL] == [False, True, True]     # the generator's plan is unchanged
    N, T = 6, 10
    data = {"query_input_ids": torch.randint(0, 50, (N, 6)), "query_attention_mask": _masks(N, 6, False, 8),
            "passage_input_ids": torch.randint(0, 50, (N, T)), "passage_attention_mask": _masks(N, T, False, 9)}
    for groups, causal in ((packed.RETRIEVER_GROUPS, False), (packed.RETRIEVER_GROUPS_CAUSAL, True)):
        sb = ShardedBatches(data, 3, 0, 1, 0, list(data), pack=dict(groups=groups, multiple={"query": 4, "passage": 8}))
        for b in sb.epoch(0, torch.device("cpu")):
            for prefix, mult in (("query", 4), ("passage", 8)):
                rows, cu = packed.pack_plan(b[f"{prefix}_attention_mask"], False, mult, last_column=causal)
                assert torch.equal(b[f"{prefix}_pack_rows"], rows) and torch.equal(b[f"{prefix}_pack_cu"], cu)
                assert (f"{prefix}_{packed.LAST_COLUMN_KEY}" in b) == causal
            again = packed.add_pack_plans({k: v for k, v in b.items() if "pack" not in k}, groups, multiple={"query": 4, "passage": 8})
            assert set(again) == set(b) and all(torch.equal(again[k], b[k]) for k in b)
            assert all(torch.is_tensor(v) for v in b.values())


# ---- the two facts (tiny_generator, fp32, bitwise) ---------------------------------------------------
@pytest.fixture(scope="module")
def tiny_lm():
    from transformers import AutoModelForCausalLM

    return AutoModelForCausalLM.from_pretrained(str(G / "tiny_generator")).eval()


def _lm_batch(left):
    B, T = 4, 16
    mask = _masks(B, T, left, 11)
    ids = torch.randint(3, 80, (B, T), generator=torch.Generator().manual_seed(12))
    return ids, mask


@pytest.mark.parametrize("left", [True, False])
def test_decoder_stack_is_the_causal_lm_calls_last_hidden_state(tiny_lm, left):
    from dalm_amd.models.rag_e2e_base_model import decoder_only

    ids, mask = _lm_batch(left)
    with torch.no_grad():
        want = tiny_lm(ids, attention_mask=mask, output_hidden_states=True, return_dict=True).hidden_states[-1]
        got = tiny_lm.model(input_ids=ids, attention_mask=mask, use_cache=False).last_hidden_state
        assert torch.equal(got, want)
        assert decoder_only(tiny_lm) and torch.equal(packed._decoder_stack(tiny_lm)(input_ids=ids, attention_mask=mask, use_cache=False)[0], want)


def test_last_column_of_a_right_padded_row_is_a_run_over_its_live_tokens_and_that_column(tiny_lm):
    """Column T - 1 of a right-padded row, padded run, against a run over {live tokens} + {column T - 1}: original columns as
    positions, causal attention, column T - 1 dead as a key.  Bitwise.  The dropped padding columns are appended BEHIND the
    pooled token, where causal attention hides them from it: they only keep the row count of every GEMM at T.  (Without them
    the two runs differ in the last bit, 2.4e-7 at most here: the CPU GEMM orders its sums by the row count - the first
    difference appears in layer 0's down_proj, 3.5e-10, with every input to it bitwise equal.)"""
    ids, mask = _lm_batch(False)
    B, T = ids.shape
    assert sorted(int(x) for x in mask.sum(1))[0] == 1 and int(mask.sum(1).max()) == T
    with torch.no_grad():
        want = tiny_lm.model(input_ids=ids, attention_mask=mask, use_cache=False).last_hidden_state[:, T - 1]
        for b in range(B):
            cols = [t for t in range(T) if mask[b, t] or t == T - 1]
            behind = [t for t in range(T) if t not in cols]
            sub_mask = torch.tensor([[int(mask[b, t]) for t in cols] + [0] * len(behind)])     # column T - 1 stays dead as a key
            got = tiny_lm.model(input_ids=ids[b:b + 1, cols + behind], attention_mask=sub_mask,
                                position_ids=torch.tensor([cols + behind]), use_cache=False).last_hidden_state[0, len(cols) - 1]
            assert torch.equal(got, want[b]), b
            # the truly shortened run - the shape the packed route computes: only its GEMM row count differs, so it agrees to
            # rounding (test_packed_cpu.py's own bound)
            short = tiny_lm.model(input_ids=ids[b:b + 1, cols], attention_mask=sub_mask[:, :len(cols)],
                                  position_ids=torch.tensor([cols]), use_cache=False).last_hidden_state[0, -1]
            assert torch.allclose(short, want[b], atol=2e-5, rtol=1e-4), (b, float((short - want[b]).abs().max()))


# ---- tiny Llama: packed rows against the padded reference call ---------------------------------------
def _reference_embedding(model, ids, mask):
    """The reference's expression (retriever_only_base_model.py:43-63), through sdpa."""
    from dalm_amd.models import attention

    model.config._attn_implementation = "sdpa"
    h = model(ids, attention_mask=mask, output_hidden_states=True, return_dict=True).hidden_states[-1]
    model.config._attn_implementation = attention.NAME
    m = eos_mask(mask).unsqueeze(-1).expand(h.size()).float()
    return torch.nn.functional.normalize(torch.sum(h * m, 1) / torch.clamp(m.sum(1), min=1e-9), p=2, dim=1)


@pytest.mark.parametrize("left,holes", [(True, False), (False, False), (True, True)])
def test_packed_causal_retriever_equals_the_padded_reference(left, holes):
    model = _tiny_llama().train()
    B, T = 4, 16
    mask = _masks(B, T, left, 1, holes)
    ids = torch.randint(3, 97, (B, T), generator=torch.Generator().manual_seed(2))
    w = torch.randn(B, 64, generator=torch.Generator().manual_seed(3))
    rows, cu = packed.pack_plan(mask, shifted=False, multiple=8, last_column=True)

    h = packed.causal_retrieval_hidden(model, ids, mask, rows, cu)                     # [n, D]
    assert torch.isfinite(h).all()
    last = h.index_select(0, cu[1:B + 1].long() - 1)
    model.config._attn_implementation = "sdpa"
    want_last = model.base_model(input_ids=ids, attention_mask=mask, use_cache=False)[0][:, T - 1]
    from dalm_amd.models import attention

    model.config._attn_implementation = attention.NAME
    assert torch.allclose(last, want_last, atol=2e-5, rtol=1e-4), float((last - want_last).abs().max())

    grads = []
    for emb in (lambda: torch.nn.functional.normalize(
            packed.causal_retrieval_hidden(model, ids, mask, rows, cu).index_select(0, cu[1:B + 1].long() - 1), p=2, dim=1),
            lambda: _reference_embedding(model, ids, mask)):
        model.zero_grad()
        e = emb()
        (e * w).sum().backward()
        grads.append((e.detach(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}))
    assert torch.allclose(grads[0][0], grads[1][0], atol=2e-5, rtol=1e-4)
    assert grads[1][1] and set(grads[0][1]) == set(grads[1][1])
    for n, g in grads[1][1].items():
        assert torch.allclose(grads[0][1][n], g, atol=2e-5, rtol=1e-4), (n, float((grads[0][1][n] - g).abs().max()))


def test_pair_call_equals_two_calls():
    """Queries and passages through the decoder stack in one packed call: the last rows of the 2 x B real sequences are the two
    separate calls' (the slack sequences of the first input sit in the middle of the joint cu)."""
    model = _tiny_llama()
    (Bq, Tq), (Bp, Tp) = (3, 8), (3, 16)
    mq, mp = _masks(Bq, Tq, False, 4), _masks(Bp, Tp, True, 5)
    iq = torch.randint(3, 97, (Bq, Tq), generator=torch.Generator().manual_seed(6))
    ip = torch.randint(3, 97, (Bp, Tp), generator=torch.Generator().manual_seed(7))
    rq, cq = packed.pack_plan(mq, False, 8, last_column=True)
    rp, cp = packed.pack_plan(mp, False, 8, last_column=True)
    seen = {}

    def pool_in_torch(h, cu, nseq_out, normalize, ops=None):
        seen["cu"] = cu
        e = h.index_select(0, (cu[1:].long() - 1).clamp_min(0))
        return torch.nn.functional.normalize(e, p=2, dim=1) if normalize else e

    from dalm_amd import fused

    orig, fused.pool_last_packed = fused.pool_last_packed, pool_in_torch
    try:
        with torch.no_grad():
            ep, eq = packed.causal_retrieval_embed_pair(model, (ip, mp, rp, cp), (iq, mq, rq, cq), True)
            wp = packed.causal_retrieval_embed(model, ip, mp, rp, cp, True)
            wq = packed.causal_retrieval_embed(model, iq, mq, rq, cq, True)
    finally:
        fused.pool_last_packed = orig
    assert ep.shape == (Bp, 64) and eq.shape == (Bq, 64)
    assert torch.allclose(ep, wp[:Bp], atol=2e-5, rtol=1e-4) and torch.allclose(eq, wq[:Bq], atol=2e-5, rtol=1e-4)


@pytest.mark.parametrize("family", ["mistral", "qwen2"])
@pytest.mark.parametrize("left", [True, False])
def test_the_other_decoder_only_types_pack_too(family, left):
    """`decoder_only` admits mistral and qwen2 next to llama: the packed decoder run's last row per sequence equals the padded
    run's column T - 1 for them as well (sliding window off: the packed attention has none, and `decoder_only` turns a model with
    a window shorter than its positions down)."""
    from transformers import MistralConfig, MistralForCausalLM, Qwen2Config, Qwen2ForCausalLM

    from dalm_amd.models import attention
    from dalm_amd.models.rag_e2e_base_model import decoder_only

    torch.manual_seed(0)
    kw = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, vocab_size=97,
              max_position_embeddings=64)
    if family == "mistral":
        model = MistralForCausalLM(MistralConfig(sliding_window=None, **kw)).eval()
        windowed = MistralConfig(sliding_window=8, **kw)
    else:
        model = Qwen2ForCausalLM(Qwen2Config(use_sliding_window=False, **kw)).eval()
        windowed = Qwen2Config(use_sliding_window=True, sliding_window=8, max_window_layers=0, **kw)
    assert decoder_only(model) and decoder_only(model, 16)
    short_window = type(model)(windowed)
    assert not decoder_only(short_window) and not decoder_only(short_window, 16) and decoder_only(short_window, 8)
    B, T = 4, 16
    mask = _masks(B, T, left, 1)
    ids = torch.randint(3, 97, (B, T), generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        want = model.base_model(input_ids=ids, attention_mask=mask, use_cache=False)[0][:, T - 1]
        assert attention.register()
        model.config._attn_implementation = attention.NAME
        assert packed.attention_is_packable(model)
        rows, cu = packed.pack_plan(mask, shifted=False, multiple=8, last_column=True)
        h = packed.causal_retrieval_hidden(model, ids, mask, rows, cu)
    last = h.index_select(0, cu[1:B + 1].long() - 1)
    assert torch.allclose(last, want, atol=2e-5, rtol=1e-4), float((last - want).abs().max())
