"""Evaluation path on the MI355X: the packed pooling kernel, the gold-rank sweep, the packed embedding sweep and the two
drivers (`evaluate_retriever`, `evaluate_rag`)."""
import csv
from pathlib import Path

import pytest
import torch

from helpers import norm_rel_err
from test_eval_host import brute_rank, reference_loop

pytestmark = pytest.mark.gpu
G = Path(__file__).parent / "golden"

# the bounds tests/test_hip_parity.py holds dalm_pool_l2norm_fwd's embeddings to (fp32 and bf16 inputs alike: the reference
# sees the same rounded inputs)
POOL_NORM_RTOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    from dalm_amd import hip

    hip.load()  # fail loudly if libdalm_hip.so is absent: no fallback
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------
# dalm_pool_l2norm_packed_fwd
# ---------------------------------------------------------------------------
POOL_PROFILES = {
    # sequence lengths (the LAST entry is a slack tail that must not be written); all hold 0, 1, 12 and 128
    "queries": [12, 0, 1, 9, 12, 14, 5, 128, 7, 11, 12, 6, 8, 10, 4, 12, 13, 3, 0, 12, 16],       # mean < 24: a wave per sequence
    "mixed": [0, 1, 12, 128, 5, 0, 77, 128, 12, 3, 40],                                            # two waves per sequence
    "passages": [128, 97, 0, 128, 1, 110, 12, 128, 64, 128, 121, 100],                             # four waves per sequence
}


# d-chunks per lane (64 lanes x 16 bytes each): f32 384 / 768 / 1024 are 2 / 3 / 4, 128 is 1; bf16 384 / 768 / 1024 are 1 / 2 / 2,
# 1280 and 2048 are 3 and 4 (f32 rows end at 1024).  The ids read <D>-dtype<i>, as a D x dtype grid would name them.
PACKED_WIDTHS = [pytest.param(D, dt, id=f"{D}-dtype{i}")
                 for i, dt in enumerate((torch.float32, torch.bfloat16)) for D in (384, 768, 1024, 128, 1280, 2048)
                 if not (dt == torch.float32 and D > 1024)]


@pytest.mark.parametrize("D,dtype", PACKED_WIDTHS)
@pytest.mark.parametrize("profile", sorted(POOL_PROFILES))
def test_packed_pool_vs_fp64_mean_pooling(dev, profile, D, dtype):
    """mean_pooling + F.normalize of the reference (rag_e2e_base_model.py:95-97,108-111) restated in fp64 on the packed rows."""
    from dalm_amd.ops import default_ops

    lens = POOL_PROFILES[profile]
    nseq, nseq_out = len(lens), len(lens) - 1
    g = torch.Generator().manual_seed(D + len(lens))
    n = sum(lens)
    h = (torch.randn(n, D, generator=g) * 0.7 + 0.1).to(dtype)
    cu = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32)
    ld = D + 8
    out = torch.full((nseq_out + 2, ld), 7.0, device=dev)
    got = default_ops().pool_packed_fwd(h.to(dev), cu.to(dev), nseq_out, out=out[:nseq_out, :D])
    assert got.data_ptr() == out.data_ptr() and got.dtype == torch.float32
    ref = torch.zeros(nseq_out, D, dtype=torch.float64)
    h64 = h.double()
    for s in range(nseq_out):
        rows = h64[int(cu[s]):int(cu[s + 1])]
        mask = torch.ones(rows.shape[0], 1, dtype=torch.float64)
        u = (rows * mask).sum(0) / torch.clamp(mask.sum(), min=1e-9)
        ref[s] = u / torch.clamp(u.norm(), min=1e-12)
    e = out[:nseq_out, :D].double().cpu()
    err, worst = norm_rel_err(e, ref), float((e - ref).abs().max())
    print(f"packed pool {profile} D={D} {dtype}: norm-rel {err:.3e}, max abs {worst:.3e}")
    assert err <= POOL_NORM_RTOL and worst <= 10 * POOL_NORM_RTOL * float(ref.abs().max())
    for s, ln in enumerate(lens[:nseq_out]):
        if ln == 0:
            assert float(e[s].abs().max()) == 0.0                      # an empty sequence gives a zero row
    assert bool((out[nseq_out:] == 7.0).all()) and bool((out[:, D:] == 7.0).all())      # untouched


# ---------------------------------------------------------------------------
# dalm_sim_gold_rank
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("block", [262144, 1100])
@pytest.mark.parametrize("threshold", [0.0, 3.0])
def test_gold_rank_exact_on_integer_scores(dev, block, threshold):
    """Q, C with integer entries in {-2..2}, D = 64: every score is an integer below 2^24, exact in f32 in any summation
    order, with many exact ties - rank, n_ge and gold_score must equal brute force exactly (ties: lower index first)."""
    from dalm_amd.retrieval import gold_rank

    g = torch.Generator().manual_seed(7)
    nq, nc, D = 70, 5000, 64
    Q = torch.randint(-2, 3, (nq, D), generator=g).float()
    C = torch.randint(-2, 3, (nc, D), generator=g).float()
    gold = torch.randint(2, nc - 2, (nq,), generator=g)
    gold[0], gold[1], gold[2] = 0, nc - 1, 1099                       # first / last corpus row, last row of a block of 1100
    for i in range(3, 23):                                           # gold rows tied with their neighbours on both sides
        C[gold[i] - 1] = C[gold[i]]
        C[gold[i] + 1] = C[gold[i]]
        C[(gold[i] + 1700) % nc] = C[gold[i]]                         # ... and with a row in another block
    S = Q.double() @ C.double().t()
    rank64, nge64 = brute_rank(S, gold, threshold)
    assert int(((S == S[torch.arange(nq), gold].unsqueeze(1)).sum(1) > 3).sum()) >= 20      # ties exist
    rank, n_ge, score = gold_rank(Q.to(dev), C.to(dev), gold.to(dev), threshold=threshold, block=block)
    assert rank.dtype == torch.int64 and n_ge.dtype == torch.int64 and score.dtype == torch.float32
    assert torch.equal(score.cpu().double(), S[torch.arange(nq), gold])
    assert torch.equal(rank.cpu(), rank64), (rank.cpu() - rank64).abs().max()
    assert torch.equal(n_ge.cpu(), nge64)


def test_gold_rank_exact_with_two_row_tiles_per_wave(dev):
    """From 4096 queries on a wave owns two 32-row tiles (the form every real evaluation set takes): the same exact
    integer-score check, on a query count that is not a multiple of 64, over one and over several corpus blocks."""
    from dalm_amd.retrieval import gold_rank

    g = torch.Generator().manual_seed(11)
    nq, nc, D = 4133, 3000, 64
    Q = torch.randint(-2, 3, (nq, D), generator=g).float()
    C = torch.randint(-2, 3, (nc, D), generator=g).float()
    gold = torch.randint(nc, (nq,), generator=g)
    gold[0], gold[nq - 1] = 0, nc - 1
    C[5] = C[4]
    gold[1], gold[2] = 4, 5                                           # a duplicated row, asked for under both indices
    S = Q.double() @ C.double().t()
    rank64, nge64 = brute_rank(S, gold, 2.0)
    for block in (262144, 1024):
        rank, n_ge, score = gold_rank(Q.to(dev), C.to(dev), gold.to(dev), threshold=2.0, block=block)
        assert torch.equal(score.cpu().double(), S[torch.arange(nq), gold])
        assert torch.equal(rank.cpu(), rank64) and torch.equal(n_ge.cpu(), nge64)
    with pytest.raises(ValueError, match="outside the corpus"):
        gold_rank(Q[:8].to(dev), C.to(dev), torch.full((8,), nc, device=dev))


@pytest.mark.parametrize("threshold", [0.0, 0.12])
@pytest.mark.parametrize("nq,nc,D,a,seed", [(300, 70000, 384, 0.16, 1), (257, 20000, 1024, 0.10, 2), (64, 3001, 256, 0.25, 3)])
def test_gold_rank_vs_fp64_brute_force(dev, nq, nc, D, a, seed, threshold):
    """Unit-norm embeddings: |rank - rank64| <= the number of corpus entries whose fp64 score lies within 2e-6 max(1, max|S|)
    of the gold score (the window test_fused_topk_vs_fp64 grants f32 scores), |n_ge - n_ge64| likewise around the threshold;
    at most 15 % of the queries may have such an entry at all, every other rank is exact."""
    from dalm_amd.eval.utils import RECALL_LADDER
    from dalm_amd.retrieval import gold_rank, metrics_from_rank

    g = torch.Generator().manual_seed(seed)
    F = torch.nn.functional
    C = F.normalize(torch.randn(nc, D, generator=g), dim=1)
    gold = torch.randint(nc, (nq,), generator=g)
    Q = F.normalize(a * C[gold] + F.normalize(torch.randn(nq, D, generator=g), dim=1), dim=1)
    S = Q.double() @ C.double().t()
    gs = S[torch.arange(nq), gold]
    rank64, nge64 = brute_rank(S, gold, threshold)
    w = 2e-6 * max(1.0, float(S.abs().max()))
    near_gold = ((S - gs.unsqueeze(1)).abs() <= w).sum(1) - 1              # the gold column itself is not a competitor
    near_thr = ((S - threshold).abs() <= w).sum(1)
    share = float((near_gold > 0).float().mean())
    print(f"nq={nq} nc={nc} D={D}: window {w:.2e}, queries with a neighbour in it {share:.1%}, "
          f"rank min/median/max {int(rank64.min())}/{int(rank64.median())}/{int(rank64.max())}")
    assert share <= 0.15                                                   # the inputs leave most ranks exactly decidable
    hit10 = float((rank64 < 10).float().mean())
    assert 0.0 < hit10 < 1.0
    rank, n_ge, score = gold_rank(Q.to(dev), C.to(dev), gold.to(dev), threshold=threshold)
    rank, n_ge, score = rank.cpu(), n_ge.cpu(), score.cpu().double()
    d_rank, d_nge = (rank - rank64).abs(), (n_ge - nge64).abs()
    print(f"  max |rank - rank64| {int(d_rank.max())}, max |n_ge - n_ge64| {int(d_nge.max())}, "
          f"max |gold_score - fp64| {float((score - gs).abs().max()):.2e}")
    assert bool((d_rank <= near_gold).all()), (d_rank - near_gold).max()
    assert bool((d_nge <= near_thr).all()), (d_nge - near_thr).max()
    torch.testing.assert_close(score, gs, rtol=1e-5, atol=w)
    if threshold > 0 and D == 1024:
        # a random unit-norm pair scores ~ N(0, 1/D): at D = 1024 the threshold 0.12 is 3.8 sigma, about 1.4 of 20 000 passages
        # pass it, so n_ge < k occurs (at D = 384 / 256 it is 2.4 / 1.9 sigma and hundreds pass)
        assert bool((nge64 < 10).any())
    # the walk over several corpus blocks gives the same counts
    rank_b, nge_b, score_b = gold_rank(Q.to(dev), C.to(dev), gold.to(dev), threshold=threshold, block=max(1000, nc // 3))
    assert torch.equal(rank_b.cpu(), rank) and torch.equal(nge_b.cpu(), n_ge) and torch.equal(score_b.cpu().double(), score)
    m = metrics_from_rank(rank, n_ge, list(RECALL_LADDER))
    assert [x["top_k"] for x in m] == list(RECALL_LADDER) and all(x["recall"] <= y["recall"] for x, y in zip(m, m[1:]))


# ---------------------------------------------------------------------------
# embedding sweep + drivers at bge-large width (depth 2)
# ---------------------------------------------------------------------------
def _words(tok):
    return sorted(w for w in tok.get_vocab() if w.isalpha())


def _write_rows(path, tok, n_rows, n_passages, seed, max_passage_words=120):
    """csv of (query, passage, answer) rows: n_passages distinct passages of 30..max words, each row picks one (repeats),
    queries of 4..12 words."""
    g = torch.Generator().manual_seed(seed)
    words = _words(tok)

    def sentence(lo, hi):
        k = int(torch.randint(lo, hi + 1, (1,), generator=g))
        return " ".join(words[int(i)] for i in torch.randint(0, len(words), (k,), generator=g))

    passages = [sentence(min(30, max_passage_words), max_passage_words) for _ in range(n_passages)]
    rows = []
    for i in range(n_rows):
        p = passages[int(torch.randint(0, n_passages, (1,), generator=g))] if i >= n_passages else passages[i]
        rows.append((sentence(4, 12), p, sentence(1, 3)))
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["query", "passage", "answer"])
        w.writerows(rows)
    return rows


def _bge_large_depth2(tok, seed=11):
    from transformers import BertConfig, BertModel

    torch.manual_seed(seed)
    return BertModel(BertConfig(hidden_size=1024, num_hidden_layers=2, num_attention_heads=16, intermediate_size=4096,
                                vocab_size=len(tok), max_position_embeddings=512, hidden_dropout_prob=0.0,
                                attention_probs_dropout_prob=0.0, pad_token_id=tok.pad_token_id))


def _fp32_eager_embeddings(state_dict, config, ids, mask, dev):
    """fp32 run of the same weights on the padded inputs: transformers' BertModel on torch SDPA, mean_pooling + normalize
    restated (fp64 accumulation of the pooled sum)."""
    from transformers import BertModel

    cfg = type(config).from_dict(config.to_dict())
    cfg._attn_implementation = "sdpa"
    ref = BertModel(cfg).to(dev).float().eval()
    ref.load_state_dict({k: v.float() for k, v in state_dict.items()})
    outs = []
    with torch.no_grad():
        for a in range(0, ids.shape[0], 32):
            i, m = ids[a:a + 32].to(dev), mask[a:a + 32].to(dev)
            h = ref(input_ids=i, attention_mask=m)[0].double()
            mm = m.unsqueeze(-1).double()
            u = (h * mm).sum(1) / torch.clamp(mm.sum(1), min=1e-9)
            outs.append(torch.nn.functional.normalize(u, p=2, dim=1))
    return torch.cat(outs).cpu()


def test_packed_sweep_vs_fp32_eager(dev, tmp_path, monkeypatch):
    """The packed bf16 sweep against an fp32 eager run of the same weights on padded inputs.  The bound is measured, not fixed:
    the existing padded bf16 path (`AutoModelForSentenceEmbedding.forward` under bf16) is compared with the same fp32 run and
    the packed sweep may be off by twice that error - both are bf16 roundings of one fp32 computation in different summation
    orders.  Error = largest L2 distance between a row's unit-norm embedding and its fp32 counterpart.
    Measured on an MI355X (bge-large width, depth 2, 320 rows): queries (7.9 % live tokens) padded bf16 2.236e-3, packed sweep
    2.236e-3; passages (58.3 % live) padded bf16 1.056e-3, packed sweep 1.056e-3.
    Rows come back in dataset order although the batches are cut from the length-sorted order."""
    from transformers import PreTrainedTokenizerFast

    import datasets

    from dalm_amd.eval import utils as EU
    from dalm_amd.models import AutoModelForSentenceEmbedding
    from dalm_amd.ops import HipOps

    tok = PreTrainedTokenizerFast.from_pretrained(str(G / "wordlevel_tokenizer"))
    rows = _write_rows(tmp_path / "rows.csv", tok, n_rows=320, n_passages=200, seed=5)
    ds = datasets.Dataset.from_dict({"query": [r[0] for r in rows], "passage": [r[1] for r in rows]})
    bert = _bge_large_depth2(tok).to(torch.bfloat16)
    sd, cfg = {k: v.clone() for k, v in bert.state_dict().items()}, bert.config
    model = AutoModelForSentenceEmbedding.from_modules(bert.to(dev), tok, normalize=True, get_peft=False).eval()
    processed = EU.preprocess_dataset(ds, tok, "query", "passage", 128)
    calls = []
    real = HipOps.pool_packed_fwd
    monkeypatch.setattr(HipOps, "pool_packed_fwd", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    worst = {}
    for prefix in ("retriever_query", "retriever_passage"):
        ids = torch.tensor(processed[f"{prefix}_input_ids"])
        mask = torch.tensor(processed[f"{prefix}_attention_mask"])
        ref = _fp32_eager_embeddings(sd, cfg, ids, mask, dev)
        n0 = len(calls)
        packed_e = EU.embed_dataset(processed, prefix, model.forward, "cuda:0", torch.bfloat16, 16, packed_sweep=True)
        assert len(calls) - n0 >= 2                                        # the packed path ran, in several batches
        assert packed_e.is_cuda and packed_e.dtype == torch.float32 and packed_e.shape == (320, 1024)
        padded = []
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            for a in range(0, 320, 16):
                padded.append(model.forward(ids[a:a + 16].to(dev), mask[a:a + 16].to(dev)).float())
        padded_e = torch.cat(padded)
        err_packed = float((packed_e.double().cpu() - ref).norm(dim=1).max())
        err_padded = float((padded_e.double().cpu() - ref).norm(dim=1).max())
        live = float(mask.sum()) / mask.numel()
        print(f"{prefix}: live tokens {live:.1%}; max row L2 error vs fp32 eager: padded bf16 {err_padded:.3e}, packed sweep {err_packed:.3e}")
        worst[prefix] = (err_padded, err_packed)
        assert err_padded > 0 and err_packed <= 2 * err_padded, worst
    # float16 takes the padded forward (no packed call) and still returns device f32 rows in dataset order
    n0 = len(calls)
    e16 = EU.embed_dataset(processed.select(range(40)), "retriever_query", model.forward, "cuda:0", torch.float16, 16)
    assert len(calls) == n0 and e16.shape == (40, 1024) and e16.is_cuda
    with pytest.raises(ValueError, match="packed_sweep"):               # asked for explicitly where it cannot run: an error
        EU.embed_dataset(processed.select(range(40)), "retriever_query", model.forward, "cuda:0", torch.float16, 16, packed_sweep=True)


def _run_reference_loop_on(captured, processed_rows, top_k):
    p_emb, q_emb = captured["retriever_passage"], captured["retriever_query"]
    uniq = list(dict.fromkeys(r[1] for r in processed_rows))
    assert p_emb.shape[0] == len(uniq) and q_emb.shape[0] == len(processed_rows)
    S = q_emb.double().cpu() @ p_emb.double().cpu().t()
    return reference_loop(S, uniq, [r[1] for r in processed_rows], top_k)


@pytest.mark.parametrize("with_adapter", [False, True])
def test_evaluate_retriever_end_to_end(dev, tmp_path, monkeypatch, with_adapter):
    """`evaluate_retriever` on a csv with repeated passages and a saved real-width depth-2 encoder (with and without a saved
    LoRA adapter): recall / precision / hit-rate equal the reference's loop (restated in test_eval_host.py) run on the
    embeddings the sweep produced; total_examples counts rows; `evaluate_rag(evaluate_generator=False)` agrees."""
    from transformers import PreTrainedTokenizerFast

    from dalm_amd.eval import utils as EU
    from dalm_amd.eval.eval_rag import evaluate_rag
    from dalm_amd.eval.eval_retriever_only import evaluate_retriever
    from dalm_amd.models import lora

    tok = PreTrainedTokenizerFast.from_pretrained(str(G / "wordlevel_tokenizer"))
    rows = _write_rows(tmp_path / "rows.csv", tok, n_rows=260, n_passages=150, seed=9)
    bert = _bge_large_depth2(tok, seed=13)
    enc_dir = tmp_path / "enc"
    bert.save_pretrained(str(enc_dir))
    tok.save_pretrained(str(enc_dir))
    adapter = None
    if with_adapter:
        lora.inject_lora(bert, ["key", "query", "value"])
        g = torch.Generator().manual_seed(3)
        for name, p in bert.named_parameters():
            if ".lora_B." in name:
                p.data.copy_(torch.randn(p.shape, generator=g) * 0.05)     # a fresh adapter's B is zero: make it count
        adapter = str(tmp_path / "adapter")
        lora.save_adapter(bert, adapter)
    from dalm_amd.ops import HipOps

    captured, packed_calls = {}, []
    real = EU.embed_dataset
    real_pool = HipOps.pool_packed_fwd

    def spy(dataset, prefix, *a, **k):
        captured[prefix] = real(dataset, prefix, *a, **k)
        return captured[prefix]

    monkeypatch.setattr(EU, "embed_dataset", spy)
    monkeypatch.setattr(HipOps, "pool_packed_fwd", lambda self, *a, **k: (packed_calls.append(1), real_pool(self, *a, **k))[1])
    kw = dict(test_batch_size=16, device="cuda:0", torch_dtype="bfloat16", top_k=10, packed_sweep=True)
    if with_adapter:             # the adapter must change the embeddings: the base run first
        evaluate_retriever(str(tmp_path / "rows.csv"), str(enc_dir), None, "passage", "query", 1024, 128, **kw)
        without = {k: v.clone() for k, v in captured.items()}
    n0 = len(packed_calls)
    res = evaluate_retriever(str(tmp_path / "rows.csv"), str(enc_dir), adapter, "passage", "query", 1024, 128, **kw)
    assert len(packed_calls) - n0 >= 4             # passages and queries went through the packed sweep, several batches each
    if with_adapter:
        for key in ("retriever_query", "retriever_passage"):
            moved = float((captured[key] - without[key]).norm(dim=1).max())
            assert moved > 1e-2, (key, moved)          # the merged adapter took part (a bf16 rerun alone moves nothing)
    ref = _run_reference_loop_on(captured, rows, 10)
    print(f"adapter={with_adapter}: {res}")
    assert res.total_examples == 260
    for key in ("recall", "precision", "hit_rate"):
        assert abs(getattr(res, key) - ref[key]) < 1e-12, (key, res, ref)
    assert res.recall_at[10] == res.recall and 0.0 < res.mrr <= 1.0
    if with_adapter:
        return
    base = {k: v.clone() for k, v in captured.items()}
    rag = evaluate_rag(str(tmp_path / "rows.csv"), str(enc_dir), str(G / "tiny_generator"), None, None, "passage", "query", "answer",
                       1024, 128, test_batch_size=16, device="cuda:0", torch_dtype="bfloat16", top_k=10, evaluate_generator=False,
                       packed_sweep=True)
    assert (rag.total_examples, rag.recall, rag.precision, rag.hit_rate) == (res.total_examples, res.recall, res.precision, res.hit_rate)
    assert torch.equal(base["retriever_query"], captured["retriever_query"])      # the sweep is deterministic


def test_evaluate_rag_generator(dev, tmp_path):
    """`evaluate_rag(evaluate_generator=True)` on the tiny golden models in fp32: the greedy tokens of
    `run_generator_on_prompts` equal Hugging Face `generate` on a freshly loaded, unpatched copy of the generator, and the
    exact-match count equals a recomputation from the decoded strings."""
    from transformers import AutoModelForCausalLM, AutoTokenizer

    from dalm_amd.eval.eval_rag import evaluate_rag, exact_match_count, run_generator_on_prompts
    from dalm_amd.models import AutoModelForRagE2E

    tok = AutoTokenizer.from_pretrained(str(G / "tiny_retriever"))
    rows = _write_rows(tmp_path / "rows.csv", tok, n_rows=21, n_passages=12, seed=2, max_passage_words=20)
    rag = AutoModelForRagE2E(str(G / "tiny_retriever"), str(G / "tiny_generator"))
    report = {}
    res = evaluate_rag(str(tmp_path / "rows.csv"), "", "", None, None, "passage", "query", "answer", 32, 48, test_batch_size=8,
                       query_batch_size=8, device="cuda:0", torch_dtype="float32", top_k=5, evaluate_generator=True,
                       rag_model=rag, report=report)
    assert res.total_examples == 21 and len(report["generated"]) == 21 and len(report["top_passages"]) == 21
    assert set(report["top_passages"]) <= {r[1] for r in rows}
    prompts = [f"#query# {r[0]} #passage# {p} #answer# " for r, p in zip(rows, report["top_passages"])]
    gtok = rag.generator_tokenizer
    decoded, tokens = [], []
    for a in range(0, 21, 8):
        d, t = run_generator_on_prompts(rag.generator_model, gtok, prompts[a:a + 8], max_length=48, torch_dtype=torch.float32,
                                        return_token_ids=True)
        decoded.extend(d)
        tokens.append(t)
    assert decoded == report["generated"]
    fresh = AutoModelForCausalLM.from_pretrained(str(G / "tiny_generator")).to(dev).eval()
    ftok = AutoTokenizer.from_pretrained(str(G / "tiny_generator"))
    ftok.pad_token = ftok.eos_token
    ftok.padding_side = "left"
    for a, t in zip(range(0, 21, 8), tokens):
        inputs = ftok(prompts[a:a + 8], return_tensors="pt", padding=True, truncation=True, max_length=48).to(dev)
        with torch.no_grad():
            want = fresh.generate(**inputs, max_length=48, do_sample=False)
        assert torch.equal(t, want.cpu()), (a, t, want)
        assert t.shape[1] > inputs["input_ids"].shape[1]                  # something was generated
    answers = [r[2] for r in rows]
    assert report["exact_match_hits"] == exact_match_count(report["generated"], answers)
    hits = sum(1 for gen, ans in zip(report["generated"], answers)
               if len(gen.split("#answer#")) >= 2 and gen.split("#answer#")[1].strip() == ans)
    assert report["exact_match_hits"] == hits
