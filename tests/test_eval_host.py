"""Host side of the evaluation drivers (no GPU): the reference's argument surface, the CLI, the rank -> metrics arithmetic
against a restatement of the reference's per-query loop, passage de-duplication, and the refusal of CPU tensors."""
import inspect
import json
from pathlib import Path

import pytest
import torch

G = Path(__file__).parent / "golden"
SIGS = json.loads((G / "eval_signatures.json").read_text())     # recorded from the imported reference (names and defaults)


# ---------------------------------------------------------------------------
# signatures / flags / CLI
# ---------------------------------------------------------------------------
def _fn_sig(fn):
    return [{"name": n, "default": (None if p.default is inspect.Parameter.empty else p.default),
             "required": p.default is inspect.Parameter.empty}
            for n, p in inspect.signature(fn).parameters.items() if p.kind is not inspect.Parameter.KEYWORD_ONLY]


@pytest.mark.parametrize("which", ["evaluate_retriever", "evaluate_rag"])
def test_driver_signatures_are_the_references(which):
    from dalm_amd.eval import eval_rag, eval_retriever_only

    fn = {"evaluate_retriever": eval_retriever_only.evaluate_retriever, "evaluate_rag": eval_rag.evaluate_rag}[which]
    assert _fn_sig(fn) == SIGS[which]
    # extensions are trailing keyword-only parameters with defaults
    extra = [p for p in inspect.signature(fn).parameters.values() if p.kind is inspect.Parameter.KEYWORD_ONLY]
    assert all(p.default is not inspect.Parameter.empty for p in extra)


@pytest.mark.parametrize("which", ["eval_retriever_only", "eval_rag"])
def test_argparse_flags_are_the_references(which, monkeypatch):
    import argparse
    import importlib

    mod = importlib.import_module(f"dalm_amd.eval.{which}")
    seen = {}

    def capture(self, *a, **k):
        seen["parser"] = self
        raise SystemExit(0)

    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", capture)
    with pytest.raises(SystemExit):
        mod.parse_args()
    got = [{"flags": list(a.option_strings), "dest": a.dest, "default": a.default, "required": bool(a.required),
            "store_true": isinstance(a, argparse._StoreTrueAction), "type": getattr(a.type, "__name__", None)}
           for a in seen["parser"]._actions if a.dest != "help"]
    assert got == SIGS[f"{which}.parse_args"]


def test_parse_args_reads_a_command_line():
    from dalm_amd.eval import eval_rag, eval_retriever_only

    a = eval_retriever_only.parse_args(["--dataset_path", "rows.csv", "--retriever_name_or_path", "enc", "--torch_dtype",
                                        "bfloat16", "--is_autoregressive"])
    assert (a.dataset_path, a.retriever_name_or_path, a.torch_dtype, a.is_autoregressive, a.top_k) == ("rows.csv", "enc", "bfloat16", True, 10)
    b = eval_rag.parse_args(["--dataset_path", "d", "--retriever_name_or_path", "r", "--generator_name_or_path", "g"])
    assert (b.max_length, b.query_batch_size, b.evaluate_generator, b.answer_column_name) == (256, 16, False, "answer")


@pytest.mark.parametrize("name", ["eval-rag", "eval-retriever"])
def test_cli_exposes_the_eval_commands(name):
    import typer.main

    from dalm_amd.cli import cli

    cmd = typer.main.get_command(cli).commands[name]
    want = SIGS[f"cli.{name}"]
    got = {p.name: p for p in cmd.params}
    assert [p.name for p in cmd.params][:len(want)] == [w["name"] for w in want]
    for w in want:
        p = got[w["name"]]
        assert (p.param_type_name == "argument") == w["argument"], w
        assert w["opts"][0] in p.opts, (w, p.opts)
    defaults = {p.name: p.default for p in cmd.params}
    assert defaults["passage_column_name"] == "Abstract" and defaults["query_column_name"] == "Question"
    assert defaults["embed_dim"] == 1024 and defaults["max_length"] == 128 and defaults["top_k"] == 10
    assert defaults["torch_dtype"] == "float16" and defaults["test_batch_size"] == 8
    assert got["retriever_name_or_path"].required
    assert "bfloat16" in got["torch_dtype"].help


def test_eval_results_model():
    from dalm_amd.eval.eval_results import EvalResults

    r = EvalResults(total_examples=4, recall=0.5, precision=0.05, hit_rate=0.5)
    assert r.mrr is None and r.recall_at is None
    r2 = EvalResults(total_examples=4, recall=0.5, precision=0.05, hit_rate=0.5, mrr=0.3, recall_at={1: 0.25, 10: 0.5})
    assert r2.recall_at[10] == 0.5 and set(r2.model_dump()) == {"total_examples", "recall", "precision", "hit_rate", "mrr", "recall_at"}


def test_reference_names_are_importable():
    from dalm_amd.eval import utils

    for name in ("construct_search_index", "get_nearest_neighbours", "calculate_precision_recall", "preprocess_function",
                 "preprocess_dataset", "filter_unique_passages", "mixed_collate_fn", "get_retriever_embeddings",
                 "get_passage_embeddings", "evaluate_retriever_on_batch", "calc_eval_results", "print_eval_results"):
        assert callable(getattr(utils, name)), name
    r = utils.calc_eval_results(4, [0.1, 0.0, 0.1, 0.1], [1.0, 0.0, 1.0, 1.0], 3)
    assert (r.total_examples, r.recall, r.hit_rate) == (4, 0.75, 0.75) and abs(r.precision - 0.075) < 1e-12


# ---------------------------------------------------------------------------
# metrics
# ---------------------------------------------------------------------------
def reference_loop(scores64, unique_passages, correct_passages, top_k, threshold=0.0):
    """The reference's evaluation, restated (dalm/eval/utils.py:44-83,253-285): top_k by score (ties: lower index), keep the
    results scoring >= threshold, set precision / recall on passage STRINGS against the single correct passage, then
    calc_eval_results.  A query with nothing retrieved scores 0 (the reference would divide by zero)."""
    nq = scores64.shape[0]
    precisions, recalls, total_hit = [], [], 0
    for i in range(nq):
        order = sorted(range(scores64.shape[1]), key=lambda j: (-float(scores64[i, j]), j))[:top_k]
        retrieved = [unique_passages[j] for j in order if float(scores64[i, j]) >= threshold]
        if not retrieved:
            precisions.append(0.0)
            recalls.append(0.0)
            continue
        got, want = set(retrieved), {correct_passages[i]}
        hit = len(got & want)
        precisions.append(hit / len(got))
        recalls.append(hit / len(want))
        total_hit += int(correct_passages[i] in retrieved)
    return {"recall": sum(recalls) / nq, "precision": sum(precisions) / nq, "hit_rate": total_hit / float(nq)}


def brute_rank(scores64, gold, threshold):
    """rank / n_ge straight from the definition (ties: lower corpus index first)."""
    nq, nc = scores64.shape
    g = scores64[torch.arange(nq), gold].unsqueeze(1)
    j = torch.arange(nc).unsqueeze(0)
    before = (scores64 > g) | ((scores64 == g) & (j < gold.unsqueeze(1)))
    before[torch.arange(nq), gold] = False
    return before.sum(1), (scores64 >= threshold).sum(1)


@pytest.mark.parametrize("seed,nq,nrows,threshold", [(0, 40, 60, 0.0), (1, 25, 30, 0.0), (2, 50, 45, 0.35), (3, 16, 12, 0.0)])
def test_metrics_from_rank_equal_the_reference_loop(seed, nq, nrows, threshold):
    """Seeded cases with duplicate passages in the dataset, negative scores, fewer than k results above the threshold, and k
    given as a list."""
    from dalm_amd.eval.utils import filter_unique_passages
    from dalm_amd.retrieval import metrics_from_rank

    import datasets

    g = torch.Generator().manual_seed(seed)
    texts = [f"passage {int(t)}" for t in torch.randint(0, max(3, nrows // 2), (nrows,), generator=g)]     # many repeats
    ds = datasets.Dataset.from_dict({"passage": texts, "query": [f"q{i}" for i in range(nrows)]})
    unique, gold_all = filter_unique_passages(ds, "passage", return_gold_index=True)
    uniq_texts = unique["passage"]
    rows = torch.randint(0, nrows, (nq,), generator=g).tolist()
    gold = torch.tensor([gold_all[r] for r in rows])
    correct = [texts[r] for r in rows]
    nc = len(uniq_texts)
    scores = torch.randn(nq, nc, generator=g, dtype=torch.float64) * 0.4           # about half of the scores negative
    scores[torch.arange(nq), gold] += 0.5 * torch.rand(nq, generator=g, dtype=torch.float64)
    scores[0] = -1.0 - torch.rand(nc, generator=g, dtype=torch.float64)             # a query with nothing at or above the threshold
    scores[1, : nc // 2] = scores[1, gold[1]]                                      # exact ties with the gold passage
    rank, n_ge = brute_rank(scores, gold, threshold)
    ks = [1, 3, 10, nc, nc + 5]
    assert int(n_ge.min()) == 0 and bool((n_ge < 10).any()) and bool((rank > 0).any())
    many = metrics_from_rank(rank, n_ge, ks)
    assert [m["top_k"] for m in many] == ks
    for k, m in zip(ks, many):
        ref = reference_loop(scores, uniq_texts, correct, k, threshold)
        for key in ("recall", "precision", "hit_rate"):
            assert abs(m[key] - ref[key]) < 1e-12, (k, key, m, ref)
        assert m == metrics_from_rank(rank, n_ge, k) and m["total_examples"] == nq
        assert abs(m["mrr"] - float((1.0 / (rank.double() + 1)).mean())) < 1e-12


def test_filter_unique_passages_keeps_first_occurrences_in_order():
    import datasets

    from dalm_amd.eval.utils import filter_unique_passages

    texts = ["b", "a", "b", "c", "a", "d", "c", "b"]
    ds = datasets.Dataset.from_dict({"passage": texts, "query": [str(i) for i in range(len(texts))]})
    unique = filter_unique_passages(ds, "passage")
    assert unique["passage"] == ["b", "a", "c", "d"] and unique["query"] == ["0", "1", "3", "5"]
    unique2, gold = filter_unique_passages(ds, "passage", return_gold_index=True)
    assert unique2["passage"] == unique["passage"] and gold == [0, 1, 0, 2, 1, 3, 2, 0]
    assert [unique2["passage"][g] for g in gold] == texts


def test_token_budget_batches_cover_every_row_once():
    from dalm_amd.eval.utils import token_budget_batches

    lengths = torch.tensor([5, 128, 7, 7, 30, 2, 64, 128, 9])
    order, cuts = token_budget_batches(lengths, 100)
    assert sorted(order.tolist()) == list(range(9)) and lengths[order].tolist() == sorted(lengths.tolist())
    assert cuts[0][0] == 0 and cuts[-1][1] == 9 and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
    for a, b in cuts:
        assert b > a and (int(lengths[order[a:b]].sum()) <= 100 or b - a == 1)


# ---------------------------------------------------------------------------
# no CPU implementation
# ---------------------------------------------------------------------------
def test_new_ops_refuse_cpu_tensors():
    from dalm_amd.ops import default_ops
    from dalm_amd.retrieval import gold_rank

    ops = default_ops()
    h, cu = torch.randn(6, 8), torch.tensor([0, 2, 6], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="HIP|MI355X|GPU"):
        ops.pool_packed_fwd(h, cu)
    q, c, gold = torch.randn(3, 8), torch.randn(5, 8), torch.tensor([0, 4, 2])
    z = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="HIP|MI355X|GPU"):
        ops.sim_gold_score(q, c, gold, 0, torch.zeros(3))
    with pytest.raises(RuntimeError, match="HIP|MI355X|GPU"):
        ops.sim_gold_rank(q, c, gold, torch.zeros(3), 0, 0.0, z, z.clone())
    with pytest.raises(RuntimeError, match="HIP|MI355X|GPU"):
        gold_rank(q, c, gold)


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    import ctypes

    from dalm_amd import _build, hip

    _build.build(verbose=False)
    lib = hip.load()
    assert lib.dalm_pool_l2norm_packed_fwd(None, 0, None, 4, 2, 2, 8, None, 8, None, None, None) == -1
    assert lib.dalm_sim_gold_score(None, None, None, 4, 4, 8, 0, ctypes.c_float(1.0), None, None) == -1
    assert lib.dalm_sim_gold_rank(None, None, None, None, 4, 4, 8, 0, ctypes.c_float(1.0), ctypes.c_float(0.0), None, None, None, 0,
                                  None) == -1
    assert lib.dalm_sim_gold_rank_workspace_bytes(300, 70000, 384) > 0
    assert lib.dalm_sim_gold_rank_workspace_bytes(0, 10, 8) == 0
