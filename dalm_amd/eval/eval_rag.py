"""`dalm eval-rag` on the MI355X path: the retriever metrics of `eval-retriever` for the retriever of a RAG-end2end model
and, with --evaluate_generator, exact match of the generator's answers on the top-1 retrieved passage - with the reference's
parameters (dalm/eval/eval_rag.py:30-313).

The retrieval numbers come from the rank sweep (`dalm_amd.retrieval.gold_rank`); the generator additionally gets each
query's best passage from `exact_topk(k=1)` (the reference only ever uses `retrieved_passages[0]`), prompts are
"#query# {q} #passage# {p} #answer# " and generation is Hugging Face `generate` under no_grad + autocast.

Deliberate differences from the reference:

1. No shuffle.  The reference shuffles its DataLoader and then zips the generations (in shuffled order) with the answer
   column (in dataset order) (eval_rag.py:234-236,275-277), so its exact match compares different rows.  Order is kept
   here and exact match compares each generation with its own row's answer.
2. Left padding for generation.  Prompts are left-padded for `generate`; the reference leaves the tokenizer's default, and a
   right-padded decoder prompt continues from pad tokens.

A query whose retrieved scores are all below the threshold 0.0 scores 0 in the retrieval metrics (the reference divides by
zero there).
"""
from __future__ import annotations

from argparse import Namespace
from typing import List, Literal, Optional

import torch

from ..models.rag_e2e_base_model import AutoModelForRagE2E
from ..retrieval import exact_topk
from ..utils import load_dataset
from .eval_results import EvalResults
from ..training.common import build_parser
from .eval_retriever_only import flag_table, select_dtype
from .utils import preprocess_dataset, print_eval_results, retrieval_metrics


RAG_FLAGS = flag_table(
    ["dataset_path", "query_column_name", "passage_column_name", "answer_column_name", "embed_dim", "max_length",
     "retriever_name_or_path", "generator_name_or_path", "retriever_peft_model_path", "generator_peft_model_path",
     "test_batch_size", "query_batch_size", "device", "torch_dtype", "top_k", "evaluate_generator", "is_retriever_autoregressive"],
    {"answer_column_name": dict(type=str, default="answer", help="Column holding the expected answers."),
     "max_length": dict(type=int, default=256, help="Token rows and generator prompts are truncated to this length."),
     "generator_name_or_path": dict(type=str, required=True, help="Generator checkpoint directory or hub identifier."),
     "generator_peft_model_path": dict(type=str, required=False, help="Directory of a saved generator LoRA adapter."),
     "query_batch_size": dict(type=int, default=16, help="Prompts per generate call."),
     "evaluate_generator": dict(action="store_true", help="Also generate answers and count exact matches."),
     "is_retriever_autoregressive": dict(action="store_true", help="The retriever is a causal LM (last-token pooling).")})


def parse_args(argv=None) -> Namespace:
    return build_parser("Retrieval metrics and generator exact match of a RAG-end2end model", RAG_FLAGS).parse_args(argv)


def run_generator_on_prompts(model, tokenizer, prompts: List[str], max_length: int = 256, *,
                             torch_dtype: Optional[torch.dtype] = torch.float16, return_token_ids: bool = False):
    """Runs the generator over the prompts (query + passage), left-padded, and returns the decoded sequences (prompt
    included, as `generate` returns them); return_token_ids=True returns (decoded, token ids on the host)."""
    side = tokenizer.padding_side
    tokenizer.padding_side = "left"
    try:
        inputs = tokenizer(prompts, return_tensors="pt", padding=True, truncation=True, max_length=max_length)
    finally:
        tokenizer.padding_side = side
    device = next(model.parameters()).device
    cast = torch_dtype in (torch.float16, torch.bfloat16)
    with torch.autocast(device.type, dtype=torch_dtype if cast else None, enabled=cast), torch.no_grad():
        outputs = model.generate(**inputs.to(device), max_length=max_length, early_stopping=True)
    outputs = outputs.cpu()
    decoded = tokenizer.batch_decode(outputs, skip_special_tokens=True)
    return (decoded, outputs) if return_token_ids else decoded


PROMPT = "#query# {query} #passage# {passage} #answer# "


def eval_generator_on_batch(model, tokenizer, queries: List[str], passages: List[str], query_batch_size: int,
                            queries_for_gen_eval: List[str], max_length: int, *,
                            torch_dtype: Optional[torch.dtype] = torch.float16):
    """Queues one prompt per (query, retrieved passage) pair behind the prompts already waiting in `queries_for_gen_eval` and
    generates in chunks of `query_batch_size`; returns (prompts still waiting - fewer than a chunk -, generations so far)."""
    if len(queries) != len(passages):
        raise ValueError(f"{len(queries)} queries but {len(passages)} passages")
    queries_for_gen_eval.extend(PROMPT.format(query=q, passage=p) for q, p in zip(queries, passages))
    done: List[str] = []
    while len(queries_for_gen_eval) >= query_batch_size:
        chunk = queries_for_gen_eval[:query_batch_size]
        del queries_for_gen_eval[:query_batch_size]
        done.extend(run_generator_on_prompts(model, tokenizer, chunk, max_length=max_length, torch_dtype=torch_dtype))
    return queries_for_gen_eval, done


def exact_match_count(generated_answers: List[str], answers: List[str]) -> int:
    """Number of generations whose text between the first and second "#answer#" marker (or the end), stripped, equals the
    row's answer; a generation without the marker counts as a miss.  The reference's exact match (eval_rag.py:277-284)."""
    if len(generated_answers) != len(answers):
        raise ValueError(f"{len(generated_answers)} generations but {len(answers)} answers")
    said = [g.split("#answer#") for g in generated_answers]
    return sum(1 for parts, answer in zip(said, answers) if len(parts) > 1 and parts[1].strip() == answer)


def evaluate_rag(
    dataset_or_path,
    retriever_name_or_path: str,
    generator_name_or_path: str,
    retriever_peft_model_path: Optional[str],
    generator_peft_model_path: Optional[str],
    passage_column_name: str,
    query_column_name: str,
    answer_column_name: str,
    embed_dim: int,
    max_length: int,
    test_batch_size: int = 8,
    query_batch_size: int = 16,
    device: str = "cuda",
    torch_dtype: Literal["float16", "bfloat16", "float32"] = "float16",
    top_k: int = 10,
    evaluate_generator: bool = True,
    retriever_is_autoregressive: bool = False,
    *,
    rag_model: Optional[AutoModelForRagE2E] = None,
    report: Optional[dict] = None,
    packed_sweep: Optional[bool] = None,
) -> EvalResults:
    """Runs rag evaluation. See `dalm eval-rag --help` for details on params.  `report` (a dict) receives the generator's
    prompts, generations and exact-match count; `packed_sweep` as in `evaluate_retriever`."""
    test_dataset = load_dataset(dataset_or_path)
    selected_torch_dtype = select_dtype(torch_dtype)
    if rag_model is None:
        rag_model = AutoModelForRagE2E(retriever_name_or_path, generator_name_or_path,
                                       retriever_is_autoregressive=retriever_is_autoregressive)
    processed_datasets = preprocess_dataset(test_dataset, rag_model.retriever_tokenizer, query_column_name,
                                            passage_column_name, max_length)
    rag_model.attach_pre_trained_peft_layers(retriever_peft_model_path, generator_peft_model_path, device)
    if retriever_peft_model_path is None:
        rag_model.retriever_model.eval().to(device)
    if generator_peft_model_path is None:
        rag_model.generator_model.eval().to(device)
    eval_results, state = retrieval_metrics(processed_datasets, passage_column_name, rag_model.retrieval_forward, device,
                                            embed_dim, selected_torch_dtype, test_batch_size, top_k, packed_sweep=packed_sweep)
    if not evaluate_generator:
        print_eval_results(eval_results)
        return eval_results

    model = rag_model.generator_model
    tokenizer = rag_model.generator_tokenizer
    tokenizer.pad_token = tokenizer.eos_token
    _scores, top1 = exact_topk(state["query_embeddings"], state["passage_embeddings"], 1)
    unique_passages = state["unique"][passage_column_name]
    top_passages = [unique_passages[i] for i in top1[:, 0].tolist()]
    waiting, generated = eval_generator_on_batch(model, tokenizer, processed_datasets[query_column_name], top_passages,
                                                 query_batch_size, [], max_length, torch_dtype=selected_torch_dtype)
    if len(waiting) > 0:
        generated.extend(run_generator_on_prompts(model, tokenizer, waiting, max_length=max_length,
                                                  torch_dtype=selected_torch_dtype))
    total_em_hit = exact_match_count(generated, processed_datasets[answer_column_name])
    if report is not None:
        report.update({"top_passages": top_passages, "generated": generated, "exact_match_hits": total_em_hit})
    print_eval_results(eval_results)
    print("Generator evaluation:")
    print("Exact match:", total_em_hit / len(processed_datasets))
    return eval_results


def main() -> None:
    kw = vars(parse_args())
    kw["dataset_or_path"] = kw.pop("dataset_path")
    kw["retriever_is_autoregressive"] = kw.pop("is_retriever_autoregressive")
    evaluate_rag(**kw)


if __name__ == "__main__":
    main()
